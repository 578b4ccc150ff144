"""SPEC.md §12b restated in NumPy, twice, for the predicted-bands tests: `bands` (vectorised: np.sort on the uint32 keys, mapped back) and `bands_def` (straight from
the definition: the rank of every particle counted one comparison at a time), and a set of WRONG reducers (MUTANTS) that each change a compared word on at least
one committed case — what the tests can tell apart.

The tensor is the canonical one, f32[B][P][H+1][13] (the oracle's, or rollout(want_traj=True)); outputs: q f32[B][Q][H+1][13], below / at uint32[B][H+1][13]."""
import math

import numpy as np

QNAN = np.uint32(0x7FC00000)
TOP = np.uint32(0xFFFFFFFF)
SIGN = np.uint32(0x80000000)


def keys(v):
    """the key of every word: NaN -> 0xFFFFFFFF; sign bit set -> ~u; else u ^ 0x80000000"""
    v = np.ascontiguousarray(v, np.float32)
    u = v.view(np.uint32)
    k = np.where((u & SIGN) != 0, ~u, u ^ SIGN).astype(np.uint32)
    return np.where(np.isnan(v), TOP, k).astype(np.uint32)


def words(k):
    """the word of every key, as float32; the NaN key gives 0x7FC00000"""
    k = np.ascontiguousarray(k, np.uint32)
    u = np.where((k & SIGN) != 0, k ^ SIGN, ~k).astype(np.uint32)
    return np.where(k == TOP, QNAN, u).astype(np.uint32).view(np.float32)


def quantile_ranks(quantiles, P):
    """quantile -> rank ceil(q P) - 1, clamped to [0, P-1]"""
    return [min(P - 1, max(0, math.ceil(float(q) * P) - 1)) for q in quantiles]


def bands(traj, ranks=None, obs=None):
    """vectorised restatement"""
    traj = np.asarray(traj, np.float32)
    B, P, T, nx = traj.shape
    k = keys(traj)
    out = {"q": None, "below": None, "at": None}
    if ranks is not None:
        ranks = [int(r) for r in ranks]
        assert all(0 <= r < P for r in ranks)
        s = np.sort(k, axis=1)
        out["q"] = np.ascontiguousarray(words(s[:, ranks]))            # [B][Q][T][13]
    if obs is not None:
        ko = keys(np.asarray(obs, np.float32).reshape(B, 1, T, nx))
        out["below"] = (k < ko).sum(axis=1).astype(np.uint32)
        out["at"] = (k == ko).sum(axis=1).astype(np.uint32)
    return out


def key_scalar(x):
    """the key of one float32, in Python integers"""
    u = int(np.float32(x).view(np.uint32))
    if x != x:
        return 0xFFFFFFFF
    return (u ^ 0xFFFFFFFF) if (u & 0x80000000) else (u ^ 0x80000000)


def bands_def(traj, ranks=None, obs=None, columns=None):
    """From the definition, one comparison at a time: particle p has n_below(p) particles with a smaller key and n_at(p) with an equal one; plane k holds the
    word of a particle with n_below <= ranks[k] < n_below + n_at. columns: an iterable of (b, t, i) to restrict the work to (the others stay 0)."""
    traj = np.asarray(traj, np.float32)
    B, P, T, nx = traj.shape
    Q = 0 if ranks is None else len(ranks)
    q = np.zeros((B, Q, T, nx), np.uint32)
    below = np.zeros((B, T, nx), np.uint32)
    at = np.zeros((B, T, nx), np.uint32)
    cols = columns if columns is not None else [(b, t, i) for b in range(B) for t in range(T) for i in range(nx)]
    for b, t, i in cols:
        kk = [key_scalar(traj[b, p, t, i]) for p in range(P)]
        if Q:
            for p in range(P):
                nb = na = 0
                for o in range(P):
                    if kk[o] < kk[p]:
                        nb += 1
                    elif kk[o] == kk[p]:
                        na += 1
                for j, r in enumerate(ranks):
                    if nb <= r < nb + na:
                        w = int(traj[b, p, t, i].view(np.uint32))
                        q[b, j, t, i] = 0x7FC00000 if kk[p] == 0xFFFFFFFF else w
        if obs is not None:
            ko = key_scalar(obs[b, t, i])
            nb = na = 0
            for o in range(P):
                if kk[o] < ko:
                    nb += 1
                elif kk[o] == ko:
                    na += 1
            below[b, t, i], at[b, t, i] = nb, na
    return {"q": q.view(np.float32) if Q else None, "below": below if obs is not None else None, "at": at if obs is not None else None}


# ---- wrong reducers: each takes (traj, ranks, obs) and returns the same dict -------------------------------------------------------------------------------
def _with_keys(keyfn, traj, ranks, obs, wordfn=words, below_le=False, at_nan=True, descending=False, rank_shift=0, group=False):
    traj = np.asarray(traj, np.float32)
    B, P, T, nx = traj.shape
    k = keyfn(traj)
    s = np.sort(k[:, :32] if group else k, axis=1)
    if descending:
        s = s[:, ::-1]
    n = s.shape[1]
    idx = [min(n - 1, max(0, int(r) + rank_shift)) for r in ranks]
    q = np.ascontiguousarray(wordfn(s[:, idx]))
    ko = keyfn(np.asarray(obs, np.float32).reshape(B, 1, T, nx))
    below = ((k <= ko) if below_le else (k < ko)).sum(axis=1).astype(np.uint32)
    at = (k == ko).sum(axis=1).astype(np.uint32)
    if not at_nan:
        at = np.where(np.isnan(obs), 0, at).astype(np.uint32)
    return {"q": q, "below": below, "at": at}


def m_padded(traj, ranks, obs):
    """the padded lanes of the last group take part, as the zero words the rollout's workspace may hold"""
    B, P, T, nx = traj.shape
    G = (P + 31) // 32
    full = np.concatenate([traj, np.zeros((B, G * 32 - P, T, nx), np.float32)], axis=1)
    return _with_keys(keys, full, ranks, obs)


def m_one_based(traj, ranks, obs):
    return _with_keys(keys, traj, ranks, obs, rank_shift=-1)


def m_descending(traj, ranks, obs):
    return _with_keys(keys, traj, ranks, obs, descending=True)


def _keys_nan_low(v):
    return np.where(np.isnan(v), np.uint32(0), keys(v)).astype(np.uint32)


def _words_nan_low(k):
    return np.where(k == 0, QNAN, words(k).view(np.uint32)).astype(np.uint32).view(np.float32)


def m_nan_low(traj, ranks, obs):
    """NaN below every number"""
    return _with_keys(_keys_nan_low, traj, ranks, obs, wordfn=_words_nan_low)


def m_float_lt(traj, ranks, obs):
    """float `<` / `==` instead of the key: -0 and +0 collapse (into +0)"""
    return _with_keys(lambda v: keys(np.asarray(v, np.float32) + np.float32(0.0)), traj, ranks, obs)


def _keys_flat(v):
    v = np.ascontiguousarray(v, np.float32)
    return np.where(np.isnan(v), TOP, v.view(np.uint32) ^ SIGN).astype(np.uint32)


def _words_flat(k):
    return np.where(k == TOP, QNAN, k ^ SIGN).astype(np.uint32).view(np.float32)


def m_neg_not_inverted(traj, ranks, obs):
    """negative words keep their magnitude order: u ^ 0x80000000 for every sign"""
    return _with_keys(_keys_flat, traj, ranks, obs, wordfn=_words_flat)


def m_below_le(traj, ranks, obs):
    return _with_keys(keys, traj, ranks, obs, below_le=True)


def m_at_no_nan(traj, ranks, obs):
    """a NaN observation finds no particle at it"""
    return _with_keys(keys, traj, ranks, obs, at_nan=False)


def m_column_transposed(traj, ranks, obs):
    """column index i (H+1) + t: the word of output column c = t 13 + i comes from column i (H+1) + t of the flat row"""
    good = bands(traj, ranks, obs)
    B, P, T, nx = traj.shape
    c = np.arange(T * nx).reshape(T, nx)
    src = (c % nx) * T + c // nx
    out = {}
    for k, a in good.items():
        flat = a.reshape(a.shape[:-2] + (T * nx,))
        out[k] = np.ascontiguousarray(flat[..., src])
    return out


def m_group_rank(traj, ranks, obs):
    """the rank taken inside the first group of 32 particles instead of over all P"""
    return _with_keys(keys, traj, ranks, obs, group=True)


MUTANTS = {"padded_lanes": m_padded, "one_based_rank": m_one_based, "descending": m_descending, "nan_below_numbers": m_nan_low, "float_less_than": m_float_lt,
           "negative_keys_not_inverted": m_neg_not_inverted, "below_le": m_below_le, "at_never_nan": m_at_no_nan, "column_transposed": m_column_transposed,
           "rank_inside_one_group": m_group_rank}


def quantile_ranks_floor(quantiles, P):
    """the wrong mapping quantile -> floor(q P), clamped"""
    return [min(P - 1, max(0, math.floor(float(q) * P))) for q in quantiles]


def differs(a, b):
    """number of compared words that differ between two result dicts: q by bits, below / at by value"""
    n = int((a["q"].view(np.uint32) != b["q"].view(np.uint32)).sum())
    return n + int((a["below"] != b["below"]).sum()) + int((a["at"] != b["at"]).sum())
