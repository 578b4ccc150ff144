"""CPU reference of the predicted outcome (SPEC.md §12c): a pure NumPy float32 function of a particle x horizon tensor f32[B][P][H+1][13]. Every particle is scored
as tests/score_loop_ref.py scores an episode — the channels ARE score_loop_ref.row_terms (called on component-first arrays, so one call forms a whole tensor's
channels), and tests/test_outcome_cpu.py holds the per-particle words EQUAL to score_loop_ref.score_rows of the particle's rows — and the words and channels are
reduced over the particles: sums in the §6.1 order of tests/tube_ref.py, extrema as the tube's, order statistics in the key order of tests/band_ref.py.
Test infrastructure.

`mutant` builds a deliberately WRONG reducer, for the discrimination tests (MUTANTS). "zeros_tied" (a float compare in the order, so that -0 and +0 are one key)
is accepted but is NOT in MUTANTS: no channel and no aggregate can be -0 — dp, dv and w2 are sums of squares, c = fma(-2, s, 1) rounds an exact zero to +0 — so
that wrong order selects the same words here; the test of the order's two zeros is tests/test_band_cpu.py's."""
import numpy as np

import band_ref as BR
import tube_ref as TR
from score_loop_ref import NONE, row_terms

F = np.float32
U = np.uint32
WORDS = 11
FLOAT_WORDS = (1, 2, 4, 5, 6, 7)
AGG_WORDS = (1, 2, 6, 7)              # sum dp, max dp, min c, max w2
OUTPUTS = ("words", "fail_step", "first_fail", "cause_ever", "chan_stat", "chan_q", "agg_stat", "agg_q")
MUTANTS = ("row0_scored", "target_of_previous_row", "nan_passes", "tilt_from_wz", "last_max", "padded_lanes_counted", "slots_mod_8", "mean_unmasked", "nan_sorted_low", "hist_last_failure", "any_is_bit_sum")


def target_rows(B, H, xref=None, target=None):
    """g f32[B][H+1][13]: row t of the instance's xref window, or of the caller's rows [Bt][Ht][13] with Ht in {1, H+1}, Bt in {1, B} (a size-1 axis: index 0)"""
    if target is None:
        g = np.asarray(xref, F)
        assert g.shape == (B, H + 1, 13)
        return g
    g = np.asarray(target, F)
    assert g.ndim == 3 and g.shape[0] in (1, B) and g.shape[1] in (1, H + 1) and g.shape[2] == 13, g.shape
    return np.ascontiguousarray(np.broadcast_to(g, (B, H + 1, 13)))


def channels(rows, g, mutant=None):
    """rows f32[B][P][H][13] against g f32[B][H][13] -> (ch f32[B][P][H][4] = dp, dv, c, w2; nf bool[B][P][H])"""
    xT = np.moveaxis(rows, -1, 0)                                         # [13][B][P][H]
    gT = np.moveaxis(np.broadcast_to(g[:, None], rows.shape), -1, 0)
    dp, dv, c, w2, _ = row_terms(xT, gT, "tilt_from_wz" if mutant == "tilt_from_wz" else None)
    nf = ~(np.abs(rows) < F(np.inf)).all(axis=-1)
    return np.stack([dp, dv, c, w2], axis=-1).astype(F), nf


def _stats(v, P, mutant=None):
    """v f32[B][P][C] -> f32[B][C][3]: the §6.1 mean (tube_ref's butterfly and slots, times float32 1/P), min, max (fmin / fmax folds from +inf / -inf)"""
    B, _, C = v.shape
    with np.errstate(all="ignore"):
        pad = F(1.0) if mutant == "mean_unmasked" else F(0.0)       # (a padded lane of the device tensor holds anything; 1 stands for it)
        T = TR._butterfly(TR._groups(v, pad))                             # [B][G][C]
        if mutant == "slots_mod_8":
            S = [np.zeros((B, C), F) for _ in range(8)]
            for g in range(T.shape[1]):
                S[g % 8] = S[g % 8] + T[:, g]
            total = ((((((S[0] + S[1]) + S[2]) + S[3]) + S[4]) + S[5]) + S[6]) + S[7]
        else:
            total = TR._slots(T)
        mean = total * (F(1.0) / F(P))
        mn = np.fmin(np.fmin.reduce(TR._butterfly(TR._groups(v, F(np.inf)), np.fmin), axis=1), F(np.inf)).astype(F)
        mx = np.fmax(np.fmax.reduce(TR._butterfly(TR._groups(v, F(-np.inf)), np.fmax), axis=1), F(-np.inf)).astype(F)
    return np.stack([mean, mn, mx], axis=-1).astype(F)


def _keys(v, mutant):
    if mutant == "zeros_tied":                                            # float compare: -0 and +0 one key
        v = np.where(v == 0, F(0.0), v).astype(F)
    k = BR.keys(v)
    if mutant == "nan_sorted_low":
        k = np.where(np.isnan(v), U(0), k).astype(U)
    return k


def _select(v, ranks, mutant=None):
    """v f32[B][P][C] -> f32[B][C][K]: the words at the ranks of the key order over the particles"""
    k = np.sort(_keys(v, mutant), axis=1)
    return np.ascontiguousarray(np.moveaxis(BR.words(k[:, list(ranks)]), 1, -1))


def outcome(traj, thresholds, xref=None, target=None, ranks=None, mutant=None):
    """traj f32[B][P][H+1][13]; thresholds (r2_pos, cos_min, w2_max); the target rows from xref [B][H+1][13] or target [Bt][Ht][13]; ranks: up to 8 in [0, P) or
    None (then chan_q and agg_q are None). -> dict of OUTPUTS."""
    assert mutant is None or mutant in MUTANTS or mutant == "zeros_tied"
    traj = np.ascontiguousarray(traj, F)
    B, P, T1, nx = traj.shape
    H = T1 - 1
    assert nx == 13
    r2, cmin, w2max = (F(t) for t in thresholds)
    assert not (np.isnan(r2) or np.isnan(cmin) or np.isnan(w2max))
    g = target_rows(B, H, xref, target)
    if mutant == "row0_scored":
        rows, gr = traj[:, :, 0:H], g[:, 0:H]
    elif mutant == "target_of_previous_row":
        rows, gr = traj[:, :, 1:], g[:, 0:H]
    else:
        rows, gr = traj[:, :, 1:], g[:, 1:]
    with np.errstate(all="ignore"):
        ch, nf = channels(rows, gr, mutant)
        dp, dv, c, w2 = (ch[..., i] for i in range(4))
        out_p = (dp > r2) if mutant == "nan_passes" else ~(dp <= r2)
        cause = (U(1) * out_p + U(2) * ~(c >= cmin) + U(4) * ~(w2 <= w2max) + U(8) * nf).astype(U)       # [B][P][H]
        # the words, row by row in time order
        words = np.zeros((B, P, WORDS), U)
        sdp, mdp, sdv, mw2 = (np.zeros((B, P), F) for _ in range(4))
        minc = np.full((B, P), np.inf, F)
        imax, nbad, causes = (np.zeros((B, P), U) for _ in range(3))
        first = np.full((B, P), NONE, U)
        last = np.full((B, P), NONE, U)
        for r in range(H):
            sdp = sdp + dp[..., r]
            up = (dp[..., r] >= mdp) if mutant == "last_max" else (dp[..., r] > mdp)
            mdp, imax = np.where(up, dp[..., r], mdp), np.where(up, U(r), imax)
            sdv = sdv + dv[..., r]
            minc = np.where(c[..., r] < minc, c[..., r], minc)
            mw2 = np.where(w2[..., r] > mw2, w2[..., r], mw2)
            bad = cause[..., r] != 0
            first = np.where(bad & (first == NONE), U(r), first)
            last = np.where(bad, U(r), last)
            causes = causes | cause[..., r]
            nbad = nbad + bad.astype(U)
        words[..., 0] = H
        for i, a in ((1, sdp), (2, mdp), (4, dp[..., H - 1]), (5, sdv), (6, minc), (7, mw2)):
            words[..., i] = np.ascontiguousarray(a, F).view(U)
        words[..., 3], words[..., 8], words[..., 9], words[..., 10] = imax, first, causes, nbad
        # counts over the particles
        bits = np.stack([(cause >> U(k)) & U(1) for k in range(4)] + [(cause != 0).astype(U)], axis=-1)           # [B][P][H][5]
        fail_step = bits.sum(axis=1).astype(U)
        if mutant == "any_is_bit_sum":
            fail_step[..., 4] = fail_step[..., :4].sum(axis=-1)
        if mutant == "padded_lanes_counted":                              # (a padded lane holds anything: counted as failing by radius)
            pad = (-P) % 32
            fail_step[..., 0] += U(pad)
            fail_step[..., 4] += U(pad)
        when = last if mutant == "hist_last_failure" else first
        slot = np.where(when == NONE, U(H), when).astype(np.int64)
        first_fail = np.zeros((B, H + 1), U)
        for b in range(B):
            first_fail[b] = np.bincount(slot[b], minlength=H + 1).astype(U)
        cause_ever = np.stack([((causes >> U(k)) & U(1)).sum(axis=1) for k in range(4)], axis=-1).astype(U)
        # channels per row, aggregates per particle
        vch = ch.reshape(B, P, H * 4)
        agg = np.stack([sdp, mdp, minc, mw2], axis=-1).astype(F)          # [B][P][4]
        out = {"words": words, "fail_step": fail_step, "first_fail": first_fail, "cause_ever": cause_ever,
               "chan_stat": _stats(vch, P, mutant).reshape(B, H, 4, 3), "chan_q": None, "agg_stat": _stats(agg, P, mutant), "agg_q": None}
        if ranks is not None:
            ranks = [int(r) for r in ranks]
            assert 1 <= len(ranks) <= 8 and all(0 <= r < P for r in ranks)
            out["chan_q"] = _select(vch, ranks, mutant).reshape(B, H, 4, len(ranks))
            out["agg_q"] = _select(agg, ranks, mutant)
    return out


BY_VALUE = {"chan_stat": (1, 2), "agg_stat": (1, 2)}                       # min / max: which of +0 and -0 a tie returns is not specified (SPEC.md §12)


def differs(a, b):
    """Number of words that differ between two outcome dicts (or an Outcome tuple's fields by name): integer outputs exactly, float words by bit pattern with
    NaNs compared as a class, the min / max columns of the two stat outputs by value."""
    n = 0
    for k in OUTPUTS:
        x, y = (a[k] if isinstance(a, dict) else getattr(a, k)), (b[k] if isinstance(b, dict) else getattr(b, k))
        if x is None or y is None:
            assert x is None and y is None, k
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, x.dtype, y.shape, y.dtype)
        if k == "words":
            d = x != y
            for w in FLOAT_WORDS:
                d[..., w] &= ~(np.isnan(x[..., w].view(F)) & np.isnan(y[..., w].view(F)))
        elif x.dtype == U:
            d = x != y
        else:
            d = (x.view(U) != y.view(U)) & ~(np.isnan(x) & np.isnan(y))
            for j in BY_VALUE.get(k, ()):
                d[..., j] = (x[..., j] != y[..., j]) & ~(np.isnan(x[..., j]) & np.isnan(y[..., j]))
        n += int(d.sum())
    return n
