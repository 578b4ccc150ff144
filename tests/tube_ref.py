"""SPEC.md §12 (predicted tube) restated in NumPy float32 on a canonical particle x horizon tensor f32[B][P][H+1][13].

Two restatements: `tube` (vectorised over instances and columns, the butterfly written out stage by stage) and `tube_scalar` (one float32 operation at a time);
tests/test_tube_cpu.py holds them against each other bit for bit and `tube`'s mean against the oracle's mean trajectory. MUTANTS is a table of wrong reducers — each a
single plausible slip — that the committed cases (tests/tube_cases.py) must tell from the right one.

Every addition and product below is a float32 NumPy operation on float32 operands: rounded once, no fma, no reassociation. Nothing here uses np.sum / np.mean."""
import numpy as np

PLANES = ("mean", "var", "min", "max", "outside")
BITS_PLANES = ("mean", "var", "outside")      # compared bit for bit; min / max by value (a tie between +0 and -0 is unspecified, SPEC.md §12)
F = np.float32
_LANE = np.arange(32)
STRIDES = (16, 8, 4, 2, 1)


def _groups(v, fill):
    """[B][P][C] -> [B][G][32][C], the padded lanes of the last group set to `fill`"""
    B, P, C = v.shape
    G = (P + 31) // 32
    out = np.full((B, G * 32, C), fill, F)
    out[:, :P] = v
    return out.reshape(B, G, 32, C)


def _butterfly(a, op=np.add, strides=STRIDES):
    """SPEC.md §6.1 over axis 2 (the 32 lanes): v_i <- op(v_i, v_{i ^ s}) for s = 16, 8, 4, 2, 1; the group total is in every lane, lane 0 is returned"""
    for s in strides:
        a = op(a, a[:, :, _LANE ^ s, :])
    return a[:, :, 0, :]


def _slots(T, sequential=False):
    """group totals [B][G][C] -> total [B][C]: slot g mod 4 in ascending g, ((S0 + S1) + S2) + S3"""
    B, G, C = T.shape
    if sequential:
        acc = np.zeros((B, C), F)
        for g in range(G):
            acc = acc + T[:, g]
        return acc
    S = [np.zeros((B, C), F) for _ in range(4)]
    for g in range(G):
        S[g % 4] = S[g % 4] + T[:, g]
    return ((S[0] + S[1]) + S[2]) + S[3]


def _fma_stage16(d, qpad):
    """the first butterfly stage with the product left unrounded inside an fma: fma(d_i, d_i, q_{i ^ 16}) (mutant 5). A float64 product of two float32 values is exact."""
    return (d.astype(np.float64) * d.astype(np.float64) + qpad[:, :, _LANE ^ 16, :].astype(np.float64)).astype(F)


def tube(traj, lo=None, hi=None, mutant=None):
    """traj: f32[B][P][H+1][13]. lo / hi: 13 bounds each (None: -inf / +inf). -> dict of the five planes, each [B][H+1][13] (outside: uint32).
    mutant: None, or a name of MUTANTS — then what that wrong reducer computes."""
    traj = np.ascontiguousarray(traj, F)
    B, P, T1, NX = traj.shape
    assert NX == 13
    C = T1 * 13
    lo = np.full(13, -np.inf, F) if lo is None else np.asarray(lo, F)
    hi = np.full(13, np.inf, F) if hi is None else np.asarray(hi, F)
    v = traj.reshape(B, P, C)                      # column c = t * 13 + i
    invP = F(1.0) / F(P)
    valid = (np.arange(((P + 31) // 32) * 32) < P).reshape(1, -1, 32, 1)
    with np.errstate(all="ignore"):
        included = mutant == "padded_lanes_included"
        pad = F(1.0) if included else F(0.0)               # (a padded lane of the device tensor holds anything; 1 stands for it)
        strides = STRIDES[::-1] if mutant == "strides_ascending" else STRIDES
        seq = mutant == "slots_sequential"
        gv = _groups(v, pad)
        total = _slots(_butterfly(gv, strides=strides), seq)
        mean = total * invP
        if mutant == "mean_unrounded":
            d = (gv.astype(np.float64) - (total.astype(np.float64) / P)[:, None, None, :]).astype(F)
        else:
            d = gv - mean[:, None, None, :]
        q = d * d if included else np.where(valid, d * d, F(0.0)).astype(F)
        if mutant == "q_fma":
            Tq = _butterfly(_fma_stage16(np.where(valid, d, F(0.0)).astype(F), q), strides=STRIDES[1:])
        else:
            Tq = _butterfly(q, strides=strides)
        var = _slots(Tq, seq) * (F(1.0) / F(P - 1) if mutant == "bessel" and P > 1 else invP)
        ext_pad = mutant == "extrema_over_padded_lanes"    # (zero padding taken for data)
        # fmin / fmax ignore a NaN operand; a column whose particles are all NaN keeps the start value
        mn = np.fmin(np.fmin.reduce(_butterfly(_groups(v, F(0.0) if ext_pad else F(np.inf)), np.fmin), axis=1), F(np.inf)).astype(F)
        mx = np.fmax(np.fmax.reduce(_butterfly(_groups(v, F(0.0) if ext_pad else F(-np.inf)), np.fmax), axis=1), F(-np.inf)).astype(F)
        lo_c, hi_c = np.tile(lo, T1), np.tile(hi, T1)
        lower_ok = v > lo_c if mutant == "bound_strict" else v >= lo_c
        inside = lower_ok & (v <= hi_c)
        if mutant == "nan_not_counted":
            inside = inside | np.isnan(v)
        outside = np.zeros((B, C), np.uint32)
        for p in range(P):
            outside = outside + (~inside[:, p]).astype(np.uint32)
    out = {"mean": mean, "var": var, "min": mn, "max": mx, "outside": outside}
    if mutant == "column_transposed":                  # column index i * (H + 1) + t
        out = {k: a.reshape(B, T1, 13).transpose(0, 2, 1).reshape(B, C) for k, a in out.items()}
    return {k: np.ascontiguousarray(a).reshape(B, T1, 13) for k, a in out.items()}


MUTANTS = ("padded_lanes_included", "slots_sequential", "bessel", "mean_unrounded", "q_fma", "strides_ascending", "bound_strict", "nan_not_counted",
           "column_transposed", "extrema_over_padded_lanes")


def _bfly_scalar(vals, op):
    a = list(vals)
    for s in STRIDES:
        a = [op(a[i], a[i ^ s]) for i in range(32)]
    return a[0]


def _fmin(a, b):
    return b if a != a else a if b != b else (a if a < b else b)


def _fmax(a, b):
    return b if a != a else a if b != b else (a if a > b else b)


def tube_scalar(traj, lo=None, hi=None):
    """The same arithmetic one float32 operation at a time: per instance, per column, per group, per lane."""
    traj = np.ascontiguousarray(traj, F)
    B, P, T1, _ = traj.shape
    G = (P + 31) // 32
    lo = np.full(13, -np.inf, F) if lo is None else np.asarray(lo, F)
    hi = np.full(13, np.inf, F) if hi is None else np.asarray(hi, F)
    invP = F(1.0) / F(P)
    out = {k: np.zeros((B, T1, 13), np.uint32 if k == "outside" else F) for k in PLANES}
    zero, pinf, ninf = F(0.0), F(np.inf), F(-np.inf)
    add = lambda x, y: F(x + y)

    def total(lane_value):
        S = [zero, zero, zero, zero]
        for g in range(G):
            S[g % 4] = F(S[g % 4] + _bfly_scalar([lane_value(g * 32 + l) if g * 32 + l < P else zero for l in range(32)], add))
        return F(F(F(S[0] + S[1]) + S[2]) + S[3])

    with np.errstate(all="ignore"):
        for b in range(B):
            for t in range(T1):
                for i in range(13):
                    col = [F(x) for x in traj[b, :, t, i]]
                    mean = F(total(lambda p: col[p]) * invP)

                    def sq(p):
                        d = F(col[p] - mean)
                        return F(d * d)
                    var = F(total(sq) * invP)
                    mn, mx, cnt = pinf, ninf, 0
                    for g in range(G):
                        mn = _fmin(mn, _bfly_scalar([col[g * 32 + l] if g * 32 + l < P else pinf for l in range(32)], _fmin))
                        mx = _fmax(mx, _bfly_scalar([col[g * 32 + l] if g * 32 + l < P else ninf for l in range(32)], _fmax))
                    for p in range(P):
                        if not (col[p] >= lo[i] and col[p] <= hi[i]):
                            cnt += 1
                    out["mean"][b, t, i], out["var"][b, t, i], out["min"][b, t, i], out["max"][b, t, i], out["outside"][b, t, i] = mean, var, mn, mx, cnt
    return out


def planes_differ(a, b):
    """number of compared words in which two tube results differ: mean, var and outside by bits (NaNs as a class), min and max by value"""
    n = 0
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if k == "outside":
            n += int((x.astype(np.uint32) != y.astype(np.uint32)).sum())
            continue
        x, y = x.astype(F), y.astype(F)
        both_nan = np.isnan(x) & np.isnan(y)
        if k in BITS_PLANES:
            n += int(((x.view(np.uint32) != y.view(np.uint32)) & ~both_nan).sum())
        else:
            n += int(((x != y) & ~both_nan).sum())
    return n
