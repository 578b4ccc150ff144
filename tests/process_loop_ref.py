"""CPU reference of the closed loop with gusts and estimator bias drawn on the device (SPEC.md §11i): process_rows, the first-order Gauss-Markov row generator,
written with orc.split, orc.normal and the software fma of the NumPy restatement (oracle/sde_mpc_numpy.py), and process_loop_ref, which is age_loop_ref
(tests/age_loop_ref.py) called with disturbance= / meas_bias= set to those rows. So the loop is the already-verified one and the only new arithmetic is the row
generator. Test infrastructure, like age_loop_ref.py.

`mutant` builds a deliberately WRONG generator, for the discrimination tests: "scale_fused" contracts scale * xi into the fma (one rounding instead of two),
"split_swapped" takes the second half of the split as the chain and the first as the draw key, "pair_adjacent" pairs counter 2 i with 2 i + 1 instead of i with
i + W / 2, "dist_per_solve" steps the disturbance process once per solve and holds its row over the period's ticks, "bias_held_on_dropout" does not step the bias
process at a solve whose valid flag is 0, "state_not_carried" starts every step from state_in. pair_adjacent needs normals of words the oracle's `normal` never
pairs, so normal_from_bits restates SPEC.md §7.2 in NumPy; tests/test_process_loop_cpu.py holds it to orc.normal bit for bit on the right pairing."""
import numpy as np

import orc
from age_loop_ref import age_loop_ref
from timed_loop_ref import R2, num_solves

F = np.float32
U32 = np.uint32
MUTANTS = ("scale_fused", "split_swapped", "pair_adjacent", "dist_per_solve", "bias_held_on_dropout", "state_not_carried")
ROW_MUTANTS = ("scale_fused", "split_swapped", "pair_adjacent", "state_not_carried")


def _fma(a, b, c):
    return F(R2.fma(F(a), F(b), F(c)))


def _poly(x, coeffs):
    y = F(coeffs[0])
    for c in coeffs[1:]:
        y = _fma(y, x, F(c))
    return y


def _log(t):
    b = int(np.asarray(t, F).reshape(1).view(U32)[0])
    e = ((b >> 23) & 255) - 126
    m = np.asarray([(b & 0x007FFFFF) | 0x3F000000], U32).view(F)[0]
    if m < F(0.707106781186547524):
        e -= 1
        x = F(F(m + m) - F(1.0))
    else:
        x = F(m - F(1.0))
    z = F(x * x)
    y = _poly(x, (7.0376836292E-2, -1.1514610310E-1, 1.1676998740E-1, -1.2420140846E-1, 1.4249322787E-1, -1.6668057665E-1, 2.0000714765E-1, -2.4999993993E-1,
                  3.3333331174E-1))
    y = F(F(y * x) * z)
    fe = F(e)
    y = _fma(F(-2.12194440e-4), fe, y)
    y = _fma(F(-0.5), z, y)
    return _fma(F(0.693359375), fe, F(x + y))


def _sqrt(a):
    y = F(R2.rsqrt(F(a)))
    s = F(a * y)
    return _fma(_fma(-s, s, a), F(F(0.5) * y), s)


def _erfinv(u):
    w = F(-_log(_fma(-u, u, F(1.0))))
    if w < F(5.0):
        w = F(w - F(2.5))
        p = _poly(w, (2.81022636e-08, 3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164, 0.246640727, 1.50140941))
    else:
        w = F(_sqrt(w) - F(3.0))
        p = _poly(w, (-0.000200214257, 0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047, 1.00167406, 2.83297682))
    return F(p * u)


def normal_from_bits(word):
    """SPEC.md §7.2 restated: the standard normal of one 32-bit word — mantissa-trick uniform in (-1, 1), sqrt(2) erfinv with every fma explicit."""
    lo = F(-0.99999994)
    f = F(np.asarray([(int(word) >> 9) | 0x3F800000], U32).view(F)[0] - F(1.0))
    u = _fma(f, F(2.0), lo)
    if not u > lo:
        u = lo
    return F(F(1.41421354) * _erfinv(u))


def draw(key, W, pairing="half"):
    """normal(key, (W,)) from single words: pairing "half" is the oracle's (counter i with i + W / 2: element i is the first word of block i, element i + W / 2 the
    second), "adjacent" the wrong one (counter 2 i with 2 i + 1)."""
    out = np.zeros(W, F)
    h = W // 2
    for i in range(h):
        a, b = orc.threefry2x32(key, i, i + h) if pairing == "half" else orc.threefry2x32(key, 2 * i, 2 * i + 1)
        out[i], out[i + h] = normal_from_bits(a), normal_from_bits(b)
    return out


def _par(a, B, W, what):
    a = np.asarray(a, F)
    if a.ndim == 1:
        a = a[None]
    assert a.shape in ((1, W), (B, W)), (what, a.shape)
    return a


def process_rows(keys, rho, scale, state, N, W, scheduled=None, mutant=None, step=None):
    """N steps of the process of width W for every episode (SPEC.md §11i). keys uint32[B][2]; rho / scale f32[1 or B][W] (or [W]); state f32[B][W] or None
    (zeros); scheduled f32[N or 1][B or 1][W] or None: the scheduled input d the row is added to. step bool[N][B] or None: where False the process does NOT step
    (chain and state stay, the row repeats the state) — the two loop-level mutants. Returns (rows f32[B][N][W], keys_next uint32[B][2], state_next f32[B][W])."""
    assert mutant is None or mutant in ROW_MUTANTS
    keys = np.asarray(keys, U32)
    B = keys.shape[0]
    keys = keys.reshape(B, 2)
    rho, scale = _par(rho, B, W, "rho"), _par(scale, B, W, "scale")
    state = np.zeros((B, W), F) if state is None else np.asarray(state, F).reshape(B, W)
    if scheduled is not None:
        scheduled = np.asarray(scheduled, F)
        assert scheduled.ndim == 3 and scheduled.shape[0] in (1, N) and scheduled.shape[1] in (1, B) and scheduled.shape[2] == W, scheduled.shape
    rows = np.zeros((B, N, W), F)
    keys_next = np.zeros((B, 2), U32)
    state_next = np.zeros((B, W), F)
    for b in range(B):
        c, g = keys[b].copy(), state[b].copy()
        rh, sc = rho[b if rho.shape[0] > 1 else 0], scale[b if scale.shape[0] > 1 else 0]
        for k in range(N):
            if step is None or step[k][b]:
                c, e = orc.split(c, 2)
                if mutant == "split_swapped":
                    c, e = e, c
                xi = draw(e, W, "adjacent") if mutant == "pair_adjacent" else orc.normal(e, W)
                g0 = state[b] if mutant == "state_not_carried" else g
                if mutant == "scale_fused":
                    g = (rh.astype(np.float64) * g0.astype(np.float64) + sc.astype(np.float64) * xi.astype(np.float64)).astype(F)
                else:
                    t = (sc * xi).astype(F)                       # one float32 rounding
                    g = np.asarray(R2.fma(rh, g0, t), F)
            d = None if scheduled is None else scheduled[k if scheduled.shape[0] > 1 else 0, b if scheduled.shape[1] > 1 else 0]
            rows[b, k] = g if d is None else (d + g).astype(F)    # one float32 add
        keys_next[b], state_next[b] = c, g
    return rows, keys_next, state_next


def process_loop_ref(cfg, model, plants, x0, xref, keys, T, dist_process=None, dist_keys=None, dist_state_in=None, bias_process=None, bias_keys=None,
                     bias_state_in=None, disturbance=None, meas_bias=None, meas_valid=None, S=1, substep_states=False, mutant=None, **kw):
    """The §11i loop: age_loop_ref with disturbance= / meas_bias= set to the rows of process_rows. dist_process / bias_process are (rho, scale) pairs of
    f32[1 or B][W]; a scheduled disturbance ([T or 1][B or 1][6], [T][6] or [6]) / meas_bias ([Ns or 1][B or 1][12], [Ns][12] or [12]) given as well is the d of
    every row. Returns what SdeMpcSolver.closed_loop returns: age_loop_ref's values, then (dist_rows [B][T][6], dist_keys_next, dist_state_next) with a disturbance
    process, then (bias_rows [B][Ns][12], bias_keys_next, bias_state_next) with a bias process, then xsub if asked for."""
    assert mutant is None or mutant in MUTANTS
    x0 = np.asarray(x0, F)
    B, T, S = x0.shape[0], int(T), int(S)
    Ns = num_solves(T, S)

    def sched(a, N, W):
        if a is None:
            return None
        a = np.asarray(a, F)
        if a.ndim == 1:
            a = a[None, None]
        elif a.ndim == 2:
            assert a.shape[0] == N
            a = a[:, None]
        return a
    more = ()
    row_mutant = mutant if mutant in ROW_MUTANTS else None
    if dist_process is not None:
        step = None
        if mutant == "dist_per_solve":
            step = np.repeat((np.arange(T) % S == 0)[:, None], B, axis=1)
        rows, c, g = process_rows(dist_keys, dist_process[0], dist_process[1], dist_state_in, T, 6, sched(disturbance, T, 6), row_mutant, step)
        disturbance = np.ascontiguousarray(rows.transpose(1, 0, 2))
        more += (rows, c, g)
    if bias_process is not None:
        step = None
        if mutant == "bias_held_on_dropout" and meas_valid is not None:
            v = np.asarray(meas_valid)
            v = v.reshape(1, 1) if v.ndim == 0 else (v[:, None] if v.ndim == 1 else v)
            step = np.broadcast_to(v != 0, (Ns, B)) if v.shape[0] > 1 else np.broadcast_to(v != 0, (1, B)).repeat(Ns, axis=0)
        rows, c, g = process_rows(bias_keys, bias_process[0], bias_process[1], bias_state_in, Ns, 12, sched(meas_bias, Ns, 12), row_mutant, step)
        meas_bias = np.ascontiguousarray(rows.transpose(1, 0, 2))
        more += (rows, c, g)
    out = age_loop_ref(cfg, model, plants, x0, xref, keys, T, disturbance=disturbance, meas_bias=meas_bias, meas_valid=meas_valid, S=S,
                       substep_states=substep_states, **kw)
    return out[:-1] + more + out[-1:] if substep_states else out + more
