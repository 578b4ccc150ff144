"""CPU reference of the episode score of SPEC.md §11h: score_rows is a pure NumPy float32 function of a closed loop's OUTPUTS — xs, us, info and, for a substep
score, xsub — and of the target rows, so that composed with age_loop_ref (tests/age_loop_ref.py) it is the CPU reference of sdempc_closed_loop_batch_scored, and
applied to what a device call returned it checks the device's words against the device's own rows. Every fma is R2.fma of the NumPy restatement
(oracle/sde_mpc_numpy.py), as in age_loop_ref.py; every other operation is one float32 operation. Test infrastructure.

`mutant` builds a deliberately WRONG score, for the discrimination tests: "target_of_xk" compares the target of tick k with the state BEFORE each scored row
(x_k for a tick score), "nan_passes" tests dp > r2_pos in place of !(dp <= r2_pos), "last_max" keeps the last maximum of dp (dp >= max replaces), "tilt_from_wz"
forms the tilt cosine from qw and qz, "strict_saturation" counts u < u_lo or u > u_hi, "flat_le" counts solves with !(opt_cost <= init_cost)."""
import numpy as np

from timed_loop_ref import R2

F = np.float32
U = np.uint32
WORDS = 16
MUTANTS = ("target_of_xk", "nan_passes", "last_max", "tilt_from_wz", "strict_saturation", "flat_le")
FLOAT_WORDS = (1, 2, 4, 5, 6, 7, 12)
NONE = U(0xFFFFFFFF)


def f2u(v):
    return np.asarray(v, F).reshape(1).view(U)[0]


def u2f(v):
    return np.asarray(v, U).reshape(1).view(F)[0]


def initial_rows(B):
    """u32[B][16]: zeros, word 6 = +inf, word 8 = 0xffffffff."""
    z = np.zeros((B, WORDS), U)
    z[:, 6] = f2u(np.inf)
    z[:, 8] = NONE
    return z


def as_words(score):
    """u32[B][16] of a structured score array [B] (SdeMpcSolver.closed_loop) or of a plain word array."""
    a = np.ascontiguousarray(score)
    return a.view(U).reshape(a.shape[0], WORDS).copy()


def words_differ(a, b):
    """Number of score words that differ between two u32[B][16] arrays: integer words as integers, float words by bit pattern with NaNs compared as a class."""
    a, b = as_words(a), as_words(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = a != b
    for w in FLOAT_WORDS:
        fa, fb = a[:, w].view(F), b[:, w].view(F)
        d[:, w] &= ~(np.isnan(fa) & np.isnan(fb))
    return int(d.sum())


def count_u32(v):
    """(u32)v of a telemetry count: v itself where 0 <= v < 2^32, else 0 (a NaN included)."""
    v = F(v)
    return U(int(v)) if (v >= F(0.0) and v < F(4294967296.0)) else U(0)


def sq3(a, b, c):
    return R2.fma(c, c, R2.fma(b, b, F(a * a)))


def row_terms(x, g, mutant=None):
    """(dp, dv, c, w2, nf) of one scored row x against the target g."""
    x, g = np.asarray(x, F), np.asarray(g, F)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (x[:6] - g[:6]).astype(F)
        dp = F(sq3(e[0], e[1], e[2]))
        dv = F(sq3(e[3], e[4], e[5]))
        a, b = (x[6], x[9]) if mutant == "tilt_from_wz" else (x[7], x[8])
        c = F(R2.fma(F(-2.0), F(F(a * a) + F(b * b)), F(1.0)))
        w2 = F(sq3(x[10], x[11], x[12]))
        nf = bool((~(np.abs(x) < F(np.inf))).any())
    return dp, dv, c, w2, nf


def score_rows(xs, us, info, xsub, score_ref, cfg, thresholds, substeps, S, score_in=None, mutant=None):
    """u32[B][16], the score words of SPEC.md §11h after a run with outputs xs [B][T+1][13], us [B][T][m], info [B][Ns][8] (Ns = ceil(T / S)) and, with substeps
    true, xsub [B][T n][13]. score_ref is [Tr][Br][13] with Tr in {1, T} and Br in {1, B} (or [T][13], or [13]); thresholds = (r2_pos, cos_min, w2_max) as float32;
    cfg (an MPCConfig) gives u_lo, u_hi, uref as its C struct holds them; score_in u32[B][16] (or a structured score array) continues a score, None starts from initial_rows."""
    assert mutant is None or mutant in MUTANTS
    xs, us, info = np.asarray(xs, F), np.asarray(us, F), np.asarray(info, F)
    B, T, m = xs.shape[0], xs.shape[1] - 1, us.shape[2]
    assert us.shape[:2] == (B, T) and info.shape == (B, -(-T // int(S)), 8)
    g = np.asarray(score_ref, F)
    if g.ndim == 1:
        g = g[None, None]
    elif g.ndim == 2:
        assert g.shape[0] == T
        g = g[:, None]
    Tr, Br = g.shape[:2]
    assert Tr in (1, T) and Br in (1, B) and g.shape[2] == 13
    r2, cmin, w2max = (F(t) for t in thresholds)
    assert not (np.isnan(r2) or np.isnan(cmin) or np.isnan(w2max))
    cc, _keep = cfg.to_cfg()                             # u_lo / u_hi / uref as the handle holds them (enforce_ubound included)
    lo, hi, uref = (np.asarray(list(v)[:m], F) for v in (cc.u_lo, cc.u_hi, cc.uref))
    n = 1
    if substeps:
        xsub = np.asarray(xsub, F)
        n = xsub.shape[1] // T
        assert xsub.shape == (B, T * n, 13)
    out = initial_rows(B) if score_in is None else as_words(score_in)
    assert out.shape == (B, WORDS)
    for b in range(B):
        w = out[b]
        cnt, imax, first, causes, nbad = w[0], w[3], w[8], w[9], w[10]
        sdp, mdp, ldp, sdv, minc, mw2 = (u2f(w[i]) for i in (1, 2, 4, 5, 6, 7))
        rows = xsub[b] if substeps else xs[b, 1:]
        before = np.concatenate([xs[b, :1], rows[:-1]])                  # the state in front of each scored row
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(T):
                gk = g[k if Tr > 1 else 0, b if Br > 1 else 0]
                for jj in range(n):
                    r = k * n + jj
                    dp, dv, c, w2, nf = row_terms((before if mutant == "target_of_xk" else rows)[r], gk, mutant)
                    out_p = bool(dp > r2) if mutant == "nan_passes" else not bool(dp <= r2)
                    cause = U(1 * out_p + 2 * (not bool(c >= cmin)) + 4 * (not bool(w2 <= w2max)) + 8 * nf)
                    sdp = F(sdp + dp)
                    if (dp >= mdp) if mutant == "last_max" else (dp > mdp):
                        mdp, imax = dp, cnt
                    ldp = dp
                    sdv = F(sdv + dv)
                    if c < minc:
                        minc = c
                    if w2 > mw2:
                        mw2 = w2
                    if cause:
                        if first == NONE:
                            first = cnt
                        causes |= cause
                        nbad = U(nbad + U(1))
                    cnt = U(cnt + U(1))
            sat, sdu = w[11], u2f(w[12])
            for k in range(T):
                u = us[b, k]
                a = F(0.0)
                for j in range(m):
                    d = F(u[j] - uref[j])
                    if (u[j] < lo[j] or u[j] > hi[j]) if mutant == "strict_saturation" else (u[j] <= lo[j] or u[j] >= hi[j]):
                        sat = U(sat + U(1))
                    a = F(R2.fma(d, d, a))
                sdu = F(sdu + a)
            nit, nls, flat = w[13], w[14], w[15]
            for j in range(info.shape[1]):
                i = info[b, j]
                nit = U((int(nit) + int(count_u32(i[2]))) & 0xFFFFFFFF)
                nls = U((int(nls) + int(count_u32(i[7]))) & 0xFFFFFFFF)
                if not ((i[6] <= i[5]) if mutant == "flat_le" else (i[6] < i[5])):
                    flat = U(flat + U(1))
        out[b] = [cnt, f2u(sdp), f2u(mdp), imax, f2u(ldp), f2u(sdv), f2u(minc), f2u(mw2), first, causes, nbad, sat, f2u(sdu), nit, nls, flat]
    return out
