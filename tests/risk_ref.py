"""SPEC.md §12a (predicted risk) restated in NumPy float32 on a canonical particle x horizon tensor f32[B][P][H+1][13].

Two restatements: `risk` (vectorised over the particles of an instance; the stage cost, the §6.1 particle sum and the software fma are those of the NumPy
restatement oracle/sde_mpc_numpy.py) and `risk_scalar` (one float32 operation at a time, with its own stage cost, its own butterfly, libm's fmaf and the rank
counted straight from the definition of the total order); tests/test_risk_cpu.py holds them against each other bit for bit. MUTANTS is a table of wrong
reducers — each a single plausible slip — that the cases of tests/risk_cases.py must tell from the right one.

Every addition and product below is a float32 operation on float32 operands: rounded once, no reassociation; an fma only where SPEC.md writes one."""
import ctypes
import os
import sys

import numpy as np

from cases import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import sde_mpc_numpy as R2  # noqa: E402

F = np.float32
OUTPUTS = ("exit", "jx", "first_exit", "outside_any", "jstat", "jq", "jtail")
MUTANTS = ("scan_from_1", "bound_strict", "nan_not_counted", "last_exit", "centre_ignored", "box_of_instance_0", "cost_at_x_t", "weight_t_plus_1",
           "padded_lanes_included", "ties_descending", "tail_from_low_end", "tail_over_P", "tail_in_sorted_position", "mean_unrounded")


def _restatement(cfg, model):
    """the NumPy restatement of (cfg, model) for its stage cost, discount table and particle sum: none of them depends on the arithmetic mode of the rollout"""
    return R2.Restatement(cfg.replace(mlp_dtype="f32", math_mode="exact"), model)


def _order(J, descending_ties=False):
    """the total order of §12a: numbers by value, NaNs last, ties by particle index -> (order, rank)"""
    P = J.size
    if descending_ties:
        order = (P - 1 - np.argsort(J[::-1], kind="stable"))      # among equals: the larger index first
        nan = np.isnan(J[order])
        order = np.concatenate([order[~nan], order[nan]])
    else:
        order = np.argsort(J, kind="stable")                      # NaNs last, equals (and +0 / -0) in index order
    rank = np.empty(P, np.int64)
    rank[order] = np.arange(P)
    return order, rank


def risk(traj, cfg, model, xref, lo=None, hi=None, centre=None, ranks=(), tail_k=None, mutant=None):
    """traj f32[B][P][H+1][13]; xref f32[B][H+1][13]; lo / hi f32[B][13] or None (then no exit outputs); centre f32[B][H+1][13] or None (e = x);
    ranks: up to 8 ranks for jq; tail_k: the tail size for jtail. -> dict of OUTPUTS (absent ones: None). mutant: a name of MUTANTS."""
    traj = np.ascontiguousarray(traj, F)
    B, P, T1, _ = traj.shape
    H = T1 - 1
    R = _restatement(cfg, model)
    assert R.H == H
    invP = F(1.0) / F(P)
    out = {k: None for k in OUTPUTS}
    bounded = lo is not None
    if bounded:
        out.update(exit=np.zeros((B, P), np.uint32), first_exit=np.zeros((B, H + 2), np.uint32), outside_any=np.zeros((B, H + 1), np.uint32))
    out.update(jx=np.zeros((B, P), F), jstat=np.zeros((B, 4), F))
    if len(ranks):
        out["jq"] = np.zeros((B, len(ranks)), F)
    if tail_k is not None:
        out["jtail"] = np.zeros(B, F)
    pad = (-P) % 32
    with np.errstate(all="ignore"):
        for b in range(B):
            x = traj[b]
            if bounded:
                bb = 0 if mutant == "box_of_instance_0" else b
                l, h = np.asarray(lo[bb], F), np.asarray(hi[bb], F)
                e = x if centre is None or mutant == "centre_ignored" else x - np.asarray(centre[b], F)[None]
                inside = ((e > l) if mutant == "bound_strict" else (e >= l)) & (e <= h)
                if mutant == "nan_not_counted":
                    inside = inside | np.isnan(e)
                o = (~inside).any(axis=2)                                          # [P][H+1]
                scan = o.copy()
                if mutant == "scan_from_1":
                    scan[:, 0] = False
                t_idx = np.arange(H + 1)
                if mutant == "last_exit":
                    ex = np.where(scan.any(axis=1), (scan * t_idx).max(axis=1), H + 1)
                else:
                    ex = np.where(scan.any(axis=1), np.argmax(scan, axis=1), H + 1)
                out["exit"][b] = ex
                out["first_exit"][b] = np.bincount(ex, minlength=H + 2)
                out["outside_any"][b] = scan.sum(axis=0)
            J = np.zeros(P, F)
            for t in range(H):
                lx = R.stage_cost(x[:, t], xref[b, t]) if mutant == "cost_at_x_t" else R.stage_cost(x[:, t + 1], xref[b, t + 1])
                J = R2.fma(R.disc[t + 1] if mutant == "weight_t_plus_1" else R.disc[t], lx, J)
            out["jx"][b] = J

            def psum(v):
                if mutant == "padded_lanes_included" and pad:                      # (a padded lane of the device tensor holds anything; 1 stands for it)
                    return R.particle_sum(np.concatenate([v, np.ones(pad, F)]).astype(F))
                return R.particle_sum(v)
            tot = psum(J)
            mean = F(tot * invP)
            d = (J.astype(np.float64) - np.float64(tot) / P).astype(F) if mutant == "mean_unrounded" else (J - mean).astype(F)
            var = F(psum((d * d).astype(F)) * invP)
            mn, mx = F(np.inf), F(-np.inf)
            for v in J:
                mn, mx = np.fmin(mn, v), np.fmax(mx, v)
            out["jstat"][b] = (mean, var, mn, mx)
            order, rank = _order(J, mutant == "ties_descending")
            if len(ranks):
                out["jq"][b] = J[order[list(ranks)]]
            if tail_k is not None:
                if mutant == "tail_in_sorted_position":
                    v = np.where(np.arange(P) >= P - tail_k, J[order], F(0.0)).astype(F)
                else:
                    sel = rank < tail_k if mutant == "tail_from_low_end" else rank >= P - tail_k
                    v = np.where(sel, J, F(0.0)).astype(F)
                out["jtail"][b] = F(psum(v) * (invP if mutant == "tail_over_P" else F(1.0) / F(tail_k)))
    return out


# ---- the scalar restatement ------------------------------------------------------------------------------------------------------------
_libm = ctypes.CDLL("libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _fma1(a, b, c):
    return F(_libm.fmaf(float(a), float(b), float(c)))


def _stage_cost_scalar(cfg, x, xr):
    """SPEC.md §5.3 at one state, one operation at a time"""
    l = F(0.0)
    for w, off in ((cfg.perr, 0), (cfg.verr, 3), (cfg.werr, 10)):
        for i in range(3):
            e = F(x[off + i] - xr[off + i])
            l = _fma1(F(F(w[i]) * e), e, l)
    qw, qx, qy, qz = (F(v) for v in x[6:10])
    rw, rx, ry, rz = (F(v) for v in xr[6:10])
    ex = _fma1(rz, qy, _fma1(-ry, qz, _fma1(-rx, qw, F(rw * qx))))
    ey = _fma1(-rz, qx, _fma1(-ry, qw, _fma1(rx, qz, F(rw * qy))))
    ez = _fma1(-rz, qw, _fma1(ry, qx, _fma1(-rx, qy, F(rw * qz))))
    for w, e in ((cfg.qerr[0], ex), (cfg.qerr[1], ey), (cfg.qerr[2], ez)):
        l = _fma1(F(F(w) * e), e, l)
    if cfg.state_id:
        for k, i in enumerate(cfg.state_id):
            w = F(F(cfg.state_penalty[k]) * F(cfg.constr_pen))
            hi = F(x[i] - F(cfg.state_bound[k][1]))
            hi = F(0.0) if hi < 0 else hi
            lo = F(F(cfg.state_bound[k][0]) - x[i])
            lo = F(0.0) if lo < 0 else lo
            l = _fma1(F(w * hi), hi, l)
            l = _fma1(F(w * lo), lo, l)
    return l


def _psum_scalar(vals):
    """SPEC.md §6.1 one addition at a time"""
    P = len(vals)
    G = (P + 31) // 32
    S = [F(0.0)] * 4
    for g in range(G):
        a = [F(vals[g * 32 + l]) if g * 32 + l < P else F(0.0) for l in range(32)]
        for s in (16, 8, 4, 2, 1):
            a = [F(a[i] + a[i ^ s]) for i in range(32)]
        S[g % 4] = F(S[g % 4] + a[0])
    return F(F(F(S[0] + S[1]) + S[2]) + S[3])


def _before(a, q, b, p):
    """is (value a of particle q) in front of (value b of particle p) in the total order?"""
    an, bn = a != a, b != b
    if an or bn:
        return (bn and not an) or (an and bn and q < p)
    return a < b or (a == b and q < p)


def risk_scalar(traj, cfg, model, xref, lo=None, hi=None, centre=None, ranks=(), tail_k=None):
    traj = np.ascontiguousarray(traj, F)
    B, P, T1, _ = traj.shape
    H = T1 - 1
    disc = []
    d = F(1.0) / F(H)
    for _ in range(H + 1):
        disc.append(d)
        d = F(d * F(cfg.discount))
    invP = F(1.0) / F(P)
    out = {k: None for k in OUTPUTS}
    bounded = lo is not None
    if bounded:
        out.update(exit=np.zeros((B, P), np.uint32), first_exit=np.zeros((B, H + 2), np.uint32), outside_any=np.zeros((B, H + 1), np.uint32))
    out.update(jx=np.zeros((B, P), F), jstat=np.zeros((B, 4), F))
    if len(ranks):
        out["jq"] = np.zeros((B, len(ranks)), F)
    if tail_k is not None:
        out["jtail"] = np.zeros(B, F)
    with np.errstate(all="ignore"):
        for b in range(B):
            J = []
            for p in range(P):
                if bounded:
                    ex = H + 1
                    for t in range(H + 1):
                        o = False
                        for i in range(13):
                            e = F(traj[b, p, t, i] - centre[b, t, i]) if centre is not None else traj[b, p, t, i]
                            if not (e >= lo[b][i] and e <= hi[b][i]):
                                o = True
                        if o:
                            out["outside_any"][b, t] += 1
                            if ex == H + 1:
                                ex = t
                    out["exit"][b, p] = ex
                    out["first_exit"][b, ex] += 1
                j = F(0.0)
                for t in range(H):
                    j = _fma1(disc[t], _stage_cost_scalar(cfg, traj[b, p, t + 1], xref[b, t + 1]), j)
                J.append(j)
            out["jx"][b] = J
            mean = F(_psum_scalar(J) * invP)
            sq = []
            for j in J:
                dd = F(j - mean)
                sq.append(F(dd * dd))
            var = F(_psum_scalar(sq) * invP)
            mn, mx = F(np.inf), F(-np.inf)
            for j in J:
                if j == j:
                    mn = j if j < mn else mn
                    mx = j if j > mx else mx
            out["jstat"][b] = (mean, var, mn, mx)
            rank = [sum(1 for q in range(P) if q != p and _before(J[q], q, J[p], p)) for p in range(P)]
            for k, r in enumerate(ranks):
                out["jq"][b, k] = J[rank.index(r)]
            if tail_k is not None:
                out["jtail"][b] = F(_psum_scalar([J[p] if rank[p] >= P - tail_k else F(0.0) for p in range(P)]) * (F(1.0) / F(tail_k)))
    return out


def outputs_differ(a, b):
    """number of compared words in which two results differ: everything by bits (NaNs as a class), min and max (jstat[:, 2:]) by value"""
    n = 0
    for k in OUTPUTS:
        x, y = a[k], b[k]
        assert (x is None) == (y is None), k
        if x is None:
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == np.uint32:
            n += int((x != y).sum())
            continue
        both_nan = np.isnan(x) & np.isnan(y)
        diff = (x.view(np.uint32) != y.view(np.uint32)) & ~both_nan
        if k == "jstat":
            diff[:, 2:] = ((x != y) & ~both_nan)[:, 2:]
        n += int(diff.sum())
    return n
