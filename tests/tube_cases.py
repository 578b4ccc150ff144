"""The cases of the predicted-tube tests (SPEC.md §12), shared by tests/test_tube_cpu.py and tests/test_gpu_tube.py.

Small shapes at which the reducer can go wrong: H = 6 gives 91 columns (two full tiles of 32 columns and one of 27), H = 7 with six motors 104 (a fourth tile of 8);
P = 1 (31 padded lanes, the lane layout of the rollout), 31 / 33 (one lane short of / past a group), 32 (no padding), 70 (three groups, the duo layout's odd group),
130 (five groups: the slot index g mod 4 wraps). B = 3 with distinct initial states. The vehicles and configurations are the asymmetric ones of tests/cases.py.

Everything a test compares against is computed ONCE per case from the CPU oracle (tensor, mean trajectory, cost) and cached for the process."""
import functools

import numpy as np

import cases as CS
import orc

B = 3
#        name            H  m  P
SHAPES = (("h6_p1", 6, 4, 1), ("h6_p31", 6, 4, 31), ("h6_p32", 6, 4, 32), ("h6_p33", 6, 4, 33), ("h6_p70", 6, 4, 70), ("h6_p130", 6, 4, 130),
          ("h7_m6_p33", 7, 6, 33))
NAMES = tuple(s[0] for s in SHAPES)
BIG = ("h6_p70", "h6_p130")            # the cases the matrix-pipe / fast arithmetics run as well
BOUNDED = (0, 1, 2, 3, 4, 5, 10, 11, 12)   # position, velocity and body-rate components carry bounds; the attitude has none (-inf / +inf)


def config(name, mlp_dtype="f32", math_mode="exact"):
    _, H, m, P = SHAPES[NAMES.index(name)]
    return CS.asymmetric_cfg(m, horizon=H, num_short_dt=H, num_particles=P, mlp_dtype=mlp_dtype, math_mode=math_mode), CS.asymmetric_model(m)


def problem(name):
    """(x0, u, xref, noise) of the case: B instances with distinct initial states"""
    cfg, _ = config(name)
    x0, xref, noise, u = CS.asymmetric_problem(cfg, B, seed=3 + NAMES.index(name))
    return x0, u, xref, noise


def oracle_rollout(cfg, model, x0, u, xref, noise):
    """-> (cost f32[B], tensor f32[B][P][H+1][13], mean f32[B][H+1][13]) of the CPU oracle"""
    O = orc.Oracle(cfg, model)
    out = [O.rollout(x0[b], u[b], xref[b], noise[b], want_traj=True, want_mean=True) for b in range(x0.shape[0])]
    return np.array([o[0] for o in out], np.float32), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def bounds_from(traj):
    """Bounds cut from the tensor itself: for each bounded component, lo and hi are the values of two particles of the tensor at t >= 1, so at least one particle
    sits exactly ON each bound, which is what tells `>=` from `>`. The instances start far apart, so one interval cannot cut through every column: lo is the
    candidate (of up to 256 order statistics over instances, particles and steps) that leaves the most columns with particles on both sides, hi the candidate
    above it that does so given lo. P = 1 (a column then has 0 or 1 outside): the 30 % and 70 % order statistics."""
    lo, hi = np.full(13, -np.inf, np.float32), np.full(13, np.inf, np.float32)
    P = traj.shape[1]
    for i in BOUNDED:
        cols = traj[:, :, 1:, i].transpose(1, 0, 2).reshape(P, -1)         # [P][columns]
        v = np.sort(cols.reshape(-1))
        if P == 1:
            lo[i], hi[i] = v[int(0.3 * (v.size - 1))], v[int(0.7 * (v.size - 1))]
            continue
        cand = v[np.unique(np.linspace(0, v.size - 1, 256).astype(int))]

        def mixed(l, h):
            out = ((cols < l) | (cols > h)).sum(axis=0)
            return int(((out > 0) & (out < P)).sum())
        lo[i] = cand[int(np.argmax([mixed(c, np.inf) for c in cand]))]
        above = cand[cand > lo[i]]
        hi[i] = above[int(np.argmax([mixed(lo[i], c) for c in above]))] if above.size else np.inf
    return lo, hi


@functools.lru_cache(maxsize=None)
def reference(name, mlp_dtype="f32", math_mode="exact"):
    """-> dict: cfg, model, x0, u, xref, noise, cost, traj, xmean (the oracle's), lo, hi. Read-only: the arrays are shared by every test of the process."""
    cfg, model = config(name, mlp_dtype, math_mode)
    x0, u, xref, noise = problem(name)
    cost, traj, xmean = oracle_rollout(cfg, model, x0, u, xref, noise)
    lo, hi = bounds_from(traj)
    d = dict(cfg=cfg, model=model, x0=x0, u=u, xref=xref, noise=noise, cost=cost, traj=traj, xmean=xmean, lo=lo, hi=hi)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def nonfinite_variant(name, b=1):
    """The case's inputs with the initial state of instance b all NaN (every word of its tensor is then NaN): (x0, u, xref, noise)"""
    x0, u, xref, noise = problem(name)
    x0 = x0.copy()
    x0[b, :] = np.nan
    return x0, u, xref, noise
