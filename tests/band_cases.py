"""The cases of the predicted-bands tests (SPEC.md §12b), shared by tests/test_band_cpu.py and tests/test_gpu_band.py.

Shapes: H = 6 with four motors gives 91 columns (two full tiles of 32 columns and one of 27), H = 7 with six motors 104. P = 1 (31 padded lanes), 31 / 32 / 33
(one lane short of a group, none padded, one past), 70 (three groups), 128 (the full in-register sort: no padded key), 130 and 300 (five and ten groups: the
ragged select path), 1024 (32 groups, H = 6 only). B = 3 with distinct initial states; vehicles and configurations are the asymmetric ones of tests/cases.py.

Ranks: {0, 1, P//2, P-2, P-1} clamped, with a duplicate, in unsorted order; Q = 8 at P = 70 and Q = 1 at P = 33.

Observations are cut from the oracle's own tensor, per column in rotation: a particle's value, the midpoint of two neighbours in sorted order, a value beyond each
extreme, NaN in one column of sixteen, and the t = 0 row equal to x0.

Everything a test compares against is computed ONCE per case from the CPU oracle and cached for the process."""
import functools

import numpy as np

import band_ref as BR
import cases as CS
import tube_cases as TC

B = 3
#        name             H  m  P
SHAPES = (("h6_p1", 6, 4, 1), ("h6_p31", 6, 4, 31), ("h6_p32", 6, 4, 32), ("h6_p33", 6, 4, 33), ("h6_p70", 6, 4, 70), ("h6_p128", 6, 4, 128),
          ("h6_p130", 6, 4, 130), ("h6_p300", 6, 4, 300), ("h6_p1024", 6, 4, 1024), ("h7_m6_p33", 7, 6, 33), ("h7_m6_p130", 7, 6, 130))
NAMES = tuple(s[0] for s in SHAPES)
BIG = ("h6_p70", "h6_p130")            # the cases the matrix-pipe / fast arithmetics run as well


def shape(name):
    return SHAPES[NAMES.index(name)][1:]


def config(name, mlp_dtype="f32", math_mode="exact"):
    H, m, P = shape(name)
    return CS.asymmetric_cfg(m, horizon=H, num_short_dt=H, num_particles=P, mlp_dtype=mlp_dtype, math_mode=math_mode), CS.asymmetric_model(m)


def problem(name):
    """(x0, u, xref, noise) of the case: B instances with distinct initial states"""
    cfg, _ = config(name)
    x0, xref, noise, u = CS.asymmetric_problem(cfg, B, seed=11 + NAMES.index(name))
    return x0, u, xref, noise


def ranks(name):
    """the ranks of the case, unsorted, with a duplicate"""
    P = shape(name)[2]
    c = lambda r: min(P - 1, max(0, r))
    if name == "h6_p33":
        return [c(P // 2)]                                                        # Q = 1
    base = [c(P - 1), 0, c(P // 2), c(1), c(P - 2), c(P // 2)]                    # Q = 6
    if name == "h6_p70":
        base += [c(P // 4), c(3 * P // 4)]                                        # Q = 8
    return base


def observations(traj, x0):
    """obs f32[B][H+1][13] cut from the tensor f32[B][P][H+1][13]; column c = t 13 + i of instance b takes kind (c + b) mod 16 == 0 -> NaN, else (c + b) mod 5:
    0 / 3 a particle's value (sorted rank 1 + 5 c mod (P - 1), so something lies below it), 1 the float32 midpoint of two neighbours in sorted order, 2 the next
    float32 below the minimum, 4 the next float32 above the maximum. The t = 0 row is x0."""
    Bn, P, T, nx = traj.shape
    s = BR.words(np.sort(BR.keys(traj), axis=1))                                   # sorted by key, [B][P][T][13]
    obs = np.zeros((Bn, T, nx), np.float32)
    for b in range(Bn):
        for t in range(T):
            for i in range(nx):
                c = t * nx + i
                col = s[b, :, t, i]
                kind = (c + b) % 5
                r = 1 + (5 * c) % (P - 1) if P > 1 else 0
                if (c + b) % 16 == 0:
                    v = np.float32(np.nan)
                elif kind in (0, 3):
                    v = col[r]
                elif kind == 1:
                    v = np.float32((np.float64(col[r - 1 if P > 1 else 0]) + np.float64(col[r])) / 2)
                elif kind == 2:
                    v = np.nextafter(col[0], np.float32(-np.inf))
                else:
                    v = np.nextafter(col[P - 1], np.float32(np.inf))
                obs[b, t, i] = v
    obs[:, 0, :] = x0
    return obs


@functools.lru_cache(maxsize=None)
def reference(name, mlp_dtype="f32", math_mode="exact"):
    """-> dict: cfg, model, x0, u, xref, noise, cost, traj (the oracle's), ranks, obs, want (band_ref.bands of the oracle's tensor). Read-only."""
    cfg, model = config(name, mlp_dtype, math_mode)
    x0, u, xref, noise = problem(name)
    cost, traj, _ = TC.oracle_rollout(cfg, model, x0, u, xref, noise)
    rk = ranks(name)
    obs = observations(traj, x0)
    want = BR.bands(traj, rk, obs)
    d = dict(cfg=cfg, model=model, x0=x0, u=u, xref=xref, noise=noise, cost=cost, traj=traj, ranks=tuple(rk), obs=obs, want=want)
    for a in list(d.values()) + list(want.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


# ---- special values: they reach the device tensor through the caller's noise and x0 only ------------------------------------------------------------------
ZERO_COMPONENT = 4          # the x0 component set to -0.0 in instances 0 and 2


def special_problem(name):
    """The case's inputs with: particles 0 and 1 on identical noise rows (exact ties at every step); particles 2, 3, 4 on NaN noise (partly-NaN columns);
    instance 1 with an all-NaN x0; component ZERO_COMPONENT of x0 set to -0.0 in instances 0 and 2. -> (x0, u, xref, noise)"""
    x0, u, xref, noise = problem(name)
    x0, noise = x0.copy(), noise.copy()
    assert noise.shape[1] >= 6
    noise[:, 1] = noise[:, 0]
    noise[:, 2:5] = np.nan
    x0[1, :] = np.nan
    x0[0, ZERO_COMPONENT] = np.float32(-0.0)
    x0[2, ZERO_COMPONENT] = np.float32(-0.0)
    return x0, u, xref, noise


def special_observations(traj, x0):
    """observations() of the tensor, with the t = 0 word of ZERO_COMPONENT +0.0 in instance 0 (every particle there is -0.0: below = P, at = 0) and -0.0 in
    instance 2 (below = 0, at = P)"""
    obs = observations(traj, x0)
    obs[0, 0, ZERO_COMPONENT] = np.float32(0.0)
    obs[2, 0, ZERO_COMPONENT] = np.float32(-0.0)
    return obs


def synthetic_special(name):
    """For the CPU tests, which have no device tensor: the oracle's tensor of the case with the special values planted directly — particle 1 a copy of particle 0,
    particles 2 .. 4 NaN from t = 1 on, instance 1 all NaN, component ZERO_COMPONENT at t = 0 exactly -0.0 in instances 0 and 2, and one column holding both
    zeros. -> (traj, x0, obs)"""
    R = reference(name)
    traj, x0 = R["traj"].copy(), R["x0"].copy()
    traj[:, 1] = traj[:, 0]
    traj[:, 2:5, 1:] = np.nan
    traj[1] = np.nan
    x0[1] = np.nan
    for b in (0, 2):
        traj[b, :, 0, ZERO_COMPONENT] = np.float32(-0.0)
        x0[b, ZERO_COMPONENT] = np.float32(-0.0)
    traj[0, 5:, 3, 2] = np.float32(0.0)            # +0.0 in most particles of one column, -0.0 in two of them
    traj[0, 0:2, 3, 2] = np.float32(-0.0)
    return traj, x0, special_observations(traj, x0)
