"""Golden-case definitions shared by tests/golden/make_golden.py and the tests."""
import os

import numpy as np

from sde4mbrl_px4_amd import MPCConfig, load_mpc_config, synthetic_hexa, synthetic_iris, synthetic_multirotor
from sde4mbrl_px4_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "configs")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def golden_cases():
    """name -> (MPCConfig, model, seed, curr_t, pos_mode)"""
    c1 = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml"))
    c2 = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml"))
    c3 = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml"))
    sh = load_mpc_config(os.path.join(CDIR, "iris_traj_shipped_h20_p1.yaml"))
    return {
        "c1_posctrl_h20_p32": (c1.replace(max_iter=40, max_no_improvement_iter=40), synthetic_iris(), 3, 0.0, True),
        "c2_traj_h12_p40_small": (c2.replace(horizon=12, num_short_dt=12, num_particles=40, max_iter=25, max_no_improvement_iter=25),
                                  synthetic_iris(), 5, 0.7, False),
        "c3_hexa_h10_p33_small": (c3.replace(horizon=10, num_short_dt=6, long_step_dt=0.1, num_particles=33, max_iter=15,
                                             max_no_improvement_iter=15, discount=0.97), synthetic_hexa(), 7, 1.3, False),
        "iris_shipped_h20_p1": (sh.replace(max_iter=30, max_no_improvement_iter=30), synthetic_iris(), 11, 0.2, False),
        # the matrix-pipe contraction modes (SPEC.md §9, §9b): the oracle evaluates them through its model of the instruction (§9a)
        "c2_traj_h12_p40_f32x3": (c2.replace(horizon=12, num_short_dt=12, num_particles=40, max_iter=25, max_no_improvement_iter=25, mlp_dtype="f32x3"),
                                  synthetic_iris(), 5, 0.7, False),
        "c3_hexa_h10_p33_f16": (c3.replace(horizon=10, num_short_dt=6, long_step_dt=0.1, num_particles=33, max_iter=15,
                                           max_no_improvement_iter=15, discount=0.97, mlp_dtype="f16"), synthetic_hexa(), 7, 1.3, False),
    }


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))


def bits_differ(a, b):
    """Number of f32 words whose bit patterns differ. NaNs are compared as a class (a NaN must sit at the
    same position on both sides, but its sign/payload is not specified: x86 SSE produces 0xFFC00000, gfx950
    0x7FC00000 for the same invalid operation — SPEC.md §3); everything else, including the sign of zero and
    infinities, is compared bit for bit."""
    fa = np.ascontiguousarray(a, np.float32)
    fb = np.ascontiguousarray(b, np.float32)
    assert fa.shape == fb.shape, (fa.shape, fb.shape)
    both_nan = np.isnan(fa) & np.isnan(fb)
    return int(((fa.view(np.uint32) != fb.view(np.uint32)) & ~both_nan).sum())


# ---- vehicles and configurations without the symmetries of the synthetic ones -------------------------------------------------------
# synthetic_iris / _hexa / _multirotor have b3 = 0, b3n = 0, ct0 = 0, Jx == Jy, sF0 == sF1, sT0 == sT1, two distinct sigma, |rotor_dir| = 1 and
# g = 9.81, and every test configuration built on them gives all motors the same uref / bounds / slew bounds: whole terms of SPEC.md §5 never
# reach a compared bit. The fixtures below break each of these, so that a kernel that drops, swaps or mis-indexes one parameter differs from
# the oracle (tests/test_asymmetric_cpu.py proves that every entry is live; tests/test_gpu_asymmetric.py runs the kernels on them).
_UREF_OFF = np.array([0.031, -0.024, 0.012, -0.043, 0.05, -0.008, 0.022, -0.037])
_U_LO = np.array([0.05, 0.02, 0.08, 0.035, 0.065, 0.01, 0.045, 0.09])
_U_HI = np.array([0.93, 0.88, 0.97, 0.85, 0.91, 0.99, 0.83, 0.95])
_SLEW_LO = -np.array([0.02, 0.035, 0.015, 0.05, 0.027, 0.041, 0.012, 0.03])
_SLEW_HI = np.array([0.03, 0.018, 0.045, 0.025, 0.038, 0.014, 0.05, 0.021])


def asymmetric_model(m=4, seed=10):
    """The synthetic vehicle of `m` motors (iris / hexa geometry for m = 4 / 6) with every symmetry broken: mass and g off their defaults,
    Jx, Jy, Jz pairwise distinct, ct0 > 0 (6 % of the hover thrust per rotor), rotor positions scaled and shifted one by one,|rotor_dir| pairwise distinct and
    none 1, six distinct residual scales, six distinct sigma, b3 six distinct non-zero values of 0.15 .. 0.45, b3n = 0.4. Magnitudes stay near
    the synthetic ones (rollouts stay finite); every value carries a seed-dependent jitter of +-4 %, smaller than the gaps between the nominal
    values, so another seed is another vehicle with the same properties."""
    import dataclasses
    base = synthetic_iris(seed) if m == 4 else synthetic_hexa(seed) if m == 6 else synthetic_multirotor(m, seed)
    rng = np.random.default_rng(4242 + 1000 * seed + m)
    f32 = lambda a: np.asarray(a, np.float32)
    jit = lambda n=None: 1.0 + 0.04 * rng.uniform(-1.0, 1.0, n)
    mass, grav = float(np.float32(base.mass * 0.913 * jit())), float(np.float32(9.62 * jit()))
    thrust = base.thrust_poly.astype(np.float64) * [0.93, 1.09, 1.0] * jit(3)
    thrust[2] = 0.06 * mass * grav / m * jit()
    mags = rng.permutation(np.concatenate([np.linspace(0.75, 0.93, (m + 1) // 2), np.linspace(1.07, 1.25, m // 2)]))
    b3 = rng.choice([-1.0, 1.0], 6) * (0.15 + 0.06 * rng.permutation(6)) * jit(6)
    return dataclasses.replace(
        base, mass=mass, grav=grav, inertia=f32(base.inertia * [0.72, 1.17, 1.0] * jit(3)), thrust_poly=f32(thrust),
        moment_poly=f32(base.moment_poly * [0.92, 1.32] * jit(2)),
        rotor_x=f32(base.rotor_x * (1.0 + 0.15 * rng.uniform(-1, 1, m)) + rng.choice([-1, 1], m) * rng.uniform(0.01, 0.02, m)),   # (no rotor stays on an axis)
        rotor_y=f32(base.rotor_y * (1.0 + 0.15 * rng.uniform(-1, 1, m)) + rng.choice([-1, 1], m) * rng.uniform(0.01, 0.02, m)),
        rotor_dir=f32(np.sign(base.rotor_dir) * mags), res_force_scale=f32(np.array([0.3, 0.2, 0.5]) * jit(3)),
        res_torque_scale=f32(base.res_torque_scale * [1.0, 1.5, 1.0] * jit(3)),
        sigma=f32(np.array([0.11, 0.15, 0.19, 0.25, 0.3, 0.36]) * jit(6)), b3=f32(b3), b3n=float(np.float32(0.4 * jit())))


def asymmetric_cfg(m=4, **kw):
    """A configuration whose per-motor settings (uref, both input bounds, both slew bounds) are pairwise distinct, with twelve distinct state
    weights, a discount below 1 and every optional cost term switched on. Keywords override."""
    u0 = {4: 0.71, 6: 0.42}.get(m, 0.6)
    d = dict(input_id=list(range(m)), uref=[float(v) for v in u0 + _UREF_OFF[:m]], input_bound=[[float(a), float(b)] for a, b in zip(_U_LO[:m], _U_HI[:m])],
             u_slew_constr=[[float(a), float(b)] for a, b in zip(_SLEW_LO[:m], _SLEW_HI[:m])], u_slew_constr_coeff=7.0, u_slew_coeff=0.6, uerr=0.9,
             perr=[90.0, 120.0, 210.0], verr=[4.0, 6.5, 9.0], qerr=[2.0, 3.5, 80.0], werr=[0.8, 1.3, 1.9], discount=0.96, res_mult=0.3,
             max_iter=6, max_no_improvement_iter=6)
    d.update(kw)
    return MPCConfig(**d)


def asymmetric_problem(cfg, B, seed=0, noise=True):
    """(x0, xref, noise, u) like _problem of tests/test_gpu_parity.py, except: odd-numbered instances carry the NEGATED initial quaternion
    (the other half of the double cover); the last instance is turned by 150 degrees about a skew axis; the warm starts are not clipped, and
    for every motor j two of its controls lie outside that motor's own bounds, one above hi_j and one below lo_j (the spikes also exceed both
    of its slew bounds), so the per-motor projection of the solve and both branches of the slew penalty are active. noise=False: None
    (callers that draw it from keys)."""
    H, P, m = cfg.horizon, cfg.num_particles, cfg.num_motors
    x0 = W.random_initial_states(B, seed)
    ax = np.array([1.0, -2.0, 0.7]) / np.linalg.norm([1.0, -2.0, 0.7])
    ang = np.deg2rad(150.0)
    x0[B - 1, 6:10] = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax]).astype(np.float32)
    x0[1::2, 6:10] = -x0[1::2, 6:10]
    xref = np.stack([W.reference_window(0.13 * (b % 160), cfg.time_steps) for b in range(B)])
    nz = W.make_noise(B, P, H, seed) if noise else None
    rng = np.random.default_rng(seed + 5)
    u = (np.asarray(cfg.uref, np.float32) + 0.1 * rng.standard_normal((B, H, m))).astype(np.float32)
    lo, hi = np.asarray(cfg.input_bound, np.float32).T
    for j in range(m):
        u[:, (j + 1) % H, j] = hi[j] + np.float32(0.07)
        u[:, (j + 1 + H // 2) % H, j] = lo[j] - np.float32(0.04)
    return x0, xref, nz, u


def _swap(a, i, j):
    a = np.array(a, np.float32, copy=True)
    a[[i, j]] = a[[j, i]]
    return a


def _roll(v):
    return list(v[1:]) + list(v[:1])


def asymmetric_mutants():
    """name -> f(model, cfg) -> (model, cfg): what a kernel that drops, swaps or mis-indexes one parameter computes, stated on the inputs.
    On the synthetic vehicles with a uniform configuration every one of these is the identity."""
    import dataclasses
    R = dataclasses.replace
    return {
        "b3_zeroed": lambda M, c: (R(M, b3=np.zeros(6, np.float32)), c),
        "b3n_zeroed": lambda M, c: (R(M, b3n=0.0), c),
        "ct0_zeroed": lambda M, c: (R(M, thrust_poly=np.array([M.thrust_poly[0], M.thrust_poly[1], 0.0], np.float32)), c),
        "Jx_Jy_swapped": lambda M, c: (R(M, inertia=_swap(M.inertia, 0, 1)), c),
        "sF0_sF1_swapped": lambda M, c: (R(M, res_force_scale=_swap(M.res_force_scale, 0, 1)), c),
        "sigma0_sigma1_swapped": lambda M, c: (R(M, sigma=_swap(M.sigma, 0, 1)), c),
        "rotor_dir_unit_magnitudes": lambda M, c: (R(M, rotor_dir=np.sign(M.rotor_dir).astype(np.float32)), c),
        "uref_rotated": lambda M, c: (M, c.replace(uref=_roll(c.uref))),
        "input_bound_rotated": lambda M, c: (M, c.replace(input_bound=_roll(c.input_bound))),
        "u_slew_constr_rotated": lambda M, c: (M, c.replace(u_slew_constr=_roll(c.u_slew_constr))),
    }


def diverging_single_rotor_case(P=32):
    """A single-rotor vehicle over a 55-step horizon: it tumbles and the explicit-Euler state overflows f32 around t = 53 — cost NaN
    (instance 0) / +inf (instance 1) and a NaN gradient (found by tests/tools/soak.py, case 5495); instance 2 repeats instance 0 at low
    throttle, which stays finite. Exercises SPEC.md §3.7 and the §8 non-finite guard in a mixed batch."""
    B = 2
    m, H, it = 1, 55, 495
    cfg = MPCConfig(horizon=H, num_short_dt=6, short_step_dt=0.05, long_step_dt=0.1, num_particles=P, input_id=[0], input_bound=[[1e-4, 1.0]],
                    uref=[0.55], u_slew_coeff=1.0, max_iter=3, max_no_improvement_iter=6, ls_maxls=5)
    model = synthetic_multirotor(m, seed=it)
    x0 = W.random_initial_states(B, 1000 + it)
    xref = np.stack([W.reference_window(0.2 * b, cfg.time_steps) for b in range(B)])
    noise = W.make_noise(B, P, H, it)
    u = np.clip(0.55 + 0.15 * np.random.default_rng(it).standard_normal((B, H, m)), 1e-4, 1).astype(np.float32)
    x0, xref, noise = (np.concatenate([a, a[:1]]) for a in (x0, xref, noise))
    u = np.concatenate([u, np.full_like(u[:1], 0.02)])
    return cfg, model, x0, xref, noise, u
