"""Inputs shared by tests/test_gpu_geo.py (GPU against the reference) and tests/test_geo_cpu.py (the reference against its mutants, its census and its float64
restatement, on the same inputs): the geometric baseline controller of SPEC.md §11l on the asymmetric vehicles of tests/cases.py with m = 3, 4 and 6 motors,
H = 6 with two step lengths, P = 1; loops at B = 5, T = 6 with n in {1, 3}, S in {1, 2}, D in {0, 2}; the stand-alone call at B = 257 (one thread past a 256-thread
block).

The states, by index modulo 8 (an episode keeps its role at every B; every state is finite):
  0  an ordinary flight near the reference
  1  4 m from the reference: the acceleration clip is active
  2  turned by 150 degrees about a skew axis: the desired acceleration points away from the body axis, the thrust command sits at c_lo
  3  3 m below the reference and level: the thrust command sits at c_hi
  4  the GUARD: the reference attitude (1/2, 1/2, 1/2, -1/2), a unit quaternion whose body x axis is vertical, so R00 = R10 = 0 exactly in float32, the heading
     vector is zero and no attitude can be formed (with max_acc below g, as shipped, a zero desired acceleration cannot be reached)
  5, 6, 7  ordinary, from other seeds
Whether each of these happens is not taken on trust: tests/test_geo_cpu.py counts them in the reference's census."""
import numpy as np

from cases import asymmetric_cfg, asymmetric_model
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import GeometricController, RateLoop

F = np.float32
H6, B5, T6, B257 = 6, 5, 6, 257
MOTORS = (3, 4, 6)
# (substeps n, solve period S, solve delay D in plant substeps), D <= S n
SHAPES = ((1, 1, 0), (3, 1, 2), (1, 2, 2), (3, 2, 0), (3, 2, 2))
ALPHA = 0.35
GAINS = dict(kp=[8.0, 7.0, 10.0], kv=[1.5, 1.75, 3.25], max_acc=7.0, attctrl_tau=0.1)
RATE = dict(kp=[0.05, 0.045, 0.09], ki=[0.2, 0.25, 0.3], integ_limit=0.04)


def geo_cfg(m, **kw):
    return asymmetric_cfg(m, **{"horizon": H6, "num_short_dt": 4, "short_step_dt": 0.05, "long_step_dt": 0.1, "num_particles": 1, "max_iter": 3,
                                "max_no_improvement_iter": 3, **kw})


def controller(model, B=None, accel_ff=False, ref_row=0, **kw):
    """for_model gains; B given: one set per episode, every parameter distinct from episode to episode (the thrust clamp included)."""
    g = dict(GAINS, accel_ff=accel_ff, ref_row=ref_row, **kw)
    if B is not None:
        r = np.random.default_rng(31)
        g["kp"] = np.asarray(GAINS["kp"]) * r.uniform(0.7, 1.3, (B, 3))
        g["kv"] = np.asarray(GAINS["kv"]) * r.uniform(0.7, 1.3, (B, 3))
        g["max_acc"] = GAINS["max_acc"] * r.uniform(0.6, 1.2, B)
        g["attctrl_tau"] = GAINS["attctrl_tau"] * r.uniform(0.7, 1.5, B)
        g.setdefault("thrust_min", r.uniform(0.1, 0.2, B))
        g.setdefault("thrust_max", r.uniform(0.7, 0.8, B))
    else:
        g.setdefault("thrust_max", float(F(GeometricController.hover_calibration(model)[0] + 0.15)))     # (below every motor's upper bound on these vehicles)
    return GeometricController.for_model(model, **g)


def params(ctl, cfg, B):
    """The controller's parameter sets as geo_ref takes them, and inv_dt of its ref_row."""
    lo, hi = np.asarray(cfg.input_bound, F).T
    _, par = ctl.arrays(B, lo, hi)
    return par, F(F(1) / F(cfg.time_steps[ctl.ref_row]))


def rate_loop(**kw):
    return RateLoop(**{**RATE, **kw})


def states(cfg, model, ctl, B, seed=300):
    """(x f32[B][13], xref f32[B][H+1][13]) with the roles of the module docstring, for the controller's ref_row and parameter sets."""
    x = W.random_initial_states(B, seed)
    x[:, 0:6] *= F(0.3)
    xref = np.stack([W.reference_window(0.1 * (b % 40), cfg.time_steps) for b in range(B)]).astype(F)
    rho = ctl.ref_row
    x[:, 0:3] += xref[:, rho, 0:3]
    ax = np.array([1.0, -2.0, 0.7]) / np.linalg.norm([1.0, -2.0, 0.7])
    ang = np.deg2rad(150.0)
    for b in range(B):
        role = b % 8
        if role == 1:
            x[b, 0:3] = xref[b, rho, 0:3] + np.array([2.5, -2.5, 2.0], F)
        elif role == 2:
            x[b, 6:10] = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax]).astype(F)
        elif role == 3:
            x[b, 0:3] = xref[b, rho, 0:3] + np.array([0.0, 0.0, -3.0], F)
            x[b, 3:6] = xref[b, rho, 3:6]
            x[b, 6:10] = [1.0, 0.0, 0.0, 0.0]
        elif role == 4:
            xref[b, rho, 6:10] = [0.5, 0.5, 0.5, -0.5]
    return x, xref


def episodes(cfg, model, ctl, B=B5, seed=300):
    """(x0, xref f32[1][B][H+1][13], keys) of a loop."""
    x0, xref = states(cfg, model, ctl, B, seed)
    keys = np.stack([prng.PRNGKey(seed + b) for b in range(B)])
    return x0, xref[None], keys


def timing(n, S, D):
    return dict(plant_substeps=n, solve_period=S, solve_delay=D, motor_lag=ALPHA)
