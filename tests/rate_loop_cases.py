"""Inputs shared by tests/test_gpu_rate_loop.py (GPU against the reference) and tests/test_rate_loop_cpu.py (the reference against its mutants and its
census, on the same inputs): the shapes of tests/scenario_cases.py — small_cfg (H = 4, P = 33, 3 iterations), B = 5, T = 7 with S = 3 — plus rate loops.

The gains are chosen by what they make the REFERENCE do (the census of rate_loop_ref, asserted in tests/test_rate_loop_cpu.py): "soft" keeps the mixer
inside the input bounds and the integrator inside its limit on most substeps, "stiff" drives motors into the input bounds (a rate error of 1 rad/s asks
for most of the command range) and "windup" integrates fast against a tight limit. A parity case can therefore not pass by never reaching a clamp."""
import numpy as np

from scenario_cases import ALPHA, B5, S3, SCHEDULE, T7, disturbance, episodes, motor_state, perturbed_plants, small_cfg  # noqa: F401
from sde4mbrl_px4_amd import synthetic_iris
from sde4mbrl_px4_amd.solver import RateLoop

RATE_LOOPS = {
    "soft": dict(kp=[0.03, 0.03, 0.08], ki=[0.3, 0.3, 0.5], integ_limit=0.05),
    "stiff": dict(kp=[0.9, 0.8, 2.5], ki=[2.0, 2.0, 3.0], integ_limit=0.2),
    "windup": dict(kp=[0.05, 0.04, 0.1], ki=[60.0, 50.0, 80.0], integ_limit=[0.004, 0.003, 0.006]),
}
WEIGHTS = (0.0, 0.35, 1.0)


def rate_loop(name, **kw):
    return RateLoop(**{**RATE_LOOPS[name], **kw})


def timing(n, D=None):
    return dict(plant_substeps=n, solve_period=S3, solve_delay=n + 1 if D is None else D, motor_lag=ALPHA)


def integ_state(B, seed=12):
    """A non-zero integrator state inside every limit above, so that a carried-in integrator is not confused with the default."""
    return np.random.default_rng(seed).uniform(-0.002, 0.002, (B, 3)).astype(np.float32)


def rate_tail(B, H, seed=13):
    return np.random.default_rng(seed).uniform(-0.8, 0.8, (B, H, 3)).astype(np.float32)


def full_mixer(m, seed=14):
    """A mixer with no symmetry at all: f32[m][3], every entry distinct."""
    return np.random.default_rng(seed).uniform(-0.6, 0.6, (m, 3)).astype(np.float32)


# the parity cases of the CPU tests (mutants, census): keyword arguments of rate_loop_ref beside (cfg, model, plants, x0, xref, keys, T7)
def ref_cases():
    """[(name, plants or None, kwargs)] on small_cfg / the synthetic Iris, B5 episodes of seed 61."""
    pl = perturbed_plants(synthetic_iris(), 3)
    out = []
    for name in RATE_LOOPS:
        out.append((name, pl, dict(rate_loop=rate_loop(name), S=S3, D=4, alpha=ALPHA, substeps=3, plant_of=np.array([0, 1, 2, 1, 0], np.int32),
                                   disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4), rate_integ_in=integ_state(B5),
                                   rate_tail_in=rate_tail(B5, 4))))
    return out
