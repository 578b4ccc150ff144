"""Inputs shared by tests/test_gpu_fault_loop.py (GPU against the reference) and tests/test_fault_loop_cpu.py (the reference against its mutants and its
census, on the same inputs): the shapes of tests/rate_loop_cases.py — small_cfg (H = 4, P = 33, 3 iterations), B = 5, T = 7 with S = 3 — plus a fault
schedule.

The schedule, per episode: 0 healthy; 1 motor 2 dead from tick 2 (inside a solve period); 2 motor 0 at kappa = 0.6 from tick 3 (a period start); 3 motor 1
stuck at 0.9 on ticks 1 - 4, released at 5; 4 motor 3 dead from tick 4 and motor 0 biased by +0.05 throughout."""
import numpy as np

from rate_loop_cases import (ALPHA, B5, S3, SCHEDULE, T7, disturbance, episodes, motor_state, perturbed_plants, rate_loop, rate_tail,  # noqa: F401
                             small_cfg, timing)
from sde4mbrl_px4_amd.solver import fault_schedule

LOOPS = (None, "stiff", "soft")          # the rate loops of the CPU cases: none, and two of tests/rate_loop_cases.py
N3, D4 = 3, 4


def faults(T=T7, B=B5, m=4):
    """f32[T][B][m][2], the table of the module docstring (m >= 4, B >= 5; further motors and episodes stay healthy)."""
    f = fault_schedule(T, B, m)
    f[2:, 1, 2] = (0.0, 0.0)
    f[3:, 2, 0] = (0.6, 0.0)
    f[1:5, 3, 1] = (0.0, 0.9)
    f[4:, 4, 3] = (0.0, 0.0)
    f[:, 4, 0] = (1.0, 0.05)
    return f


def faults_any(T, B, m, seed=21):
    """A schedule for any shape: every (tick, episode) row one of healthy / dead / weakened / stuck / biased on one motor, drawn per row, so that rows
    change inside solve periods, and no two motors of a row share a pair."""
    rng = np.random.default_rng(seed)
    f = fault_schedule(T, B, m)
    kinds = [(1.0, 0.0), (0.0, 0.0), (0.55, 0.0), (0.0, 0.8), (1.0, -0.04)]
    for k in range(T):
        for b in range(B):
            f[k, b, rng.integers(0, m)] = kinds[rng.integers(0, len(kinds))]
            f[k, b, rng.integers(0, m), 1] += np.float32(0.01) * rng.integers(0, 3)
    return f


def ref_kwargs(name):
    """Keyword arguments of fault_loop_ref for the CPU cases beside (cfg, model, plants, x0, xref, keys, T7): S = 3, D = 4, alpha = 0.35, n = 3."""
    kw = dict(S=S3, D=D4, alpha=ALPHA, substeps=N3, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4))
    if name is not None:
        kw.update(rate_loop=rate_loop(name), rate_tail_in=rate_tail(B5, 4))
    return kw
