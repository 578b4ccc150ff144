"""Inputs shared by tests/test_gpu_scenario_loop.py (GPU against the reference) and tests/test_scenario_loop_cpu.py (the reference against its
mutants, on the same inputs): the shapes of tests/test_gpu_timed_loop.py — small_cfg (H = 4, P = 33, 3 iterations), B = 5 (a partly empty last
workgroup), T = 7 with S = 3 (a partial last period), n in {1, 3}, D = n + 1, alpha = 0.35 — plus a disturbance schedule and a plant schedule."""
import os

import numpy as np

from cases import CDIR
from sde4mbrl_px4_amd import load_mpc_config, prng
from sde4mbrl_px4_amd import workload as W

S3, T7, B5, ALPHA = 3, 7, 5, 0.35
# every group that a switch must carry over to the new vehicle, sigma (hence sigma sqrt(dt)) included
AMOUNTS = dict(mass=0.2, inertia=0.2, thrust=0.2, sigma=0.3, residual=0.2)


def small_cfg(**kw):
    c1 = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml"))
    return c1.replace(**{"horizon": 4, "num_short_dt": 4, "num_particles": 33, "max_iter": 3, "max_no_improvement_iter": 3, **kw})


def episodes(cfg, B, seed):
    x0 = W.random_initial_states(B, seed)
    xref = np.stack([W.reference_window(0.1 * b, cfg.time_steps) for b in range(B)])[None]      # [1][B][H+1][13]
    keys = np.stack([prng.PRNGKey(seed + b) for b in range(B)])
    return x0, xref, keys


def perturbed_plants(model, n, seed=1):
    rng = np.random.default_rng(seed)
    return [model.perturbed(rng, **AMOUNTS) for _ in range(n)]


def motor_state(B, m, seed=9, lo=0.55, hi=0.85):
    return np.random.default_rng(seed).uniform(lo, hi, (B, m)).astype(np.float32)


def disturbance(Td, Bd, seed=4):
    """f32[Td][Bd][6]: linear accelerations of up to 3 m/s^2 (a stiff gust on a 1.5 kg vehicle), angular ones of up to 4 rad/s^2; row (0, 0) has a
    zero and a negative zero among its components."""
    rng = np.random.default_rng(seed)
    w = np.concatenate([rng.uniform(-3.0, 3.0, (Td, Bd, 3)), rng.uniform(-4.0, 4.0, (Td, Bd, 3))], axis=-1).astype(np.float32)
    w[0, 0, 1], w[0, 0, 4] = 0.0, -0.0
    return w


# int32[T7][B5] over Np = 3 plants: episode 0 never switches; 1 switches on every tick (and so returns to earlier blobs); 2 switches once inside a
# period (k = 1); 3 switches once at a period start (k = 3); 4 leaves blob 0 inside a period (k = 2) and returns to it inside the next (k = 4)
SCHEDULE = np.array([[0, 0, 0, 0, 0, 0, 0],
                     [0, 1, 2, 0, 1, 2, 0],
                     [1, 2, 2, 2, 2, 2, 2],
                     [2, 2, 2, 0, 0, 0, 0],
                     [0, 0, 1, 1, 0, 0, 0]], np.int32).T.copy()


def switch_ticks(sched):
    """[(k, b)] of every switch of a schedule int[T][B]."""
    return [(k, b) for k in range(1, sched.shape[0]) for b in range(sched.shape[1]) if sched[k, b] != sched[k - 1, b]]
