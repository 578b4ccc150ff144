"""Inputs shared by tests/test_gpu_age_loop.py (GPU against the reference) and tests/test_age_loop_cpu.py (the reference against its mutants, on the same
inputs): the shapes and observation rows of tests/obs_cases.py (obs_cfg: H = 8, P = 33, 3 iterations; B = 5; S = 2, n = 2, D = 1; T = 5 with a partial last
period and T = 6 without one), plus an age per solve and episode and a history that is no episode's x0.

The ages, per episode over the three solves, beside the dropout pattern VALID of obs_cases.py (0 drops solve 0; 1 drops solves 1 and 2; 2 never drops; 3 drops
solves 0 and 1; 4 drops the last solve):
  0: (3, 4, 0)   the age of the dropped solve 0 is never read; solve 1 reaches back a whole period (age_max = S n: the state before the plant launch); then 0
  1: (2, 1, 3)   only solve 0 is valid: it reads xhist_in
  2: (0, 0, 0)   never aged: this episode may not change in any bit
  3: (4, 2, 1)   only solve 2 is valid, one substep old
  4: (4, 3, 1)   solve 0 reads the OLDEST row of xhist_in, solve 1 the second row of the previous period; the last solve is dropped
So 0 and age_max meet in one run, every valid solve with A > 0 has moved history behind it, and the episodes with such a solve are 0, 1, 3 and 4."""
import numpy as np

from obs_cases import (B5, D1, N2, NS3, S2, T5, VALID, bias_rows, dead_motor, disturbance, episodes, full_case, held, meas_keys, motor_state,  # noqa: F401
                       noise_rows, obs_cfg, observation, perturbed_plants, plant_switch, rate_loop, rate_tail, timing)

T6, AM4 = 6, 4
AGE = np.array([[3, 4, 0],
                [2, 1, 3],
                [0, 0, 0],
                [4, 2, 1],
                [4, 3, 1]], np.int32).T.copy()             # int32[NS3][B5]
AGED_EPISODES = [0, 1, 3, 4]                               # those with a valid solve of age > 0 (at age_max = 4 and VALID)


def history(x0, AM, seed=34):
    """xhist_in f32[B][AM][13]: a vehicle that moved towards x0 by about 1e-2 per substep in every component, rows distinct (oldest first)."""
    B = x0.shape[0]
    step = np.random.default_rng(seed).uniform(0.005, 0.02, (B, 1, 13)).astype(np.float32) * np.where(np.arange(13) % 2, 1.0, -1.0).astype(np.float32)
    back = np.arange(AM, 0, -1, dtype=np.float32)[None, :, None]
    return np.ascontiguousarray(x0[:, None] - back * step, np.float32)


def aging(age_max=AM4, Ns=NS3, B=B5, shared=False, constant=False, renorm=False):
    """Keyword arguments of closed_loop / age_loop_ref: the ages above clipped to age_max, per episode or shared ([.][1]: episode 0's column, which holds 0 and
    age_max), per solve or constant ([1][.]: solve 1's row, which holds age_max at episode 0 and 0 at episode 2)."""
    a = np.minimum(AGE[:Ns, :B], age_max).astype(np.int32)
    if shared:
        a = a[:, :1]
    if constant:
        a = a[1:2]
    return dict(meas_age=np.ascontiguousarray(a), meas_age_max=age_max, meas_renorm=renorm)


def aged_case(model, x0, rate=None, T=T5, age_max=AM4, renorm=True, **kw):
    """full_case of obs_cases.py (a gust, a dead motor, a plant switch, noise, bias and dropouts, a held measurement) with ages and a history on top."""
    B = x0.shape[0]
    return dict(full_case(model, rate, B=B, T=T), **aging(age_max, -(-T // S2), B, renorm=renorm, **kw), xhist_in=history(x0, age_max))
