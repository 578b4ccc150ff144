"""Inputs shared by tests/test_gpu_obs_loop.py (GPU against the reference) and tests/test_obs_loop_cpu.py (the reference against its mutants, on the same
inputs): obs_cfg (H = 8 with two step lengths, P = 33, 3 iterations), T = 5 with S = 2 (Ns = 3, the last period partial), n = 2, D = 1, alpha = 0.35, B = 5
(a partly empty last workgroup), plus the rows of an observation.

The dropout pattern, per episode over the three solves: 0 drops solve 0; 1 drops solves 1 and 2 (two consecutive ones, the last one among them); 2 never
drops; 3 drops solves 0 and 1; 4 drops the last solve."""
import numpy as np

from rate_loop_cases import ALPHA, B5, disturbance, motor_state, perturbed_plants, rate_loop, rate_tail  # noqa: F401
from scenario_cases import episodes, small_cfg  # noqa: F401
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import fault_schedule

T5, S2, N2, D1, NS3 = 5, 2, 2, 1, 3
VALID = np.array([[0, 1, 1],
                  [1, 0, 0],
                  [1, 1, 1],
                  [0, 0, 1],
                  [1, 1, 0]], np.int32).T.copy()           # int32[NS3][B5]
# scale of an estimator's error per component group: p [m], v [m/s], theta [rad], omega [rad/s]
SCALE = np.repeat(np.array([0.05, 0.1, 0.02, 0.05], np.float32), 3)


def obs_cfg(**kw):
    return small_cfg(**{"horizon": 8, "num_short_dt": 4, "short_step_dt": 0.05, "long_step_dt": 0.1, **kw})


def timing(n=N2, D=D1, S=S2):
    return dict(plant_substeps=n, solve_period=S, solve_delay=D, motor_lag=ALPHA)


def meas_keys(B, seed=500):
    return np.stack([prng.PRNGKey(seed + b) for b in range(B)])


def noise_rows(Ns, B, seed=31):
    """sigma f32[Ns][B][12], every entry distinct and > 0 except one exact zero (row (0, 0), component 4: that component then carries its bias alone)."""
    s = (SCALE * np.random.default_rng(seed).uniform(0.5, 1.5, (Ns, B, 12))).astype(np.float32)
    s[0, 0, 4] = 0.0
    return s


def bias_rows(Ns, B, seed=32):
    """beta f32[Ns][B][12], both signs."""
    return (SCALE * np.random.default_rng(seed).uniform(-1.0, 1.0, (Ns, B, 12))).astype(np.float32)


def held(B, seed=33):
    """xmeas_in f32[B][13]: recognisable states that are no episode's x0."""
    x = np.random.default_rng(seed).uniform(-0.3, 0.3, (B, 13)).astype(np.float32)
    x[:, 6] = 1.0
    return x


def dead_motor(T, B, m=4):
    """f32[T][B][m][2]: motor 1 of every odd episode dead from tick 1 (inside the first solve period)."""
    f = fault_schedule(T, B, m)
    f[1:, 1::2, 1] = (0.0, 0.0)
    return f


def plant_switch(T, B, Np=3):
    """int32[T][B]: episode b flies plant b % Np and moves on to the next plant at tick 2 (a period start) and again at tick 3 (inside a period)."""
    s = np.tile(np.arange(B, dtype=np.int32) % Np, (T, 1))
    s[2:] = (s[2:] + 1) % Np
    s[3:] = (s[3:] + 1) % Np
    return s


def observation(Ns=NS3, B=B5, shared=False, constant=False):
    """Keyword arguments of closed_loop / obs_loop_ref: rows per episode or shared ([.][1]), per solve or constant ([1][.]); the dropout pattern above."""
    s, be, v = noise_rows(NS3, B5)[:Ns, :B], bias_rows(NS3, B5)[:Ns, :B], VALID[:Ns, :B]
    if shared:
        s, be, v = s[:, 2:3], be[:, 2:3], v[:, 1:2]
    if constant:
        s, be, v = s[1:2], be[1:2], v[:1]
    return dict(meas_noise=np.ascontiguousarray(s), meas_bias=np.ascontiguousarray(be), meas_valid=np.ascontiguousarray(v), meas_keys=meas_keys(B))


def full_case(model, rate=None, B=B5, T=T5):
    """Everything at once: per-episode plants with a switch, a gust, a dead motor, the rows of an observation with dropouts, a held measurement."""
    kw = dict(timing(), plant=perturbed_plants(model, 3), plant_of=plant_switch(T, B), disturbance=disturbance(T, B), u_act_in=motor_state(B, 4),
              fault=dead_motor(T, B), xmeas_in=held(B), **observation(-(-T // S2), B))
    if rate is not None:
        kw.update(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B, 8))
    return kw
