"""Inputs shared by tests/test_gpu_process_loop.py (GPU against the reference) and tests/test_process_loop_cpu.py (the reference against its mutants, on the same
inputs), built from the existing case helpers (score_cases.py and, through it, age_cases.py, obs_cases.py, rate_loop_cases.py and scenario_cases.py): score_cfg
(H = 6 with two step lengths, P = 33, 3 iterations), T = 5 with S = 2 (Ns = 3, the last period ragged) and T = 6, n = 2, D = 1, alpha = 0.35, B = 3 .. 5, plus the two
Gauss-Markov processes of SPEC.md §11i: coefficients distinct in every component (and in every episode when per episode), a key chain per episode that is no other
chain of the run, and start states of both signs."""
import numpy as np

from obs_cases import SCALE, VALID, bias_rows, meas_keys  # noqa: F401
from score_cases import B5, FINITE, S2, T5, T6, score_cfg, scored_episodes, targets, thresholds_from, together  # noqa: F401
from scenario_cases import disturbance  # noqa: F401
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import GaussMarkov

DT_TICK = 0.05                       # the first step length of score_cfg: the time between two control ticks
W_DIST, W_BIAS = 6, 12
# deviation of a gust per component: linear [m/s^2] and angular [rad/s^2] acceleration
GUST = np.array([0.8, 0.6, 0.4, 1.5, 1.2, 0.9], np.float64)


def chain_keys(B, seed):
    return np.stack([prng.PRNGKey(seed + b) for b in range(B)])


def dist_process(B, per_episode=True, seed=61):
    """A gust process: correlation times around 0.3 s, one step per control tick."""
    r = np.random.default_rng(seed)
    rows = B if per_episode else 1
    return GaussMarkov(GUST * r.uniform(0.5, 1.5, (rows, W_DIST)), r.uniform(0.1, 0.6, (rows, W_DIST)), DT_TICK)


def bias_process(B, per_episode=True, seed=62):
    """An estimator-bias process: correlation times around 1 s, one step per solve (S2 ticks)."""
    r = np.random.default_rng(seed)
    rows = B if per_episode else 1
    return GaussMarkov(SCALE.astype(np.float64) * r.uniform(0.5, 1.5, (rows, W_BIAS)), r.uniform(0.3, 2.0, (rows, W_BIAS)), S2 * DT_TICK)


def start_state(gm, B, W, seed):
    return gm.stationary_state(np.random.default_rng(seed), B, W)


def coeffs(gm, B, W):
    """(rho, scale) f32[1 or B][W] of a GaussMarkov, what process_loop_ref takes."""
    return gm.coeffs(B, W)


def drawn(B, dist=True, bias=True, per_episode=True, states=True):
    """Keyword arguments of closed_loop for the two processes (meas_keys included with the bias process)."""
    kw = {}
    if dist:
        gm = dist_process(B, per_episode)
        kw.update(dist_process=gm, dist_keys=chain_keys(B, 700), dist_state_in=start_state(gm, B, W_DIST, 71) if states else None)
    if bias:
        gm = bias_process(B, per_episode)
        kw.update(bias_process=gm, bias_keys=chain_keys(B, 800), bias_state_in=start_state(gm, B, W_BIAS, 72) if states else None, meas_keys=meas_keys(B))
    return kw


def for_ref(kw, B):
    """The same keyword arguments for process_loop_ref: each GaussMarkov as its (rho, scale) pair."""
    out = dict(kw)
    for name, W in (("dist_process", W_DIST), ("bias_process", W_BIAS)):
        if out.get(name) is not None:
            out[name] = coeffs(out[name], B, W)
    return out
