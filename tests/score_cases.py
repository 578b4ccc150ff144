"""Inputs shared by tests/test_gpu_score_loop.py (GPU against the reference) and tests/test_score_loop_cpu.py (the reference against its mutants, on the same
inputs), built from the existing case helpers (age_cases.py and, through it, obs_cases.py, rate_loop_cases.py and scenario_cases.py): score_cfg (H = 6 with two step lengths, P = 33, 3 iterations), T = 5 with
S = 2 (Ns = 3, the last period ragged), n = 2, D = 1, alpha = 0.35, B = 3 .. 5.

The episodes, by index (an episode keeps its role at every B, so B = 3 has no non-finite one):
  0  an ordinary flight
  1  starts from a warm start (and so a motor state) AT the upper input bound: its first tick's us row is saturated in every motor (word 11), and it is pushed away
  2  stepsize_in = 0: no solve of it ever moves, so opt_cost == init_cost in every solve (word 15 counts them; with <= they would not count)
  3  x0 has +inf in position x: dp = +inf in EVERY row (the maximum is tied from row 0 on), cause bits 1 and 8, costs inf (word 15)
  4  x0 has a NaN in position y: dp is NaN in every row — outside every radius, though dp > r2_pos is false — cause bits 1 and 8
The thresholds are taken from the oracle's own trajectories (thresholds_from): over the FINITE episodes, the median of the per-episode maxima of dp and w2 and of
the per-episode minima of c, so that each of the cause bits 1, 2 and 4 is set in at least one finite episode and clear in at least one."""
import numpy as np

from age_cases import (AM4, aging, dead_motor, disturbance, episodes, history, held, obs_cfg, observation, perturbed_plants, plant_switch, rate_loop,  # noqa: F401
                       rate_tail, timing)
from closed_loop_ref import default_warm_start
from score_loop_ref import row_terms
from sde4mbrl_px4_amd.solver import Score

T5, T6, S2, N2, NS3, B5, H6 = 5, 6, 2, 2, 3, 5, 6
FINITE = (0, 1, 2)                   # episodes whose states stay finite


def score_cfg(**kw):
    return obs_cfg(**{"horizon": H6, **kw})


def scored_episodes(cfg, B, seed):
    """(x0, xref, keys, kw): the episodes of the module docstring and the keyword arguments (timing, warm start, step sizes) of closed_loop / the reference."""
    x0, xref, keys = episodes(cfg, B, seed)
    x0 = x0.copy()
    u, s = default_warm_start(cfg, B)
    m = cfg.num_motors
    if B > 1:
        u[1] = np.asarray(list(cfg.to_cfg()[0].u_hi)[:m], np.float32)
    if B > 2:
        s[2] = 0.0
    if B > 3:
        x0[3, 0] = np.inf
    if B > 4:
        x0[4, 1] = np.nan
    return x0, xref, keys, dict(timing(), u_init=u, stepsize_in=s)


def targets(xref, T, per_tick=True, per_episode=True):
    """score_ref f32[T or 1][B or 1][13]: the target of tick k of episode b is row min(k + 1, H) of the episode's reference window (the reference at the END of the
    tick while the window lasts), so every (tick, episode) row is distinct; a size-1 axis keeps tick 1 / episode 1."""
    w = np.asarray(xref, np.float32)[0]                  # [B][H+1][13]
    H = w.shape[1] - 1
    g = np.stack([w[:, min(k + 1, H)] for k in range(T)])
    if not per_tick:
        g = g[1:2]
    if not per_episode:
        g = g[:, 1:2]
    return np.ascontiguousarray(g)


def thresholds_from(xs, xsub, score_ref, finite=FINITE, substeps=False):
    """A Score whose thresholds sit inside the oracle's own spread: the median over the finite episodes of max dp, min c and max w2 (see the module docstring)."""
    T = xs.shape[1] - 1
    g = np.asarray(score_ref, np.float32)
    mdp, mc, mw = [], [], []
    for b in finite:
        rows = xsub[b] if substeps else xs[b, 1:]
        n = rows.shape[0] // T
        t = [row_terms(rows[r], g[r // n if g.shape[0] > 1 else 0, b if g.shape[1] > 1 else 0]) for r in range(rows.shape[0])]
        mdp.append(max(v[0] for v in t)); mc.append(min(v[2] for v in t)); mw.append(max(v[3] for v in t))
    r2, c, w2 = (float(np.median(np.asarray(v, np.float64))) for v in (mdp, mc, mw))
    return Score(pos_radius=np.sqrt(r2), tilt_max=np.arccos(min(c, 1.0)), rate_max=np.sqrt(w2), substeps=substeps)


def together(model, x0, H, rate=None, T=T5):
    """A fault, a gust, a plant switch and an aged, noisy, renormalised measurement with dropouts in one run (the pieces of obs_cases.full_case and
    age_cases.aged_case at this horizon); merged over the timing of scored_episodes."""
    B = x0.shape[0]
    Ns = -(-T // S2)
    kw = dict(plant=perturbed_plants(model, 3), plant_of=plant_switch(T, B), disturbance=disturbance(T, B), fault=dead_motor(T, B), xmeas_in=held(B),
              **observation(Ns, B), **aging(AM4, Ns, B, renorm=True), xhist_in=history(np.nan_to_num(x0, nan=0.25, posinf=0.5), AM4))
    if rate is not None:
        kw.update(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B, H))
    return kw
