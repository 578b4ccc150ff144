"""Inputs shared by tests/test_gpu_track_loop.py (GPU against the reference) and tests/test_track_loop_cpu.py (the reference against its mutants, on the same
inputs), built from the existing case helpers (score_cases.py and, through it, age_cases.py, obs_cases.py, rate_loop_cases.py and scenario_cases.py): track_cfg
(obs_cfg at H = 8 with two step lengths, 3 x 0.05 s then 5 x 0.07 s: the float32 and the float64 sum of the window's clock offsets then differ in three of the
nine entries, which they do not at 4 x 0.05 s + 4 x 0.1 s; P = 33, 3 iterations),
T = 6 with S = 2, n = 2, D = 1, alpha = 0.35, B = 5 — the smallest shapes at which the code of SPEC.md §11j can go wrong, not the workload's.

The set holds four tables, all with non-uniform knot spacing and attitudes that turn by 20 degrees and more from knot to knot (the interpolated quaternion is
visibly non-unit), body rates and velocities non-zero:
  0  L = 37, periodic (period 8 s): a lemniscate with two yaw turns per lap; five bisection levels, both ends
  1  L = 5, clamped, t from 0.25 s to 2.5 s
  2  L = 2, clamped
  3  L = 1
The five episodes (params, shift = 0), at tick0 in {0, 1000}:
  0  table 0, phase EXACTLY knot 5's time, rate 1, no offset: window row 0 of tick 0 sits on a knot
  1  table 1, phase -0.4 (before t[0]), rate 1.3, an offset
  2  table 1, phase 1.9, rate 0.7: the window runs past t[L-1]
  3  table 0, rate 0 at phase 3.3: a held point
  4  table 0, phase -0.9, rate 1.7, an offset: negative trajectory times, wrapped by floor, and a wrap inside the window
With shift s episode b flies table (its table + s) % 4 instead, so that every table is met by every kind of episode; episodes past the fifth (B = 258) draw
their numbers from a seeded generator and cycle through the tables."""
import numpy as np

from obs_cases import obs_cfg, timing  # noqa: F401
from scenario_cases import episodes  # noqa: F401
from sde4mbrl_px4_amd.solver import Trajectory

T6, S2, N2, B5, H8 = 6, 2, 2, 5, 8
TICK0S = (0, 1000)
PERIOD = 8.0


def track_cfg(**kw):
    return obs_cfg(**{"num_short_dt": 3, "short_step_dt": 0.05, "long_step_dt": 0.07, **kw})


def _attitude(yaw, roll, pitch):
    """Unit quaternions [n][4] of a yaw and two small tilt components (float64)."""
    q = np.stack([np.cos(0.5 * yaw), roll, pitch, np.sin(0.5 * yaw)], axis=-1)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def lemniscate_table(L=37, period=PERIOD):
    """(t f32[L], x f32[L][13], period): knots bunched by a sine so that no two segments have the same length; t[0] = 0 and t[L-1] = period exactly."""
    s = np.arange(L, dtype=np.float64) / (L - 1)
    t = period * (s + 0.16 * (np.sin(2.0 * np.pi * s + 0.7) - np.sin(0.7)) / (2.0 * np.pi))
    t[0], t[-1] = 0.0, period
    w = 2.0 * np.pi / period
    x = np.zeros((L, 13))
    x[:, 0], x[:, 1], x[:, 2] = np.sin(w * t), np.sin(w * t) * np.cos(w * t), 1.0 + 0.2 * np.sin(2 * w * t)
    x[:, 3], x[:, 4], x[:, 5] = w * np.cos(w * t), w * np.cos(2 * w * t), 0.4 * w * np.cos(2 * w * t)
    x[:, 6:10] = _attitude(2.0 * w * t * 2.0, 0.2 * np.sin(w * t), 0.15 * np.cos(w * t))       # the half angle runs to 4 pi: the last knot's attitude is the first's
    x[:, 10], x[:, 11], x[:, 12] = 0.3 * np.cos(w * t), -0.2 * np.sin(w * t), 2.0 * w * np.ones(L)
    x[-1] = x[0]
    return t.astype(np.float32), x.astype(np.float32), np.float32(period)


def short_table(L, seed):
    """A clamped table of L knots: random spacing, a path of a few metres, a yaw step of 20 to 50 degrees per knot."""
    r = np.random.default_rng(seed)
    t = 0.25 + np.concatenate([[0.0], np.cumsum(r.uniform(0.3, 0.8, L - 1))]) if L > 1 else np.array([0.25])
    x = np.zeros((L, 13))
    x[:, 0:3] = np.cumsum(r.uniform(-0.5, 0.5, (L, 3)), axis=0) + [0.0, 0.0, 1.0]
    x[:, 3:6] = r.uniform(-1.0, 1.0, (L, 3))
    x[:, 6:10] = _attitude(np.cumsum(r.uniform(np.deg2rad(20), np.deg2rad(50), L)), r.uniform(-0.2, 0.2, L), r.uniform(-0.2, 0.2, L))
    x[:, 10:13] = r.uniform(-0.5, 0.5, (L, 3))
    return t.astype(np.float32), x.astype(np.float32), np.float32(0.0)


def raw_tables():
    """The four tables as (t, x, period), what track_loop_ref takes."""
    return [lemniscate_table(), short_table(5, 41), short_table(2, 42), short_table(1, 43)]


def tables():
    """The same as solver.Trajectory objects (the constructor finds no sign to flip: consecutive attitudes are less than 90 degrees apart)."""
    return [Trajectory.from_knots(t, x, p) for t, x, p in raw_tables()]


def params(B, shift=0, seed=51):
    """(track_of int32[B], phase f32[B], rate f32[B], offset f32[B][3]) of the module docstring."""
    r = np.random.default_rng(seed)
    of = (np.arange(B) % 4).astype(np.int32)
    phase = r.uniform(-1.0, 9.0, B).astype(np.float32)
    rate = r.uniform(0.5, 2.0, B).astype(np.float32)
    offset = r.uniform(-1.0, 1.0, (B, 3)).astype(np.float32)
    t37 = lemniscate_table()[0]
    special = [(0, t37[5], 1.0, (0.0, 0.0, 0.0)), (1, -0.4, 1.3, (0.3, -0.2, 0.1)), (1, 1.9, 0.7, (0.0, 0.0, 0.0)), (0, 3.3, 0.0, (0.0, 0.0, 0.0)),
               (0, -0.9, 1.7, (-0.25, 0.5, 0.05))]
    for b, (tb, ph, rt, off) in enumerate(special[:B]):
        of[b], phase[b], rate[b], offset[b] = tb, ph, rt, off
    of = ((of + shift) % 4).astype(np.int32)
    return of, phase, rate, offset


def tracked(B, shift=0, tick0=0, renorm=True):
    """Keyword arguments of closed_loop for the set and the episodes' numbers."""
    of, phase, rate, offset = params(B, shift)
    return dict(track=tables(), track_of=of, track_phase=phase, track_rate=rate, track_offset=offset, track_tick0=tick0, track_renorm=renorm)


def for_rows(kw):
    """The keyword arguments of track_rows / track_targets from those of closed_loop."""
    return dict(table_of=kw.get("track_of"), phase=kw.get("track_phase"), rate=kw.get("track_rate"), offset=kw.get("track_offset"), renorm=kw.get("track_renorm", True))
