"""Inputs shared by tests/test_gpu_retire.py (GPU against the reference) and tests/test_retire_cpu.py (the reference against its properties and its mutants, on
the same inputs): the retiring closed loop of SPEC.md §11n on small loops — H = 6 with two step lengths, P = 32 or 33, m = 4, 3 iterations, T = 8 with solve
period 2 (four solves; one case at T = 7, whose last period is one tick), n = 2 plant substeps, D = 1, a motor lag.

Failures are induced by a dead motor: episode b loses motor 1 from tick DEAD[b % 5] on (never, 0, 2, 4, 6), and every episode with b % 5 = 1 starts rolled by 0.5 rad, so a known subset fails in known periods. The tilt
threshold is then taken from the unretired oracle loop's own rows (pick_score): the candidate, among the tilt cosines the rows hold, whose first failures cover
the most of {first period, a middle period, the last period, never}; the tests assert the cover they need, nothing is taken on trust."""
import contextlib
import functools

import numpy as np

import loop_cases
from age_loop_ref import age_loop_ref
from obs_cases import timing
from retire_ref import retire_loop_ref
from scenario_cases import episodes, small_cfg
from score_cases import targets
from score_loop_ref import row_terms, score_rows
from sde4mbrl_px4_amd import synthetic_iris
from sde4mbrl_px4_amd.solver import Score, fault_schedule

F = np.float32
T8, S2, N2, H6, NS4 = 8, 2, 2, 6, 4
DEAD = (None, 0, 2, 4, 6)            # the tick from which motor 1 is dead, by episode index modulo 5


def retire_cfg(**kw):
    return small_cfg(**{"horizon": H6, "num_short_dt": 4, "short_step_dt": 0.05, "long_step_dt": 0.1, "num_particles": 32, **kw})


def dead_motors(T, B, m=4, dead=DEAD):
    """f32[T][B][m][2]: motor 1 of episode b dead from tick dead[b % len(dead)] on."""
    f = fault_schedule(T, B, m)
    for b in range(B):
        t = dead[b % len(dead)]
        if t is not None:
            f[t:, b, 1] = (0.0, 0.0)
    return f


def inputs(B, seed=1200, T=T8, **cfg_kw):
    """(cfg, model, x0, xref, keys, kw): the episodes and the keyword arguments (timing, fault) of closed_loop / the reference loop."""
    cfg, model = retire_cfg(**cfg_kw), synthetic_iris()
    x0, xref, keys = episodes(cfg, B, seed)
    x0 = x0.copy()
    x0[1::5, 6:10] = np.asarray([np.cos(0.25), np.sin(0.25), 0.0, 0.0], F)       # (role 1 starts rolled by 0.5 rad: it fails in the first period)
    return cfg, model, x0, xref, keys, dict(timing(n=N2, D=1, S=S2), fault=dead_motors(T, B))


def first_fail_periods(rows, g, cos_min, rpt, S):
    """int[B]: the period of each episode's first row with a tilt cosine below cos_min, -1: none."""
    B, R = rows.shape[:2]
    out = np.full(B, -1, np.int64)
    for b in range(B):
        for r in range(R):
            k = r // rpt
            c = row_terms(rows[b, r], g[k if g.shape[0] > 1 else 0, b if g.shape[1] > 1 else 0])[2]
            if not c >= cos_min:
                out[b] = k // S
                break
    return out


def pick_score(want, g, T, S, n, substeps=False):
    """A Score with a tilt threshold alone, chosen among the cosines the unretired rows hold (see the module docstring), and the failing period of each episode."""
    rows = want[-1] if substeps else want[0][:, 1:]
    rpt = n if substeps else 1
    Ns = -(-T // S)
    cs = np.unique(np.asarray([row_terms(rows[b, r], g[0, 0])[2] for b in range(rows.shape[0]) for r in range(rows.shape[1])], F))
    best = None
    for c in cs[np.isfinite(cs)]:
        p = first_fail_periods(rows, g, c, rpt, S)
        cover = (int((p == 0).any()), int(((p > 0) & (p < Ns - 1)).any()), int((p == Ns - 1).any()), int((p < 0).any()))
        key = (sum(cover), len(set(p.tolist())), float(c))
        if best is None or key > best[0]:
            best = (key, c, p)
    _, c, p = best
    score = Score(tilt_max=float(np.arccos(np.float64(c))), substeps=substeps)
    if score.cos_min != c:             # (the rounding of cos(arccos(c)): take the neighbour that reproduces the periods)
        score.cos_min = F(c)
    return score, p


def run_ref_for(loop_ref, cfg, model, x0, xref, keys, T, **kw):
    """run_ref of retire_loop_ref for closed_loop's keyword arguments on one of the reference loops, xsub last."""
    def run_ref(eps, ctx=contextlib.nullcontext):
        with ctx():
            return loop_cases.ref(loop_ref, cfg, model, x0, xref, keys, T, substep_states=True, episodes=eps, **kw)
    return run_ref


@functools.lru_cache(maxsize=None)
def prepared(B, seed=1200, substeps=False, P=32, mlp_dtype=None, math_mode=None, T=T8):
    """Everything a test of one mixed-failure case needs, computed ONCE and shared (never changed): the inputs, the unretired oracle loop, the Score, and the
    retiring reference (values, words, retired_at, live). T = 7 ends in a partial period of one tick."""
    arith = {} if mlp_dtype is None else dict(mlp_dtype=mlp_dtype, math_mode=math_mode)
    cfg, model, x0, xref, keys, kw = inputs(B, seed, T=T, num_particles=P, **arith)
    run_ref = run_ref_for(age_loop_ref, cfg, model, x0, xref, keys, T, **kw)
    plain = run_ref(None)
    g = targets(xref, T)
    score, periods = pick_score(plain, g, T, S2, N2, substeps)
    first = (plain, score_rows(plain[0], plain[1], plain[2], plain[-1], g, cfg, score.thresholds(), substeps, S2))
    vals, z, retired_at, live, _ = retire_loop_ref(run_ref, cfg, x0, g, score.thresholds(), substeps, S2, N2, T, first=first)
    return dict(cfg=cfg, model=model, x0=x0, xref=xref, keys=keys, kw=kw, run_ref=run_ref, plain=plain, z_plain=first[1], first=first, g=g, score=score,
                periods=periods, vals=vals, z=z, retired_at=retired_at, live=live, substeps=substeps, B=B)


def pattern(B):
    """bool[B] live flags at entry: wave 0 wholly live and episode 64 retired (the flip at 63|64), episode 255 live and block 1 (episodes 256 .. 511) wholly
    retired (the flip at 255|256), block 2 (B > 512) wholly live; elsewhere every third episode is retired. A wholly live block beside a wholly retired one
    exists at B = 600 only, and at the first solve only (the dead motors then retire part of block 2); B = 300 has the two flips and the wholly retired block 1
    (44 episodes), but no wholly live block."""
    live = np.arange(B) % 3 != 1
    live[:64] = True
    live[64:65] = False
    live[255:256] = True
    live[256:512] = False
    live[512:] = True
    return live
