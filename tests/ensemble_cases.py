"""Inputs shared by tests/test_gpu_ensemble.py (GPU against the reference) and tests/test_ensemble_cpu.py (the reference against its mutants, on the same inputs):
the per-row ensemble words of SPEC.md §11m on small loops — H = 6 with two step lengths, P = 32, m = 4, 3 iterations, T = 4 with solve_period 2 (two solves),
n = 2 plant substeps, D = 1, a motor lag — at B in {1, 63, 64, 65, 255, 256, 257, 300, 600}: a lone lane, the wave and block edges, a ragged last block and
three blocks, where the sequential order of the block sums shows. One case (B = 65) is scored on the substep states. G is 1 or 3; with G = 3 episodes alternate
between cohorts 0 and 1 — odd episodes, cohort 1, lose motor 1 from tick 1 on by a scheduled fault — and cohort 2 stays EMPTY. E is 0, 3 or 16.

The thresholds are taken from the oracle's own trajectories (score_cases.thresholds_from: the median over the finite episodes of the per-episode extremes), so
about half of the episodes fail, at different rows. The edges of a channel are spread geometrically around what the oracle's included rows hold, and ONE edge of
every channel is set to a value some included episode's row holds exactly, so that "<" and "<=" at an edge differ.

The gust: episode 2 (where B > 2) is hit at tick 1 by an ANGULAR acceleration of 3e38 rad/s^2 about the body x axis, finite as the entry point demands. Its
body rate jumps to about 7.5e36 rad/s, the attitude integration overflows in the tick's second substep, and from there on the oracle loop's rows of that episode
are non-finite (test_ensemble_cpu.py asserts that they are), so the nf exclusion and cause bit 8 are exercised by a state the loop produced itself, not by a
non-finite x0. A LINEAR gust of the same size does not do it: it leaves a velocity of 1.5e37 m/s and a squared position error of +inf on finite rows."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import loop_cases
from age_loop_ref import age_loop_ref
from ensemble_ref import channels, ensemble_ref
from obs_cases import dead_motor, timing
from scenario_cases import episodes, small_cfg
from score_cases import targets, thresholds_from
from score_loop_ref import score_rows
from sde4mbrl_px4_amd import synthetic_iris
from sde4mbrl_px4_amd.solver import Ensemble

F = np.float32
T4, S2, N2, H6 = 4, 2, 2, 6
GUST_EPISODE, GUST_TICK = 2, 1
# (B, G, E, over, substep score)
CASES = ((1, 1, 0, 1, False), (63, 3, 3, 1, False), (64, 1, 16, 0, False), (65, 3, 16, 1, True), (255, 3, 3, 0, False), (256, 1, 3, 1, False),
         (257, 3, 0, 0, False), (300, 3, 3, 1, False), (600, 3, 16, 1, False))
IDS = [f"B{b}-G{g}-E{e}-{'alive' if o else 'all'}{'-substeps' if s else ''}" for b, g, e, o, s in CASES]


def ens_cfg(**kw):
    return small_cfg(**{"horizon": H6, "num_short_dt": 4, "short_step_dt": 0.05, "long_step_dt": 0.1, "num_particles": 32, **kw})


def cohorts(B, G):
    """int32[B] or None: with G = 3 cohort 1 holds the odd (faulted) episodes, cohort 0 the even ones, cohort 2 nobody; with G = 1 the array is left out."""
    return None if G == 1 else (np.arange(B, dtype=np.int32) % 2)


def gust(T, B):
    """f32[T][B][6]: zeros but for the one large finite angular acceleration of the module docstring."""
    w = np.zeros((T, B, 6), F)
    if B > GUST_EPISODE:
        w[GUST_TICK, GUST_EPISODE, 3] = 3e38
    return w


def inputs(B, seed=900, T=T4, **cfg_kw):
    """(cfg, model, x0, xref, keys, kw): the episodes and the keyword arguments (timing, fault, gust) of closed_loop / the reference loop."""
    cfg, model = ens_cfg(**cfg_kw), synthetic_iris()
    x0, xref, keys = episodes(cfg, B, seed)
    kw = dict(timing(n=N2, D=1, S=S2), fault=dead_motor(T, B), disturbance=gust(T, B))
    return cfg, model, x0, xref, keys, kw


def oracle_loop(cfg, model, x0, xref, keys, T, **kw):
    """age_loop_ref for closed_loop's keyword arguments, xsub last, the episodes dealt out to a few Python threads (the oracle runs one solve per thread and gives
    the same bits at any count; every run fills its own episodes' rows and the rows are merged, as geo_loop_ref merges them). The reference loop is untouched."""
    B = x0.shape[0]
    n = max(1, min(16, os.cpu_count() or 1, B // 8))

    def part(eps):
        return loop_cases.ref(age_loop_ref, cfg, model, x0, xref, keys, T, substep_states=True, episodes=eps, **kw)
    if n == 1:
        return part(None)
    deal = [list(range(i, B, n)) for i in range(n)]
    with ThreadPoolExecutor(n) as pool:
        parts = list(pool.map(part, deal))
    out = [np.array(v, copy=True) for v in parts[0]]
    for eps, vals in zip(deal[1:], parts[1:]):
        for o, v in zip(out, vals):
            o[eps] = v[eps]
    return tuple(out)


def finite_episodes(xsub):
    return [b for b in range(xsub.shape[0]) if np.isfinite(xsub[b]).all()]


def edges_for(v, nf, E, rng):
    """f32[4][E]: per channel E edges spread geometrically (linearly for the cosine) over the finite values v f32[R][B][4] holds, one of them replaced by a value
    that occurs, then sorted."""
    e = np.zeros((4, E), F)
    for k in range(4):
        vals = v[..., k][~nf & np.isfinite(v[..., k])]
        lo, hi = float(vals.min()), float(vals.max())
        if k == 2:
            e[k] = np.linspace(lo, hi, E + 2)[1:-1]
        else:
            e[k] = np.geomspace(max(lo, 1e-12), max(hi, 2e-12), E + 2)[1:-1]
        if E:
            e[k, rng.integers(E)] = vals[rng.integers(vals.size)]
        e[k] = np.sort(e[k])
    return e


@functools.lru_cache(maxsize=None)
def prepared(B, G, E, over, substeps, seed=900, mlp_dtype=None, math_mode=None):
    """Everything a test of one case needs, computed ONCE and shared (never changed): the inputs, the oracle loop's outputs `want` (xsub last), the targets g, the
    Score, the Ensemble and cohort array, the oracle's score words, the shared per-row terms and the reference words."""
    arith = {} if mlp_dtype is None else dict(mlp_dtype=mlp_dtype, math_mode=math_mode)
    cfg, model, x0, xref, keys, kw = inputs(B, seed, **arith)
    want = oracle_loop(cfg, model, x0, xref, keys, T4, **kw)
    g = targets(xref, T4)
    fin = finite_episodes(want[-1])
    score = thresholds_from(want[0], want[-1], g, finite=fin, substeps=substeps)
    z = score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), substeps, S2)
    rows = want[-1] if substeps else want[0][:, 1:]
    rpt = N2 if substeps else 1
    terms = channels(rows, g, score.thresholds(), rpt)
    ens = Ensemble.from_device_edges(edges_for(terms[0], terms[1], E, np.random.default_rng(seed + B)), over="alive" if over else "all", n_cohorts=G)
    coh = cohorts(B, G)
    words = ensemble_ref(rows, g, z, coh, ens.edges, score.thresholds(), G, over, rpt, terms=terms)
    return dict(cfg=cfg, model=model, x0=x0, xref=xref, keys=keys, kw=kw, want=want, g=g, score=score, ens=ens, cohort=coh, z=z, rows=rows, rpt=rpt, terms=terms,
                words=words, G=G, E=E, over=over, substeps=substeps, B=B)


def reference(case, over=None, mutant=None, rows=None, z=None, words_before=None):
    """ensemble_ref on a prepared case: its own rows and words (sharing the per-row terms), or other rows / final score words (a device call's own)."""
    c = case
    terms = c["terms"] if rows is None else None
    return ensemble_ref(c["rows"] if rows is None else rows, c["g"], c["z"] if z is None else z, c["cohort"], c["ens"].edges, c["score"].thresholds(), c["G"],
                        c["over"] if over is None else over, c["rpt"], mutant=mutant, words_before=words_before, terms=terms)
