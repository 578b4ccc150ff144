"""CPU reference of the closed loop that retires failed episodes (SPEC.md §11n), built from the existing reference chain, untouched, in two passes.

Pass 1 runs the unretired loop reference and scores it with score_rows (tests/score_loop_ref.py): the first failing row of every episode gives the solve index at
which the episode is retired — the first solve after the period the row lies in; 0 for an episode whose score_in already holds a failure. Pass 2 runs the same
chain, one retired episode at a time, with the CONTROLLER's oracle wrapped the way geo_loop_ref.baseline_oracle wraps it: from that solve index on the stand-in's
`solve` returns the held tables (the last solve's, or at entry the warm start and x0 in every row) and the held info row (0, stepsize, 0 ..). Everything else of
the loop — plant, keys, chains, history, windows — is the reference's own. The score words are score_rows over the rows up to the retirement.

live_list restates the device's count / place arithmetic in NumPy: block counts of 256 episodes, wave offsets of 64 lanes and lane ranks.

`mutant` builds a deliberately WRONG variant, for the discrimination tests. Loop mutants: "retire_late" (one period late), "retire_early" (at the solve of the
failing period itself), "step_dropped" (the held info row has step size 0), "tables_reset" (a retired episode flies the call's warm start, not its held table),
"info_kept" (the held info row is the last solve's), "entry_ignored" (a failure in score_in does not retire), "scoring_not_frozen" (the words count every row),
"frozen_at_row" (the words stop at the failing row, not at the end of its period). List mutants: "list_unstable" (descending inside a wave),
"wave_mask_off_by_one" (lane 63 is left out of the wave offset), "block_mask_off_by_one" (a block's count leaves out its last thread), "n_live_wrong_block"
(n_live without the last block's count), "rank_inclusive" (a lane counts itself)."""
import contextlib
import sys

import numpy as np

from score_loop_ref import NONE, as_words, initial_rows, score_rows

F = np.float32
_LOOP_MODULES = ("timed_loop_ref", "scenario_loop_ref", "rate_loop_ref", "fault_loop_ref", "obs_loop_ref", "age_loop_ref", "plant_loop_ref", "closed_loop_ref")
LOOP_MUTANTS = ("retire_late", "retire_early", "step_dropped", "tables_reset", "info_kept", "entry_ignored", "scoring_not_frozen", "frozen_at_row")
LIST_MUTANTS = ("list_unstable", "wave_mask_off_by_one", "block_mask_off_by_one", "n_live_wrong_block", "rank_inclusive")


class _Retired:
    """An Oracle whose solve, from solve index `at` on, returns the held tables and the held info row; everything else is the wrapped oracle's."""

    def __init__(self, oracle, at, x0, mutant):
        self._o, self._at, self._x0, self._mutant = oracle, at, np.asarray(x0, F), mutant
        self._j, self._held, self._first, self._info = 0, None, None, None

    def __getattr__(self, name):
        return getattr(self._o, name)

    def solve(self, x0, xref, noise, u_init, stepsize_in, trace_cap=0):
        j, self._j = self._j, self._j + 1
        if self._first is None:            # the tables of the call's entry: the warm start, and x0 in every row
            u = np.asarray(u_init, F).copy()
            self._first = (u, np.repeat(self._x0[None], u.shape[0] + 1, axis=0))
            self._held = self._first
        if j < self._at:
            uo, xe, inf, tr = self._o.solve(x0, xref, noise, u_init, stepsize_in, trace_cap)
            self._held, self._info = (np.asarray(uo, F).copy(), np.asarray(xe, F).copy()), np.asarray(inf, F).copy()
            return uo, xe, inf, tr
        uo, xe = self._first if self._mutant == "tables_reset" else self._held
        inf = np.zeros(8, F)
        inf[1] = F(0.0) if self._mutant == "step_dropped" else F(stepsize_in)
        if self._mutant == "info_kept" and self._info is not None:
            inf = self._info.copy()
        return uo.copy(), xe.copy(), inf, None


@contextlib.contextmanager
def retired_oracle(at, x0, mutant=None):
    """Inside the block the first oracle_for call of every reference module returns the stand-in around whatever that call returned before (the real oracle, or
    geo_loop_ref's baseline stand-in when this block sits inside baseline_oracle); later calls (the plants') are untouched."""
    state = {"first": True}
    saved = {}

    def wrap(fn):
        def wrapped(cfg, model):
            o = fn(cfg, model)
            if state["first"]:
                state["first"] = False
                return _Retired(o, at, x0, mutant)
            return o
        return wrapped
    for name in _LOOP_MODULES:
        mod = sys.modules.get(name) or __import__(name)
        if hasattr(mod, "oracle_for"):
            saved[name] = mod.oracle_for
            mod.oracle_for = wrap(saved[name])
    try:
        yield
    finally:
        for name, fn in saved.items():
            sys.modules[name].oracle_for = fn


def _targets(g, T):
    g = np.asarray(g, F)
    if g.ndim == 1:
        g = g[None, None]
    elif g.ndim == 2:
        g = g[:, None]
    assert g.shape[0] in (1, T) and g.shape[2] == 13
    return g


def _targets_of(g, Tb, b):
    """The targets of episode b's first Tb ticks, [Tb or 1][1][13]."""
    g = g[:Tb] if g.shape[0] > 1 else g
    return g[:, b:b + 1] if g.shape[1] > 1 else g


def retire_solves(z, z_in, rows_per_tick, S, Ns, mutant=None):
    """int[B]: the solve index from which each episode is not solved (Ns and above: never in this call), from the score words z of the unretired run and z_in."""
    z, z_in = as_words(z), as_words(z_in)
    at = np.full(z.shape[0], 1 << 30, np.int64)
    for b in range(z.shape[0]):
        if z_in[b, 8] != NONE:
            at[b] = 1 << 30 if mutant == "entry_ignored" else 0
        elif z[b, 8] != NONE:
            tick = (int(z[b, 8]) - int(z_in[b, 0])) // rows_per_tick
            at[b] = tick // S + 1 + (1 if mutant == "retire_late" else -1 if mutant == "retire_early" else 0)
    return at


def retire_loop_ref(run_ref, cfg, x0, g, thresholds, substeps, S, n, T, score_in=None, mutant=None, first=None):
    """run_ref(episodes, ctx) -> the reference loop's values for closed_loop's arguments (xs, us, info first; xsub LAST; every value per episode), run over all
    episodes for episodes=None and over [b] otherwise; it enters the context manager ctx() right around the reference loop's call (inside geo_loop_ref's
    baseline_oracle where the controller flies, so that this stand-in wraps that one). Returns (values, score words u32[B][16], retired_at int32[B], live int32[Ns], first) where `first` is
    pass 1's (values, words) — pass it back in to share it between calls on the same inputs."""
    assert mutant is None or mutant in LOOP_MUTANTS
    x0 = np.asarray(x0, F)
    B, T, S, n = x0.shape[0], int(T), int(S), int(n)
    Ns = -(-T // S)
    g = _targets(g, T)
    rpt = n if substeps else 1
    z_in = initial_rows(B) if score_in is None else as_words(score_in)
    if first is None:
        want = run_ref(None, contextlib.nullcontext)
        first = (want, score_rows(want[0], want[1], want[2], want[-1], g, cfg, thresholds, substeps, S, score_in=z_in))
    want, z1 = first
    at = retire_solves(z1, z_in, rpt, S, Ns, mutant)
    out = [None if v is None else np.array(v, copy=True) for v in want]
    for b in range(B):
        if at[b] >= Ns:
            continue
        one = run_ref([b], lambda b=b: retired_oracle(int(at[b]), x0[b], mutant))
        for o, v in zip(out, one):
            if o is not None:
                o[b] = v[b]
    z = z_in.copy()
    for b in range(B):
        Tb = T if mutant == "scoring_not_frozen" else min(int(at[b]) * S, T)
        if z_in[b, 8] != NONE and mutant != "entry_ignored":
            Tb = 0
        if Tb == 0:
            continue
        gb = _targets_of(g, Tb, b)
        zb = score_rows(out[0][b:b + 1, :Tb + 1], out[1][b:b + 1, :Tb], out[2][b:b + 1, :-(-Tb // S)], out[-1][b:b + 1, :Tb * n], gb, cfg, thresholds, substeps, S,
                        score_in=z_in[b:b + 1])
        if mutant == "frozen_at_row" and zb[0, 8] != NONE and z_in[b, 8] == NONE:
            rows = int(zb[0, 8]) - int(z_in[b, 0]) + 1
            Tr = -(-rows // rpt)
            zb = score_rows(out[0][b:b + 1, :Tr + 1], out[1][b:b + 1, :Tr], out[2][b:b + 1, :-(-Tr // S)], out[-1][b:b + 1, :Tr * n],
                            _targets_of(g, Tr, b), cfg, thresholds, substeps, S, score_in=z_in[b:b + 1])
        z[b] = zb[0]
    retired_at = np.where(at < Ns, at, -1).astype(np.int32)
    live = np.array([(at > j).sum() for j in range(Ns)], np.int32)
    return tuple(out), z, retired_at, live, first


def live_list(live, mutant=None):
    """(list int32[n_live], n_live, block counts) of the flags live[B], by the device's arithmetic: per block of 256 episodes the sum of its four wave counts; the
    rank of a live episode is the counts of the lower blocks, plus the live lanes of the lower waves of its block, plus the live lanes below it in its wave."""
    assert mutant is None or mutant in LIST_MUTANTS
    live = np.asarray(live).astype(bool)
    B = live.size
    nblk = -(-B // 256)
    pad = np.zeros(nblk * 256, bool)
    pad[:B] = live
    waves = pad.reshape(nblk, 4, 64)
    wave_cnt = waves.sum(axis=2)
    if mutant == "wave_mask_off_by_one":
        wave_cnt = waves[:, :, :63].sum(axis=2)
    blk = wave_cnt.sum(axis=1)
    if mutant == "block_mask_off_by_one":
        blk = blk - waves[:, 3, 63]
    out = np.full(B + 256, -1, np.int64)
    for k in range(nblk):
        base = int(blk[:k].sum())
        for w in range(4):
            woff = int(wave_cnt[k, :w].sum())
            for l in range(64):
                if not waves[k, w, l]:
                    continue
                below = int(waves[k, w, :l + 1].sum()) if mutant == "rank_inclusive" else int(waves[k, w, :l].sum())
                if mutant == "list_unstable":
                    below = int(waves[k, w, l + 1:].sum())
                out[base + woff + below] = k * 256 + w * 64 + l
    n_live = int(blk[:-1].sum()) if mutant == "n_live_wrong_block" else int(blk.sum())
    return out[:n_live].astype(np.int32), n_live, blk.astype(np.uint32)
