"""CPU reference of the closed loop flown by the geometric baseline controller (SPEC.md §11l): the existing reference chain (event_loop_ref, track_loop_ref and
everything below them, untouched) with the CONTROLLER's oracle — the first oracle a loop asks oracle_for for; the plants' come after it — replaced by one whose
`solve` returns the table of §11l step 8 from geo_ref.geo_command. The solve's noise argument is still formed by the loop and simply not used, so the key schedule
is the loop's own. Test infrastructure, like the *_loop_ref.py modules, none of which is edited or copied."""
import contextlib
import sys

import numpy as np

import closed_loop_ref
from geo_ref import geo_command, geo_command64, geo_table, par_row

F = np.float32
_LOOP_MODULES = ("timed_loop_ref", "scenario_loop_ref", "rate_loop_ref", "fault_loop_ref", "obs_loop_ref", "age_loop_ref", "plant_loop_ref", "closed_loop_ref")


class _Baseline:
    """An Oracle whose solve is the controller's table; everything else (step, the configuration) is the real oracle's."""

    def __init__(self, oracle, cfg, par, accel_ff, ref_row, mutant, census, episode_of, f64=False):
        self._o, self._cfg, self._par, self._ff, self._row, self._mutant, self._census = oracle, cfg, par, accel_ff, ref_row, mutant, census
        self._inv_dt = F(F(1) / F(cfg.time_steps[ref_row]))
        self._episode_of, self._f64 = episode_of, f64

    def __getattr__(self, name):
        return getattr(self._o, name)

    def solve(self, x0, xref, noise, u_init, stepsize_in, trace_cap=0):
        b = self._episode_of()
        if self._f64:              # the float64 restatement, its command rounded to float32 (the convergence test flies both)
            c, w = geo_command64(x0, xref, par_row(self._par, b), self._ff, self._row, float(F(self._cfg.time_steps[self._row])))
            c, w = F(c), np.asarray(w, F)
        else:
            c, w = geo_command(x0, xref, par_row(self._par, b), self._ff, self._row, self._inv_dt, self._mutant, self._census)
        uopt, xevol, info = geo_table(x0, c, w, self._cfg.horizon, self._cfg.num_motors, stepsize_in)
        return uopt, xevol, info, None


@contextlib.contextmanager
def baseline_oracle(par, accel_ff=False, ref_row=0, mutant=None, census=None, f64=False):
    """Inside the block the first oracle_for call of every reference module returns the controller's stand-in; later calls (the plants') the real oracle. The yielded
    dict's "episode" names the episode whose parameter set the stand-in reads (geo_loop_ref runs one episode at a time when the sets differ)."""
    real = closed_loop_ref.oracle_for
    state = {"first": True, "episode": -1}

    def episode_of():
        return state["episode"]

    def wrapped(cfg, model):
        o = real(cfg, model)
        if state["first"]:
            state["first"] = False
            return _Baseline(o, cfg, par, accel_ff, ref_row, mutant, census, episode_of, f64)
        return o
    saved = {}
    for name in _LOOP_MODULES:
        mod = sys.modules.get(name) or __import__(name)
        if hasattr(mod, "oracle_for"):
            saved[name] = mod.oracle_for
            mod.oracle_for = wrapped
    try:
        yield state
    finally:
        for name, fn in saved.items():
            sys.modules[name].oracle_for = fn


def geo_loop_ref(loop_ref, par, cfg, model, x0, accel_ff=False, ref_row=0, mutant=None, census=None, episodes=None, f64=False, **kw):
    """loop_ref(cfg, model, x0=x0, **kw) flown by the controller (kw: the reference's own keyword arguments, plants / xref / keys / T among them). With one
    parameter set the loop runs once; with per-episode sets it runs once per episode (episodes=[b]: every reference fills episode b's rows only) and the rows
    are merged, so each run knows whose parameters it reads."""
    x0 = np.asarray(x0, F)
    per_episode = any(np.asarray(par[n]).shape[0] > 1 for n in par)
    if not per_episode:
        with baseline_oracle(par, accel_ff, ref_row, mutant, census, f64) as st:
            st["episode"] = 0
            return loop_ref(cfg, model, x0=x0, episodes=episodes, **kw)
    out = None
    for b in (range(x0.shape[0]) if episodes is None else episodes):
        with baseline_oracle(par, accel_ff, ref_row, mutant, census, f64) as st:
            st["episode"] = b
            one = loop_ref(cfg, model, x0=x0, episodes=[b], **kw)
        if out is None:
            out = [None if v is None else np.array(v, copy=True) for v in one]
        else:
            for o, v in zip(out, one):
                if o is not None:
                    o[b] = v[b]
    return tuple(out)
