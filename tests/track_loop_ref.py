"""CPU reference of the closed loop tracking a trajectory (SPEC.md §11j): track_rows, the reference-window generator, and track_targets, the score-target
generator, written with NumPy float32, the software fma of the NumPy restatement (oracle/sde_mpc_numpy.py, timed_loop_ref.R2) and age_loop_ref.renormalise; and
track_loop_ref, which is process_loop_ref (tests/process_loop_ref.py) called with xref= set to those windows (the targets come back beside it, for
score_loop_ref.score_rows). So the loop is the already-verified one and the only new arithmetic is the row. Every row is evaluated one at a time with the
bisection the specification states: nothing here is shared with solver.Trajectory. Test infrastructure, like process_loop_ref.py.

`mutant` builds a deliberately WRONG generator, for the discrimination tests: "a_fused" keeps a = (tau - t[i]) * w[i] unrounded inside the interpolation's fma (one rounding for both), "divide" divides by
t[i+1] - t[i], "clock_accumulated" adds dt tick by tick, "c_float32" sums the window's clock offsets in float32, "c_next" reads window row i at c[i+1],
"target_at_k" reads the score target of tick k at theta(k), "rate_unscaled" leaves velocity and body rates as the table has them, "wrap_fmod" wraps the
trajectory time with fmod, "search_strict" picks the segment with t[i] < tau, "no_renorm" leaves the attitude as interpolated."""
import numpy as np

from age_loop_ref import renormalise
from process_loop_ref import process_loop_ref
from timed_loop_ref import R2, num_solves

F = np.float32
MUTANTS = ("a_fused", "divide", "clock_accumulated", "c_float32", "c_next", "target_at_k", "rate_unscaled", "wrap_fmod", "search_strict", "no_renorm")


def _fma(a, b, c):
    return np.asarray(R2.fma(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)), F)


def clock(k, dt, mutant=None):
    """theta(k) = float32(k) * dt: one multiplication (the mutant: k additions)."""
    dt = F(dt)
    if mutant == "clock_accumulated":
        th = F(0.0)
        for _ in range(int(k)):
            th = F(th + dt)
        return th
    return F(F(int(k)) * dt)


def offsets(time_steps, mutant=None):
    """c[i], i = 0 .. H (and one entry more, for the c_next mutant: the last step once again): the float64 cumulative sum cast once."""
    ts = np.asarray(time_steps)
    ts = np.concatenate([ts, ts[-1:]])
    if mutant == "c_float32":
        c = [F(0.0)]
        for v in ts:
            c.append(F(c[-1] + F(v)))
        return np.asarray(c, F)
    return np.concatenate([[0.0], np.cumsum(ts.astype(F).astype(np.float64))]).astype(F)


def row(table, u, phase, rate, offset, renorm=True, mutant=None):
    """One row of SPEC.md §11j: table = (t f32[L], x f32[L][13], period) at clock value u for one episode's (phase, rate, offset)."""
    t, x, period = np.asarray(table[0], F), np.asarray(table[1], F), F(table[2])
    L = t.shape[0]
    u, phase, rate = F(u), F(phase), F(rate)
    if L == 1:
        y = x[0].copy()
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            tau = F(_fma(rate, u, phase))
            if period > 0:
                if mutant == "wrap_fmod":
                    tau = F(np.fmod(tau, period))
                else:
                    inv = F(1.0 / np.float64(period))
                    n = F(np.floor(F(tau * inv)))
                    tau = F(_fma(-n, period, tau))
            tau = tau if tau > t[0] else t[0]
            tau = tau if tau < t[L - 1] else t[L - 1]
        lo, hi = 0, L - 1
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if (t[mid] < tau) if mutant == "search_strict" else (t[mid] <= tau):
                lo = mid
            else:
                hi = mid
        i = lo
        if mutant == "divide":
            a = F(F(tau - t[i]) / F(t[i + 1] - t[i]))
        elif mutant == "a_fused":
            w = F(1.0 / (np.float64(t[i + 1]) - np.float64(t[i])))
            a = np.float64(F(tau - t[i])) * np.float64(w)                      # (exact in float64: the product is never rounded to float32)
        else:
            w = F(1.0 / (np.float64(t[i + 1]) - np.float64(t[i])))
            a = F(F(tau - t[i]) * w)
        if mutant == "a_fused":
            y = (a * (x[i + 1] - x[i]).astype(F).astype(np.float64) + x[i].astype(np.float64)).astype(F)
        else:
            y = _fma(a, (x[i + 1] - x[i]).astype(F), x[i])
    y[0:3] = (y[0:3] + np.asarray(offset, F)).astype(F)
    if mutant != "rate_unscaled":
        y[3:6] = (y[3:6] * rate).astype(F)
        y[10:13] = (y[10:13] * rate).astype(F)
    if renorm and mutant != "no_renorm":
        y = renormalise(y)
    return y


def _per_episode(B, table_of, phase, rate, offset):
    of = np.zeros(B, np.int64) if table_of is None else np.asarray(table_of, np.int64).reshape(B)
    ph = np.zeros(B, F) if phase is None else np.broadcast_to(np.asarray(phase, F), (B,))
    rt = np.ones(B, F) if rate is None else np.broadcast_to(np.asarray(rate, F), (B,))
    off = np.zeros((B, 3), F) if offset is None else np.broadcast_to(np.asarray(offset, F), (B, 3))
    return of, ph, rt, off


def track_rows(tables, time_steps, ticks, B, table_of=None, phase=None, rate=None, offset=None, renorm=True, mutant=None, episodes=None):
    """The reference windows f32[n][B][H+1][13] of the solves at the GLOBAL ticks `ticks`: row i at u = theta(k) + c[i]. tables: a list of (t, x, period).
    episodes: evaluate these only (the others stay zero)."""
    assert mutant is None or mutant in MUTANTS
    of, ph, rt, off = _per_episode(B, table_of, phase, rate, offset)
    H = len(time_steps)
    c = offsets(time_steps, mutant)
    sh = 1 if mutant == "c_next" else 0
    out = np.zeros((len(ticks), B, H + 1, 13), F)
    for g, k in enumerate(ticks):
        th = clock(k, time_steps[0], mutant)
        for b in (range(B) if episodes is None else episodes):
            for i in range(H + 1):
                out[g, b, i] = row(tables[of[b]], F(th + c[i + sh]), ph[b], rt[b], off[b], renorm, mutant)
    return out


def track_targets(tables, time_steps, ticks, B, table_of=None, phase=None, rate=None, offset=None, renorm=True, mutant=None, episodes=None):
    """The score targets f32[n][B][13] of the GLOBAL ticks `ticks`: the row at u = theta(k + 1)."""
    assert mutant is None or mutant in MUTANTS
    of, ph, rt, off = _per_episode(B, table_of, phase, rate, offset)
    out = np.zeros((len(ticks), B, 13), F)
    for g, k in enumerate(ticks):
        th = clock(k if mutant == "target_at_k" else k + 1, time_steps[0], mutant)
        for b in (range(B) if episodes is None else episodes):
            out[g, b] = row(tables[of[b]], th, ph[b], rt[b], off[b], renorm, mutant)
    return out


def track_loop_ref(cfg, model, plants, x0, tables, keys, T, track_of=None, track_phase=None, track_rate=None, track_offset=None, track_tick0=0, track_renorm=True,
                   S=1, episodes=None, mutant=None, **kw):
    """The §11j loop: process_loop_ref on the windows of track_rows, one per solve (the solve of period j sits at global tick track_tick0 + j S). Returns
    (what process_loop_ref returns, xref f32[Ns][B][H+1][13], targets f32[T][B][13])."""
    x0 = np.asarray(x0, F)
    B, T, S = x0.shape[0], int(T), int(S)
    Ns = num_solves(T, S)
    ts = np.asarray(cfg.time_steps)
    par = dict(table_of=track_of, phase=track_phase, rate=track_rate, offset=track_offset, renorm=track_renorm, mutant=mutant, episodes=episodes)
    xref = track_rows(tables, ts, [track_tick0 + j * S for j in range(Ns)], B, **par)
    g = track_targets(tables, ts, [track_tick0 + k for k in range(T)], B, **par)
    out = process_loop_ref(cfg, model, plants, x0, xref, keys, T, S=S, episodes=episodes, **kw)
    return out, xref, g
