"""CPU reference of the closed loop with motor faults and estimator dropouts drawn on the device (SPEC.md §11k): event_rows, the generator of the two Markov
chains, written with orc.split and orc.random_bits only — every decision is an integer compare — and event_loop_ref, which is process_loop_ref
(tests/process_loop_ref.py) called with fault= / meas_valid= set to the generated rows. So the loop is the already-verified one and the only new logic is the
generator. Test infrastructure, like process_loop_ref.py.

`mutant` builds a deliberately WRONG generator, for the discrimination tests: "split_swapped" takes the second half of the split as the chain and the first as the
draw key, "words_reversed" gives motor l the word of motor m - 1 - l, "le_for_lt" fires on w <= threshold, "fault_per_solve" steps the fault chain at the first tick
of a solve period only and holds its rows over the period, "onset_and_clear" tests a lane that has just failed for clearing in the same step, "state_not_carried"
starts every solve period from state_in, "scheduled_dropped" writes the neutral row in state 0 although a schedule is given, "mode_off_by_one" reads the next mode's
row, "drop_held_on_invalid" does not step the dropout chain at a solve whose scheduled flag is 0, "first_overwritten" lets a later onset overwrite `first`."""
import numpy as np

import orc
from process_loop_ref import process_loop_ref
from timed_loop_ref import num_solves

F = np.float32
U32 = np.uint32
I32 = np.int32
FAULT_MUTANTS = ("split_swapped", "words_reversed", "le_for_lt", "fault_per_solve", "onset_and_clear", "state_not_carried", "scheduled_dropped", "mode_off_by_one",
                 "first_overwritten")
DROP_MUTANTS = ("split_swapped", "le_for_lt", "onset_and_clear", "state_not_carried", "drop_held_on_invalid")
MUTANTS = FAULT_MUTANTS + ("drop_held_on_invalid",)


def _fires(w, threshold, mutant):
    return int(w) <= int(threshold) if mutant == "le_for_lt" else int(w) < int(threshold)


def _step(c, lanes, mutant):
    """(chain, words): one split and one draw of `lanes` words."""
    c, e = orc.split(c, 2)
    if mutant == "split_swapped":
        c, e = e, c
    w = orc.random_bits(e, lanes)
    return c, (w[::-1] if mutant == "words_reversed" else w)


def _next_state(s, w, onset, clear, mutant):
    """The transition of one lane: onset u32[K] cumulative, clear u32[K]."""
    K = len(onset)
    if s == 0:
        for j in range(K):
            if _fires(w, onset[j], mutant):
                if mutant == "onset_and_clear" and _fires(w, clear[j], mutant):
                    return 0
                return j + 1
        return 0
    return 0 if _fires(w, clear[s - 1], mutant) else s


def _par(a, B, tail, dtype, what):
    a = np.asarray(a, dtype)
    if a.ndim == len(tail):
        a = a[None]
    assert a.shape[1:] == tail and a.shape[0] in (1, B), (what, a.shape)
    return a


def fault_rows(keys, onset, clear, modes, state, T, tick0=0, scheduled=None, S=1, mutant=None):
    """T steps of the fault chain for every episode. keys uint32[B][2]; onset / clear u32[1 or B][m][K] (onset cumulative); modes f32[1 or B][m][K][2]; state
    int32[B][m][2] = (s, first) or None: (0, -1); scheduled f32[T or 1][B or 1][m][2] or None; S: the solve period (the two period-level mutants). Returns
    (rows f32[B][T][m][2], keys_next uint32[B][2], state_next int32[B][m][2], states int[B][T][m]: the state DURING each tick)."""
    assert mutant is None or mutant in FAULT_MUTANTS
    keys = np.asarray(keys, U32)
    B = keys.shape[0]
    onset = np.asarray(onset, U32)
    m, K = onset.shape[-2:]
    onset, clear, modes = _par(onset, B, (m, K), U32, "onset"), _par(clear, B, (m, K), U32, "clear"), _par(modes, B, (m, K, 2), F, "modes")
    state_in = np.tile(np.array([0, -1], I32), (B, m, 1)) if state is None else np.asarray(state, I32).reshape(B, m, 2)
    if scheduled is not None:
        scheduled = np.asarray(scheduled, F)
        assert scheduled.ndim == 4 and scheduled.shape[0] in (1, T) and scheduled.shape[1] in (1, B) and scheduled.shape[2:] == (m, 2), scheduled.shape
    rows = np.zeros((B, T, m, 2), F)
    states = np.zeros((B, T, m), np.int64)
    keys_next, state_next = np.zeros((B, 2), U32), np.zeros((B, m, 2), I32)
    neutral = np.array([1.0, 0.0], F)
    for b in range(B):
        c = keys[b].copy()
        s, first = state_in[b, :, 0].copy(), state_in[b, :, 1].copy()
        on, cl, md = onset[b if onset.shape[0] > 1 else 0], clear[b if clear.shape[0] > 1 else 0], modes[b if modes.shape[0] > 1 else 0]
        for k in range(T):
            if mutant == "state_not_carried" and k % S == 0:
                s = state_in[b, :, 0].copy()
            if mutant != "fault_per_solve" or k % S == 0:
                c, w = _step(c, m, mutant)
                for l in range(m):
                    sn = _next_state(int(s[l]), w[l], on[l], cl[l], mutant)
                    if s[l] == 0 and sn > 0 and (first[l] < 0 or mutant == "first_overwritten"):
                        first[l] = tick0 + k
                    s[l] = sn
            states[b, k] = s
            for l in range(m):
                if s[l] > 0:
                    rows[b, k, l] = md[l, (s[l] % K) if mutant == "mode_off_by_one" else s[l] - 1]
                elif scheduled is not None and mutant != "scheduled_dropped":
                    rows[b, k, l] = scheduled[k if scheduled.shape[0] > 1 else 0, b if scheduled.shape[1] > 1 else 0, l]
                else:
                    rows[b, k, l] = neutral
        keys_next[b] = c
        state_next[b, :, 0], state_next[b, :, 1] = s, first
    return rows, keys_next, state_next, states


def drop_rows(keys, drop, recover, state, Ns, scheduled=None, mutant=None):
    """Ns steps of the dropout chain for every episode. keys uint32[B][2]; drop / recover u32[1 or B] (or scalars); state int32[B][2] = (s, n_dropped) or None:
    zeros; scheduled int[Ns or 1][B or 1] or None: the scheduled valid flags. Returns (flags int32[B][Ns], keys_next, state_next int32[B][2], states int[B][Ns])."""
    assert mutant is None or mutant in DROP_MUTANTS
    keys = np.asarray(keys, U32)
    B = keys.shape[0]
    drop, recover = _par(np.atleast_1d(drop), B, (), U32, "drop"), _par(np.atleast_1d(recover), B, (), U32, "recover")
    state_in = np.zeros((B, 2), I32) if state is None else np.asarray(state, I32).reshape(B, 2)
    if scheduled is not None:
        scheduled = np.asarray(scheduled)
        assert scheduled.ndim == 2 and scheduled.shape[0] in (1, Ns) and scheduled.shape[1] in (1, B), scheduled.shape
    flags = np.zeros((B, Ns), I32)
    states = np.zeros((B, Ns), np.int64)
    keys_next, state_next = np.zeros((B, 2), U32), np.zeros((B, 2), I32)
    for b in range(B):
        c = keys[b].copy()
        s, n = int(state_in[b, 0]), int(state_in[b, 1])
        dr, re = drop[b if drop.shape[0] > 1 else 0], recover[b if recover.shape[0] > 1 else 0]
        for j in range(Ns):
            v = 1 if scheduled is None else int(scheduled[j if scheduled.shape[0] > 1 else 0, b if scheduled.shape[1] > 1 else 0] != 0)
            if mutant == "state_not_carried":
                s = int(state_in[b, 0])
            if not (mutant == "drop_held_on_invalid" and v == 0):
                c, w = _step(c, 1, mutant)
                s = _next_state(s, w[0], [dr], [re], mutant)
            n += s
            states[b, j] = s
            flags[b, j] = 1 if s == 0 and v else 0
        keys_next[b] = c
        state_next[b] = (s, n)
    return flags, keys_next, state_next, states


def event_rows(T, S, fault=None, drop=None, mutant=None):
    """Both generators at once. fault: dict(keys, onset, clear, modes, state=None, tick0=0, scheduled=None) or None; drop: dict(keys, drop, recover, state=None,
    scheduled=None) or None. Returns (fault part or None, drop part or None), each what fault_rows / drop_rows return."""
    f = d = None
    if fault is not None:
        f = fault_rows(fault["keys"], fault["onset"], fault["clear"], fault["modes"], fault.get("state"), T, fault.get("tick0", 0), fault.get("scheduled"), S,
                       mutant if mutant in FAULT_MUTANTS else None)
    if drop is not None:
        d = drop_rows(drop["keys"], drop["drop"], drop["recover"], drop.get("state"), num_solves(T, S), drop.get("scheduled"),
                      mutant if mutant in DROP_MUTANTS else None)
    return f, d


def _sched(a, N, tail, dtype):
    """A schedule in closed_loop's shapes ([N or 1][B or 1] + tail, [N] + tail or tail) as [N or 1][B or 1] + tail."""
    if a is None:
        return None
    a = np.asarray(a, dtype)
    if a.ndim == len(tail):
        a = a.reshape((1, 1) + tail)
    elif a.ndim == len(tail) + 1:
        assert a.shape[0] == N
        a = a[:, None]
    return a


def event_loop_ref(cfg, model, plants, x0, xref, keys, T, fault_process=None, fault_keys=None, fault_state_in=None, fault_tick0=0, drop_process=None, drop_keys=None,
                   drop_state_in=None, fault=None, meas_valid=None, S=1, substep_states=False, mutant=None, **kw):
    """The §11k loop: process_loop_ref with fault= / meas_valid= set to the rows of event_rows. fault_process is (onset, clear, modes) as fault_rows takes them,
    drop_process (drop, recover); a scheduled fault / meas_valid given as well goes through the generator. Returns what SdeMpcSolver.closed_loop returns:
    process_loop_ref's values, then (fault_rows [B][T][m][2], fault_keys_next, fault_state_next) with a fault process, then (valid_rows [B][Ns], valid_keys_next,
    valid_state_next) with a dropout process, then xsub if asked for."""
    assert mutant is None or mutant in MUTANTS
    x0 = np.asarray(x0, F)
    T, S, m = int(T), int(S), cfg.num_motors
    Ns = num_solves(T, S)
    f = d = None
    if fault_process is not None:
        f = dict(keys=fault_keys, onset=fault_process[0], clear=fault_process[1], modes=fault_process[2], state=fault_state_in, tick0=fault_tick0,
                 scheduled=_sched(fault, T, (m, 2), F))
    if drop_process is not None:
        d = dict(keys=drop_keys, drop=drop_process[0], recover=drop_process[1], state=drop_state_in, scheduled=_sched(meas_valid, Ns, (), np.int64))
    fr, dr = event_rows(T, S, f, d, mutant)
    more = ()
    if fr is not None:
        fault = np.ascontiguousarray(fr[0].transpose(1, 0, 2, 3))
        more += fr[:3]
    if dr is not None:
        meas_valid = np.ascontiguousarray(dr[0].T)
        more += dr[:3]
    out = process_loop_ref(cfg, model, plants, x0, xref, keys, T, fault=fault, meas_valid=meas_valid, S=S, substep_states=substep_states, **kw)
    return out[:-1] + more + out[-1:] if substep_states else out + more
