"""Inputs shared by tests/test_gpu_event_loop.py (GPU against the reference) and tests/test_event_loop_cpu.py (the reference against its mutants, on the same
inputs), built from the existing case helpers (process_cases.py and, through it, score_cases.py): score_cfg (H = 6 with two step lengths, P = 33, 3 iterations),
T = 5 with S = 2 (Ns = 3, the last period ragged) and T = 6, n = 2, D = 1, B = 3 .. 5, plus the two Markov chains of SPEC.md §11k: three, four and six motors (three
is the odd lane count, whose last counter is zero-padded), K = 1, 3 and 4 modes, thresholds shared and per episode and distinct in every motor, onset
probabilities around 0.25 per tick and clearing around 0.3, so that things happen within six ticks.

The chain seeds of CASES were chosen by a search over the reference generator ALONE (tests/event_loop_ref.py; no device was involved) so that, across the cases,
it shows an onset into every mode index, a clear, a motor that never fails, two motors of one episode failing in the same tick, an onset at tick 0, an onset at a
tick that is no period start, a dropout at solve 0, a recovery and an episode that is never dropped: `happenings` recomputes them and
tests/test_event_loop_cpu.py asserts each."""
import numpy as np

from process_cases import B5, S2, T5, T6, VALID, chain_keys, meas_keys, score_cfg, scored_episodes, targets, thresholds_from, together  # noqa: F401
from sde4mbrl_px4_amd.solver import Dropouts, FaultProcess
from timed_loop_ref import num_solves

# (motors, modes, episodes, ticks, thresholds per episode, seed of the fault chain, seed of the dropout chain)
CASES = {
    "iris_k3_shared": dict(m=4, K=3, B=5, T=T5, per_episode=False, fseed=900, dseed=1000),
    "iris_k4_per_episode": dict(m=4, K=4, B=4, T=T6, per_episode=True, fseed=910, dseed=1010),
    "hexa_k1_per_episode": dict(m=6, K=1, B=3, T=T5, per_episode=True, fseed=920, dseed=1020),
    "tri_k3_shared": dict(m=3, K=3, B=3, T=T6, per_episode=False, fseed=930, dseed=1033),
    # thresholds ON a drawn word (`boundary`): w < threshold is false there, w <= threshold would be true
    "tri_k3_boundary": dict(m=3, K=3, B=3, T=T5, per_episode=False, fseed=940, dseed=1040, boundary=True),
}


def fault_process(B, m, K, per_episode=True, seed=81):
    """Per motor a total onset probability around 0.25 per tick, split unevenly among the K modes; clearing around 0.3 per tick, the last mode of motor 0 permanent;
    mode rows (kappa, beta) between dead and biased, distinct in every motor and mode."""
    r = np.random.default_rng(seed + 10 * m + K)
    rows = B if per_episode else 1
    share = r.uniform(0.5, 1.5, (rows, m, K))
    p_onset = r.uniform(0.18, 0.32, (rows, m, 1)) * share / share.sum(axis=-1, keepdims=True)
    p_clear = r.uniform(0.2, 0.4, (rows, m, K))
    p_clear[:, 0, K - 1] = 0.0
    modes = np.stack([r.uniform(0.0, 0.9, (rows, m, K)), r.uniform(-0.05, 0.2, (rows, m, K))], axis=-1).astype(np.float32)
    modes[:, :, 0] = 0.0                                   # mode 0 of every motor: dead
    return FaultProcess(p_onset if per_episode else p_onset[0], p_clear if per_episode else p_clear[0], modes if per_episode else modes[0])


def dropouts(B, per_episode=True, seed=82):
    r = np.random.default_rng(seed)
    rows = B if per_episode else 1
    return Dropouts(r.uniform(0.25, 0.45, rows), r.uniform(0.3, 0.5, rows))


def start_states(B, m, K, seed=83):
    """(fault_state_in, drop_state_in) of a run that continues another: some motors already failed, with first ticks in the past, some episodes already dropped."""
    r = np.random.default_rng(seed)
    s = r.integers(0, K + 1, (B, m))
    f = np.where(s > 0, r.integers(0, 7, (B, m)), -1)
    d = r.integers(0, 2, B)
    return np.stack([s, f], axis=-1).astype(np.int32), np.stack([d, d + r.integers(0, 3, B)], axis=-1).astype(np.int32)


def first_words(key, lanes):
    """The words of a chain's first step: random_bits of the second half of split(key)."""
    import orc
    return orc.random_bits(orc.split(key, 2)[1], lanes)


def events(B, m, K, fault=True, drop=True, per_episode=True, states=False, fseed=900, dseed=1000, tick0=0, boundary=False):
    """Keyword arguments of closed_loop for the two chains (meas_keys included with the dropout chain). boundary (shared thresholds, no start states): the first
    onset threshold of motor 1 IS the word episode 0 draws for that motor at tick 0 (the later ones of the row are raised to it where they were below), and the
    dropout threshold IS the word episode 0 draws at solve 0."""
    kw = {}
    fs, ds = start_states(B, m, K) if states else (None, None)
    if fault:
        fp, fk = fault_process(B, m, K, per_episode), chain_keys(B, fseed)
        if boundary:
            assert not per_episode
            on = fp.onset.copy()
            on[0, 1] = np.maximum(on[0, 1], first_words(fk[0], m)[1])
            on[0, 1, 0] = first_words(fk[0], m)[1]
            fp = FaultProcess.from_thresholds(on, fp.clear, fp.modes)
        kw.update(fault_process=fp, fault_keys=fk, fault_state_in=fs)
        if tick0 or states:
            kw.update(fault_tick0=tick0 if tick0 else 7)
    if drop:
        dp, dk = dropouts(B, per_episode), chain_keys(B, dseed)
        if boundary:
            dp = Dropouts.from_thresholds(first_words(dk[0], 1)[0], dp.recover)
        kw.update(drop_process=dp, drop_keys=dk, drop_state_in=ds, meas_keys=meas_keys(B))
    return kw


def case_events(name, **over):
    c = CASES[name]
    return events(c["B"], c["m"], c["K"], per_episode=c["per_episode"], fseed=c["fseed"], dseed=c["dseed"], boundary=c.get("boundary", False) and not over.get("states"),
                  **over)


def for_ref(kw, B, m):
    """The same keyword arguments for event_loop_ref: the FaultProcess as its (onset, clear, modes) arrays, the Dropouts as (drop, recover); the Gauss-Markov
    processes of process_cases, if any, as process_cases.for_ref gives them."""
    from process_cases import for_ref as gm_for_ref
    out = gm_for_ref(kw, B)
    if out.get("fault_process") is not None:
        out["fault_process"] = out["fault_process"].arrays(B, m)
    if out.get("drop_process") is not None:
        out["drop_process"] = out["drop_process"].arrays(B)
    return out


def happenings(name):
    """What the reference generator shows on a case (see the module docstring): a dict of the conditions, each True or False, and the set of mode indices entered."""
    from event_loop_ref import drop_rows, fault_rows
    c = CASES[name]
    B, m, K, T = c["B"], c["m"], c["K"], c["T"]
    kw = for_ref(case_events(name), B, m)
    _, _, st, s = fault_rows(kw["fault_keys"], *kw["fault_process"], None, T)
    prev = np.concatenate([np.zeros((B, 1, m), np.int64), s[:, :-1]], axis=1)
    onset, clear = (prev == 0) & (s > 0), (prev > 0) & (s == 0)
    ticks = np.arange(T)[None, :, None]
    _, _, _, d = drop_rows(kw["drop_keys"], *kw["drop_process"], None, num_solves(T, S2))
    dprev = np.concatenate([np.zeros((B, 1), np.int64), d[:, :-1]], axis=1)
    return dict(modes=set(int(v) - 1 for v in s[onset]), clear=bool(clear.any()), never_fails=bool((s == 0).all(axis=1).any()),
                two_in_one_tick=bool((onset.sum(axis=2) >= 2).any()), onset_at_tick0=bool(onset[:, 0].any()),
                onset_inside_period=bool((onset & (ticks % S2 != 0)).any()), drop_at_solve0=bool((d[:, 0] == 1).any()),
                recovery=bool(((dprev == 1) & (d == 0)).any()), never_dropped=bool((d == 0).all(axis=1).any()),
                first_matches=bool((np.where(onset.any(axis=1), onset.argmax(axis=1), -1) == st[:, :, 1]).all()))
