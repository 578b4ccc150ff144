"""Motor faults and estimator dropouts drawn on the GPU (SPEC.md §11k, sdempc_closed_loop_batch_events): every returned value bit for bit (keys and states as
integers) against event_loop_ref (tests/event_loop_ref.py), which is the already-verified loop on the rows of the integer reference generator. Shapes of
tests/event_cases.py, the smallest at which this path can go wrong: H = 6 with two step lengths, 3 iterations, S = 2, n = 2, T = 5 (a ragged last period) and T = 6,
B = 3 to 5; every arithmetic with and without the rate loop; P = 1 and 33; three (the odd lane count), four and six motors with one, three and four modes; a threshold
ON a drawn word; each chain alone and both together with a scheduled fault and scheduled flags, both Gauss-Markov processes, a plant switch, an aged and
renormalised measurement, a score and a track; thresholds shared and per episode; the GPU against itself (the rows the call returned, fed back as fault and
meas_valid, give the same run); one period per chunk; continuation through tick0 at T = 3 + 3 and T = 2 + 4; a handle with a past and poisoned buffers; B = 258 (the
key kernel's second block and a partly empty third); outputs=False; both cfgs NULL against the tracked entry point."""
import os

import numpy as np
import pytest

import loop_cases
from cases import CDIR, asymmetric_cfg, asymmetric_model, bits_differ
from event_cases import B5, CASES, S2, T5, T6, VALID, case_events, events, for_ref, score_cfg, scored_episodes, targets, thresholds_from, together
from event_loop_ref import event_loop_ref
from fault_cases import faults_any
from loop_cases import ARITH
from process_cases import drawn
from score_loop_ref import score_rows, words_differ
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, SdeMpcSolver, event_summary
from track_cases import for_rows, tracked
from track_loop_ref import track_rows

pytestmark = pytest.mark.gpu
F = np.float32


def ref(cfg, model, x0, xref, keys, T, episodes=None, **kw):
    """The reference loop for closed_loop's keyword arguments, xsub always last."""
    return loop_cases.ref(event_loop_ref, cfg, model, x0, xref, keys, T, episodes=episodes, substep_states=True, **for_ref(kw, x0.shape[0], cfg.num_motors))


def same_values(got, want, eps=None):
    """Two returned tuples agree in shape and in every bit, the keys, states and flags as integers, None with None; eps: compare these episodes only."""
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, i
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (i, g.shape, w.shape, g.dtype, w.dtype)
        if eps is not None:
            g, w = g[eps], w[eps]
        if g.dtype == SCORE_DTYPE:
            assert words_differ(g, w) == 0, i
        elif g.dtype == np.float32:
            assert bits_differ(g, w) == 0, (i, bits_differ(g, w))
        else:
            assert np.array_equal(g, w), i


def run_both(cfg, model, x0, xref, keys, T, kw, max_batch=None, options=None):
    want = ref(cfg, model, x0, xref, keys, T, **kw)
    S = SdeMpcSolver(cfg, model, max_batch=max_batch or x0.shape[0], options=options)
    got = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
    S.solve_status()
    return S, got, want


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_every_arithmetic(mlp_dtype, math_mode, rate):
    """The five episodes of score_cases.py under both chains, thresholds shared, three modes."""
    cfg = score_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 171)
    if rate:
        from score_cases import rate_loop, rate_tail
        kw.update(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B5, cfg.horizon))
    kw.update(case_events("iris_k3_shared"))
    S, got, want = run_both(cfg, model, x0, xref, keys, T5, kw)
    same_values(got, want)
    rows, flags = got[-7], got[-4]
    assert rows.shape == (B5, T5, 4, 2) and flags.shape == (B5, 3) and flags.dtype == np.int32
    assert (rows != np.array([1, 0], F)).any() and (flags == 0).any() and (flags == 1).any()
    S.close()


@pytest.mark.parametrize("P", [1, 33])
def test_particle_counts(P):
    B = 4
    cfg = score_cfg(num_particles=P)
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B, 172)
    kw.update(case_events("iris_k4_per_episode"))
    S, got, want = run_both(cfg, model, x0, xref, keys, T6, kw)
    print("solve kernel:", S.last_kernel_name())
    same_values(got, want)
    S.close()


@pytest.mark.parametrize("case", ["iris_k4_per_episode", "hexa_k1_per_episode", "tri_k3_shared", "tri_k3_boundary"])
def test_motor_and_mode_counts(case):
    """Four motors with four modes, six with one, three (an odd lane count: the last block's second counter is zero) with three; and thresholds ON a drawn word,
    where w < threshold is false."""
    c = CASES[case]
    B, m, T = c["B"], c["m"], c["T"]
    small = dict(horizon=6, num_short_dt=4, short_step_dt=0.05, long_step_dt=0.1, num_particles=33, max_iter=3, max_no_improvement_iter=3)
    if m == 4:
        cfg, model = score_cfg(), synthetic_iris()
    elif m == 6:
        cfg, model = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(**small), synthetic_hexa()
    else:
        cfg, model = asymmetric_cfg(3, **small), asymmetric_model(3)
    x0, xref, keys, kw = scored_episodes(cfg, B, 173)
    kw.update(case_events(case))
    S, got, want = run_both(cfg, model, x0, xref, keys, T, kw)
    same_values(got, want)
    assert got[1].shape == (B, T, m) and got[-7].shape == (B, T, m, 2) and got[-5].shape == (B, m, 2)
    if c.get("boundary"):
        assert got[-4][0, 0] == 1                                                          # w == threshold does not drop
    S.close()


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("which", ["fault", "drop"])
def test_each_chain_alone(which, per_episode):
    """One chain and nothing else of its kind: the fault chain without a schedule or an observation, the dropout chain with an empty obs cfg; T = 5 and T = 6; start
    states absent and given (with a tick0)."""
    B = 4
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B, 174)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    for T, states in ((T5, False), (T6, True)):
        k = dict(kw, **events(B, 4, 3, fault=which == "fault", drop=which == "drop", per_episode=per_episode, states=states))
        want = ref(cfg, model, x0, xref, keys, T, **k)
        got = S.closed_loop(x0, xref, keys, T, substep_states=True, **k)
        S.solve_status()
        same_values(got, want)
        assert len(got) == (11 if which == "fault" else 14)
    S.close()


def everything(cfg, model, x0, T, rate, per_episode=True):
    """together() of score_cases.py — a scheduled fault, a gust schedule, a plant switch, noise, a bias schedule, scheduled dropouts, ages and renormalisation — plus
    both Gauss-Markov processes and both chains."""
    B = x0.shape[0]
    kw = together(model, x0, cfg.horizon, rate, T=T)
    kw["fault"] = faults_any(T, B, cfg.num_motors)                 # (a schedule with a distinct row per tick, episode and motor)
    kw.update({k: v for k, v in drawn(B, per_episode=per_episode).items() if k != "meas_keys"})
    kw.update({k: v for k, v in events(B, cfg.num_motors, 4, per_episode=per_episode, fseed=910, dseed=1010).items() if k != "meas_keys"})
    return kw


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
def test_everything_together_and_the_gpu_against_itself(rate):
    """Both chains on top of a scheduled fault and scheduled flags, both Gauss-Markov processes, a plant switch, an aged and renormalised measurement, a score and a
    track. Then the GPU against itself: the rows the call returned, fed back as fault and meas_valid, give the same run in every shared value — the plant kernel reads
    device-written rows exactly as staged ones. outputs=False leaves the score and the continuation values as they are, None in the row positions."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 171)
    kw.update(everything(cfg, model, x0, T5, rate))
    assert "meas_valid" in kw and "fault" in kw
    tr = tracked(B5)
    tb = [(t.t, t.x, t.period) for t in tr["track"]]
    windows = track_rows(tb, np.asarray(cfg.time_steps), [j * S2 for j in range(3)], B5, **for_rows(tr))
    want = ref(cfg, model, x0, windows, keys, T5, **kw)
    g = targets(windows, T5)
    score = thresholds_from(want[0], want[-1], g)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, None, keys, T5, substep_states=True, score=score, score_ref=g, **kw, **tr)
    S.solve_status()
    z = got[-14]
    assert z.dtype == SCORE_DTYPE
    same_values(got[:-14] + got[-13:], want)
    assert words_differ(z, score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), score.substeps, S2)) == 0
    frows, flags = got[-7], got[-4]
    sched = np.asarray(kw["fault"], F)
    healthy = np.repeat((got[-7] == sched.transpose(1, 0, 2, 3)).all(axis=-1, keepdims=True), 2, axis=-1)
    assert healthy.any() and not healthy.all()                     # some rows are the schedule's, passed through; some a mode's
    assert ((flags == 0) & (np.asarray(kw["meas_valid"]).T != 0)).any()        # a solve the chain dropped although the schedule did not
    summary = event_summary(got[-5], z)
    assert summary["faulted"] >= 1 and summary["episodes"] == B5
    # the rows fed back
    plain = {k: v for k, v in kw.items() if not k.startswith(("fault_", "drop_"))}
    fed = S.closed_loop(x0, None, keys, T5, substep_states=True, score=score, score_ref=g,
                        **dict(plain, fault=np.ascontiguousarray(frows.transpose(1, 0, 2, 3)), meas_valid=np.ascontiguousarray(flags.T)), **tr)
    same_values(fed, got[:-7] + got[-1:])
    # the chains do not depend on the schedules
    alone = S.closed_loop(x0, None, keys, T5, **{k: v for k, v in kw.items() if k not in ("fault", "meas_valid")}, **tr)
    same_values(alone[-5:-3] + alone[-2:], got[-6:-4] + got[-3:-1])
    # outputs=False
    bare = S.closed_loop(x0, None, keys, T5, substep_states=True, score=score, score_ref=g, outputs=False, **kw, **tr)
    S.solve_status()
    n = len(got)
    rows = {0, 1, 2, 7, 10 if rate else 7, n - 13, n - 10, n - 7, n - 4, n - 1}          # xs, us, info, ws, xmeas, dist_rows, bias_rows, fault_rows, valid_rows, xsub
    assert {i for i, v in enumerate(bare) if v is None} == rows
    same_values([v for i, v in enumerate(bare) if i not in rows], [v for i, v in enumerate(got) if i not in rows])
    S.close()


def test_null_cfgs_are_the_tracked_entry_point(monkeypatch):
    """sdempc_closed_loop_batch_events with both event cfgs NULL against sdempc_closed_loop_batch_tracked on every output."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 176)
    kw.update(together(model, x0, cfg.horizon, "stiff"))
    kw.update({k: v for k, v in drawn(B5).items() if k != "meas_keys"})
    tr = tracked(B5)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    plain = S.closed_loop(x0, None, keys, T5, substep_states=True, **kw, **tr)

    def through_events(lib):
        fn = _abi.events_entry(lib)                       # (resolved before the patch below: it builds its prototype from the tracked entry point's)
        return lambda h, *a: fn(h, None, None, *a, None, None, None, None, None, None)
    through_events(S.lib)
    monkeypatch.setattr(_abi, "tracked_entry", through_events)
    null = S.closed_loop(x0, None, keys, T5, substep_states=True, **kw, **tr)
    S.solve_status()
    same_values(null, plain)
    S.close()


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
def test_one_period_per_chunk_changes_no_bit(rate):
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 0: one period per chunk — the fault rows and flags of every period start the chunk's regions anew, the chains and states carry
    over in the handle's buffer; T = 5 and T = 6; thresholds shared."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 177)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    for T in (T5, T6):
        kwT = {**kw, **everything(cfg, model, x0, T, rate, per_episode=False)}
        want = ref(cfg, model, x0, xref, keys, T, **kwT)
        whole = S.closed_loop(x0, xref, keys, T, substep_states=True, **kwT)
        S.set_option("test_loop_chunk_bytes", 0)
        cut = S.closed_loop(x0, xref, keys, T, substep_states=True, **kwT)
        S.set_option("test_loop_chunk_bytes", -1)
        S.solve_status()
        same_values(whole, want)
        same_values(cut, whole)
    S.close()


def test_continuation_through_tick0_and_the_next_values():
    """The fault chain alone at T = 3 + 3 (the cut inside a solve period: its chain advances per tick, so any T continues — the solver's own values continue only at
    period ends, so the joined run is compared in the chain's values, `first` included, which needs tick0 + 3); both chains at T = 2 + 4 (whole periods) in every
    value of the joined run."""
    cfg = score_cfg()
    model = synthetic_iris()
    B = 4
    x0, xref, keys, kw = scored_episodes(cfg, B, 178)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    kf = dict(kw, **events(B, 4, 3, drop=False), fault_tick0=40)
    full = S.closed_loop(x0, xref, keys, T6, **kf)
    a = S.closed_loop(x0, xref, keys, 3, **kf)
    b = S.closed_loop(a[0][:, -1], xref, a[5], 3, **dict(kf, u_init=a[3], stepsize_in=a[4], u_act_in=a[6], fault_keys=a[-2], fault_state_in=a[-1], fault_tick0=43))
    assert bits_differ(np.concatenate([a[-3], b[-3]], axis=1), full[-3]) == 0 and np.array_equal(b[-2], full[-2]) and np.array_equal(b[-1], full[-1])
    first = full[-1][:, :, 1]
    assert ((first == -1) | ((first >= 40) & (first < 46))).all() and (first >= 43).any()             # an onset whose `first` is formed from the second call's tick0
    want = ref(cfg, model, x0, xref, keys, T6, **kf)
    same_values(full + (want[-1],), want)
    # both chains, a scheduled fault and scheduled flags, 2 + 4
    Ns = 3
    kb = dict(kw, **events(B, 4, 3), fault=faults_any(T6, B, 4), meas_valid=np.ascontiguousarray(VALID[:Ns, :B]))
    full = S.closed_loop(x0, xref, keys, T6, **kb)
    a = S.closed_loop(x0, xref, keys, 2, **dict(kb, fault=kb["fault"][:2], meas_valid=kb["meas_valid"][:1]))
    nxt = dict(kb, fault=kb["fault"][2:], meas_valid=kb["meas_valid"][1:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6], meas_keys=a[8], xmeas_in=a[9],
               fault_keys=a[11], fault_state_in=a[12], fault_tick0=2, drop_keys=a[14], drop_state_in=a[15])
    b = S.closed_loop(a[0][:, -1], xref, a[5], 4, **nxt)
    S.solve_status()
    finite = [0, 1, 2]
    assert bits_differ(np.concatenate([a[0], b[0][:, 1:]], axis=1)[finite], full[0][finite]) == 0
    assert bits_differ(np.concatenate([a[10], b[10]], axis=1), full[10]) == 0 and np.array_equal(np.concatenate([a[13], b[13]], axis=1), full[13])
    same_values([b[i] for i in (3, 4, 5, 6, 8, 9, 11, 12, 14, 15)], [full[i] for i in (3, 4, 5, 6, 8, 9, 11, 12, 14, 15)], eps=finite)
    same_values([b[i] for i in (11, 12, 14, 15)], [full[i] for i in (11, 12, 14, 15)])
    want = ref(cfg, model, x0, xref, keys, T6, **kb)
    same_values(full + (want[-1],), want)
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    """SDEMPC_OPT_TEST_WS_FILL = 255 (every new buffer starts as NaNs / all-ones words, the event buffer among them); another shape first, then a call without chains,
    the one with chains and no start states (healthy and valid, not what the buffer held), and the call without chains again."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 179)
    kw.update(together(model, x0, cfg.horizon, "stiff"))
    ke = dict(kw, **{k: v for k, v in events(B5, 4, 3).items() if k != "meas_keys"})
    want = ref(cfg, model, x0, xref, keys, T5, **ke)
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    k2 = {k: (v[:2] if k in ("u_init", "stepsize_in") else v) for k, v in scored_episodes(cfg, B5, 179)[3].items()}
    S.closed_loop(x0[:2], xref[:, :2], keys[:2], 3, **k2, **events(2, 4, 4, states=True))       # another shape first, other thresholds, failed motors left behind
    before = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **ke)
    after = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    S.solve_status()
    same_values(got, want)
    same_values(before, after)
    same_values(before, ref(cfg, model, x0, xref, keys, T5, **kw))
    S.close()


def test_second_block_and_a_partly_empty_third():
    """B = 258 with P = 1, T = 3: three blocks of the key kernel, the last with two threads; thresholds per episode. The rows, chains and states of every episode
    against the generator, six episodes against the whole loop."""
    B, T = 258, 3
    cfg = score_cfg(num_particles=1)
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B, 180)
    kw.update(events(B, 4, 3))
    eps = [0, 3, 4, 255, 256, 257]
    want = ref(cfg, model, x0, xref, keys, T, episodes=eps, **kw)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
    S.solve_status()
    same_values(got[:-7] + got[-1:], want[:-7] + want[-1:], eps=eps)
    same_values(got[-7:-1], want[-7:-1])
    S.close()
