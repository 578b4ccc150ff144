"""Gusts and estimator bias drawn on the GPU (SPEC.md §11i, sdempc_closed_loop_batch_drawn): every returned value bit for bit (keys as integers) against
process_loop_ref (tests/process_loop_ref.py), which is the already-verified aged loop on the rows of the reference generator. Shapes of tests/score_cases.py and
tests/obs_cases.py, the smallest at which this path can go wrong: H = 6 with two step lengths, 3 iterations, S = 2, n = 2, T = 5 (a ragged last period) and T = 6,
B = 3 to 5; every arithmetic with and without the rate loop; P = 1 and 33; three, four and six motors; each process alone and both together with a scheduled
disturbance and bias, a fault, a plant switch, dropouts, an aged and renormalised measurement and a score; coefficients shared and per episode; the GPU against
itself (the rows the call returned, fed back as disturbance and meas_bias, give the same run); one period per chunk; continuation through the *_next values;
a handle with a past and poisoned buffers; B = 258 (the key kernel's second block and a partly empty third); outputs=False; both cfgs NULL against the scored entry
point; and the six wrong generators of the reference, none of which may equal what the device computes."""
import os

import numpy as np
import pytest

import loop_cases
from cases import CDIR, asymmetric_cfg, asymmetric_model, bits_differ
from loop_cases import ARITH
from process_cases import (B5, S2, T5, T6, VALID, W_BIAS, W_DIST, bias_rows, disturbance, drawn, for_ref, score_cfg, scored_episodes, targets, thresholds_from,
                           together)
from process_loop_ref import MUTANTS, ROW_MUTANTS, process_loop_ref, process_rows
from score_loop_ref import score_rows, words_differ
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, SdeMpcSolver

pytestmark = pytest.mark.gpu
F = np.float32


def ref(cfg, model, x0, xref, keys, T, episodes=None, **kw):
    """The reference loop for closed_loop's keyword arguments, xsub always last."""
    return loop_cases.ref(process_loop_ref, cfg, model, x0, xref, keys, T, episodes=episodes, substep_states=True, **for_ref(kw, x0.shape[0]))


def same_values(got, want, eps=None):
    """Two returned tuples agree in shape and in every bit, the keys as integers, None with None; eps: compare these episodes only."""
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
    """The five episodes of score_cases.py under both processes, coefficients per episode, stationary start states."""
    cfg = score_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 171)
    if rate:
        from score_cases import rate_loop, rate_tail
        kw.update(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B5, cfg.horizon))
    kw.update(drawn(B5))
    S, got, want = run_both(cfg, model, x0, xref, keys, T5, kw)
    same_values(got, want)
    assert got[-7].shape == (B5, T5, W_DIST) and got[-4].shape == (B5, 3, W_BIAS) and got[-7].any() and got[-4].any()
    S.close()


@pytest.mark.parametrize("P", [1, 33])
def test_particle_counts(P):
    B = 3
    cfg = score_cfg(num_particles=P)
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B, 172)
    kw.update(drawn(B))
    S, got, want = run_both(cfg, model, x0, xref, keys, T5, kw)
    print("solve kernel:", S.last_kernel_name())
    same_values(got, want)
    S.close()


@pytest.mark.parametrize("vehicle", ["iris", "hexa", "asymmetric3"])
def test_motor_counts(vehicle):
    B = 3
    small = dict(horizon=6, num_short_dt=4, short_step_dt=0.05, long_step_dt=0.1, num_particles=33, max_iter=3, max_no_improvement_iter=3)
    if vehicle == "iris":
        cfg, model = score_cfg(), synthetic_iris()
    elif vehicle == "hexa":
        cfg, model = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(**small), synthetic_hexa()
    else:
        cfg, model = asymmetric_cfg(3, **small), asymmetric_model(3)
    x0, xref, keys, kw = scored_episodes(cfg, B, 173)
    kw.update(drawn(B))
    S, got, want = run_both(cfg, model, x0, xref, keys, T5, kw)
    same_values(got, want)
    assert got[1].shape == (B, T5, cfg.num_motors)
    S.close()


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("which", ["dist", "bias"])
def test_each_process_alone(which, per_episode):
    """One process and nothing else of its kind: the disturbance process without an observation (a scenario run with a NULL scenario cfg), the bias process with an
    empty obs cfg; T = 5 and T = 6; start states given and absent (zeros)."""
    B = 4
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B, 174)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    for T, states in ((T5, True), (T6, False)):
        k = dict(kw, **drawn(B, dist=which == "dist", bias=which == "bias", per_episode=per_episode, states=states))
        want = ref(cfg, model, x0, xref, keys, T, **k)
        got = S.closed_loop(x0, xref, keys, T, substep_states=True, **k)
        S.solve_status()
        same_values(got, want)
        assert len(got) == (11 if which == "dist" else 14)
    S.close()


def everything(cfg, model, x0, T, rate, per_episode=True):
    """together() of score_cases.py — a fault, a gust schedule, a plant switch, noise, a bias schedule, dropouts, ages and renormalisation — plus both processes."""
    B = x0.shape[0]
    kw = together(model, x0, cfg.horizon, rate, T=T)
    kw.update({k: v for k, v in drawn(B, per_episode=per_episode).items() if k != "meas_keys"})
    return kw


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
def test_everything_together_and_the_gpu_against_itself(rate):
    """Both processes on top of a scheduled disturbance and a scheduled bias, under a fault, a plant switch, dropouts, an aged and renormalised measurement and a score.
    Then the GPU against itself: the rows the call returned, fed back as disturbance and meas_bias, give the same run in every shared value — the plant kernel reads
    device-written rows exactly as staged ones — and so do the rows of the processes alone plus the schedules, the sums formed in float32. outputs=False leaves the
    score and the continuation values as they are, None in the row positions."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 171)
    kw.update(everything(cfg, model, x0, T5, rate))
    want = ref(cfg, model, x0, xref, keys, T5, **kw)
    g = targets(xref, T5)
    score = thresholds_from(want[0], want[-1], g)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, score=score, score_ref=g, **kw)
    S.solve_status()
    z = got[-8]
    assert z.dtype == SCORE_DTYPE
    same_values(got[:-8] + got[-7:], want)
    assert words_differ(z, score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), score.substeps, S2)) == 0
    # the rows fed back
    plain = {k: v for k, v in kw.items() if not k.startswith(("dist_", "bias_"))}
    dist_rows, bias_rows_ = got[-7], got[-4]
    fed = S.closed_loop(x0, xref, keys, T5, substep_states=True, score=score, score_ref=g,
                        **dict(plain, disturbance=np.ascontiguousarray(dist_rows.transpose(1, 0, 2)), meas_bias=np.ascontiguousarray(bias_rows_.transpose(1, 0, 2))))
    same_values(fed, got[:-7] + got[-1:])
    # the processes alone (no schedules), then their rows plus the schedules
    alone = S.closed_loop(x0, xref, keys, T5, **{k: v for k, v in kw.items() if k not in ("disturbance", "meas_bias")})
    d_sum = (np.asarray(kw["disturbance"], F) + alone[-6].transpose(1, 0, 2)).astype(F)
    b_sum = (np.asarray(kw["meas_bias"], F) + alone[-3].transpose(1, 0, 2)).astype(F)
    assert bits_differ(d_sum.transpose(1, 0, 2), dist_rows) == 0 and bits_differ(b_sum.transpose(1, 0, 2), bias_rows_) == 0
    same_values(alone[-5:-3] + alone[-2:], got[-6:-4] + got[-3:-1])                  # chains and states do not depend on the schedules
    fed = S.closed_loop(x0, xref, keys, T5, substep_states=True, score=score, score_ref=g, **dict(plain, disturbance=d_sum, meas_bias=b_sum))
    same_values(fed, got[:-7] + got[-1:])
    # outputs=False
    bare = S.closed_loop(x0, xref, keys, T5, substep_states=True, score=score, score_ref=g, outputs=False, **kw)
    S.solve_status()
    rows = {0, 1, 2, 7, 10 if rate else 7, len(got) - 7, len(got) - 4, len(got) - 1}          # xs, us, info, ws, xmeas, dist_rows, bias_rows, xsub
    assert {i for i, v in enumerate(bare) if v is None} == rows
    same_values([v for i, v in enumerate(bare) if i not in rows], [v for i, v in enumerate(got) if i not in rows])
    S.close()


def test_null_cfgs_are_the_scored_entry_point(monkeypatch):
    """sdempc_closed_loop_batch_drawn with both process cfgs NULL against sdempc_closed_loop_batch_scored on every output."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 176)
    kw.update(together(model, x0, cfg.horizon, "stiff"))
    g = targets(xref, T5)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    plain = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    score = thresholds_from(plain[0], plain[-1], g, substeps=True)
    scored = S.closed_loop(x0, xref, keys, T5, substep_states=True, score=score, score_ref=g, **kw)

    def through_drawn(lib):
        fn = _abi.drawn_entry(lib)                        # (resolved before the patch below: it builds its prototype from the scored entry point's)
        return lambda h, *a: fn(h, None, None, *a, None, None, None, None, None, None)
    through_drawn(S.lib)
    monkeypatch.setattr(_abi, "scored_entry", through_drawn)
    null = S.closed_loop(x0, xref, keys, T5, substep_states=True, score=score, score_ref=g, **kw)
    S.solve_status()
    same_values(null, scored)
    same_values(null[:-2] + null[-1:], plain)
    S.close()


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
def test_one_period_per_chunk_changes_no_bit(rate):
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 0: one period per chunk — the process rows of every period start the chunk's region anew, the chains and states carry over in
    the handle's buffer; T = 5 and T = 6; coefficients shared."""
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


def test_continuation_through_the_next_values():
    """The disturbance process alone at T = 3 + 3 (the cut inside a solve period: its chain advances per tick, so any T continues — the solver's own values continue
    only at period ends, so the joined run is compared in the process values); both processes at T = 2 + 4 (whole periods) in every value of the joined run."""
    cfg = score_cfg()
    model = synthetic_iris()
    B = 4
    x0, xref, keys, kw = scored_episodes(cfg, B, 178)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    kd = dict(kw, **drawn(B, bias=False))
    full = S.closed_loop(x0, xref, keys, T6, **kd)
    a = S.closed_loop(x0, xref, keys, 3, **kd)
    b = S.closed_loop(a[0][:, -1], xref, a[5], 3, **dict(kd, u_init=a[3], stepsize_in=a[4], u_act_in=a[6], dist_keys=a[-2], dist_state_in=a[-1]))
    assert bits_differ(np.concatenate([a[-3], b[-3]], axis=1), full[-3]) == 0 and np.array_equal(b[-2], full[-2]) and bits_differ(b[-1], full[-1]) == 0
    want = ref(cfg, model, x0, xref, keys, T6, **kd)
    same_values(full + (want[-1],), want)
    # both processes, a scheduled disturbance and dropouts, 2 + 4
    Ns = 3
    kb = dict(kw, **drawn(B), disturbance=disturbance(T6, B), meas_valid=np.ascontiguousarray(VALID[:Ns, :B]))
    full = S.closed_loop(x0, xref, keys, T6, **kb)
    a = S.closed_loop(x0, xref, keys, 2, **dict(kb, disturbance=kb["disturbance"][:2], meas_valid=kb["meas_valid"][:1]))
    nxt = dict(kb, disturbance=kb["disturbance"][2:], meas_valid=kb["meas_valid"][1:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6], meas_keys=a[8], xmeas_in=a[9],
               dist_keys=a[11], dist_state_in=a[12], bias_keys=a[14], bias_state_in=a[15])
    b = S.closed_loop(a[0][:, -1], xref, a[5], 4, **nxt)
    S.solve_status()
    finite = [0, 1, 2]
    assert bits_differ(np.concatenate([a[0], b[0][:, 1:]], axis=1)[finite], full[0][finite]) == 0
    for i in (10, 13):
        assert bits_differ(np.concatenate([a[i], b[i]], axis=1), full[i]) == 0, i
    same_values([b[i] for i in (3, 4, 5, 6, 8, 9, 11, 12, 14, 15)], [full[i] for i in (3, 4, 5, 6, 8, 9, 11, 12, 14, 15)], eps=finite)
    want = ref(cfg, model, x0, xref, keys, T6, **kb)
    same_values(full + (want[-1],), want)
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    """SDEMPC_OPT_TEST_WS_FILL = 255 (every new buffer starts as NaNs, the process buffer among them); another shape first, then a call without processes, the drawn one
    without start states (zeros, not what the buffer held), and the call without processes again."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 179)
    kw.update(together(model, x0, cfg.horizon, "stiff"))
    kd = dict(kw, **{k: v for k, v in drawn(B5, states=False).items() if k != "meas_keys"})
    want = ref(cfg, model, x0, xref, keys, T5, **kd)
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    k2 = {k: (v[:2] if k in ("u_init", "stepsize_in") else v) for k, v in scored_episodes(cfg, B5, 179)[3].items()}
    S.closed_loop(x0[:2], xref[:, :2], keys[:2], 3, **k2, **drawn(2))               # another shape first
    before = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kd)
    after = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    S.solve_status()
    same_values(got, want)
    same_values(before, after)
    same_values(before, loop_cases.ref(process_loop_ref, cfg, model, x0, xref, keys, T5, substep_states=True, **kw))
    S.close()


def test_second_block_and_a_partly_empty_third():
    """B = 258 with P = 1, T = 3: three blocks of the key kernel, the last with two threads. The rows, chains and states of every episode against the generator, six
    episodes against the whole loop."""
    B, T = 258, 3
    cfg = score_cfg(num_particles=1)
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B, 180)
    kw.update(drawn(B))
    eps = [0, 3, 4, 255, 256, 257]
    want = ref(cfg, model, x0, xref, keys, T, episodes=eps, **kw)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
    S.solve_status()
    same_values(got[:-7] + got[-1:], want[:-7] + want[-1:], eps=eps)
    same_values(got[-7:-1], want[-7:-1])
    S.close()


def test_no_wrong_generator_equals_the_device():
    """The six mutants of the reference on the inputs of tests/test_process_loop_cpu.py: each differs from the rows, chains or states the device returned (which equal
    the right ones)."""
    cfg = score_cfg()
    model = synthetic_iris()
    B, T, Ns = B5, T6, 3
    x0, xref, keys, kw = scored_episodes(cfg, B, 181)
    valid = np.ascontiguousarray(VALID[:Ns, :B])
    kw = dict(kw, disturbance=disturbance(T, B), meas_bias=bias_rows(Ns, B), meas_valid=valid, **drawn(B))
    S, got, want = run_both(cfg, model, x0, xref, keys, T, kw)
    same_values(got, want)
    fk = for_ref(kw, B)
    for mutant in MUTANTS:
        rm = mutant if mutant in ROW_MUTANTS else None
        step6 = np.repeat((np.arange(T) % S2 == 0)[:, None], B, axis=1) if mutant == "dist_per_solve" else None
        step12 = (valid != 0) if mutant == "bias_held_on_dropout" else None
        r6 = process_rows(kw["dist_keys"], *fk["dist_process"], kw["dist_state_in"], T, 6, scheduled=kw["disturbance"], mutant=rm, step=step6)
        r12 = process_rows(kw["bias_keys"], *fk["bias_process"], kw["bias_state_in"], Ns, 12, scheduled=kw["meas_bias"], mutant=rm, step=step12)
        d6 = bits_differ(r6[0], got[-7]) + int((r6[1] != got[-6]).sum()) + bits_differ(r6[2], got[-5])
        d12 = bits_differ(r12[0], got[-4]) + int((r12[1] != got[-3]).sum()) + bits_differ(r12[2], got[-2])
        if mutant != "bias_held_on_dropout":
            assert d6 > 0, mutant
        if mutant != "dist_per_solve":
            assert d12 > 0, mutant
    S.close()
