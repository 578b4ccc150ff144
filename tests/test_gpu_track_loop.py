"""Reference windows and score targets cut from a trajectory on the GPU (SPEC.md §11j, sdempc_closed_loop_batch_tracked and sdempc_reference_windows): everything
bit for bit. The windows the device forms against track_rows (tests/track_loop_ref.py) on every table of tests/track_cases.py, at B = 5 and at B = 258 (a partly
empty last workgroup of the row launch); every value closed_loop(track=...) returns against track_loop_ref, which is the already-verified drawn loop on the
reference's windows — every arithmetic with and without the rate loop, P = 1 and 33, three, four and six motors, the score from device-formed targets with
outputs=False, and the trajectory together with both processes, a fault, a plant switch, dropouts and an aged, renormalised measurement; the GPU against itself
(the windows it returned, fed back as an xref array); one period per chunk; continuation through track_tick0; a handle with a past and poisoned buffers; track
NULL against the drawn entry point; and the ten wrong generators of the reference, none of which may equal what the device computes. Shapes: H = 8 with step
lengths whose float32 and float64 sums differ, 3 iterations, S = 2, n = 2, T = 6, B = 5, tick0 in {0, 1000}."""
import os

import numpy as np
import pytest

from cases import CDIR, asymmetric_cfg, asymmetric_model, bits_differ
from closed_loop_ref import default_warm_start
from loop_cases import ARITH, REF_NAME
from process_cases import drawn, for_ref
from score_cases import rate_loop, rate_tail, thresholds_from, together
from score_loop_ref import score_rows, words_differ
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, SdeMpcSolver
from track_cases import B5, S2, T6, TICK0S, episodes, for_rows, params, raw_tables, tables, timing, track_cfg, tracked
from track_loop_ref import MUTANTS, track_loop_ref, track_rows, track_targets

pytestmark = pytest.mark.gpu
F = np.float32
NS3 = 3


def flight(cfg, B, seed):
    """(x0, keys, kw): initial states, keys and the timing, warm start and step sizes of closed_loop / the reference."""
    x0, _, keys = episodes(cfg, B, seed)
    u, s = default_warm_start(cfg, B)
    return x0, keys, dict(timing(), u_init=u, stepsize_in=s)


def ref(cfg, model, x0, keys, T, kw, episodes=None):
    """(the reference's values with xsub last, its windows [Ns][B][H+1][13], its targets [T][B][13]) for closed_loop's keyword arguments."""
    k = {REF_NAME.get(a, a): v for a, v in for_ref(kw, x0.shape[0]).items()}
    tb = [(t.t, t.x, t.period) for t in k.pop("track")]
    return track_loop_ref(cfg, model, k.pop("plants", None), x0, tb, keys, T, episodes=episodes, substep_states=True, **k)


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


def run_both(cfg, model, x0, keys, T, kw, options=None):
    want, xref, g = ref(cfg, model, x0, keys, T, kw)
    S = SdeMpcSolver(cfg, model, max_batch=x0.shape[0], options=options)
    got = S.closed_loop(x0, None, keys, T, substep_states=True, **kw)
    S.solve_status()
    return S, got, want, xref, g


@pytest.mark.parametrize("B", [5, 258])
def test_reference_windows_on_every_table(B):
    """The direct handle on the device code: every table under every kind of episode (the four shifts at B = 5), both tick0 values, with and without the
    renormalisation, and the NULL defaults. B = 258: 2322 rows, nine full workgroups of the row launch and one with 18 threads."""
    cfg = track_cfg()
    ts = np.asarray(cfg.time_steps)
    S = SdeMpcSolver(cfg, synthetic_iris(), max_batch=B)
    tb, tr = raw_tables(), tables()
    for shift in (range(4) if B == 5 else (1,)):
        of, ph, rt, off = params(B, shift)
        for tick0, ticks, renorm in ((0, [0, 2, 4], True), (1000, [0, 3], shift != 2)) if B == 5 else ((1000, [1, 2], True),):
            got = S.reference_windows(tr, ticks, B, track_of=of, track_phase=ph, track_rate=rt, track_offset=off, track_tick0=tick0, track_renorm=renorm)
            want = track_rows(tb, ts, [tick0 + k for k in ticks], B, of, ph, rt, off, renorm)
            assert got.shape == want.shape == (len(ticks), B, cfg.horizon + 1, 13)
            assert bits_differ(got, want) == 0, (shift, tick0, bits_differ(got, want))
    for i in range(4):                      # one table, nothing per episode: table 0, phase 0, rate 1, no offset
        got = S.reference_windows(tr[i], [7], B)
        assert bits_differ(got, track_rows(tb[i:i + 1], ts, [7], B)) == 0, i
    S.close()


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_every_arithmetic(mlp_dtype, math_mode, rate):
    """The five episodes of track_cases.py, tick0 = 1000: every returned value against the reference."""
    cfg = track_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 191)
    if rate:
        kw.update(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B5, cfg.horizon))
    kw.update(tracked(B5, tick0=1000))
    S, got, want, xref, g = run_both(cfg, model, x0, keys, T6, kw)
    same_values(got, want)
    assert got[2].shape == (B5, NS3, 8) and len(got) == (11 if rate else 8)
    S.close()


@pytest.mark.parametrize("P", [1, 33])
def test_particle_counts(P):
    cfg = track_cfg(num_particles=P)
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 192)
    kw.update(tracked(B5, shift=1))
    S, got, want, xref, g = run_both(cfg, model, x0, keys, T6, kw)
    print("solve kernel:", S.last_kernel_name())
    same_values(got, want)
    S.close()


@pytest.mark.parametrize("vehicle", ["iris", "hexa", "asymmetric3"])
def test_motor_counts(vehicle):
    B = 3
    small = dict(horizon=8, num_short_dt=3, short_step_dt=0.05, long_step_dt=0.07, num_particles=33, max_iter=3, max_no_improvement_iter=3)
    if vehicle == "iris":
        cfg, model = track_cfg(), synthetic_iris()
    elif vehicle == "hexa":
        cfg, model = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(**small), synthetic_hexa()
    else:
        cfg, model = asymmetric_cfg(3, **small), asymmetric_model(3)
    x0, keys, kw = flight(cfg, B, 193)
    kw.update(tracked(B, shift=2, tick0=1000))
    S, got, want, xref, g = run_both(cfg, model, x0, keys, T6, kw)
    same_values(got, want)
    assert got[1].shape == (B, T6, cfg.num_motors)
    S.close()


def test_score_from_device_formed_targets_and_outputs_false():
    """score_ref="track": the score words against score_rows on the reference's rows and the reference's targets, tick and substep scores; outputs=False leaves the
    score and the continuation values as they are, None in the row positions."""
    cfg = track_cfg()
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 194)
    kw.update(tracked(B5, tick0=1000))
    want, xref, g = ref(cfg, model, x0, keys, T6, kw)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    for substeps in (False, True):
        score = thresholds_from(want[0], want[-1], g, finite=range(B5), substeps=substeps)
        got = S.closed_loop(x0, None, keys, T6, substep_states=True, score=score, score_ref="track", **kw)
        S.solve_status()
        same_values(got[:-2] + got[-1:], want)
        z = score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), score.substeps, S2)
        assert got[-2].dtype == SCORE_DTYPE and words_differ(got[-2], z) == 0
        assert len(set(got[-2]["first_fail_row"])) > 1                               # the thresholds sit inside the spread: some episodes fail, some do not
        bare = S.closed_loop(x0, None, keys, T6, substep_states=True, score=score, score_ref="track", outputs=False, **kw)
        S.solve_status()
        rows = {0, 1, 2, len(got) - 1}
        assert {i for i, v in enumerate(bare) if v is None} == rows
        same_values([v for i, v in enumerate(bare) if i not in rows], [v for i, v in enumerate(got) if i not in rows])
    S.close()


def everything(cfg, model, x0, T, rate):
    """together() of score_cases.py — a fault, a gust schedule, a plant switch, noise, a bias schedule, dropouts, ages and renormalisation — plus both processes."""
    B = x0.shape[0]
    kw = together(model, x0, cfg.horizon, rate, T=T)
    kw.update({k: v for k, v in drawn(B).items() if k != "meas_keys"})
    return kw


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
def test_everything_together_and_the_gpu_against_itself(rate):
    """The trajectory on top of both §11i processes, a scheduled disturbance and bias, a fault, a plant switch, dropouts, an aged and renormalised measurement and a
    score from device-formed targets. Then the GPU against itself: the windows reference_windows returns for the run's solves and the targets the reference formed,
    fed back through the ARRAY route (xref [Ns][B][H+1][13], score_ref [T][B][13]), give the same run, word for word."""
    cfg = track_cfg()
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 195)
    kw.update(everything(cfg, model, x0, T6, rate))
    tk = tracked(B5, tick0=1000)
    want, xref, g = ref(cfg, model, x0, keys, T6, dict(kw, **tk))
    score = thresholds_from(want[0], want[-1], g, finite=range(B5))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, None, keys, T6, substep_states=True, score=score, score_ref="track", **kw, **tk)
    S.solve_status()
    same_values(got[:-8] + got[-7:], want)
    assert words_differ(got[-8], score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), score.substeps, S2)) == 0
    win = S.reference_windows(tk["track"], [j * S2 for j in range(NS3)], B5, **{k: v for k, v in tk.items() if k != "track"})
    assert bits_differ(win, xref) == 0
    fed = S.closed_loop(x0, win, keys, T6, substep_states=True, score=score, score_ref=g, **kw)
    S.solve_status()
    same_values(fed, got)
    S.close()


def test_null_track_is_the_drawn_entry_point(monkeypatch):
    """sdempc_closed_loop_batch_tracked with track NULL against sdempc_closed_loop_batch_drawn on every output (the array route, a disturbance process and a score)."""
    cfg = track_cfg()
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 196)
    kw.update(drawn(B5, bias=False))
    xref = episodes(cfg, B5, 196)[1]
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    first = S.closed_loop(x0, xref, keys, T6, substep_states=True, **kw)

    def through_tracked(lib):
        fn = _abi.tracked_entry(lib)                      # (resolved before the patch below: it builds its prototype from the drawn entry point's)
        return lambda h, *a: fn(h, None, *a)
    through_tracked(S.lib)
    monkeypatch.setattr(_abi, "drawn_entry", through_tracked)
    null = S.closed_loop(x0, xref, keys, T6, substep_states=True, **kw)
    S.solve_status()
    same_values(null, first)
    S.close()


def test_one_period_per_chunk_changes_no_bit():
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 0: one period per chunk — the window launch of every period and the target launch of every chunk take their ticks from the
    chunk's first tick; T = 6 and T = 5 (a ragged last period)."""
    cfg = track_cfg()
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 197)
    kw.update(tracked(B5, tick0=1000))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    for T in (T6, 5):
        want, xref, g = ref(cfg, model, x0, keys, T, kw)
        score = thresholds_from(want[0], want[-1], g, finite=range(B5), substeps=True)
        whole = S.closed_loop(x0, None, keys, T, substep_states=True, score=score, score_ref="track", **kw)
        S.set_option("test_loop_chunk_bytes", 0)
        cut = S.closed_loop(x0, None, keys, T, substep_states=True, score=score, score_ref="track", **kw)
        S.set_option("test_loop_chunk_bytes", -1)
        S.solve_status()
        same_values(whole[:-2] + whole[-1:], want)
        assert words_differ(whole[-2], score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), score.substeps, S2)) == 0
        same_values(cut, whole)
    S.close()


@pytest.mark.parametrize("cut", [2, 4])
def test_continuation_through_track_tick0(cut):
    """T = 2 + 4 and 4 + 2 (whole periods): the second call at track_tick0 + cut with the first call's continuation values is the joined run, the score included."""
    cfg = track_cfg()
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 198)
    kw.update(tracked(B5, tick0=1000))
    want, xref, g = ref(cfg, model, x0, keys, T6, kw)
    score = thresholds_from(want[0], want[-1], g, finite=range(B5))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    sc = dict(score=score, score_ref="track")
    full = S.closed_loop(x0, None, keys, T6, **kw, **sc)
    a = S.closed_loop(x0, None, keys, cut, **kw, **sc)
    b = S.closed_loop(a[0][:, -1], None, a[5], T6 - cut, **dict(kw, u_init=a[3], stepsize_in=a[4], u_act_in=a[6], track_tick0=1000 + cut), **sc, score_in=a[7])
    S.solve_status()
    same_values(full[:7], want[:7])
    assert bits_differ(np.concatenate([a[0], b[0][:, 1:]], axis=1), full[0]) == 0
    for i in (1, 2):
        assert bits_differ(np.concatenate([a[i], b[i]], axis=1), full[i]) == 0, i
    same_values(b[3:], full[3:])
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    """SDEMPC_OPT_TEST_WS_FILL = 255 (every new buffer starts as NaNs, the trajectory buffer among them); another shape and another set first, then an array call, the
    tracked one, and the array call again."""
    cfg = track_cfg()
    model = synthetic_iris()
    x0, keys, kw = flight(cfg, B5, 199)
    tk = tracked(B5, tick0=1000)
    want, xref, g = ref(cfg, model, x0, keys, T6, dict(kw, **tk))
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    k2 = {k: (v[:2] if k in ("u_init", "stepsize_in") else v) for k, v in kw.items()}
    S.closed_loop(x0[:2], None, keys[:2], 3, **k2, track=tables()[1])               # another shape and a smaller set first
    before = S.closed_loop(x0, xref, keys, T6, substep_states=True, **kw)
    got = S.closed_loop(x0, None, keys, T6, substep_states=True, **kw, **tk)
    after = S.closed_loop(x0, xref, keys, T6, substep_states=True, **kw)
    S.solve_status()
    same_values(got, want)
    same_values(before, after)
    same_values(before, want)                                                        # (the array route on the reference's windows is the same run)
    S.close()


def test_no_wrong_generator_equals_the_device():
    """The ten mutants of the reference on the inputs of tests/test_track_loop_cpu.py: each differs from the windows the device returned or — the targets come back
    through the score only — from the score words the device formed (which equal the right ones), at tick0 = 0 or 1000."""
    cfg = track_cfg()
    model = synthetic_iris()
    ts = np.asarray(cfg.time_steps)
    tb = raw_tables()
    x0, keys, kw = flight(cfg, B5, 200)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    dev = {}
    for tick0 in TICK0S:
        tk = tracked(B5, tick0=tick0)
        par = for_rows(tk)
        solves, ticks = [tick0 + j * S2 for j in range(NS3)], [tick0 + k for k in range(T6)]
        win = S.reference_windows(tk["track"], [j * S2 for j in range(NS3)], B5, **{k: v for k, v in tk.items() if k != "track"})
        g = track_targets(tb, ts, ticks, B5, **par)
        assert bits_differ(win, track_rows(tb, ts, solves, B5, **par)) == 0
        plain = S.closed_loop(x0, None, keys, T6, substep_states=True, **kw, **tk)
        score = thresholds_from(plain[0], plain[-1], g, finite=range(B5))
        got = S.closed_loop(x0, None, keys, T6, substep_states=True, score=score, score_ref="track", **kw, **tk)
        S.solve_status()
        words = lambda tg: score_rows(got[0], got[1], got[2], got[-1], tg, cfg, score.thresholds(), score.substeps, S2)      # noqa: E731
        assert words_differ(got[-2], words(g)) == 0
        dev[tick0] = (par, solves, ticks, win, got[-2], words)
    for mutant in MUTANTS:
        d = 0
        for tick0 in TICK0S:
            par, solves, ticks, win, z, words = dev[tick0]
            d += bits_differ(track_rows(tb, ts, solves, B5, mutant=mutant, **par), win)
            d += words_differ(words(track_targets(tb, ts, ticks, B5, mutant=mutant, **par)), z)
        assert d > 0, mutant
    S.close()
