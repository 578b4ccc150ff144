"""The geometric baseline controller on the GPU (SPEC.md §11l, sdempc_geo_command_batch and sdempc_closed_loop_batch_baseline): every returned value bit for bit
against the reference — geo_ref.geo_commands for the stand-alone call, geo_loop_ref (the existing reference chain with the controller's oracle replaced) for the
loop. Shapes of tests/geo_cases.py, the smallest at which this path can go wrong: B = 257 for the stand-alone call (one thread past a 256-thread block), one
parameter set and one per episode; loops at H = 6, P = 1, B = 5, T = 6 over n in {1, 3}, S in {1, 2}, D in {0, 2} and m in {3, 4, 6}; then each variant of the loop
once: every plant arithmetic, a measured and aged estimate, track= windows, a gust process with a fault process and a score (and outputs=False), a chunk boundary,
continuation; an MPC call before and after a baseline call on one handle; and MpcProblem.simulate(controller=)."""
import numpy as np
import pytest

import geo_cases as G
from cases import asymmetric_model, bits_differ
from event_cases import events, for_ref
from event_loop_ref import event_loop_ref
from geo_loop_ref import geo_loop_ref
from geo_ref import geo_commands
from loop_cases import ARITH, REF_NAME
from process_cases import drawn
from score_loop_ref import score_rows, words_differ
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, Score, SdeMpcSolver

pytestmark = pytest.mark.gpu
F = np.float32


def same_values(got, want, eps=None):
    """Two returned tuples agree in shape and in every bit, the keys and states as integers, None with None."""
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


def ref(cfg, model, ctl, x0, xref, keys, T, **kw):
    """The reference loop flown by the controller, for closed_loop's keyword arguments; xsub always last."""
    B = x0.shape[0]
    par, _ = G.params(ctl, cfg, B)
    kwr = {REF_NAME.get(k, k): v for k, v in for_ref(kw, B, cfg.num_motors).items()}
    kwr.setdefault("plants", None)
    return geo_loop_ref(event_loop_ref, par, cfg, model, x0, accel_ff=ctl.accel_ff, ref_row=ctl.ref_row, xref=xref, keys=keys, T=T, substep_states=True, **kwr)


@pytest.mark.parametrize("per_episode", [False, True], ids=["one_set", "per_episode"])
@pytest.mark.parametrize("m", G.MOTORS)
def test_command_bit_for_bit(m, per_episode):
    cfg, model = G.geo_cfg(m), asymmetric_model(m)
    S = SdeMpcSolver(cfg, model, max_batch=G.B257)
    for ff, row in ((False, 0), (True, 2)):
        ctl = G.controller(model, G.B257 if per_episode else None, ff, row)
        par, inv_dt = G.params(ctl, cfg, G.B257)
        x, xref = G.states(cfg, model, ctl, G.B257)
        want = geo_commands(x, xref, par, ff, row, inv_dt)
        got = S.geo_command(x, xref, ctl)
        assert got.shape == (G.B257, 4) and bits_differ(got, want) == 0, bits_differ(got, want)
        one = S.geo_command(x, xref[3], ctl)                                   # one window for every state
        assert bits_differ(one, geo_commands(x, xref[3:4], par, ff, row, inv_dt)) == 0
    S.close()


@pytest.mark.parametrize("i", range(len(G.SHAPES)))
def test_loop_shapes(i):
    """All ten rate-route outputs and the substep states; the motor count, the feed-forward and the parameter sets change with the shape."""
    n, Sp, D = G.SHAPES[i]
    m = G.MOTORS[i % 3]
    cfg, model = G.geo_cfg(m), asymmetric_model(m)
    ctl = G.controller(model, G.B5 if i % 2 else None, accel_ff=i in (1, 2, 4), ref_row=(0, 1, 0, 5, 2)[i])
    x0, xref, keys = G.episodes(cfg, model, ctl)
    kw = dict(G.timing(n, Sp, D), rate_loop=G.rate_loop())
    want = ref(cfg, model, ctl, x0, xref, keys, G.T6, **kw)
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    got = S.closed_loop(x0, xref, keys, G.T6, substep_states=True, controller=ctl, **kw)
    assert len(got) == 11
    same_values(got, want)
    Ns = -(-G.T6 // Sp)
    assert got[2].shape == (G.B5, Ns, 8) and (got[2][:, :, [0, 2, 3, 4, 5, 6, 7]] == 0).all() and (got[2][:, :, 1] == got[4][:, None]).all()
    assert (got[3] == got[3][:, :, :1]).all()                                 # u_next holds thrust rows
    assert np.isfinite(got[0]).all()
    S.close()


SMALL = (2, 2, 1)            # n, S, D: the smallest timing with a solve period and an age of up to four substeps


@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_every_plant_arithmetic(mlp_dtype, math_mode):
    cfg, model = G.geo_cfg(4), asymmetric_model(4)
    ctl = G.controller(model)
    x0, xref, keys = G.episodes(cfg, model, ctl)
    kw = dict(G.timing(*SMALL), rate_loop=G.rate_loop(), plant=model, plant_mlp_dtype=mlp_dtype, plant_math_mode=math_mode)
    want = ref(cfg, model, ctl, x0, xref, keys, G.T6, **kw)
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    same_values(S.closed_loop(x0, xref, keys, G.T6, substep_states=True, controller=ctl, **kw), want)
    S.close()


def test_from_a_measured_and_aged_estimate():
    from age_cases import AM4, aging, history
    from obs_cases import held, observation
    cfg, model = G.geo_cfg(6), asymmetric_model(6)
    ctl = G.controller(model, G.B5)
    x0, xref, keys = G.episodes(cfg, model, ctl)
    kw = dict(G.timing(*SMALL), rate_loop=G.rate_loop(), xmeas_in=held(G.B5), **observation(3, G.B5), **aging(AM4, 3, G.B5, renorm=True), xhist_in=history(x0, AM4))
    want = ref(cfg, model, ctl, x0, xref, keys, G.T6, **kw)
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    got = S.closed_loop(x0, xref, keys, G.T6, substep_states=True, controller=ctl, **kw)
    same_values(got, want)
    assert bits_differ(got[10][:, 0], x0) > 0                                  # the commands were formed from the estimate, not from the plant state
    S.close()


def test_with_track_windows():
    from track_cases import for_rows, tracked
    from track_loop_ref import track_rows
    cfg, model = G.geo_cfg(3), asymmetric_model(3)
    ctl = G.controller(model, accel_ff=True, ref_row=1)
    x0, _, keys = G.episodes(cfg, model, ctl)
    tr = tracked(G.B5, tick0=1000)
    tb = [(t.t, t.x, t.period) for t in tr["track"]]
    windows = track_rows(tb, np.asarray(cfg.time_steps), [1000 + j * 2 for j in range(3)], G.B5, **for_rows(tr))
    kw = dict(G.timing(*SMALL), rate_loop=G.rate_loop())
    want = ref(cfg, model, ctl, x0, windows, keys, G.T6, **kw)
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    same_values(S.closed_loop(x0, None, keys, G.T6, substep_states=True, controller=ctl, **kw, **tr), want)
    S.close()


def test_gusts_faults_score_and_no_outputs():
    cfg, model = G.geo_cfg(4), asymmetric_model(4)
    ctl = G.controller(model)
    x0, xref, keys = G.episodes(cfg, model, ctl)
    kw = dict(G.timing(*SMALL), rate_loop=G.rate_loop(), **drawn(G.B5, bias=False), **events(G.B5, 4, 3, drop=False))
    want = ref(cfg, model, ctl, x0, xref, keys, G.T6, **kw)
    g = np.ascontiguousarray(xref[0][:, 0][None])                              # [1][B][13]: each episode's first reference row
    score = Score(pos_radius=1.0, tilt_max=np.deg2rad(40.0), rate_max=8.0, substeps=True)
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    got = S.closed_loop(x0, xref, keys, G.T6, substep_states=True, controller=ctl, score=score, score_ref=g, **kw)
    z = got[10]
    assert z.dtype == SCORE_DTYPE
    same_values(got[:10] + got[11:], want)
    assert words_differ(z, score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), score.substeps, SMALL[1])) == 0
    assert (z["sum_steps"] == 0).all() and (z["first_fail_row"] != 0xFFFFFFFF).any() and (z["first_fail_row"] == 0xFFFFFFFF).any()
    bare = S.closed_loop(x0, xref, keys, G.T6, substep_states=True, controller=ctl, score=score, score_ref=g, outputs=False, **kw)
    rows = {0, 1, 2, 7, 11, 14, len(got) - 1}                                  # xs, us, info, ws, dist_rows, fault_rows, xsub
    assert all(bare[j] is None for j in rows)
    same_values([v for j, v in enumerate(bare) if j not in rows], [v for j, v in enumerate(got) if j not in rows])
    S.close()


def test_chunk_boundary_and_continuation():
    """One period per chunk changes no bit; T = 2 + 4 (whole periods) continues the run in every value."""
    cfg, model = G.geo_cfg(6), asymmetric_model(6)
    ctl = G.controller(model, G.B5, accel_ff=True)
    x0, xref, keys = G.episodes(cfg, model, ctl)
    kw = dict(G.timing(*SMALL), rate_loop=G.rate_loop())
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    whole = S.closed_loop(x0, xref, keys, G.T6, substep_states=True, controller=ctl, **kw)
    same_values(whole, ref(cfg, model, ctl, x0, xref, keys, G.T6, **kw))
    S.set_option("test_loop_chunk_bytes", 0)
    cut = S.closed_loop(x0, xref, keys, G.T6, substep_states=True, controller=ctl, **kw)
    S.set_option("test_loop_chunk_bytes", -1)
    same_values(cut, whole)
    a = S.closed_loop(x0, xref, keys, 2, controller=ctl, **kw)
    b = S.closed_loop(a[0][:, -1], xref, a[5], 4, u_init=a[3], stepsize_in=a[4], u_act_in=a[6], rate_integ_in=a[8], rate_tail_in=a[9], controller=ctl, **kw)
    assert bits_differ(np.concatenate([a[0], b[0][:, 1:]], axis=1), whole[0]) == 0 and bits_differ(np.concatenate([a[1], b[1]], axis=1), whole[1]) == 0
    same_values(b[3:7] + b[8:10], whole[3:7] + whole[8:10])
    S.close()


def test_the_mpc_is_untouched_by_a_baseline_call_on_the_same_handle():
    """MPC closed_loop, baseline closed_loop, plain solve, MPC closed_loop again on one handle: the two MPC results and two plain solves agree in every bit."""
    from sde4mbrl_px4_amd import workload as W
    cfg, model = G.geo_cfg(4, num_particles=33), asymmetric_model(4)
    ctl = G.controller(model)
    x0, xref, keys = G.episodes(cfg, model, ctl)
    kw = dict(G.timing(*SMALL), rate_loop=G.rate_loop())
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    noise = W.make_noise(G.B5, 33, cfg.horizon, 3)
    u0 = np.tile(np.asarray(cfg.uref, F), (G.B5, cfg.horizon, 1))
    step = np.full(G.B5, 0.01, F)
    before = S.closed_loop(x0, xref, keys, G.T6, **kw)
    solved = S.solve(x0, xref[0], noise, u0, step)
    base = S.closed_loop(x0, xref, keys, G.T6, controller=ctl, **kw)
    between = S.solve(x0, xref[0], noise, u0, step)
    after = S.closed_loop(x0, xref, keys, G.T6, **kw)
    same_values(after, before)
    same_values(between, solved)
    assert bits_differ(base[0], before[0]) > 0 and (base[2][:, :, 2] == 0).all()
    assert np.array_equal(base[5], before[5])                                  # the main key chain advances exactly as with a solve
    S.close()


def test_simulate_passes_one_episode_through():
    """MpcProblem.simulate(controller=, rate_loop=) is closed_loop of one episode (convert_to_enu off: the same frame on both sides)."""
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    cfg, model = G.geo_cfg(4), asymmetric_model(4)
    ctl = G.controller(model)
    x0, xref, keys = G.episodes(cfg, model, ctl, B=1)
    kw = dict(G.timing(*SMALL), rate_loop=G.rate_loop())
    prob = MpcProblem(cfg=cfg, model=model, convert_to_enu=False)
    xs, us, info, st, key = prob.simulate(x0[0], keys[0], G.T6, xdes=xref[0, 0, 0], controller=ctl, **{k: v for k, v in kw.items() if k != "plant_substeps"},
                                          plant=model, plant_substeps=SMALL[0])
    hold = np.tile(xref[0, 0, 0], (cfg.horizon + 1, 1))
    want = prob.solver().closed_loop(x0, hold, keys, G.T6, controller=ctl, plant=model, **kw)
    assert bits_differ(xs, want[0][0]) == 0 and bits_differ(us, want[1][0]) == 0 and bits_differ(info, want[2][0]) == 0 and np.array_equal(key, want[5][0])
    assert bits_differ(np.asarray(st.yk, F), want[3][0]) == 0 and (info[:, 2] == 0).all()
    with pytest.raises(ValueError, match="rate_loop"):
        prob.simulate(x0[0], keys[0], G.T6, xdes=xref[0, 0, 0], controller=ctl)
