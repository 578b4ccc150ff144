"""Batched closed loop from an aged, renormalised state estimate on the GPU (SPEC.md §11g, sdempc_closed_loop_batch_aged): bit for bit against the CPU reference
of tests/age_loop_ref.py on all outputs — xs, us, info, the continuation values, ws with a rate loop, xmeas, the observation chain, the held measurement,
xhist_next and xsub. Shapes of tests/age_cases.py, the smallest at which this path can go wrong: H = 8 with two step lengths, 3 iterations, S = 2, n = 2,
D = 1, T = 5 (the last period partial: the history then keeps rows of its own) and T = 6, B = 3 to 5 (a partly empty last workgroup); age_max 1, 3 and
4 = S n (the oldest row is then the plant state before the launch) and S = n = age_max = 1; ages that hit 0 and age_max in one run, per solve and episode,
shared and constant; with and without renormalisation; every arithmetic; P = 1, 32, 33 and 70; three, four and six motors; with and without a rate loop, on
top of a gust, a dead motor, a plant switch and dropouts; one period per chunk (every solve's history then comes from the previous chunk), continuation
through xhist_next, a handle with a past and poisoned buffers; all ages zero and the C entry point with `age_cfg` NULL against the observed entry point; and
the five wrong loops of the reference, none of which may equal what the device computes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loop_cases
from age_cases import (AM4, B5, NS3, S2, T5, T6, aged_case, aging, bias_rows, dead_motor, disturbance, episodes, full_case, history, meas_keys, motor_state,
                       noise_rows, obs_cfg, observation, perturbed_plants, plant_switch, rate_loop, rate_tail, timing)
from age_loop_ref import MUTANTS, age_loop_ref
from cases import CDIR, asymmetric_cfg, asymmetric_model, bits_differ
from loop_cases import ARITH, NAMES
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu

ref = functools.partial(loop_cases.ref, age_loop_ref)
OBS = ("xmeas", "meas_keys_next", "xmeas_next")


def names(rate, hist=True, xsub=True):
    return NAMES[:10 if rate else 7] + OBS + (("xhist_next",) if hist else ()) + (("xsub",) if xsub else ())


def same(got, want, rate, hist=True, xsub=True, eps=None):
    for n, g, w in zip(names(rate, hist, xsub), got, want):
        if n == "meas_keys_next":
            assert np.array_equal(g if eps is None else g[eps], w if eps is None else w[eps]), n
    loop_cases.same(got, want, eps=eps, names=names(rate, hist, xsub))


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_every_arithmetic(mlp_dtype, math_mode, rate):
    """Ages from 0 to age_max = S n, a history, renormalisation, a dead motor, a gust, a plant switch, noise, bias and dropouts in one run. The renormalisation
    is the software rsqrt in every math_mode."""
    cfg = obs_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 131)
    kw = aged_case(model, x0, rate)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **kw), rate)
    assert np.isfinite(got[0]).all() and got[0][:, 0].tobytes() == x0.tobytes()
    assert got[-5][0, 0].tobytes() == kw["xmeas_in"][0].tobytes()                     # episode 0 drops solve 0: the held row, not renormalised
    assert got[-2].tobytes() == got[-1][:, -1 - AM4:-1].tobytes()                     # xhist_next is the tail of xsub
    S.close()


@pytest.mark.parametrize("renorm", [False, True], ids=["raw", "renorm"])
@pytest.mark.parametrize("age_max", [1, 3, AM4])
def test_history_depths_whole_and_partial_last_period(age_max, renorm):
    """age_max 1 (one row: the substep before the last), 3 (rows of this period only) and 4 = S n (the oldest row is the state before the launch); T = 6 (whole
    periods) and T = 5 (the last period has 2 substeps: at age_max 3 and 4 the history keeps rows of its own). Without xsub asked for, too."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 132)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    for T in (T6, T5):
        kw = aged_case(model, x0, "stiff", T=T, age_max=age_max, renorm=renorm)
        assert kw["meas_age"].max() == age_max and kw["meas_age"].min() == 0
        got = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
        S.solve_status()
        want = ref(cfg, model, x0, xref, keys, T, substep_states=True, **kw)
        same(got, want, "stiff")
        same(S.closed_loop(x0, xref, keys, T, **kw), want[:-1], "stiff", xsub=False)      # the substep region is internal then
    S.close()


def test_one_tick_periods_of_one_substep():
    """S = 1, n = 1, age_max = 1 = S n: every solve's only history row is the plant state before the previous launch."""
    cfg = obs_cfg()
    model = synthetic_iris()
    B, T = B5, 5
    x0, xref, keys = episodes(cfg, B, 133)
    rng = np.random.default_rng(8)
    kw = dict(timing(n=1, D=1, S=1), plant=perturbed_plants(model, 3)[1], u_act_in=motor_state(B, 4), meas_noise=noise_rows(T, B), meas_bias=bias_rows(T, B),
              meas_valid=(rng.integers(0, 4, (T, B)) != 0).astype(np.int32), meas_keys=meas_keys(B), meas_age=rng.integers(0, 2, (T, B)).astype(np.int32),
              meas_age_max=1, meas_renorm=True, xhist_in=history(x0, 1))
    assert kw["meas_age"].max() == 1 and kw["meas_age"].min() == 0
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T, substep_states=True, **kw), None)
    assert got[-2][:, 0].tobytes() == got[0][:, T - 1].tobytes()
    S.close()


@pytest.mark.parametrize("constant", [False, True], ids=["per_solve", "constant"])
@pytest.mark.parametrize("shared", [False, True], ids=["per_episode", "shared"])
def test_age_rows_shared_and_per_episode_constant_and_per_solve(shared, constant):
    """Every stride of the age table: [Ns|1][B|1]; then the short forms of the Python layer ([Ns], an int), the history defaulting to x0 and age_max to the
    largest entry."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 134)
    base = dict(timing(), plant=perturbed_plants(model, 3)[1], u_act_in=motor_state(B5, 4), **observation(NS3, B5))
    a = aging(shared=shared, constant=constant)
    assert a["meas_age"].shape == (1 if constant else NS3, 1 if shared else B5) and a["meas_age"].max() == AM4
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T5, **base, **a, xhist_in=history(x0, AM4))
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T5, **base, **a, xhist_in=history(x0, AM4)), None, xsub=False)
    # no xhist_in: the vehicle sat at x0
    got = S.closed_loop(x0, xref, keys, T5, **base, **a)
    same(got, ref(cfg, model, x0, xref, keys, T5, **base, **a), None, xsub=False)
    if shared:            # [Ns] / an int: the same table in the short forms, age_max from the largest entry
        short = dict(meas_age=int(a["meas_age"][0, 0]) if constant else a["meas_age"][:, 0])
        same(S.closed_loop(x0, xref, keys, T5, **base, **short, meas_age_max=AM4), got, None, xsub=False)
        top = int(np.max(short["meas_age"]))
        less = S.closed_loop(x0, xref, keys, T5, **base, **short)
        assert less[-1].shape == (B5, top, 13) and less[-1].tobytes() == got[-1][:, AM4 - top:].tobytes()
        same(less[:-1], got[:-1], None, hist=False, xsub=False)
    S.close()


@pytest.mark.parametrize("P", [1, 32, 33, 70])
def test_particle_counts(P):
    """P = 1 (lanes), a full group, a group and one, three groups: the solve starts from the aged measurement in every layout."""
    B = 3
    cfg = obs_cfg(num_particles=P)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B, 135)
    kw = aged_case(model, x0, "stiff")
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T5, **kw)
    S.solve_status()
    print("solve kernel:", S.last_kernel_name())
    same(got, ref(cfg, model, x0, xref, keys, T5, **kw), "stiff", xsub=False)
    S.close()


@pytest.mark.parametrize("vehicle", ["hexa", "asymmetric3"])
def test_other_motor_counts(vehicle):
    """m = 6 (the hexarotor) and m = 3 (the asymmetric model); m = 4 is every other test."""
    B = 3
    small = dict(horizon=8, num_short_dt=4, short_step_dt=0.05, long_step_dt=0.1, num_particles=33, max_iter=3, max_no_improvement_iter=3)
    if vehicle == "hexa":
        cfg = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(**small)
        model = synthetic_hexa()
        pl = perturbed_plants(model, 3)
    else:
        cfg = asymmetric_cfg(3, **small)
        model = asymmetric_model(3)
        rng = np.random.default_rng(3)
        pl = [asymmetric_model(3, seed=23)] + [model.perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, moment=0.2, sigma=0.2, residual=0.2) for _ in range(2)]
    m = cfg.num_motors
    x0, xref, keys = episodes(cfg, B, 136)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    for rate in (None, "stiff"):
        kw = dict(timing(), plant=pl, plant_of=plant_switch(T5, B), disturbance=disturbance(T5, B), u_act_in=motor_state(B, m), fault=dead_motor(T5, B, m),
                  xmeas_in=x0[::-1].copy(), **observation(NS3, B), **aging(B=B, renorm=True), xhist_in=history(x0, AM4))
        if rate:
            kw.update(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B, 8))
        got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
        S.solve_status()
        assert got[1].shape == (B, T5, m)
        same(got, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **kw), rate)
    S.close()


@pytest.mark.parametrize("rate", [None, "windup"], ids=["motors", "rate"])
def test_one_period_per_chunk_does_not_change_a_bit(rate):
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 0: one period per chunk, so every solve's history comes from the previous chunk, and the age rows are staged per
    chunk; a one-row table is staged once."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 137)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    for T in (T5, T6):
        kw = aged_case(model, x0, rate, T=T)
        whole = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
        S.set_option("test_loop_chunk_bytes", 0)
        cut = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
        one = {**kw, "meas_age": kw["meas_age"][1:2]}
        cut_1 = S.closed_loop(x0, xref, keys, T, **one)
        S.set_option("test_loop_chunk_bytes", -1)
        S.solve_status()
        same(cut, whole, rate)
        same(whole, ref(cfg, model, x0, xref, keys, T, substep_states=True, **kw), rate)
        same(cut_1, ref(cfg, model, x0, xref, keys, T, **one), rate, xsub=False)
    S.close()


@pytest.mark.parametrize("rate", [None, "windup"], ids=["motors", "rate"])
def test_continuation_through_xhist_next(rate):
    """T = 8 as 4 + 4 at S = 2 on the device: the tick schedules sliced at tick 4, the per-solve rows at solve 2; the first solve of the second call is valid
    everywhere and reads xhist_in in episodes 0 and 1."""
    cfg = obs_cfg()
    model = synthetic_iris()
    B, T, Ns = 3, 8, 4
    x0, xref, keys = episodes(cfg, B, 113)                # the case of tests/test_age_loop_cpu.py
    kw = aged_case(model, x0, rate, T=T)
    kw.update(meas_age=np.array([[3, 2, 0], [4, 1, 0], [2, 3, 0], [4, 1, 0]], np.int32), meas_valid=np.array([[0, 1, 1], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.int32),
              meas_noise=noise_rows(Ns, B), meas_bias=bias_rows(Ns, B))
    ticks, solves = ("plant_of", "disturbance", "fault"), ("meas_noise", "meas_bias", "meas_valid", "meas_age")
    part = lambda t0, t1, j0, j1: {k: (v[t0:t1] if k in ticks else v[j0:j1] if k in solves else v) for k, v in kw.items()}       # noqa: E731
    S = SdeMpcSolver(cfg, model, max_batch=B)
    full = S.closed_loop(x0, xref, keys, T, substep_states=True, **kw)
    a = S.closed_loop(x0, xref, keys, 4, substep_states=True, **part(0, 4, 0, 2))
    n0 = 10 if rate else 7
    nxt = dict(u_init=a[3], stepsize_in=a[4], u_act_in=a[6], meas_keys=a[n0 + 1], xmeas_in=a[n0 + 2], xhist_in=a[n0 + 3])
    if rate:
        nxt.update(rate_integ_in=a[8], rate_tail_in=a[9])
    b = S.closed_loop(a[0][:, -1], xref, a[5], 4, substep_states=True, **{**part(4, 8, 2, 4), **nxt})
    S.solve_status()
    cat = lambda i: np.concatenate([a[i], b[i]], 1)                       # noqa: E731
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), cat(1), cat(2)) + tuple(b[3:7])
    if rate:
        joined += (cat(7),) + tuple(b[8:10])
    joined += (cat(n0),) + tuple(b[n0 + 1:n0 + 4]) + (cat(n0 + 4),)
    same(joined, full, rate)
    same(full, ref(cfg, model, x0, xref, keys, T, substep_states=True, **kw), rate)
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    """SDEMPC_OPT_TEST_WS_FILL = 255 (every new buffer starts as NaNs, the history among them); another shape and a shallower history first, then the un-aged
    observed route, the aged one, and the un-aged one again."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 138)
    kw = aged_case(model, x0, "stiff")
    plain = {k: v for k, v in kw.items() if k not in ("meas_age", "meas_age_max", "meas_renorm", "xhist_in")}
    fresh = SdeMpcSolver(cfg, model, max_batch=B5)
    want = fresh.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    want_plain = fresh.closed_loop(x0, xref, keys, T5, substep_states=True, **plain)
    fresh.close()
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    S.closed_loop(x0[:2], xref[:, :2], keys[:2], 3, **aged_case(model, x0[:2], None, T=3, age_max=2))       # another shape and depth first (the history grows after it)
    before = S.closed_loop(x0, xref, keys, T5, substep_states=True, **plain)                               # ... and the observed route
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    after = S.closed_loop(x0, xref, keys, T5, substep_states=True, **plain)
    S.solve_status()
    same(got, want, "stiff")
    same(before, want_plain, "stiff", hist=False)
    same(after, want_plain, "stiff", hist=False)
    # no xhist_in on the poisoned handle: every row is x0, none of the fill
    no_in = {**kw, "xhist_in": None}
    same(S.closed_loop(x0, xref, keys, T5, **no_in), ref(cfg, model, x0, xref, keys, T5, **no_in), "stiff", xsub=False)
    same(want, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **kw), "stiff")
    S.close()


@pytest.mark.parametrize("rate", [None, "soft"], ids=["motors", "rate"])
def test_zero_ages_and_null_age_cfg_are_the_observed_entry_point(rate):
    """Every age 0 without renormalisation through the new entry point (whatever age_max and the history are), and the C entry point with `age_cfg` NULL,
    against sdempc_closed_loop_batch_observed: every output of that entry point in every bit; xhist_next is then the tail of xsub."""
    cfg = obs_cfg()
    model = synthetic_iris()
    B, n = B5, 2
    x0, xref, keys = episodes(cfg, B, 139)
    kw = full_case(model, rate)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    want = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    for more in (dict(meas_age=0), dict(meas_age=np.zeros((NS3, B), np.int32), meas_age_max=AM4, xhist_in=history(x0, AM4)), dict(meas_age_max=3)):
        got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw, **more)
        hist = more.get("meas_age_max", 0)
        if hist:
            assert got[-2].tobytes() == got[-1][:, -1 - hist:-1].tobytes()
            got = got[:-2] + got[-1:]
        same(got, want, rate, hist=False)
    # the C entry point with age_cfg NULL and both history pointers NULL
    H, m = cfg.horizon, 4
    fp, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    blobs = [p.to_blob() for p in kw["plant"]]
    bufs = (C.c_char_p * len(blobs))(*blobs)
    sizes = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    w, f, of, ua = kw["disturbance"], kw["fault"], kw["plant_of"], kw["u_act_in"]
    sg, be, va, qk, xmi = kw["meas_noise"], kw["meas_bias"], kw["meas_valid"], kw["meas_keys"], kw["xmeas_in"]
    oc = _abi.SdempcObsCfg(C.sizeof(_abi.SdempcObsCfg), sg.ctypes.data_as(fp), be.ctypes.data_as(fp), sg.shape[0], sg.shape[1], va.ctypes.data_as(i32p), va.shape[0], va.shape[1])
    fc = _abi.SdempcFaultCfg(C.sizeof(_abi.SdempcFaultCfg), f.ctypes.data_as(fp), f.shape[0], f.shape[1])
    sc = _abi.SdempcScenarioCfg(C.sizeof(_abi.SdempcScenarioCfg), w.ctypes.data_as(fp), T5, B, T5)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S2, kw["solve_delay"], kw["motor_lag"])
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), len(blobs), n, 0.0, -1, -1)
    xr = np.ascontiguousarray(xref, np.float32)
    z = lambda *s: np.zeros(s, np.float32)                                # noqa: E731
    out = (z(B, T5 + 1, 13), z(B, T5, m), z(B, NS3, 8), z(B, H, m), z(B), np.zeros((B, 2), np.uint32), z(B, m))
    more = (z(B, T5, 4), z(B, 3), z(B, H, 3))
    obs = (z(B, NS3, 13), np.zeros((B, 2), np.uint32), z(B, 13))
    xsub = z(B, T5 * n, 13)
    rc_ = tail = None
    if rate:
        rc_, _ = S._rate_cfg(kw["rate_loop"], n, None)
        tail = kw["rate_tail_in"]
    rc = _abi.aged_entry(S.lib)(S._h, None, None, C.byref(oc), qk.ctypes.data_as(u32p), xmi.ctypes.data_as(fp), C.byref(fc), C.byref(rc_) if rate else None,
                                C.byref(sc), C.byref(tc), C.byref(pc), C.cast(bufs, C.POINTER(C.c_void_p)), sizes, of.ctypes.data_as(i32p), B, T5,
                                x0.ctypes.data_as(fp), xr.ctypes.data_as(fp), xr.shape[0], xr.shape[1], keys.ctypes.data_as(u32p), None, None, ua.ctypes.data_as(fp),
                                out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp), out[2].ctypes.data_as(C.POINTER(_abi.SdempcInfo)),
                                out[3].ctypes.data_as(fp), out[4].ctypes.data_as(fp), out[5].ctypes.data_as(u32p), out[6].ctypes.data_as(fp), None,
                                tail.ctypes.data_as(fp) if rate else None, *([a.ctypes.data_as(fp) for a in more] if rate else [None] * 3), xsub.ctypes.data_as(fp),
                                obs[0].ctypes.data_as(fp), obs[1].ctypes.data_as(u32p), obs[2].ctypes.data_as(fp), None)
    assert rc == 0, S.lib.sdempc_last_error(S._h).decode()
    S.solve_status()
    same(out + (more if rate else ()) + obs + (xsub,), want, rate, hist=False)
    S.close()


def test_no_wrong_loop_equals_the_device():
    """The five mutants of the reference on the device's inputs: each differs from what the device computed (which equals the right loop)."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 111)              # the case of tests/test_age_loop_cpu.py
    kw = aged_case(model, x0, "stiff", T=T6)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T6, substep_states=True, **kw)
    S.solve_status()
    S.close()
    eps = [1, 4]
    same(got, ref(cfg, model, x0, xref, keys, T6, substep_states=True, episodes=eps, **kw), "stiff", eps=eps)
    for mutant in MUTANTS:
        wrong = ref(cfg, model, x0, xref, keys, T6, substep_states=True, episodes=eps, mutant=mutant, **kw)
        assert sum(bits_differ(g[eps], w[eps]) for g, w in zip(got, wrong) if g.dtype == np.float32) > 0, mutant
        assert bits_differ(got[-5][eps], wrong[-5][eps]) > 0, mutant
