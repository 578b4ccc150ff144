"""Batched closed loop on a measured state on the GPU (SPEC.md §11f, sdempc_closed_loop_batch_observed): bit for bit against the CPU reference of
tests/obs_loop_ref.py on all outputs — xs, us, info, the continuation values, ws with a rate loop, xmeas, the observation chain, the held measurement and
xsub. Shapes of tests/obs_cases.py, the smallest at which this path can go wrong: H = 8 with two step lengths, 3 iterations, T = 5 at S = 2 (Ns = 3, the
last period partial), n = 2, D = 1, B = 3 to 5 (a partly empty last workgroup); rows shared and per episode, constant and per solve; a dropout pattern that
hits solve 0, two consecutive solves and the last solve; every arithmetic; P = 1, 32, 33 and 70 with the cooperative layouts on and off; three, four and six
motors; with and without a rate loop, with a dead motor, a gust and a plant switch in the same run; chunk boundaries, continuation, a handle with a past and
poisoned buffers; the C entry point with `obs` NULL and a neutral observation against the fault entry point; and the six wrong loops of the reference, none
of which may equal what the device computes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loop_cases
from cases import CDIR, asymmetric_cfg, asymmetric_model, bits_differ
from loop_cases import ARITH, NAMES
from obs_cases import (B5, NS3, S2, T5, bias_rows, dead_motor, disturbance, episodes, full_case, held, meas_keys, motor_state, noise_rows, obs_cfg, observation,
                       perturbed_plants, plant_switch, rate_loop, rate_tail, timing)
from obs_loop_ref import MUTANTS, obs_loop_ref
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu

ref = functools.partial(loop_cases.ref, obs_loop_ref)
OBS = ("xmeas", "meas_keys_next", "xmeas_next")


def names(rate, obs=True, xsub=True):
    return NAMES[:10 if rate else 7] + (OBS if obs else ()) + (("xsub",) if xsub else ())


def same(got, want, rate, obs=True, xsub=True, eps=None):
    for n, g, w in zip(names(rate, obs, xsub), got, want):
        if n == "meas_keys_next":
            assert np.array_equal(g if eps is None else g[eps], w if eps is None else w[eps]), n
    loop_cases.same(got, want, eps=eps, names=names(rate, obs, xsub))


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_every_arithmetic(mlp_dtype, math_mode, rate):
    """A dead motor, a gust, a plant switch, noise, bias and dropouts in the same run, with and without the rate loop."""
    cfg = obs_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 121)
    kw = full_case(model, rate)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **kw), rate)
    assert np.isfinite(got[0]).all() and got[0][:, 0].tobytes() == x0.tobytes()
    assert got[-4][0, 0].tobytes() == kw["xmeas_in"][0].tobytes()                     # episode 0 drops solve 0: the held row
    assert got[-4][1, 1].tobytes() == got[-4][1, 2].tobytes() == got[-4][1, 0].tobytes()      # two consecutive dropouts, the last solve among them
    assert bits_differ(got[-4][2], got[0][2, 0:T5:S2]) > 0                            # the measurement is not the state
    S.close()


@pytest.mark.parametrize("opts", [{}, {"coop": 0}], ids=["coop_on", "coop_off"])
@pytest.mark.parametrize("P", [1, 32, 33, 70])
def test_particle_counts_and_layouts(P, opts):
    """P = 1 (lanes), a full group, a group and one, three groups; with the cooperative / speculative layouts and without them."""
    B = 3
    cfg = obs_cfg(num_particles=P)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B, 122)
    kw = full_case(model, "stiff", B=B)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
    got = S.closed_loop(x0, xref, keys, T5, **kw)
    S.solve_status()
    print("solve kernel:", S.last_kernel_name())
    same(got, ref(cfg, model, x0, xref, keys, T5, **kw), "stiff", xsub=False)
    S.close()


@pytest.mark.parametrize("name,B,P,opts", [("coop", 1, 33, {"spec": 0}), ("spec", 1, 33, {})])
def test_a_lone_episode_in_the_cooperative_layouts(name, B, P, opts):
    cfg = obs_cfg(num_particles=P)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B, 123)
    kw = full_case(model, None, B=B)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
    got = S.closed_loop(x0, xref, keys, T5, **kw)
    S.solve_status()
    assert ("spec" in S.last_kernel_name()) == (name == "spec"), S.last_kernel_name()
    same(got, ref(cfg, model, x0, xref, keys, T5, **kw), None, xsub=False)
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
    x0, xref, keys = episodes(cfg, B, 124)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    for rate in (None, "stiff"):
        kw = dict(timing(), plant=pl, plant_of=plant_switch(T5, B), disturbance=disturbance(T5, B), u_act_in=motor_state(B, m), fault=dead_motor(T5, B, m),
                  xmeas_in=held(B), **observation(NS3, B))
        if rate:
            kw.update(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B, 8))
        got = S.closed_loop(x0, xref, keys, T5, **kw)
        S.solve_status()
        assert got[1].shape == (B, T5, m)
        same(got, ref(cfg, model, x0, xref, keys, T5, **kw), rate, xsub=False)
    S.close()


@pytest.mark.parametrize("constant", [False, True], ids=["per_solve", "constant"])
@pytest.mark.parametrize("shared", [False, True], ids=["per_episode", "shared"])
def test_rows_shared_and_per_episode_constant_and_per_solve(shared, constant):
    """Every stride of the three row tables: [Ns|1][B|1]; then the short forms of the Python layer, and sigma / beta / valid given alone."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 125)
    base = dict(timing(), plant=perturbed_plants(model, 3)[1], u_act_in=motor_state(B5, 4))
    o = observation(NS3, B5, shared=shared, constant=constant)
    assert o["meas_noise"].shape == (1 if constant else NS3, 1 if shared else B5, 12) and o["meas_valid"].shape == (1 if constant else NS3, 1 if shared else B5)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T5, **base, **o)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T5, **base, **o), None, xsub=False)
    if shared:            # [Ns][12] / [12] / [Ns]: the same rows in the short forms
        short = dict(o, meas_noise=o["meas_noise"][0, 0] if constant else o["meas_noise"][:, 0], meas_bias=o["meas_bias"][0, 0] if constant else o["meas_bias"][:, 0])
        if not constant:
            short["meas_valid"] = o["meas_valid"][:, 0]
        same(S.closed_loop(x0, xref, keys, T5, **base, **short), got, None, xsub=False)
    else:                 # one table alone: the others NULL (zeros / always valid)
        for only in ("meas_noise", "meas_bias", "meas_valid"):
            one = {only: o[only], "meas_keys": o["meas_keys"]}
            alone = S.closed_loop(x0, xref, keys, T5, **base, **one)
            same(alone, ref(cfg, model, x0, xref, keys, T5, **base, **one), None, xsub=False)
    S.close()


def moving_case(model, B=B5, T=T5):
    """The full case with a reference window per solve, so that every staged table moves from chunk to chunk."""
    cfg = obs_cfg()
    x0, _, keys = episodes(cfg, B, 126)
    Ns = -(-T // S2)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B)]) for j in range(Ns)])
    return cfg, x0, xref, keys


@pytest.mark.parametrize("rate", [None, "windup"], ids=["motors", "rate"])
def test_chunk_boundaries_do_not_change_a_bit(rate):
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 0: one period per chunk, so the three solves are three chunks; the rows are staged per chunk and xmeas spans them."""
    model = synthetic_iris()
    cfg, x0, xref, keys = moving_case(model)
    kw = full_case(model, rate)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    whole = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    S.set_option("test_loop_chunk_bytes", 0)
    cut = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    one = {**kw, "meas_noise": kw["meas_noise"][:1], "meas_bias": kw["meas_bias"][:1], "meas_valid": kw["meas_valid"][:1]}      # one-row tables are staged once
    cut_1 = S.closed_loop(x0, xref, keys, T5, substep_states=True, **one)
    S.solve_status()
    same(cut, whole, rate)
    same(whole, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **kw), rate)
    same(cut_1, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **one), rate)
    S.close()


@pytest.mark.parametrize("rate", [None, "windup"], ids=["motors", "rate"])
def test_continuation_split_at_a_multiple_of_the_period(rate):
    """T = 5 as 4 + 1 at S = 2: the tick schedules sliced at tick 4, the observation rows and the references at solve 2."""
    model = synthetic_iris()
    cfg, x0, xref, keys = moving_case(model)
    kw = full_case(model, rate)
    ticks, solves = ("plant_of", "disturbance", "fault"), ("meas_noise", "meas_bias", "meas_valid")
    part = lambda t0, t1, j0, j1: {k: (v[t0:t1] if k in ticks else v[j0:j1] if k in solves else v) for k, v in kw.items()}       # noqa: E731
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    full = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    a = S.closed_loop(x0, xref[:2], keys, 4, substep_states=True, **part(0, 4, 0, 2))
    nxt = dict(u_init=a[3], stepsize_in=a[4], u_act_in=a[6], meas_keys=a[-3], xmeas_in=a[-2])
    if rate:
        nxt.update(rate_integ_in=a[8], rate_tail_in=a[9])
    b = S.closed_loop(a[0][:, -1], xref[2:], a[5], 1, substep_states=True, **{**part(4, 5, 2, 3), **nxt})
    S.solve_status()
    n0 = 10 if rate else 7
    cat = lambda i: np.concatenate([a[i], b[i]], 1)                       # noqa: E731
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), cat(1), cat(2)) + tuple(b[3:7])
    if rate:
        joined += (cat(7),) + tuple(b[8:10])
    joined += (cat(n0),) + tuple(b[n0 + 1:n0 + 3]) + (cat(n0 + 3),)
    same(joined, full, rate)
    same(full, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **kw), rate)
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    """SDEMPC_OPT_TEST_WS_FILL = 255 (every new buffer starts as NaNs), another shape and the unobserved route first."""
    model = synthetic_iris()
    cfg, x0, xref, keys = moving_case(model)
    kw = full_case(model, "stiff")
    fresh = SdeMpcSolver(cfg, model, max_batch=B5)
    want = fresh.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    fresh.close()
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    S.closed_loop(x0[:2], xref[:2, :2], keys[:2], 3, **full_case(model, None, B=2, T=3))                                             # another shape first
    S.closed_loop(x0, xref, keys, T5, **{k: v for k, v in kw.items() if not k.startswith("meas_") and k != "xmeas_in"})              # ... and the fault route
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    S.solve_status()
    same(got, want, "stiff")
    same(S.closed_loop(x0, xref, keys, T5, **{**kw, "xmeas_in": None}), ref(cfg, model, x0, xref, keys, T5, **{**kw, "xmeas_in": None}), "stiff", xsub=False)
    same(want, ref(cfg, model, x0, xref, keys, T5, substep_states=True, **kw), "stiff")
    S.close()


@pytest.mark.parametrize("rate", [None, "soft"], ids=["motors", "rate"])
def test_neutral_observation_and_null_obs_are_the_fault_entry_point(rate):
    """A neutral observation (zeros, always valid) through the new entry point, and the C entry point with `obs` NULL, against sdempc_closed_loop_batch_fault:
    every output of that entry point in every bit (the cases hold no -0 component); xmeas is then the plant state at each solve."""
    cfg = obs_cfg()
    model = synthetic_iris()
    B, n = B5, 2
    x0, xref, keys = episodes(cfg, B, 127)
    assert not np.signbit(x0[x0 == 0]).any()
    kw = {k: v for k, v in full_case(model, rate).items() if not k.startswith("meas_") and k != "xmeas_in"}
    S = SdeMpcSolver(cfg, model, max_batch=B)
    want = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    for o in (dict(meas_noise=np.zeros(12, np.float32)), dict(meas_bias=np.zeros((NS3, B, 12), np.float32), meas_valid=np.ones(NS3, np.int32), xmeas_in=held(B))):
        got = S.closed_loop(x0, xref, keys, T5, substep_states=True, meas_keys=meas_keys(B), **o, **kw)
        same(got[:-4] + got[-1:], want, rate, obs=False)
        assert not np.signbit(got[0][got[0] == 0]).any()
        assert got[-4].tobytes() == got[0][:, 0:T5:S2].tobytes() and got[-2].tobytes() == got[-4][:, -1].tobytes()
    # the C entry point with obs NULL and every observation pointer NULL
    H, m = cfg.horizon, 4
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    blobs = [p.to_blob() for p in kw["plant"]]
    bufs = (C.c_char_p * len(blobs))(*blobs)
    sizes = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    w, f, of, ua = kw["disturbance"], kw["fault"], kw["plant_of"], kw["u_act_in"]
    fc = _abi.SdempcFaultCfg(C.sizeof(_abi.SdempcFaultCfg), f.ctypes.data_as(fp), f.shape[0], f.shape[1])
    sc = _abi.SdempcScenarioCfg(C.sizeof(_abi.SdempcScenarioCfg), w.ctypes.data_as(fp), T5, B, T5)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S2, kw["solve_delay"], kw["motor_lag"])
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), len(blobs), n, 0.0, -1, -1)
    xr = np.ascontiguousarray(xref, np.float32)
    z = lambda *s: np.zeros(s, np.float32)                                # noqa: E731
    out = (z(B, T5 + 1, 13), z(B, T5, m), z(B, NS3, 8), z(B, H, m), z(B), np.zeros((B, 2), np.uint32), z(B, m))
    more = (z(B, T5, 4), z(B, 3), z(B, H, 3))
    xsub = z(B, T5 * n, 13)
    rc_ = tail = None
    if rate:
        rc_, _ = S._rate_cfg(kw["rate_loop"], n, None)
        tail = kw["rate_tail_in"]
    rc = _abi.observed_entry(S.lib)(S._h, None, None, None, C.byref(fc), C.byref(rc_) if rate else None, C.byref(sc), C.byref(tc), C.byref(pc),
                                    C.cast(bufs, C.POINTER(C.c_void_p)), sizes, of.ctypes.data_as(C.POINTER(C.c_int32)), B, T5, x0.ctypes.data_as(fp),
                                    xr.ctypes.data_as(fp), xr.shape[0], xr.shape[1], keys.ctypes.data_as(u32p), None, None, ua.ctypes.data_as(fp),
                                    out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp), out[2].ctypes.data_as(C.POINTER(_abi.SdempcInfo)),
                                    out[3].ctypes.data_as(fp), out[4].ctypes.data_as(fp), out[5].ctypes.data_as(u32p), out[6].ctypes.data_as(fp), None,
                                    tail.ctypes.data_as(fp) if rate else None, *([a.ctypes.data_as(fp) for a in more] if rate else [None] * 3), xsub.ctypes.data_as(fp),
                                    None, None, None)
    assert rc == 0, S.lib.sdempc_last_error(S._h).decode()
    S.solve_status()
    same(out + (more if rate else ()) + (xsub,), want, rate, obs=False)
    S.close()


def test_no_wrong_loop_equals_the_device():
    """The six mutants of the reference on the device's inputs: each differs from what the device computed (which equals the right loop)."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 111)              # the case of tests/test_obs_loop_cpu.py
    kw = full_case(model, "stiff")
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T5, substep_states=True, **kw)
    S.solve_status()
    S.close()
    eps = [0, 4]
    same(got, ref(cfg, model, x0, xref, keys, T5, substep_states=True, episodes=eps, **kw), "stiff", eps=eps)
    for mutant in MUTANTS:
        wrong = ref(cfg, model, x0, xref, keys, T5, substep_states=True, episodes=eps, mutant=mutant, **kw)
        assert sum(bits_differ(g[eps], w[eps]) for g, w in zip(got, wrong) if g.dtype == np.float32) > 0, mutant
        assert bits_differ(got[-4][eps], wrong[-4][eps]) > 0, mutant
