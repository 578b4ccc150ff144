"""Batched closed loop with per-motor actuator faults and substep-resolution states on the GPU (SPEC.md §11e, sdempc_closed_loop_batch_fault): bit for bit
against the CPU reference of tests/fault_loop_ref.py on all outputs, xsub included. Shapes of tests/test_gpu_rate_loop.py, the smallest at which these kernels
can go wrong: H = 4 with S = 3, T = 7 (a partial last period), B = 5 (a partly empty last workgroup of four), P in {1, 33}, n in {1, 3}; the delay D in
{0, n + 1, S n} (never the tail, an arrival in the middle of a tick, always the tail); shared and per-episode plants, with a plant switch and a fault change on
the same tick; rate loop on and off, lag on and off (lag off without a rate loop: the control table is re-formed at tick starts and at the arrival only);
every arithmetic; three, four and six motors; broadcast schedules; every solve layout; continuation, chunk boundaries, a handle with a past, the substep states
alone, and the C entry point with both additions NULL against the rate and the scenario entry points. The fault schedule is that of tests/fault_cases.py,
whose census (asserted in tests/test_fault_loop_cpu.py) shows that in the reference every faulted episode and its solves do change."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loop_cases
from cases import CDIR, asymmetric_cfg, asymmetric_model, bits_differ
from fault_cases import (ALPHA, B5, S3, SCHEDULE, T7, disturbance, episodes, faults, faults_any, motor_state, perturbed_plants, rate_loop, rate_tail, small_cfg,
                         timing)
from fault_loop_ref import fault_loop_ref
from loop_cases import ARITH, NAMES
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver, fault_schedule
from test_gpu_closed_loop import LAYOUTS

pytestmark = pytest.mark.gpu

ref = functools.partial(loop_cases.ref, fault_loop_ref)


def names(rate, xsub=True):
    return NAMES[:10 if rate else 7] + (("xsub",) if xsub else ())


def same(got, want, rate, xsub=True, eps=None):
    loop_cases.same(got, want, eps=eps, names=names(rate, xsub))


def rate_kw(rate, B=B5, H=4):
    return {} if rate is None else dict(rate_loop=rate_loop(rate), rate_tail_in=rate_tail(B, H))


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("P,n", [(1, 1), (33, 3)])
def test_fault_loop_matches_reference(P, n, per_episode, rate):
    cfg = small_cfg(num_particles=P)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 91)
    pl = perturbed_plants(model, 3)
    f = faults()
    # a plant switch and a fault change on the same tick (episode 1 at tick 2, episode 4 at tick 4), inside a period and at a period start
    for k, b in ((2, 1), (4, 4)):
        assert SCHEDULE[k, b] != SCHEDULE[k - 1, b] and f[k, b].tobytes() != f[k - 1, b].tobytes()
    kw = dict(plant=pl, plant_of=SCHEDULE) if per_episode else dict(plant=pl[1])
    kw.update(u_act_in=motor_state(B5, 4), disturbance=disturbance(T7, B5), **rate_kw(rate))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    for D in (0, n + 1, S3 * n):
        healthy = S.closed_loop(x0, xref, keys, T7, **kw, **timing(n, D))
        got = S.closed_loop(x0, xref, keys, T7, fault=f, substep_states=True, **kw, **timing(n, D))
        S.solve_status()
        same(got, ref(cfg, model, x0, xref, keys, T7, fault=f, substep_states=True, **kw, **timing(n, D)), rate)
        assert np.isfinite(got[0]).all() and got[0][:, 0].tobytes() == x0.tobytes()
        assert got[-1][:, n - 1::n].tobytes() == got[0][:, 1:].tobytes()
        assert bits_differ(got[0][0], healthy[0][0]) == 0 and all(bits_differ(got[0][b], healthy[0][b]) > 0 for b in range(1, B5))     # the fault is not ignored
        assert np.array_equal(got[5], healthy[5])                                   # the key schedule is S and T only
    S.close()


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("lag", [0.0, ALPHA], ids=["lag_off", "lag_on"])
def test_lag_and_rate_loop_on_and_off(lag, rate):
    """lag off without a rate loop: the command row is rewritten at tick starts and at the arrival substep only (D = n + 1: the middle of tick 1)."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 92)
    f = faults()
    kw = dict(timing(n), plant=perturbed_plants(model, 3)[2], u_act_in=motor_state(B5, 4), fault=f, substep_states=True, **rate_kw(rate))
    kw["motor_lag"] = lag
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, **kw), rate)
    # the fault sits behind the motor state: episode 3's motor 1 is stuck at 0.9 on ticks 1 - 4, and neither us nor u_act_next ever shows it
    assert not (got[1][3, :, 1] == np.float32(0.9)).any()
    S.close()


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_every_arithmetic(mlp_dtype, math_mode, rate):
    """Disturbance, plant schedule, fault schedule and substep states together, with and without the rate loop: the twelve new kernels."""
    cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 93)
    kw = dict(timing(n), plant=perturbed_plants(model, 3), plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4), fault=faults(),
              substep_states=True, **rate_kw(rate))
    if rate:
        kw["rate_loop"] = rate_loop(rate, motor_weight=0.35)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, **kw), rate)
    S.close()


def test_plant_arithmetic_pinned_apart_from_the_controllers():
    cfg = small_cfg(mlp_dtype="f32x3", math_mode="fast")
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 94)
    kw = dict(timing(n), plant=perturbed_plants(model, 3), plant_of=SCHEDULE, fault=faults(), substep_states=True, plant_mlp_dtype="f16", plant_math_mode="exact")
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, **kw), None)
    S.close()


@pytest.mark.parametrize("vehicle", ["hexa", "asymmetric3"])
def test_other_motor_counts(vehicle):
    """m = 6 (the hexarotor) and m = 3 (the asymmetric model: no two motors alike, so a pair that reaches the wrong motor shows); m = 4 is every other test."""
    B, n = 3, 2
    if vehicle == "hexa":
        cfg = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(horizon=4, num_short_dt=4, num_particles=33, max_iter=3, max_no_improvement_iter=3)
        model = synthetic_hexa()
        pl = perturbed_plants(model, 3)
    else:
        cfg = asymmetric_cfg(3, horizon=4, num_short_dt=4, num_particles=33, max_iter=3, max_no_improvement_iter=3)
        model = asymmetric_model(3)
        rng = np.random.default_rng(3)
        pl = [asymmetric_model(3, seed=23)] + [model.perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, moment=0.2, sigma=0.2, residual=0.2) for _ in range(2)]
    m = cfg.num_motors
    x0, xref, keys = episodes(cfg, B, 95)
    f = faults_any(T7, B, m)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    for rate in (None, "stiff"):
        kw = dict(timing(n), plant=pl, plant_of=SCHEDULE[:, 1:4], disturbance=disturbance(T7, B), u_act_in=motor_state(B, m), fault=f, substep_states=True,
                  **rate_kw(rate, B))
        got = S.closed_loop(x0, xref, keys, T7, **kw)
        S.solve_status()
        assert got[1].shape == (B, T7, m) and got[-1].shape == (B, T7 * n, 13)
        same(got, ref(cfg, model, x0, xref, keys, T7, **kw), rate)
    S.close()


def test_broadcast_schedules():
    """Tf = 1, Bf = 1, both, and the two short forms of the Python layer; each equals the schedule written out in full."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 96)
    f = faults()
    kw = dict(timing(n), plant=perturbed_plants(model, 3), plant_of=SCHEDULE, u_act_in=motor_state(B5, 4), substep_states=True)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    full = {}
    for name, short, long in (("Tf1", f[4:5], np.repeat(f[4:5], T7, 0)), ("Bf1", f[:, 3:4], np.repeat(f[:, 3:4], B5, 1)),
                              ("both", f[4:5, 4:5], np.broadcast_to(f[4, 4], f.shape)), ("[T][m][2]", f[:, 3], np.repeat(f[:, 3:4], B5, 1)),
                              ("[m][2]", f[4, 4], np.broadcast_to(f[4, 4], f.shape))):
        got = S.closed_loop(x0, xref, keys, T7, fault=short, **kw)
        S.solve_status()
        same(got, ref(cfg, model, x0, xref, keys, T7, fault=short, **kw), None)
        if name not in full:
            full[name] = S.closed_loop(x0, xref, keys, T7, fault=np.ascontiguousarray(long), **kw)
        same(got, full[name], None)
    assert bits_differ(full["Tf1"][0], full["Bf1"][0]) > 0
    S.close()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_solve_layout(name):
    B, P, opts = LAYOUTS[name]
    cfg = small_cfg(num_particles=P, horizon=10, num_short_dt=10)
    model = synthetic_iris()
    T, Sp, n = 6, 2, 2
    x0, xref, keys = episodes(cfg, B, 97)
    pl = perturbed_plants(model, 3)
    of = np.random.default_rng(5).integers(0, 3, (T, B)).astype(np.int32)
    kw = dict(plant=pl, plant_of=of, disturbance=disturbance(T, B), plant_substeps=n, solve_period=Sp, solve_delay=n + 1, motor_lag=ALPHA, rate_loop=rate_loop("stiff"),
              fault=faults_any(T, B, 4), substep_states=True)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
    got = S.closed_loop(x0, xref, keys, T, **kw)
    S.solve_status()
    kname = S.last_kernel_name()
    assert ("spec" in kname) == (name == "spec"), kname
    sample = [0, B - 1] if B > 2 else list(range(B))
    same(got, ref(cfg, model, x0, xref, keys, T, episodes=sample, **kw), "stiff", eps=sample)
    S.close()


@pytest.mark.parametrize("rate", [None, "windup"], ids=["motors", "rate"])
def test_continuation_with_the_schedules_sliced(rate):
    """T = 6 as 3 + 3 at S = 3: the fault schedule and the disturbance sliced at tick 3, xsub joined."""
    cfg = small_cfg()
    model = synthetic_iris()
    B, n, T = 3, 3, 6
    x0, _, keys = episodes(cfg, B, 98)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B)]) for j in range(2)])      # one window per solve
    pl = perturbed_plants(model, 3)
    w = disturbance(T, B)
    f = faults_any(T, B, 4)
    kw = dict(timing(n), plant=pl, substep_states=True)
    if rate:
        kw["rate_loop"] = rate_loop(rate)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    full = S.closed_loop(x0, xref, keys, T, disturbance=w, fault=f, u_act_in=motor_state(B, 4), **kw)
    a = S.closed_loop(x0, xref[:1], keys, 3, disturbance=w[:3], fault=f[:3], u_act_in=motor_state(B, 4), **kw)
    more = dict(rate_integ_in=a[8], rate_tail_in=a[9]) if rate else {}
    b = S.closed_loop(a[0][:, -1], xref[1:], a[5], 3, disturbance=w[3:], fault=f[3:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6], **more, **kw)
    S.solve_status()
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), np.concatenate([a[1], b[1]], 1), np.concatenate([a[2], b[2]], 1)) + tuple(b[3:7])
    if rate:
        joined += (np.concatenate([a[7], b[7]], 1),) + tuple(b[8:10])
    joined += (np.concatenate([a[-1], b[-1]], 1),)
    same(joined, full, rate)
    same(full, ref(cfg, model, x0, xref, keys, T, disturbance=w, fault=f, u_act_in=motor_state(B, 4), **kw), rate)
    S.close()


@pytest.mark.parametrize("rate", [None, "windup"], ids=["motors", "rate"])
def test_chunk_boundaries_do_not_change_a_bit(rate):
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 1: one period per chunk, so T = 7 at S = 3 is three chunks; the fault rows are staged per chunk and xsub spans them."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, _, keys = episodes(cfg, B5, 99)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B5)]) for j in range(3)])
    kw = dict(timing(n), plant=perturbed_plants(model, 3), plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4), fault=faults(),
              substep_states=True, **rate_kw(rate))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    whole = S.closed_loop(x0, xref, keys, T7, **kw)
    S.set_option("test_loop_chunk_bytes", 1)
    cut = S.closed_loop(x0, xref, keys, T7, **kw)
    cut_1 = S.closed_loop(x0, xref, keys, T7, **{**kw, "fault": kw["fault"][:1]})         # a one-row schedule is staged once, not per chunk
    S.solve_status()
    same(cut, whole, rate)
    same(whole, ref(cfg, model, x0, xref, keys, T7, **kw), rate)
    same(cut_1, ref(cfg, model, x0, xref, keys, T7, **{**kw, "fault": kw["fault"][:1]}), rate)
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 100)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), rate_loop=rate_loop("stiff"), fault=faults(), substep_states=True)
    fresh = SdeMpcSolver(cfg, model, max_batch=B5)
    want = fresh.closed_loop(x0, xref, keys, T7, **kw)
    fresh.close()
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    S.closed_loop(x0[:2], xref[:, :2], keys[:2], 4, plant=pl[:2], plant_substeps=2, solve_period=2, fault=faults_any(4, 2, 4), substep_states=True)      # another shape first
    S.closed_loop(x0, xref, keys, T7, **{k: v for k, v in kw.items() if k not in ("fault", "substep_states")})                                          # ... and the rate route
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, want, "stiff")
    same(S.closed_loop(x0, xref, keys, T7, **{**kw, "substep_states": False}), want[:-1], "stiff", xsub=False)
    same(want, ref(cfg, model, x0, xref, keys, T7, **kw), "stiff")
    S.close()


@pytest.mark.parametrize("route", ["timed", "scenario", "rate"])
def test_substep_states_alone_equal_the_existing_route(route):
    """fault=None, substep_states=True: the existing route's outputs in every bit, plus the record; a neutral schedule [1][1][m][2] gives them too."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 101)
    kw = dict(timing(n), plant=perturbed_plants(model, 3), plant_of=SCHEDULE[0], u_act_in=motor_state(B5, 4))
    if route != "timed":
        kw.update(plant_of=SCHEDULE, disturbance=disturbance(T7, B5))
    rate = "soft" if route == "rate" else None
    kw.update(rate_kw(rate))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    want = S.closed_loop(x0, xref, keys, T7, **kw)
    got = S.closed_loop(x0, xref, keys, T7, substep_states=True, **kw)
    neutral = S.closed_loop(x0, xref, keys, T7, fault=fault_schedule(1, 1, 4), **kw)
    S.solve_status()
    same(got[:-1], want, rate, xsub=False)
    same(neutral, want, rate, xsub=False)
    assert got[-1][:, n - 1::n].tobytes() == want[0][:, 1:].tobytes()
    same(got, ref(cfg, model, x0, xref, keys, T7, substep_states=True, **kw), rate)
    S.close()


@pytest.mark.parametrize("rated", [False, True], ids=["scenario", "rate"])
def test_c_entry_point_with_both_additions_null_is_the_entry_below(rated):
    """sdempc_closed_loop_batch_fault with fault_cfg NULL (and with a cfg whose fault is NULL) and xsub NULL: the rate entry point's ten outputs with a rate
    cfg, the scenario entry point's seven without one."""
    cfg = small_cfg()
    model = synthetic_iris()
    B, n = B5, 3
    x0, xref, keys = episodes(cfg, B, 102)
    pl = perturbed_plants(model, 3)
    ua, w = motor_state(B, 4), disturbance(T7, B)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    rl = rate_loop("stiff", motor_weight=0.35)
    want = S.closed_loop(x0, xref, keys, T7, plant=pl, plant_of=SCHEDULE, disturbance=w, u_act_in=ua, **timing(n), **(dict(rate_loop=rl) if rated else {}))
    H, m = cfg.horizon, 4
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    blobs = [p.to_blob() for p in pl]
    bufs = (C.c_char_p * len(blobs))(*blobs)
    sizes = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    rc_, _ = S._rate_cfg(rl, n, None)
    sc = _abi.SdempcScenarioCfg(C.sizeof(_abi.SdempcScenarioCfg), w.ctypes.data_as(fp), T7, B, T7)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S3, n + 1, ALPHA)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), len(blobs), n, 0.0, -1, -1)
    xr = np.ascontiguousarray(xref, np.float32)
    for fc in (None, _abi.SdempcFaultCfg(C.sizeof(_abi.SdempcFaultCfg), None, 0, 0)):
        out = (np.zeros((B, T7 + 1, 13), np.float32), np.zeros((B, T7, m), np.float32), np.zeros((B, 3, 8), np.float32), np.zeros((B, H, m), np.float32),
               np.zeros(B, np.float32), np.zeros((B, 2), np.uint32), np.zeros((B, m), np.float32))
        more = (np.zeros((B, T7, 4), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, H, 3), np.float32))
        rc = _abi.fault_entry(S.lib)(S._h, None if fc is None else C.byref(fc), C.byref(rc_) if rated else None, C.byref(sc), C.byref(tc), C.byref(pc),
                                     C.cast(bufs, C.POINTER(C.c_void_p)), sizes, SCHEDULE.ctypes.data_as(C.POINTER(C.c_int32)), B, T7, x0.ctypes.data_as(fp),
                                     xr.ctypes.data_as(fp), xr.shape[0], xr.shape[1], keys.ctypes.data_as(u32p), None, None, ua.ctypes.data_as(fp),
                                     out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp), out[2].ctypes.data_as(C.POINTER(_abi.SdempcInfo)),
                                     out[3].ctypes.data_as(fp), out[4].ctypes.data_as(fp), out[5].ctypes.data_as(u32p), out[6].ctypes.data_as(fp), None, None,
                                     *([a.ctypes.data_as(fp) for a in more] if rated else [None] * 3), None)
        assert rc == 0, S.lib.sdempc_last_error(S._h).decode()
        S.solve_status()
        same(out + (more if rated else ()), want, rated, xsub=False)
    S.close()


def test_simulate_returns_the_substep_states_in_the_frame_of_x():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    cfg = small_cfg()
    model = synthetic_iris()
    T, n = 4, 3
    x0, _, keys = episodes(cfg, 1, 103)
    f = fault_schedule(T, 1, 4)[:, 0]
    f[1:, 2] = (0.0, 0.0)
    prob = MpcProblem(cfg=cfg, model=model, convert_to_enu=True)
    x = x0[0]                                   # the caller's frame; the flip is an involution in exact arithmetic only, so the solver's state is formed once, here
    xsol = enu2ned(x, np)
    xs, us, info, st, key, xsub = prob.simulate(x, keys[0], T, plant_substeps=n, solve_period=2, fault=f, substep_states=True)
    S = prob.solver()
    want = S.closed_loop(xsol[None], W.constant_reference(xsol, cfg.horizon), keys, T, plant_substeps=n, solve_period=2, fault=f[:, None], substep_states=True)
    assert xs[0].tobytes() == x.tobytes() and bits_differ(np.asarray(xs[1:]), enu2ned(want[0][0, 1:], np)) == 0 and bits_differ(np.asarray(info), want[2][0]) == 0
    assert xsub.shape == (T * n, 13) and np.asarray(xsub).tobytes() == np.ascontiguousarray(enu2ned(want[-1][0], np), np.float32).tobytes()
    assert np.asarray(xsub[n - 1::n]).tobytes() == np.asarray(xs[1:]).tobytes() and np.asarray(us).tobytes() == want[1][0].tobytes()
    healthy = prob.simulate(x, keys[0], T, plant_substeps=n, solve_period=2)
    assert len(healthy) == 5 and bits_differ(np.asarray(healthy[0]), np.asarray(xs)) > 0
