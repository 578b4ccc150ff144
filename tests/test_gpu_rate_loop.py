"""Batched closed loop through the rate-setpoint interface on the GPU (SPEC.md §11d, sdempc_closed_loop_batch_rate): bit for bit against the CPU reference
of tests/rate_loop_ref.py on all ten outputs. Shapes of tests/test_gpu_scenario_loop.py: H = 4 with S = 3, T = 7 (a partial last period), B = 5 (a partly
empty last workgroup of four), P in {1, 33}, n in {1, 3}; the delay D in {0, 2, S n} (never the tail, mid-period, always the tail); shared and per-episode
plants; every arithmetic; scenario and rate loop together; lag on and off; every blend weight; every solve layout; six and three motors; continuation,
chunk boundaries, a handle with a past, and the C entry point against the timed one. The gains are those of tests/rate_loop_cases.py, whose census (asserted in
tests/test_rate_loop_cpu.py) shows that the reference reaches both clamps on these inputs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loop_cases
from cases import CDIR, asymmetric_cfg, asymmetric_model, bits_differ
from loop_cases import ARITH, NAMES, same
from rate_loop_cases import (ALPHA, B5, S3, SCHEDULE, T7, WEIGHTS, disturbance, episodes, full_mixer, integ_state, motor_state, perturbed_plants, rate_loop,
                             rate_tail, small_cfg, timing)
from rate_loop_ref import rate_loop_ref
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver
from test_gpu_closed_loop import LAYOUTS

pytestmark = pytest.mark.gpu

ref = functools.partial(loop_cases.ref, rate_loop_ref)


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("P,n,H", [(1, 1, 4), (33, 3, 4), (1, 3, 2)])
def test_rate_loop_matches_reference(P, n, H, per_episode):
    """D = 0 never reads the tail, D = 2 switches source inside a period, D = S n flies the tail throughout; H = 2 with S = 3 reaches the min(., H - 1) rows."""
    cfg = small_cfg(num_particles=P, horizon=H, num_short_dt=H)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 71)
    pl = perturbed_plants(model, 3)
    kw = dict(plant=pl, plant_of=np.array([0, 1, 2, 1, 0], np.int32)) if per_episode else dict(plant=pl[1])
    kw.update(u_act_in=motor_state(B5, 4), rate_integ_in=integ_state(B5), rate_tail_in=rate_tail(B5, H))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    plain = S.closed_loop(x0, xref, keys, T7, **{k: v for k, v in kw.items() if not k.startswith("rate_")}, **timing(n, 2))
    for D, name in ((0, "stiff"), (2, "windup"), (S3 * n, "stiff")):
        got = S.closed_loop(x0, xref, keys, T7, rate_loop=rate_loop(name), **kw, **timing(n, D))
        S.solve_status()
        same(got, ref(cfg, model, x0, xref, keys, T7, rate_loop=rate_loop(name), **kw, **timing(n, D)))
        assert np.isfinite(got[0]).all() and got[0][:, 0].tobytes() == x0.tobytes()
        assert bits_differ(got[0][:, 1:], plain[0][:, 1:]) > 0                     # the rate loop is not ignored
        assert np.array_equal(got[5], plain[5])                                    # the key schedule is S and T only
    S.close()


@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_scenario_and_rate_loop_in_every_arithmetic(mlp_dtype, math_mode):
    """Disturbance, plant schedule (switches inside a period) and rate loop together."""
    cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 72)
    pl = perturbed_plants(model, 3)
    assert any(SCHEDULE[k, b] != SCHEDULE[k - 1, b] for k in range(1, T7) if k % S3 for b in range(B5))
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4), rate_loop=rate_loop("stiff", motor_weight=0.35),
              rate_tail_in=rate_tail(B5, 4))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, **kw))
    S.close()


def test_plant_arithmetic_pinned_apart_from_the_controllers():
    cfg = small_cfg(mlp_dtype="f32x3", math_mode="fast")
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 73)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), rate_loop=rate_loop("windup"))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, plant_mlp_dtype="f32", plant_math_mode="exact", **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, plant_mlp_dtype="f32", plant_math_mode="exact", **kw))
    assert bits_differ(got[0], S.closed_loop(x0, xref, keys, T7, **kw)[0]) > 0
    S.close()


@pytest.mark.parametrize("lag", [0.0, ALPHA], ids=["lag_off", "lag_on"])
def test_blend_weights_with_and_without_lag(lag):
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 74)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl[2], u_act_in=motor_state(B5, 4), rate_tail_in=rate_tail(B5, 4))
    kw["motor_lag"] = lag
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    runs = {}
    for w in WEIGHTS:
        rl = rate_loop("stiff", motor_weight=w)
        runs[w] = S.closed_loop(x0, xref, keys, T7, rate_loop=rl, **kw)
        S.solve_status()
        same(runs[w], ref(cfg, model, x0, xref, keys, T7, rate_loop=rl, **kw))
    assert bits_differ(runs[0.0][0], runs[0.35][0]) > 0 and bits_differ(runs[0.35][0], runs[1.0][0]) > 0
    # motor_weight = 1 flies the motor values exactly: the timed loop's seven outputs, while the integrator still runs
    same(runs[1.0][:7], S.closed_loop(x0, xref, keys, T7, **{k: v for k, v in kw.items() if k != "rate_tail_in"}), names=NAMES[:7])
    assert np.abs(runs[1.0][8]).max() > 0
    S.close()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_solve_layout(name):
    B, P, opts = LAYOUTS[name]
    cfg = small_cfg(num_particles=P, horizon=10, num_short_dt=10)
    model = synthetic_iris()
    T, Sp, n = 6, 2, 2
    x0, xref, keys = episodes(cfg, B, 75)
    pl = perturbed_plants(model, 3)
    of = np.random.default_rng(5).integers(0, 3, (T, B)).astype(np.int32)
    kw = dict(plant=pl, plant_of=of, disturbance=disturbance(T, B), plant_substeps=n, solve_period=Sp, solve_delay=n + 1, motor_lag=ALPHA, rate_loop=rate_loop("stiff"))
    S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
    got = S.closed_loop(x0, xref, keys, T, **kw)
    S.solve_status()
    kname = S.last_kernel_name()
    assert ("spec" in kname) == (name == "spec"), kname
    sample = [0, B - 1] if B > 2 else list(range(B))
    same(got, ref(cfg, model, x0, xref, keys, T, episodes=sample, **kw), eps=sample)
    S.close()


def test_hexa_six_motors():
    cfg = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(horizon=4, num_short_dt=4, num_particles=33, max_iter=3,
                                                                                      max_no_improvement_iter=3)
    model = synthetic_hexa()
    B, n = 3, 2
    x0, xref, keys = episodes(cfg, B, 76)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE[:, 1:4], disturbance=disturbance(T7, 1), u_act_in=motor_state(B, 6), rate_loop=rate_loop("stiff"))
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    assert got[1].shape == (B, T7, 6) and got[6].shape == (B, 6) and got[7].shape == (B, T7, 4)
    same(got, ref(cfg, model, x0, xref, keys, T7, **kw))
    S.close()


def test_asymmetric_three_motors_with_a_full_mixer():
    """m = 3: pairwise distinct input bounds, a thrust sum of three terms times float32(1) / float32(3), and a mixer without any symmetry."""
    cfg = asymmetric_cfg(3, horizon=4, num_short_dt=4, num_particles=33, max_iter=3, max_no_improvement_iter=3)
    A = asymmetric_model(3)
    B, n = 3, 2
    x0, xref, keys = episodes(cfg, B, 77)
    rng = np.random.default_rng(3)
    pl = [asymmetric_model(3, seed=23)] + [A.perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, moment=0.2, sigma=0.2, residual=0.2) for _ in range(2)]
    S = SdeMpcSolver(cfg, A, max_batch=B)
    for rl in (rate_loop("stiff", mixer=full_mixer(3), motor_weight=0.35), rate_loop("windup")):          # ... and the model's own rate_mixer()
        kw = dict(timing(n), plant=pl, plant_of=SCHEDULE[:, 1:4], disturbance=disturbance(T7, B), rate_loop=rl)
        got = S.closed_loop(x0, xref, keys, T7, **kw)
        S.solve_status()
        same(got, ref(cfg, A, x0, xref, keys, T7, **kw))
    S.close()


def test_continuation_carries_all_five_state_items():
    cfg = small_cfg()
    model = synthetic_iris()
    B, n, T = 3, 3, 12
    x0, _, keys = episodes(cfg, B, 78)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B)]) for j in range(4)])      # one window per solve
    pl = perturbed_plants(model, 3)
    w = disturbance(T, B)
    rl = rate_loop("windup")
    kw = dict(timing(n), plant=pl, rate_loop=rl)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    full = S.closed_loop(x0, xref, keys, T, disturbance=w, u_act_in=motor_state(B, 4), **kw)
    a = S.closed_loop(x0, xref[:2], keys, 6, disturbance=w[:6], u_act_in=motor_state(B, 4), **kw)
    b = S.closed_loop(a[0][:, -1], xref[2:], a[5], 6, disturbance=w[6:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6], rate_integ_in=a[8], rate_tail_in=a[9], **kw)
    S.solve_status()
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), np.concatenate([a[1], b[1]], 1), np.concatenate([a[2], b[2]], 1)) + tuple(b[3:7]) + \
        (np.concatenate([a[7], b[7]], 1),) + tuple(b[8:])
    same(joined, full)
    same(full, ref(cfg, model, x0, xref, keys, T, disturbance=w, u_act_in=motor_state(B, 4), **kw))
    # dropping either rate item breaks the continuation (solve_delay > 0: the tail is read)
    c = S.closed_loop(a[0][:, -1], xref[2:], a[5], 6, disturbance=w[6:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6], rate_tail_in=a[9], **kw)
    d = S.closed_loop(a[0][:, -1], xref[2:], a[5], 6, disturbance=w[6:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6], rate_integ_in=a[8], **kw)
    assert bits_differ(c[0], b[0]) > 0 and bits_differ(d[0], b[0]) > 0
    S.close()


def test_chunk_boundaries_do_not_change_a_bit():
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 1: one period per chunk, so T = 7 at S = 3 is three chunks; the integrator and the rate tail cross them on the device."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, _, keys = episodes(cfg, B5, 79)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B5)]) for j in range(3)])
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4), rate_loop=rate_loop("windup"),
              rate_integ_in=integ_state(B5), rate_tail_in=rate_tail(B5, 4))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    whole = S.closed_loop(x0, xref, keys, T7, **kw)
    S.set_option("test_loop_chunk_bytes", 1)
    cut = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(cut, whole)
    same(whole, ref(cfg, model, x0, xref, keys, T7, **kw))
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 80)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), rate_loop=rate_loop("stiff"))       # (rate state defaulted: zeros, not poison)
    fresh = SdeMpcSolver(cfg, model, max_batch=B5)
    want = fresh.closed_loop(x0, xref, keys, T7, **kw)
    fresh.close()
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    S.closed_loop(x0[:2], xref[:, :2], keys[:2], 4, plant=pl[:2], plant_substeps=2, solve_period=2, rate_loop=rate_loop("windup"),
                  rate_integ_in=integ_state(2), rate_tail_in=rate_tail(2, 4))                                                     # another B and another state first
    S.closed_loop(x0, xref, keys, T7, **{k: v for k, v in kw.items() if k != "rate_loop"})                                           # ... and the scenario route
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, want)
    same(S.closed_loop(x0, xref, keys, T7, **kw), want)
    same(want, ref(cfg, model, x0, xref, keys, T7, **kw))
    S.close()


@pytest.mark.parametrize("B", [1, B5])
def test_c_entry_point_with_a_transparent_rate_loop_is_the_timed_one(B):
    """kp = ki = 0, motor_weight = 1, no scenario (a NULL scenario cfg): the timed entry point's seven outputs exactly. B = 5: the ragged last workgroup of four."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B, 81)
    pl = perturbed_plants(model, 3)[:min(B, 3)]
    of = np.array([0, 1, 2, 1, 0], np.int32)[:B]
    ua = motor_state(B, 4)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    want = S.closed_loop(x0, xref, keys, T7, plant=pl, plant_of=of, u_act_in=ua, **timing(n))
    H, m = cfg.horizon, 4
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    out = (np.zeros((B, T7 + 1, 13), np.float32), np.zeros((B, T7, m), np.float32), np.zeros((B, 3, 8), np.float32), np.zeros((B, H, m), np.float32),
           np.zeros(B, np.float32), np.zeros((B, 2), np.uint32), np.zeros((B, m), np.float32))
    ws, gn, tn = np.zeros((B, T7, 4), np.float32), np.full((B, 3), 7.0, np.float32), np.zeros((B, H, 3), np.float32)
    blobs = [p.to_blob() for p in pl]
    bufs = (C.c_char_p * len(blobs))(*blobs)
    sizes = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    rc_ = _abi.SdempcRateCfg()
    rc_.struct_size = C.sizeof(rc_)
    rc_.motor_weight = 1.0
    for a in range(3):
        rc_.integ_limit[a] = 1.0
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S3, n + 1, ALPHA)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), len(blobs), n, 0.0, -1, -1)
    xr = np.ascontiguousarray(xref, np.float32)
    rc = _abi.rate_entry(S.lib)(S._h, C.byref(rc_), None, C.byref(tc), C.byref(pc), C.cast(bufs, C.POINTER(C.c_void_p)), sizes, of.ctypes.data_as(C.POINTER(C.c_int32)),
                                B, T7, x0.ctypes.data_as(fp), xr.ctypes.data_as(fp), xr.shape[0], xr.shape[1], keys.ctypes.data_as(u32p), None, None,
                                ua.ctypes.data_as(fp), out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp), out[2].ctypes.data_as(C.POINTER(_abi.SdempcInfo)),
                                out[3].ctypes.data_as(fp), out[4].ctypes.data_as(fp), out[5].ctypes.data_as(u32p), out[6].ctypes.data_as(fp),
                                None, None, ws.ctypes.data_as(fp), gn.ctypes.data_as(fp), tn.ctypes.data_as(fp))
    assert rc == 0, S.lib.sdempc_last_error(S._h).decode()
    S.solve_status()
    same(out, want, names=NAMES[:7])
    assert not gn.any() and np.abs(tn).max() > 0 and np.abs(ws[..., 0]).min() > 0       # zero gains: the integrator stays at its zero start; tail and setpoints are written
    S.close()
