"""Batched closed loop with a scenario on the GPU (SPEC.md §11c, sdempc_closed_loop_batch_scenario): bit for bit against the CPU reference of
tests/scenario_loop_ref.py (the oracle's solve and step, the exact software fma for the lag and the disturbance). Shapes of
tests/test_gpu_timed_loop.py: H = 4 with S = 3, T = 7 (a partial last period), B = 5 (a partly empty last workgroup), P in {1, 33}, n in {1, 3},
D = n + 1, alpha = 0.35; every shape of the disturbance tensor, a plant schedule with every kind of switch, every arithmetic, every solve layout,
continuation, chunk boundaries, a handle with a past, simulate's frame conversion and the C entry point with both schedules absent."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loop_cases
from cases import CDIR, bits_differ
from loop_cases import ARITH, NAMES
from scenario_cases import ALPHA, B5, S3, SCHEDULE, T7, disturbance, episodes, motor_state, perturbed_plants, small_cfg, switch_ticks
from scenario_loop_ref import scenario_loop_ref
from sde4mbrl_px4_amd import _abi, load_mpc_config, prng, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver
from test_gpu_asymmetric import asymmetric_cfg, asymmetric_model
from test_gpu_closed_loop import LAYOUTS

pytestmark = pytest.mark.gpu

same = functools.partial(loop_cases.same, names=NAMES[:7])
ref = functools.partial(loop_cases.ref, scenario_loop_ref)


def timing(n):
    return dict(plant_substeps=n, solve_period=S3, solve_delay=n + 1, motor_lag=ALPHA)


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("P,n,H", [(1, 1, 4), (33, 3, 4), (1, 3, 2)])
def test_disturbance_matches_reference(P, n, H, per_episode):
    """Every shape of the disturbance tensor, (Td, Bd) in {1, T} x {1, B}, and the [T][6] / [6] forms of the Python layer."""
    cfg = small_cfg(num_particles=P, horizon=H, num_short_dt=H)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 41)
    pl = perturbed_plants(model, 3)
    kw = dict(plant=pl, plant_of=np.array([0, 1, 2, 1, 0], np.int32)) if per_episode else dict(plant=pl[1])
    kw.update(timing(n), u_act_in=motor_state(B5, 4))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    calm = S.closed_loop(x0, xref, keys, T7, **kw)
    shapes = [(Td, Bd) for Td in (1, T7) for Bd in (1, B5)] if H == 4 else [(T7, B5)]
    for Td, Bd in shapes:
        w = disturbance(Td, Bd)
        got = S.closed_loop(x0, xref, keys, T7, disturbance=w, **kw)
        S.solve_status()
        same(got, ref(cfg, model, x0, xref, keys, T7, disturbance=w, **kw))
        assert np.isfinite(got[0]).all() and got[0][:, 0].tobytes() == x0.tobytes()
        assert bits_differ(got[0][:, 1:], calm[0][:, 1:]) > 0                      # the disturbance is not ignored
        assert np.array_equal(got[5], calm[5])                                     # the key schedule is S and T only
        if Bd == 1:                                                                # the shorthand forms are the full tensor
            short = S.closed_loop(x0, xref, keys, T7, disturbance=w[:, 0] if Td > 1 else w[0, 0], **kw)
            same(short, got)
    S.close()


def test_plant_schedule_matches_reference():
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 42)
    pl = perturbed_plants(model, 3)
    sw = switch_ticks(SCHEDULE)
    assert any(k % S3 for k, _ in sw) and any(k % S3 == 0 for k, _ in sw)                      # switches inside a period and at period starts
    assert (SCHEDULE[:, 0] == SCHEDULE[0, 0]).all() and (np.diff(SCHEDULE[:, 1]) != 0).all()   # one episode never switches, one on every tick
    assert SCHEDULE[0, 4] == SCHEDULE[-1, 4] != SCHEDULE[2, 4]                                 # one returns to an earlier blob
    kw = dict(timing(n), u_act_in=motor_state(B5, 4))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, plant=pl, plant_of=SCHEDULE, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, plant=pl, plant_of=SCHEDULE, **kw))
    # the switch is not ignored: the episodes that switch leave the run that stays on the first tick's plants, the one that never switches does not
    stay = S.closed_loop(x0, xref, keys, T7, plant=pl, plant_of=SCHEDULE[0], **kw)
    assert bits_differ(got[0][0], stay[0][0]) == 0
    for b in range(1, B5):
        assert bits_differ(got[0][b], stay[0][b]) > 0, b
    # a permuted set with remapped indices gives the same bits, and so does a set with a blob listed twice
    perm = np.array([2, 0, 1])                                                                  # new position of old plant p
    same(S.closed_loop(x0, xref, keys, T7, plant=[pl[1], pl[2], pl[0]], plant_of=perm[SCHEDULE].astype(np.int32), **kw), got)
    dup = np.where(SCHEDULE == 0, 3, SCHEDULE).astype(np.int32)
    dup[0] = SCHEDULE[0]
    same(S.closed_loop(x0, xref, keys, T7, plant=pl + [pl[0]], plant_of=dup, **kw), got)
    # a one-row schedule is the 1-D plant_of through the timed entry point
    one_d = S.closed_loop(x0, xref, keys, T7, plant=pl, plant_of=SCHEDULE[3], **kw)
    same(S.closed_loop(x0, xref, keys, T7, plant=pl, plant_of=SCHEDULE[3:4], **kw), one_d)
    S.solve_status()
    S.close()


def test_one_episode_dropping_a_payload():
    """B = 1 with Np = 2: more plants than episodes, which only a schedule allows."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, 1, 43)
    pl = perturbed_plants(model, 2)
    of = np.array([0, 0, 0, 0, 1, 1, 1], np.int32)[:, None]
    kw = dict(timing(n), plant=pl)
    S = SdeMpcSolver(cfg, model, max_batch=1)
    got = S.closed_loop(x0, xref, keys, T7, plant_of=of, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, plant_of=of, **kw))
    kept = S.closed_loop(x0, xref, keys, T7, plant_of=np.zeros((T7, 1), np.int32), **kw)
    assert bits_differ(got[0][:, :5], kept[0][:, :5]) == 0 and bits_differ(got[0][:, 5:], kept[0][:, 5:]) > 0
    S.close()


@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_both_schedules_in_every_arithmetic(mlp_dtype, math_mode):
    cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 44)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, **kw))
    S.close()


def test_plant_arithmetic_pinned_apart_from_the_controllers():
    cfg = small_cfg(mlp_dtype="f32x3", math_mode="fast")
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 45)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    got = S.closed_loop(x0, xref, keys, T7, plant_mlp_dtype="f32", plant_math_mode="exact", **kw)
    S.solve_status()
    same(got, ref(cfg, model, x0, xref, keys, T7, plant_mlp_dtype="f32", plant_math_mode="exact", **kw))
    assert bits_differ(got[0], S.closed_loop(x0, xref, keys, T7, **kw)[0]) > 0
    S.close()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_solve_layout(name):
    B, P, opts = LAYOUTS[name]
    cfg = small_cfg(num_particles=P, horizon=10, num_short_dt=10)
    model = synthetic_iris()
    T, Sp, n = 6, 2, 2
    x0, xref, keys = episodes(cfg, B, 46)
    pl = perturbed_plants(model, 3)
    of = np.random.default_rng(5).integers(0, 3, (T, B)).astype(np.int32)
    kw = dict(plant=pl, plant_of=of, disturbance=disturbance(T, B), plant_substeps=n, solve_period=Sp, solve_delay=n + 1, motor_lag=ALPHA)
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
    x0, xref, keys = episodes(cfg, B, 47)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE[:, 1:4], disturbance=disturbance(T7, 1), u_act_in=motor_state(B, 6))
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    assert got[1].shape == (B, T7, 6) and got[6].shape == (B, 6)
    same(got, ref(cfg, model, x0, xref, keys, T7, **kw))
    S.close()


def test_asymmetric_vehicle():
    cfg = asymmetric_cfg(4, horizon=4, num_short_dt=4, num_particles=33, max_iter=3, max_no_improvement_iter=3)
    A = asymmetric_model(4)
    B, n = 3, 2
    x0, xref, keys = episodes(cfg, B, 48)
    rng = np.random.default_rng(3)
    pl = [asymmetric_model(4, seed=23)] + [A.perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, moment=0.2, sigma=0.2, residual=0.2) for _ in range(2)]
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE[:, 1:4], disturbance=disturbance(T7, B))
    S = SdeMpcSolver(cfg, A, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, ref(cfg, A, x0, xref, keys, T7, **kw))
    S.close()


def test_continuation_with_sliced_schedules():
    cfg = small_cfg()
    model = synthetic_iris()
    B, n, T = 3, 3, 6
    x0, _, keys = episodes(cfg, B, 49)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B)]) for j in range(2)])      # one window per solve
    pl = perturbed_plants(model, 3)
    of, w = SCHEDULE[:T, 1:4], disturbance(T, B)
    kw = dict(timing(n), plant=pl)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    full = S.closed_loop(x0, xref, keys, T, plant_of=of, disturbance=w, u_act_in=motor_state(B, 4), **kw)
    a = S.closed_loop(x0, xref[:1], keys, 3, plant_of=of[:3], disturbance=w[:3], u_act_in=motor_state(B, 4), **kw)
    b = S.closed_loop(a[0][:, -1], xref[1:], a[5], 3, plant_of=of[3:], disturbance=w[3:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6], **kw)
    S.solve_status()
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), np.concatenate([a[1], b[1]], 1), np.concatenate([a[2], b[2]], 1)) + tuple(b[3:])
    same(joined, full)
    same(full, ref(cfg, model, x0, xref, keys, T, plant_of=of, disturbance=w, u_act_in=motor_state(B, 4), **kw))
    S.close()


def test_chunk_boundaries_do_not_change_a_bit():
    """SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 1: one period per chunk, so T = 7 at S = 3 is three chunks (the last one partial), with moving references
    and both schedules staged per chunk."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, _, keys = episodes(cfg, B5, 50)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B5)]) for j in range(3)])
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4))
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    assert S.get_option("test_loop_chunk_bytes") == -1
    whole = S.closed_loop(x0, xref, keys, T7, **kw)
    S.set_option("test_loop_chunk_bytes", 1)
    cut = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(cut, whole)
    same(whole, ref(cfg, model, x0, xref, keys, T7, **kw))
    # ... and the timed entry point under the same option
    tkw = dict(timing(n), plant=pl, plant_of=SCHEDULE[0])
    cut_t = S.closed_loop(x0, xref, keys, T7, **tkw)
    S.set_option("test_loop_chunk_bytes", -1)
    same(cut_t, S.closed_loop(x0, xref, keys, T7, **tkw))
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 51)
    pl = perturbed_plants(model, 3)
    kw = dict(timing(n), plant=pl, plant_of=SCHEDULE, disturbance=disturbance(T7, B5))
    fresh = SdeMpcSolver(cfg, model, max_batch=B5)
    want = fresh.closed_loop(x0, xref, keys, T7, **kw)
    fresh.close()
    S = SdeMpcSolver(cfg, model, max_batch=B5, options={"test_ws_fill": 255})       # (set before the first device call)
    assert not S.device_ready()
    S.closed_loop(x0[:2], xref[:, :2], keys[:2], 4, plant=pl[:2], plant_substeps=2, solve_period=2, disturbance=disturbance(1, 2, seed=8))    # another B first
    got = S.closed_loop(x0, xref, keys, T7, **kw)
    S.solve_status()
    same(got, want)
    same(S.closed_loop(x0, xref, keys, T7, **kw), want)
    S.close()


def test_simulate_converts_the_disturbance_into_the_solver_frame():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    cfg = small_cfg(num_particles=1)
    model = synthetic_iris()
    pl = perturbed_plants(model, 2, seed=6)
    T, Sp, n = 5, 2, 2
    x = W.random_initial_states(1, 80)[0]
    rng = prng.PRNGKey(81)
    w = disturbance(T, 1)[:, 0]
    of = np.array([0, 0, 1, 1, 0], np.int32)
    prob = MpcProblem(cfg=cfg, model=model, state_from_traj=W.lemniscate_state)             # (convert_to_enu is the default)
    assert prob.convert_to_enu
    xs, us, info, st, rng_T = prob.simulate(x, rng, T, curr_t=0.4, plant=pl, plant_substeps=n, solve_period=Sp, solve_delay=1, disturbance=w, plant_of=of)
    assert xs.shape == (T + 1, 13) and xs[0].tobytes() == x.tobytes() and info.shape == (3, 8)
    xsol = enu2ned(x, np)
    xref = np.stack([prob.xref(0.4 + j * Sp * float(cfg.time_steps[0]), xsol) for j in range(3)])[:, None]
    wsol = np.stack([w[:, 1], w[:, 0], -w[:, 2], w[:, 3], -w[:, 4], -w[:, 5]], axis=-1)      # by hand: (x, y, z) -> (y, x, -z), (wx, wy, wz) -> (wx, -wy, -wz)
    got = prob.solver().closed_loop(xsol[None], xref, rng[None], T, plant=pl, plant_of=of[:, None], plant_substeps=n, solve_period=Sp, solve_delay=1,
                                    disturbance=wsol[:, None])
    assert bits_differ(xs[1:], enu2ned(got[0][0, 1:], np)) == 0 and bits_differ(us, got[1][0]) == 0 and bits_differ(info, got[2][0]) == 0
    assert bits_differ(st.yk, got[3][0]) == 0 and np.array_equal(rng_T, got[5][0])
    same(got, scenario_loop_ref(cfg, model, pl, xsol[None], xref, rng[None], T, S=Sp, D=1, substeps=n, plant_of=of[:, None], disturbance=wsol[:, None]))
    calm = prob.simulate(x, rng, T, curr_t=0.4, plant=pl[0], plant_substeps=n, solve_period=Sp, solve_delay=1)
    assert bits_differ(xs, calm[0]) > 0


def test_c_entry_point_with_both_schedules_absent_is_the_timed_one():
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 52)
    pl = perturbed_plants(model, 3)
    of = np.array([0, 1, 2, 1, 0], np.int32)
    ua = motor_state(B5, 4)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    want = S.closed_loop(x0, xref, keys, T7, plant=pl, plant_of=of, u_act_in=ua, **timing(n))
    H, m = cfg.horizon, 4
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    out = (np.zeros((B5, T7 + 1, 13), np.float32), np.zeros((B5, T7, m), np.float32), np.zeros((B5, 3, 8), np.float32), np.zeros((B5, H, m), np.float32),
           np.zeros(B5, np.float32), np.zeros((B5, 2), np.uint32), np.zeros((B5, m), np.float32))
    blobs = [p.to_blob() for p in pl]
    bufs = (C.c_char_p * 3)(*blobs)
    sizes = (C.c_size_t * 3)(*[len(b) for b in blobs])
    sc = _abi.SdempcScenarioCfg(C.sizeof(_abi.SdempcScenarioCfg), None, 0, 0, 1)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S3, n + 1, ALPHA)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), 3, n, 0.0, -1, -1)
    xr = np.ascontiguousarray(xref, np.float32)
    rc = _abi.scenario_entry(S.lib)(S._h, C.byref(sc), C.byref(tc), C.byref(pc), C.cast(bufs, C.POINTER(C.c_void_p)), sizes, of.ctypes.data_as(C.POINTER(C.c_int32)),
                                    B5, T7, x0.ctypes.data_as(fp), xr.ctypes.data_as(fp), xr.shape[0], xr.shape[1], keys.ctypes.data_as(u32p), None, None,
                                    ua.ctypes.data_as(fp), out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp), out[2].ctypes.data_as(C.POINTER(_abi.SdempcInfo)),
                                    out[3].ctypes.data_as(fp), out[4].ctypes.data_as(fp), out[5].ctypes.data_as(u32p), out[6].ctypes.data_as(fp))
    assert rc == 0, S.lib.sdempc_last_error(S._h).decode()
    S.solve_status()
    same(out, want)
    S.close()
