"""Batched closed loop at the node's timing on the GPU (SPEC.md §11b, sdempc_closed_loop_batch_timed): bit for bit against the CPU reference of
tests/timed_loop_ref.py (a composition of the oracle's solve and step with float32 arithmetic for the motor lag). Shapes: H = 4 with S = 3 (the
shift clamp fires; at H = 2 the command-row clamp fires too), T = 7 (a partial last period), B = 5 (a partly empty last workgroup), P in {1, 33},
n in {1, 3}, every kind of arrival point, shared and per-episode plants, both lag values, every arithmetic, every solve layout, continuation."""
import functools
import os

import numpy as np
import pytest

import loop_cases
from cases import CDIR, bits_differ
from loop_cases import ARITH, NAMES
from sde4mbrl_px4_amd import load_mpc_config, prng, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver
from test_gpu_closed_loop import LAYOUTS, episodes
from timed_loop_ref import lag_step, num_solves, timed_loop_ref

pytestmark = pytest.mark.gpu

AMOUNTS = dict(mass=0.2, inertia=0.2, thrust=0.2, residual=0.2)
S3, T7 = 3, 7
same = functools.partial(loop_cases.same, names=NAMES[:7])


def small_cfg(**kw):
    c1 = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml"))
    return c1.replace(**{"horizon": 4, "num_short_dt": 4, "num_particles": 33, "max_iter": 3, "max_no_improvement_iter": 3, **kw})


def perturbed_plants(model, n, seed=1):
    rng = np.random.default_rng(seed)
    return [model.perturbed(rng, **AMOUNTS) for _ in range(n)]


def motor_state(B, m, seed=9, lo=0.55, hi=0.85):
    return np.random.default_rng(seed).uniform(lo, hi, (B, m)).astype(np.float32)


@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_period_one_no_delay_no_lag_is_the_existing_loop(mlp_dtype, math_mode):
    """S = 1, D = 0, alpha = 0 through the new entry point (u_act_in given, which the lag being off ignores) is §11a word for word, and §11 with
    the handle's own model."""
    cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    B, T, n = 5, 4, 3
    x0, xref, keys = episodes(cfg, B, 20)
    plants = perturbed_plants(model, B)
    ua = motor_state(B, 4)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    for kw in (dict(plant=plants, plant_substeps=n), dict(plant=plants[2], plant_substeps=n), dict()):
        old = S.closed_loop(x0, xref, keys, T, **kw)
        new = S.closed_loop(x0, xref, keys, T, u_act_in=ua, **kw)
        assert len(old) == 6 and len(new) == 7
        loop_cases.same(new[:6], old, names=NAMES[:6])
        assert bits_differ(new[6], old[1][:, -1]) == 0
    S.solve_status()
    S.close()


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("P,n,H", [(1, 1, 4), (33, 3, 4), (1, 2, 2)])       # (H = 2: the command row min(i, H - 1) clamps inside a period of three ticks)
def test_every_arrival_point_matches_reference(P, n, H, per_episode):
    cfg = small_cfg(num_particles=P, horizon=H, num_short_dt=H)
    model = synthetic_iris()
    B = 5
    x0, xref, keys = episodes(cfg, B, 21)
    pl = perturbed_plants(model, 3)
    kw = dict(plant=pl, plant_of=np.array([0, 1, 2, 1, 0], np.int32)) if per_episode else dict(plant=pl[1])
    rkw = dict(plants=pl, plant_of=kw["plant_of"]) if per_episode else dict(plants=pl[1])
    S = SdeMpcSolver(cfg, model, max_batch=B)
    runs = {}
    for D in sorted({0, 1, n, n + 1, S3 * n}):           # at once, one substep late, a tick late, mid-tick, never inside its own period
        got = S.closed_loop(x0, xref, keys, T7, plant_substeps=n, solve_period=S3, solve_delay=D, **kw)
        S.solve_status()
        assert got[2].shape == (B, num_solves(T7, S3), 8)
        same(got, timed_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T7, S=S3, D=D, substeps=n, **rkw))
        assert np.isfinite(got[0]).all() and got[0][:, 0].tobytes() == x0.tobytes()
        runs[D] = got
    assert bits_differ(runs[0][0], runs[n + 1][0]) > 0 and bits_differ(runs[0][1], runs[n + 1][1]) > 0       # the delay is not ignored
    assert bits_differ(runs[0][0], runs[S3 * n][0]) > 0
    assert np.array_equal(runs[0][5], runs[n + 1][5])                                                          # the key schedule is S and T only
    S.close()


@pytest.mark.parametrize("alpha", [0.35, 1.0])
def test_motor_lag_matches_reference(alpha):
    cfg = small_cfg()
    model = synthetic_iris()
    B, n = 5, 3
    x0, xref, keys = episodes(cfg, B, 22)
    plants = perturbed_plants(model, B)
    # motors that start almost at rest: while c > 2 a the subtraction c - a rounds, so (c - a) + a != c and alpha = 1 is not "off"
    # (within a factor of two of the command both operations are exact, and alpha = 1 would reproduce the bits of the lag being off)
    ua = motor_state(B, 4, lo=0.001, hi=0.05)
    uref = np.asarray(cfg.uref, np.float32)[:4]
    assert (lag_step(ua, np.tile(uref, (B, 1)), 1.0) != uref).any()
    S = SdeMpcSolver(cfg, model, max_batch=B)
    kw = dict(plant=plants, plant_substeps=n, solve_period=S3, solve_delay=n + 1)
    got = S.closed_loop(x0, xref, keys, T7, motor_lag=alpha, u_act_in=ua, **kw)
    same(got, timed_loop_ref(cfg, model, plants, x0, xref, keys, T7, S=S3, D=n + 1, alpha=alpha, substeps=n, u_act_in=ua))
    off = S.closed_loop(x0, xref, keys, T7, u_act_in=ua, **kw)
    same(off, timed_loop_ref(cfg, model, plants, x0, xref, keys, T7, S=S3, D=n + 1, substeps=n, u_act_in=ua))
    # the lag is not ignored; alpha = 1 is (c - a) + a in float32, which is not c on these inputs
    assert bits_differ(got[0], off[0]) > 0 and bits_differ(got[1], off[1]) > 0
    # without u_act_in the motor state starts at the warm start's first row
    dflt = S.closed_loop(x0, xref, keys, T7, motor_lag=alpha, **kw)
    same(dflt, timed_loop_ref(cfg, model, plants, x0, xref, keys, T7, S=S3, D=n + 1, alpha=alpha, substeps=n))
    S.solve_status()
    S.close()


def test_hexa_six_motors():
    cfg = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(horizon=4, num_short_dt=4, num_particles=33, max_iter=3,
                                                                                      max_no_improvement_iter=3)
    model = synthetic_hexa()
    B, n = 3, 2
    x0, xref, keys = episodes(cfg, B, 23)
    plants = perturbed_plants(model, B)
    ua = motor_state(B, 6)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T7, plant=plants, plant_substeps=n, solve_period=S3, solve_delay=n + 1, motor_lag=0.35, u_act_in=ua)
    assert got[1].shape == (B, T7, 6) and got[6].shape == (B, 6)
    same(got, timed_loop_ref(cfg, model, plants, x0, xref, keys, T7, S=S3, D=n + 1, alpha=0.35, substeps=n, u_act_in=ua))
    S.close()


def test_plant_arithmetic_pinned_apart_from_the_controllers():
    cfg = small_cfg(mlp_dtype="f32x3", math_mode="fast")
    model = synthetic_iris()
    B, n = 3, 2
    x0, xref, keys = episodes(cfg, B, 24)
    plants = perturbed_plants(model, B)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    kw = dict(plant_substeps=n, solve_period=S3, solve_delay=1, motor_lag=0.35)
    got = S.closed_loop(x0, xref, keys, T7, plant=plants, plant_mlp_dtype="f32", plant_math_mode="exact", **kw)
    same(got, timed_loop_ref(cfg, model, plants, x0, xref, keys, T7, S=S3, D=1, alpha=0.35, substeps=n, mlp_dtype="f32", math_mode="exact"))
    assert bits_differ(got[0], S.closed_loop(x0, xref, keys, T7, plant=plants, **kw)[0]) > 0
    S.close()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_solve_layout(name):
    B, P, opts = LAYOUTS[name]
    cfg = small_cfg(num_particles=P, horizon=10, num_short_dt=10)
    model = synthetic_iris()
    T, Sp, n = 6, 2, 2
    x0, xref, keys = episodes(cfg, B, 30)
    plants = perturbed_plants(model, B)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
    got = S.closed_loop(x0, xref, keys, T, plant=plants, plant_substeps=n, solve_period=Sp, solve_delay=n + 1, motor_lag=0.35)
    S.solve_status()
    kname = S.last_kernel_name()
    assert ("spec" in kname) == (name == "spec"), kname
    sample = [0, B - 1] if B > 2 else list(range(B))
    want = timed_loop_ref(cfg, model, plants, x0, xref, keys, T, S=Sp, D=n + 1, alpha=0.35, substeps=n, episodes=sample)
    same(got, want, eps=sample)
    S.close()


def test_continuation_at_a_multiple_of_the_period():
    cfg = small_cfg()
    model = synthetic_iris()
    B, n = 3, 3
    x0, _, keys = episodes(cfg, B, 25)
    xref = np.stack([np.stack([W.reference_window(0.15 * j + 0.1 * b, cfg.time_steps) for b in range(B)]) for j in range(2)])      # one window per solve
    plants = perturbed_plants(model, B)
    ua = motor_state(B, 4)
    kw = dict(plant=plants, plant_substeps=n, solve_period=S3, solve_delay=n + 1, motor_lag=0.35)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    full = S.closed_loop(x0, xref, keys, 6, u_act_in=ua, **kw)
    a = S.closed_loop(x0, xref[:1], keys, 3, u_act_in=ua, **kw)
    b = S.closed_loop(a[0][:, -1], xref[1:], a[5], 3, u_init=a[3], stepsize_in=a[4], u_act_in=a[6], **kw)
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), np.concatenate([a[1], b[1]], 1), np.concatenate([a[2], b[2]], 1)) + tuple(b[3:])
    same(joined, full)
    same(full, timed_loop_ref(cfg, model, plants, x0, xref, keys, 6, S=S3, D=n + 1, alpha=0.35, substeps=n, u_act_in=ua))
    S.close()


def test_episode_zero_does_not_depend_on_the_batch():
    cfg = small_cfg()
    model = synthetic_iris()
    B, n = 5, 3
    x0, xref, keys = episodes(cfg, B, 26)
    plants = perturbed_plants(model, B)
    ua = motor_state(B, 4)
    kw = dict(plant_substeps=n, solve_period=S3, solve_delay=n + 1, motor_lag=0.35)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    five = S.closed_loop(x0, xref, keys, T7, plant=plants, u_act_in=ua, **kw)
    one = S.closed_loop(x0[:1], xref[:, :1], keys[:1], T7, plant=plants[:1], u_act_in=ua[:1], **kw)
    same(one, tuple(g[:1] for g in five))
    S.close()


def test_poisoned_workspace_gives_the_same_bits():
    cfg = small_cfg()
    model = synthetic_iris()
    B, n = 5, 3
    x0, xref, keys = episodes(cfg, B, 27)
    plants = perturbed_plants(model, 2)
    of = np.array([0, 1, 1, 0, 1], np.int32)
    kw = dict(plant=plants, plant_of=of, plant_substeps=n, solve_period=S3, solve_delay=n + 1, motor_lag=0.35)
    runs = []
    for opts in ({}, {"test_ws_fill": 255}):
        S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
        runs.append(S.closed_loop(x0, xref, keys, T7, **kw))
        runs.append(S.closed_loop(x0, xref, keys, T7, **kw))           # and a second call on the same handle
        S.solve_status()
        S.close()
    for r in runs[1:]:
        same(r, runs[0])


def test_simulate_at_the_nodes_timing():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    cfg = small_cfg(num_particles=1)
    model = synthetic_iris()
    plant = model.perturbed(np.random.default_rng(6), **AMOUNTS)
    T, Sp, n = 5, 2, 2
    x = W.random_initial_states(1, 80)[0]
    rng = prng.PRNGKey(81)
    prob = MpcProblem(cfg=cfg, model=model, state_from_traj=W.lemniscate_state)
    xs, us, info, st, rng_T = prob.simulate(x, rng, T, curr_t=0.4, plant=plant, plant_substeps=n, solve_period=Sp, solve_delay=1)
    assert xs.shape == (T + 1, 13) and xs[0].tobytes() == x.tobytes() and info.shape == (3, 8)
    xsol = enu2ned(x, np)
    xref = np.stack([prob.xref(0.4 + j * Sp * float(cfg.time_steps[0]), xsol) for j in range(3)])[:, None]
    want = timed_loop_ref(cfg, model, plant, xsol[None], xref, rng[None], T, S=Sp, D=1, substeps=n)
    assert bits_differ(xs[1:], enu2ned(want[0][0, 1:], np)) == 0 and bits_differ(us, want[1][0]) == 0 and bits_differ(info, want[2][0]) == 0
    assert bits_differ(st.yk, want[3][0]) == 0 and st.stepsize == want[4][0] and np.array_equal(rng_T, want[5][0])
    plain = prob.simulate(x, rng, T, curr_t=0.4, plant=plant, plant_substeps=n)
    assert bits_differ(xs, plain[0]) > 0 and plain[2].shape == (T, 8)
