"""Batched closed loop against a separate plant on the GPU (SPEC.md §11a, sdempc_closed_loop_batch_plant): bit for bit against the CPU reference
of tests/plant_loop_ref.py (a composition of the oracle's solve and step) — own model against the plain loop, shared and per-episode perturbed
plants, substeps, an explicit step length, a plant arithmetic pinned apart from the controller's, plant_of with repeats, every solve layout,
continuation, diverging episodes, a ticketed batch and MpcProblem.simulate. Episodes are sampled for the CPU reference only where the oracle's
speed demands it (layouts, ticketed batch): the sample always holds the first and the last episode and every sampled episode must match."""
import numpy as np
import pytest

from cases import bits_differ, diverging_single_rotor_case
from loop_cases import ARITH
from plant_loop_ref import plant_loop_ref
from sde4mbrl_px4_amd import prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver
from test_gpu_closed_loop import LAYOUTS, assert_same, episodes, small_cfg

pytestmark = pytest.mark.gpu

AMOUNTS = dict(mass=0.2, inertia=0.2, thrust=0.2, residual=0.2)


def perturbed_plants(model, n, seed=1):
    rng = np.random.default_rng(seed)
    return [model.perturbed(rng, **AMOUNTS) for _ in range(n)]


@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_own_model_is_the_plain_closed_loop(mlp_dtype, math_mode):
    cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    B, T = 3, 5
    x0, xref, keys = episodes(cfg, B, 20)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    plain = S.closed_loop(x0, xref, keys, T)
    assert_same(S.closed_loop(x0, xref, keys, T, plant=model), plain)
    assert_same(S.closed_loop(x0, xref, keys, T, plant=[model] * B), plain)          # per-episode path, the same model thrice
    S.solve_status()
    S.close()


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("mlp_dtype,math_mode", ARITH)
def test_perturbed_plants_match_reference(mlp_dtype, math_mode, n):
    cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    B, T = 3, 5
    x0, xref, keys = episodes(cfg, B, 20)
    plants = perturbed_plants(model, B)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    one = S.closed_loop(x0, xref, keys, T, plant=plants[0], plant_substeps=n)
    assert_same(one, plant_loop_ref(cfg, model, plants[0], x0, xref, keys, T, substeps=n))
    per = S.closed_loop(x0, xref, keys, T, plant=plants, plant_substeps=n)
    assert_same(per, plant_loop_ref(cfg, model, plants, x0, xref, keys, T, substeps=n))
    S.solve_status()
    assert np.isfinite(per[0]).all() and per[0][:, 0].tobytes() == x0.tobytes()
    assert bits_differ(per[0], S.closed_loop(x0, xref, keys, T)[0]) > 0               # the plants are not the model
    S.close()


def test_explicit_step_length():
    cfg = small_cfg(mlp_dtype="f32x3", math_mode="fast")
    model = synthetic_iris()
    B, T, n, dt = 3, 4, 3, 0.0137                                                      # 3 x 0.0137 is not dt_0 = 0.05
    x0, xref, keys = episodes(cfg, B, 21)
    plants = perturbed_plants(model, B, seed=2)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T, plant=plants, plant_substeps=n, plant_dt=dt)
    assert_same(got, plant_loop_ref(cfg, model, plants, x0, xref, keys, T, substeps=n, dt=dt))
    assert bits_differ(got[0], S.closed_loop(x0, xref, keys, T, plant=plants, plant_substeps=n)[0]) > 0
    S.close()


def test_two_controller_arithmetics_on_one_plant():
    """The comparison the feature exists for: two controllers, one and the same vehicle (f32 / exact), each bit for bit its reference."""
    model = synthetic_iris()
    B, T = 3, 5
    plants = perturbed_plants(model, B)
    runs = []
    for mlp_dtype, math_mode in (("f32x3", "fast"), ("f32", "exact")):
        cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
        x0, xref, keys = episodes(cfg, B, 20)
        S = SdeMpcSolver(cfg, model, max_batch=B)
        got = S.closed_loop(x0, xref, keys, T, plant=plants, plant_substeps=2, plant_mlp_dtype="f32", plant_math_mode="exact")
        assert_same(got, plant_loop_ref(cfg, model, plants, x0, xref, keys, T, substeps=2, mlp_dtype="f32", math_mode="exact"))
        shared = S.closed_loop(x0, xref, keys, T, plant=plants[1], plant_mlp_dtype="f32", plant_math_mode="exact")
        assert_same(shared, plant_loop_ref(cfg, model, plants[1], x0, xref, keys, T, mlp_dtype="f32", math_mode="exact"))
        runs.append(got)
        S.close()
    assert bits_differ(runs[0][0], runs[1][0]) > 0 and np.array_equal(runs[0][5], runs[1][5])


def test_plant_of_with_repeats_and_permuted_blobs():
    cfg = small_cfg(num_particles=40)
    model = synthetic_iris()
    B, T = 5, 3
    x0, xref, keys = episodes(cfg, B, 22)
    pa, pb = perturbed_plants(model, 2)
    of = np.array([0, 1, 1, 0, 1], np.int32)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    want = S.closed_loop(x0, xref, keys, T, plant=[(pa, pb)[i] for i in of], plant_substeps=2)
    assert_same(S.closed_loop(x0, xref, keys, T, plant=[pa, pb], plant_of=of, plant_substeps=2), want)
    assert_same(S.closed_loop(x0, xref, keys, T, plant=[pb, pa], plant_of=1 - of, plant_substeps=2), want)
    assert_same(want, plant_loop_ref(cfg, model, [pa, pb], x0, xref, keys, T, plant_of=of, substeps=2))
    assert bits_differ(want[0][0], want[0][1]) > 0
    S.close()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_per_episode_plants_in_every_layout(name):
    B, P, opts = LAYOUTS[name]
    cfg = small_cfg(num_particles=P)
    model = synthetic_iris()
    T = 4
    x0, xref, keys = episodes(cfg, B, 30)
    plants = perturbed_plants(model, B)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
    got = S.closed_loop(x0, xref, keys, T, plant=plants, plant_substeps=2)
    S.solve_status()
    kname = S.last_kernel_name()
    assert ("spec" in kname) == (name == "spec"), kname
    sample = [0, B - 1] if B > 2 else list(range(B))
    want = plant_loop_ref(cfg, model, plants, x0, xref, keys, T, substeps=2, episodes=sample)
    assert_same(got, want, eps=sample)
    S.close()


def test_plant_loop_continues():
    cfg = small_cfg(num_particles=40)
    model = synthetic_iris()
    B = 3
    x0, xref, keys = episodes(cfg, B, 60)
    plants = perturbed_plants(model, B)
    kw = dict(plant=plants, plant_substeps=4)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    full = S.closed_loop(x0, xref, keys, 7, **kw)
    a = S.closed_loop(x0, xref, keys, 3, **kw)
    b = S.closed_loop(a[0][:, -1], xref, a[5], 4, u_init=a[3], stepsize_in=a[4], **kw)
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), np.concatenate([a[1], b[1]], 1), np.concatenate([a[2], b[2]], 1)) + tuple(b[3:])
    assert_same(joined, full)
    S.close()


def test_diverging_episodes_with_a_perturbed_plant():
    cfg, model, x0, xref, noise, u = diverging_single_rotor_case()
    B, T = x0.shape[0], 3
    keys = np.stack([prng.PRNGKey(300 + b) for b in range(B)])
    plant = model.perturbed(np.random.default_rng(4), **AMOUNTS)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref[None], keys, T, u_init=u, plant=plant, plant_substeps=2)
    S.solve_status()
    assert_same(got, plant_loop_ref(cfg, model, plant, x0, xref[None], keys, T, substeps=2, u_init=u))
    assert (~np.isfinite(got[2][:2])).any()                                # the diverging episodes did meet non-finite values
    alone = S.closed_loop(x0[2:], xref[None, 2:], keys[2:], T, u_init=u[2:], plant=plant, plant_substeps=2)
    assert_same(alone, tuple(g[2:] for g in got))
    assert np.isfinite(alone[0]).all()
    S.close()


def test_per_episode_plants_at_ticketed_batch_size():
    cfg = small_cfg(num_particles=40, max_iter=2, max_no_improvement_iter=2)
    model = synthetic_iris()
    B, T = 4700, 3
    x0 = W.random_initial_states(B, 70)
    xref = W.reference_window(0.0, cfg.time_steps)
    keys = prng.split(prng.PRNGKey(11), B)
    plants = perturbed_plants(model, B, seed=7)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T, plant=plants, plant_substeps=2)
    assert ", false, 3, " in S.last_kernel_name() and 3 * 6 * S.get_option("device_cus") <= B      # persistent, ticketed
    S.solve_status()
    sample = sorted(set([0] + np.random.default_rng(5).choice(B, 3, replace=False).tolist() + [B - 1]))
    want = plant_loop_ref(cfg, model, [plants[i] for i in sample], x0[sample], xref, keys[sample], T, substeps=2)
    assert_same(tuple(g[sample] for g in got), want)
    S.close()


def test_simulate_with_a_plant_is_closed_loop_in_the_solver_frame():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    cfg = small_cfg(num_particles=1)
    model = synthetic_iris()
    plant = model.perturbed(np.random.default_rng(6), **AMOUNTS)
    T = 5
    x = W.random_initial_states(1, 80)[0]
    rng = prng.PRNGKey(81)
    prob = MpcProblem(cfg=cfg, model=model, state_from_traj=W.lemniscate_state)
    xs, us, info, st, rng_T = prob.simulate(x, rng, T, curr_t=0.4, plant=plant, plant_substeps=4)
    assert xs.shape == (T + 1, 13) and xs[0].tobytes() == x.tobytes()
    xsol = enu2ned(x, np)
    xref = np.stack([prob.xref(0.4 + k * float(cfg.time_steps[0]), xsol) for k in range(T)])[:, None]
    S = SdeMpcSolver(cfg, model, max_batch=1)
    g = S.closed_loop(xsol[None], xref, rng[None], T, plant=plant, plant_substeps=4)
    assert bits_differ(xs[1:], enu2ned(g[0][0, 1:], np)) == 0 and bits_differ(us, g[1][0]) == 0 and bits_differ(info, g[2][0]) == 0
    assert bits_differ(st.yk, g[3][0]) == 0 and st.stepsize == g[4][0] and np.array_equal(rng_T, g[5][0])
    assert bits_differ(g[0], S.closed_loop(xsol[None], xref, rng[None], T)[0]) > 0
    assert_same(g, plant_loop_ref(cfg, model, plant, xsol[None], xref, rng[None], T, substeps=4))
    S.close()
