"""GPU parity on vehicles and configurations WITHOUT the symmetries and zeros of the synthetic ones (tests/cases.py: asymmetric_model,
asymmetric_cfg, asymmetric_problem): b3, b3n, ct0 != 0, Jx != Jy, six distinct residual scales and sigma, non-unit rotor_dir, g != 9.81,
per-motor-distinct uref / input bounds / slew bounds, the negated initial quaternion, a 150 degree attitude, warm starts outside every motor's
own bounds. On the synthetic vehicles whole terms of SPEC.md §5 never reach a compared bit; tests/test_asymmetric_cpu.py proves that on
these inputs every entry of the model and of the per-motor settings does. Every comparison is bit for bit against the CPU oracle: rollout
(cost, full trajectory, mean), gradient, solve (uopt, xevol, the eight telemetry words); no tolerances. The last test hands the kernels
mutated parameters and requires that they do NOT equal the oracle: what a kernel that dropped or swapped a parameter would show."""
import contextlib
import functools
import os

import numpy as np
import pytest

import kernel_census as kc
import orc
from cases import asymmetric_cfg, asymmetric_model, asymmetric_mutants, asymmetric_problem, bits_differ
from closed_loop_ref import closed_loop_ref
from plant_loop_ref import plant_loop_ref
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import SdeMpcSolver
from test_gpu_closed_loop import assert_same

pytestmark = pytest.mark.gpu

B = 3
MODE = {"f32": 0, "f16": 1, "f32x3": 2}
ARITH = [(d, mth) for d in ("f32", "f16", "f32x3") for mth in ("exact", "fast")]
H9 = dict(horizon=9, num_short_dt=4, long_step_dt=0.1)                  # both step lengths occur


@contextlib.contextmanager
def oracle_threads():
    """The oracle's particle loops on several cores (same bits at any count)."""
    orc.set_threads(min(os.cpu_count() or 1, 8))
    try:
        yield
    finally:
        orc.set_threads(1)


@functools.lru_cache(maxsize=None)
def _reference(m, mlp, math, P, seed=21):
    """Problem and oracle results of one (vehicle, arithmetic, particle count), computed once and shared by the layouts that run it."""
    cfg = asymmetric_cfg(m, num_particles=P, mlp_dtype=mlp, math_mode=math, **H9)
    model = asymmetric_model(m)
    prob = asymmetric_problem(cfg, B, seed)
    x0, xref, noise, u = prob
    O = orc.Oracle(cfg, model)
    ref = []
    with oracle_threads():
        for b in range(B):
            ref.append((O.rollout(x0[b], u[b], xref[b], noise[b], True, True), O.grad(x0[b], u[b], xref[b], noise[b]),
                        O.solve(x0[b], xref[b], noise[b], u[b], 0.01)[:3]))
    return cfg, model, prob, ref


def _run(cfg, model, prob, options):
    x0, xref, noise, u = prob
    S = SdeMpcSolver(cfg, model, max_batch=B, options=options)
    roll = S.rollout(x0, u, xref, noise, True, True)
    grad = S.grad(x0, u, xref, noise)
    sol = S.solve(x0, xref, noise, u, np.full(B, 0.01, np.float32))
    kname = S.last_kernel_name()
    S.close()
    return roll, grad, sol, kname


@functools.lru_cache(maxsize=None)
def _device_cus():
    cfg, model, prob, _ = _reference(4, "f32", "exact", 1)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    S.rollout(prob[0], prob[3], prob[1], prob[2])
    cus = S.get_option("device_cus")
    S.close()
    return cus


def _check(m, mlp, math, P, options):
    cfg, model, prob, ref = _reference(m, mlp, math, P)
    (cost, traj, xmean), (gc, grad), (uopt, xevol, info), kname = _run(cfg, model, prob, options)
    lo, hi = np.asarray(cfg.input_bound, np.float32).T
    assert np.all(uopt >= lo) and np.all(uopt <= hi) and np.all(info[:, 2] >= 5)           # each motor within ITS bounds; 5 - 6 iterations ran
    for b in range(B):
        (c, t, xm), (c2, g2), (uo, xe, io) = ref[b]
        assert cost[b] == np.float32(c) and bits_differ(traj[b], t) == 0 and bits_differ(xmean[b], xm) == 0, ("rollout", b)
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0, ("grad", b)
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, ("solve", b)
    assert kname.startswith(f"sdempc::{'exact' if math == 'exact' else 'fastm'}::"), kname
    return kname


# name -> (P, handle options). coop=0 joins the issue's `pk=0, ustg=1` so that the f32 contractions run the tile kernel with the control table
# in global memory, not the speculative kernel a batch of three would otherwise take.
LAYOUTS = {
    "lanes": (1, dict(coop=0)),
    "coop": (33, dict(spec=0)),
    "spec": (33, dict()),
    "tile": (33, dict(lane=0, coop=0)),
    "duo": (70, dict(coop=0, pk=0, duo=1)),                 # three groups: a pair without a group B
    "one_group_per_wave": (70, dict(coop=0, pk=0, duo=0)),
    "global_table": (70, dict(coop=0, pk=0, ustg=1)),
}


@pytest.mark.parametrize("mlp,math", ARITH)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_layout_and_arithmetic(layout, mlp, math):
    """m = 4, B = 3, H = 9. The lane, cooperative and speculative kernels exist for the f32 contractions only: in the matrix-pipe modes those
    three settings run tile kernels (one wave per instance at P = 1), on the same inputs."""
    P, options = LAYOUTS[layout]
    kname = _check(4, mlp, math, P, options)
    md = MODE[mlp]
    if layout == "lanes":
        want = "sdempc_solve_kernel<TeamWave, 4, 0, false, 1, false>" if mlp == "f32" else f"sdempc_solve_kernel<TeamWave, 4, {md}, false, 0, false>"     # MODE 1: lane layout
    elif layout == "spec" and mlp == "f32":
        want = "sdempc_solve_spec_kernel<4, false>"
    elif layout == "coop" and mlp == "f32":
        want = kc.coop_kernel(4, P, B, _device_cus())                                                  # MODE 2: cooperative
    elif layout in ("coop", "spec", "tile", "one_group_per_wave"):
        want = f"sdempc_solve_kernel<TeamBlock, 4, {md}, false, 0, false>"                             # MODE 0: one group per wave, control table in LDS
    elif layout == "duo":
        want = f"sdempc_solve_kernel<TeamPairT<2>, 4, {md}, false, 3, false>"
    else:
        want = f"sdempc_solve_kernel<TeamBlock, 4, {md}, false, 0, true>"
    assert kc.normalise(kname) == (want, math), kname


@pytest.mark.parametrize("mlp,math", [(d, mth) for d in ("f32", "f32x3") for mth in ("exact", "fast")])
@pytest.mark.parametrize("layout", ["tile", "duo"])
@pytest.mark.parametrize("m", [6, 3, 8])
def test_motor_counts(m, layout, mlp, math):
    """The hexarotor specialisation and the generic instantiation with its zero-padded 8-slot tables (m = 3: five padded slots; m = 8: none),
    every slot of which holds a different uref / bound / rotor here. P = 45: a ragged second group."""
    kname = _check(m, mlp, math, 45, dict(lane=0, coop=0) if layout == "tile" else dict(coop=0, pk=0, duo=1))
    if m == 6:
        want = f"sdempc_solve_kernel<TeamPairT<2>, 6, {MODE[mlp]}, false, 3, false>" if layout == "duo" else f"sdempc_solve_kernel<TeamBlock, 6, {MODE[mlp]}, false, 0, false>"
        assert kc.normalise(kname) == (want, math), kname
    else:
        assert f", 8, {MODE[mlp]}, " in kname, kname                  # (the default build carries the generic count in the one-group-per-wave tiles only)


# ---- throughput instantiations that only run when the batch exceeds the compute units ----------------------------------------------------
def _throughput(m, mlp, math, Bt, H, P, sample):
    cfg = asymmetric_cfg(m, horizon=H, num_short_dt=4, long_step_dt=0.1, num_particles=P, max_iter=3, max_no_improvement_iter=3, mlp_dtype=mlp, math_mode=math)
    model = asymmetric_model(m)
    x0, xref, _, u0 = asymmetric_problem(cfg, Bt, 11, noise=False)
    keys = prng.split(prng.PRNGKey(4), Bt)
    s0 = np.full(Bt, 0.01, np.float32)
    S = SdeMpcSolver(cfg, model, max_batch=Bt)
    assert S.get_option("pk") == -1 and S.get_option("coop") == 1 and S.get_option("ustg") == -1 and S.get_option("device_cus") < Bt     # nothing forced
    out = S.solve_keys(x0, xref, keys, u0, s0)
    kname = S.last_kernel_name()
    O = orc.Oracle(cfg, model)
    with oracle_threads():
        for b in sample:
            uo, xe, io = O.solve(x0[b], xref[b], orc.noise_from_key(keys[b], P, H), u0[b], 0.01)[:3]
            assert bits_differ(out[0][b], uo) == 0 and bits_differ(out[1][b], xe) == 0 and bits_differ(out[2][b], io) == 0, b
    return S, out, kname, (x0, xref, keys, u0, s0)


@pytest.mark.parametrize("mlp,math", [("f32x3", "fast"), ("f32", "exact")])
@pytest.mark.parametrize("m", [4, 6])
def test_six_team_workgroups(m, mlp, math):
    """1,700 instances, nothing forced: the six-team workgroup. Instances 0, 1535, 1536 (the first beyond the team slots) and the last (150 degrees,
    negated quaternion) against the oracle; the whole batch against the same launch in two-team workgroups."""
    Bt = 1700
    S, out, kname, args = _throughput(m, mlp, math, Bt, 7, 70, (0, 1535, 1536, Bt - 1))
    assert kc.normalise(kname) == (f"sdempc_solve_kernel<TeamPairT<6>, {m}, {MODE[mlp]}, false, 3, false>", math), kname
    S.set_option("hex", 0)
    o2 = S.solve_keys(*args)
    assert kc.normalise(S.last_kernel_name()) == (f"sdempc_solve_kernel<TeamPairT<2>, {m}, {MODE[mlp]}, false, 3, false>", math), S.last_kernel_name()
    assert bits_differ(out[0], o2[0]) == 0 and bits_differ(out[1], o2[1]) == 0 and bits_differ(out[2], o2[2]) == 0
    S.close()


def test_one_wave_per_instance_four_instances_per_workgroup():
    """C1 geometry (P = 32, H = 8, B = 1,280): one wave per instance, four instances per workgroup."""
    Bt = 1280
    S, out, kname, _ = _throughput(4, "f32x3", "fast", Bt, 8, 32, (0, 1, 1025, Bt - 1))
    assert "TeamWave, 4, 2, false" in kname, kname
    S.close()


# ---- closed loop: controller A, plant another asymmetric vehicle -------------------------------------------------------------------------
def _episodes(cfg, seed):
    x0, xref, _, u = asymmetric_problem(cfg, B, seed, noise=False)
    return x0, xref[None], np.stack([prng.PRNGKey(seed + b) for b in range(B)]), u


@pytest.mark.parametrize("mlp,math", ARITH)
def test_closed_loop_against_another_asymmetric_plant(mlp, math):
    """The plant step (a writing of the rigid-body step of its own) with a plant that differs from the controller's model in b3, ct0, Jx != Jy,
    sigma, ...: one shared plant of another seed, then per-episode plants perturbed from A; two substeps, warm starts outside the bounds."""
    cfg = asymmetric_cfg(4, horizon=7, num_short_dt=4, long_step_dt=0.1, num_particles=33, max_iter=4, max_no_improvement_iter=4, mlp_dtype=mlp, math_mode=math)
    A, other = asymmetric_model(4), asymmetric_model(4, seed=23)
    assert other.thrust_poly[2] != A.thrust_poly[2] and other.inertia[0] != other.inertia[1] and bits_differ(other.b3, A.b3) == 6
    rng = np.random.default_rng(3)
    plants = [A.perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, moment=0.2, sigma=0.2, residual=0.2) for _ in range(B)]
    T = 4
    x0, xref, keys, u = _episodes(cfg, 20)
    S = SdeMpcSolver(cfg, A, max_batch=B)
    one = S.closed_loop(x0, xref, keys, T, u_init=u, plant=other, plant_substeps=2)
    per = S.closed_loop(x0, xref, keys, T, u_init=u, plant=plants, plant_substeps=2)
    S.solve_status()
    S.close()
    with oracle_threads():
        assert_same(one, plant_loop_ref(cfg, A, other, x0, xref, keys, T, substeps=2, u_init=u))
        assert_same(per, plant_loop_ref(cfg, A, plants, x0, xref, keys, T, substeps=2, u_init=u))
    assert np.isfinite(per[0]).all() and bits_differ(one[0][:, 1:], per[0][:, 1:]) > 0


@pytest.mark.parametrize("mlp,math", [("f32", "exact"), ("f32x3", "fast")])
def test_plain_closed_loop(mlp, math):
    cfg = asymmetric_cfg(4, horizon=7, num_short_dt=4, long_step_dt=0.1, num_particles=33, max_iter=4, max_no_improvement_iter=4, mlp_dtype=mlp, math_mode=math)
    A = asymmetric_model(4)
    T = 4
    x0, xref, keys, u = _episodes(cfg, 30)
    S = SdeMpcSolver(cfg, A, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T, u_init=u)
    S.solve_status()
    S.close()
    with oracle_threads():
        assert_same(got, closed_loop_ref(cfg, A, x0, xref, keys, T, u_init=u))
    assert np.isfinite(got[0]).all()


# ---- mutants must be caught ----------------------------------------------------------------------------------------------------------------
# The kernels get a mutant of (A, cfg), the oracle the original: their results must differ. This is what a kernel that dropped b3 / b3n / ct0,
# swapped a pair, took |rotor_dir| = 1 or read another motor's slot would compute; with synthetic_iris() and a uniform configuration every
# mutant is the identity (asserted in tests/test_asymmetric_cpu.py) and nothing here could fail.
# Two things the oracle decides (same file): the gradient does not read input_bound — a rollout takes its controls as given, the bounds are the
# projection of the solve (SPEC.md §8) — so that mutant must leave the gradient's bits alone and change the solve's; and the negated initial
# quaternion is NOT a mutant: the oracle's cost, gradient, uopt and telemetry for q and -q are identical bit for bit, so it is dropped from the
# list (the odd-numbered instances of every parity case above carry -q instead).
SETTINGS = {"tile_f32_exact": ("f32", "exact", 33, dict(lane=0, coop=0), "TeamBlock, 4, 0, "),
            "duo_f32x3_fast": ("f32x3", "fast", 40, dict(coop=0, pk=0, duo=1), "TeamPairT<2>, 4, 2, false, 3, false>")}


@pytest.mark.parametrize("mutant", list(asymmetric_mutants()))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_mutants_are_caught(setting, mutant):
    mlp, math, P, options, kernel = SETTINGS[setting]
    cfg, A, prob, ref = _reference(4, mlp, math, P)
    Mm, cm = asymmetric_mutants()[mutant](A, cfg)
    assert Mm.to_blob() != A.to_blob() or cm != cfg
    _, (gc, grad), (uopt, xevol, info), kname = _run(cm, Mm, prob, options)
    assert kernel in kname, kname
    g_ref = np.stack([r[1][1].astype(np.float32) for r in ref])
    u_ref = np.stack([r[2][0] for r in ref])
    if mutant == "input_bound_rotated":
        assert bits_differ(grad, g_ref) == 0
    else:
        assert bits_differ(grad, g_ref) > 0
    assert bits_differ(uopt, u_ref) > 0
