"""GPU parity tests: the HIP path (through the C ABI, include/sdempc.h) against the CPU oracle and the
committed golden vectors. Integer-like bar: float32 results are required to be BIT-IDENTICAL, which
is stricter than the 1e-4 relative tolerance BASELINE.json's north_star asks for; the tolerance
version of each check is asserted as well so a future non-reproducing kernel fails with a clear message.
"""
import os

import numpy as np
import pytest

import kernel_census as kc
import orc
from cases import CDIR, bits_differ, golden_cases, load_golden
from sde4mbrl_px4_amd import MPCConfig, load_mpc_config, synthetic_hexa, synthetic_iris, synthetic_multirotor
from sde4mbrl_px4_amd import workload as W

pytestmark = pytest.mark.gpu
RTOL = 1e-4   # north_star tolerance (float32)


# execution options every solver of the running test is created with (sdempc_set_option; set by the `layout` fixture)
LAYOUT_OPTS = {}


@pytest.fixture(params=["auto", "coop", "tile"])
def layout(request, monkeypatch):
    """auto: the library picks (single-particle lanes for P = 1; for small batches the cooperative one-particle-per-wave path, in its
    speculative form when two or more groups of workgroups fit; 32-particle tiles otherwise); coop: the speculative form switched off, which
    pins the plain cooperative kernel; tile: every alternative off, which pins the tile layout on the same cases. All bit-identical.
    Selected through the handle's options (include/sdempc.h SDEMPC_OPT_*), not through the environment."""
    opts = {"auto": {}, "coop": {"spec": 0}, "tile": {"lane": 0, "coop": 0}}[request.param]
    monkeypatch.setitem(globals(), "LAYOUT_OPTS", opts)
    return request.param


def _solver(cfg, model, B, **options):
    from sde4mbrl_px4_amd.solver import SdeMpcSolver
    return SdeMpcSolver(cfg, model, max_batch=B, options={**LAYOUT_OPTS, **options})


def _close(a, b, what):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=1e-5, err_msg=what)


@pytest.mark.parametrize("name", list(golden_cases().keys()))
def test_golden_vectors(name, layout):
    cfg, model, seed, curr_t, pos = golden_cases()[name]
    g = load_golden(name)
    S = _solver(cfg, model, 1)
    cost, traj, xmean = S.rollout(g["x0"][None], g["u"][None], g["xref"][None], g["noise"][None], True, True)
    _close(cost[0], g["cost"], "cost")
    _close(traj[0, 0], g["traj_p0"], "traj")
    assert cost[0] == g["cost"] and bits_differ(traj[0, :, -1, :], g["traj_last"]) == 0 and bits_differ(xmean[0], g["xmean"]) == 0
    gc, grad = S.grad(g["x0"][None], g["u"][None], g["xref"][None], g["noise"][None])
    _close(grad[0], g["grad"], "grad")
    assert gc[0] == g["grad_cost"] and bits_differ(grad[0], g["grad"]) == 0
    uopt, xevol, info = S.solve(g["x0"][None], g["xref"][None], g["noise"][None], g["u_init"][None], np.array([g["stepsize_in"]], np.float32))
    _close(uopt[0], g["uopt"], "uopt")
    _close(xevol[0], g["xevol"], "xevol")
    assert bits_differ(uopt[0], g["uopt"]) == 0 and bits_differ(xevol[0], g["xevol"]) == 0 and bits_differ(info[0], g["info"]) == 0
    # A8 post-processing of the driver loop (sde_control.py:428-432) on the GPU outputs
    thrust = uopt[0].sum(axis=1) / uopt.shape[2]
    wopt = np.stack([thrust, xevol[0, 1:, 10], xevol[0, 1:, 11], xevol[0, 1:, 12]]).T.astype(np.float64)
    np.testing.assert_array_equal(wopt, g["wopt"])
    S.close()


def _problem(cfg, B, seed=0, pos=False):
    H, P, m = cfg.horizon, cfg.num_particles, cfg.num_motors
    x0 = W.random_initial_states(B, seed)
    xref = np.stack([W.constant_reference(W.HOVER, H) if pos else W.reference_window(0.13 * b, cfg.time_steps) for b in range(B)])
    noise = W.make_noise(B, P, H, seed)
    rng = np.random.default_rng(seed + 5)
    u = np.clip(np.asarray(cfg.uref, np.float32) + 0.1 * rng.standard_normal((B, H, m)), 1e-4, 1).astype(np.float32)
    return x0, xref, noise, u


EDGE = {
    "P1": dict(horizon=9, num_short_dt=9, num_particles=1),
    "P31": dict(horizon=7, num_short_dt=7, num_particles=31),
    "P33": dict(horizon=7, num_short_dt=3, long_step_dt=0.1, num_particles=33),
    "P160_5groups": dict(horizon=6, num_short_dt=6, num_particles=160),
    "P290_ragged": dict(horizon=5, num_short_dt=5, num_particles=290),
    "H1": dict(horizon=1, num_short_dt=1, num_particles=32),
    "H130_N_gt_256": dict(horizon=130, num_short_dt=130, num_particles=32),
    "discount_slewconstr": dict(horizon=12, num_short_dt=12, num_particles=40, discount=0.9, u_slew_coeff=0.5,
                                u_slew_constr=[[-0.02, 0.03]] * 4, u_slew_constr_coeff=10.0),
    "conservative_ls": dict(horizon=10, num_short_dt=10, num_particles=32, ls_reset_option="conservative"),
    "moment_scale": dict(horizon=10, num_short_dt=10, num_particles=32, moment_scale=0.5),
    "no_linesearch": dict(horizon=10, num_short_dt=10, num_particles=32, ls_maxls=0, stepsize=1e-4),
    "unbounded_u": dict(horizon=10, num_short_dt=10, num_particles=32, enforce_ubound=False),
    "max_iter_0": dict(horizon=8, num_short_dt=8, num_particles=32, max_iter=0),
    "max_no_improvement_1": dict(horizon=8, num_short_dt=8, num_particles=32, max_iter=12, max_no_improvement_iter=1),
    "state_constr": dict(horizon=12, num_short_dt=12, num_particles=40, state_id=[3, 4, 5, 10, 11, 12], state_penalty=[10.0, 10.0, 20.0, 10.0, 10.0, 10.0],
                         state_bound=[[-0.5, 0.5], [-0.5, 0.5], [-0.4, 0.7], [-0.8, 0.8], [-0.8, 0.8], [-0.7, 0.7]], constr_pen=0.1),   # iris_sitl_traj_mpc.yaml:16-29
    "state_constr_open_bounds_P1": dict(horizon=9, num_short_dt=9, num_particles=1, state_id=[2, 5], state_penalty=[50.0, 5.0],
                                        state_bound=[[0.2, float("inf")], [float("-inf"), 0.1]]),
    "loose_tolerance_early_stop": dict(horizon=8, num_short_dt=8, num_particles=32, max_iter=40, max_no_improvement_iter=40, rtol=5e-2),
}


@pytest.mark.parametrize("name", list(EDGE.keys()))
def test_edge_cases_bit_exact(name, layout):
    kw = dict(u_slew_coeff=1.0, max_iter=8, max_no_improvement_iter=8)
    kw.update(EDGE[name])
    cfg = MPCConfig(**kw)
    model = synthetic_iris()
    B = 3
    x0, xref, noise, u = _problem(cfg, B, seed=21)
    S, O = _solver(cfg, model, B), orc.Oracle(cfg, model)
    cost, traj, xmean = S.rollout(x0, u, xref, noise, True, True)
    gc, grad = S.grad(x0, u, xref, noise)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, cfg.horizon, 1))
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    uopt, xevol, info = S.solve(x0, xref, noise, u0, s0)
    for b in range(B):
        c, t, xm = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        _close(cost[b], c, "cost")
        assert cost[b] == np.float32(c) and bits_differ(traj[b], t) == 0 and bits_differ(xmean[b], xm) == 0
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        _close(grad[b], g2, "grad")
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], u0[b], float(s0[b]))
        _close(uopt[b], uo, "uopt")
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0
    S.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_configurations_bit_exact(seed, layout):
    """Randomised hyper-parameters (horizon, particles, motors, cost weights, time grid, optimiser knobs)."""
    rng = np.random.default_rng(1000 + seed)
    m = int(rng.choice([4, 6]))
    H = int(rng.integers(2, 40))
    kw = dict(horizon=H, num_short_dt=int(rng.integers(0, H + 1)), short_step_dt=float(rng.choice([0.02, 0.05])), long_step_dt=float(rng.choice([0.05, 0.1])),
              num_particles=int(rng.integers(1, 200)), discount=float(rng.choice([1.0, 0.98, 0.9])),
              uerr=float(rng.uniform(0, 2)), perr=list(rng.uniform(1, 200, 3)), verr=list(rng.uniform(0, 10, 3)), qerr=list(rng.uniform(0, 100, 3)),
              werr=list(rng.uniform(0, 3, 3)), res_mult=float(rng.uniform(0, 0.1)), u_slew_coeff=float(rng.uniform(0, 2)),
              max_iter=int(rng.integers(1, 9)), max_no_improvement_iter=int(rng.integers(1, 9)), beta_init=float(rng.uniform(0, 0.5)),
              ls_init_stepsize=float(rng.choice([0.01, 0.001])), ls_max_stepsize=float(rng.choice([1.0, 10.0, 0.005])), ls_coef=float(rng.choice([0.01, 0.1])),
              ls_decrease_factor=float(rng.uniform(0.3, 0.9)), ls_increase_factor=float(rng.uniform(1.0, 2.0)), ls_maxls=int(rng.integers(1, 6)),
              ls_reset_option=str(rng.choice(["increase", "conservative"])))
    if m == 6:
        kw.update(input_id=list(range(6)), input_bound=[[1e-4, 1.0]] * 6, uref=[0.42] * 6)
    if rng.random() < 0.5:
        kw.update(u_slew_constr=[[-0.05, 0.05]] * m, u_slew_constr_coeff=float(rng.uniform(1, 20)))
    cfg = MPCConfig(**kw)
    model = synthetic_iris(seed) if m == 4 else synthetic_hexa(seed)
    B = 2
    x0, xref, noise, u = _problem(cfg, B, seed=300 + seed, pos=bool(seed % 2))
    S, O = _solver(cfg, model, B), orc.Oracle(cfg, model)
    cost, traj, xmean = S.rollout(x0, u, xref, noise, True, True)
    gc, grad = S.grad(x0, u, xref, noise)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, cfg.horizon, 1))
    uopt, xevol, info = S.solve(x0, xref, noise, u0, np.full(B, cfg.ls_init_stepsize, np.float32))
    for b in range(B):
        c, t, xm = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        assert cost[b] == np.float32(c) and bits_differ(traj[b], t) == 0 and bits_differ(xmean[b], xm) == 0
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], u0[b], cfg.ls_init_stepsize)
        _close(uopt[b], uo, "uopt")
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0
    S.close()


@pytest.mark.parametrize("m", [1, 3, 5, 8])
def test_generic_motor_count_bit_exact(m, layout):
    """Motor counts other than 4 / 6 run the generic (8-slot, zero-padded) kernel instantiation."""
    cfg = MPCConfig(horizon=9, num_short_dt=9, num_particles=45, input_id=list(range(m)), input_bound=[[1e-4, 1.0]] * m, uref=[0.6] * m,
                    u_slew_coeff=0.5, max_iter=5, max_no_improvement_iter=5)
    model = synthetic_multirotor(m)
    B = 2
    x0, xref, noise, u = _problem(cfg, B, seed=40 + m)
    S, O = _solver(cfg, model, B), orc.Oracle(cfg, model)
    gc, grad = S.grad(x0, u, xref, noise)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, cfg.horizon, 1))
    uopt, xevol, info = S.solve(x0, xref, noise, u0, np.full(B, 0.01, np.float32))
    for b in range(B):
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], u0[b], 0.01)
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0
    S.close()


@pytest.mark.parametrize("P", [32, 100])
def test_diverging_rollout_non_finite_parity(P, layout):
    """A rollout that overflows f32 (single-rotor vehicle, H=55): infinities and NaN positions agree with the oracle word for word,
    the solve takes no step on a NaN gradient (SPEC.md §8 guard) and the finite instance beside it is unaffected. P=32 runs the
    one-wave team, P=100 the four-wave team. Found by tests/tools/soak.py."""
    from cases import diverging_single_rotor_case
    cfg, model, x0, xref, noise, u = diverging_single_rotor_case(P=P)
    B = len(x0)
    un = u.copy(); un[2, 3, 0] = np.nan                          # NaN in a warm start is projected to the lower bound
    S, O = _solver(cfg, model, B), orc.Oracle(cfg, model)
    cost, traj, xm = S.rollout(x0, u, xref, noise, True, True)
    gc, grad = S.grad(x0, u, xref, noise)
    uopt, xevol, info = S.solve(x0, xref, noise, un, np.full(B, 0.01, np.float32))
    assert np.isinf(gc[1]) and np.isnan(grad[1]).sum() >= 50
    for b in range(B):
        c, t, mm = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], un[b], 0.01)
        assert bits_differ(cost[b], c) == 0 and bits_differ(traj[b], t) == 0 and bits_differ(xm[b], mm) == 0
        assert bits_differ(gc[b], c2) == 0 and bits_differ(grad[b], g2.astype(np.float32)) == 0
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0
    assert np.array_equal(uopt[1], u[1]) and info[1][2] == 0 and not np.isfinite(info[1][3])
    assert info[2][2] >= 1 and np.isfinite(uopt[2]).all() and np.isfinite(xevol[2]).all()
    S.close()


@pytest.mark.parametrize("mlp", ["f16", "f32x3"])
@pytest.mark.parametrize("P", [32, 100])
def test_diverging_rollout_non_finite_parity_in_the_matrix_pipe_modes(P, mlp):
    """The same overflowing rollout through the matrix instruction: infinities entering a limb split turn into NaN (inf - inf) on both sides, NaN
    operands give NaN accumulators; positions of infinities and NaNs agree with the oracle word for word (SPEC.md §3.7, §9a 'special values')."""
    from cases import diverging_single_rotor_case
    cfg, model, x0, xref, noise, u = diverging_single_rotor_case(P=P)
    cfg = cfg.replace(mlp_dtype=mlp)
    B = len(x0)
    S, O = _solver(cfg, model, B, coop=0), orc.Oracle(cfg, model)
    cost, traj, xm = S.rollout(x0, u, xref, noise, True, True)
    gc, grad = S.grad(x0, u, xref, noise)
    uopt, xevol, info = S.solve(x0, xref, noise, u, np.full(B, 0.01, np.float32))
    assert not np.isfinite(gc[1])
    for b in range(B):
        c, t, mm = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], u[b], 0.01)
        assert bits_differ(cost[b], c) == 0 and bits_differ(traj[b], t) == 0 and bits_differ(xm[b], mm) == 0, b
        assert bits_differ(gc[b], c2) == 0 and bits_differ(grad[b], g2.astype(np.float32)) == 0, b
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0, b
    S.close()


def test_saturating_activations_and_violent_states_bit_exact():
    """Weights scaled up so that tanh / sigmoid arguments exceed their clamp ranges (|x| > 9, > 30), fast tumbling initial
    states and strong diffusion: exercises the clamped branches of SPEC.md §3 and large-magnitude arithmetic."""
    model = synthetic_iris(5)
    model.W1z = (model.W1z * 25.0).astype(np.float32)
    model.W2 = (model.W2 * 6.0).astype(np.float32)
    model.w3n = (model.w3n * 40.0).astype(np.float32)
    model.sigma = (model.sigma * 8.0).astype(np.float32)
    cfg = MPCConfig(horizon=15, num_short_dt=15, num_particles=64, u_slew_coeff=1.0, max_iter=6, max_no_improvement_iter=6)
    B = 3
    x0, xref, noise, u = _problem(cfg, B, seed=90)
    x0[:, 3:6] *= 30.0
    x0[:, 10:13] *= 60.0
    S, O = _solver(cfg, model, B), orc.Oracle(cfg, model)
    cost, traj, xmean = S.rollout(x0, u, xref, noise, True, True)
    gc, grad = S.grad(x0, u, xref, noise)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, cfg.horizon, 1))
    uopt, xevol, info = S.solve(x0, xref, noise, u0, np.full(B, 0.01, np.float32))
    assert np.all(np.isfinite(traj)) and np.all(np.isfinite(grad))
    for b in range(B):
        c, t, xm = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        assert cost[b] == np.float32(c) and bits_differ(traj[b], t) == 0 and bits_differ(xmean[b], xm) == 0
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], u0[b], 0.01)
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0
    S.close()


def test_hexa_six_motors_bit_exact(layout):
    cfg = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(horizon=14, num_short_dt=14, num_particles=96, max_iter=6, max_no_improvement_iter=6)
    model = synthetic_hexa()
    B = 2
    x0, xref, noise, u = _problem(cfg, B, seed=4)
    S, O = _solver(cfg, model, B), orc.Oracle(cfg, model)
    gc, grad = S.grad(x0, u, xref, noise)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, cfg.horizon, 1))
    uopt, xevol, info = S.solve(x0, xref, noise, u0, np.full(B, 0.01, np.float32))
    for b in range(B):
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], u0[b], 0.01)
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0
    S.close()


def test_warm_start_chain_matches_oracle(layout):
    """Three consecutive ticks, each warm-started from the previous (uopt, stepsize) like mpc_process_fn
    (sde_control.py:412: opt_state is threaded through successive calls)."""
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(horizon=16, num_short_dt=16, num_particles=64, max_iter=10, max_no_improvement_iter=10)
    model = synthetic_iris()
    S, O = _solver(cfg, model, 1), orc.Oracle(cfg, model)
    x = W.random_initial_states(1, 9)
    ug = uo = np.tile(np.asarray(cfg.uref, np.float32), (1, cfg.horizon, 1))
    sg = so = 0.01
    for tick in range(3):
        xref = W.reference_window(0.05 * tick, cfg.time_steps)[None]
        noise = W.make_noise(1, 64, 16, 100 + tick)
        ug, xe_g, info_g = S.solve(x, xref, noise, ug, np.array([sg], np.float32))
        u1, xe_o, info_o, _ = O.solve(x[0], xref[0], noise[0], uo[0], so)
        uo = u1[None]
        assert bits_differ(ug, uo) == 0 and bits_differ(xe_g[0], xe_o) == 0 and bits_differ(info_g[0], info_o) == 0
        sg, so = float(info_g[0, 1]), float(info_o[1])
        x = xe_g[:, 1, :].copy()
    S.close()


def test_batch_position_independence_and_determinism():
    cfg = MPCConfig(horizon=10, num_short_dt=10, num_particles=64, u_slew_coeff=1.0, max_iter=5, max_no_improvement_iter=5)
    model = synthetic_iris()
    B = 37
    x0, xref, noise, u = _problem(cfg, B, seed=2)
    S = _solver(cfg, model, B)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, 10, 1))
    s0 = np.full(B, 0.01, np.float32)
    a = S.solve(x0, xref, noise, u0, s0)
    b = S.solve(x0, xref, noise, u0, s0)
    for p, q in zip(a, b):
        assert bits_differ(p, q) == 0                                   # run-to-run deterministic
    perm = np.random.default_rng(0).permutation(B)
    c = S.solve(x0[perm], xref[perm], noise[perm], u0[perm], s0[perm])
    for p, q in zip(a, c):
        assert bits_differ(p[perm], q) == 0                             # result independent of batch slot
    S.close()


def test_full_size_c2_properties_and_sampled_parity():
    """BASELINE config C2 at full size (H=50, P=128): size-independent properties on a batch plus
    bit-parity of the gradient and of a shortened solve on sampled instances."""
    cfg_full = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml"))
    cfg = cfg_full.replace(max_iter=12, max_no_improvement_iter=12)
    model = synthetic_iris()
    B = 24
    x0, xref, noise, u = _problem(cfg, B, seed=50)
    S, O = _solver(cfg, model, B), orc.Oracle(cfg, model)
    cost, traj, xmean = S.rollout(x0, u, xref, noise, True, True)
    assert np.all(np.isfinite(traj)) and np.abs(np.linalg.norm(traj[..., 6:10], axis=-1) - 1).max() < 1e-5
    np.testing.assert_array_equal(traj[:, :, 0, :], np.repeat(x0[:, None, :], 128, axis=1))
    np.testing.assert_allclose(xmean, traj.mean(axis=1), rtol=3e-5, atol=3e-6)
    gc, grad = S.grad(x0, u, xref, noise)
    assert bits_differ(gc, cost) == 0                                   # forward sweep of grad == rollout
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, 50, 1))
    uopt, xevol, info = S.solve(x0, xref, noise, u0, np.full(B, 0.01, np.float32))
    assert uopt.min() >= 1e-4 and uopt.max() <= 1.0
    assert np.all(info[:, 6] <= info[:, 5]) and np.all(info[:, 2] == 12)
    c_opt, _, xm = S.rollout(x0, uopt, xref, noise, False, True)
    assert bits_differ(c_opt, info[:, 6]) == 0 and bits_differ(xm, xevol) == 0   # reported cost/trajectory belong to uopt
    for b in (0, 11, 23):
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0
        uo, xe, inf, _ = O.solve(x0[b], xref[b], noise[b], u0[b], 0.01)
        _close(uopt[b], uo, "uopt")
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], inf) == 0
    S.close()


def test_device_resident_api_equals_host_api():
    import torch
    cfg = MPCConfig(horizon=10, num_short_dt=10, num_particles=40, u_slew_coeff=1.0, max_iter=4, max_no_improvement_iter=4)
    model = synthetic_iris()
    B = 5
    x0, xref, noise, u = _problem(cfg, B, seed=8)
    S = _solver(cfg, model, B)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, 10, 1))
    s0 = np.full(B, 0.01, np.float32)
    ref = S.solve(x0, xref, noise, u0, s0)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nd = t(S.noise_to_device_layout(noise))
    tx0, txr, tu0, ts0 = t(x0), t(xref), t(u0), t(s0)
    uopt = torch.empty((B, 10, 4), device=dev); xevol = torch.empty((B, 11, 13), device=dev); info = torch.empty((B, 8), device=dev)
    S.solve_dev(B, tx0.data_ptr(), txr.data_ptr(), nd.data_ptr(), tu0.data_ptr(), ts0.data_ptr(), uopt.data_ptr(), xevol.data_ptr(), info.data_ptr(),
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert S.last_kernel_ms() > 0
    assert bits_differ(uopt.cpu().numpy(), ref[0]) == 0 and bits_differ(xevol.cpu().numpy(), ref[1]) == 0 and bits_differ(info.cpu().numpy(), ref[2]) == 0
    # layout conversion on the device == the host conversion; ragged P (40 = 32 + 8): padded lanes are zeros
    st = torch.cuda.current_stream().cuda_stream
    nd2 = torch.full_like(nd, 7.0)
    S.noise_to_device_layout_dev(B, t(noise).data_ptr(), nd2.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(nd, nd2)
    # particle x horizon tensor through the device API, canonical layout
    tu = t(u); cost = torch.empty(B, device=dev); traj = torch.empty((B, 40, 11, 13), device=dev)
    S.rollout_dev(B, tx0.data_ptr(), tu.data_ptr(), txr.data_ptr(), nd.data_ptr(), cost.data_ptr(), None, True, st)
    S.traj_to_canonical_dev(B, traj.data_ptr(), st)
    torch.cuda.synchronize()
    c_ref, traj_ref, _ = S.rollout(x0, u, xref, noise, True, True)
    assert bits_differ(cost.cpu().numpy(), c_ref) == 0 and bits_differ(traj.cpu().numpy(), traj_ref) == 0
    # the conversion is refused once the trajectory workspace no longer holds that rollout: a rollout without store_traj, a smaller one, a solve
    from sde4mbrl_px4_amd.solver import SdempcError
    S.rollout_dev(2, tx0.data_ptr(), tu.data_ptr(), txr.data_ptr(), nd.data_ptr(), cost.data_ptr(), None, True, st)
    S.traj_to_canonical_dev(2, traj.data_ptr(), st)
    with pytest.raises(SdempcError, match="fewer instances"):
        S.traj_to_canonical_dev(B, traj.data_ptr(), st)
    S.rollout_dev(B, tx0.data_ptr(), tu.data_ptr(), txr.data_ptr(), nd.data_ptr(), cost.data_ptr(), None, False, st)
    with pytest.raises(SdempcError, match="holds no rollout"):
        S.traj_to_canonical_dev(B, traj.data_ptr(), st)
    S.rollout_dev(B, tx0.data_ptr(), tu.data_ptr(), txr.data_ptr(), nd.data_ptr(), cost.data_ptr(), None, True, st)
    S.solve_dev(B, tx0.data_ptr(), txr.data_ptr(), nd.data_ptr(), tu0.data_ptr(), ts0.data_ptr(), uopt.data_ptr(), xevol.data_ptr(), info.data_ptr(), st)
    with pytest.raises(SdempcError, match="holds no rollout"):
        S.traj_to_canonical_dev(B, traj.data_ptr(), st)
    torch.cuda.synchronize()
    S.close()


def test_c5_long_horizon_shape_runs():
    """C5 geometry (H=200, P=1024) through the f32 path: one gradient, parity on the cost and gradient."""
    cfg = load_mpc_config(os.path.join(CDIR, "c5_iris_traj_h200_p1024.yaml"))
    model = synthetic_iris()
    x0, xref, noise, u = _problem(cfg, 1, seed=77)
    S, O = _solver(cfg, model, 1), orc.Oracle(cfg, model)
    gc, grad = S.grad(x0, u, xref, noise)
    c2, g2 = O.grad(x0[0], u[0], xref[0], noise[0])
    assert gc[0] == np.float32(c2) and bits_differ(grad[0], g2.astype(np.float32)) == 0
    S.close()


# ---- the matrix-pipe modes: fp16 operands (SPEC.md §9, BASELINE config C5) and the three-limb bf16 split (§9b) ----------------------
# v_mfma_f32_32x32x16_{f16,bf16} accumulate their 16 products in a hardware-specific way that the oracle models exactly (SPEC.md §9a,
# oracle/mfma16_model.c, fitted to 7.0 million hardware experiments): both modes are compared with the oracle BIT FOR BIT, like the f32 path.
def _check_bit_exact(cfg, model, B, seed, **options):
    x0, xref, noise, u = _problem(cfg, B, seed=seed)
    S, O = _solver(cfg, model, B, **options), orc.Oracle(cfg, model)
    cost, traj, xmean = S.rollout(x0, u, xref, noise, True, True)
    gc, grad = S.grad(x0, u, xref, noise)
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, cfg.horizon, 1))
    s0 = np.full(B, 0.01, np.float32)
    uopt, xevol, info = S.solve(x0, xref, noise, u0, s0)
    assert uopt.min() >= 1e-4 and uopt.max() <= 1.0 and np.all(info[:, 6] <= info[:, 5])
    for b in range(B):
        c, t, xm = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        _close(cost[b], c, "cost")
        assert cost[b] == np.float32(c) and bits_differ(traj[b], t) == 0 and bits_differ(xmean[b], xm) == 0, ("rollout", b)
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0, ("grad", b)
        uo, xe, io, _ = O.solve(x0[b], xref[b], noise[b], u0[b], 0.01)
        _close(uopt[b], uo, "uopt")
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, ("solve", b)
    S.close()
    return cost


@pytest.mark.parametrize("mlp", ["f16", "f32x3"])
@pytest.mark.parametrize("H,P,m,opts", [
    (24, 70, 4, dict()),                       # three groups, small batch: the packed-tanh latency instantiation is f32-only; one group per wave here (batch fits resident)
    (24, 70, 4, dict(duo=1)),                  # the same in the duo layout: a pair without a group B
    (12, 128, 4, dict(pk=0, duo=1)),           # C2 geometry: TeamPair duo throughput instantiation
    (12, 128, 4, dict(pk=0, duo=0)),           # one group per wave
    (9, 33, 6, dict(pk=0, duo=1)),             # six rotors, ragged second group
    (7, 300, 4, dict(pk=0, ustg=1)),           # ten groups on four waves, control table in global memory
    (16, 32, 4, dict()),                       # one group: one wave per instance (TeamWave)
])
def test_matrix_pipe_modes_match_oracle_bit_for_bit(mlp, H, P, m, opts):
    kw = dict(horizon=H, num_short_dt=max(1, H // 2), long_step_dt=0.1, num_particles=P, u_slew_coeff=1.0, max_iter=6, max_no_improvement_iter=6, mlp_dtype=mlp)
    if m != 4:
        kw.update(input_id=list(range(m)), input_bound=[[1e-4, 1.0]] * m, uref=[0.42] * m)
    cfg = MPCConfig(**kw)
    model = synthetic_iris() if m == 4 else synthetic_hexa()
    cost = _check_bit_exact(cfg, model, 3, 61, coop=0, **opts)
    # and genuinely another arithmetic than the f32 chain (f16: always; f32x3: in the last bits of most rollouts)
    if mlp == "f16":
        x0, xref, noise, u = _problem(cfg, 3, seed=61)
        S32 = _solver(cfg.replace(mlp_dtype="f32"), model, 3, coop=0, **opts)
        c32, _, _ = S32.rollout(x0, u, xref, noise)
        S32.close()
        assert bits_differ(cost, c32) > 0


def test_f32x3_differs_from_the_f32_chain_in_the_last_bits_only():
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml"))
    model = synthetic_iris()
    x0, xref, noise, u = _problem(cfg, 2, seed=9)
    out = {}
    for mlp in ("f32", "f32x3"):
        S = _solver(cfg.replace(mlp_dtype=mlp), model, 2, coop=0, pk=0)
        out[mlp] = S.rollout(x0, u, xref, noise, True, True)
        S.close()
    assert bits_differ(out["f32"][1], out["f32x3"][1]) > 0
    np.testing.assert_allclose(out["f32x3"][1], out["f32"][1], rtol=0, atol=5e-5)
    np.testing.assert_allclose(out["f32x3"][0], out["f32"][0], rtol=1e-6)


def test_c5_f16_mlp_path():
    """BASELINE config C5: H=200, P=1024 with the fp16 drift-MLP MFMA path; cost and gradient against the oracle, bit for bit."""
    cfg = load_mpc_config(os.path.join(CDIR, "c5_iris_traj_h200_p1024.yaml")).replace(mlp_dtype="f16")
    model = synthetic_iris()
    x0, xref, noise, u = _problem(cfg, 1, seed=78)
    S, O = _solver(cfg, model, 1), orc.Oracle(cfg, model)
    gc, grad = S.grad(x0, u, xref, noise)
    c2, g2 = O.grad(x0[0], u[0], xref[0], noise[0])
    assert gc[0] == np.float32(c2) and bits_differ(grad[0], g2.astype(np.float32)) == 0
    S.close()


# ---- key-derived noise (SPEC.md §7): device threefry/normal stream vs the oracle, bit for bit ----------------------------
@pytest.mark.parametrize("P,H", [(1, 20), (2, 3), (31, 7), (32, 20), (33, 5), (63, 4), (128, 50), (257, 9)])
def test_device_noise_from_keys_bit_exact(P, H):
    cfg = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml")).replace(horizon=H, num_short_dt=H, num_particles=P)
    B = 5
    keys = np.stack([orc.split([0, 10 + b], 2)[1] for b in range(B)]).astype(np.uint32)
    keys[3] = [0xFFFFFFFF, 0xFFFFFFFF]
    S = _solver(cfg, synthetic_iris(), B)
    got = S.noise_from_keys(keys)
    assert got.shape == (B, P, H, 6)
    for b in range(B):
        assert bits_differ(got[b], orc.noise_from_key(keys[b], P, H)) == 0, (P, H, b)
    # the device layout written by the generator: padded particles of the last group are exactly zero
    import torch
    nd = torch.full((S.lib.sdempc_noise_dev_floats(S._h, B),), 7.0, dtype=torch.float32, device="cuda")
    S.noise_from_keys_dev(keys, nd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dev = nd.cpu().numpy().reshape(B, (P + 31) // 32, H, 6, 32)
    assert np.array_equal(dev, S.noise_to_device_layout(got))
    S.close()


def test_solve_with_keys_equals_solve_with_oracle_noise():
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(horizon=14, num_short_dt=14, num_particles=72, max_iter=7, max_no_improvement_iter=7)
    B = 3
    x0, xref, _, u = _problem(cfg, B, 3)
    keys = np.stack([orc.split([0, 10], 3)[b] for b in range(B)]).astype(np.uint32)
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    S = _solver(cfg, synthetic_iris(), B)
    uk, xk, ik = S.solve_keys(x0, xref, keys, u, s0)
    noise = np.stack([orc.noise_from_key(keys[b], 72, 14) for b in range(B)])
    un, xn, inn = S.solve(x0, xref, noise, u, s0)
    assert bits_differ(uk, un) == 0 and bits_differ(xk, xn) == 0 and bits_differ(ik, inn) == 0
    O = orc.Oracle(cfg, synthetic_iris())
    uo, xo, io = O.solve_batch(x0, xref, noise, u, s0)
    _close(uk, uo, "uopt")
    assert bits_differ(uk, uo) == 0 and bits_differ(xk, xo) == 0 and bits_differ(ik, io) == 0
    S.close()


# ---- math_mode: fast (SPEC.md §10): hardware transcendentals, checked bit for bit through the model of the three instructions (§10a) ------
@pytest.mark.parametrize("mlp,P", [("f32", 70), ("f16", 70), ("f32x3", 70), ("f32", 1), ("f32", 33), ("f32x3", 32), ("f32x3", 7), ("f16", 31)])
def test_fast_math_mode_matches_oracle_bit_for_bit(mlp, P, layout):
    """(f32 contractions: the `layout` fixture also takes the mode through the lane layouts — single-particle lanes, speculative and plain cooperative kernels;
    P <= 32 in the matrix-pipe modes: the one-wave-per-instance instantiation of the tile kernels, whose telemetry a register-pressure experiment once lost)"""
    cfg = MPCConfig(horizon=24 if P == 70 else 9, num_short_dt=9, long_step_dt=0.1, num_particles=P, u_slew_coeff=1.0, max_iter=8, max_no_improvement_iter=8, mlp_dtype=mlp, math_mode="fast")
    model = synthetic_iris()
    B = 4
    x0, xref, noise, u = _problem(cfg, B, 11)
    S = _solver(cfg, model, B)
    O = orc.Oracle(cfg, model)                                   # v_exp_f32 / v_rcp_f32 / v_rsq_f32 as oracle/transc_model.c models them
    Ox = orc.Oracle(cfg.replace(math_mode="exact"), model)
    cost, traj, xmean = S.rollout(x0, u, xref, noise, True, True)
    gc, grad = S.grad(x0, u, xref, noise)
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    uopt, xevol, info = S.solve(x0, xref, noise, u, s0)
    for b in range(B):
        co, tro, xmo = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        assert cost[b] == np.float32(co) and bits_differ(traj[b], tro) == 0 and bits_differ(xmean[b], xmo) == 0
        gco, go = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(gco) and bits_differ(grad[b], go.astype(np.float32)) == 0
        uo, xe, io, _ = O.solve(x0[b], xref[b], noise[b], u[b], float(s0[b]))
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0
        # ... and the mode stays within the north star's tolerance of the SPEC §3 arithmetic
        cx, trx, _ = Ox.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        assert abs(cost[b] - cx) <= (2e-5 if mlp != "f16" else 2e-4) * abs(cx) and bits_differ(traj[b], trx) > 0      # (another arithmetic, a few 1e-7 apart)
    S.close()


def test_transcendental_instructions_match_their_model():
    """oracle/transc_model.c against the hardware itself (tools/transc_study/libtransc.so: one instruction per element): the recorded binades, the
    rules that cover the rest of the 2^32 inputs (reduction of |x| >= 2, exponent invariance of rcp / rsq, flush to zero, overflow, specials)."""
    import ctypes
    import torch
    so = os.path.join(os.path.dirname(CDIR), "tools", "transc_study", "libtransc.so")
    if not os.path.exists(so):
        pytest.skip("tools/transc_study/libtransc.so not built (python __graft_entry__.py builds it)")
    L = ctypes.CDLL(so)
    L.transc_eval_array.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    rng = np.random.default_rng(5)
    N = 1 << 22
    for func in (0, 1, 2):
        bits = [rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)]                                   # anything, NaNs and sub-normals included
        if func == 2:       # exp: the argument range of a step (|x| up to a few tens), the reduction range, both edges
            bits.append((rng.standard_normal(N) * np.exp2(rng.integers(-32, 8, N))).astype(np.float32).view(np.uint32))
            bits.append(np.concatenate([np.linspace(-152, -120, N // 2), np.linspace(120, 130, N // 2)]).astype(np.float32).view(np.uint32))
        else:               # rcp / rsq: what the step feeds them (1 + e^x >= 1; |q|^2 near 1) and every exponent
            bits.append((1.0 + np.exp2(rng.uniform(-30, 30, N))).astype(np.float32).view(np.uint32))
            bits.append((rng.uniform(0.5, 2.0, N) * np.exp2(rng.integers(-126, 127, N))).astype(np.float32).view(np.uint32))
        xb = np.concatenate(bits + [np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 1, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF,
                                              0xFF7FFFFF, 0x3F800000, 0xBF800000, 0xC2FC0000, 0xC2FC0001, 0x42FFFFFF, 0x43000000], np.uint32)])
        xin = torch.from_numpy(xb.view(np.int32)).cuda()
        out = torch.empty_like(xin)
        assert L.transc_eval_array(func, xin.data_ptr(), xb.size, out.data_ptr()) == 0
        hw = out.cpu().numpy().view(np.uint32)
        model = orc.hw_eval(func, xb.view(np.float32)).view(np.uint32)
        nan = (np.isnan(hw.view(np.float32)) & np.isnan(model.view(np.float32)))
        bad = np.flatnonzero((hw != model) & ~nan)
        assert bad.size == 0, (func, [(hex(xb[i]), hex(hw[i]), hex(model[i])) for i in bad[:5]])


def test_binary16_limb_split_instructions_match_their_statement():
    """SPEC.md §10c rests on two instructions: v_cvt_pk_f16_f32 (round to nearest even to binary16, sub-normals kept, in the kernels' FP mode) and
    v_fma_mix_f32 (x - (float)limb, exact). The split as the kernels write it (tools/transc_study/libtransc.so) against IEEE binary16 rounding (NumPy)
    on 16 million values of the activation range [0, 1], the weights' range, every binary16 boundary case and anything else."""
    import ctypes
    import torch
    so = os.path.join(os.path.dirname(CDIR), "tools", "transc_study", "libtransc.so")
    if not os.path.exists(so):
        pytest.skip("tools/transc_study/libtransc.so not built (python __graft_entry__.py builds it)")
    L = ctypes.CDLL(so)
    if not hasattr(L, "transc_split2h"):
        pytest.skip("libtransc.so predates the limb-split probe")
    L.transc_split2h.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    rng = np.random.default_rng(9)
    N = 1 << 22
    x = np.concatenate([rng.random(N, dtype=np.float32), (1.0 / (1.0 + np.exp2(8 * rng.standard_normal(N)))).astype(np.float32),     # activations r
                        (6 * rng.standard_normal(N) / np.sqrt(32)).astype(np.float32),                                                  # forward weights
                        np.exp2(-rng.uniform(0, 40, N)).astype(np.float32),                                                           # down into the sub-normal limbs and below
                        np.array([0.0, 1.0, 0.5, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.000001, 2.0 ** -26, 65504.0, 65519.0, 1.0009765, 1.00048828125, 1.00146484375,
                                  0.33325195, 6.1e-5, 6.0975e-5, -0.75, -2.0 ** -24], np.float32)])
    if x.size & 1: x = x[:-1]
    xin = torch.from_numpy(x.view(np.int32).copy()).cuda()
    out = torch.empty_like(xin)
    assert L.transc_split2h(xin.data_ptr(), x.size // 2, out.data_ptr()) == 0
    o = out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    l1 = np.stack([o[:, 0] & 0xFFFF, o[:, 0] >> 16], axis=1).reshape(-1).astype(np.uint16)       # low half: the first value of the pair
    l2 = np.stack([o[:, 1] & 0xFFFF, o[:, 1] >> 16], axis=1).reshape(-1).astype(np.uint16)
    w1 = x.astype(np.float16)
    w2 = (x - w1.astype(np.float32)).astype(np.float16)
    assert np.array_equal(l1, w1.view(np.uint16)) and np.array_equal(l2, w2.view(np.uint16))
    # and the pair represents the value to 2^-22 of it at worst (sub-normal second limbs: to 2^-25 absolute)
    rec = w1.astype(np.float64) + w2.astype(np.float64)
    assert np.all(np.abs(rec - x.astype(np.float64)) <= np.maximum(np.abs(x.astype(np.float64)) * 2.0 ** -22, 2.0 ** -25))


# ---- the latency layouts on full-length solves (hundreds of phases: hits, misses, third / fourth trials) ---------------------------
@pytest.mark.parametrize("cfg_name,iters", [("c2_iris_traj_h50_p128.yaml", 200), ("c1_iris_posctrl_h20_p32.yaml", 100), ("iris_traj_shipped_h20_p1.yaml", 200)])
def test_single_instance_full_length_solve_bit_exact(cfg_name, iters, layout):
    cfg = load_mpc_config(os.path.join(CDIR, cfg_name))
    assert cfg.max_iter == iters
    model = synthetic_iris()
    x0, xref, _, _ = _problem(cfg, 1, 21, pos="posctrl" in cfg_name)
    key = orc.split([0, 10], 2)[1][None].astype(np.uint32)
    S = _solver(cfg, model, 1)
    yk, i0 = S.reset()
    s0 = np.array([i0["stepsize"]], np.float32)
    uopt, xevol, info = S.solve_keys(x0, xref, key, yk[None], s0)
    noise = orc.noise_from_key(key[0], cfg.num_particles, cfg.horizon)
    uo, xe, io, _ = orc.Oracle(cfg, model).solve(x0[0], xref[0], noise, yk, float(s0[0]))
    _close(uopt[0], uo, "uopt")
    assert io[2] > 50 and bits_differ(uopt[0], uo) == 0 and bits_differ(xevol[0], xe) == 0 and bits_differ(info[0], io) == 0
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("math_mode", ["fast", "exact"])
def test_c3_single_instance_speculative_kernel_bit_exact(math_mode):
    """C3 (hexarotor, P = 256, H = 50: 300 controls) in the speculative kernel's streamed hand-off: eight particle groups (both four-group chunks of a particle
    total polled in one round), two gradient elements per thread in the head, four groups of 64 workgroups (trials 1 / 2, gradients at y2 / xk: every
    line search that ends on trial 1 is a miss and takes the sequential phases) — a full-length solve against the oracle, both math modes."""
    cfg = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(math_mode=math_mode)
    model = synthetic_hexa()
    x0, xref, _, _ = _problem(cfg, 1, 33)
    key = orc.split([0, 12], 2)[1][None].astype(np.uint32)
    S = _solver(cfg, model, 1)
    yk, i0 = S.reset()
    s0 = np.array([i0["stepsize"]], np.float32)
    uopt, xevol, info = S.solve_keys(x0, xref, key, yk[None], s0)
    assert kc.normalise(S.last_kernel_name()) == ("sdempc_solve_spec_kernel<6, false>", math_mode), S.last_kernel_name()
    noise = orc.noise_from_key(key[0], cfg.num_particles, cfg.horizon)
    orc.set_threads(min(os.cpu_count() or 1, 8))          # (the oracle's particle loops on every core: same bits)
    try:
        uo, xe, io, _ = orc.Oracle(cfg, model).solve(x0[0], xref[0], noise, yk, float(s0[0]))
    finally:
        orc.set_threads(1)
    assert io[2] > 50 and bits_differ(uopt[0], uo) == 0 and bits_differ(xevol[0], xe) == 0 and bits_differ(info[0], io) == 0
    S.close()


# ---- cooperative layouts on a GPU they cannot have to themselves: bounded barrier, fallback to the tile layout ----------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", ["1", "0"])
def test_barrier_timeout_falls_back_to_tile_layout(spec):
    """A spin budget of 0 us (SDEMPC_OPT_COOP_SPIN_US) makes every grid barrier give up on its first unsuccessful poll (what happens,
    after the budget, when the workgroups of a cooperative launch are not all resident). Device API: NaN telemetry + sdempc_solve_status = EDEVICE, and the handle
    leaves the cooperative layouts; host-pointer API: the batch is re-run in the tile layout, results equal the oracle's bit for bit."""
    import torch
    from sde4mbrl_px4_amd.solver import SdempcError
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(horizon=12, num_short_dt=12, num_particles=72, max_iter=6, max_no_improvement_iter=6)
    B = 2
    x0, xref, noise, u = _problem(cfg, B, 5)
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    uo, xo, io = orc.Oracle(cfg, synthetic_iris()).solve_batch(x0, xref, noise, u, s0)
    opts = dict(spec=int(spec), coop_spin_us=0)
    # host-pointer entry point: transparent fallback
    S = _solver(cfg, synthetic_iris(), B, **opts)
    ug, xg, ig = S.solve(x0, xref, noise, u, s0)
    assert S.layout_fallbacks() == 1
    assert bits_differ(ug, uo) == 0 and bits_differ(xg, xo) == 0 and bits_differ(ig, io) == 0
    ug, xg, ig = S.solve(x0, xref, noise, u, s0)                  # the handle stays on the tile layout: no second timeout
    assert S.layout_fallbacks() == 1 and bits_differ(ug, uo) == 0
    assert S.get_option("coop") == 0                               # reported as off after the fallback
    S.close()
    # device entry point: the caller asks for the status
    S = _solver(cfg, synthetic_iris(), B, **opts)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = dict(x0=t(x0), xref=t(xref), nd=t(S.noise_to_device_layout(noise)), u=t(u), s=t(s0))
    uopt, xev, info = torch.zeros((B, 12, 4), device="cuda"), torch.zeros((B, 13, 13), device="cuda"), torch.zeros((B, 8), device="cuda")
    run = lambda: S.solve_dev(B, d["x0"].data_ptr(), d["xref"].data_ptr(), d["nd"].data_ptr(), d["u"].data_ptr(), d["s"].data_ptr(),
                              uopt.data_ptr(), xev.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    run()
    torch.cuda.synchronize()
    with pytest.raises(SdempcError, match="barrier"):
        S.solve_status()
    assert np.isnan(info.cpu().numpy()).any() and S.layout_fallbacks() == 1
    run()
    torch.cuda.synchronize()
    S.solve_status()
    assert bits_differ(uopt.cpu().numpy(), uo) == 0 and bits_differ(info.cpu().numpy(), io) == 0
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", ["1", "0"])
def test_absent_workgroup_gives_up_within_a_few_budgets(spec):
    """A workgroup of a cooperative-layout grid that never becomes resident (fault injection: SDEMPC_OPT_TEST_ABSENT_WG makes one leave at once) with a
    NON-ZERO spin budget: the first grid barrier runs out of budget and raises the error flag; from then on no wait of the kernel may cost another budget
    — neither the later barriers (they see the flag) nor the tagged hand-offs of the reduction phases (they look at the flag too and latch: before
    round 5 each of them waited a full budget, 30 iterations x 20 ms here). The launch must return within a few budgets, report the give-up, and the
    host-pointer entry point must still deliver the oracle's bits through the tile layout."""
    import time
    import torch
    from sde4mbrl_px4_amd.solver import SdempcError
    budget_us, n_it = 20000, 30
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(horizon=12, num_short_dt=12, num_particles=72, max_iter=n_it, max_no_improvement_iter=n_it)
    B = 1
    x0, xref, noise, u = _problem(cfg, B, 5)
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    uo, xo, io = orc.Oracle(cfg, synthetic_iris()).solve_batch(x0, xref, noise, u, s0)
    assert io[0, 2] == n_it                                   # the healthy solve runs all iterations: thirty reduction phases to wait in
    S = _solver(cfg, synthetic_iris(), B, spec=int(spec), coop_spin_us=budget_us)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = dict(x0=t(x0), xref=t(xref), nd=t(S.noise_to_device_layout(noise)), u=t(u), s=t(s0))
    uopt, xev, info = torch.zeros((B, 12, 4), device="cuda"), torch.zeros((B, 13, 13), device="cuda"), torch.zeros((B, 8), device="cuda")
    run = lambda: S.solve_dev(B, d["x0"].data_ptr(), d["xref"].data_ptr(), d["nd"].data_ptr(), d["u"].data_ptr(), d["s"].data_ptr(),
                              uopt.data_ptr(), xev.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    run(); torch.cuda.synchronize(); S.solve_status()              # healthy launch first (module load, workspaces): the oracle's bits, a cooperative kernel
    want = "sdempc_solve_spec_kernel<4, false>" if spec == "1" else kc.coop_kernel(4, 72, B, S.get_option("device_cus"))
    assert bits_differ(uopt.cpu().numpy(), uo) == 0 and kc.normalise(S.last_kernel_name()) == (want, "exact"), S.last_kernel_name()
    S.set_option("test_absent_wg", 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    with pytest.raises(SdempcError, match="barrier"):
        S.solve_status()
    assert np.isnan(info.cpu().numpy()).any() and S.layout_fallbacks() == 1
    assert dt < 4 * budget_us * 1e-6, f"the launch took {dt * 1e3:.0f} ms with a {budget_us / 1e3:.0f} ms budget: a wait behind the give-up cost a budget again"
    assert dt > 0.5 * budget_us * 1e-6                          # (and it did wait for its budget once)
    # host-pointer entry point on a re-armed handle: gives up once more, re-runs in the tile layout, identical results
    S.set_option("coop", 1)
    ug, xg, ig = S.solve(x0, xref, noise, u, s0)
    assert S.layout_fallbacks() == 2 and bits_differ(ug, uo) == 0 and bits_differ(xg, xo) == 0 and bits_differ(ig, io) == 0
    S.set_option("test_absent_wg", -1)
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", ["1", "0"])
@pytest.mark.parametrize("opt", ["coop_launch", "coop_fence"])
def test_runtime_cooperative_launch_and_fenced_barrier_bit_exact(spec, opt):
    """SDEMPC_OPT_COOP_LAUNCH: the cooperative layouts launched through hipLaunchCooperativeKernel; SDEMPC_OPT_COOP_FENCE: agent-scope
    release / acquire fences around every grid barrier. Both give the oracle's bits too."""
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(horizon=12, num_short_dt=12, num_particles=72, max_iter=6, max_no_improvement_iter=6)
    B = 2
    x0, xref, noise, u = _problem(cfg, B, 6)
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    uo, xo, io = orc.Oracle(cfg, synthetic_iris()).solve_batch(x0, xref, noise, u, s0)
    S = _solver(cfg, synthetic_iris(), B, spec=int(spec), **{opt: 1})
    ug, xg, ig = S.solve(x0, xref, noise, u, s0)
    assert S.layout_fallbacks() == 0
    assert bits_differ(ug, uo) == 0 and bits_differ(xg, xo) == 0 and bits_differ(ig, io) == 0
    S.close()


# ---- long horizons: the per-step control table of the throughput solve kernel moves from LDS to global memory -------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,P,m", [(200, 40, 4), (50, 70, 4), (64, 33, 6), (300, 8, 4)])
def test_global_control_table_instantiation_bit_exact(H, P, m):
    """SDEMPC_OPT_USTG = 1 + SDEMPC_OPT_PK = 0 force the instantiation that long-horizon throughput launches pick by themselves (three workgroups per
    CU instead of two at C5): same bits as the oracle, and as the LDS-table instantiation."""
    kw = dict(horizon=H, num_short_dt=H, num_particles=P, u_slew_coeff=1.0, max_iter=4, max_no_improvement_iter=4)
    if m == 6:
        kw.update(input_id=list(range(6)), input_bound=[[1e-4, 1.0]] * 6, uref=[0.42] * 6)
    cfg = MPCConfig(**kw)
    model = synthetic_iris() if m == 4 else synthetic_hexa()
    B = 3
    x0, xref, noise, u = _problem(cfg, B, 9)
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    O = orc.Oracle(cfg, model)
    res = {}
    for flag in ("1", "0", "auto"):          # auto: H = 200 / 300 choose the global table by themselves (3 instead of 2 / 2 instead of 1 per CU)
        S = _solver(cfg, model, B, coop=0, pk=0, ustg={"1": 1, "0": 0, "auto": -1}[flag])
        res[flag] = S.solve(x0, xref, noise, u, s0)
        S.close()
    for b in range(B):
        uo, xe, io, _ = O.solve(x0[b], xref[b], noise[b], u[b], float(s0[b]))
        for flag in ("1", "0", "auto"):
            ug, xg, ig = res[flag]
            assert bits_differ(ug[b], uo) == 0 and bits_differ(xg[b], xe) == 0 and bits_differ(ig[b], io) == 0, (flag, b)


# ---- every single-GPU BASELINE config at FULL size, in the kernel instantiation the bench times ---------------------------------------
# A batch larger than one group per wave holds resident (three workgroups per CU: 768 instances at C2) makes launch_solve_team pick the
# throughput instantiation by itself (three waves per SIMD, scalar tanh; for P > 32 the duo layout, template MODE 3 / 4: sdempc_solve_kernel<TeamPair | TeamBlock, m, F16, false, 3 | 4, USTG> — the kernel `bench.py`
# names in roofline.kernel, read back from the HIP runtime through sdempc_last_kernel_name), with no option forced.
def _full_size_case(cfg_name, B, iters, mlp="f32", sample=(0, 1), seed=0, stepsize=None, math="exact"):
    from sde4mbrl_px4_amd import prng
    cfg = load_mpc_config(os.path.join(CDIR, cfg_name)).replace(max_iter=iters, max_no_improvement_iter=iters, mlp_dtype=mlp, math_mode=math)
    model = synthetic_iris() if cfg.num_motors == 4 else synthetic_hexa()
    pos = "posctrl" in cfg_name
    H, P = cfg.horizon, cfg.num_particles
    x0 = W.random_initial_states(B, seed)
    xref = np.stack([W.constant_reference(W.HOVER, H) if pos else W.reference_window(0.05 * (b % 160), cfg.time_steps) for b in range(B)])
    keys = prng.split(prng.PRNGKey(10), B)                                # launch seed 10 (iris_sdectrl.launch:8), one key per instance
    S = _solver(cfg, model, B)
    assert S.get_option("pk") == -1 and S.get_option("coop") == 1 and S.get_option("ustg") == -1     # nothing forced
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    s0 = np.full(B, i0["stepsize"] if stepsize is None else stepsize, np.float32)
    uopt, xevol, info = S.solve_keys(x0, xref, keys, u0, s0)
    assert S.get_option("device_cus") < B                                 # grid > CUs: the throughput instantiation ran
    kname = S.last_kernel_name()
    ns = "exact" if math == "exact" else "fastm"
    mode = {"f32": 0, "f16": 1, "f32x3": 2}[mlp]
    assert kname.startswith(f"sdempc::{ns}::sdempc_solve_kernel<sdempc::{ns}::Team") and f", {cfg.num_motors}, {mode}, false" in kname, kname
    if P > 32:                                                            # scalar-tanh (throughput) instantiation of the duo layout: MODE 3 (noise
        assert ", false, 3, " in kname or ", false, 4, " in kname, kname  # through LDS staging rows) or, when LDS has no room for them (C5), MODE 4
    # ... and exactly the instantiation the dispatcher's LDS arithmetic picks for this shape and batch (tests/kernel_census.py)
    assert kc.normalise(kname) == (kc.throughput_kernel(H, P, cfg.num_motors, mode, B, S.get_option("device_cus")), "exact" if math == "exact" else "fast"), kname
    assert np.all(info[:, 2] == iters) and np.all(info[:, 6] <= info[:, 5]) and uopt.min() >= 1e-4 and uopt.max() <= 1.0
    O = orc.Oracle(cfg, model)                                            # (math_mode fast: through the instruction model, SPEC.md §10a)
    res = []
    for b in sample:
        noise = orc.noise_from_key(keys[b], P, H)
        res.append((b, O.solve(x0[b], xref[b], noise, u0[b], float(s0[b]))[:3]))
    S.close()
    return uopt, xevol, info, res


@pytest.mark.parametrize("cfg_name,B,iters,sample", [
    ("c2_iris_traj_h50_p128.yaml", 1024, 10, (0, 100, 255, 256, 300, 1023)),    # C2: the bench workload (four particle groups: two per wave in the duo layout)
    ("c3_hexa_traj_h50_p256.yaml", 320, 6, (0, 257, 319)),                      # C3: six rotors, eight particle groups on four waves
    ("c1_iris_posctrl_h20_p32.yaml", 1280, 20, (0, 1025, 1279)),                # C1 geometry: one wave per instance, four instances per workgroup
])
def test_baseline_configs_full_size_throughput_kernel_bit_exact(cfg_name, B, iters, sample):
    uopt, xevol, info, res = _full_size_case(cfg_name, B, iters, sample=sample)
    for b, (uo, xe, io) in res:
        _close(uopt[b], uo, "uopt")
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, b


@pytest.mark.parametrize("mlp", ["f32", "f32x3"])
def test_batches_that_fit_resident_run_one_group_per_wave(mlp):
    """launch_solve_team: an instance of up to four particle groups runs two groups per wave in the duo layout only when the batch is larger
    than one group per wave holds resident (three four-wave workgroups per CU); below that the four-waves-per-instance tile layout is the
    shorter chain (C2: 149 against 245 ms per launch up to 256 instances). Same bits either way, and the oracle's."""
    from sde4mbrl_px4_amd import prng
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(max_iter=6, max_no_improvement_iter=6, mlp_dtype=mlp)
    model = synthetic_iris()
    B, H, P = 300, cfg.horizon, cfg.num_particles
    x0 = W.random_initial_states(B, 5)
    xref = np.stack([W.reference_window(0.05 * (b % 160), cfg.time_steps) for b in range(B)])
    keys = prng.split(prng.PRNGKey(12), B)
    S = _solver(cfg, model, B)
    assert S.get_option("device_cus") < B <= 3 * S.get_option("device_cus")
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    s0 = np.full(B, i0["stepsize"], np.float32)
    uopt, xevol, info = S.solve_keys(x0, xref, keys, u0, s0)
    kn = S.last_kernel_name()
    f16 = kc.F16_OF[mlp]
    assert kc.normalise(kn) == (f"sdempc_solve_kernel<TeamBlock, 4, {f16}, false, 0, false>", "exact"), kn
    S.set_option("duo", 1)
    u2, x2, i2 = S.solve_keys(x0, xref, keys, u0, s0)
    assert kc.normalise(S.last_kernel_name()) == (f"sdempc_solve_kernel<TeamPairT<2>, 4, {f16}, false, 3, false>", "exact"), S.last_kernel_name()
    assert bits_differ(uopt, u2) == 0 and bits_differ(xevol, x2) == 0 and bits_differ(info, i2) == 0
    O = orc.Oracle(cfg, model)
    for b in (0, 299):
        uo, xe, io = O.solve(x0[b], xref[b], orc.noise_from_key(keys[b], P, H), u0[b], float(s0[b]))[:3]
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, b
    S.close()


def test_c2_full_size_fast_math_mode_in_the_duo_layout_bit_exact():
    """`math_mode: fast` (hardware transcendentals, SPEC.md §10) runs the same duo throughput kernels as the exact mode (namespace fastm): full-size
    C2, B > CUs, against the oracle evaluating the three instructions through their model (§10a) — bit for bit, in both f32 contraction arithmetics."""
    for mlp in ("f32", "f32x3"):
        uopt, xevol, info, res = _full_size_case("c2_iris_traj_h50_p128.yaml", 1024, 30, mlp=mlp, sample=(0, 1023), math="fast")
        for b, (uo, xe, io) in res:
            assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, (mlp, b)
            assert np.abs(uopt[b] - 0.71).max() > 1e-4                              # the iterations moved the controls


@pytest.mark.parametrize("config,mlp,math", [("c5", "f16", "exact"), ("c5", "f32x3", "exact"), ("c5", "f16", "fast"), ("c5", "f32x3", "fast"), ("c3", "f32x3", "fast")])
def test_full_length_solves_match_the_committed_oracle_results(config, mlp, math):
    """BASELINE config 5 end to end in its own mode (`mlp_dtype: f16`; and in f32x3), in BOTH math modes — `fast` is the arithmetic bench.py's C5 legs time —
    and config 3 in the arithmetic bench.py times it in: ONE full-length solve each (C5: H = 200, P = 1024, 200 iterations, ~400 line-search rollouts) against
    what the CPU oracle computed for the same instance (tests/golden/make_c5_fullsize.py: 10 - 60 minutes on one core, hence committed rather than
    recomputed), bit for bit: uopt, xevol, the eight telemetry words."""
    import importlib.util
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_c5_fullsize", os.path.join(gdir, "make_c5_fullsize.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    assert (config, mlp, math) in mk.COMMITTED
    g = np.load(mk.golden_path(mlp, math, config))
    cfg, x0, xref, key = mk.problem(mlp, math, config)
    assert cfg.math_mode == math and cfg.mlp_dtype == mlp
    S = _solver(cfg, mk.model_of(config), 1)
    yk, i0 = S.reset()
    assert bits_differ(yk, g["u0"]) == 0 and np.float32(i0["stepsize"]) == g["stepsize"]
    uopt, xevol, info = S.solve_keys(x0, xref, key, yk[None], np.array([i0["stepsize"]], np.float32))
    assert info[0, 2] == 200 and info[0, 7] > 300
    assert bits_differ(uopt[0], g["uopt"]) == 0 and bits_differ(xevol[0], g["xevol"]) == 0 and bits_differ(info[0], g["info"]) == 0
    S.close()


def test_ticketed_persistent_launch_matches_striped_launches_bit_for_bit():
    """From three instances per team on, a persistent duo launch hands its instances out by ticket (order of completion) instead of striping
    them over the teams (sdempc_kernels.hip, launch_persistent). Which team solves an instance must not change a bit: C2 at B = 4700 (> 3 x
    1536 team slots: ticketed) against the same instances solved in striped launches of 600, and against the oracle on two of them."""
    from sde4mbrl_px4_amd import prng
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(max_iter=2, max_no_improvement_iter=2)
    model = synthetic_iris()
    B, H, P = 4700, cfg.horizon, cfg.num_particles
    x0 = W.random_initial_states(B, 3)
    xref = np.stack([W.reference_window(0.05 * (b % 160), cfg.time_steps) for b in range(B)])
    keys = prng.split(prng.PRNGKey(10), B)
    S = _solver(cfg, model, B)
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    s0 = np.full(B, i0["stepsize"], np.float32)
    S.work_counters(reset=True)
    uopt, xevol, info = S.solve_keys(x0, xref, keys, u0, s0)
    assert 3 * 6 * S.get_option("device_cus") <= B
    assert kc.normalise(S.last_kernel_name()) == ("sdempc_solve_kernel<TeamPairT<6>, 4, 0, false, 3, false>", "exact")    # a launch that fills the device: one six-team workgroup per CU
    assert S.work_counters()[0] == B                                      # every instance solved exactly once
    S.set_option("hex", 0)                                                # the same launch in two-team workgroups (three per CU): same bits
    uh, xh, ih = S.solve_keys(x0, xref, keys, u0, s0)
    assert kc.normalise(S.last_kernel_name()) == ("sdempc_solve_kernel<TeamPairT<2>, 4, 0, false, 3, false>", "exact"), S.last_kernel_name()
    assert bits_differ(uopt, uh) == 0 and bits_differ(xevol, xh) == 0 and bits_differ(info, ih) == 0
    S.set_option("hex", 1)
    S.work_counters(reset=True)
    assert S.solve_keys(x0, xref, keys, u0, s0)[0].tobytes() == uopt.tobytes() and S.work_counters()[0] == B
    ub, xb, ib = S.solve_keys(x0, xref, keys, u0, s0)                     # second ticketed launch of the handle: the ticket word is not reset between launches
    assert S.work_counters()[0] == 2 * B and bits_differ(uopt, ub) == 0 and bits_differ(xevol, xb) == 0 and bits_differ(info, ib) == 0
    for sl in (slice(0, 600), slice(2300, 2900), slice(4100, 4700)):
        u2, x2, i2 = S.solve_keys(x0[sl], xref[sl], keys[sl], u0[sl], s0[sl])
        assert bits_differ(uopt[sl], u2) == 0 and bits_differ(xevol[sl], x2) == 0 and bits_differ(info[sl], i2) == 0
    O = orc.Oracle(cfg, model)
    for b in (1536, 4699):
        uo, xe, io = O.solve(x0[b], xref[b], orc.noise_from_key(keys[b], P, H), u0[b], float(s0[b]))[:3]
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0
    S.close()


@pytest.mark.parametrize("m,mlp", [(4, "f16"), (6, "f32x3"), (6, "f32"), (8, "f16"), (8, "f32x3")])
def test_six_team_workgroups_every_motor_count_and_contraction_mode(m, mlp):
    """The six-team workgroup (TeamHex, launches that fill every team slot of the device) exists per motor count (4 / 6 / 8 motor
    instantiations) and contraction mode; the ticket test covers (4, f32), bench.py's verification (4, f32x3). Here the others, small
    horizon, 1,700 instances: sampled instances against the oracle, the whole batch against the same launch in two-team workgroups."""
    from sde4mbrl_px4_amd import prng
    model = synthetic_multirotor(m, seed=3) if m == 8 else (synthetic_iris() if m == 4 else synthetic_hexa())
    kw = dict(horizon=7, num_short_dt=4, long_step_dt=0.1, num_particles=70, u_slew_coeff=1.0, max_iter=3, max_no_improvement_iter=3, mlp_dtype=mlp)
    if m != 4:
        kw.update(input_id=list(range(m)), input_bound=[[1e-4, 1.0]] * m, uref=[0.42] * m)
    cfg = MPCConfig(**kw)
    B, H, P = 1700, cfg.horizon, cfg.num_particles
    x0 = W.random_initial_states(B, 11)
    xref = np.stack([W.reference_window(0.05 * (b % 97), cfg.time_steps) for b in range(B)])
    keys = prng.split(prng.PRNGKey(4), B)
    S = _solver(cfg, model, B)
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    s0 = np.full(B, i0["stepsize"], np.float32)
    uopt, xevol, info = S.solve_keys(x0, xref, keys, u0, s0)
    from sde4mbrl_px4_amd import _abi
    if m == 8 and not (_abi.load_library().sdempc_build_flags() & 1):
        # the default build carries the generic motor count in the one-group-per-wave tile layouts only (make EXTRA=-DSDEMPC_ALL_VARIANTS=1 adds the rest;
        # include/sdempc.h: sdempc_build_flags): same bits from another layout
        assert kc.normalise(S.last_kernel_name()) == (f"sdempc_solve_kernel<TeamBlock, 8, {kc.F16_OF[mlp]}, false, 0, false>", "exact"), S.last_kernel_name()
    else:
        assert kc.normalise(S.last_kernel_name()) == (f"sdempc_solve_kernel<TeamPairT<6>, {m}, {kc.F16_OF[mlp]}, false, 3, false>", "exact"), S.last_kernel_name()
        S.set_option("hex", 0)
        u2, x2, i2 = S.solve_keys(x0, xref, keys, u0, s0)
        assert kc.normalise(S.last_kernel_name()) == (f"sdempc_solve_kernel<TeamPairT<2>, {m}, {kc.F16_OF[mlp]}, false, 3, false>", "exact"), S.last_kernel_name()
        assert bits_differ(uopt, u2) == 0 and bits_differ(xevol, x2) == 0 and bits_differ(info, i2) == 0
    O = orc.Oracle(cfg, model)
    for b in (0, 5, 1535, 1536, B - 1):
        uo, xe, io = O.solve(x0[b], xref[b], orc.noise_from_key(keys[b], P, H), u0[b], float(s0[b]))[:3]
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, b
    S.close()


def test_workspaces_scale_with_team_slots_not_with_the_batch():
    """A persistent throughput launch indexes its trajectory / checkpoint / partial-sum workspaces by team slot (1,536 on an MI355X), not by
    instance: a C2 launch of 98,304 instances (64 rounds of the grid) takes the device memory of its inputs and outputs (15 GB of noise)
    plus 2.3 GB of workspace — per-instance workspaces would add 150 GB — and every instance is solved exactly once, bit for bit."""
    import torch
    from sde4mbrl_px4_amd import prng
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(max_iter=1, max_no_improvement_iter=1, mlp_dtype="f32x3")
    model = synthetic_iris()
    B, H, P = 98304, cfg.horizon, cfg.num_particles
    x0 = W.random_initial_states(B, 7)
    xr1 = np.stack([W.reference_window(0.05 * b, cfg.time_steps) for b in range(160)])
    xref = xr1[np.arange(B) % 160]
    keys = prng.split(prng.PRNGKey(10), B)
    free0, _ = torch.cuda.mem_get_info(0)
    S = _solver(cfg, model, B)
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    s0 = np.full(B, i0["stepsize"], np.float32)
    S.work_counters(reset=True)
    uopt, xevol, info = S.solve_keys(x0, xref, keys, u0, s0)
    free1, _ = torch.cuda.mem_get_info(0)
    assert S.work_counters()[0] == B
    used = (free0 - free1) / 2**30
    assert used < 26.0, f"{used:.1f} GiB of device memory for a {B}-instance launch"
    O = orc.Oracle(cfg, model)
    for b in (0, 1535, 1536, 50000, B - 1):
        uo, xe, io = O.solve(x0[b], xref[b], orc.noise_from_key(keys[b], P, H), u0[b], float(s0[b]))[:3]
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, b
    S.close()


@pytest.mark.parametrize("mlp", ["f32", "f16", "f32x3"])
def test_c5_full_size_solve_bit_exact(mlp):
    """BASELINE config C5 (H=200, P=1024: 32 particle groups per instance, control table in global memory) as a SOLVE at full size, B > CUs,
    bit for bit against the oracle in all three contraction modes — f32, the fp16-operand MLP mode C5 names (SPEC.md §9), and the three-limb
    bf16 split (§9b); the two matrix-pipe modes through the oracle's model of the instruction (§9a).
    The 10 s open-loop horizon from a random initial state is violently ill-conditioned (|g|^2 ~ 1e16): the solve starts from a step size of
    1e-11 so that its three iterations all take steps (from the YAML's 0.01 the line search only shrinks the step for the first dozens)."""
    uopt, xevol, info, res = _full_size_case("c5_iris_traj_h200_p1024.yaml", 260, 3, mlp=mlp, sample=(259,), stepsize=1e-11)
    for b, (uo, xe, io) in res:
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0
    assert info[259, 6] < 0.7 * info[259, 5] and np.abs(uopt[259] - 0.71).max() > 1e-4      # the iterations moved the controls


@pytest.mark.parametrize("cfg_name,B,iters,sample", [
    ("c2_iris_traj_h50_p128.yaml", 1024, 10, (0, 257, 1023)),                   # C2: the bench workload in the f32x3 mode bench.py reports
    ("c3_hexa_traj_h50_p256.yaml", 320, 4, (319,)),
])
def test_baseline_configs_full_size_f32x3_bit_exact(cfg_name, B, iters, sample):
    uopt, xevol, info, res = _full_size_case(cfg_name, B, iters, mlp="f32x3", sample=sample)
    for b, (uo, xe, io) in res:
        _close(uopt[b], uo, "uopt")
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, b


# ---- duo tile layout (64 particles per wave) against the one-group-per-wave layout and the oracle -------------------------------------
@pytest.mark.parametrize("H,P,m", [(9, 33, 4), (12, 64, 4), (7, 65, 6), (10, 128, 4), (6, 160, 4), (5, 257, 8), (200, 40, 4), (50, 300, 6)])
def test_duo_tile_layout_bit_exact(H, P, m):
    """SDEMPC_OPT_PK = 0 pins the throughput instantiation on a small batch; SDEMPC_OPT_DUO picks 64 particles per wave (default) or one
    32-particle group per wave. Odd group counts (a pair without a group B), ragged last groups, two- and four-wave teams, the control
    table in LDS and in global memory: all give the oracle's bits."""
    kw = dict(horizon=H, num_short_dt=max(1, H // 2), long_step_dt=0.1, num_particles=P, u_slew_coeff=1.0, max_iter=5, max_no_improvement_iter=5)
    if m != 4:
        kw.update(input_id=list(range(m)), input_bound=[[1e-4, 1.0]] * m, uref=[0.42] * m)
    cfg = MPCConfig(**kw)
    model = synthetic_multirotor(m, seed=3) if m == 8 else (synthetic_iris() if m == 4 else synthetic_hexa())
    B = 3
    x0, xref, noise, u = _problem(cfg, B, 13)
    s0 = np.full(B, cfg.ls_init_stepsize, np.float32)
    O = orc.Oracle(cfg, model)
    ref = [O.solve(x0[b], xref[b], noise[b], u[b], float(s0[b]))[:3] for b in range(B)]
    for opts in (dict(duo=1), dict(duo=0), dict(duo=1, ustg=1), dict(duo=1, ustg=0)):
        S = _solver(cfg, model, B, coop=0, pk=0, **opts)
        ug, xg, ig = S.solve(x0, xref, noise, u, s0)
        S.close()
        for b in range(B):
            assert bits_differ(ug[b], ref[b][0]) == 0 and bits_differ(xg[b], ref[b][1]) == 0 and bits_differ(ig[b], ref[b][2]) == 0, (opts, b)


def test_work_counters_and_gradient_reuse():
    """sdempc_work_counters: a cold start whose first iterations fail at the same point (the line search only shrinks the step) re-uses the
    gradient instead of re-evaluating it: fewer gradient evaluations than iterations, identical results (the oracle evaluates every one)."""
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(max_iter=14, max_no_improvement_iter=14)
    model = synthetic_iris()
    B = 2
    x0, xref, noise, _ = _problem(cfg, B, 31)
    S = _solver(cfg, model, B, coop=0)
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    s0 = np.full(B, i0["stepsize"], np.float32)
    ug, xg, ig = S.solve(x0, xref, noise, u0, s0)
    solves, grads, fwd = S.work_counters()
    assert solves == B and fwd == int(ig[:, 7].sum()) + 2 * B
    assert grads < int(ig[:, 2].sum()) and grads >= B                    # some iterations re-used their gradient
    S.work_counters(reset=True)
    assert S.work_counters() == (0, 0, 0)
    O = orc.Oracle(cfg, model)
    for b in range(B):
        uo, xe, io, _ = O.solve(x0[b], xref[b], noise[b], u0[b], float(s0[b]))
        assert bits_differ(ug[b], uo) == 0 and bits_differ(xg[b], xe) == 0 and bits_differ(ig[b], io) == 0
    S.close()
