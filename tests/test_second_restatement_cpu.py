"""The second, independent restatement of SPEC.md (oracle/sde_mpc_numpy.py: NumPy float32 with an exact software fma, all particles at
once; torch float64 autograd for the gradient) against the C oracle. Pins the oracle against a shared-mistake-free second writing of the
same specification; both remain unpinned against the reference's JAX path, which cannot run here."""
import os
import sys

import numpy as np
import pytest

import orc
from cases import ROOT, asymmetric_cfg, asymmetric_model, asymmetric_problem, bits_differ
from sde4mbrl_px4_amd import MPCConfig, synthetic_hexa, synthetic_iris, synthetic_multirotor
from sde4mbrl_px4_amd import workload as W

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import sde_mpc_numpy as R2  # noqa: E402


def _asymmetric(m, **kw):
    """The asymmetric fixtures (tests/cases.py): instance 1 of 2 carries the 150 degree attitude AND the negated quaternion."""
    cfg = asymmetric_cfg(m, **kw)
    x0, xref, noise, u = asymmetric_problem(cfg, 2, 17)
    return cfg, asymmetric_model(m), x0[1], xref[1], noise[1], u[1]


def _case(name):
    if name.startswith("asymmetric"):       # no symmetry, no zero term, per-motor-distinct settings; m = 4 / 6 / generic (8-slot tables)
        m = {"asymmetric": 4, "asymmetric_hexa": 6, "asymmetric_m5": 5}[name]
        return _asymmetric(m, horizon=8, num_short_dt=5, long_step_dt=0.1, num_particles=40 if m == 4 else 9, max_iter=7, max_no_improvement_iter=7)
    if name == "iris":
        cfg = MPCConfig(horizon=8, num_short_dt=5, long_step_dt=0.1, num_particles=40, u_slew_coeff=1.0, max_iter=7, max_no_improvement_iter=7)
        model = synthetic_iris()
    elif name == "hexa_slew_constr":
        cfg = MPCConfig(horizon=6, num_short_dt=6, num_particles=33, discount=0.95, input_id=list(range(6)), input_bound=[[1e-4, 1.0]] * 6, uref=[0.42] * 6,
                        u_slew_coeff=0.5, u_slew_constr=[[-0.05, 0.04]] * 6, u_slew_constr_coeff=7.0, res_mult=0.5, max_iter=6, max_no_improvement_iter=3,
                        moment_scale=0.8, ls_maxls=3)
        model = synthetic_hexa()
    elif name == "state_constr":
        cfg = MPCConfig(horizon=7, num_short_dt=7, num_particles=35, u_slew_coeff=1.0, max_iter=6, max_no_improvement_iter=6,
                        state_id=[3, 4, 5, 10, 11, 12], state_penalty=[10.0, 10.0, 20.0, 10.0, 10.0, 10.0], constr_pen=0.1,
                        state_bound=[[-0.5, 0.5], [-0.5, 0.5], [-0.4, 0.7], [-0.8, 0.8], [-0.8, 0.8], [-0.7, 0.7]])      # iris_sitl_traj_mpc.yaml:16-29
        model = synthetic_iris()
    else:   # one particle, three rotors, fixed step size, no bounds
        cfg = MPCConfig(horizon=9, num_short_dt=9, num_particles=1, input_id=[0, 1, 2], input_bound=[[1e-4, 1.0]] * 3, uref=[0.6] * 3, enforce_ubound=False,
                        ls_maxls=0, stepsize=2e-4, max_iter=5, max_no_improvement_iter=5)
        model = synthetic_multirotor(3, seed=4)
    H, P, m = cfg.horizon, cfg.num_particles, cfg.num_motors
    x0 = W.random_initial_states(1, 17)[0]
    xref = W.reference_window(0.3, cfg.time_steps)
    noise = W.make_noise(1, P, H, 5)[0]
    u = np.clip(np.asarray(cfg.uref, np.float32) + 0.1 * np.random.default_rng(2).standard_normal((H, m)), 1e-4, 1).astype(np.float32)
    return cfg, model, x0, xref, noise, u


CASES = ["iris", "hexa_slew_constr", "single_particle", "state_constr", "asymmetric"]
MORE_ASYMMETRIC = ["asymmetric_hexa", "asymmetric_m5"]


def test_software_fma_is_exact():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 20000).astype(np.float32) for _ in range(3))
    c = np.where(rng.random(20000) < 0.5, -(a * b), c).astype(np.float32)          # heavy cancellation: the case double rounding gets wrong
    got = R2.fma(a, b, c)
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert bits_differ(got, want) == 0


def test_elementary_functions_match_the_c_oracle_bit_for_bit():
    x = np.concatenate([np.linspace(-12, 12, 4001), np.random.default_rng(1).standard_normal(2000) * 3]).astype(np.float32)
    x = x[: (x.size // 4) * 4]
    t = R2.tanh4(x.reshape(-1, 4)).reshape(-1)
    want = np.zeros_like(x)
    L = orc.lib()
    import ctypes as C
    for i in range(0, x.size, 4):
        L.orc_tanh4(x[i:i + 4].ctypes.data_as(C.POINTER(C.c_float)), want[i:i + 4].ctypes.data_as(C.POINTER(C.c_float)))
    assert bits_differ(t, want) == 0
    pos = np.abs(x) + np.float32(1e-3)
    assert bits_differ(R2.rcp(pos), np.array([L.orc_rcp(float(v)) for v in pos], np.float32)) == 0
    assert bits_differ(R2.rsqrt(pos), np.array([L.orc_rsqrt(float(v)) for v in pos], np.float32)) == 0
    assert bits_differ(R2.sigmoid(x * 4), np.array([L.orc_sigmoid(float(v)) for v in x * 4], np.float32)) == 0


@pytest.mark.parametrize("name", CASES + MORE_ASYMMETRIC)
def test_forward_rollout_bit_identical_to_the_c_oracle(name):
    cfg, model, x0, xref, noise, u = _case(name)
    O, N = orc.Oracle(cfg, model), R2.Restatement(cfg, model)
    c_o, traj_o, mean_o = O.rollout(x0, u, xref, noise, want_traj=True, want_mean=True)
    c_n, traj_n, mean_n = N.rollout(x0, u, xref, noise)
    assert np.float32(c_o) == c_n and bits_differ(traj_n, traj_o) == 0 and bits_differ(mean_n, mean_o) == 0


@pytest.mark.parametrize("name", CASES + MORE_ASYMMETRIC)
def test_adjoint_sweep_bit_identical_to_the_c_oracle(name):
    """SPEC.md §5.4-§5.5 written a second time (all particles at once, NumPy float32 with the exact software fma): cost and gradient of the
    second restatement equal the C oracle's bit for bit — the hand-derived vector-Jacobian product is no longer a single point of failure."""
    cfg, model, x0, xref, noise, u = _case(name)
    O, N = orc.Oracle(cfg, model), R2.Restatement(cfg, model)
    c_o, g_o = O.grad(x0, u, xref, noise)
    c_n, g_n = N.cost_grad(x0, u, xref, noise)
    assert np.float32(c_o) == c_n and bits_differ(g_n, g_o.astype(np.float32)) == 0


@pytest.mark.parametrize("name", CASES)
def test_full_solve_of_the_second_restatement_bit_identical_to_the_c_oracle(name):
    """SPEC.md §8 on the second restatement's OWN cost and gradient (no oracle callback anywhere): same iterates, same line-search
    decisions, same telemetry as the C oracle's solve."""
    cfg, model, x0, xref, noise, u = _case(name)
    O, N = orc.Oracle(cfg, model), R2.Restatement(cfg, model)
    s0 = cfg.ls_init_stepsize if cfg.ls_maxls > 0 else cfg.stepsize
    uo, _, info_o, _ = O.solve(x0, xref, noise, u, s0)
    un, info_n = N.solve_own(x0, xref, noise, u, s0)
    assert info_o[2] >= 3 and bits_differ(un, uo) == 0 and bits_differ(info_n, info_o) == 0


@pytest.mark.parametrize("name", CASES)
def test_adjoint_against_reverse_mode_autodiff(name):
    """The hand-derived vector-Jacobian product of the oracle (SPEC.md §5.4-§5.5) against torch.autograd on a float64 writing of the model
    that shares no code with it: float64 oracle build to 1e-6 (its tables — discount powers, sigma sqrt(dt) — are computed in float64, here
    in float32 as SPEC.md says), float32 oracle (software tanh, f32 accumulation) to 2e-4 of the largest entry."""
    import torch
    cfg, model, x0, xref, noise, u = _case(name)
    ut = torch.tensor(u.astype(np.float64), requires_grad=True)
    J = R2.torch_cost(cfg, model, x0, ut, xref, noise)
    J.backward()
    g_ad = ut.grad.numpy()
    c64, g64 = orc.Oracle(cfg, model, double=True).grad(x0, u, xref, noise)
    c32, g32 = orc.Oracle(cfg, model).grad(x0, u, xref, noise)
    scale = np.abs(g_ad).max()
    Jv = float(J.detach())
    assert abs(c64 - Jv) <= 1e-6 * abs(Jv)
    np.testing.assert_allclose(g64, g_ad, rtol=0, atol=1e-6 * scale)
    np.testing.assert_allclose(g32, g_ad, rtol=0, atol=2e-4 * scale)
    assert abs(c32 - Jv) <= 2e-5 * abs(Jv)


# ---- the matrix-pipe modes (SPEC.md §9, §9a, §9b) written a second time: Python-integer model of the instruction, NumPy around it ------------------
@pytest.mark.parametrize("dtn", ["f16", "bf16"])
def test_second_model_of_the_matrix_instruction_reproduces_the_hardware(dtn):
    """oracle/sde_mpc_numpy.py: mfma16_dot (exact Python integers, no fast paths) against the recorded hardware answers — every fifth one of the
    committed sample — and therefore against oracle/mfma16_model.c on the same inputs."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"mfma16_{dtn}.npz"))
    bad = []
    for n in range(0, len(g["d"]), 5):
        c = g["c"][n:n + 1].view(np.float32)[0]
        if not np.isfinite(c):
            continue
        got = np.asarray(R2.mfma16_dot(dtn == "bf16", g["a"][n], g["b"][n], c), np.float32).view(np.uint32)
        if got != g["d"][n]:
            bad.append(n)
    assert not bad, bad[:5]


@pytest.mark.parametrize("mlp,vehicle", [("f32x3", "iris"), ("f16", "iris"), ("f32x3", "asymmetric"), ("f16", "asymmetric")], ids=["f32x3", "f16", "f32x3-asymmetric", "f16-asymmetric"])
def test_matrix_pipe_modes_bit_identical_to_the_c_oracle(mlp, vehicle):
    """Rollout, gradient and a short full solve of a tiny problem (2 particles, 3 steps) in the two matrix-pipe modes: the second restatement
    (limb split / fp16 rounding in NumPy, the instruction in Python integers) equals the C oracle bit for bit."""
    cfg = MPCConfig(horizon=3, num_short_dt=2, long_step_dt=0.1, num_particles=2, u_slew_coeff=1.0, max_iter=2, max_no_improvement_iter=2, mlp_dtype=mlp)
    model = synthetic_iris()
    x0 = W.random_initial_states(1, 3)[0]
    xref = W.reference_window(0.1, cfg.time_steps)
    noise = W.make_noise(1, 2, 3, 2)[0]
    u = np.clip(0.71 + 0.1 * np.random.default_rng(1).standard_normal((3, 4)), 1e-4, 1).astype(np.float32)
    if vehicle == "asymmetric":
        cfg, model, x0, xref, noise, u = _asymmetric(4, horizon=3, num_short_dt=2, long_step_dt=0.1, num_particles=2, max_iter=2, max_no_improvement_iter=2, mlp_dtype=mlp)
    O, N = orc.Oracle(cfg, model), R2.Restatement(cfg, model)
    c_o, traj_o, mean_o = O.rollout(x0, u, xref, noise, want_traj=True, want_mean=True)
    c_n, traj_n, mean_n = N.rollout(x0, u, xref, noise)
    assert np.float32(c_o) == c_n and bits_differ(traj_n, traj_o) == 0 and bits_differ(mean_n, mean_o) == 0
    c_o, g_o = O.grad(x0, u, xref, noise)
    c_n, g_n = N.cost_grad(x0, u, xref, noise)
    assert np.float32(c_o) == c_n and bits_differ(g_n, g_o.astype(np.float32)) == 0
    uo, _, info_o, _ = O.solve(x0, xref, noise, u, 0.01)
    un, info_n = N.solve_own(x0, xref, noise, u, 0.01)
    assert bits_differ(un, uo) == 0 and bits_differ(info_n, info_o) == 0


def _hw():
    return R2.HwTransc(orc.TRANSC_DIR)


@pytest.mark.parametrize("func", ["rcp", "rsq", "exp2"])
def test_second_model_of_the_transcendental_instructions_equals_the_c_model(func):
    """SPEC.md §10a in NumPy (whole arrays, blocks read straight from the committed files) against oracle/transc_model.c: every special class, the
    edges of every rule, and 300,000 random bit patterns per function — bit for bit (NaN payloads included)."""
    rng = np.random.default_rng({"rcp": 1, "rsq": 2, "exp2": 3}[func])
    u = rng.integers(0, 2 ** 32, size=300_000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0x7F800001, 0xFFC12345, 0x7E800000, 0x7F000000, 0x7E000000, 0x42FE0000, 0x42FFFFFF, 0x43000000, 0xC2FC0000, 0xC2FE0000, 0xC3000000,
                     0xC3150000, 0x30800000, 0x307FFFFF, 0xB0800000, 0x3FFFFFFF, 0x40000000, 0xC0000000, 0x40000001], np.uint32)
    near = (np.array([0x3F800000, 0x40000000, 0x42FE0000, 0x30800000, 0x00800000], np.uint32)[:, None] + np.arange(-64, 64, dtype=np.int64)[None, :]).astype(np.uint32).ravel()
    if func == "exp2":      # (most random patterns are huge: add arguments of the size the activations see)
        u = np.concatenate([u, (rng.standard_normal(200_000) * 8).astype(np.float32).view(np.uint32)])
    x = np.concatenate([u, edge, near]).view(np.float32)
    got = getattr(_hw(), func)(x)
    want = orc.hw_eval({"rcp": 0, "rsq": 1, "exp2": 2}[func], x)
    assert bits_differ(got, want) == 0


@pytest.mark.parametrize("mlp,vehicle", [(d, v) for v in ("iris", "asymmetric") for d in ("f32", "f32x3", "f16")],
                         ids=["f32", "f32x3", "f16", "f32-asymmetric", "f32x3-asymmetric", "f16-asymmetric"])
def test_fast_math_mode_bit_identical_to_the_c_oracle(mlp, vehicle):
    """math_mode fast written a second time (SPEC.md §10b: the weight sets built in NumPy float32, the activation kept as r, the three instructions
    through the NumPy statement of §10a): rollout, gradient and a short full solve equal the C oracle bit for bit, in every contraction arithmetic."""
    big = mlp == "f32"
    H, P = (6, 9) if big else (3, 2)
    cfg = MPCConfig(horizon=H, num_short_dt=2, long_step_dt=0.1, num_particles=P, u_slew_coeff=1.0, res_mult=0.5, max_iter=3 if big else 2, max_no_improvement_iter=3,
                    mlp_dtype=mlp, math_mode="fast")
    model = synthetic_iris()
    x0 = W.random_initial_states(1, 3)[0]
    xref = W.reference_window(0.1, cfg.time_steps)
    noise = W.make_noise(1, P, H, 2)[0]
    u = np.clip(0.71 + 0.1 * np.random.default_rng(1).standard_normal((H, 4)), 1e-4, 1).astype(np.float32)
    if vehicle == "asymmetric":     # (b3, b3n != 0: the folded biases of SPEC.md §10b start from them)
        cfg, model, x0, xref, noise, u = _asymmetric(4, horizon=H, num_short_dt=2, long_step_dt=0.1, num_particles=P, max_iter=3 if big else 2, max_no_improvement_iter=3,
                                                     mlp_dtype=mlp, math_mode="fast")
    O, N = orc.Oracle(cfg, model), R2.Restatement(cfg, model, hw=_hw())
    c_o, traj_o, mean_o = O.rollout(x0, u, xref, noise, want_traj=True, want_mean=True)
    c_n, traj_n, mean_n = N.rollout(x0, u, xref, noise)
    assert np.float32(c_o) == c_n and bits_differ(traj_n, traj_o) == 0 and bits_differ(mean_n, mean_o) == 0
    c_o, g_o = O.grad(x0, u, xref, noise)
    c_n, g_n = N.cost_grad(x0, u, xref, noise)
    assert np.float32(c_o) == c_n and bits_differ(g_n, g_o.astype(np.float32)) == 0
    uo, _, info_o, _ = O.solve(x0, xref, noise, u, 0.01)
    un, info_n = N.solve_own(x0, xref, noise, u, 0.01)
    assert bits_differ(un, uo) == 0 and bits_differ(info_n, info_o) == 0
    # and the mode stays what it claims to be: the exact arithmetic's gradient to 1e-5 of its largest entry (f16: the operands are quantised differently)
    E = orc.Oracle(cfg.replace(math_mode="exact"), model)
    _, g_e = E.grad(x0, u, xref, noise)
    assert np.abs(g_e - g_o).max() <= (2e-3 if mlp == "f16" else 1e-5) * np.abs(g_e).max()
