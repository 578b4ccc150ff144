"""The kernels on models OFF the synthetic weight scale (tests/scale_cases.py; SPEC.md §10e), against the CPU oracle, bit for bit.

H = 8, B = 3. Layouts (tests/KERNELS.md): P = 32 `coop=0` TeamWave, P = 33 `coop=0 duo=0` TeamBlock, P = 70 `coop=0 duo=1` TeamPairT<2> (its adjoint is reached
by the solve only), P = 130 `coop=0` TeamBlock mode 3. Every case runs `grad` and a six-iteration `solve`; every assertion is bits_differ(...) == 0.

Cases: both ends of the band the output-layer normalisation leaves alone (uniform k = -2, 2), one k beyond each end where only SOME rows are normalised (k = -3, 3),
one far beyond each end (k = -14, 16) — those two must ALSO equal the device result of the canonical model (every row at the target binade: the k = 0 of the
normalisation) bit for bit —, both spread cases, two models with eoff in 5 .. 9, the f16_rtz_host branch models, and the 2^-110 cost (gradient only).
The fast matrix-pipe modes run every case on all four layouts; f32x3/exact and f16/exact (no normalisation, the f32 chain on
W3) run at P = 33 and P = 70. The eoff = -40 model cannot be evaluated with binary16 limbs (its scaled adjoints flush to zero): it is one of the refused models."""
import functools

import numpy as np
import pytest

import cases as CS
import kernel_census as kc
import scale_cases as SC
from cases import bits_differ
from plant_loop_ref import plant_loop_ref
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import SdeMpcSolver, SdempcError
from test_gpu_asymmetric import oracle_threads
from test_gpu_closed_loop import assert_same

pytestmark = pytest.mark.gpu

B = 3
MODE = {"f32": 0, "f16": 1, "f32x3": 2}
TEAM = {32: "sdempc_solve_kernel<TeamWave, 4, {md}, false, 0, false>", 33: "sdempc_solve_kernel<TeamBlock, 4, {md}, false, 0, false>",
        70: "sdempc_solve_kernel<TeamPairT<2>, 4, {md}, false, 3, false>", 130: "sdempc_solve_kernel<TeamBlock, 4, {md}, false, 3, false>"}
FAST_CASES = ("k-2", "k+2", "k-3", "k+3", "k-14", "k+16", "spread_torque_low", "spread_force_low", "eoff_mid", "w2+4", "f16_subnormal", "f16_normal", "tiny_cost")


def _model(name):
    return SC.canonical(SC.base_model()) if name == "canonical" else SC.base_model() if name == "tiny_cost" else SC.model_of(name)


def _cfg(name, mlp, mm, P):
    cfg = SC.config(P, mlp, mm)
    return SC.tiny_cost_cfg(cfg) if name == "tiny_cost" else cfg


@functools.lru_cache(maxsize=None)
def _oracle(name, mlp, mm, P):
    cfg, M = _cfg(name, mlp, mm, P), _model(name)
    with oracle_threads():
        return SC.oracle_grads(cfg, M, B), (None if name == "tiny_cost" else SC.oracle_solves(cfg, M, B))


@functools.lru_cache(maxsize=None)
def _device(name, mlp, mm, P):
    cfg, M = _cfg(name, mlp, mm, P), _model(name)
    x0, u, xref, noise = SC.problem(P, B)
    S = SdeMpcSolver(cfg, M, max_batch=B, options=SC.LAYOUTS[P])
    gc, g = S.grad(x0, u, xref, noise)
    sol = kname = None
    if name != "tiny_cost":
        sol = S.solve(x0, xref, noise, u, np.full(B, cfg.ls_init_stepsize, np.float32))
        kname = S.last_kernel_name()
    S.close()
    return (gc, g), sol, kname


def _check(name, mlp, mm, P):
    (gc, g), sol, kname = _device(name, mlp, mm, P)
    (oc, og), osol = _oracle(name, mlp, mm, P)
    assert np.array_equal(gc, oc.astype(np.float32)) and bits_differ(g, og.astype(np.float32)) == 0, ("grad", name, mlp, mm, P)
    assert np.all(np.isfinite(g)) and np.any(g != 0)
    if sol is not None:
        for a, b, what in zip(sol, osol, ("uopt", "xevol", "info")):
            assert bits_differ(a, b) == 0, (what, name, mlp, mm, P)
        assert np.all(osol[2][:, 2] >= 1)
        assert kc.normalise(kname) == (TEAM[P].format(md=MODE[mlp]), mm), kname
    return (gc, g), sol


@pytest.mark.parametrize("mlp", ["f32x3", "f16"])
@pytest.mark.parametrize("P", [32, 33, 70, 130])
@pytest.mark.parametrize("name", FAST_CASES)
def test_fast_matrix_pipe_modes_off_the_synthetic_scale(name, P, mlp):
    _check(name, mlp, "fast", P)


@pytest.mark.parametrize("mlp", ["f32x3", "f16"])
@pytest.mark.parametrize("P", [33, 70])
@pytest.mark.parametrize("name", ["k-14", "k+16"])
def test_a_rescale_beyond_the_band_is_the_canonical_model_on_the_device(name, P, mlp):
    """metamorphic, on the device: the rescaled model's gradient and solve equal those of the canonical model bit for bit (and both equal the oracle's)"""
    (gc, g), sol = _check(name, mlp, "fast", P)
    (gc0, g0), sol0 = _check("canonical", mlp, "fast", P)
    assert np.array_equal(gc, gc0) and bits_differ(g, g0) == 0
    for a, b in zip(sol, sol0):
        assert bits_differ(a, b) == 0


@pytest.mark.parametrize("P", [33, 70])
@pytest.mark.parametrize("mlp,name", [("f32x3", "k-14"), ("f32x3", "k+16"), ("f32x3", "spread_force_low"), ("f32x3", "w2-12"), ("f32x3", "eoff_low"),
                                      ("f16", "k-14"), ("f16", "f16_subnormal"), ("f16", "f16_normal"), ("f16", "f16_saturating")])
def test_exact_matrix_pipe_modes_off_the_synthetic_scale(mlp, name, P):
    """math_mode exact: no normalisation and no refusal (W3 stays on the f32 chain); every branch of the fp16 rounding of the weights"""
    _check(name, mlp, "exact", P)


def test_closed_loop_against_a_rescaled_plant():
    """P = 33, T = 4, f32x3/fast: the plant is the controller's model with its output layer times 2^-14 (prepared like the handle's own model, normalisation
    included): the loop equals the reference loop, and the loop against the canonical plant, bit for bit"""
    cfg = SC.config(33, "f32x3", "fast", max_iter=4, max_no_improvement_iter=4)
    A = SC.base_model()
    x0, xref, _, u = CS.asymmetric_problem(cfg, B, 20, noise=False)
    xref, keys, T = xref[None], np.stack([prng.PRNGKey(20 + b) for b in range(B)]), 4
    S = SdeMpcSolver(cfg, A, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T, u_init=u, plant=SC.model_of("k-14"), plant_substeps=2)
    canon = S.closed_loop(x0, xref, keys, T, u_init=u, plant=SC.canonical(A), plant_substeps=2)
    S.solve_status()
    S.close()
    with oracle_threads():
        assert_same(got, plant_loop_ref(cfg, A, SC.model_of("k-14"), x0, xref, keys, T, substeps=2, u_init=u))
    for a, b in zip(got, canon):
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            assert bits_differ(a, b) == 0
    assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("name", ["eoff_low", "eoff_clamp", "w2-12", "f16_saturating"])
def test_a_refused_model_is_an_error_and_the_handle_stays_usable(name):
    """sdempc_create refuses the model in the fast matrix-pipe modes (SDEMPC_EINVAL = -1); as a plant of a live handle it is refused by the call, which leaves
    the handle as it was: the next gradient is the oracle's"""
    M = SC.model_of(name)
    for mlp in ("f32x3", "f16"):
        with pytest.raises(SdempcError, match=r"\(-1\).*model refused"):
            SdeMpcSolver(SC.config(33, mlp, "fast"), M, max_batch=B)
    cfg = SC.config(33, "f32x3", "fast", max_iter=4, max_no_improvement_iter=4)
    A = SC.base_model()
    x0, xref, _, u = CS.asymmetric_problem(cfg, B, 20, noise=False)
    keys = np.stack([prng.PRNGKey(20 + b) for b in range(B)])
    S = SdeMpcSolver(cfg, A, max_batch=B, options=SC.LAYOUTS[33])
    with pytest.raises(SdempcError, match=r"error -1: plant: model refused"):
        S.closed_loop(x0, xref[None], keys, 2, u_init=u, plant=M)
    px0, pu, pxref, pnoise = SC.problem(33, B)
    gc, g = S.grad(px0, pu, pxref, pnoise)
    S.close()
    (oc, og), _ = _oracle("base", "f32x3", "fast", 33)
    assert np.array_equal(gc, oc.astype(np.float32)) and bits_differ(g, og.astype(np.float32)) == 0
