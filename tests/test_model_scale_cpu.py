"""The matrix-pipe fast modes (SPEC.md §10e) on models OFF the synthetic weight scale, on the CPU (cases: tests/scale_cases.py).

* Metamorphic exactness — the test of the test. A function-preserving rescale (W3 row and b3 times 2^k, the residual scale times 2^-k) must leave f32/exact and
  f32/fast bit-identical to k = 0: rollout cost and tensor, gradient, and a six-iteration solve, in the C oracle and in the NumPy restatement.
* The referee at every scale: f32x3/exact and f32x3/fast no further from float64 than 1.5 x f32/exact on the same model and instance (the criterion of
  tests/test_arithmetic_referee_cpu.py); the f16 modes, lossy by design, no lossier than 1.5 x their own k = 0 error under function-preserving rescales.
  Before the normalisation of §10e the same table read 3.1 x at k = -6, 498 x at k = -14, 2.1 x at k = +12 and 4.6e4 x at k = +16 in f32x3/fast
  (profiles/model_scale_referee.txt).
* The normalisation leaves every model of the suite untouched (exponent 0 in every row), and is refused, not rounded, where it cannot be exact.
* What the modes refuse (a binary16 operand weight beyond 65504, eoff < 8, 0 < C2 < 2^-6: W2 times 2^-12 misses the referee's worst-entry bound at 1.59 x) is refused by sdempc_create with SDEMPC_EINVAL, by the C oracle and by the restatement.
* Wrong variants of the rule, through the NumPy restatement: each fails a named assertion."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cases as CS
import orc
import scale_cases as SC
from cases import bits_differ
from sde4mbrl_px4_amd import _abi, synthetic_hexa, synthetic_iris, synthetic_multirotor

sys.path.insert(0, os.path.join(CS.ROOT, "oracle"))
import sde_mpc_numpy as R2  # noqa: E402

P, B = 33, 2
F32_MODES = ("exact", "fast")
# k dropped from the metamorphic comparison, per output, with the reason (the issue allows two of the eleven uniform k per output): none is — at k = -20 .. 20
# the smallest scaled quantity (b3 2^-20, about 1e-7) and the largest (a residual scale times 2^20, about 5e5) are far inside float32's normal range
DROPPED = {"rollout": (), "grad": (), "solve": ()}


def _hw():
    return R2.HwTransc(orc.TRANSC_DIR)


def _c_outputs(model, mm, m=4):
    cfg = SC.config(P, "f32", mm, m=m)
    return SC.oracle_rollouts(cfg, model, B), SC.oracle_grads(cfg, model, B), SC.oracle_solves(cfg, model, B)


@pytest.mark.parametrize("mm", F32_MODES)
@pytest.mark.parametrize("m", [4, 6])
def test_metamorphic_exactness_in_the_c_oracle(m, mm):
    """every function-preserving rescale (eleven uniform k, the band ends, both spread cases; m = 6: uniform k = -14, 12): bit-identical to k = 0"""
    base = _c_outputs(SC.base_model(m), mm, m)
    assert np.all(base[2][2][:, 2] >= 5)                                # the solves ran their iterations
    names = list(SC.preserving_cases(m)) if m == 4 else ["k-14", "k+12"]
    for name in names:
        (c, t), (gc, g), (u, x, info) = _c_outputs(SC.model_of(name, m), mm, m)
        (c0, t0), (gc0, g0), (u0, x0, info0) = base
        k = SC.preserving_cases(m)[name][0]
        if k not in DROPPED["rollout"]:
            assert np.array_equal(c, c0) and bits_differ(t, t0) == 0, ("rollout", name)
        if k not in DROPPED["grad"]:
            assert np.array_equal(gc, gc0) and bits_differ(g.astype(np.float32), g0.astype(np.float32)) == 0 and np.array_equal(g, g0), ("grad", name)
        if k not in DROPPED["solve"]:
            assert bits_differ(u, u0) == 0 and bits_differ(x, x0) == 0 and bits_differ(info, info0) == 0, ("solve", name)


@pytest.mark.parametrize("mm", F32_MODES)
def test_metamorphic_exactness_in_the_numpy_restatement(mm):
    """the same in oracle/sde_mpc_numpy.py (instance 0; the largest and smallest uniform k, one inside, and both spread cases)"""
    cfg = SC.config(P, "f32", mm)
    x0, u, xref, noise = (a[0] for a in SC.problem(P, B))
    hw = _hw() if mm == "fast" else None

    def run(model):
        N = R2.Restatement(cfg, model, hw=hw)
        return N.rollout(x0, u, xref, noise), N.cost_grad(x0, u, xref, noise), N.solve_own(x0, xref, noise, u, cfg.ls_init_stepsize)
    (c0, t0, m0), (gc0, g0), (u0, i0) = run(SC.base_model())
    # and the restatement is the C oracle (so the comparison below is not between two copies of one mistake)
    (co, to), (_, go), (uo, _, io) = _c_outputs(SC.base_model(), mm)
    assert np.float32(co[0]) == c0 and bits_differ(t0, to[0]) == 0 and bits_differ(g0, go[0].astype(np.float32)) == 0 and bits_differ(u0, uo[0]) == 0 and bits_differ(i0, io[0]) == 0
    for name in ("k-20", "k-3", "k+20", "spread_torque_low", "spread_force_low"):
        (c, t, mn), (gc, g), (uu, ii) = run(SC.model_of(name))
        assert c == c0 and bits_differ(t, t0) == 0 and bits_differ(mn, m0) == 0, ("rollout", name)
        assert gc == gc0 and bits_differ(g, g0) == 0, ("grad", name)
        assert bits_differ(uu, u0) == 0 and bits_differ(ii, i0) == 0, ("solve", name)


# ---- the referee ------------------------------------------------------------------------------------------------------------------------------------------
REFEREED = list(SC.preserving_cases()) + ["w2-8", "w2+4", "w1z-8", "w1z+3", "w3n-8", "w3n+4", "eoff_mid"]


@pytest.mark.parametrize("name", REFEREED)
def test_referee_at_every_scale(name):
    """f32x3/exact and f32x3/fast: gradient rms and worst-entry error against float64 of the SAME model at most 1.5 x those of f32/exact (B = 2, P = 33)"""
    r = SC.referee(name)
    base = r["f32/exact"]
    print(name, {k: v for k, v in r.items() if k != "f64"})
    assert 1e-9 < base[0] < 1e-5, base                   # f32 gradients are f32-accurate, and not float64 by accident
    for a in ("f32x3/exact", "f32x3/fast"):
        assert r[a] is not None, (name, a, "refused")
        assert r[a][0] <= 1.5 * base[0] and r[a][1] <= 1.5 * base[1], (name, a, r[a], base)


def test_referee_with_six_motors():
    for name in ("k-14", "k+0", "k+12"):
        r = SC.referee(name, m=6)
        base = r["f32/exact"]
        assert 1e-9 < base[0] < 1e-5
        for a in ("f32x3/exact", "f32x3/fast"):
            assert r[a][0] <= 1.5 * base[0] and r[a][1] <= 1.5 * base[1], (name, a, r[a], base)
        for a in ("f16/exact", "f16/fast"):
            own = SC.referee("k+0", m=6)[a]
            assert r[a][0] <= 1.5 * own[0] and r[a][1] <= 1.5 * own[1], (name, a, r[a], own)


@pytest.mark.parametrize("name", list(SC.preserving_cases()))
def test_f16_modes_do_not_become_lossier_under_a_function_preserving_rescale(name):
    own = SC.referee("k+0")
    r = SC.referee(name)
    for a in ("f16/exact", "f16/fast"):
        assert r[a][0] <= 1.5 * own[a][0] and r[a][1] <= 1.5 * own[a][1], (name, a, r[a], own[a])


def test_every_rescale_beyond_the_band_is_the_canonical_model_bit_for_bit():
    """after the fix every function-preserving rescale that leaves the band gives ONE gradient in f32x3/fast and f16/fast: that of the model with every row at
    the target binade — so the k = 0 ratio of the table holds at every k"""
    for mlp in ("f32x3", "f16"):
        cfg = SC.config(P, mlp, "fast")
        c0, g0 = SC.oracle_grads(cfg, SC.canonical(SC.base_model()), B)
        for name in ("k-20", "k-14", "k-10", "k-6", "k+6", "k+12", "k+16", "k+20"):
            c, g = SC.oracle_grads(cfg, SC.model_of(name), B)
            assert np.array_equal(c, c0) and np.array_equal(g, g0), (mlp, name)


# ---- the rule itself ----------------------------------------------------------------------------------------------------------------------------------------
def _suite_models():
    """every model the existing tests, goldens and the referee fixture use (and their seeds' neighbours)"""
    out = [("golden " + n, v[1]) for n, v in CS.golden_cases().items()]
    for s in list(range(0, 24)) + [495]:
        out += [(f"iris {s}", synthetic_iris(s)), (f"hexa {s}", synthetic_hexa(s)), (f"asym4 {s}", CS.asymmetric_model(4, s)), (f"asym6 {s}", CS.asymmetric_model(6, s))]
        out += [(f"multirotor {m} {s}", synthetic_multirotor(m, s)) for m in (1, 3, 5, 8)]
    rng = np.random.default_rng(0)
    out += [(f"perturbed {i}", synthetic_iris().perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, moment=0.2, sigma=0.3, residual=0.3)) for i in range(8)]
    out.append(("diverging", CS.diverging_single_rotor_case()[1]))
    return out


def test_the_band_holds_every_model_of_the_suite():
    """exponent 0 in every row, eoff = 10, nothing refused: no committed golden or fixture changes by a bit. The band's margin: the rows of these models have
    their largest entry in [2^-3, 2^0] (g in -2 .. 0); the band is g in -3 .. 2, and on the parent the ratio stayed within 1.2 from g = -5 to g = 10."""
    gs = set()
    for name, M in _suite_models():
        assert not SC.row_exponents(M).any(), name
        gs.update(int(g) for g in SC.row_binades(M))
        for mlp in ("f32x3", "f16"):
            assert SC.eoff(M, mlp) == 10 and not SC.refused(M, mlp, "fast"), (name, mlp)
    assert gs <= {-2, -1, 0} and SC.BAND_LO < min(gs) and max(gs) < SC.BAND_HI, gs


def test_the_three_statements_of_the_rule_agree():
    """tests/scale_cases.py (what the tests expect), oracle/sde_mpc_numpy.py and — through bit-identical gradients of a tiny problem — the C oracle"""
    cfg = CS.asymmetric_cfg(4, horizon=3, num_short_dt=2, long_step_dt=0.1, num_particles=2, max_iter=2, max_no_improvement_iter=2, mlp_dtype="f32x3", math_mode="fast")
    x0, xref, noise, u = (a[1] for a in CS.asymmetric_problem(cfg, 2, 17))
    assert (SC.BAND_LO, SC.BAND_HI, SC.BAND_TO, SC.EOFF_MIN, SC.C2_MIN) == (R2.W3_BAND_LO, R2.W3_BAND_HI, R2.W3_BAND_TO, R2.ADJ_EOFF_MIN, R2.ADJ_C2_MIN)
    hw = _hw()
    for name in ("k-14", "k-3", "k-2", "k+2", "k+3", "k+16", "spread_force_low", "w2+4", "eoff_mid", "f16_subnormal", "f16_normal"):
        M = SC.model_of(name)
        for mlp in ("f32x3", "f16"):
            c = cfg.replace(mlp_dtype=mlp)
            N = R2.Restatement(c, M, hw=hw)
            assert np.array_equal(N.w3_exponents, SC.row_exponents(M)) and N.adj_eoff == SC.eoff(M, mlp), (name, mlp)
            if mlp == "f32x3" or name in ("k-14", "k+3"):
                co, go = orc.Oracle(c, M).grad(x0, u, xref, noise)
                cn, gn = N.cost_grad(x0, u, xref, noise)
                assert np.float32(co) == cn and bits_differ(gn, go.astype(np.float32)) == 0, (name, mlp)
    assert 5 <= SC.eoff(SC.model_of("eoff_mid")) <= 9 and 5 <= SC.eoff(SC.model_of("w2+4")) <= 9 and 5 <= SC.eoff(SC.model_of("k+3")) <= 9
    assert {SC.eoff(SC.model_of(n)) for n in ("eoff_mid", "w2+4", "k+3")} == {8, 9}
    assert SC.eoff(SC.model_of("eoff_clamp")) == -40 and SC.eoff(SC.model_of("eoff_low")) == SC.EOFF_MIN - 1


def test_f16_branch_models_reach_every_branch_and_boundary():
    cs = {b: SC.f16_branch_census(SC.f16_branch_model(b)) for b in SC.F16_BRANCHES}
    assert cs["subnormal"]["subnormal"] > 500 and cs["subnormal"]["on_lo"] == 2
    assert cs["normal"]["saturating"] == 0 and cs["normal"]["on_lo"] == 2 and cs["normal"]["normal"] > 1300
    assert cs["saturating"]["saturating"] >= 20 and cs["saturating"]["on_hi"] == 1
    # the oracle's rounding on the boundaries: 2^-14 and 65504 stay, the next float32 above 65504 saturates, 2^-24 stays, 2^-25 becomes 0
    L = orc.lib()
    L.orc_f16_rtz_value.restype, L.orc_f16_rtz_value.argtypes = C.c_double, [C.c_double]
    for x, want in ((2.0 ** -14, 2.0 ** -14), (65504.0, 65504.0), (float(np.nextafter(np.float32(65504), np.float32(np.inf))), 65504.0), (2.0 ** -24, 2.0 ** -24),
                    (2.0 ** -25, 0.0), (-1e9, -65504.0), (-(2.0 ** -14) * (1 - 2.0 ** -12), -(2.0 ** -14) * (1 - 2.0 ** -10))):
        assert L.orc_f16_rtz_value(x) == want, (x, want)


def test_tiny_cost_reaches_the_exponent_clamp_of_the_adjoint_scale():
    """every cost weight times 2^-110: the largest output adjoint of at least one particle and step is non-zero and below 2^-100 (§10e step 1: e <- max(e, -100)),
    the gradient stays finite and non-zero, and the restatement equals the C oracle bit for bit there"""
    cfg = SC.tiny_cost_cfg(CS.asymmetric_cfg(4, horizon=3, num_short_dt=2, long_step_dt=0.1, num_particles=2, mlp_dtype="f32x3", math_mode="fast"))
    x0, xref, noise, u = (a[1] for a in CS.asymmetric_problem(cfg, 2, 17))
    M = SC.base_model()
    N = R2.Restatement(cfg, M, hw=_hw())
    N.adj_mx_log = []
    cn, gn = N.cost_grad(x0, u, xref, noise)
    mx = np.array(N.adj_mx_log)
    assert np.any((mx > 0) & (mx < 2.0 ** -101)), mx
    co, go = orc.Oracle(cfg, M).grad(x0, u, xref, noise)
    assert np.float32(co) == cn and bits_differ(gn, go.astype(np.float32)) == 0
    assert np.all(np.isfinite(go)) and np.any(go != 0)
    # and at the device tests' shape the gradient is the float64 one to f32 accuracy, scaled by 2^-110 (nothing was flushed on the way)
    big = SC.tiny_cost_cfg(SC.config(P, "f32x3", "fast"))
    _, g = SC.oracle_grads(big, M, B)
    _, g64 = SC.oracle_grads(SC.config(P), M, B, double=True)
    rms, worst = SC.grad_error(np.ldexp(g, 110), g64)
    assert rms < 1e-5, (rms, worst)


# ---- what the modes refuse ------------------------------------------------------------------------------------------------------------------------------------
REFUSED = {"eoff_low": "eoff", "eoff_clamp": "eoff", "w2-12": "C2", "f16_saturating": "65504", "w2_huge": "65504", "inexact": "not exact"}


def _refused_model(name):
    if name == "w2_huge":
        return SC.scaled(SC.base_model(), W2=17)
    if name == "inexact":                       # residual scales so small that their compensation 2^-20 lands on float32's sub-normal grid: the rescale would round
        import dataclasses
        M = SC.rescaled(SC.base_model(), -20)
        return dataclasses.replace(M, res_force_scale=(M.res_force_scale * np.float32(2.0 ** -135)).astype(np.float32))
    return SC.model_of(name)


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_models_are_refused_through_the_c_abi_without_a_device(name):
    """sdempc_create: SDEMPC_EINVAL, a message that names the bound and the mode, in f32x3/fast and f16/fast only; the C oracle and the restatement refuse alike"""
    lib = _abi.load_library()
    M = _refused_model(name)
    blob = M.to_blob()
    buf = C.create_string_buffer(blob, len(blob))
    for mlp, mm in SC.ARITHS:
        cfg_py = SC.config(P, mlp, mm)
        cfg, keep = cfg_py.to_cfg()
        h = C.c_void_p()
        rc = lib.sdempc_create(C.byref(cfg), buf, len(blob), 2, C.byref(h))
        want = mm == "fast" and mlp != "f32"
        if name == "inexact":
            assert want == (mm == "fast" and mlp != "f32")
        else:
            assert SC.refused(M, mlp, mm) == want, (name, mlp, mm)
        if want:
            msg = lib.sdempc_last_error(None).decode()
            assert rc == -1 and not h.value, (name, mlp, mm, rc)          # SDEMPC_EINVAL
            assert "model refused" in msg and "math_mode fast" in msg and "f32x3 / f16" in msg and REFUSED[name] in msg, msg
            x0, u, xref, noise = (a[0] for a in SC.problem(P, B))
            with pytest.raises(AssertionError, match="-1"):
                orc.Oracle(cfg_py, M).grad(x0, u, xref, noise)
            with pytest.raises(ValueError, match="refused"):
                R2.Restatement(cfg_py, M, hw=_hw())
        else:
            assert rc == 0 and h.value, (name, mlp, mm, lib.sdempc_last_error(None))
            lib.sdempc_destroy(h)


def test_accepted_models_are_created():
    lib = _abi.load_library()
    for name in list(SC.preserving_cases()) + ["w2+4", "eoff_mid", "f16_subnormal", "f16_normal"]:
        blob = SC.model_of(name).to_blob()
        buf = C.create_string_buffer(blob, len(blob))
        for mlp in ("f32x3", "f16"):
            cfg, keep = SC.config(P, mlp, "fast").to_cfg()
            h = C.c_void_p()
            assert lib.sdempc_create(C.byref(cfg), buf, len(blob), 2, C.byref(h)) == 0, (name, mlp, lib.sdempc_last_error(None))
            lib.sdempc_destroy(h)


# ---- wrong variants of the rule, through the NumPy restatement -------------------------------------------------------------------------------------------------
def _named_assertions(wrong):
    """The assertions a statement of §10e's normalisation must pass, on a tiny problem (3 steps, 2 particles, f32x3/fast) -> the names of those that fail.
      beyond_band_is_canonical    a uniform rescale beyond the band gives the gradient of the canonical model, bit for bit
      spread_is_canonical         so does the spread case (force rows as given would keep the torque rows 2^-12 too small)
      cost_is_unchanged           the rollout cost of the rescaled model is that of the model (the function is preserved)
      eoff_as_stated              the scale offset is the one §10e states (tests/scale_cases.py: eoff), on a model at the clamp of 10 and on one below it
                                  (one less is an exact power of two away: the gradient keeps its bits until a limb leaves binary16's range)
      equals_the_c_oracle         cost and gradient equal the C oracle's bit for bit
      referee                     the gradient is within 1.5 x f32/exact's distance (rms) of the float64 gradient"""
    cfg = CS.asymmetric_cfg(4, horizon=3, num_short_dt=2, long_step_dt=0.1, num_particles=2, mlp_dtype="f32x3", math_mode="fast")
    x0, xref, noise, u = (a[1] for a in CS.asymmetric_problem(cfg, 2, 17))
    hw = _hw()
    base = SC.base_model()
    # (rows of the canonical model sit at the target binade; the spread case is cut from IT, so that its untouched force rows are inside the band)
    canon = SC.canonical(base)
    grad = lambda M, w: R2.Restatement(cfg, M, hw=hw, wrong=w).cost_grad(x0, u, xref, noise)
    c0, g0 = grad(canon, None)
    failed = []
    far, spread = SC.rescaled(canon, -14), SC.rescaled(canon, SC.SPREAD["spread_torque_low"])
    cf, gf = grad(far, wrong)
    cs, gs = grad(spread, wrong)
    if bits_differ(gf, g0):
        failed.append("beyond_band_is_canonical")
    if bits_differ(gs, g0):
        failed.append("spread_is_canonical")
    if cf != c0 or cs != c0:
        failed.append("cost_is_unchanged")
    if R2.Restatement(cfg, far, hw=hw, wrong=wrong).adj_eoff != SC.eoff(far) or R2.Restatement(cfg, SC.model_of("k+3"), hw=hw, wrong=wrong).adj_eoff != SC.eoff(SC.model_of("k+3")):
        failed.append("eoff_as_stated")
    co, go = orc.Oracle(cfg, far).grad(x0, u, xref, noise)
    if np.float32(co) != cf or bits_differ(gf, go.astype(np.float32)):
        failed.append("equals_the_c_oracle")
    f64 = orc.Oracle(cfg.replace(mlp_dtype="f32", math_mode="exact"), far, double=True).grad(x0, u, xref, noise)[1]
    f32 = orc.Oracle(cfg.replace(mlp_dtype="f32", math_mode="exact"), far).grad(x0, u, xref, noise)[1]
    rel = lambda g: float(np.sqrt(np.mean(((np.asarray(g, np.float64) - f64) / np.abs(f64).max()) ** 2)))
    if not rel(gf) <= 1.5 * rel(f32):
        failed.append("referee")
    return failed


def test_the_rule_as_stated_passes_every_named_assertion():
    assert _named_assertions(None) == []


@pytest.mark.parametrize("wrong,must_fail", [("no_normalisation", ("beyond_band_is_canonical", "referee")), ("b3_not_scaled", ("cost_is_unchanged",)),
                                             ("no_compensation", ("cost_is_unchanged",)), ("common_exponent_from_force_rows", ("spread_is_canonical",)),
                                             ("eoff_off_by_one", ("eoff_as_stated",))])
def test_wrong_variants_of_the_rule_fail_a_named_assertion(wrong, must_fail):
    failed = _named_assertions(wrong)
    assert set(must_fail) <= set(failed), (wrong, failed)
