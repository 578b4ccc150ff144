"""The cases of the model-scale tests (SPEC.md §10e, §10d), shared by tests/test_model_scale_cpu.py and tests/test_gpu_model_scale.py.

Every vehicle of the suite draws its MLP weights as N(0, 1) / sqrt(n_in): one weight scale. The models here leave it.

Function-preserving rescales (`rescaled`): row i of W3 and b3[i] times 2^k_i, the matching residual scale (res_force_scale for rows 0..2, res_torque_scale for
rows 3..5) times 2^-k_i. SPEC.md §5.2 uses a drift output o_i only in the products sF_i o_i / sT_i o_i, and §5.4 forms the output adjoints as products with the
same scales, so in float32 the rescaled model computes the same bits as long as nothing under- or overflows. "uniform k": every row by the same k of UNIFORM_K;
"spread": the force rows at 0 and the torque rows at -12, and the mirror image.

The density net has NO exactly compensating parameter: its output passes through a sigmoid (§5.2: eta = sigmoid(w3n . h1n + b3n)), and what multiplies eta
afterwards (sigma_i sqrt(dt), res_mult) cannot undo a scale inside the sigmoid. w3n is therefore covered among the scalings that change the function.

Scalings that DO change the function are judged against the float64 evaluation of the same model: W2 and b2 times 2^{-12, -8, 4}, W1z times 2^{-8, 3}, w3n times
2^{-8, 4}, one model whose scale offset `eoff` of §10e lies in 5..9 and one at its clamp of -40 (`eoff` restates §10e in NumPy: the tests assert the ranges).

`f16_branch_model`: W1z / W2 entries in each branch of the host's round-toward-zero to binary16 (§9): below 2^-14 (the sub-normal grid), inside the normal range,
beyond 65504 (saturation), and one entry exactly on each boundary.

`tiny_cost_cfg`: every cost weight times 2^-110, so that the output adjoints of a particle fall below 2^-100: the `e <- max(e, -100)` clamp of §10e step 1.

Shapes: H = 8, num_short_dt = 8; B = 3 on the device, B = 2 in the referee tests; m = 4, and one m = 6 case of uniform k.

Everything a test compares against is computed ONCE per case from the CPU oracle and cached for the process."""
import dataclasses
import functools

import numpy as np

import cases as CS
import orc

F = np.float32
H = 8
UNIFORM_K = (-20, -14, -10, -6, -3, 0, 3, 6, 12, 16, 20)
BAND_ENDS = (-2, 2)          # the uniform k at which every row of asymmetric_model(4) is still inside the no-normalisation band (its rows: g = -1, one g = 0)
SPREAD = {"spread_torque_low": (0, 0, 0, -12, -12, -12), "spread_force_low": (-12, -12, -12, 0, 0, 0)}
ARITHS = (("f32", "exact"), ("f32x3", "exact"), ("f32", "fast"), ("f32x3", "fast"), ("f16", "exact"), ("f16", "fast"))
LAYOUTS = {32: {"coop": 0}, 33: {"coop": 0, "duo": 0}, 70: {"coop": 0, "duo": 1}, 130: {"coop": 0}}          # tests/KERNELS.md: TeamWave, TeamBlock, TeamPairT<2>, TeamBlock mode 3

# SPEC.md §10e: a row of W3 is left as given when the binary exponent (frexp) of its largest entry is in BAND_LO .. BAND_HI (the entry in [2^-4, 2^2)), else it is
# brought to BAND_TO (the entry in [2^-2, 2^-1)); the matrix-pipe fast modes refuse a scale offset below EOFF_MIN and a non-zero C2 below C2_MIN. Restated here on purpose: the tests compare
# these numbers with what the library and both oracles do.
BAND_LO, BAND_HI, BAND_TO, EOFF_MIN, C2_MIN = -3, 2, -1, 8, 2.0 ** -6


def pow2(k):
    return np.ldexp(F(1), np.asarray(k, np.int32)).astype(F)


def rescaled(model, k_rows):
    """the same function with row i of the output layer times 2^k_rows[i] (an int, or six of them)"""
    k = np.broadcast_to(np.asarray(k_rows, np.int32), (6,))
    up, dn = pow2(k), pow2(-k)
    return dataclasses.replace(model, W3=(model.W3 * up[:, None]).astype(F), b3=(model.b3 * up).astype(F),
                               res_force_scale=(model.res_force_scale * dn[:3]).astype(F), res_torque_scale=(model.res_torque_scale * dn[3:]).astype(F))


def scaled(model, **exps):
    """the model with the named arrays times 2^e: scaled(M, W2=4, b2=4) — NOT the same function"""
    return dataclasses.replace(model, **{n: (F(getattr(model, n)) * pow2(e)).astype(F) if n != "b3n" else float(F(model.b3n) * pow2(e)) for n, e in exps.items()})


def base_model(m=4):
    return CS.asymmetric_model(m)


def preserving_cases(m=4):
    """name -> k_rows of every function-preserving rescale"""
    d = {f"k{k:+d}": (k,) * 6 for k in UNIFORM_K}
    if m == 4:
        d.update({f"k{k:+d}": (k,) * 6 for k in BAND_ENDS})
        d.update(SPREAD)
    return d


def changing_cases():
    """name -> model of every scaling that changes the function (m = 4)"""
    M = base_model()
    d = {f"w2{e:+d}": scaled(M, W2=e, b2=e) for e in (-12, -8, 4)}
    d.update({f"w1z{e:+d}": scaled(M, W1z=e) for e in (-8, 3)})
    d.update({f"w3n{e:+d}": scaled(M, w3n=e) for e in (-8, 4)})
    d["eoff_mid"] = scaled(M, W2=3)            # eoff = 9 (W2 alone, b2 as given). W2 alone times 2^4 (eoff = 8) is not a referee case of the matrix pipe: there f32/fast
                                               # and f32x3/fast share one worst entry at 1.60 x f32/exact's — the hardware tanh at saturated units, not the limbs
    d["eoff_low"] = scaled(M, W2=5)            # eoff = 7: below EOFF_MIN, refused by the matrix-pipe fast modes (on the parent: worst entry 1.56 x f32/exact's)
    d["eoff_clamp"] = scaled(M, w3n=60)        # eoff = -40: refused likewise
    return d


def row_exponents(model):
    """SPEC.md §10e, "normalisation of the output layer": per row i, g_i = the binary exponent of max_k |W3[i][k]| as frexp returns it; the row is left alone
    (n_i = 0) when BAND_LO <= g_i <= BAND_HI or the row is zero or not finite, otherwise n_i = BAND_TO - g_i. -> int[6]"""
    n = np.zeros(6, np.int32)
    for i in range(6):
        mx = F(np.abs(F(model.W3[i])).max())
        if mx > 0 and np.isfinite(mx):
            g = int(np.frexp(mx)[1])
            if not (BAND_LO <= g <= BAND_HI):
                n[i] = BAND_TO - g
    return n


def row_binades(model):
    """the binary exponents g_i of the rows' largest entries"""
    return np.array([int(np.frexp(F(np.abs(F(model.W3[i])).max()))[1]) for i in range(6)], np.int32)


def canonical(model):
    """the same function with EVERY row of W3 brought to BAND_TO: the fixed point of the normalisation, the model every rescale beyond the band is mapped to"""
    return rescaled(model, BAND_TO - row_binades(model))


def normalised(model):
    """what sdempc_create makes of the model in math_mode fast with mlp_dtype f32x3 / f16 (§10e)"""
    return rescaled(model, row_exponents(model))


def eoff(model, mlp_dtype="f32x3", normalise=True, with_c2=False):
    """SPEC.md §10e's scale offset of the model, restated in NumPy float32 (f16: on that mode's weights, §10b); with_c2: -> (eoff, C2)"""
    M = normalised(model) if normalise else model
    c = F(2.885390043258667)
    W2 = F(M.W2)
    if mlp_dtype == "f16":
        q = _rtz()
        W2f = (F(-2) * q((c * q(W2)).astype(F))).astype(F)
        V2 = ((F(-2) * W2f).astype(F) / c).astype(F)
    else:
        V2 = (F(4) * W2).astype(F)
    W3f, w3nf = (F(-2) * F(M.W3)).astype(F), (F(-2) * F(M.w3n)).astype(F)
    B3 = Bn = C2 = F(0)
    for k in range(32):
        s3, s2 = F(0), F(0)
        for i in range(6):
            s3 = F(s3 + abs(W3f[i, k]))
        for j in range(32):
            s2 = F(s2 + abs(V2[j, k]))
        B3, C2, Bn = max(B3, s3), max(C2, s2), max(Bn, F(abs(w3nf[k])))
    with np.errstate(over="ignore"):
        bound = max(F(B3 * F(0.25)), F(Bn * F(0.25)), F(F(C2 * F(B3 * F(0.25))) * F(0.25)))
    e = 10
    if bound > 0 and np.isfinite(bound):
        e = min(10, 14 - int(np.frexp(bound)[1]))
    return (max(e, -40), float(C2)) if with_c2 else max(e, -40)


# ---- mlp_dtype f16: every branch of the host's round-toward-zero to binary16 ------------------------------------------------------------------------------
def f16_branch_model(branch):
    """branch "subnormal": every other entry (at random) of W1z times 2^-13 and of W2 times 2^-12 (|w| below 2^-14: the 2^-24 grid); "normal": the model as it is, with one W1z and one W2 entry
    exactly 2^-14 and two larger ones (6, 40); "saturating": sixteen W2 entries and eight W1z entries beyond 65504 (up to 2^20), one exactly 65504 and one the next
    float32 above it. The boundaries sit on entries whose sign is kept. The saturating model is accepted by math_mode exact only: in fast mode -2 (c w) has no
    binary16 value and the model is refused (SPEC.md §10e, "What the mode accepts")."""
    M = base_model()
    W1z, W2 = F(M.W1z).copy(), F(M.W2).copy()
    sg = lambda a: np.where(a < 0, F(-1), F(1))
    if branch == "subnormal":
        rng = np.random.default_rng(78)
        W1z = np.where(rng.random(W1z.shape) < 0.5, W1z * pow2(-13), W1z).astype(F)
        W2 = np.where(rng.random(W2.shape) < 0.5, W2 * pow2(-12), W2).astype(F)
        W1z[3, 2] = sg(W1z[3, 2]) * pow2(-14)
        W2[5, 7] = sg(W2[5, 7]) * pow2(-14)
        W2[6, 9] = sg(W2[6, 9]) * pow2(-24)                  # the smallest sub-normal, and below it: rounds to zero
        W2[7, 11] = sg(W2[7, 11]) * pow2(-25)
    elif branch == "normal":
        W1z[3, 2] = sg(W1z[3, 2]) * pow2(-14)
        W2[5, 7] = sg(W2[5, 7]) * pow2(-14)
        W2[9, 1] = sg(W2[9, 1]) * F(6.0)
        W1z[40, 4] = sg(W1z[40, 4]) * F(40.0)
    else:
        assert branch == "saturating"
        rng = np.random.default_rng(77)
        for n in range(16):
            j, k = int(rng.integers(32)), int(rng.integers(32))
            W2[j, k] = sg(W2[j, k]) * F(65504.0) * F(1.0 + 30.0 * rng.random())
        for n in range(8):
            r, k = int(rng.integers(64)), int(rng.integers(6))
            W1z[r, k] = sg(W1z[r, k]) * F(70000.0) * F(1.0 + 10.0 * rng.random())
        W2[9, 1] = sg(W2[9, 1]) * F(65504.0)
        W2[10, 2] = sg(W2[10, 2]) * np.nextafter(F(65504.0), F(np.inf))
    return dataclasses.replace(M, W1z=W1z, W2=W2)


F16_BRANCHES = ("subnormal", "normal", "saturating")


def f16_branch_census(model):
    """how many |W1z|, |W2| entries lie in each branch of f16_rtz_host, and on each boundary"""
    a = np.abs(np.concatenate([F(model.W1z).ravel(), F(model.W2).ravel()]))
    return dict(subnormal=int(((a < pow2(-14)) & (a > 0)).sum()), normal=int(((a >= pow2(-14)) & (a <= F(65504.0))).sum()), saturating=int((a > F(65504.0)).sum()),
                on_lo=int((a == pow2(-14)).sum()), on_hi=int((a == F(65504.0)).sum()))


# ---- configurations and problems ---------------------------------------------------------------------------------------------------------------------------
def config(P, mlp_dtype="f32", math_mode="exact", m=4, **kw):
    return CS.asymmetric_cfg(m, horizon=H, num_short_dt=H, num_particles=P, mlp_dtype=mlp_dtype, math_mode=math_mode, **kw)


COST_KEYS = ("perr", "verr", "qerr", "werr", "uerr", "u_slew_coeff", "u_slew_constr_coeff", "res_mult")


def tiny_cost_cfg(cfg, e=-110):
    """every cost weight of the configuration times 2^e"""
    s = float(np.ldexp(1.0, e))
    kw = {}
    for k in COST_KEYS:
        v = getattr(cfg, k)
        kw[k] = [float(x) * s for x in v] if isinstance(v, (list, tuple, np.ndarray)) else float(v) * s
    return cfg.replace(**kw)


@functools.lru_cache(maxsize=None)
def problem(P, B, m=4):
    """(x0, u, xref, noise) of B instances — asymmetric_problem(cfg, B, seed=3), the instance the issue's table was measured on"""
    x0, xref, noise, u = CS.asymmetric_problem(config(P, m=m), B, seed=3)
    for a in (x0, xref, noise, u):
        a.setflags(write=False)
    return x0, u, xref, noise


def refused(model, mlp_dtype, math_mode):
    """SPEC.md §10e, "What the mode accepts", restated: math_mode fast with mlp_dtype f32x3 / f16 refuses a model with a binary16 operand weight beyond 65504
    (the forward -2 c W2, f16: -2 f16_rtz(c f16_rtz(W2)); the adjoint's 4 W2, W1z, W1u, -2 W3) or with eoff < EOFF_MIN, or with a non-zero C2 (the largest absolute column sum of the adjoint's 4 W2) below C2_MIN"""
    if math_mode != "fast" or mlp_dtype == "f32":
        return False
    M = normalised(model)
    c = F(2.885390043258667)
    with np.errstate(over="ignore"):
        if mlp_dtype == "f16":
            q = _rtz()
            w2f = (F(-2) * q((c * q(F(M.W2))).astype(F))).astype(F)
            ims = [w2f, ((F(-2) * w2f).astype(F) / c).astype(F), (q((c * q(F(M.W1z))).astype(F)) / c).astype(F)]
        else:
            ims = [(F(-2) * (c * F(M.W2)).astype(F)).astype(F), (F(4) * F(M.W2)).astype(F), F(M.W1z)]
        ims += [F(M.W1u), (F(-2) * F(M.W3)).astype(F)]
    e, C2 = eoff(model, mlp_dtype, with_c2=True)
    return max(float(np.abs(a).max()) for a in ims) > 65504.0 or e < EOFF_MIN or 0 < C2 < C2_MIN


def _rtz():
    L = orc.lib()
    L.orc_f16_rtz_value.restype = orc.C.c_double
    L.orc_f16_rtz_value.argtypes = [orc.C.c_double]
    return np.vectorize(lambda w: F(L.orc_f16_rtz_value(float(w))), otypes=[F])


def oracle_grads(cfg, model, B, double=False):
    """-> (cost f64[B], grad f64[B][H][m]) of the oracle on problem(P, B)"""
    x0, u, xref, noise = problem(cfg.num_particles, B, cfg.num_motors)
    if double:
        cfg = cfg.replace(mlp_dtype="f32", math_mode="exact")
    if not double and refused(model, cfg.mlp_dtype, cfg.math_mode):
        return None, None
    O = orc.Oracle(cfg, model, double=double)
    r = [O.grad(x0[b], u[b], xref[b], noise[b]) for b in range(B)]
    return np.array([c for c, _ in r]), np.stack([g for _, g in r])


def oracle_solves(cfg, model, B):
    """-> (uopt f32[B][H][m], xevol f32[B][H+1][13], info f32[B][8]) of the oracle's solve from problem(P, B), initial step cfg.ls_init_stepsize"""
    x0, u, xref, noise = problem(cfg.num_particles, B, cfg.num_motors)
    O = orc.Oracle(cfg, model)
    r = [O.solve(x0[b], xref[b], noise[b], u[b], cfg.ls_init_stepsize)[:3] for b in range(B)]
    return tuple(np.stack([x[i] for x in r]) for i in range(3))


def oracle_rollouts(cfg, model, B):
    """-> (cost f64[B], traj f32[B][P][H+1][13])"""
    x0, u, xref, noise = problem(cfg.num_particles, B, cfg.num_motors)
    O = orc.Oracle(cfg, model)
    r = [O.rollout(x0[b], u[b], xref[b], noise[b], want_traj=True)[:2] for b in range(B)]
    return np.array([c for c, _ in r]), np.stack([t for _, t in r])


def grad_error(g, g64):
    """(rms, worst entry) of the gradient error over the float64 gradient's largest entry, over every instance (benchlib/referee.py's figures)"""
    from benchlib import referee as R
    rows = [R.gradient_error(g[b], g64[b]) for b in range(len(g))]
    rms = np.array([r["rms_rel"] for r in rows])
    return float(np.sqrt(np.mean(rms * rms))), float(max(r["max_rel"] for r in rows))


_MODELS = {}


def model_of(name, m=4):
    """the model of a case name: a key of preserving_cases(), of changing_cases(), "f16_<branch>" or "base" """
    key = (name, m)
    if key not in _MODELS:
        if name == "base":
            M = base_model(m)
        elif name in preserving_cases(m):
            M = rescaled(base_model(m), preserving_cases(m)[name])
        elif name.startswith("f16_"):
            M = f16_branch_model(name[4:])
        else:
            M = changing_cases()[name]
        _MODELS[key] = M
    return _MODELS[key]


@functools.lru_cache(maxsize=None)
def referee(name, P=33, B=2, m=4):
    """-> {arithmetic "mlp/mm": (rms, worst), or None where the mode refuses the model} of the case's gradients against float64 of the SAME model, and "f64": the float64 gradients. Read-only."""
    M = model_of(name, m)
    _, g64 = oracle_grads(config(P, m=m), M, B, double=True)
    out = {"f64": g64}
    for mlp, mm in ARITHS:
        with np.errstate(all="ignore"):
            g = oracle_grads(config(P, mlp, mm, m=m), M, B)[1]
            out[f"{mlp}/{mm}"] = None if g is None else grad_error(g, g64)          # None: the mode refuses the model
    g64.setflags(write=False)
    return out
