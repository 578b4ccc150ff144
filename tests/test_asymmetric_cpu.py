"""The asymmetric fixtures of tests/cases.py on the CPU: they have the properties they promise, every entry of the model and of the per-motor
settings is LIVE in the oracle's results at the shapes tests/test_gpu_asymmetric.py runs (so a kernel that drops, swaps or mis-indexes one of
them cannot equal the oracle bit for bit), and every mutant of that file's mutant test changes the oracle's own gradient and solve."""
import dataclasses
import itertools
import os

import numpy as np
import pytest

import orc
from cases import asymmetric_cfg, asymmetric_model, asymmetric_mutants, asymmetric_problem, bits_differ
from sde4mbrl_px4_amd import synthetic_iris

B = 3


def _distinct(*arrays):
    v = np.concatenate([np.abs(np.asarray(a, np.float64)).ravel() for a in arrays])
    return all(abs(a - b) > 1e-3 * max(a, b) for a, b in itertools.combinations(v, 2))


@pytest.mark.parametrize("m", [3, 4, 6, 8])
def test_fixtures_break_every_symmetry(m):
    A, A2 = asymmetric_model(m), asymmetric_model(m, seed=11)
    assert A.mass != synthetic_iris().mass and A.grav != 9.81
    assert _distinct(A.inertia) and _distinct(A.res_force_scale, A.res_torque_scale) and _distinct(A.sigma) and _distinct(A.b3) and _distinct(A.rotor_dir)
    assert np.all(A.thrust_poly > 0) and A.thrust_poly[2] < 0.1 * A.mass * A.grav / m and _distinct(A.moment_poly)
    assert np.all(np.abs(np.abs(A.rotor_dir) - 1) > 0.01) and np.all(np.abs(A.b3) > 0.1) and np.all(np.abs(A.b3) < 0.5) and A.b3n > 0.3
    assert _distinct(A.rotor_x) and _distinct(A.rotor_y)                       # no rotor is the mirror image of another
    assert A2.thrust_poly[2] != A.thrust_poly[2] and A2.inertia[0] != A2.inertia[1] and bits_differ(A.b3, A2.b3) == 6
    c = asymmetric_cfg(m)
    lo, hi = np.asarray(c.input_bound).T
    slo, shi = np.asarray(c.u_slew_constr).T
    assert all(_distinct(v) for v in (c.uref, lo, hi, slo, shi)) and np.all(lo < np.asarray(c.uref)) and np.all(np.asarray(c.uref) < hi)
    assert _distinct(c.perr, c.verr, c.qerr, c.werr) and c.discount < 1 and c.res_mult > 0 and c.u_slew_coeff > 0 and c.u_slew_constr_coeff > 0
    cfg = asymmetric_cfg(m, horizon=7, num_short_dt=4, long_step_dt=0.1, num_particles=5)
    x0, xref, noise, u = asymmetric_problem(cfg, B, 21)
    assert np.all(x0[1, 6] < 0) and x0[0, 6] > 0 and abs(2 * np.degrees(np.arccos(x0[B - 1, 6])) - 150) < 1e-3
    assert np.all((u > hi).any(axis=1)) and np.all((u < lo).any(axis=1))       # every motor of every instance, both sides
    ds = np.diff(u, axis=1)
    assert np.all((ds > shi).any(axis=1)) and np.all((ds < slo).any(axis=1))
    O = orc.Oracle(cfg, A)
    for b in range(B):
        assert np.isfinite(O.rollout(x0[b], u[b], xref[b], noise[b], True)[1]).all()


def _results(cfg, model, prob, with_solve):
    """The oracle's cost and gradient at the warm start of every instance (and, with_solve, uopt and the telemetry of the solve from it)."""
    x0, xref, noise, u = prob
    O = orc.Oracle(cfg, model)
    out = []
    for b in range(x0.shape[0]):
        c, g = O.grad(x0[b], u[b], xref[b], noise[b])
        out += [np.float32(c).reshape(1), g.astype(np.float32).ravel()]
        if with_solve:
            uo, _, info, _ = O.solve(x0[b], xref[b], noise[b], u[b], 0.01)
            out += [uo.ravel(), info]
    return np.concatenate(out)


def _bump(v):
    v = np.float32(v)
    return np.float32(v * np.float32(1.001)) if v != 0 else np.float32(1e-3)


def _entries(a):
    """Every entry of a field with up to 8 entries; first, last and one interior entry of a weight array."""
    a = np.asarray(a)
    if a.size <= 8:
        return list(np.ndindex(a.shape))
    return [tuple(np.unravel_index(i, a.shape)) for i in (0, (a.size // 2) + (a.shape[-1] // 3), a.size - 1)]


@pytest.mark.parametrize("m,P", [(4, 1), (4, 33), (6, 45), (3, 45)])
def test_every_entry_is_live_in_the_oracle(m, P):
    """Changing ANY one entry (by 0.1 %) changes bits of the oracle's (cost, gradient) over the B = 3 instances of the GPU tests' smallest shapes
    (H = 9 with both step lengths; P = 1 is the smallest). No entry is exempt. input_bound is the one setting the gradient does not read
    (SPEC.md §5: a rollout takes its controls as given; the bounds are the projection of the solve, §8), so its entries — and, for good
    measure, uref's and u_slew_constr's again — must change (uopt, telemetry) of the solve from the warm start instead."""
    cfg = asymmetric_cfg(m, horizon=9, num_short_dt=4, long_step_dt=0.1, num_particles=P)
    A = asymmetric_model(m)
    prob = asymmetric_problem(cfg, B, 21)
    base, base_s = _results(cfg, A, prob, False), _results(cfg, A, prob, True)
    dead = []
    for name in ("mass", "grav", "b3n"):
        if bits_differ(_results(cfg, dataclasses.replace(A, **{name: float(_bump(getattr(A, name)))}), prob, False), base) == 0:
            dead.append(name)
    for name in A._ARRAY_FIELDS:
        for idx in _entries(getattr(A, name)):
            a = np.array(getattr(A, name), np.float32, copy=True)
            a[idx] = _bump(a[idx])
            if bits_differ(_results(cfg, dataclasses.replace(A, **{name: a}), prob, False), base) == 0:
                dead.append((name, idx))
    for name in ("uref", "input_bound", "u_slew_constr"):
        for idx in np.ndindex(np.asarray(getattr(cfg, name)).shape):
            a = np.array(getattr(cfg, name), np.float64)
            a[idx] = float(_bump(a[idx]))
            c2 = cfg.replace(**{name: a.tolist()})
            if name != "input_bound" and bits_differ(_results(c2, A, prob, False), base) == 0:
                dead.append((name, idx, "grad"))
            if bits_differ(_results(c2, A, prob, True), base_s) == 0:
                dead.append((name, idx, "solve"))
    assert not dead, dead


@pytest.mark.parametrize("mlp,math,P", [("f32", "exact", 33), ("f32x3", "fast", 40)])
def test_every_mutant_changes_the_oracles_results(mlp, math, P):
    """The two settings of the GPU mutant test, oracle against oracle: each mutant changes bits of the gradient and of uopt. Two statements of
    the reference itself: the gradient does not read input_bound (that mutant shows in the solve only), and the negated initial quaternion is
    no mutant at all — q and -q give the same cost, gradient, uopt and telemetry bit for bit (every term is even or odd in q and negation is
    exact), which is why the GPU file runs -q as a parity case and not as a mutant."""
    cfg = asymmetric_cfg(4, horizon=9, num_short_dt=4, long_step_dt=0.1, num_particles=P, mlp_dtype=mlp, math_mode=math)
    A = asymmetric_model(4)
    x0, xref, noise, u = prob = asymmetric_problem(cfg, B, 21)
    n_g = 1 + 9 * 4                                                             # per instance: cost and gradient first, then uopt and telemetry
    split = lambda r: (r.reshape(B, -1)[:, :n_g], r.reshape(B, -1)[:, n_g:])
    g0, s0 = split(_results(cfg, A, prob, True))
    # the symmetric vehicle with a uniform configuration, same shapes and warm starts: every mutant is the identity there
    sym = synthetic_iris()
    ucfg = cfg.replace(uref=[0.71] * 4, input_bound=[[0.05, 0.93]] * 4, u_slew_constr=[[-0.02, 0.03]] * 4)
    orc.set_threads(min(os.cpu_count() or 1, 8))                               # (the oracle's particle loops on several cores: same bits)
    try:
        r_sym = _results(ucfg, sym, prob, True) if mlp == "f32" else None
        for name, f in asymmetric_mutants().items():
            g1, s1 = split(_results(*f(A, cfg)[::-1], prob, True))
            assert bits_differ(s1, s0) > 0, name
            assert (bits_differ(g1, g0) > 0) == (name != "input_bound_rotated"), name
            if r_sym is not None:
                assert bits_differ(_results(*f(sym, ucfg)[::-1], prob, True), r_sym) == 0, name
        xq = x0.copy(); xq[:, 6:10] = -xq[:, 6:10]
        assert bits_differ(_results(cfg, A, (xq, xref, noise, u), True), _results(cfg, A, prob, True)) == 0
    finally:
        orc.set_threads(1)
