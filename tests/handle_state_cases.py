"""Inputs and oracle results shared by tests/test_gpu_handle_state.py (the kernels on a handle with a past) and tests/test_handle_state_cpu.py
(the conditions those tests rest on, shown with the oracle alone): the scripted life of one handle, the poison instances, the guarded-buffer
cases and the sentinel. Test infrastructure, like cases.py."""
import functools
import os

import numpy as np

import orc
from cases import CDIR
from closed_loop_ref import closed_loop_ref
from sde4mbrl_px4_amd import load_mpc_config, prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W

H = 10
ARITH = [("f32", "exact"), ("f32", "fast"), ("f32x3", "fast"), ("f16", "exact")]
SENTINEL = 0x5EA7D00D          # what guards and payloads of the caller-owned buffers are prefilled with: a finite float32 (6.04e18) no result equals
GUARD = 4096                   # words in front of and behind every payload


def cfg_for(P, mlp="f32", math="exact", **kw):
    """Iris, H = 10 with both step lengths, at most 8 iterations."""
    c1 = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml"))
    return c1.replace(**{"horizon": H, "num_short_dt": 6, "long_step_dt": 0.1, "num_particles": P, "max_iter": 5, "max_no_improvement_iter": 5,
                         "mlp_dtype": mlp, "math_mode": math, **kw})


def oracle_threads(n=None):
    orc.set_threads(min(os.cpu_count() or 1, 8) if n is None else n)


def problem(cfg, B, seed):
    """(x0, xref, noise, u, stepsize): every instance with its own state, reference window, noise, warm start and step size."""
    P, m = cfg.num_particles, cfg.num_motors
    x0 = W.random_initial_states(B, seed)
    xref = np.stack([W.reference_window(0.11 * b + 0.01 * seed, cfg.time_steps) for b in range(B)]).astype(np.float32)
    noise = W.make_noise(B, P, H, seed)
    u = np.clip(np.asarray(cfg.uref, np.float32) + 0.1 * np.random.default_rng(seed + 5).standard_normal((B, H, m)), 1e-4, 1).astype(np.float32)
    s = (0.01 * (1 + np.arange(B) % 3)).astype(np.float32)
    return x0, xref, noise, u, s


def poison_problem(cfg, B, seed):
    """Instances whose states overflow float32 within the horizon: finite body rates of 1e30 rad/s and velocities of 1e35 m/s, different in
    every instance (the quaternion update squares the rate: inf, then NaN)."""
    x0, xref, noise, u, s = problem(cfg, B, seed)
    scale = (1.0 + np.arange(B, dtype=np.float32))[:, None]
    x0[:, 10:13] = np.float32(1e30) * scale * np.array([1.0, -2.0, 0.5], np.float32)
    x0[:, 3:6] = np.float32(1e35) * scale * np.array([-1.0, 0.5, 2.0], np.float32)
    assert np.isfinite(x0).all()
    return x0, xref, noise, u, s


# ---- A. the scripted life of one handle (max_batch = 48, P = 70: three particle groups, the last one ragged, a duo pair without a group B) ----
LIFE_P, LIFE_MAX_BATCH = 70, 48
SPEC, COOP = "sdempc_solve_spec_kernel<4, false>", "sdempc_solve_kernel<TeamBlock, 4, 0, {pk}, 2, false>"
# (kind, B, options set on the live handle before the call, seed, normalised last_kernel_name() in the f32 modes (tests/kernel_census.py: normalise;
# {pk}: true while B x coop_nwg(P) workgroups leave one per CU, launch_coop_m))
LIFE = [
    ("solve", 1, {}, 101, SPEC),
    ("solve", 3, {"spec": 0}, 102, COOP),                   # plain cooperative
    ("poison", 40, {"coop": 0, "duo": 1}, 103, "sdempc_solve_kernel<TeamPairT<2>, 4, 0, false, 3, false>"),  # the first B = 40: the workspaces grow here
    ("poison", 2, {"coop": 1}, 104, COOP),
    ("solve", 2, {"spec": 1}, 105, SPEC),
    ("solve", 3, {"spec": 0}, 106, COOP),
    ("rollout", 5, {}, 107, None),
    ("grad", 7, {}, 108, None),
    ("solve", 40, {"coop": 0, "duo": 1}, 109, "sdempc_solve_kernel<TeamPairT<2>, 4, 0, false, 3, false>"),   # rows the poison call left NaN in
    ("solve", 40, {"duo": 0}, 110, "sdempc_solve_kernel<TeamBlock, 4, 0, false, 0, false>"),
    ("solve", 4, {"ustg": 1}, 111, "sdempc_solve_kernel<TeamBlock, 4, 0, false, 0, true>"),
    ("solve", 2, {"ustg": -1, "duo": -1, "spec": 1, "coop": 1}, 112, SPEC),
    ("closed_loop", 3, {}, 113, SPEC),
    ("solve_keys", 6, {}, 114, SPEC),
    ("rollout", 2, {}, 115, None),
]
LOOP_T = 3


def life_inputs(cfg, i):
    kind, B, _, seed, _ = LIFE[i]
    if kind == "poison":
        return poison_problem(cfg, B, seed)
    if kind in ("closed_loop", "solve_keys"):
        x0, xref, _, u, s = problem(cfg, B, seed)
        return x0, xref, np.stack([prng.PRNGKey(seed + b) for b in range(B)]), u, s
    return problem(cfg, B, seed)


def sample_of(B, seed):
    """Instances compared with the oracle: all of a small batch; the first, the last and three drawn ones of a larger one."""
    if B <= 8:
        return list(range(B))
    return sorted({0, B - 1, *np.random.default_rng(seed).choice(np.arange(1, B - 1), 3, replace=False).tolist()})


def oracle_call(O, cfg, model, kind, inputs, idx):
    """Oracle outputs of one call for the instances idx: a tuple of arrays [len(idx)][...] in the order the solver returns them."""
    x0, xref, nz, u, s = inputs
    P = cfg.num_particles
    if kind in ("solve", "poison", "solve_keys"):
        noise = (lambda b: orc.noise_from_key(nz[b], P, H)) if kind == "solve_keys" else (lambda b: nz[b])
        r = [O.solve(x0[b], xref[b], noise(b), u[b], float(s[b]))[:3] for b in idx]
        return tuple(np.stack([q[k] for q in r]) for k in range(3))
    if kind == "rollout":
        r = [O.rollout(x0[b], u[b], xref[b], nz[b], True, True) for b in idx]
        return np.array([q[0] for q in r], np.float32), np.stack([q[1] for q in r]), np.stack([q[2] for q in r])
    if kind == "grad":
        r = [O.grad(x0[b], u[b], xref[b], nz[b]) for b in idx]
        return np.array([q[0] for q in r], np.float32), np.stack([q[1].astype(np.float32) for q in r])
    assert kind == "closed_loop"
    full = closed_loop_ref(cfg, model, x0, xref[None], nz, LOOP_T, u_init=u, stepsize_in=s, episodes=idx, O=O)
    return tuple(a[idx] for a in full)


@functools.lru_cache(maxsize=None)
def life_reference(mlp, math, full=False):
    """[(idx, oracle outputs)] per call of the script. full: every instance (the CPU conditions), else sample_of."""
    cfg, model = cfg_for(LIFE_P, mlp, math), synthetic_iris()
    O = orc.Oracle(cfg, model)
    oracle_threads()
    try:
        out = []
        for i, (kind, B, _, seed, _) in enumerate(LIFE):
            idx = list(range(B)) if full else sample_of(B, seed)
            out.append((idx, oracle_call(O, cfg, model, kind, life_inputs(cfg, i), idx)))
        return out
    finally:
        oracle_threads(1)


# ---- B / C. small f32 cases on fresh inputs: one oracle result per (P, seed), shared by the layouts and entry points that run it ----
@functools.lru_cache(maxsize=None)
def small_reference(P, seed=7, B=3, mlp="f32", math="exact"):
    cfg, model = cfg_for(P, mlp, math), synthetic_iris()
    prob = problem(cfg, B, seed)
    O = orc.Oracle(cfg, model)
    oracle_threads()
    try:
        idx = list(range(B))
        return cfg, model, prob, {k: oracle_call(O, cfg, model, k, prob, idx) for k in ("solve", "rollout", "grad")}
    finally:
        oracle_threads(1)


def holds_sentinel(*arrays):
    return sum(int((np.ascontiguousarray(a, np.float32).view(np.uint32) == SENTINEL).sum()) for a in arrays)
