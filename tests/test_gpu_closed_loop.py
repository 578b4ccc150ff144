"""Batched closed loop on the GPU (SPEC.md §11, sdempc_closed_loop_batch): bit for bit against the CPU reference of tests/closed_loop_ref.py
(a composition of the oracle's solve and step), against a host loop of single-tick GPU solves, in every layout, across
continuation, with diverging episodes and at a batch size that needs ticketed persistent launches."""
import functools
import os

import numpy as np
import pytest

import orc
import loop_cases
from cases import CDIR, bits_differ, diverging_single_rotor_case
from closed_loop_ref import closed_loop_ref
from sde4mbrl_px4_amd import load_mpc_config, prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu


def small_cfg(**kw):
    c1 = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml"))
    return c1.replace(**{"horizon": 10, "num_short_dt": 10, "num_particles": 33, "max_iter": 8, "max_no_improvement_iter": 8, **kw})


def episodes(cfg, B, seed):
    x0 = W.random_initial_states(B, seed)
    xref = np.stack([W.reference_window(0.1 * b, cfg.time_steps) for b in range(B)])[None]      # [1][B][H+1][13]
    keys = np.stack([prng.PRNGKey(seed + b) for b in range(B)])
    return x0, xref, keys


assert_same = functools.partial(loop_cases.same, names=loop_cases.NAMES[:6])


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
@pytest.mark.parametrize("mlp_dtype", ["f32", "f16", "f32x3"])
def test_closed_loop_matches_reference(mlp_dtype, math_mode):
    cfg = small_cfg(mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    B, T = 3, 5
    x0, xref, keys = episodes(cfg, B, 20)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T)
    S.solve_status()
    assert_same(got, closed_loop_ref(cfg, model, x0, xref, keys, T))
    assert np.isfinite(got[0]).all() and got[0][:, 0].tobytes() == x0.tobytes()
    S.close()


LAYOUTS = {  # name -> (B, P, handle options); the same loop in each, all bit-identical to the reference
    "lane": (1, 1, {"coop": 0}),          # (with the cooperative layouts on, a lone P = 1 instance takes the speculative one)
    "coop": (1, 33, {"spec": 0}),
    "spec": (1, 33, {}),
    "tile": (1, 33, {"lane": 0, "coop": 0}),
    "duo": (40, 40, {"duo": 1, "coop": 0}),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_closed_loop_in_every_layout(name):
    B, P, opts = LAYOUTS[name]
    cfg = small_cfg(num_particles=P)
    model = synthetic_iris()
    T = 4
    x0, xref, keys = episodes(cfg, B, 30)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
    got = S.closed_loop(x0, xref, keys, T)
    S.solve_status()
    kname = S.last_kernel_name()
    assert ("spec" in kname) == (name == "spec"), kname
    if name in ("lane", "coop"):
        assert {"lane": "TeamWave, 4, 0, false, 1,", "coop": ", 2, "}[name] in kname, kname      # MODE 1: lane layout, 2: cooperative
    sample = [0, B - 1] if B > 2 else list(range(B))
    want = closed_loop_ref(cfg, model, x0, xref, keys, T, episodes=sample)
    assert_same(got, want, eps=sample)
    S.close()


def host_loop(S, O, x0, xref, keys, T, u0, s0):
    """The same ticks driven from the host: solve_keys (GPU) + Oracle.step + prng.split."""
    B = x0.shape[0]
    Tx, Bx = xref.shape[:2]
    x, r, y, s = x0.copy(), keys.copy(), u0.copy(), s0.copy()
    xs, us, info = [x.copy()], [], []
    for k in range(T):
        sp = [prng.split(r[b], 2) for b in range(B)]
        sub = np.stack([q[1] for q in sp])
        xr = np.stack([xref[k if Tx > 1 else 0, b if Bx > 1 else 0] for b in range(B)])
        uo, _, inf = S.solve_keys(x, xr, sub, y, s)
        sp2 = [prng.split(q[0], 2) for q in sp]
        r = np.stack([q[0] for q in sp2])
        x = np.stack([O.step(x[b], uo[b, 0], orc.normal(sp2[b][1], 6), t=0)[0] for b in range(B)])
        y = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)
        s = inf[:, 1].copy()
        xs.append(x.copy()); us.append(uo[:, 0].copy()); info.append(inf)
    return np.stack(xs, 1), np.stack(us, 1), np.stack(info, 1), y, s, r


@pytest.mark.parametrize("tx,bx", [("T", "1"), ("1", "B"), ("T", "B")])
def test_closed_loop_equals_host_loop_of_gpu_solves(tx, bx):
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(horizon=12, num_short_dt=12, num_particles=40, max_iter=6,
                                                                                      max_no_improvement_iter=6)
    model = synthetic_iris()
    B, T = 5, 6
    Tx, Bx = (T if tx == "T" else 1), (B if bx == "B" else 1)
    x0 = W.random_initial_states(B, 50)
    xref = np.stack([np.stack([W.reference_window(0.05 * k + 0.3 * b, cfg.time_steps) for b in range(Bx)]) for k in range(Tx)])
    keys = prng.split(prng.PRNGKey(9), B)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    u0[:, :, 1] += 0.01 * np.arange(B, dtype=np.float32)[:, None]          # warm starts that differ per episode
    s0 = np.full(B, i0["stepsize"], np.float32) * (1 + np.arange(B, dtype=np.float32))
    got = S.closed_loop(x0, xref, keys, T, u_init=u0, stepsize_in=s0)
    want = host_loop(S, orc.Oracle(cfg, model), x0, xref, keys, T, u0, s0)
    assert_same(got, want)
    S.close()


def test_closed_loop_continues():
    cfg = small_cfg(num_particles=40)
    model = synthetic_iris()
    B = 3
    x0, xref, keys = episodes(cfg, B, 60)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    full = S.closed_loop(x0, xref, keys, 7)
    a = S.closed_loop(x0, xref, keys, 3)
    b = S.closed_loop(a[0][:, -1], xref, a[5], 4, u_init=a[3], stepsize_in=a[4])
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), np.concatenate([a[1], b[1]], 1), np.concatenate([a[2], b[2]], 1)) + tuple(b[3:])
    assert_same(joined, full)
    S.close()


def test_closed_loop_diverging_episodes():
    """Two episodes whose solves meet non-finite costs (SPEC.md §3.7, §8) beside a finite one: the loop carries on exactly as the oracle
    composition does, and the finite episode is what it is on its own."""
    cfg, model, x0, xref, noise, u = diverging_single_rotor_case()
    B, T = x0.shape[0], 3
    keys = np.stack([prng.PRNGKey(300 + b) for b in range(B)])
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref[None], keys, T, u_init=u)
    S.solve_status()
    assert_same(got, closed_loop_ref(cfg, model, x0, xref[None], keys, T, u_init=u))
    assert (~np.isfinite(got[2][:2])).any()                                # the diverging episodes did meet non-finite values
    alone = S.closed_loop(x0[2:], xref[None, 2:], keys[2:], T, u_init=u[2:])
    assert_same(alone, tuple(g[2:] for g in got))
    assert np.isfinite(alone[0]).all()
    S.close()


def test_closed_loop_at_ticketed_batch_size():
    cfg = small_cfg(num_particles=40, max_iter=2, max_no_improvement_iter=2)
    model = synthetic_iris()
    B, T = 4700, 3
    x0 = W.random_initial_states(B, 70)
    xref = W.reference_window(0.0, cfg.time_steps)                           # one window, every tick, every episode
    keys = prng.split(prng.PRNGKey(11), B)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    got = S.closed_loop(x0, xref, keys, T)
    assert ", false, 3, " in S.last_kernel_name() and 3 * 6 * S.get_option("device_cus") <= B      # persistent, ticketed
    S.solve_status()
    sample = sorted(np.random.default_rng(5).choice(B, 3, replace=False).tolist()) + [B - 1]
    want = closed_loop_ref(cfg, model, x0[sample], xref, keys[sample], T)
    assert_same(tuple(g[sample] for g in got), want)
    S.close()


def test_simulate_is_closed_loop_in_the_solver_frame():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    cfg = small_cfg(num_particles=1)
    model = synthetic_iris()
    T = 5
    x = W.random_initial_states(1, 80)[0]
    rng = prng.PRNGKey(81)
    prob = MpcProblem(cfg=cfg, model=model, state_from_traj=W.lemniscate_state)
    xs, us, info, st, rng_T = prob.simulate(x, rng, T, curr_t=0.4)
    assert xs.shape == (T + 1, 13) and xs[0].tobytes() == x.tobytes()
    xsol = enu2ned(x, np)
    xref = np.stack([prob.xref(0.4 + k * float(cfg.time_steps[0]), xsol) for k in range(T)])[:, None]
    S = SdeMpcSolver(cfg, model, max_batch=1)
    g = S.closed_loop(xsol[None], xref, rng[None], T)
    assert bits_differ(xs[1:], enu2ned(g[0][0, 1:], np)) == 0 and bits_differ(us, g[1][0]) == 0 and bits_differ(info, g[2][0]) == 0
    assert bits_differ(st.yk, g[3][0]) == 0 and st.stepsize == g[4][0] and np.array_equal(rng_T, g[5][0])
    prob.shift_warm_start = False
    with pytest.raises(ValueError):
        prob.simulate(x, rng, 1)
    S.close()
