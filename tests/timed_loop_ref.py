"""CPU reference of the batched closed loop at the node's timing (SPEC.md §11b): solve period S, solve delay D (plant substeps), first-order
motor lag alpha. Written with the existing oracle only: orc.split, orc.noise_from_key, orc.normal(p, 6 n), Oracle(cfg, model).solve and
Oracle(plant_cfg, plant).step(..., t=0) (plant_loop_ref.plant_cfg), plus float32 arithmetic for the lag: one rounded subtraction and one fma,
the exact software fma of the NumPy restatement (oracle/sde_mpc_numpy.py). Test infrastructure, like plant_loop_ref.py (whose loop this is at
S = 1, D = 0, alpha = 0)."""
import os
import sys

import numpy as np

import orc
from closed_loop_ref import default_warm_start, oracle_for
from plant_loop_ref import plant_cfg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import sde_mpc_numpy as R2  # noqa: E402

F = np.float32


def num_solves(T, S):
    return -(-int(T) // int(S))


def lag_step(a, c, alpha):
    """a_l <- fma(alpha, c_l - a_l, a_l) in float32 (alpha > 0), or c exactly (alpha = 0)."""
    a, c = np.asarray(a, F), np.asarray(c, F)
    if F(alpha) == F(0.0):
        return c.copy()
    d = (c - a).astype(F)                                  # one rounded float32 subtraction
    return np.asarray(R2.fma(np.full_like(d, F(alpha)), d, a), F)


def key_schedule(r, S, T):
    """The keys of SPEC.md §11b for one episode: ([sub_j for every solve], [p_k for every tick], r after tick T - 1). Depends on S and T only."""
    subs, ps = [], []
    r = np.asarray(r, np.uint32).reshape(2).copy()
    for k in range(T):
        if k % S == 0:
            r1, sub = orc.split(r, 2)
            subs.append(sub.copy())
            r, p = orc.split(r1, 2)
        else:
            r, p = orc.split(r, 2)
        ps.append(p.copy())
    return subs, ps, r.copy()


def timed_loop_ref(cfg, model, plants, x0, xref, keys, T, S=1, D=0, alpha=0.0, plant_of=None, substeps=1, dt=None, mlp_dtype=None, math_mode=None,
                   u_init=None, stepsize_in=None, u_act_in=None, episodes=None):
    """The §11b loop per episode. plants: one model / blob or a sequence (None: the controller's model); xref f32[Tx][Bx][H+1][13] with Tx in
    {1, Ns}. Returns (xs [B][T+1][13], us [B][T][m], info [B][Ns][8], u_next, stepsize_next, keys_next, u_act_next)."""
    x0 = np.asarray(x0, F)
    B, H, m, P = x0.shape[0], cfg.horizon, cfg.num_motors, cfg.num_particles
    T, S, D, n = int(T), int(S), int(D), int(substeps)
    assert S >= 1 and 0 <= D <= S * n and 0.0 <= float(alpha) <= 1.0
    Ns = num_solves(T, S)
    if plants is None:
        plants = model
    plants = [plants] if hasattr(plants, "to_blob") or isinstance(plants, (bytes, bytearray)) else list(plants)
    Np = len(plants)
    if plant_of is None:
        assert Np in (1, B)
        plant_of = np.zeros(B, np.int32) if Np == 1 else np.arange(B, dtype=np.int32)
    plant_of = np.asarray(plant_of, np.int32)
    xref = np.asarray(xref, F)
    if xref.ndim == 2:
        xref = xref[None, None]
    Tx, Bx = xref.shape[:2]
    assert Tx in (1, Ns) and Bx in (1, B)
    keys = np.asarray(keys, np.uint32).reshape(B, 2)
    du, ds = default_warm_start(cfg, B)
    u_init = du if u_init is None else np.asarray(u_init, F)
    stepsize_in = ds if stepsize_in is None else np.asarray(stepsize_in, F)
    O = oracle_for(cfg, model)
    pcfg = plant_cfg(cfg, n, dt, mlp_dtype, math_mode)
    OP = {}
    xs = np.zeros((B, T + 1, 13), F)
    us = np.zeros((B, T, m), F)
    info = np.zeros((B, Ns, 8), F)
    u_next = np.zeros((B, H, m), F)
    s_next = np.zeros(B, F)
    k_next = np.zeros((B, 2), np.uint32)
    a_next = np.zeros((B, m), F)
    for b in (range(B) if episodes is None else episodes):
        pi = int(plant_of[b])
        if pi not in OP:
            OP[pi] = oracle_for(pcfg, plants[pi])
        x, r, y, s = x0[b].copy(), keys[b].copy(), u_init[b].copy(), F(stepsize_in[b])
        a = (y[0] if u_act_in is None else np.asarray(u_act_in, F)[b]).copy()
        xs[b, 0] = x
        for j in range(Ns):
            for i in range(min(S, T - j * S)):
                k = j * S + i
                if i == 0:
                    r1, sub = orc.split(r, 2)
                    uo, _, inf, _ = O.solve(x, xref[j if Tx > 1 else 0, b if Bx > 1 else 0], orc.noise_from_key(sub, P, H), y, s)
                    r, p = orc.split(r1, 2)
                else:
                    r, p = orc.split(r, 2)
                Xi = orc.normal(p, 6 * n).reshape(n, 6)
                for jj in range(n):
                    q = i * n + jj
                    c = (uo if q >= D else y)[min(i, H - 1)]
                    a = lag_step(a, c, alpha)
                    if jj == 0:
                        us[b, k] = a
                    x, _ = OP[pi].step(x, a, Xi[jj], t=0)
                xs[b, k + 1] = x
            y = np.stack([uo[min(t + S, H - 1)] for t in range(H)])
            s = F(inf[1])
            info[b, j] = inf
        u_next[b], s_next[b], k_next[b], a_next[b] = y, s, r, a
    return xs, us, info, u_next, s_next, k_next, a_next
