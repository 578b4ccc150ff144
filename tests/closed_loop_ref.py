"""CPU reference of the batched closed loop (SPEC.md §11), written with the existing oracle only: orc.split, orc.noise_from_key,
orc.normal(key, 6), Oracle.solve and Oracle.step(..., t=0). Test infrastructure, like orc.py."""
import numpy as np

import orc


def default_warm_start(cfg, B):
    """What sdempc_reset / MpcProblem.m_reset give: uref tiled, and ls_init_stepsize if ls_maxls > 0, else stepsize."""
    u = np.tile(np.asarray(cfg.uref, np.float32)[: cfg.num_motors], (B, cfg.horizon, 1))
    s = np.full(B, cfg.ls_init_stepsize if cfg.ls_maxls > 0 else cfg.stepsize, np.float32)
    return u, s


def oracle_for(cfg, model):
    return orc.Oracle(cfg, model, fast=getattr(cfg, "math_mode", "exact") == "fast")


def closed_loop_ref(cfg, model, x0, xref, keys, T, u_init=None, stepsize_in=None, episodes=None, O=None):
    """The §11 loop per episode. x0 f32[B][13]; xref f32[Tx][Bx][H+1][13]; keys uint32[B][2]. episodes: indices to compute (default all);
    the rows of the others stay zero. Returns (xs [B][T+1][13], us [B][T][m], info [B][T][8], u_next, stepsize_next, keys_next)."""
    x0 = np.asarray(x0, np.float32)
    B, H, m, P = x0.shape[0], cfg.horizon, cfg.num_motors, cfg.num_particles
    xref = np.asarray(xref, np.float32)
    if xref.ndim == 2:
        xref = xref[None, None]
    Tx, Bx = xref.shape[:2]
    keys = np.asarray(keys, np.uint32).reshape(B, 2)
    du, ds = default_warm_start(cfg, B)
    u_init = du if u_init is None else np.asarray(u_init, np.float32)
    stepsize_in = ds if stepsize_in is None else np.asarray(stepsize_in, np.float32)
    O = O or oracle_for(cfg, model)
    xs = np.zeros((B, T + 1, 13), np.float32)
    us = np.zeros((B, T, m), np.float32)
    info = np.zeros((B, T, 8), np.float32)
    u_next = np.zeros((B, H, m), np.float32)
    s_next = np.zeros(B, np.float32)
    k_next = np.zeros((B, 2), np.uint32)
    for b in (range(B) if episodes is None else episodes):
        x, r, y, s = x0[b].copy(), keys[b].copy(), u_init[b].copy(), np.float32(stepsize_in[b])
        xs[b, 0] = x
        for k in range(T):
            r1, sub = orc.split(r, 2)
            noise = orc.noise_from_key(sub, P, H)
            uo, _, inf, _ = O.solve(x, xref[k if Tx > 1 else 0, b if Bx > 1 else 0], noise, y, s)
            r, p = orc.split(r1, 2)
            x, _ = O.step(x, uo[0], orc.normal(p, 6), t=0)
            y = np.concatenate([uo[1:], uo[-1:]], axis=0)
            s = np.float32(inf[1])
            xs[b, k + 1], us[b, k], info[b, k] = x, uo[0], inf
        u_next[b], s_next[b], k_next[b] = y, s, r
    return xs, us, info, u_next, s_next, k_next
