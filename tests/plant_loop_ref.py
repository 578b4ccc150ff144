"""CPU reference of the batched closed loop against a separate plant (SPEC.md §11a), written with the existing oracle only: orc.split,
orc.noise_from_key, orc.normal(p, 6 n), Oracle(cfg, model).solve and Oracle(cfg_plant, plant).step(..., t=0), where cfg_plant is the
controller's config with time_steps[0] = the plant's step length and the plant's two arithmetic switches. Test infrastructure, like
closed_loop_ref.py (whose loop this is, with steps 3 - 4 replaced)."""
import numpy as np

import orc
from closed_loop_ref import default_warm_start, oracle_for


def plant_dt(cfg, substeps, dt=None):
    """The plant's step length as float32: dt, or float32(time_steps[0]) / float32(substeps) (one float32 division)."""
    if dt is not None and float(dt) != 0.0:
        return np.float32(dt)
    return np.float32(np.float32(cfg.time_steps[0]) / np.float32(substeps))


def plant_cfg(cfg, substeps=1, dt=None, mlp_dtype=None, math_mode=None):
    """The controller's config with time_steps[0] = the plant's step length (asserted, as a float32) and the plant's arithmetic."""
    d = plant_dt(cfg, substeps, dt)
    kw = {"short_step_dt": float(d), "num_short_dt": max(1, min(cfg.num_short_dt, cfg.horizon))}
    if mlp_dtype is not None:
        kw["mlp_dtype"] = mlp_dtype
    if math_mode is not None:
        kw["math_mode"] = math_mode
    pc = cfg.replace(**kw)
    assert np.float32(pc.time_steps[0]).tobytes() == d.tobytes(), (pc.time_steps[0], d)
    return pc


def plant_loop_ref(cfg, model, plants, x0, xref, keys, T, plant_of=None, substeps=1, dt=None, mlp_dtype=None, math_mode=None, u_init=None,
                   stepsize_in=None, episodes=None):
    """The §11a loop per episode. plants: one model / blob or a sequence of them; plant_of int[B] (None: all 0 for one plant, identity for
    B plants). Other arguments and the returned tuple are closed_loop_ref's."""
    x0 = np.asarray(x0, np.float32)
    B, H, m, P = x0.shape[0], cfg.horizon, cfg.num_motors, cfg.num_particles
    plants = [plants] if hasattr(plants, "to_blob") or isinstance(plants, (bytes, bytearray)) else list(plants)
    Np, n = len(plants), int(substeps)
    if plant_of is None:
        assert Np in (1, B)
        plant_of = np.zeros(B, np.int32) if Np == 1 else np.arange(B, dtype=np.int32)
    plant_of = np.asarray(plant_of, np.int32)
    xref = np.asarray(xref, np.float32)
    if xref.ndim == 2:
        xref = xref[None, None]
    Tx, Bx = xref.shape[:2]
    keys = np.asarray(keys, np.uint32).reshape(B, 2)
    du, ds = default_warm_start(cfg, B)
    u_init = du if u_init is None else np.asarray(u_init, np.float32)
    stepsize_in = ds if stepsize_in is None else np.asarray(stepsize_in, np.float32)
    O = oracle_for(cfg, model)
    pcfg = plant_cfg(cfg, n, dt, mlp_dtype, math_mode)
    OP = {}
    xs = np.zeros((B, T + 1, 13), np.float32)
    us = np.zeros((B, T, m), np.float32)
    info = np.zeros((B, T, 8), np.float32)
    u_next = np.zeros((B, H, m), np.float32)
    s_next = np.zeros(B, np.float32)
    k_next = np.zeros((B, 2), np.uint32)
    for b in (range(B) if episodes is None else episodes):
        pi = int(plant_of[b])
        if pi not in OP:
            OP[pi] = oracle_for(pcfg, plants[pi])
        x, r, y, s = x0[b].copy(), keys[b].copy(), u_init[b].copy(), np.float32(stepsize_in[b])
        xs[b, 0] = x
        for k in range(T):
            r1, sub = orc.split(r, 2)
            noise = orc.noise_from_key(sub, P, H)
            uo, _, inf, _ = O.solve(x, xref[k if Tx > 1 else 0, b if Bx > 1 else 0], noise, y, s)
            r, p = orc.split(r1, 2)
            Xi = orc.normal(p, 6 * n).reshape(n, 6)          # ONE draw of 6 n values, row j for substep j
            for j in range(n):
                x, _ = OP[pi].step(x, uo[0], Xi[j], t=0)
            y = np.concatenate([uo[1:], uo[-1:]], axis=0)
            s = np.float32(inf[1])
            xs[b, k + 1], us[b, k], info[b, k] = x, uo[0], inf
        u_next[b], s_next[b], k_next[b] = y, s, r
    return xs, us, info, u_next, s_next, k_next
