"""CPU reference of the batched closed loop on a measured state (SPEC.md §11f): the loop of fault_loop_ref.py with the measurement in front of every solve — the
solve starts from the held measurement xm, the plant goes on from x. Written with the existing oracle only: orc.split, orc.normal(me, 12),
Oracle(cfg, model).solve, Oracle(plant_cfg, blob).step(..., t=0), the fma of the NumPy restatement (oracle/sde_mpc_numpy.py) and the helpers of the other
*_loop_ref.py modules (lag_step, gust, rate_command, faulted). Test infrastructure, like fault_loop_ref.py (whose result this returns, by calling it, when
meas_keys is None).

`mutant` builds a deliberately WRONG loop, for the discrimination tests: "quat_sign" flips one sign of the attitude product, "pair_next" draws the twelve
normals pairing counter i with i + 1 instead of i + 6, "chain_held" does not advance the observation chain on a dropout, "no_beta" drops the bias,
"plant_from_xm" steps the plant from the measurement instead of the state, "theta_omega_swapped" gives the attitude the body-rate slots of e and the body
rates the attitude slots."""
import ctypes as C

import numpy as np

import orc
from closed_loop_ref import default_warm_start, oracle_for
from fault_loop_ref import fault_loop_ref, faulted
from plant_loop_ref import plant_cfg, plant_dt
from rate_loop_ref import rate_command, rate_constants, thrust_setpoint
from scenario_loop_ref import gust
from timed_loop_ref import R2, lag_step, num_solves

F = np.float32
MUTANTS = ("quat_sign", "pair_next", "chain_held", "no_beta", "plant_from_xm", "theta_omega_swapped")


def _normal_pair_next(key):
    """Twelve normals from blocks (0, 1), (2, 3), .. (10, 11): element 2 i is the first word of block i, element 2 i + 1 the second (a WRONG pairing)."""
    fn = orc.lib().orc_bits_to_normal
    fn.restype, fn.argtypes = C.c_float, [C.c_uint32]
    out = np.zeros(12, F)
    for i in range(6):
        a, b = orc.threefry2x32(key, 2 * i, 2 * i + 1)
        out[2 * i], out[2 * i + 1] = fn(a), fn(b)
    return out


def measure(x, me_key, sigma_row, beta_row, mutant=None):
    """xm of one valid solve: e = fma(sigma, normal(me, (12,)), beta); p, v, omega plus their e; the attitude times (1, e[6:9] / 2) from the right."""
    x = np.asarray(x, F)
    sigma, beta = np.asarray(sigma_row, F).reshape(12), np.asarray(beta_row, F).reshape(12)
    xi = _normal_pair_next(me_key) if mutant == "pair_next" else orc.normal(me_key, 12)
    if mutant == "no_beta":
        beta = np.zeros(12, F)
    e = np.asarray(R2.fma(sigma.copy(), xi, beta.copy()), F)
    th, om = (e[9:12], e[6:9]) if mutant == "theta_omega_swapped" else (e[6:9], e[9:12])
    xm = np.zeros(13, F)
    xm[0:3] = x[0:3] + e[0:3]
    xm[3:6] = x[3:6] + e[3:6]
    xm[10:13] = x[10:13] + om
    h = (F(0.5) * th).astype(F)
    w, qx, qy, qz = x[6], x[7], x[8], x[9]
    f = R2.fma
    s = F(1.0) if mutant == "quat_sign" else F(-1.0)
    xm[6] = f(-qz, h[2], f(-qy, h[1], f(-qx, h[0], w)))
    xm[7] = f(-qz, h[1], f(qy, h[2], f(w, h[0], qx)))
    xm[8] = f(s * qx, h[2], f(qz, h[0], f(w, h[1], qy)))
    xm[9] = f(-qy, h[0], f(qx, h[1], f(w, h[2], qz)))
    return xm


def _rows(v, Ns, B, tail, dtype):
    """[No][Bo] + tail from the short forms tail and [Ns] + tail; None stays None."""
    if v is None:
        return None
    a = np.asarray(v, dtype)
    if a.shape == tail:
        a = a[None, None]
    elif a.shape == (Ns,) + tail:
        a = a[:, None]
    assert a.ndim == len(tail) + 2 and a.shape[0] in (1, Ns) and a.shape[1] in (1, B) and a.shape[2:] == tail, a.shape
    return a


def obs_loop_ref(cfg, model, plants, x0, xref, keys, T, meas_keys=None, meas_noise=None, meas_bias=None, meas_valid=None, xmeas_in=None, rate_loop=None,
                 fault=None, substep_states=False, S=1, D=0, alpha=0.0, plant_of=None, disturbance=None, substeps=1, dt=None, mlp_dtype=None, math_mode=None,
                 u_init=None, stepsize_in=None, u_act_in=None, rate_integ_in=None, rate_tail_in=None, episodes=None, mutant=None):
    """The §11f loop per episode; arguments as fault_loop_ref plus meas_keys uint32[B][2], meas_noise / meas_bias (f32[No][Bo][12], [Ns][12] or [12]; None:
    zeros), meas_valid (int[Nv][Bv] or [Ns]; None: always valid) and xmeas_in ([B][13]; None: x0). Returns fault_loop_ref's values (seven without a rate loop,
    ten with one), then xmeas [B][Ns][13], meas_keys_next [B][2], xmeas_next [B][13], then xsub when substep_states is set. meas_keys=None: fault_loop_ref's own
    result."""
    assert mutant is None or mutant in MUTANTS
    if meas_keys is None:
        assert mutant is None and meas_noise is None and meas_bias is None and meas_valid is None and xmeas_in is None
        return fault_loop_ref(cfg, model, plants, x0, xref, keys, T, rate_loop=rate_loop, fault=fault, substep_states=substep_states, S=S, D=D, alpha=alpha,
                              plant_of=plant_of, disturbance=disturbance, substeps=substeps, dt=dt, mlp_dtype=mlp_dtype, math_mode=math_mode, u_init=u_init,
                              stepsize_in=stepsize_in, u_act_in=u_act_in, rate_integ_in=rate_integ_in, rate_tail_in=rate_tail_in, episodes=episodes)
    x0 = np.asarray(x0, F)
    B, H, m, P = x0.shape[0], cfg.horizon, cfg.num_motors, cfg.num_particles
    T, S, D, n = int(T), int(S), int(D), int(substeps)
    assert S >= 1 and 0 <= D <= S * n and 0.0 <= float(alpha) <= 1.0
    assert rate_loop is not None or (rate_integ_in is None and rate_tail_in is None)
    Ns = num_solves(T, S)
    if plants is None:
        plants = model
    plants = [plants] if hasattr(plants, "to_blob") or isinstance(plants, (bytes, bytearray)) else list(plants)
    Np = len(plants)
    if plant_of is None:
        assert Np in (1, B)
        plant_of = np.zeros(B, np.int32) if Np == 1 else np.arange(B, dtype=np.int32)
    plant_of = np.asarray(plant_of, np.int32)
    if plant_of.ndim == 1:
        plant_of = plant_of[None]
    Tp = plant_of.shape[0]
    assert Tp in (1, T) and plant_of.shape[1] == B and plant_of.min() >= 0 and plant_of.max() < Np
    Td = Bd = 1
    if disturbance is not None:
        disturbance = np.asarray(disturbance, F)
        if disturbance.ndim == 1:
            disturbance = disturbance[None, None]
        elif disturbance.ndim == 2:
            assert disturbance.shape[0] == T
            disturbance = disturbance[:, None]
        Td, Bd = disturbance.shape[:2]
        assert Td in (1, T) and Bd in (1, B) and disturbance.shape[2] == 6
    Tf = Bf = 1
    if fault is not None:
        fault = np.asarray(fault, F)
        if fault.ndim == 2:
            fault = fault[None, None]
        elif fault.ndim == 3:
            assert fault.shape[0] == T
            fault = fault[:, None]
        Tf, Bf = fault.shape[:2]
        assert Tf in (1, T) and Bf in (1, B) and fault.shape[2:] == (m, 2) and np.isfinite(fault).all()
    sigma, beta, valid = _rows(meas_noise, Ns, B, (12,), F), _rows(meas_bias, Ns, B, (12,), F), _rows(meas_valid, Ns, B, (), np.int32)
    assert sigma is None or (np.isfinite(sigma).all() and (sigma >= 0).all())
    assert beta is None or np.isfinite(beta).all()
    assert valid is None or np.isin(valid, (0, 1)).all()
    zero = np.zeros(12, F)

    def row(a, j, b):
        return a[j if a.shape[0] > 1 else 0, b if a.shape[1] > 1 else 0]
    xref = np.asarray(xref, F)
    if xref.ndim == 2:
        xref = xref[None, None]
    Tx, Bx = xref.shape[:2]
    assert Tx in (1, Ns) and Bx in (1, B)
    keys = np.asarray(keys, np.uint32).reshape(B, 2)
    meas_keys = np.asarray(meas_keys, np.uint32).reshape(B, 2)
    xm_in = x0 if xmeas_in is None else np.asarray(xmeas_in, F).reshape(B, 13)
    du, ds = default_warm_start(cfg, B)
    u_init = du if u_init is None else np.asarray(u_init, F)
    stepsize_in = ds if stepsize_in is None else np.asarray(stepsize_in, F)
    g_in = np.zeros((B, 3), F) if rate_integ_in is None else np.asarray(rate_integ_in, F)
    t_in = np.zeros((B, H, 3), F) if rate_tail_in is None else np.asarray(rate_tail_in, F)
    O = oracle_for(cfg, model)
    pcfg = plant_cfg(cfg, n, dt, mlp_dtype, math_mode)
    dtp = plant_dt(cfg, n, dt)
    K = inv_m = None
    if rate_loop is not None:
        K = rate_constants(cfg, model, rate_loop, dtp)
        inv_m = K[5]
    OP = {}
    xs = np.zeros((B, T + 1, 13), F)
    us = np.zeros((B, T, m), F)
    ws = np.zeros((B, T, 4), F)
    info = np.zeros((B, Ns, 8), F)
    u_next = np.zeros((B, H, m), F)
    s_next = np.zeros(B, F)
    k_next = np.zeros((B, 2), np.uint32)
    a_next = np.zeros((B, m), F)
    g_next = np.zeros((B, 3), F)
    t_next = np.zeros((B, H, 3), F)
    xsub = np.zeros((B, T * n, 13), F)
    xmeas = np.zeros((B, Ns, 13), F)
    q_next = np.zeros((B, 2), np.uint32)
    xm_next = np.zeros((B, 13), F)
    for b in (range(B) if episodes is None else episodes):
        x, r, y, s = x0[b].copy(), keys[b].copy(), u_init[b].copy(), F(stepsize_in[b])
        a = (y[0] if u_act_in is None else np.asarray(u_act_in, F)[b]).copy()
        g, wt = g_in[b].copy(), t_in[b].copy()
        q, xm = meas_keys[b].copy(), xm_in[b].copy()
        xs[b, 0] = x
        for j in range(Ns):
            for i in range(min(S, T - j * S)):
                k = j * S + i
                if i == 0:
                    ok = valid is None or int(row(valid, j, b)) != 0
                    if ok or mutant != "chain_held":
                        q, me = orc.split(q, 2)                      # the observation chain advances at EVERY solve
                    if ok:
                        xm = measure(x, me, zero if sigma is None else row(sigma, j, b), zero if beta is None else row(beta, j, b), mutant)
                    xmeas[b, j] = xm
                    r1, sub = orc.split(r, 2)
                    uo, xe, inf, _ = O.solve(xm, xref[j if Tx > 1 else 0, b if Bx > 1 else 0], orc.noise_from_key(sub, P, H), y, s)
                    xe = np.asarray(xe, F)
                    r, p = orc.split(r1, 2)
                    if mutant == "plant_from_xm":
                        x = xm.copy()
                else:
                    r, p = orc.split(r, 2)
                pi = int(plant_of[k if Tp > 1 else 0, b])
                if pi not in OP:
                    OP[pi] = oracle_for(pcfg, plants[pi])
                w = None if disturbance is None else disturbance[k if Td > 1 else 0, b if Bd > 1 else 0]
                kb = None if fault is None else fault[k if Tf > 1 else 0, b if Bf > 1 else 0]
                Xi = orc.normal(p, 6 * n).reshape(n, 6)
                rw = min(i, H - 1)
                for jj in range(n):
                    qq = i * n + jj
                    fresh = qq >= D
                    u_row = (uo if fresh else y)[rw]
                    if rate_loop is None:
                        c = u_row
                    else:
                        cbar = thrust_setpoint(u_row, inv_m)
                        wstar = (xe[rw + 1, 10:13] if fresh else wt[rw]).astype(F)
                        c, g, _, _ = rate_command(K, u_row, cbar, wstar, x[10:13], g)          # the rate loop reads the PLANT's rates
                    a = lag_step(a, c, alpha)
                    if jj == 0:
                        us[b, k] = a
                        if rate_loop is not None:
                            ws[b, k, 0], ws[b, k, 1:] = cbar, wstar
                    at = a if kb is None else faulted(a, kb)
                    x, _ = OP[pi].step(x, at, Xi[jj], t=0)
                    if w is not None:
                        x = gust(x, w, dtp)
                    xsub[b, k * n + jj] = x
                xs[b, k + 1] = x
            y = np.stack([uo[min(t + S, H - 1)] for t in range(H)])
            if rate_loop is not None:
                wt = np.stack([xe[min(t + S, H - 1) + 1, 10:13] for t in range(H)]).astype(F)
            s = F(inf[1])
            info[b, j] = inf
        u_next[b], s_next[b], k_next[b], a_next[b], g_next[b], t_next[b] = y, s, r, a, g, wt
        q_next[b], xm_next[b] = q, xm
    out = (xs, us, info, u_next, s_next, k_next, a_next)
    if rate_loop is not None:
        out += (ws, g_next, t_next)
    out += (xmeas, q_next, xm_next)
    return out + (xsub,) if substep_states else out
