"""CPU reference of the batched closed loop from an aged, renormalised state estimate (SPEC.md §11g): the loop of obs_loop_ref.py with a per-episode history
list z (every substep state of the episode, xhist_in in front of x0) and `measure` fed z_{c - A} instead of the current state; with meas_renorm the attitude of
the measurement is then scaled by rsqrt of its squared length. Written with the existing oracle only: what obs_loop_ref.py uses, plus rsqrt and fma of the NumPy
restatement (oracle/sde_mpc_numpy.py). Test infrastructure, like obs_loop_ref.py (whose result this returns, by calling it, when nothing aged is given).

`mutant` builds a deliberately WRONG loop, for the discrimination tests: "age_off_by_one" reads z_{c - A + 1} for A > 0, "age_in_ticks" counts the age in
control ticks (z_{c - A n}, as far back as the list goes), "renorm_before_error" renormalises the attitude of x before the error instead of xm after it,
"dropout_updates" lets the history through on a dropout (xm = z_{c - A}, no error), "hist_newest_first" reads xhist_in newest first."""
import numpy as np

import orc
from closed_loop_ref import default_warm_start, oracle_for
from fault_loop_ref import faulted
from obs_loop_ref import _rows, measure, obs_loop_ref
from plant_loop_ref import plant_cfg, plant_dt
from rate_loop_ref import rate_command, rate_constants, thrust_setpoint
from scenario_loop_ref import gust
from timed_loop_ref import R2, lag_step, num_solves

F = np.float32
MUTANTS = ("age_off_by_one", "age_in_ticks", "renorm_before_error", "dropout_updates", "hist_newest_first")


def renormalise(x):
    """x with its attitude x[6:10] scaled to unit length: s = fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 q0))), r = rsqrt(s) (SPEC.md §3.2), q_i r."""
    x = np.asarray(x, F).copy()
    q0, q1, q2, q3 = x[6], x[7], x[8], x[9]
    s = R2.fma(q3, q3, R2.fma(q2, q2, R2.fma(q1, q1, F(q0 * q0))))
    r = F(R2.rsqrt(s))
    x[6:10] = [F(q0 * r), F(q1 * r), F(q2 * r), F(q3 * r)]
    return x


def age_loop_ref(cfg, model, plants, x0, xref, keys, T, meas_age=None, meas_age_max=None, meas_renorm=False, xhist_in=None, meas_keys=None, meas_noise=None,
                 meas_bias=None, meas_valid=None, xmeas_in=None, rate_loop=None, fault=None, substep_states=False, S=1, D=0, alpha=0.0, plant_of=None,
                 disturbance=None, substeps=1, dt=None, mlp_dtype=None, math_mode=None, u_init=None, stepsize_in=None, u_act_in=None, rate_integ_in=None,
                 rate_tail_in=None, episodes=None, mutant=None):
    """The §11g loop per episode; arguments as obs_loop_ref plus meas_age (an int, int[Ns] or int[Na][Ba]; None: zeros), meas_age_max (None: the largest age),
    meas_renorm and xhist_in ([B][age_max][13], oldest first; None: x0 in every row). Returns obs_loop_ref's values with xhist_next [B][age_max][13] behind
    xmeas_next when age_max > 0 (xsub stays last). Nothing aged given: obs_loop_ref's own result."""
    assert mutant is None or mutant in MUTANTS
    if meas_age is None and meas_age_max is None and not meas_renorm and xhist_in is None:
        assert mutant is None
        return obs_loop_ref(cfg, model, plants, x0, xref, keys, T, meas_keys=meas_keys, meas_noise=meas_noise, meas_bias=meas_bias, meas_valid=meas_valid,
                            xmeas_in=xmeas_in, rate_loop=rate_loop, fault=fault, substep_states=substep_states, S=S, D=D, alpha=alpha, plant_of=plant_of,
                            disturbance=disturbance, substeps=substeps, dt=dt, mlp_dtype=mlp_dtype, math_mode=math_mode, u_init=u_init, stepsize_in=stepsize_in,
                            u_act_in=u_act_in, rate_integ_in=rate_integ_in, rate_tail_in=rate_tail_in, episodes=episodes)
    assert meas_keys is not None, "an aged estimate is an observed one"
    x0 = np.asarray(x0, F)
    B, H, m, P = x0.shape[0], cfg.horizon, cfg.num_motors, cfg.num_particles
    T, S, D, n = int(T), int(S), int(D), int(substeps)
    assert S >= 1 and 0 <= D <= S * n and 0.0 <= float(alpha) <= 1.0
    assert rate_loop is not None or (rate_integ_in is None and rate_tail_in is None)
    Ns = num_solves(T, S)
    age = _rows(meas_age, Ns, B, (), np.int64)
    AM = int(meas_age_max) if meas_age_max is not None else (0 if age is None else int(age.max()))
    assert 0 <= AM <= min(S, T) * n and (age is None or (age.min() >= 0 and age.max() <= AM))
    assert xhist_in is None or AM > 0
    xh_in = np.repeat(x0[:, None], AM, axis=1) if xhist_in is None else np.asarray(xhist_in, F).reshape(B, AM, 13)
    if mutant == "hist_newest_first":
        xh_in = xh_in[:, ::-1]
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
    xh_next = np.zeros((B, AM, 13), F)
    for b in (range(B) if episodes is None else episodes):
        x, r, y, s = x0[b].copy(), keys[b].copy(), u_init[b].copy(), F(stepsize_in[b])
        a = (y[0] if u_act_in is None else np.asarray(u_act_in, F)[b]).copy()
        g, wt = g_in[b].copy(), t_in[b].copy()
        q, xm = meas_keys[b].copy(), xm_in[b].copy()
        z = [xh_in[b, i].copy() for i in range(AM)] + [x.copy()]          # z[-1] is the current state z_c, z[-1 - A] is z_{c - A}
        xs[b, 0] = x
        for j in range(Ns):
            for i in range(min(S, T - j * S)):
                k = j * S + i
                if i == 0:
                    ok = valid is None or int(row(valid, j, b)) != 0
                    q, me = orc.split(q, 2)                          # the observation chain advances at EVERY solve
                    A = 0 if age is None else int(row(age, j, b))
                    if mutant == "age_off_by_one" and A > 0:
                        A -= 1
                    if mutant == "age_in_ticks":
                        A = min(A * n, len(z) - 1)
                    if ok:
                        xa = z[-1 - A]
                        if mutant == "renorm_before_error" and meas_renorm:
                            xa = renormalise(xa)
                        xm = measure(xa, me, zero if sigma is None else row(sigma, j, b), zero if beta is None else row(beta, j, b))
                        if meas_renorm and mutant != "renorm_before_error":
                            xm = renormalise(xm)
                    elif mutant == "dropout_updates":
                        xm = z[-1 - A].copy()
                    xmeas[b, j] = xm
                    r1, sub = orc.split(r, 2)
                    uo, xe, inf, _ = O.solve(xm, xref[j if Tx > 1 else 0, b if Bx > 1 else 0], orc.noise_from_key(sub, P, H), y, s)
                    xe = np.asarray(xe, F)
                    r, p = orc.split(r1, 2)
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
                        c, g, _, _ = rate_command(K, u_row, cbar, wstar, x[10:13], g)          # the rate loop reads the PLANT's current rates
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
                    z.append(np.asarray(x, F).copy())
                xs[b, k + 1] = x
            y = np.stack([uo[min(t + S, H - 1)] for t in range(H)])
            if rate_loop is not None:
                wt = np.stack([xe[min(t + S, H - 1) + 1, 10:13] for t in range(H)]).astype(F)
            s = F(inf[1])
            info[b, j] = inf
        u_next[b], s_next[b], k_next[b], a_next[b], g_next[b], t_next[b] = y, s, r, a, g, wt
        q_next[b], xm_next[b] = q, xm
        if AM:
            xh_next[b] = np.stack(z[-1 - AM:-1])                      # z_{T n - AM} .. z_{T n - 1}
    out = (xs, us, info, u_next, s_next, k_next, a_next)
    if rate_loop is not None:
        out += (ws, g_next, t_next)
    out += (xmeas, q_next, xm_next)
    if AM:
        out += (xh_next,)
    return out + (xsub,) if substep_states else out
