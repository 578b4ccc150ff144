"""CPU reference of the batched closed loop with per-motor actuator faults and substep-resolution states (SPEC.md §11e): the loop of rate_loop_ref.py
(of scenario_loop_ref.py when rate_loop is None) with one exact fma between the motor state and the plant step, at_l = fma(kappa_l, a_l, beta_l), and
a record of the state after every plant substep. Written with the existing oracle only: orc.split, orc.noise_from_key, orc.normal(p, 6 n),
Oracle(cfg, model).solve, Oracle(plant_cfg, blob).step(..., t=0), timed_loop_ref.lag_step, scenario_loop_ref.gust, rate_loop_ref.rate_command and
the fma of the NumPy restatement (oracle/sde_mpc_numpy.py). Test infrastructure, like rate_loop_ref.py (whose result this returns, by calling it,
when fault is None and substep_states is False).

`mutant` builds a deliberately WRONG loop, for the discrimination test of tests/test_fault_loop_cpu.py: "row_prev" reads the fault row of tick k - 1
(tick 0: row 0), "motors_reversed" gives motor l the pair of motor m - 1 - l, "no_beta" drops beta, "fed_back" writes the faulted value back into the
motor state (so that the lag, us and u_act_next see it)."""
import numpy as np

import orc
from closed_loop_ref import default_warm_start, oracle_for
from plant_loop_ref import plant_cfg, plant_dt
from rate_loop_ref import rate_command, rate_constants, rate_loop_ref, thrust_setpoint
from scenario_loop_ref import gust
from timed_loop_ref import R2, lag_step, num_solves

F = np.float32
MUTANTS = ("row_prev", "motors_reversed", "no_beta", "fed_back")


def faulted(a, kb, mutant=None):
    """fma(kappa_l, a_l, beta_l) per motor; kb f32[m][2]."""
    kb = np.asarray(kb, F)
    if mutant == "motors_reversed":
        kb = kb[::-1]
    beta = np.zeros(kb.shape[0], F) if mutant == "no_beta" else kb[:, 1]
    return np.asarray(R2.fma(kb[:, 0].copy(), np.asarray(a, F), beta.copy()), F)


def fault_loop_ref(cfg, model, plants, x0, xref, keys, T, rate_loop=None, fault=None, substep_states=False, S=1, D=0, alpha=0.0, plant_of=None,
                   disturbance=None, substeps=1, dt=None, mlp_dtype=None, math_mode=None, u_init=None, stepsize_in=None, u_act_in=None, rate_integ_in=None,
                   rate_tail_in=None, episodes=None, mutant=None):
    """The §11e loop per episode; arguments as rate_loop_ref plus fault (f32[Tf][Bf][m][2] with Tf in {1, T} and Bf in {1, B}, or [T][m][2], or [m][2];
    None: no fma at all) and substep_states. Returns rate_loop_ref's values (seven without a rate loop, ten with one), followed by
    xsub [B][T n][13] when substep_states is set. fault=None and substep_states=False: rate_loop_ref's own result."""
    assert mutant is None or mutant in MUTANTS
    common = dict(S=S, D=D, alpha=alpha, plant_of=plant_of, disturbance=disturbance, substeps=substeps, dt=dt, mlp_dtype=mlp_dtype, math_mode=math_mode,
                  u_init=u_init, stepsize_in=stepsize_in, u_act_in=u_act_in, rate_integ_in=rate_integ_in, rate_tail_in=rate_tail_in, episodes=episodes)
    if fault is None and not substep_states:
        assert mutant is None
        return rate_loop_ref(cfg, model, plants, x0, xref, keys, T, rate_loop=rate_loop, **common)
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
    xref = np.asarray(xref, F)
    if xref.ndim == 2:
        xref = xref[None, None]
    Tx, Bx = xref.shape[:2]
    assert Tx in (1, Ns) and Bx in (1, B)
    keys = np.asarray(keys, np.uint32).reshape(B, 2)
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
    for b in (range(B) if episodes is None else episodes):
        x, r, y, s = x0[b].copy(), keys[b].copy(), u_init[b].copy(), F(stepsize_in[b])
        a = (y[0] if u_act_in is None else np.asarray(u_act_in, F)[b]).copy()
        g, wt = g_in[b].copy(), t_in[b].copy()
        xs[b, 0] = x
        for j in range(Ns):
            for i in range(min(S, T - j * S)):
                k = j * S + i
                if i == 0:
                    r1, sub = orc.split(r, 2)
                    uo, xe, inf, _ = O.solve(x, xref[j if Tx > 1 else 0, b if Bx > 1 else 0], orc.noise_from_key(sub, P, H), y, s)
                    xe = np.asarray(xe, F)
                    r, p = orc.split(r1, 2)
                else:
                    r, p = orc.split(r, 2)
                pi = int(plant_of[k if Tp > 1 else 0, b])
                if pi not in OP:
                    OP[pi] = oracle_for(pcfg, plants[pi])
                w = None if disturbance is None else disturbance[k if Td > 1 else 0, b if Bd > 1 else 0]
                kf = max(k - 1, 0) if mutant == "row_prev" else k
                kb = None if fault is None else fault[kf if Tf > 1 else 0, b if Bf > 1 else 0]
                Xi = orc.normal(p, 6 * n).reshape(n, 6)
                row = min(i, H - 1)
                for jj in range(n):
                    q = i * n + jj
                    fresh = q >= D
                    u_row = (uo if fresh else y)[row]
                    if rate_loop is None:
                        c = u_row
                    else:
                        cbar = thrust_setpoint(u_row, inv_m)
                        wstar = (xe[row + 1, 10:13] if fresh else wt[row]).astype(F)
                        c, g, _, _ = rate_command(K, u_row, cbar, wstar, x[10:13], g)
                    a = lag_step(a, c, alpha)
                    if jj == 0:
                        us[b, k] = a
                        if rate_loop is not None:
                            ws[b, k, 0], ws[b, k, 1:] = cbar, wstar
                    at = a if kb is None else faulted(a, kb, mutant)          # between the command and the rotor: a stays the lag state
                    x, _ = OP[pi].step(x, at, Xi[jj], t=0)
                    if mutant == "fed_back":
                        a = at
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
    out = (xs, us, info, u_next, s_next, k_next, a_next)
    if rate_loop is not None:
        out += (ws, g_next, t_next)
    return out + (xsub,) if substep_states else out
