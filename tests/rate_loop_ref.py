"""CPU reference of the batched closed loop through the rate-setpoint interface (SPEC.md §11d): the loop of scenario_loop_ref.py with the vehicle's
inner rate loop in front of the motor lag — setpoint (mean thrust, predicted body rates), rate error, clamped integrator, torque demand, mixer clamped
to the input bounds, blend with the solution's motor values. Written with the existing oracle only: orc.split, orc.noise_from_key, orc.normal(p, 6 n),
Oracle(cfg, model).solve, Oracle(plant_cfg, blob).step(..., t=0), timed_loop_ref.lag_step, scenario_loop_ref.gust and the fma of the NumPy restatement
(oracle/sde_mpc_numpy.py); everything else is one rounded float32 operation per line. Test infrastructure, like scenario_loop_ref.py (whose result
this returns, by calling it, when rate_loop is None).

`mutant` builds a deliberately WRONG loop, for the discrimination test of tests/test_rate_loop_cpu.py: "omega_stale" forms the rate error with the body
rates of the tick start instead of the current substep's, "row_r" takes the rate setpoint from xevol[r] instead of xevol[r + 1], "p_before_i" forms the
torque demand with the integrator BEFORE its update, "no_clamp" drops the mixer's clamp to the input bounds, "tail_unshifted" hands the next period the
rate tail without the shift by S rows, "sum_reversed" sums the thrust right to left."""
import numpy as np

import orc
from closed_loop_ref import default_warm_start, oracle_for
from plant_loop_ref import plant_cfg, plant_dt
from scenario_loop_ref import gust, scenario_loop_ref
from timed_loop_ref import R2, lag_step, num_solves

F = np.float32
MUTANTS = ("omega_stale", "row_r", "p_before_i", "no_clamp", "tail_unshifted", "sum_reversed")


def clamp(v, lo, hi):
    """v < lo ? lo : (v > hi ? hi : v), element by element (a NaN passes through)."""
    v, lo, hi = np.asarray(v, F), np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(F)


def thrust_setpoint(u_row, inv_m, reverse=False):
    """(u[0] + u[1] + ... + u[m-1]) * inv_m, the sum left to right, every operation rounded to float32."""
    u = np.asarray(u_row, F)
    if reverse:
        u = u[::-1]
    s = F(u[0])
    for l in range(1, u.shape[0]):
        s = F(s + u[l])
    return F(s * F(inv_m))


def rate_constants(cfg, model, rate_loop, dtp):
    """(kp[3], ki_dt[3], glim[3], M[m][3], w, inv_m, lo[m], hi[m]) as float32: what the Python layer and the library hand to the kernel."""
    m = cfg.num_motors
    M = np.asarray(model.rate_mixer() if rate_loop.mixer is None else rate_loop.mixer, F)
    assert M.shape == (m, 3)
    ki_dt = (np.asarray(rate_loop.ki, F) * F(dtp)).astype(F)
    bounds = np.asarray(cfg.input_bound, np.float64)[:m].astype(F)
    return (np.asarray(rate_loop.kp, F), ki_dt, np.asarray(rate_loop.integ_limit, F), M, F(rate_loop.motor_weight), F(F(1.0) / F(m)),
            bounds[:, 0].copy(), bounds[:, 1].copy())


def rate_command(K, u_row, cbar, wstar, omega, g, mutant=None):
    """Steps 2 - 6 of §11d for one substep: returns (c[m], g', input clamp active, integrator clamp active)."""
    kp, ki_dt, glim, M, w, _, lo, hi = K
    e = (np.asarray(wstar, F) - np.asarray(omega, F)).astype(F)
    g_raw = np.asarray(R2.fma(ki_dt, e, g), F)
    g_new = clamp(g_raw, -glim, glim)
    tau = np.asarray(R2.fma(kp, e, g if mutant == "p_before_i" else g_new), F)
    mix = np.full(M.shape[0], cbar, F)
    for a in range(3):
        mix = np.asarray(R2.fma(M[:, a], np.full(M.shape[0], tau[a], F), mix), F)
    c_om = mix if mutant == "no_clamp" else clamp(mix, lo, hi)
    u_row = np.asarray(u_row, F)
    if w == F(0.0):
        c = c_om
    elif w == F(1.0):
        c = u_row.copy()
    else:
        c = np.asarray(R2.fma(np.full_like(c_om, w), (u_row - c_om).astype(F), c_om), F)
    return c, g_new, bool((mix.tobytes() != clamp(mix, lo, hi).tobytes())), bool(g_raw.tobytes() != g_new.tobytes())


def rate_loop_ref(cfg, model, plants, x0, xref, keys, T, rate_loop=None, S=1, D=0, alpha=0.0, plant_of=None, disturbance=None, substeps=1, dt=None,
                  mlp_dtype=None, math_mode=None, u_init=None, stepsize_in=None, u_act_in=None, rate_integ_in=None, rate_tail_in=None, episodes=None,
                  mutant=None, census=False):
    """The §11d loop per episode; arguments as scenario_loop_ref plus rate_loop (a solver.RateLoop, or anything with its attributes), rate_integ_in [B][3]
    and rate_tail_in [B][H][3] (None: zeros). Returns the seven values of scenario_loop_ref followed by (ws [B][T][4], rate_integ_next [B][3],
    rate_tail_next [B][H][3]); with census=True, that tuple and a dict counting the plant substeps in which an input-bound clamp was active ("input"),
    in which an integrator clamp was active ("integ") and with neither ("free"). rate_loop=None: scenario_loop_ref's own result."""
    assert mutant is None or mutant in MUTANTS
    if rate_loop is None:
        assert rate_integ_in is None and rate_tail_in is None and mutant is None and not census
        return scenario_loop_ref(cfg, model, plants, x0, xref, keys, T, S=S, D=D, alpha=alpha, plant_of=plant_of, disturbance=disturbance, substeps=substeps,
                                 dt=dt, mlp_dtype=mlp_dtype, math_mode=math_mode, u_init=u_init, stepsize_in=stepsize_in, u_act_in=u_act_in, episodes=episodes)
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
    if plant_of.ndim == 1:
        plant_of = plant_of[None]
    Tp = plant_of.shape[0]
    assert Tp in (1, T) and plant_of.shape[1] == B and plant_of.min() >= 0 and plant_of.max() < Np
    if disturbance is not None:
        disturbance = np.asarray(disturbance, F)
        if disturbance.ndim == 1:
            disturbance = disturbance[None, None]
        elif disturbance.ndim == 2:
            assert disturbance.shape[0] == T
            disturbance = disturbance[:, None]
        Td, Bd = disturbance.shape[:2]
        assert Td in (1, T) and Bd in (1, B) and disturbance.shape[2] == 6
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
    count = dict(input=0, integ=0, free=0)
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
                Xi = orc.normal(p, 6 * n).reshape(n, 6)
                om_tick = x[10:13].copy()
                row = min(i, H - 1)
                for jj in range(n):
                    q = i * n + jj
                    fresh = q >= D
                    u_row = (uo if fresh else y)[row]
                    cbar = thrust_setpoint(u_row, inv_m, reverse=mutant == "sum_reversed")
                    wstar = (xe[row if mutant == "row_r" else row + 1, 10:13] if fresh else wt[row]).astype(F)
                    c, g, hit_in, hit_g = rate_command(K, u_row, cbar, wstar, om_tick if mutant == "omega_stale" else x[10:13], g, mutant)
                    count["input"] += hit_in
                    count["integ"] += hit_g
                    count["free"] += not (hit_in or hit_g)
                    a = lag_step(a, c, alpha)
                    if jj == 0:
                        us[b, k] = a
                        ws[b, k, 0], ws[b, k, 1:] = cbar, wstar
                    x, _ = OP[pi].step(x, a, Xi[jj], t=0)
                    if w is not None:
                        x = gust(x, w, dtp)
                xs[b, k + 1] = x
            y = np.stack([uo[min(t + S, H - 1)] for t in range(H)])
            wt = np.stack([xe[min(t + (0 if mutant == "tail_unshifted" else S), H - 1) + 1, 10:13] for t in range(H)]).astype(F)
            s = F(inf[1])
            info[b, j] = inf
        u_next[b], s_next[b], k_next[b], a_next[b], g_next[b], t_next[b] = y, s, r, a, g, wt
    out = (xs, us, info, u_next, s_next, k_next, a_next, ws, g_next, t_next)
    return (out, count) if census else out
