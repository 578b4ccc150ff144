"""CPU reference of the batched closed loop with a scenario (SPEC.md §11c): the loop of timed_loop_ref.py plus a disturbance schedule
(six exact software fmas on the state after every plant step) and a plant schedule (Oracle.step of ANOTHER blob from a tick on). Written with
the existing oracle only: orc.split, orc.noise_from_key, orc.normal(p, 6 n), Oracle(cfg, model).solve, Oracle(plant_cfg, blob).step(..., t=0),
timed_loop_ref.lag_step and the fma of the NumPy restatement (oracle/sde_mpc_numpy.py). Test infrastructure, like timed_loop_ref.py (whose loop
this is with both schedules absent).

`mutant` builds a deliberately WRONG loop, for the discrimination test of tests/test_scenario_loop_cpu.py (the GPU parity shows nothing about a
choice on which the right and the wrong loop give the same bits): "fma_first" applies the six fmas before the step instead of after it, "dt0"
uses the controller's dt_0 instead of the plant's step length, "keep_sdt" lets a switched-in plant keep the sigma (hence sigma sqrt(dt)) of the
plant it replaced (the plant of the tick before the switch) until the next switch."""
import dataclasses

import numpy as np

import orc
from closed_loop_ref import default_warm_start, oracle_for
from plant_loop_ref import plant_cfg, plant_dt
from timed_loop_ref import R2, lag_step, num_solves

F = np.float32
MUTANTS = ("fma_first", "dt0", "keep_sdt")


def gust(x, w, dt):
    """v_i <- fma(w_v[i], dt, v_i) (x[3 + i]) and om_i <- fma(w_om[i], dt, om_i) (x[10 + i]), i = 0..2; position and attitude untouched."""
    x = np.array(x, F, copy=True)
    w = np.asarray(w, F).reshape(6)
    d = np.full(3, F(dt), F)
    x[3:6] = np.asarray(R2.fma(w[0:3], d, x[3:6]), F)
    x[10:13] = np.asarray(R2.fma(w[3:6], d, x[10:13]), F)
    return x


def scenario_loop_ref(cfg, model, plants, x0, xref, keys, T, S=1, D=0, alpha=0.0, plant_of=None, disturbance=None, substeps=1, dt=None,
                      mlp_dtype=None, math_mode=None, u_init=None, stepsize_in=None, u_act_in=None, episodes=None, mutant=None):
    """The §11c loop per episode. plants: one model / blob or a sequence (None: the controller's model); plant_of int[B] or int[Tp][B] with Tp in
    {1, T}; disturbance f32[Td][Bd][6] with Td in {1, T} and Bd in {1, B} (or [T][6], or [6]), None: no fmas at all. Returns the 7-tuple of
    timed_loop_ref."""
    assert mutant is None or mutant in MUTANTS
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
    assert Tp in (1, T) and plant_of.shape[1] == B and 1 <= Np <= B * Tp and plant_of.min() >= 0 and plant_of.max() < Np
    if disturbance is not None:
        disturbance = np.asarray(disturbance, F)
        if disturbance.ndim == 1:
            disturbance = disturbance[None, None]
        elif disturbance.ndim == 2:
            assert disturbance.shape[0] == T
            disturbance = disturbance[:, None]
        Td, Bd = disturbance.shape[:2]
        assert Td in (1, T) and Bd in (1, B) and disturbance.shape[2] == 6 and np.isfinite(disturbance).all()
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
    dtp = F(cfg.time_steps[0]) if mutant == "dt0" else plant_dt(cfg, n, dt)
    OP = {}

    def plant_oracle(pi, sigma_of=None):
        key = (pi, sigma_of)
        if key not in OP:
            mdl = plants[pi]
            if sigma_of is not None:            # (the "keep_sdt" mutant: the new vehicle with the old one's sigma)
                mdl = dataclasses.replace(mdl, sigma=np.array(plants[sigma_of].sigma, F, copy=True))
            OP[key] = oracle_for(pcfg, mdl)
        return OP[key]

    xs = np.zeros((B, T + 1, 13), F)
    us = np.zeros((B, T, m), F)
    info = np.zeros((B, Ns, 8), F)
    u_next = np.zeros((B, H, m), F)
    s_next = np.zeros(B, F)
    k_next = np.zeros((B, 2), np.uint32)
    a_next = np.zeros((B, m), F)
    for b in (range(B) if episodes is None else episodes):
        x, r, y, s = x0[b].copy(), keys[b].copy(), u_init[b].copy(), F(stepsize_in[b])
        a = (y[0] if u_act_in is None else np.asarray(u_act_in, F)[b]).copy()
        xs[b, 0] = x
        prev = sig = int(plant_of[0, b])     # the plant of the previous tick; ("keep_sdt") the plant whose sigma the current one flies with
        for j in range(Ns):
            for i in range(min(S, T - j * S)):
                k = j * S + i
                if i == 0:
                    r1, sub = orc.split(r, 2)
                    uo, _, inf, _ = O.solve(x, xref[j if Tx > 1 else 0, b if Bx > 1 else 0], orc.noise_from_key(sub, P, H), y, s)
                    r, p = orc.split(r1, 2)
                else:
                    r, p = orc.split(r, 2)
                pi = int(plant_of[k if Tp > 1 else 0, b])
                if pi != prev:                # a switch: the mutant keeps the sigma of the blob that is replaced
                    sig, prev = (prev if mutant == "keep_sdt" else pi), pi
                OPk = plant_oracle(pi, sig if sig != pi else None)
                w = None if disturbance is None else disturbance[k if Td > 1 else 0, b if Bd > 1 else 0]
                Xi = orc.normal(p, 6 * n).reshape(n, 6)
                for jj in range(n):
                    q = i * n + jj
                    c = (uo if q >= D else y)[min(i, H - 1)]
                    a = lag_step(a, c, alpha)
                    if jj == 0:
                        us[b, k] = a
                    if w is not None and mutant == "fma_first":
                        x = gust(x, w, dtp)
                    x, _ = OPk.step(x, a, Xi[jj], t=0)
                    if w is not None and mutant != "fma_first":
                        x = gust(x, w, dtp)
                xs[b, k + 1] = x
            y = np.stack([uo[min(t + S, H - 1)] for t in range(H)])
            s = F(inf[1])
            info[b, j] = inf
        u_next[b], s_next[b], k_next[b], a_next[b] = y, s, r, a
    return xs, us, info, u_next, s_next, k_next, a_next
