#!/usr/bin/env python3
"""Count, on the CPU oracle, the line-search trials whose Armijo bound thr = fma(ls_coef, g.d1, c_y) is negative (SPEC.md §8, implementation
note: with non-negative cost weights such a trial is rejected whatever its cost, and the kernels roll it out only when it is the last trial
of its line search). Per instance: trials, trials with thr < 0, and how many of those are not the last trial of their line search — what
sdempc_work_counters out[3] counts on the GPU.

The optimiser is the NumPy restatement's (oracle/sde_mpc_numpy.py Restatement.solve) driven by the C oracle's cost and gradient, as in
tests/test_solve_paths_cpu.py: the event record of the C oracle does not hold g.d1, the restatement's callables see every trial point. The
result is checked against the C oracle's own solve bit for bit before anything is printed.

usage: tests/tools/armijo_census.py                                   # instances 0-5 of the bench batch (C2, f32 / exact), a few CPU-minutes
       tests/tools/armijo_census.py --horizon 12 --particles 40 --ls-coef 0.5 --stepsize-in 1.0 --max-iter 14 --instances 2 --mlp-dtype f32x3 --math-mode fast
"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import orc
import sde_mpc_numpy as R
from sde4mbrl_px4_amd import load_mpc_config, synthetic_iris, prng
from sde4mbrl_px4_amd import workload as W

F = np.float32


def census(cfg, model, x0, xref, noise, u0, s0):
    """-> (trials, trials with thr < 0, of those not the last of their line search, info) of one solve"""
    O = orc.Oracle(cfg, model)
    N = R.Restatement(cfg, model, hw=R.HwTransc(orc.TRANSC_DIR) if cfg.math_mode == "fast" else None)
    at = {}                      # the gradient call's (c_y, g, yk): every trial until the next one is measured from it
    thr = []                     # one list of bounds per iteration

    def grad_fn(yy):
        c, g = O.grad(x0, yy, xref, noise)
        at.update(c_y=F(c), g=np.asarray(g, F), yk=np.asarray(yy, F).copy())
        thr.append([])
        return c, g

    def cost_fn(uu):
        if at:                   # (the call before the first gradient is the initial cost, not a trial)
            gd = N.dot256(at["g"], np.asarray(uu, F) - at["yk"])
            thr[-1].append(R.fma(F(cfg.ls_coef), gd, at["c_y"]))
        return O.rollout(x0, uu, xref, noise)[0]

    un, info = N.solve(cost_fn, grad_fn, u0, s0)
    uo, _, io, _ = O.solve(x0, xref, noise, u0, s0)
    assert un.tobytes() == uo.tobytes() and info.tobytes() == io.tobytes(), "the restatement's solve differs from the C oracle's"
    trials = sum(len(t) for t in thr)
    assert trials == int(info[7])
    neg = sum(sum(1 for v in t if v < 0) for t in thr)
    nonfinal = sum(sum(1 for v in t[:cfg.ls_maxls - 1] if v < 0) for t in thr)      # a line search that ends early ends on an ACCEPTED trial, whose thr >= c_n >= 0
    return trials, neg, nonfinal, info


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "c2_iris_traj_h50_p128.yaml"))
    ap.add_argument("--instances", type=int, default=6)
    ap.add_argument("--horizon", type=int, default=0)
    ap.add_argument("--particles", type=int, default=0)
    ap.add_argument("--ls-coef", type=float, default=None)
    ap.add_argument("--stepsize-in", type=float, default=None)
    ap.add_argument("--max-iter", type=int, default=0)
    ap.add_argument("--mlp-dtype", default="f32", choices=["f32", "f16", "f32x3"])
    ap.add_argument("--math-mode", default="exact", choices=["exact", "fast"])
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 1)
    a = ap.parse_args()
    cfg = load_mpc_config(a.config).replace(mlp_dtype=a.mlp_dtype, math_mode=a.math_mode)
    if a.horizon: cfg = cfg.replace(horizon=a.horizon)
    if a.particles: cfg = cfg.replace(num_particles=a.particles)
    if a.ls_coef is not None: cfg = cfg.replace(ls_coef=a.ls_coef)
    if a.max_iter: cfg = cfg.replace(max_iter=a.max_iter)
    s0 = cfg.ls_init_stepsize if a.stepsize_in is None else a.stepsize_in
    orc.set_threads(a.threads)
    B, H, P = a.instances, cfg.horizon, cfg.num_particles
    model = synthetic_iris()
    x0 = W.random_initial_states(B, 0)                   # the bench batch (benchlib/legs.py): instance b of rank 0
    keys = prng.split(prng.PRNGKey(10), B)
    u0 = np.tile(np.asarray(cfg.uref, F)[None], (H, 1))
    print(f"{os.path.basename(a.config)} H={H} P={P} {a.mlp_dtype}/{a.math_mode} ls_coef={cfg.ls_coef} stepsize_in={s0} max_iter={cfg.max_iter} maxls={cfg.ls_maxls}")
    tot = np.zeros(3, np.int64)
    for b in range(B):
        xref = W.reference_window(0.05 * (b % 160), cfg.time_steps)
        t, n, nf, info = census(cfg, model, x0[b], xref, orc.noise_from_key(keys[b], P, H), u0, s0)
        tot += (t, n, nf)
        print(f"instance {b}: N_it {int(info[2])}  trials {t}  thr<0 {n}  non-final thr<0 {nf}  ({nf / (t + 2):.4f} of the trials + 2 counted as rollouts)", flush=True)
    print(f"all {B}: trials {tot[0]}  thr<0 {tot[1]}  non-final thr<0 {tot[2]}  ({tot[2] / (tot[0] + 2 * B):.4f} of the counted rollouts)")
