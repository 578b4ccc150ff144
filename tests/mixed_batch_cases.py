"""Mixed batches for the persistent duo launches: pools of DISTINCT instances that end in different ways under one configuration, a fixed
pseudo-random arrangement of pool instances over the positions of a batch, and the grid arithmetic that says which positions one team solves one
after another.

A persistent launch (sdempc_kernels.hip: sdempc_solve_kernel MODE 3 / 4, launch_persistent) re-uses one LDS carve, one workspace slot, the staging
rows, the reduction scratch and the pair barrier word from instance to instance. The pools below put, on one team, a solve that the non-finite guard
ended (NaN left in the gradient, the momentum point, the trajectory rows) in front of a healthy one, a one-iteration solve in front of a full-length
one, and the reverse of each. tests/test_mixed_batch_cpu.py proves the stated properties of the pools and of the arrangement from the oracle's
records; tests/test_gpu_mixed_batch.py runs the launches and compares EVERY position with the oracle, bit for bit.
Nothing in this file supplies an expected value: expected values are the oracle's.
"""
import dataclasses
import functools
import os

import numpy as np

import kernel_census as kc
import orc
import solve_paths as sp
from cases import asymmetric_cfg, asymmetric_model, asymmetric_problem

MODE = {"f32": 0, "f16": 1, "f32x3": 2}
ABNORMAL = ("k0_nonfinite", "kgt0", "tol1")          # what a team solves before (and after) a full-length finite instance


h_mode4 = sp.h_mode4          # the shortest horizon at which the dispatcher takes the two-wave team without staging rows (MODE 4)


# ---- pools ------------------------------------------------------------------------------------------------------------------------------------
# What is done to instance i of asymmetric_problem(cfg, K, seed) (SPEC.md §8 defines the handling of each; none of them is an invalid input):
#   healthy        nothing
#   tiny_step      stepsize_in = (1 + i) 1e-30: xn == yk, the tolerance test ends the solve after one iteration
#   step_1, step_100   stepsize_in = 1 + i / 64, 100 + i: the line search shrinks it (or exhausts)
#   x0_huge        x0[10:13] *= 1e30: the rollout overflows; guard at k = 0, non-finite outputs
#   nan_noise      NaN noise on one particle: guard at k = 0, non-finite outputs
#   nan_x0         x0 all NaN
#   inf_xref       xref[4, 0] = inf: infinite cost, guard at k = 0, while the trajectory stays finite
#   u_low          u_init at every motor's lower bound
#   u_opt          u_init = the oracle's own uopt (f32 / exact) of the untouched instance: a solve that starts where one ended
@dataclasses.dataclass(frozen=True)
class Pool:
    base: str                    # the case of tests/solve_paths.py whose settings the pool copies
    H: int
    max_iter: int
    seed: int
    kinds: tuple                 # one entry per instance
    cfg: tuple = ()              # further overrides, ((name, value), ...)

    @property
    def K(self):
        return len(self.kinds)


# Every other instance keeps stepsize_in = (1 + i / 64) x the base case's. The kinds were placed with the oracle until each pool met the conditions
# that tests/test_mixed_batch_cpu.py asserts (under guard_kgt0_p80's settings an untouched instance meets the guard after one or two iterations and
# stepsize_in near 1 is what runs to max_iter; max_no_improvement_iter = 4 gives the copies of mix_p80's settings their fourth way to end).
_H = "healthy"
POOLS = {
    "mix": Pool("mix_p80", 10, 12, 31, (_H, "tiny_step", _H, "x0_huge", _H, "u_low", "nan_noise", _H, "inf_xref", _H, "step_100", "u_opt",
                                        _H, "nan_x0", "tiny_step", _H, "step_1", _H, "x0_huge", _H, "u_opt", _H, "step_1", _H), (("max_no_improvement_iter", 4),)),
    "guard": Pool("guard_kgt0_p80", 6, 6, 32, ("step_1", "step_1", "tiny_step", "step_1", "x0_huge", "step_1", _H, "step_100", "inf_xref", "step_1", "u_low", "step_1",
                                               "nan_noise", "step_1", "step_1", "u_opt", "step_1", "step_1", "tiny_step", "nan_x0", "step_1", _H, "step_1", "step_1")),
    "mode4": Pool("mix_p80", 0, 6, 33, (_H, "tiny_step", _H, "x0_huge", _H, "inf_xref", "u_low", _H, "nan_noise", "step_100", _H, "u_opt"),
                  (("max_no_improvement_iter", 4),)),     # H: h_mode4(m)
}


def pool_cfg(pool, P, m=4, **kw):
    p = POOLS[pool]
    H = p.H or h_mode4(m)
    base = dict(sp.CASES[p.base].cfg)
    base.update(sp._shape(H, P, p.max_iter), **dict(p.cfg))
    if H > 20:
        base.update(short_step_dt=0.01, long_step_dt=0.02)          # (the long horizon spans seconds, as the short ones do: kernel_census.Row.cfg_kw)
    return asymmetric_cfg(m, **{**base, **kw})


@functools.lru_cache(maxsize=None)
def problem(pool, P, m=4):
    """(cfg, model, x0, xref, noise, u_init, stepsize_in) of the K instances of a pool with P particles and m motors; read-only arrays."""
    p = POOLS[pool]
    cfg, model, K = pool_cfg(pool, P, m), asymmetric_model(m), p.K
    x0, xref, noise, u = asymmetric_problem(cfg, K, p.seed)
    x0, xref, noise, u = x0.copy(), xref.copy(), noise.copy(), u.copy()
    s = (np.float32(sp.CASES[p.base].s_in) * (1 + np.arange(K, dtype=np.float32) / 64)).astype(np.float32)      # every instance its own step size
    lo = np.asarray(cfg.input_bound, np.float32)[:, 0]
    opt = [i for i, k in enumerate(p.kinds) if k == "u_opt"]
    if opt:
        O = orc.Oracle(cfg, model)
        orc.set_threads(min(os.cpu_count() or 1, 8))
        try:
            for i in opt:
                u[i] = O.solve(x0[i], xref[i], noise[i], u[i], float(s[i]))[0]
        finally:
            orc.set_threads(1)
    for i, k in enumerate(p.kinds):
        if k == "tiny_step":
            s[i] = 1e-30 * (1 + i)
        elif k == "step_1":
            s[i] = 1.0 + i / 64
        elif k == "step_100":
            s[i] = 100.0 + i
        elif k == "x0_huge":
            x0[i, 10:13] *= np.float32(1e30)
        elif k == "nan_noise":
            noise[i, i % P] = np.nan
        elif k == "nan_x0":
            x0[i] = np.nan
        elif k == "inf_xref":
            xref[i, 4, 0] = np.inf
        elif k == "u_low":
            u[i] = lo
        else:
            assert k in (_H, "u_opt"), k
    for a in (x0, xref, noise, u, s):
        a.setflags(write=False)
    return cfg, model, x0, xref, noise, u, s


@functools.lru_cache(maxsize=None)
def reference(pool, P, m=4, math_mode="exact", mlp_dtype="f32"):
    """Oracle results of the pool's instances in one arithmetic, computed once: [(uopt, xevol, info, solve_paths.Record)]."""
    cfg, model, x0, xref, noise, u, s = problem(pool, P, m)
    cfg = cfg.replace(math_mode=math_mode, mlp_dtype=mlp_dtype)
    O = orc.Oracle(cfg, model)
    orc.set_threads(min(os.cpu_count() or 1, 8))
    try:
        out = []
        for i in range(POOLS[pool].K):
            uo, xe, io, ev = O.solve_events(x0[i], xref[i], noise[i], u[i], float(s[i]))
            for a in (uo, xe, io, ev):
                a.setflags(write=False)
            out.append((uo, xe, io, sp.Record(cfg, ev)))
    finally:
        orc.set_threads(1)
    return out


def ending(ref_i):
    """How instance `ref_i` (an entry of reference()) ended, from the oracle's record alone: 'k0_nonfinite' / 'k0_finite' (guard at k = 0, by whether
    xevol is finite), 'kgt0' (guard later), 'tol1' (tolerance stop after one iteration), 'full' (max_iter iterations, every output finite), else
    the cause's name."""
    uo, xe, io, rec = ref_i
    n, cause = int(io[2]) if np.isfinite(io[2]) else len(rec.ev), int(rec.col("cause")[-1]) if len(rec.ev) else 0
    if cause == 4:
        return "kgt0" if len(rec.ev) > 1 else ("k0_finite" if np.isfinite(xe).all() else "k0_nonfinite")
    if n == rec.cfg.max_iter and all(np.isfinite(a).all() for a in (uo, xe, io)):
        return "full"
    if cause == 2 and n == 1:
        return "tol1"
    return sp.CAUSES.get(cause, "none")


def endings(pool, P, m=4, math_mode="exact", mlp_dtype="f32"):
    return [ending(r) for r in reference(pool, P, m, math_mode, mlp_dtype)]


# ---- arrangement ------------------------------------------------------------------------------------------------------------------------------
def order(B, K, seed=2024):
    """idx[b]: the pool instance at position b, a fixed pseudo-random sequence (not b % K: a stride of the grid that divides K would hand a team
    the same instance every round)."""
    return np.random.default_rng(seed).integers(0, K, B)


def batch(pool, P, B, m=4):
    cfg, model, x0, xref, noise, u, s = problem(pool, P, m)
    idx = order(B, POOLS[pool].K)
    return cfg, model, x0[idx], xref[idx], noise[idx], u[idx], s[idx], idx


WAVES = {"TeamPairT<2>": (4, 2), "TeamPairT<6>": (12, 6), "TeamBlock2": (2, 1), "TeamBlock": (4, 1)}      # team shape -> (waves, teams) per workgroup


def kernel_name(team, m, mlp, mode=3, ustg=False):
    return f"sdempc_solve_kernel<{team}, {m}, {MODE[mlp]}, false, {mode}, {'true' if ustg else 'false'}>"


def team_slots(kernel, H, m, cus):
    """Teams of a persistent launch of `kernel` (a normalised name) that fills the device: launch_persistent's grid,
    min(12 / waves, 156 KiB / smem_bytes) workgroups per CU x CUs x teams per workgroup; the LDS arithmetic is tests/kernel_census.py's."""
    team = next(t for t in ("TeamPairT<2>", "TeamPairT<6>", "TeamBlock2", "TeamBlock") if f"<{t}," in kernel)
    mode, ustg = kernel.rstrip(">").split(", ")[-2:]
    waves, ipb = WAVES[team]
    sb = kc.smem_bytes(H, m, ipb, False, ustg == "false", waves if mode == "3" else 0)
    return max(1, min(12 // waves, kc.LDS_CAP // sb)) * cus * ipb


def ticketed(B, slots):
    return B >= 3 * slots


def team_sequences(B, slots):
    """Striped order: the positions team `slot` solves one after another."""
    return [list(range(slot, B, slots)) for slot in range(min(slots, B))]


def successions(idx, kinds, slots):
    """{(kind before, kind after)} over the consecutive solves of every team of a striped launch."""
    k = np.asarray(kinds)[np.asarray(idx)]
    return set(zip(k[:-slots].tolist(), k[slots:].tolist())) if len(k) > slots else set()


def required_successions(kinds):
    ab = [a for a in ABNORMAL if a in kinds]
    return {(a, "full") for a in ab} | {("full", a) for a in ab}


# ---- work counters ----------------------------------------------------------------------------------------------------------------------------
def expected_work(ref, idx):
    """(solves, gradient evaluations, forward-only rollouts) of the sequential loop over the positions `idx`, from the event records (the rule of
    tests/test_gpu_solve_paths.py: an iteration rejected from a plain step leaves yk where it was and the next one re-uses its gradient; two more
    rollouts per solve)."""
    per = []
    for uo, xe, io, rec in ref:
        stayed = rec.col("yk_stayed") == 1 if len(rec.ev) else np.zeros(0, bool)
        per.append((len(rec.ev) - int(stayed[:-1].sum()), int(io[7]) + 2))
    per = np.asarray(per, np.int64)[np.asarray(idx)]
    return len(idx), int(per[:, 0].sum()), int(per[:, 1].sum())


@functools.lru_cache(maxsize=None)
def settled_trials(pool, P, m=4):
    """Per pool instance, f32 / exact: the non-final line-search trials whose Armijo bound is negative (sdempc_work_counters out[3]), by the rule of
    tests/tools/armijo_census.py (census(): the NumPy restatement's optimiser on the oracle's cost and gradient, checked there against the oracle's
    solve bit for bit)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("armijo_census", os.path.join(sp.ROOT, "tests", "tools", "armijo_census.py"))
    ac = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ac)
    cfg, model, x0, xref, noise, u, s = problem(pool, P, m)
    orc.set_threads(min(os.cpu_count() or 1, 8))
    try:
        return tuple(ac.census(cfg, model, x0[i], xref[i], noise[i], u[i], float(s[i]))[2] for i in range(POOLS[pool].K))
    finally:
        orc.set_threads(1)


# ---- the launches of tests/test_gpu_mixed_batch.py --------------------------------------------------------------------------------------------
P2, P4 = 70, 130          # three particle groups (the last of six particles): two-wave teams; five groups (the last of two): the four-wave team
PAIR = dict(coop=0, pk=0, duo=1, hex=0)


@dataclasses.dataclass(frozen=True)
class Launch:
    pool: str
    P: int
    m: int
    team: str
    mode: int                    # MODE template argument
    ustg: bool
    how: str                     # "striped": B = 2 slots + 37; "ticketed": B = 3 slots + 91
    options: tuple
    mlp: str = "f32"
    math: str = "exact"

    @property
    def id(self):
        return f"{self.pool}-{self.team}-m{self.m}-mode{self.mode}{'g' if self.ustg else ''}-{self.how}-{self.mlp}-{self.math}"

    def H(self):
        return pool_cfg(self.pool, self.P, self.m).horizon

    def kernel(self):
        return kernel_name(self.team, self.m, self.mlp, self.mode, self.ustg)

    def slots(self, cus):
        return team_slots(self.kernel(), self.H(), self.m, cus)

    def B(self, cus):
        n = self.slots(cus)
        return 2 * n + 37 if self.how == "striped" else 3 * n + 91


def _launches():
    opt = lambda **kw: tuple(sorted(kw.items()))
    L = []
    for pool in ("mix", "guard"):
        for how in ("striped", "ticketed"):
            L.append(Launch(pool, P2, 4, "TeamPairT<2>", 3, False, how, opt(**PAIR)))
            L.append(Launch(pool, P2, 4, "TeamPairT<6>", 3, False, how, opt(coop=0, pk=0, duo=1)))
            L.append(Launch(pool, P4, 4, "TeamBlock", 3, False, how, opt(coop=0, pk=0)))
        L.append(Launch(pool, P2, 4, "TeamBlock2", 3, True, "striped", opt(coop=0, pk=0, duo=1, ustg=1)))
    L.append(Launch("mode4", P2, 4, "TeamBlock2", 4, True, "striped", opt(coop=0, pk=0, duo=1, hex=0)))
    L.append(Launch("mix", P2, 6, "TeamPairT<2>", 3, False, "ticketed", opt(**PAIR)))
    for pool in ("mix", "guard"):
        for mlp, math in (("f16", "exact"), ("f32x3", "fast")):
            L.append(Launch(pool, P2, 4, "TeamPairT<2>", 3, False, "ticketed", opt(**PAIR), mlp, math))
            L.append(Launch(pool, P4, 4, "TeamBlock", 3, False, "striped", opt(coop=0, pk=0), mlp, math))
        L.append(Launch(pool, P2, 4, "TeamPairT<2>", 3, False, "ticketed", opt(**PAIR), "f16", "fast"))
    return L


LAUNCHES = _launches()
