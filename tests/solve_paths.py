"""The paths of the optimiser (SPEC.md §8), named; the census of a solve's event record; the cases that reach every one of them; and the
role model of the speculative kernel's state machine, which says where the gradient of the next iteration comes from.

The optimiser exists twice on the device (solve_instance in sdempc_kernels.hip; the state machine of sdempc_spec.inc.h) and which branch an
iteration takes depends on the data. tests/test_solve_paths_cpu.py proves, with the oracle's event record (orc.Oracle.solve_events), that the
cases below reach every named path and every reachable cell of {gradient source} x {groups per instance}, and that ten one-line-wrong
optimisers each change a compared bit on them; tests/test_gpu_solve_paths.py runs the same cases through the kernels, bit for bit.
Nothing in this file supplies an expected value: expected values are the oracle's.
"""
import dataclasses
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":      # (run as a script to rewrite tests/SOLVE_PATHS.md: the package lies one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kernel_census as kc
import orc
from cases import asymmetric_cfg, asymmetric_model, asymmetric_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX_MD = os.path.join(ROOT, "tests", "SOLVE_PATHS.md")
F = {n: i for i, n in enumerate(orc.EVENT_FIELDS)}
CAUSES = {1: "end_max_iter", 2: "end_tolerance", 3: "end_no_improvement", 4: "end_nonfinite_guard"}


@dataclasses.dataclass(frozen=True)
class Record:
    """The event record of one solve: ev float32 [n][len(orc.EVENT_FIELDS)] (one row per iteration; the non-finite guard's row included)."""
    cfg: object
    ev: np.ndarray

    def col(self, name):
        return self.ev[:, F[name]]


# ---- path names ---------------------------------------------------------------------------------------------------------------------------
# name -> predicate on (row r of the record as a dict of floats, the next row or None, cfg). The same list stands in SPEC.md §8.
def _ls_end(j, accepted):
    return lambda r, nx, c: r["cause"] != 4 and (r["nls"] == j if j < 5 else r["nls"] >= 5) and r["accepted"] == accepted


ITERATION_PATHS = {}
for _j, _n in ((1, "1"), (2, "2"), (3, "3"), (4, "4"), (5, "5plus")):
    ITERATION_PATHS[f"ls_end_{_n}_accepted"] = _ls_end(_j, 1)
    ITERATION_PATHS[f"ls_end_{_n}_rejected"] = _ls_end(_j, 0)
_ran = lambda r: r["cause"] != 4
ITERATION_PATHS.update({
    "ls_armijo_held_accepted": lambda r, nx, c: _ran(r) and r["armijo"] == 1 and r["accepted"] == 1,
    "ls_armijo_held_rejected": lambda r, nx, c: _ran(r) and r["armijo"] == 1 and r["accepted"] == 0,      # c_n <= Armijo bound of c_y, yet c_n >= c_x
    "ls_exhausted_accepted": lambda r, nx, c: _ran(r) and r["armijo"] == 0 and r["accepted"] == 1,
    "ls_exhausted_rejected": lambda r, nx, c: _ran(r) and r["armijo"] == 0 and r["accepted"] == 0,
    "maxls_0": lambda r, nx, c: _ran(r) and c.ls_maxls == 0,
    "maxls_1": lambda r, nx, c: _ran(r) and c.ls_maxls == 1,
    "maxls_2": lambda r, nx, c: _ran(r) and c.ls_maxls == 2,
    "maxls_3": lambda r, nx, c: _ran(r) and c.ls_maxls == 3,
    "maxls_ge4": lambda r, nx, c: _ran(r) and c.ls_maxls >= 4,
    "restart": lambda r, nx, c: _ran(r) and r["accepted"] == 1 and r["restart"] == 1,
    "momentum": lambda r, nx, c: _ran(r) and r["accepted"] == 1 and r["restart"] == 0,
    "momentum_yk_clamped": lambda r, nx, c: _ran(r) and r["accepted"] == 1 and r["restart"] == 0 and r["yk_clamped"] > 0,
    "rejected_from_plain": lambda r, nx, c: _ran(r) and r["accepted"] == 0 and r["plain"] == 1,             # yk stays: the kernels re-use (c_y, g, |g|^2)
    "rejected_from_momentum": lambda r, nx, c: _ran(r) and r["accepted"] == 0 and r["plain"] == 0 and r["stop_suppressed"] == 0,
    "rejected_from_momentum_stop_suppressed": lambda r, nx, c: _ran(r) and r["accepted"] == 0 and r["plain"] == 0 and r["stop_suppressed"] == 1,
    "step_cap_after_increase": lambda r, nx, c: _ran(r) and r["increased"] == 1 and r["capped"] == 1,
    "conservative_carries_shrunk_step": lambda r, nx, c: (_ran(r) and c.ls_reset_option == "conservative" and c.ls_maxls > 0 and r["s"] < r["s0"]
                                                          and nx is not None and nx["cause"] != 4 and nx["s0"] == r["s"]),
    "end_max_iter": lambda r, nx, c: r["cause"] == 1,
    "end_tolerance": lambda r, nx, c: r["cause"] == 2,
    "end_no_improvement": lambda r, nx, c: r["cause"] == 3,
    "end_nonfinite_guard": lambda r, nx, c: r["cause"] == 4,
    "guard_at_k0": lambda r, nx, c: r["cause"] == 4 and r["k"] == 0,
    "guard_at_k_gt0": lambda r, nx, c: r["cause"] == 4 and r["k"] > 0,
    "moment_scale_kr_ge1": lambda r, nx, c: _ran(r) and c.moment_scale is not None and r["accepted"] == 1 and r["restart"] == 0 and r["kr"] >= 1,
})
SOLVE_PATHS = {"max_iter_0": lambda rec: rec.cfg.max_iter == 0 and len(rec.ev) == 0}
PATH_NAMES = tuple(ITERATION_PATHS) + tuple(SOLVE_PATHS)

def rows(rec):
    out = [dict(zip(orc.EVENT_FIELDS, map(float, r)), k=k) for k, r in enumerate(rec.ev)]
    return out


def census(records):
    """The set of path names that the solve(s) behind `records` (one Record or several) reached."""
    if isinstance(records, Record):
        records = [records]
    seen = set()
    for rec in records:
        rr = rows(rec)
        for i, r in enumerate(rr):
            nx = rr[i + 1] if i + 1 < len(rr) else None
            seen.update(n for n, f in ITERATION_PATHS.items() if f(r, nx, rec.cfg))
        seen.update(n for n, f in SOLVE_PATHS.items() if f(rec))
    return seen


# ---- the role model of the state machine (sdempc_spec.inc.h, header comment and the comment on a.coop_ngrp) ------------------------------
# `ng` groups of workgroups per instance take the roles T1, T2, S(y2), S(xk), S(y1), T3, S(y3) in this order: T_j evaluates trial j of the line
# search, S(p) the gradient at the point p the optimiser may move to (y_j: where it goes when the search ends on trial j with an improvement;
# xk: no improvement). With one trial per iteration (maxls <= 1) the group of S(y2) evaluates S(y1). Trials beyond the side-by-side ones run
# one at a time; an iteration accepted on such a trial moves to a point nobody evaluated.
SOURCES = ("y1", "y2", "y3", "xk", "recompute_sequential", "recompute_absent")
NGS = (2, 3, 4, 5, 6, 7)


def spec_groups(P, B, cus):
    """Groups per instance the speculative kernel runs a batch of B with (launch_solve_spec): min(7, CUs / (B ceil(P / 4))); 0: not that kernel."""
    nwg = (P + 3) // 4
    return min(7, cus // (B * nwg)) if B <= cus // (2 * nwg) else 0


def batch_for(ng, P, cus, cap=64):
    """A batch that the speculative kernel runs with `ng` groups per instance on `cus` compute units: the largest one that does not repeat an
    instance of the pool, else the smallest; None when no batch up to `cap` gives that count."""
    fit = [B for B in range(1, cap + 1) if spec_groups(P, B, cus) == ng]
    return max([B for B in fit if B <= POOL], default=fit[0]) if fit else None


def trial_shape(ng, maxls):
    """'one', 'two' or 'three': how many trials of an iteration run side by side."""
    return "three" if ng >= 6 and maxls > 2 else "two" if maxls > 1 else "one"


def next_gradient_source(ng, maxls, r):
    """Where the state machine takes (c_y, g) of the iteration after the one with record row `r` from: one of SOURCES, or None when the solve
    ends with `r` (no next iteration; the speculation is switched off in the last iteration of max_iter as well)."""
    if r["cause"] != 0:
        return None
    side = {"one": 1, "two": 2, "three": 3}[trial_shape(ng, maxls)]
    if not r["accepted"]:
        return "xk" if ng >= 4 else "recompute_absent"
    j = int(r["nls"])
    if j > side:
        return "recompute_sequential"
    if j == 1:
        return "y1" if ng >= 5 or (ng >= 3 and side == 1) else "recompute_absent"
    if j == 2:
        return "y2" if ng >= 3 else "recompute_absent"
    return "y3" if ng >= 7 else "recompute_absent"


# The cells of SOURCES x NGS that the role order allows (every other one is empty by construction, not by omission):
#   y1 needs S(y1): ng >= 5, or the group of S(y2) when there is one trial only (ng >= 3 and maxls <= 1);
#   y2 needs S(y2): ng >= 3;   y3 needs T3 and S(y3): ng = 7;   xk needs S(xk): ng >= 4;
#   an accepted sequential trial exists at every ng (trial 3 up to ng = 5, trial 4 from ng = 6);
#   a missing role: ng = 2 (all), 3 (y1 of a two-trial iteration, xk), 4 (y1 of a two-trial iteration), 6 (y3); at ng = 5 and 7 every point
#   that a side-by-side trial or a rejection leads to has its group.
REACHABLE_CELLS = frozenset(
    [("y1", g) for g in (3, 4, 5, 6, 7)] + [("y2", g) for g in (3, 4, 5, 6, 7)] + [("y3", 7)] + [("xk", g) for g in (4, 5, 6, 7)]
    + [("recompute_sequential", g) for g in NGS] + [("recompute_absent", g) for g in (2, 3, 4, 6)])


def cells(ng, rec):
    """{(source, ng)} and the trial shapes that the solve with Record `rec` visits in the speculative kernel at `ng` groups per instance."""
    rr = rows(rec)
    src = {(next_gradient_source(ng, rec.cfg.ls_maxls, r), ng) for r in rr} - {(None, ng)}
    shapes = {trial_shape(ng, rec.cfg.ls_maxls) for r in rr if r["cause"] != 4}
    return src, shapes


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
POOL = 6          # instances per case; a batch of B takes instance b % POOL at position b


@dataclasses.dataclass(frozen=True)
class Case:
    m: int
    cfg: dict                    # overrides of asymmetric_cfg(m)
    seed: int
    declares: tuple              # the path names this case is there for
    spec_ng: tuple = ()          # groups per instance it runs the speculative kernel with (the batch follows from the device: batch_for)
    fast_ng: tuple = ()          # those of spec_ng that run in math_mode fast as well
    s_in: float = 0.01
    warm: str = "spikes"         # "spikes": asymmetric_problem's warm start; "flat": uref; "low": every motor at its lower bound
    x0_scale: tuple = ()         # (first state index, count, factor) applied to x0: the guard cases

    def config(self, **kw):
        return asymmetric_cfg(self.m, **{**self.cfg, **kw})

    @property
    def P(self):
        return self.cfg["num_particles"]


def _shape(H, P, it, **kw):
    return {**dict(horizon=H, num_short_dt=(H + 1) // 2, long_step_dt=0.1, num_particles=P, max_iter=it, max_no_improvement_iter=it), **kw}


# Found on the CPU with the oracle (the settings were turned until the union of the censuses was the whole list and every mutant of
# orc.MUTANTS showed). Twelve iterations at most, H <= 12, P in {1, 20, 80, 100}.
CASES = {
    "mix_p80": Case(4, _shape(10, 80, 12), 3, ("ls_end_1_rejected", "ls_end_2_accepted", "ls_end_3_accepted", "ls_end_4_accepted", "ls_end_4_rejected", "maxls_ge4", "momentum",
                                               "momentum_yk_clamped", "rejected_from_plain", "rejected_from_momentum", "end_max_iter", "ls_exhausted_rejected"),
                    spec_ng=(7, 6, 4, 3, 2), fast_ng=(7, 6, 4, 3, 2)),
    "mix_p100": Case(4, _shape(9, 100, 10), 4, ("ls_end_1_accepted", "ls_end_2_rejected", "ls_exhausted_accepted", "ls_armijo_held_accepted", "ls_armijo_held_rejected",
                                                "rejected_from_momentum_stop_suppressed", "end_tolerance"), spec_ng=(7, 5, 3, 2), fast_ng=(5,)),
    "maxls1_p80": Case(4, _shape(8, 80, 10, ls_maxls=1), 5, ("maxls_1", "end_no_improvement", "ls_end_1_accepted", "ls_end_1_rejected"), spec_ng=(7, 4, 3, 2), fast_ng=(4, 3)),
    "maxls2_p20": Case(4, _shape(8, 20, 10, ls_maxls=2), 6, ("maxls_2", "ls_end_2_accepted", "ls_end_2_rejected", "ls_exhausted_accepted"), spec_ng=(7, 6)),
    "maxls3_p80": Case(4, _shape(8, 80, 10, ls_maxls=3, ls_decrease_factor=0.5), 7, ("maxls_3", "ls_end_3_accepted", "ls_end_3_rejected"), spec_ng=(7, 6, 4, 2), fast_ng=(6,)),
    "maxls6_p20": Case(4, _shape(8, 20, 10, ls_maxls=6, ls_decrease_factor=0.6), 8, ("ls_end_5plus_accepted", "ls_end_5plus_rejected"), spec_ng=(7, 6, 5), fast_ng=(7, 5), s_in=0.05),
    "maxls0_p80": Case(4, _shape(8, 80, 10, ls_maxls=0, stepsize=2e-3), 9, ("maxls_0", "ls_end_1_accepted", "ls_end_1_rejected"), spec_ng=(4, 3)),
    "conservative_p20": Case(4, _shape(8, 20, 10, ls_reset_option="conservative"), 10, ("conservative_carries_shrunk_step",), spec_ng=(7,), s_in=0.03),
    "cap_p80": Case(4, _shape(8, 80, 8, ls_max_stepsize=0.004, ls_increase_factor=1.5), 11, ("step_cap_after_increase",), spec_ng=(6,), s_in=0.004),
    "noimp2_p20": Case(4, _shape(10, 20, 12, max_no_improvement_iter=2), 12, ("end_max_iter", "rejected_from_plain", "rejected_from_momentum"), spec_ng=(7,), s_in=0.004),
    # ^ max_no_improvement_iter = 2 with rejections that an acceptance separates: noimp is cleared in between and the solve runs on to max_iter;
    #   the case is there for the mutant noimp_not_cleared, which ends it early
    "band_p20": Case(4, _shape(10, 20, 12, rtol=3e-3), 13, ("end_tolerance", "rejected_from_momentum"), spec_ng=(7,)),
    "restart_p80": Case(4, _shape(8, 80, 12, beta_init=6.0, ls_coef=0.5), 21, ("restart", "momentum"), spec_ng=(6, 3), fast_ng=(6,), s_in=0.002),
    "mscale_p1": Case(4, _shape(12, 1, 12, moment_scale=0.6), 14, ("moment_scale_kr_ge1",), spec_ng=(7, 5)),
    "hexa_p80": Case(6, _shape(7, 80, 8), 15, ("momentum", "rejected_from_momentum_stop_suppressed"), spec_ng=(7, 4), fast_ng=(4,)),
    "tri_p20": Case(3, _shape(7, 20, 8), 16, ("momentum", "ls_end_4_accepted"), spec_ng=(7,)),
    "tiny_step_p20": Case(4, _shape(6, 20, 6), 17, ("ls_armijo_held_rejected", "end_tolerance"), spec_ng=(7,), s_in=1e-30),      # xn == yk: the Armijo test holds with equality
    "max_iter_0_p20": Case(4, _shape(6, 20, 0, max_no_improvement_iter=1), 18, ("max_iter_0",), spec_ng=(7,)),
    "guard_k0_p20": Case(4, _shape(6, 20, 4), 19, ("end_nonfinite_guard", "guard_at_k0"), spec_ng=(7,), x0_scale=(10, 3, 1e30)),
    # Without enforce_ubound the momentum point yk is not projected: beta_init = 1e3 throws it out of the finite region of the model after the
    # first accepted step, while xk, uopt and xevol stay finite. The guard then ends the solve at the head of iteration 1 (2 on the instance
    # whose first step is rejected), which in the state machine has just consumed a speculated gradient (y1, y2, xk -> y2) or recomputed it
    # (accepted on the sequential trial 4) while the other groups of the instance are speculating.
    "guard_kgt0_p80": Case(4, _shape(6, 80, 6, enforce_ubound=False, beta_init=1e3), 19, ("end_nonfinite_guard", "guard_at_k_gt0"),
                           spec_ng=(7, 6, 4, 3, 2), fast_ng=(7, 4, 2)),
    "guard_kgt0_maxls0_p20": Case(4, _shape(6, 20, 6, enforce_ubound=False, beta_init=1e3, ls_maxls=0, stepsize=1e-3), 19, ("guard_at_k_gt0", "maxls_0"), spec_ng=(7, 3)),
}
GUARD_CASES = ("guard_k0_p20", "guard_kgt0_p80", "guard_kgt0_maxls0_p20")


# ---- twins for the duo kernels --------------------------------------------------------------------------------------------------------------
# The duo layout needs two particle groups at least (P >= 33): two-wave teams up to four groups (TeamPairT<2>, TeamBlock2), the four-wave team
# beyond (TeamBlock). The cases above with P = 20 or P = 1 get a twin at P = 40 (two groups, the second of eight particles) with the same settings
# and seed; the four-wave team and the horizon at which the dispatcher drops the noise staging rows (MODE 4) get twins of six cases that together
# reach the paths listed in DUO_REQUIRED. Found with the oracle's census, as the table above was; `declares` is what each twin is there for.
def h_mode4(m=4):
    """The shortest horizon at which launch_duo_m takes the two-wave team without staging rows: the dispatcher's arithmetic, tests/kernel_census.py."""
    return kc.shortest_h(lambda H: not kc.pair_fits(H, m) and kc.duo_pick(H, m, 2) == 2)


def _twin(name, declares=None, P=None, H=None, it=None):
    c = CASES[name]
    d = dict(c.cfg)
    if P is not None:
        d["num_particles"] = P
    if H is not None:
        d.update(horizon=H, num_short_dt=(H + 1) // 2)
        if H > 20:
            d.update(short_step_dt=0.01, long_step_dt=0.02)          # (a long horizon spans seconds, as the short ones do: kernel_census.Row.cfg_kw)
    if it is not None:
        if d["max_no_improvement_iter"] == d["max_iter"]:
            d["max_no_improvement_iter"] = it
        d["max_iter"] = it
    return dataclasses.replace(c, cfg=d, declares=c.declares if declares is None else declares, spec_ng=(), fast_ng=())


P40_TWINS = ("maxls2_p20", "maxls6_p20", "conservative_p20", "noimp2_p20", "band_p20", "mscale_p1", "tiny_step_p20", "max_iter_0_p20", "guard_k0_p20",
             "guard_kgt0_maxls0_p20")          # (tri_p20, m = 3: the default build has no duo instantiation of the generic motor count)
_SIX = {  # base case -> what its twin declares at (P = 130, H as the base) and at (P = 70, H = h_mode4(), max_iter = 6)
    "mix_p80": (("momentum", "rejected_from_momentum", "rejected_from_plain", "ls_exhausted_rejected", "end_max_iter", "end_tolerance"),
                ("momentum", "rejected_from_momentum", "end_max_iter")),
    "restart_p80": (("restart", "momentum"), ("restart", "momentum")),
    "maxls1_p80": (("maxls_1", "end_no_improvement", "rejected_from_plain"), ("maxls_1", "end_no_improvement", "ls_exhausted_rejected", "rejected_from_plain")),
    "tiny_step_p20": (("end_tolerance", "ls_armijo_held_rejected"), ("end_tolerance", "rejected_from_plain")),
    "guard_k0_p20": (("end_nonfinite_guard", "guard_at_k0"), ("end_nonfinite_guard", "guard_at_k0")),
    "guard_kgt0_p80": (("end_nonfinite_guard", "guard_at_k_gt0"), ("end_nonfinite_guard", "guard_at_k_gt0")),
}
_stem = lambda n: n.rsplit("_p", 1)[0]
DUO_CASES = {f"{_stem(n)}_p40": _twin(n, P=40) for n in P40_TWINS}
DUO_CASES.update({f"{_stem(n)}_p130": _twin(n, d[0], P=130) for n, d in _SIX.items()})
DUO_CASES.update({f"{_stem(n)}_h4": _twin(n, d[1], P=70, H=h_mode4(), it=6) for n, d in _SIX.items()})
ALL_CASES = {**CASES, **DUO_CASES}
DUO_GUARD_CASES = tuple(n for n in DUO_CASES if n.startswith("guard_"))


@functools.lru_cache(maxsize=None)
def problem(name):
    """(cfg, model, x0, xref, noise, u_init, stepsize_in) of the POOL instances of case `name`."""
    c = ALL_CASES[name]
    cfg, model = c.config(), asymmetric_model(c.m)
    x0, xref, noise, u = asymmetric_problem(cfg, POOL, c.seed)
    lo = np.asarray(cfg.input_bound, np.float32)[:, 0]
    if c.warm == "flat":
        u = np.tile(np.asarray(cfg.uref, np.float32), (POOL, cfg.horizon, 1))
    elif c.warm == "low":
        u = np.tile(lo, (POOL, cfg.horizon, 1))
    if c.x0_scale:
        i, n, f = c.x0_scale
        x0 = x0.copy()
        x0[:, i:i + n] *= np.float32(f)
    for a in (x0, xref, noise, u):
        a.setflags(write=False)
    return cfg, model, x0, xref, noise, u, np.float32(c.s_in)


def batch(name, B):
    """The inputs of a batch of B instances of case `name` and, per position, the pool instance it is."""
    cfg, model, x0, xref, noise, u, s = problem(name)
    idx = np.arange(B) % POOL
    return cfg, model, x0[idx], xref[idx], noise[idx], u[idx], np.full(B, s, np.float32), idx


@functools.lru_cache(maxsize=None)
def reference(name, math_mode="exact", mlp_dtype="f32"):
    """Oracle results of the POOL instances of a case in one arithmetic, computed once: [(uopt, xevol, info, Record)]."""
    cfg, model, x0, xref, noise, u, s = problem(name)
    cfg = cfg.replace(math_mode=math_mode, mlp_dtype=mlp_dtype)
    O = orc.Oracle(cfg, model)
    orc.set_threads(min(os.cpu_count() or 1, 8))
    try:
        out = []
        for b in range(POOL):
            uo, xe, io, ev = O.solve_events(x0[b], xref[b], noise[b], u[b], float(s))
            out.append((uo, xe, io, Record(cfg, ev)))
    finally:
        orc.set_threads(1)
    return out


# ---- the configurations the GPU tests run, and what each of them covers -------------------------------------------------------------------
# the sequential loop (solve_instance), pinned by options: name -> (handle options, cases)
SEQUENTIAL = {
    "coop": (dict(spec=0), ("mix_p80", "mix_p100", "maxls1_p80", "maxls3_p80", "restart_p80", "hexa_p80", "guard_kgt0_p80")),
    "tile": (dict(lane=0, coop=0), tuple(CASES)),
    "duo": (dict(coop=0, pk=0, duo=1), ("mix_p80",)),
    "lane": (dict(coop=0), ("mscale_p1",)),
}
MATRIX_PIPE = (("mix_p80", "f16"), ("maxls3_p80", "f32x3"))          # one case each in the matrix-pipe contraction modes (tile kernels)

# the sequential loop in the persistent duo kernels (sdempc_solve_kernel<Team, M, F16, false, MODE, USTG>), one entry per team shape:
# name -> (handle options, Team, MODE, USTG, cases). Which shape a launch takes follows from the groups per instance, the horizon and the options
# (launch_duo, launch_duo_small, launch_duo_m); tests/test_solve_paths_cpu.py checks every (entry, case) against the dispatcher's arithmetic in
# tests/kernel_census.py, tests/test_gpu_solve_paths.py against the kernel name the launch reports.
_SIX_OF = lambda tag: tuple(f"{_stem(n)}_{tag}" for n in _SIX)
DUO = {
    "pair": (dict(coop=0, pk=0, duo=1), "TeamPairT<2>", 3, False,
             tuple(n for n, c in CASES.items() if 33 <= c.P <= 128 and c.m in (4, 6)) + tuple(f"{_stem(n)}_p40" for n in P40_TWINS)),
    "block2_ustg": (dict(coop=0, pk=0, duo=1, ustg=1), "TeamBlock2", 3, True,
                    ("mix_p80", "restart_p80", "maxls1_p80", "tiny_step_p40", "guard_k0_p40", "guard_kgt0_p80")),
    "block2_mode4": (dict(coop=0, pk=0, duo=1), "TeamBlock2", 4, True, _SIX_OF("h4")),
    "block_p130": (dict(coop=0, pk=0), "TeamBlock", 3, False, _SIX_OF("p130")),
}
# what each team shape other than the pair reaches at least (the pair's configurations reach every name of PATH_NAMES); a tuple: one of these
DUO_REQUIRED = ("momentum", ("rejected_from_momentum", "rejected_from_momentum_stop_suppressed"), "rejected_from_plain", "restart", "ls_exhausted_rejected",
                ("maxls_0", "maxls_1"), "end_tolerance", "end_no_improvement", "guard_at_k0", "guard_at_k_gt0")
# one guard case and one case of mixed endings per matrix-pipe mode and in math_mode fast, in the pair: (case, mlp_dtype, math_mode)
DUO_ARITH = tuple((n, mlp, math) for mlp, math in (("f16", "exact"), ("f32x3", "exact"), ("f32x3", "fast"), ("f16", "fast")) for n in ("guard_kgt0_p80", "mix_p100"))


def duo_kernel(layout, name, mlp="f32"):
    """The normalised name of the kernel that entry `layout` of DUO runs case `name` with."""
    _, team, mode, ustg, _ = DUO[layout]
    m = ALL_CASES[name].m
    return f"sdempc_solve_kernel<{team}, {m if m in (4, 6) else 8}, {kc.F16_OF[mlp]}, false, {mode}, {'true' if ustg else 'false'}>"


def configurations(cus=256):
    """[(case, kernel, ng or None, B, math_mode, mlp_dtype)] of tests/test_gpu_solve_paths.py on a device of `cus` compute units."""
    out = []
    for name, c in CASES.items():
        for math, ngs in (("exact", c.spec_ng), ("fast", c.fast_ng)):
            out += [(name, "spec", ng, batch_for(ng, c.P, cus), math, "f32") for ng in ngs]
    for lay, (_, names) in SEQUENTIAL.items():
        out += [(name, lay, None, POOL, "exact", "f32") for name in names]
    out += [(name, "tile", None, POOL, "exact", mlp) for name, mlp in MATRIX_PIPE]
    for lay, (_, _, _, _, names) in DUO.items():
        out += [(name, lay, None, POOL, "exact", "f32") for name in names]
    out += [(name, "pair", None, POOL, math, mlp) for name, mlp, math in DUO_ARITH]
    return out


def records_of(conf):
    name, kernel, ng, B, math, mlp = conf
    ref = reference(name, math, mlp)
    return [ref[i][3] for i in sorted(set(range(B if B < POOL else POOL)))]


def covered_cells(cus=256):
    """{(source, ng): [configuration]} and {trial shape: [configuration]} over the speculative-kernel configurations."""
    cc, shapes = {}, {}
    for conf in configurations(cus):
        if conf[1] != "spec" or conf[3] is None:
            continue
        for rec in records_of(conf):
            src, shp = cells(conf[2], rec)
            for cell in src:
                cc.setdefault(cell, [])
                if conf not in cc[cell]:
                    cc[cell].append(conf)
            for sh in shp:
                shapes.setdefault(sh, [])
                if conf not in shapes[sh]:
                    shapes[sh].append(conf)
    return cc, shapes


def matrix_markdown(cus=256):
    """The text of tests/SOLVE_PATHS.md: path x (case, kernel, ng, math mode) and gradient source x ng, as the oracle's event records give them."""
    L = ["# Optimiser paths reached by the solve-path cases", "",
         "Generated by `tests/solve_paths.py` (`python tests/solve_paths.py` rewrites it; `tests/test_solve_paths_cpu.py` fails when it is stale).",
         f"Computed on the CPU from the oracle's event records, for a device of {cus} compute units. A configuration is one launch of",
         "`tests/test_gpu_solve_paths.py`: case, kernel (`spec`: the speculative state machine with `ng` groups per instance; `coop`, `tile`, `duo`,",
         "`lane`: the sequential loop in that layout; `pair`, `block2_ustg`, `block2_mode4`, `block_p130`: the sequential loop in the persistent duo",
         "kernels, by team shape: `TeamPairT<2>`, `TeamBlock2` MODE 3 with the control table in global memory, `TeamBlock2` MODE 4, `TeamBlock` MODE 3),",
         "batch, math mode and contraction mode.", "", "## Paths", ""]
    L += [f"{i + 1}. `{n}`" for i, n in enumerate(PATH_NAMES)]
    L += ["", "## Path x configuration", "", "| case | kernel | ng | B | math | mlp | paths reached (numbers above) |", "|---|---|---|---|---|---|---|"]
    for conf in configurations(cus):
        seen = census(records_of(conf))
        L.append("| " + " | ".join(str("-" if v is None else v) for v in conf) + " | " + " ".join(str(i + 1) for i, n in enumerate(PATH_NAMES) if n in seen) + " |")
    L += ["", "## Configurations per path", ""]
    for n in PATH_NAMES:
        k = sum(n in census(records_of(conf)) for conf in configurations(cus))
        L.append(f"- `{n}`: {k}")
    cc, shapes = covered_cells(cus)
    L += ["", "## Source of the next gradient x groups per instance (speculative kernel)", "",
          "Cell: `case/math` of the configurations that reach it; `.`: the role order does not allow the cell (see `REACHABLE_CELLS`).", "",
          "| source | " + " | ".join(f"ng = {g}" for g in NGS) + " |", "|---|" + "---|" * len(NGS)]
    for src in SOURCES:
        L.append(f"| `{src}` | " + " | ".join((" ".join(sorted({f"{c[0]}/{c[4]}" for c in cc.get((src, g), [])})) or "MISSING") if (src, g) in REACHABLE_CELLS else "." for g in NGS) + " |")
    L += ["", "Trials side by side: " + "; ".join(f"`{sh}` in {len(v)} configurations" for sh, v in sorted(shapes.items())), ""]
    return "\n".join(L)


if __name__ == "__main__":
    with open(MATRIX_MD, "w") as f:
        f.write(matrix_markdown())
