"""The cases of the predicted-risk tests (SPEC.md §12a), shared by tests/test_risk_cpu.py and tests/test_gpu_risk.py.

Shapes, vehicles and problems are those of tests/tube_cases.py (H = 6 with P in {1, 31, 32, 33, 70, 130}, H = 7 with six motors and P = 33, B = 3): one lane
short of / past a group, no padding, three groups, and five groups, where the slot index g mod 4 wraps and — with eight halves per workgroup — one half still
takes a single group (more than eight groups, where a half walks two, is the P = 290 case of tests/test_gpu_risk.py).

A static absolute box is useless here: the vehicle moves much further over the horizon than its particles spread, so every particle leaves any box cut from the
tensor at t = 0. The box therefore sits on the DEVIATION from the oracle's mean trajectory, per instance: lo_i / hi_i are the 3 % / 97 % order statistics, over
particles and steps t >= 1, of x - xmean for the bounded components, so a particle sits exactly ON each bound (which is what tells >= from >).

Everything a test compares against is computed ONCE per case from the CPU oracle and cached for the process."""
import functools

import numpy as np

import risk_ref as RR
import tube_cases as TC
from sde4mbrl_px4_amd.solver import quantile_ranks, tail_count

B = TC.B
NAMES = TC.NAMES
BIG = TC.BIG
BOUNDED = TC.BOUNDED
QUANTILES = (0.0, 0.5, 0.9, 1.0)
TAIL = 0.1
ANCHOR = dict(res_mult=0.0, uerr=0.0, u_slew_coeff=0.0, u_slew_constr_coeff=0.0)      # the cost is then the particle mean of the tracking cost alone


def bounds_from(traj, centre):
    """-> lo, hi f32[B][13]: per instance the 3 % / 97 % order statistics of the deviation from `centre` over particles and steps t >= 1 (bounded components)"""
    nb = traj.shape[0]
    lo, hi = np.full((nb, 13), -np.inf, np.float32), np.full((nb, 13), np.inf, np.float32)
    for b in range(nb):
        dev = traj[b] - centre[b][None]                       # ONE float32 subtraction, as the reducer forms it
        for i in BOUNDED:
            v = np.sort(dev[:, 1:, i].reshape(-1))
            lo[b, i], hi[b, i] = v[int(np.floor(0.03 * (v.size - 1)))], v[int(np.ceil(0.97 * (v.size - 1)))]
    return lo, hi


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _freeze(a)
    return d


def _finish(d):
    """adds lo, hi (around the oracle's mean), ranks, tail_k and `want` = risk_ref.risk with centre = xmean"""
    P = d["cfg"].num_particles
    d["lo"], d["hi"] = bounds_from(d["traj"], d["xmean"])
    d["ranks"] = tuple(quantile_ranks(QUANTILES, P))
    d.setdefault("tail_k", tail_count(TAIL, P))
    d["want"] = want(d, d["xmean"])
    return _freeze(d)


def want(d, centre, lo="case", hi="case", cfg=None):
    """risk_ref.risk of the case's oracle tensor for another centre / box / cost configuration"""
    return RR.risk(d["traj"], cfg or d["cfg"], d["model"], d["xref"], d["lo"] if isinstance(lo, str) else lo, d["hi"] if isinstance(hi, str) else hi, centre,
                   d["ranks"], d["tail_k"])


@functools.lru_cache(maxsize=None)
def reference(name, mlp_dtype="f32", math_mode="exact"):
    """-> dict: tube_cases.reference(name) (cfg, model, x0, u, xref, noise, cost, traj, xmean of the oracle) with lo, hi f32[B][13], ranks, tail_k, want"""
    return _finish(dict(TC.reference(name, mlp_dtype, math_mode)))


def _rolled(cfg, model, x0, u, xref, noise):
    cost, traj, xmean = TC.oracle_rollout(cfg, model, x0, u, xref, noise)
    return dict(cfg=cfg, model=model, x0=x0, u=u, xref=xref, noise=noise, cost=cost, traj=traj, xmean=xmean)


TIED = (7, 20, 32)


@functools.lru_cache(maxsize=None)
def tie_case():
    """h6_p33 with the noise of particle 7 copied to particles 20 and 32 (32 is the only valid lane of the padded second group): three bit-identical trajectories
    and tracking costs. tail_k is chosen from the reference so that the tail cuts through the trio — which of the three are in it then changes the lanes the
    §6.1 sum finds its values in — and, among those, so that the restatement with ties broken by DESCENDING index differs in jtail (both are
    statements about the reference, none about the code under test)."""
    R = TC.reference("h6_p33")
    noise = R["noise"].copy()
    for p in TIED[1:]:
        noise[:, p] = noise[:, TIED[0]]
    d = _rolled(R["cfg"], R["model"], R["x0"], R["u"], R["xref"], noise)
    P = 33
    d["lo"], d["hi"] = bounds_from(d["traj"], d["xmean"])
    d["ranks"] = tuple(quantile_ranks(QUANTILES, P))
    cuts = []
    for k in range(1, P):
        d["tail_k"] = k
        w = want(d, d["xmean"])
        rank = np.argsort(np.argsort(w["jx"], axis=1, kind="stable"), axis=1, kind="stable")
        n_in = (rank[:, list(TIED)] >= P - k).sum(axis=1)
        if ((n_in > 0) & (n_in < 3)).any():
            m = RR.risk(d["traj"], d["cfg"], d["model"], d["xref"], d["lo"], d["hi"], d["xmean"], d["ranks"], k, mutant="ties_descending")
            cuts.append((k, RR.outputs_differ(w, m)))
    assert cuts, "no tail size cuts through the tied trio"
    d["cuts"] = tuple(cuts)
    d["tail_k"] = next((k for k, n in cuts if n), cuts[0][0])
    return _finish(d)


@functools.lru_cache(maxsize=None)
def state_constr_case():
    """h6_p33 with state_constr on the velocity components, its bounds the 30 % / 70 % order statistics of the oracle's own tensor (t >= 1): the tensor crosses
    them, so the penalty terms of §5.3 are live in jx. The dynamics do not see the cost: the tensor is the one of h6_p33."""
    R = TC.reference("h6_p33")
    sb = []
    for i in (3, 4, 5):
        v = np.sort(R["traj"][:, :, 1:, i].reshape(-1))
        sb.append([float(v[int(0.3 * (v.size - 1))]), float(v[int(0.7 * (v.size - 1))])])
    cfg = R["cfg"].replace(state_id=[3, 4, 5], state_penalty=[10.0, 15.0, 20.0], constr_pen=0.5, state_bound=sb)
    return _finish(_rolled(cfg, R["model"], R["x0"], R["u"], R["xref"], R["noise"]))


@functools.lru_cache(maxsize=None)
def anchor_case(name):
    """the case with every cost term but the tracking cost switched off: the oracle's rollout cost is then the particle mean of Jx"""
    R = TC.reference(name)
    return _finish(_rolled(R["cfg"].replace(**ANCHOR), R["model"], R["x0"], R["u"], R["xref"], R["noise"]))


@functools.lru_cache(maxsize=None)
def nonfinite_case(b=1):
    """h6_p33 with the initial state of instance b all NaN: every word of its tensor is NaN. Box, ranks and tail are those of h6_p33."""
    R = reference("h6_p33")
    x0, u, xref, noise = TC.nonfinite_variant("h6_p33", b)
    d = _rolled(R["cfg"], R["model"], x0, u, xref, noise)
    d.update(lo=R["lo"], hi=R["hi"], ranks=R["ranks"], tail_k=R["tail_k"])
    d["want"] = want(d, R["xmean"])               # (centre: the finite case's mean, so that the neighbours' words are those of the run without the NaNs)
    d["centre"] = R["xmean"]
    return _freeze(d)
