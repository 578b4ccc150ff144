"""The cases of the predicted-outcome tests (SPEC.md §12c), shared by tests/test_outcome_cpu.py and tests/test_gpu_outcome.py.

Shapes: H = 6 with four motors, P = 1 (31 padded lanes), 31 / 32 / 33 (one lane short of a group, none padded, one past), 70 (three groups), 128 (the full
in-register sort), 130 (five groups: the slot wrap, g = 4 joins slot 0) and 300 (ten groups: more groups than the workgroup has halves); H = 7 with six motors,
P = 33 (seven rows: the last half of the workgroup idles beside a working one). B = 3 with distinct initial states; vehicles and configurations are the
asymmetric ones of tests/cases.py. The order statistics exist up to P = 128 (OUTCOME_RANK_MAX_P); above that the cases carry no ranks and the refusal is tested.

Thresholds come from the oracle's own tensor by the rule of tests/score_cases.py: the median over the particles of max dp, min c and max w2 against the xref
window — over the particles of instance THRESHOLD_INSTANCE: the instances start far apart, so a median over all of them would separate instances, not
particles; this way every criterion fails in about half of that instance's particles and in all or none of the others'. reference() ASSERTS, for every case with P >= 31, that each of the three cause bits is
set in some particle and clear in another and that first_fail has at least two non-empty slots besides "never".

Targets: the xref window (default), and rows cut from a shifted window in the four shapes tgt_steps in {1, H+1} x tgt_batch in {1, B}.

Ranks as tests/band_cases.py: unsorted, with a duplicate, K = 6; K = 8 at P = 70 and K = 1 at P = 33.

Everything a test compares against is computed ONCE per case from the CPU oracle and cached for the process."""
import functools

import numpy as np

import cases as CS
import outcome_ref as OR
import tube_cases as TC
from sde4mbrl_px4_amd.solver import Score

B = 3
RANK_MAX_P = 128
THRESHOLD_INSTANCE = 0
#        name             H  m  P
SHAPES = (("h6_p1", 6, 4, 1), ("h6_p31", 6, 4, 31), ("h6_p32", 6, 4, 32), ("h6_p33", 6, 4, 33), ("h6_p70", 6, 4, 70), ("h6_p128", 6, 4, 128),
          ("h6_p130", 6, 4, 130), ("h6_p300", 6, 4, 300), ("h7_m6_p33", 7, 6, 33))
NAMES = tuple(s[0] for s in SHAPES)
BIG = ("h6_p70", "h6_p130")            # the cases the matrix-pipe / fast arithmetics run as well
TARGET_SHAPES = ((False, False), (False, True), (True, False), (True, True))       # (per step, per instance)


def shape(name):
    return SHAPES[NAMES.index(name)][1:]


def config(name, mlp_dtype="f32", math_mode="exact"):
    H, m, P = shape(name)
    return CS.asymmetric_cfg(m, horizon=H, num_short_dt=H, num_particles=P, mlp_dtype=mlp_dtype, math_mode=math_mode), CS.asymmetric_model(m)


def problem(name):
    """(x0, u, xref, noise) of the case: B instances with distinct initial states"""
    cfg, _ = config(name)
    x0, xref, noise, u = CS.asymmetric_problem(cfg, B, seed=23 + NAMES.index(name))
    return x0, u, xref, noise


def ranks(name):
    """the ranks of the case, unsorted, with a duplicate; None above the particle limit of the order statistics"""
    P = shape(name)[2]
    if P > RANK_MAX_P:
        return None
    c = lambda r: min(P - 1, max(0, r))
    if name == "h6_p33":
        return [c(P // 2)]                                                        # K = 1
    base = [c(P - 1), 0, c(P // 2), c(1), c(P - 2), c(P // 2)]                    # K = 6
    if name == "h6_p70":
        base += [c(P // 4), c(3 * P // 4)]                                        # K = 8
    return base


def targets(xref, per_step=True, per_instance=True):
    """target rows f32[B or 1][H+1 or 1][13] that are NOT the xref window: each row of it shifted by a few centimetres and cm/s, differently per instance and
    step, so every (instance, step) row is distinct; a size-1 axis keeps step 2 / instance 1."""
    w = np.asarray(xref, np.float32).copy()                                        # [B][H+1][13]
    Bn, T1, _ = w.shape
    shift = 0.03 * (1 + np.arange(Bn))[:, None, None] * np.cos(np.arange(T1)[None, :, None] + np.arange(6)[None, None, :])
    w[:, :, :6] += shift.astype(np.float32)
    if not per_step:
        w = w[:, 2:3]
    if not per_instance:
        w = w[1:2]
    return np.ascontiguousarray(w)


def score_from(traj, xref):
    """A Score whose thresholds sit inside the tensor's own spread: the median over the particles of instance THRESHOLD_INSTANCE of max dp, min c and max w2
    over the rows t >= 1"""
    H = traj.shape[2] - 1
    b = slice(THRESHOLD_INSTANCE, THRESHOLD_INSTANCE + 1)
    with np.errstate(all="ignore"):
        ch, _ = OR.channels(traj[b, :, 1:], np.asarray(xref, np.float32)[b, 1:])
        r2, c, w2 = (float(np.nanmedian(np.asarray(v, np.float64))) for v in (ch[..., 0].max(axis=2), ch[..., 2].min(axis=2), ch[..., 3].max(axis=2)))
    assert H >= 1 and np.isfinite([r2, c, w2]).all()
    return Score(pos_radius=np.sqrt(r2), tilt_max=np.arccos(min(c, 1.0)), rate_max=np.sqrt(w2))


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _freeze(a)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, mlp_dtype="f32", math_mode="exact"):
    """-> dict: cfg, model, x0, u, xref, noise, cost, traj (the oracle's), score, thresholds, ranks, want (outcome_ref.outcome of the oracle's tensor against the
    xref window). Read-only."""
    cfg, model = config(name, mlp_dtype, math_mode)
    x0, u, xref, noise = problem(name)
    cost, traj, _ = TC.oracle_rollout(cfg, model, x0, u, xref, noise)
    score = score_from(traj, xref)
    rk = ranks(name)
    want = OR.outcome(traj, score.thresholds(), xref=xref, ranks=rk)
    P, H = cfg.num_particles, cfg.horizon
    if P >= 31:
        ever = (want["words"][..., 9].reshape(-1, 1) >> np.arange(3, dtype=np.uint32)) & 1
        assert ever.any(axis=0).all() and (~ever.astype(bool)).any(axis=0).all(), (name, "a cause bit is set in every particle or in none", ever.sum(axis=0))
        assert (want["first_fail"][:, :H].sum(axis=0) > 0).sum() >= 2, (name, "first failures fall into fewer than two rows", want["first_fail"])
    return _freeze(dict(cfg=cfg, model=model, x0=x0, u=u, xref=xref, noise=noise, cost=cost, traj=traj, score=score, thresholds=score.thresholds(),
                        ranks=None if rk is None else tuple(rk), want=want))


# ---- special values: they reach the device tensor through the caller's noise and x0 only ------------------------------------------------------------------
def special_problem(name):
    """The case's inputs with: particles 0 and 1 on identical noise rows (exact ties in every channel at every step); particles 2, 3, 4 on NaN noise (cause
    bit 8, NaN channel values beside finite ones); instance 1 with an all-NaN x0; instance 2 with a +inf position component. -> (x0, u, xref, noise)"""
    x0, u, xref, noise = problem(name)
    x0, noise = x0.copy(), noise.copy()
    assert noise.shape[1] >= 6
    noise[:, 1] = noise[:, 0]
    noise[:, 2:5] = np.nan
    x0[1, :] = np.nan
    x0[2, 0] = np.inf
    return x0, u, xref, noise


def synthetic_special(name):
    """For the CPU tests, which have no device tensor: the oracle's tensor of the case with the special values planted directly — particle 1 a copy of particle 0,
    particles 2 .. 4 NaN from t = 1 on, instance 1 all NaN, instance 2 with x = +inf from t = 1 on in particle 5 and in every particle's first component at t = 3.
    -> traj"""
    traj = reference(name)["traj"].copy()
    assert traj.shape[1] >= 8
    traj[:, 1] = traj[:, 0]
    traj[:, 2:5, 1:] = np.nan
    traj[1] = np.nan
    traj[2, 5, 1:, 0] = np.inf
    traj[2, :, 3, 0] = np.inf
    return traj
