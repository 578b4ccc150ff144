"""What the closed-loop GPU tests (tests/test_gpu_*_loop.py, tests/test_gpu_loop_entries.py) share: the arithmetics, the names of the values
SdeMpcSolver.closed_loop returns, the bit-for-bit comparison and the call of a CPU reference with closed_loop's keyword arguments."""
import numpy as np

from cases import bits_differ

ARITH = [(d, mth) for d in ("f32", "f16", "f32x3") for mth in ("exact", "fast")]
# the ten values of the rate call; the plain and plant calls return the first six, the timed and scenario calls the first seven
NAMES = ("xs", "us", "info", "u_next", "stepsize_next", "keys_next", "u_act_next", "ws", "rate_integ_next", "rate_tail_next")
REF_NAME = dict(plant="plants", plant_substeps="substeps", solve_period="S", solve_delay="D", motor_lag="alpha", plant_mlp_dtype="mlp_dtype",
                plant_math_mode="math_mode", plant_dt="dt")


def same(got, want, eps=None, names=NAMES):
    """got and want hold exactly the values `names` lists, equal in shape and in every bit (the keys as integers); eps: compare these episodes only."""
    assert len(got) == len(want) == len(names)
    for n, g, w in zip(names, got, want):
        if eps is not None:
            g, w = g[eps], w[eps]
        assert g.shape == w.shape, (n, g.shape, w.shape)
        if n == "keys_next":
            assert np.array_equal(g, w), n
        else:
            assert bits_differ(g, w) == 0, (n, bits_differ(g, w))


def ref(loop_ref, cfg, model, x0, xref, keys, T, episodes=None, **kw):
    """The reference loop_ref (scenario_loop_ref, rate_loop_ref) for the keyword arguments of SdeMpcSolver.closed_loop."""
    return loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T, episodes=episodes, **{"plants": None, **{REF_NAME.get(k, k): v for k, v in kw.items()}})
