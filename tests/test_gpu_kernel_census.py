"""Every kernel of the default build that the library can name (tests/kernel_census.py: ROWS), run once on the GPU: the handle options and the call of
the row, the reported kernel name EQUAL to the row's, no layout fallback, a clean solve status, and every output against the CPU oracle bit for bit
on the row's sample of instances — uopt, xevol and the eight telemetry words of a solve; cost and gradient; cost, particle trajectories and mean.
The matrix-pipe contraction modes and `math_mode: fast` go through the oracle's instruction models. A row whose name differs on the device at hand
is a wrong row: re-derive it in the table."""
import numpy as np
import pytest

import kernel_census as kc
from cases import bits_differ
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_cus():
    from sde4mbrl_px4_amd import MPCConfig, synthetic_iris
    S = SdeMpcSolver(MPCConfig(horizon=2, num_short_dt=2), synthetic_iris(), max_batch=1)
    S.rollout(np.zeros((1, 13), np.float32), np.full((1, 2, 4), 0.5, np.float32), np.zeros((1, 3, 13), np.float32), np.zeros((1, 1, 2, 6), np.float32))
    cus = S.get_option("device_cus")          # (known once the handle has bound its device)
    S.close()
    assert cus >= 16
    return cus


@pytest.mark.parametrize("row", kc.ROWS, ids=lambda r: r.id)
def test_kernel_of_the_row_runs_and_matches_the_oracle(row, device_cus):
    prob, ref = kc.reference(row, device_cus)
    B = row.B(device_cus)
    S = SdeMpcSolver(row.cfg(), row.model(), max_batch=B, options=dict(row.options))
    x0, xref, u, noise = prob["x0"], prob["xref"], prob["u"], prob["noise"]
    if row.kind == "solve":
        out = S.solve(x0, xref, noise, u, prob["s0"])
    elif row.kind == "solve_keys":
        out = S.solve_keys(x0, xref, prob["keys"], u, prob["s0"])
    elif row.kind == "grad":
        out = S.grad(x0, u, xref, noise)
    else:
        out = S.rollout(x0, u, xref, noise, True, True)
    name = S.last_kernel_name()
    S.solve_status()
    assert S.layout_fallbacks() == 0
    S.close()
    assert kc.normalise(name) == (row.kernel, row.mode), name
    for b, r in ref.items():
        if row.kind in ("solve", "solve_keys"):
            want = r[:3]
        elif row.kind == "grad":
            want = (np.float32(r[0]), r[1].astype(np.float32))
        else:
            want = (np.float32(r[0]), r[1], r[2])
        diff = [bits_differ(got[b], w) for got, w in zip(out, want)]
        assert diff == [0] * len(want), (b, diff)
