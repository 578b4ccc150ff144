"""Every kernel that only the all-variants build carries (tests/kernel_census.py: ALL_ROWS; csrc/allvariants/libsdempc.so, `make allvariants`), run
once on the GPU, and the two rows on the two sides of that build's packed-tanh threshold. This process keeps the default library: the second
library is loaded in ONE fresh child process per module (tests/census_all_child.py, SDEMPC_LIB pointing at it), which runs the rows one after
another as tests/test_gpu_kernel_census.py runs the default ones and stops at the first exception or non-zero status without starting another row.
Here, per row: the reported kernel name EQUAL to the row's, and uopt, xevol and the eight telemetry words against the CPU oracle bit for bit on the
row's sample of instances. A row that the child never reached fails and names the row at which the child stopped; a missing library fails."""
import os
import pickle
import subprocess
import sys
import time

import pytest

import kernel_census as kc
from cases import bits_differ

pytestmark = pytest.mark.gpu

CHILD = os.path.join(kc.ROOT, "tests", "census_all_child.py")
AV_LIB = os.path.join(kc.AV_DIR, "libsdempc.so")
CHILD_LIMIT_S = 8.4         # three times the 2.8 s the child took on an MI355X (measured twice: the module alone, and within the whole GPU suite)


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """{"problem": why nothing ran, or None; "cus"; "rows": {id: record}; "stopped": what ended the child early, or None}. Never raises: every
    row's test fails with the reason."""
    res = {"problem": None, "cus": None, "rows": {}, "stopped": None}
    if not os.path.exists(AV_LIB):
        res["problem"] = f"{AV_LIB} is missing: make -C sde4mbrl_px4_amd/csrc allvariants (build() makes it)"
        return res
    out = str(tmp_path_factory.mktemp("census_all") / "results.pkl")
    t0 = time.monotonic()
    try:
        r = subprocess.run([sys.executable, CHILD, out], env=dict(os.environ, SDEMPC_LIB=AV_LIB), timeout=CHILD_LIMIT_S, capture_output=True, text=True)
        rc, tail = r.returncode, (r.stdout[-1500:] + "\n" + r.stderr[-3000:])
    except subprocess.TimeoutExpired as e:
        rc, tail = f"none: killed at the limit of {CHILD_LIMIT_S} s (counts as hung)", str(e.stdout)[-1500:] + "\n" + str(e.stderr)[-3000:]
    print(f"child: {time.monotonic() - t0:.1f} s, exit status {rc}")
    records = []
    if os.path.exists(out):
        with open(out, "rb") as f:
            try:
                while True:
                    records.append(pickle.load(f))
            except (EOFError, pickle.UnpicklingError):
                pass
    for rec in records:
        if "cus" in rec:
            res["cus"] = rec["cus"]
        elif "stopped" in rec:
            res["stopped"] = f"the child stopped at row {rec['stopped']}: {rec['error']}"
        else:
            res["rows"][rec["id"]] = rec
    if rc != 0 and res["stopped"] is None:
        nxt = next((x.id for x in kc.ALL_ROWS if x.id not in res["rows"]), "(after the last row)")
        res["stopped"] = f"the child ended with exit status {rc} at row {nxt}"
    if res["stopped"]:
        res["stopped"] += "\n" + tail
    if res["cus"] is None:
        res["problem"] = f"the child ran no row (exit status {rc}):\n{tail}"
    return res


@pytest.mark.parametrize("row", kc.ALL_ROWS, ids=lambda r: r.id)
def test_kernel_of_the_row_runs_and_matches_the_oracle(row, child):
    assert child["problem"] is None, child["problem"]
    assert row.id in child["rows"], f"never reached: {child['stopped']}"
    rec, cus = child["rows"][row.id], child["cus"]
    assert kc.normalise(rec["name"]) == (row.kernel, row.mode), rec["name"]
    prob, ref = kc.reference(row, cus)
    assert sorted(ref) == row.sample(cus)
    for b, r in ref.items():
        diff = [bits_differ(got[b], w) for got, w in zip(rec["out"], r[:3])]
        assert diff == [0, 0, 0], (b, diff)
