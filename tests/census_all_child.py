"""Child process of tests/test_gpu_kernel_census_all.py: `python tests/census_all_child.py RESULTS`, started with SDEMPC_LIB naming the all-variants
build (csrc/allvariants/libsdempc.so), so that the pytest process itself keeps the default library. Runs the rows of kernel_census.ALL_ROWS one
after another as tests/test_gpu_kernel_census.py runs the default ones (handle options, call kind, reported kernel name, solve status, no layout
fallback) and appends one pickled record per row to RESULTS, flushed row by row: first {"cus": ...}, then {"id", "name", "out"} each. Nothing is
compared here: the parent holds the oracle. The first exception or non-zero status appends {"stopped": id, "error": ...} and ends the process with
status 1 before another row starts."""
import os
import pickle
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(results):
    import torch                                  # torch's HIP runtime comes up first, as in conftest.py
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    import numpy as np

    import kernel_census as kc
    from sde4mbrl_px4_amd import MPCConfig, _abi, synthetic_iris
    from sde4mbrl_px4_amd.solver import SdeMpcSolver

    assert _abi.load_library().sdempc_build_flags() & 1, f"{_abi.lib_path()} is not an all-variants build"
    with open(results, "wb") as f:
        def put(rec):
            pickle.dump(rec, f)
            f.flush()

        S = SdeMpcSolver(MPCConfig(horizon=2, num_short_dt=2), synthetic_iris(), max_batch=1)
        S.rollout(np.zeros((1, 13), np.float32), np.full((1, 2, 4), 0.5, np.float32), np.zeros((1, 3, 13), np.float32), np.zeros((1, 1, 2, 6), np.float32))
        cus = S.get_option("device_cus")          # (known once the handle has bound its device)
        S.close()
        assert cus >= 16
        put({"cus": cus})
        for row in kc.ALL_ROWS:
            t0 = time.monotonic()
            try:
                prob = kc.problem(row, cus)
                S = SdeMpcSolver(row.cfg(), row.model(), max_batch=row.B(cus), options=dict(row.options))
                if row.kind == "solve":
                    out = S.solve(prob["x0"], prob["xref"], prob["noise"], prob["u"], prob["s0"])
                else:
                    assert row.kind == "solve_keys", row.kind
                    out = S.solve_keys(prob["x0"], prob["xref"], prob["keys"], prob["u"], prob["s0"])
                name = S.last_kernel_name()
                S.solve_status()
                assert S.layout_fallbacks() == 0
                S.close()
            except BaseException as e:
                put({"stopped": row.id, "error": "".join(traceback.format_exception_only(type(e), e)).strip()})
                traceback.print_exc()
                return 1
            put({"id": row.id, "name": name, "out": tuple(np.asarray(o) for o in out)})
            print(f"{time.monotonic() - t0:6.2f} s  {row.id}  {name}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
