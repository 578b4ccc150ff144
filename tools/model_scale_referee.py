#!/usr/bin/env python3
"""The referee of SPEC.md §10d away from the synthetic weight scale: gradient error of every arithmetic against float64 of the SAME model, on the cases of
tests/scale_cases.py (H = 8, P = 33, B = 2, CPU oracle only). Prints the table kept in profiles/model_scale_referee.txt.

    python tools/model_scale_referee.py [--more]        (--more: uniform k from -24 to 30 in f32x3/fast, the scan the band of §10e was chosen from)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import scale_cases as SC  # noqa: E402


def row(name, m=4):
    r = SC.referee(name, m=m)
    base = r["f32/exact"]
    M = SC.model_of(name, m)
    cells = []
    for mlp, mm in SC.ARITHS:
        if r[f"{mlp}/{mm}"] is None:
            cells.append(f"{'refused':^28s}")
            continue
        rms, worst = r[f"{mlp}/{mm}"]
        cells.append(f"{rms:9.2e} {worst:9.2e} {rms / base[0]:8.3g}")
    n = SC.row_exponents(M)
    return f"{name + (' m6' if m == 6 else ''):18s} | " + " | ".join(cells) + f" | n = {','.join(str(int(v)) for v in n)} eoff = {SC.eoff(M)} (as given: {SC.eoff(M, normalise=False)})"


def main():
    print("gradient error over the float64 gradient's largest entry: rms, worst entry, rms as a multiple of f32/exact's; asymmetric_model, asymmetric_cfg(H = 8, P = 33),")
    print("asymmetric_problem(cfg, 2, seed = 3); n: the row exponents of §10e's normalisation, eoff: §10e's scale offset of the normalised model")
    print(f"{'case':18s} | " + " | ".join(f"{mlp + '/' + mm:^28s}" for mlp, mm in SC.ARITHS))
    for name in SC.preserving_cases():
        print(row(name), flush=True)
    for k in (-14, 0, 12):
        print(row(f"k{k:+d}", m=6), flush=True)
    for name in SC.changing_cases():
        print(row(name), flush=True)
    for b in SC.F16_BRANCHES:
        print(row("f16_" + b), flush=True)
    if "--more" in sys.argv:
        print("\nuniform k, f32x3/fast only: rms as a multiple of f32/exact's (worst entry likewise)")
        M0 = SC.base_model()
        _, g64 = SC.oracle_grads(SC.config(33), M0, 2, double=True)
        b = SC.grad_error(SC.oracle_grads(SC.config(33), M0, 2)[1], g64)
        for k in list(range(-24, 9)) + [10, 12, 14, 15, 16, 18, 20, 24, 30]:
            M = SC.rescaled(M0, k)
            with np.errstate(all="ignore"):
                e = SC.grad_error(SC.oracle_grads(SC.config(33, "f32x3", "fast"), M, 2)[1], g64)
            print(f"k = {k:+3d}: {e[0] / b[0]:10.4g} ({e[1] / b[1]:10.4g})  eoff = {SC.eoff(M)} (as given: {SC.eoff(M, normalise=False)})", flush=True)


if __name__ == "__main__":
    main()
