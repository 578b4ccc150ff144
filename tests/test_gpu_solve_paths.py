"""Every optimiser path in both solve kernels against the oracle, bit for bit: the cases of tests/solve_paths.py (whose coverage of the
named paths of SPEC.md §8 and of the speculative kernel's roles tests/test_solve_paths_cpu.py proves) through SdeMpcSolver.solve, in the
speculative state machine at 2..7 groups per instance and in the sequential loop of the cooperative, tile, duo and lane layouts."""
import functools

import numpy as np
import pytest

import kernel_census as kc
import solve_paths as sp
from cases import bits_differ
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu
MODE = {"f32": 0, "f16": 1, "f32x3": 2}


@functools.lru_cache(maxsize=None)
def device_cus():
    cfg, model, x0, xref, noise, u, s0, _ = sp.batch("max_iter_0_p20", 1)
    S = SdeMpcSolver(cfg, model, max_batch=1)
    S.solve(x0, xref, noise, u, s0)
    cus = S.get_option("device_cus")
    S.close()
    return cus


def _solve(name, B, math, mlp, options):
    """-> (kernel name, layout fallbacks, work counters) of one launch whose uopt, xevol and info equal the oracle's in every word."""
    cfg, model, x0, xref, noise, u, s0, idx = sp.batch(name, B)
    cfg = cfg.replace(math_mode=math, mlp_dtype=mlp)
    ref = sp.reference(name, math, mlp)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=options)
    S.work_counters(reset=True)
    uopt, xevol, info = S.solve(x0, xref, noise, u, s0)
    kname, fb, wc = S.last_kernel_name(), S.layout_fallbacks(), S.work_counters()
    S.close()
    for b in range(B):
        uo, xe, io, _ = ref[idx[b]]
        words = (bits_differ(uopt[b], uo), bits_differ(xevol[b], xe), bits_differ(info[b], io))
        assert words == (0, 0, 0), (name, b, words, info[b], io)
    assert kname.startswith(f"sdempc::{'exact' if math == 'exact' else 'fastm'}::"), kname
    return kname, fb, wc, idx


def test_device_reaches_two_to_seven_groups_per_instance():
    """The batches are chosen from the device's compute units so that the speculative kernel runs with exactly ng = 2..7 over this module."""
    cus = device_cus()
    confs = [c for c in sp.configurations(cus) if c[1] == "spec"]
    missing = sorted({(c[0], c[2]) for c in confs if c[3] is None})
    assert not missing, f"a device of {cus} compute units cannot run these (case, groups per instance) pairs in the speculative kernel: {missing}"
    for math in ("exact", "fast"):
        assert {c[2] for c in confs if c[4] == math} == set(sp.NGS), (cus, math)
    assert all(sp.spec_groups(sp.CASES[c[0]].P, c[3], cus) == c[2] for c in confs)


SPEC = [(n, ng, math) for n, c in sp.CASES.items() for math, ngs in (("exact", c.spec_ng), ("fast", c.fast_ng)) for ng in ngs]


@pytest.mark.parametrize("name,ng,math", SPEC, ids=[f"{n}-ng{g}-{mth}" for n, g, mth in SPEC])
def test_speculative_kernel(name, ng, math):
    """Auto layout. P = 1 (mscale_p1) is the DIRECT instantiation, hexa_p80 the six-motor one; tri_p20 (m = 3) runs the state machine where
    the build has the generic instantiation and the layout the default build gives it otherwise."""
    c, cus = sp.CASES[name], device_cus()
    B = sp.batch_for(ng, c.P, cus)
    if B is None:
        pytest.fail(f"{cus} compute units: no batch of {name} (P = {c.P}) runs with {ng} groups per instance")
    kname, fb, _, _ = _solve(name, B, math, "f32", {})
    assert fb == 0, fb
    if c.m in (4, 6) or "spec" in kname:
        assert f"sdempc_solve_spec_kernel<{c.m if c.m in (4, 6) else 8}, {'true' if c.P == 1 else 'false'}>" in kname, kname      # <motors, DIRECT>
    else:
        assert "sdempc_solve_kernel" in kname, kname


def _expected_work(name, idx, math="exact", mlp="f32"):
    """(solves, gradient evaluations, forward-only rollouts) of the sequential loop, from the event records: an iteration that was rejected
    from a plain step leaves yk where it was, and the next one re-uses its gradient; two more rollouts per solve (initial cost, final mean)."""
    ref = sp.reference(name, math, mlp)
    grads = fwd = 0
    for i in idx:
        io, rec = ref[i][2], ref[i][3]
        stayed = rec.col("yk_stayed") == 1 if len(rec.ev) else np.zeros(0, bool)
        grads += len(rec.ev) - int(stayed[:-1].sum())
        fwd += int(io[7]) + 2
    return len(idx), grads, fwd


SEQ = [(lay, n) for lay, (_, names) in sp.SEQUENTIAL.items() for n in names]


@pytest.mark.parametrize("layout,name", SEQ, ids=[f"{lay}-{n}" for lay, n in SEQ])
def test_sequential_loop(layout, name):
    """solve_instance in the plain cooperative, tile, duo and lane layouts, pinned by options and checked by kernel name; its work counters
    against the census (the re-used gradients are the kernel's own addition to SPEC.md §8)."""
    c = sp.CASES[name]
    kname, fb, wc, idx = _solve(name, sp.POOL, "exact", "f32", sp.SEQUENTIAL[layout][0])
    assert fb == 0 and "sdempc_solve_kernel" in kname and "spec" not in kname, kname
    mk = c.m if c.m in (4, 6) else 8
    if layout == "coop":
        assert f"TeamBlock, {mk}, 0, " in kname and ", 2, false>" in kname, kname
    elif layout == "duo":
        assert f"TeamPairT<2>, {mk}, 0, false, 3, false>" in kname, kname
    elif layout == "lane":
        assert f"TeamWave, {mk}, 0, false, 1," in kname, kname
    else:
        assert (f"TeamBlock, {mk}, 0, " if c.P > 32 else f"TeamWave, {mk}, 0, ") in kname and ", 2, false>" not in kname and ", false, 1," not in kname, kname
    assert wc == _expected_work(name, idx), (wc, _expected_work(name, idx))


DUO = [(lay, n) for lay, e in sp.DUO.items() for n in e[4]]


@pytest.mark.parametrize("layout,name", DUO, ids=[f"{lay}-{n}" for lay, n in DUO])
def test_sequential_loop_in_the_duo_kernels(layout, name):
    """solve_instance in the persistent duo kernels, one instantiation per team shape (two-wave teams in pairs; 128-thread workgroups with the
    control table in global memory, and without staging rows at the horizon that selects MODE 4; the four-wave team), pinned by options and
    checked by the reported kernel name; every output word against the oracle, the work counters against the census."""
    kname, fb, wc, idx = _solve(name, sp.POOL, "exact", "f32", sp.DUO[layout][0])
    assert fb == 0 and kc.normalise(kname) == (sp.duo_kernel(layout, name), "exact"), kname
    assert wc == _expected_work(name, idx), (wc, _expected_work(name, idx))


@pytest.mark.parametrize("name,mlp,math", sp.DUO_ARITH, ids=[f"{n}-{mlp}-{math}" for n, mlp, math in sp.DUO_ARITH])
def test_sequential_loop_in_the_pair_kernel_matrix_pipe_modes_and_fast_math(name, mlp, math):
    """A guard case and a case of mixed endings in TeamPairT<2> with the layer-2 contractions on the matrix pipe, and in math_mode fast."""
    kname, fb, wc, idx = _solve(name, sp.POOL, math, mlp, sp.DUO["pair"][0])
    assert fb == 0 and kc.normalise(kname) == (sp.duo_kernel("pair", name, mlp), "exact" if math == "exact" else "fast"), kname
    assert wc == _expected_work(name, idx, math, mlp), (wc, _expected_work(name, idx, math, mlp))


@pytest.mark.parametrize("name,mlp", sp.MATRIX_PIPE)
def test_sequential_loop_matrix_pipe_modes(name, mlp):
    """One case each with the layer-2 contractions on the matrix pipe (tile kernels: the cooperative layouts are f32 only)."""
    c = sp.CASES[name]
    kname, fb, wc, idx = _solve(name, sp.POOL, "exact", mlp, dict(lane=0, coop=0))
    assert fb == 0 and f"TeamBlock, {c.m}, {MODE[mlp]}, " in kname, kname
    assert wc == _expected_work(name, idx, "exact", mlp)
