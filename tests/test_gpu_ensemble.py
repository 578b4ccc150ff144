"""Per-row ensemble words formed on the GPU (SPEC.md §11m, sdempc_closed_loop_batch_ensemble): every word of every (row, cohort) against ensemble_ref
(tests/ensemble_ref.py) of the rows and score words the call ITSELF returned, and against ensemble_ref of the oracle-driven loop. A NaN word equals any NaN;
everything else compares bit for bit. Shapes of tests/ensemble_cases.py, the smallest at which this path can go wrong: H = 6, P = 32, m = 4, T = 4 with two
solves, n = 2; B = 1, 63, 64, 65, 255, 256, 257, 300 and 600 (a lone lane, the wave and block edges, a ragged last block, three blocks); G = 1 and 3 with an empty
cohort; E = 0, 3 and 16; both inclusion rules; a tick score and a substep score; an episode the loop itself drives non-finite. f32 / exact on every case,
f32x3 / fast and f16 / fast at B = 300. Then: outputs=False, two chunks, a continuation through score_in, the geometric controller, guard words around ens_out,
a poisoned handle, and every other output unchanged by ensemble=."""
import ctypes as C

import numpy as np
import pytest

import ensemble_cases as EC
import geo_cases
from cases import bits_differ
from ensemble_ref import BASE, ens_words_differ, ensemble_ref
from score_cases import targets
from score_loop_ref import score_rows, words_differ
from sde4mbrl_px4_amd import _abi
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, SdeMpcSolver, ensemble_summary

pytestmark = pytest.mark.gpu
U = np.uint32


def fly(S, c, T=EC.T4, **over):
    """closed_loop on a prepared case: (xs, us, info, u_next, stepsize_next, keys_next, u_act_next, score, ENSEMBLE WORDS, xsub)."""
    kw = dict(c["kw"], substep_states=True, score=c["score"], score_ref=c["g"], ensemble=c["ens"], cohort=c["cohort"])
    kw.update(over)
    return S.closed_loop(c["x0"], c["xref"], c["keys"], T, **kw)


def same_values(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, i
        elif g.dtype == SCORE_DTYPE:
            assert words_differ(g, w) == 0, i
        elif g.dtype == np.float32:
            assert g.shape == w.shape and bits_differ(g, w) == 0, (i, bits_differ(g, w))
        else:
            assert np.array_equal(g, w), i


def check(c, got):
    """The device's words equal ensemble_ref of its OWN rows and score words, and ensemble_ref of the oracle loop; its other values equal the oracle's."""
    z, words, xsub = got[-3], got[-2], got[-1]
    assert words.dtype == U and words.shape == (EC.T4 * c["rpt"], c["G"], BASE + 4 * c["E"])
    own = EC.reference(c, rows=xsub if c["substeps"] else got[0][:, 1:], z=z)
    assert ens_words_differ(words, own) == 0
    assert ens_words_differ(words, c["words"]) == 0
    assert words_differ(z, c["z"]) == 0
    same_values(got[:7] + got[-1:], c["want"])
    return words


@pytest.mark.parametrize("case", EC.CASES, ids=EC.IDS)
def test_every_case(case):
    c = EC.prepared(*case)
    S = SdeMpcSolver(c["cfg"], c["model"], max_batch=c["B"])
    got = fly(S, c)
    S.solve_status()
    words = check(c, got)
    s = ensemble_summary(words, c["ens"])
    assert s["n"].sum(axis=1).tolist() == [c["B"]] * words.shape[0] and (np.nan_to_num(s["survival"], nan=1.0) <= 1.0).all()
    S.close()


@pytest.mark.parametrize("mlp_dtype,math_mode", [("f32x3", "fast"), ("f16", "fast")])
def test_other_arithmetics_at_300(mlp_dtype, math_mode):
    c = EC.prepared(300, 3, 3, 1, False, mlp_dtype=mlp_dtype, math_mode=math_mode)
    S = SdeMpcSolver(c["cfg"], c["model"], max_batch=300)
    got = fly(S, c)
    S.solve_status()
    check(c, got)
    S.close()


@pytest.mark.parametrize("B", [65, 300])
def test_outputs_false_two_chunks_and_no_other_output_changes(B):
    """The same words without the per-row outputs and with one period per chunk (SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES = 0: two chunks, two pairs of ensemble launches);
    and with ensemble= every other returned value is what the call without it returns."""
    c = EC.prepared(*[k for k in EC.CASES if k[0] == B][0])
    S = SdeMpcSolver(c["cfg"], c["model"], max_batch=B)
    got = fly(S, c)
    words = check(c, got)
    bare = fly(S, c, outputs=False)
    assert bare[0] is None and bare[-1] is None and ens_words_differ(bare[-2], words) == 0 and words_differ(bare[-3], got[-3]) == 0
    S.set_option("test_loop_chunk_bytes", 0)
    cut = fly(S, c)
    cut_bare = fly(S, c, outputs=False, substep_states=False)
    S.set_option("test_loop_chunk_bytes", -1)
    assert ens_words_differ(cut[-2], words) == 0 and ens_words_differ(cut_bare[-1], words) == 0
    same_values(cut[:-2] + cut[-1:], got[:-2] + got[-1:])
    plain = fly(S, c, ensemble=None, cohort=None)
    S.solve_status()
    assert len(plain) == len(got) - 1
    same_values(plain, got[:-2] + got[-1:])
    S.close()


def test_continuation_through_score_in():
    """2 T ticks in one call against T + T through score_in and the other continuation values: the second call's words are rows T .. 2T-1 of the long call's, which
    equal the reference of the oracle flown for 2 T ticks."""
    B, T = 65, 2 * EC.T4
    c = EC.prepared(65, 3, 16, 1, True)
    cfg, model, x0, xref, keys, kw = EC.inputs(B, T=T)
    want = EC.oracle_loop(cfg, model, x0, xref, keys, T, **kw)
    g = targets(xref, T)
    score = EC.thresholds_from(want[0], want[-1], g, finite=EC.finite_episodes(want[-1]))
    z = score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), False, EC.S2)
    ref = ensemble_ref(want[0][:, 1:], g, z, c["cohort"], c["ens"].edges, score.thresholds(), 3, 1)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    common = dict(substep_states=True, score=score, ensemble=c["ens"], cohort=c["cohort"])
    full = S.closed_loop(x0, xref, keys, T, score_ref=g, **common, **kw)
    half = EC.T4
    ka = dict(kw, fault=kw["fault"][:half], disturbance=kw["disturbance"][:half])
    a = S.closed_loop(x0, xref, keys, half, score_ref=g[:half], **common, **ka)
    kb = dict(kw, fault=kw["fault"][half:], disturbance=kw["disturbance"][half:], u_init=a[3], stepsize_in=a[4], u_act_in=a[6])
    b = S.closed_loop(a[0][:, -1], xref, a[5], half, score_ref=g[half:], score_in=a[-3], **common, **kb)
    S.solve_status()
    assert ens_words_differ(full[-2], ref) == 0
    assert ens_words_differ(a[-2], full[-2][:half]) == 0 and ens_words_differ(b[-2], full[-2][half:]) == 0
    assert words_differ(b[-3], full[-3]) == 0 and words_differ(full[-3], z) == 0
    assert (b[-2][..., 2] >= a[-2][-1, :, 2]).all()                                          # the failed-by-now count keeps counting
    S.close()


def test_geometric_controller():
    """The baseline controller flown under the same ensemble: the words against the reference of the call's own rows and score; the score and every other output
    are those of the baseline call without ensemble=; and the MPC's words on the same episodes are a different array (the paired comparison has two sides)."""
    c = EC.prepared(65, 3, 16, 1, True)
    ctl, rate = geo_cases.controller(c["model"]), geo_cases.rate_loop()
    S = SdeMpcSolver(c["cfg"], c["model"], max_batch=65)
    got = fly(S, c, controller=ctl, rate_loop=rate)
    plain = fly(S, c, controller=ctl, rate_loop=rate, ensemble=None, cohort=None)
    mpc = fly(S, c, rate_loop=rate)
    S.solve_status()
    z_at = [i for i, v in enumerate(got) if v is not None and v.dtype == SCORE_DTYPE][0]
    words, z, xsub = got[z_at + 1], got[z_at], got[-1]
    assert words.dtype == U and ens_words_differ(words, EC.reference(c, rows=xsub, z=z)) == 0
    same_values(plain, got[:z_at + 1] + got[z_at + 2:])
    assert ens_words_differ(mpc[z_at + 1], EC.reference(c, rows=mpc[-1], z=mpc[z_at])) == 0 and ens_words_differ(mpc[z_at + 1], words) > 0
    S.close()


def test_ens_out_sits_between_guard_words(monkeypatch):
    """The entry point writes R * G * W words at ens_out and not one word in front of or behind them."""
    c = EC.prepared(257, 3, 0, 0, False)
    S = SdeMpcSolver(c["cfg"], c["model"], max_batch=257)
    real = _abi.ensemble_entry(S.lib)
    n = EC.T4 * 3 * BASE
    buf = np.full(n + 128, 0xA5A5A5A5, U)

    def guarded(lib):
        return lambda h, ens, out, *rest: real(h, ens, buf[64:64 + n].ctypes.data_as(C.POINTER(C.c_uint32)), *rest)
    monkeypatch.setattr(_abi, "ensemble_entry", guarded)
    got = fly(S, c)
    S.solve_status()
    assert (buf[:64] == 0xA5A5A5A5).all() and (buf[64 + n:] == 0xA5A5A5A5).all() and not got[-2].any()
    assert ens_words_differ(buf[64:64 + n].reshape(EC.T4, 3, BASE), c["words"]) == 0
    S.close()


def test_handle_with_a_past_and_poisoned_buffers():
    """SDEMPC_OPT_TEST_WS_FILL = 255 (every new buffer starts as NaNs, the partial and combined words among them); a smaller batch and other cohorts first."""
    c, small = EC.prepared(300, 3, 3, 1, False), EC.prepared(63, 3, 3, 1, False)
    S = SdeMpcSolver(c["cfg"], c["model"], max_batch=300, options={"test_ws_fill": 255})
    assert not S.device_ready()
    first = fly(S, small)
    got = fly(S, c)
    again = fly(S, small, outputs=False)
    S.solve_status()
    check(c, got)
    check(small, first)
    assert ens_words_differ(again[-2], small["words"]) == 0
    S.close()
