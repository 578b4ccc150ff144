"""CPU reference of the per-row ensemble words of SPEC.md §11m: ensemble_ref is a pure NumPy float32 function of a closed loop's scored rows, the target rows, the
FINAL score words of the call, the cohorts and the edges. The per-row quantities (dp, dv, c, w2, nf) are row_terms of tests/score_loop_ref.py, the cause bits are
formed from them as score_rows forms them, so a channel here is the score's channel. The float sums carry the one association the SPEC states — blocks of 256
consecutive episodes, per wave of 64 lanes the xor butterfly d = 1 .. 32 (every lane forms x_l + x_{l xor d}), (s0 + s1) + (s2 + s3) per block, the blocks added
in ascending order to a total that starts at +0 — vectorised over [blocks][4][64]. Applied to the oracle loop's rows it is the CPU reference of
sdempc_closed_loop_batch_ensemble; applied to what a device call returned it checks the device's words against the device's own rows. Test infrastructure.

`mutant` builds a deliberately WRONG reducer, one line each, for the discrimination tests (MUTANTS, in the order of the issue that asked for them)."""
import numpy as np

from score_loop_ref import NONE, as_words, row_terms

F = np.float32
U = np.uint32
BASE = 20
MUTANTS = ("sequential_sum", "blocks_reversed", "chained_block_sum", "edge_le", "alive_le", "nf_included", "cohort_off_by_one", "local_row_index",
           "first_before_scoring", "min_max_swapped")


def butterfly_sum(x, mutant=None):
    """The §11m sum of x f32[B] (excluded episodes already +0): pad to whole blocks with +0, [blocks][4][64], butterfly, block sums, ascending total."""
    x = np.asarray(x, F)
    nblk = -(-x.shape[0] // 256)
    v = np.zeros(nblk * 256, F)
    v[:x.shape[0]] = x
    if mutant == "sequential_sum":
        t = F(0.0)
        for a in v[:x.shape[0]]:
            t = F(t + a)
        return t
    v = v.reshape(nblk, 4, 64)
    lane = np.arange(64)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in (1, 2, 4, 8, 16, 32):
            v = (v + v[:, :, lane ^ d]).astype(F)
        s = v[:, :, 0]
        assert (v == s[:, :, None]).all() or np.isnan(v).any()       # all lanes of a wave end equal
        if mutant == "chained_block_sum":
            blk = (((s[:, 0] + s[:, 1]).astype(F) + s[:, 2]).astype(F) + s[:, 3]).astype(F)
        else:
            blk = ((s[:, 0] + s[:, 1]).astype(F) + (s[:, 2] + s[:, 3]).astype(F)).astype(F)
        t = F(0.0)
        for k in (range(nblk - 1, -1, -1) if mutant == "blocks_reversed" else range(nblk)):
            t = F(t + blk[k])
    return t


def channels(rows, targets, thresholds, rows_per_tick=1):
    """(v f32[R][B][4], nf bool[R][B], cause u32[R][B]) of rows f32[B][R][13] against targets [Tr][Br][13]: row_terms of score_loop_ref per row, the cause as
    score_rows forms it. Tick k of the call owns rows k * rows_per_tick .. (k + 1) * rows_per_tick - 1."""
    rows, g = np.asarray(rows, F), np.asarray(targets, F)
    if g.ndim == 1:
        g = g[None, None]
    elif g.ndim == 2:
        g = g[:, None]
    B, R = rows.shape[:2]
    r2, cmin, w2max = (F(t) for t in thresholds)
    v, nf, cause = np.zeros((R, B, 4), F), np.zeros((R, B), bool), np.zeros((R, B), U)
    for i in range(R):
        k = i // rows_per_tick
        for b in range(B):
            dp, dv, c, w2, bad = row_terms(rows[b, i], g[k if g.shape[0] > 1 else 0, b if g.shape[1] > 1 else 0])
            v[i, b] = (dp, dv, c, w2)
            nf[i, b] = bad
            cause[i, b] = 1 * (not bool(dp <= r2)) + 2 * (not bool(c >= cmin)) + 4 * (not bool(w2 <= w2max)) + 8 * bad
    return v, nf, cause


def ensemble_ref(rows, targets, words, cohort, edges, thresholds, G, over=1, rows_per_tick=1, mutant=None, words_before=None, terms=None):
    """u32[R][G][20 + 4 E]: the words of SPEC.md §11m for scored rows f32[B][R][13] (xs[:, 1:], or xsub for a substep score), targets [Tr][Br][13], the FINAL
    score words u32[B][16] (or the structured array) of the call that scored these rows, cohort int[B] (None: zeros), edges f32[4][E]. terms: channels(...) of the
    same rows, computed once and shared. words_before: the score words the call started from (only the mutant that reads word 8 too early looks at them)."""
    assert mutant is None or mutant in MUTANTS
    rows = np.asarray(rows, F)
    B, R = rows.shape[:2]
    z = as_words(words)
    coh = np.zeros(B, np.int64) if cohort is None else np.asarray(cohort, np.int64)
    edges = np.asarray(edges, F).reshape(4, -1)
    E = edges.shape[1]
    v, nf, cause = channels(rows, targets, thresholds, rows_per_tick) if terms is None else terms
    first = z[:, 8]
    if mutant == "first_before_scoring":
        first = np.full(B, NONE, U) if words_before is None else as_words(words_before)[:, 8]
    if mutant == "cohort_off_by_one":
        coh = coh + 1
    out = np.zeros((R, G, BASE + 4 * E), U)
    for i in range(R):
        r = (z[:, 0] - U(R) + U(i)).astype(U)                    # the global index of the row: word 0 before it was counted (unsigned wrap)
        if mutant == "local_row_index":
            r = np.full(B, i, U)
        before = first <= r if mutant == "alive_le" else first < r
        by_now = first <= r
        fin = np.ones(B, bool) if mutant == "nf_included" else ~nf[i]
        alive = fin & ~(before & bool(over))
        for g in range(G):
            in_g = coh == g
            inc = in_g & alive
            w = out[i, g]
            w[0], w[1], w[2], w[3] = in_g.sum(), inc.sum(), (in_g & by_now).sum(), (in_g & (cause[i] != 0)).sum()
            for bit in range(4):
                w[4 + bit] = (in_g & ((cause[i] >> bit) & 1 == 1)).sum()
            for k in range(4):
                val = v[i, :, k]
                w[8 + 3 * k] = np.asarray(butterfly_sum(np.where(inc, val, F(0.0)), mutant), F).reshape(1).view(U)[0]
                mn, mx = F(np.inf), F(-np.inf)
                for a in val[inc]:                               # "v < cur replaces" / "v > cur replaces", in episode order
                    if a < mn:
                        mn = a
                    if a > mx:
                        mx = a
                if mutant == "min_max_swapped":
                    mn, mx = mx, mn
                w[9 + 3 * k] = np.asarray(mn, F).reshape(1).view(U)[0]
                w[10 + 3 * k] = np.asarray(mx, F).reshape(1).view(U)[0]
                for j in range(E):
                    with np.errstate(invalid="ignore"):
                        below = val <= edges[k, j] if mutant == "edge_le" else val < edges[k, j]
                    w[BASE + k * E + j] = (inc & below).sum()
    return out


def ens_words_differ(a, b):
    """Number of words that differ between two u32[R][G][W] arrays: the float words (8 .. 19) by bit pattern with a NaN equal to any NaN, every other word as an integer."""
    a, b = np.ascontiguousarray(a, U), np.ascontiguousarray(b, U)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = a != b
    fa, fb = a[..., 8:BASE].view(F), b[..., 8:BASE].view(F)
    d[..., 8:BASE] &= ~(np.isnan(fa) & np.isnan(fb))
    return int(d.sum())
