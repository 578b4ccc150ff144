// sdempc_retire.inc.h — SPEC.md §11n: failed episodes of a closed-loop batch are retired at the next solve-period boundary and only the live set is solved. Included
// by sdempc_prng.hip (DI and the structs of sdempc_kernels.h are in scope). No kernel is added: sdempc_loop_keys_period_kernel hosts the two LIVE-LIST forms,
// launched after a period's scoring launch, and sdempc_broadcast_rows_kernel hosts the GATHER and SCATTER forms around the period's dense solve.
//
// Count form: one thread per episode. live[b] becomes live[b] AND (score word 8 of b is still all ones); an episode that leaves the live set takes retired_at[b] =
// Y.solve (the next solve of the call, or -1 when the call has none left). The workgroup's live count is the sum of the population counts of its four wave ballots
// and goes to blk[k]. Place form: the rank of a live episode is (sum of blk[0 .. k-1]) + (live lanes of the lower waves of the block) + (live lanes below it in its
// wave, mbcnt), and list[rank] = b: the list ascends in b whatever the arrival order of workgroups and waves, with no atomic and no inter-workgroup wait (the counts
// come from the launch before). The last block writes n_live. Threads past B stay for the workgroup barrier and are masked out of every ballot.
// Gather / scatter: plain word copies between row list[i] of per-episode buffers and row i of dense staging, 16 bytes per thread where a segment's row length is a
// multiple of four words and both bases are 16-byte aligned (the launch decides), else 4 bytes. The scatter form has one further grid row: it writes the held info
// row (0, step, 0 ..) of every retired episode and folds the give-up words of the dense solve's cooperative barriers into the loop's sticky flag.
#pragma once

namespace sdempc {

DI void retire_live_list(const LoopRetire& Y, int B) {
    __shared__ uint32_t ret_lds[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x;
    const int b = k * 256 + tid;
    bool lv = false;
    if (b < B) {
        if (Y.place) lv = Y.live[b] != 0;
        else {
            const bool was = Y.init != 0 || Y.live[b] != 0;
            lv = was && Y.words[(size_t)b * 16 + 8] == 0xffffffffu;
            Y.live[b] = lv ? 1 : 0;
            if (Y.init) Y.retired_at[b] = lv ? -1 : 0;
            else if (was && !lv) Y.retired_at[b] = Y.solve;
            if (Y.count) Y.count[b] = Y.init ? Y.words[(size_t)b * 16] : Y.count[b] + (uint32_t)Y.rows;
        }
    }
    const unsigned long long bal = __ballot(lv);
    if (lane == 0) ret_lds[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    const uint32_t c0 = ret_lds[0], c1 = ret_lds[1], c2 = ret_lds[2], c3 = ret_lds[3];
    if (!Y.place) {
        if (tid == 0) Y.blk[k] = (c0 + c1) + (c2 + c3);
        return;
    }
    uint32_t base = 0u;
    for (int j = 0; j < k; ++j) base += Y.blk[j];                    // (wave-uniform: scalar loads)
    const uint32_t woff = wave == 0 ? 0u : wave == 1 ? c0 : wave == 2 ? c0 + c1 : c0 + c1 + c2;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (lv) Y.list[base + woff + below] = b;
    if (k == (int)gridDim.x - 1 && tid == 0) *Y.n_live = (int32_t)(base + (c0 + c1) + (c2 + c3));
}

// grid: x = chunks of 256 copy units of one row, y = dense position i0 + blockIdx.y (the scatter form: y = n is the held-row pass over the episodes)
DI void compact_rows(const LoopCompact& Q) {
    const int i = Q.i0 + (int)blockIdx.y;
    unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (i >= Q.n) {                                      // (scatter form only: the launch adds this grid row)
        const unsigned stride = gridDim.x * 256u;
        for (unsigned b = t; b < (unsigned)Q.B; b += stride)
            if (Q.live[b] == 0) {
                float* inf = Q.held_info + (size_t)b * 8;
                inf[0] = 0.0f; inf[1] = Q.held_step[b];
#pragma unroll
                for (int c = 2; c < 8; ++c) inf[c] = 0.0f;
            }
        if (Q.coop_bar)
            for (unsigned j = t; j < (unsigned)Q.n; j += stride)
                if (Q.coop_bar[(size_t)COOP_BAR_WORDS * j + 1] != 0u) *Q.gave_up = 1u;
        return;
    }
    const int e = Q.list[i];
    const size_t from = Q.scatter ? (size_t)i : (size_t)e, to = Q.scatter ? (size_t)e : (size_t)i;
#pragma unroll
    for (int s = 0; s < COMPACT_SEGS; ++s) {             // (constant indices into the argument: no copy of it in scratch)
        if (s >= Q.nseg) return;
        const unsigned len = (unsigned)Q.seg[s].words;
        const unsigned units = Q.seg[s].vec ? len >> 2 : len;
        if (t < units) {
            if (Q.seg[s].vec) reinterpret_cast<uint4*>(Q.seg[s].dst + to * len)[t] = reinterpret_cast<const uint4*>(Q.seg[s].src + from * len)[t];
            else Q.seg[s].dst[to * len + t] = Q.seg[s].src[from * len + t];
            return;
        }
        t -= units;
    }
}

}  // namespace sdempc
