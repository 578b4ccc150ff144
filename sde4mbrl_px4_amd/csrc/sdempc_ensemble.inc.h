// sdempc_ensemble.inc.h — SPEC.md §11m: per-row histories of a closed-loop batch reduced over its EPISODES, by cohort, on the device. Included by sdempc_prng.hip
// (FMA, DI and the structs of sdempc_kernels.h are in scope); hosted by sdempc_loop_keys_period_kernel as two further forms, launched after a chunk's scoring launch.
//
// score_row below is the ONE statement of the per-row quantities of SPEC.md §11h (include/sdempc.h at sdempc_score_cfg): the scoring form of the kernel and the
// partial form here both call it, so an ensemble channel is the score's channel bit for bit.
//
// Partial form: grid (blocks of 256 consecutive episodes) x (rows of the launch). Thread (k, i, l) holds episode b = 256 k + l at chunk row row0 + i; threads past
// B stay to the end (the workgroup barriers need them) and are masked out of every count. Per cohort g the workgroup forms the W = 20 + 4 E words of
// (row, block, g): counts are population counts of wave ballots; a float sum is the xor butterfly over the 64 lanes of a wave (d = 1, 2, 4, 8, 16, 32; every lane
// forms x_l + x_{l xor d}, so all lanes of a wave end equal), the four wave sums meet in workgroup memory and the block sum is (s0 + s1) + (s2 + s3); min and max
// take the same butterfly (no value is a NaN or -0 there, so the order does not matter). The words go to part[i][k][g][.].
// Combine form: one thread per (row, cohort, word) walks the blocks in ascending order: counts add, a float sum starts at +0 and takes one plain add per block,
// min / max replace on v < cur / v > cur. The words go to out[i][g][.].
#pragma once

namespace sdempc {

// (dp, dv, c, w2, nf) of one scored row x against the target (g0 .. g5), and its cause bits against the thresholds: every multiply and fma as SPEC.md §11h writes them
DI uint32_t score_row(const float* x, float g0, float g1, float g2, float g3, float g4, float g5, float r2_pos, float cos_min, float w2_max, float& dp, float& dv,
                      float& c, float& w2, bool& nf) {
    nf = false;
#pragma unroll
    for (int i = 0; i < 13; ++i) nf = nf || !(__builtin_fabsf(x[i]) < __builtin_inff());
    const float e0 = x[0] - g0, e1 = x[1] - g1, e2 = x[2] - g2;
    dp = FMA(e2, e2, FMA(e1, e1, e0 * e0));
    const float f0 = x[3] - g3, f1 = x[4] - g4, f2 = x[5] - g5;
    dv = FMA(f2, f2, FMA(f1, f1, f0 * f0));
    c = FMA(-2.0f, x[7] * x[7] + x[8] * x[8], 1.0f);
    w2 = FMA(x[12], x[12], FMA(x[11], x[11], x[10] * x[10]));
    return (!(dp <= r2_pos) ? 1u : 0u) | (!(c >= cos_min) ? 2u : 0u) | (!(w2 <= w2_max) ? 4u : 0u) | (nf ? 8u : 0u);
}

DI uint32_t ens_count(bool pred) { return (uint32_t)__popcll(__ballot(pred)); }

DI void ens_partial(const LoopEnsemble& N, int B) {
    __shared__ uint32_t ens_lds[4 * ENS_MAX_WORDS];
    const int E = N.E, W = ENS_BASE_WORDS + 4 * E;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x, i = blockIdx.y;
    const int b = k * 256 + tid;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};               // dp, dv, c, w2 (constant indices after unrolling: registers)
    uint32_t cause = 0u;
    bool nf = false, before = false, by_now = false;
    int coh = -1;                                        // (a thread past B belongs to no cohort)
    if (b < B) {
        const int row = N.row0 + i;
        const float* g = N.ref + (size_t)(row / N.rows_per_tick) * N.ref_tick_stride + (size_t)b * N.ref_ep_stride;
        const float* x = N.rows + ((size_t)row * B + b) * 13;
        cause = score_row(x, g[0], g[1], g[2], g[3], g[4], g[5], N.r2_pos, N.cos_min, N.w2_max, v[0], v[1], v[2], v[3], nf);
        // the global index of this row: word 0 after the chunk's scoring launch counts every row of the chunk
        // (SPEC.md §11n: a retired episode's word 0 is frozen, and the loop's own count of its rows stands in)
        const uint32_t r = (N.count ? N.count[b] : N.words[(size_t)b * 16]) - (uint32_t)N.chunk_rows + (uint32_t)row;
        const uint32_t f = N.words[(size_t)b * 16 + 8];
        before = f < r; by_now = f <= r;
        coh = N.cohort[b];
    }
    const bool alive = !nf && !(N.over != 0 && before);
    uint32_t* mine = ens_lds + wave * W;
    uint32_t* dst = N.part + ((size_t)i * gridDim.x + k) * (size_t)N.G * W;
    for (int g = 0; g < N.G; ++g) {
        const bool in_g = coh == g, inc = in_g && alive;
        const uint32_t c0 = ens_count(in_g), c1 = ens_count(inc), c2 = ens_count(in_g && by_now), c3 = ens_count(in_g && cause != 0u);
        const uint32_t c4 = ens_count(in_g && (cause & 1u)), c5 = ens_count(in_g && (cause & 2u)), c6 = ens_count(in_g && (cause & 4u)), c7 = ens_count(in_g && (cause & 8u));
        if (lane == 0) { mine[0] = c0; mine[1] = c1; mine[2] = c2; mine[3] = c3; mine[4] = c4; mine[5] = c5; mine[6] = c6; mine[7] = c7; }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const float val = v[ch];
            float s = inc ? val : 0.0f;
            // (a value that could never replace the start value stands as the start value: the result of "v < cur replaces" in any order)
            float mn = inc && val < __builtin_inff() ? val : __builtin_inff();
            float mx = inc && val > -__builtin_inff() ? val : -__builtin_inff();
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                s = s + __shfl_xor(s, d);
                const float a = __shfl_xor(mn, d), z = __shfl_xor(mx, d);
                mn = a < mn ? a : mn;
                mx = z > mx ? z : mx;
            }
            if (lane == 0) { mine[8 + 3 * ch] = __float_as_uint(s); mine[9 + 3 * ch] = __float_as_uint(mn); mine[10 + 3 * ch] = __float_as_uint(mx); }
            for (int j = 0; j < E; ++j) {
                const uint32_t below = ens_count(inc && val < N.edges[ch * E + j]);
                if (lane == 0) mine[ENS_BASE_WORDS + ch * E + j] = below;
            }
        }
        __syncthreads();
        if (tid < W) {
            const uint32_t a0 = ens_lds[tid], a1 = ens_lds[W + tid], a2 = ens_lds[2 * W + tid], a3 = ens_lds[3 * W + tid];
            uint32_t o;
            if (tid < 8 || tid >= ENS_BASE_WORDS) o = a0 + a1 + a2 + a3;
            else {
                const float s0 = __uint_as_float(a0), s1 = __uint_as_float(a1), s2 = __uint_as_float(a2), s3 = __uint_as_float(a3);
                const int kind = (tid - 8) % 3;
                float y;
                if (kind == 0) y = (s0 + s1) + (s2 + s3);
                else if (kind == 1) { const float p = s1 < s0 ? s1 : s0, q = s3 < s2 ? s3 : s2; y = q < p ? q : p; }
                else { const float p = s1 > s0 ? s1 : s0, q = s3 > s2 ? s3 : s2; y = q > p ? q : p; }
                o = __float_as_uint(y);
            }
            dst[(size_t)g * W + tid] = o;
        }
        __syncthreads();                                 // (the next cohort writes the same words of workgroup memory)
    }
}

DI void ens_combine(const LoopEnsemble& N) {
    const int W = ENS_BASE_WORDS + 4 * N.E, GW = N.G * W;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)N.nrows * GW) return;
    const int i = (int)(t / GW), gw = (int)(t - (long long)i * GW), wd = gw % W;
    const uint32_t* p = N.part + (size_t)i * N.nblk * GW + gw;
    uint32_t o;
    if (wd < 8 || wd >= ENS_BASE_WORDS) {
        o = 0u;
        for (int k = 0; k < N.nblk; ++k) o += p[(size_t)k * GW];
    } else {
        const int kind = (wd - 8) % 3;
        float y = kind == 0 ? 0.0f : kind == 1 ? __builtin_inff() : -__builtin_inff();
        for (int k = 0; k < N.nblk; ++k) {
            const float a = __uint_as_float(p[(size_t)k * GW]);
            if (kind == 0) y = y + a;
            else if (kind == 1) y = a < y ? a : y;
            else y = a > y ? a : y;
        }
        o = __float_as_uint(y);
    }
    N.out[t] = o;
}

}  // namespace sdempc
