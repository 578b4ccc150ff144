// sdempc_outcome.inc.h — predicted outcome (SPEC.md §12c): every particle of the particle x horizon tensor a store_traj rollout left in the handle is scored as
// §11h scores an episode — rows x_1 .. x_H against the target rows: squared position and velocity error, tilt cosine, squared body rate, the four cause bits —
// and the score words and channels are reduced over the valid particles: per-step failure counts, the first-failure histogram, the causes ever met, and per
// row and per horizon aggregate the mean / min / max and up to eight order statistics of each channel. Included by sdempc_prng.hip after sdempc_band.inc.h
// (whose key order and in-register sort it uses, with the half-wave butterflies of sdempc_tube.inc.h and the slot fold of sdempc_risk.inc.h): the reducer
// runs as one more mode of sdempc_noise_kernel, selected by OutcomeArgs::traj.
//
// Path replaced (reference): none on the device — the reference returns the particle mean and the expected cost only (sde_control.py:698,717); a predicted
// failure probability was a host loop over rollout(want_traj=True), i.e. a relayout and a copy of the whole tensor.
//
// Mapping: one workgroup of 256 threads per instance, eight 32-lane halves, two phases, each only where one of its outputs is asked for.
//   SWEEP (words, fail_step, first_fail, cause_ever, agg_stat, agg_q) — risk's: half h takes the particle groups g = h, h + 8, ... with the particle in the
//     lane and walks t = 1 .. H in order: 13 loads of one 128-byte line each per step, addresses independent of the data; the target row is uniform (scalar
//     loads). The running §11h words stay in registers; per step five ballots + popcounts go into LDS counters; after the walk the histogram and the cause
//     counts by LDS atomics, the four horizon aggregates into LDS with their §6.1 group totals and extrema. Then four threads fold the groups (agg_stat) and
//     half k < 4 selects the ranks of aggregate k from its LDS copy (agg_q).
//   ROWS (chan_stat, chan_q) — the tube's: half h takes the rows r = h, h + 8, ...; per row it forms the four channels of every group from 11 lines each
//     (the attitude's w and z are not needed), reduces them as the tube reduces a column, and selects per channel. No LDS, no barrier. The lines come from
//     the cache where the sweep ran first.
//   Selection, in the key order of §12b: G <= 4 (up to P = 128) the in-register bitonic sort of sdempc_band.inc.h over the <= 4 words per lane (padded lanes
//     key 0xFFFFFFFF), lane k fetches rank ranks[k]. There is no path above that: the launcher refuses chan_q and agg_q for P > OUTCOME_RANK_MAX_P (a
//     bit-by-bit select beside the sort, as the bands form has one, cost the hosting kernel a second register of spilled scalars and every form 12 bytes of
//     scratch). Every other output has no particle limit: G > 4 forms chan_stat in one pass per channel, loading only that channel's lines.
// Padded lanes are masked everywhere. Dynamic LDS only (outcome_lds_words_host, sized by the launcher): the noise, tube and bands modes allocate none.
#pragma once
#include <stddef.h>

namespace sdempc {

// The arguments of sdempc_noise_kernel as they lie in its kernel argument segment (each at its natural alignment, in order), and this mode's own struct read
// THERE through a constant-address-space pointer: scalar loads where a member is used. Read as a by-value parameter, every member the mode touches anywhere was
// loaded ahead of its first loop and carried in scalar registers through all of them; the hosting kernel then needed a second vector register for spilled
// scalars and the risk form's sweep lost a register pair to scratch. Each phase takes a fresh opaque copy of the pointer, so nothing loaded for one phase
// stays live into the next.
struct NoiseKernargs { const uint32_t* keys; float* out; int P, G, HC, b0; TubeArgs T; RiskArgs R; BandArgs Q; OutcomeArgs W; };
typedef const __attribute__((address_space(4))) OutcomeArgs* OutcomeK;
DI OutcomeK outcome_args() {
    const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(NoiseKernargs, W);
    asm volatile("" : "+s"(p));
    return (OutcomeK)p;
}

// SPEC.md §11h "Per row", restated (the arithmetic of the scoring form of sdempc_loop_keys_period_kernel; tests pin the two to each other through
// score_loop_ref). x: the instance's tensor (uniform), o: this lane's word of component 0 of the row in it (32 floats per component) — a scalar base and a
// 32-bit lane offset, not a pointer per lane: the row phase has no register pairs to spare. gt: the target row (uniform). ch = {dp, dv, c, w2}.
DI void outcome_channels(const float* x, uint32_t o, const float* gt, float* ch) {
    const float x0 = x[o], x1 = x[o + 32u], x2 = x[o + 64u], x3 = x[o + 96u], x4 = x[o + 128u], x5 = x[o + 160u], qx = x[o + 224u], qy = x[o + 256u];
    const float w0 = x[o + 320u], w1 = x[o + 352u], w2 = x[o + 384u];
    const float e0 = x0 - gt[0], e1 = x1 - gt[1], e2 = x2 - gt[2];
    ch[0] = FMA(e2, e2, FMA(e1, e1, e0 * e0));
    const float f0 = x3 - gt[3], f1 = x4 - gt[4], f2 = x5 - gt[5];
    ch[1] = FMA(f2, f2, FMA(f1, f1, f0 * f0));
    ch[2] = FMA(-2.0f, qx * qx + qy * qy, 1.0f);
    ch[3] = FMA(w2, w2, FMA(w1, w1, w0 * w0));
}

// rank rank_l's key of a sorted half (band_sort128: rank r is register r & 3 of lane r >> 2), fetched by this lane
DI uint32_t outcome_pick(const uint32_t* a, int rank_l) {
    const int src = (int)((threadIdx.x & 32u) + (unsigned)(rank_l >> 2)) * 4;
    const uint32_t x0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[0]), x1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[1]);
    const uint32_t x2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[2]), x3 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[3]);
    const int rs = rank_l & 3;
    return rs == 0 ? x0 : rs == 1 ? x1 : rs == 2 ? x2 : x3;
}

// the SWEEP phase: every particle's §11h words over t = 1 .. H, the counters and the aggregates into LDS
DI void outcome_sweep(OutcomeK W, int P, int G, int b, uint32_t* s_fail, uint32_t* s_hist, uint32_t* s_cause, float* s_gs, float* s_val) {
    const int H = W->H, C = (H + 1) * 13;
    const int tid = threadIdx.x, l = tid & 31, half = tid >> 5;
    const bool want_fail = W->fail_step != nullptr;      // (wave-uniform)
    const bool want_agg = W->agg_stat || W->agg_q;
    const float* tg = W->tgt + (size_t)b * W->tgt_bstride;
    const size_t gstride = (size_t)C * 32;
    for (int g = half; g < G; g += 8) {                  // (uniform in the half; every cross-lane step below stays inside it)
        const int p = g * 32 + l;
        const bool valid = p < P;
        const float* tp = W->traj + ((size_t)b * G + g) * gstride + l;
        float sdp = 0.0f, mdp = 0.0f, ldp = 0.0f, sdv = 0.0f, minc = __builtin_inff(), mw2 = 0.0f;
        uint32_t imax = 0u, first = 0xffffffffu, causes = 0u, nbad = 0u;
        for (int t = 1; t <= H; ++t) {
            const float* gt = tg + (size_t)t * W->tgt_tstride;
            float xa[13];
#pragma unroll
            for (int i = 0; i < 13; ++i) xa[i] = tp[(size_t)(t * 13 + i) * 32];
            // nf: some |x_i| < inf fails, i.e. the largest magnitude word is an infinity's or a NaN's (integer max: one compare, no lane mask per component)
            uint32_t mag = 0u;
#pragma unroll
            for (int i = 0; i < 13; ++i) mag = band_max(mag, __float_as_uint(xa[i]) & 0x7FFFFFFFu);
            const bool nf = mag >= 0x7F800000u;
            const float e0 = xa[0] - gt[0], e1 = xa[1] - gt[1], e2 = xa[2] - gt[2];
            const float dp = FMA(e2, e2, FMA(e1, e1, e0 * e0));
            const float f0 = xa[3] - gt[3], f1 = xa[4] - gt[4], f2 = xa[5] - gt[5];
            const float dv = FMA(f2, f2, FMA(f1, f1, f0 * f0));
            const float c = FMA(-2.0f, xa[7] * xa[7] + xa[8] * xa[8], 1.0f);
            const float w2 = FMA(xa[12], xa[12], FMA(xa[11], xa[11], xa[10] * xa[10]));
            const uint32_t cause = (!(dp <= W->r2_pos) ? 1u : 0u) | (!(c >= W->cos_min) ? 2u : 0u) | (!(w2 <= W->w2_max) ? 4u : 0u) | (nf ? 8u : 0u);
            const uint32_t r = (uint32_t)(t - 1);
            sdp = sdp + dp;
            if (dp > mdp) { mdp = dp; imax = r; }
            ldp = dp;
            sdv = sdv + dv;
            if (c < minc) minc = c;
            if (w2 > mw2) mw2 = w2;
            if (cause) {
                if (first == 0xffffffffu) first = r;
                causes |= cause;
                nbad += 1u;
            }
            if (want_fail) {
                uint32_t n = 0u;                         // lane k < 5 of the half adds count k (an opaque copy of the lane index: the five lane masks
                int lk = l;                              // are formed here, not carried in scalar register pairs through the sweep)
                asm volatile("" : "+v"(lk));
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const uint32_t nk = band_count(valid && (k < 4 ? (cause >> k) & 1u : cause) != 0u);
                    n = lk == k ? nk : n;
                }
                if (n) atomicAdd(&s_fail[r * 5u + (uint32_t)lk], n);
            }
        }
        if (valid) {
            atomicAdd(&s_hist[first == 0xffffffffu ? (uint32_t)H : first], 1u);
            if (W->words) {
                uint32_t* w = W->words + ((size_t)b * P + p) * OUTCOME_WORDS;
                w[0] = (uint32_t)H; w[1] = __float_as_uint(sdp); w[2] = __float_as_uint(mdp); w[3] = imax; w[4] = __float_as_uint(ldp);
                w[5] = __float_as_uint(sdv); w[6] = __float_as_uint(minc); w[7] = __float_as_uint(mw2); w[8] = first; w[9] = causes; w[10] = nbad;
            }
        }
        {
            uint32_t n = 0u;
            int lk = l;
            asm volatile("" : "+v"(lk));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t nk = band_count(valid && ((causes >> k) & 1u) != 0u);
                n = lk == k ? nk : n;
            }
            if (n) atomicAdd(&s_cause[lk], n);
        }
        if (want_agg) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = k == 0 ? sdp : k == 1 ? mdp : k == 2 ? minc : mw2;
                s_val[p * 4 + k] = a;
                const float tot = tube_sum32(valid ? a : 0.0f);
                const float mn = tube_min32(valid ? a : __builtin_inff());
                const float mx = tube_max32(valid ? a : -__builtin_inff());
                if (l == 0) { s_gs[g * 12 + k * 3 + 0] = tot; s_gs[g * 12 + k * 3 + 1] = mn; s_gs[g * 12 + k * 3 + 2] = mx; }
            }
        }
    }
}

// the ROWS phase: chan_stat and chan_q of the rows r = half, half + 8, ...; rank_l: ranks[l] in lane l < n_ranks of each half
DI void outcome_rows(OutcomeK W, int P, int G, int b, int nq, int rank_l) {
    const int H = W->H, C = (H + 1) * 13;
    const int l0 = threadIdx.x & 31, half = threadIdx.x >> 5;
    const float* tg = W->tgt + (size_t)b * W->tgt_bstride;
    const uint32_t gstride = (uint32_t)C * 32u;          // (an instance's tensor stays below 2^31 words: launch_noise_from_keys' own limit on P H)
    const float* tb = W->traj + (size_t)b * G * gstride;
#pragma nounroll
    for (int r = half; r < H; r += 8) {                  // (uniform in the half; every cross-lane step below stays inside it)
        const float* gt = tg + (size_t)(r + 1) * W->tgt_tstride;
        // (the lane predicates of a row are formed here, from an opaque copy of the lane index: hoisted out of the row loop, the twenty-odd lane masks would each
        // hold a scalar register pair through it — sdempc_band.inc.h)
        int l = l0;
        asm volatile("" : "+v"(l));
        const uint32_t row = (uint32_t)(r + 1) * 416u + (uint32_t)l;
        const uint32_t o = (uint32_t)r * 4u;             // (row, channel) index inside the instance; the stores below: a scalar base and a 32-bit lane offset
        if (G <= 4) {                                    // (wave-uniform) the row's <= 4 words per lane and channel, kept
            float v[4][4];                               // [channel][group] (constant indices after unrolling: registers)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float ch[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (s < G) outcome_channels(tb, row + (uint32_t)s * gstride, gt, ch);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k][s] = ch[k];
                __builtin_amdgcn_sched_barrier(0);       // (one group's 11 lines in flight at a time: all 44 cost the kernel its register budget)
            }
            if (W->chan_stat) {
                float res = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float S[4], mn = __builtin_inff(), mx = -__builtin_inff();
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const bool valid = s * 32 + l < P;
                        S[s] = 0.0f;
                        if (s < G) {
                            S[s] = S[s] + tube_sum32(valid ? v[k][s] : 0.0f);
                            mn = __builtin_fminf(mn, tube_min32(valid ? v[k][s] : __builtin_inff()));
                            mx = __builtin_fmaxf(mx, tube_max32(valid ? v[k][s] : -__builtin_inff()));
                        }
                    }
                    const float mean = (((S[0] + S[1]) + S[2]) + S[3]) * W->invP;
                    res = l == 3 * k ? mean : l == 3 * k + 1 ? mn : l == 3 * k + 2 ? mx : res;
                }
                if (l < 12) (W->chan_stat + (size_t)b * H * 12)[o * 3u + (uint32_t)l] = res;
            }
            if (nq) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t a[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) a[s] = s * 32 + l < P ? band_key(v[k][s]) : 0xFFFFFFFFu;
                    band_sort128(a, l);
                    const uint32_t x = outcome_pick(a, rank_l);
                    if (l < nq) (W->chan_q + (size_t)b * H * 4 * nq)[(o + k) * (uint32_t)nq + (uint32_t)l] = __uint_as_float(band_word(x));
                }
            }
        } else {
            if (W->chan_stat) {                          // one pass per channel: only that channel's lines are loaded
                float res = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float S[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mn = __builtin_inff(), mx = -__builtin_inff();
                    for (int g0 = 0; g0 < G; g0 += 4) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int g = g0 + s;
                            if (g < G) {                 // (wave-uniform)
                                const bool valid = g * 32 + l < P;
                                float ch[4];
                                outcome_channels(tb, row + (uint32_t)g * gstride, gt, ch);
                                S[s] = S[s] + tube_sum32(valid ? ch[k] : 0.0f);
                                mn = __builtin_fminf(mn, tube_min32(valid ? ch[k] : __builtin_inff()));
                                mx = __builtin_fmaxf(mx, tube_max32(valid ? ch[k] : -__builtin_inff()));
                            }
                        }
                    }
                    const float mean = (((S[0] + S[1]) + S[2]) + S[3]) * W->invP;
                    res = l == 3 * k ? mean : l == 3 * k + 1 ? mn : l == 3 * k + 2 ? mx : res;
                }
                if (l < 12) (W->chan_stat + (size_t)b * H * 12)[o * 3u + (uint32_t)l] = res;
            }
        }
    }
}

// dynamic LDS of one workgroup (outcome_lds_words_host, sdempc_kernels.h): fail[5 H] hist[H+1] cause[4] gs[G][12] val[G*32][4]
// the outcome mode of sdempc_noise_kernel: one workgroup per instance b. P, G as in the noise mode.
DI void outcome_reduce(int P, int G, int b) {
    OutcomeK W = outcome_args();
    extern __shared__ uint32_t outcome_lds[];
    const int H = W->H;
    const int tid = threadIdx.x, l = tid & 31, half = tid >> 5;
    uint32_t* s_fail = outcome_lds;                      // [H][5]
    uint32_t* s_hist = s_fail + 5 * H;                   // [H+1]
    uint32_t* s_cause = s_hist + (H + 1);                // [4]
    float* s_gs = (float*)(s_cause + 4);                 // [G][4][3]: group total, min, max of each aggregate
    float* s_val = s_gs + 12 * G;                        // [G*32][4]: the aggregates per particle
    const int nq = W->n_ranks;                           // (0 where neither chan_q nor agg_q is given)

    if (W->words || W->fail_step || W->first_fail || W->cause_ever || W->agg_stat || W->agg_q) {       // (wave-uniform)
        for (int i = tid; i < 6 * H + 5; i += 256) s_fail[i] = 0u;
        __syncthreads();
        outcome_sweep(W, P, G, b, s_fail, s_hist, s_cause, s_gs, s_val);
        __syncthreads();
        if (W->fail_step)
            for (int i = tid; i < 5 * H; i += 256) W->fail_step[(size_t)b * 5 * H + i] = s_fail[i];
        if (W->first_fail)
            for (int i = tid; i <= H; i += 256) W->first_fail[(size_t)b * (H + 1) + i] = s_hist[i];
        if (W->cause_ever && tid < 4) W->cause_ever[(size_t)b * 4 + tid] = s_cause[tid];
        if (W->agg_stat && tid < 4) {
            const float* T = s_gs + tid * 3;             // [g][12]: total, min, max of aggregate tid in group g
            float mn = __builtin_inff(), mx = -__builtin_inff();
            float S[4] = {0.0f, 0.0f, 0.0f, 0.0f};       // the §6.1 slots (constant indices after unrolling: registers)
            for (int g0 = 0; g0 < G; g0 += 4) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (g0 + s < G) {
                        S[s] = S[s] + T[(g0 + s) * 12];
                        mn = __builtin_fminf(mn, T[(g0 + s) * 12 + 1]);
                        mx = __builtin_fmaxf(mx, T[(g0 + s) * 12 + 2]);
                    }
            }
            float* o = W->agg_stat + ((size_t)b * 4 + tid) * 3;
            o[0] = (((S[0] + S[1]) + S[2]) + S[3]) * W->invP;
            o[1] = mn;
            o[2] = mx;
        }
    }
    W = outcome_args();
    int rank_l = 0;                                      // ranks[l] in lane l of each half, formed behind the sweep: one register less in it
#pragma unroll
    for (int k = 0; k < OUTCOME_MAX_RANKS; ++k) rank_l = l == k ? W->ranks[k] : rank_l;   // (constant indices into the argument: no copy of it in scratch)
    if (W->agg_q && half < 4) {                          // (uniform in the half) half k selects aggregate k
        const float* val = s_val + half;                 // [p][4]
        uint32_t a[4];                                   // (G <= 4: the launcher refuses the order statistics above OUTCOME_RANK_MAX_P)
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = s < G && s * 32 + l < P ? band_key(val[(s * 32 + l) * 4]) : 0xFFFFFFFFu;
        band_sort128(a, l);
        const uint32_t x = outcome_pick(a, rank_l);
        if (l < nq) W->agg_q[((size_t)b * 4 + half) * nq + l] = __uint_as_float(band_word(x));
    }
    if (W->chan_stat || W->chan_q) outcome_rows(W, P, G, b, W->chan_q ? nq : 0, rank_l);
}

}  // namespace sdempc
