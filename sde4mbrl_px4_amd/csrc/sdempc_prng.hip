// sdempc_prng.hip — key-derived noise on the device (SPEC.md §7): threefry2x32 counter-based generator with JAX's key
// conventions, mantissa-trick uniform, sqrt(2)*erfinv normal, written straight into the particle-minor layout
// f32[B][G][H][6][32] that the rollout kernels stream.
//
// Path replaced (reference): the key plumbing of the MPC node — jax.random.PRNGKey(seed) and its 3-way split
// (sde4mbrl_px4/mpc_controller/sde_control.py:338-341), one key into and out of every m_mpc call
// (sde_control.py:349-350,400-416,698,717). With this kernel the noise tensor never exists on the host: the boundary hands
// over 8 bytes of key per instance instead of P*H*6 floats over PCIe.
//
// Mapping: integer ALU + a short f32 polynomial per element, HBM-write-bound. One thread computes one threefry block, i.e. the
// two tensor elements e and e + N/2 (N = P*H*6; legacy JAX layout: first half of the counters in x0, second half in x1).
// Threads are ordered particle-fastest so that both stores of a wave fill whole 128-byte rows of the [..][32] layout.
// All f32 arithmetic is the explicit fma sequence of SPEC.md §7.2 (bit-identical to oracle/prng_oracle.c).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sdempc_kernels.h"

namespace sdempc {

#define FMA(a, b, c) __builtin_fmaf((a), (b), (c))
#define DI __device__ __forceinline__

DI uint32_t rotl32(uint32_t x, int r) { return __builtin_rotateleft32(x, r); }

DI void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
    const uint32_t k2 = k0 ^ k1 ^ 0x1BD11BDAu;
#define TF_ROUND(r) { x0 += x1; x1 = rotl32(x1, r); x1 ^= x0; }
    x0 += k0; x1 += k1;
    TF_ROUND(13) TF_ROUND(15) TF_ROUND(26) TF_ROUND(6)
    x0 += k1; x1 += k2 + 1u;
    TF_ROUND(17) TF_ROUND(29) TF_ROUND(16) TF_ROUND(24)
    x0 += k2; x1 += k0 + 2u;
    TF_ROUND(13) TF_ROUND(15) TF_ROUND(26) TF_ROUND(6)
    x0 += k0; x1 += k1 + 3u;
    TF_ROUND(17) TF_ROUND(29) TF_ROUND(16) TF_ROUND(24)
    x0 += k1; x1 += k2 + 4u;
    TF_ROUND(13) TF_ROUND(15) TF_ROUND(26) TF_ROUND(6)
    x0 += k2; x1 += k0 + 5u;
#undef TF_ROUND
}

DI float log_spec(float t) {
    const uint32_t b = __float_as_uint(t);
    int e = (int)((b >> 23) & 255u) - 126;
    const float m = __uint_as_float((b & 0x007FFFFFu) | 0x3F000000u);
    float x;
    if (m < 0.707106781186547524f) { e -= 1; x = (m + m) - 1.0f; } else x = m - 1.0f;
    const float z = x * x;
    float y = 7.0376836292E-2f;
    y = FMA(y, x, -1.1514610310E-1f);
    y = FMA(y, x, 1.1676998740E-1f);
    y = FMA(y, x, -1.2420140846E-1f);
    y = FMA(y, x, 1.4249322787E-1f);
    y = FMA(y, x, -1.6668057665E-1f);
    y = FMA(y, x, 2.0000714765E-1f);
    y = FMA(y, x, -2.4999993993E-1f);
    y = FMA(y, x, 3.3333331174E-1f);
    y = (y * x) * z;
    const float fe = (float)e;
    y = FMA(-2.12194440e-4f, fe, y);
    y = FMA(-0.5f, z, y);
    float r = x + y;
    r = FMA(0.693359375f, fe, r);
    return r;
}
DI float sqrt_spec(float a) {
    float y = __uint_as_float(0x5F3759DFu - (__float_as_uint(a) >> 1));
    const float h = 0.5f * a;
#pragma unroll
    for (int i = 0; i < 3; ++i) { float t = y * y; t = FMA(-h, t, 1.5f); y = y * t; }
    float s = a * y;
    const float r = FMA(-s, s, a);
    return FMA(r, 0.5f * y, s);
}
// SPEC.md §3.2 restated (the software form, whatever the handle's math_mode): sqrt_spec above is this y followed by one correction step
DI float rsqrt_spec(float a) {
    float y = __uint_as_float(0x5F3759DFu - (__float_as_uint(a) >> 1));
    const float h = 0.5f * a;
#pragma unroll
    for (int i = 0; i < 3; ++i) { float t = y * y; t = FMA(-h, t, 1.5f); y = y * t; }
    return y;
}
DI float erfinv_spec(float u) {
    float w = -log_spec(FMA(-u, u, 1.0f));
    float p;
    if (w < 5.0f) {
        w = w - 2.5f;
        p = 2.81022636e-08f;
        p = FMA(p, w, 3.43273939e-07f);
        p = FMA(p, w, -3.5233877e-06f);
        p = FMA(p, w, -4.39150654e-06f);
        p = FMA(p, w, 0.00021858087f);
        p = FMA(p, w, -0.00125372503f);
        p = FMA(p, w, -0.00417768164f);
        p = FMA(p, w, 0.246640727f);
        p = FMA(p, w, 1.50140941f);
    } else {
        w = sqrt_spec(w) - 3.0f;
        p = -0.000200214257f;
        p = FMA(p, w, 0.000100950558f);
        p = FMA(p, w, 0.00134934322f);
        p = FMA(p, w, -0.00367342844f);
        p = FMA(p, w, 0.00573950773f);
        p = FMA(p, w, -0.0076224613f);
        p = FMA(p, w, 0.00943887047f);
        p = FMA(p, w, 1.00167406f);
        p = FMA(p, w, 2.83297682f);
    }
    return p * u;
}
DI float bits_to_normal(uint32_t bits) {
    const float lo = -0.99999994f;
    const float f = __uint_as_float((bits >> 9) | 0x3F800000u) - 1.0f;
    float u = FMA(f, 2.0f, lo);
    if (!(u > lo)) u = lo;
    return 1.41421354f * erfinv_spec(u);
}

}  // namespace sdempc
#include "sdempc_tube.inc.h"
#include "sdempc_risk.inc.h"
#include "sdempc_band.inc.h"
#include "sdempc_outcome.inc.h"
#include "sdempc_geo.inc.h"
#include "sdempc_ensemble.inc.h"
#include "sdempc_retire.inc.h"
namespace sdempc {

// grid: x = chunks of 256 threads over [pg][r][lane] (pg < ceil(ceil(P/2)/32), r < H*6), y = instance
// SPEC.md §12 (T.traj given; keys, out and HC are then not read): the TUBE form of the launch — x = tiles of 32 columns of the particle x horizon tensor, y = instance
// (sdempc_tube.inc.h). T.traj null (every noise launch): not one access more.
// SPEC.md §12a (R.traj given; keys, out, HC and T are then not read): the RISK form — x = 1, y = instance, dynamic LDS of risk_lds_words_host words.
// R.traj null (every noise and tube launch): not one access more. The second launch bound asks for the 8 waves / SIMD the kernel had before this form: its scalar
// registers stay below 96 (the risk form's later-phase arguments are spilled to lanes of a vector register outside its loops), scratch stays 0.
// SPEC.md §12b (Q.traj given; keys, out, HC, T and R are then not read): the BANDS form — the tube's grid, x = tiles of 32 columns, y = instance (sdempc_band.inc.h).
// Q.traj null (every noise, tube and risk launch): not one access more.
// SPEC.md §12c (W.traj given; keys, out, HC, T, R and Q are then not read): the OUTCOME form — x = 1, y = instance, dynamic LDS of outcome_lds_words_host words
// (sdempc_outcome.inc.h). W.traj null (every noise, tube, risk and bands launch): not one access more.
__global__ void __launch_bounds__(256, 8) sdempc_noise_kernel(const uint32_t* __restrict__ keys, float* __restrict__ out, int P, int G, int HC, int b0, TubeArgs T,
                                                           RiskArgs R, BandArgs Q, OutcomeArgs W) {
    const int b = b0 + blockIdx.y;
    // (wave-uniform; ONE test of all mode pointers, so that the noise form waits for one batch of scalar loads and takes one branch, as it did with one mode —
    // its workgroups are short, and a second dependent load in front of `keys` showed in its time)
    if (__builtin_expect((reinterpret_cast<uintptr_t>(T.traj) | reinterpret_cast<uintptr_t>(R.traj) | reinterpret_cast<uintptr_t>(Q.traj) |
                          reinterpret_cast<uintptr_t>(W.traj)) != 0, 0)) {
        // (the outcome form LAST, and read in place, not from W: in front of the others it cost the bands form a second register of spilled scalars — profiles/outcome_resources.txt)
        if (Q.traj) band_reduce(Q, P, G, b);
        else if (R.traj) risk_reduce(R, P, G, b);
        else if (T.traj) tube_reduce(T, P, G, b);
        else outcome_reduce(P, G, b);
        return;
    }
    const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
    const unsigned N = (unsigned)P * (unsigned)HC, half = N / 2;          // N is even (HC = 6H)
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = k & 31u, r = (k >> 5) % (unsigned)HC, pg = (k >> 5) / (unsigned)HC;
    const unsigned p = pg * 32u + lane;
    const unsigned e0 = p * (unsigned)HC + r;
    if (p >= (unsigned)P || e0 >= half) return;
    uint32_t x0 = e0, x1 = e0 + half;
    threefry2x32(k0, k1, x0, x1);
    float* ob = out + (size_t)b * G * HC * 32;
    ob[((size_t)(p >> 5) * HC + r) * 32 + (p & 31u)] = bits_to_normal(x0);
    const unsigned e1 = e0 + half, p1 = e1 / (unsigned)HC, r1 = e1 - p1 * (unsigned)HC;
    ob[((size_t)(p1 >> 5) * HC + r1) * 32 + (p1 & 31u)] = bits_to_normal(x1);
}

hipError_t launch_noise_from_keys(const uint32_t* keys_dev, float* out, int B, int P, int G, int H, hipStream_t st) {
    if (B < 1 || P < 1 || H < 1 || G != (P + 31) / 32 || (long long)P * H * 6 >= (1ll << 31)) return hipErrorInvalidValue;
    const int HC = H * 6;
    if (P & 31) {   // padded particles of the last group read as zero noise
        hipError_t e = hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * G * HC * 32, st);
        if (e != hipSuccess) return e;
    }
    const int np1 = (P + 1) / 2, npg = (np1 + 31) / 32;
    const long long threads = (long long)npg * 32 * HC;
    const unsigned gx = (unsigned)((threads + 255) / 256);
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        sdempc_noise_kernel<<<dim3(gx, nb), 256, 0, st>>>(keys_dev, out, P, G, HC, b0, TubeArgs{}, RiskArgs{}, BandArgs{}, OutcomeArgs{});
    }
    return hipGetLastError();
}

// SPEC.md §12: one workgroup per (tile of 32 columns, instance); every word of every plane given is written
hipError_t launch_tube(const TubeArgs& T, int B, int P, int G, int H, hipStream_t st) {
    if (B < 1 || P < 1 || H < 1 || G != (P + 31) / 32 || !T.traj || T.C != (H + 1) * 13) return hipErrorInvalidValue;
    if (!T.mean && !T.var && !T.mn && !T.mx && !T.outside) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)((T.C + 31) / 32);
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        sdempc_noise_kernel<<<dim3(gx, nb), 256, 0, st>>>(nullptr, nullptr, P, G, 0, b0, T, RiskArgs{}, BandArgs{}, OutcomeArgs{});
    }
    return hipGetLastError();
}

// SPEC.md §12a: one workgroup per instance; every word of every output given is written
hipError_t launch_risk(const RiskArgs& R, int B, int P, int G, hipStream_t st) {
    if (B < 1 || P < 1 || R.H < 1 || G != (P + 31) / 32 || !R.traj) return hipErrorInvalidValue;
    const bool want_x = R.exit || R.first_exit || R.outside_any, want_j = R.jx || R.jstat || R.jq || R.jtail;
    if (!want_x && !want_j) return hipErrorInvalidValue;
    if ((want_x && (!R.lo || !R.hi)) || (!want_x && R.lo) || (want_j && (!R.xref || !R.disc)) || (R.sc_n && !R.sc_tab)) return hipErrorInvalidValue;
    if (R.jq && (R.n_ranks < 1 || R.n_ranks > RISK_MAX_RANKS)) return hipErrorInvalidValue;
    for (int k = 0; R.jq && k < R.n_ranks; ++k)
        if (R.ranks[k] < 0 || R.ranks[k] >= P) return hipErrorInvalidValue;
    if (R.jtail && (R.tail_k < 1 || R.tail_k > P)) return hipErrorInvalidValue;
    if ((R.jq || R.jtail) && P > RISK_RANK_MAX_P) return hipErrorInvalidValue;
    const size_t lds = sizeof(uint32_t) * risk_lds_words_host(R.H, G);
    if (lds > RISK_MAX_LDS) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        sdempc_noise_kernel<<<dim3(1, nb), 256, lds, st>>>(nullptr, nullptr, P, G, 0, b0, TubeArgs{}, R, BandArgs{}, OutcomeArgs{});
    }
    return hipGetLastError();
}

// SPEC.md §12b: the tube's grid; every word of every output given is written
hipError_t launch_bands(const BandArgs& N, int B, int P, int G, int H, hipStream_t st) {
    if (B < 1 || P < 1 || H < 1 || G != (P + 31) / 32 || !N.traj || N.C != (H + 1) * 13) return hipErrorInvalidValue;
    if (!N.q && !N.below && !N.at) return hipErrorInvalidValue;
    if ((N.below || N.at) && !N.obs) return hipErrorInvalidValue;
    if (N.q && (N.n_ranks < 1 || N.n_ranks > BAND_MAX_RANKS)) return hipErrorInvalidValue;
    for (int k = 0; N.q && k < N.n_ranks; ++k)
        if (N.ranks[k] < 0 || N.ranks[k] >= P) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)((N.C + 31) / 32);
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        sdempc_noise_kernel<<<dim3(gx, nb), 256, 0, st>>>(nullptr, nullptr, P, G, 0, b0, TubeArgs{}, RiskArgs{}, N, OutcomeArgs{});
    }
    return hipGetLastError();
}

// SPEC.md §12c: one workgroup per instance; every word of every output given is written
hipError_t launch_outcome(const OutcomeArgs& W, int B, int P, int G, hipStream_t st) {
    if (B < 1 || P < 1 || W.H < 1 || G != (P + 31) / 32 || !W.traj || !W.tgt) return hipErrorInvalidValue;
    if (!W.words && !W.fail_step && !W.first_fail && !W.cause_ever && !W.chan_stat && !W.chan_q && !W.agg_stat && !W.agg_q) return hipErrorInvalidValue;
    if (W.r2_pos != W.r2_pos || W.cos_min != W.cos_min || W.w2_max != W.w2_max) return hipErrorInvalidValue;
    if ((W.tgt_tstride != 0 && W.tgt_tstride != 13) || (W.tgt_bstride != 0 && W.tgt_bstride != 13 && W.tgt_bstride != (W.H + 1) * 13)) return hipErrorInvalidValue;
    const bool want_q = W.chan_q || W.agg_q;
    if (want_q ? (W.n_ranks < 1 || W.n_ranks > OUTCOME_MAX_RANKS) : W.n_ranks != 0) return hipErrorInvalidValue;
    for (int k = 0; k < W.n_ranks; ++k)
        if (W.ranks[k] < 0 || W.ranks[k] >= P) return hipErrorInvalidValue;
    if (want_q && P > OUTCOME_RANK_MAX_P) return hipErrorInvalidValue;
    const size_t lds = sizeof(uint32_t) * outcome_lds_words_host(W.H, G);
    if (lds > RISK_MAX_LDS) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        sdempc_noise_kernel<<<dim3(1, nb), 256, lds, st>>>(nullptr, nullptr, P, G, 0, b0, TubeArgs{}, RiskArgs{}, BandArgs{}, W);
    }
    return hipGetLastError();
}

// ---- closed loop (SPEC.md §11): the key schedule of one tick, on device-resident keys ----
// split(r, 2) = random_bits(r, 4): counters (0, 2) and (1, 3) give the words [y0(0), y0(1), y1(0), y1(1)]; the first key is
// {y0(0), y0(1)}, the second {y1(0), y1(1)}.
DI void split2(uint32_t k0, uint32_t k1, uint32_t* first, uint32_t* second) {
    uint32_t a0 = 0u, a1 = 2u, c0 = 1u, c1 = 3u;
    threefry2x32(k0, k1, a0, a1);
    threefry2x32(k0, k1, c0, c1);
    first[0] = a0; first[1] = c0;
    second[0] = a1; second[1] = c1;
}
// SPEC.md §11h: (u32) of a telemetry count — the value itself where 0 <= v < 2^32, else 0 (a NaN among them)
DI uint32_t score_u32(float v) { return v >= 0.0f && v < 4294967296.0f ? (uint32_t)v : 0u; }
// one thread per episode: (r', s) = split(r_k), (r_{k+1}, p) = split(r'), xi_k = normal(p, (6,)) (random_bits(p, 6) pairs counter i with
// i + 3). keys: r_k in, r_{k+1} out; sub: s (the solve's noise key); xi: [B][6]
__global__ void __launch_bounds__(256) sdempc_loop_keys_kernel(uint32_t* __restrict__ keys, uint32_t* __restrict__ sub, float* __restrict__ xi, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    uint32_t r1[2], s[2], r2[2], p[2];
    split2(keys[2 * b], keys[2 * b + 1], r1, s);
    split2(r1[0], r1[1], r2, p);
    sub[2 * b] = s[0]; sub[2 * b + 1] = s[1];
    keys[2 * b] = r2[0]; keys[2 * b + 1] = r2[1];
#pragma unroll
    for (uint32_t i = 0; i < 3; ++i) {
        uint32_t x0 = i, x1 = i + 3u;
        threefry2x32(p[0], p[1], x0, x1);
        xi[6 * b + i] = bits_to_normal(x0);
        xi[6 * b + 3 + i] = bits_to_normal(x1);
    }
}

// SPEC.md §11a: the same schedule with n plant substeps per tick — xi_k = normal(p, (n, 6)), ONE draw of 6 n values (random_bits(p, 6 n) pairs
// counter i with i + 3 n: element i of the flat draw is the first word of block i, element 3 n + i the second). xi: [B][n][6]; n = 1 is the kernel above.
__global__ void __launch_bounds__(256) sdempc_loop_keys_sub_kernel(uint32_t* __restrict__ keys, uint32_t* __restrict__ sub, float* __restrict__ xi, int B, int n) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    uint32_t r1[2], s[2], r2[2], p[2];
    split2(keys[2 * b], keys[2 * b + 1], r1, s);
    split2(r1[0], r1[1], r2, p);
    sub[2 * b] = s[0]; sub[2 * b + 1] = s[1];
    keys[2 * b] = r2[0]; keys[2 * b + 1] = r2[1];
    const uint32_t half = 3u * (uint32_t)n;
    float* row = xi + (size_t)b * 2u * half;
    for (uint32_t i = 0; i < half; ++i) {
        uint32_t x0 = i, x1 = i + half;
        threefry2x32(p[0], p[1], x0, x1);
        row[i] = bits_to_normal(x0);
        row[half + i] = bits_to_normal(x1);
    }
}

hipError_t launch_loop_keys(uint32_t* keys_dev, uint32_t* sub_dev, float* xi_dev, int B, hipStream_t st, int substeps) {
    if (B < 1 || substeps < 1) return hipErrorInvalidValue;
    if (substeps == 1) sdempc_loop_keys_kernel<<<(B + 255) / 256, 256, 0, st>>>(keys_dev, sub_dev, xi_dev, B);
    else sdempc_loop_keys_sub_kernel<<<(B + 255) / 256, 256, 0, st>>>(keys_dev, sub_dev, xi_dev, B, substeps);
    return hipGetLastError();
}

// SPEC.md §11b: the schedule of one solve period of `ticks` control ticks. Tick 0 is the tick of the kernels above ((r', s) = split(r), (r, p) = split(r'));
// every later tick has no solve: (r, p) = split(r). Each tick draws normal(p, (n, 6)) as above. xi: [B][xi_ticks][n][6], rows 0 .. ticks-1 written.
// SPEC.md §11f (O.q given): the same thread first forms the measurement the period's solve starts from — (q, me) = split(q) on the observation chain, at every
// solve; unless the solve's valid flag is 0, xi = normal(me, (12,)) (random_bits(me, 12) pairs counter i with i + 6), e_i = fma(sigma_i, xi_i, beta_i), added to
// position, velocity and body rates, and the attitude multiplied by (1, e[6..8] / 2) from the right, not renormalised. O.q null: not one access more.
// SPEC.md §11g (O.age / O.renorm given): the state the measurement is formed from is A = age[b] plant substeps old — row age_max - A of the history (a per-thread
// gather; A = 0 reads O.x as before) — and the attitude of xm is scaled to unit length with the software rsqrt. O.age null and O.renorm 0: not one access more.
// SPEC.md §11h (Z.words given; ticks = 0, O empty, keys / sub / xi null and untouched): the SCORING form of the launch, one per chunk. Thread b walks the chunk's rows
// of its episode in time order — rows, then tick rows, then solve rows; the buffers are [row][B][.], so neighbouring threads read neighbouring rows — and carries
// the 16 score words of the episode in registers from Z.words[b] back to Z.words[b]. Z.words null (every period launch): not one access more.
// SPEC.md §11i (G.bias.chain / G.dist.chain given): the same thread steps the episode's Gauss-Markov processes — the bias process once, in front of the measurement,
// whose beta is then the row this thread has just written (dropout or not); the disturbance process once per tick, beside the schedule's tick loop, into row (i, b) of
// the period's disturbance rows. One step is one split, W / 2 blocks, and per component one multiply and one fma (kept apart: -ffp-contract=off). Both null: not one
// access more.
// SPEC.md §11k (E.drop.chain / E.fault.chain given): the same thread steps the episode's event chains, in integers alone — the dropout chain once, in front of the bias
// step and the measurement, whose valid flag is then the word this thread has just written (O.valid addresses it); the fault chain once per tick, beside the
// disturbance step, into row (i, b) of the period's fault rows. One step is one split, ceil(lanes / 2) blocks and per lane at most K + 1 compares; chain and
// per-motor states stay in registers at constant indices (motor loops unrolled to 8, as the scoring form's). Both null: not one access more.
// SPEC.md §11l (A.x given; ticks = 0, O / Z / G / E empty, keys / sub / xi null and untouched): the BASELINE form of the launch, one per solve period where the solve
// is launched otherwise. Thread b forms the geometric controller's command of episode b and fills the tables the plant launch reads (sdempc_geo.inc.h). A.x null
// (every period and scoring launch): not one access more.
// SPEC.md §11m (N.part given; ticks = 0, O / Z / G / E / A empty, keys / sub / xi null and untouched): the two ENSEMBLE forms of the launch, after a chunk's scoring
// launch (sdempc_ensemble.inc.h) — the partial form on a grid of (blocks of episodes) x (rows), whose threads past B stay for its workgroup barriers and are masked,
// and the combine form, one thread per (row, cohort, word): both leave before the `b >= B` return. N.part null (every launch before §11m): not one access more.
// SPEC.md §11n (Y.live given; ticks = 0, O / Z / G / E / A / N empty, keys / sub / xi null and untouched): the two LIVE-LIST forms of the launch, after a period's scoring
// launch (sdempc_retire.inc.h) — one thread per episode, threads past B stay for the workgroup barrier and are masked: both leave before the `b >= B` return. The
// scoring and baseline forms take a mask of the same flags (Z.live, A.live). Y.live, Z.live and A.live null (every launch before §11n): not one access more.
__global__ void __launch_bounds__(256) sdempc_loop_keys_period_kernel(uint32_t* __restrict__ keys, uint32_t* __restrict__ sub, float* __restrict__ xi, int B, int ticks,
                                                                      int xi_ticks, int n, LoopObserve O, LoopScore Z, LoopProcess G, LoopEvents E,
                                                                      LoopBaseline A, LoopEnsemble N, LoopRetire Y) {
    if (N.part) {                                        // (wave-uniform)
        if (N.combine) ens_combine(N);
        else ens_partial(N, B);
        return;
    }
    if (Y.live) {                                        // (wave-uniform)
        retire_live_list(Y, B);
        return;
    }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    if (A.x) {                                           // (wave-uniform)
        if (A.live && A.live[b] == 0) {                  // SPEC.md §11n: a retired episode keeps its tables; its info row is the held one
            float* inf = A.info + (size_t)b * 8;
            inf[0] = 0.0f; inf[1] = A.step[b];
#pragma unroll
            for (int c = 2; c < 8; ++c) inf[c] = 0.0f;
            return;
        }
        geo_fill(A, b);
        return;
    }
    if (Z.words) {                                       // (wave-uniform)
        if (Z.live && Z.live[b] == 0) return;            // SPEC.md §11n: a retired episode's words are frozen
        uint32_t* w = Z.words + (size_t)b * 16;
        uint32_t cnt = w[0], imax = w[3], first = w[8], causes = w[9], nbad = w[10];
        float sdp = __uint_as_float(w[1]), mdp = __uint_as_float(w[2]), ldp = __uint_as_float(w[4]), sdv = __uint_as_float(w[5]);
        float minc = __uint_as_float(w[6]), mw2 = __uint_as_float(w[7]);
        for (int i = 0; i < Z.ticks; ++i) {
            const float* g = Z.ref + (size_t)i * Z.ref_tick_stride + (size_t)b * Z.ref_ep_stride;
            const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3], g4 = g[4], g5 = g[5];
            for (int jj = 0; jj < Z.rows_per_tick; ++jj) {
                const float* x = Z.rows + ((size_t)(i * Z.rows_per_tick + jj) * B + b) * 13;
                bool nf;
                float dp, dv, c, w2;                     // (the row's quantities, stated once for this form and the ensemble forms: sdempc_ensemble.inc.h)
                const uint32_t cause = score_row(x, g0, g1, g2, g3, g4, g5, Z.r2_pos, Z.cos_min, Z.w2_max, dp, dv, c, w2, nf);
                sdp = sdp + dp;
                if (dp > mdp) { mdp = dp; imax = cnt; }
                ldp = dp;
                sdv = sdv + dv;
                if (c < minc) minc = c;
                if (w2 > mw2) mw2 = w2;
                if (cause) {
                    if (first == 0xffffffffu) first = cnt;
                    causes |= cause;
                    nbad += 1u;
                }
                cnt += 1u;
            }
        }
        w[0] = cnt; w[1] = __float_as_uint(sdp); w[2] = __float_as_uint(mdp); w[3] = imax; w[4] = __float_as_uint(ldp); w[5] = __float_as_uint(sdv);
        w[6] = __float_as_uint(minc); w[7] = __float_as_uint(mw2); w[8] = first; w[9] = causes; w[10] = nbad;
        uint32_t sat = w[11];
        float sdu = __uint_as_float(w[12]);
        for (int i = 0; i < Z.ticks; ++i) {
            const float* u = Z.us + ((size_t)i * B + b) * Z.m;
            float a = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j)                  // (constant indices into the argument: no copy of it in scratch)
                if (j < Z.m) {
                    const float uj = u[j], d = uj - Z.uref[j];
                    if (uj <= Z.u_lo[j] || uj >= Z.u_hi[j]) sat += 1u;
                    a = FMA(d, d, a);
                }
            sdu = sdu + a;
        }
        w[11] = sat; w[12] = __float_as_uint(sdu);
        uint32_t nit = w[13], nls = w[14], flat = w[15];
        for (int j = 0; j < Z.solves; ++j) {
            const float* inf = Z.info + ((size_t)j * B + b) * 8;
            nit += score_u32(inf[2]);
            nls += score_u32(inf[7]);
            if (!(inf[6] < inf[5])) flat += 1u;
        }
        w[13] = nit; w[14] = nls; w[15] = flat;
        return;
    }
    if (E.drop.chain) {                                  // (wave-uniform)
        const LoopEventDrop& Ed = E.drop;
        uint32_t c2[2], ek[2];
        split2(Ed.chain[2 * b], Ed.chain[2 * b + 1], c2, ek);
        Ed.chain[2 * b] = c2[0]; Ed.chain[2 * b + 1] = c2[1];
        uint32_t w = 0u, pad = 0u;                       // random_bits(e, 1): the first word of block (0, 0)
        threefry2x32(ek[0], ek[1], w, pad);
        const int s = Ed.state[2 * b];
        const int sn = s == 0 ? (w < Ed.drop[(size_t)b * Ed.par_ep_stride] ? 1 : 0) : (w < Ed.recover[(size_t)b * Ed.par_ep_stride] ? 0 : 1);
        Ed.state[2 * b] = sn; Ed.state[2 * b + 1] += sn;
        const int scheduled = Ed.sched ? Ed.sched[(size_t)b * Ed.sched_ep_stride] : 1;
        Ed.dst[b] = sn == 0 && scheduled != 0 ? 1 : 0;
    }
    const float* pbeta = nullptr;                    // this solve's beta where the bias process wrote it
    if (G.bias.chain) {                                  // (wave-uniform)
        const LoopProcessHalf& Pb = G.bias;
        uint32_t c2[2], ek[2];
        split2(Pb.chain[2 * b], Pb.chain[2 * b + 1], c2, ek);
        Pb.chain[2 * b] = c2[0]; Pb.chain[2 * b + 1] = c2[1];
        float* g = Pb.state + (size_t)b * 12;
        const float* rh = Pb.rho + (size_t)b * Pb.par_ep_stride;
        const float* sc = Pb.scale + (size_t)b * Pb.par_ep_stride;
        const float* d = Pb.sched ? Pb.sched + (size_t)b * Pb.sched_ep_stride : nullptr;
        float* row = Pb.dst + (size_t)b * 12;
#pragma unroll
        for (uint32_t i = 0; i < 6; ++i) {
            uint32_t x0 = i, x1 = i + 6u;
            threefry2x32(ek[0], ek[1], x0, x1);
            const float t0 = sc[i] * bits_to_normal(x0), t1 = sc[i + 6] * bits_to_normal(x1);
            const float g0 = FMA(rh[i], g[i], t0), g1 = FMA(rh[i + 6], g[i + 6], t1);
            g[i] = g0; g[i + 6] = g1;
            row[i] = d ? d[i] + g0 : g0;
            row[i + 6] = d ? d[i + 6] + g1 : g1;
        }
        pbeta = row;
    }
    if (O.q) {
        uint32_t q2[2], me[2];
        split2(O.q[2 * b], O.q[2 * b + 1], q2, me);
        O.q[2 * b] = q2[0]; O.q[2 * b + 1] = q2[1];
        float* xm = O.xm + (size_t)b * 13;
        if (!O.valid || O.valid[(size_t)b * O.valid_ep_stride] != 0) {
            const float* x = O.x + (size_t)b * 13;
            if (O.age) {
                const int A = O.age[(size_t)b * O.age_ep_stride];
                if (A > 0) x = O.hist + (size_t)(O.age_max - A) * O.hist_row_stride + (size_t)b * 13;
            }
            const float* sg = O.sigma ? O.sigma + (size_t)b * O.ep_stride : nullptr;
            const float* bt = pbeta ? pbeta : O.beta ? O.beta + (size_t)b * O.ep_stride : nullptr;
            float e[12];
#pragma unroll
            for (uint32_t i = 0; i < 6; ++i) {
                uint32_t x0 = i, x1 = i + 6u;
                threefry2x32(me[0], me[1], x0, x1);
                e[i] = FMA(sg ? sg[i] : 0.0f, bits_to_normal(x0), bt ? bt[i] : 0.0f);
                e[i + 6] = FMA(sg ? sg[i + 6] : 0.0f, bits_to_normal(x1), bt ? bt[i + 6] : 0.0f);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                xm[i] = x[i] + e[i];
                xm[3 + i] = x[3 + i] + e[3 + i];
                xm[10 + i] = x[10 + i] + e[9 + i];
            }
            const float h0 = 0.5f * e[6], h1 = 0.5f * e[7], h2 = 0.5f * e[8];
            const float qw = x[6], qx = x[7], qy = x[8], qz = x[9];
            xm[6] = FMA(-qz, h2, FMA(-qy, h1, FMA(-qx, h0, qw)));
            xm[7] = FMA(-qz, h1, FMA(qy, h2, FMA(qw, h0, qx)));
            xm[8] = FMA(-qx, h2, FMA(qz, h0, FMA(qw, h1, qy)));
            xm[9] = FMA(-qy, h0, FMA(qx, h1, FMA(qw, h2, qz)));
            if (O.renorm) {                              // (wave-uniform)
                const float q0 = xm[6], q1 = xm[7], q2 = xm[8], q3 = xm[9];
                const float r = rsqrt_spec(FMA(q3, q3, FMA(q2, q2, FMA(q1, q1, q0 * q0))));
                xm[6] = q0 * r; xm[7] = q1 * r; xm[8] = q2 * r; xm[9] = q3 * r;
            }
        }
        float* row = O.xmeas + (size_t)b * 13;       // (a dropout: the held row; xm was written by this thread or before this launch)
#pragma unroll
        for (int i = 0; i < 13; ++i) row[i] = xm[i];
    }
    uint32_t r[2] = {keys[2 * b], keys[2 * b + 1]};
    const uint32_t half = 3u * (uint32_t)n;
    const LoopProcessHalf& Pd = G.dist;
    uint32_t dc[2] = {0u, 0u};
    float dg[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // (constant indices after unrolling: registers)
    if (Pd.chain) {                                      // (wave-uniform)
        dc[0] = Pd.chain[2 * b]; dc[1] = Pd.chain[2 * b + 1];
#pragma unroll
        for (int e = 0; e < 6; ++e) dg[e] = Pd.state[(size_t)b * 6 + e];
    }
    const LoopEventFault& Ef = E.fault;
    uint32_t fc[2] = {0u, 0u};
    // the states of the m <= 8 motors, three bits each (s <= 4), in ONE register; `first` stays in memory, written by the step that leaves state 0 for the first time
    uint32_t fp = 0u;
    // (one row per episode, chain and states, and one row of parameters: every access below is one of two pointers plus a constant, so no address is formed per motor
    // and mode and none can be kept in registers across the tick loop)
    uint32_t* fe = Ef.chain ? Ef.chain + (size_t)b * EVENT_EP_WORDS : nullptr;
    if (Ef.chain) {                                      // (wave-uniform)
        fc[0] = fe[0]; fc[1] = fe[1];
#pragma unroll
        for (int l = 0; l < 8; ++l)
            if (l < Ef.m) fp |= fe[2 + 2 * l] << (3 * l);
    }
    for (int i = 0; i < ticks; ++i) {
        if (Ef.chain) {
            uint32_t c2[2], ek[2];
            split2(fc[0], fc[1], c2, ek);
            fc[0] = c2[0]; fc[1] = c2[1];
            const int K = Ef.K, m = Ef.m, hf = (m + 1) >> 1;
            const uint32_t* on = Ef.par + (size_t)b * Ef.par_ep_stride;      // onset u32[8][4], clear u32[8][4], modes f32[8][4][2]
            const uint32_t* cr = on + 32;
            const uint32_t* md = on + 64;                        // (the rows are copied as words: no arithmetic is done on them)
            const uint32_t sch = (uint32_t)i * (uint32_t)Ef.sched_tick_stride + (uint32_t)b * (uint32_t)Ef.sched_ep_stride;
            const uint32_t out = ((uint32_t)i * (uint32_t)B + (uint32_t)b) * (uint32_t)m * 2u;
#pragma unroll
            for (int l = 0; l < 8; ++l)
                if (l < m) {
                    // word l of random_bits(e, m): the first word of block l where l < hf, else the second of block l - hf (whose first counter is l - hf; an odd
                    // m's last block pairs with a zero counter). Each lane runs its own block: a second pass over a block costs less than holding m words.
                    const int k = l < hf ? l : l - hf;
                    uint32_t x0 = (uint32_t)k, x1 = k + hf < m ? (uint32_t)(k + hf) : 0u;
                    threefry2x32(ek[0], ek[1], x0, x1);
                    const uint32_t w = l < hf ? x0 : x1;
                    const uint32_t s = (fp >> (3 * l)) & 7u;
                    uint32_t sn;
                    if (s == 0u) {
                        uint32_t cnt = 0u;                   // thresholds at or below the word: the smallest j with w < onset[j], the row being nondecreasing
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < K && w >= on[l * 4 + j]) cnt += 1u;
                        sn = cnt < (uint32_t)K ? cnt + 1u : 0u;
                        if (sn > 0u && (int32_t)fe[3 + 2 * l] < 0) fe[3 + 2 * l] = (uint32_t)(Ef.tick0 + i);
                    } else sn = w < cr[l * 4 + (int)s - 1] ? 0u : s;
                    fp = (fp & ~(7u << (3 * l))) | sn << (3 * l);
                    uint32_t r0 = 0x3f800000u, r1 = 0u;          // the neutral row (1, 0)
                    if (sn > 0u) {
                        const uint32_t* mode = md + (l * 4 + (int)sn - 1) * 2;
                        r0 = mode[0]; r1 = mode[1];
                    } else if (Ef.sched) { r0 = Ef.sched[sch + 2u * l]; r1 = Ef.sched[sch + 2u * l + 1u]; }
                    Ef.dst[out + 2u * l] = r0; Ef.dst[out + 2u * l + 1u] = r1;
                }
        }
        if (Pd.chain) {
            uint32_t c2[2], ek[2];
            split2(dc[0], dc[1], c2, ek);
            dc[0] = c2[0]; dc[1] = c2[1];
            const float* rh = Pd.rho + (size_t)b * Pd.par_ep_stride;
            const float* sc = Pd.scale + (size_t)b * Pd.par_ep_stride;
            const float* d = Pd.sched ? Pd.sched + (size_t)i * Pd.sched_tick_stride + (size_t)b * Pd.sched_ep_stride : nullptr;
            float* row = Pd.dst + ((size_t)i * B + b) * 6;
#pragma unroll
            for (uint32_t e = 0; e < 3; ++e) {
                uint32_t x0 = e, x1 = e + 3u;
                threefry2x32(ek[0], ek[1], x0, x1);
                const float t0 = sc[e] * bits_to_normal(x0), t1 = sc[e + 3] * bits_to_normal(x1);
                dg[e] = FMA(rh[e], dg[e], t0);
                dg[e + 3] = FMA(rh[e + 3], dg[e + 3], t1);
                row[e] = d ? d[e] + dg[e] : dg[e];
                row[e + 3] = d ? d[e + 3] + dg[e + 3] : dg[e + 3];
            }
        }
        uint32_t r2[2], p[2];
        if (i == 0) {
            uint32_t r1[2], s[2];
            split2(r[0], r[1], r1, s);
            sub[2 * b] = s[0]; sub[2 * b + 1] = s[1];
            split2(r1[0], r1[1], r2, p);
        } else split2(r[0], r[1], r2, p);
        r[0] = r2[0]; r[1] = r2[1];
        float* row = xi + ((size_t)b * xi_ticks + i) * 2u * half;
        for (uint32_t e = 0; e < half; ++e) {
            uint32_t x0 = e, x1 = e + half;
            threefry2x32(p[0], p[1], x0, x1);
            row[e] = bits_to_normal(x0);
            row[half + e] = bits_to_normal(x1);
        }
    }
    keys[2 * b] = r[0]; keys[2 * b + 1] = r[1];
    if (Pd.chain) {
        Pd.chain[2 * b] = dc[0]; Pd.chain[2 * b + 1] = dc[1];
#pragma unroll
        for (int e = 0; e < 6; ++e) Pd.state[(size_t)b * 6 + e] = dg[e];
    }
    if (Ef.chain) {
        fe[0] = fc[0]; fe[1] = fc[1];
#pragma unroll
        for (int l = 0; l < 8; ++l)
            if (l < Ef.m) fe[2 + 2 * l] = (fp >> (3 * l)) & 7u;
    }
}

hipError_t launch_loop_keys_period(uint32_t* keys_dev, uint32_t* sub_dev, float* xi_dev, int B, int ticks, int xi_ticks, int substeps, hipStream_t st, const LoopObserve& O,
                                   const LoopScore& Z, const LoopProcess& G, const LoopEvents& E, const LoopBaseline& A, const LoopEnsemble& N, const LoopRetire& Y) {
    if (B < 1 || substeps < 1 || ticks < 0 || xi_ticks < ticks) return hipErrorInvalidValue;
    if (Y.live) {   // SPEC.md §11n: a present block is complete and stands alone
        if (ticks != 0 || N.part || Z.words || A.x || O.q || O.age || O.renorm || keys_dev || sub_dev || xi_dev || G.dist.chain || G.bias.chain || E.fault.chain || E.drop.chain) return hipErrorInvalidValue;
        if (!Y.blk || Y.nblk != (B + 255) / 256 || (Y.place != 0 && Y.place != 1) || (Y.init != 0 && Y.init != 1)) return hipErrorInvalidValue;
        if (Y.place ? (!Y.list || !Y.n_live || Y.init) : (!Y.words || !Y.retired_at || Y.rows < 0 || Y.solve < -1)) return hipErrorInvalidValue;
        sdempc_loop_keys_period_kernel<<<(unsigned)Y.nblk, 256, 0, st>>>(nullptr, nullptr, nullptr, B, 0, 0, substeps, O, Z, G, E, A, N, Y);
        return hipGetLastError();
    }
    if (N.part) {   // SPEC.md §11m: a present block is complete, stands alone, and addresses rows the chunk's scoring launch counted
        if (ticks != 0 || Z.words || A.x || O.q || O.age || O.renorm || keys_dev || sub_dev || xi_dev || G.dist.chain || G.bias.chain || E.fault.chain || E.drop.chain) return hipErrorInvalidValue;
        if (!N.out || !N.words || !N.cohort || !N.rows || !N.ref || (N.E > 0 && !N.edges)) return hipErrorInvalidValue;
        if (N.G < 1 || N.G > ENS_MAX_COHORTS || N.E < 0 || N.E > ENS_MAX_EDGES || (N.over != 0 && N.over != 1) || (N.combine != 0 && N.combine != 1)) return hipErrorInvalidValue;
        if (N.rows_per_tick < 1 || N.row0 < 0 || N.nrows < 1 || N.nrows > 65535 || N.row0 + N.nrows > N.chunk_rows || N.nblk != (B + 255) / 256) return hipErrorInvalidValue;
        if ((N.ref_tick_stride != 0 && N.ref_tick_stride < 13) || (N.ref_ep_stride != 0 && N.ref_ep_stride != 13)) return hipErrorInvalidValue;
        if (N.r2_pos != N.r2_pos || N.cos_min != N.cos_min || N.w2_max != N.w2_max) return hipErrorInvalidValue;
        if (N.combine) {
            const long long threads = (long long)N.nrows * N.G * (ENS_BASE_WORDS + 4 * N.E);
            sdempc_loop_keys_period_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(nullptr, nullptr, nullptr, B, 0, 0, substeps, O, Z, G, E, A, N, LoopRetire{});
        } else sdempc_loop_keys_period_kernel<<<dim3((unsigned)N.nblk, (unsigned)N.nrows), 256, 0, st>>>(nullptr, nullptr, nullptr, B, 0, 0, substeps, O, Z, G, E, A, N, LoopRetire{});
        return hipGetLastError();
    }
    // ticks = 0 is the scoring form or the baseline form and nothing else: score words or a state, no observation, no key buffers
    if ((ticks == 0) != (Z.words != nullptr || A.x != nullptr) || (Z.words && A.x)) return hipErrorInvalidValue;
    if (A.x) {      // SPEC.md §11l: a present block is complete and addresses rows inside the window
        if (O.q || O.age || O.renorm || keys_dev || sub_dev || xi_dev || G.dist.chain || G.bias.chain || E.fault.chain || E.drop.chain) return hipErrorInvalidValue;
        if (!A.xref || !A.par || A.H < 1 || A.m < 1 || A.m > 8 || A.ref_row < 0 || A.ref_row > A.H - 1) return hipErrorInvalidValue;
        if ((A.xref_ep_stride != 0 && A.xref_ep_stride != (A.H + 1) * 13) || (A.par_ep_stride != 0 && A.par_ep_stride != GEO_PAR_WORDS)) return hipErrorInvalidValue;
        if ((A.accel_ff != 0 && A.accel_ff != 1) || A.inv_dt != A.inv_dt) return hipErrorInvalidValue;
        if (!A.out && (!A.uopt || !A.xevol || !A.info || !A.step)) return hipErrorInvalidValue;
    }
    if (Z.words) {
        if (O.q || O.age || O.renorm || keys_dev || sub_dev || xi_dev || G.dist.chain || G.bias.chain || E.fault.chain || E.drop.chain) return hipErrorInvalidValue;
        if (!Z.rows || !Z.us || !Z.info || !Z.ref || Z.ticks < 1 || Z.solves < 1 || Z.solves > Z.ticks || Z.rows_per_tick < 1 || Z.m < 1 || Z.m > 8) return hipErrorInvalidValue;
        if ((Z.ref_tick_stride != 0 && Z.ref_tick_stride < 13) || (Z.ref_ep_stride != 0 && Z.ref_ep_stride != 13)) return hipErrorInvalidValue;
        if (Z.r2_pos != Z.r2_pos || Z.cos_min != Z.cos_min || Z.w2_max != Z.w2_max) return hipErrorInvalidValue;
    } else if (!A.x && (!keys_dev || !sub_dev || !xi_dev)) return hipErrorInvalidValue;
    if (O.q && (!O.x || !O.xm || !O.xmeas || (O.ep_stride != 0 && O.ep_stride != 12) || (O.valid_ep_stride != 0 && O.valid_ep_stride != 1))) return hipErrorInvalidValue;
    if ((O.age || O.renorm) && !O.q) return hipErrorInvalidValue;
    if (O.age && (!O.hist || O.age_max < 1 || O.hist_row_stride < B * 13 || (O.age_ep_stride != 0 && O.age_ep_stride != 1))) return hipErrorInvalidValue;
    // SPEC.md §11i: a present half is complete, its strides are W or 0 (Bd * W or 0 between steps), and the bias half replaces O.beta of an observation
    for (int w = 0; w < 2; ++w) {
        const LoopProcessHalf& P = w ? G.bias : G.dist;
        const int W = w ? 12 : 6;
        if (!P.chain) continue;
        if (!P.state || !P.rho || !P.scale || !P.dst || (P.par_ep_stride != 0 && P.par_ep_stride != W)) return hipErrorInvalidValue;
        if (P.sched && ((P.sched_ep_stride != 0 && P.sched_ep_stride != W) || (P.sched_tick_stride != 0 && P.sched_tick_stride < W))) return hipErrorInvalidValue;
    }
    if (G.bias.chain && (!O.q || O.beta)) return hipErrorInvalidValue;
    // SPEC.md §11k: a present half is complete; the fault half's counts and clock are in range, the dropout half writes the flags the observation reads
    if (E.fault.chain) {
        const LoopEventFault& F = E.fault;
        if (!F.par || !F.dst || F.K < 1 || F.K > 4 || F.m < 1 || F.m > 8) return hipErrorInvalidValue;
        if ((F.par_ep_stride != 0 && F.par_ep_stride != EVENT_PAR_WORDS) || F.tick0 < 0 || (long long)F.tick0 + ticks > (1ll << 24)) return hipErrorInvalidValue;
        if (F.sched && ((F.sched_ep_stride != 0 && F.sched_ep_stride != 2 * F.m) || (F.sched_tick_stride != 0 && F.sched_tick_stride < 2 * F.m))) return hipErrorInvalidValue;
    }
    if (E.drop.chain) {
        const LoopEventDrop& D = E.drop;
        if (!D.state || !D.drop || !D.recover || !D.dst || (D.par_ep_stride != 0 && D.par_ep_stride != 1)) return hipErrorInvalidValue;
        if (D.sched && D.sched_ep_stride != 0 && D.sched_ep_stride != 1) return hipErrorInvalidValue;
        if (!O.q || O.valid != D.dst || O.valid_ep_stride != 1) return hipErrorInvalidValue;
    }
    sdempc_loop_keys_period_kernel<<<(B + 255) / 256, 256, 0, st>>>(keys_dev, sub_dev, xi_dev, B, ticks, xi_ticks, substeps, O, Z, G, E, A, LoopEnsemble{}, LoopRetire{});
    return hipGetLastError();
}

// SPEC.md §11j: one row of episode b's trajectory at clock value u, into y[13] (constant indices after unrolling: registers). Every multiply and fma is the one
// written (-ffp-contract=off). The segment search is this thread's own: it may diverge inside a wave. Whatever tau is (a NaN among it: an overflowing rate), the
// segment index stays inside the table.
DI void track_row(const LoopTrack& K, int b, float u, float* y) {
    const int tb = K.table_of[b];
    const int f = K.first[tb], L = K.knots[tb];
    const float* t = K.t + f;
    const float* x0 = K.x + (size_t)f * 13;
    const float rate = K.rate[b];
    if (L == 1) {
#pragma unroll
        for (int c = 0; c < 13; ++c) y[c] = x0[c];
    } else {
        float tau = FMA(rate, u, K.phase[b]);
        const float period = K.period[tb];
        if (period > 0.0f) {
            const float n = __builtin_floorf(tau * K.inv_period[tb]);
            tau = FMA(-n, period, tau);
        }
        const float ta = t[0], tz = t[L - 1];
        tau = tau > ta ? tau : ta;
        tau = tau < tz ? tau : tz;
        int lo = 0, hi = L - 1;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (t[mid] <= tau) lo = mid; else hi = mid;
        }
        const float a = (tau - t[lo]) * K.w[f + lo];
        const float* xa = x0 + (size_t)lo * 13;
#pragma unroll
        for (int c = 0; c < 13; ++c) y[c] = FMA(a, xa[13 + c] - xa[c], xa[c]);
    }
    const float* off = K.offset + (size_t)b * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        y[c] = y[c] + off[c];
        y[3 + c] = y[3 + c] * rate;
        y[10 + c] = y[10 + c] * rate;
    }
    if (K.renorm) {                                      // (wave-uniform)
        const float q0 = y[6], q1 = y[7], q2 = y[8], q3 = y[9];
        const float r = rsqrt_spec(FMA(q3, q3, FMA(q2, q2, FMA(q1, q1, q0 * q0))));
        y[6] = q0 * r; y[7] = q1 * r; y[8] = q2 * r; y[9] = q3 * r;
    }
}

// rows[b] = row for b < B (one reference window shared by every episode of a closed-loop batch), n floats per row
// SPEC.md §11j (K.t given; row, n and total are then not read): the TRACKING form of the launch. Thread i forms row i of rows f32[groups][B][K.rows][13] from the
// trajectory set and stores its 13 floats, so neighbouring threads write neighbouring rows. K.t null (every launch before §11j): not one access more.
// SPEC.md §11n (Q.list given; row, rows, n, total and K are then not read): the GATHER and SCATTER forms of the launch, x = chunks of 256 copy units of one row,
// y = dense row (sdempc_retire.inc.h). Q.list null (every launch before §11n): not one access more.
__global__ void __launch_bounds__(256) sdempc_broadcast_rows_kernel(const float* __restrict__ row, float* __restrict__ rows, int n, long long total, LoopTrack K,
                                                                    LoopCompact Q) {
    if (Q.list) {                                        // (wave-uniform)
        compact_rows(Q);
        return;
    }
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (K.t) {                                           // (wave-uniform)
        const long long per_group = (long long)K.B * K.rows;
        if (i >= per_group * K.groups) return;
        const int g = (int)(i / per_group);
        const int e = (int)(i - (long long)g * per_group);
        const int b = e / K.rows, r = e - b * K.rows;
        const float theta = (float)(K.tick0 + g) * K.dt;
        float y[13];
        track_row(K, b, theta + K.c[r], y);
        float* o = rows + i * 13;
#pragma unroll
        for (int c = 0; c < 13; ++c) o[c] = y[c];
        return;
    }
    if (i < total) rows[i] = row[i % n];
}

hipError_t launch_broadcast_rows(const float* row_dev, float* rows_dev, int n, int B, hipStream_t st, const LoopTrack& K, const LoopCompact& Q0) {
    if (Q0.list) {  // SPEC.md §11n: a present block is complete; a segment is copied 16 bytes at a time where its row length and both bases allow
        LoopCompact Q = Q0;
        if (K.t || row_dev || rows_dev || Q.n < 0 || Q.B < 1 || Q.n > Q.B || Q.nseg < 1 || Q.nseg > COMPACT_SEGS || (Q.scatter != 0 && Q.scatter != 1)) return hipErrorInvalidValue;
        if (Q.scatter ? (!Q.live || !Q.held_info || !Q.held_step || (Q.coop_bar && !Q.gave_up)) : Q.n < 1) return hipErrorInvalidValue;
        unsigned units = 0;
        for (int s = 0; s < Q.nseg; ++s) {
            LoopCompact::Seg& g = Q.seg[s];
            if (!g.src || !g.dst || g.words < 1) return hipErrorInvalidValue;
            g.vec = (g.words & 3) == 0 && ((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst)) & 15u) == 0 ? 1 : 0;
            units += (unsigned)(g.vec ? g.words >> 2 : g.words);
        }
        const unsigned gx = (units + 255u) / 256u;
        const int rows_y = Q.n + (Q.scatter ? 1 : 0);   // (the scatter form's held-row pass is grid row n)
        for (int i0 = 0; i0 < rows_y; i0 += 65535) {
            Q.i0 = i0;
            const int ny = rows_y - i0 < 65535 ? rows_y - i0 : 65535;
            sdempc_broadcast_rows_kernel<<<dim3(gx, (unsigned)ny), 256, 0, st>>>(nullptr, nullptr, 0, 0, K, Q);
        }
        return hipGetLastError();
    }
    if (K.t) {      // SPEC.md §11j: a present set is complete, and its clock stays exact in float32
        if (!rows_dev || !K.w || !K.x || !K.first || !K.knots || !K.period || !K.inv_period || !K.c || !K.table_of || !K.phase || !K.rate || !K.offset) return hipErrorInvalidValue;
        if (K.B < 1 || K.rows < 1 || K.groups < 1 || K.tick0 < 0 || (long long)K.tick0 + K.groups > (1ll << 24) || (K.renorm != 0 && K.renorm != 1)) return hipErrorInvalidValue;
        const long long threads = (long long)K.B * K.rows * K.groups;
        if (threads > (1ll << 31) - 256) return hipErrorInvalidValue;
        sdempc_broadcast_rows_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(nullptr, rows_dev, 0, 0, K, LoopCompact{});
        return hipGetLastError();
    }
    if (B < 1 || n < 1) return hipErrorInvalidValue;
    const long long total = (long long)n * B;
    sdempc_broadcast_rows_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(row_dev, rows_dev, n, total, K, LoopCompact{});
    return hipGetLastError();
}

}  // namespace sdempc
