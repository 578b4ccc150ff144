// sdempc_loop.inc.h — the plant of the batched closed loop (SPEC.md §11): one Euler–Maruyama step of the handle's own model per episode and
// tick, plus the hand-over to the next tick's solve (applied control, shifted warm start, step size).
// Fragment of sdempc_kernels.hip, translation unit SDEMPC_TU = 4: included inside namespace sdempc::{exact|fastm} (compiled once per math mode).
//
// The step is the rollout's own device code: step_fwd at t = 0 on a control table built by block_prepass, i.e. the arithmetic of step 0
// of every rollout (Oracle.step(x, u, xi, t=0)), in every mlp_dtype and math mode. One wave per episode, four episodes per workgroup
// (TeamWave): all 32 particle columns of the tile carry the same state and noise, and lane 0's copy is the result. The kernel gets the
// handle's argument block with H = 1 (a one-step horizon: the staged tables and the control table hold step 0 only); L.H is the solve's horizon.
// Arguments: LoopAdvance (sdempc_kernels.h).
template <int F16>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_advance_kernel(KArgs a, LoopAdvance L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = L.H, m = a.m;
    const int tid = TeamWave::tid();
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * TeamWave::IPB + TeamWave::team());
    Smem sm = carve(smem, 1, m, TeamWave::team());
    WaveW ww;
    load_weights(a, sm, ww, threadIdx.x, TeamWave::BNT);
    __syncthreads();
    if (b >= L.B) return;           // (wave-uniform; no workgroup-wide barrier below)
    const int lane = tid & 63, h = lane >> 5;
    const float* uo = L.uopt + (size_t)b * H * m;
    block_prepass<TeamWave>(a, sm, uo, tid);          // control table row 0 from uopt_k[0]
    float x[NX], xn[NX], xi[NN];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
#pragma unroll
    for (int i = 0; i < NN; ++i) xi[i] = L.xi[(size_t)b * NN + i];
    TeamWave::sync();
    StepAux A;
    step_fwd<F16, false>(a, sm, ww, 0, h, lane, x, xi, xn, A);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) { L.x[(size_t)b * NX + i] = xn[i]; L.xs[(size_t)b * NX + i] = xn[i]; }
        L.step[b] = L.info[(size_t)b * 8 + 1];
        if (L.coop_bar && L.coop_bar[(size_t)COOP_BAR_WORDS * b + 1] != 0u) *L.gave_up = 1u;
    }
    if (lane < m) L.us[(size_t)b * m + lane] = uo[lane];
    float* un = L.u + (size_t)b * H * m;
    for (int e = tid; e < H * m; e += TeamWave::NT) {   // y_{k+1} = [uopt_k[1:], uopt_k[H-1]]
        const int t = e / m;
        un[e] = uo[(t + 1 < H ? t + 1 : t) * m + (e - t * m)];
    }
}

hipError_t launch_loop_advance(const KArgs& a, const LoopAdvance& L, hipStream_t st) {
    if (L.B < 1 || L.H != a.H) return hipErrorInvalidValue;
    KArgs k = a;
    k.H = 1;
    const size_t sb = smem_bytes(1, k.m, TeamWave::IPB);
    const dim3 grid((L.B + TeamWave::IPB - 1) / TeamWave::IPB);
    return with_f16(k.f16, [&](auto F16) {
        sdempc_loop_advance_kernel<F16><<<grid, TeamWave::BNT, sb, st>>>(k, L);
        return hipGetLastError();
    });
}
