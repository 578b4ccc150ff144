// sdempc_api.cpp — C ABI (include/sdempc.h) over the HIP kernels in sdempc_kernels.hip.
//
// Reference-side counterpart: the solver objects built in SDEControlROS.load_single_mpc
// (sde4mbrl_px4/mpc_controller/sde_control.py:681-721) and used by mpc_process_fn (:328-450).
// Host logic only: argument checking, table construction (time grid, discount, momentum), lazy HIP
// context creation (the reference builds its solvers before fork(), sde_control.py:69-75), staging
// buffers for the host-pointer entry points and layout conversion. No arithmetic of the hot path
// runs on the host and there is no CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cxxabi.h>

#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sdempc.h"
#include "sdempc_kernels.h"

using namespace sdempc;
static_assert(blob::FLOATS == SDEMPC_BLOB_FLOATS, "blob layout: sdempc_kernels.h and include/sdempc.h");

namespace {
std::string g_create_error;

// SPEC.md §9: round toward zero to the nearest IEEE binary16 value; overflow saturates at 65504.
float f16_rtz_host(float x) {
    uint32_t u; memcpy(&u, &x, 4);
    const uint32_t sign = u & 0x80000000u, mag = u & 0x7FFFFFFFu;
    if (mag >= 0x7F800000u) return x;
    const int e = (int)(mag >> 23) - 127;
    float r;
    if (e > 15) r = 65504.0f;
    else if (e >= -14) { uint32_t t = mag & ~0x1FFFu; memcpy(&r, &t, 4); }
    else { float a; memcpy(&a, &mag, 4); r = floorf(a * 16777216.0f) / 16777216.0f; }
    uint32_t ru; memcpy(&ru, &r, 4); ru |= sign; memcpy(&r, &ru, 4);
    return r;
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// SPEC.md §10e: the rows of W3 are left as given when the binary exponent (frexp) of their largest entry is in W3_BAND_LO .. W3_BAND_HI, else brought to
// W3_BAND_TO; the smallest scale offset and the smallest non-zero bound C2 the matrix-pipe fast modes accept
constexpr int W3_BAND_LO = -3, W3_BAND_HI = 2, W3_BAND_TO = -1, ADJ_EOFF_MIN = 8;
constexpr float ADJ_C2_MIN = 0.015625f;

// What a model blob becomes for one arithmetic and one time grid — the one statement of it, for the handle's own model (sdempc_create) and for the plants of
// sdempc_closed_loop_batch_plant: the device payload (mlp_dtype f16: the fp16 rounding of SPEC.md §9; math_mode fast: the forward block and the block of
// the vector-Jacobian products of §10b), the kernels' model constants (ModelK, with the scale offset of §10e) and sigma_i * sqrt(dt_t) (SPEC.md §5: float32).
// f: the blob's float payload (SDEMPC_BLOB_FLOATS); mlp_dtype / math_mode already validated.
struct PreparedModel {
    std::vector<float> blob_f;   // one block, or two in math_mode fast
    std::vector<float> sdt;      // [nsteps][6]
    ModelK M;
};
// -> nullptr, or why the model is refused in this arithmetic (SPEC.md §10e, "What the mode accepts": the caller returns SDEMPC_EINVAL with this text).
const char* prepare_model(const float* f, int mlp_dtype, int math_mode, const float* time_steps, int nsteps, PreparedModel& out) {
    std::vector<float>& B = out.blob_f;
    B.assign(f, f + SDEMPC_BLOB_FLOATS);
    const bool mpfast = math_mode == 1 && mlp_dtype != 0;
    if (mpfast) {
        // SPEC.md §10e, "Normalisation of the output layer": the binary16 limbs of the adjoint's W3'^T image and of the scaled output adjoints need the rows of
        // W3 in a fixed range. Row i of W3 and b3[i] times 2^n_i, the residual scale of that output times 2^-n_i: the same function (§5.2 uses o_i only as
        // sF_i o_i / sT_i o_i), exact in float32. n_i = 0 when the largest entry of the row is in [2^-4, 2^2) (every synthetic vehicle), else the power that
        // brings it into [2^-2, 2^-1). A row whose rescale would round (an underflow, an overflow) is refused. The oracle states the same (parse_blob).
        for (int i = 0; i < 6; ++i) {
            float mx = 0.0f;
            for (int k = 0; k < 32; ++k) mx = fmaxf(mx, fabsf(B[blob::W3 + i * 32 + k]));
            if (!(mx > 0.0f && mx < INFINITY)) continue;
            int g = 0;
            (void)frexpf(mx, &g);
            if (g >= W3_BAND_LO && g <= W3_BAND_HI) continue;
            const int n = W3_BAND_TO - g;
            float* s = &B[40 + i];                          // sF[0..2], sT[0..2]
            bool exact = true;
            auto mul = [&](float& v, int e) { const float w = ldexpf(v, e); if (ldexpf(w, -e) != v && v == v) exact = false; v = w; };
            for (int k = 0; k < 32; ++k) mul(B[blob::W3 + i * 32 + k], n);
            mul(B[blob::B3 + i], n);
            mul(*s, -n);
            if (!exact) return "math_mode fast with mlp_dtype f32x3 / f16: a row of W3 lies outside [2^-4, 2^2) and its rescale (W3 row, b3, residual scale) is not exact in float32";
        }
    }
    if (mlp_dtype == 1) {   // layer-1 state-input weights and layer-2 weights live in fp16 (forward and adjoint alike)
        for (int i = 0; i < 64 * 6; ++i) B[blob::W1Z + i] = f16_rtz_host(B[blob::W1Z + i]);
        for (int i = 0; i < 32 * 32; ++i) B[blob::W2 + i] = f16_rtz_host(B[blob::W2 + i]);
    }
    if (math_mode == 1) {
        // SPEC.md §10b: the hardware tanh is evaluated as r = rcp(1 + exp2(a')), a' = (2 log2 e) a, tanh(a) = 1 - 2 r. The pre-scale goes into the weights
        // and biases that feed a tanh (one rounding each), the affine map 1 - 2 r into the weights and biases that consume one (exact factors, biases by
        // sequential sums), and the derivative 1 - tanh^2 = 4 (r - r^2) leaves its factor 4 in the transposed weights (exact). The device blob becomes
        // two blocks of the same layout: [forward weights][weights of the vector-Jacobian products]; float32 host arithmetic, no contraction.
        const float c = 2.885390043258667f;
        const std::vector<float> o = B;
        std::vector<float> F = o, V = o;
        for (int i = 0; i < 64 * 6; ++i) { float w = c * o[blob::W1Z + i]; F[blob::W1Z + i] = mlp_dtype == 1 ? f16_rtz_host(w) : w; }
        for (int i = 0; i < 64; ++i) F[blob::B1 + i] = c * o[blob::B1 + i];
        for (int i = 0; i < 32 * 8; ++i) F[blob::W1U + i] = c * o[blob::W1U + i];
        for (int j = 0; j < 32; ++j) {
            float sum = c * o[blob::B2 + j];
            for (int k = 0; k < 32; ++k) {
                float w = c * o[blob::W2 + j * 32 + k];
                if (mlp_dtype == 1) w = f16_rtz_host(w);
                sum = sum + w;
                F[blob::W2 + j * 32 + k] = -2.0f * w;
            }
            F[blob::B2 + j] = sum;
        }
        for (int i = 0; i < 6; ++i) {
            float sum = o[blob::B3 + i];
            for (int k = 0; k < 32; ++k) { sum = sum + o[blob::W3 + i * 32 + k]; F[blob::W3 + i * 32 + k] = -2.0f * o[blob::W3 + i * 32 + k]; }
            F[blob::B3 + i] = sum;
        }
        {
            float sum = o[blob::B3N];
            for (int k = 0; k < 32; ++k) { sum = sum + o[blob::W3N + k]; F[blob::W3N + k] = -2.0f * o[blob::W3N + k]; }
            F[blob::B3N] = sum;
        }
        for (int i = 0; i < 32 * 32; ++i) V[blob::W2 + i] = 4.0f * o[blob::W2 + i];
        for (int i = 0; i < 6 * 32; ++i) V[blob::W3 + i] = 4.0f * o[blob::W3 + i];
        for (int k = 0; k < 32; ++k) V[blob::W3N + k] = 4.0f * o[blob::W3N + k];
        if (mlp_dtype == 1) {
            // mlp_dtype f16 quantises c * w once more (toward zero), so the forward pass evaluates the weights F / c, not the Wq the blob held:
            // the vector-Jacobian products differentiate what was evaluated (SPEC.md §10b, last item of "Adjoint")
            for (int i = 0; i < 64 * 6; ++i) V[blob::W1Z + i] = F[blob::W1Z + i] / c;
            for (int i = 0; i < 32 * 32; ++i) V[blob::W2 + i] = (-2.0f * F[blob::W2 + i]) / c;
        }
        B = F;
        B.insert(B.end(), V.begin(), V.end());
    }
    out.sdt.resize((size_t)nsteps * SDEMPC_NNOISE);
    const float* sigma = f + blob::SIGMA;
    for (int t = 0; t < nsteps; ++t) {
        float sq = sqrtf(time_steps[t]);
        for (int i = 0; i < SDEMPC_NNOISE; ++i) out.sdt[(size_t)t * SDEMPC_NNOISE + i] = sigma[i] * sq;
    }
    ModelK& M = out.M;
    memset(&M, 0, sizeof M);
    M.inv_mass = f[0]; M.grav = f[1];
    for (int i = 0; i < 3; ++i) { M.J[i] = f[2 + i]; M.iJ[i] = f[5 + i]; }
    M.ct2 = f[8]; M.ct1 = f[9]; M.ct0 = f[10]; M.cm2 = f[11]; M.cm1 = f[12];
    for (int j = 0; j < 8; ++j) { M.rx[j] = f[16 + j]; M.ry[j] = f[24 + j]; M.dir[j] = f[32 + j]; }
    for (int i = 0; i < 3; ++i) { M.sF[i] = B[40 + i]; M.sT[i] = B[43 + i]; }      // (§10e: the normalised ones)
    for (int i = 0; i < 6; ++i) M.b3[i] = B[blob::B3 + i];      // (math_mode fast: the forward block's, SPEC.md §10b)
    M.b3n = B[blob::B3N];
    M.adj_s0 = -2.0f; M.adj_i0 = 1.0f;
    if (math_mode == 1 && mlp_dtype != 0) {
        // SPEC.md §10e: the scale offset of the adjoint's binary16 contractions. With the largest output adjoint of a particle scaled into [2^eoff, 2^(eoff+1)),
        // |abar2| < 2^(eoff+1) B3/4, |abar1n| < 2^(eoff+1) Bn/4, |abar1d| < 2^(eoff+1) C2 B3/16 (|r - r^2| <= 1/4; B3, Bn: absolute column sums of the forward
        // output weights, C2: of 4 W2): eoff = min(10, 14 - e) with 2^e > the largest of the three bounds keeps all of them below 2^15 (binary16 ends at 65504).
        // float32 host arithmetic, sums in ascending index order; the oracle derives the same number by the same statements.
        const float* F = B.data();
        const float* V = F + SDEMPC_BLOB_FLOATS;
        float B3 = 0.0f, Bn = 0.0f, C2 = 0.0f;
        for (int k = 0; k < 32; ++k) {
            float s3 = 0.0f, s2 = 0.0f;
            for (int i = 0; i < 6; ++i) s3 = s3 + fabsf(F[blob::W3 + i * 32 + k]);
            for (int j = 0; j < 32; ++j) s2 = s2 + fabsf(V[blob::W2 + j * 32 + k]);
            B3 = fmaxf(B3, s3); C2 = fmaxf(C2, s2); Bn = fmaxf(Bn, fabsf(F[blob::W3N + k]));
        }
        const float bound = fmaxf(fmaxf(B3 * 0.25f, Bn * 0.25f), (C2 * (B3 * 0.25f)) * 0.25f);
        int e = 0, eoff = 10;
        if (bound > 0.0f && bound < INFINITY) { (void)frexpf(bound, &e); if (14 - e < eoff) eoff = 14 - e; }
        if (eoff < -40) eoff = -40;
        M.adj_s0 = ldexpf(-2.0f, eoff); M.adj_i0 = ldexpf(1.0f, -eoff);
        // SPEC.md §10e, "What the mode accepts": a weight beyond binary16's largest finite value has no limbs, and below eoff = ADJ_EOFF_MIN the second limbs
        // of the scaled output adjoints are sub-normal. Neither has an exact host-side cure: the model is refused, not evaluated wrongly.
        float wmax = 0.0f;
        for (int i = 0; i < 32 * 32; ++i) wmax = fmaxf(wmax, fmaxf(fabsf(F[blob::W2 + i]), fabsf(V[blob::W2 + i])));
        for (int i = 0; i < 64 * 6; ++i) wmax = fmaxf(wmax, fabsf(V[blob::W1Z + i]));
        for (int i = 0; i < 32 * 8; ++i) wmax = fmaxf(wmax, fabsf(V[blob::W1U + i]));
        for (int i = 0; i < 6 * 32; ++i) wmax = fmaxf(wmax, fabsf(F[blob::W3 + i]));
        if (wmax > 65504.0f) return "math_mode fast with mlp_dtype f32x3 / f16: a weight of a binary16 operand image (-2 c W2, 4 W2, W1z, W1u, -2 W3) exceeds 65504 in magnitude";
        if (C2 > 0.0f && C2 < ADJ_C2_MIN) return "math_mode fast with mlp_dtype f32x3 / f16: the largest absolute column sum C2 of 4 W2 is below 2^-6 (the second binary16 limbs of W2 are sub-normal)";
        if (eoff < ADJ_EOFF_MIN) return "math_mode fast with mlp_dtype f32x3 / f16: the scale offset eoff of the adjoint's binary16 contractions is below 8 (bound = max(B3/4, Bn/4, C2 B3/16) >= 2^7: W2 or w3n too large)";
    }
    return nullptr;
}
}  // namespace

struct sdempc_handle {
    sdempc_cfg cfg;
    std::vector<float> time_steps;
    std::vector<float> blob_f;  // float payload of the model blob
    int m = 0, H = 0, P = 0, G = 0, max_batch = 0;
    int device = 0;
    bool dev_ready = false;
    mutable std::string err;
    KArgs base;
    unsigned ticket_total = 0;   // running value of the device ticket word (KArgs::ticket_host points here; sdempc_kernels.hip, launch_persistent)
    int ws_rows = 0;             // rows (instances or team slots) the trajectory / checkpoint / partial-sum / control-table workspaces hold
    int traj_batch = 0;          // instances whose particle x horizon tensor the trajectory workspace holds (last rollout with store_traj); 0: none —
                                 // any later launch that writes the workspace (gradient, solve) or a reallocation of it resets this
    bool last_ticketed = false;  // the last solve launch handed its instances out by ticket: sdempc_solve_status compares the word with the mirror
    // host tables
    std::vector<float> h_sdt, h_disc, h_beta;
    // device tables
    DevBuf d_dt, d_sdt, d_disc, d_beta, d_wts, d_sctab;
    // workspace + staging (sized for max_batch)
    DevBuf d_ustg;            // per-step control table [B][H][36] of the solve kernel's long-horizon instantiation (KArgs::ustg)
    DevBuf d_part, d_act, d_traj, d_x0, d_u, d_xref, d_noise, d_step, d_cost, d_grad, d_xmean, d_uopt, d_info;
    // canonical-layout staging of the host-pointer entry points (allocated on their first use)
    DevBuf d_noise_canon, d_traj_canon, d_keys;
    // predicted tube (sdempc_tube_batch / _keys, allocated on their first use): the five planes mean, var, min, max f32 and outside u32, each [max_batch][(H+1)*13]
    DevBuf d_tube;
    // predicted bands (sdempc_bands_batch / _keys, allocated on their first use): obs f32, q f32[8 planes], below u32, at u32 — eleven planes, each [max_batch][(H+1)*13]
    DevBuf d_band;
    // predicted risk (sdempc_risk_batch / _keys / _dev, allocated on their first use; risk_regions): staged bounds and centre rows (the particle mean of
    // centre_mode 3 among them) and the staging copies of the seven outputs
    DevBuf d_risk;
    // predicted outcome (sdempc_outcome_batch / _keys, allocated on their first use; outcome_regions): the staged target rows and the staging copies of the
    // eight outputs
    DevBuf d_outcome;
    // closed loop (sdempc_closed_loop_batch, allocated on its first use): d_loop = keys u32[max_batch][2], solve keys u32[max_batch][2], plant noise
    // f32[max_batch][6], one flag word; d_loop_chunk = the per-tick outputs of one chunk of ticks and the reference windows it reads (grown, never shrunk)
    DevBuf d_loop, d_loop_chunk;
    // closed loop against a separate plant (sdempc_closed_loop_batch_plant): the prepared plants of the current call (model constants, payloads, sigma sqrt(dt),
    // step length, plant_of) and the plant noise of a tick, one allocation (grown, never shrunk); plant_stage: its host image, alive until the call returns
    DevBuf d_plant;
    std::vector<char> plant_stage;
    // closed loop through the rate-setpoint interface (sdempc_closed_loop_batch_rate, allocated on its first use): integrator f32[max_batch][3], rate tail f32[max_batch][H][3]
    DevBuf d_rate;
    // closed loop on a measured state (sdempc_closed_loop_batch_observed, allocated on its first use): observation keys u32[max_batch][2], held measurement f32[max_batch][13]
    DevBuf d_obs;
    // closed loop from an aged estimate (sdempc_closed_loop_batch_aged, allocated on its first use and grown with age_max): the last age_max substep states
    // f32[age_max][B][13], oldest first
    DevBuf d_hist;
    // closed loop scored on the device (sdempc_closed_loop_batch_scored with a score cfg, allocated on its first use): the score words u32[max_batch][16]
    DevBuf d_score;
    // per-row ensemble histories (sdempc_closed_loop_batch_ensemble with an ensemble cfg; allocated on first use, grown, never shrunk): the cohorts i32[max_batch], the
    // edges f32[4][ENS_MAX_EDGES], then for one slab of rows the combined words u32[rows][G][W] and the per-block partial words u32[rows][nblk][G][W]
    DevBuf d_ens;
    // retiring failed episodes (sdempc_closed_loop_batch_retire with a retire cfg; allocated on first use): per row of max_batch live i32, retired_at i32, list i32 and
    // the row count u32, then the block counts u32[ceil(max_batch / 256)] and n_live; behind them, each part 16-byte aligned and sized for max_batch rows, the dense
    // staging of the live set's solve: x0 [13], xref [(H+1) 13], u [H m], step, subkey [2] in, and uopt [H m], xevol [(H+1) 13], info [8] out
    DevBuf d_retire;
    // closed loop with processes drawn on the device (sdempc_closed_loop_batch_drawn with a process cfg, allocated on its first use), per row of max_batch: the
    // disturbance chain u32[2] and state f32[6], the bias chain u32[2] and state f32[12], then rho and scale of each (f32[6], f32[6], f32[12], f32[12])
    DevBuf d_proc;
    // closed loop with events drawn on the device (sdempc_closed_loop_batch_events with an event cfg, allocated on its first use), per row of max_batch: the fault
    // chain's row (EVENT_EP_WORDS: key u32[2], then (s, first) i32 per motor), the dropout chain u32[2] and state i32[2], then the row of fault parameters
    // (EVENT_PAR_WORDS: onset u32[8][4], clear u32[8][4], modes f32[8][4][2]) and the dropout thresholds (u32 drop, u32 recover)
    DevBuf d_evt;
    // the geometric baseline controller (sdempc_closed_loop_batch_baseline, sdempc_geo_command_batch; allocated on first use): the parameter rows f32[max_batch][GEO_PAR_WORDS],
    // then the commands f32[max_batch][4] of sdempc_geo_command_batch
    DevBuf d_geo;
    // closed loop tracking a trajectory (sdempc_closed_loop_batch_tracked with a track cfg, sdempc_reference_windows; allocated on first use, grown, never shrunk): the set of
    // the current call — first / knots i32[n_tables], period / inv_period f32[n_tables], t / w f32[sum L], x f32[sum L][13], c f32[H+1], table_of i32[B], phase / rate f32[B],
    // offset f32[B][3] — in one allocation; track_stage: its host image, alive until the call returns
    DevBuf d_track;
    std::vector<char> track_stage;
    DevBuf d_work;            // u64[4] work counters (KArgs::work)
    // cooperative latency path of the solve (allocated on its first use, sized for coop_cap instances)
    DevBuf d_coop_bar, d_coop_pp, d_coop_ck;
    int coop_cap = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    const void* last_fn = nullptr;   // host function pointer of the kernel the last *_dev launch started (sdempc_last_kernel_name)
    int spin_us = -1;         // SDEMPC_OPT_COOP_SPIN_US: budget of one grid barrier in microseconds; -1 = derived (coop_spin_ticks)
    float coop_ms_last = 0.0f;   // duration of the last cooperative-layout solve that completed (0: none measured yet)
    int last_coop_B = 0;      // > 0: the last solve launch took the cooperative path with this many instances (error flags to check)
    bool coop_off = false;    // a grid barrier timed out once: this handle stays on the one-workgroup-per-instance layouts
    int layout_fallbacks = 0; // how often that happened (sdempc_layout_fallbacks)
    int loop_chunk_bytes = -1;   // SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES: device bytes per chunk of closed-loop ticks; -1: the built-in LOOP_CHUNK_BYTES
    int ws_fill = -1;         // SDEMPC_OPT_TEST_WS_FILL: 0..255 = byte every float-valued device buffer is filled with right after its hipMalloc (dev_alloc); -1: none
};

namespace {

int fail(sdempc_handle* h, int code, const char* fmt, const char* detail = "") {
    char buf[512];
    snprintf(buf, sizeof buf, fmt, detail);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

// No exception may cross the C ABI (include/sdempc.h: "never aborts or throws"; an exception in the reference's forked worker would
// end mpc_process silently, sde_control.py:365-419): every entry point runs inside guarded(), which turns std::bad_alloc into
// SDEMPC_ENOMEM and anything else into SDEMPC_EINVAL. The handlers themselves allocate nothing that can throw past them.
void set_error_nothrow(const sdempc_handle* h, const char* msg) noexcept {
    try { if (h) h->err = msg; else g_create_error = msg; } catch (...) { /* no room even for the message: the code still reports it */ }
}
// size and header of a model blob (SPEC.md §2); its motor count is header word 2
int check_blob(sdempc_handle* h, const void* model_blob, size_t blob_bytes) {
    if (!model_blob || blob_bytes < sizeof(int32_t) * SDEMPC_BLOB_HEADER_INTS + sizeof(float) * SDEMPC_BLOB_FLOATS)
        return fail(h, SDEMPC_EBLOB, "model blob too small%s");
    const int32_t* hd = (const int32_t*)model_blob;
    if (hd[0] != SDEMPC_BLOB_MAGIC || hd[1] != 1 || hd[3] != SDEMPC_HID || hd[4] != 6 || hd[5] != SDEMPC_NNOISE)
        return fail(h, SDEMPC_EBLOB, "model blob header mismatch%s");
    return 0;
}
template <class F>
int guarded(const sdempc_handle* h, F&& f) noexcept {
    try { return f(); }
    catch (const std::bad_alloc&) { set_error_nothrow(h, "out of host memory"); return SDEMPC_ENOMEM; }
    catch (const std::length_error&) { set_error_nothrow(h, "a table size derived from the arguments exceeds what the host can allocate"); return SDEMPC_ENOMEM; }
    catch (const std::exception& e) { set_error_nothrow(h, e.what()); return SDEMPC_EINVAL; }
    catch (...) { set_error_nothrow(h, "unexpected exception inside libsdempc"); return SDEMPC_EINVAL; }
}

#define HIPCHK(h, call)                                                                 \
    do {                                                                                \
        hipError_t e__ = (call);                                                        \
        if (e__ != hipSuccess) {                                                        \
            char b__[400];                                                              \
            snprintf(b__, sizeof b__, "%s failed: %s", #call, hipGetErrorString(e__)); \
            (h)->err = b__;                                                             \
            return SDEMPC_EDEVICE;                                                      \
        }                                                                               \
    } while (0)

// Environment variables give the DEFAULTS of a new handle's options, read once here (sdempc_create); the launch path never reads the
// environment. Unset or malformed -> the built-in default.
int env_int(const char* name, int dflt, int lo, int hi) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || v < lo || v > hi) return dflt;
    return (int)v;
}
void default_options(sdempc_handle* h) {
    LaunchOpts& o = h->base.opt;
    o.cus = 256;                                       // replaced by the device's count when the device is bound (ensure_device)
    o.lane = env_int("SDEMPC_LANE", 1, 0, 1);
    o.coop = env_int("SDEMPC_COOP", 1, 0, 1);
    o.spec = env_int("SDEMPC_SPEC", 1, 0, 1);
    o.pk = env_int("SDEMPC_PK", -1, -1, 1);
    o.ustg = env_int("SDEMPC_USTG", -1, -1, 1);
    o.duo = env_int("SDEMPC_DUO", -1, -1, 1);
    o.coop_launch = env_int("SDEMPC_COOP_LAUNCH", 0, 0, 1);
    o.coop_fence = env_int("SDEMPC_COOP_FENCE", 0, 0, 1);
    o.hex = env_int("SDEMPC_HEX", 1, 0, 1);
    o.absent_wg = -1;                                  // fault injection is a per-handle option only (SDEMPC_OPT_TEST_ABSENT_WG): never from the environment
    h->spin_us = env_int("SDEMPC_COOP_SPIN_US", -1, -1, 10 * 1000 * 1000);
}
// Budget of one grid barrier of the cooperative layouts, in 10 ns ticks (KArgs::coop_spin). A barrier is passed ~780 times per C2
// solve, microseconds each; one that waits this long means the grid is not fully resident (the GPU is shared) and the launch gives
// up so that the caller's control tick falls back to the one-workgroup-per-instance layout instead of stalling. Derived: five times
// the last completed cooperative solve of this handle, between 2 ms and 100 ms; 100 ms before the first one.
unsigned coop_spin_ticks(const sdempc_handle* h) {
    if (h->spin_us >= 0) return (unsigned)((uint64_t)h->spin_us * 100u > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)h->spin_us * 100u);
    float ms = h->coop_ms_last > 0.0f ? 5.0f * h->coop_ms_last : 100.0f;
    if (ms < 2.0f) ms = 2.0f;
    if (ms > 100.0f) ms = 100.0f;
    return (unsigned)(ms * 1e5f);
}

// Work the host put on the null stream (hipMemset) is over before anything is enqueued behind it on another stream: the handle's own stream and
// the streams callers pass are non-blocking, i.e. not ordered against the null stream by the runtime.
int null_stream_done(sdempc_handle* h) {
    HIPCHK(h, hipStreamSynchronize(nullptr));
    return 0;
}
// fill: a float-valued buffer whose initial contents nothing may depend on — SDEMPC_OPT_TEST_WS_FILL writes its byte over it, complete before
// the caller goes on to its launch path (include/sdempc.h lists the buffers that are exempt, and why)
int dev_alloc(sdempc_handle* h, DevBuf& b, size_t bytes, bool fill = false) {
    if (bytes == 0) bytes = 16;
    HIPCHK(h, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    if (fill && h->ws_fill >= 0) {
        HIPCHK(h, hipMemset(b.p, h->ws_fill, bytes));
        return null_stream_done(h);
    }
    return 0;
}
void dev_free(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

size_t noise_floats(const sdempc_handle* h, int B) { return (size_t)B * h->G * h->H * SDEMPC_NNOISE * 32; }
size_t traj_floats(const sdempc_handle* h, int B) { return (size_t)B * h->G * (h->H + 1) * SDEMPC_NX * 32; }

int ensure_device_impl(sdempc_handle* h) {
    if (h->dev_ready) {
        HIPCHK(h, hipSetDevice(h->device));
        return 0;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(h, SDEMPC_EDEVICE, "no HIP device available (%s); sdempc has no CPU fallback", hipGetErrorString(e));
    if (h->device >= n) return fail(h, SDEMPC_EDEVICE, "device ordinal out of range%s");
    HIPCHK(h, hipSetDevice(h->device));
    {   // compute units of THIS handle's device (the layout heuristics count workgroups against it)
        int cus = 0;
        HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        if (cus > 0) h->base.opt.cus = cus;
    }
    HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreate(&h->ev0));
    HIPCHK(h, hipEventCreate(&h->ev1));
    const int H = h->H, m = h->m, B = h->max_batch;
    int rc;
    if ((rc = dev_alloc(h, h->d_dt, sizeof(float) * H))) return rc;
    if ((rc = dev_alloc(h, h->d_sdt, sizeof(float) * H * SDEMPC_NNOISE))) return rc;
    if ((rc = dev_alloc(h, h->d_disc, sizeof(float) * (H + 1)))) return rc;
    if ((rc = dev_alloc(h, h->d_beta, sizeof(float) * h->h_beta.size()))) return rc;
    if ((rc = dev_alloc(h, h->d_wts, sizeof(float) * h->blob_f.size()))) return rc;
    HIPCHK(h, hipMemcpy(h->d_dt.p, h->time_steps.data(), sizeof(float) * H, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_sdt.p, h->h_sdt.data(), sizeof(float) * H * SDEMPC_NNOISE, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_disc.p, h->h_disc.data(), sizeof(float) * (H + 1), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_beta.p, h->h_beta.data(), sizeof(float) * h->h_beta.size(), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_wts.p, h->blob_f.data(), sizeof(float) * h->blob_f.size(), hipMemcpyHostToDevice));
    if (h->cfg.num_state_constr > 0) {       // state_constr table (SPEC.md §5.3)
        CostK::StateBound tab[SDEMPC_NX];
        for (int k = 0; k < h->cfg.num_state_constr; ++k)
            tab[k] = CostK::StateBound{h->cfg.state_id[k], h->cfg.state_w[k], h->cfg.state_lo[k], h->cfg.state_hi[k]};
        if ((rc = dev_alloc(h, h->d_sctab, sizeof(CostK::StateBound) * h->cfg.num_state_constr))) return rc;
        HIPCHK(h, hipMemcpy(h->d_sctab.p, tab, sizeof(CostK::StateBound) * h->cfg.num_state_constr, hipMemcpyHostToDevice));
        h->base.C.sc_n = h->cfg.num_state_constr;
        h->base.C.sc_tab = (const CostK::StateBound*)h->d_sctab.p;
    }
    if ((rc = dev_alloc(h, h->d_x0, sizeof(float) * B * SDEMPC_NX, true))) return rc;
    if ((rc = dev_alloc(h, h->d_u, sizeof(float) * B * H * m, true))) return rc;
    if ((rc = dev_alloc(h, h->d_xref, sizeof(float) * B * (H + 1) * SDEMPC_NX, true))) return rc;
    if ((rc = dev_alloc(h, h->d_noise, sizeof(float) * noise_floats(h, B), true))) return rc;
    if ((rc = dev_alloc(h, h->d_step, sizeof(float) * B, true))) return rc;
    if ((rc = dev_alloc(h, h->d_cost, sizeof(float) * B, true))) return rc;
    if ((rc = dev_alloc(h, h->d_grad, sizeof(float) * B * H * m, true))) return rc;
    if ((rc = dev_alloc(h, h->d_xmean, sizeof(float) * B * (H + 1) * SDEMPC_NX, true))) return rc;
    if ((rc = dev_alloc(h, h->d_uopt, sizeof(float) * B * H * m, true))) return rc;
    if ((rc = dev_alloc(h, h->d_info, sizeof(float) * B * 8, true))) return rc;
    if ((rc = dev_alloc(h, h->d_work, sizeof(unsigned long long) * 5))) return rc;      // 4 counters + the persistent launches' instance ticket
    HIPCHK(h, hipMemset(h->d_work.p, 0, h->d_work.bytes));
    if ((rc = null_stream_done(h))) return rc;
    h->base.work = (unsigned long long*)h->d_work.p;
    h->base.ticket_host = &h->ticket_total;
    h->ticket_total = 0;                                   // matches the zeroed ticket word
    h->base.dt = (const float*)h->d_dt.p;
    h->base.sdt = (const float*)h->d_sdt.p;
    h->base.disc = (const float*)h->d_disc.p;
    h->base.beta = (const float*)h->d_beta.p;
    h->base.wts = (const float*)h->d_wts.p;
    h->dev_ready = true;
    return 0;
}

// The kernels' own workspaces — particle x horizon tensor, activation checkpoint, per-group partial sums, control table in global memory —
// hold `rows` instances: one row per instance for the one-workgroup-per-instance layouts, one per TEAM SLOT for the persistent throughput
// launches, which is what keeps a large batch small (C2: 1.5 MB per row; 1,536 slots = 2.3 GB whatever the batch). Allocated on the first
// launch that needs them and grown when a later launch needs more rows (never shrunk).
int ensure_workspace(sdempc_handle* h, int rows) {
    if (rows <= h->ws_rows) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));          // nothing may still be using the old rows (caller streams: the caller's business, as for every _dev entry point)
    for (DevBuf* b : {&h->d_traj, &h->d_act, &h->d_part, &h->d_ustg}) dev_free(*b);
    h->ws_rows = 0; h->base.ws_rows = 0; h->traj_batch = 0;
    h->base.traj = h->base.act = h->base.part = h->base.ustg = nullptr;
    const int H = h->H;
    int rc;
    if ((rc = dev_alloc(h, h->d_traj, sizeof(float) * traj_floats(h, rows), true))) return rc;
    // Zeroed since the first version, as hygiene: no kernel reads a word of it that the same launch has not written (every lane of a group row is
    // stored before the adjoint sweep loads it; sdempc_traj_to_canonical_dev is refused unless a store_traj rollout filled the rows, and skips the
    // padded particles) — so SDEMPC_OPT_TEST_WS_FILL fills it like the others.
    if (h->ws_fill < 0) {
        HIPCHK(h, hipMemset(h->d_traj.p, 0, h->d_traj.bytes));
        if ((rc = null_stream_done(h))) return rc;
    }
    if ((rc = dev_alloc(h, h->d_act, sizeof(float) * (size_t)rows * h->G * H * ACT_STRIDE, true))) return rc;
    if ((rc = dev_alloc(h, h->d_part, sizeof(float) * (size_t)rows * h->G * part_stride(H), true))) return rc;
    if ((rc = dev_alloc(h, h->d_ustg, sizeof(float) * (size_t)rows * H * 36, true))) return rc;
    h->base.traj = (float*)h->d_traj.p;
    h->base.act = (float*)h->d_act.p;
    h->base.part = (float*)h->d_part.p;
    h->base.ustg = (float*)h->d_ustg.p;
    h->ws_rows = rows;
    h->base.ws_rows = rows;
    return 0;
}

void release_device(sdempc_handle* h);

// Lazy device initialisation; a failure half-way (e.g. out of HBM) releases what was allocated so that a later call starts clean.
int ensure_device(sdempc_handle* h) {
    const bool was_ready = h->dev_ready;
    const int rc = ensure_device_impl(h);
    if (rc != 0 && !was_ready) { const std::string keep = h->err; release_device(h); h->err = keep; }
    return rc;
}

int check_batch(sdempc_handle* h, int B) {
    if (!h) return SDEMPC_EINVAL;
    if (B < 1) return fail(h, SDEMPC_EINVAL, "batch must be >= 1%s");
    if (B > h->max_batch) return fail(h, SDEMPC_ECAPACITY, "batch exceeds max_batch given to sdempc_create%s");
    return 0;
}

// does the trajectory workspace hold the particle x horizon tensor of at least B instances? (sdempc_traj_to_canonical_dev, sdempc_tube_batch_dev)
int check_traj_held(sdempc_handle* h, int B) {
    if (B > h->traj_batch)
        return fail(h, SDEMPC_EINVAL, h->traj_batch ? "the trajectory workspace holds fewer instances than asked for (last rollout with store_traj was smaller)%s"
                                                     : "the trajectory workspace holds no rollout: run a rollout with store_traj first (a gradient evaluation, a solve or a "
                                                       "workspace reallocation since then has overwritten it)%s");
    return 0;
}

// every check of a tube request (SPEC.md §12) that needs no device; no HIP call
int check_tube(sdempc_handle* h, const sdempc_tube_cfg* cfg, const void* mean, const void* var, const void* mn, const void* mx, const void* outside) {
    if (cfg && cfg->struct_size != (int32_t)sizeof(sdempc_tube_cfg)) return fail(h, SDEMPC_EINVAL, "sdempc_tube_cfg.struct_size mismatch%s");
    if (!mean && !var && !mn && !mx && !outside) return fail(h, SDEMPC_EINVAL, "no output plane asked for: mean, var, min, max and outside are all NULL%s");
    if (outside && !cfg) return fail(h, SDEMPC_EINVAL, "outside needs a sdempc_tube_cfg (the bounds it counts against)%s");
    if (cfg)
        for (int i = 0; i < SDEMPC_NX; ++i)
            if (cfg->lo[i] != cfg->lo[i] || cfg->hi[i] != cfg->hi[i]) return fail(h, SDEMPC_EINVAL, "a bound of sdempc_tube_cfg is NaN (use -inf / +inf for no bound)%s");
    return 0;
}

void noise_to_dev_layout(const sdempc_handle* h, int B, const float* in, float* out) {
    const int P = h->P, H = h->H, G = h->G;
    memset(out, 0, sizeof(float) * noise_floats(h, B));
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < P; ++p) {
            const int g = p / 32, l = p % 32;
            for (int t = 0; t < H; ++t)
                for (int i = 0; i < SDEMPC_NNOISE; ++i)
                    out[((((size_t)b * G + g) * H + t) * SDEMPC_NNOISE + i) * 32 + l] = in[(((size_t)b * P + p) * H + t) * SDEMPC_NNOISE + i];
        }
}

int stage_common(sdempc_handle* h, int B, const float* x0, const float* u, const float* xref, const float* noise) {
    const int H = h->H, m = h->m;
    int rc;
    if (!h->d_noise_canon.p && (rc = dev_alloc(h, h->d_noise_canon, sizeof(float) * (size_t)h->max_batch * h->P * H * SDEMPC_NNOISE, true))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_x0.p, x0, sizeof(float) * B * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_u.p, u, sizeof(float) * B * H * m, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_xref.p, xref, sizeof(float) * B * (H + 1) * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    // the caller's canonical [B][P][H][6] tensor goes up as it is; the particle-minor layout is made on the device
    HIPCHK(h, hipMemcpyAsync(h->d_noise_canon.p, noise, sizeof(float) * (size_t)B * h->P * H * SDEMPC_NNOISE, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_relayout(true, (const float*)h->d_noise_canon.p, (float*)h->d_noise.p, B, h->P, h->G, H * SDEMPC_NNOISE, h->stream));
    return 0;
}

// keys (host u32[B][2]) -> device staging -> noise in the device layout at out_dev, on stream st
int noise_from_keys(sdempc_handle* h, int B, const uint32_t* keys, float* out_dev, hipStream_t st) {
    int rc;
    if (!h->d_keys.p && (rc = dev_alloc(h, h->d_keys, sizeof(uint32_t) * 2 * (size_t)h->max_batch))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_keys.p, keys, sizeof(uint32_t) * 2 * (size_t)B, hipMemcpyHostToDevice, st));
    HIPCHK(h, launch_noise_from_keys((const uint32_t*)h->d_keys.p, out_dev, B, h->P, h->G, h->H, st));
    return 0;
}

// after a synchronised cooperative solve: did any grid barrier give up? (telemetry is NaN in that case as well)
// Did a grid barrier of the last (cooperative-layout) solve launch give up? Call after the launch's stream has been synchronised.
int coop_timed_out(sdempc_handle* h, bool* timed_out) {
    *timed_out = false;
    if (h->last_coop_B <= 0) return 0;
    std::vector<unsigned> f(COOP_BAR_WORDS * (size_t)h->last_coop_B);
    HIPCHK(h, hipMemcpy(f.data(), h->d_coop_bar.p, sizeof(unsigned) * f.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < h->last_coop_B; ++b)
        if (f[COOP_BAR_WORDS * b + 1] != 0u) *timed_out = true;
    if (*timed_out) {                    // the workgroups were not all resident (GPU shared with other work): no second try on this handle
        h->coop_off = true;
        h->layout_fallbacks += 1;
        h->last_coop_B = 0;
    } else if (h->timed) {               // completed: its duration scales the next launch's barrier budget (coop_spin_ticks)
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess && ms > 0.0f) h->coop_ms_last = ms;
    }
    return 0;
}

// A ticketed persistent launch (sdempc_kernels.hip, launch_persistent) draws its instances relative to the value the device's ticket word
// had at launch, which the host mirrors (ticket_total) on the assumption that every launch advances the word by exactly its batch size.
// Anything that breaks the assumption — a kernel that was aborted, two launches of one handle overlapping on different streams, a
// captured graph replaying a launch with its baked-in base — would leave instances unsolved with stale outputs. Call after the launch's
// stream has been synchronised: compares the word with the mirror, re-synchronises the mirror and reports the launch as failed.
int tickets_consistent(sdempc_handle* h) {
    if (!h->last_ticketed || !h->dev_ready) return 0;
    h->last_ticketed = false;
    unsigned word = 0;
    HIPCHK(h, hipMemcpy(&word, (const char*)h->d_work.p + 4 * sizeof(unsigned long long), sizeof word, hipMemcpyDeviceToHost));
    if (word == h->ticket_total) return 0;
    char msg[256];
    snprintf(msg, sizeof msg, "ticketed launch: the device's ticket word reads %u where the host expects %u (aborted kernel, overlapping launches of one "
                              "handle, or a replayed graph); instances of that launch may be unsolved", word, h->ticket_total);
    h->ticket_total = word;
    return fail(h, SDEMPC_EDEVICE, "%s", msg);
}

template <class F>
int timed_launch(sdempc_handle* h, hipStream_t st, F&& f) {
    HIPCHK(h, hipEventRecord(h->ev0, st));
    hipError_t e = f();
    if (e != hipSuccess) return fail(h, SDEMPC_EDEVICE, "kernel launch failed: %s", hipGetErrorString(e));
    HIPCHK(h, hipEventRecord(h->ev1, st));
    h->timed = true;
    h->last_fn = last_launched_kernel();
    return 0;
}


int solve_staged(sdempc_handle* h, int32_t B, float* uopt, float* xevol, sdempc_info* info);
struct LoopIo {
    int B, T, xref_ticks, xref_batch;
    const float *x0, *xref;
    const uint32_t* keys;
    const float *u_init, *stepsize_in;
    float *xs, *us;
    sdempc_info* info;
    float *u_next, *stepsize_next;
    uint32_t* keys_next;
};
// SPEC.md §11a: the plant set of one sdempc_closed_loop_batch_plant call, staged on the device (stage_plants)
struct PlantRun {
    KArgs k;        // argument block of launch_loop: the handle's with the plant's arithmetic and step length (one shared plant: its M / wts / sdt too)
    LoopPlant Q;
    float* xi;      // [B][substeps][6] plant noise of a tick
    float dt;       // the plant's step length
};
// SPEC.md §11b: the timing of one sdempc_closed_loop_batch_timed call. With it LoopIo::xref_ticks counts SOLVES (1 or Ns) and LoopIo::info is [B][Ns].
struct TimedRun {
    int S, D;                   // solve period in ticks, solve delay in plant substeps
    float alpha;                // motor lag (0: off)
    const float* u_act_in;      // [B][m] or null (u_init[b][0])
    float* u_act_next;          // [B][m] or null
};
// SPEC.md §11c: the schedules of one sdempc_closed_loop_batch_scenario call (host pointers; staged per chunk by closed_loop_run)
struct ScenarioRun {
    const float* dist;          // [Td][Bd][6] or null
    int Td, Bd;
    const int32_t* plant_of;    // [Tp][B] or null (identity); read only when the plant set has more than one member
    int Tp;
};
// SPEC.md §11d: the rate loop of one sdempc_closed_loop_batch_rate call (host pointers)
struct RateRun {
    const sdempc_rate_cfg* cfg;
    float inv_m;
    const float *integ_in, *tail_in;    // [B][3] / [B][H][3] or null (zeros)
    float *ws, *integ_next, *tail_next; // [B][T][4]; [B][3] / [B][H][3] or null
};
// SPEC.md §11e: the additions of one sdempc_closed_loop_batch_fault call (host pointers; the fault rows are staged per chunk by closed_loop_run). Given only when
// at least one of the two is: with both absent the call is the rate / scenario call, launch for launch.
struct FaultRun {
    const float* fault;         // [Tf][Bf][m][2] or null
    int Tf, Bf;
    float* xsub;                // [B][T * substeps][13] or null
};
// SPEC.md §11f: the observation of one sdempc_closed_loop_batch_observed call (host pointers; the sigma / beta / valid rows are staged per chunk by closed_loop_run
// when they move). Given only when the call has an obs cfg: without one the call is the fault call, launch for launch.
struct ObsRun {
    const float *sigma, *beta;  // [To][Bo][12] or null (zeros)
    int To, Bo;
    const int32_t* valid;       // [Tv][Bv] or null (always valid)
    int Tv, Bv;
    const uint32_t* keys;       // [B][2]
    const float* xmeas_in;      // [B][13] or null (x0)
    float* xmeas;               // [B][Ns][13] or null
    uint32_t* keys_next;        // [B][2] or null
    float* xmeas_next;          // [B][13] or null
    // SPEC.md §11g (sdempc_closed_loop_batch_aged with an age cfg; all absent otherwise): the age rows are staged per chunk when they move, like valid
    const int32_t* age;         // [Ta][Ba] or null (every age 0)
    int Ta, Ba;
    int age_max;                // rows of the history; 0: no history
    bool renorm;
    const float* xhist_in;      // [B][age_max][13] or null (every row x0)
    float* xhist_next;          // [B][age_max][13] or null
};
// SPEC.md §11h: the scoring of one sdempc_closed_loop_batch_scored call (host pointers; the target rows are staged per chunk by closed_loop_run when they move).
// Given only when the call has a score cfg: without one the call is the aged call, launch for launch. With it the per-row outputs of the call may be NULL.
struct ScoreRun {
    const sdempc_score_cfg* cfg;
    const uint32_t* score_in;   // [B][16] or null (the initial row)
    uint32_t* score_out;        // [B][16]
};
// SPEC.md §11i: the processes of one sdempc_closed_loop_batch_drawn call (host pointers). Given only when the call has a process cfg: without one the call is the
// scored call, launch for launch.
struct ProcRun {
    const sdempc_process_cfg* dist;     // or null (W = 6, one step per control tick)
    const sdempc_process_cfg* bias;     // or null (W = 12, one step per solve)
    float* dist_rows;                   // [B][T][6] or null
    uint32_t* dist_keys_next;           // [B][2] or null
    float* dist_state_next;             // [B][6] or null
    float* bias_rows;                   // [B][Ns][12] or null
    uint32_t* bias_keys_next;           // [B][2] or null
    float* bias_state_next;             // [B][12] or null
};
// SPEC.md §11j: the trajectory set of one sdempc_closed_loop_batch_tracked / sdempc_reference_windows call, staged (stage_track). Given only when the call has a track
// cfg: without one the call is the drawn call, launch for launch.
struct TrackRun {
    LoopTrack K;                // device pointers of the staged set, dt, renorm; tick0 = the cfg's; B / rows / groups are set per launch
    bool score_targets;
};
// SPEC.md §11k: the event chains of one sdempc_closed_loop_batch_events call (host pointers). Given only when the call has an event cfg: without one the call is the
// tracked call, launch for launch.
struct EventRun {
    const sdempc_fault_process_cfg* fault;      // or null (m lanes, one step per control tick)
    const sdempc_dropout_process_cfg* drop;     // or null (one lane, one step per solve)
    float* fault_rows;                          // [B][T][m][2] or null
    uint32_t* fault_keys_next;                  // [B][2] or null
    int32_t* fault_state_next;                  // [B][m][2] or null
    int32_t* valid_rows;                        // [B][Ns] or null
    uint32_t* valid_keys_next;                  // [B][2] or null
    int32_t* valid_state_next;                  // [B][2] or null
};
// SPEC.md §11l: the baseline controller of one sdempc_closed_loop_batch_baseline call (host pointers, checked by check_geo). Given only by that entry point: without it
// the call is the events call, launch for launch.
struct GeoRun {
    const sdempc_geo_cfg* cfg;
    float inv_dt;                               // float32(1) / float32(time_steps[ref_row])
};
// SPEC.md §11m: the ensemble reducer of one sdempc_closed_loop_batch_ensemble call (host pointers, checked at the front of closed_loop_call). Given only when the
// call has an ensemble cfg: without one the call is the baseline (or, without a geo cfg, the events) call, launch for launch.
struct EnsRun {
    const sdempc_ensemble_cfg* cfg;
    uint32_t* out;                              // [R][G][W], R = T (tick score) or T * substeps (substep score)
};
// SPEC.md §11n: the outputs of one sdempc_closed_loop_batch_retire call (host pointers, checked at the front of closed_loop_call). Given only when the call has a
// retire cfg: without one the call is the ensemble call, launch for launch.
struct RetireRun {
    int32_t* retired_at;                        // [B]
    int32_t* live;                              // [Ns]
};
constexpr size_t ENS_SLAB_BYTES = 32u << 20;    // device bytes of partial words one pair of ensemble launches may fill: a chunk with more rows is reduced in slabs
constexpr size_t PROC_WORDS = 2 + 6 + 2 + 12 + 2 * 6 + 2 * 12;     // words of d_proc per row of max_batch
constexpr size_t EVT_MODES = 4;
constexpr size_t EVT_WORDS = EVENT_EP_WORDS + 2 + 2 + EVENT_PAR_WORDS + 2;      // words of d_evt per row of max_batch
static_assert(SDEMPC_MAX_MOTORS == 8, "EVENT_EP_WORDS / EVENT_PAR_WORDS (sdempc_kernels.h) hold eight motors");
inline int loop_solves(int T, int S) { return (int)(((long long)T + S - 1) / S); }       // Ns = ceil(T / S)
// One closed-loop call as its entry point describes it. The five entry points are five nested layers (SPEC.md §11, §11a .. §11d): each takes everything the one
// below it takes, so `layer` says which parts are present; the arguments of an absent part stay null.
enum LoopLayer { LOOP_PLAIN, LOOP_PLANT, LOOP_TIMED, LOOP_SCENARIO, LOOP_RATE };
struct LoopCall {
    LoopLayer layer;
    LoopIo io;                                  // (from LOOP_TIMED on, xref_ticks counts SOLVES)
    const sdempc_plant_cfg* pc;                 // LOOP_PLANT ..: the plant set
    const void* const* plant_blobs;
    const size_t* plant_blob_bytes;
    const int32_t* plant_of;                    // [B]; from LOOP_SCENARIO on [plant_ticks][B]
    const sdempc_timing_cfg* tc;                // LOOP_TIMED ..
    const float* u_act_in;
    float* u_act_next;
    const sdempc_scenario_cfg* sc;              // LOOP_SCENARIO ..; LOOP_RATE alone takes NULL (no scenario)
    const sdempc_rate_cfg* rc;                  // LOOP_RATE
    const float *rate_integ_in, *rate_tail_in;
    float *ws, *rate_integ_next, *rate_tail_next;
    bool faulted;                               // sdempc_closed_loop_batch_fault (SPEC.md §11e): LOOP_RATE or LOOP_SCENARIO (sc may then be NULL too) with fc / xsub
    const sdempc_fault_cfg* fc;                 // or NULL: no fault
    float* xsub;                                // or NULL
    bool observed;                              // sdempc_closed_loop_batch_observed (SPEC.md §11f): the fault call with oc and the five observation pointers
    const sdempc_obs_cfg* oc;                   // or NULL: no observation (the five pointers must then be NULL)
    const uint32_t* obs_keys;
    const float* xmeas_in;
    float* xmeas;
    uint32_t* obs_keys_next;
    float* xmeas_next;
    bool aged;                                  // sdempc_closed_loop_batch_aged (SPEC.md §11g): the observed call with ac and the two history pointers
    const sdempc_age_cfg* ac;                   // or NULL: no age (the two pointers must then be NULL)
    const float* xhist_in;
    float* xhist_next;
    bool scored;                                // sdempc_closed_loop_batch_scored (SPEC.md §11h): the aged call with zc and the two score pointers
    const sdempc_score_cfg* zc;                 // or NULL: no score (the two pointers must then be NULL, and no per-row output may be)
    const uint32_t* score_in;
    uint32_t* score_out;
    bool drawn;                                 // sdempc_closed_loop_batch_drawn (SPEC.md §11i): the scored call with the two process cfgs and their six outputs
    ProcRun pr;                                 // (a NULL cfg: its three outputs must be NULL)
    const sdempc_track_cfg* track;              // sdempc_closed_loop_batch_tracked (SPEC.md §11j): the drawn call with a trajectory set in place of xref; or NULL
    bool events;                                // sdempc_closed_loop_batch_events (SPEC.md §11k): the tracked call with the two event cfgs and their six outputs
    EventRun er;                                // (a NULL cfg: its three outputs must be NULL)
    bool baseline;                              // sdempc_closed_loop_batch_baseline (SPEC.md §11l): the events call with the geometric controller in place of the solve
    const sdempc_geo_cfg* geo;
    bool ensembled;                             // sdempc_closed_loop_batch_ensemble (SPEC.md §11m): the baseline call (geo NULL: the events call) with ens / ens_out
    const sdempc_ensemble_cfg* ens;             // or NULL: no ensemble (ens_out must then be NULL)
    uint32_t* ens_out;
    bool retiring;                              // sdempc_closed_loop_batch_retire (SPEC.md §11n): the ensemble call with retire / retired_at / live_per_solve
    const sdempc_retire_cfg* retire;            // or NULL: nobody is retired (the two outputs must then be NULL)
    int32_t* retired_at;
    int32_t* live_per_solve;
};
int check_geo(sdempc_handle* h, const sdempc_geo_cfg* g, int B, float* inv_dt);
int stage_geo(sdempc_handle* h, const sdempc_geo_cfg& g, hipStream_t st);
int closed_loop_call(sdempc_handle* h, const LoopCall& c);
int check_loop_args(sdempc_handle* h, const LoopIo& io, int solves, bool rows_optional = false, bool tracked = false);
int check_track(sdempc_handle* h, const sdempc_track_cfg* tk, int B, long long ticks);
int stage_track(sdempc_handle* h, const sdempc_track_cfg& tk, int B, TrackRun* out);
int check_plant_args(sdempc_handle* h, const sdempc_plant_cfg* pc, const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int B, int sched_rows);
int closed_loop_attempts(sdempc_handle* h, const LoopIo& io, const PlantRun* plant, const TimedRun* timed, const ScenarioRun* scen, const RateRun* rate, const FaultRun* flt = nullptr,
                         const ObsRun* obs = nullptr, const ScoreRun* score = nullptr, const ProcRun* proc = nullptr, const TrackRun* track = nullptr,
                         const EventRun* evt = nullptr, const GeoRun* geo = nullptr, const EnsRun* ens = nullptr, const RetireRun* ret = nullptr);
int closed_loop_run(sdempc_handle* h, const LoopIo& io, const PlantRun* plant, const TimedRun* timed, const ScenarioRun* scen, const RateRun* rate, const FaultRun* flt, const ObsRun* obs,
                    const ScoreRun* score, const ProcRun* proc, const TrackRun* track, const EventRun* evt, const GeoRun* geo, const EnsRun* ens, const RetireRun* ret, bool* again);
int stage_plants(sdempc_handle* h, const sdempc_plant_cfg& pc, const void* const* blobs, const int32_t* plant_of, int B, PlantRun* out, int xi_ticks = 1);
}  // namespace

extern "C" {

int sdempc_abi_version(void) { return SDEMPC_ABI_VERSION; }
int sdempc_build_flags(void) { return SDEMPC_ALL_VARIANTS ? SDEMPC_BUILD_ALL_VARIANTS : 0; }

const char* sdempc_last_error(const sdempc_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int sdempc_create(const sdempc_cfg* cfg, const void* model_blob, size_t blob_bytes, int32_t max_batch, sdempc_handle** out) {
    return guarded(nullptr, [&]() -> int {
    if (!out) return fail(nullptr, SDEMPC_EINVAL, "out is NULL%s");
    *out = nullptr;
    if (!cfg || cfg->struct_size != (int32_t)sizeof(sdempc_cfg)) return fail(nullptr, SDEMPC_EINVAL, "cfg NULL or struct_size mismatch%s");
    if (int rc = check_blob(nullptr, model_blob, blob_bytes)) return rc;
    const int32_t* hd = (const int32_t*)model_blob;
    const int m = hd[2];
    if (m < 1 || m > SDEMPC_MAX_MOTORS || m != cfg->num_motors) return fail(nullptr, SDEMPC_EINVAL, "num_motors of cfg and model blob differ or out of range%s");
    if (cfg->horizon < 1 || cfg->horizon > 4096 || cfg->num_particles < 1 || !cfg->time_steps || max_batch < 1)
        return fail(nullptr, SDEMPC_EINVAL, "horizon/num_particles/time_steps/max_batch invalid%s");
    if (cfg->max_iter < 0 || cfg->ls_maxls < 0 || cfg->max_no_improvement_iter < 1) return fail(nullptr, SDEMPC_EINVAL, "apg parameters invalid%s");
    if (cfg->num_state_constr < 0 || cfg->num_state_constr > SDEMPC_NX) return fail(nullptr, SDEMPC_EINVAL, "num_state_constr out of range%s");
    for (int k = 0; k < cfg->num_state_constr; ++k)
        if (cfg->state_id[k] < 0 || cfg->state_id[k] >= SDEMPC_NX || (k > 0 && cfg->state_id[k] <= cfg->state_id[k - 1]))
            return fail(nullptr, SDEMPC_EINVAL, "state_id must be strictly ascending indices into the 13-state%s");
    for (int t = 0; t < cfg->horizon; ++t)
        if (!(cfg->time_steps[t] > 0.0f)) return fail(nullptr, SDEMPC_EINVAL, "time_steps must be positive%s");
    if (smem_bytes(cfg->horizon, m, team_ipb((cfg->num_particles + 31) / 32, cfg->horizon, m)) > 160 * 1024) return fail(nullptr, SDEMPC_EINVAL, "horizon too large for one workgroup's LDS (160 KiB)%s");
    if (cfg->max_iter > 10 * 1000 * 1000) return fail(nullptr, SDEMPC_EINVAL, "max_iter beyond 10^7%s");
    std::unique_ptr<sdempc_handle> hp(new (std::nothrow) sdempc_handle());      // released into *out on success only
    sdempc_handle* h = hp.get();
    if (!h) return fail(nullptr, SDEMPC_ENOMEM, "out of memory%s");
    h->cfg = *cfg;
    h->H = cfg->horizon; h->P = cfg->num_particles; h->m = m; h->G = (h->P + 31) / 32; h->max_batch = max_batch;
    h->time_steps.assign(cfg->time_steps, cfg->time_steps + h->H);
    h->cfg.time_steps = h->time_steps.data();
    const float* f = (const float*)(hd + SDEMPC_BLOB_HEADER_INTS);
    if (cfg->mlp_dtype < 0 || cfg->mlp_dtype > 2) return fail(nullptr, SDEMPC_EINVAL, "mlp_dtype must be 0 (f32), 1 (f16) or 2 (f32x3)%s");
    if (cfg->math_mode != 0 && cfg->math_mode != 1) return fail(nullptr, SDEMPC_EINVAL, "math_mode must be 0 (exact) or 1 (fast)%s");
    PreparedModel pm;
    if (const char* why = prepare_model(f, cfg->mlp_dtype, cfg->math_mode, h->time_steps.data(), h->H, pm)) return fail(nullptr, SDEMPC_EINVAL, "model refused: %s", why);
    h->blob_f = std::move(pm.blob_f);
    // tables (SPEC.md §5: float32 host arithmetic)
    h->h_sdt = std::move(pm.sdt);
    h->h_disc.resize(h->H + 1);
    float d = 1.0f / (float)h->H;
    for (int t = 0; t <= h->H; ++t) { h->h_disc[t] = d; d = d * cfg->discount; }
    h->h_beta.resize(cfg->max_iter + 2);
    for (int i = 0; i < cfg->max_iter + 2; ++i) {
        float b = (i == 0) ? cfg->beta_init : (float)(i + 1) / (float)(i + 4);
        if (i > 0 && cfg->use_moment_scale) b = cfg->moment_scale * b;
        h->h_beta[i] = b;
    }
    // kernel argument block
    KArgs& a = h->base;
    memset(&a, 0, sizeof a);
    a.H = h->H; a.P = h->P; a.m = m; a.G = h->G;
    a.invP = 1.0f / (float)h->P;
    a.f16 = cfg->mlp_dtype;              // 0 f32, 1 fp16 operands (SPEC.md §9), 2 three-limb bf16 split of the layer-2 contractions (§9b)
    a.fast = cfg->math_mode == 1;
    a.M = pm.M;
    for (int i = 0; i < 3; ++i) { a.C.perr[i] = cfg->perr[i]; a.C.verr[i] = cfg->verr[i]; a.C.qerr[i] = cfg->qerr[i]; a.C.werr[i] = cfg->werr[i]; }
    a.C.res_mult = cfg->res_mult; a.C.uerr = cfg->uerr; a.C.slew = cfg->u_slew_coeff; a.C.slew_cc = cfg->u_slew_constr_coeff;
    a.C.has_sc = cfg->has_slew_constr;
    for (int j = 0; j < 8; ++j) {
        a.C.slew_lo[j] = cfg->u_slew_lo[j]; a.C.slew_hi[j] = cfg->u_slew_hi[j]; a.C.uref[j] = cfg->uref[j];
        a.C.ulo[j] = cfg->u_lo[j]; a.C.uhi[j] = cfg->u_hi[j];
    }
    a.C.sc_n = 0; a.C.sc_tab = nullptr;       // the table goes to the device with the other tables (ensure_device)
    // KArgs::nonneg: every weight a cost term is multiplied by is >= 0 (a NaN compares false). Each term is then fma(w * e, e, l) or d * c with
    // non-negative operands, rounding is monotone, and so no stage, control or total cost is negative (SPEC.md §8, implementation note).
    bool nonneg = cfg->res_mult >= 0.0f && cfg->uerr >= 0.0f && cfg->u_slew_coeff >= 0.0f && cfg->u_slew_constr_coeff >= 0.0f;
    for (int i = 0; i < 3; ++i) nonneg = nonneg && cfg->perr[i] >= 0.0f && cfg->verr[i] >= 0.0f && cfg->qerr[i] >= 0.0f && cfg->werr[i] >= 0.0f;
    for (int k = 0; k < cfg->num_state_constr; ++k) nonneg = nonneg && cfg->state_w[k] >= 0.0f;
    for (int t = 0; t <= h->H; ++t) nonneg = nonneg && h->h_disc[t] >= 0.0f;
    a.nonneg = nonneg ? 1 : 0;
    a.A.max_iter = cfg->max_iter; a.A.max_noimp = cfg->max_no_improvement_iter; a.A.maxls = cfg->ls_maxls;
    a.A.reset_inc = cfg->ls_reset_option == 1;
    a.A.atol = cfg->atol; a.A.rtol = cfg->rtol; a.A.stepsize = cfg->stepsize; a.A.smax = cfg->ls_max_stepsize;
    a.A.coef = cfg->ls_coef; a.A.dec = cfg->ls_decrease_factor; a.A.inc = cfg->ls_increase_factor;
    default_options(h);
    *out = hp.release();
    return SDEMPC_OK;
    });
}

void sdempc_destroy(sdempc_handle* h) {
    if (!h) return;
    release_device(h);
    delete h;
}

}  // extern "C"

namespace {
void release_device(sdempc_handle* h) {
    if (h->dev_ready || h->stream || h->d_dt.p) {
        (void)hipSetDevice(h->device);
        for (DevBuf* b : {&h->d_sctab, &h->d_ustg, &h->d_part, &h->d_act, &h->d_dt, &h->d_sdt, &h->d_disc, &h->d_beta, &h->d_wts, &h->d_traj, &h->d_x0, &h->d_u, &h->d_xref, &h->d_noise, &h->d_noise_canon, &h->d_traj_canon, &h->d_keys, &h->d_tube, &h->d_band, &h->d_risk, &h->d_outcome, &h->d_loop, &h->d_loop_chunk, &h->d_plant, &h->d_rate, &h->d_obs, &h->d_hist, &h->d_score, &h->d_ens, &h->d_retire, &h->d_proc, &h->d_evt, &h->d_geo, &h->d_track, &h->d_work, &h->d_coop_bar, &h->d_coop_pp, &h->d_coop_ck,
                          &h->d_step, &h->d_cost, &h->d_grad, &h->d_xmean, &h->d_uopt, &h->d_info})
            dev_free(*b);
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        h->ev0 = h->ev1 = nullptr; h->stream = nullptr; h->coop_cap = 0; h->ws_rows = 0;
    }
    h->dev_ready = false; h->timed = false;
}
}  // namespace

extern "C" {

int sdempc_set_device(sdempc_handle* h, int32_t device) {
    return guarded(h, [&]() -> int {
    if (!h) return SDEMPC_EINVAL;
    if (h->dev_ready) return fail(h, SDEMPC_EINVAL, "sdempc_set_device must precede the first device call%s");
    if (device < 0) return fail(h, SDEMPC_EINVAL, "negative device ordinal%s");
    h->device = device;
    return SDEMPC_OK;
    });
}

int sdempc_device_ready(const sdempc_handle* h) { return h && h->dev_ready ? 1 : 0; }

int sdempc_set_option(sdempc_handle* h, int32_t key, int32_t value) {
    return guarded(h, [&]() -> int {
    if (!h) return SDEMPC_EINVAL;
    LaunchOpts& o = h->base.opt;
    auto flag = [&](int& dst) { if (value != 0 && value != 1) return fail(h, SDEMPC_EINVAL, "option value must be 0 or 1%s"); dst = value; return (int)SDEMPC_OK; };
    auto tri = [&](int& dst) { if (value < -1 || value > 1) return fail(h, SDEMPC_EINVAL, "option value must be -1 (auto), 0 or 1%s"); dst = value; return (int)SDEMPC_OK; };
    switch (key) {
        case SDEMPC_OPT_LANE: return flag(o.lane);
        case SDEMPC_OPT_COOP: { int rc = flag(o.coop); if (rc == SDEMPC_OK && value == 1) h->coop_off = false; return rc; }
        case SDEMPC_OPT_SPEC: return flag(o.spec);
        case SDEMPC_OPT_PK:
            if (value == 1 && !SDEMPC_ALL_VARIANTS) return fail(h, SDEMPC_EINVAL, "this build carries no packed-tanh instantiations (make EXTRA=-DSDEMPC_ALL_VARIANTS=1)%s");
            return tri(o.pk);
        case SDEMPC_OPT_USTG: return tri(o.ustg);
        case SDEMPC_OPT_DUO: return tri(o.duo);
        case SDEMPC_OPT_COOP_LAUNCH: return flag(o.coop_launch);
        case SDEMPC_OPT_COOP_FENCE: return flag(o.coop_fence);
        case SDEMPC_OPT_HEX: return flag(o.hex);
        case SDEMPC_OPT_TEST_ABSENT_WG:
            if (value < -1) return fail(h, SDEMPC_EINVAL, "absent workgroup must be -1 (none) or a workgroup index%s");
            o.absent_wg = value;
            return SDEMPC_OK;
        case SDEMPC_OPT_TEST_WS_FILL:
            if (value < -1 || value > 255) return fail(h, SDEMPC_EINVAL, "workspace fill must be -1 (none) or a byte value 0..255%s");
            h->ws_fill = value;
            return SDEMPC_OK;
        case SDEMPC_OPT_COOP_SPIN_US:
            if (value < -1) return fail(h, SDEMPC_EINVAL, "spin budget must be -1 (derived) or >= 0 microseconds%s");
            h->spin_us = value;
            return SDEMPC_OK;
        case SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES:
            if (value < -1) return fail(h, SDEMPC_EINVAL, "loop chunk bytes must be -1 (built-in) or >= 0%s");
            h->loop_chunk_bytes = value;
            return SDEMPC_OK;
        default: return fail(h, SDEMPC_EINVAL, "unknown option key%s");
    }
    });
}

int sdempc_get_option(const sdempc_handle* h, int32_t key, int32_t* value) {
    return guarded(h, [&]() -> int {
    if (!h || !value) return SDEMPC_EINVAL;
    const LaunchOpts& o = h->base.opt;
    switch (key) {
        case SDEMPC_OPT_LANE: *value = o.lane; break;
        case SDEMPC_OPT_COOP: *value = o.coop && !h->coop_off; break;
        case SDEMPC_OPT_SPEC: *value = o.spec; break;
        case SDEMPC_OPT_PK: *value = o.pk; break;
        case SDEMPC_OPT_USTG: *value = o.ustg; break;
        case SDEMPC_OPT_DUO: *value = o.duo; break;
        case SDEMPC_OPT_COOP_LAUNCH: *value = o.coop_launch; break;
        case SDEMPC_OPT_COOP_FENCE: *value = o.coop_fence; break;
        case SDEMPC_OPT_HEX: *value = o.hex; break;
        case SDEMPC_OPT_TEST_ABSENT_WG: *value = o.absent_wg; break;
        case SDEMPC_OPT_TEST_WS_FILL: *value = h->ws_fill; break;
        case SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES: *value = h->loop_chunk_bytes; break;
        case SDEMPC_OPT_COOP_SPIN_US: *value = h->spin_us >= 0 ? h->spin_us : (int32_t)(coop_spin_ticks(h) / 100u); break;
        case SDEMPC_OPT_DEVICE_CUS: *value = o.cus; break;
        default: return SDEMPC_EINVAL;
    }
    return SDEMPC_OK;
    });
}

int sdempc_reset(sdempc_handle* h, const float* x, const float* xdes, float* yk, sdempc_info* info) {
    return guarded(h, [&]() -> int {
    if (!h || !yk || !info) return SDEMPC_EINVAL;
    (void)x; (void)xdes;
    for (int t = 0; t < h->H; ++t)
        for (int j = 0; j < h->m; ++j) yk[t * h->m + j] = h->cfg.uref[j];
    memset(info, 0, sizeof *info);
    info->stepsize = h->cfg.ls_maxls > 0 ? h->cfg.ls_init_stepsize : h->cfg.stepsize;
    return SDEMPC_OK;
    });
}

size_t sdempc_noise_dev_floats(const sdempc_handle* h, int32_t B) { return h ? noise_floats(h, B) : 0; }
size_t sdempc_traj_dev_floats(const sdempc_handle* h, int32_t B) { return h ? traj_floats(h, B) : 0; }

int sdempc_noise_to_device_layout(const sdempc_handle* h, int32_t B, const float* noise_host, float* out_host) {
    return guarded(h, [&]() -> int {
    if (!h || !noise_host || !out_host || B < 1) return SDEMPC_EINVAL;
    noise_to_dev_layout(h, B, noise_host, out_host);
    return SDEMPC_OK;
    });
}

int sdempc_noise_to_device_layout_dev(sdempc_handle* h, int32_t B, const void* noise_canonical_dev, void* noise_out_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!noise_canonical_dev || !noise_out_dev) return fail(h, SDEMPC_EINVAL, "NULL device pointer%s");
    if ((rc = ensure_device(h))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(h, launch_relayout(true, (const float*)noise_canonical_dev, (float*)noise_out_dev, B, h->P, h->G, h->H * SDEMPC_NNOISE, st));
    return SDEMPC_OK;
    });
}

int sdempc_traj_to_canonical_dev(sdempc_handle* h, int32_t B, void* traj_out_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!traj_out_dev) return fail(h, SDEMPC_EINVAL, "NULL device pointer%s");
    if ((rc = ensure_device(h))) return rc;
    if ((rc = check_traj_held(h, B))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(h, launch_relayout(false, (const float*)h->d_traj.p, (float*)traj_out_dev, B, h->P, h->G, (h->H + 1) * SDEMPC_NX, st));
    return SDEMPC_OK;
    });
}

int sdempc_rollout_batch_dev(sdempc_handle* h, int32_t B, const void* x0_dev, const void* u_dev, const void* xref_dev, const void* noise_dev,
                             void* cost_dev, void* xmean_dev, int32_t store_traj, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0_dev || !u_dev || !xref_dev || !noise_dev || !cost_dev) return fail(h, SDEMPC_EINVAL, "NULL device pointer%s");
    if ((rc = ensure_device(h))) return rc;
    if ((rc = ensure_workspace(h, B))) return rc;
    KArgs a = h->base;
    a.x0 = (const float*)x0_dev; a.u = (const float*)u_dev; a.xref = (const float*)xref_dev; a.noise = (const float*)noise_dev;
    a.cost = (float*)cost_dev; a.xmean = (float*)xmean_dev; a.store_traj = store_traj;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    h->traj_batch = 0;
    rc = timed_launch(h, st, [&] { return launch_rollout(a, B, st); });
    if (rc == SDEMPC_OK && store_traj) h->traj_batch = B;
    return rc;
    });
}

int sdempc_grad_batch_dev(sdempc_handle* h, int32_t B, const void* x0_dev, const void* u_dev, const void* xref_dev, const void* noise_dev,
                          void* cost_dev, void* grad_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0_dev || !u_dev || !xref_dev || !noise_dev || !cost_dev || !grad_dev) return fail(h, SDEMPC_EINVAL, "NULL device pointer%s");
    if ((rc = ensure_device(h))) return rc;
    if ((rc = ensure_workspace(h, B))) return rc;
    KArgs a = h->base;
    a.x0 = (const float*)x0_dev; a.u = (const float*)u_dev; a.xref = (const float*)xref_dev; a.noise = (const float*)noise_dev;
    a.cost = (float*)cost_dev; a.grad = (float*)grad_dev;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    h->traj_batch = 0;       // (the gradient's forward sweep streams x_t through the trajectory workspace)
    return timed_launch(h, st, [&] { return launch_grad(a, B, st); });
    });
}

int sdempc_solve_batch_dev(sdempc_handle* h, int32_t B, const void* x0_dev, const void* xref_dev, const void* noise_dev, const void* u_init_dev,
                           const void* stepsize_dev, void* uopt_dev, void* xevol_dev, void* info_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0_dev || !xref_dev || !noise_dev || !u_init_dev || !stepsize_dev || !uopt_dev || !xevol_dev || !info_dev)
        return fail(h, SDEMPC_EINVAL, "NULL device pointer%s");
    if ((rc = ensure_device(h))) return rc;
    {   // workspace rows of this launch: the batch, or the team slots of a persistent throughput launch
        KArgs probe = h->base; probe.B = B;
        if ((rc = ensure_workspace(h, solve_workspace_rows(probe, B)))) return rc;
    }
    h->traj_batch = 0;       // (a solve's gradient evaluations stream through the trajectory workspace, indexed by team slot)
    KArgs a = h->base;
    a.x0 = (const float*)x0_dev; a.u = (const float*)u_init_dev; a.xref = (const float*)xref_dev; a.noise = (const float*)noise_dev;
    a.stepsize_in = (const float*)stepsize_dev; a.uopt = (float*)uopt_dev; a.xmean = (float*)xevol_dev; a.info = (float*)info_dev;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // Small batches of multi-particle instances: one instance over ceil(P/4) workgroups, one particle per wave (latency path).
    // Same results bit for bit; only taken when every workgroup of the grid is resident at once.
    const bool coop_ok = !a.f16 && !h->coop_off && a.C.sc_n == 0;     // lane layouts: f32 contractions (either math mode), built without the state-bound terms
    const int smax = coop_ok ? spec_max_instances(h->P, h->H, h->m, a.opt) : 0;
    int cmax = coop_ok ? coop_max_instances(h->P, h->H, h->m, a.opt) : 0;
    if (smax > cmax) cmax = smax;
    if (B <= cmax) {
        if (!h->d_coop_bar.p) {
            const int cap = cmax < h->max_batch ? cmax : h->max_batch;
            if ((rc = dev_alloc(h, h->d_coop_bar, sizeof(unsigned) * COOP_BAR_WORDS * (size_t)cap))) return rc;
            if ((rc = dev_alloc(h, h->d_coop_pp, sizeof(float) * coop_pp_floats(h->H, h->G) * cap, true))) return rc;
            if ((rc = dev_alloc(h, h->d_coop_ck, sizeof(float) * coop_ck_floats(h->H, h->P) * cap, true))) return rc;
            h->coop_cap = cap;
        }
        if (B <= h->coop_cap) {
            HIPCHK(h, hipMemsetAsync(h->d_coop_bar.p, 0, sizeof(unsigned) * COOP_BAR_WORDS * (size_t)B, st));
            a.coop_bar = (unsigned*)h->d_coop_bar.p; a.coop_pp = (float*)h->d_coop_pp.p; a.coop_ck = (float*)h->d_coop_ck.p;
            a.coop_spin = coop_spin_ticks(h);
            h->last_coop_B = B; h->last_ticketed = false;
            if (B <= smax) {
                // the speculative kernel's outputs are tagged words {value, tag} that readers poll (streamed hand-off, sdempc_spec.inc.h): no tag of an
                // earlier launch may survive (12 MB per C2 instance, a few microseconds of the 20 ms the launch takes)
                HIPCHK(h, hipMemsetAsync(h->d_coop_pp.p, 0, sizeof(float) * coop_pp_floats(h->H, h->G) * (size_t)B, st));
                return timed_launch(h, st, [&] { return launch_solve_spec(a, B, st); });
            }
            if (B <= coop_max_instances(h->P, h->H, h->m, a.opt)) return timed_launch(h, st, [&] { return launch_solve_coop(a, B, st); });
            h->last_coop_B = 0;
        }
    }
    h->last_coop_B = 0;
    const unsigned tickets_before = h->ticket_total;
    rc = timed_launch(h, st, [&] { return launch_solve(a, B, st); });
    h->last_ticketed = rc == SDEMPC_OK && h->ticket_total != tickets_before;
    return rc;
    });
}

int sdempc_noise_from_keys_dev(sdempc_handle* h, int32_t B, const uint32_t* keys, void* noise_out_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!keys || !noise_out_dev) return fail(h, SDEMPC_EINVAL, "NULL pointer%s");
    if ((rc = ensure_device(h))) return rc;
    return noise_from_keys(h, B, keys, (float*)noise_out_dev, stream ? (hipStream_t)stream : h->stream);
    });
}

int sdempc_noise_from_keys(sdempc_handle* h, int32_t B, const uint32_t* keys, float* noise) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!keys || !noise) return fail(h, SDEMPC_EINVAL, "NULL pointer%s");
    if ((rc = ensure_device(h))) return rc;
    const size_t nf = (size_t)h->P * h->H * SDEMPC_NNOISE;
    if (!h->d_noise_canon.p && (rc = dev_alloc(h, h->d_noise_canon, sizeof(float) * (size_t)h->max_batch * nf, true))) return rc;
    if ((rc = noise_from_keys(h, B, keys, (float*)h->d_noise.p, h->stream))) return rc;
    HIPCHK(h, launch_relayout(false, (const float*)h->d_noise.p, (float*)h->d_noise_canon.p, B, h->P, h->G, h->H * SDEMPC_NNOISE, h->stream));
    HIPCHK(h, hipMemcpyAsync(noise, h->d_noise_canon.p, sizeof(float) * B * nf, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
    });
}

int sdempc_last_kernel_name(const sdempc_handle* h, char* buf, size_t n) {
    return guarded(h, [&]() -> int {
    if (!h || !buf || n < 2) return SDEMPC_EINVAL;
    buf[0] = 0;
    if (!h->last_fn) return SDEMPC_OK;
    const char* mangled = hipKernelNameRefByPtr(h->last_fn, h->stream);
    if (!mangled) return SDEMPC_OK;
    int status = 0;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    std::string name = (status == 0 && dem) ? dem : mangled;
    free(dem);
    if (name.rfind("void ", 0) == 0) name = name.substr(5);
    const size_t par = name.rfind("(sdempc::KArgs)");
    if (par != std::string::npos) name = name.substr(0, par);
    snprintf(buf, n, "%s", name.c_str());
    return SDEMPC_OK;
    });
}

float sdempc_last_kernel_ms(const sdempc_handle* h) {
    if (!h || !h->timed) return -1.0f;
    if (hipEventSynchronize(h->ev1) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) return -1.0f;
    return ms;
}

int sdempc_rollout_batch(sdempc_handle* h, int32_t B, const float* x0, const float* u, const float* xref, const float* noise, float* cost,
                         float* traj, float* xmean) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !noise || !cost) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = ensure_device(h))) return rc;
    if ((rc = stage_common(h, B, x0, u, xref, noise))) return rc;
    rc = sdempc_rollout_batch_dev(h, B, h->d_x0.p, h->d_u.p, h->d_xref.p, h->d_noise.p, h->d_cost.p, xmean ? h->d_xmean.p : nullptr, traj ? 1 : 0, h->stream);
    if (rc) return rc;
    const int H = h->H, P = h->P;
    HIPCHK(h, hipMemcpyAsync(cost, h->d_cost.p, sizeof(float) * B, hipMemcpyDeviceToHost, h->stream));
    if (xmean) HIPCHK(h, hipMemcpyAsync(xmean, h->d_xmean.p, sizeof(float) * B * (H + 1) * SDEMPC_NX, hipMemcpyDeviceToHost, h->stream));
    if (traj) {
        const size_t nf = (size_t)P * (H + 1) * SDEMPC_NX;
        if (!h->d_traj_canon.p && (rc = dev_alloc(h, h->d_traj_canon, sizeof(float) * h->max_batch * nf, true))) return rc;
        if ((rc = sdempc_traj_to_canonical_dev(h, B, h->d_traj_canon.p, h->stream))) return rc;
        HIPCHK(h, hipMemcpyAsync(traj, h->d_traj_canon.p, sizeof(float) * B * nf, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
    });
}

int sdempc_grad_batch(sdempc_handle* h, int32_t B, const float* x0, const float* u, const float* xref, const float* noise, float* cost, float* grad) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !noise || !cost || !grad) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = ensure_device(h))) return rc;
    if ((rc = stage_common(h, B, x0, u, xref, noise))) return rc;
    rc = sdempc_grad_batch_dev(h, B, h->d_x0.p, h->d_u.p, h->d_xref.p, h->d_noise.p, h->d_cost.p, h->d_grad.p, h->stream);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(cost, h->d_cost.p, sizeof(float) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(grad, h->d_grad.p, sizeof(float) * B * h->H * h->m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
    });
}

int sdempc_solve_batch(sdempc_handle* h, int32_t B, const float* x0, const float* xref, const float* noise, const float* u_init,
                       const float* stepsize_in, float* uopt, float* xevol, sdempc_info* info) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !xref || !noise || !u_init || !stepsize_in || !uopt || !xevol || !info) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = ensure_device(h))) return rc;
    if ((rc = stage_common(h, B, x0, u_init, xref, noise))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_step.p, stepsize_in, sizeof(float) * B, hipMemcpyHostToDevice, h->stream));
    return solve_staged(h, B, uopt, xevol, info);
    });
}

int sdempc_solve_batch_keys(sdempc_handle* h, int32_t B, const float* x0, const float* xref, const uint32_t* keys, const float* u_init,
                            const float* stepsize_in, float* uopt, float* xevol, sdempc_info* info) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !xref || !keys || !u_init || !stepsize_in || !uopt || !xevol || !info) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = ensure_device(h))) return rc;
    const int H = h->H, m = h->m;
    HIPCHK(h, hipMemcpyAsync(h->d_x0.p, x0, sizeof(float) * B * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_u.p, u_init, sizeof(float) * B * H * m, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_xref.p, xref, sizeof(float) * B * (H + 1) * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_step.p, stepsize_in, sizeof(float) * B, hipMemcpyHostToDevice, h->stream));
    if ((rc = noise_from_keys(h, B, keys, (float*)h->d_noise.p, h->stream))) return rc;
    return solve_staged(h, B, uopt, xevol, info);
    });
}

int sdempc_tube_batch_dev(sdempc_handle* h, const sdempc_tube_cfg* cfg, int32_t B, void* mean_dev, void* var_dev, void* min_dev, void* max_dev, void* outside_dev,
                          void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if ((rc = check_tube(h, cfg, mean_dev, var_dev, min_dev, max_dev, outside_dev))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = check_traj_held(h, B))) return rc;
    TubeArgs T{};
    T.traj = (const float*)h->d_traj.p;
    T.mean = (float*)mean_dev; T.var = (float*)var_dev; T.mn = (float*)min_dev; T.mx = (float*)max_dev; T.outside = (uint32_t*)outside_dev;
    if (cfg)
        for (int i = 0; i < SDEMPC_NX; ++i) { T.lo[i] = cfg->lo[i]; T.hi[i] = cfg->hi[i]; }
    T.invP = h->base.invP;
    T.C = (h->H + 1) * SDEMPC_NX;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(h, launch_tube(T, B, h->P, h->G, h->H, st));
    return SDEMPC_OK;
    });
}

namespace {
// the staged inputs (d_x0, d_u, d_xref, d_noise on the handle's stream) -> one store_traj rollout, the reducer, the planes asked for back on the host
int tube_staged(sdempc_handle* h, const sdempc_tube_cfg* cfg, int32_t B, float* cost, float* mean, float* var, float* mn, float* mx, uint32_t* outside) {
    int rc = sdempc_rollout_batch_dev(h, B, h->d_x0.p, h->d_u.p, h->d_xref.p, h->d_noise.p, h->d_cost.p, nullptr, 1, h->stream);
    if (rc) return rc;
    const size_t n = (size_t)(h->H + 1) * SDEMPC_NX, plane = sizeof(float) * (size_t)h->max_batch * n;
    if (!h->d_tube.p && (rc = dev_alloc(h, h->d_tube, 5 * plane, true))) return rc;
    char* d = (char*)h->d_tube.p;
    void* host[5] = {mean, var, mn, mx, outside};
    void* dev[5];
    for (int k = 0; k < 5; ++k) dev[k] = host[k] ? d + k * plane : nullptr;
    if ((rc = sdempc_tube_batch_dev(h, cfg, B, dev[0], dev[1], dev[2], dev[3], dev[4], h->stream))) return rc;
    if (cost) HIPCHK(h, hipMemcpyAsync(cost, h->d_cost.p, sizeof(float) * B, hipMemcpyDeviceToHost, h->stream));
    for (int k = 0; k < 5; ++k)
        if (host[k]) HIPCHK(h, hipMemcpyAsync(host[k], dev[k], sizeof(float) * B * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
}
}  // namespace

int sdempc_tube_batch(sdempc_handle* h, const sdempc_tube_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const float* noise, float* cost,
                      float* mean, float* var, float* min, float* max, uint32_t* outside) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !noise) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = check_tube(h, cfg, mean, var, min, max, outside))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = stage_common(h, B, x0, u, xref, noise))) return rc;
    return tube_staged(h, cfg, B, cost, mean, var, min, max, outside);
    });
}

int sdempc_tube_batch_keys(sdempc_handle* h, const sdempc_tube_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const uint32_t* keys, float* cost,
                           float* mean, float* var, float* min, float* max, uint32_t* outside) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !keys) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = check_tube(h, cfg, mean, var, min, max, outside))) return rc;
    if ((rc = ensure_device(h))) return rc;
    const int H = h->H, m = h->m;
    HIPCHK(h, hipMemcpyAsync(h->d_x0.p, x0, sizeof(float) * B * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_u.p, u, sizeof(float) * B * H * m, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_xref.p, xref, sizeof(float) * B * (H + 1) * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    if ((rc = noise_from_keys(h, B, keys, (float*)h->d_noise.p, h->stream))) return rc;
    return tube_staged(h, cfg, B, cost, mean, var, min, max, outside);
    });
}

// ---- predicted risk (SPEC.md §12a) ----
namespace {
struct RiskOut { void *exit, *jx, *first_exit, *outside_any, *jstat, *jq, *jtail; };
constexpr int RISK_REGIONS = 10;     // lo, hi, centre, then the seven outputs in RiskOut's order

// byte offsets of d_risk's regions, each sized for max_batch instances; off[RISK_REGIONS] = total
void risk_regions(const sdempc_handle* h, size_t* off, size_t* per_instance) {
    const size_t C = (size_t)(h->H + 1) * SDEMPC_NX;
    const size_t words[RISK_REGIONS] = {SDEMPC_NX, SDEMPC_NX, C, (size_t)h->P, (size_t)h->P, (size_t)h->H + 2, (size_t)h->H + 1, 4, RISK_MAX_RANKS, 1};
    size_t o = 0;
    for (int k = 0; k < RISK_REGIONS; ++k) {
        off[k] = o;
        if (per_instance) per_instance[k] = sizeof(float) * words[k];
        o += (sizeof(float) * words[k] * (size_t)h->max_batch + 255) & ~(size_t)255;
    }
    off[RISK_REGIONS] = o;
}

int ensure_risk_buf(sdempc_handle* h) {
    if (h->d_risk.p) return 0;
    size_t off[RISK_REGIONS + 1];
    risk_regions(h, off, nullptr);
    return dev_alloc(h, h->d_risk, off[RISK_REGIONS], true);
}

// every check of a risk request (SPEC.md §12a) that needs no device; no HIP call. have_*: whether the caller gave that input.
int check_risk(sdempc_handle* h, const sdempc_risk_cfg* cfg, bool have_lo, bool have_hi, bool have_centre, bool have_xref, const RiskOut& O) {
    if (!cfg) return fail(h, SDEMPC_EINVAL, "NULL sdempc_risk_cfg%s");
    if (cfg->struct_size != (int32_t)sizeof(sdempc_risk_cfg)) return fail(h, SDEMPC_EINVAL, "sdempc_risk_cfg.struct_size mismatch%s");
    const bool want_x = O.exit || O.first_exit || O.outside_any, want_j = O.jx || O.jstat || O.jq || O.jtail;
    if (!want_x && !want_j) return fail(h, SDEMPC_EINVAL, "no output asked for: exit, jx, first_exit, outside_any, jstat, jq and jtail are all NULL%s");
    if (cfg->centre_mode < 0 || cfg->centre_mode > 3) return fail(h, SDEMPC_EINVAL, "sdempc_risk_cfg.centre_mode out of range (0 none, 1 caller's rows, 2 xref, 3 particle mean)%s");
    if (have_lo != have_hi) return fail(h, SDEMPC_EINVAL, "lo and hi come together%s");
    if (want_x && !have_lo) return fail(h, SDEMPC_EINVAL, "exit, first_exit and outside_any need bounds (lo, hi)%s");
    if (want_x && cfg->centre_mode == 1 && !have_centre) return fail(h, SDEMPC_EINVAL, "centre_mode 1 needs the caller's centre rows%s");
    if ((want_j || (want_x && cfg->centre_mode == 2)) && !have_xref) return fail(h, SDEMPC_EINVAL, "jx, jstat, jq, jtail and centre_mode 2 need xref%s");
    if (O.jq) {
        if (cfg->n_ranks < 1 || cfg->n_ranks > RISK_MAX_RANKS) return fail(h, SDEMPC_EINVAL, "jq needs 1 <= sdempc_risk_cfg.n_ranks <= 8%s");
        for (int k = 0; k < cfg->n_ranks; ++k)
            if (cfg->ranks[k] < 0 || cfg->ranks[k] >= h->P) return fail(h, SDEMPC_EINVAL, "a rank of sdempc_risk_cfg.ranks is outside 0 .. P-1%s");
    }
    if (O.jtail && (cfg->tail_k < 1 || cfg->tail_k > h->P)) return fail(h, SDEMPC_EINVAL, "jtail needs 1 <= sdempc_risk_cfg.tail_k <= P%s");
    if ((O.jq || O.jtail) && h->P > RISK_RANK_MAX_P) return fail(h, SDEMPC_EINVAL, "jq and jtail are limited to 4096 particles (the selection stage); the other outputs are not%s");
    if (sizeof(uint32_t) * risk_lds_words_host(h->H, h->G) > RISK_MAX_LDS)
        return fail(h, SDEMPC_EINVAL, "horizon and particle count too large for the risk reducer's workgroup memory (4 (2 H + 29 + 37 ceil(P / 32)) bytes > 64 KiB)%s");
    return 0;
}

int check_risk_bounds(sdempc_handle* h, int B, const float* lo, const float* hi) {
    if (lo && hi)
        for (size_t i = 0; i < (size_t)B * SDEMPC_NX; ++i)
            if (lo[i] != lo[i] || hi[i] != hi[i]) return fail(h, SDEMPC_EINVAL, "a risk bound is NaN (use -inf / +inf for no bound)%s");
    return 0;
}
}  // namespace

int sdempc_risk_batch_dev(sdempc_handle* h, const sdempc_risk_cfg* cfg, int32_t B, const void* lo_dev, const void* hi_dev, const void* centre_dev, const void* xref_dev,
                          void* exit_dev, void* jx_dev, void* first_exit_dev, void* outside_any_dev, void* jstat_dev, void* jq_dev, void* jtail_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    const RiskOut O{exit_dev, jx_dev, first_exit_dev, outside_any_dev, jstat_dev, jq_dev, jtail_dev};
    if ((rc = check_risk(h, cfg, lo_dev != nullptr, hi_dev != nullptr, centre_dev != nullptr, xref_dev != nullptr, O))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = check_traj_held(h, B))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const bool want_x = exit_dev || first_exit_dev || outside_any_dev;
    RiskArgs R{};
    R.traj = (const float*)h->d_traj.p;
    R.xref = (const float*)xref_dev;
    R.disc = h->base.disc;
    if (want_x) {
        R.lo = (const float*)lo_dev; R.hi = (const float*)hi_dev;
        if (cfg->centre_mode == 1) R.centre = (const float*)centre_dev;
        else if (cfg->centre_mode == 2) R.centre = (const float*)xref_dev;
        else if (cfg->centre_mode == 3) {                // the §12 mean plane first, into the handle's own rows
            if ((rc = ensure_risk_buf(h))) return rc;
            size_t off[RISK_REGIONS + 1];
            risk_regions(h, off, nullptr);
            TubeArgs T{};
            T.traj = R.traj;
            T.mean = (float*)((char*)h->d_risk.p + off[2]);
            T.invP = h->base.invP;
            T.C = (h->H + 1) * SDEMPC_NX;
            HIPCHK(h, launch_tube(T, B, h->P, h->G, h->H, st));
            R.centre = T.mean;
        }
    }
    R.sc_n = h->base.C.sc_n; R.sc_tab = h->base.C.sc_tab;
    R.exit = (uint32_t*)exit_dev; R.jx = (float*)jx_dev; R.first_exit = (uint32_t*)first_exit_dev; R.outside_any = (uint32_t*)outside_any_dev;
    R.jstat = (float*)jstat_dev; R.jq = (float*)jq_dev; R.jtail = (float*)jtail_dev;
    for (int i = 0; i < 3; ++i) { R.perr[i] = h->base.C.perr[i]; R.verr[i] = h->base.C.verr[i]; R.qerr[i] = h->base.C.qerr[i]; R.werr[i] = h->base.C.werr[i]; }
    R.invP = h->base.invP;
    R.H = h->H;
    if (jtail_dev) { R.tail_k = cfg->tail_k; R.inv_tail = 1.0f / (float)cfg->tail_k; }
    if (jq_dev) {
        R.n_ranks = cfg->n_ranks;
        for (int k = 0; k < cfg->n_ranks; ++k) R.ranks[k] = cfg->ranks[k];
    }
    HIPCHK(h, launch_risk(R, B, h->P, h->G, st));
    return SDEMPC_OK;
    });
}

namespace {
// the staged inputs (d_x0, d_u, d_xref, d_noise on the handle's stream) -> one store_traj rollout, the reducer, the outputs asked for back on the host
int risk_staged(sdempc_handle* h, const sdempc_risk_cfg* cfg_in, int32_t B, const float* lo, const float* hi, const float* centre, float* cost, const RiskOut& O) {
    int rc = ensure_risk_buf(h);
    if (rc) return rc;
    size_t off[RISK_REGIONS + 1], per[RISK_REGIONS];
    risk_regions(h, off, per);
    char* d = (char*)h->d_risk.p;
    // centre_mode 3: the rollout's own mean trajectory IS the §12 mean plane (SPEC.md §6.3), so the rollout writes the centre rows and the reducer takes them as
    // caller's rows — the tensor is not read a second time for them
    sdempc_risk_cfg staged = *cfg_in;
    const bool own_mean = staged.centre_mode == 3 && (O.exit || O.first_exit || O.outside_any);
    if (own_mean) staged.centre_mode = 1;
    const sdempc_risk_cfg* cfg = &staged;
    if ((rc = sdempc_rollout_batch_dev(h, B, h->d_x0.p, h->d_u.p, h->d_xref.p, h->d_noise.p, h->d_cost.p, own_mean ? d + off[2] : nullptr, 1, h->stream))) return rc;
    const void* in[3] = {lo, hi, cfg_in->centre_mode == 1 ? centre : nullptr};
    void* in_dev[3];
    for (int k = 0; k < 3; ++k) {
        in_dev[k] = in[k] ? d + off[k] : nullptr;
        if (in[k]) HIPCHK(h, hipMemcpyAsync(in_dev[k], in[k], per[k] * B, hipMemcpyHostToDevice, h->stream));
    }
    void* host[7] = {O.exit, O.jx, O.first_exit, O.outside_any, O.jstat, O.jq, O.jtail};
    void* dev[7];
    for (int k = 0; k < 7; ++k) dev[k] = host[k] ? d + off[3 + k] : nullptr;
    per[3 + 5] = sizeof(float) * (size_t)(O.jq ? cfg->n_ranks : 0);      // jq is [B][n_ranks]
    if (own_mean) in_dev[2] = d + off[2];
    if ((rc = sdempc_risk_batch_dev(h, cfg, B, in_dev[0], in_dev[1], in_dev[2], h->d_xref.p, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], h->stream))) return rc;
    if (cost) HIPCHK(h, hipMemcpyAsync(cost, h->d_cost.p, sizeof(float) * B, hipMemcpyDeviceToHost, h->stream));
    for (int k = 0; k < 7; ++k)
        if (host[k]) HIPCHK(h, hipMemcpyAsync(host[k], dev[k], per[3 + k] * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
}
}  // namespace

int sdempc_risk_batch(sdempc_handle* h, const sdempc_risk_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const float* noise, const float* lo,
                      const float* hi, const float* centre, float* cost, uint32_t* exit, float* jx, uint32_t* first_exit, uint32_t* outside_any, float* jstat, float* jq,
                      float* jtail) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !noise) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    const RiskOut O{exit, jx, first_exit, outside_any, jstat, jq, jtail};
    if ((rc = check_risk(h, cfg, lo != nullptr, hi != nullptr, centre != nullptr, true, O))) return rc;
    if ((rc = check_risk_bounds(h, B, lo, hi))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = stage_common(h, B, x0, u, xref, noise))) return rc;
    return risk_staged(h, cfg, B, lo, hi, centre, cost, O);
    });
}

int sdempc_risk_batch_keys(sdempc_handle* h, const sdempc_risk_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const uint32_t* keys,
                           const float* lo, const float* hi, const float* centre, float* cost, uint32_t* exit, float* jx, uint32_t* first_exit, uint32_t* outside_any,
                           float* jstat, float* jq, float* jtail) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !keys) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    const RiskOut O{exit, jx, first_exit, outside_any, jstat, jq, jtail};
    if ((rc = check_risk(h, cfg, lo != nullptr, hi != nullptr, centre != nullptr, true, O))) return rc;
    if ((rc = check_risk_bounds(h, B, lo, hi))) return rc;
    if ((rc = ensure_device(h))) return rc;
    const int H = h->H, m = h->m;
    HIPCHK(h, hipMemcpyAsync(h->d_x0.p, x0, sizeof(float) * B * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_u.p, u, sizeof(float) * B * H * m, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_xref.p, xref, sizeof(float) * B * (H + 1) * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    if ((rc = noise_from_keys(h, B, keys, (float*)h->d_noise.p, h->stream))) return rc;
    return risk_staged(h, cfg, B, lo, hi, centre, cost, O);
    });
}

// ---- predicted bands (SPEC.md §12b) ----
namespace {
// every check of a bands request (SPEC.md §12b) that needs no device; no HIP call
int check_bands(sdempc_handle* h, const sdempc_bands_cfg* cfg, bool have_obs, const void* q, const void* below, const void* at) {
    if (cfg && cfg->struct_size != (int32_t)sizeof(sdempc_bands_cfg)) return fail(h, SDEMPC_EINVAL, "sdempc_bands_cfg.struct_size mismatch%s");
    if (!q && !below && !at) return fail(h, SDEMPC_EINVAL, "no output asked for: q, below and at are all NULL%s");
    if ((below || at) && !have_obs) return fail(h, SDEMPC_EINVAL, "below and at need the observed rows (obs)%s");
    if (q) {
        if (!cfg) return fail(h, SDEMPC_EINVAL, "q needs a sdempc_bands_cfg (the ranks it selects)%s");
        if (cfg->n_ranks < 1 || cfg->n_ranks > BAND_MAX_RANKS) return fail(h, SDEMPC_EINVAL, "q needs 1 <= sdempc_bands_cfg.n_ranks <= 8%s");
        for (int k = 0; k < cfg->n_ranks; ++k)
            if (cfg->ranks[k] < 0 || cfg->ranks[k] >= h->P) return fail(h, SDEMPC_EINVAL, "a rank of sdempc_bands_cfg.ranks is outside 0 .. P-1%s");
    }
    return 0;
}
}  // namespace

int sdempc_bands_batch_dev(sdempc_handle* h, const sdempc_bands_cfg* cfg, int32_t B, const void* obs_dev, void* q_dev, void* below_dev, void* at_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if ((rc = check_bands(h, cfg, obs_dev != nullptr, q_dev, below_dev, at_dev))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = check_traj_held(h, B))) return rc;
    BandArgs N{};
    N.traj = (const float*)h->d_traj.p;
    if (below_dev || at_dev) { N.obs = (const float*)obs_dev; N.below = (uint32_t*)below_dev; N.at = (uint32_t*)at_dev; }
    if (q_dev) {
        N.q = (float*)q_dev;
        N.n_ranks = cfg->n_ranks;
        for (int k = 0; k < cfg->n_ranks; ++k) N.ranks[k] = cfg->ranks[k];
    }
    N.C = (h->H + 1) * SDEMPC_NX;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(h, launch_bands(N, B, h->P, h->G, h->H, st));
    return SDEMPC_OK;
    });
}

namespace {
// the staged inputs (d_x0, d_u, d_xref, d_noise on the handle's stream) -> obs staged, one store_traj rollout, the reducer, the outputs asked for back on the host
int bands_staged(sdempc_handle* h, const sdempc_bands_cfg* cfg, int32_t B, const float* obs, float* cost, float* q, uint32_t* below, uint32_t* at) {
    int rc;
    const size_t n = (size_t)(h->H + 1) * SDEMPC_NX, plane = sizeof(float) * (size_t)h->max_batch * n;
    if (!h->d_band.p && (rc = dev_alloc(h, h->d_band, (3 + BAND_MAX_RANKS) * plane, true))) return rc;
    char* d = (char*)h->d_band.p;
    void* d_obs = d, *d_below = d + plane, *d_at = d + 2 * plane, *d_q = d + 3 * plane;
    const bool want_obs = below || at;
    if (want_obs) HIPCHK(h, hipMemcpyAsync(d_obs, obs, sizeof(float) * B * n, hipMemcpyHostToDevice, h->stream));
    if ((rc = sdempc_rollout_batch_dev(h, B, h->d_x0.p, h->d_u.p, h->d_xref.p, h->d_noise.p, h->d_cost.p, nullptr, 1, h->stream))) return rc;
    if ((rc = sdempc_bands_batch_dev(h, cfg, B, want_obs ? d_obs : nullptr, q ? d_q : nullptr, below ? d_below : nullptr, at ? d_at : nullptr, h->stream))) return rc;
    if (cost) HIPCHK(h, hipMemcpyAsync(cost, h->d_cost.p, sizeof(float) * B, hipMemcpyDeviceToHost, h->stream));
    if (q) HIPCHK(h, hipMemcpyAsync(q, d_q, sizeof(float) * B * n * cfg->n_ranks, hipMemcpyDeviceToHost, h->stream));
    if (below) HIPCHK(h, hipMemcpyAsync(below, d_below, sizeof(uint32_t) * B * n, hipMemcpyDeviceToHost, h->stream));
    if (at) HIPCHK(h, hipMemcpyAsync(at, d_at, sizeof(uint32_t) * B * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
}
}  // namespace

int sdempc_bands_batch(sdempc_handle* h, const sdempc_bands_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const float* noise, const float* obs,
                       float* cost, float* q, uint32_t* below, uint32_t* at) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !noise) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = check_bands(h, cfg, obs != nullptr, q, below, at))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = stage_common(h, B, x0, u, xref, noise))) return rc;
    return bands_staged(h, cfg, B, obs, cost, q, below, at);
    });
}

int sdempc_bands_batch_keys(sdempc_handle* h, const sdempc_bands_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const uint32_t* keys,
                            const float* obs, float* cost, float* q, uint32_t* below, uint32_t* at) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !keys) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = check_bands(h, cfg, obs != nullptr, q, below, at))) return rc;
    if ((rc = ensure_device(h))) return rc;
    const int H = h->H, m = h->m;
    HIPCHK(h, hipMemcpyAsync(h->d_x0.p, x0, sizeof(float) * B * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_u.p, u, sizeof(float) * B * H * m, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_xref.p, xref, sizeof(float) * B * (H + 1) * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    if ((rc = noise_from_keys(h, B, keys, (float*)h->d_noise.p, h->stream))) return rc;
    return bands_staged(h, cfg, B, obs, cost, q, below, at);
    });
}

// ---- predicted outcome (SPEC.md §12c) ----
namespace {
struct OutcomeOut { void *words, *fail_step, *first_fail, *cause_ever, *chan_stat, *chan_q, *agg_stat, *agg_q; };
constexpr int OUTCOME_REGIONS = 9;   // target rows, then the eight outputs in OutcomeOut's order

// byte offsets of d_outcome's regions, each sized for max_batch instances; off[OUTCOME_REGIONS] = total
void outcome_regions(const sdempc_handle* h, size_t* off, size_t* per_instance) {
    const size_t H = (size_t)h->H;
    const size_t words[OUTCOME_REGIONS] = {(H + 1) * SDEMPC_NX, (size_t)h->P * OUTCOME_WORDS, H * 5, H + 1, 4, H * 12, H * 4 * OUTCOME_MAX_RANKS, 12, 4 * OUTCOME_MAX_RANKS};
    size_t o = 0;
    for (int k = 0; k < OUTCOME_REGIONS; ++k) {
        off[k] = o;
        if (per_instance) per_instance[k] = sizeof(float) * words[k];
        o += (sizeof(float) * words[k] * (size_t)h->max_batch + 255) & ~(size_t)255;
    }
    off[OUTCOME_REGIONS] = o;
}

// every check of an outcome request (SPEC.md §12c) that needs no device, in the documented order; no HIP call. have_*: whether the caller gave that input.
int check_outcome(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int B, bool have_target, bool have_xref, const OutcomeOut& O) {
    if (!cfg) return fail(h, SDEMPC_EINVAL, "NULL sdempc_outcome_cfg%s");
    if (cfg->struct_size != (int32_t)sizeof(sdempc_outcome_cfg)) return fail(h, SDEMPC_EINVAL, "sdempc_outcome_cfg.struct_size mismatch%s");
    if (cfg->r2_pos != cfg->r2_pos || cfg->cos_min != cfg->cos_min || cfg->w2_max != cfg->w2_max)
        return fail(h, SDEMPC_EINVAL, "a threshold of sdempc_outcome_cfg is NaN (use +inf / -inf / +inf to switch a criterion off)%s");
    if (!O.words && !O.fail_step && !O.first_fail && !O.cause_ever && !O.chan_stat && !O.chan_q && !O.agg_stat && !O.agg_q)
        return fail(h, SDEMPC_EINVAL, "no output asked for: words, fail_step, first_fail, cause_ever, chan_stat, chan_q, agg_stat and agg_q are all NULL%s");
    if (O.chan_q || O.agg_q) {
        if (cfg->n_ranks < 1 || cfg->n_ranks > OUTCOME_MAX_RANKS) return fail(h, SDEMPC_EINVAL, "chan_q and agg_q need 1 <= sdempc_outcome_cfg.n_ranks <= 8%s");
        for (int k = 0; k < cfg->n_ranks; ++k)
            if (cfg->ranks[k] < 0 || cfg->ranks[k] >= h->P) return fail(h, SDEMPC_EINVAL, "a rank of sdempc_outcome_cfg.ranks is outside 0 .. P-1%s");
        if (h->P > OUTCOME_RANK_MAX_P)
            return fail(h, SDEMPC_EINVAL, "chan_q and agg_q are limited to 128 particles (the selection sorts four particle groups in registers); the other outputs are not%s");
    }
    if (cfg->target_mode < 0 || cfg->target_mode > 1) return fail(h, SDEMPC_EINVAL, "sdempc_outcome_cfg.target_mode out of range (0 xref, 1 caller's rows)%s");
    if (cfg->target_mode == 1) {
        if (cfg->tgt_steps != 1 && cfg->tgt_steps != h->H + 1) return fail(h, SDEMPC_EINVAL, "sdempc_outcome_cfg.tgt_steps must be 1 or H+1%s");
        if (cfg->tgt_batch != 1 && cfg->tgt_batch != B) return fail(h, SDEMPC_EINVAL, "sdempc_outcome_cfg.tgt_batch must be 1 or B%s");
        if (!have_target) return fail(h, SDEMPC_EINVAL, "target_mode 1 needs the caller's target rows%s");
    } else if (!have_xref) return fail(h, SDEMPC_EINVAL, "target_mode 0 needs xref%s");
    if (sizeof(uint32_t) * outcome_lds_words_host(h->H, h->G) > RISK_MAX_LDS)
        return fail(h, SDEMPC_EINVAL, "horizon and particle count too large for the outcome reducer's workgroup memory (4 (6 H + 5 + 140 ceil(P / 32)) bytes > 64 KiB)%s");
    return 0;
}
}  // namespace

int sdempc_outcome_batch_dev(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int32_t B, const void* target_dev, const void* xref_dev, void* words_dev,
                             void* fail_step_dev, void* first_fail_dev, void* cause_ever_dev, void* chan_stat_dev, void* chan_q_dev, void* agg_stat_dev,
                             void* agg_q_dev, void* stream) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    const OutcomeOut O{words_dev, fail_step_dev, first_fail_dev, cause_ever_dev, chan_stat_dev, chan_q_dev, agg_stat_dev, agg_q_dev};
    if ((rc = check_outcome(h, cfg, B, target_dev != nullptr, xref_dev != nullptr, O))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = check_traj_held(h, B))) return rc;
    OutcomeArgs W{};
    W.traj = (const float*)h->d_traj.p;
    if (cfg->target_mode == 1) {
        W.tgt = (const float*)target_dev;
        W.tgt_tstride = cfg->tgt_steps > 1 ? SDEMPC_NX : 0;
        W.tgt_bstride = cfg->tgt_batch > 1 ? cfg->tgt_steps * SDEMPC_NX : 0;
    } else {
        W.tgt = (const float*)xref_dev;
        W.tgt_tstride = SDEMPC_NX;
        W.tgt_bstride = (h->H + 1) * SDEMPC_NX;
    }
    W.words = (uint32_t*)words_dev; W.fail_step = (uint32_t*)fail_step_dev; W.first_fail = (uint32_t*)first_fail_dev; W.cause_ever = (uint32_t*)cause_ever_dev;
    W.chan_stat = (float*)chan_stat_dev; W.chan_q = (float*)chan_q_dev; W.agg_stat = (float*)agg_stat_dev; W.agg_q = (float*)agg_q_dev;
    W.r2_pos = cfg->r2_pos; W.cos_min = cfg->cos_min; W.w2_max = cfg->w2_max;
    W.invP = h->base.invP;
    W.H = h->H;
    if (chan_q_dev || agg_q_dev) {
        W.n_ranks = cfg->n_ranks;
        for (int k = 0; k < cfg->n_ranks; ++k) W.ranks[k] = cfg->ranks[k];
    }
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(h, launch_outcome(W, B, h->P, h->G, st));
    return SDEMPC_OK;
    });
}

namespace {
// the staged inputs (d_x0, d_u, d_xref, d_noise on the handle's stream) -> the target rows staged, one store_traj rollout, the reducer, the outputs asked for
// back on the host
int outcome_staged(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int32_t B, const float* target, float* cost, const OutcomeOut& O) {
    int rc;
    size_t off[OUTCOME_REGIONS + 1], per[OUTCOME_REGIONS];
    outcome_regions(h, off, per);
    if (!h->d_outcome.p && (rc = dev_alloc(h, h->d_outcome, off[OUTCOME_REGIONS], true))) return rc;
    char* d = (char*)h->d_outcome.p;
    void* d_target = nullptr;
    if (cfg->target_mode == 1) {
        d_target = d + off[0];
        HIPCHK(h, hipMemcpyAsync(d_target, target, sizeof(float) * (size_t)cfg->tgt_batch * cfg->tgt_steps * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    }
    if ((rc = sdempc_rollout_batch_dev(h, B, h->d_x0.p, h->d_u.p, h->d_xref.p, h->d_noise.p, h->d_cost.p, nullptr, 1, h->stream))) return rc;
    void* host[8] = {O.words, O.fail_step, O.first_fail, O.cause_ever, O.chan_stat, O.chan_q, O.agg_stat, O.agg_q};
    void* dev[8];
    for (int k = 0; k < 8; ++k) dev[k] = host[k] ? d + off[1 + k] : nullptr;
    per[1 + 5] = sizeof(float) * (size_t)h->H * 4 * (size_t)(O.chan_q ? cfg->n_ranks : 0);      // chan_q is [B][H][4][n_ranks]
    per[1 + 7] = sizeof(float) * 4 * (size_t)(O.agg_q ? cfg->n_ranks : 0);                      // agg_q is [B][4][n_ranks]
    if ((rc = sdempc_outcome_batch_dev(h, cfg, B, d_target, h->d_xref.p, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], h->stream))) return rc;
    if (cost) HIPCHK(h, hipMemcpyAsync(cost, h->d_cost.p, sizeof(float) * B, hipMemcpyDeviceToHost, h->stream));
    for (int k = 0; k < 8; ++k)
        if (host[k]) HIPCHK(h, hipMemcpyAsync(host[k], dev[k], per[1 + k] * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
}
}  // namespace

int sdempc_outcome_batch(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const float* noise,
                         const float* target, float* cost, uint32_t* words, uint32_t* fail_step, uint32_t* first_fail, uint32_t* cause_ever, float* chan_stat,
                         float* chan_q, float* agg_stat, float* agg_q) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !noise) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    const OutcomeOut O{words, fail_step, first_fail, cause_ever, chan_stat, chan_q, agg_stat, agg_q};
    if ((rc = check_outcome(h, cfg, B, target != nullptr, true, O))) return rc;
    if ((rc = ensure_device(h))) return rc;
    if ((rc = stage_common(h, B, x0, u, xref, noise))) return rc;
    return outcome_staged(h, cfg, B, target, cost, O);
    });
}

int sdempc_outcome_batch_keys(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const uint32_t* keys,
                              const float* target, float* cost, uint32_t* words, uint32_t* fail_step, uint32_t* first_fail, uint32_t* cause_ever,
                              float* chan_stat, float* chan_q, float* agg_stat, float* agg_q) {
    return guarded(h, [&]() -> int {
    int rc = check_batch(h, B);
    if (rc) return rc;
    if (!x0 || !u || !xref || !keys) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    const OutcomeOut O{words, fail_step, first_fail, cause_ever, chan_stat, chan_q, agg_stat, agg_q};
    if ((rc = check_outcome(h, cfg, B, target != nullptr, true, O))) return rc;
    if ((rc = ensure_device(h))) return rc;
    const int H = h->H, m = h->m;
    HIPCHK(h, hipMemcpyAsync(h->d_x0.p, x0, sizeof(float) * B * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_u.p, u, sizeof(float) * B * H * m, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_xref.p, xref, sizeof(float) * B * (H + 1) * SDEMPC_NX, hipMemcpyHostToDevice, h->stream));
    if ((rc = noise_from_keys(h, B, keys, (float*)h->d_noise.p, h->stream))) return rc;
    return outcome_staged(h, cfg, B, target, cost, O);
    });
}

int sdempc_closed_loop_batch(sdempc_handle* h, int32_t B, int32_t T, const float* x0, const float* xref, int32_t xref_ticks, int32_t xref_batch,
                             const uint32_t* keys, const float* u_init, const float* stepsize_in, float* xs, float* us, sdempc_info* info,
                             float* u_next, float* stepsize_next, uint32_t* keys_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};                   // no plant set: the handle's own model, one step of time_steps[0] per tick (SPEC.md §11)
    c.layer = LOOP_PLAIN;
    c.io = {B, T, xref_ticks, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_plant(sdempc_handle* h, const sdempc_plant_cfg* pc, const void* const* plant_blobs, const size_t* plant_blob_bytes,
                                   const int32_t* plant_of, int32_t B, int32_t T, const float* x0, const float* xref, int32_t xref_ticks,
                                   int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in, float* xs, float* us,
                                   sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = LOOP_PLANT;
    c.io = {B, T, xref_ticks, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_timed(sdempc_handle* h, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc, const void* const* plant_blobs,
                                   const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0, const float* xref,
                                   int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in,
                                   const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next, float* stepsize_next,
                                   uint32_t* keys_next, float* u_act_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = LOOP_TIMED;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_scenario(sdempc_handle* h, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc,
                                      const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T,
                                      const float* x0, const float* xref, int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init,
                                      const float* stepsize_in, const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next,
                                      float* stepsize_next, uint32_t* keys_next, float* u_act_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_rate(sdempc_handle* h, const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc,
                                  const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T,
                                  const float* x0, const float* xref, int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init,
                                  const float* stepsize_in, const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next,
                                  float* stepsize_next, uint32_t* keys_next, float* u_act_next, const float* rate_integ_in, const float* rate_tail_in,
                                  float* ws, float* rate_integ_next, float* rate_tail_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = LOOP_RATE;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_fault(sdempc_handle* h, const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc,
                                   const sdempc_plant_cfg* pc, const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T,
                                   const float* x0, const float* xref, int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init,
                                   const float* stepsize_in, const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next,
                                   float* stepsize_next, uint32_t* keys_next, float* u_act_next, const float* rate_integ_in, const float* rate_tail_in,
                                   float* ws, float* rate_integ_next, float* rate_tail_next, float* xsub) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_observed(sdempc_handle* h, const sdempc_obs_cfg* oc, const uint32_t* obs_keys, const float* xmeas_in, const sdempc_fault_cfg* fc,
                                      const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc,
                                      const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0,
                                      const float* xref, int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in,
                                      const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next,
                                      float* u_act_next, const float* rate_integ_in, const float* rate_tail_in, float* ws, float* rate_integ_next, float* rate_tail_next,
                                      float* xsub, float* xmeas, uint32_t* obs_keys_next, float* xmeas_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_aged(sdempc_handle* h, const sdempc_age_cfg* ac, const float* xhist_in, const sdempc_obs_cfg* oc, const uint32_t* obs_keys, const float* xmeas_in,
                                  const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc,
                                  const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0,
                                  const float* xref, int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in,
                                  const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next,
                                  float* u_act_next, const float* rate_integ_in, const float* rate_tail_in, float* ws, float* rate_integ_next, float* rate_tail_next,
                                  float* xsub, float* xmeas, uint32_t* obs_keys_next, float* xmeas_next, float* xhist_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_scored(sdempc_handle* h, const sdempc_score_cfg* zc, const uint32_t* score_in, const sdempc_age_cfg* ac, const float* xhist_in,
                                    const sdempc_obs_cfg* oc, const uint32_t* obs_keys, const float* xmeas_in, const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_,
                                    const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc, const void* const* plant_blobs,
                                    const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0, const float* xref, int32_t xref_solves,
                                    int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in, const float* u_act_in, float* xs, float* us,
                                    sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next, float* u_act_next, const float* rate_integ_in,
                                    const float* rate_tail_in, float* ws, float* rate_integ_next, float* rate_tail_next, float* xsub, float* xmeas, uint32_t* obs_keys_next,
                                    float* xmeas_next, float* xhist_next, uint32_t* score_out) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    c.scored = true; c.zc = zc; c.score_in = score_in; c.score_out = score_out;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_drawn(sdempc_handle* h, const sdempc_process_cfg* dist_proc, const sdempc_process_cfg* bias_proc, const sdempc_score_cfg* zc,
                                   const uint32_t* score_in, const sdempc_age_cfg* ac, const float* xhist_in, const sdempc_obs_cfg* oc, const uint32_t* obs_keys,
                                   const float* xmeas_in, const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc,
                                   const sdempc_plant_cfg* pc, const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T,
                                   const float* x0, const float* xref, int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init,
                                   const float* stepsize_in, const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next, float* stepsize_next,
                                   uint32_t* keys_next, float* u_act_next, const float* rate_integ_in, const float* rate_tail_in, float* ws, float* rate_integ_next,
                                   float* rate_tail_next, float* xsub, float* xmeas, uint32_t* obs_keys_next, float* xmeas_next, float* xhist_next, uint32_t* score_out,
                                   float* dist_rows, uint32_t* dist_keys_next, float* dist_state_next, float* bias_rows, uint32_t* bias_keys_next, float* bias_state_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    c.scored = true; c.zc = zc; c.score_in = score_in; c.score_out = score_out;
    c.drawn = true; c.pr = {dist_proc, bias_proc, dist_rows, dist_keys_next, dist_state_next, bias_rows, bias_keys_next, bias_state_next};
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_tracked(sdempc_handle* h, const sdempc_track_cfg* track, const sdempc_process_cfg* dist_proc, const sdempc_process_cfg* bias_proc,
                                     const sdempc_score_cfg* zc, const uint32_t* score_in, const sdempc_age_cfg* ac, const float* xhist_in, const sdempc_obs_cfg* oc,
                                     const uint32_t* obs_keys, const float* xmeas_in, const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc,
                                     const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc, const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of,
                                     int32_t B, int32_t T, const float* x0, const float* xref, int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init,
                                     const float* stepsize_in, const float* u_act_in, float* xs, float* us, sdempc_info* info, float* u_next, float* stepsize_next,
                                     uint32_t* keys_next, float* u_act_next, const float* rate_integ_in, const float* rate_tail_in, float* ws, float* rate_integ_next,
                                     float* rate_tail_next, float* xsub, float* xmeas, uint32_t* obs_keys_next, float* xmeas_next, float* xhist_next, uint32_t* score_out,
                                     float* dist_rows, uint32_t* dist_keys_next, float* dist_state_next, float* bias_rows, uint32_t* bias_keys_next, float* bias_state_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    c.scored = true; c.zc = zc; c.score_in = score_in; c.score_out = score_out;
    c.drawn = true; c.pr = {dist_proc, bias_proc, dist_rows, dist_keys_next, dist_state_next, bias_rows, bias_keys_next, bias_state_next};
    c.track = track;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_events(sdempc_handle* h, const sdempc_fault_process_cfg* fault_proc, const sdempc_dropout_process_cfg* drop_proc, const sdempc_track_cfg* track,
                                    const sdempc_process_cfg* dist_proc, const sdempc_process_cfg* bias_proc, const sdempc_score_cfg* zc, const uint32_t* score_in,
                                    const sdempc_age_cfg* ac, const float* xhist_in, const sdempc_obs_cfg* oc, const uint32_t* obs_keys, const float* xmeas_in,
                                    const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc,
                                    const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0, const float* xref,
                                    int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in, const float* u_act_in, float* xs,
                                    float* us, sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next, float* u_act_next, const float* rate_integ_in,
                                    const float* rate_tail_in, float* ws, float* rate_integ_next, float* rate_tail_next, float* xsub, float* xmeas, uint32_t* obs_keys_next,
                                    float* xmeas_next, float* xhist_next, uint32_t* score_out, float* dist_rows, uint32_t* dist_keys_next, float* dist_state_next, float* bias_rows,
                                    uint32_t* bias_keys_next, float* bias_state_next, float* fault_rows, uint32_t* fault_keys_next, int32_t* fault_state_next, int32_t* valid_rows,
                                    uint32_t* valid_keys_next, int32_t* valid_state_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    c.scored = true; c.zc = zc; c.score_in = score_in; c.score_out = score_out;
    c.drawn = true; c.pr = {dist_proc, bias_proc, dist_rows, dist_keys_next, dist_state_next, bias_rows, bias_keys_next, bias_state_next};
    c.track = track;
    c.events = true; c.er = {fault_proc, drop_proc, fault_rows, fault_keys_next, fault_state_next, valid_rows, valid_keys_next, valid_state_next};
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_baseline(sdempc_handle* h, const sdempc_geo_cfg* geo, const sdempc_fault_process_cfg* fault_proc, const sdempc_dropout_process_cfg* drop_proc,
                                      const sdempc_track_cfg* track, const sdempc_process_cfg* dist_proc, const sdempc_process_cfg* bias_proc, const sdempc_score_cfg* zc,
                                      const uint32_t* score_in, const sdempc_age_cfg* ac, const float* xhist_in, const sdempc_obs_cfg* oc, const uint32_t* obs_keys, const float* xmeas_in,
                                      const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_, const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc,
                                      const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0, const float* xref,
                                      int32_t xref_solves, int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in, const float* u_act_in, float* xs,
                                      float* us, sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next, float* u_act_next, const float* rate_integ_in,
                                      const float* rate_tail_in, float* ws, float* rate_integ_next, float* rate_tail_next, float* xsub, float* xmeas, uint32_t* obs_keys_next,
                                      float* xmeas_next, float* xhist_next, uint32_t* score_out, float* dist_rows, uint32_t* dist_keys_next, float* dist_state_next, float* bias_rows,
                                      uint32_t* bias_keys_next, float* bias_state_next, float* fault_rows, uint32_t* fault_keys_next, int32_t* fault_state_next, int32_t* valid_rows,
                                      uint32_t* valid_keys_next, int32_t* valid_state_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    c.scored = true; c.zc = zc; c.score_in = score_in; c.score_out = score_out;
    c.drawn = true; c.pr = {dist_proc, bias_proc, dist_rows, dist_keys_next, dist_state_next, bias_rows, bias_keys_next, bias_state_next};
    c.track = track;
    c.events = true; c.er = {fault_proc, drop_proc, fault_rows, fault_keys_next, fault_state_next, valid_rows, valid_keys_next, valid_state_next};
    c.baseline = true; c.geo = geo;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_ensemble(sdempc_handle* h, const sdempc_ensemble_cfg* ens, uint32_t* ens_out, const sdempc_geo_cfg* geo, const sdempc_fault_process_cfg* fault_proc,
                                      const sdempc_dropout_process_cfg* drop_proc, const sdempc_track_cfg* track, const sdempc_process_cfg* dist_proc,
                                      const sdempc_process_cfg* bias_proc, const sdempc_score_cfg* zc, const uint32_t* score_in, const sdempc_age_cfg* ac, const float* xhist_in,
                                      const sdempc_obs_cfg* oc, const uint32_t* obs_keys, const float* xmeas_in, const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_,
                                      const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc, const void* const* plant_blobs,
                                      const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0, const float* xref, int32_t xref_solves,
                                      int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in, const float* u_act_in, float* xs, float* us,
                                      sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next, float* u_act_next, const float* rate_integ_in,
                                      const float* rate_tail_in, float* ws, float* rate_integ_next, float* rate_tail_next, float* xsub, float* xmeas, uint32_t* obs_keys_next,
                                      float* xmeas_next, float* xhist_next, uint32_t* score_out, float* dist_rows, uint32_t* dist_keys_next, float* dist_state_next, float* bias_rows,
                                      uint32_t* bias_keys_next, float* bias_state_next, float* fault_rows, uint32_t* fault_keys_next, int32_t* fault_state_next, int32_t* valid_rows,
                                      uint32_t* valid_keys_next, int32_t* valid_state_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    c.scored = true; c.zc = zc; c.score_in = score_in; c.score_out = score_out;
    c.drawn = true; c.pr = {dist_proc, bias_proc, dist_rows, dist_keys_next, dist_state_next, bias_rows, bias_keys_next, bias_state_next};
    c.track = track;
    c.events = true; c.er = {fault_proc, drop_proc, fault_rows, fault_keys_next, fault_state_next, valid_rows, valid_keys_next, valid_state_next};
    c.baseline = geo != nullptr; c.geo = geo;      // (geo NULL: the MPC's own solves, i.e. the events call)
    c.ensembled = true; c.ens = ens; c.ens_out = ens_out;
    return closed_loop_call(h, c);
    });
}

int sdempc_closed_loop_batch_retire(sdempc_handle* h, const sdempc_retire_cfg* retire, int32_t* retired_at, int32_t* live_per_solve, const sdempc_ensemble_cfg* ens, uint32_t* ens_out, const sdempc_geo_cfg* geo, const sdempc_fault_process_cfg* fault_proc,
                                      const sdempc_dropout_process_cfg* drop_proc, const sdempc_track_cfg* track, const sdempc_process_cfg* dist_proc,
                                      const sdempc_process_cfg* bias_proc, const sdempc_score_cfg* zc, const uint32_t* score_in, const sdempc_age_cfg* ac, const float* xhist_in,
                                      const sdempc_obs_cfg* oc, const uint32_t* obs_keys, const float* xmeas_in, const sdempc_fault_cfg* fc, const sdempc_rate_cfg* rc_,
                                      const sdempc_scenario_cfg* sc, const sdempc_timing_cfg* tc, const sdempc_plant_cfg* pc, const void* const* plant_blobs,
                                      const size_t* plant_blob_bytes, const int32_t* plant_of, int32_t B, int32_t T, const float* x0, const float* xref, int32_t xref_solves,
                                      int32_t xref_batch, const uint32_t* keys, const float* u_init, const float* stepsize_in, const float* u_act_in, float* xs, float* us,
                                      sdempc_info* info, float* u_next, float* stepsize_next, uint32_t* keys_next, float* u_act_next, const float* rate_integ_in,
                                      const float* rate_tail_in, float* ws, float* rate_integ_next, float* rate_tail_next, float* xsub, float* xmeas, uint32_t* obs_keys_next,
                                      float* xmeas_next, float* xhist_next, uint32_t* score_out, float* dist_rows, uint32_t* dist_keys_next, float* dist_state_next, float* bias_rows,
                                      uint32_t* bias_keys_next, float* bias_state_next, float* fault_rows, uint32_t* fault_keys_next, int32_t* fault_state_next, int32_t* valid_rows,
                                      uint32_t* valid_keys_next, int32_t* valid_state_next) {
    return guarded(h, [&]() -> int {
    LoopCall c{};
    c.layer = rc_ ? LOOP_RATE : LOOP_SCENARIO;
    c.io = {B, T, xref_solves, xref_batch, x0, xref, keys, u_init, stepsize_in, xs, us, info, u_next, stepsize_next, keys_next};
    c.pc = pc; c.plant_blobs = plant_blobs; c.plant_blob_bytes = plant_blob_bytes; c.plant_of = plant_of;
    c.tc = tc; c.u_act_in = u_act_in; c.u_act_next = u_act_next;
    c.sc = sc;
    c.rc = rc_; c.rate_integ_in = rate_integ_in; c.rate_tail_in = rate_tail_in; c.ws = ws; c.rate_integ_next = rate_integ_next; c.rate_tail_next = rate_tail_next;
    c.faulted = true; c.fc = fc; c.xsub = xsub;
    c.observed = true; c.oc = oc; c.obs_keys = obs_keys; c.xmeas_in = xmeas_in; c.xmeas = xmeas; c.obs_keys_next = obs_keys_next; c.xmeas_next = xmeas_next;
    c.aged = true; c.ac = ac; c.xhist_in = xhist_in; c.xhist_next = xhist_next;
    c.scored = true; c.zc = zc; c.score_in = score_in; c.score_out = score_out;
    c.drawn = true; c.pr = {dist_proc, bias_proc, dist_rows, dist_keys_next, dist_state_next, bias_rows, bias_keys_next, bias_state_next};
    c.track = track;
    c.events = true; c.er = {fault_proc, drop_proc, fault_rows, fault_keys_next, fault_state_next, valid_rows, valid_keys_next, valid_state_next};
    c.baseline = geo != nullptr; c.geo = geo;      // (geo NULL: the MPC's own solves, i.e. the events call)
    c.ensembled = true; c.ens = ens; c.ens_out = ens_out;
    c.retiring = true; c.retire = retire; c.retired_at = retired_at; c.live_per_solve = live_per_solve;
    return closed_loop_call(h, c);
    });
}

int sdempc_geo_command_batch(sdempc_handle* h, const sdempc_geo_cfg* geo, int32_t B, const float* x, const float* xref, int32_t Bx, float* out) {
    return guarded(h, [&]() -> int {
    if (!h) return SDEMPC_EINVAL;
    float inv_dt = 0.0f;
    int rc = check_geo(h, geo, B, &inv_dt);
    if (rc) return rc;
    if ((rc = check_batch(h, B))) return rc;
    if (Bx != 1 && Bx != B) return fail(h, SDEMPC_EINVAL, "baseline: Bx must be 1 or B%s");
    if (!x || !xref || !out) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    if ((rc = ensure_device(h))) return rc;
    hipStream_t st = h->stream;
    if ((rc = stage_geo(h, *geo, st))) return rc;
    const size_t XR = (size_t)(h->H + 1) * SDEMPC_NX;
    HIPCHK(h, hipMemcpyAsync(h->d_x0.p, x, sizeof(float) * (size_t)B * SDEMPC_NX, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_xref.p, xref, sizeof(float) * (size_t)Bx * XR, hipMemcpyHostToDevice, st));
    LoopBaseline A{};
    A.x = (const float*)h->d_x0.p; A.xref = (const float*)h->d_xref.p; A.xref_ep_stride = Bx > 1 ? (int)XR : 0;
    A.par = (const float*)h->d_geo.p; A.par_ep_stride = geo->batch > 1 ? GEO_PAR_WORDS : 0;
    A.accel_ff = geo->accel_ff; A.ref_row = geo->ref_row; A.inv_dt = inv_dt; A.H = h->H; A.m = h->m;
    A.out = (float*)h->d_geo.p + (size_t)GEO_PAR_WORDS * h->max_batch;
    HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, 1, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, A));
    HIPCHK(h, hipMemcpyAsync(out, A.out, sizeof(float) * 4 * (size_t)B, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return SDEMPC_OK;
    });
}

int sdempc_reference_windows(sdempc_handle* h, const sdempc_track_cfg* track, int32_t B, int32_t n, const int32_t* ticks, float* out) {
    return guarded(h, [&]() -> int {
    if (!h) return SDEMPC_EINVAL;
    if (!track) return fail(h, SDEMPC_EINVAL, "track: cfg is NULL%s");
    int rc = check_track(h, track, B, 0);
    if (rc) return rc;
    if ((rc = check_batch(h, B))) return rc;
    if (n < 1 || !ticks || !out) return fail(h, SDEMPC_EINVAL, "reference windows: n must be >= 1, ticks and out not NULL%s");
    for (int g = 0; g < n; ++g)
        if (ticks[g] < 0 || (long long)track->tick0 + ticks[g] >= (1ll << 24)) return fail(h, SDEMPC_EINVAL, "reference windows: a tick is negative or tick0 + tick >= 2^24%s");
    if ((rc = ensure_device(h))) return rc;
    TrackRun run;
    if ((rc = stage_track(h, *track, B, &run))) return rc;
    const size_t XR = (size_t)(h->H + 1) * SDEMPC_NX;
    LoopTrack K = run.K;
    K.B = B; K.rows = h->H + 1; K.groups = 1;
    for (int g = 0; g < n; ++g) {
        K.tick0 = track->tick0 + ticks[g];
        HIPCHK(h, launch_broadcast_rows(nullptr, (float*)h->d_xref.p, 0, 0, h->stream, K));
        HIPCHK(h, hipMemcpyAsync(out + (size_t)g * B * XR, h->d_xref.p, sizeof(float) * B * XR, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SDEMPC_OK;
    });
}

int sdempc_solve_status(sdempc_handle* h) {
    return guarded(h, [&]() -> int {
    if (!h) return SDEMPC_EINVAL;
    bool to = false;
    int rc = coop_timed_out(h, &to);
    if (rc) return rc;
    if ((rc = tickets_consistent(h))) return rc;
    return to ? fail(h, SDEMPC_EDEVICE, "cooperative solve: a grid barrier timed out (workgroups not co-resident); results invalid, "
                                        "the handle now stays on the one-workgroup-per-instance layouts%s") : SDEMPC_OK;
    });
}

int32_t sdempc_layout_fallbacks(const sdempc_handle* h) { return h ? h->layout_fallbacks : 0; }

int sdempc_work_counters(sdempc_handle* h, uint64_t out[4], int32_t reset) {
    return guarded(h, [&]() -> int {
    if (!h || !out) return SDEMPC_EINVAL;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!h->dev_ready) return SDEMPC_OK;
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long v[4];
    HIPCHK(h, hipMemcpy(v, h->d_work.p, sizeof v, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    if (reset) {
        HIPCHK(h, hipMemset(h->d_work.p, 0, sizeof v));
        return null_stream_done(h);     // (the next solve may be enqueued on a non-blocking stream)
    }
    return SDEMPC_OK;
    });
}

}  // extern "C"

namespace {
// Solve on the staged inputs (handle buffers) and fetch the results. If a grid barrier of the cooperative layouts gave up — their
// workgroups were not all resident, i.e. the GPU is shared with other work — the same batch runs once more in the one-workgroup-per-
// instance layout (bit-identical results by construction) and the handle keeps off the cooperative layouts from then on.
int solve_staged(sdempc_handle* h, int32_t B, float* uopt, float* xevol, sdempc_info* info) {
    for (int attempt = 0;; ++attempt) {
        int rc = sdempc_solve_batch_dev(h, B, h->d_x0.p, h->d_xref.p, h->d_noise.p, h->d_u.p, h->d_step.p, h->d_uopt.p, h->d_xmean.p, h->d_info.p, h->stream);
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(uopt, h->d_uopt.p, sizeof(float) * B * h->H * h->m, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(xevol, h->d_xmean.p, sizeof(float) * B * (h->H + 1) * SDEMPC_NX, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(info, h->d_info.p, sizeof(float) * B * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        bool to = false;
        if ((rc = coop_timed_out(h, &to))) return rc;
        if ((rc = tickets_consistent(h))) return rc;
        if (!to) return SDEMPC_OK;
        if (attempt) return fail(h, SDEMPC_EDEVICE, "cooperative solve: a grid barrier timed out twice%s");
    }
}
// The one path behind the closed-loop entry points: every check of the call's parts, in one fixed order (ensemble cfg with its edges and cohorts, baseline cfg, event structs and their arrays, track struct, process structs and their arrays, score struct, age struct, observation struct, fault struct, rate, scenario struct,
// timing, loop arguments, plant_ticks, plant set, solve_delay, disturbance, fault schedule, observation rows, age rows, score target rows; a part the layer lacks is skipped) and before the first HIP call, then the plant set onto the device and the loop.
int closed_loop_call(sdempc_handle* h, const LoopCall& c) {
    if (!h) return SDEMPC_EINVAL;
    const LoopIo& io = c.io;
    const int B = io.B, T = io.T;
    const bool timed = c.layer >= LOOP_TIMED, scenario = c.layer >= LOOP_SCENARIO, rated = c.layer == LOOP_RATE;
    const sdempc_rate_cfg* rc_ = c.rc;
    const sdempc_scenario_cfg* sc = c.sc;
    const sdempc_timing_cfg* tc = c.tc;
    auto finite = [](float v) { return fabsf(v) < INFINITY; };
    const float inv_m = 1.0f / (float)h->m;
    if (c.retiring) {          // SPEC.md §11n: outputs and cfg come together; the cfg's own fields; then the score it reads and the ensemble it may not feed
        const sdempc_retire_cfg* rt = c.retire;
        if ((rt == nullptr) != (c.retired_at == nullptr) || (rt == nullptr) != (c.live_per_solve == nullptr))
            return fail(h, SDEMPC_EINVAL, "retire: retire, retired_at and live_per_solve must be given together%s");
        if (rt) {
            if (rt->struct_size != (int32_t)sizeof(sdempc_retire_cfg)) return fail(h, SDEMPC_EINVAL, "retire: struct_size mismatch%s");
            if (rt->reserved != 0) return fail(h, SDEMPC_EINVAL, "retire: reserved must be 0%s");
            if (!c.zc) return fail(h, SDEMPC_EINVAL, "retire: a retire cfg needs a score cfg (an episode is retired by its score)%s");
            if (c.ens && c.ens->struct_size == (int32_t)sizeof(sdempc_ensemble_cfg) && c.ens->over == 0)
                return fail(h, SDEMPC_EINVAL, "retire: an ensemble over every finite row (over 0) may not be combined with retire (use over 1)%s");
        }
    }
    if (c.ensembled) {         // SPEC.md §11m: output and cfg come together; the cfg's own fields, edges and cohorts; then the score it reduces
        const sdempc_ensemble_cfg* en = c.ens;
        if ((en == nullptr) != (c.ens_out == nullptr)) return fail(h, SDEMPC_EINVAL, "ensemble: ens and ens_out must be given together%s");
        if (en) {
            if (en->struct_size != (int32_t)sizeof(sdempc_ensemble_cfg)) return fail(h, SDEMPC_EINVAL, "ensemble: struct_size mismatch%s");
            if (en->n_cohorts < 1 || en->n_cohorts > ENS_MAX_COHORTS) return fail(h, SDEMPC_EINVAL, "ensemble: n_cohorts must be between 1 and 16%s");
            if (en->n_edges < 0 || en->n_edges > ENS_MAX_EDGES) return fail(h, SDEMPC_EINVAL, "ensemble: n_edges must be between 0 and 16%s");
            if (en->over != 0 && en->over != 1) return fail(h, SDEMPC_EINVAL, "ensemble: over must be 0 (every finite row) or 1 (alive)%s");
            const int E = en->n_edges;
            if (E > 0 && !en->edges) return fail(h, SDEMPC_EINVAL, "ensemble: edges is NULL with n_edges > 0%s");
            for (int e = 0; e < 4 * E; ++e)
                if (en->edges[e] != en->edges[e]) return fail(h, SDEMPC_EINVAL, "ensemble: an edge is NaN%s");
            for (int k = 0; k < 4; ++k)
                for (int j = 1; j < E; ++j)
                    if (en->edges[k * E + j] < en->edges[k * E + j - 1]) return fail(h, SDEMPC_EINVAL, "ensemble: the edges of a channel must ascend%s");
            for (int b = 0; en->cohort && b < B; ++b)
                if (en->cohort[b] < 0 || en->cohort[b] >= en->n_cohorts) return fail(h, SDEMPC_EINVAL, "ensemble: a cohort entry lies outside [0, n_cohorts)%s");
            if (!c.zc) return fail(h, SDEMPC_EINVAL, "ensemble: an ensemble cfg needs a score cfg%s");
        }
    }
    GeoRun run_g{c.geo, 0.0f};
    if (c.baseline) {        // SPEC.md §11l: the controller's cfg, then the interface it publishes to
        if (int rc = check_geo(h, c.geo, B, &run_g.inv_dt)) return rc;
        if (!rc_) return fail(h, SDEMPC_EINVAL, "baseline: the controller publishes thrust and body rates and needs a rate cfg%s");
        if (rc_->struct_size == (int32_t)sizeof(sdempc_rate_cfg) && rc_->motor_weight != 0.0f) return fail(h, SDEMPC_EINVAL, "baseline: motor_weight must be 0 (the table holds no motor values)%s");
    }
    if (c.events) {            // SPEC.md §11k: an output needs its cfg; then the fault cfg, the dropout cfg, and the observation chain the dropouts need
        const EventRun& er = c.er;
        const int m = h->m;
        if (!er.fault && (er.fault_rows || er.fault_keys_next || er.fault_state_next))
            return fail(h, SDEMPC_EINVAL, "events: fault_rows / fault_keys_next / fault_state_next must be NULL without fault_proc%s");
        if (!er.drop && (er.valid_rows || er.valid_keys_next || er.valid_state_next))
            return fail(h, SDEMPC_EINVAL, "events: valid_rows / valid_keys_next / valid_state_next must be NULL without drop_proc%s");
        if (const sdempc_fault_process_cfg* p = er.fault) {
            if (p->struct_size != (int32_t)sizeof(sdempc_fault_process_cfg)) return fail(h, SDEMPC_EINVAL, "events: fault_proc struct_size mismatch%s");
            if (p->n_modes < 1 || p->n_modes > (int)EVT_MODES) return fail(h, SDEMPC_EINVAL, "events: n_modes must be between 1 and 4%s");
            if (p->batch != 1 && p->batch != B) return fail(h, SDEMPC_EINVAL, "events: fault_proc batch must be 1 or B%s");
            if (!p->onset || !p->clear || !p->modes || !p->keys) return fail(h, SDEMPC_EINVAL, "events: onset, clear, modes or keys of fault_proc is NULL%s");
            const int K = p->n_modes;
            if (B >= 1) {          // (B < 1 is refused below, with the loop arguments)
                for (size_t r = 0; r < (size_t)p->batch * m; ++r)
                    for (int j = 1; j < K; ++j)
                        if (p->onset[r * K + j] < p->onset[r * K + j - 1]) return fail(h, SDEMPC_EINVAL, "events: an onset row decreases (the thresholds are cumulative)%s");
                for (size_t e = 0; e < (size_t)p->batch * m * K * 2; ++e)
                    if (!finite(p->modes[e])) return fail(h, SDEMPC_EINVAL, "events: modes holds a non-finite entry%s");
                for (size_t e = 0; p->state_in && e < (size_t)B * m; ++e)
                    if (p->state_in[2 * e] < 0 || p->state_in[2 * e] > K || p->state_in[2 * e + 1] < -1)
                        return fail(h, SDEMPC_EINVAL, "events: fault_proc state_in holds a state outside 0 .. n_modes or a first tick below -1%s");
            }
            if (p->tick0 < 0 || (long long)p->tick0 + T >= (1ll << 24)) return fail(h, SDEMPC_EINVAL, "events: tick0 must be >= 0 and tick0 + T below 2^24%s");
        }
        if (const sdempc_dropout_process_cfg* p = er.drop) {
            if (p->struct_size != (int32_t)sizeof(sdempc_dropout_process_cfg)) return fail(h, SDEMPC_EINVAL, "events: drop_proc struct_size mismatch%s");
            if (p->batch != 1 && p->batch != B) return fail(h, SDEMPC_EINVAL, "events: drop_proc batch must be 1 or B%s");
            if (!p->drop || !p->recover || !p->keys) return fail(h, SDEMPC_EINVAL, "events: drop, recover or keys of drop_proc is NULL%s");
            for (size_t e = 0; p->state_in && B >= 1 && e < (size_t)B; ++e)
                if (p->state_in[2 * e] < 0 || p->state_in[2 * e] > 1 || p->state_in[2 * e + 1] < 0)
                    return fail(h, SDEMPC_EINVAL, "events: drop_proc state_in holds a state outside 0 .. 1 or a negative count%s");
        }
        if (er.drop && !c.obs_keys) return fail(h, SDEMPC_EINVAL, "events: drop_proc needs an obs cfg and obs_keys%s");
    }
    const EventRun* evt = c.events && (c.er.fault || c.er.drop) ? &c.er : nullptr;
    const sdempc_track_cfg* tk = c.track;
    if (tk) {                  // SPEC.md §11j: the trajectory set, then what may not be given beside it
        if (int rc = check_track(h, tk, B, T)) return rc;
        if (io.xref || io.xref_ticks != 0) return fail(h, SDEMPC_EINVAL, "track: xref must be NULL and xref_solves 0 with a track cfg%s");
        if (tk->score_targets && !c.zc) return fail(h, SDEMPC_EINVAL, "track: score_targets needs a score cfg%s");
        if (tk->score_targets && c.zc->struct_size == (int32_t)sizeof(sdempc_score_cfg) && c.zc->score_ref) return fail(h, SDEMPC_EINVAL, "track: score_ref must be NULL with score_targets%s");
    }
    const bool targets = tk && tk->score_targets;
    if (c.drawn) {             // SPEC.md §11i: each process cfg with its coefficients, chain and state; an output needs its cfg
        const ProcRun& pr = c.pr;
        if (!pr.dist && (pr.dist_rows || pr.dist_keys_next || pr.dist_state_next))
            return fail(h, SDEMPC_EINVAL, "process: dist_rows / dist_keys_next / dist_state_next must be NULL without dist_proc%s");
        if (!pr.bias && (pr.bias_rows || pr.bias_keys_next || pr.bias_state_next))
            return fail(h, SDEMPC_EINVAL, "process: bias_rows / bias_keys_next / bias_state_next must be NULL without bias_proc%s");
        for (int w = 0; w < 2; ++w) {
            const sdempc_process_cfg* p = w ? pr.bias : pr.dist;
            const int W = w ? 12 : SDEMPC_NNOISE;
            if (!p) continue;
            if (p->struct_size != (int32_t)sizeof(sdempc_process_cfg)) return fail(h, SDEMPC_EINVAL, "process: struct_size mismatch%s");
            if (p->batch != 1 && p->batch != B) return fail(h, SDEMPC_EINVAL, "process: batch must be 1 or B%s");
            if (!p->rho || !p->scale || !p->keys) return fail(h, SDEMPC_EINVAL, "process: rho, scale or keys is NULL%s");
            if (B < 1) continue;           // (refused below, with the loop arguments)
            for (size_t e = 0; e < (size_t)p->batch * W; ++e) {
                if (!(p->rho[e] >= 0.0f) || !(p->rho[e] <= 1.0f)) return fail(h, SDEMPC_EINVAL, "process: rho holds an entry outside [0, 1]%s");
                if (!finite(p->scale[e]) || p->scale[e] < 0.0f) return fail(h, SDEMPC_EINVAL, "process: scale holds a non-finite or negative entry%s");
            }
            for (size_t e = 0; p->state_in && e < (size_t)B * W; ++e)
                if (!finite(p->state_in[e])) return fail(h, SDEMPC_EINVAL, "process: state_in holds a non-finite entry%s");
        }
        if (pr.bias && !c.obs_keys) return fail(h, SDEMPC_EINVAL, "process: bias_proc needs an obs cfg and obs_keys%s");
    }
    const ProcRun* proc = c.drawn && (c.pr.dist || c.pr.bias) ? &c.pr : nullptr;
    const sdempc_score_cfg* zc = c.scored ? c.zc : nullptr;
    if (c.scored) {
        if (!zc && (c.score_in || c.score_out)) return fail(h, SDEMPC_EINVAL, "score: score_in / score_out must be NULL without a score cfg%s");
        if (zc) {
            if (zc->struct_size != (int32_t)sizeof(sdempc_score_cfg)) return fail(h, SDEMPC_EINVAL, "score: struct_size mismatch%s");
            if (zc->substeps != 0 && zc->substeps != 1) return fail(h, SDEMPC_EINVAL, "score: substeps must be 0 (tick states) or 1 (plant substep states)%s");
            if (zc->r2_pos != zc->r2_pos || zc->cos_min != zc->cos_min || zc->w2_max != zc->w2_max) return fail(h, SDEMPC_EINVAL, "score: a threshold is NaN%s");
            if (!zc->score_ref && !targets) return fail(h, SDEMPC_EINVAL, "score: score_ref is NULL%s");
            if (!c.score_out) return fail(h, SDEMPC_EINVAL, "score: score_out is NULL%s");
        }
    }
    if (c.aged) {
        if (c.ac && c.ac->struct_size != (int32_t)sizeof(sdempc_age_cfg)) return fail(h, SDEMPC_EINVAL, "age: struct_size mismatch%s");
        if (c.ac && !c.oc) return fail(h, SDEMPC_EINVAL, "age: an age cfg needs an obs cfg%s");
        if (!c.ac && (c.xhist_in || c.xhist_next)) return fail(h, SDEMPC_EINVAL, "age: xhist_in / xhist_next must be NULL without an age cfg%s");
    }
    if (c.observed) {
        if (c.oc && c.oc->struct_size != (int32_t)sizeof(sdempc_obs_cfg)) return fail(h, SDEMPC_EINVAL, "obs: struct_size mismatch%s");
        if (!c.oc && (c.obs_keys || c.xmeas_in || c.xmeas || c.obs_keys_next || c.xmeas_next))
            return fail(h, SDEMPC_EINVAL, "obs: obs_keys / xmeas_in / xmeas / obs_keys_next / xmeas_next must be NULL without an obs cfg%s");
        if (c.oc && !c.obs_keys) return fail(h, SDEMPC_EINVAL, "obs: obs_keys is NULL%s");
    }
    if (c.faulted) {
        if (c.fc && c.fc->struct_size != (int32_t)sizeof(sdempc_fault_cfg)) return fail(h, SDEMPC_EINVAL, "fault: struct_size mismatch%s");
        if (!rated && (c.rate_integ_in || c.rate_tail_in || c.ws || c.rate_integ_next || c.rate_tail_next))
            return fail(h, SDEMPC_EINVAL, "fault: rate_integ_in / rate_tail_in / ws / rate_integ_next / rate_tail_next must be NULL without a rate cfg%s");
    }
    if (rated) {
        if (!rc_ || rc_->struct_size != (int32_t)sizeof(sdempc_rate_cfg)) return fail(h, SDEMPC_EINVAL, "rate: cfg NULL or struct_size mismatch%s");
        for (int a = 0; a < 3; ++a) {
            if (!finite(rc_->kp[a]) || !finite(rc_->ki_dt[a])) return fail(h, SDEMPC_EINVAL, "rate: kp / ki_dt hold a non-finite gain%s");
            if (!finite(rc_->integ_limit[a])) return fail(h, SDEMPC_EINVAL, "rate: integ_limit holds a non-finite limit%s");
            if (rc_->integ_limit[a] < 0.0f) return fail(h, SDEMPC_EINVAL, "rate: integ_limit must be >= 0%s");
        }
        for (int l = 0; l < h->m; ++l)
            for (int a = 0; a < 3; ++a)
                if (!finite(rc_->mixer[l][a])) return fail(h, SDEMPC_EINVAL, "rate: mixer holds a non-finite entry%s");
        if (!(rc_->motor_weight >= 0.0f) || !(rc_->motor_weight <= 1.0f)) return fail(h, SDEMPC_EINVAL, "rate: motor_weight must be in [0, 1]%s");
        if (rc_->inv_m != 0.0f && !(rc_->inv_m == inv_m)) return fail(h, SDEMPC_EINVAL, "rate: inv_m must be 0 or (float)1 / (float)num_motors%s");
        if (!c.ws && !zc) return fail(h, SDEMPC_EINVAL, "rate: ws is NULL%s");
        if (sc && sc->struct_size != (int32_t)sizeof(sdempc_scenario_cfg)) return fail(h, SDEMPC_EINVAL, "scenario: struct_size mismatch%s");
    } else if (scenario) {
        if ((!sc && !c.faulted) || (sc && sc->struct_size != (int32_t)sizeof(sdempc_scenario_cfg))) return fail(h, SDEMPC_EINVAL, "scenario: cfg NULL or struct_size mismatch%s");
    }
    if (timed) {
        if (!tc || tc->struct_size != (int32_t)sizeof(sdempc_timing_cfg)) return fail(h, SDEMPC_EINVAL, "timing: cfg NULL or struct_size mismatch%s");
        if (tc->solve_period < 1) return fail(h, SDEMPC_EINVAL, "timing: solve_period must be >= 1%s");
        if (!(tc->lag_alpha >= 0.0f) || !(tc->lag_alpha <= 1.0f)) return fail(h, SDEMPC_EINVAL, "timing: lag_alpha must be 0 (off) or in (0, 1]%s");
    }
    int rc = check_loop_args(h, io, !timed ? T : (T >= 1 ? loop_solves(T, tc->solve_period) : 1), zc != nullptr, tk != nullptr);
    if (rc) return rc;
    const int Tp = scenario && sc ? sc->plant_ticks : 1;           // rows of plant_of
    if (Tp != 1 && Tp != T) return fail(h, SDEMPC_EINVAL, "scenario: plant_ticks must be 1 or T%s");
    if (Tp > 1 && !c.plant_of) return fail(h, SDEMPC_EINVAL, "scenario: plant_of may not be NULL with plant_ticks > 1%s");
    if (c.layer >= LOOP_PLANT && (rc = check_plant_args(h, c.pc, c.plant_blobs, c.plant_blob_bytes, c.plant_of, B, Tp))) return rc;
    if (timed && (tc->solve_delay < 0 || (long long)tc->solve_delay > (long long)tc->solve_period * c.pc->substeps))
        return fail(h, SDEMPC_EINVAL, "timing: solve_delay must be between 0 and solve_period * substeps (one solve at a time)%s");
    const float* dist = scenario && sc ? sc->dist : nullptr;
    if (dist) {
        if (sc->dist_ticks != 1 && sc->dist_ticks != T) return fail(h, SDEMPC_EINVAL, "scenario: dist_ticks must be 1 or T%s");
        if (sc->dist_batch != 1 && sc->dist_batch != B) return fail(h, SDEMPC_EINVAL, "scenario: dist_batch must be 1 or B%s");
        const size_t nd = (size_t)sc->dist_ticks * sc->dist_batch * SDEMPC_NNOISE;
        for (size_t e = 0; e < nd; ++e)
            if (!finite(dist[e])) return fail(h, SDEMPC_EINVAL, "scenario: dist holds a non-finite entry%s");
    }
    const float* fault = c.faulted && c.fc ? c.fc->fault : nullptr;
    if (fault) {
        if (c.fc->fault_ticks != 1 && c.fc->fault_ticks != T) return fail(h, SDEMPC_EINVAL, "fault: fault_ticks must be 1 or T%s");
        if (c.fc->fault_batch != 1 && c.fc->fault_batch != B) return fail(h, SDEMPC_EINVAL, "fault: fault_batch must be 1 or B%s");
        const size_t nf = (size_t)c.fc->fault_ticks * c.fc->fault_batch * h->m * 2;
        for (size_t e = 0; e < nf; ++e)
            if (!finite(fault[e])) return fail(h, SDEMPC_EINVAL, "fault: the schedule holds a non-finite entry%s");
    }
    const sdempc_obs_cfg* oc = c.observed ? c.oc : nullptr;
    if (oc) {
        const int Ns = loop_solves(T, tc->solve_period);
        if (oc->sigma || oc->beta) {
            if (oc->obs_solves != 1 && oc->obs_solves != Ns) return fail(h, SDEMPC_EINVAL, "obs: obs_solves must be 1 or ceil(T / solve_period)%s");
            if (oc->obs_batch != 1 && oc->obs_batch != B) return fail(h, SDEMPC_EINVAL, "obs: obs_batch must be 1 or B%s");
            const size_t no = (size_t)oc->obs_solves * oc->obs_batch * 12;
            for (size_t e = 0; oc->sigma && e < no; ++e)
                if (!finite(oc->sigma[e]) || oc->sigma[e] < 0.0f) return fail(h, SDEMPC_EINVAL, "obs: sigma holds a non-finite or negative entry%s");
            for (size_t e = 0; oc->beta && e < no; ++e)
                if (!finite(oc->beta[e])) return fail(h, SDEMPC_EINVAL, "obs: beta holds a non-finite entry%s");
        }
        if (oc->valid) {
            if (oc->valid_solves != 1 && oc->valid_solves != Ns) return fail(h, SDEMPC_EINVAL, "obs: valid_solves must be 1 or ceil(T / solve_period)%s");
            if (oc->valid_batch != 1 && oc->valid_batch != B) return fail(h, SDEMPC_EINVAL, "obs: valid_batch must be 1 or B%s");
            const size_t nv = (size_t)oc->valid_solves * oc->valid_batch;
            for (size_t e = 0; e < nv; ++e)
                if (oc->valid[e] != 0 && oc->valid[e] != 1) return fail(h, SDEMPC_EINVAL, "obs: valid holds an entry other than 0 / 1%s");
        }
    }
    const sdempc_age_cfg* ac = c.aged ? c.ac : nullptr;
    if (ac) {
        const int Ns = loop_solves(T, tc->solve_period);
        const long long lim = (long long)(tc->solve_period < T ? tc->solve_period : T) * c.pc->substeps;        // one period of memory
        if (ac->age_max < 0 || ac->age_max > lim) return fail(h, SDEMPC_EINVAL, "age: age_max must be between 0 and min(solve_period, T) * substeps%s");
        if (ac->age) {
            if (ac->age_solves != 1 && ac->age_solves != Ns) return fail(h, SDEMPC_EINVAL, "age: age_solves must be 1 or ceil(T / solve_period)%s");
            if (ac->age_batch != 1 && ac->age_batch != B) return fail(h, SDEMPC_EINVAL, "age: age_batch must be 1 or B%s");
            const size_t na = (size_t)ac->age_solves * ac->age_batch;
            for (size_t e = 0; e < na; ++e)
                if (ac->age[e] < 0 || ac->age[e] > ac->age_max) return fail(h, SDEMPC_EINVAL, "age: age holds an entry outside [0, age_max]%s");
        }
        if (ac->renormalise != 0 && ac->renormalise != 1) return fail(h, SDEMPC_EINVAL, "age: renormalise must be 0 or 1%s");
        if (ac->age_max == 0 && (c.xhist_in || c.xhist_next)) return fail(h, SDEMPC_EINVAL, "age: xhist_in / xhist_next must be NULL with age_max 0%s");
    }
    if (zc && !targets) {
        if (zc->ref_ticks != 1 && zc->ref_ticks != T) return fail(h, SDEMPC_EINVAL, "score: ref_ticks must be 1 or T%s");
        if (zc->ref_batch != 1 && zc->ref_batch != B) return fail(h, SDEMPC_EINVAL, "score: ref_batch must be 1 or B%s");
    }
    if ((rc = ensure_device(h))) return rc;
    if (c.layer == LOOP_PLAIN) return closed_loop_attempts(h, io, nullptr, nullptr, nullptr, nullptr);
    const TimedRun run_t{timed ? tc->solve_period : 1, timed ? tc->solve_delay : 0, timed ? tc->lag_alpha : 0.0f, c.u_act_in, c.u_act_next};
    const ScenarioRun run_s{dist, dist ? sc->dist_ticks : 1, dist ? sc->dist_batch : 1, c.plant_of, Tp};
    const RateRun run_r{rc_, inv_m, c.rate_integ_in, c.rate_tail_in, c.ws, c.rate_integ_next, c.rate_tail_next};
    const FaultRun run_f{fault, fault ? c.fc->fault_ticks : 1, fault ? c.fc->fault_batch : 1, c.faulted ? c.xsub : nullptr};
    const bool rows = oc && (oc->sigma || oc->beta);
    const ObsRun run_o{oc ? oc->sigma : nullptr, oc ? oc->beta : nullptr, rows ? oc->obs_solves : 1, rows ? oc->obs_batch : 1, oc ? oc->valid : nullptr,
                       oc && oc->valid ? oc->valid_solves : 1, oc && oc->valid ? oc->valid_batch : 1, c.obs_keys, c.xmeas_in, c.xmeas, c.obs_keys_next, c.xmeas_next,
                       ac ? ac->age : nullptr, ac && ac->age ? ac->age_solves : 1, ac && ac->age ? ac->age_batch : 1, ac ? ac->age_max : 0, ac && ac->renormalise != 0,
                       c.xhist_in, c.xhist_next};
    PlantRun run;
    // (a schedule is staged per chunk by the loop, where stage_plants takes the set itself; the noise of a whole solve period sits beside the set)
    if ((rc = stage_plants(h, *c.pc, c.plant_blobs, scenario ? nullptr : c.plant_of, B, &run, !timed ? 1 : (tc->solve_period < T ? tc->solve_period : T)))) return rc;
    const ScoreRun run_z{zc, c.score_in, c.score_out};
    TrackRun run_k;
    if (tk && (rc = stage_track(h, *tk, B, &run_k))) return rc;
    const EnsRun run_e{c.ens, c.ens_out};
    const RetireRun run_y{c.retired_at, c.live_per_solve};
    return closed_loop_attempts(h, io, &run, timed ? &run_t : nullptr, scenario ? &run_s : nullptr, rated ? &run_r : nullptr,
                                run_f.fault || run_f.xsub || (evt && evt->fault) ? &run_f : nullptr, oc ? &run_o : nullptr, zc ? &run_z : nullptr, proc, tk ? &run_k : nullptr, evt,
                                c.baseline ? &run_g : nullptr, c.ens ? &run_e : nullptr, c.retiring && c.retire ? &run_y : nullptr);
}
// every check of a geometric-controller cfg (SPEC.md §11l), shared by the two entry points that take one; no HIP call. inv_dt: what the launch is given
int check_geo(sdempc_handle* h, const sdempc_geo_cfg* g, int B, float* inv_dt) {
    auto ok = [](float v) { return fabsf(v) < INFINITY && v >= 0.0f; };
    auto finite = [](float v) { return fabsf(v) < INFINITY; };
    if (!g || g->struct_size != (int32_t)sizeof(sdempc_geo_cfg)) return fail(h, SDEMPC_EINVAL, "baseline: cfg NULL or struct_size mismatch%s");
    if (g->batch != 1 && g->batch != B) return fail(h, SDEMPC_EINVAL, "baseline: batch must be 1 or B%s");
    if (!g->kp || !g->kv || !g->amax || !g->inv_tau || !g->g || !g->kT || !g->k0 || !g->c_lo || !g->c_hi) return fail(h, SDEMPC_EINVAL, "baseline: a parameter array is NULL%s");
    if (g->accel_ff != 0 && g->accel_ff != 1) return fail(h, SDEMPC_EINVAL, "baseline: accel_ff must be 0 or 1%s");
    if (g->ref_row < 0 || g->ref_row > h->H - 1) return fail(h, SDEMPC_EINVAL, "baseline: ref_row must be between 0 and H - 1%s");
    const float want = 1.0f / h->time_steps[g->ref_row];
    if (g->inv_dt != 0.0f && !(g->inv_dt == want)) return fail(h, SDEMPC_EINVAL, "baseline: inv_dt must be 0 or (float)1 / time_steps[ref_row]%s");
    *inv_dt = want;
    for (int r = 0; B >= 1 && r < g->batch; ++r) {     // (B < 1 is refused with the loop arguments)
        for (int a = 0; a < 3; ++a)
            if (!ok(g->kp[3 * r + a]) || !ok(g->kv[3 * r + a])) return fail(h, SDEMPC_EINVAL, "baseline: kp / kv hold a non-finite or negative gain%s");
        if (!ok(g->amax[r]) || !ok(g->inv_tau[r]) || !ok(g->g[r])) return fail(h, SDEMPC_EINVAL, "baseline: amax, inv_tau or g is non-finite or negative%s");
        if (!finite(g->kT[r]) || !finite(g->k0[r])) return fail(h, SDEMPC_EINVAL, "baseline: kT or k0 is non-finite%s");
        if (!(g->c_lo[r] <= g->c_hi[r])) return fail(h, SDEMPC_EINVAL, "baseline: c_lo must not exceed c_hi%s");
        for (int l = 0; l < h->m; ++l)
            if (!(g->c_lo[r] >= h->cfg.u_lo[l]) || !(g->c_hi[r] <= h->cfg.u_hi[l])) return fail(h, SDEMPC_EINVAL, "baseline: c_lo / c_hi must lie inside every motor's input_bound%s");
    }
    return 0;
}
// the parameter rows of a checked cfg onto the device (d_geo: GEO_PAR_WORDS floats per set), on st; the host image is copied before the call returns
int stage_geo(sdempc_handle* h, const sdempc_geo_cfg& g, hipStream_t st) {
    int rc;
    if (!h->d_geo.p && (rc = dev_alloc(h, h->d_geo, sizeof(float) * (GEO_PAR_WORDS + 4) * (size_t)h->max_batch, true))) return rc;
    std::vector<float> rows((size_t)g.batch * GEO_PAR_WORDS, 0.0f);
    for (int r = 0; r < g.batch; ++r) {
        float* row = &rows[(size_t)r * GEO_PAR_WORDS];
        for (int a = 0; a < 3; ++a) { row[a] = g.kp[3 * r + a]; row[3 + a] = g.kv[3 * r + a]; }
        row[6] = g.amax[r]; row[7] = g.inv_tau[r]; row[8] = g.g[r]; row[9] = g.kT[r]; row[10] = g.k0[r]; row[11] = g.c_lo[r]; row[12] = g.c_hi[r];
    }
    HIPCHK(h, hipMemcpyAsync(h->d_geo.p, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));       // (rows dies with this frame)
    return 0;
}
// every check of a trajectory set (SPEC.md §11j), shared by the two entry points that take one; no HIP call. ticks: control ticks of the call (tick0 + ticks < 2^24)
int check_track(sdempc_handle* h, const sdempc_track_cfg* tk, int B, long long ticks) {
    auto finite = [](float v) { return fabsf(v) < INFINITY; };
    if (tk->struct_size != (int32_t)sizeof(sdempc_track_cfg)) return fail(h, SDEMPC_EINVAL, "track: struct_size mismatch%s");
    if (tk->n_tables < 1) return fail(h, SDEMPC_EINVAL, "track: n_tables must be >= 1%s");
    if (!tk->knots || !tk->t || !tk->x) return fail(h, SDEMPC_EINVAL, "track: knots, t or x is NULL%s");
    size_t f = 0;
    for (int j = 0; j < tk->n_tables; ++j) {
        const int L = tk->knots[j];
        if (L < 1) return fail(h, SDEMPC_EINVAL, "track: a table has fewer than 1 knot%s");
        const float* t = tk->t + f;
        for (int i = 0; i < L; ++i)
            if (!finite(t[i]) || (i > 0 && !(t[i] > t[i - 1]))) return fail(h, SDEMPC_EINVAL, "track: t must be finite and strictly increasing%s");
        for (size_t e = 0; e < (size_t)L * SDEMPC_NX; ++e)
            if (!finite(tk->x[f * SDEMPC_NX + e])) return fail(h, SDEMPC_EINVAL, "track: x holds a non-finite entry%s");
        const float period = tk->period ? tk->period[j] : 0.0f;
        if (!finite(period) || period < 0.0f) return fail(h, SDEMPC_EINVAL, "track: period must be finite and >= 0%s");
        if (period > 0.0f && (t[0] != 0.0f || t[L - 1] != period)) return fail(h, SDEMPC_EINVAL, "track: a periodic table needs t[0] = 0 and t[L-1] = period%s");
        f += (size_t)L;
    }
    for (int b = 0; b < B; ++b) {
        if (tk->table_of && (tk->table_of[b] < 0 || tk->table_of[b] >= tk->n_tables)) return fail(h, SDEMPC_EINVAL, "track: table_of holds an index outside [0, n_tables)%s");
        if (tk->phase && !finite(tk->phase[b])) return fail(h, SDEMPC_EINVAL, "track: phase holds a non-finite entry%s");
        if (tk->rate && (!finite(tk->rate[b]) || tk->rate[b] < 0.0f)) return fail(h, SDEMPC_EINVAL, "track: rate holds a non-finite or negative entry%s");
        for (int a = 0; tk->offset && a < 3; ++a)
            if (!finite(tk->offset[(size_t)b * 3 + a])) return fail(h, SDEMPC_EINVAL, "track: offset holds a non-finite entry%s");
    }
    if ((tk->renorm != 0 && tk->renorm != 1) || (tk->score_targets != 0 && tk->score_targets != 1)) return fail(h, SDEMPC_EINVAL, "track: renorm and score_targets must be 0 or 1%s");
    if (tk->tick0 < 0) return fail(h, SDEMPC_EINVAL, "track: tick0 must be >= 0%s");
    if ((long long)tk->tick0 + ticks >= (1ll << 24)) return fail(h, SDEMPC_EINVAL, "track: tick0 + T must stay below 2^24 (the clock is float32(tick) * dt)%s");
    return 0;
}
// SPEC.md §11j. Forms w, inv_period and c, fills in the defaults of the per-episode numbers (table 0, phase 0, rate 1, offset 0) and stages the set on the device ONCE per
// call, in one allocation and one copy on the handle's stream. The launches only read it, so a re-run finds it as it was. The arguments were checked by the caller.
int stage_track(sdempc_handle* h, const sdempc_track_cfg& tk, int B, TrackRun* out) {
    const int NT = tk.n_tables, H = h->H;
    size_t SL = 0;
    for (int j = 0; j < NT; ++j) SL += (size_t)tk.knots[j];
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_first = 0, o_knots = o_first + up16(sizeof(int32_t) * NT), o_period = o_knots + up16(sizeof(int32_t) * NT), o_inv = o_period + up16(sizeof(float) * NT);
    const size_t o_t = o_inv + up16(sizeof(float) * NT), o_w = o_t + up16(sizeof(float) * SL), o_x = o_w + up16(sizeof(float) * SL), o_c = o_x + up16(sizeof(float) * SL * SDEMPC_NX);
    const size_t o_of = o_c + up16(sizeof(float) * (H + 1)), o_phase = o_of + up16(sizeof(int32_t) * B), o_rate = o_phase + up16(sizeof(float) * B);
    const size_t o_off = o_rate + up16(sizeof(float) * B), total = o_off + up16(sizeof(float) * B * 3);
    std::vector<char>& stg = h->track_stage;
    stg.assign(total, 0);
    int32_t* first = (int32_t*)&stg[o_first];
    float* inv = (float*)&stg[o_inv];
    float* w = (float*)&stg[o_w];
    float* cc = (float*)&stg[o_c];
    size_t f = 0;
    for (int j = 0; j < NT; ++j) {
        const int L = tk.knots[j];
        first[j] = (int32_t)f;
        for (int i = 0; i + 1 < L; ++i) w[f + i] = (float)(1.0 / ((double)tk.t[f + i + 1] - (double)tk.t[f + i]));
        const float period = tk.period ? tk.period[j] : 0.0f;
        inv[j] = period > 0.0f ? (float)(1.0 / (double)period) : 0.0f;
        f += (size_t)L;
    }
    memcpy(&stg[o_knots], tk.knots, sizeof(int32_t) * NT);
    if (tk.period) memcpy(&stg[o_period], tk.period, sizeof(float) * NT);
    memcpy(&stg[o_t], tk.t, sizeof(float) * SL);
    memcpy(&stg[o_x], tk.x, sizeof(float) * SL * SDEMPC_NX);
    double acc = 0.0;
    for (int i = 0; i <= H; ++i) { cc[i] = (float)acc; if (i < H) acc += (double)h->time_steps[i]; }
    if (tk.table_of) memcpy(&stg[o_of], tk.table_of, sizeof(int32_t) * B);
    if (tk.phase) memcpy(&stg[o_phase], tk.phase, sizeof(float) * B);
    float* rate = (float*)&stg[o_rate];
    for (int b = 0; b < B; ++b) rate[b] = tk.rate ? tk.rate[b] : 1.0f;
    if (tk.offset) memcpy(&stg[o_off], tk.offset, sizeof(float) * B * 3);
    int rc;
    if (h->d_track.bytes < total) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        dev_free(h->d_track);
        if ((rc = dev_alloc(h, h->d_track, total, true))) return rc;      // (every byte a launch reads is copied in below, on the stream, before anything reads it)
    }
    char* d = (char*)h->d_track.p;
    HIPCHK(h, hipMemcpyAsync(d, stg.data(), total, hipMemcpyHostToDevice, h->stream));
    LoopTrack& K = out->K;
    K = LoopTrack{};
    K.t = (const float*)(d + o_t); K.w = (const float*)(d + o_w); K.x = (const float*)(d + o_x);
    K.first = (const int32_t*)(d + o_first); K.knots = (const int32_t*)(d + o_knots); K.period = (const float*)(d + o_period); K.inv_period = (const float*)(d + o_inv);
    K.c = (const float*)(d + o_c); K.table_of = (const int32_t*)(d + o_of); K.phase = (const float*)(d + o_phase); K.rate = (const float*)(d + o_rate);
    K.offset = (const float*)(d + o_off);
    K.dt = h->time_steps[0]; K.tick0 = tk.tick0; K.B = B; K.renorm = tk.renorm;
    out->score_targets = tk.score_targets != 0;
    return 0;
}
// argument checks every closed-loop entry point shares; no HIP call
// rows_optional (SPEC.md §11h, a call with a score cfg): xs / us / info may be NULL
// tracked (SPEC.md §11j, a call with a track cfg): xref is NULL and its two counts are not read
int check_loop_args(sdempc_handle* h, const LoopIo& io, int solves, bool rows_optional, bool tracked) {
    int rc = check_batch(h, io.B);
    if (rc) return rc;
    if (io.T < 1) return fail(h, SDEMPC_EINVAL, "closed loop: T must be >= 1%s");
    if (tracked) {
        if (!io.x0 || !io.keys || (!rows_optional && (!io.xs || !io.us || !io.info))) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
        return 0;
    }
    if (io.xref_ticks != 1 && io.xref_ticks != solves)
        return fail(h, SDEMPC_EINVAL, solves == io.T ? "closed loop: xref_ticks must be 1 or T%s" : "closed loop: xref_solves must be 1 or ceil(T / solve_period)%s");
    if (io.xref_batch != 1 && io.xref_batch != io.B) return fail(h, SDEMPC_EINVAL, "closed loop: xref_batch must be 1 or B%s");
    if (!io.x0 || !io.xref || !io.keys || (!rows_optional && (!io.xs || !io.us || !io.info))) return fail(h, SDEMPC_EINVAL, "NULL host pointer%s");
    return 0;
}
// every check of a plant set (SPEC.md §11a), shared by the four entry points that take one; no HIP call
// sched_rows: rows of plant_of (SPEC.md §11c: a plant index per tick and episode; 1 everywhere else)
int check_plant_args(sdempc_handle* h, const sdempc_plant_cfg* pc, const void* const* plant_blobs, const size_t* plant_blob_bytes, const int32_t* plant_of, int B, int sched_rows) {
    int rc;
    if (!pc || pc->struct_size != (int32_t)sizeof(sdempc_plant_cfg)) return fail(h, SDEMPC_EINVAL, "plant: cfg NULL or struct_size mismatch%s");
    if (pc->num_plants < 1 || (long long)pc->num_plants > (long long)B * sched_rows)
        return fail(h, SDEMPC_EINVAL, sched_rows > 1 ? "plant: num_plants must be between 1 and B * plant_ticks%s" : "plant: num_plants must be between 1 and B%s");
    if (pc->substeps < 1 || pc->substeps > SDEMPC_PLANT_MAX_SUBSTEPS) return fail(h, SDEMPC_EINVAL, "plant: substeps must be between 1 and SDEMPC_PLANT_MAX_SUBSTEPS (64)%s");
    if (!(pc->dt >= 0.0f) || !(pc->dt < INFINITY)) return fail(h, SDEMPC_EINVAL, "plant: dt must be finite and >= 0 (0: time_steps[0] / substeps)%s");
    if (pc->mlp_dtype < -1 || pc->mlp_dtype > 2) return fail(h, SDEMPC_EINVAL, "plant: mlp_dtype must be -1 (the handle's), 0 (f32), 1 (f16) or 2 (f32x3)%s");
    if (pc->math_mode < -1 || pc->math_mode > 1) return fail(h, SDEMPC_EINVAL, "plant: math_mode must be -1 (the handle's), 0 (exact) or 1 (fast)%s");
    if (!plant_blobs || !plant_blob_bytes) return fail(h, SDEMPC_EINVAL, "plant: NULL blob table%s");
    const int Np = pc->num_plants;
    if (!plant_of && Np != 1 && Np != B) return fail(h, SDEMPC_EINVAL, "plant: plant_of may be NULL only when num_plants is 1 or B%s");
    if (plant_of)
        for (size_t b = 0; b < (size_t)B * sched_rows; ++b)
            if (plant_of[b] < 0 || plant_of[b] >= Np) return fail(h, SDEMPC_EINVAL, "plant: plant_of holds an index outside [0, num_plants)%s");
    for (int p = 0; p < Np; ++p) {
        if ((rc = check_blob(h, plant_blobs[p], plant_blob_bytes[p]))) return rc;
        if (((const int32_t*)plant_blobs[p])[2] != h->m) return fail(h, SDEMPC_EINVAL, "plant: num_motors of a plant blob differs from the handle's%s");
    }
    return 0;
}
// the loop, and once more from the host inputs if a cooperative-layout barrier gave up or the ticket count was off (closed_loop_run)
int closed_loop_attempts(sdempc_handle* h, const LoopIo& io, const PlantRun* plant, const TimedRun* timed, const ScenarioRun* scen, const RateRun* rate, const FaultRun* flt,
                         const ObsRun* obs, const ScoreRun* score, const ProcRun* proc, const TrackRun* track, const EventRun* evt, const GeoRun* geo, const EnsRun* ens,
                         const RetireRun* ret) {
    for (int attempt = 0;; ++attempt) {
        bool again = false;
        int rc = closed_loop_run(h, io, plant, timed, scen, rate, flt, obs, score, proc, track, evt, geo, ens, ret, &again);
        if (rc) return rc;
        if (!again) return SDEMPC_OK;
        if (attempt) return fail(h, SDEMPC_EDEVICE, "closed loop: a cooperative-layout grid barrier gave up or the ticket count was off twice%s");
    }
}
// SPEC.md §11a. Prepares every plant blob for the plant's arithmetic and step length exactly as sdempc_create prepares the handle's (prepare_model) and
// stages the set on the device ONCE per call, in one allocation and one copy on the handle's stream: [ModelK x Np][payload x Np][sigma sqrt(dt) x Np][dt]
// [plant_of x B], then room for the plant noise of a tick (of xi_ticks ticks: a solve period of SPEC.md §11b). The arguments were checked by the caller.
int stage_plants(sdempc_handle* h, const sdempc_plant_cfg& pc, const void* const* blobs, const int32_t* plant_of, int B, PlantRun* out, int xi_ticks) {
    const int Np = pc.num_plants, n = pc.substeps;
    const int dtype = pc.mlp_dtype < 0 ? h->cfg.mlp_dtype : pc.mlp_dtype, mode = pc.math_mode < 0 ? h->cfg.math_mode : pc.math_mode;
    const float dt = pc.dt == 0.0f ? h->time_steps[0] / (float)n : pc.dt;
    const size_t stride = (size_t)SDEMPC_BLOB_FLOATS * (mode == 1 ? 2 : 1);
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_model = 0, o_wts = up16(sizeof(ModelK) * Np), o_sdt = o_wts + up16(sizeof(float) * stride * Np);
    const size_t o_dt = o_sdt + up16(sizeof(float) * SDEMPC_NNOISE * Np), o_of = o_dt + 16, o_xi = o_of + up16(sizeof(int32_t) * (plant_of ? B : 0));
    const size_t total = o_xi + sizeof(float) * (size_t)B * n * SDEMPC_NNOISE * (size_t)xi_ticks;      // (§11b: the noise of a whole solve period)
    std::vector<char>& stg = h->plant_stage;
    stg.assign(o_xi, 0);
    PreparedModel pm;
    for (int p = 0; p < Np; ++p) {
        if (const char* why = prepare_model((const float*)((const int32_t*)blobs[p] + SDEMPC_BLOB_HEADER_INTS), dtype, mode, &dt, 1, pm))
            return fail(h, SDEMPC_EINVAL, "plant: model refused: %s", why);
        memcpy(&stg[o_model + sizeof(ModelK) * p], &pm.M, sizeof(ModelK));
        memcpy(&stg[o_wts + sizeof(float) * stride * p], pm.blob_f.data(), sizeof(float) * stride);
        memcpy(&stg[o_sdt + sizeof(float) * SDEMPC_NNOISE * p], pm.sdt.data(), sizeof(float) * SDEMPC_NNOISE);
        if (p == 0) out->k.M = pm.M;
    }
    memcpy(&stg[o_dt], &dt, sizeof dt);
    if (plant_of) memcpy(&stg[o_of], plant_of, sizeof(int32_t) * B);
    int rc;
    if (h->d_plant.bytes < total) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        dev_free(h->d_plant);
        if ((rc = dev_alloc(h, h->d_plant, total, true))) return rc;      // (tables and indices are copied in below, on the stream, before anything reads them)
    }
    char* d = (char*)h->d_plant.p;
    HIPCHK(h, hipMemcpyAsync(d, stg.data(), o_xi, hipMemcpyHostToDevice, h->stream));
    const ModelK M0 = out->k.M;
    out->k = h->base;
    out->k.f16 = dtype; out->k.fast = mode == 1;
    out->k.M = M0;                                      // (read by the kernel only when every episode shares plant 0)
    out->k.wts = (const float*)(d + o_wts); out->k.sdt = (const float*)(d + o_sdt); out->k.dt = (const float*)(d + o_dt);
    const bool shared = Np == 1;
    out->Q.models = shared ? nullptr : (const ModelK*)(d + o_model);
    out->Q.wts = out->k.wts; out->Q.sdt = out->k.sdt;
    out->Q.plant_of = plant_of && !shared ? (const int*)(d + o_of) : nullptr;
    out->Q.wts_stride = (int)stride; out->Q.substeps = n;
    out->xi = (float*)(d + o_xi);
    out->dt = dt;
    return 0;
}
// Device memory the per-tick buffers of one chunk of closed-loop ticks may take (sdempc_closed_loop_batch): the outputs (x_{k+1}, u_k, info_k)
// of every episode and, when the reference moves per tick, the chunk's reference windows. T itself is unbounded: outputs are copied back and
// references staged once per chunk (one host synchronisation per chunk, none per tick).
constexpr size_t LOOP_CHUNK_BYTES = (size_t)256 << 20;

// SPEC.md §11. Stages the host inputs, enqueues every tick of a chunk on the handle's stream (key schedule, noise, solve, plant step), copies
// the chunk's outputs back and checks, once per chunk, whether a grid barrier of a cooperative-layout solve gave up or the ticket count of the
// persistent launches is off: *again = true then, and the caller runs the whole batch once more from the host inputs (the handle has left
// the cooperative layouts; results are the same in every layout).
// SPEC.md §11b (timed): the unit of work is a solve PERIOD of S ticks — one key schedule, one solve and one plant launch per period, chunks of whole
// periods, info and moving references per solve. Without `timed` a period is one tick and every launch is the one it was (S = 1 below).
// SPEC.md §11c (scen, with timed and plant): the chunk's disturbance rows and plant-schedule rows (one per TICK) are staged per chunk beside the moving
// references and counted in the chunk's bytes; a schedule of one row is staged once. The plant launch then takes a LoopScenario.
// SPEC.md §11d (rate, with scen, timed and plant): the integrator and the rate tail live in d_rate (staged from the inputs, or zeroed, with the other inputs, so that a
// re-run starts from them again) and carry over period and chunk boundaries there; the chunk's setpoint rows ws sit behind its other outputs and are counted in
// the chunk's bytes. The plant launch then takes a LoopRate and reads the solve's mean trajectories where the solve left them (d_xmean).
// SPEC.md §11e (flt, with scen, timed and plant; with or without rate): the chunk's fault rows (one per TICK) are staged like the disturbance rows, behind the
// setpoint rows; the chunk's substep states xsub (substeps rows per tick) sit behind them, are counted in the chunk's bytes and copied back with the other outputs.
// The plant launch then takes a LoopFault.
// SPEC.md §11f (obs, with scen-or-not, timed and plant): the observation keys and the held measurement live in d_obs (staged from the inputs with the other inputs, so that a
// re-run starts from them again); the period's key schedule forms the measurement (LoopObserve) and the solve starts from it (d_xm) instead of d_x, which stays the
// plant's. The chunk's xmeas rows (one per SOLVE) sit behind xsub, are counted in the chunk's bytes and copied back with info; the sigma / beta / valid rows sit
// behind them, staged per chunk when they move (one per solve, like moving references) and once otherwise.
// SPEC.md §11g (obs with an age cfg): the last age_max substep states before the coming solve live in d_hist as [age_max][B][13], oldest first (staged from xhist_in or
// x0 with the other inputs, so that a re-run starts from them again). With age_max > 0 the run takes the §11e kernels with an xsub region in the chunk whether or not the
// caller asked for xsub (copied back only if they did): after each plant launch the history is refilled, by device-to-device copies on the stream, from the period's
// substep rows — and, where it reaches back that far, from the plant state before the launch and from its own newer rows (a partial last period). So it carries over
// period and chunk boundaries in d_hist alone. The age rows sit behind the valid rows, staged like them.
// SPEC.md §11h (score, with timed and plant): the score words live in d_score (staged from score_in, or as the initial row, with the other inputs, so that a re-run starts
// from them again). At the end of every chunk ONE launch of the period's key-schedule kernel in its scoring form walks the chunk's rows — xs, or xsub with substeps = 1,
// which then exists in the chunk as with age_max > 0 — and its us and info rows. The target rows sit behind the age rows, staged per chunk when they move (one per TICK) and
// once otherwise. A per-row output the caller passed as NULL is neither copied back nor scattered.
// SPEC.md §11i (proc, with scen, timed and plant): the process chains, states and coefficients live in d_proc (staged from the cfgs with the other inputs, so that a re-run
// starts from them again). The period's key-schedule launch takes a LoopProcess: with a disturbance process it writes the period's rows of a [Tc][B][6] region of the chunk,
// which the plant launch then reads as its disturbance (a scheduled disturbance given as well is staged beside it, as before, and read by the key schedule); with a bias
// process it writes the solve's row of a [Pc][B][12] region and forms the measurement from it (a scheduled beta likewise). Both regions count in the chunk's bytes and
// are copied back and scattered only when the caller asked for the rows.
// SPEC.md §11j (track, with timed and plant): the trajectory set lives in d_track (staged once per call by stage_track). In front of every solve ONE launch of the row-filling
// kernel in its tracking form writes the B windows of the period's first tick into d_xref, where a shared window was broadcast to before; the chunk has no xref region and
// takes no xref copy. With score targets, one more launch per chunk writes the chunk's [Tc][B][13] target rows in front of the scoring launch, in place of their copy.
// SPEC.md §11k (evt, with scen, timed and plant): the event chains, states, thresholds and modes live in d_evt (staged from the cfgs with the other inputs, so that a re-run
// starts from them again). The period's key-schedule launch takes a LoopEvents: with a fault chain it writes the period's rows of a [Tc][B][m][2] region of the chunk, which
// the plant launch then reads as its fault rows (a scheduled fault given as well is staged beside it, as before, and read by the key schedule); with a dropout chain it
// writes the solve's flags into a [Pc][B] region, which the measurement reads as its valid flags (scheduled flags likewise). Both regions count in the chunk's bytes and are
// copied back and scattered only when the caller asked for the rows.
// SPEC.md §11n (ret, with score): the live flags, the list, n_live and the dense staging live in d_retire. The scoring launch runs once per PERIOD, masked by the live
// flags, followed by the two live-list launches; n_live is read back in front of every solve (one synchronisation per period). With n_live == B the period's launches are
// the ones they were; below B the solve runs on the gathered live set and its results are scattered back (coop_bar then stays out of the plant launch: the scatter folds
// the give-up words); with the controller the baseline launch takes the mask. The ensemble launches stay per chunk and count rows by the loop's own counter.
int closed_loop_run(sdempc_handle* h, const LoopIo& io, const PlantRun* plant, const TimedRun* timed, const ScenarioRun* scen, const RateRun* rate, const FaultRun* flt, const ObsRun* obs,
                    const ScoreRun* score, const ProcRun* proc, const TrackRun* track, const EventRun* evt, const GeoRun* geo, const EnsRun* ens, const RetireRun* ret, bool* again) {
    *again = false;
    const bool flown = geo && rate && timed && plant;                      // (SPEC.md §11l: the geometric controller in place of the solve)
    const bool tracked = track && timed && plant;                          // (SPEC.md §11j)
    const int B = io.B, T = io.T, Bx = tracked ? 0 : io.xref_batch, H = h->H, m = h->m, NX = SDEMPC_NX;
    const int S = timed ? (timed->S < T ? timed->S : T) : 1;               // (a period longer than the run is one period of T ticks)
    const int Ns = loop_solves(T, S);
    const bool seen = obs && timed;
    const int AM = seen ? obs->age_max : 0;                                 // rows of the history (SPEC.md §11g)
    const bool scoring = score && timed && plant, score_sub = scoring && score->cfg->substeps == 1;
    const bool faulty = flt && flt->fault, subs_out = flt && flt->xsub, subs = subs_out || AM > 0 || score_sub;      // (the history is fed from the chunk's substep rows, and so is a substep score)
    const int nsub = plant ? plant->Q.substeps : 1;
    const size_t XR = (size_t)(H + 1) * NX, OUT = (size_t)S * (NX + m + (rate ? 4 : 0) + (subs ? (size_t)nsub * NX : 0)) + 8 + (seen ? NX : 0);       // floats per reference window / per episode-period of output
    const bool xref_moves = !tracked && io.xref_ticks > 1;
    const bool gust = scen && scen->dist, sched = scen && plant && plant->Q.models;        // (one shared plant: nothing to schedule)
    const bool dist_moves = gust && scen->Td > 1, sched_moves = sched && scen->Tp > 1;
    const size_t DR = gust ? (size_t)scen->Bd * SDEMPC_NNOISE : 0, SR = sched ? (size_t)B : 0;       // floats per tick row of the disturbance / words of the schedule
    const bool fault_moves = faulty && flt->Tf > 1;
    const size_t FR = faulty ? (size_t)flt->Bf * m * 2 : 0;                                          // floats per tick row of the fault schedule
    const bool noisy = seen && obs->sigma, biased = seen && obs->beta, gated = seen && obs->valid;
    const bool obs_moves = (noisy || biased) && obs->To > 1, valid_moves = gated && obs->Tv > 1;
    const size_t OR = noisy || biased ? (size_t)obs->Bo * 12 : 0, VR = gated ? (size_t)obs->Bv : 0;   // floats per solve row of sigma / of beta; words per solve row of valid
    const size_t ORS = (noisy ? OR : 0) + (biased ? OR : 0);
    const bool old = seen && obs->age, age_moves = old && obs->Ta > 1;
    const size_t AR = old ? (size_t)obs->Ba : 0;                                                       // words per solve row of age
    const bool targets = tracked && scoring && track->score_targets;                                   // (the target rows are formed on the device, one per tick and episode)
    const bool sref_moves = scoring && (targets || score->cfg->ref_ticks > 1);
    const size_t ZR = scoring ? (size_t)(targets ? B : score->cfg->ref_batch) * NX : 0;                                // floats per tick row of the score targets (SPEC.md §11h)
    const bool gproc = proc && proc->dist && scen && timed && plant, bproc = proc && proc->bias && seen;      // (SPEC.md §11i)
    const int NG = SDEMPC_NNOISE, NB = 12;                                                              // widths of the two processes
    const bool fproc = evt && evt->fault && flt && scen && timed && plant, dproc = evt && evt->drop && seen;   // (SPEC.md §11k)
    const int KF = fproc ? evt->fault->n_modes : 0;
    const size_t EF = (size_t)B * m * 2;                                                                // floats per tick row of the drawn fault rows
    const size_t per_period = (fproc ? (size_t)S * EF : 0) + (dproc ? (size_t)B : 0) + (gproc ? (size_t)S * B * NG : 0) + (bproc ? (size_t)B * NB : 0) + (size_t)B * OUT + (xref_moves ? (size_t)Bx * XR : 0) + (dist_moves ? (size_t)S * DR : 0) + (sched_moves ? (size_t)S * SR : 0) +
                              (fault_moves ? (size_t)S * FR : 0) + (obs_moves ? ORS : 0) + (valid_moves ? VR : 0) + (age_moves ? AR : 0) + (sref_moves ? (size_t)S * ZR : 0);
    const size_t fixed = (xref_moves ? 0 : (size_t)Bx * XR) + (dist_moves ? 0 : DR) + (sched_moves ? 0 : SR) + (fault_moves ? 0 : FR) + (obs_moves ? 0 : ORS) + (valid_moves ? 0 : VR) + (age_moves ? 0 : AR) + (sref_moves ? 0 : ZR);
    const size_t cap = (h->loop_chunk_bytes < 0 ? LOOP_CHUNK_BYTES : (size_t)h->loop_chunk_bytes) / sizeof(float);
    const size_t fit = cap > fixed ? (cap - fixed) / per_period : 0;
    const int Pc = (int)(fit < 1 ? 1 : (fit < (size_t)Ns ? fit : (size_t)Ns));      // periods per chunk
    const size_t Tc = (size_t)Pc * S;                                               // tick rows per chunk
    const size_t chunk_floats = (size_t)Pc * per_period + fixed;
    int rc;
    if (!h->d_loop.p && (rc = dev_alloc(h, h->d_loop, sizeof(uint32_t) * (size_t)h->max_batch * (10 + SDEMPC_MAX_MOTORS) + 16, true))) return rc;
    if (h->d_loop_chunk.bytes < sizeof(float) * chunk_floats) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        dev_free(h->d_loop_chunk);
        if ((rc = dev_alloc(h, h->d_loop_chunk, sizeof(float) * chunk_floats, true))) return rc;
    }
    if (rate && !h->d_rate.p && (rc = dev_alloc(h, h->d_rate, sizeof(float) * (size_t)h->max_batch * 3 * (1 + H), true))) return rc;
    if (seen && !h->d_obs.p && (rc = dev_alloc(h, h->d_obs, (sizeof(uint32_t) * 2 + sizeof(float) * NX) * (size_t)h->max_batch, true))) return rc;
    const size_t HR = (size_t)B * NX;                                // floats per history row
    if (AM > 0 && h->d_hist.bytes < sizeof(float) * (size_t)AM * h->max_batch * NX) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        dev_free(h->d_hist);
        if ((rc = dev_alloc(h, h->d_hist, sizeof(float) * (size_t)AM * h->max_batch * NX, true))) return rc;
    }
    float* d_hist = AM > 0 ? (float*)h->d_hist.p : nullptr;          // [AM][B][13] (SPEC.md §11g)
    if (scoring && !h->d_score.p && (rc = dev_alloc(h, h->d_score, sizeof(uint32_t) * 16 * (size_t)h->max_batch, true))) return rc;
    uint32_t* d_score = scoring ? (uint32_t*)h->d_score.p : nullptr; // [B][16] (SPEC.md §11h)
    if ((gproc || bproc) && !h->d_proc.p && (rc = dev_alloc(h, h->d_proc, sizeof(uint32_t) * PROC_WORDS * (size_t)h->max_batch, true))) return rc;
    const size_t MB = (size_t)h->max_batch;
    uint32_t* p_dchain = (uint32_t*)h->d_proc.p;                     // [B][2] (SPEC.md §11i; the layout is the one stated at d_proc)
    float* p_dstate = p_dchain ? (float*)(p_dchain + 2 * MB) : nullptr;                  // [B][6]
    uint32_t* p_bchain = p_dchain ? (uint32_t*)(p_dstate + NG * MB) : nullptr;           // [B][2]
    float* p_bstate = p_dchain ? (float*)(p_bchain + 2 * MB) : nullptr;                  // [B][12]
    float* p_drho = p_dchain ? p_bstate + NB * MB : nullptr, *p_dscale = p_dchain ? p_drho + NG * MB : nullptr;
    float* p_brho = p_dchain ? p_dscale + NG * MB : nullptr, *p_bscale = p_dchain ? p_brho + NB * MB : nullptr;
    if ((fproc || dproc) && !h->d_evt.p && (rc = dev_alloc(h, h->d_evt, sizeof(uint32_t) * EVT_WORDS * (size_t)h->max_batch, true))) return rc;
    uint32_t* e_fep = (uint32_t*)h->d_evt.p;                         // [B][EVENT_EP_WORDS] (SPEC.md §11k; the layout is the one stated at d_evt, each part sized for max_batch rows)
    uint32_t* e_dchain = e_fep ? e_fep + EVENT_EP_WORDS * MB : nullptr;                  // [B][2]
    int32_t* e_dstate = e_fep ? (int32_t*)(e_dchain + 2 * MB) : nullptr;                 // [B][2]
    uint32_t* e_par = e_fep ? (uint32_t*)(e_dstate + 2 * MB) : nullptr;                  // [batch][EVENT_PAR_WORDS]
    uint32_t* e_drop = e_fep ? e_par + EVENT_PAR_WORDS * MB : nullptr, *e_recover = e_fep ? e_drop + MB : nullptr;     // [batch]
    // SPEC.md §11m: the ensemble words of a chunk are formed after its scoring launch, in slabs of rows no larger than ENS_SLAB_BYTES of partial words
    const bool ensemble = ens && scoring;
    const int EG = ensemble ? ens->cfg->n_cohorts : 0, EE = ensemble ? ens->cfg->n_edges : 0, EW = ENS_BASE_WORDS + 4 * EE, nblk = (B + 255) / 256;
    const size_t ens_rows_max = Tc * (score_sub ? (size_t)nsub : 1), ens_row_words = (size_t)(nblk + 1) * EG * EW;     // (per row: the combined words and nblk blocks of partial words)
    size_t ens_slab = ensemble ? ENS_SLAB_BYTES / (sizeof(uint32_t) * ens_row_words) : 0;
    ens_slab = ens_slab < 1 ? 1 : ens_slab;
    ens_slab = ens_slab > 65535 ? 65535 : ens_slab;                  // (the partial form's rows are the grid's y extent)
    ens_slab = ens_slab > ens_rows_max ? ens_rows_max : ens_slab;
    const size_t ens_head = MB + 4 * ENS_MAX_EDGES;                  // words in front of the slab: cohorts, edges
    if (ensemble && h->d_ens.bytes < sizeof(uint32_t) * (ens_head + ens_slab * ens_row_words)) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        dev_free(h->d_ens);
        if ((rc = dev_alloc(h, h->d_ens, sizeof(uint32_t) * (ens_head + ens_slab * ens_row_words), true))) return rc;
    }
    int32_t* n_cohort = ensemble ? (int32_t*)h->d_ens.p : nullptr;   // [B]
    float* n_edges = ensemble ? (float*)(n_cohort + MB) : nullptr;   // [4][E]
    uint32_t* n_out = ensemble ? (uint32_t*)(n_edges + 4 * ENS_MAX_EDGES) : nullptr;         // [slab][G][W]
    uint32_t* n_part = ensemble ? n_out + ens_slab * EG * EW : nullptr;                      // [slab][nblk][G][W]
    // SPEC.md §11n: the live flags, the list and the dense staging of the live set's solve (the layout is the one stated at d_retire, each part sized for max_batch rows)
    const bool retire = ret && scoring;
    const size_t HM = (size_t)H * m;
    auto up4 = [](size_t words) { return (words + 3) & ~(size_t)3; };
    const size_t nblk_max = (MB + 255) / 256;
    const size_t o_live = 0, o_rat = o_live + up4(MB), o_list = o_rat + up4(MB), o_cnt = o_list + up4(MB), o_blk = o_cnt + up4(MB), o_nl = o_blk + up4(nblk_max);
    const size_t o_sx = o_nl + 4, o_sxr = o_sx + up4(MB * NX), o_su = o_sxr + up4(MB * XR), o_sstep = o_su + up4(MB * HM), o_ssub = o_sstep + up4(MB);
    const size_t o_suo = o_ssub + up4(2 * MB), o_sxe = o_suo + up4(MB * HM), o_sinf = o_sxe + up4(MB * XR), retire_words = o_sinf + up4(MB * 8);
    if (retire && !h->d_retire.p && (rc = dev_alloc(h, h->d_retire, sizeof(uint32_t) * retire_words, true))) return rc;
    uint32_t* y_base = retire ? (uint32_t*)h->d_retire.p : nullptr;
    int32_t* y_live = retire ? (int32_t*)(y_base + o_live) : nullptr;       // [B]
    int32_t* y_nlive = retire ? (int32_t*)(y_base + o_nl) : nullptr;        // [1]
    uint32_t* d_q = (uint32_t*)h->d_obs.p;                           // q [B][2] (SPEC.md §11f)
    float* d_xm = d_q ? (float*)(d_q + 2 * (size_t)h->max_batch) : nullptr;   // xm [B][13]
    float* d_integ = (float*)h->d_rate.p;                            // g [B][3] (SPEC.md §11d)
    float* d_tail = d_integ ? d_integ + 3 * (size_t)h->max_batch : nullptr;   // wt [B][H][3]
    uint32_t* d_keys = (uint32_t*)h->d_loop.p;                      // r_k, advanced in place
    uint32_t* d_sub = d_keys + 2 * (size_t)h->max_batch;             // the solve's noise keys of the tick
    float* d_xi6 = (float*)(d_sub + 2 * (size_t)h->max_batch);       // plant noise of the tick (SPEC.md §11: six values per episode)
    unsigned* d_gave_up = (unsigned*)(d_xi6 + 6 * (size_t)h->max_batch);
    float* d_mot = (float*)(d_gave_up + 4);                          // motor state a [B][m] (SPEC.md §11b)
    float* d_xi = plant ? plant->xi : d_xi6;                         // (SPEC.md §11a: 6 * substeps values per episode, beside the staged plants)
    float* c_xs = (float*)h->d_loop_chunk.p;                         // [Tc][B][13]
    float* c_us = c_xs + Tc * B * NX;                                // [Tc][B][m]
    float* c_info = c_us + Tc * B * m;                               // [Pc][B][8]
    float* c_xref = c_info + (size_t)Pc * B * 8;                     // [Pc or 1][Bx][H+1][13]
    float* c_dist = c_xref + (xref_moves ? (size_t)Pc : 1) * Bx * XR;         // [Tc or 1][Bd][6] (SPEC.md §11c)
    int32_t* c_sched = (int32_t*)(c_dist + (dist_moves ? Tc : 1) * DR);       // [Tc or 1][B]
    float* c_ws = (float*)(c_sched + (sched_moves ? Tc : 1) * SR);            // [Tc][B][4] (SPEC.md §11d)
    float* c_fault = c_ws + (rate ? Tc * B * 4 : 0);                          // [Tc or 1][Bf][m][2] (SPEC.md §11e)
    float* c_xsub = c_fault + (fault_moves ? Tc : 1) * FR;                    // [Tc * nsub][B][13]
    float* c_xmeas = c_xsub + (subs ? Tc * nsub * B * NX : 0);                // [Pc][B][13] (SPEC.md §11f)
    float* c_sigma = c_xmeas + (seen ? (size_t)Pc * B * NX : 0);              // [Pc or 1][Bo][12]
    float* c_beta = c_sigma + (noisy ? (obs_moves ? (size_t)Pc : 1) * OR : 0);        // [Pc or 1][Bo][12]
    int32_t* c_valid = (int32_t*)(c_beta + (biased ? (obs_moves ? (size_t)Pc : 1) * OR : 0));    // [Pc or 1][Bv]
    int32_t* c_age = c_valid + (gated ? (valid_moves ? (size_t)Pc : 1) * VR : 0);                // [Pc or 1][Ba] (SPEC.md §11g)
    float* c_sref = (float*)(c_age + (old ? (age_moves ? (size_t)Pc : 1) * AR : 0));             // [Tc or 1][Br][13] (SPEC.md §11h)
    float* c_pdist = c_sref + (scoring ? (sref_moves ? Tc : 1) * ZR : 0);                        // [Tc][B][6] (SPEC.md §11i)
    float* c_pbeta = c_pdist + (gproc ? Tc * B * NG : 0);                                        // [Pc][B][12]
    float* c_efault = c_pbeta + (bproc ? (size_t)Pc * B * NB : 0);                               // [Tc][B][m][2] (SPEC.md §11k)
    int32_t* c_evalid = (int32_t*)(c_efault + (fproc ? Tc * EF : 0));                            // [Pc][B]
    float* d_x = (float*)h->d_x0.p;                                  // x_k: the solve's initial states, advanced in place (SPEC.md §11f: the plant's; the solve reads d_xm)
    hipStream_t st = h->stream;
    // inputs (host vectors live until the synchronisation at the end of the first chunk)
    std::vector<float> u0, s0, a0, hh;
    std::vector<uint32_t> z0;
    const float* u_in = io.u_init;
    const float* s_in = io.stepsize_in;
    if (!u_in) {               // sdempc_reset: uref tiled
        u0.resize((size_t)B * H * m);
        for (size_t e = 0; e < u0.size(); ++e) u0[e] = h->cfg.uref[e % m];
        u_in = u0.data();
    }
    if (!s_in) {
        s0.assign(B, h->cfg.ls_maxls > 0 ? h->cfg.ls_init_stepsize : h->cfg.stepsize);
        s_in = s0.data();
    }
    HIPCHK(h, hipMemcpyAsync(d_x, io.x0, sizeof(float) * B * NX, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(d_keys, io.keys, sizeof(uint32_t) * 2 * B, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_u.p, u_in, sizeof(float) * (size_t)B * H * m, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_step.p, s_in, sizeof(float) * B, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemsetAsync(d_gave_up, 0, sizeof(unsigned), st));
    if (timed) {               // the motor state starts as u_act_in, or as the first row of the warm start
        const float* a_in = timed->u_act_in;
        if (!a_in) {
            a0.resize((size_t)B * m);
            for (int b = 0; b < B; ++b) memcpy(&a0[(size_t)b * m], u_in + (size_t)b * H * m, sizeof(float) * m);
            a_in = a0.data();
        }
        HIPCHK(h, hipMemcpyAsync(d_mot, a_in, sizeof(float) * (size_t)B * m, hipMemcpyHostToDevice, st));
    }
    if (rate) {                // integrator and rate tail start as given, or at zero
        if (rate->integ_in) HIPCHK(h, hipMemcpyAsync(d_integ, rate->integ_in, sizeof(float) * (size_t)B * 3, hipMemcpyHostToDevice, st));
        else HIPCHK(h, hipMemsetAsync(d_integ, 0, sizeof(float) * (size_t)B * 3, st));
        if (rate->tail_in) HIPCHK(h, hipMemcpyAsync(d_tail, rate->tail_in, sizeof(float) * (size_t)B * H * 3, hipMemcpyHostToDevice, st));
        else HIPCHK(h, hipMemsetAsync(d_tail, 0, sizeof(float) * (size_t)B * H * 3, st));
    }
    if (seen) {                // the observation chain and the held measurement start as given (xmeas_in NULL: x0)
        HIPCHK(h, hipMemcpyAsync(d_q, obs->keys, sizeof(uint32_t) * 2 * B, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(d_xm, obs->xmeas_in ? obs->xmeas_in : io.x0, sizeof(float) * B * NX, hipMemcpyHostToDevice, st));
        if (noisy && !obs_moves) HIPCHK(h, hipMemcpyAsync(c_sigma, obs->sigma, sizeof(float) * OR, hipMemcpyHostToDevice, st));
        if (biased && !obs_moves) HIPCHK(h, hipMemcpyAsync(c_beta, obs->beta, sizeof(float) * OR, hipMemcpyHostToDevice, st));
        if (gated && !valid_moves) HIPCHK(h, hipMemcpyAsync(c_valid, obs->valid, sizeof(int32_t) * VR, hipMemcpyHostToDevice, st));
        if (old && !age_moves) HIPCHK(h, hipMemcpyAsync(c_age, obs->age, sizeof(int32_t) * AR, hipMemcpyHostToDevice, st));
    }
    if (AM > 0) {              // the history starts as given, row-major on the device (xhist_in NULL: the vehicle sat at x0)
        hh.resize((size_t)AM * HR);
        for (int i = 0; i < AM; ++i)
            for (int b = 0; b < B; ++b)
                memcpy(&hh[(size_t)i * HR + (size_t)b * NX], obs->xhist_in ? obs->xhist_in + ((size_t)b * AM + i) * NX : io.x0 + (size_t)b * NX, sizeof(float) * NX);
        HIPCHK(h, hipMemcpyAsync(d_hist, hh.data(), sizeof(float) * hh.size(), hipMemcpyHostToDevice, st));
    }
    if (scoring) {             // the score words start as given, or as the initial row (SPEC.md §11h: counts 0, min c = +inf, first failing row all ones)
        const uint32_t* z_in = score->score_in;
        if (!z_in) {
            const float pinf = INFINITY;
            uint32_t row0[16] = {0};
            memcpy(&row0[6], &pinf, sizeof pinf);
            row0[8] = 0xffffffffu;
            z0.resize((size_t)B * 16);
            for (int b = 0; b < B; ++b) memcpy(&z0[(size_t)b * 16], row0, sizeof row0);
            z_in = z0.data();
        }
        HIPCHK(h, hipMemcpyAsync(d_score, z_in, sizeof(uint32_t) * 16 * (size_t)B, hipMemcpyHostToDevice, st));
        if (!sref_moves) HIPCHK(h, hipMemcpyAsync(c_sref, score->cfg->score_ref, sizeof(float) * ZR, hipMemcpyHostToDevice, st));      // (targets: they move)
    }
    std::vector<float> xe0;
    if (retire) {              // SPEC.md §11n: the tables a retired episode flies are defined by the call — the warm start, and x0 in every row of xevol
        xe0.resize((size_t)B * XR);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t <= H; ++t) memcpy(&xe0[(size_t)b * XR + (size_t)t * NX], io.x0 + (size_t)b * NX, sizeof(float) * NX);
        HIPCHK(h, hipMemcpyAsync(h->d_uopt.p, u_in, sizeof(float) * (size_t)B * HM, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(h->d_xmean.p, xe0.data(), sizeof(float) * xe0.size(), hipMemcpyHostToDevice, st));
    }
    if (ensemble) {            // the cohorts (NULL: all 0) and the edges as given (SPEC.md §11m)
        if (ens->cfg->cohort) HIPCHK(h, hipMemcpyAsync(n_cohort, ens->cfg->cohort, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, st));
        else HIPCHK(h, hipMemsetAsync(n_cohort, 0, sizeof(int32_t) * (size_t)B, st));
        if (EE > 0) HIPCHK(h, hipMemcpyAsync(n_edges, ens->cfg->edges, sizeof(float) * 4 * (size_t)EE, hipMemcpyHostToDevice, st));
    }
    for (int w = 0; w < 2; ++w) {      // the process chains, states (NULL: zeros) and coefficients start as given (SPEC.md §11i)
        if (!(w ? bproc : gproc)) continue;
        const sdempc_process_cfg& pc = w ? *proc->bias : *proc->dist;
        const size_t W = w ? NB : NG;
        float* state = w ? p_bstate : p_dstate;
        HIPCHK(h, hipMemcpyAsync(w ? p_bchain : p_dchain, pc.keys, sizeof(uint32_t) * 2 * B, hipMemcpyHostToDevice, st));
        if (pc.state_in) HIPCHK(h, hipMemcpyAsync(state, pc.state_in, sizeof(float) * B * W, hipMemcpyHostToDevice, st));
        else HIPCHK(h, hipMemsetAsync(state, 0, sizeof(float) * B * W, st));
        HIPCHK(h, hipMemcpyAsync(w ? p_brho : p_drho, pc.rho, sizeof(float) * pc.batch * W, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(w ? p_bscale : p_dscale, pc.scale, sizeof(float) * pc.batch * W, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> e0, e1;
    if (fproc) {               // the fault chain's rows (key, then (s, first) per motor; state_in NULL: (0, -1)) and the parameter rows start as given (SPEC.md §11k)
        const sdempc_fault_process_cfg& pc = *evt->fault;
        e0.assign((size_t)B * EVENT_EP_WORDS, 0u);
        for (int b = 0; b < B; ++b) {
            uint32_t* row = &e0[(size_t)b * EVENT_EP_WORDS];
            row[0] = pc.keys[2 * b]; row[1] = pc.keys[2 * b + 1];
            for (int l = 0; l < m; ++l) {
                row[2 + 2 * l] = pc.state_in ? (uint32_t)pc.state_in[((size_t)b * m + l) * 2] : 0u;
                row[3 + 2 * l] = pc.state_in ? (uint32_t)pc.state_in[((size_t)b * m + l) * 2 + 1] : 0xffffffffu;
            }
        }
        e1.assign((size_t)pc.batch * EVENT_PAR_WORDS, 0u);
        for (int r = 0; r < pc.batch; ++r)
            for (int l = 0; l < m; ++l)
                for (int j = 0; j < KF; ++j) {
                    uint32_t* row = &e1[(size_t)r * EVENT_PAR_WORDS];
                    const size_t e = ((size_t)r * m + l) * KF + j;
                    row[l * 4 + j] = pc.onset[e];
                    row[32 + l * 4 + j] = pc.clear[e];
                    memcpy(&row[64 + (l * 4 + j) * 2], pc.modes + 2 * e, 2 * sizeof(float));
                }
        HIPCHK(h, hipMemcpyAsync(e_fep, e0.data(), sizeof(uint32_t) * e0.size(), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(e_par, e1.data(), sizeof(uint32_t) * e1.size(), hipMemcpyHostToDevice, st));
    }
    if (dproc) {
        const sdempc_dropout_process_cfg& pc = *evt->drop;
        HIPCHK(h, hipMemcpyAsync(e_dchain, pc.keys, sizeof(uint32_t) * 2 * B, hipMemcpyHostToDevice, st));
        if (pc.state_in) HIPCHK(h, hipMemcpyAsync(e_dstate, pc.state_in, sizeof(int32_t) * 2 * B, hipMemcpyHostToDevice, st));
        else HIPCHK(h, hipMemsetAsync(e_dstate, 0, sizeof(int32_t) * 2 * B, st));
        HIPCHK(h, hipMemcpyAsync(e_drop, pc.drop, sizeof(uint32_t) * pc.batch, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(e_recover, pc.recover, sizeof(uint32_t) * pc.batch, hipMemcpyHostToDevice, st));
    }
    if (!tracked && !xref_moves) {
        HIPCHK(h, hipMemcpyAsync(c_xref, io.xref, sizeof(float) * Bx * XR, hipMemcpyHostToDevice, st));
        if (Bx != B) HIPCHK(h, launch_broadcast_rows(c_xref, (float*)h->d_xref.p, (int)XR, B, st));
    }
    std::vector<int32_t> ident;
    if (gust && !dist_moves) HIPCHK(h, hipMemcpyAsync(c_dist, scen->dist, sizeof(float) * DR, hipMemcpyHostToDevice, st));
    if (faulty && !fault_moves) HIPCHK(h, hipMemcpyAsync(c_fault, flt->fault, sizeof(float) * FR, hipMemcpyHostToDevice, st));
    if (sched && !sched_moves) {
        const int32_t* row = scen->plant_of;
        if (!row) {                // (no plant_of: num_plants == B, the identity)
            ident.resize(B);
            for (int b = 0; b < B; ++b) ident[b] = b;
            row = ident.data();
        }
        HIPCHK(h, hipMemcpyAsync(c_sched, row, sizeof(int32_t) * SR, hipMemcpyHostToDevice, st));
    }
    if (io.xs)
        for (int b = 0; b < B; ++b) memcpy(io.xs + (size_t)b * (T + 1) * NX, io.x0 + (size_t)b * NX, sizeof(float) * NX);
    // the plant launch's arguments: built once, only pointers and `ticks` move from period to period
    LoopAdvance L;
    L.uopt = (const float*)h->d_uopt.p; L.xi = d_xi;
    L.x = d_x; L.u = (float*)h->d_u.p; L.step = (float*)h->d_step.p; L.gave_up = d_gave_up;
    L.B = B; L.H = H;
    LoopPeriod R{};
    LoopScenario C{};
    LoopRate W{};
    LoopFault V{};
    LoopObserve O{};           // (q null: absent)
    LoopScore Z{};             // (words null: absent; the period launches never take it)
    if (scoring) {
        const sdempc_score_cfg& zc = *score->cfg;
        Z.words = d_score; Z.rows = score_sub ? c_xsub : c_xs; Z.us = c_us; Z.info = c_info; Z.ref = c_sref;
        Z.ref_tick_stride = sref_moves ? (int)ZR : 0; Z.ref_ep_stride = targets || zc.ref_batch > 1 ? NX : 0;
        Z.rows_per_tick = score_sub ? nsub : 1; Z.m = m;
        Z.r2_pos = zc.r2_pos; Z.cos_min = zc.cos_min; Z.w2_max = zc.w2_max;
        for (int l = 0; l < 8; ++l) { Z.u_lo[l] = l < m ? h->cfg.u_lo[l] : 0.0f; Z.u_hi[l] = l < m ? h->cfg.u_hi[l] : 0.0f; Z.uref[l] = l < m ? h->cfg.uref[l] : 0.0f; }
    }
    LoopEnsemble N{};          // (part null: absent; only the launches after a chunk's scoring launch take it)
    if (ensemble) {            // rows, targets and thresholds are the scoring launch's own
        N.part = n_part; N.out = n_out; N.words = d_score; N.cohort = n_cohort; N.edges = n_edges;
        N.rows = Z.rows; N.ref = Z.ref; N.ref_tick_stride = Z.ref_tick_stride; N.ref_ep_stride = Z.ref_ep_stride; N.rows_per_tick = Z.rows_per_tick;
        N.nblk = nblk; N.G = EG; N.E = EE; N.over = ens->cfg->over;
        N.r2_pos = Z.r2_pos; N.cos_min = Z.cos_min; N.w2_max = Z.w2_max;
    }
    LoopRetire Y{};            // (live null: absent; only the launches after a period's scoring launch take it)
    LoopCompact Qg{}, Qs{};    // (list null: absent; the gather and the scatter around a dense solve)
    if (retire) {              // live_0 from the staged score words; the list and n_live of the first solve
        Y.live = y_live; Y.words = d_score; Y.retired_at = (int32_t*)(y_base + o_rat); Y.blk = y_base + o_blk; Y.list = (int32_t*)(y_base + o_list); Y.n_live = y_nlive;
        Y.count = ensemble ? y_base + o_cnt : nullptr; Y.nblk = nblk;
        N.count = Y.count;
        Y.init = 1; Y.solve = 0;
        HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, LoopBaseline{}, LoopEnsemble{}, Y));
        Y.init = 0; Y.place = 1;
        HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, LoopBaseline{}, LoopEnsemble{}, Y));
        Qg.list = Qs.list = Y.list; Qg.B = Qs.B = B; Qs.scatter = 1;
        Qg.nseg = 5;           // the solve's state, window, warm start, step size and subkey (the state and the window are set per period)
        Qg.seg[0].dst = y_base + o_sx; Qg.seg[0].words = NX;
        Qg.seg[1].dst = y_base + o_sxr; Qg.seg[1].words = (int)XR;
        Qg.seg[2].src = (const uint32_t*)h->d_u.p; Qg.seg[2].dst = y_base + o_su; Qg.seg[2].words = (int)HM;
        Qg.seg[3].src = (const uint32_t*)h->d_step.p; Qg.seg[3].dst = y_base + o_sstep; Qg.seg[3].words = 1;
        Qg.seg[4].src = d_sub; Qg.seg[4].dst = y_base + o_ssub; Qg.seg[4].words = 2;
        Qs.nseg = 3;           // the solve's tables and its info rows (set per period)
        Qs.seg[0].src = y_base + o_suo; Qs.seg[0].dst = (uint32_t*)h->d_uopt.p; Qs.seg[0].words = (int)HM;
        Qs.seg[1].src = y_base + o_sxe; Qs.seg[1].dst = (uint32_t*)h->d_xmean.p; Qs.seg[1].words = (int)XR;
        Qs.seg[2].src = y_base + o_sinf; Qs.seg[2].words = 8;
        Qs.live = y_live; Qs.held_step = (const float*)h->d_step.p; Qs.gave_up = d_gave_up;
    }
    LoopTrack K{};             // (t null: absent)
    if (tracked) K = track->K;
    LoopProcess G{};           // (chains null: absent)
    if (gproc) {
        G.dist.chain = p_dchain; G.dist.state = p_dstate; G.dist.rho = p_drho; G.dist.scale = p_dscale; G.dist.par_ep_stride = proc->dist->batch > 1 ? NG : 0;
        G.dist.sched_tick_stride = dist_moves ? (int)DR : 0; G.dist.sched_ep_stride = gust && scen->Bd > 1 ? NG : 0;
    }
    if (bproc) {
        G.bias.chain = p_bchain; G.bias.state = p_bstate; G.bias.rho = p_brho; G.bias.scale = p_bscale; G.bias.par_ep_stride = proc->bias->batch > 1 ? NB : 0;
        G.bias.sched_ep_stride = biased && obs->Bo > 1 ? NB : 0;
    }
    LoopBaseline A{};          // (x null: absent)
    if (flown) {
        if ((rc = stage_geo(h, *geo->cfg, st))) return rc;
        A.par = (const float*)h->d_geo.p; A.par_ep_stride = geo->cfg->batch > 1 ? GEO_PAR_WORDS : 0;
        A.accel_ff = geo->cfg->accel_ff; A.ref_row = geo->cfg->ref_row; A.inv_dt = geo->inv_dt; A.H = H; A.m = m;
        A.uopt = (float*)h->d_uopt.p; A.xevol = (float*)h->d_xmean.p; A.step = (const float*)h->d_step.p;
        h->last_coop_B = 0;    // (no solve of this run can leave a barrier word to read)
    }
    LoopEvents E{};            // (chains null: absent)
    if (fproc) {
        E.fault.chain = e_fep; E.fault.par = e_par; E.fault.par_ep_stride = evt->fault->batch > 1 ? EVENT_PAR_WORDS : 0; E.fault.K = KF; E.fault.m = m;
        E.fault.sched_tick_stride = fault_moves ? (int)FR : 0; E.fault.sched_ep_stride = faulty && flt->Bf > 1 ? 2 * m : 0;
    }
    if (dproc) {
        E.drop.chain = e_dchain; E.drop.state = e_dstate; E.drop.drop = e_drop; E.drop.recover = e_recover; E.drop.par_ep_stride = evt->drop->batch > 1 ? 1 : 0;
        E.drop.sched_ep_stride = gated && obs->Bv > 1 ? 1 : 0;
    }
    if (seen) {
        O.q = d_q; O.x = d_x; O.xm = d_xm; O.ep_stride = obs->Bo > 1 ? 12 : 0; O.valid_ep_stride = obs->Bv > 1 ? 1 : 0;
        O.renorm = obs->renorm ? 1 : 0;
        if (old && AM > 0) { O.hist = d_hist; O.hist_row_stride = (int)HR; O.age_ep_stride = obs->Ba > 1 ? 1 : 0; O.age_max = AM; }      // (age_max 0: every age is 0)
    }
    if (flt) { V.fault_tick_stride = fault_moves ? (int)FR : 0; V.fault_ep_stride = faulty && flt->Bf > 1 ? 2 * m : 0; }
    if (fproc) { V.fault_tick_stride = (int)EF; V.fault_ep_stride = 2 * m; }       // (the plant reads the rows the key schedule wrote)
    if (timed) { R.act = d_mot; R.alpha = timed->alpha; R.xi_ticks = S; R.shift = timed->S < H ? timed->S : H; }
    if (scen) {
        C.dist_tick_stride = dist_moves ? (int)DR : 0; C.dist_ep_stride = gust && scen->Bd > 1 ? SDEMPC_NNOISE : 0;
        if (gproc) { C.dist_tick_stride = B * NG; C.dist_ep_stride = NG; }       // (the plant reads the rows the key schedule wrote)
        C.plant_tick_stride = sched_moves ? B : 0;
        C.dtp = plant->dt;
    }
    if (rate) {
        const sdempc_rate_cfg& rc_ = *rate->cfg;
        for (int a = 0; a < 3; ++a) { W.kp[a] = rc_.kp[a]; W.ki_dt[a] = rc_.ki_dt[a]; W.glim[a] = rc_.integ_limit[a]; }
        for (int l = 0; l < 8; ++l) {
            for (int a = 0; a < 3; ++a) W.M[l][a] = l < m ? rc_.mixer[l][a] : 0.0f;
            W.lo[l] = l < m ? h->cfg.u_lo[l] : 0.0f; W.hi[l] = l < m ? h->cfg.u_hi[l] : 0.0f;
        }
        W.inv_m = rate->inv_m; W.w = rc_.motor_weight;
        W.xevol = (const float*)h->d_xmean.p; W.wt = d_tail; W.g = d_integ;
    }
    std::vector<float> hx, hu, hi, hw, hs, hm, hn, hg, hb, hf;
    std::vector<int32_t> hv;
    std::vector<uint32_t> he;
    for (int j0 = 0; j0 < Ns; j0 += Pc) {
        const int np = Ns - j0 < Pc ? Ns - j0 : Pc;                                  // periods of this chunk
        const size_t k0 = (size_t)j0 * S;
        const int nk = (int)((size_t)T - k0 < (size_t)np * S ? (size_t)T - k0 : (size_t)np * S);      // ticks of this chunk
        if (xref_moves) HIPCHK(h, hipMemcpyAsync(c_xref, io.xref + (size_t)j0 * Bx * XR, sizeof(float) * np * Bx * XR, hipMemcpyHostToDevice, st));
        if (dist_moves) HIPCHK(h, hipMemcpyAsync(c_dist, scen->dist + k0 * DR, sizeof(float) * nk * DR, hipMemcpyHostToDevice, st));
        if (sched_moves) HIPCHK(h, hipMemcpyAsync(c_sched, scen->plant_of + k0 * SR, sizeof(int32_t) * nk * SR, hipMemcpyHostToDevice, st));
        if (fault_moves) HIPCHK(h, hipMemcpyAsync(c_fault, flt->fault + k0 * FR, sizeof(float) * nk * FR, hipMemcpyHostToDevice, st));
        if (obs_moves && noisy) HIPCHK(h, hipMemcpyAsync(c_sigma, obs->sigma + (size_t)j0 * OR, sizeof(float) * np * OR, hipMemcpyHostToDevice, st));
        if (obs_moves && biased) HIPCHK(h, hipMemcpyAsync(c_beta, obs->beta + (size_t)j0 * OR, sizeof(float) * np * OR, hipMemcpyHostToDevice, st));
        if (valid_moves) HIPCHK(h, hipMemcpyAsync(c_valid, obs->valid + (size_t)j0 * VR, sizeof(int32_t) * np * VR, hipMemcpyHostToDevice, st));
        if (age_moves) HIPCHK(h, hipMemcpyAsync(c_age, obs->age + (size_t)j0 * AR, sizeof(int32_t) * np * AR, hipMemcpyHostToDevice, st));
        if (sref_moves && !targets) HIPCHK(h, hipMemcpyAsync(c_sref, score->cfg->score_ref + k0 * ZR, sizeof(float) * nk * ZR, hipMemcpyHostToDevice, st));
        for (int jc = 0; jc < np; ++jc) {
            const int ticks = nk - jc * S < S ? nk - jc * S : S;                    // (the last period of the run may be partial)
            if (seen) {
                O.xmeas = c_xmeas + (size_t)jc * B * NX;
                O.sigma = noisy ? c_sigma + (obs_moves ? (size_t)jc * OR : 0) : nullptr;
                O.beta = biased ? c_beta + (obs_moves ? (size_t)jc * OR : 0) : nullptr;
                O.valid = gated ? c_valid + (valid_moves ? (size_t)jc * VR : 0) : nullptr;
                if (O.hist) O.age = c_age + (age_moves ? (size_t)jc * AR : 0);
            }
            if (gproc) {               // (the scheduled rows and the written rows of this period's first tick)
                G.dist.sched = gust ? c_dist + (dist_moves ? (size_t)jc * S * DR : 0) : nullptr;
                G.dist.dst = c_pdist + (size_t)jc * S * B * NG;
            }
            if (bproc) {               // (the scheduled beta goes through the process, which writes the row the measurement reads)
                G.bias.sched = O.beta;
                G.bias.dst = c_pbeta + (size_t)jc * B * NB;
                O.beta = nullptr;
            }
            if (fproc) {               // (the scheduled rows and the written rows of this period's first tick, and its global tick)
                E.fault.sched = faulty ? (const uint32_t*)(c_fault + (fault_moves ? (size_t)jc * S * FR : 0)) : nullptr;
                E.fault.dst = (uint32_t*)(c_efault + (size_t)jc * S * EF);
                E.fault.tick0 = evt->fault->tick0 + (int)(k0 + (size_t)jc * S);
            }
            if (dproc) {               // (the scheduled flags go through the chain, which writes the flags the measurement reads)
                E.drop.sched = O.valid;
                E.drop.dst = c_evalid + (size_t)jc * B;
                O.valid = E.drop.dst; O.valid_ep_stride = 1;
            }
            if (timed) HIPCHK(h, launch_loop_keys_period(d_keys, d_sub, d_xi, B, ticks, S, plant->Q.substeps, st, O, LoopScore{}, G, E));
            else if (plant) HIPCHK(h, launch_loop_keys(d_keys, d_sub, d_xi, B, st, plant->Q.substeps));
            else HIPCHK(h, launch_loop_keys(d_keys, d_sub, d_xi, B, st));
            int n_live = B;
            if (retire) {              // SPEC.md §11n: four bytes and one synchronisation per period — the size of this period's solve
                HIPCHK(h, hipMemcpyAsync(&n_live, y_nlive, sizeof n_live, hipMemcpyDeviceToHost, st));
                HIPCHK(h, hipStreamSynchronize(st));
                if (n_live < 0 || n_live > B) return fail(h, SDEMPC_EDEVICE, "closed loop: the live count read back lies outside [0, B]%s");
                ret->live[j0 + jc] = n_live;
            }
            const bool dense = retire && !flown && n_live < B;         // (n_live == B: exactly the launches of a call without retire)
            if (!flown && !dense) HIPCHK(h, launch_noise_from_keys(d_sub, (float*)h->d_noise.p, B, h->P, h->G, H, st));      // (SPEC.md §11l: the split happened, its draw is not used)
            const float* win = c_xref + (xref_moves ? (size_t)jc * Bx * XR : 0);
            const float* xr = win;
            if (tracked) {             // the windows of this solve's tick, cut where the solve reads them
                K.tick0 = track->K.tick0 + (int)(k0 + (size_t)jc * S); K.B = B; K.rows = H + 1; K.groups = 1;
                HIPCHK(h, launch_broadcast_rows(nullptr, (float*)h->d_xref.p, 0, 0, st, K));
                xr = (const float*)h->d_xref.p;
            } else if (Bx != B) {
                if (xref_moves) HIPCHK(h, launch_broadcast_rows(win, (float*)h->d_xref.p, (int)XR, B, st));
                xr = (const float*)h->d_xref.p;
            }
            float* info_j = c_info + (size_t)jc * B * 8;
            if (flown) {               // the controller's tables where the solve would have left its own, from the B windows the solve would have read
                A.x = seen ? d_xm : d_x; A.info = info_j;
                A.xref = xr; A.xref_ep_stride = (int)XR;
                A.live = retire ? y_live : nullptr;
                HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, A));
            } else if (dense) {        // SPEC.md §11n: the live set alone, in a dense batch — gather, noise from the dense subkeys, solve on the staging, scatter
                h->last_coop_B = 0;
                if (n_live > 0) {
                    Qg.n = n_live;
                    Qg.seg[0].src = (const uint32_t*)(seen ? d_xm : d_x); Qg.seg[1].src = (const uint32_t*)xr;
                    HIPCHK(h, launch_broadcast_rows(nullptr, nullptr, 0, 0, st, LoopTrack{}, Qg));
                    HIPCHK(h, launch_noise_from_keys(y_base + o_ssub, (float*)h->d_noise.p, n_live, h->P, h->G, H, st));
                    if ((rc = sdempc_solve_batch_dev(h, n_live, y_base + o_sx, y_base + o_sxr, h->d_noise.p, y_base + o_su, y_base + o_sstep, y_base + o_suo, y_base + o_sxe,
                                                     y_base + o_sinf, st))) return rc;
                }
                Qs.n = n_live; Qs.seg[2].dst = (uint32_t*)info_j; Qs.held_info = info_j;
                Qs.coop_bar = h->last_coop_B > 0 ? (const unsigned*)h->d_coop_bar.p : nullptr;      // (indexed by dense position: folded into the sticky flag here)
                HIPCHK(h, launch_broadcast_rows(nullptr, nullptr, 0, 0, st, LoopTrack{}, Qs));
            } else if ((rc = sdempc_solve_batch_dev(h, B, seen ? d_xm : d_x, xr, h->d_noise.p, h->d_u.p, h->d_step.p, h->d_uopt.p, h->d_xmean.p, info_j, st))) return rc;
            L.info = info_j; L.coop_bar = !dense && h->last_coop_B > 0 ? (const unsigned*)h->d_coop_bar.p : nullptr;
            L.xs = c_xs + (size_t)jc * S * B * NX; L.us = c_us + (size_t)jc * S * B * m;
            if (timed) {
                const size_t t0 = (size_t)jc * S;                                    // first tick row of this period inside the chunk
                const long long never = (long long)ticks * plant->Q.substeps;       // (a solution that arrives at the period's end is flown by the next period, as its tail)
                R.ticks = ticks; R.arrive = (int)(timed->D < never ? timed->D : never);
                if (scen) {
                    C.dist = gproc ? c_pdist + t0 * B * NG : gust ? c_dist + (dist_moves ? t0 * DR : 0) : nullptr;
                    C.plant = sched ? c_sched + (sched_moves ? t0 * SR : 0) : nullptr;
                }
                if (rate) W.ws = c_ws + t0 * B * 4;
                if (flt || subs) {
                    V.fault = fproc ? c_efault + t0 * EF : faulty ? c_fault + (fault_moves ? t0 * FR : 0) : nullptr;
                    V.xsub = subs ? c_xsub + t0 * nsub * B * NX : nullptr;
                }
            }
            // SPEC.md §11g: with d = ticks * nsub substeps in this period, row i of the history after it is z_{c + d - AM + i}: an old row i + d (a partial last
            // period: moved down in blocks no longer than the shift, in ascending order), the plant state before the launch (i = AM - d), or substep row d - AM + i - 1
            const int d = ticks * nsub;
            if (AM > 0 && d <= AM) {
                for (int i = 0; i < AM - d; i += d) {
                    const int len = AM - d - i < d ? AM - d - i : d;
                    HIPCHK(h, hipMemcpyAsync(d_hist + (size_t)i * HR, d_hist + (size_t)(i + d) * HR, sizeof(float) * len * HR, hipMemcpyDeviceToDevice, st));
                }
                HIPCHK(h, hipMemcpyAsync(d_hist + (size_t)(AM - d) * HR, d_x, sizeof(float) * HR, hipMemcpyDeviceToDevice, st));
            }
            HIPCHK(h, launch_loop(plant ? plant->k : h->base, L, plant ? &plant->Q : nullptr, timed ? &R : nullptr, scen ? &C : nullptr, rate ? &W : nullptr, st,
                                  (flt || subs) && timed && scen ? &V : nullptr));
            if (AM > 0) {
                const int i0 = AM - d + 1 > 0 ? AM - d + 1 : 0;
                if (i0 < AM) HIPCHK(h, hipMemcpyAsync(d_hist + (size_t)i0 * HR, V.xsub + (size_t)(d - AM + i0 - 1) * HR, sizeof(float) * (AM - i0) * HR, hipMemcpyDeviceToDevice, st));
            }
            if (retire) {              // SPEC.md §11n: this period's rows into the words of the live episodes, then the live set of the next solve
                const size_t t0 = (size_t)jc * S;
                if (targets) {
                    K.tick0 = track->K.tick0 + (int)(k0 + t0) + 1; K.B = B; K.rows = 1; K.groups = ticks;
                    HIPCHK(h, launch_broadcast_rows(nullptr, c_sref + t0 * ZR, 0, 0, st, K));
                }
                LoopScore Zp = Z;
                Zp.rows = Z.rows + t0 * Z.rows_per_tick * B * NX; Zp.us = c_us + t0 * B * m; Zp.info = info_j; Zp.ref = c_sref + (sref_moves ? t0 * ZR : 0);
                Zp.ticks = ticks; Zp.solves = 1; Zp.live = y_live;
                HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, Zp));
                Y.solve = j0 + jc + 1 < Ns ? j0 + jc + 1 : -1; Y.rows = ticks * Z.rows_per_tick;
                Y.place = 0;
                HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, LoopBaseline{}, LoopEnsemble{}, Y));
                Y.place = 1;
                HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, LoopBaseline{}, LoopEnsemble{}, Y));
            }
        }
        if (scoring && !retire) {  // SPEC.md §11h: the chunk's rows into the score words, one thread per episode
            Z.ticks = nk; Z.solves = np;
            if (targets) {         // SPEC.md §11j: the target of chunk tick i is the row at theta(k0 + i + 1)
                K.tick0 = track->K.tick0 + (int)k0 + 1; K.B = B; K.rows = 1; K.groups = nk;
                HIPCHK(h, launch_broadcast_rows(nullptr, c_sref, 0, 0, st, K));
            }
            HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, Z));
        }
        if (ensemble) {            // SPEC.md §11m: the chunk's rows over the episodes, slab by slab — partial words per block, then the blocks in ascending order
            N.chunk_rows = nk * Z.rows_per_tick;
            for (int r0 = 0; r0 < N.chunk_rows; r0 += (int)ens_slab) {
                N.row0 = r0; N.nrows = N.chunk_rows - r0 < (int)ens_slab ? N.chunk_rows - r0 : (int)ens_slab;
                N.combine = 0;
                HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, LoopBaseline{}, N));
                N.combine = 1;
                HIPCHK(h, launch_loop_keys_period(nullptr, nullptr, nullptr, B, 0, 0, nsub, st, LoopObserve{}, LoopScore{}, LoopProcess{}, LoopEvents{}, LoopBaseline{}, N));
                HIPCHK(h, hipMemcpyAsync(ens->out + (k0 * Z.rows_per_tick + (size_t)r0) * EG * EW, n_out, sizeof(uint32_t) * (size_t)N.nrows * EG * EW, hipMemcpyDeviceToHost, st));
            }
        }
        unsigned gave_up = 0;
        if (io.xs) {
            hx.resize((size_t)nk * B * NX);
            HIPCHK(h, hipMemcpyAsync(hx.data(), c_xs, sizeof(float) * hx.size(), hipMemcpyDeviceToHost, st));
        }
        if (io.us) {
            hu.resize((size_t)nk * B * m);
            HIPCHK(h, hipMemcpyAsync(hu.data(), c_us, sizeof(float) * hu.size(), hipMemcpyDeviceToHost, st));
        }
        if (io.info) {
            hi.resize((size_t)np * B * 8);
            HIPCHK(h, hipMemcpyAsync(hi.data(), c_info, sizeof(float) * hi.size(), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(h, hipMemcpyAsync(&gave_up, d_gave_up, sizeof gave_up, hipMemcpyDeviceToHost, st));
        if (rate && rate->ws) {
            hw.resize((size_t)nk * B * 4);
            HIPCHK(h, hipMemcpyAsync(hw.data(), c_ws, sizeof(float) * hw.size(), hipMemcpyDeviceToHost, st));
        }
        if (subs_out) {
            hs.resize((size_t)nk * nsub * B * NX);
            HIPCHK(h, hipMemcpyAsync(hs.data(), c_xsub, sizeof(float) * hs.size(), hipMemcpyDeviceToHost, st));
        }
        if (seen && obs->xmeas) {
            hm.resize((size_t)np * B * NX);
            HIPCHK(h, hipMemcpyAsync(hm.data(), c_xmeas, sizeof(float) * hm.size(), hipMemcpyDeviceToHost, st));
        }
        if (gproc && proc->dist_rows) {
            hg.resize((size_t)nk * B * NG);
            HIPCHK(h, hipMemcpyAsync(hg.data(), c_pdist, sizeof(float) * hg.size(), hipMemcpyDeviceToHost, st));
        }
        if (bproc && proc->bias_rows) {
            hb.resize((size_t)np * B * NB);
            HIPCHK(h, hipMemcpyAsync(hb.data(), c_pbeta, sizeof(float) * hb.size(), hipMemcpyDeviceToHost, st));
        }
        if (fproc && evt->fault_rows) {
            hf.resize((size_t)nk * EF);
            HIPCHK(h, hipMemcpyAsync(hf.data(), c_efault, sizeof(float) * hf.size(), hipMemcpyDeviceToHost, st));
        }
        if (dproc && evt->valid_rows) {
            hv.resize((size_t)np * B);
            HIPCHK(h, hipMemcpyAsync(hv.data(), c_evalid, sizeof(int32_t) * hv.size(), hipMemcpyDeviceToHost, st));
        }
        if (j0 + np == Ns) {
            if (fproc && (evt->fault_keys_next || evt->fault_state_next)) {
                he.resize((size_t)B * EVENT_EP_WORDS);
                HIPCHK(h, hipMemcpyAsync(he.data(), e_fep, sizeof(uint32_t) * he.size(), hipMemcpyDeviceToHost, st));
            }
            if (dproc && evt->valid_keys_next) HIPCHK(h, hipMemcpyAsync(evt->valid_keys_next, e_dchain, sizeof(uint32_t) * 2 * B, hipMemcpyDeviceToHost, st));
            if (dproc && evt->valid_state_next) HIPCHK(h, hipMemcpyAsync(evt->valid_state_next, e_dstate, sizeof(int32_t) * 2 * B, hipMemcpyDeviceToHost, st));
            if (gproc && proc->dist_keys_next) HIPCHK(h, hipMemcpyAsync(proc->dist_keys_next, p_dchain, sizeof(uint32_t) * 2 * B, hipMemcpyDeviceToHost, st));
            if (gproc && proc->dist_state_next) HIPCHK(h, hipMemcpyAsync(proc->dist_state_next, p_dstate, sizeof(float) * B * NG, hipMemcpyDeviceToHost, st));
            if (bproc && proc->bias_keys_next) HIPCHK(h, hipMemcpyAsync(proc->bias_keys_next, p_bchain, sizeof(uint32_t) * 2 * B, hipMemcpyDeviceToHost, st));
            if (bproc && proc->bias_state_next) HIPCHK(h, hipMemcpyAsync(proc->bias_state_next, p_bstate, sizeof(float) * B * NB, hipMemcpyDeviceToHost, st));
            if (retire) HIPCHK(h, hipMemcpyAsync(ret->retired_at, Y.retired_at, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
            if (scoring) HIPCHK(h, hipMemcpyAsync(score->score_out, d_score, sizeof(uint32_t) * 16 * (size_t)B, hipMemcpyDeviceToHost, st));
            if (AM > 0 && obs->xhist_next) {
                hn.resize((size_t)AM * HR);
                HIPCHK(h, hipMemcpyAsync(hn.data(), d_hist, sizeof(float) * hn.size(), hipMemcpyDeviceToHost, st));
            }
            if (seen && obs->keys_next) HIPCHK(h, hipMemcpyAsync(obs->keys_next, d_q, sizeof(uint32_t) * 2 * B, hipMemcpyDeviceToHost, st));
            if (seen && obs->xmeas_next) HIPCHK(h, hipMemcpyAsync(obs->xmeas_next, d_xm, sizeof(float) * B * NX, hipMemcpyDeviceToHost, st));
            if (rate && rate->integ_next) HIPCHK(h, hipMemcpyAsync(rate->integ_next, d_integ, sizeof(float) * (size_t)B * 3, hipMemcpyDeviceToHost, st));
            if (rate && rate->tail_next) HIPCHK(h, hipMemcpyAsync(rate->tail_next, d_tail, sizeof(float) * (size_t)B * H * 3, hipMemcpyDeviceToHost, st));
            if (io.u_next) HIPCHK(h, hipMemcpyAsync(io.u_next, h->d_u.p, sizeof(float) * (size_t)B * H * m, hipMemcpyDeviceToHost, st));
            if (io.stepsize_next) HIPCHK(h, hipMemcpyAsync(io.stepsize_next, h->d_step.p, sizeof(float) * B, hipMemcpyDeviceToHost, st));
            if (io.keys_next) HIPCHK(h, hipMemcpyAsync(io.keys_next, d_keys, sizeof(uint32_t) * 2 * B, hipMemcpyDeviceToHost, st));
            if (timed && timed->u_act_next) HIPCHK(h, hipMemcpyAsync(timed->u_act_next, d_mot, sizeof(float) * (size_t)B * m, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(h, hipStreamSynchronize(st));
        if (gave_up) {             // the workgroups of a cooperative layout were not all resident: no second try on this handle
            h->coop_off = true;
            h->layout_fallbacks += 1;
            h->last_coop_B = 0;
            *again = true;
            return 0;
        }
        if (tickets_consistent(h) != 0) { *again = true; return 0; }     // (the mirror is re-synchronised)
        if (io.xs || io.us || (rate && rate->ws))
            for (int kc = 0; kc < nk; ++kc)
                for (int b = 0; b < B; ++b) {
                    const size_t r = (size_t)kc * B + b, k = k0 + kc;
                    if (io.xs) memcpy(io.xs + ((size_t)b * (T + 1) + k + 1) * NX, &hx[r * NX], sizeof(float) * NX);
                    if (io.us) memcpy(io.us + ((size_t)b * T + k) * m, &hu[r * m], sizeof(float) * m);
                    if (rate && rate->ws) memcpy(rate->ws + ((size_t)b * T + k) * 4, &hw[r * 4], sizeof(float) * 4);
                }
        if (gproc && proc->dist_rows)
            for (int kc = 0; kc < nk; ++kc)
                for (int b = 0; b < B; ++b)
                    memcpy(proc->dist_rows + ((size_t)b * T + k0 + kc) * NG, &hg[((size_t)kc * B + b) * NG], sizeof(float) * NG);
        if (bproc && proc->bias_rows)
            for (int jc = 0; jc < np; ++jc)
                for (int b = 0; b < B; ++b)
                    memcpy(proc->bias_rows + ((size_t)b * Ns + j0 + jc) * NB, &hb[((size_t)jc * B + b) * NB], sizeof(float) * NB);
        if (fproc && evt->fault_rows)
            for (int kc = 0; kc < nk; ++kc)
                for (int b = 0; b < B; ++b)
                    memcpy(evt->fault_rows + ((size_t)b * T + k0 + kc) * m * 2, &hf[((size_t)kc * B + b) * m * 2], sizeof(float) * m * 2);
        for (int b = 0; !he.empty() && b < B; ++b) {
            const uint32_t* row = &he[(size_t)b * EVENT_EP_WORDS];
            if (evt->fault_keys_next) memcpy(evt->fault_keys_next + 2 * (size_t)b, row, 2 * sizeof(uint32_t));
            if (evt->fault_state_next) memcpy(evt->fault_state_next + (size_t)b * m * 2, row + 2, sizeof(int32_t) * m * 2);
        }
        if (dproc && evt->valid_rows)
            for (int jc = 0; jc < np; ++jc)
                for (int b = 0; b < B; ++b)
                    evt->valid_rows[(size_t)b * Ns + j0 + jc] = hv[(size_t)jc * B + b];
        if (subs_out)
            for (size_t rr = 0; rr < (size_t)nk * nsub; ++rr)
                for (int b = 0; b < B; ++b)
                    memcpy(flt->xsub + ((size_t)b * T * nsub + k0 * nsub + rr) * NX, &hs[(rr * B + b) * NX], sizeof(float) * NX);
        if (io.info)
            for (int jc = 0; jc < np; ++jc)
                for (int b = 0; b < B; ++b)
                    memcpy((float*)io.info + ((size_t)b * Ns + j0 + jc) * 8, &hi[((size_t)jc * B + b) * 8], sizeof(float) * 8);
        if (seen && obs->xmeas)
            for (int jc = 0; jc < np; ++jc)
                for (int b = 0; b < B; ++b)
                    memcpy(obs->xmeas + ((size_t)b * Ns + j0 + jc) * NX, &hm[((size_t)jc * B + b) * NX], sizeof(float) * NX);
        if (!hn.empty())
            for (int i = 0; i < AM; ++i)
                for (int b = 0; b < B; ++b)
                    memcpy(obs->xhist_next + ((size_t)b * AM + i) * NX, &hn[(size_t)i * HR + (size_t)b * NX], sizeof(float) * NX);
    }
    return 0;
}
}  // namespace
