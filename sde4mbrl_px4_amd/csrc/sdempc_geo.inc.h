// sdempc_geo.inc.h — the geometric baseline controller of SPEC.md §11l, included by sdempc_prng.hip (FMA, DI, rsqrt_spec are that file's).
//
// Path replaced (reference): the node's only native component, a geometric tracking controller — PD position feedback with a clip on
// the norm of the acceleration, a desired attitude from the desired acceleration and the reference heading, the SO(3) attitude error as body-rate commands
// and a collective thrust along the CURRENT body z axis. It publishes what the rate loop of §11d consumes: mean thrust and three body rates.
//
// Mapping: about 100 flops and 39 + 13 words per episode, one thread per episode inside sdempc_loop_keys_period_kernel (its BASELINE form), so that a
// campaign flies the baseline through the same device loop as the MPC with no state copied back per tick. Every product and fma below is the one §11l
// states (-ffp-contract=off); tests/geo_ref.py restates them in NumPy.
#pragma once

namespace sdempc {

// R(q) of SPEC.md §5.2, row-major
DI void geo_rot(const float* q, float* R) {
    const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const float xx = qx * qx, yy = qy * qy, zz = qz * qz;
    const float xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
    R[0] = FMA(-2.0f, yy + zz, 1.0f); R[1] = 2.0f * (xy - wz);          R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);          R[4] = FMA(-2.0f, xx + zz, 1.0f); R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);          R[7] = 2.0f * (yz + wx);          R[8] = FMA(-2.0f, xx + yy, 1.0f);
}
DI float geo_dot(float a0, float a1, float a2, float b0, float b1, float b2) { return FMA(a2, b2, FMA(a1, b1, a0 * b0)); }
// SPEC.md §3.6 / §11d: a NaN maps to lo
DI float geo_clamp(float v, float lo, float hi) { return !(v > lo) ? lo : (v > hi ? hi : v); }

// One command: x[13] the state the solve would have started from, w0 / w1 rows ref_row and ref_row + 1 of the window, g the parameter row of the episode
// (GEO_PAR_WORDS floats: kp[3], kv[3], amax, inv_tau, g, kT, k0, c_lo, c_hi). out = (c, omega*[3]).
DI void geo_command(const float* x, const float* w0, const float* w1, const float* g, int accel_ff, float inv_dt, float* out) {
    const float amax = g[6], inv_tau = g[7], grav = g[8], kT = g[9], k0 = g[10], c_lo = g[11], c_hi = g[12];
    float a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float ep = x[i] - w0[i], ev = x[3 + i] - w0[3 + i];
        a[i] = -FMA(g[3 + i], ev, g[i] * ep);
    }
    const float n2 = geo_dot(a[0], a[1], a[2], a[0], a[1], a[2]);
    if (n2 > amax * amax) {
        const float s = amax * rsqrt_spec(n2);
        a[0] = a[0] * s; a[1] = a[1] * s; a[2] = a[2] * s;
    }
    float d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float ff = accel_ff ? (w1[3 + i] - w0[3 + i]) * inv_dt : 0.0f;
        d[i] = a[i] + ff;
    }
    d[2] = d[2] + grav;
    const float nd = geo_dot(d[0], d[1], d[2], d[0], d[1], d[2]);
    const float rz = rsqrt_spec(nd);
    const float z0 = d[0] * rz, z1 = d[1] * rz, z2 = d[2] * rz;
    // the heading: the horizontal part of the reference attitude's body x axis, (R00, R10, 0) of R(q_ref)
    const float rw = w0[6], rx = w0[7], ry = w0[8], rzz = w0[9];
    const float c0 = FMA(-2.0f, ry * ry + rzz * rzz, 1.0f), c1 = 2.0f * (rx * ry + rw * rzz);
    // zb x xc with xc2 = 0
    const float y0 = -(z2 * c1), y1 = z2 * c0, y2 = FMA(z0, c1, -(z1 * c0));
    const float ny = geo_dot(y0, y1, y2, y0, y1, y2);
    const float rn = rsqrt_spec(ny);
    const float yb0 = y0 * rn, yb1 = y1 * rn, yb2 = y2 * rn;
    const float xb0 = FMA(yb1, z2, -(yb2 * z1)), xb1 = FMA(yb2, z0, -(yb0 * z2)), xb2 = FMA(yb0, z1, -(yb1 * z0));
    float R[9];
    geo_rot(x + 6, R);
    // M = Rd^T R(q): M[i][j] = (column i of Rd) . (column j of R)
    const float m12 = geo_dot(yb0, yb1, yb2, R[2], R[5], R[8]), m21 = geo_dot(z0, z1, z2, R[1], R[4], R[7]);
    const float m20 = geo_dot(z0, z1, z2, R[0], R[3], R[6]), m02 = geo_dot(xb0, xb1, xb2, R[2], R[5], R[8]);
    const float m01 = geo_dot(xb0, xb1, xb2, R[1], R[4], R[7]), m10 = geo_dot(yb0, yb1, yb2, R[0], R[3], R[6]);
    const float t = geo_dot(d[0], d[1], d[2], R[2], R[5], R[8]);       // a_des along the CURRENT body z axis
    const bool ok = nd > 0.0f && ny > 0.0f;                           // (zero or NaN: no attitude can be formed)
    out[0] = geo_clamp(ok ? FMA(kT, t, k0) : k0, c_lo, c_hi);
    out[1] = ok ? inv_tau * (m12 - m21) : 0.0f;
    out[2] = ok ? inv_tau * (m20 - m02) : 0.0f;
    out[3] = ok ? inv_tau * (m01 - m10) : 0.0f;
}

// The BASELINE form of the period's key-schedule launch (SPEC.md §11l step 8): thread b fills the tables the rate-loop plant launch reads in place of a solve's.
// With A.out given instead (sdempc_geo_command_batch) it stores (c, omega*) and nothing else.
DI void geo_fill(const LoopBaseline& A, int b) {
    const float* x = A.x + (size_t)b * 13;
    const float* w0 = A.xref + (size_t)b * A.xref_ep_stride + (size_t)A.ref_row * 13;
    float cw[4];
    geo_command(x, w0, w0 + 13, A.par + (size_t)b * A.par_ep_stride, A.accel_ff, A.inv_dt, cw);
    if (A.out) {
        float* o = A.out + (size_t)b * 4;
        o[0] = cw[0]; o[1] = cw[1]; o[2] = cw[2]; o[3] = cw[3];
        return;
    }
    const int H = A.H, m = A.m;
    float* u = A.uopt + (size_t)b * H * m;
    for (int e = 0; e < H * m; ++e) u[e] = cw[0];
    float* xe = A.xevol + (size_t)b * (H + 1) * 13;
#pragma unroll
    for (int c = 0; c < 13; ++c) xe[c] = x[c];
    for (int t = 1; t <= H; ++t) {
        float* row = xe + (size_t)t * 13;
#pragma unroll
        for (int c = 0; c < 10; ++c) row[c] = 0.0f;
        row[10] = cw[1]; row[11] = cw[2]; row[12] = cw[3];
    }
    float* inf = A.info + (size_t)b * 8;
    inf[0] = 0.0f; inf[1] = A.step[b];
#pragma unroll
    for (int c = 2; c < 8; ++c) inf[c] = 0.0f;
}

}  // namespace sdempc
