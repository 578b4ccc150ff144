"""CPU reference of the geometric baseline controller (SPEC.md §11l): geo_command, the NumPy float32 restatement — every product rounded to float32, every fma
the software one of the NumPy restatement (oracle/sde_mpc_numpy.py), rsqrt the software one of SPEC.md §3.2 — in the order §11l fixes; geo_command64, a float64
restatement in plain matrix algebra (np.cross, np.linalg.norm, matrix products: no statement about any order), and geo_table, step 8 of §11l. Test
infrastructure, like rate_loop_ref.py.

`mutant` builds a deliberately WRONG controller, for the discrimination tests: "gravity_subtracted" forms a_des with -g, "velocity_sign" feeds +kv e_v back,
"clip_per_component" clips every component of a_fb to [-amax, amax] instead of the norm, "clip_without_amax" scales a clipped a_fb to unit length, "thrust_along_desired"
projects a_des on the DESIRED zb, "m_transposed" takes M = R(q)^T Rd, "heading_from_current" takes xc from the current attitude, "ff_from_previous_rows" forms the
feed-forward from rows rho - 1, rho (rho = 0: rows 0, 0), "no_guard" returns whatever the arithmetic gives, "clamp_before_offset" clamps kT (a . z) and then adds
k0."""
import numpy as np

from timed_loop_ref import R2

F = np.float32
MUTANTS = ("gravity_subtracted", "velocity_sign", "clip_per_component", "clip_without_amax", "thrust_along_desired", "m_transposed", "heading_from_current",
           "ff_from_previous_rows", "no_guard", "clamp_before_offset")
PAR_NAMES = ("kp", "kv", "amax", "inv_tau", "g", "kT", "k0", "c_lo", "c_hi")


def fma(a, b, c):
    return F(R2.fma(F(a), F(b), F(c)))


def rsqrt(a):
    with np.errstate(all="ignore"):
        return F(R2.rsqrt(F(a)))


def dot(a, b):
    """fma(a2, b2, fma(a1, b1, a0 b0))"""
    return fma(a[2], b[2], fma(a[1], b[1], F(F(a[0]) * F(b[0]))))


def clamp(v, lo, hi):
    """SPEC.md §3.6: a NaN maps to lo."""
    return F(lo) if not (v > lo) else (F(hi) if v > hi else F(v))


def rot(q):
    """R(q) of SPEC.md §5.2, f32[3][3]."""
    qw, qx, qy, qz = (F(v) for v in q)
    xx, yy, zz = F(qx * qx), F(qy * qy), F(qz * qz)
    xy, xz, yz, wx, wy, wz = F(qx * qy), F(qx * qz), F(qy * qz), F(qw * qx), F(qw * qy), F(qw * qz)
    two = F(2)
    return np.array([[fma(-2, F(yy + zz), 1), F(two * F(xy - wz)), F(two * F(xz + wy))],
                     [F(two * F(xy + wz)), fma(-2, F(xx + zz), 1), F(two * F(yz - wx))],
                     [F(two * F(xz - wy)), F(two * F(yz + wx)), fma(-2, F(xx + yy), 1)]], F)


def par_row(par, b):
    """The parameter set of episode b from a dict of arrays with 1 or B rows (GeometricController.arrays)."""
    return {n: np.asarray(par[n], F)[b if np.asarray(par[n]).shape[0] > 1 else 0] for n in PAR_NAMES}


def geo_command(x, xref, p, accel_ff=False, ref_row=0, inv_dt=None, mutant=None, census=None):
    """(c, omega* f32[3]) for one state x f32[13] and one window xref f32[H+1][13]; p a parameter set (par_row); inv_dt float32(1) / float32(time_steps[ref_row]),
    needed with accel_ff. census (a dict): counts what happened — clip / no_clip, lo / hi / inside, guard, ff / no_ff."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(all="ignore"):
        x, xref = np.asarray(x, F), np.asarray(xref, F)
        w0, w1 = xref[ref_row], xref[ref_row + 1]
        kp, kv = np.asarray(p["kp"], F), np.asarray(p["kv"], F)
        amax, inv_tau, g, kT, k0, c_lo, c_hi = (F(p[n]) for n in PAR_NAMES[2:])
        a = np.zeros(3, F)
        for i in range(3):
            ep, ev = F(x[i] - w0[i]), F(x[3 + i] - w0[3 + i])
            if mutant == "velocity_sign":
                ev = F(-ev)
            a[i] = F(-fma(kv[i], ev, F(kp[i] * ep)))
        n2 = dot(a, a)
        clipped = False
        if mutant == "clip_per_component":
            clipped = bool((np.abs(a) > amax).any())
            a = np.clip(a, -amax, amax).astype(F)
        elif n2 > F(amax * amax):
            clipped = True
            s = rsqrt(n2) if mutant == "clip_without_amax" else F(amax * rsqrt(n2))
            a = np.array([F(a[0] * s), F(a[1] * s), F(a[2] * s)], F)
        if mutant == "ff_from_previous_rows":
            w0f, w1f = xref[max(ref_row - 1, 0)], xref[ref_row]
        else:
            w0f, w1f = w0, w1
        d = np.zeros(3, F)
        for i in range(3):
            ff = F(F(w1f[3 + i] - w0f[3 + i]) * F(inv_dt)) if accel_ff else F(0)
            d[i] = F(a[i] + ff)
        d[2] = F(d[2] - g) if mutant == "gravity_subtracted" else F(d[2] + g)
        nd = dot(d, d)
        rz = rsqrt(nd)
        zb = np.array([F(d[0] * rz), F(d[1] * rz), F(d[2] * rz)], F)
        R = rot(x[6:10])
        Rh = R if mutant == "heading_from_current" else None
        if Rh is None:
            rw, rx, ry, rzz = w0[6:10]
            c0, c1 = fma(-2, F(F(ry * ry) + F(rzz * rzz)), 1), F(F(2) * F(F(rx * ry) + F(rw * rzz)))
        else:
            c0, c1 = Rh[0, 0], Rh[1, 0]
        y = np.array([F(-F(zb[2] * c1)), F(zb[2] * c0), fma(zb[0], c1, F(-F(zb[1] * c0)))], F)
        ny = dot(y, y)
        rn = rsqrt(ny)
        yb = np.array([F(y[0] * rn), F(y[1] * rn), F(y[2] * rn)], F)
        xb = np.array([fma(yb[1], zb[2], F(-F(yb[2] * zb[1]))), fma(yb[2], zb[0], F(-F(yb[0] * zb[2]))), fma(yb[0], zb[1], F(-F(yb[1] * zb[0])))], F)
        Rd = (xb, yb, zb)

        def M(i, j):
            if mutant == "m_transposed":
                i, j = j, i
            return dot(Rd[i], R[:, j])
        w = np.array([F(inv_tau * F(M(1, 2) - M(2, 1))), F(inv_tau * F(M(2, 0) - M(0, 2))), F(inv_tau * F(M(0, 1) - M(1, 0)))], F)
        t = dot(d, zb) if mutant == "thrust_along_desired" else dot(d, R[:, 2])
        if mutant == "clamp_before_offset":
            c = F(clamp(F(kT * t), c_lo, c_hi) + k0)
        else:
            c = clamp(fma(kT, t, k0), c_lo, c_hi)
        guard = not (nd > 0 and ny > 0)
        if guard and mutant != "no_guard":
            w = np.zeros(3, F)
            c = clamp(k0, c_lo, c_hi)
        if census is not None:
            for k in ("clip" if clipped else "no_clip", "guard" if guard else None, "ff" if accel_ff else "no_ff",
                      None if guard else ("lo" if c == c_lo else "hi" if c == c_hi else "inside")):
                if k:
                    census[k] = census.get(k, 0) + 1
        return F(c), w


def geo_command64(x, xref, p, accel_ff=False, ref_row=0, dt=None):
    """The same controller in float64 with plain matrix algebra, from the float32 inputs: (c, omega*[3]) as float64. No guard: callers keep it away from the
    degenerate states. dt: time_steps[ref_row] (float64 of the float32 value), needed with accel_ff."""
    x, xref = np.asarray(x, np.float64), np.asarray(xref, np.float64)
    w0, w1 = xref[ref_row], xref[ref_row + 1]
    P = {n: np.asarray(p[n], np.float64) for n in PAR_NAMES}

    def rot64(q):
        w, a, b, c = q
        return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)],
                         [2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)],
                         [2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)]])
    a = -(P["kp"] * (x[0:3] - w0[0:3]) + P["kv"] * (x[3:6] - w0[3:6]))
    n = np.linalg.norm(a)
    if n > P["amax"]:
        a = a * (P["amax"] / n)
    if accel_ff:
        a = a + (w1[3:6] - w0[3:6]) / float(dt)
    d = a + np.array([0.0, 0.0, float(P["g"])])
    zb = d / np.linalg.norm(d)
    Rr = rot64(w0[6:10])
    xc = np.array([Rr[0, 0], Rr[1, 0], 0.0])
    yb = np.cross(zb, xc)
    yb = yb / np.linalg.norm(yb)
    xb = np.cross(yb, zb)
    Rd = np.stack([xb, yb, zb], axis=1)
    R = rot64(x[6:10])
    E = Rd.T @ R - R.T @ Rd
    vee = np.array([E[2, 1], E[0, 2], E[1, 0]])
    w = -(2.0 * float(P["inv_tau"])) * 0.5 * vee
    c = float(np.clip(float(P["kT"]) * float(d @ R[:, 2]) + float(P["k0"]), float(P["c_lo"]), float(P["c_hi"])))
    return c, w


def geo_table(x, c, w, H, m, s):
    """SPEC.md §11l step 8: (uopt f32[H][m], xevol f32[H+1][13], info f32[8]) of one solve."""
    uopt = np.full((H, m), c, F)
    xevol = np.zeros((H + 1, 13), F)
    xevol[0] = np.asarray(x, F)
    xevol[1:, 10:13] = w
    info = np.zeros(8, F)
    info[1] = F(s)
    return uopt, xevol, info


def geo_commands(x, xref, par, accel_ff=False, ref_row=0, inv_dt=None, mutant=None, census=None):
    """geo_command over a batch: x f32[B][13], xref f32[1 or B][H+1][13], par a dict of arrays with 1 or B rows. Returns f32[B][4] = (c, omega*)."""
    x, xref = np.asarray(x, F), np.asarray(xref, F)
    out = np.zeros((x.shape[0], 4), F)
    for b in range(x.shape[0]):
        c, w = geo_command(x[b], xref[b if xref.shape[0] > 1 else 0], par_row(par, b), accel_ff, ref_row, inv_dt, mutant, census)
        out[b, 0], out[b, 1:] = c, w
    return out
