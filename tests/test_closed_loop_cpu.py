"""Batched closed loop (SPEC.md §11) without a GPU: argument checks of sdempc_closed_loop_batch (no HIP call may happen before them)
and the CPU reference of tests/closed_loop_ref.py against its definition."""
import ctypes as C
import os

import numpy as np
import pytest

import orc
from cases import CDIR
from closed_loop_ref import closed_loop_ref, default_warm_start
from sde4mbrl_px4_amd import _abi, load_mpc_config, prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.sde_mpc_design import _next_key


def small_cfg(**kw):
    c1 = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml"))
    return c1.replace(**{"horizon": 10, "num_short_dt": 10, "num_particles": 33, "max_iter": 8, "max_no_improvement_iter": 8, **kw})


class _Args:
    """ctypes buffers of one sdempc_closed_loop_batch call."""

    def __init__(self, cfg, B, T, Tx=1, Bx=1):
        H, m = cfg.horizon, cfg.num_motors
        self.x0 = np.zeros((B, 13), np.float32)
        self.xref = np.zeros((Tx, Bx, H + 1, 13), np.float32)
        self.keys = np.zeros((B, 2), np.uint32)
        n = max(T, 1)
        self.xs = np.zeros((B, n + 1, 13), np.float32)
        self.us = np.zeros((B, n, m), np.float32)
        self.info = np.zeros((B, n, 8), np.float32)

    def call(self, lib, h, B, T, Tx, Bx, null=None):
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        p = {"x0": self.x0.ctypes.data_as(fp), "xref": self.xref.ctypes.data_as(fp), "keys": self.keys.ctypes.data_as(u32p),
             "xs": self.xs.ctypes.data_as(fp), "us": self.us.ctypes.data_as(fp), "info": self.info.ctypes.data_as(C.POINTER(_abi.SdempcInfo))}
        if null:
            p[null] = None
        return lib.sdempc_closed_loop_batch(h, B, T, p["x0"], p["xref"], Tx, Bx, p["keys"], None, None, p["xs"], p["us"], p["info"],
                                            None, None, None)


def test_closed_loop_argument_checks_make_no_hip_call():
    lib = _abi.load_library()
    cfg = small_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    try:
        cases = [  # (B, T, Tx, Bx, null pointer, expected code)
            (5, 3, 1, 1, None, -5),           # B > max_batch
            (4, 0, 1, 1, None, -1),           # T = 0
            (4, 3, 2, 1, None, -1),           # xref_ticks not in {1, T}
            (4, 3, 0, 1, None, -1),
            (4, 3, 1, 2, None, -1),           # xref_batch not in {1, B}
            (4, 3, 1, 0, None, -1),
        ] + [(4, 3, 1, 1, name, -1) for name in ("x0", "xref", "keys", "xs", "us", "info")]
        for B, T, Tx, Bx, null, want in cases:
            a = _Args(cfg, B, T, max(Tx, 1), max(Bx, 1))
            rc = a.call(lib, h, B, T, Tx, Bx, null)
            assert rc == want, (B, T, Tx, Bx, null, rc, lib.sdempc_last_error(h))
            assert lib.sdempc_last_error(h)
            assert lib.sdempc_device_ready(h) == 0
    finally:
        lib.sdempc_destroy(h)


def test_reference_tick0_solve_key_is_m_mpc_key():
    """The solve of tick 0 draws its noise from split(r_0)[1], exactly what m_mpc hands the solver."""
    r0 = prng.PRNGKey(1234)
    r1, sub = orc.split(r0, 2)
    new_rng, sub_m = _next_key(r0)
    assert np.array_equal(sub, sub_m) and np.array_equal(r1, new_rng)


def test_plant_noise_is_bits_of_six():
    r0 = prng.PRNGKey(77)
    r1, _ = orc.split(r0, 2)
    _, p = orc.split(r1, 2)
    xi = orc.normal(p, 6)
    bits = prng.random_bits(p, 6)
    assert np.array_equal(orc.random_bits(p, 6), bits)
    want = np.array([orc.lib().orc_bits_to_normal(int(v)) for v in bits], np.float32)
    assert xi.tobytes() == want.tobytes()
    longer = orc.normal(p, 12)[:6]       # SPEC.md §7.1: counter i pairs with i + n/2, so a longer draw is a different stream
    assert xi.tobytes() != longer.tobytes()


def test_reference_one_tick_is_one_solve_and_one_step():
    cfg = small_cfg(max_iter=4, max_no_improvement_iter=4)
    model = synthetic_iris()
    x0 = W.random_initial_states(2, 40)
    xref = W.constant_reference(W.HOVER, cfg.horizon)
    keys = np.stack([prng.PRNGKey(5), prng.PRNGKey(6)])
    xs, us, info, u_next, s_next, k_next = closed_loop_ref(cfg, model, x0, xref, keys, 1)
    O = orc.Oracle(cfg, model)
    u0, s0 = default_warm_start(cfg, 2)
    for b in range(2):
        r1, sub = orc.split(keys[b], 2)
        uo, _, inf, _ = O.solve(x0[b], xref, orc.noise_from_key(sub, cfg.num_particles, cfg.horizon), u0[b], s0[b])
        r2, p = orc.split(r1, 2)
        xn, _ = O.step(x0[b], uo[0], orc.normal(p, 6), t=0)
        assert xs[b, 0].tobytes() == x0[b].tobytes()
        assert xs[b, 1].tobytes() == xn.tobytes() and us[b, 0].tobytes() == uo[0].tobytes() and info[b, 0].tobytes() == inf.tobytes()
        assert u_next[b].tobytes() == np.concatenate([uo[1:], uo[-1:]]).tobytes()
        assert s_next[b] == inf[1] and np.array_equal(k_next[b], r2)
