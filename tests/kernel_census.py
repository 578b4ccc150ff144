"""Census of the kernels of the default build: for every kernel that `libsdempc.so` carries, the call that makes the host dispatcher
(sde4mbrl_px4_amd/csrc/sdempc_kernels.hip: launch_solve, launch_solve_team, launch_duo*, launch_coop_m, launch_spec_m, launch_lane, launch_grad,
launch_rollout) pick exactly that instantiation, at the smallest shape at which it still is the pick and can still go wrong.

  * ROWS: one Row per kernel whose name the library reports back (note_kernel -> sdempc_last_kernel_name): every solve, speculative, gradient and
    rollout kernel, in both math modes. tests/test_gpu_kernel_census.py runs each row, requires the reported name to EQUAL the row's and compares
    every output with the CPU oracle bit for bit; tests/test_kernel_census_cpu.py proves on the CPU that the table names exactly the kernels of
    the build and that every row's problem moves (iterations, an accepted step, a gradient in every motor column).
  * ALL_ROWS: one Row per kernel that only the all-variants build carries (`make allvariants`, csrc/allvariants/libsdempc.so: the generic 8-slot
    instantiation in the duo, six-team, cooperative, speculative and global-control-table layouts; the packed-tanh latency kernels), and two rows on
    the two sides of the batch size at which that build's dispatcher stops taking a packed-tanh kernel. tests/test_gpu_kernel_census_all.py runs them
    in a child process that has that library loaded. The stated limit of this census: the kernels common to both builds get no second set of rows;
    of the second library's own copies of them only the one behind the threshold row is run.
  * ELSEWHERE: the kernels whose choice is route and arithmetic alone and whose names cannot be read back (the closed loop's plant steps: launch_loop
    does not call note_kernel; the PRNG kernels; the layout conversions): the existing GPU test that runs each.
  * UNREACHED: kernels that are built but that no input can dispatch, with the dispatcher's own words for why.

Shapes. P: 1 (lane kernels), 32 (TeamWave: one group), 33 (two groups, the second one particle), 70 (three groups: a duo pair without its second
group), 130 (five groups, the last with two particles: more groups than waves, hence the four-wave duo team). H = 8 with two step lengths, except
where the LDS budget selects the instantiation: there H is the shortest horizon at which the dispatcher's own arithmetic (smem_bytes below, a
restatement of the one in sdempc_kernels.hip) makes the pick, and the row's note carries the derivation. max_iter = 3. B = 3 where handle options
force the layout (5 for the one-wave teams: a second workgroup with one of its four teams in use); a function of the device's CU count where the
batch size is what selects the kernel. The oracle runs on a sample of instances: the first, the last and one across a workgroup boundary.

`python tests/kernel_census.py` rewrites tests/KERNELS.md and tests/KERNELS_ALL.md."""
import dataclasses
import functools
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc")
AV_DIR = os.path.join(CSRC, "allvariants")          # `make allvariants`: the all-variants build, objects and library
KERNELS_MD = os.path.join(ROOT, "tests", "KERNELS.md")
KERNELS_ALL_MD = os.path.join(ROOT, "tests", "KERNELS_ALL.md")
CUS = 256                       # compute units of an MI355X: what the CPU-side checks and KERNELS.md evaluate the batch expressions for
F16_OF = {"f32": 0, "f16": 1, "f32x3": 2}
MLP_OF = {v: k for k, v in F16_OF.items()}
MODES = ("exact", "fast")


# ---- kernel names: one normal form for the symbol table's and the runtime's spelling ---------------------------------------------------
def normalise(name):
    """(kernel, math mode) of a demangled kernel name, as `nm -C` prints a host stub or as sdempc_last_kernel_name reports the launch:
    `void`, `__device_stub__`, the qualifiers `sdempc::`, `exact::`, `fastm::` and the parameter list are stripped; the math mode ("exact", "fast",
    or "" for a kernel outside both namespaces) is what the stripped qualifier said."""
    s = name.strip()
    mode = "fast" if "fastm::" in s else ("exact" if "exact::" in s else "")
    if s.endswith(")"):                          # the parameter list: the last top-level parenthesis group
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += (s[i] == ")") - (s[i] == "(")
            if depth == 0:
                s = s[:i]
                break
    if s.startswith("void "):
        s = s[5:]
    for q in ("__device_stub__", "sdempc::", "exact::", "fastm::"):
        s = s.replace(q, "")
    return s.strip(), mode


def built_kernels(where=CSRC):
    """{(kernel, mode)} of what is built in the directory `where`, from the symbol table (one __device_stub__ per kernel): of libsdempc.so, else of the
    objects beside it. None when nothing is built or nm is missing."""
    if not shutil.which("nm") or not os.path.isdir(where):
        return None
    so = os.path.join(where, "libsdempc.so")
    files = [so] if os.path.exists(so) else sorted(os.path.join(where, f) for f in os.listdir(where) if f.endswith(".o"))
    if not files:
        return None
    out = set()
    for f in files:
        txt = subprocess.run(["nm", "-C", "--defined-only", f], capture_output=True, text=True, check=True).stdout
        for line in txt.splitlines():
            if "__device_stub__" in line:
                out.add(normalise(re.sub(r"^[0-9a-fA-F]*\s+\S\s+", "", line)))
    return out or None


# ---- the dispatcher's LDS arithmetic (sdempc_kernels.hip: smem_floats, smem_bytes, launch_duo_m, launch_duo_small, use_global_ust) -----------
LDS_CAP = 156 * 1024
NZ_STAGE = 6 * 64


def smem_bytes(H, m, ipb=1, coop=False, ust_lds=True, nz_waves=0):
    r4 = lambda n: (n + 3) & ~3
    shared = 6 * 32 + 4 * 32 + 6 * 2 * 32 + m * 32 + 2 * 32 * 32 + 1024 + r4(H) + r4(H * 6) + r4(H + 1)
    per_team = (H * 36 if ust_lds else 0) + r4((H + 1) * 13) + 16 + 6 * r4(H * m)
    return 4 * (shared + ipb * per_team + ((r4(H * 12) + H * 64 + 4 * H * 8) if coop else 0) + nz_waves * NZ_STAGE)


def duo_pick(H, m, waves, ustg=-1):
    """launch_duo_m: 0 staging rows + control table in LDS (MODE 3, USTG false), 1 staging rows + table in global memory (MODE 3, USTG true), 2 neither
    in LDS (MODE 4)."""
    by_regs = 12 // waves
    per_cu = lambda ust_lds, stage: min(by_regs, LDS_CAP // smem_bytes(H, m, 1, False, ust_lds, waves if stage else 0))
    can_g, must_g = ustg != 0, ustg == 1
    pick, best = (1, per_cu(False, True)) if must_g else (0, per_cu(True, True))
    if not must_g and can_g and per_cu(False, True) > best:
        pick, best = 1, per_cu(False, True)
    if can_g and per_cu(False, False) > best:
        pick = 2
    return pick


def pair_fits(H, m):
    """launch_duo_small: two two-wave teams per workgroup, three workgroups per CU with both control tables in LDS"""
    return smem_bytes(H, m, 2, False, True, 4) * 3 <= LDS_CAP


def global_table(H, m):
    """use_global_ust with the option on auto, four-wave team"""
    per_cu = lambda b: min(3, LDS_CAP // b)
    return per_cu(smem_bytes(H, m, 1, False, False)) > per_cu(smem_bytes(H, m, 1))


def coop_kernel(M, P, B, cus=CUS):
    """launch_coop_m: the one-workgroup-per-CU build while B x coop_nwg(P) <= CUs, the two-waves-per-SIMD one beyond"""
    return f"sdempc_solve_kernel<TeamBlock, {M}, 0, {'true' if B * ((P + 3) // 4) <= cus else 'false'}, 2, false>"


def throughput_kernel(H, P, m, f16, B, cus=CUS):
    """launch_solve / launch_solve_team with no option forced, for a batch beyond the cooperative layouts, m in (4, 6), default build"""
    G = (P + 31) // 32
    if G == 1 and smem_bytes(H, m, 4) <= 80 * 1024:
        return f"sdempc_solve_kernel<TeamWave, {m}, {f16}, false, 0, false>"
    gtab = global_table(H, m)
    if G <= 4 and B <= min(3, LDS_CAP // smem_bytes(H, m, 1, False, not gtab)) * cus:
        return f"sdempc_solve_kernel<TeamBlock, {m}, {f16}, false, 0, {'true' if gtab else 'false'}>"
    if G > 4:
        return f"sdempc_solve_kernel<TeamBlock, {m}, {f16}, false, {('3, false', '3, true', '4, true')[duo_pick(H, m, 4)]}>"
    if B >= 6 * cus and smem_bytes(H, m, 6, False, True, 12) <= LDS_CAP:
        return f"sdempc_solve_kernel<TeamPairT<6>, {m}, {f16}, false, 3, false>"
    if pair_fits(H, m):
        return f"sdempc_solve_kernel<TeamPairT<2>, {m}, {f16}, false, 3, false>"
    return f"sdempc_solve_kernel<TeamBlock2, {m}, {f16}, false, {('3, false', '3, true', '4, true')[duo_pick(H, m, 2)]}>"


def shortest_h(pred, lo=6, hi=2000):
    return next(H for H in range(lo, hi) if pred(H))


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Row:
    kernel: str                 # normalised name
    mode: str                   # math mode: "exact" / "fast"
    kind: str                   # solve (host noise tensor), solve_keys (noise drawn on the device), grad, rollout
    m: int                      # motors: 4 synthetic_iris, 6 synthetic_hexa, 5 asymmetric_model(5) in the generic 8-slot instantiations
    mlp: str
    P: int
    H: int
    batch: str                  # expression in `cus` (the device's compute units)
    options: tuple              # handle options, ((name, value), ...)
    note: str = ""
    stepsize: float = 0.01      # stepsize_in of the solve
    tag: str = ""               # tells apart the rows of a kernel that has more than one (ALL_ROWS: the packed-tanh threshold)

    @property
    def id(self):
        return f"{self.mode}-{self.kernel}".replace(" ", "") + (f"-{self.tag}" if self.tag else "")

    @property
    def vehicle(self):
        return {4: "synthetic_iris", 6: "synthetic_hexa"}.get(self.m, f"asymmetric_model({self.m})")

    def B(self, cus=CUS):
        return int(eval(self.batch, {"__builtins__": {}}, {"cus": int(cus)}))

    def cfg_kw(self):
        # two step lengths; the horizons that the LDS budget dictates take shorter steps, so that they span seconds as the short ones do
        dts = dict(short_step_dt=0.05, long_step_dt=0.1) if self.H <= 20 else dict(short_step_dt=0.01, long_step_dt=0.02)
        return dict(horizon=self.H, num_short_dt=max(1, self.H // 2), num_particles=self.P, u_slew_coeff=1.0, max_iter=3,
                    max_no_improvement_iter=3, mlp_dtype=self.mlp, math_mode=self.mode, **dts)

    def cfg(self):
        from cases import asymmetric_cfg
        from sde4mbrl_px4_amd import MPCConfig
        kw = self.cfg_kw()
        if self.m == 4:
            return MPCConfig(**kw)
        if self.m == 6:
            return MPCConfig(input_id=list(range(6)), input_bound=[[1e-4, 1.0]] * 6, uref=[0.42] * 6, **kw)
        return asymmetric_cfg(self.m, **kw)

    def model(self):
        from cases import asymmetric_model
        from sde4mbrl_px4_amd import synthetic_hexa, synthetic_iris
        return synthetic_iris() if self.m == 4 else synthetic_hexa() if self.m == 6 else asymmetric_model(self.m)

    def sample(self, cus=CUS):
        """instances the oracle runs: the first, the last, and the two sides of the first workgroup boundary that the batch has"""
        B = self.B(cus)
        ipb = 4 if "TeamWave" in self.kernel else 2 if "TeamPairT<2>" in self.kernel else 6 if "TeamPairT<6>" in self.kernel else 1
        return sorted({0, B - 1} | {b for b in (ipb - 1, ipb) if b < B})


GENERIC_M = 5                   # what runs the 8-slot instantiations: three zero-padded slots, asymmetric vehicle and per-motor settings
SEED = 17


def _rows():
    rows = []
    opt = lambda **kw: tuple(sorted(kw.items()))
    m_of = lambda M: GENERIC_M if M == 8 else M
    for mode in MODES:
        add = lambda kernel, kind, M, f, P, H, batch, options, note="", **kw: rows.append(
            Row(kernel, mode, kind, m_of(M), MLP_OF[f], P, H, str(batch), options, note, **kw))
        for f in (0, 1, 2):
            for M in (4, 6, 8):
                # one group per wave, MODE 0. f32 contractions: coop=0 keeps a small batch out of the cooperative layouts (sdempc_solve_batch_dev)
                add(f"sdempc_solve_kernel<TeamWave, {M}, {f}, false, 0, false>", "solve", M, f, 32, 8, 5, opt(coop=0))
                add(f"sdempc_solve_kernel<TeamBlock, {M}, {f}, false, 0, false>", "solve", M, f, 33, 8, 3, opt(coop=0, duo=0))
                add(f"sdempc_grad_kernel<TeamWave, {M}, {f}, 0>", "grad", M, f, 32, 8, 5, opt())
                add(f"sdempc_grad_kernel<TeamBlock, {M}, {f}, 0>", "grad", M, f, 130, 8, 3, opt())
            add(f"sdempc_rollout_kernel<TeamWave, {f}, 0>", "rollout", 4, f, 32, 8, 5, opt())
            add(f"sdempc_rollout_kernel<TeamBlock, {f}, 0>", "rollout", 6, f, 130, 8, 3, opt())
            for M in (4, 6):
                m = M
                # control table in global memory because the LDS budget says so (use_global_ust, option on auto); B = 3 fits resident, so duo = auto
                # keeps one group per wave (one_group_per_wave_batch)
                Hg = shortest_h(lambda H: global_table(H, m))
                add(f"sdempc_solve_kernel<TeamBlock, {M}, {f}, false, 0, true>", "solve", M, f, 33, Hg, 3, opt(coop=0),
                    f"use_global_ust: H = {Hg} is the shortest horizon with smem_bytes(H, {m}, 1) = {smem_bytes(Hg, m)} > 156 KiB / 3 = {LDS_CAP // 3} "
                    f">= {smem_bytes(Hg, m, 1, False, False)} without the table: three workgroups per CU instead of two", stepsize=1e-4)
                # two-wave teams in pairs: B = 3 forced (M = 6), or picked by the batch (M = 4): one more than one group per wave holds resident
                if M == 4:
                    add(f"sdempc_solve_kernel<TeamPairT<2>, {M}, {f}, false, 3, false>", "solve_keys", M, f, 70, 8, "3 * cus + 1", opt(),
                        "takes_duo on auto: B > 3 workgroups per CU x CUs (one_group_per_wave_batch), B < 6 x CUs (no six-team workgroups)")
                else:
                    add(f"sdempc_solve_kernel<TeamPairT<2>, {M}, {f}, false, 3, false>", "solve", M, f, 70, 8, 3, opt(coop=0, duo=1))
                add(f"sdempc_solve_kernel<TeamPairT<6>, {M}, {f}, false, 3, false>", "solve_keys", M, f, 70, 8, "6 * cus", opt(),
                    "launch_duo_small: B >= 6 x CUs fills every team slot")
                # two-wave teams in 128-thread workgroups: when the pair does not fit (LDS table, option ustg = 0 so that launch_duo_m cannot move it)
                Hp = shortest_h(lambda H: not pair_fits(H, m))
                assert duo_pick(Hp, m, 2, 0) == 0
                add(f"sdempc_solve_kernel<TeamBlock2, {M}, {f}, false, 3, false>", "solve", M, f, 70, Hp, 3, opt(coop=0, duo=1, ustg=0),
                    f"launch_duo_small: H = {Hp} is the shortest horizon at which 3 x smem_bytes(H, {m}, 2, nz_waves = 4) = 3 x {smem_bytes(Hp, m, 2, False, True, 4)} "
                    f"> 156 KiB = {LDS_CAP}: no TeamPair; ustg = 0 pins launch_duo_m's pick 0", stepsize=1e-3)
                add(f"sdempc_solve_kernel<TeamBlock2, {M}, {f}, false, 3, true>", "solve", M, f, 70, 8, 3, opt(coop=0, duo=1, ustg=1))
                H4 = shortest_h(lambda H: not pair_fits(H, m) and duo_pick(H, m, 2) == 2)
                add(f"sdempc_solve_kernel<TeamBlock2, {M}, {f}, false, 4, true>", "solve", M, f, 70, H4, 3, opt(coop=0, duo=1),
                    f"launch_duo_m, ustg on auto: H = {H4} is the shortest horizon at which the pair does not fit and dropping the staging rows as well buys a "
                    f"workgroup per CU: {LDS_CAP} // {smem_bytes(H4, m, 1, False, False, 0)} > {LDS_CAP} // {smem_bytes(H4, m, 1, False, False, 2)} "
                    f"(table in LDS: {smem_bytes(H4, m, 1, False, True, 2)})", stepsize=1e-4)
                # four-wave duo team: more than four groups; duo on auto takes it at any batch size
                add(f"sdempc_solve_kernel<TeamBlock, {M}, {f}, false, 3, false>", "solve", M, f, 130, 8, 3, opt(coop=0))
                add(f"sdempc_solve_kernel<TeamBlock, {M}, {f}, false, 3, true>", "solve", M, f, 130, 8, 3, opt(coop=0, ustg=1))
                H4b = shortest_h(lambda H: duo_pick(H, m, 4) == 2)
                add(f"sdempc_solve_kernel<TeamBlock, {M}, {f}, false, 4, true>", "solve", M, f, 130, H4b, 3, opt(coop=0),
                    f"launch_duo_m, ustg on auto: H = {H4b} is the shortest horizon at which only the carve without table and staging rows keeps the most "
                    f"workgroups per CU: {LDS_CAP} // {smem_bytes(H4b, m, 1, False, False, 0)} > {LDS_CAP} // {smem_bytes(H4b, m, 1, False, False, 4)} "
                    f"(table in LDS: {smem_bytes(H4b, m, 1, False, True, 4)})", stepsize=3e-6 if M == 4 else 1e-4)
        # f32 contractions only: the lane layouts
        for M in (4, 6, 8):
            # P = 1; spec = 0 because a single particle is welcome in the speculative kernel (spec_max_instances)
            add(f"sdempc_solve_kernel<TeamWave, {M}, 0, false, 1, false>", "solve", M, 0, 1, 8, 5, opt(spec=0))
            add(f"sdempc_grad_kernel<TeamWave, {M}, 0, 1>", "grad", M, 0, 1, 8, 5, opt())
        add("sdempc_rollout_kernel<TeamWave, 0, 1>", "rollout", 4, 0, 1, 8, 5, opt())
        for M in (4, 6):
            # cooperative: nine workgroups per instance at P = 33. One workgroup per CU while B x 9 <= CUs, two beyond
            add(f"sdempc_solve_kernel<TeamBlock, {M}, 0, true, 2, false>", "solve", M, 0, 33, 8, 3, opt(spec=0))
            add(f"sdempc_solve_kernel<TeamBlock, {M}, 0, false, 2, false>", "solve", M, 0, 33, 8, "cus // 9 + 1", opt(spec=0),
                "launch_coop_m: B x coop_nwg(33) = B x 9 > CUs, B <= coop_max_instances = (2 CUs - 16) / 9")
            add(f"sdempc_solve_spec_kernel<{M}, false>", "solve", M, 0, 33, 8, 3, opt())
            add(f"sdempc_solve_spec_kernel<{M}, true>", "solve", M, 0, 1, 8, 3, opt())
    return rows


ROWS = _rows()


def _all_rows():
    """The kernels that only the all-variants build carries. Options and shapes are those of the matching M = 4 / M = 6 rows of _rows(), with one
    addition: takes_pk, on auto, sends every f32 / exact launch of at most `cus` workgroups to a packed-tanh kernel in that build, so the f32 / exact
    rows of B = 3 that are about another kernel carry pk = 0 (the cooperative and speculative layouts are chosen before takes_pk is asked)."""
    rows = []
    opt = lambda **kw: tuple(sorted(kw.items()))
    m = GENERIC_M
    for mode in MODES:
        add = lambda kernel, kind, M, f, P, H, batch, options, note="", **kw: rows.append(
            Row(kernel, mode, kind, m if M == 8 else M, MLP_OF[f], P, H, str(batch), options, note, **kw))
        for f in (0, 1, 2):
            pk0 = dict(pk=0) if f == 0 and mode == "exact" else {}
            Hg = shortest_h(lambda H: global_table(H, m))
            add(f"sdempc_solve_kernel<TeamBlock, 8, {f}, false, 0, true>", "solve", 8, f, 33, Hg, 3, opt(coop=0, **pk0),
                f"use_global_ust: H = {Hg} is the shortest horizon with smem_bytes(H, {m}, 1) = {smem_bytes(Hg, m)} > 156 KiB / 3 = {LDS_CAP // 3} "
                f">= {smem_bytes(Hg, m, 1, False, False)} without the table: three workgroups per CU instead of two", stepsize=1e-4)
            # two-wave teams in pairs: one row picked by the batch (noise drawn on the device), the others forced at B = 3
            if f == 2 and mode == "exact":
                add(f"sdempc_solve_kernel<TeamPairT<2>, 8, {f}, false, 3, false>", "solve_keys", 8, f, 70, 8, "3 * cus + 1", opt(),
                    "takes_duo on auto: B > 3 workgroups per CU x CUs (one_group_per_wave_batch), B < 6 x CUs (no six-team workgroups)")
            else:
                add(f"sdempc_solve_kernel<TeamPairT<2>, 8, {f}, false, 3, false>", "solve", 8, f, 70, 8, 3, opt(coop=0, duo=1, **pk0))
            add(f"sdempc_solve_kernel<TeamPairT<6>, 8, {f}, false, 3, false>", "solve_keys", 8, f, 70, 8, "6 * cus", opt(),
                "launch_duo_small: B >= 6 x CUs fills every team slot")
            Hp = shortest_h(lambda H: not pair_fits(H, m))
            assert duo_pick(Hp, m, 2, 0) == 0
            add(f"sdempc_solve_kernel<TeamBlock2, 8, {f}, false, 3, false>", "solve", 8, f, 70, Hp, 3, opt(coop=0, duo=1, ustg=0, **pk0),
                f"launch_duo_small: H = {Hp} is the shortest horizon at which 3 x smem_bytes(H, {m}, 2, nz_waves = 4) = 3 x {smem_bytes(Hp, m, 2, False, True, 4)} "
                f"> 156 KiB = {LDS_CAP}: no TeamPair; ustg = 0 pins launch_duo_m's pick 0", stepsize=1e-3)
            add(f"sdempc_solve_kernel<TeamBlock2, 8, {f}, false, 3, true>", "solve", 8, f, 70, 8, 3, opt(coop=0, duo=1, ustg=1, **pk0))
            H4 = shortest_h(lambda H: not pair_fits(H, m) and duo_pick(H, m, 2) == 2)
            add(f"sdempc_solve_kernel<TeamBlock2, 8, {f}, false, 4, true>", "solve", 8, f, 70, H4, 3, opt(coop=0, duo=1, **pk0),
                f"launch_duo_m, ustg on auto: H = {H4} is the shortest horizon at which the pair does not fit and dropping the staging rows as well buys a "
                f"workgroup per CU: {LDS_CAP} // {smem_bytes(H4, m, 1, False, False, 0)} > {LDS_CAP} // {smem_bytes(H4, m, 1, False, False, 2)} "
                f"(table in LDS: {smem_bytes(H4, m, 1, False, True, 2)})", stepsize=1e-4)
            add(f"sdempc_solve_kernel<TeamBlock, 8, {f}, false, 3, false>", "solve", 8, f, 130, 8, 3, opt(coop=0, **pk0))
            add(f"sdempc_solve_kernel<TeamBlock, 8, {f}, false, 3, true>", "solve", 8, f, 130, 8, 3, opt(coop=0, ustg=1, **pk0))
            H4b = shortest_h(lambda H: duo_pick(H, m, 4) == 2)
            add(f"sdempc_solve_kernel<TeamBlock, 8, {f}, false, 4, true>", "solve", 8, f, 130, H4b, 3, opt(coop=0, **pk0),
                f"launch_duo_m, ustg on auto: H = {H4b} is the shortest horizon at which only the carve without table and staging rows keeps the most "
                f"workgroups per CU: {LDS_CAP} // {smem_bytes(H4b, m, 1, False, False, 0)} > {LDS_CAP} // {smem_bytes(H4b, m, 1, False, False, 4)} "
                f"(table in LDS: {smem_bytes(H4b, m, 1, False, True, 4)})", stepsize=1e-4)
        # f32 contractions only: the cooperative and speculative layouts, as at M = 4 / 6
        add("sdempc_solve_kernel<TeamBlock, 8, 0, true, 2, false>", "solve", 8, 0, 33, 8, 3, opt(spec=0))
        add("sdempc_solve_kernel<TeamBlock, 8, 0, false, 2, false>", "solve", 8, 0, 33, 8, "cus // 9 + 1", opt(spec=0),
            "launch_coop_m: B x coop_nwg(33) = B x 9 > CUs, B <= coop_max_instances = (2 CUs - 16) / 9")
        add("sdempc_solve_spec_kernel<8, false>", "solve", 8, 0, 33, 8, 3, opt())
        add("sdempc_solve_spec_kernel<8, true>", "solve", 8, 0, 1, 8, 3, opt())
        if mode == "exact":
            # packed tanh: pk on auto takes every f32 / exact launch of at most `cus` workgroups; shapes of the one-group-per-wave rows
            for M in (4, 6, 8):
                add(f"sdempc_solve_kernel<TeamWave, {M}, 0, true, 0, false>", "solve", M, 0, 32, 8, 5, opt(coop=0))
                add(f"sdempc_solve_kernel<TeamBlock, {M}, 0, true, 0, false>", "solve", M, 0, 33, 8, 3, opt(coop=0, duo=0))
                add(f"sdempc_solve_kernel<TeamBlock8, {M}, 0, true, 0, false>", "solve", M, 0, 130, 8, 3, opt(coop=0),
                    "launch_solve_team: more than four groups, so the packed-tanh launch takes the eight-wave team")
            # the two sides of takes_pk's threshold; the second runs a kernel common to both builds from this library's own code object
            add("sdempc_solve_kernel<TeamBlock, 4, 0, true, 0, false>", "solve", 4, 0, 33, 8, "cus", opt(coop=0, duo=0),
                "takes_pk on auto: B = CUs workgroups is the largest packed-tanh launch", tag="threshold")
            add("sdempc_solve_kernel<TeamBlock, 4, 0, false, 0, false>", "solve", 4, 0, 33, 8, "cus + 1", opt(coop=0, duo=0),
                "takes_pk on auto: one workgroup more than CUs", tag="threshold")
    return rows


ALL_ROWS = _all_rows()

# ---- kernels whose names cannot be read back: the existing GPU test that runs each ------------------------------------------------------------
ARITH = [(d, mth) for d in ("f32", "f16", "f32x3") for mth in MODES]      # tests/loop_cases.py
LOOP_ROUTES = {     # launch_loop's if-chain, top to bottom -> (kernel, test); the plant's math mode picks the namespace, its mlp_dtype F16
    "no period, no plant set": ("sdempc_loop_tick_kernel<{f}, false>", "test_gpu_closed_loop::test_closed_loop_matches_reference[{mlp}-{mode}]"),
    "no period, a plant set": ("sdempc_loop_tick_kernel<{f}, true>", "test_gpu_plant_loop::test_perturbed_plants_match_reference[{mlp}-{mode}-4]"),
    "fault and rate loop": ("sdempc_loop_period_kernel<{f}, true, true, true>", "test_gpu_fault_loop::test_every_arithmetic[{mlp}-{mode}-rate]"),
    "fault": ("sdempc_loop_period_kernel<{f}, true, false, true>", "test_gpu_fault_loop::test_every_arithmetic[{mlp}-{mode}-motors]"),
    "rate loop": ("sdempc_loop_period_kernel<{f}, true, true, false>", "test_gpu_rate_loop::test_scenario_and_rate_loop_in_every_arithmetic[{mlp}-{mode}]"),
    "scenario": ("sdempc_loop_period_kernel<{f}, true, false, false>", "test_gpu_scenario_loop::test_both_schedules_in_every_arithmetic[{mlp}-{mode}]"),
    "period alone": ("sdempc_loop_period_kernel<{f}, false, false, false>", "test_gpu_timed_loop::test_period_one_no_delay_no_lag_is_the_existing_loop[{mlp}-{mode}]"),
}


def _elsewhere():
    out = {}
    for mlp, mode in ARITH:
        for kern, test in LOOP_ROUTES.values():
            out[(kern.format(f=F16_OF[mlp]), mode)] = test.format(mlp=mlp, mode=mode)
    out.update({
        ("sdempc_noise_kernel", ""): "test_gpu_parity::test_device_noise_from_keys_bit_exact[33-5]",
        ("sdempc_loop_keys_kernel", ""): "test_gpu_closed_loop::test_closed_loop_matches_reference[f32-exact]",
        ("sdempc_loop_keys_sub_kernel", ""): "test_gpu_plant_loop::test_perturbed_plants_match_reference[f32-exact-4]",
        ("sdempc_loop_keys_period_kernel", ""): "test_gpu_timed_loop::test_every_arrival_point_matches_reference[33-3-4-shared]",
        ("sdempc_broadcast_rows_kernel", ""): "test_gpu_closed_loop::test_closed_loop_equals_host_loop_of_gpu_solves[T-1]",
        # canonical -> device layout: every host-pointer call's noise tensor; device -> canonical: trajectories and key-derived noise on the way out
        ("sdempc_relayout_kernel<true>", "exact"): "test_gpu_parity::test_edge_cases_bit_exact[tile-P33]",
        ("sdempc_relayout_kernel<false>", "exact"): "test_gpu_parity::test_device_noise_from_keys_bit_exact[33-5]",
    })
    return out


ELSEWHERE = _elsewhere()

# built, but no input dispatches them (at most four names; removing an instantiation is a change of its own)
UNREACHED = {
    ("sdempc_relayout_kernel<true>", "fast"): "launch_relayout(...) { return exact::launch_relayout(to_dev, in, out, B, P, G, C, st); }: the layout conversion has no "
                                              "transcendentals, the entry point takes the exact namespace's copy in either math mode",
    ("sdempc_relayout_kernel<false>", "fast"): "launch_relayout(...) { return exact::launch_relayout(to_dev, in, out, B, P, G, C, st); }",
}


def table_names():
    return {(r.kernel, r.mode) for r in ROWS} | set(ELSEWHERE) | set(UNREACHED)


def all_names():
    """what the all-variants build carries beyond table_names()"""
    return {(r.kernel, r.mode) for r in ALL_ROWS} - table_names()


# ---- a row's problem and its oracle results -----------------------------------------------------------------------------------------------------
def problem(row, cus=CUS):
    """x0 [B][13], xref [B][H+1][13], u [B][H][m], s0 [B], and either noise [B][P][H][6] (kind solve / grad / rollout) or keys uint32[B][2] with
    noise None (solve_keys: drawn on the device; the oracle's copy of an instance comes from noise_of)."""
    from cases import asymmetric_problem
    from sde4mbrl_px4_amd import prng
    from sde4mbrl_px4_amd import workload as W
    cfg, B = row.cfg(), row.B(cus)
    by_keys = row.kind == "solve_keys"
    if row.m in (4, 6):
        x0 = W.random_initial_states(B, SEED)
        xref = np.stack([W.reference_window(0.13 * (b % 160), cfg.time_steps) for b in range(B)])
        noise = None if by_keys else W.make_noise(B, row.P, row.H, SEED)
        rng = np.random.default_rng(SEED + 5)
        u = np.clip(np.asarray(cfg.uref, np.float32) + 0.1 * rng.standard_normal((B, row.H, row.m)), 1e-4, 1).astype(np.float32)
    else:
        x0, xref, noise, u = asymmetric_problem(cfg, B, SEED, noise=not by_keys)
    keys = prng.split(prng.PRNGKey(SEED), B) if by_keys else None
    return dict(x0=x0, xref=xref, noise=noise, keys=keys, u=u, s0=np.full(B, row.stepsize, np.float32))


def noise_of(prob, row, b):
    import orc
    return prob["noise"][b] if prob["noise"] is not None else orc.noise_from_key(prob["keys"][b], row.P, row.H)


@functools.lru_cache(maxsize=None)
def reference(row, cus=CUS):
    """(problem, {b: oracle results of instance b}) over row.sample(): solve rows (uopt, xevol, info, events); grad rows (cost, grad float64);
    rollout rows (cost, traj, mean). The float32 oracle, through the instruction models in the matrix-pipe modes and in math_mode fast."""
    import orc
    prob = problem(row, cus)
    O = orc.Oracle(row.cfg(), row.model())
    ref = {}
    orc.set_threads(min(os.cpu_count() or 1, 8))          # (the oracle's particle loops on several cores: same bits at any count)
    try:
        for b in row.sample(cus):
            nz = noise_of(prob, row, b)
            if row.kind in ("solve", "solve_keys"):
                ref[b] = O.solve_events(prob["x0"][b], prob["xref"][b], nz, prob["u"][b], float(prob["s0"][b]))
            elif row.kind == "grad":
                ref[b] = O.grad(prob["x0"][b], prob["u"][b], prob["xref"][b], nz)
            else:
                ref[b] = O.rollout(prob["x0"][b], prob["u"][b], prob["xref"][b], nz, True, True)
    finally:
        orc.set_threads(1)
    return prob, ref


# ---- tests/KERNELS.md ---------------------------------------------------------------------------------------------------------------------------
def kernels_markdown():
    per_kind = {k: sum(r.kind == k for r in ROWS) for k in ("solve", "solve_keys", "grad", "rollout")}
    L = ["# Kernels of the default build and what runs each", "",
         "Generated by `tests/kernel_census.py` (`python tests/kernel_census.py` rewrites it; `tests/test_kernel_census_cpu.py` fails when it is stale, and",
         "when the names below are not exactly the kernels in the built library's symbol table).", "",
         f"{len(ROWS)} rows of `tests/test_gpu_kernel_census.py` ({', '.join(f'{v} {k}' for k, v in per_kind.items())}), {len(ELSEWHERE)} kernels mapped to existing "
         f"tests, {len(UNREACHED)} built but unreachable. `cus`: the device's compute units (256 on an MI355X).", "",
         "## Rows: the reported kernel name must equal the row's, every output the oracle's bits", "",
         "| mode | kernel | call | vehicle | mlp | P | H | B | options | why this shape |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in ROWS:
        L.append(f"| {r.mode} | `{r.kernel}` | {r.kind} | `{r.vehicle}` | {r.mlp} | {r.P} | {r.H} | `{r.batch}` | "
                 f"{' '.join(f'{k}={v}' for k, v in r.options) or '-'} | {r.note or '-'} |")
    L += ["", "## Kernels that existing tests run (their names are not reported back)", "",
          "Closed loop: `launch_loop`'s if-chain, top to bottom; the plant's math mode picks the namespace and its `mlp_dtype` the first template argument.", ""]
    L += [f"- {route}: `{kern.format(f='F16')}`" for route, (kern, _) in LOOP_ROUTES.items()]
    L += ["", "| mode | kernel | test |", "|---|---|---|"]
    L += [f"| {mode or '-'} | `{k}` | `{t}` |" for (k, mode), t in ELSEWHERE.items()]
    L += ["", "## Built but unreachable", "", "| mode | kernel | what bars it |", "|---|---|---|"]
    L += [f"| {mode} | `{k}` | {why} |" for (k, mode), why in UNREACHED.items()]
    L.append("")
    return "\n".join(L)


def kernels_all_markdown():
    L = ["# Kernels that only the all-variants build carries and what runs each", "",
         "Generated by `tests/kernel_census.py` (`python tests/kernel_census.py` rewrites it; `tests/test_kernel_census_cpu.py` fails when it is stale, and",
         "when the names below together with those of `tests/KERNELS.md` are not exactly the kernels in the symbol table of `csrc/allvariants/libsdempc.so`).", "",
         f"{len(ALL_ROWS)} rows of `tests/test_gpu_kernel_census_all.py`: {len(all_names())} kernels and {sum(bool(r.tag) for r in ALL_ROWS)} rows on the two sides of the "
         "packed-tanh threshold. The kernels common to both builds are run from the default library only (`tests/KERNELS.md`). `cus`: the device's compute "
         "units (256 on an MI355X).", "",
         "| mode | kernel | call | vehicle | mlp | P | H | B | options | why this shape |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in ALL_ROWS:
        L.append(f"| {r.mode} | `{r.kernel}` | {r.kind} | `{r.vehicle}` | {r.mlp} | {r.P} | {r.H} | `{r.batch}` | "
                 f"{' '.join(f'{k}={v}' for k, v in r.options) or '-'} | {r.note or '-'} |")
    L.append("")
    return "\n".join(L)


if __name__ == "__main__":
    with open(KERNELS_MD, "w") as f:
        f.write(kernels_markdown())
    with open(KERNELS_ALL_MD, "w") as f:
        f.write(kernels_all_markdown())
