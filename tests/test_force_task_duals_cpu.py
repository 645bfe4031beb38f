"""CPU: the 48 QP multipliers of the default step under a per-robot force task (wbc_step with WBC_DUALS_TASK,
DESIGN.md 25).

  * tests/force_duals_oracle.py's 74-row certificate on the numpy oracle's own x with least-squares multipliers, on
    every set of tests/force_task_duals_oracle.py, held against the committed record
    profiles/force_task_duals/oracle_residuals.json (what the GPU tests' bounds are set from);
  * the certificate has teeth under the task: against the QP without the task's changes to H and g, without the eight
    force multipliers, or with one multiplier off by 1e-6, it fails, clear of the GPU bound;
  * the counts the GPU tests lean on, measured on the oracle;
  * the boundary: constants, Python names, the Makefile's unit list, the launchers' argument check and the compiler's
    resource report of the two new kernel units.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import force_duals_oracle as FD
import force_task_duals_oracle as FTD
import force_task_oracle as FT
import wbc_np as W
from quadrupedwholebodycontroller_amd import _capi
from unit_reports import build_host_program, report, run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrupedwholebodycontroller_amd", "csrc")
# as tests/test_force_duals_cpu.py: an fp64 least-squares fit of a few dozen multipliers to 42 equations whose entries
# reach 1e2-1e4 beside a gradient normalised to O(1)
ORACLE_BOUND = 1e-11
COLD_SETS = (*FTD.COLD_TB, *FTD.COLD_T, FTD.TABLES_SET, FTD.DIRECT_SET)


# 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sets", [COLD_SETS, (FTD.RAMP_SET,), tuple(FTD.OFFTROT_SETS)], ids=["cold", "ramp", "offtrot"])
def test_certificate_on_the_oracles_own_x(sets):
    """Every set: primal feasible, stationary to rounding, complementary at the oracle's own activity threshold, and the
    worst figures per set within 2 x the committed record (and not 100 x below it)."""
    assert sorted(FTD.record()) == sorted(FTD.record("primal")) == sorted(FTD.ALL_SETS)
    both, recs = FTD.measure(sets), {k: FTD.record(k) for k in FTD.KINDS}
    for name in sets:
        n_ok = 0
        for c in FTD.controllers(name):
            if c.qp_status != W.QP_OK:
                continue
            n_ok += 1
            x = c.qp_solution
            viol, stat, _, comp = FD.certificate48(c, x, FD.lsq_duals48(c, x))
            assert viol <= 1e-7 * (1.0 + np.abs(c.qp[2] @ x).max()), (name, viol)
            assert stat <= ORACLE_BOUND, (name, stat)
            assert comp <= 1e-7, (name, comp)
        assert n_ok > 0, name
        for kind, cap in (("stationarity", ORACLE_BOUND), ("primal", 1e-10)):
            got, rec = both[kind][name], recs[kind][name]
            print(f"oracle {kind} {name}: {got:.2e} (record {rec:.2e}), {n_ok} OK")
            assert 0.0 < got <= cap and 0.0 < rec <= cap, (name, kind, got, rec)
            assert got <= 2.0 * rec and got >= 0.01 * rec, (name, kind, got, rec)


# 2 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,median", zip(FTD.COLD_TB, (0.3, 0.04, 0.1)))
def test_the_certificate_sees_the_task(name, median):
    """Certified against the QP without the task's two changes to H and g, the oracle's own x and multipliers fail:
    measured, a median residual of 0.6 / 0.08 / 0.2 on the three sets (half of that is asserted) and at least 4.4e-3
    on every robot of straight_5 (4e-3 is asserted), nine orders over the GPU bound."""
    bound = FTD.gpu_bound(name)
    res = []
    for c in FTD.controllers(name):
        if c.qp_status != W.QP_OK:
            continue
        d = FD.lsq_duals48(c, c.qp_solution)
        assert FD.certificate48(c, c.qp_solution, d)[1] <= bound
        res.append(FD.certificate48(FTD.without_task(c), c.qp_solution, d)[1])
    print(f"{name}: without the task's H and g the residual is {min(res):.2e} .. {max(res):.2e}, median {np.median(res):.2e}")
    assert np.median(res) >= median, (name, np.median(res))
    if name.startswith("straight"):
        assert min(res) >= 4e-3, res


@pytest.mark.parametrize("name", FTD.COLD_TB)
def test_the_certificate_has_teeth(name):
    """With entries 40..47 zeroed the stationarity residual is at least 2.0e-2 on every robot that has a non-zero force
    multiplier (measured 2.06e-2 / 3.09e-2 / 1.46e-1); one multiplier scaled by 1 + 1e-6 puts the residual above the
    GPU test's bound of the set."""
    bound = FTD.gpu_bound(name)
    dropped, scaled = [], []
    for b, c in enumerate(FTD.controllers(name)):
        if not FD.has_force_multiplier(c):
            continue
        x = c.qp_solution
        d = FD.lsq_duals48(c, x)
        assert FD.certificate48(c, x, d)[1] <= bound, b
        d0 = d.copy()
        d0[FD.DUAL_LEN:] = 0.0
        dropped.append(FD.certificate48(c, x, d0)[1])
        assert dropped[-1] >= 2.0e-2, (name, b, dropped[-1])
        d2 = d.copy()
        r = FD.DUAL_LEN + int(np.argmax(d[FD.DUAL_LEN:]))
        d2[r] *= 1.0 + 1e-6
        scaled.append(FD.certificate48(c, x, d2)[1])
        assert scaled[-1] > bound, (name, b, scaled[-1], bound)
    print(f"{name}: {len(dropped)} robots with a force multiplier; the eight dropped: residual {min(dropped):.2e} .. "
          f"{max(dropped):.2e}; one scaled by 1 + 1e-6: {min(scaled):.1e} .. {max(scaled):.1e} (bound {bound:.1e})")


# 3 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_ok,n_force,n_indep,n_any_alone", [("stance_cold_64", 64, 51, 43, 28), ("rl_random_61", 61, 45, 40, 52),
                                                                   ("straight_5", 5, 3, 3, 4)])
def test_gpu_sets_have_multipliers(name, n_ok, n_force, n_indep, n_any_alone):
    """Measured on the oracle, asserted exactly: OK robots; under task + bounds the robots with a force multiplier and,
    of those, the robots whose priced rows (tests/test_gpu_force_duals.py's 1e-9 significance filter) are independent;
    under the task alone no robot with a force multiplier and the robots with any multiplier (the same filter)."""
    sig = lambda v: np.abs(v) > 1e-9 * (1.0 + np.abs(v).max())
    cs = [c for c in FTD.controllers(name + "_tb") if c.qp_status == W.QP_OK]
    ds = [FD.lsq_duals48(c, c.qp_solution) for c in cs]
    have = sum(bool(d[FD.DUAL_LEN:].any()) for d in ds)
    indep = sum(bool(sig(d)[FD.DUAL_LEN:].any() and FD.active_rows_independent(c, np.where(sig(d), d, 0.0))) for c, d in zip(cs, ds))
    alone = [c for c in FTD.controllers(name + "_t") if c.qp_status == W.QP_OK]
    da = np.array([FD.lsq_duals48(c, c.qp_solution) for c in alone])
    print(f"{name}: {len(cs)} OK, {have} with a force multiplier, {indep} of them with independent priced rows; the task alone: "
          f"{int(da[:, FD.DUAL_LEN:].any(axis=1).sum())} with a force multiplier, {sum(bool(sig(d).any()) for d in da)} with any")
    assert (len(cs), have, indep) == (n_ok, n_force, n_indep)
    assert len(alone) == n_ok and not da[:, FD.DUAL_LEN:].any()
    assert sum(bool(sig(d).any()) for d in da) == n_any_alone  # (the least-squares fit leaves 1e-12 on rows that do not bind)


def test_stateful_sets_have_what_the_gpu_tests_need():
    """The ramp and every off-trot run carry force multipliers; the direct-point set's every robot-cycle ends on one or
    two priced rows, one of them a force row, under a weight other than 1."""
    for name in (FTD.RAMP_SET, *FTD.OFFTROT_SETS):
        ok = [c for c in FTD.controllers(name) if c.qp_status == W.QP_OK]
        n = sum(FD.has_force_multiplier(c) for c in ok)
        print(f"{name}: {n} of {len(ok)} OK robot-cycles with a force multiplier")
        assert 4 * n >= len(ok) > 0, (name, n, len(ok))
    _, t, _, cycles = FTD.direct_point_set()
    assert np.all(t[:, FT.FT_WEIGHT] != 1.0) and t[:, :12].any(axis=1).sum() >= 7  # (table(48, 11)'s rows b % 8 = 1 have fref = 0)
    for row in cycles:
        for c in row:
            nz = np.nonzero(FD.lsq_duals48(c, c.qp_solution))[0]
            assert c.qp_status == W.QP_OK and 1 <= len(nz) <= 2 and nz.max() >= 40, nz


# 4 ----------------------------------------------------------------------------------------------
def test_names_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert int(re.search(r"#define WBC_DUALS_TASK (\d+)u", hdr).group(1)) == _capi.DUALS_TASK == 8192
    assert int(re.search(r"#define WBC_DUALS_FORCE (\d+)u", hdr).group(1)) == _capi.DUALS_FORCE == 4096
    assert int(re.search(r"WBC_DUAL_FORCE_LEN = (\d+)", hdr).group(1)) == _capi.DUAL_FORCE_LEN == 48
    flags = [int(v) for v in re.findall(r"#define WBC_[A-Z_]+ (\d+)u", hdr)]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)  # one bit each, none shared
    assert not re.search(r"wbc_\w*task_duals", hdr)  # no new getter: the 48 are read through the force-duals ones
    import quadrupedwholebodycontroller_amd as pkg
    assert pkg.DUALS_TASK == 8192 and "DUALS_TASK" in pkg.__all__
    assert sorted(_capi.FORCE_DUAL_SYMBOLS) == ["wbc_device_force_duals", "wbc_get_force_duals"]


def test_makefile_lists_and_library_symbols():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    ktu = re.search(r"^KTU := (.*)$", mk, re.M).group(1).split()
    at = ktu.index("ftd0")
    assert ktu[at:at + 4] == ["ftd0", "ftd1", "ft0", "ft1"] and ktu[at - 1] == "lm1", ktu
    flags = lambda v: re.search(rf"^{v} := (.*)$", mk, re.M).group(1).split()
    assert flags("FTD0_KFLAGS") == flags("FN0_KFLAGS") and flags("FTD1_KFLAGS") == flags("FN0_KFLAGS")
    assert "KFLAGS_ftd0 = $(FTD0_KFLAGS)" in mk and "KFLAGS_ftd1 = $(FTD1_KFLAGS)" in mk
    for u in ("ftd0", "ftd1"):
        src = open(os.path.join(CSRC, f"wbc_kernel_{u}.hip")).read()
        assert f"#define WBC_STEP_LAUNCHER wbc_launch_update_solve_{u}\n" in src and "#define WBC_STEP_DUALS 1\n" in src
        assert f"#define WBC_STEP_INSTANCE {u[-1]}, false, true, true, true, true, true, true " in src
    eng = open(os.path.join(CSRC, "wbc_engine.cpp")).read()
    assert "wbc_launch_update_solve_ftd1 : wbc_launch_update_solve_ftd0" in eng
    assert "WBC_STEP_UNITS_FTD" not in eng  # picked by the flag, not in a numbered list
    lib = os.path.join(ROOT, "quadrupedwholebodycontroller_amd", "libwbc_hip.so")
    assert os.path.exists(lib), "libwbc_hip.so is not built (run __graft_entry__.build())"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for s in ("wbc_launch_update_solve_ftd0", "wbc_launch_update_solve_ftd1", "wbc_get_force_duals", "wbc_device_force_duals"):
        assert re.search(rf" T {s}$", syms, re.M), s


PROG = r"""
#include <cstdio>
#include <cstring>
#include "wbc.h"
#include "wbc_layout.h"
int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "names")) {
        std::printf("%u %u %u %d\n", (unsigned)WBC_DUALS, (unsigned)WBC_DUALS_FORCE, (unsigned)WBC_DUALS_TASK, (int)WBC_DUAL_FORCE_LEN);
        return 0;
    }
    // "refused": lines of STF nwaves stateful modes rp cn bb lm fn ft (pointers: 0 = null): the argument check of the
    // ftd launchers, step_args_refused with their WBC_STEP_INSTANCE (STF, false, and all six table flags)
    int stf, nwaves, stateful, modes, prp, pcn, pbb, plm, pfn, pft;
    static const double tab[28] = {0};
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d", &stf, &nwaves, &stateful, &modes, &prp, &pcn, &pbb, &plm, &pfn, &pft) == 10) {
        wbc::KernelArgs a;
        std::memset(&a, 0, sizeof(a));
        a.nwaves = nwaves;
        a.stateful = stateful;
        a.modes = modes;
        a.rp = prp ? tab : nullptr;
        a.cn = pcn ? tab : nullptr;
        a.bb = pbb ? tab : nullptr;
        a.lm = plm ? tab : nullptr;
        a.fn = pfn ? tab : nullptr;
        a.ft = pft ? tab : nullptr;
        std::printf("%d\n", (int)wbc::step_args_refused(stf, false, true, true, true, true, true, true, a));
    }
    return 0;
}
"""


def test_flag_and_launcher_argument_check_host(tmp_path):
    """A stand-alone host program (address and undefined-behaviour sanitizers where the toolchain links them): the
    header's three duals flags, and the ftd launchers' argument check: refused without waves, on the other STF, under
    mode hypotheses, and without any of the parameter, normal, base-body, force-bound and force-task tables (the
    engine supplies its own); a null limits table is accepted."""
    exe = build_host_program(tmp_path, "ftd", PROG)
    assert [int(v) for v in run_host_program(exe, "names")[0]] == [2048, 4096, 8192, 48]
    import itertools
    cases = [(stf, n, s, m, *p) for stf in (0, 1) for n in (0, 3) for s in (0, 1) for m in (0, 4) for p in itertools.product((0, 1), repeat=6)]
    got = run_host_program(exe, "refused", "".join(" ".join(map(str, c)) + "\n" for c in cases))
    assert len(got) == len(cases)
    n_ok = 0
    for (stf, n, s, m, rp, cn, bb, lm, fn, ft), g in zip(cases, got):
        want = n <= 0 or s != stf or m != 0 or not (rp and cn and bb and fn and ft)
        assert int(g[0]) == int(want), (stf, n, s, m, rp, cn, bb, lm, fn, ft)
        n_ok += not want
    assert n_ok == 4  # each STF with and without a limits table


# 5 ----------------------------------------------------------------------------------------------
def callee_frame(asm):
    """The ScratchSize the compiler prints behind the unit's drain_fallbacks (bytes per lane)."""
    body = asm[asm.index("\n_ZN3wbc15drain_fallbacks"):]
    return int(re.search(r"^; ScratchSize: (\d+)", body, re.M).group(1))


@pytest.mark.parametrize("unit,var,kernel", [
    ("ftd0", "FTD0_KFLAGS", "wbc_update_solve_duals_kernelILi0ELb0ELb1ELb1ELb1ELb1ELb1ELb1E"),
    ("ftd1", "FTD1_KFLAGS", "wbc_update_solve_duals_kernelILi1ELb0ELb1ELb1ELb1ELb1ELb1ELb1E"),
])
def test_new_units_resources(unit, var, kernel):
    """The compiler's resource report of the force-task duals units: 256 VGPRs at the most, 40 272 B of LDS (ft0's), one
    wave per SIMD, no scratch instruction in the kernel's own body, the unit holding its kernel and one drain_fallbacks
    of its own tag (24 / 25); the fallback callee's frame (the ScratchSize the compiler prints behind drain_fallbacks)
    at most ft0's callee's, read from the compiler here, + 64 B (DESIGN.md 23's allowance).  Measured: ft0 956 B, ftd0
    and ftd1 1020 B.  The kernel's own figure is the callee's plus what the kernel reserves itself: 0 B in ft0 and
    ftd0, 48 B in ftd1 (1068 B in all), which no instruction of its body touches; it is held to the same 48 B."""
    with ThreadPoolExecutor(2) as ex:
        (new, asm), (old, old_asm) = ex.map(lambda a: report(*a), [(unit, var), ("ft0", "FT0_KFLAGS")])
    assert len(new) == 1 and len(old) == 1, (list(new), list(old))
    (name, rep), (oname, ref) = next(iter(new.items())), next(iter(old.items()))
    assert kernel in name and "wbc_update_solve_kernelILi0E" in oname, (name, oname)
    print(unit, rep, "against ft0", ref)
    assert rep["VGPRs"] <= 256 and rep["VGPRs"] + rep["AGPRs"] <= 512, rep
    assert rep["LDS Size [bytes/block]"] == ref["LDS Size [bytes/block]"] == 40272, (rep, ref)
    assert rep["Occupancy [waves/SIMD]"] == ref["Occupancy [waves/SIMD]"] == 1, (rep, ref)
    frame, ref_frame = callee_frame(asm), callee_frame(old_asm)
    print(unit, "callee frame", frame, "ft0's", ref_frame)
    assert ref_frame == ref["ScratchSize [bytes/lane]"], (ref_frame, ref)
    assert frame <= ref_frame + 64, (frame, ref_frame)
    assert frame <= rep["ScratchSize [bytes/lane]"] <= frame + 48, (frame, rep)
    starts = [l.split(":")[0] for l in asm.split("\n") if re.match(r"^_Z\w+:", l)]
    assert len(starts) == 2 and sum("drain_fallbacks" in n for n in starts) == 1, starts
    assert any(f"drain_fallbacksILi{24 + int(unit[-1])}E" in n for n in starts), starts
    body = asm[asm.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    assert not re.search(r"^\s+scratch_", body, re.M), re.findall(r"^\s+scratch_\S+", body, re.M)[:4]
