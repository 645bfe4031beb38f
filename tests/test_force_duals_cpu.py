"""CPU: the 48 QP multipliers of the default step under per-foot normal-force bounds (wbc_step with
WBC_DUALS_FORCE).

  * the 74-row certificate of tests/force_duals_oracle.py on the numpy oracle's own x with least-squares
    multipliers: the residuals per input set, held against the committed record
    profiles/force_duals/oracle_residuals.json (what the GPU test's bounds are set from);
  * the certificate has teeth: without the eight force multipliers, or with one multiplier off by 1e-6, it fails;
  * the GPU test's input sets have what it needs so that it cannot pass with no force row active;
  * the boundary: dual_rows on 40 and 48 entries, constants, symbols, the Makefile's unit list and the compiler's
    resource report of the two new kernel units.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import force_duals_oracle as FD
import wbc_np as W
from quadrupedwholebodycontroller_amd import _capi, dual_rows
from unit_reports import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrupedwholebodycontroller_amd", "csrc")
# as tests/test_duals_cpu.py: an fp64 least-squares fit of a few dozen multipliers to 42 equations whose entries
# reach 1e2-1e4 beside a gradient normalised to O(1); 1e-11 is 60 x the worst measured (1.5e-13) and far below the
# 2e-2 that a missing force multiplier leaves
ORACLE_BOUND = 1e-11


# 1 ----------------------------------------------------------------------------------------------
def test_certificate_on_the_oracles_own_x():
    """Every set (the three cold sets under table(B, 7), the five-table set, every cycle of the ramp): primal
    feasible, stationary to rounding, complementary at the oracle's own activity threshold, and the worst figures
    per set within 2 x the committed record (and not 100 x below it: a record of another quantity would be)."""
    both, recs = FD.measure(), {k: FD.record(k) for k in FD.KINDS}
    assert all(sorted(both[k]) == sorted(recs[k]) == sorted(FD.ALL_SETS) for k in FD.KINDS)
    for name in FD.ALL_SETS:
        n_ok = 0
        for c in FD.controllers(name):
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
@pytest.mark.parametrize("name", FD.COLD_SETS)
def test_the_certificate_has_teeth(name):
    """With entries 40..47 zeroed the stationarity residual is at least 1e-3 on every robot that has a non-zero
    force multiplier (measured: 2.1e-2 and more); one multiplier scaled by 1 + 1e-6 puts the residual above the
    GPU test's bound of the set."""
    bound = FD.gpu_bound(name)
    dropped, scaled = [], []
    for b, c in enumerate(FD.controllers(name)):
        if not FD.has_force_multiplier(c):
            continue
        x = c.qp_solution
        d = FD.lsq_duals48(c, x)
        assert FD.certificate48(c, x, d)[1] <= bound, b
        d0 = d.copy()
        d0[FD.DUAL_LEN:] = 0.0
        dropped.append(FD.certificate48(c, x, d0)[1])
        assert dropped[-1] >= 1e-3, (name, b, dropped[-1])
        d2 = d.copy()
        r = FD.DUAL_LEN + int(np.argmax(d[FD.DUAL_LEN:]))
        d2[r] *= 1.0 + 1e-6
        scaled.append(FD.certificate48(c, x, d2)[1])
        assert scaled[-1] > bound, (name, b, scaled[-1], bound)
    print(f"{name}: {len(dropped)} robots with a force multiplier; the eight dropped: residual {min(dropped):.1e} .. "
          f"{max(dropped):.1e}; one scaled by 1 + 1e-6: {min(scaled):.1e} .. {max(scaled):.1e} (bound {bound:.1e})")


# 3 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_ok,n_min", [("stance_cold_64", 64, 50), ("rl_random_61", 61, 40), ("straight_5", 5, 3)])
def test_gpu_sets_have_force_multipliers(name, n_ok, n_min):
    """OK robots, and robots with a non-zero force multiplier (measured 53, 46, 3); on the first two sets both
    sides occur (measured 23 / 77 and 13 / 77 rows at fn_min / fn_max)."""
    cs = FD.controllers(name)
    ok = [c for c in cs if c.qp_status == W.QP_OK]
    ds = np.array([FD.lsq_duals48(c, c.qp_solution) for c in ok])
    have = int(np.any(ds[:, FD.DUAL_LEN:] != 0.0, axis=1).sum())
    lo, hi = int((ds[:, FD.DUAL_LEN::2] != 0).sum()), int((ds[:, FD.DUAL_LEN + 1::2] != 0).sum())
    print(f"{name}: {len(ok)} OK, {have} with a force multiplier, rows at fn_min {lo}, at fn_max {hi}, largest {ds[:, FD.DUAL_LEN:].max():.3g}")
    assert len(ok) == n_ok and have >= n_min, (len(ok), have)
    if name != "straight_5":
        assert lo > 0 and hi > 0, (lo, hi)


def test_ramp_and_five_tables_have_force_multipliers():
    """On the ramp at least half of the OK robot-cycles carry a force multiplier; the five-table set at least four
    robots (as many as tests/test_gpu_force_bounds.py asks to have a tight bound)."""
    ok = [c for c in FD.controllers(FD.RAMP_SET) if c.qp_status == W.QP_OK]
    n = sum(FD.has_force_multiplier(c) for c in ok)
    print(f"ramp: {n} of {len(ok)} OK robot-cycles with a force multiplier")
    assert len(ok) > 8 * 130 // 2 and 2 * n >= len(ok), (n, len(ok))
    assert sum(FD.has_force_multiplier(c) for c in FD.controllers(FD.TABLES_SET)) >= 4


# 4 ----------------------------------------------------------------------------------------------
def test_dual_rows_on_40_and_48_entries():
    B = 3
    d = np.zeros((B, 48))
    d[0, 4 * 2 + 1] = 2.0          # leg 2, face 1
    d[1, 16 + 2 * 11 + 1] = 4.0    # joint 11 at its upper bound
    d[1, 40 + 2 * 3] = 5.0         # foot 3 at fn_min
    d[2, 40 + 2 * 1 + 1] = 6.0     # foot 1 at fn_max
    r = dual_rows(d)
    assert sorted(r) == ["force", "friction", "torque"]
    assert r["friction"].shape == (B, 4, 4) and r["torque"].shape == (B, 12) and r["force"].shape == (B, 4)
    assert r["friction"][0, 2, 1] == 2.0 and r["friction"].sum() == 2.0
    assert r["torque"][1, 11] == -4.0 and np.abs(r["torque"]).sum() == 4.0  # the force entries stay out of the torques
    assert r["force"][1, 3] == 5.0 and r["force"][2, 1] == -6.0 and np.abs(r["force"]).sum() == 11.0
    r40 = dual_rows(d[:, :40])
    assert sorted(r40) == ["friction", "torque"]
    assert np.array_equal(r40["friction"], r["friction"]) and np.array_equal(r40["torque"], r["torque"])
    # the signed entries are qpOASES' multipliers of the two-sided rows
    for c in FD.controllers("straight_5"):
        d1 = FD.lsq_duals48(c, c.qp_solution)
        y = FD.expand48(c, c.qp_solution, d1)
        rr = dual_rows(d1[None])
        assert np.array_equal(rr["force"][0], y[70:74]) and np.array_equal(rr["torque"][0], y[34:46])
        assert np.array_equal(rr["friction"][0].ravel(), -y[18:34])
    for bad in (np.zeros(48), np.zeros((2, 47)), np.zeros((2, 41)), np.zeros((2, 4, 12))):
        with pytest.raises(ValueError, match="need shape"):
            dual_rows(bad)


def test_names_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert int(re.search(r"#define WBC_DUALS_FORCE (\d+)u", hdr).group(1)) == _capi.DUALS_FORCE == 4096
    assert int(re.search(r"WBC_DUAL_FORCE_LEN = (\d+)", hdr).group(1)) == _capi.DUAL_FORCE_LEN == FD.DUAL_FORCE_LEN == 48
    assert int(re.search(r"WBC_DUAL_LEN = (\d+)", hdr).group(1)) == _capi.DUAL_LEN == 40 and _capi.DUALS == 2048
    flags = [int(v) for v in re.findall(r"#define WBC_[A-Z_]+ (\d+)u", hdr)]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)  # one bit each, none shared
    for s in ("wbc_get_force_duals", "wbc_device_force_duals"):
        assert s in _capi.C_API_SYMBOLS and s in _capi.FORCE_DUAL_SYMBOLS and re.search(rf"int32_t {s}\(", hdr)
    import quadrupedwholebodycontroller_amd as pkg
    assert pkg.DUALS_FORCE == 4096 and pkg.DUAL_FORCE_LEN == 48
    assert callable(pkg.Engine.force_duals) and callable(pkg.Engine.device_force_duals)


def test_makefile_lists_and_library_symbols():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    ktu = re.search(r"^KTU := (.*)$", mk, re.M).group(1).split()
    assert ktu[-4:] == ["fnd0", "fnd1", "fn0", "fn1"] and ktu[-6:-4] == ["lmd0", "lmd1"], ktu
    flags = lambda v: re.search(rf"^{v} := (.*)$", mk, re.M).group(1).split()
    assert flags("FND0_KFLAGS") == flags("FN0_KFLAGS") and flags("FND1_KFLAGS") == flags("FN0_KFLAGS")
    assert "KFLAGS_fnd0 = $(FND0_KFLAGS)" in mk and "KFLAGS_fnd1 = $(FND1_KFLAGS)" in mk
    lib = os.path.join(ROOT, "quadrupedwholebodycontroller_amd", "libwbc_hip.so")
    assert os.path.exists(lib), "libwbc_hip.so is not built (run __graft_entry__.build())"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for s in ("wbc_get_force_duals", "wbc_device_force_duals", "wbc_launch_update_solve_fnd0", "wbc_launch_update_solve_fnd1"):
        assert re.search(rf" T {s}$", syms, re.M), s


# 5 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,var,kernel", [
    ("fnd0", "FND0_KFLAGS", "wbc_update_solve_duals_kernelILi0ELb0ELb1ELb1ELb1ELb1ELb1E"),
    ("fnd1", "FND1_KFLAGS", "wbc_update_solve_duals_kernelILi1ELb0ELb1ELb1ELb1ELb1ELb1E"),
])
def test_new_units_resources(unit, var, kernel):
    """The compiler's resource report of the force-bound duals units: at most 256 VGPRs, at most 40 960 B of LDS
    (four workgroups per CU), one wave per SIMD, no scratch instruction in the kernel's own body, the unit holding
    its kernel and one drain_fallbacks; the report's scratch figure (the fallback callee's frame) at most fn0's,
    read from the compiler here, + 64 B (du0 over bb0 was + 24 B)."""
    with ThreadPoolExecutor(2) as ex:
        (new, asm), (old, _) = ex.map(lambda a: report(*a), [(unit, var), ("fn0", "FN0_KFLAGS")])
    assert len(new) == 1 and len(old) == 1, (list(new), list(old))
    (name, rep), (oname, ref) = next(iter(new.items())), next(iter(old.items()))
    assert kernel in name and "wbc_update_solve_kernelILi0E" in oname, (name, oname)
    print(unit, rep, "against fn0", ref)
    assert rep["VGPRs"] <= 256 and rep["VGPRs"] + rep["AGPRs"] <= 512, rep
    assert rep["LDS Size [bytes/block]"] <= 40960, rep
    assert rep["Occupancy [waves/SIMD]"] == ref["Occupancy [waves/SIMD]"] == 1, (rep, ref)
    assert rep["ScratchSize [bytes/lane]"] <= ref["ScratchSize [bytes/lane]"] + 64, (rep, ref)
    starts = [l.split(":")[0] for l in asm.split("\n") if re.match(r"^_Z\w+:", l)]
    assert len(starts) == 2 and sum("drain_fallbacks" in n for n in starts) == 1, starts
    body = asm[asm.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    assert not re.search(r"^\s+scratch_", body, re.M), re.findall(r"^\s+scratch_\S+", body, re.M)[:4]
