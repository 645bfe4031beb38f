"""CPU: the per-robot base body (wbc_set_base_body, include/wbc.h): its oracles
(tests/base_body_oracle.py: the numpy and C oracles given one model per robot), the payload composite
(base_body_with_payload), the Python table forms (base_body_table, what Engine.set_base_body passes to
wbc_set_base_body) with each validation error, the host functions of wbc_layout.h (bb_bad_entry, the
instance choice and the argument check of the three new units) in a stand-alone program, and the
compiler's resource report of the units (wbc_kernel_bb0.hip, wbc_kernel_bb1.hip, wbc_kernel_bbs.hip).

wbc_set_base_body validates on the host too, but it needs an engine and an engine needs a device: that
validation's test is tests/test_gpu_base_body.py's."""
import itertools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import base_body_oracle as BB
import wbc_np as W
import wbc_ref as R
from quadrupedwholebodycontroller_amd import _capi, base_body_row, base_body_table, base_body_with_payload, workloads
from unit_reports import build_host_program, report, run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tau", "grf", "x", "status", "iters")


def test_names_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert int(re.search(r"WBC_BB_LEN = (\d+)", hdr).group(1)) == _capi.BB_LEN == _capi.TABLES["base_body"] == 14
    for name, col in (("MASS", _capi.BB_MASS), ("COM", _capi.BB_COM), ("INERTIA", _capi.BB_INERTIA)):
        assert int(re.search(rf"WBC_BB_{name} = (\d+)", hdr).group(1)) == col
    for s in ("wbc_set_base_body", "wbc_bind_device_base_body", "wbc_get_base_body"):
        assert s in _capi.C_API_SYMBOLS and re.search(rf"int32_t {s}\(", hdr)


# 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stance_cold", "rl_random"])
def test_default_row_is_the_stock_oracles(name):
    B = 8
    inp = getattr(workloads, name)(B, seed=91)
    rows = np.tile(BB.default_row(), (B, 1))
    stock = W.run_batch(inp["base_pose"], inp["nu"], inp["qj"], inp["ref"], inp["contacts"], inp["switching"])
    mine = BB.np_run_batch(inp, rows)
    for k in KEYS:
        assert np.array_equal(mine[k], stock[k]), ("numpy", k)
    for method in (R.LITERAL, R.REDUCED):
        stock, mine = R.run_batch(inp, method=method), BB.c_run_batch(inp, rows, method)
        for k in KEYS:
            assert np.array_equal(mine[k], stock[k]), ("C", method, k)


# 2 ----------------------------------------------------------------------------------------------
def _two_body(m0, c0, I0, mp, p, Ip):
    """Mass, CoM and inertia about the CoM of two rigid bodies, from first principles: the inertia of
    each about the origin (its own plus its mass at its CoM), summed, then moved to the composite CoM."""
    def about_origin(m, c, I):
        return I + m * ((c @ c) * np.eye(3) - np.outer(c, c))
    M = m0 + mp
    c = (m0 * c0 + mp * p) / M
    IO = about_origin(m0, c0, I0) + about_origin(mp, p, Ip)
    return M, c, IO - M * ((c @ c) * np.eye(3) - np.outer(c, c))


def test_payload_composite_against_two_bodies():
    model = R.model_params()[0]
    base = base_body_row(model)
    m0, c0, I0 = base[0], base[1:4], base[4:13].reshape(3, 3)
    g = np.random.default_rng(3)
    N = 32
    mass = g.uniform(0.0, 0.6, N) * m0
    pos = g.uniform(BB.PAYLOAD_LO, BB.PAYLOAD_HI, (N, 3))
    A = g.normal(size=(N, 3, 3))
    Ip = 0.05 * np.einsum("nij,nkj->nik", A, A)
    for inertia in (None, Ip):
        rows = base_body_with_payload(model, mass, pos, inertia)
        assert rows.shape == (N, 14) and not rows[:, 13].any()
        base_body_table(N, model, rows)  # every composite is a valid row
        for n in range(N):
            M, c, I = _two_body(m0, c0, I0, mass[n], pos[n], np.zeros((3, 3)) if inertia is None else Ip[n])
            assert abs(rows[n, 0] - M) <= 1e-15 * M
            assert np.abs(rows[n, 1:4] - c).max() <= 1e-15 * max(1.0, np.abs(c).max())
            assert np.abs(rows[n, 4:13].reshape(3, 3) - I).max() <= 1e-14 * np.trace(I)
            one = base_body_with_payload(model, mass[n], pos[n], None if inertia is None else Ip[n])
            assert one.shape == (14,) and np.array_equal(one, rows[n])  # vectorised = one at a time
    # no payload: the model's own row, bit for bit, wherever the (absent) payload sits
    assert np.array_equal(base_body_with_payload(model, 0.0, [0.2, -0.1, 0.15]), base)
    assert np.array_equal(base_body_with_payload(model, np.zeros(5), pos[:5]), np.tile(base, (5, 1)))
    assert np.array_equal(BB.payload_rows(4, frac=0.0), np.tile(base, (4, 1)))
    rows = BB.payload_rows(16)
    assert rows.shape == (16, 14) and np.all(rows[:, 0] >= m0) and np.all(rows[:, 0] <= 1.6 * m0)
    assert np.array_equal(rows, BB.payload_rows(16))


# 3 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stance_cold", "rl_random"])
def test_payload_oracles_agree(name):
    """B = 16 under payload_rows: numpy LITERAL against C LITERAL against C REDUCED, at the bounds of
    tests/test_oracle_reduced.py (x 1e-9 and tau 1e-8 between the numpy forms; tau / grf 1e-7 and x 1e-8
    between the C forms), the numpy and the C LITERAL at the tighter of each; the oracle's mass matrix
    carries the row's mass; and the payload matters."""
    B = 16
    inp = getattr(workloads, name)(B, seed=91)
    rows = BB.payload_rows(B)
    npy, lit, red = BB.np_run_batch(inp, rows), BB.c_run_batch(inp, rows, R.LITERAL), BB.c_run_batch(inp, rows, R.REDUCED)
    assert np.all(lit["status"] == W.QP_OK) and np.array_equal(npy["status"], lit["status"]) and np.array_equal(red["status"], lit["status"])
    worst = {}
    for what, a, b, tols in (("numpy vs C literal", npy, lit, dict(tau=1e-8, grf=1e-7, x=1e-9)),
                             ("C reduced vs C literal", red, lit, dict(tau=1e-7, grf=1e-7, x=1e-8))):
        for k, tol in tols.items():
            err = max(np.abs(a[k][r] - b[k][r]).max() / (1.0 + np.abs(b[k][r]).max()) for r in range(B))
            worst[what, k] = err
            assert err <= tol, (what, k, err)
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    plain = R.run_batch(inp)
    moved = np.abs(lit["tau"] - plain["tau"]).max(axis=1)
    print(f"{name}: payload moves tau by {moved.min():.3g} .. {moved.max():.3g} N m")
    assert (moved > 1e-3).sum() >= B - 1
    links = BB.MODEL.mass.sum()
    for b in range(B):
        kd = W.KinDyn(BB.np_model(rows[b]), inp["base_pose"][b], inp["nu"][b], inp["qj"][b])
        total = rows[b, 0] + links
        assert np.abs(kd.M[:3, :3] - total * np.eye(3)).max() <= 1e-12 * total, b
        assert abs(BB.np_model(rows[b]).total_mass - total) <= 1e-13 * total
        assert abs(BB.c_model(rows[b]).total_mass - BB.np_model(rows[b]).total_mass) == 0.0


# 4 ----------------------------------------------------------------------------------------------
def test_table_forms_and_validation():
    B = 5
    model = R.model_params()[0]
    base = base_body_row(model)
    rows = BB.payload_rows(B)
    t = base_body_table(B, model, rows)
    assert t.shape == (B, 14) and t.flags["C_CONTIGUOUS"] and np.array_equal(t, rows)
    assert np.array_equal(base_body_table(B, model, rows[2]), np.tile(rows[2], (B, 1)))
    assert np.array_equal(base_body_table(B, model, {}), np.tile(base, (B, 1)))
    r2 = rows.copy()
    r2[:, 13] = np.nan  # the reserved column is ignored on input and written as 0
    assert np.array_equal(base_body_table(B, model, r2), rows)
    # the dict form: one value or per-robot values, missing entries from the model
    d = base_body_table(B, model, {"mass": 20.0})
    assert np.all(d[:, 0] == 20.0) and np.array_equal(d[:, 1:], np.tile(base[1:], (B, 1)))
    d = base_body_table(B, model, {"mass": rows[:, 0], "com": rows[:, 1:4], "inertia": rows[:, 4:13].reshape(B, 3, 3)})
    assert np.array_equal(d, rows)
    d = base_body_table(B, model, {"com": [0.01, 0.0, 0.05], "inertia": rows[1, 4:13]})
    assert np.all(d[:, 0] == base[0]) and np.all(d[:, 1:4] == [0.01, 0.0, 0.05]) and np.array_equal(d[:, 4:13], np.tile(rows[1, 4:13], (B, 1)))
    assert np.array_equal(base_body_table(B, model, {"inertia": rows[:, 4:13]})[:, 4:13], rows[:, 4:13])
    for bad_shape in (rows[:4], rows[:, :13], np.ones(13), np.ones((B, 2, 7))):
        with pytest.raises(ValueError, match="need shape"):
            base_body_table(B, model, bad_shape)
    with pytest.raises(ValueError, match="unknown base body entries"):
        base_body_table(B, model, {"weight": 1.0})
    for key, v in (("mass", np.ones(B + 1)), ("com", np.ones((B, 2))), ("inertia", np.ones((B, 3))), ("mass", np.ones((B, 1)))):
        with pytest.raises(ValueError, match=f"base body {key}: need"):
            base_body_table(B, model, {key: v})
    # every validation error, naming row and column
    I = rows[0, 4:13].reshape(3, 3)
    asym = I.copy()
    asym[0, 2] += 1e-6 * np.trace(I)
    indef = I.copy()
    indef[1, 1] = -indef[1, 1]
    flat = np.diag([1.0, 1.0, 0.0]) @ I @ np.diag([1.0, 1.0, 0.0])
    offd = I.copy()
    offd[0, 1] = offd[1, 0] = 1.5 * np.sqrt(I[0, 0] * I[1, 1])
    cases = [(0, np.nan, 0, "mass"), (0, 0.0, 0, "mass"), (0, -1.0, 0, "mass"), (2, np.inf, 2, "com_y"), (9, np.nan, 9, "I_yz")]
    for b in (0, 3, 4):
        for col, v, bad_col, nm in cases:
            r = rows.copy()
            r[b, col] = v
            with pytest.raises(ValueError, match=rf"row {b}, column {bad_col} \({nm}\)"):
                base_body_table(B, model, r)
        for mat, bad_col, nm in ((asym, 6, "I_xz"), (indef, 8, "I_yy"), (flat, 12, "I_zz"), (offd, 8, "I_yy"), (-I, 4, "I_xx")):
            r = rows.copy()
            r[b, 4:13] = mat.ravel()
            assert _capi.base_body_bad_entry(r[b]) == bad_col
            with pytest.raises(ValueError, match=rf"row {b}, column {bad_col} \({nm}\)"):
                base_body_table(B, model, r)
    ok = I.copy()
    ok[0, 2] += 0.5e-9 * np.trace(I)  # inside the symmetry tolerance
    r = rows.copy()
    r[1, 4:13] = ok.ravel()
    base_body_table(B, model, r)


# 5 ----------------------------------------------------------------------------------------------
PROG = r"""
#include <cstdio>
#include <cstring>
#include "wbc_layout.h"
int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "names")) {
#define X(unit) std::printf("%d " #unit "\n", (int)wbc::STEP_##unit);
        WBC_STEP_UNITS(X)
        WBC_STEP_UNITS_BB(X)
#undef X
        std::printf("%d count\n%d all\n", (int)wbc::STEP_INSTANCES, (int)wbc::STEP_ALL_INSTANCES);
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "instance")) {
        for (int i = 0; i < 32; ++i)
            std::printf("%d %d %d %d %d %d %d\n", i >> 4 & 1, i >> 3 & 1, i >> 2 & 1, i >> 1 & 1, i & 1,
                        (int)wbc::step_instance(i >> 3 & 1, i >> 2 & 1, i >> 1 & 1, i & 1, (i >> 4 & 1) != 0),
                        (int)wbc::step_instance(i >> 3 & 1, i >> 2 & 1, i >> 1 & 1, i & 1));
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "rows")) {
        // rows of WBC_BB_LEN doubles in a heap block of exactly that size (the reserved column is the
        // last double: reading past it would be out of bounds)
        double v[WBC_BB_LEN];
        for (;;) {
            for (int c = 0; c < WBC_BB_LEN; ++c)
                if (std::scanf("%lf", &v[c]) != 1) return 0;
            double* row = new double[WBC_BB_LEN - 1];
            std::memcpy(row, v, (WBC_BB_LEN - 1) * sizeof(double));
            std::printf("%d\n", wbc::bb_bad_entry(row));
            delete[] row;
        }
    }
    // "refused": lines of STF SONLY RP CN BB nwaves stateful modes qmap rp cn bb (pointers: 0 = null)
    int stf, sonly, rp, cn, bb, nwaves, stateful, modes, qmap, prp, pcn, pbb;
    static const int32_t map[4] = {0, 0, 0, 0};
    static const double tab[14] = {0};
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &stf, &sonly, &rp, &cn, &bb, &nwaves, &stateful, &modes, &qmap, &prp,
                      &pcn, &pbb) == 12) {
        wbc::KernelArgs a;
        std::memset(&a, 0, sizeof(a));
        a.nwaves = nwaves;
        a.stateful = stateful;
        a.modes = modes;
        a.qmap = qmap ? map : nullptr;
        a.rp = prp ? tab : nullptr;
        a.cn = pcn ? tab : nullptr;
        a.bb = pbb ? tab : nullptr;
        std::printf("%d %d %d\n", (int)wbc::step_args_refused(stf, sonly != 0, rp != 0, cn != 0, a, bb != 0),
                    (int)wbc::step_args_refused(stf, sonly != 0, rp != 0, cn != 0, bb != 0, a),
                    (int)wbc::step_args_refused(stf, sonly != 0, rp != 0, cn != 0, a));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout_bin(tmp_path_factory):
    """The program above, built with the address and undefined-behaviour sanitizers when the host
    toolchain links them (a stand-alone program: nothing is preloaded), else without."""
    return build_host_program(tmp_path_factory.mktemp("base_body"), "b", PROG)


def test_bb_bad_entry_host(layout_bin):
    """wbc_layout.h's predicate over good, NaN, zero-mass, asymmetric and indefinite rows, and equal to the
    Python one (_capi.base_body_bad_entry) on all of them."""
    rows = BB.payload_rows(6)
    I = rows[0, 4:13].reshape(3, 3)
    cases = [(r, -1) for r in rows] + [(BB.default_row(), -1)]

    def edit(col=None, v=None, mat=None):
        r = rows[1].copy()
        if col is not None:
            r[col] = v
        if mat is not None:
            r[4:13] = np.asarray(mat).ravel()
        return r
    cases += [(edit(c, np.nan), c) for c in range(13)] + [(edit(5, np.inf), 5), (edit(13, np.nan), -1)]
    cases += [(edit(0, 0.0), 0), (edit(0, -3.0), 0), (edit(0, 1e-300), -1)]
    for (i, j), col in (((0, 1), 5), ((0, 2), 6), ((1, 2), 9)):
        a = I.copy()
        a[i, j] += 1e-6 * np.trace(I)
        cases.append((edit(mat=a), col))
        a = I.copy()
        a[i, j] += 0.5e-9 * np.trace(I)
        cases.append((edit(mat=a), -1))
    cases += [(edit(mat=-I), 4), (edit(mat=np.diag([1.0, -1.0, 1.0])), 8), (edit(mat=np.diag([1.0, 1.0, 0.0])), 12),
              (edit(mat=np.diag([1.0, 1.0, -2.0])), 12), (edit(mat=np.zeros((3, 3))), 4),
              (edit(mat=[[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), 8),
              (edit(mat=[[1.0, 0.0, 0.9], [0.0, 1.0, 0.9], [0.9, 0.9, 1.0]]), 12)]
    text = "".join(" ".join(repr(float(v)) for v in r) + "\n" for r, _ in cases)
    got = [int(l[0]) for l in run_host_program(layout_bin, "rows", text)]
    assert len(got) == len(cases)
    for (r, want), g in zip(cases, got):
        assert g == want == _capi.base_body_bad_entry(r), (r, want, g)


def test_instance_choice_and_argument_check_with_bb(layout_bin):
    """step_instance with bb names the three new units, whose values go on from STEP_INSTANCES; without it
    (the default) it is what it was.  step_args_refused for the BB instances refuses what their cn
    instance refuses, and a missing base-body table; with BB false (the default) it is what it was."""
    names = {n: int(i) for i, n in run_host_program(layout_bin, "names")}
    assert names.pop("count") == 9 and names.pop("all") == 12
    assert [names[n] for n in ("bb0", "bb1", "bbs")] == [9, 10, 11] and sorted(names.values()) == list(range(12))
    for bb, cn, rp, all_stance, stateful, got, plain in ([int(v) for v in r] for r in run_host_program(layout_bin, "instance")):
        assert 0 <= plain < 9
        if not bb:
            assert got == plain
        elif all_stance and stateful:
            assert 9 <= got < 12  # cannot occur (step_all_stance is false for a stateful step)
        else:
            assert got == names["bbs" if all_stance else "bb1" if stateful else "bb0"], (cn, rp, all_stance, stateful)
    insts = list(itertools.product((0, 1), repeat=5))
    args = [dict(nwaves=n, stateful=s, modes=m, qmap=q, rp=r, cn=c, bb=b)
            for n, s, m, q, r, c, b in itertools.product((-1, 0, 3), (0, 1, 2), (0, 4), (0, 1), (0, 1), (0, 1), (0, 1))]
    text = "".join(" ".join(str(v) for v in (*inst, a["nwaves"], a["stateful"], a["modes"], a["qmap"], a["rp"], a["cn"], a["bb"])) + "\n"
                   for inst in insts for a in args)
    got = iter([int(v) for v in l] for l in run_host_program(layout_bin, "refused", text))
    units = {(0, 0, 1, 1, 1): "bb0", (1, 0, 1, 1, 1): "bb1", (0, 1, 1, 1, 1): "bbs"}
    seen = {u: [0, 0] for u in units.values()}
    for inst in insts:
        stf, sonly, rp, cn, bb = inst
        for a in args:
            trailing, ordered, plain = next(got)
            base = bool(a["nwaves"] <= 0 or bool(a["stateful"]) != bool(stf) or (sonly and (a["modes"] or a["qmap"])) or
                        (rp and (a["modes"] or not a["rp"])) or (cn and not a["cn"]))
            assert plain == int(base), (inst, a)
            assert trailing == ordered == int(base or bool(bb and not a["bb"])), (inst, a)
            if inst in units:
                seen[units[inst]][trailing] += 1
    assert all(n_ok > 0 and n_ref > 0 for n_ok, n_ref in seen.values()), seen


# 6 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,var,kernel,base,base_var", [
    ("bb0", "BB0_KFLAGS", "wbc_update_solve_kernelILi0ELb0ELb1ELb1ELb1E", "step0", "STEP0_KFLAGS"),
    ("bb1", "BB1_KFLAGS", "wbc_update_solve_kernelILi1ELb0ELb1ELb1ELb1E", "step1", "STEP1_KFLAGS"),
    ("bbs", "BBS_KFLAGS", "wbc_update_solve_kernelILi0ELb1ELb1ELb1ELb1E", "stance", "STANCE_KFLAGS"),
])
def test_new_units_resources(unit, var, kernel, base, base_var):
    """The base-body instances keep the default step's footprint, by the assertions of
    tests/test_contact_normals_cpu.py::test_new_units_resources against the instance each stands in for:
    at most 40 960 B of LDS (the rows' 448 B included), one wave per SIMD, VGPRs + AGPRs <= 512, a
    reported scratch size no larger than the base's (the fallback callee's frame), no scratch instruction
    in the kernel's own body, and the unit holding the kernel and one drain_fallbacks only."""
    with ThreadPoolExecutor(2) as ex:
        (new, asm), (old, _) = ex.map(lambda a: report(*a), [(unit, var), (base, base_var)])
    assert len(new) == 1 and len(old) == 1, (list(new), list(old))
    (name, rep), (_, ref) = next(iter(new.items())), next(iter(old.items()))
    assert kernel in name, name
    print(unit, rep, "against", base, ref)
    assert rep["LDS Size [bytes/block]"] <= 40960, rep
    assert rep["Occupancy [waves/SIMD]"] == ref["Occupancy [waves/SIMD]"] == 1, (rep, ref)
    assert rep["ScratchSize [bytes/lane]"] <= ref["ScratchSize [bytes/lane]"], (rep, ref)
    assert rep["VGPRs"] + rep["AGPRs"] <= 512, rep
    lines = asm.split("\n")
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
    ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
    assert len(starts) == 2 and sum("drain_fallbacks" in n for _, n in starts) == 1, [n for _, n in starts]
    for i, n in starts:
        if "drain_fallbacks" not in n:
            body = lines[i:min(x for x in ends if x > i)]
            assert not [l for l in body if "scratch_" in l], n
