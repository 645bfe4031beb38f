"""CPU: the per-robot contact normals' oracle (tests/contact_normals_oracle.py) against the stock numpy
oracle, an interior-point solve and its own reduced form; the Python table forms
(quadrupedwholebodycontroller_amd.contact_normal_table, what Engine.set_contact_normals passes to
wbc_set_contact_normals) with each validation error; and the compiler's resource report of the kernel
units that read the table (wbc_kernel_cn0.hip, wbc_kernel_cn1.hip, wbc_kernel_cns.hip).

wbc_set_contact_normals validates on the host too, but it needs an engine and an engine needs a device:
that validation's test is tests/test_gpu_contact_normals.py's."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import contact_normals_oracle as CN
import qp_ipm as Q
import wbc_np as W
from quadrupedwholebodycontroller_amd import _capi, contact_normal_table, workloads
from unit_reports import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tau", "grf", "x", "status", "iters")


def test_names_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert int(re.search(r"WBC_CN_LEN = (\d+)", hdr).group(1)) == _capi.CN_LEN == 12
    for s in ("wbc_set_contact_normals", "wbc_bind_device_contact_normals", "wbc_get_contact_normals"):
        assert s in _capi.C_API_SYMBOLS and re.search(rf"int32_t {s}\(", hdr)


def test_frame_rule():
    """Orthonormal, right-handed, t1 in the plane of e_x and n; exact on level ground whatever |m|."""
    for c in (0.5, 0.7, 1.0, 1.3, 2.0):
        n, t1, t2 = CN.frame([0.0, 0.0, c])
        assert np.array_equal(n, [0, 0, 1]) and np.array_equal(t1, [1, 0, 0]) and np.array_equal(t2, [0, 1, 0])
    for m in CN.normals(8, 5, 1.0).reshape(-1, 3) * 1.7:
        n, t1, t2 = CN.frame(m)
        F = np.array([t1, t2, n])
        assert np.abs(F @ F.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(F) - 1.0) < 1e-15
        assert abs(t1[1] * n[2] - t1[2] * n[1]) < 1e-15 and t1[0] > 0  # t1 x n has no x part: t1 in span(e_x, n)
        mu = 0.6
        D = CN.faces(m, mu)
        assert np.abs((D * D).sum(axis=1) - (1.0 + mu * mu)).max() < 1e-15


@pytest.mark.parametrize("name", ["stance_cold", "rl_random"])
def test_flat_normals_are_the_stock_oracle(name):
    B = 8
    inp = getattr(workloads, name)(B, seed=11)
    stock = W.run_batch(inp["base_pose"], inp["nu"], inp["qj"], inp["ref"], inp["contacts"], inp["switching"])
    for c in (1.0, 2.0):
        flat = CN.run_batch(inp, np.tile([0.0, 0.0, c], (B, 4, 1)))
        for k in KEYS:
            assert np.array_equal(flat[k], stock[k]), (k, c)


@pytest.mark.parametrize("name", ["stance_cold", "rl_random"])
def test_literal_against_ipm_and_the_edited_reduced_form(name):
    """B = 16, feet tilted by up to 0.35 rad: the literal Goldfarb-Idnani solve against the interior
    point on the same 42 x 70 QP (x to 1e-8, the bound of tests/test_oracle_ipm.py; measured 9e-15
    relative at B = 48), against the reduced 12-variable problem with its friction rows edited (tau
    to 1e-12; measured 5e-14), and against flat ground (the slopes move the torques)."""
    B = 16
    inp = getattr(workloads, name)(B, seed=11)
    nrm = CN.normals(B, 5, 0.35)
    lit = CN.run_batch(inp, nrm)
    flat = CN.run_batch(inp, np.tile(CN.FLAT, (B, 1, 1)))
    assert np.all(lit["status"] == W.QP_OK), lit["status"]
    assert (np.abs(lit["tau"] - flat["tau"]).max(axis=1) > 1e-6).sum() >= B // 2
    worst_x = worst_tau = worst_grf = 0.0
    for b in range(B):
        c = CN.controller(inp, b, nrm[b])
        c.step()
        x, st = Q.solve(*c.qp)
        assert st == W.QP_OK, b
        worst_x = max(worst_x, np.abs(x - lit["x"][b]).max() / (1.0 + np.abs(lit["x"][b]).max()))
        r = CN.reduced_step(CN.controller(inp, b, nrm[b]))
        assert r is not None and r[2] == W.QP_OK, b
        worst_tau = max(worst_tau, np.abs(r[0] - lit["tau"][b]).max() / (1.0 + np.abs(lit["tau"][b]).max()))
        worst_grf = max(worst_grf, np.abs(r[1][18:30] - lit["grf"][b]).max() / (1.0 + np.abs(lit["grf"][b]).max()))
    print(f"{name}: literal vs IPM x {worst_x:.2e}; literal vs edited reduced tau {worst_tau:.2e}, grf {worst_grf:.2e}")
    assert worst_x <= 1e-8 and worst_tau <= 1e-12 and worst_grf <= 1e-12


def test_table_forms_and_validation():
    B = 5
    nrm = CN.normals(B, 5, 0.6)
    t = contact_normal_table(B, nrm)
    assert t.shape == (B, 12) and t.flags["C_CONTIGUOUS"] and np.array_equal(t, nrm.reshape(B, 12))
    assert np.array_equal(contact_normal_table(B, nrm.reshape(B, 12)), t)
    assert np.array_equal(contact_normal_table(B, nrm[0]), np.tile(nrm[0].reshape(12), (B, 1)))
    assert np.array_equal(contact_normal_table(B, [0, 0, 1]), np.tile([0.0, 0.0, 1.0], (B, 4)))
    for shape_bad in (nrm[:4], nrm.reshape(B, 6, 2), np.ones(12), np.ones((B, 3))):
        with pytest.raises(ValueError, match="need shape"):
            contact_normal_table(B, shape_bad)
    t70, t59 = np.deg2rad(70.0), np.deg2rad(59.0)
    bad = {"nan": [np.nan, 0.0, 1.0], "inf": [0.0, np.inf, 1.0], "zero": [0.0, 0.0, 0.0], "short": [0.0, 0.0, 0.49],
           "long": [0.0, 0.0, 2.01], "down": [0.1, 0.0, -1.0], "70 degrees": [np.sin(t70), 0.0, np.cos(t70)]}
    for what, m in bad.items():
        assert not CN.valid(m), what
        for b, l in ((0, 0), (3, 2), (4, 3)):
            n2 = nrm.copy()
            n2[b, l] = m
            with pytest.raises(ValueError, match=rf"row {b}, foot {l} \({_capi.FOOT_NAMES[l]}\)"):
                contact_normal_table(B, n2)
    for m in ([0.0, 0.0, 0.5], [0.0, 0.0, 2.0], [np.sin(t59), 0.0, np.cos(t59)], [0.0, -1.2 * np.sin(t59), 1.2 * np.cos(t59)]):
        assert CN.valid(m)
        contact_normal_table(B, m)


@pytest.mark.parametrize("unit,var,kernel,base,base_var", [
    ("cn0", "CN0_KFLAGS", "wbc_update_solve_kernelILi0ELb0ELb1ELb1E", "step0", "STEP0_KFLAGS"),
    ("cn1", "CN1_KFLAGS", "wbc_update_solve_kernelILi1ELb0ELb1ELb1E", "step1", "STEP1_KFLAGS"),
    ("cns", "CNS_KFLAGS", "wbc_update_solve_kernelILi0ELb1ELb1ELb1E", "stance", "STANCE_KFLAGS"),
])
def test_new_units_resources(unit, var, kernel, base, base_var):
    """The contact-normal instances keep the default step's footprint, by the assertions of
    tests/test_robot_params_cpu.py::test_new_units_resources against the instance each stands in for:
    at most 40 960 B of LDS, one wave per SIMD, VGPRs + AGPRs <= 512, a reported scratch size no larger
    than the base's (the fallback callee's frame), no scratch instruction in the kernel's own body, and
    the unit holding the kernel and one drain_fallbacks only."""
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


# ---------------------------------------------------------------------------------------------------
# The C oracle's per-foot normals (oracle/wbc_ref.c friction_faces, wbc_ref_state::normals): the fast
# stateful checker of the cn1 / bb1 kernel instances (tests/test_gpu_stateful_offtrot.py), pinned here
# by the numpy oracle above.
import margins as M  # noqa: E402
import stateful_sequences as S  # noqa: E402
import wbc_ref as R  # noqa: E402

SEQ = dict(B=8, dwell=3, seed=5)
IN_KEYS = ("base_pose", "nu", "qj", "ref")


def _c_sequence(latch, method, nrm):
    robots = R.Robots(np.arange(SEQ["B"]), method=method, normals=nrm)
    out = [robots.step(s) for s in S.sequence(SEQ["B"], SEQ["dwell"], SEQ["seed"], latch)]
    return {k: np.array([o[k] for o in out]) for k in KEYS}


@pytest.mark.parametrize("method", [R.LITERAL, R.REDUCED], ids=["literal", "reduced"])
def test_c_flat_normals_are_the_c_oracle_without(method):
    """Normals (0, 0, 1) on every foot against no normals at all (the stock code path, which the new
    argument leaves alone): tau, x, grf, status and iters equal element for element, cold on
    rl_random(61) and over the latched off-trot sequence with its hotstarts (6 144 robot-cycles)."""
    inp = workloads.rl_random(61, seed=11)
    a, b = R.run_batch(inp, method=method), R.run_batch(inp, method=method, normals=np.tile(CN.FLAT, (61, 1, 1)))
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), ("cold", k)
    a, b = _c_sequence(True, method, None), _c_sequence(True, method, np.tile(CN.FLAT, (SEQ["B"], 1, 1)))
    assert np.sum(a["status"] == W.QP_OK) >= 0.9 * a["status"].size
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), ("sequence", k)


@pytest.mark.parametrize("name,B", [("rl_random", 61), ("stance_cold", 64)])
def test_c_sloped_cold_against_numpy(name, B):
    """Cold, feet tilted by up to 0.35 rad: C LITERAL against the numpy literal QP on the same frames, C
    REDUCED against the numpy reduced problem with its friction rows edited (iters equal: the same
    12-variable working-set walk), at the bounds of tests/test_oracle_reduced.py (x 1e-9, tau 1e-8 of
    1 + max|.|); and the slopes move the C oracle's torques as they move the numpy oracle's."""
    inp = getattr(workloads, name)(B, seed=11)
    nrm = CN.normals(B, 5, 0.35)
    lit, red = R.run_batch(inp, normals=nrm), R.run_batch(inp, method=R.REDUCED, normals=nrm)
    ref = CN.run_batch(inp, nrm)
    assert np.array_equal(lit["status"], ref["status"]) and np.array_equal(red["status"], ref["status"])
    assert np.all(ref["status"] == W.QP_OK), ref["status"]
    assert (np.abs(lit["tau"] - R.run_batch(inp)["tau"]).max(axis=1) > 1e-6).sum() >= B // 2
    worst = dict(tau=0.0, x=0.0, rtau=0.0, rx=0.0)
    for b in range(B):
        worst["tau"] = max(worst["tau"], M.norm_err(lit["tau"][b], ref["tau"][b]))
        worst["x"] = max(worst["x"], M.norm_err(lit["x"][b], ref["x"][b]))
        assert np.array_equal(lit["grf"][b], lit["x"][b, 18:30])
        r = CN.reduced_step(CN.controller(inp, b, nrm[b]))
        assert r is not None and r[2] == red["status"][b], b
        assert r[3] == red["iters"][b], (b, r[3], red["iters"][b])
        worst["rtau"] = max(worst["rtau"], M.norm_err(red["tau"][b], r[0]))
        worst["rx"] = max(worst["rx"], M.norm_err(red["x"][b], r[1]))
    print(name, worst)
    assert worst["tau"] <= 1e-8 and worst["rtau"] <= 1e-8 and worst["x"] <= 1e-9 and worst["rx"] <= 1e-9, worst


@pytest.mark.parametrize("latch", [True, False], ids=["latched", "unlatched"])
def test_c_sloped_stateful_against_numpy(latch):
    """Robots 0 and 1 over the first 240 cycles (80 dwells) of the off-trot sequence under rows 0 and 1
    of normals(8, 5, 0.35): the stateful C LITERAL robot against a stateful SlopedWBC.  Status equal, tau
    within margins.TAU, bbar[6:], W, r1 and rsw within margins.STATEFUL_INTERMEDIATE, as
    tests/test_stateful_sequences_cpu.py::test_numpy_and_c_oracle_agree_on_stateful_intermediates does on
    flat ground.  Latched every solve is OK; unlatched both statuses occur (134 OK, 46 INFEASIBLE on the
    first 90 cycles)."""
    n, nrm = 240, CN.normals(SEQ["B"], 5, 0.35)
    model, params = W.Model(), W.default_params()
    n_ok = n_inf = 0
    for b in (0, 1):
        c_robot, np_robot = R.Robot(), CN.SlopedWBC(model, params, nrm[b])
        for k, s in enumerate(S.sequence(SEQ["B"], SEQ["dwell"], SEQ["seed"], latch)[:n]):
            con, sw = int(s["contacts"][b]), int(s["switching"][b])
            c = c_robot.step(*[s[q][b] for q in IN_KEYS], con, sw, debug=True, normals=nrm[b])
            CN.load(np_robot, s, b)
            np_robot.step()
            d, ref = c["dbg"], np_robot.debug_record()
            assert c["status"] == np_robot.qp_status, (latch, b, k)
            for q in ("bbar", "W", "r1", "rsw"):
                x, y = (d[q][6:], ref[q][6:]) if q == "bbar" else (d[q], ref[q])
                tol = M.STATEFUL_INTERMEDIATE[q]
                err = float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y))))
                assert M.record(f"oracle spread {q}, sloped", err, tol) <= tol, (latch, b, k, q)
            if c["status"] == W.QP_OK:
                n_ok += 1
                err = float(np.max(np.abs(c["tau"] - np_robot.tau) / np.maximum(1.0, np.abs(np_robot.tau))))
                assert M.record("oracle spread tau, sloped", err, M.TAU) <= M.TAU, (latch, b, k)
            else:
                n_inf += c["status"] == W.QP_INFEASIBLE
    print("latched" if latch else "unlatched", "OK", n_ok, "INFEASIBLE", n_inf, "of", 2 * n)
    assert n_ok == 2 * n if latch else (n_ok >= 0.1 * 2 * n and n_inf >= 0.1 * 2 * n and n_ok + n_inf == 2 * n)


def test_c_normals_under_the_host_sanitizers(tmp_path):
    """oracle/wbc_ref.c with the stand-alone driver oracle/sanitize_normals_main.c, compiled with
    -fsanitize=address,undefined (oracle/Makefile `sanitize`) and run once: one robot per QP form through
    30 cycles of a mask-changing sequence with normals set, replaced and cleared.  A program of its own on
    the CPU; a sanitizer report ends it with a non-zero status."""
    import subprocess

    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "sanitize", f"SAN_OUT={tmp_path}/sanitize_normals"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sanitize_normals: done" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
