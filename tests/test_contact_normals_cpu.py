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
from test_robot_params_cpu import _report

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
        (new, asm), (old, _) = ex.map(lambda a: _report(*a), [(unit, var), (base, base_var)])
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
