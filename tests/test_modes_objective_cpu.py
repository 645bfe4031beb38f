"""CPU: the QP objective of contact-mode hypotheses (wbc_step_modes with WBC_OBJECTIVE / WBC_BEST).

  * the closed form the kernels evaluate equals 1/2 x^T H x + g^T x of the reference QP;
  * the value is well conditioned: the LITERAL and the REDUCED numpy oracle agree on it far inside the bound the
    GPU test holds the engine to (the spread is recorded in profiles/modes_objective/oracle_spread.json);
  * the stress set has what the GPU test needs so that it cannot pass vacuously (OK and INFEASIBLE hypotheses
    side by side, states with no feasible hypothesis under a subset, an argmin well outside rounding);
  * the boundary: constants, symbols, and the compiler's resource report of the new kernel unit.
"""
import json
import os
import re

import numpy as np

import modes_objective_oracle as MO
import wbc_np as W
from quadrupedwholebodycontroller_amd import _capi
from unit_reports import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The two oracles' objectives against each other, normalised |d| / (1 + |obj|).  The engine's error counts as a
# defect above 1e-9 (tests/test_gpu_modes_objective.py); the reference's own uncertainty has to sit well below
# that line for the line to mean anything: a tenth of it.  Measured: 1.0e-13 (rl), 1.9e-12 (stress), where the x of
# the two oracles differ by up to 4e-8 and the terms of the sum reach 1e8 beside objectives of 1e4.
SPREAD_BOUND = 1e-10
# the closed form against x^T H x / 2 + g^T x: the same sum in another order, terms up to 1e8 beside |obj| >= 6e3,
# so a few thousand ulps of the result at the worst; measured 8.4e-15 (rl), 1.4e-15 (stress)
CLOSED_BOUND = 1e-9


def _norm(a, b):
    return np.abs(a - b) / (1.0 + np.abs(b))


def test_closed_form_equals_the_qp_objective():
    o = MO.oracle_modes("rl")
    assert (o["status"] == W.QP_OK).all()  # all 128 hypotheses solve: the whole set is compared
    err = _norm(o["closed"], o["obj"]).max()
    print("closed form vs 1/2 x^T H x + g^T x, rl:", err)
    assert err < CLOSED_BOUND
    ok = o["status"] == W.QP_OK
    assert 5e3 < np.abs(o["obj"][ok]).min() and np.abs(o["obj"][ok]).max() < 5e6  # the sizes DESIGN.md 19 quotes
    s = MO.oracle_modes("stress")
    ok = s["status"] == W.QP_OK
    assert _norm(s["closed"][ok], s["obj"][ok]).max() < CLOSED_BOUND


def test_literal_and_reduced_oracle_agree_on_the_objective():
    spread = {}
    for name in ("rl", "stress"):
        o = MO.oracle_modes(name)
        ok = o["status"] == W.QP_OK
        assert np.isfinite(o["reduced"][ok]).all()  # the reduction is usable on every hypothesis of both sets
        assert np.isinf(o["reduced"][~ok]).all() and np.isinf(o["obj"][~ok]).all()
        spread[name] = float(_norm(o["reduced"][ok], o["obj"][ok]).max())
        print("oracle spread", name, spread[name])
        assert spread[name] < SPREAD_BOUND, (name, spread[name])
    rec = json.load(open(os.path.join(ROOT, "profiles", "modes_objective", "oracle_spread.json")))
    for name in spread:  # the committed record is of this measurement (libm and BLAS may move the last digits)
        assert rec["spread"][name] < SPREAD_BOUND and 0.01 < (spread[name] + 1e-16) / (rec["spread"][name] + 1e-16) < 100


def test_stress_set_preconditions():
    o = MO.oracle_modes("stress")
    st, obj = o["status"], o["obj"]
    assert st.shape == (16, 16)
    assert set(st.ravel().tolist()) == {W.QP_OK, W.QP_INFEASIBLE}
    ok = st == W.QP_OK
    mixed = int(sum(ok[s].any() and not ok[s].all() for s in range(16)))
    print("stress: OK", ok.mean(), "mixed states", mixed)
    assert mixed >= 5            # measured 7
    assert ok.mean() >= 0.60     # measured 0.82
    sub = MO.STRESS_SUBSET
    none_ok = [s for s in range(16) if not ok[s][sub].any()]
    print("stress: no OK hypothesis under", sub, "in states", none_ok)
    assert len(none_ok) >= 3     # measured 5: states 0, 4, 7, 12, 14
    best, val = MO.best_modes(obj[:, sub], st[:, sub])
    assert all(best[s] == -1 and np.isinf(val[s]) for s in none_ok) and (best >= 0).sum() == 16 - len(none_ok)
    gaps = []
    for s in range(16):
        v = np.sort(obj[s][ok[s]])
        assert len(v) >= 2
        gaps.append((v[1] - v[0]) / (1.0 + abs(v[0])))
    print("stress: smallest gap between best and second best", min(gaps))
    assert min(gaps) > 1e-4      # measured 5.7e-3: the argmin is never inside rounding


def test_best_modes_tie_rule():
    obj = np.array([[3.0, 1.0, 1.0, 2.0], [np.inf, np.inf, 5.0, 5.0], [1.0, 0.5, 0.5, 0.5], [7.0, 7.0, 7.0, 7.0]])
    status = np.array([[0, 0, 0, 0], [2, 2, 0, 0], [0, 2, 0, 0], [2, 1, 3, 2]])
    best, val = MO.best_modes(obj, status)
    assert best.tolist() == [1, 2, 2, -1]
    assert val[:3].tolist() == [1.0, 5.0, 0.5] and np.isinf(val[3])


def test_tie_set_mask_15_wins_everywhere():
    """The GPU test's tie set (stance_cold(8, seed=22) under [15, 10, 5, 15, 0]): the four-contact hypothesis has
    the lowest objective in all 8 states, so the repeated mask 15 ties for the minimum in every one of them."""
    from quadrupedwholebodycontroller_amd import workloads

    base, params, model = workloads.stance_cold(8, seed=22), W.default_params(), W.Model()
    modes = [15, 10, 5, 15, 0]
    rows = [[MO.oracle_row(base, params, s, k, model) for k in modes] for s in range(8)]
    status = np.array([[r[0] for r in row] for row in rows])
    obj = np.array([[r[1] for r in row] for row in rows])
    assert np.array_equal(obj[:, 0], obj[:, 3]) and (status[:, 0] == W.QP_OK).all()
    assert (obj[:, 0] == obj.min(axis=1)).all()
    assert MO.best_modes(obj, status)[0].tolist() == [0] * 8


def test_flags_symbols_and_header():
    hdr = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert re.search(r"#define WBC_OBJECTIVE 512u", hdr) and re.search(r"#define WBC_BEST 1024u", hdr)
    assert (_capi.OBJECTIVE, _capi.BEST) == (512, 1024)
    assert "getObjVal()" in hdr.split("#ifndef WBC_H")[0]  # the mapping line of the header comment
    lib = _capi.load_library()
    for s in ("wbc_get_objective", "wbc_device_objective", "wbc_get_best_modes", "wbc_device_best_modes"):
        assert s in _capi.MODE_OUT_SYMBOLS and s in _capi.C_API_SYMBOLS and re.search(rf"int32_t {s}\(", hdr)
        assert hasattr(lib, s), s
    for m in ("objective", "best_modes", "device_objective", "device_best_modes"):
        assert callable(getattr(_capi.Engine, m))
    # KernelArgs::obj is the last member: no other argument's offset moves
    lay = open(os.path.join(ROOT, "quadrupedwholebodycontroller_amd", "csrc", "wbc_layout.h")).read()
    body = lay[lay.index("struct KernelArgs {"):]
    body = body[:body.index("\n};")]
    members = [l.strip() for l in body.split("\n") if l.strip().endswith(";") and not l.strip().startswith("//")]
    assert members[-1] == "double* obj;" and members[-2] == "const double* bb;"


def test_new_unit_resources():
    """wbc_kernel_modes_obj.hip keeps the mode loop's footprint: one wave per SIMD, at most 40 960 B of LDS, no
    scratch instruction in the kernel's own body, and the unit holds its kernel and one drain_fallbacks only."""
    rep, asm = report("modes_obj", "MODES_OBJ_KFLAGS")
    assert len(rep) == 1, list(rep)
    name, r = next(iter(rep.items()))
    print("modes_obj", r)
    assert "wbc_modes_obj_kernel" in name
    assert r["Occupancy [waves/SIMD]"] == 1
    assert r["LDS Size [bytes/block]"] <= 40960
    assert r["VGPRs"] + r["AGPRs"] <= 512
    lines = asm.split("\n")
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
    ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
    assert len(starts) == 2 and sum("drain_fallbacks" in n for _, n in starts) == 1, [n for _, n in starts]
    for i, n in starts:
        if "drain_fallbacks" not in n:
            body = lines[i:min(x for x in ends if x > i)]
            assert not [l for l in body if "scratch_" in l], n
