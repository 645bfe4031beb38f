"""GPU: the QP multipliers of the default step (wbc_step with WBC_DUALS, wbc_get_duals / wbc_device_duals,
include/wbc.h; wbc_kernel_du0.hip stateless, wbc_kernel_du1.hip stateful).

The checker is tests/duals_oracle.py's certificate: the engine's own x and its 40 multipliers against the
literal 42 x 70 QP the numpy oracle assembles for the same robot (no working set, Householder or Givens step of
any oracle is involved).  The stationarity bound of an input set is the numpy oracle's own residual on that set
(profiles/duals/oracle_residuals.json, measured by tests/test_duals_cpu.py) times 53, the widest margin
tests/margins.py grants the engine over an oracle.  It is relative (over 1 + max |H x + g|).  The primal violation
is absolute, as wbc_np.kkt_residuals computes it.  Read literally against the stationarity bound it cannot be met
by the oracle itself (its own x violates rows of size 1e3 by 5.4e-12 on the 20 N m stress set, whose stationarity
bound is 2.3e-12; 1.2e-12 against 7.0e-13 on the tables set), so it is bounded as stationarity is: the oracle's own
absolute violation on the set, from the same record, times 53 (DESIGN.md 20 states both figures).  The signs are
held to -bound (1 + max entry), complementarity to 1e-7, the oracle's own activity threshold."""
import numpy as np

import margins as M
import pytest

import duals_oracle as D
import wbc_np as W
from quadrupedwholebodycontroller_amd import (COLD, DEBUG, DUALS, FUSED, GROUP, NO_X, QP_OK, RESIDENT, SPLIT, STATELESS, TIMED,
                                              Engine, WbcError, default_params, dual_rows, workloads)
import table_steps as T
from table_steps import ERR_ARG, ERR_STATE, assert_identical, last_error, load
from table_steps import table as rp_table

pytestmark = pytest.mark.gpu


def params(over=None):
    p = default_params()
    for k, v in (over or {}).items():
        setattr(p, k, v)
    return p


def engine(B, over=None):
    return Engine(B, params=params(over))


def run(inp, flags, over=None, t=None, nrm=None, rows=None, duals=True):
    """One step on a fresh engine: (outputs, duals or None).  Every call that reads the duals passes WBC_DUALS in `flags`."""
    out = T.run(inp, flags, duals, params=params(over), robot_params=t, contact_normals=nrm, base_body=rows)
    return out, out.pop("dual", None)


def certify(name, cs, out, d, contacts, what=""):
    """The per-robot checks of the module docstring on every robot of a step; returns the worst stationarity."""
    bound, pbound = D.gpu_bound(name), D.gpu_bound(name, "primal")
    worst = dict(stat=0.0, viol=0.0, comp=0.0, sign=0.0)
    n_active = 0
    for b, c in enumerate(cs):
        assert out["status"][b] == c.qp_status, (what, b, out["status"][b], c.qp_status)
        if c.qp_status != QP_OK:
            assert not d[b].any(), (what, b, "a robot that is not OK has 40 zeros")
            continue
        assert np.count_nonzero(d[b]) <= 12, (what, b)
        for leg in range(4):
            if not (int(contacts[b]) >> leg) & 1:
                assert not d[b, 4 * leg:4 * leg + 4].any(), (what, b, leg, "a swing leg's faces are 0")
        n_active += bool(d[b].any())
        x = out["x"][b]
        viol, stat, sign, comp = D.certificate(c, x, d[b])
        print(f"[duals] {what or name} robot {b}: stationarity {stat:.2e} primal {viol:.2e} min {sign:.2e} complementarity {comp:.2e} "
              f"active {np.count_nonzero(d[b])}")
        worst["stat"], worst["viol"], worst["comp"] = max(worst["stat"], stat), max(worst["viol"], viol), max(worst["comp"], comp)
        worst["sign"] = max(worst["sign"], -sign / (1.0 + d[b].max()))
    M.record(f"stationarity {name}", worst["stat"], bound)
    M.record(f"primal {name}", worst["viol"], pbound)
    M.record(f"sign {name}", worst["sign"], bound)
    M.record(f"complementarity {name}", worst["comp"], 1e-7)
    assert worst["stat"] <= bound, (what, worst)
    assert worst["viol"] <= pbound, (what, worst)
    assert worst["sign"] <= bound, (what, worst)
    assert worst["comp"] <= 1e-7, (what, worst)
    return n_active


# 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stress52_20Nm", "stress53_6Nm", "rl_random_45", "stance_cold_16"])
def test_cold_certificate(name):
    """engine.step(STATELESS | DUALS): the two stress sets at B = 48 (every mask; at 6 N m one robot is not OK), a
    batch that is no multiple of four, and the all-stance set (the stance form, on du0)."""
    inp, over, cs = D.cold_set(name)
    out, d = run(inp, STATELESS | DUALS, over)
    n = certify(name, cs, out, d, inp["contacts"])
    assert n >= len(cs) // 2, n


# 2 ----------------------------------------------------------------------------------------------
def test_fallback_certificate():
    """Every fifth robot has a stretched leg; where that leg is a stance leg (robots 0 and 15: masks 13 and 15)
    the 12-variable reduction is not usable and the QP is solved by drain_fallbacks' 24-variable method, whose
    working set is mapped to the 40 rows.  That those solves took the fallback is read from `iters`, which counts
    the working-set changes of the method that ran (include/wbc.h): the general method counts the swing slack rows
    too, so on a robot with a swing leg it counts more than the 12-variable form.  WBC_FUSED runs the general
    method on every robot: the default step's count equals the fused step's on the fallback robots and is smaller
    on every other robot with a swing leg; robot 0 (mask 13) is a fallback robot with a swing leg and active rows."""
    name = "straight_20"
    inp, over, cs = D.cold_set(name)
    out, d = run(inp, STATELESS | DUALS, over)
    certify(name, cs, out, d, inp["contacts"])
    plain, _ = run(inp, STATELESS, over, duals=False)
    assert_identical(out, plain, what="fallback set")
    fused, _ = run(inp, STATELESS | FUSED, over, duals=False)
    masks = inp["contacts"].astype(int)
    fb = [b for b in range(0, 20, 5) if (masks[b] >> (b % 4)) & 1]
    print("masks", masks.tolist(), "fallback robots", fb, "iters", out["iters"].tolist(), "fused", fused["iters"].tolist())
    assert fb == [0, 15] and masks[0] == 13
    for b in range(20):
        assert fused["status"][b] == out["status"][b] == QP_OK, b
        if b in fb:
            assert out["iters"][b] == fused["iters"][b], (b, out["iters"][b], fused["iters"][b])
        elif masks[b] != 15:
            assert out["iters"][b] < fused["iters"][b], (b, out["iters"][b], fused["iters"][b])
    assert all(d[b].any() for b in fb), [np.count_nonzero(d[b]) for b in fb]


# 3 ----------------------------------------------------------------------------------------------
def _tables(B):
    import base_body_oracle as BB
    import contact_normals_oracle as CN
    return dict(t=rp_table(B), nrm=CN.normals(B, 5, 0.35), rows=BB.payload_rows(B))


@pytest.mark.parametrize("B", [45, 5])
@pytest.mark.parametrize("which", ["none", "t", "nrm", "rows", "all"])
def test_nothing_else_moves_cold(which, B):
    """tau, grf, x, status and iters with WBC_DUALS are the bits of the same engine without it: no table, each
    table alone (the rng(7) parameters, sloped normals, payload rows of tests/test_gpu_base_body.py) and all
    three, mixed masks and all-stance, B = 45 and B = 5."""
    tabs = _tables(B)
    kw = {} if which == "none" else tabs if which == "all" else {which: tabs[which]}
    for name in ("rl_random", "stance_cold"):
        inp = getattr(workloads, name)(B, seed=91)
        e = Engine(B)
        load(e, inp)
        if "t" in kw:
            e.set_robot_params(kw["t"])
        if "nrm" in kw:
            e.set_contact_normals(kw["nrm"])
        if "rows" in kw:
            e.set_base_body(kw["rows"])
        e.step(STATELESS)
        plain = e.outputs()
        e.step(STATELESS | DUALS)
        out, d = e.outputs(), e.duals()
        assert_identical(out, plain, what=(which, name, B))
        assert d.shape == (B, 40) and np.isfinite(d).all() and (d[out["status"] != QP_OK] == 0).all()
        # WBC_NO_X: x is not written, everything else and the duals keep their bits
        e.step(STATELESS | DUALS | NO_X)
        o2, d2 = e.outputs(), e.duals()
        for k in ("tau", "grf", "status", "iters"):
            assert np.array_equal(o2[k], plain[k]), (which, name, k, "NO_X")
        assert np.array_equal(d2, d), (which, name, "duals under NO_X")
        # WBC_TIMED and WBC_DEBUG are allowed and change nothing
        e.step(STATELESS | DUALS | TIMED | DEBUG)
        assert_identical(e.outputs(), plain, what=(which, name, "TIMED | DEBUG"))
        assert np.array_equal(e.duals(), d)
        # an unflagged step after a flagged one: the plain step's bits, and the getters refuse again
        e.step(STATELESS)
        assert_identical(e.outputs(), plain, what=(which, name, "unflagged after flagged"))
        with pytest.raises(WbcError):
            e.duals()
        e.close()
        if name == "rl_random":
            assert d.any()


def test_nothing_else_moves_group_and_stateful():
    """Device-bound masks under WBC_GROUP (the device-built wave map), and 20 stateful trot steps, hotstarted and
    WBC_COLD: every output's bits with the flag are those without it."""
    torch = pytest.importorskip("torch")
    B = 45
    inp = workloads.rl_random(B, seed=91)
    masks = torch.from_numpy(inp["contacts"]).cuda()
    torch.cuda.synchronize()
    e = Engine(B)
    load(e, inp)
    e.bind_device_inputs(contacts=masks.data_ptr())
    ref_d = None
    for flags in (STATELESS | GROUP, STATELESS):
        e.step(flags)
        plain = e.outputs()
        e.step(flags | DUALS)
        assert_identical(e.outputs(), plain, what=("device masks", flags))
        d = e.duals()
        assert ref_d is None or np.array_equal(d, ref_d)  # grouped or not: a robot's bits are its own
        ref_d = d
    e.close()
    assert ref_d.any()
    B = 8
    for flags in (0, COLD):
        a, b = Engine(B), Engine(B)
        for k, s in enumerate(list(workloads.trot_sequence(B, steps=20, seed=2))[:20]):
            load(a, s)
            load(b, s)
            a.step(flags)
            b.step(flags | DUALS)
            assert_identical(b.outputs(), a.outputs(), what=("trot", flags, k))
        a.close()
        b.close()


# 4 ----------------------------------------------------------------------------------------------
def test_all_three_tables_certificate():
    """B = 16 under per-robot friction 0.4 + 0.05 b, max_torque 30 + 3 b, sloped normals and payload rows, against
    contact_normals_oracle.SlopedWBC given each robot's model, parameters and normals: 15 robots hold an active row."""
    inp, tabs, cs = D.cold_set(D.TABLES_SET)
    out, d = run(inp, STATELESS | DUALS, None, tabs["cols"], tabs["normals"], tabs["rows"])
    n = certify(D.TABLES_SET, cs, out, d, inp["contacts"])
    assert n == 15, n
    r = dual_rows(d)
    assert r["friction"].shape == (16, 4, 4) and r["torque"].shape == (16, 12) and (r["friction"] >= 0).all()
    # a saturated joint: tau sits at the robot's own limit, on the side the multiplier's sign names
    lim = tabs["cols"]["max_torque"]
    for b, j in zip(*np.nonzero(r["torque"])):
        assert abs(out["tau"][b, j] + np.sign(r["torque"][b, j]) * lim[b]) <= 1e-7 * (1.0 + lim[b]), (b, j)


# 5 ----------------------------------------------------------------------------------------------
def test_stateful_certificate_hot_and_cold():
    """The trot at B = 8, 30 cycles, 40 N m so that torque rows bind: the hotstarted run (du1's direct warm points
    and re-added sets) and the WBC_COLD run, each cycle certified against the stateful numpy oracle's QP of that
    cycle; the two runs' multipliers agree to the bound on robots whose active rows are independent (the
    multipliers are then unique: the same non-zero pattern in both runs and full row rank of the active rows
    together with the equality rows)."""
    seq, cycles = D.trot_set()
    B, name = D.TROT["B"], D.TROT_SET
    bound = D.gpu_bound(name)
    over = dict(max_torque=D.TROT["max_torque"])
    hot, cold = engine(B, over), engine(B, over)
    n_active = n_cmp = n_hot_iters = n_cold_iters = n_direct = 0
    worst = 0.0
    for k, inp in enumerate(seq):
        res = {}
        for tag, e, flags in (("hot", hot, DUALS), ("cold", cold, DUALS | COLD)):
            load(e, inp)
            e.step(flags)
            res[tag] = (e.outputs(), e.duals())
            n_active += certify(name, cycles[k], *res[tag], inp["contacts"], what=f"{tag} cycle {k}")
        (oh, dh), (oc, dc) = res["hot"], res["cold"]
        n_hot_iters += int(oh["iters"].sum())
        # the hotstart's direct point: a warm set of one or two rows accepted without a working-set change, whose
        # multipliers come from its 1 x 1 / 2 x 2 system (and were certified above)
        nz = np.count_nonzero(dh, axis=1)
        n_direct += int(((oh["iters"] == 0) & (oh["status"] == QP_OK) & (nz >= 1) & (nz <= 2)).sum()) if k > 0 else 0
        n_cold_iters += int(oc["iters"].sum())
        for b, c in enumerate(cycles[k]):
            if not np.array_equal(dh[b] != 0, dc[b] != 0) or not dh[b].any():
                continue
            A = c.qp[2]
            act = [18 + r if r < 16 else 34 + (r - 16) // 2 for r in np.nonzero(dh[b])[0]]
            E = A[:18][np.any(A[:18] != 0.0, axis=1)]
            rows = np.vstack([E, A[act]])
            if np.linalg.matrix_rank(rows) < rows.shape[0]:
                continue
            n_cmp += 1
            worst = max(worst, float(np.abs(dh[b] - dc[b]).max() / (1.0 + np.abs(dc[b]).max())))
    hot.close()
    cold.close()
    print(f"trot: {n_active} certified robot-cycles with an active row, {n_cmp} compared hot against cold; iters hot {n_hot_iters} cold {n_cold_iters}")
    assert n_active >= B * len(seq) // 2 and n_cmp >= B * len(seq) // 4
    assert n_hot_iters < n_cold_iters  # the hotstart ran
    print(f"trot: {n_direct} hotstarted robot-cycles ended at a direct point with a non-empty warm set")
    assert n_direct >= B  # iters == 0 with one or two non-zero multipliers: the direct point carried them
    assert M.record("duals hot vs WBC_COLD", worst, bound) <= bound


# 6 ----------------------------------------------------------------------------------------------
def test_a_robot_depends_on_its_own_inputs_only():
    """A permuted batch gives permuted dual bits (B = 45: another wave map, other wave-mates, another padding)."""
    inp, over, _ = D.cold_set("rl_random_45")
    out, d = run(inp, STATELESS | DUALS, over)
    perm = np.random.default_rng(4).permutation(45)
    pout, pd = run(T.take(inp, perm), STATELESS | DUALS, over)
    assert_identical(pout, out, idx_b=perm, what="permuted")
    assert np.array_equal(pd, d[perm])


def test_device_pointer_holds_the_duals():
    torch = pytest.importorskip("torch")
    import ctypes as C
    inp, over, _ = D.cold_set("rl_random_45")
    B = 45
    e = engine(B, over)
    load(e, inp)
    e.step(STATELESS | DUALS)
    d = e.duals()
    ptr = e.device_duals()
    assert ptr
    # the same bits behind the device pointer: a device-to-device copy into a torch tensor
    hip_memcpy = e.lib.hipMemcpy
    hip_memcpy.argtypes, hip_memcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    t = torch.empty((B, 40), dtype=torch.float64, device="cuda")
    e.synchronize()
    assert hip_memcpy(t.data_ptr(), ptr, t.numel() * t.element_size(), 3) == 0  # hipMemcpyDeviceToDevice
    assert np.array_equal(t.cpu().numpy(), d) and d.any()
    e.step(STATELESS | DUALS)
    assert e.device_duals() == ptr  # the buffer is the engine's own, allocated once
    e.close()


# 7 ----------------------------------------------------------------------------------------------
def test_errors():
    """WBC_DUALS is WBC_ERR_ARG on wbc_update, wbc_solve, wbc_cycle and wbc_step_modes, and on wbc_step with
    WBC_SPLIT, WBC_FUSED or WBC_RESIDENT; the getters are WBC_ERR_STATE before a flagged step and after an
    unflagged one."""
    B = 4
    inp = workloads.rl_random(B, seed=91)
    e = Engine(B)
    load(e, inp)
    for get in (e.duals, e.device_duals):
        with pytest.raises(WbcError) as ei:
            get()
        assert f"({ERR_STATE})" in str(ei.value) and "did not carry WBC_DUALS" in last_error(e)
    calls = {
        "wbc_update": lambda: e.update(STATELESS | DUALS),
        "wbc_solve": lambda: e.solve(STATELESS | DUALS),
        "wbc_cycle": lambda: T.cycle(e, inp, STATELESS | DUALS),
        "wbc_step split": lambda: e.step(STATELESS | DUALS | SPLIT),
        "wbc_step fused": lambda: e.step(STATELESS | DUALS | FUSED),
        "wbc_step resident": lambda: e.step(STATELESS | DUALS | RESIDENT),
    }
    for name, call in calls.items():
        with pytest.raises(WbcError) as ei:
            call()
        assert f"({ERR_ARG})" in str(ei.value) and last_error(e).startswith(name.split()[0] + ": WBC_DUALS"), (name, last_error(e))
    e.set_modes([15, 5])
    with pytest.raises(WbcError) as ei:
        e.step_modes(STATELESS | DUALS)
    assert f"({ERR_ARG})" in str(ei.value) and last_error(e).startswith("wbc_step_modes: WBC_DUALS")
    e.set_modes(None)
    load(e, inp)
    e.step(STATELESS | DUALS)
    d = e.duals()
    assert d.shape == (B, 40) and e.device_duals()
    e.step(STATELESS)
    for get in (e.duals, e.device_duals):
        with pytest.raises(WbcError) as ei:
            get()
        assert f"({ERR_STATE})" in str(ei.value)
    # the refused calls above changed nothing: the flagged step still gives the same bits
    e.step(STATELESS | DUALS)
    assert np.array_equal(e.duals(), d)
    e.close()
