"""GPU: the 48 QP multipliers of the default step under a per-robot force task (wbc_step with WBC_DUALS_TASK, read with
wbc_get_force_duals / wbc_device_force_duals, include/wbc.h; wbc_kernel_ftd0.hip stateless, wbc_kernel_ftd1.hip
stateful).

The checker is tests/force_duals_oracle.py's certificate on tests/force_task_oracle.ForceTaskWBC's literal 74-row QP:
the engine's own x and its 48 multipliers against the QP the numpy oracle assembles for the same robot and cycle.
The bounds of an input set are the numpy oracle's own figures on that set
(profiles/force_task_duals/oracle_residuals.json, held by tests/test_force_task_duals_cpu.py) times 53, as
DESIGN.md 20, 21 and 23 built theirs; the signs are held to -bound (1 + max entry), complementarity to 1e-7."""
import ctypes as C

import numpy as np

import margins as M
import pytest

import force_bounds_oracle as FO
import force_duals_oracle as FD
import force_task_duals_oracle as FTD
import force_task_oracle as FT
import limits_oracle as LO
import table_steps as T
from quadrupedwholebodycontroller_amd import (COLD, DEBUG, DUALS, DUALS_FORCE, DUALS_TASK, FUSED, GROUP, NO_X, QP_NUMERIC, QP_OK,
                                              RESIDENT, SPLIT, STATELESS, TIMED, Engine, WbcError, dual_rows, workloads)
from table_steps import ERR_ARG, ERR_STATE, assert_identical, inputs, last_error, load

pytestmark = pytest.mark.gpu
TABLES = ("robot_params", "contact_normals", "base_body", "limits", "force_bounds", "force_task")


def engine(inp, **tables):
    """An engine loaded with `inp` under the given tables, set in the engine's order, the force task last."""
    e = Engine(len(inp["contacts"]))
    load(e, inp)
    for name in TABLES:
        if tables.get(name) is not None:
            getattr(e, "set_" + name)(tables[name])
    return e


def run(inp, flags, **tables):
    """One step on a fresh engine: (outputs, the 48 multipliers when the step carries a 48-entry flag, else None)."""
    e = engine(inp, **tables)
    e.step(flags)
    out, d = e.outputs(), (e.force_duals() if flags & (DUALS_TASK | DUALS_FORCE) else None)
    e.close()
    return out, d


def certify(name, cs, out, d, contacts, what=""):
    """The per-robot checks of the module docstring on every robot of a step; the number of robots with a non-zero
    force multiplier."""
    bound, pbound = FTD.gpu_bound(name), FTD.gpu_bound(name, "primal")
    worst = dict(stat=0.0, viol=0.0, comp=0.0, sign=0.0)
    n_force = 0
    assert d.shape == (len(cs), 48) and np.isfinite(d).all(), what
    for b, c in enumerate(cs):
        assert out["status"][b] == c.qp_status, (what, b, out["status"][b], c.qp_status)
        if c.qp_status != QP_OK:
            assert not d[b].any(), (what, b, "a robot that is not OK has 48 zeros")
            continue
        assert np.count_nonzero(d[b]) <= 12, (what, b)
        for leg in range(4):
            if not (int(contacts[b]) >> leg) & 1:
                assert not d[b, 4 * leg:4 * leg + 4].any() and not d[b, 40 + 2 * leg:42 + 2 * leg].any(), (what, b, leg)
        n_force += bool(d[b, 40:].any())
        viol, stat, sign, comp = FD.certificate48(c, out["x"][b], d[b])
        print(f"[task duals] {what or name} robot {b}: stationarity {stat:.2e} primal {viol:.2e} min {sign:.2e} complementarity "
              f"{comp:.2e} active {np.count_nonzero(d[b])} force {np.count_nonzero(d[b, 40:])}")
        worst["stat"], worst["viol"], worst["comp"] = max(worst["stat"], stat), max(worst["viol"], viol), max(worst["comp"], comp)
        worst["sign"] = max(worst["sign"], -sign / (1.0 + d[b].max()))
    M.record(f"stationarity {name}", worst["stat"], bound)
    M.record(f"primal {name}", worst["viol"], pbound)
    M.record(f"sign {name}", worst["sign"], bound)
    M.record(f"complementarity {name}", worst["comp"], 1e-7)
    assert worst["stat"] <= bound, (what, worst, bound)
    assert worst["viol"] <= pbound, (what, worst, pbound)
    assert worst["sign"] <= bound, (what, worst, bound)
    assert worst["comp"] <= 1e-7, (what, worst)
    return n_force


# 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [*FTD.COLD_TB, *FTD.COLD_T])
def test_cold_certificate_and_counts(name):
    """step(STATELESS | DUALS_TASK) under table(B, 11, contacts), with and without force_bounds_oracle.table(B, 7): the
    all-stance set (the stance form under weights from 0.1 to 100), every mask with a ragged last wave, and the
    stretched legs (the in-wave fallback, tags 24 / 25).  As many robots carry a force multiplier as on the oracle,
    and where a robot's priced rows are independent its force multipliers are the oracle's least-squares ones to the
    stationarity bound times 1 + max lambda (tests/test_gpu_force_duals.py's rule and bound)."""
    inp, t, fn, cs = FTD.cold_set(name)
    out, d = run(inp, STATELESS | DUALS_TASK, force_bounds=fn, force_task=t)
    n = certify(name, cs, out, d, inp["contacts"])
    want = sum(FD.has_force_multiplier(c) for c in cs)
    print(f"{name}: {n} robots with a force multiplier (oracle {want}), {int(d.any(axis=1).sum())} with any")
    assert n == want
    assert d.any()
    if name.startswith("stance_cold"):  # the stance form with w != 1 delivers multipliers of the unscaled rows
        w = t[:, FT.FT_WEIGHT]
        assert np.all(inp["contacts"] == 15) and w.min() < 0.2 and w.max() > 50.0
        assert np.any((w != 1.0) & d.any(axis=1)), "no robot with w != 1 and a non-zero multiplier"
    if fn is None:
        return
    sig = lambda v: np.abs(v) > 1e-9 * (1.0 + np.abs(v).max())
    bound, n_cmp, n_want, worst = FTD.gpu_bound(name), 0, 0, 0.0
    for b, c in enumerate(cs):
        if c.qp_status != QP_OK:
            continue
        ref = FD.lsq_duals48(c, c.qp_solution)
        n_want += bool(sig(ref)[40:].any() and FD.active_rows_independent(c, np.where(sig(ref), ref, 0.0)))
        rows = np.where(sig(ref) | sig(d[b]), 1.0, 0.0)
        if not rows[40:].any() or not FD.active_rows_independent(c, rows):
            continue
        n_cmp += 1
        err = np.abs(d[b, 40:] - ref[40:]).max() / (1.0 + np.abs(ref).max())
        worst = max(worst, err)
    M.record(f"force multipliers vs least squares {name}", worst, bound)
    print(f"{name}: {n_cmp} robots compared with the least-squares multipliers (oracle-side count {n_want}), worst {worst:.2e}")
    assert worst <= bound, (name, worst, bound)
    assert n_cmp >= n_want > 0, (n_cmp, n_want)


def test_six_tables_certificate():
    """B = 16 under rng(7) parameters, sloped normals, payload base bodies, limits, force bounds and the seed-11 task,
    against the oracle given each robot's own rows."""
    inp, tabs, cs = FTD.six_tables()
    out, d = run(inp, STATELESS | DUALS_TASK, **tabs)
    n = certify(FTD.TABLES_SET, cs, out, d, inp["contacts"])
    assert n == sum(FD.has_force_multiplier(c) for c in cs), n
    r = dual_rows(d)
    assert r["force"].shape == (16, 4) and r["friction"].shape == (16, 4, 4) and r["torque"].shape == (16, 12)


# 2 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, COLD], ids=["hotstart", "cold"])
def test_ramp_certificate(flags):
    """The load ramp with a fresh task every cycle (B = 8, 130 trot steps, both tables rewritten into device-bound
    tensors every cycle, every robot reset before cycle RESET_AT) on ftd1: every cycle certified against the stateful
    oracle's QP of that cycle and robot."""
    torch = pytest.importorskip("torch")
    R, cycles = FTD.ramp_snapshots()
    B = R["B"]
    e = Engine(B)
    dfn, dft = torch.from_numpy(R["bounds"][0].copy()).cuda(), torch.from_numpy(R["tasks"][0].copy()).cuda()
    torch.cuda.synchronize()
    e.bind_device_force_bounds(dfn)
    e.bind_device_force_task(dft)
    n_force = n_ok = n_direct = 0
    for k, inp in enumerate(R["seq"]):
        if k == FO.RESET_AT:
            e.reset()
        e.synchronize()
        dfn.copy_(torch.from_numpy(R["bounds"][k]))
        dft.copy_(torch.from_numpy(R["tasks"][k]))
        torch.cuda.synchronize()
        load(e, inp)
        e.step(flags | DUALS_TASK)
        out, d = e.outputs(), e.force_duals()
        n_force += certify(FTD.RAMP_SET, cycles[k], out, d, inp["contacts"], what=f"ramp flags {flags} cycle {k}")
        n_ok += int((out["status"] == QP_OK).sum())
        n_direct += int(((out["iters"] == 0) & (out["status"] == QP_OK) & d[:, 40:].any(axis=1)).sum()) if k > 0 else 0
    e.close()
    want = sum(FD.has_force_multiplier(c) for row in cycles for c in row)
    print(f"ramp flags {flags}: {n_force} of {n_ok} OK robot-cycles with a force multiplier (oracle {want}); {n_direct} ended with iters == 0")
    assert n_ok > B * len(R["seq"]) // 2 and n_force == want > 0


def test_the_direct_point_carries_a_force_row_under_the_task():
    """A standing batch, B = 8, three cycles on identical inputs, each robot under a task with w != 1 and fn_max of one
    foot 3 N under its unbounded normal force: cycles 2 and 3 hotstart from a warm set of one force row, which
    solve16 accepts from its 1 x 1 system (whose matrix carries w and whose right-hand side -w fref) without a
    working-set change; they end with iters == 0 and a non-zero force multiplier, and pass the certificate."""
    inp, t, fn, cycles = FTD.direct_point_set()
    B = len(inp["contacts"])
    assert np.all(t[:, FT.FT_WEIGHT] != 1.0)
    for k, row in enumerate(cycles):
        for b, c in enumerate(row):
            nz = np.nonzero(FD.lsq_duals48(c, c.qp_solution))[0]
            assert c.qp_status == QP_OK and 1 <= len(nz) <= 2 and nz.max() >= 40, (k, b, nz)
    e = Engine(B)
    e.set_force_bounds(fn)
    e.set_force_task(t)
    n_direct = 0
    for k, row in enumerate(cycles):
        load(e, inp)
        e.step(DUALS_TASK)
        out, d = e.outputs(), e.force_duals()
        n = certify(FTD.DIRECT_SET, row, out, d, inp["contacts"], what=f"direct point cycle {k + 1}")
        assert n == B, (k, n)
        if k > 0:
            n_direct += int(((out["iters"] == 0) & (out["status"] == QP_OK) & d[:, 40:].any(axis=1)).sum())
    e.close()
    print(f"direct point: {n_direct} of {2 * B} robot-cycles of cycles 2 and 3 ended with iters == 0 and a non-zero force multiplier")
    assert n_direct == 2 * B, n_direct


# 3 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rl_random_61", "straight_5"])
def test_nothing_else_moves_cold(name):
    """tau, grf, x, status and iters with the flag are the bits of the same engine without it (ft0 against ftd0) under
    the task and the bounds; WBC_NO_X, WBC_TIMED | WBC_DEBUG and the two older bits beside the flag change nothing;
    device-bound masks with and without WBC_GROUP give every robot the same dual bits."""
    torch = pytest.importorskip("torch")
    inp, t, fn, _ = FTD.cold_set(name + "_tb")
    B = len(inp["contacts"])
    e = engine(inp, force_bounds=fn, force_task=t)
    e.step(STATELESS)
    plain = e.outputs()
    e.step(STATELESS | DUALS_TASK)
    out, d = e.outputs(), e.force_duals()
    assert_identical(out, plain, what=name)
    assert d.shape == (B, 48) and d[:, 40:].any()
    e.step(STATELESS | DUALS_TASK | NO_X)
    o2 = e.outputs()
    for k in ("tau", "grf", "status", "iters"):
        assert np.array_equal(o2[k], plain[k]), (name, k, "NO_X")
    assert np.array_equal(e.force_duals(), d), (name, "duals under NO_X")
    e.step(STATELESS | DUALS_TASK | DUALS | DUALS_FORCE | TIMED | DEBUG)  # (the older bits are ignored beside the flag)
    assert_identical(e.outputs(), plain, what=(name, "DUALS | DUALS_FORCE | TIMED | DEBUG"))
    assert np.array_equal(e.force_duals(), d)
    e.step(STATELESS)
    assert_identical(e.outputs(), plain, what=(name, "unflagged after flagged"))
    with pytest.raises(WbcError):
        e.force_duals()
    masks = torch.from_numpy(inp["contacts"]).cuda()
    torch.cuda.synchronize()
    e.bind_device_inputs(contacts=masks.data_ptr())
    for flags in (STATELESS | GROUP, STATELESS):
        e.step(flags)
        pl = e.outputs()
        e.step(flags | DUALS_TASK)
        assert_identical(e.outputs(), pl, what=(name, "device masks", flags))
        assert np.array_equal(e.force_duals(), d), (name, "device masks", flags)
    e.close()


@pytest.mark.parametrize("flags", [0, COLD], ids=["hotstart", "cold"])
def test_nothing_else_moves_stateful(flags):
    """20 stateful trot steps at B = 8 under table(8, 7) bounds and the sequence's tasks: ftd1's outputs are ft1's bits."""
    B = 8
    fn = FO.table(B)
    seq = list(workloads.trot_sequence(B, steps=20, seed=2))[:20]
    tasks = FT.sequence_tables(seq)
    a, b = Engine(B), Engine(B)
    for e in (a, b):
        e.set_force_bounds(fn)
    for k, s in enumerate(seq):
        for e in (a, b):
            e.set_force_task(tasks[k])
            load(e, s)
        a.step(flags)
        b.step(flags | DUALS_TASK)
        assert_identical(b.outputs(), a.outputs(), what=("trot", flags, k))
    a.close()
    b.close()


@pytest.mark.parametrize("bounds", [False, True], ids=["no_bounds", "bounds7"])
@pytest.mark.parametrize("limits", [False, True], ids=["no_limits", "limits7"])
def test_reduction_to_duals_force(bounds, limits):
    """With no force-task table, with the plain rows set and with them device-bound: all 48 entries and tau, grf, x,
    status and iters are the bits WBC_DUALS_FORCE gives for the same step; cold on every mask and on the stretched
    legs, and over 10 stateful trot steps."""
    torch = pytest.importorskip("torch")
    for name, B in (("rl_random", 45), ("straight", 5)):
        inp = inputs(name, B)
        lm, fn = (LO.table(B) if limits else None), (FO.table(B) if bounds else None)
        ref, dref = run(inp, STATELESS | DUALS_FORCE, limits=lm, force_bounds=fn)
        assert dref.any()
        plain = np.tile(FT.PLAIN, (B, 1))
        for what, ft in (("no table", None), ("plain rows", plain)):
            out, d = run(inp, STATELESS | DUALS_TASK, limits=lm, force_bounds=fn, force_task=ft)
            assert_identical(out, ref, what=(name, what))
            assert np.array_equal(d, dref), (name, what)
        dev = torch.from_numpy(plain.copy()).cuda()
        torch.cuda.synchronize()
        e = engine(inp, limits=lm, force_bounds=fn)
        e.bind_device_force_task(dev)
        e.step(STATELESS | DUALS_TASK)
        assert_identical(e.outputs(), ref, what=(name, "device-bound"))
        assert np.array_equal(e.force_duals(), dref), (name, "device-bound")
        e.close()
    B = 8
    engines = [Engine(B) for _ in range(3)]
    for e in engines:
        if limits:
            e.set_limits(LO.table(B))
        if bounds:
            e.set_force_bounds(FO.table(B))
    engines[2].set_force_task(np.tile(FT.PLAIN, (B, 1)))
    for k, s in enumerate(list(workloads.trot_sequence(B, steps=10, seed=2))[:10]):
        for e in engines:
            load(e, s)
        engines[0].step(DUALS_FORCE)
        dref = engines[0].force_duals()
        for e in engines[1:]:
            e.step(DUALS_TASK)
            assert_identical(e.outputs(), engines[0].outputs(), what=("trot", k))
            assert np.array_equal(e.force_duals(), dref), ("trot", k)
    for e in engines:
        e.close()


# 4 ----------------------------------------------------------------------------------------------
def test_device_bound_task_with_invalid_rows():
    """NaN in fref and weight 0 in a device-bound task table: those robots get WBC_QP_NUMERIC, zero outputs and 48
    zeros; every other robot the bits, multipliers included, of a run without the bad rows (stateless, and the first
    stateful step)."""
    torch = pytest.importorskip("torch")
    inp, t, fn, _ = FTD.cold_set("rl_random_61_tb")
    bad, rows_bad = t.copy(), np.array([4, 17, 60])
    bad[4, 5], bad[17, 12], bad[60, 12] = np.nan, 0.0, np.inf
    others = np.setdiff1d(np.arange(61), rows_bad)
    dev = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    for flags in (STATELESS, 0):
        ref, dref = run(inp, flags | DUALS_TASK, force_bounds=fn, force_task=t)
        e = engine(inp, force_bounds=fn)
        e.bind_device_force_task(dev)
        e.step(flags | DUALS_TASK)
        out, d = e.outputs(), e.force_duals()
        e.close()
        assert np.all(out["status"][rows_bad] == QP_NUMERIC) and not d[rows_bad].any()
        for k in ("tau", "grf", "x"):
            assert not out[k][rows_bad].any(), k
        assert_identical(out, ref, idx_a=others, idx_b=others, what=("others", flags))
        assert np.array_equal(d[others], dref[others]) and dref[rows_bad].any()


def test_a_robot_depends_on_its_own_inputs_only():
    """A permuted batch gives permuted dual bits (B = 61: another wave map, other wave-mates, another padding)."""
    inp, t, fn, _ = FTD.cold_set("rl_random_61_tb")
    out, d = run(inp, STATELESS | DUALS_TASK, force_bounds=fn, force_task=t)
    perm = np.random.default_rng(4).permutation(61)
    pout, pd = run(T.take(inp, perm), STATELESS | DUALS_TASK, force_bounds=fn[perm], force_task=t[perm])
    assert_identical(pout, out, idx_b=perm, what="permuted")
    assert np.array_equal(pd, d[perm])


def test_device_pointer_holds_the_duals():
    torch = pytest.importorskip("torch")
    inp, t, fn, _ = FTD.cold_set("rl_random_61_tb")
    B = 61
    e = engine(inp, force_bounds=fn, force_task=t)
    e.step(STATELESS | DUALS_TASK)
    d = e.force_duals()
    ptr = e.device_force_duals()
    assert ptr
    hip_memcpy = e.lib.hipMemcpy
    hip_memcpy.argtypes, hip_memcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    buf = torch.empty((B, 48), dtype=torch.float64, device="cuda")
    e.synchronize()
    assert hip_memcpy(buf.data_ptr(), ptr, buf.numel() * buf.element_size(), 3) == 0  # hipMemcpyDeviceToDevice
    assert np.array_equal(buf.cpu().numpy(), d) and d[:, 40:].any()
    e.set_force_task(None)
    e.step(STATELESS | DUALS_FORCE)
    assert e.device_force_duals() == ptr  # one buffer for both 48-entry flags
    e.close()


def test_errors():
    """WBC_DUALS_TASK is WBC_ERR_ARG on wbc_update, wbc_solve, wbc_cycle and wbc_step_modes, and on wbc_step with
    WBC_SPLIT, WBC_FUSED or WBC_RESIDENT; WBC_DUALS and WBC_DUALS_FORCE keep their refusals under the task; the
    getters' state in both directions."""
    B = 4
    inp = inputs("rl_random", B)
    e = Engine(B)
    load(e, inp)
    e.update(STATELESS)  # (wbc_solve checks that an update ran before it looks at this flag)
    calls = {
        "wbc_solve": lambda: e.solve(STATELESS | DUALS_TASK),
        "wbc_update": lambda: e.update(STATELESS | DUALS_TASK),
        "wbc_cycle": lambda: T.cycle(e, inp, STATELESS | DUALS_TASK),
    }
    for name, call in calls.items():
        with pytest.raises(WbcError) as ei:
            call()
        assert f"({ERR_ARG})" in str(ei.value) and last_error(e) == f"{name}: WBC_DUALS_TASK is a flag of the default wbc_step", (name, last_error(e))
    for form in (SPLIT, FUSED, RESIDENT):
        for extra in (0, DUALS, DUALS_FORCE):
            with pytest.raises(WbcError) as ei:
                e.step(STATELESS | DUALS_TASK | form | extra)
            assert f"({ERR_ARG})" in str(ei.value)
            # (beside the new flag the older bits are ignored: the refusal names the new one)
            assert last_error(e) == "wbc_step: WBC_DUALS_TASK belongs to the default form (not WBC_SPLIT / WBC_FUSED / WBC_RESIDENT)"
    e.set_modes([15, 5])
    with pytest.raises(WbcError) as ei:
        e.step_modes(STATELESS | DUALS_TASK)
    assert f"({ERR_ARG})" in str(ei.value) and last_error(e) == "wbc_step_modes: WBC_DUALS_TASK is a flag of the default wbc_step"
    e.set_modes(None)
    load(e, inp)
    # the getters in both directions, without a table
    e.step(STATELESS | DUALS)
    assert e.duals().shape == (B, 40)
    with pytest.raises(WbcError):
        e.force_duals()
    e.step(STATELESS | DUALS_TASK)
    assert e.force_duals().shape == (B, 48) and e.device_force_duals()
    for get, nm in ((e.duals, "wbc_get_duals"), (e.device_duals, "wbc_device_duals")):
        with pytest.raises(WbcError) as ei:
            get()
        assert f"({ERR_STATE})" in str(ei.value) and last_error(e).startswith(f"{nm}: the last wbc_step carried WBC_DUALS_FORCE")
    e.step(STATELESS | DUALS)
    assert e.duals().shape == (B, 40)
    # under the task: the older flags keep their refusals, letter for letter; the new flag runs
    t = FT.table(B, 11, inp["contacts"])
    e.set_force_task(t)
    for flag, nm in ((DUALS, "WBC_DUALS"), (DUALS_FORCE, "WBC_DUALS_FORCE")):
        with pytest.raises(WbcError) as ei:
            e.step(STATELESS | flag)
        assert f"({ERR_STATE})" in str(ei.value)
        assert last_error(e) == (f"wbc_step: {nm} with a per-robot force task in force (no duals instance reads the table; clear it "
                                 "with wbc_set_force_task(h, NULL))")
    with pytest.raises(WbcError) as ei:  # every existing check first: the table's own refusal of the split form
        e.step(STATELESS | DUALS_TASK | SPLIT)
    assert f"({ERR_STATE})" in str(ei.value)
    assert last_error(e) == "wbc_step: WBC_SPLIT with a per-robot force task in force (default form only; clear it with wbc_set_force_task(h, NULL))"
    ref, _ = run(inp, STATELESS, force_task=t)
    e.step(STATELESS | DUALS_TASK)
    assert_identical(e.outputs(), ref, what="flagged under the task")
    d = e.force_duals()
    assert d.any()
    e.step(STATELESS)
    assert_identical(e.outputs(), ref, what="unflagged after flagged")
    for get in (e.force_duals, e.device_force_duals, e.duals, e.device_duals):
        with pytest.raises(WbcError) as ei:
            get()
        assert f"({ERR_STATE})" in str(ei.value)
    e.step(STATELESS | DUALS_TASK)
    assert np.array_equal(e.force_duals(), d)
    e.close()


def test_each_unit_is_reached():
    """B = 5: the stateless step (ftd0) and the stateful one (ftd1) both report, under a task of w = 50 that pulls
    every foot to 110 N, the multipliers of an fn_max of 40 N: on the fn_max side, on feet that sit at 40 N, and about
    w times what WBC_DUALS_FORCE reports for the same bound without the task's pull."""
    B = 5
    inp = inputs("stance_cold", B)
    e = Engine(B)
    e.set_force_bounds(dict(fn_max=40.0))
    e.set_force_task(dict(f_ref=np.tile([0.0, 0.0, 110.0], 4).reshape(4, 3), weight=50.0))
    load(e, inp)
    for flags in (STATELESS, 0):
        e.step(flags | DUALS_TASK)
        out, d = e.outputs(), e.force_duals()
        assert np.all(out["status"] == QP_OK)
        nf = FO.normal_forces(out["grf"])
        r = dual_rows(d)["force"]
        assert (r <= 0).all() and (r < 0).any(axis=1).all(), (flags, r)
        assert np.all(np.abs(nf[r < 0] - 40.0) <= 1e-7) and not r[nf < 40.0 - 1e-6].any(), (flags, nf, r)
        assert np.abs(r).max() > 50.0 * 10.0, r  # w (110 - 40) less what the dynamics take: the multipliers grow with w
    e.close()
