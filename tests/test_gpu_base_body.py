"""GPU: the per-robot base body (wbc_set_base_body / wbc_bind_device_base_body / wbc_get_base_body,
include/wbc.h): a [B][14] table from which the default step takes each robot's base mass, CoM and
inertia, a payload on the trunk (wbc_kernel_bb0.hip stateless, wbc_kernel_bb1.hip stateful,
wbc_kernel_bbs.hip for all-stance stateless steps).

The checkers are tests/base_body_oracle.py's: the C and numpy oracles given one model per robot.  The
tables are base_body_oracle.payload_rows(B): a point payload of up to 60 % of the base mass somewhere
on the trunk; the input sets are tests/table_steps.py's inputs(name, B) (seed 91; the straight-leg set
from seed 81), on which the C oracle returns WBC_QP_OK for every robot under these payloads; bounds are
tests/margins.py's."""
import ctypes as C

import numpy as np

import margins as M
import pytest

import base_body_oracle as BB
import contact_normals_oracle as CN
import stateful_sequences as S
import table_steps as T
import wbc_ref as R
from quadrupedwholebodycontroller_amd import (COLD, DEBUG, FUSED, GROUP, QP_NUMERIC, QP_OK, RESIDENT, SPLIT, STATELESS, Engine,
                                              WbcError, split_debug, workloads)
from table_steps import (ERR_ARG, ERR_STATE, assert_identical, check_against_c_oracles, inputs, last_error, load, moved,
                         row_dict)
from table_steps import table as rp_table

pytestmark = pytest.mark.gpu

BODY = T.Table("base_body")
_ORACLE = {}


def oracle(name, B):
    """(inputs, payload rows, LITERAL and REDUCED C oracle outputs with robot b under row b), computed once."""
    key = (name, B)
    if key not in _ORACLE:
        inp, rows = inputs(name, B), BB.payload_rows(B)
        _ORACLE[key] = (inp, rows, BB.c_run_batch(inp, rows, R.LITERAL), BB.c_run_batch(inp, rows, R.REDUCED))
    return _ORACLE[key]


def run(inp, rows=None, t=None, nrm=None, flags=STATELESS):
    return T.run(inp, flags, robot_params=t, contact_normals=nrm, base_body=rows)


# 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("stance_cold", 64), ("rl_random", 61), ("rl_random", 5), ("straight", 64)])
def test_payload_matches_oracle_cold(name, B):
    """Cold steps under payload_rows against the C oracle on every robot: host-copied masks (the
    stance-only instance on the all-stance sets, the wave map on rl_random), then device-bound masks with
    and without WBC_GROUP.  B = 61 and 5 leave a ragged last wave; every fifth robot of the straight-leg
    set takes the in-wave fallback, which reads nothing of the table (its problem record carries the
    robot's mass and inertia) and still must give the payload's torques.  Status as the LITERAL oracle's
    (all OK here), tau / x / grf within the margins, iters as the REDUCED oracle's with no allowance (on
    the straight set for the bent robots, as in tests/test_gpu_robot_params.py)."""
    torch = pytest.importorskip("torch")
    inp, rows, lit, red = oracle(name, B)
    assert np.all(lit["status"] == QP_OK), lit["status"]
    bent = np.nonzero(np.arange(B) % 5 != 0)[0] if name == "straight" else None
    out = run(inp, rows)
    check_against_c_oracles(out, lit, red, name, bent)
    if name == "straight":
        fb = np.arange(0, B, 5)
        d = np.abs(run(inp)["tau"][fb] - out["tau"][fb]).max(axis=1)
        print(f"straight robots: tau moved by {d.min():.3g} .. {d.max():.3g} N m")
        assert np.all(d > 1e-3), d
    e = Engine(B)
    load(e, inp)
    e.set_base_body(rows)
    masks = torch.from_numpy(inp["contacts"]).cuda()
    torch.cuda.synchronize()
    e.bind_device_inputs(contacts=masks.data_ptr())
    for flags in (STATELESS | GROUP, STATELESS):
        e.step(flags)
        check_against_c_oracles(e.outputs(), lit, red, f"{name}, device masks, flags {flags}", bent)
    e.close()


# 2 ----------------------------------------------------------------------------------------------
def test_intermediates_under_debug():
    """WBC_DEBUG at B = 8 (mixed masks) against the numpy oracle with one model per robot."""
    B = 8
    inp, rows = inputs("rl_random", B), BB.payload_rows(B)
    e = Engine(B)
    load(e, inp)
    e.set_base_body(rows)
    e.step(STATELESS | DEBUG)
    out, dbg = e.outputs(), e.debug()
    e.close()
    for b in range(B):
        c = BB.np_controller(inp, b, rows[b])
        c.step()
        d, ref = split_debug(dbg[b]), c.debug_record()
        for k in ("com", "comvel", "Mbar_b", "Mbar_j", "Jbar", "W"):
            err = np.max(np.abs(d[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k])))
            assert M.record(k, err, M.INTERMEDIATE[k]) < M.INTERMEDIATE[k], (b, k, err)
        assert out["status"][b] == c.qp_status, b
        if c.qp_status == QP_OK:
            assert M.close(out["tau"][b], c.tau, M.TAU, "tau"), b


# 3 ----------------------------------------------------------------------------------------------
def test_the_table_is_read():
    """A table that is accepted and ignored cannot pass: at least 60 of 64 robots' torques move by more
    than 1e-3 N m against the same engine's plain step (the C oracle: 64 of 64)."""
    B = 64
    inp, rows, lit, _ = oracle("stance_cold", B)
    assert moved(lit, R.run_batch(inp)) == B
    e = Engine(B)
    load(e, inp)
    e.step(STATELESS)
    plain = e.outputs()
    e.set_base_body(rows)
    assert np.array_equal(e.base_body(), rows)
    e.step(STATELESS)
    out = e.outputs()
    e.close()
    n = moved(out, plain)
    print(f"{n} of {B} robots' tau moved by the payload")
    assert n >= 60, n


# 4 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [64, 5])
@pytest.mark.parametrize("others", ["alone", "params", "flat", "sloped", "params+sloped"])
def test_default_row_is_the_plain_step(others, B):
    """The model's own base as every robot's row gives the bits of the step without the table: alone,
    with the rng(7) parameter table, with flat and with sloped normals; all-stance and mixed masks cold,
    and 20 stateful trot steps."""
    t = rp_table(B) if "params" in others else None
    nrm = np.array([0.0, 0.0, 1.0]) if others == "flat" else CN.normals(B, 5, 0.35) if "sloped" in others else None
    e = Engine(B)
    row = e.base_body()
    assert np.array_equal(row, np.tile(BB.default_row(), (B, 1)))
    e.close()
    for name in ("stance_cold", "rl_random"):
        inp = inputs(name, B)
        assert_identical(run(inp, row, t, nrm), run(inp, None, t, nrm), what=(others, name))
        assert_identical(run(inp, row[0], t, nrm), run(inp, None, t, nrm), what=(others, name, "one row"))
    seq = list(workloads.trot_sequence(B, steps=20, seed=2))[:20]
    engines = [Engine(B), Engine(B)]
    for e in engines:
        if t is not None:
            e.set_robot_params(t)
        if nrm is not None:
            e.set_contact_normals(nrm)
    engines[1].set_base_body(row)
    for k, inp in enumerate(seq):
        outs = []
        for e in engines:
            load(e, inp)
            e.step(0)
            outs.append(e.outputs())
        assert_identical(outs[1], outs[0], what=(others, "trot", k))
    for e in engines:
        e.close()


# 5 ----------------------------------------------------------------------------------------------
def test_all_three_tables_at_once():
    """rng(7) parameters, normals(B, 5, 0.35) and the payload at B = 16 (mixed masks), against the numpy
    oracle of tests/contact_normals_oracle.py given each robot's own model, parameters and normals."""
    B = 16
    inp, rows, t, nrm = inputs("rl_random", B), BB.payload_rows(B), rp_table(B), CN.normals(B, 5, 0.35)
    ref = BB.np_run_batch(inp, rows, [row_dict(t[b]) for b in range(B)], CN.SlopedWBC, [dict(normals=nrm[b]) for b in range(B)])
    out = run(inp, rows, t, nrm)
    assert np.sum(ref["status"] == QP_OK) >= B - 4, ref["status"]
    T.check_against_oracle(out, ref, "three tables")


# 6 ----------------------------------------------------------------------------------------------
def test_a_robot_depends_on_its_own_row_only():
    """A permuted batch gives permuted bits, and changing one robot's row changes that robot alone."""
    B = 61
    inp, rows, _, _ = oracle("rl_random", B)
    T.own_row_only(BODY, inp, rows, 17, BB.payload_rows(B, seed=12)[17])


# 7 ----------------------------------------------------------------------------------------------
def test_stateful_trot_with_the_table_swapped():
    """130 trot steps at B = 6 (the mask switch at step 100), the table swapped at step 60 (payload seeds
    11 and 12), against one stateful C oracle robot per row whose model is swapped at the same step: the
    history is not touched, so the finite differences of step 60 see the change as the reference's would
    see a changed model.  tau and x at the stateful margins; the same run under WBC_COLD within 1e-9."""
    B, steps, swap = 6, 130, 60
    tables = [BB.payload_rows(B, seed=11), BB.payload_rows(B, seed=12)]
    robots = [BB.CRobot(tables[0][b]) for b in range(B)]
    hot, cold, plain = Engine(B), Engine(B), Engine(B)
    n_ok = n_moved = 0
    for k, inp in enumerate(workloads.trot_sequence(B, steps=steps, seed=2)):
        if k in (0, swap):
            rows = tables[0 if k == 0 else 1]
            for e in (hot, cold):
                e.set_base_body(rows)
            for b in range(B):
                robots[b].set_row(rows[b])
        for e in (hot, cold, plain):
            load(e, inp)
        hot.step(0)
        cold.step(COLD)
        plain.step(0)
        oh, oc, op = hot.outputs(), cold.outputs(), plain.outputs()
        assert np.array_equal(oh["status"], oc["status"]), k
        for b in range(B):
            o = robots[b].step(inp["base_pose"][b], inp["nu"][b], inp["qj"][b], inp["ref"][b], inp["contacts"][b], inp["switching"][b])
            assert oh["status"][b] == o["status"], (k, b)
            if o["status"] == QP_OK:
                assert M.close(oh["tau"][b], o["tau"], M.STATEFUL_TAU, "tau"), (k, b)
                assert M.close(oh["x"][b], o["x"], M.STATEFUL_X, "x"), (k, b)
                assert M.close(oc["tau"][b], oh["tau"][b], 1e-9, "tau, WBC_COLD"), (k, b)
                n_ok += 1
        n_moved += moved(oh, op)
    for e in (hot, cold, plain):
        e.close()
    print(f"{n_ok} of {B * steps} solves OK, {n_moved} robot-steps moved by the payload")
    assert n_ok > B * steps // 2 and n_moved > B * steps // 2


# 8 ----------------------------------------------------------------------------------------------
def test_device_bound_table_with_invalid_rows():
    """NaN, zero mass, an asymmetric and an indefinite inertia in a device-bound table: those robots get
    WBC_QP_NUMERIC and zeros, every other robot the bits of a run without the bad rows (stateless, and
    the first stateful step of a fresh engine)."""
    inp, rows, _, _ = oracle("rl_random", 61)
    I = rows[0, 4:13].reshape(3, 3)
    asym = I.copy()
    asym[0, 1] += 1e-6 * np.trace(I)
    bad = rows.copy()
    bad[3, 2] = np.nan
    bad[17, 0] = 0.0
    bad[30, 4:13] = asym.ravel()
    bad[44, 4:13] = np.diag([1.0, -1.0, 1.0]).ravel()
    bad[60, 12] = np.inf
    T.device_bound_invalid_rows(BODY, inp, rows, bad, np.array([3, 17, 30, 44, 60]))  # (the reserved column reads back as 0)


# 8b ---------------------------------------------------------------------------------------------
def test_device_bound_row_invalid_for_one_cycle():
    """A device-bound table in a stateful run (B = 8, the first 40 cycles of the latched off-trot sequence of
    tests/stateful_sequences.py) whose row for robot 3 holds a NaN CoM on cycle 20 only: that robot returns
    WBC_QP_NUMERIC and zeros on that cycle, and every other robot has, on all 40 cycles, the bits of a run
    whose table never held the bad row.

    What robot 3 returns after the row is valid again is recorded here and in DESIGN.md 18, not asserted
    against an oracle (the reference has no such state): the flagged cycle marks the robot's first input
    non-finite and its history takes that (e_int, Tdot_inv, the old Jacobian forms).  On MI355X, cycles
    21..39, masks 0 0 0 4 4 4 0 0 0 5 5 5 0 0 0 6 6 6 0 with a latched change every third cycle: status
    WBC_QP_OK on all 19; cycle 21 (all-swing, still reading Tdot_inv) non-finite tau and x; the other
    all-swing cycles (22-23, 27-29, 33-35, 39) the clean run's bits; every cycle with a stance leg (24-26,
    30-32, 36-38) non-finite tau and x, through W's ki * e_int term.  The test prints this record.  A reset
    of the robot clears it: after cycle 39 robot 3 is reset in both runs, and six more cycles must give both
    runs the same bits on every robot (asserted: engine against engine)."""
    torch = pytest.importorskip("torch")
    B, steps, at, who, more = 8, 40, 20, 3, 6
    rows = BB.payload_rows(B)
    seq = S.sequence(B, 3, 5, True)[:steps + more]
    runs = {}
    for name in ("clean", "bad"):
        d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        torch.cuda.synchronize()
        e = Engine(B)
        e.bind_device_base_body(d)
        outs = []
        for k, s in enumerate(seq):
            if name == "bad" and k in (at, at + 1):
                d[who, 2] = float("nan") if k == at else float(rows[who, 2])
                torch.cuda.synchronize()
            if k == steps:
                e.reset((np.arange(B) == who).astype(np.uint8))
            e.set_state(s["base_pose"], s["nu"], s["qj"])
            e.set_reference(s["ref"], s["contacts"], s["switching"])
            e.step(0)
            outs.append(e.outputs())
        e.close()
        runs[name] = {k: np.array([o[k] for o in outs]) for k in ("tau", "grf", "x", "status", "iters")}
    clean, bad = runs["clean"], runs["bad"]
    assert np.sum(clean["status"] == QP_OK) >= 0.9 * steps * B
    assert bad["status"][at, who] == QP_NUMERIC
    for k in ("tau", "grf", "x"):
        assert not bad[k][at, who].any(), k
    others = np.arange(B) != who
    for k in ("tau", "grf", "x", "status", "iters"):
        assert np.array_equal(bad[k][:, others], clean[k][:, others]), k
        assert np.array_equal(bad[k][:at, who], clean[k][:at, who]), k
        assert np.array_equal(bad[k][steps:], clean[k][steps:]), (k, "after the reset")
    assert np.isfinite(bad["tau"][steps:]).all() and np.isfinite(bad["x"][steps:]).all()
    after = bad["status"][at + 1:steps, who]
    kinds = "".join("=" if all(np.array_equal(bad[k][c, who], clean[k][c, who]) for k in ("tau", "grf", "x", "status", "iters"))
                    else "n" if not (np.isfinite(bad["tau"][c, who]).all() and np.isfinite(bad["x"][c, who]).all()) else "d"
                    for c in range(at + 1, steps))
    print(f"robot {who}, cycles {at + 1}..{steps - 1} (= the clean run's bits, d finite but different, n not finite): {kinds}; "
          f"status {after.tolist()}, clean {clean['status'][at + 1:steps, who].tolist()}; masks {[int(s['contacts'][who]) for s in seq[at:steps]]}, "
          f"switching {[int(s['switching'][who]) for s in seq[at:steps]]}; "
          f"worst |tau - clean| on the d cycles {max([np.abs(bad['tau'][c, who] - clean['tau'][c, who]).max() for c in range(at + 1, steps) if kinds[c - at - 1] == 'd'], default=0.0):.3g}")


# 9 ----------------------------------------------------------------------------------------------
REFUSALS = T.refusal_texts("a per-robot base body table is in force", "a per-robot base body table in force",
                           "clear it with wbc_set_base_body(h, NULL)")
assert REFUSALS["cycle_resident"] == ("wbc_cycle: WBC_RESIDENT with a per-robot base body table in force (plain cycle only; "
                                      "clear it with wbc_set_base_body(h, NULL))")
assert REFUSALS["step_modes"] == ("wbc_step_modes: a per-robot base body table is in force (default wbc_step only; clear it with "
                                  "wbc_set_base_body(h, NULL))")


def test_host_validation_refusals_cycle_and_clearing():
    B = 4
    inp, rows = inputs("rl_random", B), BB.payload_rows(B)
    e = Engine(B)
    load(e, inp)
    e.set_base_body(rows)
    # host validation through the C call (the Python table form validates first: tested on the CPU)
    for b, col, v, nm in ((2, 0, 0.0, "mass"), (1, 3, np.nan, "com_z"), (3, 8, -1.0, "I_yy"), (0, 5, 1.0, "I_xy")):
        t = rows.copy()
        t[b, col] = v
        rc = e.lib.wbc_set_base_body(e.h, t.ctypes.data_as(C.c_void_p))
        assert rc == ERR_ARG and last_error(e).startswith(f"wbc_set_base_body: row {b}, column {col} ({nm}) = "), last_error(e)
        assert last_error(e).endswith(": need finite entries, mass > 0 and a symmetric (to 1e-9 of its trace), positive definite inertia")
        assert np.array_equal(e.base_body(), rows)  # the old table stays in force
    assert e.lib.wbc_bind_device_base_body(e.h, 8) == ERR_ARG  # not 16-byte aligned
    assert last_error(e) == "wbc_bind_device_base_body: the table must be 16-byte aligned"
    t = rows.copy()
    t[:, 13] = np.nan  # the reserved column: ignored on input, read back as 0
    assert e.lib.wbc_set_base_body(e.h, t.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(e.base_body(), rows)
    # the step, and the plain wbc_cycle equal to it
    e.step(STATELESS)
    out = e.outputs()
    assert moved(out, run(inp)) == B
    assert_identical(T.cycle(e, inp, STATELESS), out, what="cycle")
    # refusals, letter for letter
    T.refused_forms(e, inp, REFUSALS)
    # the other tables are named first, as before
    e.set_contact_normals(np.array([0.0, 0.0, 1.0]))
    with pytest.raises(WbcError):
        e.update(STATELESS)
    assert last_error(e) == "wbc_update: contact normals are in force (default wbc_step only; clear them with wbc_set_contact_normals(h, NULL))"
    e.set_contact_normals(None)
    e.set_base_body(None)
    e.set_modes([15, 5])
    e.set_base_body(rows)
    with pytest.raises(WbcError) as ei:
        e.step_modes(STATELESS)
    assert last_error(e) == REFUSALS["step_modes"] and f"({ERR_STATE})" in str(ei.value)
    # cleared: wbc_step_modes and every other form run again and match an engine that never had the table
    e.set_base_body(None)
    assert np.array_equal(e.base_body(), np.tile(BB.default_row(), (B, 1)))
    f = Engine(B)
    T.cleared_matches_fresh(e, f, inp, (STATELESS, STATELESS | SPLIT, STATELESS | FUSED, 0), (STATELESS, STATELESS | RESIDENT))
    for eng in (e, f):
        eng.close()


@pytest.mark.parametrize("step", ["all_stance", "mixed", "stateful"])
def test_each_unit_is_reached(step):
    """B = 5: two waves, the second ragged.  Under the payload an all-stance stateless step (bbs), a
    mixed-mask stateless step (bb0) and a stateful step (bb1) each match the C oracle, and move the
    torques of all five robots against the plain step; that the right cell of the launcher table is chosen
    is tests/test_base_body_cpu.py's."""
    B = 5
    inp = inputs("stance_cold" if step == "all_stance" else "rl_random", B)
    rows = BB.payload_rows(B)
    flags = 0 if step == "stateful" else STATELESS
    out, plain = run(inp, rows, flags=flags), run(inp, flags=flags)
    lit = BB.c_run_batch(inp, rows, R.LITERAL)  # (a fresh engine's first stateful step is a cold one)
    assert np.array_equal(out["status"], lit["status"])
    for b in np.nonzero(lit["status"] == QP_OK)[0]:
        assert M.close(out["tau"][b], lit["tau"][b], M.TAU, "tau"), (step, b)
    assert moved(out, plain) == B
