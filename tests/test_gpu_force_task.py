"""GPU: per-robot reference contact forces (wbc_set_force_task / wbc_bind_device_force_task / wbc_get_force_task,
include/wbc.h): a [B][14] table from which the default step takes 1/2 w |f_l - fref_l|^2 in place of 1/2 |f_l|^2 for
every stance foot (wbc_kernel_ft0.hip stateless, wbc_kernel_ft1.hip stateful).

The checker is tests/force_task_oracle.py: the numpy oracle with the weight on the stance forces' diagonal and
w fref off their gradient, on the shared sets under table(B, 11, contacts) (every robot OK there and the forces
moved on most: tests/test_force_task_cpu.py).  Bounds are tests/margins.py's."""
import ctypes as C

import numpy as np

import margins as M
import pytest

import base_body_oracle as BB
import contact_normals_oracle as CN
import force_bounds_oracle as FO
import force_task_oracle as FT
import limits_oracle as LO
import table_steps as T
from quadrupedwholebodycontroller_amd import (COLD, DEBUG, DUALS, DUALS_FORCE, FUSED, GROUP, NO_X, QP_OK, RESIDENT, SPLIT, STATELESS,
                                              TIMED, Engine, WbcError, force_task_row, workloads)
from table_steps import ERR_ARG, ERR_STATE, assert_identical, inputs, last_error, load, row_dict
from table_steps import table as rp_table

pytestmark = pytest.mark.gpu

INF = np.inf


def run(inp, ft=None, fn=None, lm=None, t=None, nrm=None, rows=None, flags=STATELESS):
    """One step of a fresh engine under the given tables, set in the engine's order, the force task last."""
    e = Engine(len(inp["contacts"]))
    load(e, inp)
    for name, tab in (("robot_params", t), ("contact_normals", nrm), ("base_body", rows), ("limits", lm), ("force_bounds", fn),
                      ("force_task", ft)):
        if tab is not None:
            getattr(e, "set_" + name)(tab)
    e.step(flags)
    out = e.outputs()
    e.close()
    return out


class ForceTaskTable(T.Table):
    def run(self, inp, t, flags=STATELESS):
        return run(inp, t, flags=flags)


FTT = ForceTaskTable("force_task")


def check_against_oracle(out, ref, what):
    """table_steps.check_against_oracle, and zero outputs on the robots the oracle did not solve."""
    T.check_against_oracle(out, ref, what)
    for k in ("tau", "grf", "x"):
        assert not out[k][ref["status"] != QP_OK].any(), (what, k)


# 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FT.COLD)
def test_seed11_table_matches_oracle_cold(name):
    """Cold steps under table(B, 11, contacts) against the oracle on every robot: host masks, then device-bound
    masks with and without WBC_GROUP.  stance_cold runs the stance form with the weighted rank-6 factor, rl_random
    at B = 61 the general form of all 16 masks with a ragged last wave, the straight-leg set the in-wave fallback
    (tags 22 / 23), which reads the robot's own row."""
    torch = pytest.importorskip("torch")
    inp, t, ref = FT.cold_set(name)
    B = len(inp["contacts"])
    assert np.all(ref["status"] == QP_OK)
    out = run(inp, t)
    check_against_oracle(out, ref, name)
    e = Engine(B)
    load(e, inp)
    e.set_force_task(t)
    assert np.array_equal(e.force_task(), t)
    masks = torch.from_numpy(inp["contacts"]).cuda()
    torch.cuda.synchronize()
    e.bind_device_inputs(contacts=masks.data_ptr())
    for flags in (STATELESS | GROUP, STATELESS):
        e.step(flags)
        check_against_oracle(e.outputs(), ref, f"{name}, device masks, flags {flags}")
    e.close()
    # the task moved the forces
    assert FT.moved_robots(out["grf"], run(inp)["grf"]) == FT.moved_robots(ref["grf"], FT.plain_set(name)[2]["grf"]) >= B - 11


# 2 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [61, 5])
def test_default_row_is_the_force_bound_step(B):
    """What wbc_get_force_task returns without a table (0 x 12, 1, 0), set as the table or bound as a device table,
    gives the force-bound instance's bits under seed-7 limits and force-bound tables (tau, grf, x, status, iters):
    cold on all-stance, mixed masks and stretched legs."""
    torch = pytest.importorskip("torch")
    e = Engine(B)
    plain = e.force_task()
    assert np.array_equal(plain, np.tile(force_task_row(), (B, 1))) and np.array_equal(plain[0], FT.PLAIN)
    e.close()
    lm, fn = LO.table(B), FO.table(B)
    dev = torch.from_numpy(plain.copy()).cuda()
    torch.cuda.synchronize()
    for name in ("stance_cold", "rl_random", "straight"):
        inp = inputs(name, B)
        ref = run(inp, None, fn, lm)
        assert_identical(run(inp, plain, fn, lm), ref, what=name)
        e = Engine(B)
        load(e, inp)
        e.set_limits(lm)
        e.set_force_bounds(fn)
        e.bind_device_force_task(dev)
        e.step(STATELESS)
        assert_identical(e.outputs(), ref, what=(name, "device-bound"))
        e.close()


@pytest.mark.parametrize("name", FT.COLD)
def test_default_row_is_the_plain_step(name):
    """With every other table at its default the row (0 x 12, 1, 0), set or device-bound, gives the plain step's bits
    on the three cold sets: stance_cold_64 runs the stance form, whose rank-6 factor takes w = 1 and c = 1."""
    torch = pytest.importorskip("torch")
    inp = FT.SETS[name]()
    B = len(inp["contacts"])
    plain = np.tile(FT.PLAIN, (B, 1))
    ref = run(inp)
    assert_identical(run(inp, plain), ref, what=name)
    dev = torch.from_numpy(plain.copy()).cuda()
    torch.cuda.synchronize()
    e = Engine(B)
    load(e, inp)
    e.bind_device_force_task(dev)
    e.step(STATELESS)
    assert_identical(e.outputs(), ref, what=(name, "device-bound"))
    e.close()


def test_default_row_over_stateful_trot_steps():
    """20 stateful trot steps at B = 5: the default row gives the plain step's bits with no other table, and the
    force-bound instance's under seed-7 limits and force-bound tables."""
    B = 5
    lm, fn, plain = LO.table(B), FO.table(B), np.tile(FT.PLAIN, (B, 1))
    engines = [Engine(B) for _ in range(4)]
    for e in engines[:2]:
        e.set_limits(lm)
        e.set_force_bounds(fn)
    engines[1].set_force_task(plain)
    engines[3].set_force_task(plain)
    for k, inp in enumerate(list(workloads.trot_sequence(B, steps=20, seed=2))[:20]):
        outs = []
        for e in engines:
            load(e, inp)
            e.step(0)
            outs.append(e.outputs())
        assert_identical(outs[1], outs[0], what=("trot, force bounds", k))
        assert_identical(outs[3], outs[2], what=("trot, plain", k))
    for e in engines:
        e.close()


# 3 ----------------------------------------------------------------------------------------------
def test_swing_feet_entries_are_not_read():
    """Changing the fref entries of every swing foot on rl_random_61 changes no bit."""
    inp, t, _ = FT.cold_set("rl_random_61")
    swing = np.repeat(~FT.stance(inp["contacts"]), 3, axis=1)
    assert swing.any() and (~swing).any()
    t2 = t.copy()
    t2[:, :12][swing] = np.random.default_rng(5).uniform(-500.0, 500.0, int(swing.sum()))
    assert_identical(run(inp, t2), run(inp, t), what="swing fref")


# 4 ----------------------------------------------------------------------------------------------
def test_distance_to_the_reference_falls_with_the_weight():
    """stance_cold_64 under one fref and w = 0.1, 1, 10, 100 on every robot: each robot's sum over its stance feet of
    |f - fref|^2 does not increase (1e-9 relative slack) and is the oracle's to 1e-9 (1 + |d|)."""
    inp = FT.cold_set("stance_cold_64")[0]
    prev = None
    for w, t, ref in FT.weight_sweep("stance_cold_64"):
        out = run(inp, t)
        assert np.all(out["status"] == QP_OK), w
        d, want = FT.distances(out["grf"], t, inp["contacts"]), FT.distances(ref["grf"], t, inp["contacts"])
        err = float(np.max(np.abs(d - want) / (1.0 + np.abs(want))))
        M.record(f"distance, w = {w}", err, 1e-9)
        assert err <= 1e-9, (w, err)
        if prev is not None:
            assert np.all(d <= prev * (1.0 + 1e-9) + 1e-9), (w, float(np.max(d - prev)))
        prev = d


# 5 ----------------------------------------------------------------------------------------------
def test_all_six_tables_at_once():
    """rng(7) parameters, sloped normals, payload base bodies, limits table(B, 7), force bounds table(B, 7) and the
    force task table(B, 11, contacts) at B = 16 (mixed masks) against the oracle given each robot's own model,
    parameters, normals, limits, bounds and task; the same without a limits table (the parameter table's own
    max_torque and friction stand)."""
    B = 16
    inp = inputs("rl_random", B)
    t, nrm, rows, lm, fn = rp_table(B), CN.normals(B, 5, 0.35), BB.payload_rows(B), LO.table(B), FO.table(B)
    ft = FT.table(B, 11, inp["contacts"])
    prm = [row_dict(t[b]) for b in range(B)]
    want = FT.run_batch(inp, ft, fn, lm, prm, nrm, rows)
    assert np.sum(want["status"] == QP_OK) >= B - 4, want["status"]
    out = run(inp, ft, fn, lm, t, nrm, rows)
    check_against_oracle(out, want, "six tables")
    assert FT.moved_robots(out["grf"], run(inp, None, fn, lm, t, nrm, rows)["grf"]) >= B // 2
    want = FT.run_batch(inp, ft, fn, np.array([LO.row(-r[1], r[1], r[0]) for r in t]), prm, nrm, rows)
    check_against_oracle(run(inp, ft, fn, None, t, nrm, rows), want, "five tables, no limits")


# 6 ----------------------------------------------------------------------------------------------
def test_a_robot_depends_on_its_own_row_only():
    """A permuted batch gives permuted bits, and changing one robot's row changes that robot alone."""
    inp, t, _ = FT.cold_set("rl_random_61")
    b = 20
    assert inp["contacts"][b] != 0
    T.own_row_only(FTT, inp, t, b, force_task_row(t[b, :12] + 40.0, 50.0))


# 7 ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequence_runs():
    """The stateful sequence on the engine, hotstarted and under WBC_COLD: the table rewritten into a device-bound
    tensor every cycle, every robot reset before cycle RESET_AT; per run the outputs of every cycle."""
    torch = pytest.importorskip("torch")
    S = FT.sequence_reference()
    B = S["B"]
    runs = {}
    for flags in (0, COLD):
        e = Engine(B)
        dev = torch.from_numpy(S["tables"][0].copy()).cuda()
        torch.cuda.synchronize()
        e.bind_device_force_task(dev)
        outs = []
        for k, inp in enumerate(S["seq"]):
            if k == FT.RESET_AT:
                e.reset()
            e.synchronize()
            dev.copy_(torch.from_numpy(S["tables"][k]))
            torch.cuda.synchronize()
            load(e, inp)
            e.step(flags)
            outs.append(e.outputs())
        e.close()
        runs[flags] = outs
    return runs


@pytest.mark.parametrize("flags", [0, COLD], ids=["hotstart", "cold"])
def test_stateful_sequence(sequence_runs, flags):
    """B = 8, 130 trot steps, a fresh table(8, 100 + k, contacts) every cycle under weights 10 ** linspace(-1, 2, 8),
    against the stateful oracle per cycle and robot at the stateful margins; status identical on every solve (the
    oracle's are all OK); the task moves the forces by more than 1 N on every robot."""
    S = FT.sequence_reference()
    B = S["B"]
    moved = np.zeros(B, bool)
    for k, out in enumerate(sequence_runs[flags]):
        for b in range(B):
            tau, x, grf, s = S["ref"][k][b]
            assert s == QP_OK and out["status"][b] == s, (k, b)
            assert M.close(out["tau"][b], tau, M.STATEFUL_TAU, "tau"), (k, b)
            assert M.close(out["x"][b], x, M.STATEFUL_X, "x"), (k, b)
            moved[b] |= np.abs(out["grf"][b] - S["plain_grf"][k][b]).max() > 1.0
    assert moved.all(), moved


HOT_COLD = 100 * M.BITS  # the hotstarted and the cold run of one kernel on one QP: two orders of additions to one optimum


def test_sequence_hotstarted_and_cold_agree(sequence_runs):
    for k, (a, b) in enumerate(zip(sequence_runs[0], sequence_runs[COLD])):
        assert np.array_equal(a["status"], b["status"]), k
        for r in range(len(a["status"])):
            assert M.close(a["tau"][r], b["tau"][r], HOT_COLD, "tau hot/cold"), (k, r)
            assert M.close(a["x"][r], b["x"][r], HOT_COLD, "x hot/cold"), (k, r)


# 8 ----------------------------------------------------------------------------------------------
def test_device_bound_table_with_invalid_rows():
    """NaN and inf in fref, weight 0, -1, NaN and +inf in a device-bound table: those robots get WBC_QP_NUMERIC and
    zeros, every other robot the bits of a run without the bad rows (stateless and the first stateful step); an
    unbind restores the host table."""
    inp, t, _ = FT.cold_set("rl_random_61")
    bad = t.copy()
    bad[4, 5] = np.nan
    bad[13, 11] = INF
    bad[17, 12] = 0.0
    bad[30, 12] = -1.0
    bad[44, 12] = np.nan
    bad[60, 12] = INF
    T.device_bound_invalid_rows(FTT, inp, t, bad, np.array([4, 13, 17, 30, 44, 60]),
                                host=FT.table(len(t), 12, inp["contacts"]))


# 9 ----------------------------------------------------------------------------------------------
REFUSALS = {
    "update": "wbc_update: a per-robot force task is in force (default wbc_step only; clear it with wbc_set_force_task(h, NULL))",
    "solve": "wbc_solve: a per-robot force task is in force (default wbc_step only; clear it with wbc_set_force_task(h, NULL))",
    "step_modes": ("wbc_step_modes: a per-robot force task is in force (default wbc_step only; clear it with "
                   "wbc_set_force_task(h, NULL))"),
    "step_split": ("wbc_step: WBC_SPLIT with a per-robot force task in force (default form only; clear it with "
                   "wbc_set_force_task(h, NULL))"),
    "step_fused": ("wbc_step: WBC_FUSED with a per-robot force task in force (default form only; clear it with "
                   "wbc_set_force_task(h, NULL))"),
    "cycle_split": ("wbc_cycle: WBC_SPLIT with a per-robot force task in force (plain cycle only; clear it with "
                    "wbc_set_force_task(h, NULL))"),
    "cycle_fused": ("wbc_cycle: WBC_FUSED with a per-robot force task in force (plain cycle only; clear it with "
                    "wbc_set_force_task(h, NULL))"),
    "cycle_resident": ("wbc_cycle: WBC_RESIDENT with a per-robot force task in force (plain cycle only; clear it with "
                       "wbc_set_force_task(h, NULL))"),
    "step_duals": ("wbc_step: WBC_DUALS with a per-robot force task in force (no duals instance reads the table; clear it "
                   "with wbc_set_force_task(h, NULL))"),
    "step_duals_force": ("wbc_step: WBC_DUALS_FORCE with a per-robot force task in force (no duals instance reads the table; "
                         "clear it with wbc_set_force_task(h, NULL))"),
}
assert REFUSALS == {**T.refusal_texts("a per-robot force task is in force", "a per-robot force task in force",
                                      "clear it with wbc_set_force_task(h, NULL)"),
                    "step_duals": REFUSALS["step_duals"], "step_duals_force": REFUSALS["step_duals_force"]}


def test_host_validation_refusals_cycle_and_clearing():
    B = 4
    inp = inputs("rl_random", B)
    t = FT.table(B, 11, inp["contacts"])
    e = Engine(B)
    load(e, inp)
    e.set_force_task(t)
    # host validation: the message names row and column, the previous table stays
    for b, col, v, nm in ((2, 0, np.nan, "f_ref[0][0]"), (1, 7, INF, "f_ref[2][1]"), (3, 11, -INF, "f_ref[3][2]"),
                          (0, 12, 0.0, "weight"), (2, 12, -1.0, "weight"), (1, 12, np.nan, "weight"), (3, 12, INF, "weight")):
        bad = t.copy()
        bad[b, col] = v
        rc = e.lib.wbc_set_force_task(e.h, bad.ctypes.data_as(C.c_void_p))
        assert rc == ERR_ARG and last_error(e).startswith(f"wbc_set_force_task: row {b}, column {col} ({nm}) = "), last_error(e)
        assert last_error(e).endswith(": need finite f_ref and a finite weight > 0")
        assert np.array_equal(e.force_task(), t)
        with pytest.raises(WbcError, match=rf"row {b}, column {col}"):
            e.set_force_task(bad)
    ok = t.copy()
    ok[:, 13] = np.nan  # the reserved column is ignored on input and 0 from the getter
    e.set_force_task(ok)
    assert np.array_equal(e.force_task(), t)
    assert e.lib.wbc_bind_device_force_task(e.h, 8) == ERR_ARG  # not 16-byte aligned
    assert last_error(e) == "wbc_bind_device_force_task: the table must be 16-byte aligned"
    # the step under every supported flag, and the plain wbc_cycle equal to it
    e.step(STATELESS)
    out = e.outputs()
    assert FT.moved_robots(out["grf"], run(inp)["grf"]) >= B - 1
    assert_identical(T.cycle(e, inp, STATELESS), out, what="cycle")
    for flags in (STATELESS | DEBUG, STATELESS | TIMED, STATELESS | GROUP):
        e.step(flags)
        assert_identical(e.outputs(), out, what=flags)
    e.step(STATELESS | NO_X)
    for k in ("tau", "grf", "status", "iters"):
        assert np.array_equal(e.outputs()[k], out[k]), k
    # refusals, letter for letter
    T.refused_forms(e, inp, REFUSALS, extra={"step_duals": lambda: e.step(STATELESS | DUALS),
                                             "step_duals_force": lambda: e.step(STATELESS | DUALS_FORCE)})
    # the other tables are named first, as before
    e.set_force_bounds(FO.table(B))
    with pytest.raises(WbcError):
        e.update(STATELESS)
    assert last_error(e) == ("wbc_update: per-foot force bounds are in force (default wbc_step only; clear them with "
                             "wbc_set_force_bounds(h, NULL))")
    with pytest.raises(WbcError):
        e.step(STATELESS | DUALS)
    assert last_error(e) == ("wbc_step: WBC_DUALS with per-foot force bounds in force (the 40 multipliers have no entry for a force "
                             "row; clear them with wbc_set_force_bounds(h, NULL))")
    e.set_force_bounds(None)
    e.set_force_task(None)
    e.set_modes([15, 5])
    e.set_force_task(t)
    with pytest.raises(WbcError) as ei:
        e.step_modes(STATELESS)
    assert last_error(e) == REFUSALS["step_modes"] and f"({ERR_STATE})" in str(ei.value)
    # cleared: every refused form runs again and matches an engine that never had the table
    e.set_force_task(None)
    assert np.array_equal(e.force_task(), np.tile(FT.PLAIN, (B, 1)))
    f = Engine(B)
    T.cleared_matches_fresh(e, f, inp, (STATELESS, STATELESS | SPLIT, STATELESS | FUSED, STATELESS | DUALS, STATELESS | DUALS_FORCE, 0),
                            (STATELESS, STATELESS | SPLIT, STATELESS | RESIDENT))
    for eng in (e, f):
        eng.close()


def test_each_unit_is_reached_and_dict_form():
    """B = 5: the stateless step (ft0) and the stateful one (ft1) both pull the forces to a reference set through the
    dict form, which keeps the other entries: under w = 1000 every stance force lies within 2 N of fref, which the
    plain step's are not."""
    B = 5
    inp = inputs("stance_cold", B)
    fref = np.tile([5.0, -5.0, 110.0], 4)
    e = Engine(B)
    e.set_force_task(dict(weight=1000.0))
    assert np.array_equal(e.force_task(), np.tile(force_task_row(0.0, 1000.0), (B, 1)))
    e.set_force_task(dict(f_ref=fref.reshape(4, 3)))
    assert np.array_equal(e.force_task(), np.tile(force_task_row(fref, 1000.0), (B, 1)))
    load(e, inp)
    assert np.abs(run(inp)["grf"] - fref).max() > 10.0
    for flags in (STATELESS, 0):
        e.step(flags)
        out = e.outputs()
        assert np.all(out["status"] == QP_OK)
        assert np.abs(out["grf"] - fref).max() < 2.0, (flags, np.abs(out["grf"] - fref).max())
    e.close()
