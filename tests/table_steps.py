"""What the GPU tests of the per-robot tables share (parameters, contact normals, base body, limits, force
bounds; tests/test_gpu_*.py): the input sets and the parameter-table generator, one `run` that sets any of the
five tables in the engine's order, the two comparisons (bit identity, and the oracle at tests/margins.py's
bounds), the refusal sentences of csrc/wbc_engine.cpp, and the scenarios every table is put through.  Which
shapes, rows and bad entries a test uses stays in the test's own file.

A plain module: it holds no test and no fixture, and importing it needs no GPU."""
import dataclasses

import numpy as np

import margins as M
import pytest

from quadrupedwholebodycontroller_amd import (DUALS, FUSED, QP_NUMERIC, QP_OK, RESIDENT, ROBOT_PARAM_NAMES, SPLIT, STATELESS,
                                              Engine, WbcError, workloads)

KEYS = ("tau", "grf", "x", "status", "iters")
ERR_ARG, ERR_STATE = -1, -3
RANGES = dict(friction=(0.35, 1.5), max_torque=(15, 80), kp=(3000, 9000), kp_z=(5000, 15000), kd=(900, 2700), ki=(0, 50),
              kp_swing=(125, 500), kd_swing=(10, 40), slack_weight=(100, 10000))


# --- inputs and the parameter table -----------------------------------------------------------------
def table(B, seed=7):
    """The [B, 10] parameter table of numpy.random.default_rng(seed), uniform per column over RANGES."""
    g = np.random.default_rng(seed)
    t = np.zeros((B, 10))
    for c, name in enumerate(ROBOT_PARAM_NAMES):
        t[:, c] = g.uniform(*RANGES[name], B)
    return t


def row_dict(row):
    return {n: float(row[c]) for c, n in enumerate(ROBOT_PARAM_NAMES)}


def take(inp, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in inp.items()}


def inputs(name, B):
    if name == "straight":
        return workloads.straight_legs(workloads.stance_cold(B, seed=81))
    return getattr(workloads, name)(B, seed=91)


# --- engine calls -------------------------------------------------------------------------------------
def load(e, inp):
    e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
    e.set_reference(inp["ref"], inp["contacts"], inp["switching"])


def cycle(e, inp, flags):
    return e.cycle(inp["base_pose"], inp["nu"], inp["qj"], inp["ref"], inp["contacts"], inp["switching"], flags)


def last_error(e):
    return e.lib.wbc_last_error().decode()


def run(inp, flags=STATELESS, duals=False, *, params=None, robot_params=None, contact_normals=None, base_body=None, limits=None,
        force_bounds=None):
    """One step of a fresh engine (of `params`, else the defaults) under the given tables, set in this order; the
    outputs, with the 40 multipliers under "dual" when `duals` (the step then carries WBC_DUALS)."""
    e = Engine(len(inp["contacts"]), params=params)
    load(e, inp)
    if robot_params is not None:
        e.set_robot_params(robot_params)
    if contact_normals is not None:
        e.set_contact_normals(contact_normals)
    if base_body is not None:
        e.set_base_body(base_body)
    if limits is not None:
        e.set_limits(limits)
    if force_bounds is not None:
        e.set_force_bounds(force_bounds)
    e.step(flags | (DUALS if duals else 0))
    out = e.outputs()
    if duals:
        out["dual"] = e.duals()
    e.close()
    return out


# --- comparisons --------------------------------------------------------------------------------------
def moved(a, b, by=1e-3):
    """Robots whose tau differs by more than `by` N m."""
    return int((np.abs(a["tau"] - b["tau"]).max(axis=1) > by).sum())


def assert_identical(a, b, idx_a=None, idx_b=None, what=""):
    """The five outputs bit for bit, of a[k][idx_a] against b[k][idx_b] (None: all robots)."""
    for k in KEYS:
        va = a[k] if idx_a is None else a[k][idx_a]
        vb = b[k] if idx_b is None else b[k][idx_b]
        assert np.array_equal(va, vb), (what, k)


def check_against_oracle(out, ref, what):
    """Status as the oracle's on every robot; tau, grf and x within the margins on the robots it solved."""
    assert np.array_equal(out["status"], ref["status"]), (what, out["status"], ref["status"])
    for b in np.nonzero(ref["status"] == QP_OK)[0]:
        assert M.close(out["tau"][b], ref["tau"][b], M.TAU, "tau"), (what, b)
        assert M.close(out["grf"][b], ref["grf"][b], M.GRF, "grf"), (what, b)
        assert M.close(out["x"][b], ref["x"][b], M.X, "x"), (what, b)


def check_against_c_oracles(out, lit, red, what, iters_rows=None):
    """The above against the C oracle's LITERAL method, which must have solved all but four robots at the most;
    iters as its REDUCED method's on `iters_rows` (None: every robot), with no allowance."""
    check_against_oracle(out, lit, what)
    B = len(lit["status"])
    assert (lit["status"] == QP_OK).sum() >= B - 4, (what, lit["status"])
    rows = np.arange(B) if iters_rows is None else iters_rows
    assert np.array_equal(out["iters"][rows], red["iters"][rows]), (what, out["iters"][rows], red["iters"][rows])


# --- refusal sentences --------------------------------------------------------------------------------
def refusal_texts(is_phrase, with_phrase, clear_call):
    """wbc_last_error() of the eight calls that refuse a table in force, from how the engine names the table
    ("contact normals are in force", "contact normals in force") and its way out ("clear them with
    wbc_set_contact_normals(h, NULL)")."""
    is_ = f"{is_phrase} (default wbc_step only; {clear_call})"
    with_ = f" with {with_phrase} ({{}}; {clear_call})"
    return {
        "update": "wbc_update: " + is_,
        "solve": "wbc_solve: " + is_,
        "step_modes": "wbc_step_modes: " + is_,
        "step_split": "wbc_step: WBC_SPLIT" + with_.format("default form only"),
        "step_fused": "wbc_step: WBC_FUSED" + with_.format("default form only"),
        "cycle_split": "wbc_cycle: WBC_SPLIT" + with_.format("plain cycle only"),
        "cycle_fused": "wbc_cycle: WBC_FUSED" + with_.format("plain cycle only"),
        "cycle_resident": "wbc_cycle: WBC_RESIDENT" + with_.format("plain cycle only"),
    }


# --- one table ----------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Table:
    """One of the five tables by its name in the API: Engine.set_<name> / bind_device_<name> / <name>() (which call
    wbc_set_<name> / wbc_bind_device_<name> / wbc_get_<name>), and run()'s keyword."""
    name: str

    def set(self, e, t):
        getattr(e, "set_" + self.name)(t)

    def bind(self, e, t):
        getattr(e, "bind_device_" + self.name)(t)

    def get(self, e):
        return getattr(e, self.name)()

    def run(self, inp, t, flags=STATELESS):
        return run(inp, flags, **{self.name: t})


# --- scenarios ----------------------------------------------------------------------------------------
def own_row_only(desc, inp, t, b, new_row, by=1e-3):
    """A permuted batch gives permuted bits; row b replaced by `new_row` moves robot b's tau by more than `by`
    N m and no other robot by a bit."""
    B = len(inp["contacts"])
    out = desc.run(inp, t)
    perm = np.random.default_rng(4).permutation(B)
    assert_identical(desc.run(take(inp, perm), t[perm]), out, idx_b=perm, what="permuted")
    t2 = t.copy()
    t2[b] = new_row
    out2 = desc.run(inp, t2)
    others = np.arange(B) != b
    assert_identical(out2, out, idx_a=others, idx_b=others, what="other robots")
    assert np.abs(out2["tau"][b] - out["tau"][b]).max() > by


def device_bound_invalid_rows(desc, inp, t, bad, rows_bad, host=None):
    """`bad` (t with the rows `rows_bad` made unacceptable) device-bound, for a stateless step and the first
    stateful one: the table reads back as `bad`; the bad rows' robots get WBC_QP_NUMERIC and zeros, every other
    robot the bits of a run under t.  With a host table `host` set under it: the unbind restores `host`, and the
    next stateless step is a run under `host`."""
    torch = pytest.importorskip("torch")
    B = len(inp["contacts"])
    others = np.setdiff1d(np.arange(B), rows_bad)
    d = torch.from_numpy(np.ascontiguousarray(bad)).cuda()
    torch.cuda.synchronize()
    for flags in (STATELESS, 0):
        ref = desc.run(inp, t, flags)
        e = Engine(B)
        load(e, inp)
        if host is not None:
            desc.set(e, host)
        desc.bind(e, d)
        e.step(flags)
        out = e.outputs()
        assert np.array_equal(desc.get(e), bad, equal_nan=True)
        assert np.all(out["status"][rows_bad] == QP_NUMERIC), out["status"][rows_bad]
        for k in ("tau", "grf", "x"):
            assert not out[k][rows_bad].any(), k
        assert_identical(out, ref, idx_a=others, idx_b=others, what=("others", flags))
        if host is not None:
            desc.bind(e, None)
            assert np.array_equal(desc.get(e), host)
            if flags == STATELESS:
                e.step(flags)
                assert_identical(e.outputs(), desc.run(inp, host, flags), what="unbound: the host table")
        e.close()


def refused_forms(e, inp, want, extra=None):
    """The seven calls that do not read a table (and those of `extra`, name -> call), each refused with
    WBC_ERR_STATE and want[name] as wbc_last_error(), letter for letter."""
    calls = {
        "update": lambda: e.update(STATELESS),
        "solve": lambda: e.solve(STATELESS),
        "step_split": lambda: e.step(STATELESS | SPLIT),
        "step_fused": lambda: e.step(STATELESS | FUSED),
        "cycle_split": lambda: cycle(e, inp, STATELESS | SPLIT),
        "cycle_fused": lambda: cycle(e, inp, STATELESS | FUSED),
        "cycle_resident": lambda: cycle(e, inp, STATELESS | RESIDENT),
        **(extra or {}),
    }
    for name, call in calls.items():
        with pytest.raises(WbcError) as ei:
            call()
        assert last_error(e) == want[name], name
        assert f"({ERR_STATE})" in str(ei.value), name


def cleared_matches_fresh(e, f, inp, step_flags, cycle_flags, modes=(15, 5)):
    """e: an engine whose table was cleared while it held the mode list `modes`; f: one that never had a table.
    wbc_step_modes on the first B / len(modes) states, then without the modes a step under each of
    `step_flags`, update + solve, and a cycle under each of `cycle_flags`: the same bits on both engines."""
    states = take(inp, slice(0, len(inp["contacts"]) // len(modes)))
    f.set_modes(list(modes))
    for eng in (e, f):
        load(eng, states)
        eng.step_modes(STATELESS)
    assert_identical(e.outputs(), f.outputs(), what="cleared, step_modes")
    for eng in (e, f):
        eng.set_modes(None)
    for flags in step_flags:
        for eng in (e, f):
            load(eng, inp)
            eng.step(flags)
        assert_identical(e.outputs(), f.outputs(), what=("cleared", flags))
    for eng in (e, f):
        eng.update(STATELESS)
        eng.solve(STATELESS)
    assert_identical(e.outputs(), f.outputs(), what="cleared, update + solve")
    for flags in cycle_flags:
        assert_identical(cycle(e, inp, flags), cycle(f, inp, flags), what=("cleared cycle", flags))
