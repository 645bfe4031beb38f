"""GPU: the stateful step away from the trot -- a base that turns, rolls and pitches, twelve joints
on their own sines and every ordered mask change (tests/stateful_sequences.py), with and without the
switching latch -- against the C oracle, cycle by cycle and robot by robot.

What the trot never feeds the stateful kernels (wbc_update_solve_kernel<1>, its per-robot-parameter
instance and the split update kernel): a rotating base in the compact T_old / Tdot / Tdot_inv / Jbar_old
forms (H_ROLD, H_MAOLD, H_DOLD, H_JBJOLD); a mask change whose derivatives are not zeroed, where the
mask Jbar_old belongs to (H_KOLD) decides kap_new J - kap_old J_old (quirk A.7); working-set rows that
survive a mask change (7 -> 5, 15 -> 13); a first cycle after a reset on a tilted, moving robot; and
infeasible QPs in a stateful run (about a quarter of the unlatched solves).

All runs: B = 8 robots, 768 cycles, one engine per case, one `wbc_ref.Robot` per row.  Each oracle run
and each engine run is made once and shared (read-only) between the cases that need it.  Stateful
intermediates (bbar[6:], W, r1, rsw) are held to margins.STATEFUL_INTERMEDIATE, the others to the
bounds of tests/test_gpu_parity.py; tau / x on the default path to margins.STATEFUL_TAU / _X, elsewhere
to margins.TAU / X; grf to margins.GRF (under the table: see test_table).  Every case asserts how many rows it compared.

test_tables and the two cases after it take the same sequence through the stateful normals instance
(wbc_kernel_cn1.hip) and the stateful base-body instance (wbc_kernel_bb1.hip), alone and with the other
tables in force, against C robots given the same rows (oracle/wbc_ref.c's per-foot normals,
tests/base_body_oracle.py's per-robot model).
"""
import numpy as np

import margins as M
import pytest

import base_body_oracle as BB
import contact_normals_oracle as CN
import stateful_sequences as S
import wbc_ref as R
from quadrupedwholebodycontroller_amd import COLD, DEBUG, QP_INFEASIBLE, QP_OK, SPLIT, Engine, split_debug
from table_steps import row_dict, table

pytestmark = pytest.mark.gpu

B, DWELL, SEED = 8, 3, 5
T = 256 * DWELL
RESET_AT, RESET_ROBOTS = 300, (1, 4, 6)
TILT = 0.35  # rad: the normal tables are contact_normals_oracle.normals(B, seed, TILT)
SWAP_AT, SWAP_TO = 300, (6, 12)  # the swap case: at this cycle (a mask change) the normals go to seed 6, the payloads to seed 12
IN_KEYS = ("base_pose", "nu", "qj", "ref")
STATEFUL_Q = ("bbar", "W", "r1", "rsw")
OTHER_Q = ("com", "comvel", "pose", "vc", "M", "Cnu", "Mbar_b", "Mbar_j", "Jbar")  # what the C oracle's record holds

_ORACLE, _ENGINE = {}, {}


def _freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def tables(tab, nrm, bb):
    """(parameter rows, normals, base-body rows) of the seeds given; None where no table is in force."""
    return (table(B, tab) if tab is not None else None, CN.normals(B, nrm, TILT) if nrm is not None else None,
            BB.payload_rows(B, seed=bb) if bb is not None else None)


def oracle(latch, method, hotstart=True, tab=None, reset=False, nrm=None, bb=None, swap=False, ulp=None):
    """One stateful C-oracle robot per row over the sequence: status, iters [T, B], tau, grf, x and
    (LITERAL) the debug record's quantities [T, B, ...].  tab, nrm, bb: the seeds of a parameter table,
    a normals table and a payload table (robot b under row b of each).  swap: at cycle SWAP_AT the
    normals and the payloads are replaced by those of seeds SWAP_TO, the history untouched.  ulp: a seed;
    every input is then moved by at most one ulp (the oracle's own sensitivity, for the CPU tests)."""
    key = (latch, method, hotstart, tab, reset, nrm, bb, swap, ulp)
    if key in _ORACLE:
        return _ORACLE[key]
    rows, normals, payload = tables(tab, nrm, bb)
    kw = lambda b: row_dict(rows[b]) if rows is not None else {}
    new = lambda b: (R.Robot(hotstart=hotstart, method=method, **kw(b)) if payload is None else
                     BB.CRobot(payload[b], hotstart=hotstart, method=method, **kw(b)))
    robots = [new(b) for b in range(B)]
    dbg = method == R.LITERAL
    g = np.random.default_rng(ulp) if ulp is not None else None
    res = {}
    for k, s in enumerate(S.sequence(B, DWELL, SEED, latch)):
        if reset and k == RESET_AT:
            for b in RESET_ROBOTS:
                robots[b] = new(b)
        if swap and k == SWAP_AT:
            _, normals, payload = tables(None, SWAP_TO[0], SWAP_TO[1])
            for b in range(B):
                robots[b].set_row(payload[b])
        for b in range(B):
            a = [s[q][b] for q in IN_KEYS]
            if g is not None:
                a = [v * (1.0 + 2.0 ** -52 * g.uniform(-1, 1, v.shape)) for v in a]
            o = robots[b].step(*a, int(s["contacts"][b]), int(s["switching"][b]), debug=dbg,
                               normals=None if normals is None else normals[b])
            o.update(o.pop("dbg", {}))
            for q, v in o.items():
                res.setdefault(q, []).append(v)
    out = {q: np.array(v).reshape((T, B) + np.shape(v[0])) for q, v in res.items()}
    _ORACLE[key] = _freeze(out)
    return out


def engine(latch, flags, tab=None, reset=False, nrm=None, bb=None, swap=False):
    """The engine over the sequence; flags: one value, or a tuple rotated per cycle.  The debug
    records are kept when every cycle's flags hold DEBUG.  tab, nrm, bb, swap: as oracle()."""
    key = (latch, flags, tab, reset, nrm, bb, swap)
    if key in _ENGINE:
        return _ENGINE[key]
    fl = flags if isinstance(flags, tuple) else (flags,)
    dbg = all(f & DEBUG for f in fl)
    rows, normals, payload = tables(tab, nrm, bb)
    e = Engine(B)
    if rows is not None:
        e.set_robot_params(rows)
    if normals is not None:
        e.set_contact_normals(normals)
    if payload is not None:
        e.set_base_body(payload)
    res = {}
    for k, s in enumerate(S.sequence(B, DWELL, SEED, latch)):
        if reset and k == RESET_AT:
            e.reset(np.isin(np.arange(B), RESET_ROBOTS).astype(np.uint8))
        if swap and k == SWAP_AT:
            _, normals, payload = tables(None, SWAP_TO[0], SWAP_TO[1])
            e.set_contact_normals(normals)
            e.set_base_body(payload)
        e.set_state(s["base_pose"], s["nu"], s["qj"])
        e.set_reference(s["ref"], s["contacts"], s["switching"])
        e.step(fl[k % len(fl)])
        o = e.outputs()
        if dbg:
            recs = [split_debug(r) for r in e.debug()]
            for q in STATEFUL_Q + OTHER_Q:
                o[q] = np.array([r[q].ravel() for r in recs])
        for q, v in o.items():
            res.setdefault(q, []).append(v)
    e.close()
    out = {q: np.array(v) for q, v in res.items()}
    _ENGINE[key] = _freeze(out)
    return out


def norm_err(a, b):
    """margins.norm_err per row: max|a - b| / (1 + max|b|) over the last axis."""
    return np.max(np.abs(a - b), axis=-1) / (1.0 + np.max(np.abs(b), axis=-1))


def rel_err(a, b):
    """test_gpu_parity's measure per row: max over the last axis of |a - b| / max(1, |b|)."""
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)), axis=-1)


class Report:
    """Collects every miss of a case, so that one run shows all figures; `done` asserts."""

    def __init__(self, what):
        self.what, self.misses = what, []

    def equal(self, name, a, b):
        bad = np.argwhere(a != b)
        M.record(f"{name} mismatch fraction", len(bad) / max(1, a.size), 0.0)
        if len(bad):
            self.misses.append((name, "differs at", len(bad), "first (cycle, robot)", bad[0].tolist()))

    def within(self, name, err, rows, tol):
        """err [T, B], compared on the rows selected by the boolean mask `rows`."""
        sel = np.where(rows, err, 0.0)
        at = np.unravel_index(np.argmax(sel), sel.shape)
        if M.record(name, sel[at], tol) > tol:
            self.misses.append((name, float(sel[at]), "bound", tol, "worst (cycle, robot)", [int(i) for i in at],
                                "rows over the bound", int(np.sum(sel > tol))))

    def done(self):
        assert not self.misses, (self.what, self.misses)


def outputs_vs(rep, out, ref, tols):
    """status equal; tau, x (and grf when bounded) on the oracle's OK rows; zeros where the oracle
    returns zeros.  Returns the OK-row mask."""
    rep.equal("status", out["status"], ref["status"])
    ok = ref["status"] == QP_OK
    for q, tol in tols.items():
        rep.within(q, norm_err(out[q], ref[q]), ok, tol)
        if np.any(out[q][~ok] != 0.0):
            rep.misses.append((q, "not zero on a row the oracle zeroes"))
    return ok


def intermediates_vs(rep, out, lit):
    every = np.ones((T, B), bool)
    for q in STATEFUL_Q:
        a, b = (out[q][..., 6:], lit[q][..., 6:]) if q == "bbar" else (out[q], lit[q])
        rep.within(q, rel_err(a, b), every, M.STATEFUL_INTERMEDIATE[q])
    for q in OTHER_Q:
        rep.within(q, rel_err(out[q], lit[q]), every, M.INTERMEDIATE.get(q, 1e-13))


DEFAULT_TOLS = {"tau": M.STATEFUL_TAU, "x": M.STATEFUL_X, "grf": M.GRF}


def default_case(latch, reset=False):
    what = ("latched" if latch else "unlatched") + "-default" + ("-reset" if reset else "")
    out = engine(latch, DEBUG, reset=reset)
    lit, red = oracle(latch, R.LITERAL, reset=reset), oracle(latch, R.REDUCED, reset=reset)
    rep = Report(what)
    ok = outputs_vs(rep, out, lit, DEFAULT_TOLS)
    intermediates_vs(rep, out, lit)
    rep.equal("iters", out["iters"], red["iters"])
    return rep, ok, lit


def test_latched_default():
    """step(DEBUG), switching latched at every change: every solve of the oracle's is QP_OK."""
    rep, ok, lit = default_case(True)
    assert ok.sum() >= 0.9 * T * B, ok.sum()
    rep.done()


def test_unlatched_default():
    """switching = 0 throughout: the derivatives are differenced across the mask change (H_KOLD) and
    the working set is carried across it; both statuses occur and both are compared."""
    rep, ok, lit = default_case(False)
    n_inf = np.sum(lit["status"] == QP_INFEASIBLE)
    assert ok.sum() >= 0.1 * T * B and n_inf >= 0.1 * T * B, (ok.sum(), n_inf)
    assert ok.sum() + n_inf == T * B
    rep.done()


@pytest.mark.parametrize("latch", [True, False], ids=["latched", "unlatched"])
def test_reset_inside_the_run(latch):
    """reset(mask) on robots 1, 4, 6 at cycle 300 (fresh oracle robots for them): their next cycle is
    a first cycle (T_old = I, J_old = 0, Tdot_inv = 0, e_int = 0, no working set) on a tilted, moving
    robot, whatever the others carry on.  Cycle 300 is a mask change: latched, it zeroes the
    derivatives of that cycle; unlatched, r1 / rsw hold J / dt there."""
    rep, ok, lit = default_case(latch, reset=True)
    assert ok.sum() >= (0.9 if latch else 0.1) * T * B, ok.sum()
    plain = oracle(latch, R.LITERAL)
    for b in range(B):  # the oracle run did change, for those robots alone
        changed = any(np.any(lit[q][RESET_AT, b] != plain[q][RESET_AT, b]) for q in STATEFUL_Q)
        assert changed == (b in RESET_ROBOTS), b
    rep.done()


def test_latched_cold():
    """COLD: the history is carried, every QP starts cold; against hotstart=False robots, and the
    hot engine run of latched-default at the few-ulp bound."""
    out, hot = engine(True, COLD), engine(True, DEBUG)
    lit, red = oracle(True, R.LITERAL, hotstart=False), oracle(True, R.REDUCED, hotstart=False)
    rep = Report("latched-cold")
    ok = outputs_vs(rep, out, lit, DEFAULT_TOLS)
    rep.equal("iters", out["iters"], red["iters"])
    rep.equal("status hot vs cold", hot["status"], out["status"])
    for q in ("tau", "x"):
        rep.within(f"{q} hot vs cold", norm_err(hot[q], out[q]), ok, M.BITS)
    assert ok.sum() >= 0.9 * T * B, ok.sum()
    assert out["iters"].sum() > 2 * hot["iters"].sum()  # the two runs did differ in how they started
    rep.done()


def test_latched_split():
    """SPLIT: the update kernel and the general solve kernels, iterations in the general form's
    convention (the LITERAL oracle's)."""
    out, lit = engine(True, SPLIT), oracle(True, R.LITERAL)
    rep = Report("latched-split")
    ok = outputs_vs(rep, out, lit, {"tau": M.TAU, "x": M.X})
    rep.equal("iters", out["iters"], lit["iters"])
    assert ok.sum() >= 0.9 * T * B, ok.sum()
    rep.done()


def test_mixed_forms():
    """One engine, flags 0, COLD, SPLIT, 0, ... per cycle: the history is shared between the forms
    (the working-set tag differs per form, so no iteration check)."""
    out, lit = engine(True, (0, COLD, SPLIT)), oracle(True, R.LITERAL)
    rep = Report("mixed-forms")
    ok = outputs_vs(rep, out, lit, {"tau": M.TAU, "x": M.X})
    assert ok.sum() >= 0.9 * T * B, ok.sum()
    rep.done()


@pytest.mark.parametrize("latch", [True, False], ids=["latched", "unlatched"])
def test_table(latch):
    """The per-robot-parameter stateful instance (wbc_kernel_rp1.hip) off the trot, under
    table_steps.table(8, 11), robot b against Robot(**row_dict(row b)): status, tau, x and grf
    against LITERAL, iters against REDUCED.  grf is held to margins.STATEFUL_TABLE_GRF, not margins.GRF:
    under this table the run has QPs (robot 0, cycle 355: one stance leg carrying 0.14 N on the edge of
    its friction cone beside joint accelerations of 300) where one ulp on the inputs moves the oracle's
    own grf by 1.2e-11 of its norm, and rows where the literal solve's noise in forces near zero is
    6.7e-11 (tests/test_stateful_sequences_cpu.py measures both); the engine's worst, 6.7e-11 against
    LITERAL and 2.8e-11 against REDUCED, is that."""
    out = engine(latch, 0, tab=11)
    lit, red = oracle(latch, R.LITERAL, tab=11), oracle(latch, R.REDUCED, tab=11)
    rep = Report("table")
    ok = outputs_vs(rep, out, lit, {"tau": M.TAU, "x": M.X, "grf": M.STATEFUL_TABLE_GRF})
    rep.equal("iters", out["iters"], red["iters"])
    n_inf = np.sum(lit["status"] == QP_INFEASIBLE)
    if latch:
        assert ok.sum() >= 0.9 * T * B, ok.sum()
    else:
        assert ok.sum() >= 0.1 * T * B and n_inf >= 0.1 * T * B, (ok.sum(), n_inf)
    rep.done()


# The normals (wbc_kernel_cn1.hip) and base-body (wbc_kernel_bb1.hip) stateful instances ---------------
# name -> the seeds of the tables in force; tests/test_stateful_sequences_cpu.py shows on the oracle alone
# that each meets the feasibility shares below and that each table moves the torques.
COMBOS = {"normals": dict(nrm=5), "params_normals": dict(tab=11, nrm=5), "payload": dict(bb=11),
          "all_three": dict(tab=11, nrm=5, bb=11)}
TABLE_TOLS = {"tau": M.TAU, "x": M.X, "grf": M.STATEFUL_TABLE_GRF}


def table_case(what, latch, **kw):
    """step(DEBUG) under the tables of `kw` against one C robot per row under row b of each: status on
    every row, tau / x / grf on the oracle's OK rows and zeros elsewhere, the whole debug record against
    LITERAL, iters against REDUCED with no allowance.  Returns (report, OK mask, LITERAL run, engine run)."""
    out = engine(latch, DEBUG, **kw)
    lit, red = oracle(latch, R.LITERAL, **kw), oracle(latch, R.REDUCED, **kw)
    rep = Report(what)
    ok = outputs_vs(rep, out, lit, TABLE_TOLS)
    intermediates_vs(rep, out, lit)
    rep.equal("iters", out["iters"], red["iters"])
    n_inf = int(np.sum(lit["status"] == QP_INFEASIBLE))
    print(f"{what}: status compared on {out['status'].size} rows, values on {int(ok.sum())} OK rows, {n_inf} INFEASIBLE")
    assert out["status"].shape == lit["status"].shape == (T, B) and T * B == 6144
    if latch:
        assert ok.sum() >= 0.9 * T * B, ok.sum()
    else:
        assert ok.sum() >= 0.1 * T * B and n_inf >= 0.1 * T * B and ok.sum() + n_inf == T * B, (ok.sum(), n_inf)
    return rep, ok, lit, out


@pytest.mark.parametrize("latch", [True, False], ids=["latched", "unlatched"])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_tables(combo, latch):
    """The cn1 instance (normals(8, 5, 0.35), alone and with table(8, 11)) and the bb1 instance
    (payload_rows(8), alone and with both other tables) off the trot: a hot-started working set carries
    friction rows 4 l + rr across a mask change onto a pyramid on another frame, and the base-body row
    enters the mass sum, the centroidal inertia, the bias forces and W's gravity term, hence bbar, r1 and
    rsw through the finite differences of a turning base, in waves whose four robots are on four masks.
    Bounds: margins.TAU / X, STATEFUL_TABLE_GRF, STATEFUL_INTERMEDIATE / INTERMEDIATE; the oracles' own
    spread under the same tables is tests/test_stateful_sequences_cpu.py's."""
    rep, _, _, _ = table_case(f"{combo}, {'latched' if latch else 'unlatched'}", latch, **COMBOS[combo])
    rep.done()


def test_tables_swapped_at_an_unlatched_mask_change():
    """"all three", unlatched; at cycle 300, a mask change, the normals are replaced by seed 6 and the
    payloads by seed 12 in the engine and in the oracle robots alike, the history untouched: r1 and rsw of
    that cycle difference the new model's Jacobians against the old model's, and must be the oracle's
    (the whole run is compared, cycle 300 once more on its own).  The oracle's cycle-300 record does differ
    from the unswapped run's."""
    kw = COMBOS["all_three"]
    rep, ok, lit, out = table_case("all three, swapped, unlatched", False, swap=True, **kw)
    plain = oracle(False, R.LITERAL, **kw)
    assert all(np.array_equal(lit[q][:SWAP_AT], plain[q][:SWAP_AT]) for q in STATEFUL_Q + ("tau",))
    for b in range(B):
        assert any(np.any(lit[q][SWAP_AT, b] != plain[q][SWAP_AT, b]) for q in STATEFUL_Q), b
    assert np.any(np.abs(lit["rsw"][SWAP_AT] - plain["rsw"][SWAP_AT]) > 1e-3) or \
        np.any(np.abs(lit["r1"][SWAP_AT] - plain["r1"][SWAP_AT]) > 1e-3)
    for q in ("r1", "rsw"):
        err = rel_err(out[q][SWAP_AT], lit[q][SWAP_AT])
        assert M.record(f"{q} at the swap", err.max(), M.STATEFUL_INTERMEDIATE[q]) <= M.STATEFUL_INTERMEDIATE[q], (q, err)
    rep.done()


def test_reset_under_tables():
    """reset of robots 1, 4 and 6 at cycle 300 with "all three" in force, latched: test_reset_inside_the_run's
    assertions under the tables (the tables stay in force across the reset; fresh oracle robots under the
    same rows)."""
    kw = COMBOS["all_three"]
    rep, ok, lit, _ = table_case("all three, reset, latched", True, reset=True, **kw)
    plain = oracle(True, R.LITERAL, **kw)
    for b in range(B):  # the oracle run did change, for those robots alone
        changed = any(np.any(lit[q][RESET_AT, b] != plain[q][RESET_AT, b]) for q in STATEFUL_Q)
        assert changed == (b in RESET_ROBOTS), b
    rep.done()
