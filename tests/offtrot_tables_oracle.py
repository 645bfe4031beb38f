"""The oracle runs of the limits, force-bound and force-task stateful steps off the trot (the checker of
tests/test_gpu_offtrot_tables.py, shown to be fit for it by tests/test_offtrot_tables_cpu.py).

tests/stateful_sequences.py at B = 4 (one full wave, each robot on its own mask and offset), DWELL = 3, SEED = 5:
768 cycles, every ordered mask change per robot, latched and unlatched, on one stateful
tests/force_task_oracle.ForceTaskWBC per robot, whose class chain carries limits, bounds, task, normals,
parameters and base body.  The tables, all seeded:
    limits        limits_oracle.table(4, 7), fixed (swapped to seed 8 at cycle SWAP_AT in the swap run);
    force bounds  force_bounds_oracle.table(4, 300 + k // 3): a fresh table per dwell, so rows appear, vanish and
                  change sides at the mask changes and stay put inside a dwell;
    force task    force_task_oracle.table(4, 100 + k, contacts of cycle k) under WEIGHTS, fresh every cycle.
CASES names which of them a run is under: "lm", "fn" (limits and bounds), "ft" (limits, bounds and task) and
"all" (those three with table(4, 11) parameters, normals(4, 5, 0.35) and payload_rows(4)).

Each run is made once and shared read-only.  The numpy oracle solves every QP from the empty working set, so the
same run checks the hot-started engine and the one under WBC_COLD.

A plain module: it holds no test and no fixture, and importing it needs no GPU."""
import numpy as np

import base_body_oracle as BB
import contact_normals_oracle as CN
import force_bounds_oracle as FO
import force_task_oracle as FT
import limits_oracle as LO
import stateful_sequences as S
import wbc_np as W
from table_steps import row_dict, table

B, DWELL, SEED = 4, 3, 5
T = 256 * DWELL
NL = 4
LM_SEED, FN_SEED0, FT_SEED0 = 7, 300, 100
SWAP_AT, SWAP_TO = 300, 8  # the swap run: at this cycle (a mask change) the limits go to seed 8
RESET_AT, RESET_ROBOTS = 300, (1, 3)
TAB_SEED, NRM_SEED, TILT, BB_SEED = 11, 5, 0.35, 11
WEIGHTS = 10.0 ** np.linspace(-1.0, 2.0, B)
IN_KEYS = ("base_pose", "nu", "qj", "ref")
CASES = {"lm": dict(fn=False, ft=False, six=False), "fn": dict(fn=True, ft=False, six=False),
         "ft": dict(fn=True, ft=True, six=False), "all": dict(fn=True, ft=True, six=True)}
SNAP_CASES = ("lm", "fn")  # the runs that keep the QP of every mask-change cycle (the duals certificates)
LM_ROWS = 70  # the literal QP's rows without the four force rows
TIGHT = 1e-7

_ORACLE = {}


def sequence(latch):
    return S.sequence(B, DWELL, SEED, latch)


def masks(latch=True):
    """[T, B] contact masks of the sequence."""
    return np.array([s["contacts"] for s in sequence(latch)])


def stance(latch=True):
    """[T, B, 4] booleans: foot l of robot b in stance at cycle k."""
    return ((masks(latch).astype(int)[:, :, None] >> np.arange(NL)) & 1) == 1


def change_cycles():
    """The cycles on which a dwell starts (k % DWELL == 0): the first is the entry from mask 15."""
    return np.arange(0, T, DWELL)


def limits_table(k=0, swap=False):
    return LO.table(B, SWAP_TO if swap and k >= SWAP_AT else LM_SEED)


def bounds_table(k):
    return FO.table(B, FN_SEED0 + k // DWELL)


def task_table(k, contacts):
    t = FT.table(B, FT_SEED0 + k, contacts)
    t[:, FT.FT_WEIGHT] = WEIGHTS
    return t


def six_tables():
    """(parameter rows, normals, base-body rows) of the "all" case."""
    return table(B, TAB_SEED), CN.normals(B, NRM_SEED, TILT), BB.payload_rows(B, seed=BB_SEED)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def oracle(case, latch, swap=False, reset=False, ulp=None, steps=T):
    """One stateful ForceTaskWBC per robot over the sequence (its first `steps` cycles) under the tables of `case`:
    status, iters [steps, B], tau, grf, x [steps, B, ...], and for the cases of SNAP_CASES "snap": {(k, b):
    force_duals_oracle.Snapshot} on the mask-change cycles (the "lm" case's QP cut to its 70 rows: the four force
    rows it drops are unbounded).
    swap: the limits go to seed SWAP_TO at cycle SWAP_AT, the history untouched.  reset: robots RESET_ROBOTS are
    replaced by fresh ones under the same rows before cycle RESET_AT.  ulp: a seed; every input is then moved by
    at most one ulp (the oracle's own sensitivity)."""
    key = (case, latch, swap, reset, ulp, steps)
    if key in _ORACLE:
        return _ORACLE[key]
    from force_duals_oracle import Snapshot  # (imports this module's siblings; kept out of the import cycle)

    what = CASES[case]
    rows, normals, payload = six_tables() if what["six"] else (None, None, None)
    new = lambda b: FT.ForceTaskWBC(BB.np_model(payload[b]) if payload is not None else BB.MODEL,
                                    row_dict(rows[b]) if rows is not None else None,
                                    normals[b] if normals is not None else None)
    robots = [new(b) for b in range(B)]
    g = np.random.default_rng(ulp) if ulp is not None else None
    snap = {} if case in SNAP_CASES and ulp is None else None
    res = {q: [] for q in ("tau", "grf", "x", "status", "iters")}
    for k, s in enumerate(sequence(latch)[:steps]):
        if reset and k == RESET_AT:
            for b in RESET_ROBOTS:
                robots[b] = new(b)
        lm = limits_table(k, swap)
        fn = bounds_table(k) if what["fn"] else None
        ft = task_table(k, s["contacts"]) if what["ft"] else None
        for b, c in enumerate(robots):
            c.limits = lm[b].copy()
            if fn is not None:
                c.bounds = fn[b].copy()
            if ft is not None:
                c.task = ft[b].copy()
            a = [s[q][b] for q in IN_KEYS]
            if g is not None:
                a = [v * (1.0 + 2.0 ** -52 * g.uniform(-1, 1, v.shape)) for v in a]
            c.set_state(a[0], a[1], a[2])
            c.set_reference(a[3], [(int(s["contacts"][b]) >> i) & 1 for i in range(NL)], bool(s["switching"][b]))
            tau, grf, x, st, it = c.step()
            for q, v in zip(("tau", "grf", "x", "status", "iters"), (tau, grf, x, st, it)):
                res[q].append(np.array(v))
            if snap is not None and k % DWELL == 0:
                sn = Snapshot(c)
                if case == "lm":
                    H, gq, A, lb, ub = sn.qp
                    assert np.all(lb[LM_ROWS:] <= -W.INFTY) and np.all(ub[LM_ROWS:] >= W.INFTY)
                    sn.qp = (H, gq, A[:LM_ROWS], lb[:LM_ROWS], ub[:LM_ROWS])
                snap[(k, b)] = sn
    out = {q: np.array(v).reshape((steps, B) + np.shape(v[0])) for q, v in res.items()}
    _freeze(out)
    if snap is not None:
        out["snap"] = snap
    _ORACLE[key] = out
    return out


def snapshots(case, latch):
    """The Snapshots of a duals run, flat: case "lm" unlatched is the swap run, as the GPU case's."""
    return list(oracle(case, latch, swap=(case == "lm" and not latch))["snap"].values())


# --- what keeps the cases honest: counts on an oracle run ------------------------------------------------
def mask_changes(latch=True):
    """Per robot the number of distinct ordered mask changes (previous mask, mask) over the dwell starts, the
    previous mask of cycle 0 being 15."""
    m = masks(latch)[::DWELL]
    prev = np.vstack([np.full((1, B), 15, m.dtype), m[:-1]])
    return [len(set(zip(prev[:, b].tolist(), m[:, b].tolist()))) for b in range(B)]


def tight_force(run, latch, six=False):
    """[T, B, 4] booleans: stance foot l's normal force sits at one of its finite bounds (|n . f - bound| < TIGHT)
    on an OK row."""
    st = stance(latch)
    normals = six_tables()[1] if six else None
    out = np.zeros((T, B, NL), bool)
    for k in range(T):
        t = bounds_table(k)
        nf = FO.normal_forces(run["grf"][k], normals)
        with np.errstate(invalid="ignore"):
            at = (np.abs(nf - t[:, FO.FN_MIN:FO.FN_MAX]) < TIGHT) | (np.abs(nf - t[:, FO.FN_MAX:]) < TIGHT)
        out[k] = at & st[k] & (run["status"][k] == W.QP_OK)[:, None]
    return out


def tight_across_a_change(tf, latch):
    """How many robot-cycles of a mask change have a force bound tight on one leg in the cycle before and in the
    cycle of the change (tf: tight_force's result)."""
    m = masks(latch)
    changed = np.zeros((T, B), bool)
    changed[1:] = m[1:] != m[:-1]
    both = np.zeros((T, B), bool)
    both[1:] = np.any(tf[1:] & tf[:-1], axis=2)
    return int(np.sum(both & changed))


def tight_torque(run, swap=False):
    """[T, B] booleans: a torque of an OK row sits at one of its limits."""
    out = np.zeros((T, B), bool)
    for k in range(T):
        lm = limits_table(k, swap)
        tau = run["tau"][k]
        at = (np.abs(tau - lm[:, LO.TAU_MIN:LO.TAU_MAX]) < TIGHT) | (np.abs(tau - lm[:, LO.TAU_MAX:LO.FRICTION]) < TIGHT)
        out[k] = np.any(at, axis=1) & (run["status"][k] == W.QP_OK)
    return out


def shares(run, latch):
    """(OK rows, INFEASIBLE rows), after asserting the share the issue of these cases sets: latched at least 0.9 T B
    OK; unlatched at least 0.5 T B OK, at least 0.2 T B INFEASIBLE and no third status."""
    n_ok, n_inf = int(np.sum(run["status"] == W.QP_OK)), int(np.sum(run["status"] == W.QP_INFEASIBLE))
    assert run["status"].shape == (T, B) and T * B == 3072
    if latch:
        assert n_ok >= 0.9 * T * B, (n_ok, n_inf)
    else:
        assert n_ok >= 0.5 * T * B and n_inf >= 0.2 * T * B and n_ok + n_inf == T * B, (n_ok, n_inf)
    return n_ok, n_inf


def honest(case, latch, run, swap=False):
    """The conditions of a case on its oracle run, asserted; the counts, for the record: OK and INFEASIBLE rows, rows
    with a tight torque limit, and (under force bounds) rows with a tight force bound and the robot-cycles of a
    mask change that carry one over on the same leg."""
    n_ok, n_inf = shares(run, latch)
    assert min(mask_changes(latch)) >= 255, mask_changes(latch)
    n_tq = int(tight_torque(run, swap).sum())
    assert n_tq >= 0.5 * n_ok, (case, latch, n_tq, n_ok)
    counts = dict(ok=n_ok, infeasible=n_inf, tight_torque=n_tq)
    if CASES[case]["fn"]:
        tf = tight_force(run, latch, CASES[case]["six"])
        n_tf, n_across = int(np.any(tf, axis=2).sum()), tight_across_a_change(tf, latch)
        counts.update(tight_force=n_tf, tight_across_a_change=n_across)
        if case in ("fn", "ft"):
            assert 3 * n_tf >= n_ok, (case, latch, n_tf, n_ok)
            assert n_across >= (100 if latch else 5), (case, latch, n_across)
    return counts


def swap_changes_the_oracle_run():
    """Cycle SWAP_AT is a mask change for every robot; the swapped oracle run is the unswapped one before it and
    differs from it on every robot in the dwell that starts there (the unswapped run is made to that dwell's end)."""
    seq = sequence(False)
    assert np.all(seq[SWAP_AT - 1]["contacts"] != seq[SWAP_AT]["contacts"])
    plain, swapped = oracle("lm", False, steps=SWAP_AT + DWELL), oracle("lm", False, swap=True)
    dwell = slice(SWAP_AT, SWAP_AT + DWELL)
    for q in ("tau", "x", "status"):
        assert np.array_equal(plain[q][:SWAP_AT], swapped[q][:SWAP_AT]), q
    for b in range(B):
        assert any(np.any(plain[q][dwell, b] != swapped[q][dwell, b]) for q in ("tau", "x", "status")), b


def reset_changes_the_oracle_run():
    """The reset changes the oracle run at cycle RESET_AT for robots RESET_ROBOTS and for no other robot (the run
    without it is made to that cycle's dwell's end), and it is the same run before that cycle."""
    plain, reset = oracle("all", True, steps=RESET_AT + DWELL), oracle("all", True, reset=True)
    for q in ("tau", "x", "status"):
        assert np.array_equal(plain[q][:RESET_AT], reset[q][:RESET_AT]), q
    for b in range(B):
        changed = any(np.any(plain[q][RESET_AT, b] != reset[q][RESET_AT, b]) for q in ("tau", "x", "status"))
        assert changed == (b in RESET_ROBOTS), b
