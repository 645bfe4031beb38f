"""CPU: the oracle runs of tests/offtrot_tables_oracle.py, before any GPU run.

The GPU cases of tests/test_gpu_offtrot_tables.py are only as good as their inputs and their checker.  Here the
inputs are shown to cover what they claim at B = 4 (every ordered mask change per robot, four masks in one wave),
each oracle run to meet the conditions that keep its case honest (the shares of OK and INFEASIBLE rows, a torque limit
tight on half the OK rows, a force bound tight on a third of them, and a force bound tight on one leg in the cycle
before and in the cycle of a mask change: the thing no trot ever feeds the warm set), the swap and the reset to change
the run, the duals sets to carry force multipliers, and the oracle's own spread under inputs moved by one ulp to
stay below a tenth of every bound the engine is held to.  The seeds are the issue's (limits 7, bounds 300 + k // 3,
task 100 + k, parameters 11, normals 5, payloads 11): none had to be changed."""
import numpy as np

import margins as M
import pytest

import force_duals_oracle as FD
import offtrot_tables_oracle as O
import wbc_np as W

B, T, DWELL = O.B, O.T, O.DWELL
TOLS = {"tau": M.TAU, "x": M.X, "grf": M.STATEFUL_TABLE_GRF}
# case, latched, the run's keywords: the seven oracle runs the GPU cases compare against
RUNS = [("lm", True, {}), ("lm", False, dict(swap=True)), ("fn", True, {}), ("fn", False, {}), ("ft", True, {}), ("ft", False, {}),
        ("all", True, dict(reset=True))]
RUN_IDS = [f"{c}-{'latched' if l else 'unlatched'}" + "".join(f"-{k}" for k in kw) for c, l, kw in RUNS]


def norm_err(a, b):
    """test_gpu_stateful_offtrot.norm_err: max|a - b| / (1 + max|b|) over the last axis."""
    return np.max(np.abs(a - b), axis=-1) / (1.0 + np.max(np.abs(b), axis=-1))


def test_the_sequence_at_four_robots():
    """B = 4 is one wave.  Every robot makes at least 255 distinct ordered mask changes, holds each mask for three
    cycles, and the four robots of a cycle are on three masks or more on average; cycle 300 (the swap, the reset)
    is a mask change for every robot."""
    for latch in (True, False):
        m = O.masks(latch)
        assert m.shape == (T, B) and T * B == 3072
        assert min(O.mask_changes(latch)) >= 255, O.mask_changes(latch)
        assert np.array_equal(m, np.repeat(m[::DWELL], DWELL, axis=0))
        assert np.mean([len(set(r.tolist())) for r in m]) > 3.0
        assert np.all(m[O.SWAP_AT - 1] != m[O.SWAP_AT]) and O.SWAP_AT == O.RESET_AT and O.SWAP_AT % DWELL == 0
        sw = np.array([s["switching"] for s in O.sequence(latch)])
        assert sw.any() == latch
    print("distinct ordered mask changes per robot:", O.mask_changes(True))


@pytest.mark.parametrize("case,latch,kw", RUNS, ids=RUN_IDS)
def test_conditions_that_keep_the_cases_honest(case, latch, kw):
    """offtrot_tables_oracle.honest on every oracle run a GPU case compares against (measured, latched / unlatched:
    3071 / 2148 rows OK under the bounds, 2176 unlatched under the swapped limits alone, the rest INFEASIBLE; a torque
    limit tight on 81-95 % of the OK rows; a force bound tight on 1980 / 1385 (fn) and 1961 / 1364 (ft) rows, and
    carried across a mask change on the same leg on 330 / 14 and 355 / 11 robot-cycles).  x and grf are zero wherever
    the oracle is not OK (its tau there is bbar alone; the GPU cases hold the engine's to zero without reading it)."""
    run = O.oracle(case, latch, **kw)
    counts = O.honest(case, latch, run, kw.get("swap", False))
    print(case, "latched" if latch else "unlatched", kw, counts)
    bad = run["status"] != W.QP_OK
    for q in ("x", "grf"):
        assert run[q].shape[:2] == (T, B) and not run[q][bad].any(), q


def test_the_swap_and_the_reset_change_the_oracle_run():
    """The oracle halves of the swap of case 1 and the reset of case 4: the swapped run equals the unswapped one
    before cycle 300 and differs from it on every robot in the dwell that starts there; the reset changes robots 1 and
    3 at cycle 300, no other robot there and no robot before."""
    O.swap_changes_the_oracle_run()
    O.reset_changes_the_oracle_run()


@pytest.mark.parametrize("latch", [True, False], ids=["latched", "unlatched"])
def test_the_duals_sets_carry_force_multipliers(latch):
    """The 1024 robot-cycles of the mask-change cycles (k % 3 == 0) that the certificates of lmd1 and fnd1 run on:
    OK and INFEASIBLE robots both occur unlatched, and at least a third of fnd1's OK robot-cycles carry a non-zero
    force multiplier on the oracle's own x."""
    for case in O.SNAP_CASES:
        cs = O.snapshots(case, latch)
        ok = [c for c in cs if c.qp_status == W.QP_OK]
        assert len(cs) == T // DWELL * B == 1024 and len(ok) > 0
        assert all(c.qp[2].shape[0] == (O.LM_ROWS if case == "lm" else FD.NROWS) for c in cs[:8])
        if not latch:
            assert len(ok) < len(cs)
        if case == "fn":
            n = sum(FD.has_force_multiplier(c) for c in ok)
            print(f"fn, {'latched' if latch else 'unlatched'}: {n} of {len(ok)} OK robot-cycles with a force multiplier ({len(cs)} certified)")
            assert 3 * n >= len(ok), (n, len(ok))


@pytest.mark.parametrize("case,latch,kw", [r for r in RUNS if r[0] in ("ft", "all")], ids=[i for i, r in zip(RUN_IDS, RUNS) if r[0] in ("ft", "all")])
def test_the_oracles_own_spread(case, latch, kw):
    """Cases 3 and 4 again with every input moved by at most one ulp: no status flips, and tau, x and grf move by at
    most a tenth of the bound the engine is held to, in the GPU cases' measure (measured at B = 8 under limits,
    bounds and task: 4.1e-13, 3.3e-13 and 4.7e-12 against 1e-9, 1e-9 and 7e-10).  The figures go to the margins
    record (profiles/offtrot_tables/oracle_spread.json)."""
    run, moved = O.oracle(case, latch, **kw), O.oracle(case, latch, ulp=0, **kw)
    flips = int(np.sum(run["status"] != moved["status"]))
    ok = run["status"] == W.QP_OK
    tag = f"{case}, {'latched' if latch else 'unlatched'}"
    worst = {q: float(np.where(ok, norm_err(moved[q], run[q]), 0.0).max()) for q in TOLS}
    print(tag, "status flips", flips, "spread", worst)
    assert M.record(f"oracle status flips, {tag}, inputs moved by an ulp", flips, 0) == 0
    for q, bound in TOLS.items():
        assert M.record(f"oracle spread {q}, {tag}, inputs moved by an ulp", worst[q], 0.1 * bound) <= 0.1 * bound, (q, worst[q])
