"""GPU: the stateful force-task duals instance (wbc_kernel_ftd1.hip, wbc_step with WBC_DUALS_TASK) away
from the trot, on tests/test_gpu_offtrot_tables.py's harness: tests/stateful_sequences.py at B = 4, 768 cycles, every
ordered mask change, latched and unlatched, under the "ft" tables (limits, a fresh force-bound table per dwell, a fresh
task every cycle) and the "all" tables (those with parameters, normals and base bodies), hot-started and under
WBC_COLD.  On every cycle the five outputs are the bits of the ft1 run without the flag; on every mask-change cycle the
engine's x and its 48 multipliers close tests/force_duals_oracle.py's certificate on the stateful oracle's QP of that
cycle and robot (tests/force_task_duals_oracle.offtrot_snapshots), within ENGINE_MARGIN times the oracle's own residual
on the set (profiles/force_task_duals/oracle_residuals.json)."""
import numpy as np

import margins as M
import pytest

import force_duals_oracle as FD
import force_task_duals_oracle as FTD
import offtrot_tables_oracle as O
from quadrupedwholebodycontroller_amd import COLD, DUALS_FORCE, DUALS_TASK, QP_OK
from table_steps import assert_identical
from test_gpu_offtrot_tables import engine, tag

pytestmark = pytest.mark.gpu

B, T, DWELL = O.B, O.T, O.DWELL
# the harness reads the 48 entries back when the flags carry the WBC_DUALS_FORCE bit, which the engine ignores beside
# WBC_DUALS_TASK
FLAG = DUALS_TASK | DUALS_FORCE
RUNS = [("ft", True, 0), ("ft", False, 0), ("all", True, 0), ("all", False, 0), ("ft", True, COLD), ("all", True, COLD)]
IDS = [f"{c}-{tag(l)}{'-cold' if f else ''}" for c, l, f in RUNS]


@pytest.mark.parametrize("case,latch,flags", RUNS, ids=IDS)
def test_ftd1_moves_nothing_else_and_certifies(case, latch, flags):
    flagged, bare = engine(case, latch, flags | FLAG), engine(case, latch, flags)
    assert flagged["status"].shape == (T, B) and T * B == 3072
    assert_identical(flagged, bare, what=(case, tag(latch), flags))
    assert flagged["dual"].shape == (T, B, 48) and np.isfinite(flagged["dual"]).all() and flagged["dual"].any()
    name = f"offtrot_{case}_{tag(latch)}"
    snap = FTD.offtrot_snapshots(case, latch)
    bound, pbound = FTD.gpu_bound(name), FTD.gpu_bound(name, "primal")
    worst = dict(stat=0.0, viol=0.0, comp=0.0, sign=0.0)
    n = n_ok = n_force = n_want = 0
    for k in O.change_cycles():
        contacts = O.sequence(latch)[k]["contacts"]
        for b in range(B):
            c, d, x = snap[(int(k), b)], flagged["dual"][k, b], flagged["x"][k, b]
            n += 1
            assert flagged["status"][k, b] == c.qp_status, (k, b, flagged["status"][k, b], c.qp_status)
            if c.qp_status != QP_OK:
                assert not d.any(), (k, b, "a robot that is not OK has all-zero multipliers")
                continue
            n_ok += 1
            assert np.count_nonzero(d) <= 12, (k, b)
            for leg in range(4):
                if not (int(contacts[b]) >> leg) & 1:
                    assert not d[4 * leg:4 * leg + 4].any() and not d[40 + 2 * leg:42 + 2 * leg].any(), (k, b, leg)
            viol, stat, sign, comp = FD.certificate48(c, x, d)
            worst["stat"], worst["viol"], worst["comp"] = max(worst["stat"], stat), max(worst["viol"], viol), max(worst["comp"], comp)
            worst["sign"] = max(worst["sign"], -sign / (1.0 + d.max()))
            n_want += FD.has_force_multiplier(c)
            n_force += bool(d[40:].any())
    print(f"{name} flags {flags}: {n} robot-cycles certified, {n_ok} OK; {n_force} with a force multiplier (oracle {n_want}); "
          f"worst {worst}; bounds {bound:.2e} / {pbound:.2e}")
    M.record(f"stationarity {name}", worst["stat"], bound)
    M.record(f"primal {name}", worst["viol"], pbound)
    M.record(f"sign {name}", worst["sign"], bound)
    M.record(f"complementarity {name}", worst["comp"], 1e-7)
    assert n == T // DWELL * B == 1024 and n_ok == sum(c.qp_status == QP_OK for c in snap.values()) > 0, (n, n_ok)
    assert worst["stat"] <= bound, (worst, bound)
    assert worst["viol"] <= pbound, (worst, pbound)
    assert worst["sign"] <= bound, worst
    assert worst["comp"] <= 1e-7, worst
    assert n_force > 0 and n_want > 0, (n_force, n_want)
