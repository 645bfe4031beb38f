"""The checker of the default step's QP multipliers (wbc_step with WBC_DUALS, include/wbc.h):
a per-robot optimality certificate on the reference's literal 42 x 70 QP that needs no second solver.

H is positive definite, so x is the optimum of  min 1/2 x'Hx + g'x  s.t.  lb <= Ax <= ub  if and only if it is
primal feasible and multipliers y exist with H x + g = A' y, y <= 0 only on rows tight at ub, y >= 0 only on
rows tight at lb, y = 0 on slack rows (qpOASES' convention).  The engine returns 40 of them, lambda >= 0 per
friction face and torque side; the others follow from x (`expand`), the 18 equality multipliers by a
least-squares fit, whose residual is the stationarity residual `certificate` reports.

Rows of A (wbc_np.ReferenceWBC.assemble_qp): 0-5 base dynamics, 6-17 R1, 18-33 friction faces (ub = 0),
34-45 torque rows (two-sided), 46-57 R4 (ub = rsw), 58-69 R5 (lb = rsw).

Also the input sets the CPU and the GPU tests share, each robot's stepped numpy controller computed once, and
the committed record of the oracle's own residuals (profiles/duals/oracle_residuals.json), from which the GPU
test's bound is set:  python tests/duals_oracle.py  measures them again and rewrites the record."""
import json
import os
import sys

import numpy as np

if __name__ == "__main__":  # run as a script: the paths tests/conftest.py sets for the tests
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import base_body_oracle as BB
import contact_normals_oracle as CN
import wbc_np as W
from quadrupedwholebodycontroller_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "duals", "oracle_residuals.json")
NEQ, NFR, NTQ, NSW = 18, 16, 12, 12
FR0, TQ0, R40, R50 = NEQ, NEQ + NFR, NEQ + NFR + NTQ, NEQ + NFR + NTQ + NSW
DUAL_LEN = 40
# the widest margin tests/margins.py grants the engine over an oracle ("times 6-53")
ENGINE_MARGIN = 53.0


def expand(c, x, dual40):
    """y (70) in qpOASES' convention for controller c (c.qp = (H, g, A, lb, ub) after step()): rows 18-33
    -lambda_friction, rows 34-45 lambda_side0 - lambda_side1, rows 46-69 from x (of each R4 / R5 pair the
    tighter row carries -+ slack_weight * s_i, the other 0), rows 0-17 zero (fitted by `certificate`)."""
    H, g, A, lb, ub = c.qp
    d = np.asarray(dual40, float)
    y = np.zeros(A.shape[0])
    y[FR0:TQ0] = -d[:NFR]
    y[TQ0:R40] = d[NFR::2] - d[NFR + 1::2]
    Ax = A @ x
    r4, r5 = (Ax - ub)[R40:R50], (Ax - lb)[R50:]
    ws = c.params["slack_weight"] * x[30:42]
    four = np.abs(r4) <= np.abs(r5)
    y[R40:R50] = np.where(four, -ws, 0.0)
    y[R50:] = np.where(four, 0.0, ws)
    return y


def certificate(c, x, dual40):
    """(primal violation as wbc_np.kkt_residuals computes it; stationarity: max |H x + g - A' y| after the
    least-squares fit of the equality multipliers, over 1 + max |H x + g|; signs: the smallest of the 40
    entries; complementarity: over the rows with a non-zero entry, the largest |A_i x - bound_i| / (1 + |A_i x|))."""
    H, g, A, lb, ub = c.qp
    x, d = np.asarray(x, float), np.asarray(dual40, float)
    Ax = A @ x
    lo = np.where(lb <= -W.INFTY, -np.inf, lb)
    hi = np.where(ub >= W.INFTY, np.inf, ub)
    viol = float(np.maximum(np.maximum(lo - Ax, Ax - hi), 0.0).max(initial=0.0))
    y = expand(c, x, d)
    grad = H @ x + g
    res = grad - A[NEQ:].T @ y[NEQ:]
    E = A[:NEQ][np.any(A[:NEQ] != 0.0, axis=1)]
    if E.shape[0]:
        fit, *_ = np.linalg.lstsq(E.T, res, rcond=None)
        res = res - E.T @ fit
    stat = float(np.abs(res).max() / (1.0 + np.abs(grad).max()))
    comp = 0.0
    for r in np.nonzero(d)[0]:
        i = FR0 + r if r < NFR else TQ0 + (r - NFR) // 2
        bound = ub[i] if (r < NFR or (r - NFR) % 2 == 1) else lb[i]
        comp = max(comp, abs(Ax[i] - bound) / (1.0 + abs(Ax[i])))
    return viol, stat, float(d.min()), float(comp)


def lsq_duals(c, x):
    """The 40 entries from the oracle's own x: least-squares multipliers on the tight rows, found with the
    1e-7 (1 + |Ax|) activity test of wbc_np.kkt_residuals (grad + A_act' lam = 0, so y = -lam)."""
    H, g, A, lb, ub = c.qp
    _, _, act, lam = W.kkt_residuals(H, g, A, lb, ub, x)
    y = np.zeros(A.shape[0])
    y[act] = -lam
    Ax = A @ x
    d = np.zeros(DUAL_LEN)
    d[:NFR] = -y[FR0:TQ0]
    at_lb = np.abs(Ax - lb)[TQ0:R40] <= np.abs(Ax - ub)[TQ0:R40]
    d[NFR::2] = np.where(at_lb, y[TQ0:R40], 0.0)
    d[NFR + 1::2] = np.where(at_lb, 0.0, -y[TQ0:R40])
    return d


# ---------------------------------------------------------------------------------------------------------
# input sets
# ---------------------------------------------------------------------------------------------------------
def stress_inputs(B, seed):
    from test_gpu_stress import stress_inputs as f  # (the module is GPU-marked; the generator is plain numpy)
    return f(B, seed)


def tables16():
    """The construction of tests/test_gpu_base_body.py::test_all_three_tables_at_once at B = 16 with per-robot
    friction 0.4 + 0.05 b and max_torque 30 + 3 b: (inputs, parameter columns, normals, base-body rows)."""
    B = 16
    b = np.arange(B)
    return (workloads.rl_random(B, seed=91), dict(friction=0.4 + 0.05 * b, max_torque=30.0 + 3.0 * b),
            CN.normals(B, 5, 0.35), BB.payload_rows(B))


# name -> (inputs, engine-wide parameter overrides); the cold sets on flat ground with the model's own base
COLD_SETS = {
    "stress51_80Nm": (lambda: stress_inputs(48, 51), dict(max_torque=80.0)),
    "stress52_20Nm": (lambda: stress_inputs(48, 52), dict(max_torque=20.0)),
    "stress53_6Nm": (lambda: stress_inputs(48, 53), dict(max_torque=6.0)),
    "rl_random_48": (lambda: workloads.rl_random(48, seed=3), {}),
    "stance_cold_16": (lambda: workloads.stance_cold(16, seed=1), {}),
    # the GPU test's further sets: a batch that is no multiple of four, and stretched legs (the fallback)
    "rl_random_45": (lambda: workloads.rl_random(45, seed=3), {}),
    "straight_20": (lambda: workloads.straight_legs(workloads.rl_random(20, seed=3), every=5), {}),
}
TABLES_SET = "tables_16"
TROT_SET = "trot_8x30_40Nm"
TROT = dict(B=8, steps=30, seed=2, max_torque=40.0)
# the mask-change cycles of the limits step off the trot (tests/offtrot_tables_oracle.py, lmd1): set -> latched
OFFTROT_SETS = {"offtrot_lm_latched": True, "offtrot_lm_unlatched": False}
_CACHE = {}


def _step_controller(c, inp, b):
    CN.load(c, inp, b)
    c.step()
    return c


def cold_set(name):
    """(inputs, parameter overrides, the stepped numpy controller of every robot), computed once."""
    if name not in _CACHE:
        if name == TABLES_SET:
            inp, cols, nrm, rows = tables16()
            cs = []
            for b in range(len(inp["contacts"])):
                c = BB.np_controller(inp, b, rows[b], {k: float(v[b]) for k, v in cols.items()}, CN.SlopedWBC, normals=nrm[b])
                c.step()
                cs.append(c)
            _CACHE[name] = (inp, dict(cols=cols, normals=nrm, rows=rows), cs)
        else:
            make, over = COLD_SETS[name]
            inp = make()
            model = W.Model()
            _CACHE[name] = (inp, over, [_step_controller(W.ReferenceWBC(model, dict(over)), inp, b) for b in range(len(inp["contacts"]))])
    return _CACHE[name]


def trot_set():
    """(the TROT sequence's inputs per cycle, per cycle and robot (qp, x, status) of the stateful numpy oracle)."""
    if TROT_SET not in _CACHE:
        B = TROT["B"]
        seq = list(workloads.trot_sequence(B, steps=TROT["steps"], seed=TROT["seed"]))[:TROT["steps"]]
        model = W.Model()
        robots = [W.ReferenceWBC(model, dict(max_torque=TROT["max_torque"])) for _ in range(B)]
        cycles = []
        for inp in seq:
            row = []
            for b, c in enumerate(robots):
                _step_controller(c, inp, b)
                row.append(Snapshot(c))
            cycles.append(row)
        _CACHE[TROT_SET] = (seq, cycles)
    return _CACHE[TROT_SET]


def offtrot_set(name):
    """The Snapshots (70-row QPs) of offtrot_tables_oracle's limits run on its 256 mask-change cycles, B = 4."""
    import offtrot_tables_oracle as OT  # (it imports this module through the oracles' chain)

    return OT.snapshots("lm", OFFTROT_SETS[name])


class Snapshot:
    """What `expand` and `certificate` read of a controller, kept after the controller has stepped on."""

    def __init__(self, c):
        self.qp, self.params, self.qp_status = c.qp, c.params, c.qp_status
        self.qp_solution = c.qp_solution.copy()


KINDS = ("stationarity", "primal")


def oracle_residual(cs):
    """(the worst stationarity residual, the worst primal violation) of `certificate` over the OK controllers, on
    the oracle's own x.  The primal violation is absolute, as wbc_np.kkt_residuals computes it."""
    stat = viol = 0.0
    for c in cs:
        if c.qp_status == W.QP_OK:
            v, r, _, _ = certificate(c, c.qp_solution, lsq_duals(c, c.qp_solution))
            stat, viol = max(stat, r), max(viol, v)
    return stat, viol


def measure():
    """{"stationarity": {set: worst}, "primal": {set: worst}} of the numpy oracle on its own x."""
    res = {name: oracle_residual(cold_set(name)[2]) for name in (*COLD_SETS, TABLES_SET)}
    res[TROT_SET] = oracle_residual([c for row in trot_set()[1] for c in row])
    for name in OFFTROT_SETS:
        res[name] = oracle_residual(offtrot_set(name))
    return {kind: {name: v[i] for name, v in res.items()} for i, kind in enumerate(KINDS)}


def record(kind="stationarity"):
    return json.load(open(RECORD))[kind]


def gpu_bound(name, kind="stationarity"):
    """The GPU test's bound of a set: the oracle's own figure of that kind times ENGINE_MARGIN.  "stationarity" is
    relative (over 1 + max |H x + g|), "primal" the absolute violation of wbc_np.kkt_residuals."""
    return ENGINE_MARGIN * record(kind)[name]


if __name__ == "__main__":
    res = measure()
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump({"what": "worst stationarity residual (relative) and worst primal violation (absolute, as wbc_np.kkt_residuals "
                           "computes it) of tests/duals_oracle.py certificate() on the numpy oracle's own x with least-squares "
                           "multipliers, per input set; the GPU bounds are these times 53 (tests/test_gpu_duals.py)",
                   **res}, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1))
