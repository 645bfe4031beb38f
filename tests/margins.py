"""Parity margins: what each GPU parity test actually achieved against its bound.

Tests call `record(quantity, achieved, bound)` (an error normalised as the test normalises it, or a
mismatch fraction) and `close(a, b, tol, quantity)` for the usual max|a - b| <= tol (1 + max|b|)
check.  Each record is printed (visible with pytest -s / -v on failure) and kept per (test,
quantity) as the worst value seen; conftest.py writes them at the end of the session to
$WBC_MARGINS_OUT (default gpurun_out/parity_margins.json) as
{test: {quantity: {"achieved", "bound", "margin" = bound / achieved}}}."""
import os

import numpy as np

_RECORDS = {}

# Bounds of the GPU parity tests, tightened (round 4) to the worst error the tests achieve on MI355X
# times 6-53 (the "worst" comments: profiles/r05/parity_margins.json, regenerated with
# tools/margins_report.py), far inside SURVEY.md 8c's contract (x* 1e-8 (1 + |x*|), tau 1e-7 N m,
# intermediates 1e-12): a change that moves the engine's rounding shows up here first.
TAU = 1e-9        # tau against the oracle (cold, stateful, stress); worst 1.6e-10 (stress6, split kernels)
X = 1e-9          # x* against the oracle; worst 1.9e-11
GRF = 2e-11       # ground reaction forces against the oracle; worst 7.7e-13
BITS = 1e-13      # two engine paths that should agree to a few ulps (kernels of one form); worst 4.6e-15
INTERMEDIATE = {"W": 5e-12, "Mbar_b": 1e-12, "rsw": 1e-12,  # worst 1.5e-13, 2.1e-14, 3.1e-14; others 1e-13 (worst 9.1e-15)
                # kinematics and the J / Mbar_j blocks: within a few ulps (worst 6.7e-16)
                **{k: 1e-14 for k in ("Jbar", "Jfeet", "Mbar_j", "com", "comvel", "pfeet", "pose", "vc", "vfeet", "r1")}}
GOLD = 1e-12      # tau against the committed cold fixtures and ragged batches (worst 1.3e-13)
REPLAY = 1e-13    # the C++ shim's replay of the golden trajectories (worst 1.4e-14)

# Stateful steps off the trot (tests/test_gpu_stateful_offtrot.py, the golden trajectories' intermediates): 10 x the
# worst error of the engine against the C oracle on MI355X over those cases, rounded up to one digit
# (profiles/r08/stateful_offtrot/parity_margins.json).  "spread": the numpy and the C oracle against each other on the
# same inputs (tests/test_stateful_sequences_cpu.py, profiles/r08/stateful_offtrot/oracle_spread.json).  r1 and rsw hold
# the 1 / dt = 400 amplification and reach 1e3 on a first cycle (J / dt); W's worst is kp_z = 1e4 times two ulps of the
# CoM height on a component near 0.3 (18 x the spread: the oracles share one libm and one kinematics order)
STATEFUL_INTERMEDIATE = {"bbar": 5e-13,  # worst 4.6e-14, spread 2.1e-14
                         "W": 3e-11,     # worst 2.3e-12, spread 1.3e-13
                         "r1": 2e-11,    # worst 1.2e-12, spread 4.4e-13
                         "rsw": 9e-12}   # worst 8.8e-13, spread 2.9e-13
# tau and x of the default path's stateful kernel against the LITERAL oracle on those cases (TAU and X above also cover
# the split kernels and the stress sets): worst 5.7e-13 and 2.6e-12, both on unlatched rows
STATEFUL_TAU = 6e-12
STATEFUL_X = 3e-11
# grf against the LITERAL oracle under the per-robot table off the trot: the reference's own error.  Where the forces
# are zero or tiny beside accelerations of 1e3 (a first cycle, an unlatched change) the 42 x 70 solve leaves 7e-11 of
# absolute noise in them, and grf is normalised by its own size: the LITERAL and the REDUCED oracle differ by 6.7e-11
# there, and one ulp on the inputs moves the REDUCED oracle's own grf by 1.5e-11 where a stance leg carries 0.1 N on the
# edge of its cone (CPU, tests/test_stateful_sequences_cpu.py).  10 x the larger; the engine's worst is 6.7e-11.
STATEFUL_TABLE_GRF = 7e-10


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]


def record(quantity, achieved, bound):
    achieved = float(achieved)
    t = _RECORDS.setdefault(_test_id(), {})
    cur = t.get(quantity)
    if cur is None or achieved > cur["achieved"]:
        t[quantity] = {"achieved": achieved, "bound": float(bound),
                       "margin": (float(bound) / achieved) if achieved > 0 else None}
    print(f"[margin] {_test_id()} {quantity}: {achieved:.3e} (bound {bound:.1e})")
    return achieved


def norm_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b)) / (1.0 + np.max(np.abs(b))))


def close(a, b, tol, quantity="max|a-b|/(1+max|b|)"):
    """max|a - b| <= tol (1 + max|b|), with the achieved value recorded."""
    return record(quantity, norm_err(a, b), tol) <= tol


def records():
    return _RECORDS
