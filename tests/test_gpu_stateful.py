"""GPU parity, part 2: committed golden fixtures, stateful trajectories, resets, ragged batches,
device-bound I/O and non-finite inputs -- all through the C-ABI (libwbc_hip.so).

Stateful mode (flags without WBC_STATELESS) carries the reference's per-robot history across
steps: finite differences of T, Jbar_c, Jbar_s (cpp:384-402), the one-cycle lag of Tdot_inv
(cpp:289,293), the integral error (cpp:442) and the first-cycle quirks T_old = I, J_old = 0
(cpp:86-88).  The checker is the C restatement (oracle/wbc_ref.c,
one `Robot` per robot, same inputs) and the committed trajectory fixtures.

Tolerances (tests/margins.py): x* and tau 1e-9 * (1 + |.|_inf) against the oracle, including the
stateful trajectories, whose finite-difference history goes through the 1/dt = 400 amplification
(worst measured 7e-14, profiles/r04/parity_margins.json); 1e-12 against the committed cold fixtures,
1e-13 between a hot and a cold start of one QP; QP status identical.
"""
import os

import numpy as np

import margins as M
import pytest

import wbc_ref as R
from quadrupedwholebodycontroller_amd import DEBUG, STATELESS, Engine, split_debug, workloads

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def close_to(a, b, tol, quantity="value"):
    return M.close(a, b, tol, quantity)


def run_cold(inp):
    B = inp["base_pose"].shape[0]
    e = Engine(B)
    e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
    e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
    e.step(STATELESS)
    out = e.outputs()
    e.close()
    return out


@pytest.mark.parametrize("name", ["stance_cold", "rl_random", "all_masks"])
def test_cold_golden_fixtures(name):
    g = load(name)
    inp = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    out = run_cold(inp)
    assert np.array_equal(out["status"], g["out_status"]), name
    for b in np.nonzero(g["out_status"] == 0)[0]:
        assert close_to(out["x"][b], g["out_x"][b], M.X, "x"), (name, b, "x")
        assert close_to(out["tau"][b], g["out_tau"][b], M.GOLD, "tau"), (name, b, "tau")


@pytest.mark.parametrize("name", ["traj_stance_hold", "traj_trot"])
def test_stateful_trajectory_golden(name):
    g = load(name)
    T, nr = g["in_base_pose"].shape[:2]
    e = Engine(nr)
    for t in range(T):
        e.set_state(g["in_base_pose"][t], g["in_nu"][t], g["in_qj"][t])
        e.set_reference(g["in_ref"][t], g["in_contacts"][t], g["in_switching"][t])
        e.step(DEBUG)
        o = e.outputs()
        assert np.array_equal(o["status"], g["out_status"][t]), t
        for j, rec in enumerate(e.debug()):  # the stateful intermediates, feasible or not
            d = split_debug(rec)
            for k, a, b in (("bbar", d["bbar"][6:], g["out_bbar"][t, j][6:]), ("r1", d["r1"], g["out_r1"][t, j]),
                            ("rsw", d["rsw"], g["out_rsw"][t, j])):
                err = np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
                assert M.record(k, err, M.STATEFUL_INTERMEDIATE[k]) <= M.STATEFUL_INTERMEDIATE[k], (t, j, k)
        for j in range(nr):
            if g["out_status"][t, j] == 0:
                assert close_to(o["x"][j], g["out_x"][t, j], M.X, "x"), (t, j, "x")
                assert close_to(o["tau"][j], g["out_tau"][t, j], M.TAU, "tau"), (t, j, "tau")
    e.close()


def _trot_steps(B, steps, seed):
    return list(workloads.trot_sequence(B, steps=steps, seed=seed))[:steps]


def test_stateful_trot_batch_vs_c_oracle():
    """64 robots x 120 trot steps (two contact switches), history carried on the GPU."""
    B, steps = 64, 120
    seq = _trot_steps(B, steps, seed=21)
    robots = [R.Robot() for _ in range(B)]
    e = Engine(B)
    n_checked = 0
    for t, inp in enumerate(seq):
        e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
        e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        e.step(0)
        o = e.outputs()
        for j in range(B):
            r = robots[j].step(inp["base_pose"][j], inp["nu"][j], inp["qj"][j], inp["ref"][j],
                               int(inp["contacts"][j]), int(inp["switching"][j]))
            assert o["status"][j] == r["status"], (t, j)
            if r["status"] == 0:
                assert close_to(o["tau"][j], r["tau"], M.TAU, "tau"), (t, j)
                assert close_to(o["x"][j], r["x"], M.X, "x"), (t, j)
                n_checked += 1
    e.close()
    assert n_checked > B * steps // 2


def test_reset_mask_restarts_selected_robots():
    """wbc_reset(mask) == setInitialState() + firstControllerIteration_ for the masked robots only."""
    B, steps = 16, 40
    seq = _trot_steps(B, steps, seed=22)
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)
    robots = [R.Robot() for _ in range(B)]
    e = Engine(B)
    for t, inp in enumerate(seq):
        if t == 20:
            e.reset(mask)
            for j in np.nonzero(mask)[0]:
                robots[j] = R.Robot()
        e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
        e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        e.step(0)
        o = e.outputs()
        for j in range(B):
            r = robots[j].step(inp["base_pose"][j], inp["nu"][j], inp["qj"][j], inp["ref"][j],
                               int(inp["contacts"][j]), int(inp["switching"][j]))
            assert o["status"][j] == r["status"], (t, j)
            if r["status"] == 0:
                assert close_to(o["tau"][j], r["tau"], M.TAU, "tau"), (t, j)
    e.close()


@pytest.mark.parametrize("B", [1, 7, 63, 65, 1000])
def test_ragged_batches_vs_c_oracle(B):
    inp = workloads.rl_random(B, seed=100 + B)
    out = run_cold(inp)
    ref = R.run_batch(inp)
    assert np.array_equal(out["status"], ref["status"])
    ok = ref["status"] == 0
    for b in np.nonzero(ok)[0]:
        assert close_to(out["x"][b], ref["x"][b], M.X, "x"), b
        assert close_to(out["tau"][b], ref["tau"][b], M.GOLD, "tau"), b


def test_nonfinite_input_is_isolated():
    inp = workloads.stance_cold(128, seed=31)
    bad = [3, 64, 127]
    inp["nu"][3, 7] = np.nan
    inp["qj"][64, 2] = np.inf
    inp["ref"][127, 0] = np.nan
    out = run_cold(inp)
    assert all(out["status"][b] == 3 for b in bad)  # WBC_QP_NUMERIC
    good = np.setdiff1d(np.arange(128), bad)
    ref = R.run_batch({k: v[good] for k, v in inp.items()})
    assert np.array_equal(out["status"][good], ref["status"])
    assert close_to(out["tau"][good], ref["tau"], M.GOLD, "tau")


def test_device_bound_inputs_and_outputs():
    """wbc_bind_device_inputs/outputs: the step reads and writes caller-owned HBM, no copies."""
    import torch

    B = 300
    inp = workloads.rl_random(B, seed=41)
    host = run_cold(inp)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
    tau = torch.zeros(B, 12, dtype=torch.float64, device="cuda")
    grf = torch.zeros(B, 12, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    e = Engine(B)
    e.bind_device_inputs(d["base_pose"].data_ptr(), d["nu"].data_ptr(), d["qj"].data_ptr(), d["ref"].data_ptr(),
                         d["contacts"].data_ptr(), d["switching"].data_ptr())
    e.bind_device_outputs(tau=tau.data_ptr(), grf=grf.data_ptr(), status=status.data_ptr())
    e.step(STATELESS)
    e.synchronize()
    assert np.array_equal(tau.cpu().numpy(), host["tau"])
    assert np.array_equal(grf.cpu().numpy(), host["grf"])
    assert np.array_equal(status.cpu().numpy(), host["status"])
    e.close()


def test_no_x_flag_keeps_published_outputs():
    """WBC_NO_X skips only the x[42] row; tau, grf, status, iters are bit-identical."""
    from quadrupedwholebodycontroller_amd import NO_X

    B = 200
    inp = workloads.rl_random(B, seed=51)
    e = Engine(B)
    e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
    e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
    e.step(STATELESS)
    full = e.outputs()
    e.step(STATELESS | NO_X)
    lean = e.outputs()
    e.close()
    for k in ("tau", "grf", "status", "iters"):
        assert np.array_equal(full[k], lean[k]), k


def test_hotstart_same_solution_fewer_iterations():
    """Stateful steps hotstart the dual active set from the previous working set (qpOASES
    SQProblem::hotstart, cpp:531); WBC_COLD keeps the history but starts the QP cold.  Same
    torques, fewer active-set iterations over a trot (the working set persists within a stance
    phase; rejected warm sets fall back to the cold start)."""
    from quadrupedwholebodycontroller_amd import COLD

    B, steps = 128, 150
    seq = _trot_steps(B, steps, seed=23)
    hot, cold = Engine(B), Engine(B)
    it_hot = it_cold = 0
    for t, inp in enumerate(seq):
        for e in (hot, cold):
            e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
            e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        hot.step(0)
        cold.step(COLD)
        oh, oc = hot.outputs(), cold.outputs()
        assert np.array_equal(oh["status"], oc["status"]), t
        ok = oc["status"] == 0
        assert close_to(oh["tau"][ok], oc["tau"][ok], M.BITS, "tau"), t
        assert close_to(oh["x"][ok], oc["x"][ok], M.BITS, "x"), t
        if t > 0:
            it_hot += int(oh["iters"].sum())
            it_cold += int(oc["iters"].sum())
    hot.close()
    cold.close()
    assert it_hot < 0.5 * it_cold, (it_hot, it_cold)


def test_stateful_trot_with_stretched_legs_vs_c_oracle():
    """Stateful steps where a stretched (singular) leg makes the 12-variable reduction unusable
    whenever that leg is in stance: those cycles are solved by the update wave's general 24-variable
    fallback, the others by the 12-variable form with its hotstart, and the history
    (finite differences, working sets in either numbering) carries across the switches."""
    B, steps = 24, 60
    seq = [workloads.straight_legs(inp, every=3) for inp in _trot_steps(B, steps, seed=23)]
    robots = [R.Robot() for _ in range(B)]
    e = Engine(B)
    n_checked = 0
    for t, inp in enumerate(seq):
        e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
        e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        e.step(0)
        o = e.outputs()
        for j in range(B):
            r = robots[j].step(inp["base_pose"][j], inp["nu"][j], inp["qj"][j], inp["ref"][j],
                               int(inp["contacts"][j]), int(inp["switching"][j]))
            assert o["status"][j] == r["status"], (t, j)
            if r["status"] == 0:
                assert close_to(o["tau"][j], r["tau"], M.TAU, "tau"), (t, j)
                assert close_to(o["x"][j], r["x"], M.X, "x"), (t, j)
                n_checked += 1
    e.close()
    assert n_checked > B * steps // 2


def test_long_trot_no_drift_vs_c_oracle():
    """2000 stateful cycles (5 s at 400 Hz, 20 contact switches) of 64 robots against the C
    oracle's stateful robots (the REDUCED method: the same 12-variable form and hotstart): status and
    iteration counts equal at every cycle, tau at the parity tolerance at every cycle.  The integral
    error e_int and the finite-difference history accumulate over the whole run, so a bias in either
    would grow here: the worst error of the last 200 cycles is at most 10 x that of the first 200."""
    B, steps = 64, 2000
    robots = R.Robots(np.arange(B), method=R.REDUCED)
    e = Engine(B)
    err = np.zeros(steps)
    for t, inp in enumerate(workloads.trot_sequence(B, steps=steps, seed=24)):
        e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
        e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        e.step(0)
        o = e.outputs()
        r = robots.step(inp)
        assert np.array_equal(o["status"], r["status"]) and np.array_equal(o["iters"], r["iters"]), t
        ok = r["status"] == 0
        assert close_to(o["tau"][ok], r["tau"][ok], M.TAU, "tau"), t
        err[t] = M.norm_err(o["tau"][ok], r["tau"][ok])
    e.close()
    # no growth with time: the worst error of the last 200 cycles against that of the first 200 (both
    # spans hold two contact switches), with a floor of a few ulps so that two noise-level numbers
    # cannot fail it
    early = M.record("tau, first 200 cycles", err[:200].max(), M.TAU)
    late = M.record("tau, last 200 cycles", err[-200:].max(), M.TAU)
    assert late <= max(10.0 * early, M.BITS), (early, late)
