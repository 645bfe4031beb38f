"""GPU: the QP objective of contact-mode hypotheses and the best feasible hypothesis per state
(wbc_step_modes with WBC_OBJECTIVE / WBC_BEST).

The flags change nothing else: tau, grf, x, status and iters stay the bits of the step without them and of
the per-row step, at every number M of hypotheses per wave (the objective instance of the mode loop,
wbc_kernel_modes_obj.hip, runs at every M, 1 included), and the objective's own bits depend neither on M nor
on WBC_NO_X.  The value is checked against the numpy oracle's 1/2 x^T H x + g^T x
(tests/modes_objective_oracle.py), the selection against the oracle's argmin on a set where feasible and
infeasible hypotheses mix, the tie rule on a repeated mask, the fallback solve's instance on stretched legs.
"""
import ctypes as C
import os

import numpy as np

import margins as M
import modes_objective_oracle as MO
import pytest

import wbc_np as W
from quadrupedwholebodycontroller_amd import (BEST, NO_X, OBJECTIVE, SPLIT, STATELESS, Engine, WbcError, default_params,
                                              workloads)
from table_steps import ERR_ARG, ERR_STATE, last_error
from test_gpu_modes import per_row, replicated
from test_gpu_tables_and_bindings import REFUSALS

pytestmark = pytest.mark.gpu

KEYS = ("tau", "grf", "x", "status", "iters")
# The engine's objective against the numpy oracle's, |d| / (1 + |obj_oracle|) per OK row: 10 x the worst error
# the engine shows on MI355X over this file's cases, rounded up to one digit (the policy of margins.py's
# STATEFUL_* bounds; profiles/modes_objective/parity_margins.json).  Worst: 1.3e-12, on the stress set at 3 N m
# (rl_random 4.9e-14, the stretched legs' fallback solves 1.8e-13); the LITERAL and the REDUCED numpy oracle differ
# by 1.9e-12 on that set (tests/test_modes_objective_cpu.py).  An error above 1e-9 would not be a bound to adopt
# but a defect to find.
OBJ_BOUND = 2e-11


def engine(base, modes, m=None, max_torque=None):
    """An engine of S x K hypotheses loaded with the S states; m: WBC_MODES_M (read by wbc_set_modes)."""
    S, K = base["base_pose"].shape[0], len(modes)
    p = None
    if max_torque is not None:
        p = default_params()
        p.max_torque = max_torque
    e = Engine(S * K, params=p)
    old = os.environ.pop("WBC_MODES_M", None)
    if m is not None:
        os.environ["WBC_MODES_M"] = str(m)
    try:
        e.set_modes(modes)
    finally:
        os.environ.pop("WBC_MODES_M", None)
        if old is not None:
            os.environ["WBC_MODES_M"] = old
    e.set_state(base["base_pose"], base["nu"], base["qj"])
    e.set_reference(base["ref"], base["contacts"], base["switching"])
    return e


def stepped(base, modes, flags, m=None, max_torque=None):
    """One wbc_step_modes: the outputs, the objective (S, K) and, under BEST, the best modes."""
    S, K = base["base_pose"].shape[0], len(modes)
    e = engine(base, modes, m, max_torque)
    e.step_modes(flags)
    out = e.outputs()
    out["objective"] = e.objective().reshape(S, K)
    if flags & BEST:
        out["best"] = e.best_modes()
    e.close()
    return out


def obj_err(got, want, ok):
    return float((np.abs(got[ok] - want[ok]) / (1.0 + np.abs(want[ok]))).max())


def check_objective(out, oracle_status, oracle_obj, what):
    """Status equal to the oracle's, +inf exactly where it is not OK, the bound on the OK rows."""
    S, K = oracle_status.shape
    status = out["status"].reshape(S, K)
    assert np.array_equal(status, oracle_status), what
    ok = status == W.QP_OK
    assert np.isposinf(out["objective"][~ok]).all() and np.isfinite(out["objective"][ok]).all(), what
    assert M.record(what, obj_err(out["objective"], oracle_obj, ok), OBJ_BOUND) <= OBJ_BOUND, what


# --- the flags change nothing else ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def rl10():
    base, modes = workloads.rl_random(10, seed=21), list(range(16))  # S = 10: the last wave has two padding segments
    want = per_row(replicated(base, modes))
    ref = stepped(base, modes, STATELESS | OBJECTIVE)["objective"]
    ref.setflags(write=False)
    return base, modes, want, ref


@pytest.mark.parametrize("m", [None, 1, 2, 4, 16])
def test_flags_change_nothing_else(rl10, m):
    base, modes, want, ref = rl10
    e = engine(base, modes, m)
    assert m is None or e.modes_per_wave() == m
    e.step_modes(STATELESS)
    plain = e.outputs()
    for k in KEYS:
        assert np.array_equal(plain[k], want[k]), (k, "plain against the per-row step")
    for flags, keys in ((STATELESS | OBJECTIVE, KEYS), (STATELESS | BEST, KEYS),
                        (STATELESS | OBJECTIVE | NO_X, ("tau", "grf", "status", "iters")), (STATELESS | BEST | NO_X, ("tau", "grf", "status", "iters"))):
        e.step_modes(flags)
        out = e.outputs()
        for k in keys:
            assert np.array_equal(out[k], plain[k]) and np.array_equal(out[k], want[k]), (k, flags)
        assert np.array_equal(e.objective().reshape(10, 16), ref), ("objective bits", flags, m)
    e.close()
    ok = want["status"].reshape(10, 16) == W.QP_OK
    assert ok.mean() > 0.5 and np.isfinite(ref[ok]).all() and np.isposinf(ref[~ok]).all()


# --- the value ------------------------------------------------------------------------------------------
def test_objective_against_the_oracle():
    base, _, _ = MO.inputs("rl")
    o = MO.oracle_modes("rl")
    out = stepped(base, MO.ALL_MASKS, STATELESS | OBJECTIVE)
    check_objective(out, o["status"], o["obj"], "objective rl_random(8) x 16")


@pytest.fixture(scope="module")
def stress():
    base, _, max_torque = MO.inputs("stress")
    return base, max_torque, MO.oracle_modes("stress")


def test_stress_set_objective_and_best(stress):
    base, max_torque, o = stress
    out = stepped(base, MO.ALL_MASKS, STATELESS | BEST, max_torque=max_torque)
    check_objective(out, o["status"], o["obj"], "objective stress(16, 3 N m) x 16")
    ok = o["status"] == W.QP_OK
    assert 0 < (~ok).sum() < ok.sum()  # (tests/test_modes_objective_cpu.py pins the mix)
    want, _ = MO.best_modes(o["obj"], o["status"])
    b = out["best"]
    assert np.array_equal(b["best"], want), (b["best"], want)
    assert np.array_equal(b["objective"], out["objective"][np.arange(16), want])


def test_stress_subset_with_states_that_have_no_feasible_hypothesis(stress):
    base, max_torque, o = stress
    sub = MO.STRESS_SUBSET
    out = stepped(base, sub, STATELESS | BEST, max_torque=max_torque)
    K = len(sub)
    assert np.array_equal(out["status"].reshape(16, K), o["status"][:, sub])
    want, _ = MO.best_modes(o["obj"][:, sub], o["status"][:, sub])
    none_ok = want < 0
    assert none_ok.sum() >= 3 and (~none_ok).sum() >= 3
    b = out["best"]
    assert np.array_equal(b["best"], want), (b["best"], want)
    assert np.isposinf(b["objective"][none_ok]).all() and np.isfinite(b["objective"][~none_ok]).all()
    assert not b["tau"][none_ok].any() and not b["grf"][none_ok].any()
    rows = np.arange(16)[~none_ok] * K + want[~none_ok]
    assert np.array_equal(b["tau"][~none_ok], out["tau"][rows]) and b["tau"][~none_ok].any()


def test_tie_goes_to_the_lowest_index():
    base, modes = workloads.stance_cold(8, seed=22), [15, 10, 5, 15, 0]
    out = stepped(base, modes, STATELESS | BEST)
    obj = out["objective"]
    assert np.array_equal(obj[:, 0], obj[:, 3]) and np.isfinite(obj[:, 0]).all()  # the repeated mask: the same bits
    wins15 = obj[:, 0] == obj.min(axis=1)
    assert wins15.all()  # the four-contact hypothesis wins in all 8 states (as on the CPU)
    assert np.array_equal(out["best"]["best"][wins15], np.zeros(wins15.sum(), np.int32))  # index 0, never 3


# --- the fallback solve's instance ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stretched():
    base = workloads.straight_legs(workloads.stance_cold(24, seed=25), every=2)
    params, model = W.default_params(), W.Model()
    status = np.zeros((24, 16), np.int32)
    obj = np.full((24, 16), np.inf)
    for s in range(24):
        for k in range(16):
            status[s, k], obj[s, k], _ = MO.oracle_row(base, params, s, k, model)
    return base, status, obj


@pytest.mark.parametrize("m", [None, 1, 4, 16])
def test_fallback_objective(stretched, m):
    """A stretched leg in stance makes the 12-variable reduction unusable: those hypotheses are solved by the
    wave's general 24-variable fallback (drain_fallbacks' objective instance), which forms the objective from
    its own recovered x."""
    base, status, obj = stretched
    modes = MO.ALL_MASKS
    out = stepped(base, modes, STATELESS | OBJECTIVE, m=m)
    want = per_row(replicated(base, modes))
    for k in KEYS:
        assert np.array_equal(out[k], want[k]), k
    check_objective(out, status, obj, "objective stretched legs(24) x 16")
    if m is not None:  # bit-identical across M: against the engine's own choice
        assert np.array_equal(out["objective"], stepped(base, modes, STATELESS | OBJECTIVE)["objective"])


# --- the gather and the device pointers --------------------------------------------------------------------
def test_gather_and_device_pointers():
    import torch

    base, modes = workloads.rl_random(10, seed=21), list(range(16))
    S, K = 10, 16
    e = engine(base, modes)
    e.step_modes(STATELESS | BEST)
    out, obj, b = e.outputs(), e.objective(), e.best_modes()
    assert (b["best"] >= 0).all() and len(set(b["best"].tolist())) > 1
    rows = np.arange(S) * K + b["best"]
    assert np.array_equal(b["tau"], out["tau"][rows]) and np.array_equal(b["grf"], out["grf"][rows])
    assert np.array_equal(b["objective"], obj[rows])
    assert np.array_equal(b["best"], MO.best_modes(obj.reshape(S, K), out["status"].reshape(S, K))[0])
    # the same bits behind the device pointers: device-to-device copies into torch tensors
    hip_memcpy = e.lib.hipMemcpy
    hip_memcpy.argtypes, hip_memcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int

    def read(ptr, shape, dtype):
        t = torch.empty(shape, dtype=dtype, device="cuda")
        assert ptr and hip_memcpy(t.data_ptr(), ptr, t.numel() * t.element_size(), 3) == 0  # hipMemcpyDeviceToDevice
        return t.cpu().numpy()

    e.synchronize()
    assert np.array_equal(read(e.device_objective(), (S * K,), torch.float64), obj)
    d = e.device_best_modes()
    assert np.array_equal(read(d["best"], (S,), torch.int32), b["best"])
    assert np.array_equal(read(d["objective"], (S,), torch.float64), b["objective"])
    assert np.array_equal(read(d["tau"], (S, 12), torch.float64), b["tau"])
    assert np.array_equal(read(d["grf"], (S, 12), torch.float64), b["grf"])
    # any pointer of wbc_get_best_modes may be NULL
    only = np.zeros(S, np.int32)
    assert e.lib.wbc_get_best_modes(e.h, only.ctypes.data_as(C.c_void_p), None, None, None) == 0
    assert np.array_equal(only, b["best"])
    e.close()


# --- errors ----------------------------------------------------------------------------------------------
def raises(e, call, code, text=None):
    with pytest.raises(WbcError) as ei:
        call()
    assert f"({code})" in str(ei.value), str(ei.value)
    if text is not None:
        assert last_error(e) == text


def test_errors():
    inp = workloads.rl_random(8, seed=31)
    e = Engine(8)
    e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
    e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
    for flag in (OBJECTIVE, BEST):
        raises(e, lambda: e.step(STATELESS | flag), ERR_ARG)
        raises(e, lambda: e.update(STATELESS | flag), ERR_ARG)
        e.update(STATELESS)
        raises(e, lambda: e.solve(STATELESS | flag), ERR_ARG)
        raises(e, lambda: e.cycle(inp["base_pose"], inp["nu"], inp["qj"], inp["ref"], inp["contacts"], inp["switching"],
                                  STATELESS | flag), ERR_ARG)
    e.step(STATELESS)  # the engine still steps
    e.close()

    base = workloads.rl_random(4, seed=32)
    e = engine(base, [15, 5])
    for getter in (e.objective, e.device_objective, e.best_modes, e.device_best_modes):
        raises(e, getter, ERR_STATE)  # before any flagged step
    for flag in (OBJECTIVE, BEST):
        raises(e, lambda: e.step_modes(STATELESS | SPLIT | flag), ERR_ARG)
    raises(e, lambda: e.step_modes(OBJECTIVE), ERR_ARG, "wbc_step_modes: hypotheses are cold steps (WBC_STATELESS)")
    e.step_modes(STATELESS | OBJECTIVE)
    assert e.objective().shape == (8,) and e.device_objective()
    raises(e, e.best_modes, ERR_STATE)  # WBC_OBJECTIVE alone
    raises(e, e.device_best_modes, ERR_STATE)
    e.step_modes(STATELESS | BEST)
    assert e.best_modes()["best"].shape == (4,) and e.objective().shape == (8,)
    e.step_modes(STATELESS)  # an unflagged step
    for getter in (e.objective, e.device_objective, e.best_modes, e.device_best_modes):
        raises(e, getter, ERR_STATE)
    # a table in force: refuse_tables' own text, also with the flags
    e.set_robot_params({"friction": 0.8})
    for flags in (STATELESS | OBJECTIVE, STATELESS | BEST, STATELESS | BEST | SPLIT):
        raises(e, lambda: e.step_modes(flags), ERR_STATE, REFUSALS["rp"]["step_modes"])
    e.set_robot_params(None)
    e.set_modes(None)
    raises(e, lambda: e.step_modes(STATELESS | BEST), ERR_STATE, "wbc_step_modes: no mode hypotheses set (wbc_set_modes)")
    e.close()
