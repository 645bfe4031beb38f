"""CPU: the shared checks of tests/table_steps.py fail when they should, on fabricated outputs: assert_identical on
one ulp in any of the five outputs, check_against_oracle on a status and just past each of margins.TAU / GRF / X;
and refusal_texts gives the engine's sentences (csrc/wbc_engine.cpp's refuse_tables) letter for letter."""
import numpy as np

import margins as M
import pytest

import table_steps as T
from quadrupedwholebodycontroller_amd import QP_INFEASIBLE, QP_OK

B = 6


@pytest.fixture(autouse=True)
def own_records(monkeypatch):
    """margins.close records what it is given: keep these fabricated errors out of the session's parity margins."""
    monkeypatch.setattr(M, "_RECORDS", {})


def outputs(seed=0):
    g = np.random.default_rng(seed)
    return dict(tau=g.uniform(-40.0, 40.0, (B, 12)), grf=g.uniform(-90.0, 90.0, (B, 12)), x=g.uniform(-5.0, 5.0, (B, 42)),
                status=np.zeros(B, np.int32), iters=g.integers(0, 9, B).astype(np.int32))


def copy(out):
    return {k: v.copy() for k, v in out.items()}


def one_ulp(out, key, b):
    """A copy with robot b's last entry of `key` one ulp up (status and iters: one more)."""
    o = copy(out)
    v = o[key][b:b + 1].reshape(-1)
    v[-1] = np.nextafter(v[-1], np.inf) if v.dtype.kind == "f" else v[-1] + 1
    return o


@pytest.mark.parametrize("key", T.KEYS)
def test_assert_identical_sees_one_ulp_in_each_output(key):
    a = outputs()
    T.assert_identical(a, copy(a))
    b = one_ulp(a, key, 2)
    with pytest.raises(AssertionError):
        T.assert_identical(a, b)
    with pytest.raises(AssertionError):
        T.assert_identical(b, a)
    others, some = np.arange(B) != 2, np.array([0, 2, 5])
    T.assert_identical(a, b, idx_a=others, idx_b=others)  # a change outside the index passes
    for idx in (some, np.arange(B) == 2):  # a change inside raises
        with pytest.raises(AssertionError):
            T.assert_identical(a, b, idx_a=idx, idx_b=idx)


@pytest.mark.parametrize("key", T.KEYS)
def test_assert_identical_applies_each_index_to_its_own_side(key):
    a = outputs()
    perm = np.random.default_rng(4).permutation(B)
    p = T.take(a, perm)
    T.assert_identical(p, a, idx_b=perm)
    T.assert_identical(a, p, idx_a=perm)
    with pytest.raises(AssertionError):
        T.assert_identical(p, a, idx_a=perm)
    with pytest.raises(AssertionError):
        T.assert_identical(one_ulp(p, key, 1), a, idx_b=perm)


def off_by(ref, key, b, factor, tol):
    """A copy of ref whose robot b misses `key` by factor * tol in margins.norm_err's normalisation."""
    o = copy(ref)
    j = int(np.argmin(np.abs(ref[key][b])))  # (not the largest entry: 1 + max|b| stays the reference's)
    o[key][b, j] += factor * tol * (1.0 + np.abs(ref[key][b]).max())
    assert (M.norm_err(o[key][b], ref[key][b]) > tol) == (factor > 1.0)
    return o


@pytest.mark.parametrize("key,tol", [("tau", M.TAU), ("grf", M.GRF), ("x", M.X)])
def test_check_against_oracle_holds_each_margin(key, tol):
    ref = outputs(1)
    T.check_against_oracle(copy(ref), ref, "equal")
    T.check_against_oracle(off_by(ref, key, 3, 0.98, tol), ref, "just below")
    with pytest.raises(AssertionError):
        T.check_against_oracle(off_by(ref, key, 3, 1.02, tol), ref, "just above")
    with pytest.raises(AssertionError):
        T.check_against_oracle(off_by(ref, key, B - 1, 1.02, tol), ref, "just above, last robot")


def test_check_against_oracle_status():
    ref = outputs(1)
    out = copy(ref)
    out["status"][4] = QP_INFEASIBLE
    with pytest.raises(AssertionError):
        T.check_against_oracle(out, ref, "status")
    # a robot the oracle did not solve: the status must agree, the values are not compared
    ref["status"][4] = QP_INFEASIBLE
    assert QP_INFEASIBLE != QP_OK
    for k in ("tau", "grf", "x"):
        out[k][4] = 1e3
    T.check_against_oracle(out, ref, "not OK")
    out["tau"][3, 0] += 1e-3  # (and the solved robots still are)
    with pytest.raises(AssertionError):
        T.check_against_oracle(out, ref, "not OK, another robot off")


def test_check_against_c_oracles_adds_iters_and_the_solved_count():
    ref = outputs(1)
    out = copy(ref)
    T.check_against_c_oracles(out, ref, ref, "equal")
    out["iters"][1] += 1
    with pytest.raises(AssertionError):
        T.check_against_c_oracles(out, ref, ref, "iters")
    T.check_against_c_oracles(out, ref, ref, "iters, not on that row", iters_rows=np.array([0, 2, 3, 4, 5]))
    with pytest.raises(AssertionError):
        T.check_against_c_oracles(off_by(ref, "tau", 0, 1.02, M.TAU), ref, ref, "tau")
    bad = copy(ref)
    bad["status"][:5] = QP_INFEASIBLE  # the oracle solved one robot of six
    with pytest.raises(AssertionError):
        T.check_against_c_oracles(copy(bad), bad, bad, "too few solved")


def test_moved_counts_robots():
    a = outputs()
    b = copy(a)
    b["tau"][1, 3] += 2e-3
    b["tau"][4, 0] -= 5e-5
    assert T.moved(a, b) == 1 and T.moved(a, b, by=1e-6) == 2 and T.moved(a, copy(a)) == 0


SENTENCES = {
    "robot_params": (("a per-robot parameter table is in force", "a per-robot parameter table in force",
                      "clear it with wbc_set_robot_params(h, NULL)"), "cycle_resident",
                     "wbc_cycle: WBC_RESIDENT with a per-robot parameter table in force (plain cycle only; clear it with "
                     "wbc_set_robot_params(h, NULL))"),
    "contact_normals": (("contact normals are in force", "contact normals in force", "clear them with wbc_set_contact_normals(h, NULL)"),
                        "step_modes",
                        "wbc_step_modes: contact normals are in force (default wbc_step only; clear them with "
                        "wbc_set_contact_normals(h, NULL))"),
    "base_body": (("a per-robot base body table is in force", "a per-robot base body table in force",
                   "clear it with wbc_set_base_body(h, NULL)"), "step_split",
                  "wbc_step: WBC_SPLIT with a per-robot base body table in force (default form only; clear it with "
                  "wbc_set_base_body(h, NULL))"),
    "limits": (("per-robot limits are in force", "per-robot limits in force", "clear them with wbc_set_limits(h, NULL)"), "update",
               "wbc_update: per-robot limits are in force (default wbc_step only; clear them with wbc_set_limits(h, NULL))"),
    "force_bounds": (("per-foot force bounds are in force", "per-foot force bounds in force",
                      "clear them with wbc_set_force_bounds(h, NULL)"), "cycle_fused",
                     "wbc_cycle: WBC_FUSED with per-foot force bounds in force (plain cycle only; clear them with "
                     "wbc_set_force_bounds(h, NULL))"),
}


@pytest.mark.parametrize("name", SENTENCES)
def test_refusal_texts_letter_for_letter(name):
    phrases, key, sentence = SENTENCES[name]
    texts = T.refusal_texts(*phrases)
    assert sorted(texts) == ["cycle_fused", "cycle_resident", "cycle_split", "solve", "step_fused", "step_modes", "step_split",
                             "update"]
    assert texts[key] == sentence
    # every call is named at the head of its own sentence, and the way out at the end of each
    heads = dict(update="wbc_update: ", solve="wbc_solve: ", step_modes="wbc_step_modes: ", step_split="wbc_step: WBC_SPLIT with ",
                 step_fused="wbc_step: WBC_FUSED with ", cycle_split="wbc_cycle: WBC_SPLIT with ",
                 cycle_fused="wbc_cycle: WBC_FUSED with ", cycle_resident="wbc_cycle: WBC_RESIDENT with ")
    for k, text in texts.items():
        assert text.startswith(heads[k]) and text.endswith(f"; {phrases[2]})"), (k, text)
