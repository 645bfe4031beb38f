"""CPU: the off-trot sequence generator (tests/stateful_sequences.py) and the oracles on it.

The GPU tests of tests/test_gpu_stateful_offtrot.py are only as good as their inputs and their
checker: here the inputs are shown to cover what they claim (all 256 ordered mask changes per robot,
a yaw through +-pi, feasible and infeasible solves), the C oracle's two QP forms to agree on every
status, the hotstart to pay, and the numpy and the C restatement of the reference to agree on the
stateful intermediates.  The last figure is the reference's own spread: the engine's error on
bbar / W / r1 / rsw is judged against it (tests/margins.py STATEFUL_INTERMEDIATE).
"""
import numpy as np

import margins as M
import stateful_sequences as S
import wbc_np as W
import wbc_ref as R

B, DWELL, SEED = 8, 3, 5
STEPS = 256 * DWELL
KEYS = ("base_pose", "nu", "qj", "ref")


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))


def run(latch, **kw):
    """status, iters [STEPS, B] and tau, x, grf of B stateful C-oracle robots over the sequence."""
    robots = R.Robots(np.arange(B), **kw)
    out = [robots.step(s) for s in S.sequence(B, DWELL, SEED, latch)]
    return {k: np.array([o[k] for o in out]) for k in ("status", "iters", "tau", "x", "grf")}


_RUNS = {}


def cached(latch, method, hotstart=True):
    key = (latch, method, hotstart)
    if key not in _RUNS:
        _RUNS[key] = run(latch, method=method, hotstart=hotstart)
    return _RUNS[key]


def test_circuit_is_eulerian_and_fixed():
    circ = S.mask_circuit()
    assert circ[0] == 15 and len(circ) == 256
    edges = set(zip(circ.tolist(), np.roll(circ, -1).tolist()))
    assert len(edges) == 256
    assert np.array_equal(circ[:8], [15, 0, 0, 1, 0, 2, 0, 3])  # successors in ascending order


def test_every_robot_makes_every_mask_change():
    for latch in (True, False):
        seq = S.sequence(B, DWELL, SEED, latch)
        assert len(seq) == STEPS
        masks = np.array([s["contacts"] for s in seq])
        sw = np.array([s["switching"] for s in seq])
        prev = np.vstack([np.full((1, B), 15, np.uint8), masks[:-1]])
        for b in range(B):
            changes = set(zip(prev[::DWELL, b].tolist(), masks[::DWELL, b].tolist()))
            assert len(changes) == 256, (b, len(changes))
            # the mask is held for `dwell` cycles
            assert np.array_equal(masks[:, b], np.repeat(masks[::DWELL, b], DWELL))
        assert np.array_equal(sw, (masks != prev) if latch else np.zeros_like(masks))
        # different offsets: a batch step mixes masks
        assert np.mean([len(set(m.tolist())) for m in masks]) > B / 2
    # robot 0 starts on mask 15, unlatched, with a turned base
    s0 = S.sequence(B, DWELL, SEED, True)[0]
    assert s0["contacts"][0] == 15 and s0["switching"][0] == 0 and abs(s0["base_pose"][0, 6]) < 0.999


def test_inputs_are_consistent():
    """Unit quaternions; nu is the derivative of the pose and joints (central differences of the
    generator's own samples); the desired yaw is the actual one in (-pi, pi]."""
    seq = S.sequence(B, DWELL, SEED, True)
    dt = 1.0 / S.LOOP_RATE
    for k in (1, 200, 766):
        a, s, c = seq[k - 1], seq[k], seq[k + 1]
        assert np.allclose(np.linalg.norm(s["base_pose"][:, 3:7], axis=1), 1.0, atol=1e-14)
        assert np.allclose((c["qj"] - a["qj"]) / (2 * dt), s["nu"][:, 6:], atol=2e-3)
        assert np.allclose((c["base_pose"][:, :3] - a["base_pose"][:, :3]) / (2 * dt), s["nu"][:, :3], atol=1e-4)
        for b in range(B):
            Ra, Rc = (W.quat_to_R(*x["base_pose"][b, 3:7]) for x in (a, c))
            Rs = W.quat_to_R(*s["base_pose"][b, 3:7])
            Sw = (Rc - Ra) / (2 * dt) @ Rs.T  # Rdot R' = S(omega), omega in the world frame
            om = np.array([Sw[2, 1], Sw[0, 2], Sw[1, 0]])
            assert np.allclose(om, s["nu"][b, 3:6], atol=2e-3), (k, b)
            assert abs(W.eul_angles_rpy(Rs)[2] - s["ref"][b, 5]) < 1e-12, (k, b)
        assert np.all((s["ref"][:, 5] > -np.pi) & (s["ref"][:, 5] <= np.pi))


def test_a_yaw_passes_pi():
    yaw = S.yaw_of(B, SEED, STEPS, DWELL)
    turns = np.floor((yaw + np.pi) / (2 * np.pi))
    assert np.any(turns.max(axis=0) != turns.min(axis=0))
    des = np.array([s["ref"][:, 5] for s in S.sequence(B, DWELL, SEED, True)])
    assert np.max(np.abs(np.diff(des, axis=0))) > 6.0  # the desired yaw jumps by 2 pi with it


def test_literal_and_reduced_agree_on_status():
    for latch in (True, False):
        lit, red = cached(latch, R.LITERAL), cached(latch, R.REDUCED)
        assert np.array_equal(lit["status"], red["status"]), latch
        ok = lit["status"] == W.QP_OK
        for k, tol in (("tau", M.TAU), ("x", M.X)):
            for t, b in zip(*np.nonzero(ok)):
                err = M.norm_err(red[k][t, b], lit[k][t, b])
                assert err <= tol, (latch, k, t, b, err)


def test_literal_and_reduced_grf_under_the_table():
    """The reference's own error on grf under table_steps.table(8, 11), robot b under row b,
    in the GPU tests' measure max|a - b| / (1 + max|grf|): the two QP forms against each other (forces
    near zero beside accelerations of 1e3 keep the literal 42 x 70 solve's absolute noise), and the
    12-variable form against itself with every input moved by at most one ulp (a barely loaded stance
    leg on the edge of its friction cone).  Both are far above the spread on tau; ten times the larger
    (6.7e-11), rounded up, is margins.STATEFUL_TABLE_GRF."""
    from table_steps import row_dict, table

    rows, g = table(B, 11), np.random.default_rng(0)
    for latch in (True, False):
        forms = ulp = 0.0
        for b in range(B):
            kw = row_dict(rows[b])
            lit, red, moved = R.Robot(**kw), R.Robot(method=R.REDUCED, **kw), R.Robot(method=R.REDUCED, **kw)
            for s in S.sequence(B, DWELL, SEED, latch):
                a = [s[q][b] for q in KEYS]
                con = [int(s["contacts"][b]), int(s["switching"][b])]
                l, r = lit.step(*a, *con), red.step(*a, *con)
                m = moved.step(*[v * (1.0 + 2.0 ** -52 * g.uniform(-1, 1, v.shape)) for v in a], *con)
                assert l["status"] == r["status"], (latch, b)
                if l["status"] == W.QP_OK:
                    forms = max(forms, M.norm_err(r["grf"], l["grf"]))
                    if m["status"] == W.QP_OK:
                        ulp = max(ulp, M.norm_err(m["grf"], r["grf"]))
        tag = "latched" if latch else "unlatched"
        bound = M.STATEFUL_TABLE_GRF  # the oracles meet what the engine is held to; the figures are recorded
        assert M.record(f"oracle spread grf, table, {tag}, LITERAL vs REDUCED", forms, bound) <= bound
        assert M.record(f"oracle spread grf, table, {tag}, inputs moved by an ulp", ulp, bound) <= bound


def test_latched_is_feasible_unlatched_is_both():
    n = STEPS * B
    lat, unl = cached(True, R.LITERAL)["status"], cached(False, R.LITERAL)["status"]
    assert np.sum(lat == W.QP_OK) >= 0.9 * n
    assert np.sum(unl == W.QP_OK) >= 0.1 * n and np.sum(unl == W.QP_INFEASIBLE) >= 0.1 * n
    print("latched OK", np.sum(lat == W.QP_OK), "unlatched OK / INFEASIBLE", np.sum(unl == W.QP_OK),
          np.sum(unl == W.QP_INFEASIBLE), "of", n)


def test_hotstart_halves_the_iterations():
    hot, cold = cached(True, R.REDUCED), cached(True, R.REDUCED, hotstart=False)
    assert np.array_equal(hot["status"], cold["status"])
    assert hot["iters"].sum() < 0.5 * cold["iters"].sum(), (hot["iters"].sum(), cold["iters"].sum())


def test_numpy_and_c_oracle_agree_on_stateful_intermediates():
    """One robot (robot 0: first cycle unlatched on a turned base), 240 cycles (80 dwells), latched
    and unlatched: the two restatements of the reference on bbar[6:], W, r1, rsw and tau.  The worst
    disagreements go to the margins record as the reference's own spread; the bound here is the
    stateful intermediate bound of the GPU tests (the engine is held to what the oracles hold)."""
    n, b = 240, 0
    model, params = W.Model(), W.default_params()
    for latch in (True, False):
        c_robot, np_robot = R.Robot(), W.ReferenceWBC(model, params)
        for k, s in enumerate(S.sequence(B, DWELL, SEED, latch)[:n]):
            con, sw = int(s["contacts"][b]), int(s["switching"][b])
            c = c_robot.step(*[s[q][b] for q in KEYS], con, sw, debug=True)
            np_robot.set_state(s["base_pose"][b], s["nu"][b], s["qj"][b])
            np_robot.set_reference(s["ref"][b], [(con >> i) & 1 for i in range(4)], bool(sw))
            np_robot.step()
            d, ref = c["dbg"], np_robot.debug_record()
            assert c["status"] == np_robot.qp_status, (latch, k)
            for q in ("bbar", "W", "r1", "rsw"):
                x, y = (d[q][6:], ref[q][6:]) if q == "bbar" else (d[q], ref[q])
                tol = M.STATEFUL_INTERMEDIATE[q]
                assert M.record(f"oracle spread {q}", rel_err(x, y), tol) <= tol, (latch, k, q)
            if c["status"] == W.QP_OK:
                assert M.record("oracle spread tau", rel_err(c["tau"], np_robot.tau), M.TAU) <= M.TAU, (latch, k)


# The table combinations of tests/test_gpu_stateful_offtrot.py::test_tables, on the oracle alone ---------
import pytest  # noqa: E402

import test_gpu_stateful_offtrot as OT  # noqa: E402  (its oracle(), cache and COMBOS: importing it needs no GPU)

# each combination with one of its tables taken out: what that table must move
LESS = {"normals": {"normals": {}}, "payload": {"payload": {}},
        "params_normals": {"params": dict(nrm=5), "normals": dict(tab=11)},
        "all_three": {"params": dict(nrm=5, bb=11), "normals": dict(tab=11, bb=11), "payload": dict(tab=11, nrm=5)}}


@pytest.mark.parametrize("combo", list(OT.COMBOS))
def test_table_combinations_on_the_oracle(combo):
    """What the GPU cases of a table combination rest on, shown by the C oracle before any GPU run, with
    the seeds the issue of those cases names (table(8, 11), normals(8, 5, 0.35), payload_rows(8): none had
    to be changed):
      * latched, at least 0.9 of the 6 144 solves are OK; unlatched, at least 0.1 are OK, at least 0.1
        INFEASIBLE, and there is no third status;
      * LITERAL and REDUCED agree on every status;
      * every table in force matters: with it taken out, tau moves by more than 1e-3 N m on at least half
        of the rows that are OK in both runs (latched);
      * the oracles' own spread on tau, x and grf in the GPU tests' measure, recorded and held to the
        bounds the engine is held to: LITERAL against REDUCED, and REDUCED against itself with every
        input moved by at most one ulp."""
    kw, n = OT.COMBOS[combo], STEPS * B
    for latch in (True, False):
        tag = "latched" if latch else "unlatched"
        lit, red, ulp = (OT.oracle(latch, R.LITERAL, **kw), OT.oracle(latch, R.REDUCED, **kw),
                         OT.oracle(latch, R.REDUCED, ulp=0, **kw))
        assert lit["status"].shape == (STEPS, B)
        n_ok, n_inf = int(np.sum(lit["status"] == W.QP_OK)), int(np.sum(lit["status"] == W.QP_INFEASIBLE))
        print(combo, tag, "OK", n_ok, "INFEASIBLE", n_inf, "of", n)
        if latch:
            assert n_ok >= 0.9 * n and n_ok + n_inf == n, (n_ok, n_inf)
        else:
            assert n_ok >= 0.1 * n and n_inf >= 0.1 * n and n_ok + n_inf == n, (n_ok, n_inf)
        assert np.array_equal(lit["status"], red["status"]), tag
        ok = lit["status"] == W.QP_OK
        ok_ulp = ok & (ulp["status"] == W.QP_OK)
        assert ok_ulp.sum() >= 0.99 * ok.sum()
        for q, bound in OT.TABLE_TOLS.items():
            forms = np.where(ok, OT.norm_err(red[q], lit[q]), 0.0).max()
            moved = np.where(ok_ulp, OT.norm_err(ulp[q], red[q]), 0.0).max()
            assert M.record(f"oracle spread {q}, {combo}, {tag}, LITERAL vs REDUCED", forms, bound) <= bound
            assert M.record(f"oracle spread {q}, {combo}, {tag}, inputs moved by an ulp", moved, bound) <= bound
    lit = OT.oracle(True, R.LITERAL, **kw)
    for name, less in LESS[combo].items():
        other = OT.oracle(True, R.LITERAL, **less)
        both = (lit["status"] == W.QP_OK) & (other["status"] == W.QP_OK)
        frac = np.mean((np.abs(lit["tau"] - other["tau"]).max(axis=-1) > 1e-3)[both])
        print(combo, ": without the", name, "table tau moves on", f"{frac:.3f}", "of", int(both.sum()), "rows")
        assert both.sum() >= 0.9 * n and frac >= 0.5, (name, frac)


def test_the_swap_and_the_reset_change_the_oracle_run():
    """The oracle halves of test_tables_swapped_at_an_unlatched_mask_change and test_reset_under_tables:
    cycle 300 is a mask change for every robot, the swapped run equals the unswapped one before it and
    differs from it there on every robot, and the reset changes robots 1, 4 and 6 alone."""
    kw = OT.COMBOS["all_three"]
    seq = S.sequence(B, DWELL, SEED, False)
    assert OT.SWAP_AT == OT.RESET_AT == 300 and np.all(seq[299]["contacts"] != seq[300]["contacts"])
    plain, swapped = OT.oracle(False, R.LITERAL, **kw), OT.oracle(False, R.LITERAL, swap=True, **kw)
    for q in OT.STATEFUL_Q + ("tau", "status"):
        assert np.array_equal(plain[q][:300], swapped[q][:300]), q
    for b in range(B):
        assert any(np.any(plain[q][300, b] != swapped[q][300, b]) for q in ("r1", "rsw")), b
    plain, reset = OT.oracle(True, R.LITERAL, **kw), OT.oracle(True, R.LITERAL, reset=True, **kw)
    for b in range(B):
        changed = any(np.any(plain[q][300, b] != reset[q][300, b]) for q in OT.STATEFUL_Q)
        assert changed == (b in OT.RESET_ROBOTS), b
