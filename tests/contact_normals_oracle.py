"""The oracle of the per-robot contact normals (wbc_set_contact_normals, include/wbc.h),
built on the numpy oracle without changing what it computes: a subclass of wbc_np.ReferenceWBC whose friction rows
stand on each foot's own frame, the same edit on the reduced 12-variable problem of
wbc_reduced.reduced_problem, and the generator of the normal tables the tests use.

For foot l with ground normal m (world frame):
    n = m / |m|,   t1 = (e_x - (e_x . n) n) / |...|,   t2 = n x t1
and the four faces of its pyramid are the reference's (cpp:404-424), in its order, bounds (-inf, 0]:
    t1 - mu n,   -(t1 + mu n),   t2 - mu n,   -(t2 + mu n)."""
import numpy as np

import wbc_np as W
import wbc_reduced as WR

NL, NJ, NV = 4, 12, 42
FLAT = np.tile([0.0, 0.0, 1.0], (NL, 1))


def frame(m):
    """(n, t1, t2) of one foot's normal m."""
    m = np.asarray(m, float)
    n = m / np.sqrt(m @ m)
    u = np.array([1.0 - n[0] * n[0], 0.0 - n[0] * n[1], 0.0 - n[0] * n[2]])
    t1 = u * (1.0 / np.sqrt(u @ u))
    t2 = np.array([n[1] * t1[2] - n[2] * t1[1], n[2] * t1[0] - n[0] * t1[2], n[0] * t1[1] - n[1] * t1[0]])
    return n, t1, t2


def faces(m, mu):
    """D (4 x 3) of one foot: rows D[rr] f <= 0."""
    n, t1, t2 = frame(m)
    return np.vstack([t1 - mu * n, -(t1 + mu * n), t2 - mu * n, -(t2 + mu * n)])


def valid(m):
    """The validity rule of one foot's normal (wbc_layout.h cn_valid)."""
    m = np.asarray(m, float)
    s = float(m @ m)
    return bool(np.isfinite(m).all() and 0.25 <= s <= 4.0 and m[2] > 0.0 and 4.0 * m[2] * m[2] >= s)


def normals(B, seed, tilt):
    """[B, 4, 3] unit normals, each tilted by up to `tilt` rad from z in a uniform direction."""
    g = np.random.default_rng(seed)
    th = g.uniform(0, tilt, (B, 4))
    ph = g.uniform(0, 2 * np.pi, (B, 4))
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=2)


class SlopedWBC(W.ReferenceWBC):
    """wbc_np.ReferenceWBC on sloped ground: `normals` is [4, 3], one ground normal per foot (it may be
    replaced between steps).  Only the friction rows of the literal 42 x 70 QP change."""

    def __init__(self, model=None, params=None, normals=None):
        super().__init__(model, params)
        self.normals = FLAT.copy() if normals is None else np.asarray(normals, float).reshape(NL, 3).copy()

    def compute_non_sliding_constraints(self):
        mu = self.params["friction"]
        Dfr = np.zeros((4 * NL, 3 * NL))
        for l in range(NL):
            Dfr[4 * l:4 * l + 4, 3 * l:3 * l + 3] = faces(self.normals[l], mu) * self.foot_contacts[l]
        return Dfr


def sloped_reduced_problem(c):
    """wbc_reduced.reduced_problem(c) with the friction rows (ids < 16) of CI on c.normals' frames."""
    rp = WR.reduced_problem(c)
    if rp is None:
        return None
    mu = c.params["friction"]
    for k, pid in enumerate(rp["ids"]):
        if pid < 16:
            l, rr = divmod(pid, 4)
            row = np.zeros(12)
            row[3 * l:3 * l + 3] = -faces(c.normals[l], mu)[rr]
            rp["CI"][k] = row
    return rp


def reduced_step(c):
    """wbc_reduced.reduced_step on the edited problem: (tau, x42, status, iters), or None (no reduction).
    Rows are selected as the engine and the C oracle's REDUCED form select them, by slack over the norm
    of the reference's row (the problem's `nsel`) with the reference row's tolerance, so `iters` counts
    the same working-set walk as theirs."""
    c.update_state()
    c.assemble_qp()
    rp = sloped_reduced_problem(c)
    if rp is None:
        return None
    if not rp["vac_ok"]:
        return np.zeros(NJ), np.zeros(NV), W.QP_INFEASIBLE, 0
    tm, bbj = c.params["max_torque"], c.bbar[6:]
    tolv = [1e-10 if pid < 16 else 1e-10 * max(1.0, abs(-tm - (-1.0 if pid & 1 else 1.0) * bbj[(pid - 16) // 2])) for pid in rp["ids"]]
    z, stt, it, _ = W.gi_solve(rp["H"], rp["g"], np.zeros((0, 12)), np.zeros(0), rp["CI"], rp["ci"], c.params["max_wsr"],
                               selnorm=np.sqrt(np.maximum(rp["nsel"], 1e-300)), tolv=tolv)
    if stt != W.QP_OK:
        return np.zeros(NJ), np.zeros(NV), stt, it
    x, tau = WR.to_x42(c, rp, z)
    return tau, x, stt, it


def controller(inp, b, nrm=None, params=None, model=None, cls=SlopedWBC):
    """A fresh controller loaded with robot b of `inp` (cold: from setInitialState, explicit switching)."""
    c = cls(model, params) if cls is W.ReferenceWBC else cls(model, params, nrm)
    load(c, inp, b)
    return c


def load(c, inp, b):
    c.set_state(inp["base_pose"][b], inp["nu"][b], inp["qj"][b])
    c.set_reference(inp["ref"][b], [(int(inp["contacts"][b]) >> i) & 1 for i in range(NL)], bool(inp["switching"][b]))


def run_batch(inp, nrm, params_rows=None, model=None):
    """Cold batch under the literal QP: robot b on normals nrm[b] ([B, 4, 3]) and, when given, the
    parameter dict params_rows[b].  tau, grf, x, status, iters as the engine's outputs."""
    B = len(inp["contacts"])
    model = model or W.Model()
    out = dict(tau=np.zeros((B, NJ)), grf=np.zeros((B, NJ)), x=np.zeros((B, NV)), status=np.zeros(B, int),
               iters=np.zeros(B, int))
    for b in range(B):
        c = controller(inp, b, nrm[b], params_rows[b] if params_rows is not None else None, model)
        out["tau"][b], out["grf"][b], out["x"][b], out["status"][b], out["iters"][b] = c.step()
    return out
