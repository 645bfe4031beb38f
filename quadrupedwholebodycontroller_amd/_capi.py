"""ctypes binding of the C-ABI in include/wbc.h (libwbc_hip.so, built in-tree).

There is no CPU fallback: if the HIP library is missing or no GPU is present, loading or
creating an engine raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WBC_LIB", os.path.join(HERE, "libwbc_hip.so"))

NUM_JOINTS, NV, NC = 12, 42, 70
POSE_LEN, NU_LEN, REF_LEN = 7, 18, 54
STATELESS, DEBUG, NO_X, SPLIT, TIMED, COLD, FUSED, GROUP, RESIDENT = 1, 2, 4, 8, 16, 32, 64, 128, 256
# wbc_step_modes only: each hypothesis' QP objective; the best feasible hypothesis per state (implies OBJECTIVE)
OBJECTIVE, BEST = 512, 1024
# wbc_step only (default form): each robot's QP multipliers of the friction faces and torque limits
DUALS = 2048
DUAL_LEN = 40  # WBC_DUAL_LEN: rows 4 leg + face, then 16 + 2 joint + side (side 0: tau >= -max, side 1: tau <= +max)
# wbc_step only (default form), implies DUALS: the 40 and the multipliers of the per-foot normal-force bounds
DUALS_FORCE = 4096
# wbc_step only (default form), implies DUALS_FORCE: the same 48 under a per-robot force task (with or without one in force)
DUALS_TASK = 8192
DUAL_FORCE_LEN = 48  # WBC_DUAL_FORCE_LEN: the 40 rows, then 40 + 2 leg + side (side 0: n.f >= fn_min, side 1: n.f <= fn_max)
QP_OK, QP_MAX_ITER, QP_INFEASIBLE, QP_NUMERIC = 0, 1, 2, 3
# columns of the per-robot parameter table (WBC_RP_* in include/wbc.h; rows of RP_LEN doubles, the last reserved)
ROBOT_PARAM_NAMES = ("friction", "max_torque", "kp", "kp_z", "kd", "ki", "kp_swing", "kd_swing", "slack_weight")
RP_LEN = 10
# the per-robot contact-normal table (WBC_CN_LEN in include/wbc.h): three doubles per foot, legs LH, LF, RF, RH
CN_LEN = 12
FOOT_NAMES = ("LH", "LF", "RF", "RH")
# the per-robot base-body table (WBC_BB_* in include/wbc.h): mass, com[3] (base frame), inertia[9] (about
# the CoM, base axes, row-major), one reserved
BB_LEN = 14
BB_MASS, BB_COM, BB_INERTIA = 0, 1, 4
BASE_BODY_NAMES = ("mass", "com", "inertia")
BB_COLUMN_NAMES = ("mass", "com_x", "com_y", "com_z", "I_xx", "I_xy", "I_xz", "I_yx", "I_yy", "I_yz", "I_zx", "I_zy", "I_zz")
# the per-robot limits table (WBC_LM_* in include/wbc.h): tau_min[12], tau_max[12] (joint order of tau), mu per
# foot (LH, LF, RF, RH)
LM_LEN = 28
LM_TAU_MIN, LM_TAU_MAX, LM_FRICTION = 0, 12, 24
LIMIT_NAMES = ("tau_min", "tau_max", "friction")
# the per-foot normal-force bound table (WBC_FN_* in include/wbc.h): fn_min[4], fn_max[4] (LH, LF, RF, RH), N;
# -inf / +inf: no bound
FN_LEN = 8
FN_MIN, FN_MAX = 0, 4
FORCE_BOUND_NAMES = ("fn_min", "fn_max")
# the per-robot force-task table (WBC_FT_* in include/wbc.h): fref[12] (LH, LF, RF, RH; world frame, N), the
# robot's weight > 0, one reserved column
FT_LEN = 14
FT_FREF, FT_WEIGHT = 0, 12
FORCE_TASK_NAMES = ("f_ref", "weight")

# the per-robot tables of the default step: name -> row length; the C entry points of table <name> are
# wbc_set_<name>, wbc_bind_device_<name> and wbc_get_<name>
TABLES = {"robot_params": RP_LEN, "contact_normals": CN_LEN, "base_body": BB_LEN, "limits": LM_LEN, "force_bounds": FN_LEN,
          "force_task": FT_LEN}
TABLE_SYMBOLS = [f"wbc_{verb}_{name}" for name in TABLES for verb in ("set", "bind_device", "get")]
# the objective and best-mode outputs of wbc_step_modes (WBC_OBJECTIVE / WBC_BEST)
MODE_OUT_SYMBOLS = ["wbc_get_objective", "wbc_device_objective", "wbc_get_best_modes", "wbc_device_best_modes"]
# the multipliers of wbc_step (WBC_DUALS)
DUAL_SYMBOLS = ["wbc_get_duals", "wbc_device_duals"]
# and with the force rows' (WBC_DUALS_FORCE)
FORCE_DUAL_SYMBOLS = ["wbc_get_force_duals", "wbc_device_force_duals"]

# WBC_DBG_* offsets (include/wbc.h)
DBG = dict(COM=0, COMVEL=3, POSE=6, VC=12, M=18, CNU=342, JFEET=360, PFEET=576, VFEET=588, MBARB=600, MBARJ=636,
           JBAR=780, BBAR=996, WRENCH=1014, R1=1020, RSW=1032, STAMPS=1044, LEN=1052)

# every entry point declared in include/wbc.h
C_API_SYMBOLS = [
    "wbc_default_params", "wbc_anymal_model", "wbc_create", "wbc_destroy", "wbc_batch", "wbc_set_stream",
    "wbc_set_state", "wbc_set_reference", "wbc_bind_device_inputs", "wbc_bind_device_outputs", "wbc_reset", "wbc_update", "wbc_solve",
    "wbc_step", "wbc_set_modes", "wbc_step_modes", "wbc_modes_per_wave", "wbc_cycle", "wbc_synchronize", "wbc_get_output", "wbc_device_outputs", "wbc_get_debug", "wbc_last_kernel_ms",
    "wbc_last_error", "wbc_model_from_urdf", *TABLE_SYMBOLS, *MODE_OUT_SYMBOLS, *DUAL_SYMBOLS,
    *FORCE_DUAL_SYMBOLS,
]


class WbcLink(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("p", C.c_double * 3), ("axis", C.c_double * 3), ("mass", C.c_double),
                ("com", C.c_double * 3), ("inertia", C.c_double * 9)]


class WbcModel(C.Structure):
    _fields_ = [("base_mass", C.c_double), ("base_com", C.c_double * 3), ("base_inertia", C.c_double * 9),
                ("link", (WbcLink * 3) * 4), ("foot", (C.c_double * 3) * 4), ("total_mass", C.c_double)]


class WbcParams(C.Structure):
    _fields_ = [("friction", C.c_double), ("loop_rate", C.c_double), ("max_torque", C.c_double),
                ("kp", C.c_double), ("kp_z", C.c_double), ("kd", C.c_double), ("ki", C.c_double),
                ("kp_swing", C.c_double), ("kd_swing", C.c_double), ("slack_weight", C.c_double),
                ("initial_reference_pose", C.c_double * 6), ("gravity", C.c_double), ("max_wsr", C.c_int32),
                ("reserved", C.c_int32)]


_lib = None


def load_library(path: str = LIB_PATH):
    """Load libwbc_hip.so (raises OSError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OSError(f"HIP engine library not built: {path} (run __graft_entry__.build())")
    # One HIP runtime per process: torch bundles its own libamdhip64 (soname libamdhip64.so.7,
    # requested as "libamdhip64.so").  Loaded first, it satisfies our DT_NEEDED
    # libamdhip64.so.7 and both share it; loaded after us, it would be mapped a second time and
    # torch's device init fails ("No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    P, I32, U32 = C.c_void_p, C.c_int32, C.c_uint32
    dp = C.POINTER(C.c_double)
    sig = {
        "wbc_default_params": ([C.POINTER(WbcParams)], I32),
        "wbc_anymal_model": ([C.POINTER(WbcModel)], I32),
        "wbc_create": ([C.POINTER(WbcModel), C.POINTER(WbcParams), I32, I32, C.POINTER(P)], I32),
        "wbc_destroy": ([P], I32),
        "wbc_batch": ([P], I32),
        "wbc_set_stream": ([P, P], I32),
        "wbc_set_state": ([P, P, P, P], I32),
        "wbc_set_reference": ([P, P, P, P], I32),
        "wbc_bind_device_inputs": ([P, P, P, P, P, P, P], I32),
        "wbc_bind_device_outputs": ([P, P, P, P, P, P], I32),
        "wbc_reset": ([P, P], I32),
        "wbc_update": ([P, U32], I32),
        "wbc_solve": ([P, U32], I32),
        "wbc_step": ([P, U32], I32),
        "wbc_set_modes": ([P, I32, P], I32),
        "wbc_cycle": ([P, P, P, P, P, P, P, U32, P, P, P, P, P], I32),
        "wbc_step_modes": ([P, U32], I32),
        "wbc_modes_per_wave": ([P, C.POINTER(C.c_int32)], I32),
        "wbc_synchronize": ([P], I32),
        "wbc_get_output": ([P, P, P, P, P, P], I32),
        "wbc_device_outputs": ([P, C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P)], I32),
        "wbc_get_debug": ([P, P], I32),
        "wbc_last_kernel_ms": ([P, dp], I32),
        "wbc_last_error": ([], C.c_char_p),
        "wbc_model_from_urdf": ([C.c_char_p, P, P, C.c_char_p, C.POINTER(WbcModel)], I32),
        **{name: ([P, P], I32) for name in TABLE_SYMBOLS},
        "wbc_get_objective": ([P, P], I32),
        "wbc_device_objective": ([P, C.POINTER(P)], I32),
        "wbc_get_best_modes": ([P, P, P, P, P], I32),
        "wbc_device_best_modes": ([P, C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P)], I32),
        "wbc_get_duals": ([P, P], I32),
        "wbc_device_duals": ([P, C.POINTER(P)], I32),
        "wbc_get_force_duals": ([P, P], I32),
        "wbc_device_force_duals": ([P, C.POINTER(P)], I32),
    }
    for name, (argt, rest) in sig.items():
        if name in ("wbc_modes_per_wave", *TABLE_SYMBOLS, *MODE_OUT_SYMBOLS, *DUAL_SYMBOLS, *FORCE_DUAL_SYMBOLS) and not hasattr(lib, name):
            continue  # earlier builds loaded through WBC_LIB (A/B variants, tools/build_rev.sh) lack these
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = rest
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_params() -> WbcParams:
    p = WbcParams()
    load_library().wbc_default_params(C.byref(p))
    return p


def model_from_urdf(path: str, legs=None, joints=None, foot_suffix=None) -> WbcModel:
    """wbc_model_from_urdf: lumped 12-DoF quadruped model from a URDF file (raises WbcError)."""
    lib = load_library()

    def names(v):
        if v is None:
            return None
        arr = (C.c_char_p * len(v))(*[x.encode() for x in v])
        return C.cast(arr, C.c_void_p), arr

    m = WbcModel()
    lg, jn = names(legs), names(joints)
    rc = lib.wbc_model_from_urdf(path.encode(), lg[0] if lg else None, jn[0] if jn else None,
                                 foot_suffix.encode() if foot_suffix else None, C.byref(m))
    if rc != 0:
        raise WbcError(f"wbc_model_from_urdf failed ({rc}): {lib.wbc_last_error().decode()}")
    return m


def anymal_model() -> WbcModel:
    m = WbcModel()
    load_library().wbc_anymal_model(C.byref(m))
    return m


class WbcError(RuntimeError):
    pass


def robot_param_table(batch: int, params: WbcParams, table) -> np.ndarray:
    """The [B, RP_LEN] table of wbc_set_robot_params from an [B, 10] or [B, 9] array, or from a dict of
    column name (ROBOT_PARAM_NAMES) -> scalar or length-B array, whose missing columns take the
    engine-wide value of `params`.  The reserved column is 0."""
    B = int(batch)
    out = np.zeros((B, RP_LEN))
    if isinstance(table, dict):
        unknown = sorted(set(table) - set(ROBOT_PARAM_NAMES))
        if unknown:
            raise ValueError(f"unknown robot parameter columns {unknown}; columns are {ROBOT_PARAM_NAMES}")
        for c, name in enumerate(ROBOT_PARAM_NAMES):
            v = np.asarray(table[name], np.float64) if name in table else np.float64(getattr(params, name))
            if v.ndim not in (0, 1) or (v.ndim == 1 and v.shape[0] != B):
                raise ValueError(f"robot parameter {name}: need a scalar or {B} values, got shape {v.shape}")
            out[:, c] = v
        return out
    t = np.asarray(table, np.float64)
    if t.ndim != 2 or t.shape[0] != B or t.shape[1] not in (RP_LEN - 1, RP_LEN):
        raise ValueError(f"robot parameter table: need shape ({B}, {RP_LEN}) or ({B}, {RP_LEN - 1}), got {t.shape}")
    out[:, :RP_LEN - 1] = t[:, :RP_LEN - 1]
    return out


def contact_normal_table(batch: int, normals) -> np.ndarray:
    """The [B, CN_LEN] table of wbc_set_contact_normals from a (B, 12) or (B, 4, 3) array (row b: the
    ground normal at each foot of robot b, world frame, legs LH, LF, RF, RH), or from one (3,) normal or
    one (4, 3) set of four, broadcast to all robots.  Validated as the engine validates it (finite,
    0.25 <= |m|^2 <= 4, m_z / |m| >= 0.5); ValueError names the row and the foot."""
    B = int(batch)
    t = np.asarray(normals, np.float64)
    if t.shape == (3,):
        t = np.broadcast_to(t, (B, 4, 3))
    elif t.shape == (4, 3):
        t = np.broadcast_to(t, (B, 4, 3))
    elif t.shape == (B, CN_LEN):
        t = t.reshape(B, 4, 3)
    elif t.shape != (B, 4, 3):
        raise ValueError(f"contact normals: need shape ({B}, {CN_LEN}), ({B}, 4, 3), (4, 3) or (3,), got {t.shape}")
    s = (t * t).sum(axis=2)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(t).all(axis=2) & (s >= 0.25) & (s <= 4.0) & (t[:, :, 2] > 0.0) & (4.0 * t[:, :, 2] ** 2 >= s)
    if not ok.all():
        b, l = (int(v) for v in np.argwhere(~ok)[0])
        raise ValueError(f"contact normals: row {b}, foot {l} ({FOOT_NAMES[l]}) = {tuple(t[b, l])}: need finite entries, "
                         "0.25 <= |m|^2 <= 4 and m_z / |m| >= 0.5")
    return np.ascontiguousarray(t.reshape(B, CN_LEN))


def base_body_row(model: WbcModel) -> np.ndarray:
    """The model's own base body as a (BB_LEN,) row: what wbc_get_base_body returns without a table."""
    row = np.zeros(BB_LEN)
    row[BB_MASS] = model.base_mass
    row[BB_COM:BB_COM + 3] = list(model.base_com)
    row[BB_INERTIA:BB_INERTIA + 9] = list(model.base_inertia)
    return row


def base_body_bad_entry(row) -> int:
    """The validity rule of one base-body row (wbc_layout.h bb_bad_entry): -1, or the first failing column."""
    r = np.asarray(row, np.float64)
    for c in range(BB_LEN - 1):
        if not np.isfinite(r[c]):
            return c
    if not r[BB_MASS] > 0.0:
        return BB_MASS
    I = r[BB_INERTIA:BB_INERTIA + 9]
    tol = 1e-9 * abs(I[0] + I[4] + I[8])
    for lo, hi in ((1, 3), (2, 6), (5, 7)):
        if not abs(I[lo] - I[hi]) <= tol:
            return BB_INERTIA + lo
    a, d, f = I[0], I[4], I[8]
    b, c, e = 0.5 * (I[1] + I[3]), 0.5 * (I[2] + I[6]), 0.5 * (I[5] + I[7])
    if not a > 0.0:
        return BB_INERTIA
    if not a * d - b * b > 0.0:
        return BB_INERTIA + 4
    if not a * (d * f - e * e) - b * (b * f - e * c) + c * (b * e - d * c) > 0.0:
        return BB_INERTIA + 8
    return -1


def base_body_table(batch: int, model: WbcModel, table) -> np.ndarray:
    """The [B, BB_LEN] table of wbc_set_base_body from a (B, 14) array, one (14,) row broadcast to all
    robots, or a dict of BASE_BODY_NAMES -> one value or per-robot values (mass: scalar or (B,); com: (3,)
    or (B, 3); inertia: (3, 3), (9,), (B, 3, 3) or (B, 9)), whose missing entries take the model's base.
    Validated as the engine validates it (finite, mass > 0, inertia symmetric to 1e-9 of its trace and
    positive definite); ValueError names the row and the column.  The reserved column is 0."""
    B = int(batch)
    out = np.tile(base_body_row(model), (B, 1))
    if isinstance(table, dict):
        unknown = sorted(set(table) - set(BASE_BODY_NAMES))
        if unknown:
            raise ValueError(f"unknown base body entries {unknown}; entries are {BASE_BODY_NAMES}")
        if "mass" in table:
            v = np.asarray(table["mass"], np.float64)
            if v.shape not in ((), (B,)):
                raise ValueError(f"base body mass: need a scalar or {B} values, got shape {v.shape}")
            out[:, BB_MASS] = v
        if "com" in table:
            v = np.asarray(table["com"], np.float64)
            if v.shape not in ((3,), (B, 3)):
                raise ValueError(f"base body com: need shape (3,) or ({B}, 3), got {v.shape}")
            out[:, BB_COM:BB_COM + 3] = v
        if "inertia" in table:
            v = np.asarray(table["inertia"], np.float64)
            if v.shape not in ((3, 3), (9,), (B, 3, 3), (B, 9)):
                raise ValueError(f"base body inertia: need shape (3, 3), (9,), ({B}, 3, 3) or ({B}, 9), got {v.shape}")
            out[:, BB_INERTIA:BB_INERTIA + 9] = v.reshape(-1, 9)
    else:
        t = np.asarray(table, np.float64)
        if t.shape not in ((BB_LEN,), (B, BB_LEN)):
            raise ValueError(f"base body table: need shape ({B}, {BB_LEN}) or ({BB_LEN},), got {t.shape}")
        out[:, :] = t
    out[:, BB_LEN - 1] = 0.0
    for b in range(B):
        c = base_body_bad_entry(out[b])
        if c >= 0:
            raise ValueError(f"base body: row {b}, column {c} ({BB_COLUMN_NAMES[c]}) = {out[b, c]:g}: need finite entries, "
                             "mass > 0 and a symmetric (to 1e-9 of its trace), positive definite inertia")
    return out


def base_body_with_payload(model: WbcModel, mass, position, inertia=None) -> np.ndarray:
    """Base-body rows for a payload rigidly fixed to the trunk: a body of `mass` (scalar or (N,)) with its
    CoM at `position` ((3,) or (N, 3), base frame) and inertia `inertia` about its own CoM in base axes
    ((3, 3) or (N, 3, 3); None: a point mass).  The composite with the model's base, by the parallel-axis
    theorem about the composite CoM:
        M = m0 + mp,   c = c0 + (mp / M) (p - c0),   I = I0 + Ip + (m0 mp / M) (|d|^2 1 - d d^T),  d = p - c0.
    Returns (N, BB_LEN), or (BB_LEN,) for one payload; zero mass gives the model's own row bit for bit."""
    mp = np.asarray(mass, np.float64)
    p = np.asarray(position, np.float64)
    single = mp.ndim == 0 and p.ndim == 1 and (inertia is None or np.ndim(inertia) == 2)
    N = max([1] + [v.shape[0] for v, nd in ((mp, 1), (p, 2)) if v.ndim == nd]
            + ([np.shape(inertia)[0]] if inertia is not None and np.ndim(inertia) == 3 else []))
    mp = np.broadcast_to(mp, (N,))
    p = np.broadcast_to(p, (N, 3))
    Ip = np.zeros((N, 3, 3)) if inertia is None else np.broadcast_to(np.asarray(inertia, np.float64), (N, 3, 3))
    base = base_body_row(model)
    m0, c0, I0 = base[BB_MASS], base[BB_COM:BB_COM + 3], base[BB_INERTIA:BB_INERTIA + 9].reshape(3, 3)
    M = m0 + mp
    d = p - c0
    mu = m0 * mp / M
    pa = (d * d).sum(axis=1)[:, None, None] * np.eye(3) - d[:, :, None] * d[:, None, :]
    out = np.zeros((N, BB_LEN))
    out[:, BB_MASS] = M
    out[:, BB_COM:BB_COM + 3] = c0 + (mp / M)[:, None] * d
    out[:, BB_INERTIA:BB_INERTIA + 9] = (I0 + Ip + mu[:, None, None] * pa).reshape(N, 9)
    return out[0] if single else out


def limits_row(tau_min, tau_max, friction) -> np.ndarray:
    """One (LM_LEN,) row of the limits table: tau_min and tau_max a scalar or (12,) (joint order of tau),
    friction a scalar or (4,) (feet LH, LF, RF, RH).  limits_row(-T, T, mu) is the row of a robot with
    max_torque T and friction mu."""
    row = np.empty(LM_LEN)
    for name, v, at, n in (("tau_min", tau_min, LM_TAU_MIN, NUM_JOINTS), ("tau_max", tau_max, LM_TAU_MAX, NUM_JOINTS),
                           ("friction", friction, LM_FRICTION, 4)):
        v = np.asarray(v, np.float64)
        if v.shape not in ((), (n,)):
            raise ValueError(f"limits {name}: need a scalar or shape ({n},), got {v.shape}")
        row[at:at + n] = v
    return row


def limits_bad_column(row) -> int:
    """The validity rule of one limits row (wbc_layout.h lm_bad_column): -1, or the first failing column."""
    r = np.asarray(row, np.float64)
    for c in range(LM_LEN):
        if not np.isfinite(r[c]):
            return c
        if LM_TAU_MAX <= c < LM_FRICTION and not r[c - LM_TAU_MAX + LM_TAU_MIN] <= r[c]:
            return c
        if c >= LM_FRICTION and r[c] < 0.0:
            return c
    return -1


def limits_table(batch: int, defaults, table) -> np.ndarray:
    """The [B, LM_LEN] table of wbc_set_limits from a (B, 28) array, one (28,) row broadcast to all robots,
    or a dict of LIMIT_NAMES -> a scalar, one (12,) / (4,) vector, a (B,) value per robot or a (B, 12) /
    (B, 4) array, whose missing entries take the rows of `defaults` ((B, 28): Engine.limits()).  Validated
    as the engine validates it (finite, tau_min <= tau_max per joint, friction >= 0); ValueError names the
    row and the column."""
    B = int(batch)
    out = np.array(np.broadcast_to(np.asarray(defaults, np.float64), (B, LM_LEN)))
    if isinstance(table, dict):
        unknown = sorted(set(table) - set(LIMIT_NAMES))
        if unknown:
            raise ValueError(f"unknown limits entries {unknown}; entries are {LIMIT_NAMES}")
        for name, at, n in (("tau_min", LM_TAU_MIN, NUM_JOINTS), ("tau_max", LM_TAU_MAX, NUM_JOINTS), ("friction", LM_FRICTION, 4)):
            if name not in table:
                continue
            v = np.asarray(table[name], np.float64)
            if v.shape == (B,) and B != n:
                v = v[:, None]
            elif v.shape not in ((), (n,), (B, n)):
                raise ValueError(f"limits {name}: need a scalar, shape ({n},), ({B},) or ({B}, {n}), got {v.shape}")
            out[:, at:at + n] = v
    else:
        t = np.asarray(table, np.float64)
        if t.shape not in ((LM_LEN,), (B, LM_LEN)):
            raise ValueError(f"limits table: need shape ({B}, {LM_LEN}) or ({LM_LEN},), got {t.shape}")
        out[:, :] = t
    for b in range(B):
        c = limits_bad_column(out[b])
        if c >= 0:
            name, k = (("tau_min", c) if c < LM_TAU_MAX else ("tau_max", c - LM_TAU_MAX) if c < LM_FRICTION
                       else ("friction", c - LM_FRICTION))
            raise ValueError(f"limits: row {b}, column {c} ({name}[{k}]) = {out[b, c]:g}: need finite entries, "
                             "tau_min <= tau_max per joint, friction >= 0")
    return np.ascontiguousarray(out)


def force_bounds_row(fn_min=-np.inf, fn_max=np.inf) -> np.ndarray:
    """One (FN_LEN,) row of the force-bound table: fn_min and fn_max a scalar or (4,) (feet LH, LF, RF, RH), in
    newtons along each foot's contact normal; -inf / +inf (the defaults) mean no bound."""
    row = np.empty(FN_LEN)
    for name, v, at in (("fn_min", fn_min, FN_MIN), ("fn_max", fn_max, FN_MAX)):
        v = np.asarray(v, np.float64)
        if v.shape not in ((), (4,)):
            raise ValueError(f"force bounds {name}: need a scalar or shape (4,), got {v.shape}")
        row[at:at + 4] = v
    return row


def force_bounds_bad_column(row) -> int:
    """The validity rule of one force-bound row (wbc_layout.h fn_bad_column): -1, or the first failing column:
    NaN or +inf in fn_min, NaN or -inf in fn_max, fn_min > fn_max (at fn_max's column)."""
    r = np.asarray(row, np.float64)
    for c in range(FN_LEN):
        if c < FN_MAX and not r[c] < np.inf:
            return c
        if c >= FN_MAX and (not r[c] > -np.inf or not r[c - FN_MAX + FN_MIN] <= r[c]):
            return c
    return -1


def force_bounds_table(batch: int, defaults, table) -> np.ndarray:
    """The [B, FN_LEN] table of wbc_set_force_bounds from a (B, 8) array, one (8,) row broadcast to all robots,
    or a dict of FORCE_BOUND_NAMES -> a scalar, one (4,) vector, a (B,) value per robot or a (B, 4) array, whose
    missing entries take the rows of `defaults` ((B, 8): Engine.force_bounds()).  The engine validates it."""
    B = int(batch)
    out = np.array(np.broadcast_to(np.asarray(defaults, np.float64), (B, FN_LEN)))
    if isinstance(table, dict):
        unknown = sorted(set(table) - set(FORCE_BOUND_NAMES))
        if unknown:
            raise ValueError(f"unknown force bound entries {unknown}; entries are {FORCE_BOUND_NAMES}")
        for name, at in (("fn_min", FN_MIN), ("fn_max", FN_MAX)):
            if name not in table:
                continue
            v = np.asarray(table[name], np.float64)
            if v.shape == (B,) and B != 4:
                v = v[:, None]
            elif v.shape not in ((), (4,), (B, 4)):
                raise ValueError(f"force bounds {name}: need a scalar, shape (4,), ({B},) or ({B}, 4), got {v.shape}")
            out[:, at:at + 4] = v
    else:
        t = np.asarray(table, np.float64)
        if t.shape not in ((FN_LEN,), (B, FN_LEN)):
            raise ValueError(f"force bounds table: need shape ({B}, {FN_LEN}) or ({FN_LEN},), got {t.shape}")
        out[:, :] = t
    return np.ascontiguousarray(out)


def force_task_row(f_ref=0.0, weight=1.0) -> np.ndarray:
    """One (FT_LEN,) row of the force-task table: f_ref a scalar, (12,) or (4, 3) (feet LH, LF, RF, RH; world frame,
    newtons), weight > 0; the defaults are the plain regulariser's row (0 x 12, 1, 0)."""
    row = np.zeros(FT_LEN)
    f = np.asarray(f_ref, np.float64)
    if f.shape not in ((), (12,), (4, 3)):
        raise ValueError(f"force task f_ref: need a scalar or shape (12,) or (4, 3), got {f.shape}")
    row[FT_FREF:FT_WEIGHT] = f.reshape(-1) if f.shape else f
    w = np.asarray(weight, np.float64)
    if w.shape != ():
        raise ValueError(f"force task weight: need a scalar, got shape {w.shape}")
    row[FT_WEIGHT] = w
    return row


def force_task_bad_column(row) -> int:
    """The validity rule of one force-task row (wbc_layout.h ft_bad_column): -1, or the first failing column: a
    non-finite entry of f_ref or of the weight, weight <= 0.  The reserved column is not read."""
    r = np.asarray(row, np.float64)
    for c in range(FT_WEIGHT):
        if not np.isfinite(r[FT_FREF + c]):
            return FT_FREF + c
    return FT_WEIGHT if not (np.isfinite(r[FT_WEIGHT]) and r[FT_WEIGHT] > 0.0) else -1


def force_task_table(batch: int, defaults, table) -> np.ndarray:
    """The [B, FT_LEN] table of wbc_set_force_task from a (B, 14) array, one (14,) row broadcast to all robots, or a
    dict of FORCE_TASK_NAMES -> f_ref: a scalar, one (12,) or (4, 3) vector, a (B, 12) or (B, 4, 3) array; weight: a
    scalar or a (B,) value per robot; missing entries take the rows of `defaults` ((B, 14): Engine.force_task()).
    The engine validates it."""
    B = int(batch)
    out = np.array(np.broadcast_to(np.asarray(defaults, np.float64), (B, FT_LEN)))
    if isinstance(table, dict):
        unknown = sorted(set(table) - set(FORCE_TASK_NAMES))
        if unknown:
            raise ValueError(f"unknown force task entries {unknown}; entries are {FORCE_TASK_NAMES}")
        if "f_ref" in table:
            v = np.asarray(table["f_ref"], np.float64)
            if v.shape not in ((), (12,), (4, 3), (B, 12), (B, 4, 3)):
                raise ValueError(f"force task f_ref: need a scalar, shape (12,), (4, 3), ({B}, 12) or ({B}, 4, 3), got {v.shape}")
            out[:, FT_FREF:FT_WEIGHT] = v.reshape(B, 12) if v.shape in ((B, 12), (B, 4, 3)) else (v.reshape(-1) if v.shape else v)
        if "weight" in table:
            v = np.asarray(table["weight"], np.float64)
            if v.shape not in ((), (B,)):
                raise ValueError(f"force task weight: need a scalar or shape ({B},), got {v.shape}")
            out[:, FT_WEIGHT] = v
    else:
        t = np.asarray(table, np.float64)
        if t.shape not in ((FT_LEN,), (B, FT_LEN)):
            raise ValueError(f"force task table: need shape ({B}, {FT_LEN}) or ({FT_LEN},), got {t.shape}")
        out[:, :] = t
    return np.ascontiguousarray(out)


class Engine:
    """A batch of B robots on one GPU (wraps wbc_engine*)."""

    def __init__(self, batch: int, device: int = 0, params: WbcParams | None = None, model: WbcModel | None = None):
        self.lib = load_library()
        self.batch = int(batch)
        self.n_modes = 0
        self._stream = None  # the bound caller stream object (kept alive while bound)
        self._bound_tables = {}  # table name -> the bound device table's owner (kept alive while bound)
        self.params = WbcParams.from_buffer_copy(params) if params else default_params()  # the engine-wide wbc_params
        self.model = WbcModel.from_buffer_copy(model) if model else anymal_model()  # the engine's model
        self.h = C.c_void_p()
        rc = self.lib.wbc_create(C.byref(model) if model else None, C.byref(params) if params else None,
                                 self.batch, int(device), C.byref(self.h))
        self._check(rc, "wbc_create")

    def _check(self, rc, what):
        if rc != 0:
            raise WbcError(f"{what} failed ({rc}): {self.lib.wbc_last_error().decode()}")

    def close(self):
        if self.h:
            self.lib.wbc_destroy(self.h)  # synchronizes the bound stream, which is still alive here
            self.h = C.c_void_p()
        self._stream = None
        self._bound_tables = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- inputs -------------------------------------------------------------------------
    @property
    def input_rows(self) -> int:
        """Rows of the input arrays: B robots, or B / K states under K mode hypotheses."""
        return self.batch // self.n_modes if self.n_modes else self.batch

    def set_state(self, base_pose=None, nu=None, qj=None):
        B = self.input_rows
        arrs = [None if v is None else np.ascontiguousarray(v, np.float64).reshape(B, n)
                for v, n in ((base_pose, POSE_LEN), (nu, NU_LEN), (qj, NUM_JOINTS))]
        self._check(self.lib.wbc_set_state(self.h, *[_ptr(a) for a in arrs]), "wbc_set_state")

    def set_reference(self, ref=None, contacts=None, switching=None):
        B = self.input_rows
        r = None if ref is None else np.ascontiguousarray(ref, np.float64).reshape(B, REF_LEN)
        c = None if contacts is None else np.ascontiguousarray(contacts, np.uint8).reshape(B)
        s = None if switching is None else np.ascontiguousarray(switching, np.uint8).reshape(B)
        self._check(self.lib.wbc_set_reference(self.h, _ptr(r), _ptr(c), _ptr(s)), "wbc_set_reference")

    def bind_device_inputs(self, base_pose=0, nu=0, qj=0, ref=0, contacts=0, switching=0):
        """Integer device pointers (e.g. torch tensor .data_ptr()); 0 = engine-owned buffer."""
        v = [C.c_void_p(int(x)) if x else None for x in (base_pose, nu, qj, ref, contacts, switching)]
        self._check(self.lib.wbc_bind_device_inputs(self.h, *v), "wbc_bind_device_inputs")

    def bind_device_outputs(self, tau=0, grf=0, x=0, status=0, iters=0):
        """Integer device pointers of caller-owned output buffers; 0 = engine-owned buffer."""
        v = [C.c_void_p(int(p)) if p else None for p in (tau, grf, x, status, iters)]
        self._check(self.lib.wbc_bind_device_outputs(self.h, *v), "wbc_bind_device_outputs")

    # the per-robot tables (TABLES): set from the host, bind a device table, read back
    def _set_table(self, name, t):
        self._check(getattr(self.lib, f"wbc_set_{name}")(self.h, _ptr(t)), f"wbc_set_{name}")

    def _bind_table(self, name, table):
        ptr = int(table.data_ptr()) if hasattr(table, "data_ptr") else int(table or 0)
        self._check(getattr(self.lib, f"wbc_bind_device_{name}")(self.h, C.c_void_p(ptr) if ptr else None),
                    f"wbc_bind_device_{name}")
        self._bound_tables[name] = table if ptr else None

    def _get_table(self, name) -> np.ndarray:
        out = np.zeros((self.batch, TABLES[name]))
        self._check(getattr(self.lib, f"wbc_get_{name}")(self.h, _ptr(out)), f"wbc_get_{name}")
        return out

    def set_robot_params(self, table):
        """wbc_set_robot_params: per-robot friction, max_torque, gains and slack_weight for the default
        step.  `table`: an [B, 10] or [B, 9] array (columns ROBOT_PARAM_NAMES), or a dict of column name
        to scalar or length-B array (missing columns: the engine's wbc_params); None clears the table."""
        self._set_table("robot_params", None if table is None else
                        np.ascontiguousarray(robot_param_table(self.batch, self.params, table)))

    def bind_device_robot_params(self, table=0):
        """wbc_bind_device_robot_params: a caller-owned device table [B, 10] of doubles (no copy, no host
        validation): an integer device pointer, or an object with data_ptr() (a torch tensor), which the
        engine keeps referenced while it is bound.  0 / None: the engine-owned table, or none."""
        self._bind_table("robot_params", table)

    def robot_params(self) -> np.ndarray:
        """wbc_get_robot_params: the [B, 10] table in force (without one: the engine-wide values in B rows)."""
        return self._get_table("robot_params")

    def set_contact_normals(self, normals):
        """wbc_set_contact_normals: the ground normal at each foot of each robot (sloped ground) for the
        default step.  `normals`: a (B, 12) or (B, 4, 3) array, or one (3,) normal / one (4, 3) set
        broadcast to all robots (contact_normal_table); None clears the table: flat ground."""
        self._set_table("contact_normals", None if normals is None else contact_normal_table(self.batch, normals))

    def bind_device_contact_normals(self, table=0):
        """wbc_bind_device_contact_normals: a caller-owned device table [B, 12] of doubles (no copy, no
        host validation): an integer device pointer, or an object with data_ptr() (a torch tensor), which
        the engine keeps referenced while it is bound.  0 / None: the engine-owned table, or none."""
        self._bind_table("contact_normals", table)

    def contact_normals(self) -> np.ndarray:
        """wbc_get_contact_normals: the [B, 12] table in force (without one: (0, 0, 1) for every foot)."""
        return self._get_table("contact_normals")

    def set_base_body(self, table):
        """wbc_set_base_body: per-robot base body (mass, CoM, inertia: a payload on the trunk) for the
        default step.  `table`: a (B, 14) array, one (14,) row, or a dict {mass, com, inertia} of one
        value or per-robot arrays (base_body_table; rows for a payload: base_body_with_payload); None
        clears the table: the model's base."""
        self._set_table("base_body", None if table is None else base_body_table(self.batch, self.model, table))

    def bind_device_base_body(self, table=0):
        """wbc_bind_device_base_body: a caller-owned device table [B, 14] of doubles (no copy, no host
        validation): an integer device pointer, or an object with data_ptr() (a torch tensor), which the
        engine keeps referenced while it is bound.  0 / None: the engine-owned table, or none."""
        self._bind_table("base_body", table)

    def base_body(self) -> np.ndarray:
        """wbc_get_base_body: the [B, 14] table in force (without one: the model's base in every row)."""
        return self._get_table("base_body")

    def set_limits(self, table):
        """wbc_set_limits: per-robot joint torque bounds [tau_min, tau_max] and per-foot friction for the
        default step.  `table`: a (B, 28) array, one (28,) row (limits_row), or a dict {tau_min, tau_max,
        friction} of scalars, (12,) / (4,) vectors or per-robot arrays (limits_table), whose missing entries
        keep what limits() returns now; None clears the table: max_torque and friction again."""
        self._set_table("limits", None if table is None else
                        limits_table(self.batch, self.limits() if isinstance(table, dict) else 0.0, table))

    def bind_device_limits(self, table=0):
        """wbc_bind_device_limits: a caller-owned device table [B, 28] of doubles (no copy, no host
        validation; it may be rewritten on the engine's stream every cycle): an integer device pointer, or
        an object with data_ptr() (a torch tensor), which the engine keeps referenced while it is bound.
        0 / None: the engine-owned table, or none."""
        self._bind_table("limits", table)

    def limits(self) -> np.ndarray:
        """wbc_get_limits: the [B, 28] table in force (without one: -max_torque x 12, +max_torque x 12 and
        friction x 4 per robot, from its parameter row or the engine-wide params)."""
        return self._get_table("limits")

    def set_force_bounds(self, table):
        """wbc_set_force_bounds: per-foot bounds fn_min <= n . f <= fn_max on the normal contact force of
        every stance foot, for the default step (contact load ramps).  `table`: a (B, 8) array, one (8,) row
        (force_bounds_row), or a dict {fn_min, fn_max} of scalars, (4,) vectors or per-robot arrays
        (force_bounds_table), whose missing entries keep what force_bounds() returns now; -inf / +inf mean
        no bound.  Validation is the engine's (WbcError names the row and column).  None clears the table."""
        self._set_table("force_bounds", None if table is None else
                        force_bounds_table(self.batch, self.force_bounds() if isinstance(table, dict) else 0.0, table))

    def bind_device_force_bounds(self, table=0):
        """wbc_bind_device_force_bounds: a caller-owned device table [B, 8] of doubles (no copy, no host
        validation; it may be rewritten on the engine's stream every cycle, as a load ramp is): an integer
        device pointer, or an object with data_ptr() (a torch tensor), which the engine keeps referenced while
        it is bound.  0 / None: the engine-owned table, or none."""
        self._bind_table("force_bounds", table)

    def force_bounds(self) -> np.ndarray:
        """wbc_get_force_bounds: the [B, 8] table in force (without one: -inf x 4, +inf x 4 per robot)."""
        return self._get_table("force_bounds")

    def set_force_task(self, table):
        """wbc_set_force_task: per-robot reference contact forces for the default step: the regulariser of every
        stance foot becomes weight / 2 |f - f_ref|^2 (a planner's forces, tracked softly; world frame, newtons).
        `table`: a (B, 14) array, one (14,) row (force_task_row), or a dict {f_ref, weight} of scalars, (12,) /
        (4, 3) vectors or per-robot arrays (force_task_table), whose missing entries keep what force_task()
        returns now.  Validation is the engine's (WbcError names the row and column).  None clears the table."""
        self._set_table("force_task", None if table is None else
                        force_task_table(self.batch, self.force_task() if isinstance(table, dict) else 0.0, table))

    def bind_device_force_task(self, table=0):
        """wbc_bind_device_force_task: a caller-owned device table [B, 14] of doubles (no copy, no host
        validation; it may be rewritten on the engine's stream every cycle, as a planner's forces are): an
        integer device pointer, or an object with data_ptr() (a torch tensor), which the engine keeps referenced
        while it is bound.  0 / None: the engine-owned table, or none."""
        self._bind_table("force_task", table)

    def force_task(self) -> np.ndarray:
        """wbc_get_force_task: the [B, 14] table in force, its reserved column 0 (without one: 0 x 12, 1, 0 per
        robot)."""
        return self._get_table("force_task")

    def set_stream(self, stream):
        """Bind a caller stream: a torch.cuda.Stream (or any object with `cuda_stream`), which the engine
        keeps referenced until it is unbound (set_stream(0 / None)) or closed, so the stream outlives
        its binding (include/wbc.h wbc_set_stream); or a raw hipStream_t as an int, which the caller
        must keep alive that long.  0 / None: the engine's own stream."""
        ptr = int(getattr(stream, "cuda_stream", stream) or 0)
        self._check(self.lib.wbc_set_stream(self.h, C.c_void_p(ptr) if ptr else None), "wbc_set_stream")
        self._stream = stream if ptr else None

    # --- execution ----------------------------------------------------------------------
    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.batch)
        self._check(self.lib.wbc_reset(self.h, _ptr(m)), "wbc_reset")

    def update(self, flags: int = 0):
        self._check(self.lib.wbc_update(self.h, flags), "wbc_update")

    def solve(self, flags: int = 0):
        self._check(self.lib.wbc_solve(self.h, flags), "wbc_solve")

    def step(self, flags: int = 0):
        self._check(self.lib.wbc_step(self.h, flags), "wbc_step")

    def cycle(self, base_pose, nu, qj, ref, contacts, switching, flags: int = 0, want_x: bool = True):
        """wbc_cycle: one synchronous host-to-host control cycle (one H2D copy, the step, one D2H copy)."""
        B = self.batch
        f = lambda v, n: np.ascontiguousarray(v, np.float64).reshape(B, n)
        ins = [f(base_pose, POSE_LEN), f(nu, NU_LEN), f(qj, NUM_JOINTS), f(ref, REF_LEN),
               np.ascontiguousarray(contacts, np.uint8).reshape(B), np.ascontiguousarray(switching, np.uint8).reshape(B)]
        tau = np.zeros((B, NUM_JOINTS)); grf = np.zeros((B, NUM_JOINTS)); x = np.zeros((B, NV)) if want_x else None
        st = np.zeros(B, np.int32); it = np.zeros(B, np.int32)
        self._check(self.lib.wbc_cycle(self.h, *[_ptr(a) for a in ins], flags, _ptr(tau), _ptr(grf), _ptr(x), _ptr(st),
                                       _ptr(it)), "wbc_cycle")
        return dict(tau=tau, grf=grf, x=x, status=st, iters=it)

    def set_modes(self, modes=None):
        """wbc_set_modes: solve every state under each contact mask in `modes` (None / [] clears)."""
        m = None if modes is None or len(modes) == 0 else np.ascontiguousarray(modes, np.uint8).ravel()
        n = 0 if m is None else m.size
        self._check(self.lib.wbc_set_modes(self.h, n, _ptr(m)), "wbc_set_modes")
        self.n_modes = n

    def step_modes(self, flags: int = 1):
        """wbc_step_modes: one cold step of every (state, mode) hypothesis (flags need STATELESS)."""
        self._check(self.lib.wbc_step_modes(self.h, flags), "wbc_step_modes")

    def modes_per_wave(self) -> int:
        """wbc_modes_per_wave: hypotheses per wave of wbc_step_modes (1: one per segment; M > 1: the
        mode loop, wbc_modes_kernel); 0 without modes."""
        m = C.c_int32(0)
        self._check(self.lib.wbc_modes_per_wave(self.h, C.byref(m)), "wbc_modes_per_wave")
        return int(m.value)

    def synchronize(self):
        self._check(self.lib.wbc_synchronize(self.h), "wbc_synchronize")

    def last_kernel_ms(self) -> float:
        ms = C.c_double()
        self._check(self.lib.wbc_last_kernel_ms(self.h, C.byref(ms)), "wbc_last_kernel_ms")
        return ms.value

    # --- outputs ------------------------------------------------------------------------
    def outputs(self):
        B = self.batch
        tau = np.zeros((B, NUM_JOINTS)); grf = np.zeros((B, NUM_JOINTS)); x = np.zeros((B, NV))
        st = np.zeros(B, np.int32); it = np.zeros(B, np.int32)
        self._check(self.lib.wbc_get_output(self.h, _ptr(tau), _ptr(grf), _ptr(x), _ptr(st), _ptr(it)),
                    "wbc_get_output")
        return dict(tau=tau, grf=grf, x=x, status=st, iters=it)

    def device_outputs(self):
        ptrs = [C.c_void_p() for _ in range(5)]
        self._check(self.lib.wbc_device_outputs(self.h, *[C.byref(p) for p in ptrs]), "wbc_device_outputs")
        return dict(zip(("tau", "grf", "x", "status", "iters"), (p.value for p in ptrs)))

    def duals(self) -> np.ndarray:
        """wbc_get_duals: (B, 40) multipliers of the friction faces (rows 4 leg + face) and torque limits
        (rows 16 + 2 joint + side) after step(... | DUALS); 0 for a row that does not bind, all 0 where
        status is not QP_OK.  dual_rows() reshapes them."""
        d = np.zeros((self.batch, DUAL_LEN))
        self._check(self.lib.wbc_get_duals(self.h, _ptr(d)), "wbc_get_duals")
        return d

    def device_duals(self) -> int:
        """wbc_device_duals: the device address of the (B, 40) multipliers."""
        p = C.c_void_p()
        self._check(self.lib.wbc_device_duals(self.h, C.byref(p)), "wbc_device_duals")
        return p.value

    def force_duals(self) -> np.ndarray:
        """wbc_get_force_duals: (B, 48) multipliers after step(... | DUALS_FORCE) or step(... | DUALS_TASK) (the
        flag under a force task: the multipliers of the QP with the task's H and g, which grow with its weight
        w, numbered alike): the 40 of duals(), then the
        per-foot normal-force bounds' (rows 40 + 2 leg + side: side 0 n.f >= fn_min, side 1 n.f <= fn_max); 0 for
        a row that does not exist or does not bind, all 0 where status is not QP_OK.  dual_rows() reshapes them."""
        d = np.zeros((self.batch, DUAL_FORCE_LEN))
        self._check(self.lib.wbc_get_force_duals(self.h, _ptr(d)), "wbc_get_force_duals")
        return d

    def device_force_duals(self) -> int:
        """wbc_device_force_duals: the device address of the (B, 48) multipliers."""
        p = C.c_void_p()
        self._check(self.lib.wbc_device_force_duals(self.h, C.byref(p)), "wbc_device_force_duals")
        return p.value

    def objective(self) -> np.ndarray:
        """wbc_get_objective: (B,) QP objective of each hypothesis after step_modes(... | OBJECTIVE), row
        s * K + k as the other outputs; +inf where status is not QP_OK."""
        obj = np.zeros(self.batch)
        self._check(self.lib.wbc_get_objective(self.h, _ptr(obj)), "wbc_get_objective")
        return obj

    def device_objective(self) -> int:
        """wbc_device_objective: the device address of the (B,) objectives."""
        p = C.c_void_p()
        self._check(self.lib.wbc_device_objective(self.h, C.byref(p)), "wbc_device_objective")
        return p.value

    def best_modes(self):
        """wbc_get_best_modes after step_modes(... | BEST): per state the index into the modes of its best
        feasible hypothesis (-1: none), that hypothesis' objective (+inf: none), tau and grf."""
        S = self.input_rows
        best = np.zeros(S, np.int32); obj = np.zeros(S); tau = np.zeros((S, NUM_JOINTS)); grf = np.zeros((S, NUM_JOINTS))
        self._check(self.lib.wbc_get_best_modes(self.h, _ptr(best), _ptr(obj), _ptr(tau), _ptr(grf)), "wbc_get_best_modes")
        return dict(best=best, objective=obj, tau=tau, grf=grf)

    def device_best_modes(self):
        """wbc_device_best_modes: the device addresses of best (int32 [S]), objective [S], tau and grf [S, 12]."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.lib.wbc_device_best_modes(self.h, *[C.byref(p) for p in ptrs]), "wbc_device_best_modes")
        return dict(zip(("best", "objective", "tau", "grf"), (p.value for p in ptrs)))

    def debug(self):
        out = np.zeros((self.batch, DBG["LEN"]))
        self._check(self.lib.wbc_get_debug(self.h, _ptr(out)), "wbc_get_debug")
        return out


def dual_rows(d):
    """The (B, 40) multipliers of Engine.duals() by constraint: {"friction": (B, 4, 4) >= 0, leg by face in
    the reference's order; "torque": (B, 12) signed, side 0 - side 1: positive where joint j sits at
    -max_torque, negative at +max_torque (qpOASES' sign of the two-sided row's multiplier)}.  The (B, 48)
    multipliers of Engine.force_duals() give a third item, "force": (B, 4) signed, side 0 - side 1: positive
    where foot l sits at fn_min, negative at fn_max."""
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] not in (DUAL_LEN, DUAL_FORCE_LEN):
        raise ValueError(f"duals: need shape (B, {DUAL_LEN}) or (B, {DUAL_FORCE_LEN}), got {d.shape}")
    t = d[:, 16:DUAL_LEN].reshape(-1, NUM_JOINTS, 2)
    rows = {"friction": d[:, :16].reshape(-1, 4, 4).copy(), "torque": t[:, :, 0] - t[:, :, 1]}
    if d.shape[1] == DUAL_FORCE_LEN:
        f = d[:, DUAL_LEN:].reshape(-1, 4, 2)
        rows["force"] = f[:, :, 0] - f[:, :, 1]
    return rows


def split_debug(rec):
    """Debug record (WBC_DBG_LEN,) -> dict of named arrays (same keys as oracle debug_record)."""
    D = DBG
    return dict(com=rec[D["COM"]:D["COM"] + 3], comvel=rec[D["COMVEL"]:D["COMVEL"] + 3],
                pose=rec[D["POSE"]:D["POSE"] + 6], vc=rec[D["VC"]:D["VC"] + 6],
                M=rec[D["M"]:D["M"] + 324].reshape(18, 18), Cnu=rec[D["CNU"]:D["CNU"] + 18],
                Jfeet=rec[D["JFEET"]:D["JFEET"] + 216].reshape(12, 18), pfeet=rec[D["PFEET"]:D["PFEET"] + 12],
                vfeet=rec[D["VFEET"]:D["VFEET"] + 12], Mbar_b=rec[D["MBARB"]:D["MBARB"] + 36].reshape(6, 6),
                Mbar_j=rec[D["MBARJ"]:D["MBARJ"] + 144].reshape(12, 12),
                Jbar=rec[D["JBAR"]:D["JBAR"] + 216].reshape(12, 18), bbar=rec[D["BBAR"]:D["BBAR"] + 18],
                W=rec[D["WRENCH"]:D["WRENCH"] + 6], r1=rec[D["R1"]:D["R1"] + 12], rsw=rec[D["RSW"]:D["RSW"] + 12])


# --- batched motion planner (include/wbc_planner.h) -----------------------------------------------
class WbcPlannerParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("step_length", "height_control_point", "x_offset", "y_offset",
                                          "step_duration", "body_height", "body_initial_velocity",
                                          "body_final_velocity", "dt")]


PLANNER_API_SYMBOLS = ["wbc_planner_default_params", "wbc_planner_create", "wbc_planner_destroy",
                       "wbc_planner_set_stream", "wbc_planner_set_command", "wbc_planner_reset", "wbc_planner_tick",
                       "wbc_planner_device_outputs", "wbc_planner_get_output"]


def _planner_lib():
    lib = load_library()
    if not getattr(lib, "_planner_sigs", False):
        P, I32 = C.c_void_p, C.c_int32
        PP = C.POINTER(P)
        sig = {
            "wbc_planner_default_params": ([C.POINTER(WbcPlannerParams)], I32),
            "wbc_planner_create": ([C.POINTER(WbcPlannerParams), I32, I32, C.POINTER(P)], I32),
            "wbc_planner_destroy": ([P], I32),
            "wbc_planner_set_stream": ([P, P], I32),
            "wbc_planner_set_command": ([P, P], I32),
            "wbc_planner_reset": ([P, P], I32),
            "wbc_planner_tick": ([P], I32),
            "wbc_planner_device_outputs": ([P, PP, PP, PP, PP], I32),
            "wbc_planner_get_output": ([P, P, P, P, P], I32),
        }
        for name, (argt, rest) in sig.items():
            fn = getattr(lib, name)
            fn.argtypes = argt
            fn.restype = rest
        lib._planner_sigs = True
    return lib


class Planner:
    """B motion planners on one GPU (wraps wbc_planner*): one tick = one plannerLoop rate.sleep()."""

    def __init__(self, batch: int, device: int = 0, params: WbcPlannerParams | None = None):
        self.lib = _planner_lib()
        self.batch = int(batch)
        self.h = C.c_void_p()
        rc = self.lib.wbc_planner_create(C.byref(params) if params else None, self.batch, int(device), C.byref(self.h))
        self._check(rc, "wbc_planner_create")

    def _check(self, rc, what):
        if rc != 0:
            raise WbcError(f"{what} failed ({rc}): {self.lib.wbc_last_error().decode()}")

    def close(self):
        if self.h:
            self.lib.wbc_planner_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int):
        self._check(self.lib.wbc_planner_set_stream(self.h, C.c_void_p(int(stream_ptr)) if stream_ptr else None),
                    "wbc_planner_set_stream")

    def set_command(self, cmd):
        c = np.ascontiguousarray(cmd, np.float64).reshape(self.batch, 3)
        self._check(self.lib.wbc_planner_set_command(self.h, _ptr(c)), "wbc_planner_set_command")

    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.batch)
        self._check(self.lib.wbc_planner_reset(self.h, _ptr(m)), "wbc_planner_reset")

    def tick(self):
        self._check(self.lib.wbc_planner_tick(self.h), "wbc_planner_tick")

    def device_outputs(self):
        p = [C.c_void_p() for _ in range(4)]
        self._check(self.lib.wbc_planner_device_outputs(self.h, *[C.byref(x) for x in p]), "wbc_planner_device_outputs")
        return dict(zip(("ref", "contacts", "switching", "published"), (x.value for x in p)))

    def outputs(self):
        B = self.batch
        ref = np.zeros((B, REF_LEN))
        con, sw, pub = (np.zeros(B, np.uint8) for _ in range(3))
        self._check(self.lib.wbc_planner_get_output(self.h, _ptr(ref), _ptr(con), _ptr(sw), _ptr(pub)),
                    "wbc_planner_get_output")
        return dict(ref=ref, contacts=con, switching=sw, published=pub)
