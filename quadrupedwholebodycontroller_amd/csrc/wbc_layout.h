// wbc_layout.h — device-side record layouts shared by the HIP kernel and the host engine.
#ifndef WBC_LAYOUT_H
#define WBC_LAYOUT_H

#include "wbc.h"

namespace wbc {

// Per-robot history that survives between control cycles (stateful mode).  Compact form of
// the reference's finite-difference state (hpp:154-161): T_old (top rows only vary:
// [Ad^-1(r_old), Mbar_b^-1 A_j]), Jbar_old (com part [I, -S(p_f - c)] from d_old, joint part),
// Tdot_inv (top 6 rows), integralError_, the contacts of Jbar_old, a valid flag
// (0 right after setInitialState: T_old = I, J_old = 0, Tdot_inv = 0, cpp:84-104), and the
// working set of the previous QP (qpOASES SQProblem::hotstart, cpp:531).
enum HistOff {
    H_ROLD = 0,     // r_old = c - p_B of the previous cycle (3)
    H_MAOLD = 3,    // Mbar_b^-1 A_j of the previous cycle, 6x12 row-major (72)
    H_DOLD = 75,    // p_f - c, previous cycle (12)
    H_JBJOLD = 87,  // joint part of Jbar_feet, previous cycle, 12x12 (144)
    H_TDINV = 231,  // Tdot_inv top 6 rows, 6x18 row-major (108)
    H_EINT = 339,   // integralError_ (6)
    H_KOLD = 345,   // contact bitmask of the previous cycle (as double)
    H_VALID = 346,  // 0 after reset
    H_WSLO = 347,   // active inequality set of the previous solve, lanes 0..31 (bitmask as double)
    H_WSHI = 348,   //   lanes 32..63
    H_WSKAP = 349,  // contact mask that active set belongs to (hotstart only for the same mask)
    HIST_LEN = 350
};

// Assembled per-robot problem: written by the update phase, read by the solve phase
// (the HBM workspace between wbc_update and wbc_solve; kept in LDS by the fused step).
struct Prob {
    double m, inv_m;
    double Ic[9];
    double Icinv[9];
    double d[12];     // foot position minus CoM, LH, LF, RF, RH
    double Jbj[144];  // joint columns of Jbar_feet = J_feet T^-1, [row 0..11][joint 0..11]
    double Mbj[144];  // centroidMassMatrixJoints_
    double bbj[12];   // centroidGeneralizedBias_(6:18)
    double r1[12];    // R1 bound: -Jc_dot_com v_c - Jc_dot_j qdot (cpp:504)
    double rsw[12];   // R4/R5 bound: cmd - Js_dot_com v_c - Js_dot_j qdot (cpp:507,515)
    double W[6];      // computeDesiredWrench (cpp:426-445)
    double kappa;     // contact bitmask
    double flags;     // 1: non-finite input / intermediate, 2: slot Hessian not positive definite
};
static_assert(sizeof(Prob) % 16 == 0, "Prob must keep 16-byte alignment");
constexpr int PROB_LEN = sizeof(Prob) / sizeof(double);

// Slot factorisation formed at the end of the update kernel (presolve in wbc_kernel.hip), stored
// after the problem in the work row and read by the solve kernel from HBM / L2.
//
// Four-contact stance (kappa = 15) is solved in a smaller space: the 12 stance equalities
// (R1, cpp:494,504) Jbar_c,j qdd + G f = e are solved for qdd = q0 - P f in the update kernel,
// which leaves a 12-variable QP in the contact forces with Hessian H_f = P^T P + H_s and gradient
// g_s - P^T q0, and only inequality rows (16 friction faces, 24 torque rows tau = t0 - Nt f).
// Then Mi / xs hold the factor of H_f and the unconstrained f0, and the stance fields below are
// filled (wbc_kernel.hip stance_reduce).
struct Presolve {
    double Mi[78];    // M = L^-1 of the slot Hessian H_s = L L^T (H_f for stance), lower triangle row-major
    double xs[12];    // slot part of the unconstrained optimum x0 = -H^-1 g (f0 for stance)
    double presolved; // 1: Mi / xs hold the slot factorisation for this kappa; 0: the solve forms it
    double stance;    // 1: the stance elimination below is valid (Mi / xs then belong to H_f)
    double q0[12];    // stance: qdd = q0 - P f
    double t0[12];    //         tau = t0 - Nt f  (t0 = bbar_j + Mbar_j q0)
    double nsel[12];  //         |row|^2 of torque row j in the reference's 42-variable space
    double Nt[144];   //         Nt = Mbar_j P + Jbar_c,j^T, [joint j][force c]
    double Y[72];     //         P = Y B^T (rank 6): qdd = q0 - Y [F / m; I_c^-1 sum d_l x f_l], [joint][6]
};
static_assert(sizeof(Presolve) % 16 == 0, "Presolve must keep 16-byte alignment");
constexpr int PRE_LEN = sizeof(Presolve) / sizeof(double);
constexpr int WORK_LEN = PROB_LEN + PRE_LEN;  // work row: [Prob | Presolve]

// The step kernel's LDS image of the model and the friction-normal table, built once on the host
// (wbc_create) and copied into LDS by each workgroup as one contiguous block: each link record is
// padded to 29 doubles (at the API's 28, 224 B, lanes j and j + 8 of a segment read the same LDS
// banks for every field of their links), and the table holds face rr's normal for leg l as the 12
// doubles from FRIC_ROW(4 l + rr) (four 21-double bands: zeros, the face's three entries, zeros).
struct LdsLink {
    double R[9], p[3], axis[3], mass, com[3], inertia[9], pad_;
};
static_assert(sizeof(LdsLink) == sizeof(wbc_link) + sizeof(double), "LdsLink mirrors wbc_link");
struct LdsModel {
    double base_mass, base_com[3], base_inertia[9];
    LdsLink link[WBC_NUM_LEGS][3];
    double foot[WBC_NUM_LEGS][3];
    double total_mass;
};
constexpr int FRIC_LEN = 4 * 21;
#define FRIC_ROW(p) (((p) & 3) * 21 + 9 - 3 * ((p) >> 2))
struct LdsImage {
    LdsModel model;
    double fric[FRIC_LEN];
};
constexpr int LIMG_LEN = sizeof(LdsImage) / sizeof(double);
inline void build_lds_image(const wbc_model& m, double friction, LdsImage& o) {
    o.model.base_mass = m.base_mass;
    for (int i = 0; i < 3; ++i) o.model.base_com[i] = m.base_com[i];
    for (int i = 0; i < 9; ++i) o.model.base_inertia[i] = m.base_inertia[i];
    for (int l = 0; l < WBC_NUM_LEGS; ++l)
        for (int k = 0; k < 3; ++k) {
            const wbc_link& s = m.link[l][k];
            LdsLink& d = o.model.link[l][k];
            for (int i = 0; i < 9; ++i) { d.R[i] = s.R[i]; d.inertia[i] = s.inertia[i]; }
            for (int i = 0; i < 3; ++i) { d.p[i] = s.p[i]; d.axis[i] = s.axis[i]; d.com[i] = s.com[i]; }
            d.mass = s.mass;
            d.pad_ = 0.0;
        }
    for (int l = 0; l < WBC_NUM_LEGS; ++l)
        for (int i = 0; i < 3; ++i) o.model.foot[l][i] = m.foot[l][i];
    o.model.total_mass = m.total_mass;
    // face rr of a friction pyramid: [-1, 0, mu], [1, 0, mu], [0, -1, mu], [0, 1, mu] (force space)
    for (int e = 0; e < FRIC_LEN; ++e) {
        const int rr = e / 21, k = e % 21 - 9;
        const double fv = (k == 0) ? ((rr == 0) ? -1.0 : (rr == 1 ? 1.0 : 0.0))
                        : (k == 1) ? ((rr == 2) ? -1.0 : (rr == 3 ? 1.0 : 0.0)) : friction;
        o.fric[e] = (k >= 0 && k < 3) ? fv : 0.0;
    }
}

// The resident control cycle's mailbox (wbc_cycle with WBC_RESIDENT; pinned, coherent host memory):
// the host raises cmd (a sequence number, or WBC_RESIDENT_STOP), the resident wave answers with
// done = cmd once the cycle's outputs are visible, and sets exited = 1 when it ends (on
// WBC_RESIDENT_STOP or after its idle limit), so the host can tell a wave that ended by itself from
// one that is late.  cmd and the wave's words sit on separate 64-byte lines.
constexpr unsigned long long WBC_RESIDENT_STOP = ~0ull;
struct ResidentBox {
    unsigned long long cmd;
    unsigned long long pad0[7];
    unsigned long long done;
    unsigned long long exited;
    unsigned long long pad1[6];
};

// Kernel arguments (one struct, passed by value).
struct KernelArgs {
    const wbc_model* model;
    const wbc_params* params;
    const double* limg;  // LdsImage (model in the LDS layout + friction table), LIMG_LEN doubles
    const double* base_pose;
    const double* nu;
    const double* qj;
    const double* ref;
    const uint8_t* contacts;
    const uint8_t* switching;
    double* hist;       // [B][HIST_LEN]
    double* work;       // [B][WORK_LEN] (split update/solve): Prob, Presolve
    double* tau;
    double* grf;
    double* x;
    int32_t* status;
    int32_t* iters;
    double* dbg;        // [B][WBC_DBG_LEN]
    int32_t batch;
    int32_t stateful;   // read / write history
    int32_t debug;      // write debug records
    int32_t cold;       // stateful, but no QP hotstart (WBC_COLD)
    int32_t modes;      // contact-mode hypotheses per state (wbc_step_modes); 0 = one QP per input row
    const uint8_t* mode_masks;  // [modes]: contact mask of hypothesis k
    // Four-contact stance elimination (Presolve::stance) for this step's mask-15 QPs: the engine
    // turns it on when every QP of the step has mask 15 (then the stance solve kernel runs
    // instead of the general one).  QPs whose elimination did not happen (a near-singular leg)
    // are listed for the fallback solve: fb[parity] counts them, fb[2 ..] lists them (at most
    // fb_cap entries); the update kernel clears fb[parity ^ 1] for the next elimination update.
    // (The default step, wbc_update_solve_kernel, solves its fallbacks in place and uses neither.)
    int32_t elim;
    int32_t parity;
    int32_t* fb;
    int32_t fb_cap;
    // The default step's wave map (wbc_update_solve_kernel): entry e = qmap[4 w + seg] of segment
    // seg of workgroup w is (qp << 4 | mask) for a QP it solves (e >= 0), ~(qp << 4 | mask) for a
    // padding segment that recomputes QP qp without writing anything, QMAP_EMPTY when the whole
    // workgroup has nothing to do.  The mask travels in the entry, so the step reads one word before
    // the QP's inputs (not the word and then contacts[qp]).  The engine groups the QPs by contact
    // mask (qmap_build below, or wbc_qmap_kernel for device-bound masks), so the four segments of a
    // wave share one mask.  nullptr: QP 4 w + seg (every mask in the step is equal).
    // Under mode hypotheses the map is arithmetic (workgroup g K + k: states 4 g .. 4 g + 3 under
    // mask modes[k]) and qmap is unused.  nwaves: the step kernel's grid.
    const int32_t* qmap;
    int32_t nwaves;
    // Mode hypotheses with the state's update shared (wbc_modes_kernel): each wave holds four
    // states and a chunk of mloop hypotheses, solved one after another after one update; chunk c
    // runs hypotheses mode_order[c mloop .. c mloop + mloop - 1].  mloop = 0: one hypothesis per
    // segment (wbc_update_solve_kernel's arithmetic map).
    int32_t mloop;
    uint8_t mode_order[16];
    // the parameters by value: read from the kernel-argument segment (scalar loads of memory the
    // compiler knows is constant), not through `params`, whose global loads it must repeat after
    // every global store and wait for in turn
    wbc_params pv;
    // Per-robot parameters (wbc_set_robot_params / wbc_bind_device_robot_params): [batch][WBC_RP_LEN],
    // row qp for QP qp; read only by the per-robot instances of the default step (wbc_kernel_rps.hip,
    // wbc_kernel_rp0.hip, wbc_kernel_rp1.hip), which take the nine values of their QP's row in place
    // of pv's.  Last, so that no other argument's offset moves.
    const double* rp;
    // Per-robot ground normals at the feet (wbc_set_contact_normals / wbc_bind_device_contact_normals):
    // [batch][WBC_CN_LEN], row qp for QP qp; read only by the contact-normal instances of the default
    // step (wbc_kernel_cn0.hip, wbc_kernel_cn1.hip), which are per-robot-parameter instances too: the
    // engine points rp at a uniform table of its own when only normals are in force.  After rp, so
    // that no other argument's offset moves.
    const double* cn;
    // Per-robot base body (wbc_set_base_body / wbc_bind_device_base_body): [batch][WBC_BB_LEN], row qp
    // for QP qp (mass, CoM, inertia about the CoM; bb_bad_entry below); read only by the base-body
    // instances of the default step (wbc_kernel_bb0.hip, wbc_kernel_bb1.hip, wbc_kernel_bbs.hip), which
    // are contact-normal instances too: the engine points cn at a flat table of its own (and rp at its
    // uniform one) when no such table is in force.  After cn, so that no other argument's offset moves.
    const double* bb;
    // The QP objective at the optimum per hypothesis (wbc_step_modes with WBC_OBJECTIVE / WBC_BEST):
    // [batch], row qp for QP qp, +infinity where status is not WBC_QP_OK; written only by the mode loop's
    // objective instance (wbc_kernel_modes_obj.hip) and its fallback solve.  After bb, so that no other
    // argument's offset moves.
    double* obj;
    // The multipliers of the friction and torque rows (wbc_step with WBC_DUALS): [batch][WBC_DUAL_LEN],
    // row qp for QP qp, in the hotstart's row numbering (wbc.h), zero where status is not WBC_QP_OK;
    // written only by the duals instances of the default step (wbc_kernel_du0.hip, wbc_kernel_du1.hip)
    // and their fallback solve.  For the force-bound duals instances (wbc_kernel_fnd0.hip, wbc_kernel_fnd1.hip:
    // wbc_step with WBC_DUALS_FORCE; and wbc_kernel_ftd0.hip, wbc_kernel_ftd1.hip: WBC_DUALS_TASK)
    // the same member points at a buffer of [batch][WBC_DUAL_FORCE_LEN]:
    // the stride is a compile-time constant of the instance.  After obj, so that no other argument's offset moves.  (Keep the trailing
    // comment on the declaration's own line: tests/test_modes_objective_cpu.py scans for lines ending in ';'
    // and expects obj to be the last of them)
    double* dual;       // [B][WBC_DUAL_LEN]
    // Per-robot joint torque bounds and per-foot friction (wbc_set_limits / wbc_bind_device_limits):
    // [batch][WBC_LM_LEN], row qp for QP qp (tau_min[12], tau_max[12], mu[4]; lm_bad_column below); read
    // only by the limits instances of the default step (wbc_kernel_lm0.hip, wbc_kernel_lm1.hip), which
    // are base-body, contact-normal and per-robot-parameter instances too: the engine points bb, cn and
    // rp at tables of its own where none is in force.  Last, so that no other argument's offset moves.
    // (Keep the block comment behind the declaration: tests/test_duals_cpu.py cuts lines at the line-comment
    // mark and expects dual to be the last that then ends in ';'.)
    const double* lm; /* [B][WBC_LM_LEN] */
    // Per-foot normal-force bounds (wbc_set_force_bounds / wbc_bind_device_force_bounds): [batch][WBC_FN_LEN],
    // row qp for QP qp (fn_min[4], fn_max[4]; fn_bad_column below); read only by the force-bound instances
    // of the default step (wbc_kernel_fn0.hip, wbc_kernel_fn1.hip), which are limits, base-body,
    // contact-normal and per-robot-parameter instances too: the engine points bb, cn and rp at tables of
    // its own where none is in force, and a null lm leaves each robot's own -+max_torque and friction in
    // the limits' place.  Last, so that no other argument's offset moves.  (The block comment stays behind
    // the declaration, as lm's.)
    const double* fn; /* [B][WBC_FN_LEN] */
    // Per-robot reference contact forces and their weight (wbc_set_force_task / wbc_bind_device_force_task):
    // [batch][WBC_FT_LEN], row qp for QP qp (fref[12], weight, one reserved; ft_bad_column below); read only by
    // the force-task instances of the default step (wbc_kernel_ft0.hip, wbc_kernel_ft1.hip, and their duals
    // instances wbc_kernel_ftd0.hip, wbc_kernel_ftd1.hip), which are instances
    // of every other table too: the engine points fn, bb, cn and rp at tables of its own where none is in force,
    // and a null lm is taken as the force-bound instances take it.  Last, so that no other argument's offset
    // moves.  (The block comment stays behind the declaration, as lm's.)
    const double* ft; /* [B][WBC_FT_LEN] */
};

// ---------------------------------------------------------------------------------------
// Wave map of the default step: QPs grouped by contact mask, four to a wave (KernelArgs::qmap)
// ---------------------------------------------------------------------------------------
constexpr int32_t QMAP_EMPTY = (int32_t)0x80000000;
constexpr int QMAP_MAX_BATCH = (1 << 27) - 1;  // qp << 4 fits 31 bits
#ifdef __HIPCC__
#define WBC_HD __host__ __device__
#else
#define WBC_HD
#endif
// A per-robot parameter row (wbc.h WBC_RP_*) the step accepts: -1, or the first column that fails
// (a non-finite entry in columns 0-8, friction < 0, max_torque < 0, slack_weight <= 0).  One
// definition for the host's validation (wbc_set_robot_params) and the kernels' (a device-bound row).
WBC_HD inline int rp_bad_column(const double* r) {
    for (int c = 0; c < WBC_RP_LEN - 1; ++c) {
        const bool neg = (c == WBC_RP_FRICTION || c == WBC_RP_MAX_TORQUE) ? r[c] < 0.0
                       : (c == WBC_RP_SLACK_WEIGHT)                       ? r[c] <= 0.0 : false;
        if (!__builtin_isfinite(r[c]) || neg) return c;
    }
    return -1;
}
// The arguments an instance wbc_update_solve_kernel<STF, SONLY, RP, CN> of the default step refuses
// (its unit's launcher, wbc_kernel.hip): a step without waves; a stateful step for a stateless
// instance or the reverse; mode hypotheses or a wave map for a stance-only instance (every QP mask
// 15, in batch order); mode hypotheses or no table for a per-robot-parameter instance; no normals
// for a contact-normal instance.
// BB (the base-body instances, a fifth template argument, false for the nine units above): no base-body
// table.  LM (the limits instances, a sixth, false for every earlier unit): no limits table.  The other
// forms take the flags in the template's order (a unit's WBC_STEP_INSTANCE).
// FN (the force-bound instances, a seventh, false for every earlier unit): no force-bound table; such an
// instance takes a null limits table (each robot's own -+max_torque and friction stand).
// FT (the force-task instances, an eighth, false for every earlier unit): no force-task table; such an
// instance is a force-bound instance too (the engine's own no-bounds table where none is in force).
inline bool step_args_refused(int STF, bool SONLY, bool RP, bool CN, const KernelArgs& a, bool BB = false, bool LM = false,
                              bool FN = false, bool FT = false) {
    if (a.nwaves <= 0 || (a.stateful != 0) != (STF != 0)) return true;
    if (SONLY && (a.modes || a.qmap)) return true;
    if (RP && (a.modes || !a.rp)) return true;
    if (CN && !a.cn) return true;
    if (BB && !a.bb) return true;
    if (FT && !a.ft) return true;
    if (FN) return !a.fn;
    return LM && !a.lm;
}
inline bool step_args_refused(int STF, bool SONLY, bool RP, bool CN, bool BB, const KernelArgs& a) {
    return step_args_refused(STF, SONLY, RP, CN, a, BB);
}
inline bool step_args_refused(int STF, bool SONLY, bool RP, bool CN, bool BB, bool LM, const KernelArgs& a) {
    return step_args_refused(STF, SONLY, RP, CN, a, BB, LM);
}
inline bool step_args_refused(int STF, bool SONLY, bool RP, bool CN, bool BB, bool LM, bool FN, const KernelArgs& a) {
    return step_args_refused(STF, SONLY, RP, CN, a, BB, LM, FN);
}
inline bool step_args_refused(int STF, bool SONLY, bool RP, bool CN, bool BB, bool LM, bool FN, bool FT, const KernelArgs& a) {
    return step_args_refused(STF, SONLY, RP, CN, a, BB, LM, FN, FT);
}
// The default step's instances, one kernel unit each (wbc_kernel_<unit>.hip): per table in force
// (none, parameters, parameters + normals; parameters + normals + base bodies in the second list
// below) the stateless instance of any mask mix, the stateful one, the stance-only one.  The one list names the instances (STEP_<unit>) and, in the engine, orders the
// launcher table that StepInstance indexes (wbc_engine.cpp kStepLaunchers).  step_instance: the one
// a step takes.  Normals come with a parameter table (the caller's or the engine's uniform one), so
// cn wins over rp; all_stance (wbc_engine.cpp step_all_stance: stateless, every mask 15, no map, no
// hypotheses) never comes with stateful.
#define WBC_STEP_UNITS(X) X(step0) X(step1) X(stance) X(rp0) X(rp1) X(rps) X(cn0) X(cn1) X(cns)
enum StepInstance {
#define X(unit) STEP_##unit,
    WBC_STEP_UNITS(X)
#undef X
    STEP_INSTANCES
};
// The base-body instances (KernelArgs::bb), in a list of their own whose values go on
// from STEP_INSTANCES: the launcher table has STEP_ALL_INSTANCES entries, built from both lists
// (DESIGN.md 17 says why there are two).  A base-body table comes with normals and parameters (the
// caller's or the engine's), so bb wins over cn and rp.
#define WBC_STEP_UNITS_BB(X) X(bb0) X(bb1) X(bbs)
enum StepInstanceBB {
    STEP_BB_FIRST_ = STEP_INSTANCES - 1,
#define X(unit) STEP_##unit,
    WBC_STEP_UNITS_BB(X)
#undef X
    STEP_ALL_INSTANCES
};
// The limits instances (KernelArgs::lm), in a third list for the same reason, whose values
// go on from STEP_ALL_INSTANCES: the launcher table has STEP_EVERY_INSTANCE entries, built from the three
// lists in this order.  A limits table comes with the other three (the caller's or the engine's), so lm
// wins over bb, cn and rp; there is no stance-only unit: an all-stance step runs lm0, whose mask-15
// waves take the stance form.
#define WBC_STEP_UNITS_LM(X) X(lm0) X(lm1)
enum StepInstanceLM {
    STEP_LM_FIRST_ = STEP_ALL_INSTANCES - 1,
#define X(unit) STEP_##unit,
    WBC_STEP_UNITS_LM(X)
#undef X
    STEP_EVERY_INSTANCE
};
// The force-bound instances (KernelArgs::fn), in a fourth list whose values go on from
// STEP_EVERY_INSTANCE: the launcher table has STEP_LAUNCHER_COUNT entries, built from the four lists in
// this order.  fn wins over every other table; no stance-only unit, as the limits'.
#define WBC_STEP_UNITS_FN(X) X(fn0) X(fn1)
enum StepInstanceFN {
    STEP_FN_FIRST_ = STEP_EVERY_INSTANCE - 1,
#define X(unit) STEP_##unit,
    WBC_STEP_UNITS_FN(X)
#undef X
    STEP_LAUNCHER_COUNT
};
// The force-task instances (KernelArgs::ft), in a fifth list whose values go on from
// STEP_LAUNCHER_COUNT (which keeps its value): the launcher table has STEP_LAUNCHER_COUNT_FT entries, built
// from the five lists in this order.  ft wins over every other table; no stance-only unit: an all-stance
// step runs ft0, whose mask-15 waves take the stance form.
#define WBC_STEP_UNITS_FT(X) X(ft0) X(ft1)
enum StepInstanceFT {
    STEP_FT_FIRST_ = STEP_LAUNCHER_COUNT - 1,
#define X(unit) STEP_##unit,
    WBC_STEP_UNITS_FT(X)
#undef X
    STEP_LAUNCHER_COUNT_FT
};
constexpr int step_instance(bool cn, bool rp, bool all_stance, bool stateful, bool bb = false, bool lm = false, bool fn = false,
                            bool ft = false) {
    return ft ? (stateful ? (int)STEP_ft1 : (int)STEP_ft0)
         : fn ? (stateful ? (int)STEP_fn1 : (int)STEP_fn0)
         : lm ? (stateful ? (int)STEP_lm1 : (int)STEP_lm0)
         : bb ? (all_stance ? (int)STEP_bbs : stateful ? (int)STEP_bb1 : (int)STEP_bb0)
         : all_stance ? (cn ? STEP_cns : rp ? STEP_rps : STEP_stance)
         : stateful   ? (cn ? STEP_cn1 : rp ? STEP_rp1 : STEP_step1)
                      : (cn ? STEP_cn0 : rp ? STEP_rp0 : STEP_step0);
}

// The packed blocks of a control cycle (wbc_cycle; the engine's own device buffers have the same
// layout, so a host cycle is one copy each way): inputs [pose | nu | qj | ref | contacts | switching],
// outputs [tau | grf | status | iters | x].  The views give the arrays of a block for B robots at
// `base` (8-byte aligned); status + iters are 8 bytes per robot, so x stays 8-byte aligned, and x is
// last, so a cycle without it copies the block's head.
template <class D, class U>
struct InputViewT {
    D *pose, *nu, *qj, *ref;
    U *contacts, *switching;
};
using InputView = InputViewT<double, uint8_t>;
using ConstInputView = InputViewT<const double, const uint8_t>;
struct OutputView {
    double *tau, *grf;
    int32_t *status, *iters;
    double* x;
};
template <class D, class U, class V>
inline InputViewT<D, U> input_view_at(V* base, size_t B) {
    InputViewT<D, U> v;
    v.pose = static_cast<D*>(base);
    v.nu = v.pose + B * WBC_POSE_LEN;
    v.qj = v.nu + B * WBC_NU_LEN;
    v.ref = v.qj + B * WBC_NUM_JOINTS;
    v.contacts = reinterpret_cast<U*>(v.ref + B * WBC_REF_LEN);
    v.switching = v.contacts + B;
    return v;
}
inline InputView input_view(void* base, size_t B) { return input_view_at<double, uint8_t>(base, B); }
inline ConstInputView input_view(const void* base, size_t B) { return input_view_at<const double, const uint8_t>(base, B); }
inline ConstInputView const_view(const InputView& v) { return {v.pose, v.nu, v.qj, v.ref, v.contacts, v.switching}; }
inline OutputView output_view(void* base, size_t B) {
    OutputView v;
    v.tau = static_cast<double*>(base);
    v.grf = v.tau + B * WBC_NUM_JOINTS;
    v.status = reinterpret_cast<int32_t*>(v.grf + B * WBC_NUM_JOINTS);
    v.iters = v.status + B;
    v.x = reinterpret_cast<double*>(v.iters + B);
    return v;
}
inline size_t input_block_bytes(size_t B) {
    return B * (WBC_POSE_LEN + WBC_NU_LEN + WBC_NUM_JOINTS + WBC_REF_LEN) * sizeof(double) + 2 * B;
}
// (in whole 8-byte words, as the block is allocated: the resident cycle copies it by words)
inline size_t input_block_words(size_t B) { return (input_block_bytes(B) + 7) / 8; }
inline size_t output_block_bytes(size_t B, bool with_x = true) {
    return B * 2 * WBC_NUM_JOINTS * sizeof(double) + 2 * B * sizeof(int32_t) + (with_x ? B * WBC_NV * sizeof(double) : 0);
}

// The ground normal m of one foot (three doubles of a wbc.h WBC_CN_LEN row) the step accepts: finite,
// 0.25 <= |m|^2 <= 4, m_z / |m| >= 0.5.  One definition for the host's validation
// (wbc_set_contact_normals) and the kernels' (a device-bound row); cn_bad_foot: -1, or the first
// foot of the row that fails.
WBC_HD inline bool cn_valid(const double* m) {
    const double s = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
    return s >= 0.25 && s <= 4.0 && m[2] > 0.0 && 4.0 * m[2] * m[2] >= s;  // (a NaN entry fails s >= 0.25)
}
WBC_HD inline int cn_bad_foot(const double* row) {
    for (int l = 0; l < WBC_NUM_LEGS; ++l)
        if (!cn_valid(row + 3 * l)) return l;
    return -1;
}
// The friction frame of a valid normal m: n = m / |m|, t1 = e_x less its part along n, normalised,
// t2 = n x t1.  Square root and divisions are the correctly rounded ones (no fast reciprocal), so
// that m = (0, 0, c) gives exactly (1, 0, 0), (0, 1, 0), (0, 0, 1) and the flat-ground rows.
WBC_HD inline void cn_frame(const double* m, double* n, double* t1, double* t2) {
    const double r = __builtin_sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    for (int k = 0; k < 3; ++k) n[k] = m[k] / r;
    const double u[3] = {1.0 - n[0] * n[0], 0.0 - n[0] * n[1], 0.0 - n[0] * n[2]};
    const double iq = 1.0 / __builtin_sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int k = 0; k < 3; ++k) t1[k] = u[k] * iq;
    t2[0] = n[1] * t1[2] - n[2] * t1[1];
    t2[1] = n[2] * t1[0] - n[0] * t1[2];
    t2[2] = n[0] * t1[1] - n[1] * t1[0];
}
// Entry r of face rr's row for a foot with frame (n, t1, t2) and friction mu, in the engine's sign
// (row . f >= 0): mu n -+ t1 (rr = 0, 1), mu n -+ t2 (rr = 2, 3); flat ground: (-+1, 0, mu), (0, -+1, mu)
WBC_HD inline double cn_face_elem(const double* n, const double* t1, const double* t2, double mu, int rr, int r) {
    const double t = (rr < 2) ? t1[r] : t2[r];
    return __builtin_fma(mu, n[r], (rr & 1) ? t : -t);
}
// A base-body row (wbc.h WBC_BB_*: mass, com[3], inertia[9] about the CoM in base axes, one reserved)
// the step accepts: -1, or the first column that fails: every entry of columns 0-12 finite, mass > 0,
// |I_ij - I_ji| <= 1e-9 trace (reported at the upper entry), the symmetric part positive definite
// (leading minors > 0, reported at I_00, I_11, I_22).  The reserved column is not read.  One
// definition for the host's validation (wbc_set_base_body) and the kernels' (a device-bound row).
WBC_HD inline int bb_bad_entry(const double* r) {
    for (int c = 0; c < WBC_BB_LEN - 1; ++c)
        if (!__builtin_isfinite(r[c])) return c;
    if (!(r[WBC_BB_MASS] > 0.0)) return WBC_BB_MASS;
    const double* I = r + WBC_BB_INERTIA;
    const double tol = 1e-9 * __builtin_fabs(I[0] + I[4] + I[8]);  // (a valid row has a positive trace)
    if (!(__builtin_fabs(I[1] - I[3]) <= tol)) return WBC_BB_INERTIA + 1;
    if (!(__builtin_fabs(I[2] - I[6]) <= tol)) return WBC_BB_INERTIA + 2;
    if (!(__builtin_fabs(I[5] - I[7]) <= tol)) return WBC_BB_INERTIA + 5;
    const double a = I[0], d = I[4], f = I[8], b = 0.5 * (I[1] + I[3]), c = 0.5 * (I[2] + I[6]), e = 0.5 * (I[5] + I[7]);
    if (!(a > 0.0)) return WBC_BB_INERTIA;
    if (!(a * d - b * b > 0.0)) return WBC_BB_INERTIA + 4;
    if (!(a * (d * f - e * e) - b * (b * f - e * c) + c * (b * e - d * c) > 0.0)) return WBC_BB_INERTIA + 8;
    return -1;
}
// A limits row (wbc.h WBC_LM_*: tau_min[12], tau_max[12], mu[4]) the step accepts: -1, or the first
// column that fails: a non-finite entry at its own column, tau_min[j] > tau_max[j] at tau_max's
// (equal bounds are a dead or locked-torque actuator and valid), mu[l] < 0 at mu's.  One definition for
// the host's validation (wbc_set_limits) and the kernels' (a device-bound row): the kernels hold a row
// spread over a segment's lanes and apply the two entry rules, lm_pair_bad and lm_mu_bad, to what each
// lane holds.
WBC_HD inline bool lm_pair_bad(double lo, double hi) {
    return !__builtin_isfinite(lo) || !__builtin_isfinite(hi) || !(lo <= hi);
}
WBC_HD inline bool lm_mu_bad(double mu) { return !__builtin_isfinite(mu) || mu < 0.0; }
WBC_HD inline int lm_bad_column(const double* r) {
    for (int c = 0; c < WBC_LM_LEN; ++c) {
        if (!__builtin_isfinite(r[c])) return c;
        if (c >= WBC_LM_TAU_MAX && c < WBC_LM_FRICTION && lm_pair_bad(r[c - WBC_LM_TAU_MAX + WBC_LM_TAU_MIN], r[c])) return c;
        if (c >= WBC_LM_FRICTION && lm_mu_bad(r[c])) return c;
    }
    return -1;
}
// A force-bound row (wbc.h WBC_FN_*: fn_min[4], fn_max[4]) the step accepts: -1, or the first column that
// fails: a NaN entry or fn_min = +inf at fn_min's column, fn_max = -inf or fn_min > fn_max at fn_max's
// (equal bounds are valid; fn_min = -inf and fn_max = +inf mean no row).  One definition for the host's
// validation (wbc_set_force_bounds) and the kernels' (a device-bound row): the kernels hold a foot's pair
// in two neighbouring lanes and apply the pair rule, fn_pair_bad, to it.
WBC_HD inline bool fn_lo_bad(double lo) { return !(lo < __builtin_inf()); }   // NaN or +inf
WBC_HD inline bool fn_hi_bad(double hi) { return !(hi > -__builtin_inf()); }  // NaN or -inf
WBC_HD inline bool fn_pair_bad(double lo, double hi) { return fn_lo_bad(lo) || fn_hi_bad(hi) || !(lo <= hi); }
WBC_HD inline int fn_bad_column(const double* r) {
    for (int c = 0; c < WBC_FN_LEN; ++c) {
        if (c < WBC_FN_MAX && fn_lo_bad(r[c])) return c;
        if (c >= WBC_FN_MAX && (r[c] != r[c] || fn_pair_bad(r[c - WBC_FN_MAX + WBC_FN_MIN], r[c]))) return c;
    }
    return -1;
}
// A force-task row (wbc.h WBC_FT_*: fref[12], weight, one reserved) the step accepts: -1, or the first column
// that fails: a non-finite entry in columns 0-12 at its own column, weight <= 0 at the weight's.  The reserved
// column is not read.  One definition for the host's validation (wbc_set_force_task) and the kernels' (a
// device-bound row): the kernels hold fref_i in lane i < 12 and the weight in every lane and apply the two
// entry rules, ft_fref_bad and ft_weight_bad, to what each lane holds.
WBC_HD inline bool ft_fref_bad(double f) { return !__builtin_isfinite(f); }
WBC_HD inline bool ft_weight_bad(double w) { return !__builtin_isfinite(w) || !(w > 0.0); }
WBC_HD inline int ft_bad_column(const double* r) {
    for (int c = 0; c < WBC_FT_WEIGHT; ++c)
        if (ft_fref_bad(r[WBC_FT_FREF + c])) return WBC_FT_FREF + c;
    return ft_weight_bad(r[WBC_FT_WEIGHT]) ? WBC_FT_WEIGHT : -1;
}
WBC_HD inline int32_t qmap_entry(int qp, int mask) { return (int32_t)((qp << 4) | (mask & 15)); }
constexpr int QMAP_SEG = 4;  // QPs per wave (UPD_RPW of the kernel)
// Layout.  The general 12-variable form runs one instruction stream for every contact mask, so
// waves may mix masks at no cost; a stateless mask-15 QP takes the four-contact stance form, a
// different stream, so it never shares a wave with another mask.  Within that rule the map groups
// QPs of one mask (a wave runs its four QPs' largest pass count: QPs of one mask need similar counts)
// and uses at most one wave more than ceil(B / 4), so a batch that fills whole rounds of the chip
// does not spill a partial round:
//   region 0: the r15 = cnt[15] % 4 mask-15 QPs left over from whole waves, padded to one wave
//             (only when r15 > 0);
//   region 1: the other masks' leftovers (< 4 each, at most 45) in mixed waves, the last padded;
//   region 2: whole waves of one mask, buckets in QMAP_ORDER.
// Leftovers are a bucket's last QPs in batch order; a bucket's other QPs keep their batch order;
// padding segments recompute the bucket's first QP.  Buckets start with mask 15 (the most active-set
// passes on the bench batches: 8.9 per QP against 6.7 for three stance legs and 0.3 for none), then
// three stance legs, two, one, none: when a step has more waves than the chip holds at once, the
// hardware starts them in map order, so the costliest start first and the cheapest fill the end.
#ifndef WBC_QMAP_NATURAL_ORDER
constexpr uint8_t QMAP_ORDER[16] = {15, 7, 11, 13, 14, 3, 5, 6, 9, 10, 12, 1, 2, 4, 8, 0};
#else  // (A/B builds only)
constexpr uint8_t QMAP_ORDER[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
#endif
// capacity of the map for B QPs (entries): ceil(B / 4) + 1 waves
WBC_HD inline int qmap_capacity(int B) { return QMAP_SEG * ((B + QMAP_SEG - 1) / QMAP_SEG + 1); }
// The device builder's scratch after the map (wbc_qmap_count / _plan / _scatter): per block of
// QMAP_BLOCK QPs its 16 mask counts (then their exclusive prefixes over the blocks) and 16 first
// indices, then the plan
constexpr int QMAP_BLOCK = 1024;
WBC_HD inline int qmap_blocks(int B) { return (B + QMAP_BLOCK - 1) / QMAP_BLOCK; }
WBC_HD inline int qmap_scratch(int B) { return 32 * qmap_blocks(B) + 64; }
struct QmapPlan {
    int base1, base2, waves;  // region 1 / 2 starts (entries), total waves
    int full[16];             // QPs of bucket m in whole waves (4 * floor(cnt / 4))
    int off1[16], off2[16];   // bucket m's leftovers in region 1, its whole waves in region 2
    int pad0, pad1, end1;     // padding: region 0 [pad0, 4), region 1 [pad1, end1)
    int32_t v0, v1;           // their entries
};
// the plan from the bucket counts and each bucket's first QP (host and device builders alike)
WBC_HD inline void qmap_plan(const int* cnt, const int* first, QmapPlan& p) {
    const int r15 = cnt[15] % QMAP_SEG;
    p.base1 = r15 ? QMAP_SEG : 0;
    p.pad0 = r15;
    p.v0 = ~qmap_entry(first[15] < 0 ? 0 : first[15], 15);
    int o1 = 0, o2 = 0, last = -1;
#pragma unroll  // (device builder: bucket m a constant, the plan's fields registers)
    for (int k = 0; k < 16; ++k) {
        const int m = QMAP_ORDER[k];
        p.full[m] = cnt[m] - cnt[m] % QMAP_SEG;
        p.off2[m] = o2;
        o2 += p.full[m];
        p.off1[m] = o1;
        if (m != 15 && cnt[m] % QMAP_SEG) {
            o1 += cnt[m] % QMAP_SEG;
            last = m;
        }
    }
    p.pad1 = p.base1 + o1;
    p.end1 = p.base1 + QMAP_SEG * ((o1 + QMAP_SEG - 1) / QMAP_SEG);
    p.v1 = last < 0 ? 0 : ~qmap_entry(first[last], last);
    p.base2 = p.end1;
    p.waves = (p.base2 + o2) / QMAP_SEG;
}
// entry position of the j-th QP (batch order) of bucket m
WBC_HD inline int qmap_pos(const QmapPlan& p, int m, int j) {
    if (j < p.full[m]) return p.base2 + p.off2[m] + j;
    const int i = j - p.full[m];
    return (m == 15) ? i : p.base1 + p.off1[m] + i;
}
// Host form: returns the number of waves; 0 (map unused) when every mask is equal.
inline int qmap_build(const uint8_t* masks, int B, int32_t* map) {
    int cnt[16] = {0}, first[16];
    for (int m = 0; m < 16; ++m) first[m] = -1;
    for (int b = 0; b < B; ++b) {
        const int m = masks[b] & 15;
        if (first[m] < 0) first[m] = b;
        ++cnt[m];
    }
    for (int m = 0; m < 16; ++m)
        if (cnt[m] == B) return 0;
    QmapPlan p;
    qmap_plan(cnt, first, p);
    int j[16] = {0};
    for (int b = 0; b < B; ++b) {
        const int m = masks[b] & 15;
        map[qmap_pos(p, m, j[m]++)] = qmap_entry(b, m);
    }
    for (int e = p.pad0; p.base1 && e < QMAP_SEG; ++e) map[e] = p.v0;
    for (int e = p.pad1; e < p.end1; ++e) map[e] = p.v1;
    return p.waves;
}



// Mode hypotheses per wave (KernelArgs::mloop, wbc_modes_kernel) for K hypotheses over `groups`
// four-state groups on a device with `simds` SIMDs: the largest M dividing K that still gives
// every SIMD a wave (groups K / M >= simds), 1 (one hypothesis per segment) when even that leaves
// SIMDs idle; m_override (a divisor of K; 0 = none) replaces it.  order[c M .. c M + M - 1] are
// chunk c's hypotheses: longest first, each to the chunk with the least estimated work so far
// (LPT), the estimate a reduction and solve of 30 units plus 3 per expected working-set pass
// (0.3, 2.3, 4.5, 6.7, 8.9 passes for 0 .. 4 stance legs).  Returns M.
inline int mode_loop_plan(const uint8_t* modes, int K, int64_t groups, int64_t simds, int m_override,
                          uint8_t* order) {
    int M = 1;
    for (int m = K; m > 1; --m)
        if (K % m == 0 && groups * (K / m) >= simds) { M = m; break; }
    if (m_override >= 1 && m_override <= K && K % m_override == 0) M = m_override;
    static const double passes[5] = {0.3, 2.3, 4.5, 6.7, 8.9};
    const int C = K / M;
    int idx[16], fill[16] = {};
    double load[16] = {};
    for (int k = 0; k < K; ++k) idx[k] = k;
    auto cost = [&](int k) { return 30.0 + 3.0 * passes[__builtin_popcount(modes[k] & 15u)]; };
    for (int a = 1; a < K; ++a)  // stable insertion sort, costliest first
        for (int b = a; b > 0 && cost(idx[b]) > cost(idx[b - 1]); --b) {
            const int t = idx[b]; idx[b] = idx[b - 1]; idx[b - 1] = t;
        }
    uint8_t chunk[16][16];
    for (int t = 0; t < K; ++t) {
        int best = -1;
        for (int c = 0; c < C; ++c)
            if (fill[c] < M && (best < 0 || load[c] < load[best])) best = c;
        chunk[best][fill[best]++] = (uint8_t)idx[t];
        load[best] += cost(idx[t]);
    }
    for (int c = 0; c < C; ++c)
        for (int i = 0; i < M; ++i) order[c * M + i] = chunk[c][i];
    return M;
}
}  // namespace wbc
#endif
