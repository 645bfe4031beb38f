/*
 * wbc.h — C-ABI of the MI355X batched whole-body-control engine.
 *
 * Drop-in boundary for the per-cycle hot path of the reference's `WholeBodyController`
 * (include/anymal_wbc/whole_body_controller.hpp:35-171, src/whole_body_controller.cpp:256-577):
 *
 *   reference call (file:line)                                   -> C-ABI entry point
 *   WholeBodyController::WholeBodyController()  cpp:22-59         -> wbc_create
 *   WholeBodyController::~WholeBodyController() cpp:61-63         -> wbc_destroy
 *   loadParameters()                            cpp:122-148       -> wbc_params (wbc_default_params)
 *   ModelLoader::loadModelFromFile(urdf)        cpp:26-40         -> wbc_model (wbc_anymal_model)
 *   floatingBaseStateCallback/jointStateCallback cpp:187-254      -> wbc_set_state
 *   referenceCallback(WbcReferenceMsg)          cpp:150-185       -> wbc_set_reference
 *   setInitialState() + firstControllerIteration_ cpp:65-120,523  -> wbc_reset
 *   updateState()                               cpp:256-294       -> wbc_update
 *   solveQP() + computeJointTorques()           cpp:466-577       -> wbc_solve
 *   controlLoop() body (update; solve; torques) cpp:650-652       -> wbc_step (fused)
 *   jointTorquePub_/desiredGroundReactionForcesPub_ cpp:563,576   -> wbc_get_output
 *   qpReturnValue_ != SUCCESSFUL_RETURN          cpp:654           -> per-robot status[] (WBC_QP_*)
 *   qpOASES getObjVal() of the solver of cpp:517-533               -> wbc_get_objective (wbc_step_modes, WBC_OBJECTIVE)
 *   qpOASES getDualSolution() of the same solver, rows R2 and R3   -> wbc_get_duals (wbc_step, WBC_DUALS)
 *
 * Conventions
 *  - Everything is fp64.  Sizes are compile-time constants of the reference (hpp:27-32).
 *  - A handle owns B robots ("batch").  Host arrays are robot-major per quantity
 *    (array[b * width + k]); each quantity is its own array (struct of arrays).
 *  - Leg / joint order: LH, LF, RF, RH x (HAA, HFE, KFE) — the reference's model order
 *    (cpp:81,234,327-341).  Contact bit i of contacts[b] = footContacts_[i] (cpp:183).
 *  - base_pose[b] = (px, py, pz, qx, qy, qz, qw) as in gazebo_msgs/ModelStates.pose (cpp:209-218).
 *  - nu[b] = (v_lin world (3), omega world (3), qdot (12)) = [baseVel_; jointVel_] (cpp:228,287).
 *  - ref[b] = WbcReferenceMsg field order (msg/WbcReferenceMsg.msg:1-6): desiredComPose (6),
 *    desiredComVelocity (6), desiredComAcceleration (6), desiredSwingLegsPosition (12),
 *    desiredSwingLegsVelocity (12), desiredSwingLegsAcceleration (12).
 *  - switching[b] = isSwitchingFootState_ (cpp:176-184); the caller latches it (quirk A.7).
 *  - Every call returns WBC_OK (0) or a negative error; no exceptions cross the boundary.
 *  - A handle is used by one host thread.  Inputs are snapshotted when the step kernel reads
 *    them, which removes the reference's callback/control-thread race (cpp:499,681-682).
 */
#ifndef WBC_H
#define WBC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WBC_NUM_LEGS 4
#define WBC_NUM_JOINTS 12
#define WBC_NUM_DOF 18
#define WBC_NV 42 /* qpNumberOfVariables, hpp:31 */
#define WBC_NC 70 /* qpNumberOfConstraints, hpp:32 */
#define WBC_POSE_LEN 7
#define WBC_NU_LEN 18
#define WBC_REF_LEN 54

/* One lumped rigid body hanging off a revolute joint (tools/gen_model.py). */
typedef struct wbc_link {
    double R[9];       /* parent body frame -> joint frame at q = 0, row-major */
    double p[3];       /* joint origin in the parent body frame */
    double axis[3];    /* joint axis in the joint (= child body) frame */
    double mass;
    double com[3];     /* child body frame */
    double inertia[9]; /* about the com, child body axes, row-major */
} wbc_link;

/* Lumped ANYmal model: replaces iDynTree::Model built from urdf/anymal.urdf (cpp:26-40). */
typedef struct wbc_model {
    double base_mass;
    double base_com[3];
    double base_inertia[9];
    wbc_link link[WBC_NUM_LEGS][3]; /* legs LH, LF, RF, RH; links after HAA, HFE, KFE */
    double foot[WBC_NUM_LEGS][3];   /* {LH,LF,RF,RH}_FOOT origin in the SHANK body frame */
    double total_mass;              /* model_.getTotalMass(), cpp:72 */
} wbc_model;

/* Controller parameters: config/params_controller.yaml:1-12, read at cpp:122-148. */
typedef struct wbc_params {
    double friction;     /* mu */
    double loop_rate;    /* Hz; finite-difference step 1/loop_rate (cpp:394) */
    double max_torque;   /* torque limit rows R3 (cpp:506,513) */
    double kp, kp_z, kd, ki;        /* wrench PD(I) gains (cpp:429-432) */
    double kp_swing, kd_swing;      /* swing-foot PD (cpp:449-450) */
    double slack_weight;            /* R block of slacks (cpp:476) */
    double initial_reference_pose[6];
    double gravity;                 /* gravityAcceleration, hpp:30 */
    int32_t max_wsr;                /* nWSR = 100 (cpp:517) */
    int32_t reserved;
} wbc_params;

/* API return codes. */
enum {
    WBC_OK = 0,
    WBC_ERR_ARG = -1,
    WBC_ERR_HIP = -2,
    WBC_ERR_STATE = -3,
    WBC_ERR_NO_DEVICE = -4
};

/* Per-robot QP status (status[] output); 0 mirrors qpOASES SUCCESSFUL_RETURN (cpp:654). */
enum {
    WBC_QP_OK = 0,
    WBC_QP_MAX_ITER = 1,   /* more than max_wsr working-set changes (nWSR exceeded; see iters below) */
    WBC_QP_INFEASIBLE = 2, /* constraints inconsistent */
    WBC_QP_NUMERIC = 3     /* non-finite input or factorisation breakdown */
};

/* Step flags. */
#define WBC_STATELESS 1u /* cold step: history = reset values; history is neither read nor written.
                          * Without it the step is stateful: finite-difference history, integral
                          * error and a QP hotstart from the previous working set (as qpOASES
                          * SQProblem::hotstart, src/whole_body_controller.cpp:531). */
#define WBC_DEBUG 2u     /* also write the per-robot debug record (wbc_get_debug) */
#define WBC_NO_X 4u      /* skip the x[42] output (tau, grf, status, iters are still written) */
#define WBC_SPLIT 8u     /* wbc_step / wbc_step_modes as the split kernels (update, then the general
                          * 24-variable or four-contact solve kernel: wbc_update + wbc_solve) */
#define WBC_TIMED 16u    /* wbc_step records HIP events around its kernels (wbc_last_kernel_ms) */
#define WBC_COLD 32u     /* stateful, but the QP starts cold (no hotstart from the previous working set) */
#define WBC_FUSED 64u    /* wbc_step as the one-robot-per-wave kernel of the general 24-variable method */
#define WBC_GROUP 128u   /* device-bound contact masks (wbc_bind_device_inputs): group the QPs by mask on
                          * the stream before the step (one small kernel), as the engine does on the
                          * host for masks it copies.  Same results either way; it pays when the masks
                          * are mixed (waves of one mask), not when they are all equal (a trot). */
#define WBC_RESIDENT 256u /* wbc_cycle only, B <= 4: the step stays resident on the GPU between cycles (one
                          * workgroup polling a pinned mailbox), so a cycle costs no kernel launch and no
                          * stream synchronisation (the B = 1 drop-in).  The resident wave
                          * ends after 100 ms without a cycle, or at any other call on the engine (which
                          * waits for it); the next WBC_RESIDENT cycle starts it again.  Same results as a
                          * plain wbc_cycle. */
#define WBC_OBJECTIVE 512u /* wbc_step_modes only (default form): also write each hypothesis' QP objective at its
                          * optimum (wbc_get_objective / wbc_device_objective) */
#define WBC_BEST 1024u   /* wbc_step_modes only (default form), implies WBC_OBJECTIVE: after the step, choose each
                          * state's best feasible hypothesis (wbc_get_best_modes / wbc_device_best_modes) */
#define WBC_DUALS 2048u  /* wbc_step only (default form): also write each robot's QP multipliers of the friction
                          * faces and torque limits (wbc_get_duals / wbc_device_duals) */
#define WBC_DUALS_FORCE 4096u /* wbc_step only (default form), implies WBC_DUALS: the same 40 multipliers and the 8 of
                          * the per-foot normal-force bounds, 48 per robot (wbc_get_force_duals /
                          * wbc_device_force_duals); allowed with and without a force-bound table in force */
#define WBC_DUALS_TASK 8192u /* wbc_step only (default form), implies WBC_DUALS_FORCE: the same 48 multipliers under a
                          * per-robot force task (wbc_set_force_task), read with the same two getters; allowed
                          * with and without a force-task table in force */

/* Debug record layout (doubles per robot), written by update/step under WBC_DEBUG. */
enum {
    WBC_DBG_COM = 0,        /* c (3)                       getCenterOfMassPosition (cpp:260) */
    WBC_DBG_COMVEL = 3,     /* c-dot (3)                   getCenterOfMassVelocity (cpp:261) */
    WBC_DBG_POSE = 6,       /* currentPose_ (6)            cpp:264 */
    WBC_DBG_VC = 12,        /* centerOfMassVelocity_ (6)   cpp:261 */
    WBC_DBG_M = 18,         /* mass matrix 18x18 row-major cpp:266 */
    WBC_DBG_CNU = 342,      /* C(q,nu) nu (18)             cpp:544-551 */
    WBC_DBG_JFEET = 360,    /* foot Jacobians rows 0-2, 12x18 (LH,LF,RF,RH) cpp:327-341 */
    WBC_DBG_PFEET = 576,    /* foot positions (12)         cpp:344-362 */
    WBC_DBG_VFEET = 588,    /* foot velocities (12)        cpp:364-382 */
    WBC_DBG_MBARB = 600,    /* centroidMassMatrixBase_ 6x6 cpp:271 */
    WBC_DBG_MBARJ = 636,    /* centroidMassMatrixJoints_ 12x12 cpp:272 */
    WBC_DBG_JBAR = 780,     /* J_feet T^-1 (unmasked) 12x18 cpp:278-284 */
    WBC_DBG_BBAR = 996,     /* centroidGeneralizedBias_ (18) cpp:289 */
    WBC_DBG_WRENCH = 1014,  /* computeDesiredWrench (6)    cpp:426-445 */
    WBC_DBG_R1 = 1020,      /* R1 bounds: -Jc_dot v (12)   cpp:504 */
    WBC_DBG_RSW = 1032,     /* R4/R5 bound: cmd - Js_dot v (12) cpp:507,515 */
    WBC_DBG_STAMPS = 1044,  /* diagnostic builds only (-DWBC_STAMPS): s_memtime per phase (8) */
    WBC_DBG_LEN = 1052
};

typedef struct wbc_engine wbc_engine;

/* Defaults of config/params_controller.yaml and the lumped reference URDF. */
int32_t wbc_default_params(wbc_params* out);
int32_t wbc_anymal_model(wbc_model* out);
/* Model from a URDF file at run time (replaces ModelLoader::loadModelFromFile +
 * KinDynComputations::loadRobotModel, cpp:26-40, and the getFrameIndex lookups, cpp:327-379): any
 * 12-DoF quadruped whose legs are 3-revolute-joint chains off the floating base.  Fixed joints are
 * lumped into their parent bodies (exact for M, C nu and frame kinematics).  legs: the 4 leg name
 * prefixes in model order (NULL = LH, LF, RF, RH); joints: the 3 joint suffixes from the base out
 * (NULL = HAA, HFE, KFE), joint names <leg>_<suffix>; foot frames <leg>_<foot_suffix> (NULL = FOOT). */
int32_t wbc_model_from_urdf(const char* urdf_path, const char* const* legs, const char* const* joints,
                            const char* foot_suffix, wbc_model* out);

int32_t wbc_create(const wbc_model* model, const wbc_params* params, int32_t batch, int32_t device,
                   wbc_engine** out);
int32_t wbc_destroy(wbc_engine* h);
int32_t wbc_batch(const wbc_engine* h);
/* Use a caller-owned hipStream_t (NULL = the engine's own stream).  Work queued on the previous
 * stream is drained first (the call synchronizes it), so switching streams never races.  A bound
 * caller stream must stay alive until it is unbound (wbc_set_stream(h, NULL)) or the engine is
 * destroyed: both synchronize it.  (No event is recorded after each launch to track the stream:
 * its packet would cost ~3 us per step.) */
int32_t wbc_set_stream(wbc_engine* h, void* hip_stream);

/* Host inputs, copied to device on the engine stream. Any pointer may be NULL (= unchanged). */
int32_t wbc_set_state(wbc_engine* h, const double* base_pose, const double* nu, const double* qj);
int32_t wbc_set_reference(wbc_engine* h, const double* ref, const uint8_t* contacts,
                          const uint8_t* switching);
/* Device-resident inputs (no copy): the step reads these pointers directly.  NULL restores
 * the engine-owned buffer for that quantity. */
int32_t wbc_bind_device_inputs(wbc_engine* h, const double* d_base_pose, const double* d_nu,
                               const double* d_qj, const double* d_ref, const uint8_t* d_contacts,
                               const uint8_t* d_switching);

/* Caller-owned device output buffers (no copy): the step writes into these pointers directly
 * (e.g. a tensor that an RCCL all-gather then reads).  NULL restores the engine-owned buffer. */
int32_t wbc_bind_device_outputs(wbc_engine* h, double* d_tau, double* d_grf, double* d_x, int32_t* d_status,
                                int32_t* d_iters);

/* Reset robots to setInitialState() (cpp:65-120) + first-iteration cold start.  mask NULL = all. */
int32_t wbc_reset(wbc_engine* h, const uint8_t* mask);

/* updateState(): dynamics, centroidal transform, finite differences, assembly (stream-ordered). */
int32_t wbc_update(wbc_engine* h, uint32_t flags);
/* solveQP() + computeJointTorques() on the problem assembled by the last wbc_update. */
int32_t wbc_solve(wbc_engine* h, uint32_t flags);
/* update + solve + torques for one control cycle.  By default one kernel, four robots per wave:
 * each robot's QP is reduced exactly to 12 variables (the swing slacks and stance equalities
 * eliminated) and solved in place, any contact mask, stateless or stateful (with
 * the hotstart); a robot whose reduction is not usable (a near-singular stance leg) is solved with
 * the general 24-variable method by the same wave, inside the same launch (drain_fallbacks,
 * DESIGN.md 4.9).  A robot's result depends only on its own inputs, mask and flags, never on its
 * batch neighbours; the QPs are grouped by contact mask (one mask per wave: the host-copied masks'
 * map is built when they are copied, device-bound masks' under WBC_GROUP).
 * WBC_SPLIT: the update kernel then the solve kernels, the problem passing through HBM (the form
 * wbc_update + wbc_solve run); WBC_FUSED: one robot per wave, the general method with the problem
 * in LDS.  All forms return the same x and tau (to rounding) and the same status while the
 * working-set cap does not bind.  `iters` counts the working-set changes of the method that ran:
 * the 12-variable form's friction and torque rows by default, the general form's rows (the swing
 * slack rows included, the convention of a dense active set on the reference's 42 x 70 QP) under
 * WBC_SPLIT / WBC_FUSED.  WBC_QP_MAX_ITER is judged on that count against max_wsr, so near the cap
 * the default form (fewer changes for the same QP) can return WBC_QP_OK where the split / fused
 * forms return WBC_QP_MAX_ITER.
 * Every form picks the row to add as the most violated one by slack / |reference row|, with near-
 * ties treated as ties: the lowest row id among the rows within WBC_TIE_BAND (relative) of the
 * most violated, so the route (and `iters`) does not depend on rounding when two rows are violated
 * alike in exact arithmetic.  The C oracle (oracle/wbc_ref.c) applies the same rule.
 * The general form (WBC_SPLIT / WBC_FUSED and the default step's fallback) also treats an r_k (the
 * pending row's coefficient on active slot k) below WBC_R_REL times the largest |r| as zero, not as
 * a drop candidate: when the pending row depends on the active set (an infeasible QP), those r_k
 * are rounding noise, and the number of noise drops before WBC_QP_INFEASIBLE would otherwise
 * depend on the form's rounding. */
#define WBC_TIE_BAND 1e-9
#define WBC_R_REL 1e-12
int32_t wbc_step(wbc_engine* h, uint32_t flags);
int32_t wbc_synchronize(wbc_engine* h);
/* Which constraints bind, and how hard: the Lagrange multipliers of the QP's inequality rows that can be
 * active at an optimum with positive price, the 16 friction faces (R2, cpp:404-424) and the 24 torque
 * limits (R3, cpp:495,506,513), what qpOASES' getDualSolution() returns for those rows.
 * wbc_step(flags | WBC_DUALS) in its default form also writes dual[b * WBC_DUAL_LEN + r] for robot b, in
 * the row numbering the hotstart stores:
 *     r = 4 leg + face              the friction faces, in the reference's R2 order
 *     r = 16 + 2 j + side           joint j's torque rows: side 0 is tau_j >= -max_torque,
 *                                   side 1 is tau_j <= +max_torque
 * Each entry is the multiplier lambda_r >= 0 of the reference's row as the reference writes it (unscaled:
 * the face (+-1, 0, mu) . f_l >= 0 in the foot's frame, the torque row in N m): the objective's rate of
 * change per unit of relaxation of that row (a saturated actuator's lambda is what 1 N m more would buy).
 * An entry is 0 for a row outside the final working set, for every face of a swing leg, and a robot
 * whose status is not WBC_QP_OK has all 40 entries 0, like its other outputs.  At most 12 entries of a
 * robot are non-zero.
 * They are the multipliers of the same rows of the reference's 42 x 70 QP: the default step eliminates
 * a, the swing slacks and the stance equalities exactly, which changes neither the
 * objective's value nor these rows' slacks at any point, so the reduced QP's multipliers on them are the
 * full QP's.  In qpOASES' sign convention (lbA <= A x <= ubA, H x + g = A^T y) they are y = -lambda on a
 * friction row and on side 1 (upper bounds), y = +lambda on side 0 (a lower bound).  The other
 * multipliers follow from x: of a swing leg's slack pair R4 / R5 (cpp:496-497,507-515), whichever row
 * is tight carries slack_weight * s_i (stationarity in s_i), the other 0; the 18 equality multipliers
 * (R0 / R1) are then fixed by stationarity, H x + g = A^T y, a least-squares fit of at most 18 unknowns
 * to 42 equations whose residual certifies x: with primal feasibility, lambda >= 0 and lambda_r = 0 on
 * slack rows it is the KKT system of a strictly convex QP, so x is its optimum.
 * Allowed stateless, stateful and with WBC_COLD, with WBC_DEBUG, WBC_NO_X, WBC_TIMED and WBC_GROUP, and
 * with any of the per-robot tables in force; tau, grf, x, status and iters are bit-identical to a step
 * without the flag.  The buffer is the engine's own, allocated at the first step that carries the flag
 * and written on the engine's stream as the other outputs are (the device pointer stays valid until
 * wbc_destroy).  wbc_get_duals is synchronous.  Both getters return WBC_ERR_STATE unless the last
 * wbc_step carried the flag.  WBC_DUALS with WBC_SPLIT, WBC_FUSED or WBC_RESIDENT, or on wbc_update /
 * wbc_solve / wbc_cycle / wbc_step_modes, is WBC_ERR_ARG. */
enum { WBC_DUAL_LEN = 40 };
int32_t wbc_get_duals(wbc_engine* h, double* dual /* [B][40] */);
int32_t wbc_device_duals(wbc_engine* h, double** d_dual);
/* The same under per-foot normal-force bounds (wbc_set_force_bounds below): wbc_step(flags | WBC_DUALS_FORCE)
 * in its default form writes dual[b * WBC_DUAL_FORCE_LEN + r] for robot b.  Entries 0..39 are WBC_DUALS' own,
 * in the same numbering, and
 *     r = 40 + 2 leg + side         the leg's force row: side 0 is n_l . f_l >= fn_min[l],
 *                                   side 1 is n_l . f_l <= fn_max[l]
 * holds the multiplier lambda_r >= 0 of that row in newtons of normal force: what one newton more of
 * fn_max (or less of fn_min) would buy, so a foot held by its load ramp and not by its friction cone shows
 * a non-zero entry 41 + 2 leg and zero faces.  In qpOASES' sign convention for the two-sided row,
 * y = lambda_side0 - lambda_side1.  An entry is 0 for a row that does not exist (an infinite bound, a foot
 * in swing) or does not bind, and all 48 are 0 unless the status is WBC_QP_OK.  A force row contains no
 * slack and none of the eliminated variables' own rows, so the elimination argument above covers it
 * (DESIGN.md 23).
 * The flag implies WBC_DUALS (that bit is ignored beside it); WBC_DUALS alone stays what it is, 40 entries,
 * and stays refused while a force-bound table is in force.  Allowed as WBC_DUALS is (stateless, stateful,
 * WBC_COLD, WBC_DEBUG, WBC_NO_X, WBC_TIMED, WBC_GROUP, any combination of the per-robot tables), with or
 * without a force-bound table: without one the step runs under the engine's own no-bounds table, entries
 * 40..47 are 0 and entries 0..39 hold WBC_DUALS' bits, so a caller who switches a load ramp on and off
 * keeps one code path.  tau, grf, x, status and iters are bit-identical to the step without the flag.
 * The buffer is the engine's own ([B][48], apart from WBC_DUALS' [B][40]: the strides differ, so neither
 * stands in for the other), allocated at the first step that carries the flag, written on the engine's
 * stream and freed by wbc_destroy.  wbc_get_force_duals is synchronous.  Both getters return WBC_ERR_STATE
 * unless the last wbc_step carried WBC_DUALS_FORCE, and after such a step wbc_get_duals / wbc_device_duals
 * return WBC_ERR_STATE.  WBC_DUALS_FORCE with WBC_SPLIT, WBC_FUSED or WBC_RESIDENT, or on wbc_update /
 * wbc_solve / wbc_cycle / wbc_step_modes, is WBC_ERR_ARG. */
/* Under a per-robot force task (wbc_set_force_task below) the flag is WBC_DUALS_TASK: wbc_step(flags |
 * WBC_DUALS_TASK) in its default form writes the same [B][WBC_DUAL_FORCE_LEN] vector in the same numbering into
 * the same buffer, read with the same two getters (after such a step they succeed, and wbc_get_duals /
 * wbc_device_duals return WBC_ERR_STATE as after WBC_DUALS_FORCE).  The multipliers are those of the QP the
 * step solves: the 74-row problem whose diagonal entries 18 + 3 l + k of a stance leg carry w and whose
 * gradient entries lose w fref[3 l + k].  The task changes H and g and no row, so the elimination argument
 * above holds word for word; what changes is the scale: lambda is in units of the objective per row unit, and
 * the objective's force part is 1/2 w |f - fref|^2, so the multipliers grow with w (a row that keeps a foot
 * from its reference force prices a newton at about w times the distance to the reference).  The flag implies
 * WBC_DUALS_FORCE (that bit and WBC_DUALS' are ignored beside it); the two older flags keep their refusals
 * while a force-task table is in force.  Allowed as WBC_DUALS_FORCE is, with any combination of the six
 * per-robot tables, the force task included, and without a force-task table: then the step runs under the
 * engine's own table of (0 x 12, 1, 0) rows (built at the first such step, freed by wbc_destroy) and all 48
 * entries, tau, grf, x, status and iters are WBC_DUALS_FORCE's bits, so a caller who switches the task on and
 * off keeps one code path.  Under a table, tau, grf, x, status and iters are bit-identical to the step without
 * the flag.  WBC_DUALS_TASK with WBC_SPLIT, WBC_FUSED or WBC_RESIDENT, or on wbc_update / wbc_solve /
 * wbc_cycle / wbc_step_modes, is WBC_ERR_ARG. */
enum { WBC_DUAL_FORCE_LEN = 48 };
int32_t wbc_get_force_duals(wbc_engine* h, double* dual /* [B][48] */);
int32_t wbc_device_force_duals(wbc_engine* h, double** d_dual);

/* Contact-mode hypotheses (BASELINE configs[4]: every state solved under several contact masks).
 * After wbc_set_modes(h, K, modes) with K dividing the batch B, the engine holds S = B / K states:
 * wbc_set_state / wbc_set_reference / bound device inputs hold S rows (contacts[] is not read), and
 * wbc_step_modes solves K QPs per state: output row s * K + k is state s under contact mask
 * modes[k] (4-bit, footContacts_ order), bit-identical to a wbc_step on that state with
 * contacts = modes[k] (same flags).  By default each hypothesis runs in its own 16-lane segment
 * (the state's inputs read from L2 by its K segments, nothing through HBM); WBC_SPLIT computes the
 * dynamics and assembly (updateState, cpp:256-294) once per state and writes them to HBM for K
 * general solves.
 * Hypotheses are cold steps: flags must include WBC_STATELESS (WBC_DEBUG is refused).
 * wbc_update / wbc_solve / wbc_step return WBC_ERR_STATE while modes are set; K = 0 clears them. */
#define WBC_MAX_MODES 16
int32_t wbc_set_modes(wbc_engine* h, int32_t n_modes, const uint8_t* modes);
int32_t wbc_step_modes(wbc_engine* h, uint32_t flags);
/* Hypotheses per wave of the default wbc_step_modes (no reference counterpart; diagnostics): 1 =
 * one hypothesis per 16-lane segment (wbc_update_solve_kernel); M > 1 = the mode loop
 * (wbc_modes_kernel: one update per state and wave, then M hypotheses in turn), chosen by
 * wbc_set_modes from the batch and the device's CU count (WBC_MODES_M in the environment overrides
 * it with a divisor of n_modes).  Results are bit-identical either way. */
int32_t wbc_modes_per_wave(wbc_engine* h, int32_t* m);
/* Which hypothesis to use: the QP's own objective at the optimum, what qpOASES' getObjVal() returns for
 * the reference's problem (cpp:466-515: H = S^T Jc,com Jc,com^T S + R, R = diag(I_30, slack_weight I_12),
 * g = -S^T Jc,com W),
 *     obj = 1/2 x^T H x + g^T x
 *         = 1/2 (|a|^2 + |qdd|^2 + |f|^2 + slack_weight |s|^2) + 1/2 |E^T f|^2 - W . (E^T f),
 * with x = [a; qdd; f; s], E^T f = (sum_l f_l, sum_l d_l x f_l) over the stance legs and W the desired
 * wrench (cpp:426-445), formed in the solve where those live.
 * wbc_step_modes(flags | WBC_OBJECTIVE) also writes obj[s * K + k], laid out as the other outputs;
 * a hypothesis whose status is not WBC_QP_OK has obj = +infinity (its other outputs are zero as ever).
 * WBC_NO_X is allowed and does not change the objective's bits; tau, grf, x, status and iters are
 * bit-identical to a step without the flag.  WBC_BEST (implies WBC_OBJECTIVE) then chooses per state
 * s the index k into modes[] (not the mask) of the lowest objective among its WBC_QP_OK hypotheses
 * (compared as doubles, a tie to the lowest k) and gathers that row's tau and grf, bit for bit, into
 * [S][12] arrays, with the objective in obj[s]; a state with no OK hypothesis has best = -1,
 * obj = +infinity, zero tau and grf.  wbc_get_best_modes: any pointer may be NULL.
 * The buffers are the engine's own, allocated at the first step that carries a flag, and written on the
 * engine's stream as the other outputs are (the device pointers stay valid until wbc_destroy).  The
 * getters return WBC_ERR_STATE unless the last wbc_step_modes carried the matching flag.  Either
 * flag with WBC_SPLIT, or on wbc_step / wbc_update / wbc_solve / wbc_cycle, is WBC_ERR_ARG. */
int32_t wbc_get_objective(wbc_engine* h, double* obj /* [B] */);
int32_t wbc_device_objective(wbc_engine* h, double** d_obj);
int32_t wbc_get_best_modes(wbc_engine* h, int32_t* best /* [S] */, double* obj /* [S] */, double* tau /* [S][12] */,
                           double* grf /* [S][12] */);
int32_t wbc_device_best_modes(wbc_engine* h, int32_t** d_best, double** d_obj, double** d_tau, double** d_grf);

/* Per-robot controller parameters (an RL batch with randomised friction, actuator limit and gains;
 * a sweep over gains): a table of doubles, row-major [B][WBC_RP_LEN], row b for robot b.  Rows are
 * 80 bytes, so a table that starts 16-byte aligned keeps every row 16-byte aligned (required of a
 * device-bound table).  While a table is in force the default wbc_step reads the nine values of
 * each robot's QP from its row instead of the engine-wide wbc_params; loop_rate, gravity, max_wsr
 * and initial_reference_pose stay engine-wide.  A robot's result depends only on its own row. */
enum {
    WBC_RP_FRICTION = 0,     /* wbc_params::friction */
    WBC_RP_MAX_TORQUE = 1,   /* max_torque */
    WBC_RP_KP = 2,           /* kp */
    WBC_RP_KP_Z = 3,         /* kp_z */
    WBC_RP_KD = 4,           /* kd */
    WBC_RP_KI = 5,           /* ki */
    WBC_RP_KP_SWING = 6,     /* kp_swing */
    WBC_RP_KD_SWING = 7,     /* kd_swing */
    WBC_RP_SLACK_WEIGHT = 8, /* slack_weight */
    /* 9: reserved (ignored on input, written as 0 by wbc_get_robot_params) */
    WBC_RP_LEN = 10
};
/* Host table, validated and then copied on the engine stream (the call synchronizes it, so the
 * caller may reuse the array).  A non-finite entry in columns 0-8, friction < 0, max_torque < 0 or
 * slack_weight <= 0 returns WBC_ERR_ARG, wbc_last_error names the row and the column, and the table
 * in force before the call stays in force.  NULL clears the table: back to the engine-wide
 * wbc_params.
 * While a table is in force (this one or a device-bound one):
 *  - supported: wbc_step in its default form (stateless, stateful and WBC_COLD; with WBC_DEBUG,
 *    WBC_NO_X, WBC_TIMED and WBC_GROUP) and plain wbc_cycle.  A robot's row may change between
 *    stateful cycles; history and hotstart carry over as they do when the inputs change.
 *  - refused with WBC_ERR_STATE (wbc_last_error names the call or flag): wbc_update, wbc_solve,
 *    wbc_step_modes, and wbc_step / wbc_cycle with WBC_SPLIT, WBC_FUSED or WBC_RESIDENT.  These
 *    forms read the engine-wide parameters only; they run as before once the table is cleared
 *    (wbc_set_robot_params(h, NULL) and no device table bound). */
int32_t wbc_set_robot_params(wbc_engine* h, const double* table);
/* Caller-owned device table [B][WBC_RP_LEN] (no copy, no host validation; as
 * wbc_bind_device_inputs: the step reads the pointer directly).  NULL restores the engine-owned
 * table of wbc_set_robot_params, or none if none was set.  On the device a row that fails the
 * predicate above gives that robot WBC_QP_NUMERIC and zero outputs, as a non-finite input does; no
 * other robot is touched. */
int32_t wbc_bind_device_robot_params(wbc_engine* h, const double* d_table);
/* The table in force, [B][WBC_RP_LEN] to the host (synchronous); without a table, the engine-wide
 * values broadcast to B rows.  Column 9 is written as 0. */
int32_t wbc_get_robot_params(wbc_engine* h, double* table);

/* Per-robot ground normals at the feet (sloped and rough terrain): a table of doubles, row-major
 * [B][WBC_CN_LEN], row b for robot b: the contact normal at each foot in the world frame, legs in
 * footContacts_ order (LH, LF, RF, RH), three doubles per foot.  Rows are 96 bytes, so a table that
 * starts 16-byte aligned keeps every row 16-byte aligned (required of a device-bound table).  For
 * foot l with normal m the friction pyramid of the QP (cpp:404-424) stands on the frame
 *     n = m / |m|,   t1 = (e_x - (e_x . n) n) / |...|,   t2 = n x t1
 * and its four faces are, in the reference's order and with bounds (-inf, 0],
 *     t1 - mu n,   -(t1 + mu n),   t2 - mu n,   -(t2 + mu n);
 * m = (0, 0, c), c > 0, gives exactly the flat-ground rows.  The forces of the QP are world-frame, so
 * nothing else of the problem changes.  A foot's normal is valid when its entries are finite,
 * 0.25 <= |m|^2 <= 4 and m_z / |m| >= 0.5 (slopes up to 60 degrees); swing feet are validated too. */
enum { WBC_CN_LEN = 12 };
/* Host table, validated and then copied on the engine stream (the call synchronizes it, so the
 * caller may reuse the array).  An invalid foot returns WBC_ERR_ARG, wbc_last_error names the row
 * and the foot, and the table in force before the call stays in force.  NULL clears the table: back
 * to flat ground.
 * While normals are in force (this table or a device-bound one), with or without a robot-parameter
 * table:
 *  - supported: wbc_step in its default form (stateless, stateful and WBC_COLD; with WBC_DEBUG,
 *    WBC_NO_X, WBC_TIMED and WBC_GROUP) and plain wbc_cycle.  Normals may change between stateful
 *    cycles; history and hotstart carry over (a warm set that no longer fits is rejected by the
 *    hotstart's own check, and the solve starts cold).
 *  - refused with WBC_ERR_STATE (wbc_last_error names the call or flag): wbc_update, wbc_solve,
 *    wbc_step_modes, and wbc_step / wbc_cycle with WBC_SPLIT, WBC_FUSED or WBC_RESIDENT.  These
 *    forms stand on flat ground only; they run as before once the normals are cleared
 *    (wbc_set_contact_normals(h, NULL) and no device table bound). */
int32_t wbc_set_contact_normals(wbc_engine* h, const double* table);
/* Caller-owned device table [B][WBC_CN_LEN] (no copy, no host validation; the step reads the pointer
 * directly).  NULL restores the engine-owned table of wbc_set_contact_normals, or none if none was
 * set.  On the device a row with an invalid foot gives that robot WBC_QP_NUMERIC and zero outputs,
 * as a non-finite input does; no other robot is touched. */
int32_t wbc_bind_device_contact_normals(wbc_engine* h, const double* d_table);
/* The table in force, [B][WBC_CN_LEN] to the host as given (synchronous); without one, (0, 0, 1)
 * for every foot. */
int32_t wbc_get_contact_normals(wbc_engine* h, double* table);

/* Per-robot base body (a payload on the trunk; randomised mass, CoM and inertia): a table of doubles,
 * row-major [B][WBC_BB_LEN], row b for robot b.  Rows are 112 bytes, so a table that starts 16-byte
 * aligned keeps every row 16-byte aligned (required of a device-bound table).  Robot b is the engine's
 * model with its base body (wbc_model::base_mass, base_com, base_inertia) replaced by row b; link
 * bodies, joint frames and feet are the model's.  The total mass, the CoM, the centroidal inertia and
 * the bias forces follow from the row; the mass of the desired wrench's gravity term is
 *     model.total_mass + (row.mass - model.base_mass),
 * so the model's own base as a row (what wbc_get_base_body returns without a table) gives the plain
 * step bit for bit.  A row is valid when columns 0-12 are finite, mass > 0, the inertia is symmetric
 * to 1e-9 of its trace and its symmetric part is positive definite. */
enum {
    WBC_BB_MASS = 0,    /* wbc_model::base_mass [kg] */
    WBC_BB_COM = 1,     /* base_com[3], base frame [m] */
    WBC_BB_INERTIA = 4, /* base_inertia[9], about the CoM, base axes, row-major [kg m^2] */
    /* 13: reserved (ignored on input, written as 0 by wbc_get_base_body) */
    WBC_BB_LEN = 14
};
/* Host table, validated and then copied on the engine stream (the call synchronizes it, so the
 * caller may reuse the array).  An invalid row returns WBC_ERR_ARG, wbc_last_error names the row and
 * the column, and the table in force before the call stays in force.  NULL clears the table: back to
 * the model's base.
 * While a base-body table is in force (this one or a device-bound one), with or without the other
 * two tables:
 *  - supported: wbc_step in its default form (stateless, stateful and WBC_COLD; with WBC_DEBUG,
 *    WBC_NO_X, WBC_TIMED and WBC_GROUP) and plain wbc_cycle.  A row may change between stateful
 *    cycles: the finite differences of the next cycle then see the change exactly as the reference's
 *    would see a changed model (its history holds the previous cycle's T and Jbar, not the model).
 *  - refused with WBC_ERR_STATE (wbc_last_error names the call or flag): wbc_update, wbc_solve,
 *    wbc_step_modes, and wbc_step / wbc_cycle with WBC_SPLIT, WBC_FUSED or WBC_RESIDENT.  These
 *    forms compute with the model's base only; they run as before once the table is cleared
 *    (wbc_set_base_body(h, NULL) and no device table bound). */
int32_t wbc_set_base_body(wbc_engine* h, const double* table);
/* Caller-owned device table [B][WBC_BB_LEN] (no copy, no host validation; the step reads the pointer
 * directly).  NULL restores the engine-owned table of wbc_set_base_body, or none if none was set.  On
 * the device an invalid row gives that robot WBC_QP_NUMERIC and zero outputs, as a non-finite input
 * does; no other robot is touched. */
int32_t wbc_bind_device_base_body(wbc_engine* h, const double* d_table);
/* The table in force, [B][WBC_BB_LEN] to the host (synchronous); without one, the model's base in
 * every row.  Column 13 is written as 0. */
int32_t wbc_get_base_body(wbc_engine* h, double* table);

/* Per-robot joint torque bounds and per-foot friction coefficients (actuator limits that differ per
 * joint, are asymmetric and change every cycle with the torque-speed envelope; a derated or dead
 * actuator; feet on different ground): a table of doubles, row-major [B][WBC_LM_LEN], row b for robot
 * b.  Rows are 224 bytes, so a table that starts 16-byte aligned keeps every row 16-byte aligned
 * (required of a device-bound table).  While a limits table is in force the torque rows of robot b's
 * QP are, per joint j,
 *     tau_j >= tau_min[j]  (side 0)      tau_j <= tau_max[j]  (side 1)
 * in the row numbering of WBC_DUALS, and the friction faces of foot l use mu[l] (on that foot's own
 * frame under contact normals).  The friction and max_torque columns of a parameter table, and of
 * wbc_params, are then not read for that robot's rows; the gains and the slack weight still come from
 * them.  The row (-max_torque x 12, +max_torque x 12, friction x 4), which wbc_get_limits returns
 * without a table, gives the step without a limits table bit for bit.  A row is valid when its 28
 * entries are finite, tau_min[j] <= tau_max[j] (equal: a dead or locked-torque actuator) and
 * mu[l] >= 0.  A bound is a finite number: an unbounded joint is a large one. */
enum {
    WBC_LM_TAU_MIN = 0,   /* [12] lower torque bound per joint, N m (joint order of tau) */
    WBC_LM_TAU_MAX = 12,  /* [12] upper torque bound per joint */
    WBC_LM_FRICTION = 24, /* [4]  mu per foot (LH, LF, RF, RH) */
    WBC_LM_LEN = 28
};
/* Host table, validated and then copied on the engine stream (the call synchronizes it, so the
 * caller may reuse the array).  An invalid row returns WBC_ERR_ARG, wbc_last_error names the row and
 * the column, and the table in force before the call stays in force.  NULL clears the table: back
 * to max_torque and friction.
 * While a limits table is in force (this one or a device-bound one), with or without the other
 * three tables:
 *  - supported: wbc_step in its default form (stateless, stateful and WBC_COLD; with WBC_DEBUG,
 *    WBC_NO_X, WBC_TIMED, WBC_GROUP and WBC_DUALS) and plain wbc_cycle.  A row may change between
 *    stateful cycles: the hotstart's own check rejects a warm set that no longer fits.
 *  - refused with WBC_ERR_STATE (wbc_last_error names the call or flag): wbc_update, wbc_solve,
 *    wbc_step_modes, and wbc_step / wbc_cycle with WBC_SPLIT, WBC_FUSED or WBC_RESIDENT.  These
 *    forms read max_torque and friction only; they run as before once the table is cleared
 *    (wbc_set_limits(h, NULL) and no device table bound). */
int32_t wbc_set_limits(wbc_engine* h, const double* table);
/* Caller-owned device table [B][WBC_LM_LEN] (no copy, no host validation; the step reads the pointer
 * directly, so a caller may rewrite it on the engine's stream every cycle).  NULL restores the
 * engine-owned table of wbc_set_limits, or none if none was set.  On the device an invalid row gives
 * that robot WBC_QP_NUMERIC and zero outputs, as a non-finite input does; no other robot is touched. */
int32_t wbc_bind_device_limits(wbc_engine* h, const double* d_table);
/* The table in force, [B][WBC_LM_LEN] to the host (synchronous); without one, every robot's
 * (-max_torque x 12, +max_torque x 12, friction x 4), from its parameter row when a parameter table is
 * in force, else from wbc_params. */
int32_t wbc_get_limits(wbc_engine* h, double* table);

/* Per-foot bounds on the normal contact force (contact load ramps: a gait scheduler unloads a foot
 * before lift-off by lowering fn_max to 0 over the last cycles of stance and raises it again after
 * touchdown; fn_min keeps a minimum load on a foot that must not slip): a table of doubles, row-major
 * [B][WBC_FN_LEN], row b for robot b, in newtons.  Rows are 64 bytes.  While a force-bound table is in
 * force the QP of robot b gains, per stance foot l,
 *     fn_min[l] <= n_l . f_l <= fn_max[l],
 * n_l the unit contact normal of foot l (m_l / |m_l| under contact normals, else e_z).  fn_min = -inf
 * and fn_max = +inf mean "no row": the row (-inf x 4, +inf x 4), which wbc_get_force_bounds returns
 * without a table, gives the step without the table bit for bit.  A row is invalid when an entry is
 * NaN, fn_min[l] = +inf, fn_max[l] = -inf or fn_min[l] > fn_max[l] (equal bounds are valid).  A valid
 * row without a feasible point (fn_max < 0, say) is the solver's business: WBC_QP_INFEASIBLE.  In the
 * hotstart's row numbering the rows are 40 + 2 l (n.f >= fn_min) and 41 + 2 l (n.f <= fn_max). */
enum {
    WBC_FN_MIN = 0, /* [4] lower bound of n_l . f_l per foot (LH, LF, RF, RH), N; -inf: none */
    WBC_FN_MAX = 4, /* [4] upper bound; +inf: none */
    WBC_FN_LEN = 8
};
/* Host table, validated and then copied on the engine stream (the call synchronizes it).  An invalid
 * row returns WBC_ERR_ARG, wbc_last_error names the row and the column, and the previous table stays
 * in force.  NULL: back to no table of the engine's own (a bound device table stays in force).
 * Supported under the table: the default wbc_step (stateless, stateful, WBC_COLD, WBC_NO_X, WBC_GROUP)
 * and the plain wbc_cycle, with any of the other per-robot tables in force.  Refused with
 * WBC_ERR_STATE: wbc_update, wbc_solve, wbc_step_modes, wbc_step / wbc_cycle with WBC_SPLIT, WBC_FUSED
 * or WBC_RESIDENT, and wbc_step with WBC_DUALS (a binding force row has no entry among the 40
 * multipliers).  WBC_DUALS_FORCE gives the multipliers under the table: the 40 and the force rows' 8
 * (wbc_get_force_duals above). */
int32_t wbc_set_force_bounds(wbc_engine* h, const double* table);
/* Caller-owned device table [B][WBC_FN_LEN] (no copy, no host validation; 16-byte aligned; a caller may
 * rewrite it on the engine's stream every cycle).  NULL restores the engine-owned table, or none.  On
 * the device an invalid row gives that robot WBC_QP_NUMERIC and zero outputs; no other robot is touched. */
int32_t wbc_bind_device_force_bounds(wbc_engine* h, const double* d_table);
/* The table in force, [B][WBC_FN_LEN] to the host (synchronous); without one (-inf x 4, +inf x 4). */
int32_t wbc_get_force_bounds(wbc_engine* h, double* table);

/* Per-robot reference contact forces, a force-tracking task in the QP's objective (a planner above the
 * whole-body controller, an MPC say, computes reference ground-reaction forces and the step stays near
 * them while it honours the dynamics, the cones and the actuators): a table of doubles, row-major
 * [B][WBC_FT_LEN], row b for robot b.  Rows are 112 bytes, so a 16-byte-aligned table keeps aligned
 * rows.  While a force-task table is in force the regulariser of every stance foot l of robot b changes
 *     1/2 |f_l|^2   ->   1/2 w_b |f_l - fref_{b,l}|^2        (the constant dropped),
 * fref in the world frame, in newtons, legs in the order LH, LF, RF, RH, w_b > 0 one weight per robot: in
 * the reference's 42-variable QP the diagonal entries 18 + 3 l + k of a stance leg gain w - 1 and the
 * gradient entries lose w fref[3 l + k].  Nothing else of the problem changes: the rows, their numbering
 * in the hotstart and the multipliers are what they are without the table.  A swing foot's three fref
 * entries are validated but not read, and its force stays 0.  The row (0 x 12, 1, 0), which
 * wbc_get_force_task returns without a table, gives the step without the table bit for bit.  A row is
 * invalid when an entry of columns 0-12 is not finite or weight <= 0. */
enum {
    WBC_FT_FREF = 0,    /* [12] reference force per foot (LH, LF, RF, RH), world frame, N */
    WBC_FT_WEIGHT = 12, /* weight w of the robot's force task, > 0; 1: the plain regulariser's */
    WBC_FT_LEN = 14     /* column 13 is reserved: ignored on input, 0 from wbc_get_force_task */
};
/* Host table, validated and then copied on the engine stream (the call synchronizes it).  An invalid
 * row returns WBC_ERR_ARG, wbc_last_error names the row and the column, and the previous table stays
 * in force.  NULL: back to no table of the engine's own (a bound device table stays in force).
 * Supported under the table: the default wbc_step (stateless, stateful, WBC_COLD, WBC_DEBUG, WBC_NO_X,
 * WBC_TIMED, WBC_GROUP) and the plain wbc_cycle, with any of the other per-robot tables in force.
 * Refused with WBC_ERR_STATE: wbc_update, wbc_solve, wbc_step_modes, wbc_step / wbc_cycle with
 * WBC_SPLIT, WBC_FUSED or WBC_RESIDENT, and wbc_step with WBC_DUALS or WBC_DUALS_FORCE (neither
 * flag's instance reads the table).  WBC_DUALS_TASK gives the 48 multipliers under the table
 * (wbc_get_force_duals above). */
int32_t wbc_set_force_task(wbc_engine* h, const double* table);
/* Caller-owned device table [B][WBC_FT_LEN] (no copy, no host validation; 16-byte aligned; a caller may
 * rewrite it on the engine's stream every cycle, as a planner's forces are).  NULL restores the
 * engine-owned table, or none.  On the device an invalid row gives that robot WBC_QP_NUMERIC and zero
 * outputs; no other robot is touched. */
int32_t wbc_bind_device_force_task(wbc_engine* h, const double* d_table);
/* The table in force, [B][WBC_FT_LEN] to the host (synchronous), its reserved column 0; without one
 * (0 x 12, 1, 0). */
int32_t wbc_get_force_task(wbc_engine* h, double* table);

/* One synchronous control cycle, host arrays in and out (the low-latency path for small batches,
 * e.g. the B = 1 drop-in of whole_body_controller_node): the inputs are packed into pinned staging
 * and sent in one H2D copy, the step runs (flags as wbc_step), and the outputs come back in one D2H
 * copy and one synchronize.  Same results as wbc_set_state + wbc_set_reference + wbc_step +
 * wbc_get_output.  Inputs are all required; any output may be NULL (x NULL also skips computing
 * it, as WBC_NO_X).  Input and output bindings (wbc_bind_device_*) are left as they were: the
 * cycle reads and writes the engine's own buffers for this one step.  Refused while mode
 * hypotheses are set. */
int32_t wbc_cycle(wbc_engine* h, const double* base_pose, const double* nu, const double* qj, const double* ref,
                  const uint8_t* contacts, const uint8_t* switching, uint32_t flags, double* tau, double* grf,
                  double* x, int32_t* status, int32_t* iters);

/* Outputs (host copies, synchronous).  Any pointer may be NULL.
 * tau [B][12], grf [B][12] (= x[18:30]), x [B][42], status [B], iters [B].
 * A robot whose status is not WBC_QP_OK gets tau, grf and x all zero (the reference publishes
 * qpOASES' last iterate and then stops its control loop, cpp:652-659; a batch keeps running, so
 * a failed robot publishes zeros instead of an unconverged iterate).  iters is the cap
 * (max_wsr) under WBC_QP_MAX_ITER. */
int32_t wbc_get_output(wbc_engine* h, double* tau, double* grf, double* x, int32_t* status,
                       int32_t* iters);
/* Device pointers of the output buffers (valid until wbc_destroy). */
int32_t wbc_device_outputs(wbc_engine* h, double** d_tau, double** d_grf, double** d_x,
                           int32_t** d_status, int32_t** d_iters);
/* Debug records [B][WBC_DBG_LEN] of the last update/step run with WBC_DEBUG. */
int32_t wbc_get_debug(wbc_engine* h, double* out);

/* Device time of the last wbc_step run with WBC_TIMED (ms, HIP events on the engine stream). */
int32_t wbc_last_kernel_ms(wbc_engine* h, double* ms);
const char* wbc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* WBC_H */
