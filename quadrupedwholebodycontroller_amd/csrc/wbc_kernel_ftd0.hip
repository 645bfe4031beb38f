// wbc_kernel_ftd0.hip — the stateless default step under per-robot reference contact forces that also writes the
// QP multipliers of the friction, torque and force rows, 48 per robot
// (wbc_update_solve_duals_kernel<0, false, true, true, true, true, true, true>, KernelArgs::ft and KernelArgs::dual
// as [B][WBC_DUAL_FORCE_LEN]: wbc_step with WBC_DUALS_TASK).  wbc_kernel_ft0.hip's
// configuration with solve16's DU flag: the task changes H and g and no row, so the output stage is fnd0's; an
// all-stance wave takes the stance form here as ft0's does (J0 = c I + Q (L6^-T - c I) Q^T), and its multipliers are
// those of the unscaled rows.  A translation unit of its own (Makefile FTD0_KFLAGS); the code is wbc_kernel.hip's,
// which WBC_STEP_INSTANCE limits to this one kernel and its launcher; WBC_STEP_DUALS names the kernel and turns the
// multipliers on.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_ftd0
#define WBC_STEP_INSTANCE 0, false, true, true, true, true, true, true  // STF, SONLY, RP, CN, BB, LM, FN, FT
#define WBC_STEP_DUALS 1
#include "wbc_kernel.hip"
