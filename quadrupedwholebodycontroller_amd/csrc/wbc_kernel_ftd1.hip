// wbc_kernel_ftd1.hip — the stateful default step under per-robot reference contact forces that also writes the
// QP multipliers of the friction, torque and force rows, 48 per robot
// (wbc_update_solve_duals_kernel<1, false, true, true, true, true, true, true>, KernelArgs::ft and KernelArgs::dual
// as [B][WBC_DUAL_FORCE_LEN]: wbc_step with WBC_DUALS_TASK).  wbc_kernel_ft1.hip's
// configuration with solve16's DU flag; the hotstart's direct point solves its 1 x 1 / 2 x 2 system from the reduced
// rows and gradient, which carry the task's w and w fref, and fills its slots as fnd1's does.  A translation unit of
// its own (Makefile FTD1_KFLAGS); the code is wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one kernel
// and its launcher; WBC_STEP_DUALS names the kernel and turns the multipliers on.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_ftd1
#define WBC_STEP_INSTANCE 1, false, true, true, true, true, true, true  // STF, SONLY, RP, CN, BB, LM, FN, FT
#define WBC_STEP_DUALS 1
#include "wbc_kernel.hip"
