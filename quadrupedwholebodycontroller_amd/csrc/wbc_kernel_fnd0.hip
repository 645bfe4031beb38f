// wbc_kernel_fnd0.hip — the stateless default step under per-foot normal-force bounds that also writes the QP
// multipliers of the friction, torque and force rows, 48 per robot
// (wbc_update_solve_duals_kernel<0, false, true, true, true, true, true>, KernelArgs::fn and KernelArgs::dual
// as [B][WBC_DUAL_FORCE_LEN]: wbc_step with WBC_DUALS_FORCE).  wbc_kernel_fn0.hip's
// configuration with solve16's DU flag, whose output stage under FN also stores the third slot of lanes 8..15.
// A translation unit of its own (Makefile FND0_KFLAGS); the code is wbc_kernel.hip's, which WBC_STEP_INSTANCE
// limits to this one kernel and its launcher; WBC_STEP_DUALS names the kernel and turns the multipliers on.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_fnd0
#define WBC_STEP_INSTANCE 0, false, true, true, true, true, true  // STF, SONLY, RP, CN, BB, LM, FN
#define WBC_STEP_DUALS 1
#include "wbc_kernel.hip"
