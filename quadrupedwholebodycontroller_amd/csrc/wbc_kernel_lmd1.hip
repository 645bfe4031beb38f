// wbc_kernel_lmd1.hip — the stateful default step under per-robot torque bounds and per-foot friction that
// also writes the QP multipliers of the friction and torque rows
// (wbc_update_solve_duals_kernel<1, false, true, true, true, true>, KernelArgs::lm and KernelArgs::dual:
// wbc_step with WBC_DUALS while a limits table is in force).  wbc_kernel_lm1.hip's
// configuration with solve16's DU flag.  A translation unit of its own (Makefile LMD1_KFLAGS); the code
// is wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one kernel and its launcher;
// WBC_STEP_DUALS names the kernel and turns the multipliers on.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_lmd1
#define WBC_STEP_INSTANCE 1, false, true, true, true, true  // STF, SONLY, RP, CN, BB, LM
#define WBC_STEP_DUALS 1
#include "wbc_kernel.hip"
