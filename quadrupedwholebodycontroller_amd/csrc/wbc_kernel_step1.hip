// wbc_kernel_step1.hip — the stateful default step (wbc_update_solve_kernel<1>: history, hotstart),
// BASELINE configs[2]'s trot.  A translation unit of its own so that the Makefile can schedule it
// apart from the other kernels (STEP1_KFLAGS: DESIGN.md 4.24); the code is wbc_kernel.hip's, which
// WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_step1
#define WBC_STEP_INSTANCE 1, false, false, false  // STF, SONLY, RP, CN
#include "wbc_kernel.hip"
