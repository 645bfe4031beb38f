// wbc_kernel_rp1.hip — the stateful default step under a per-robot parameter table
// (wbc_update_solve_kernel<1, false, true>, KernelArgs::rp).  A translation unit of
// its own (Makefile RP1_KFLAGS); the code is wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one
// kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_rp1
#define WBC_STEP_INSTANCE 1, false, true, false  // STF, SONLY, RP, CN
#include "wbc_kernel.hip"
