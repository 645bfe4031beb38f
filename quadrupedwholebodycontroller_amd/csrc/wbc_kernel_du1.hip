// wbc_kernel_du1.hip — the stateful default step that also writes the QP multipliers of the friction
// and torque rows (wbc_update_solve_duals_kernel<1, false, true, true, true>, KernelArgs::dual: wbc_step
// with WBC_DUALS, hotstarted or WBC_COLD).  As wbc_kernel_du0.hip: the base-body
// instance's configuration with solve16's DU flag, every table bound by the engine.  A translation unit
// of its own (Makefile DU1_KFLAGS); the code is wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to
// this one kernel and its launcher; WBC_STEP_DUALS names the kernel and turns the multipliers on.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_du1
#define WBC_STEP_INSTANCE 1, false, true, true, true  // STF, SONLY, RP, CN, BB
#define WBC_STEP_DUALS 1
#include "wbc_kernel.hip"
