// wbc_kernel_lm0.hip — the stateless default step under per-robot joint torque bounds and per-foot friction
// (wbc_update_solve_kernel<0, false, true, true, true, true>, KernelArgs::lm: wbc_set_limits /
// wbc_bind_device_limits).  A base-body, contact-normal and per-robot-parameter instance
// too (the engine feeds it the model's base, flat normals and its uniform parameters where no such table
// is in force), of any mask mix: an all-stance step runs here as well.  A translation unit of its own (Makefile LM0_KFLAGS); the code is
// wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_lm0
#define WBC_STEP_INSTANCE 0, false, true, true, true, true  // STF, SONLY, RP, CN, BB, LM
#include "wbc_kernel.hip"
