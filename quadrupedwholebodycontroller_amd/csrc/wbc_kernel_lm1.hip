// wbc_kernel_lm1.hip — the stateful default step under per-robot joint torque bounds and per-foot friction
// (wbc_update_solve_kernel<1, false, true, true, true, true>, KernelArgs::lm: wbc_set_limits /
// wbc_bind_device_limits).  A base-body, contact-normal and per-robot-parameter instance
// too (the engine feeds it the model's base, flat normals and its uniform parameters where no such table
// is in force).  A translation unit of its own (Makefile LM1_KFLAGS); the code is
// wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_lm1
#define WBC_STEP_INSTANCE 1, false, true, true, true, true  // STF, SONLY, RP, CN, BB, LM
#include "wbc_kernel.hip"
