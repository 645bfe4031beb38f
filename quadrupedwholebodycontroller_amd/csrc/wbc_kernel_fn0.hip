// wbc_kernel_fn0.hip — the stateless default step under per-foot normal-force bounds
// (wbc_update_solve_kernel<0, false, true, true, true, true, true>, KernelArgs::fn: wbc_set_force_bounds /
// wbc_bind_device_force_bounds).  A limits, base-body, contact-normal and per-robot-parameter
// instance too (the engine feeds it the model's base, flat normals and its uniform parameters where no such
// table is in force; without a limits table each robot's own -+max_torque and friction stand), of any mask
// mix: an all-stance step runs here as well.  A translation unit of its own (Makefile FN0_KFLAGS); the code
// is wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_fn0
#define WBC_STEP_INSTANCE 0, false, true, true, true, true, true  // STF, SONLY, RP, CN, BB, LM, FN
#include "wbc_kernel.hip"
