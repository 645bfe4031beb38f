// wbc_kernel_ft1.hip — the stateful default step under per-robot reference contact forces
// (wbc_update_solve_kernel<1, false, true, true, true, true, true, true>, KernelArgs::ft: wbc_set_force_task /
// wbc_bind_device_force_task).  A force-bound, limits, base-body, contact-normal and
// per-robot-parameter instance too (the engine feeds it its no-bounds table, the model's base, flat normals and
// its uniform parameters where no such table is in force; without a limits table each robot's own -+max_torque
// and friction stand).  A translation unit of its own (Makefile FT1_KFLAGS); the code is wbc_kernel.hip's, which
// WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_ft1
#define WBC_STEP_INSTANCE 1, false, true, true, true, true, true, true  // STF, SONLY, RP, CN, BB, LM, FN, FT
#include "wbc_kernel.hip"
