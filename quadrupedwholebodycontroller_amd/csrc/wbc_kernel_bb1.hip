// wbc_kernel_bb1.hip — the stateful default step under a per-robot base body
// (wbc_update_solve_kernel<1, false, true, true, true>, KernelArgs::bb: wbc_set_base_body /
// wbc_bind_device_base_body).  A contact-normal and per-robot-parameter instance too
// (the engine feeds it flat normals and its uniform parameters when no such table is in force).  A
// translation unit of its own (Makefile BB1_KFLAGS); the code is wbc_kernel.hip's, which
// WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_bb1
#define WBC_STEP_INSTANCE 1, false, true, true, true  // STF, SONLY, RP, CN, BB
#include "wbc_kernel.hip"
