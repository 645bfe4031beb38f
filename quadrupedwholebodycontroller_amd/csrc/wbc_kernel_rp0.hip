// wbc_kernel_rp0.hip — the stateless default step under a per-robot parameter table
// (wbc_update_solve_kernel<0, false, true>, KernelArgs::rp: wbc_set_robot_params /
// wbc_bind_device_robot_params), any mask mix, all-stance steps included.  A
// translation unit of its own, as the other one-kernel units: the existing units' code stays as it
// is, and the Makefile schedules this one by itself (RP0_KFLAGS); the code is wbc_kernel.hip's,
// which WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_rp0
#define WBC_STEP_INSTANCE 0, false, true, false  // STF, SONLY, RP, CN
#include "wbc_kernel.hip"
