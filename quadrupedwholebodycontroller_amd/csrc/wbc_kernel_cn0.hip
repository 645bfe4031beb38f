// wbc_kernel_cn0.hip — the stateless default step under per-robot contact normals
// (wbc_update_solve_kernel<0, false, true, true>, KernelArgs::cn: wbc_set_contact_normals /
// wbc_bind_device_contact_normals), any mask mix, all-stance steps included.  A translation unit of its
// own (Makefile CN0_KFLAGS); the code is wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one kernel
// and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_cn0
#define WBC_STEP_INSTANCE 0, false, true, true  // STF, SONLY, RP, CN
#include "wbc_kernel.hip"
