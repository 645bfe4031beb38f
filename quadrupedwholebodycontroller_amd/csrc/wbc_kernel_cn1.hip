// wbc_kernel_cn1.hip — the stateful default step under per-robot contact normals
// (wbc_update_solve_kernel<1, false, true, true>, KernelArgs::cn: wbc_set_contact_normals /
// wbc_bind_device_contact_normals).  A translation unit of its
// own (Makefile CN1_KFLAGS); the code is wbc_kernel.hip's, which WBC_CN1_TU limits to this one kernel
// and its launcher.
#define WBC_CN1_TU 1
#include "wbc_kernel.hip"
