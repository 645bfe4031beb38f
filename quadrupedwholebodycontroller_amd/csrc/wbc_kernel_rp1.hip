// wbc_kernel_rp1.hip — the stateful default step under a per-robot parameter table
// (wbc_update_solve_kernel<1, false, true>, KernelArgs::rp).  A translation unit of
// its own (Makefile RP1_KFLAGS); the code is wbc_kernel.hip's, which WBC_RP1_TU limits to this one
// kernel and its launcher.
#define WBC_RP1_TU 1
#include "wbc_kernel.hip"
