// wbc_kernel_cns.hip — the stance-only default step under per-robot contact normals
// (wbc_update_solve_kernel<0, true, true, true>, KernelArgs::cn): a stateless step whose
// QPs all have contact mask 15, the general 12-variable form compiled out, as wbc_kernel_rps.hip.
// A translation unit of its own (Makefile CNS_KFLAGS); the code is wbc_kernel.hip's, which
// WBC_STEP_INSTANCE limits to this one kernel and its launcher.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_cns
#define WBC_STEP_INSTANCE 0, true, true, true  // STF, SONLY, RP, CN
#include "wbc_kernel.hip"
