// wbc_kernel_du0.hip — the stateless default step that also writes the QP multipliers of the friction
// and torque rows (wbc_update_solve_duals_kernel<0, false, true, true, true>, KernelArgs::dual: wbc_step
// with WBC_DUALS, wbc_get_duals / wbc_device_duals).  The base-body instance's
// configuration with solve16's DU flag: the engine binds all three tables (its uniform parameters, flat
// normals and default base-body rows where the caller has none), so the one unit serves every table
// combination and every mask mix, all-stance steps included.  A translation unit of its own (Makefile
// DU0_KFLAGS); the code is wbc_kernel.hip's, which WBC_STEP_INSTANCE limits to this one kernel and its
// launcher; WBC_STEP_DUALS names the kernel and turns the multipliers on.
#define WBC_STEP_LAUNCHER wbc_launch_update_solve_du0
#define WBC_STEP_INSTANCE 0, false, true, true, true  // STF, SONLY, RP, CN, BB
#define WBC_STEP_DUALS 1
#include "wbc_kernel.hip"
