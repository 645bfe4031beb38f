// wbc_kernel_modes_obj.hip — the mode loop's objective instance (wbc_modes_obj_kernel: wbc_step_modes
// with WBC_OBJECTIVE / WBC_BEST): wbc_modes_kernel's code with the QP objective formed in
// the solve's output stage and stored to KernelArgs::obj.  A translation unit of its own, under the
// mode loop's scheduler flags (Makefile MODES_OBJ_KFLAGS), so that the mode loop's own code object
// stays what it is; WBC_MODES_TU limits wbc_kernel.hip to the one kernel and its launcher,
// WBC_MODES_OBJ names them and turns the objective on.
#define WBC_MODES_TU 1
#define WBC_MODES_OBJ 1
#include "wbc_kernel.hip"
