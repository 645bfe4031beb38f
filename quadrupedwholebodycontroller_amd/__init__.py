"""quadrupedwholebodycontroller_amd — MI355X-native batched whole-body-control QP engine.

The hot path of the reference's `WholeBodyController` (updateState -> solveQP ->
computeJointTorques, src/whole_body_controller.cpp:650-652) as hand-written HIP for gfx950,
behind the C-ABI in include/wbc.h.  This package is the Python view of that C-ABI:

  Engine          batched handle (wbc_create ... wbc_get_output), see _capi.py; per-robot controller
                  parameters: Engine.set_robot_params / bind_device_robot_params / robot_params;
                  per-robot ground normals at the feet (sloped ground): Engine.set_contact_normals /
                  bind_device_contact_normals / contact_normals;
                  per-robot base body (a payload on the trunk): Engine.set_base_body /
                  bind_device_base_body / base_body, base_body_with_payload;
                  per-robot joint torque bounds and per-foot friction: Engine.set_limits /
                  bind_device_limits / limits, limits_row;
                  per-foot bounds on the normal contact force (load ramps): Engine.set_force_bounds /
                  bind_device_force_bounds / force_bounds, force_bounds_row;
                  per-robot reference contact forces (a force-tracking task in the QP's objective):
                  Engine.set_force_task / bind_device_force_task / force_task, force_task_row;
                  contact-mode hypotheses (set_modes / step_modes) with each hypothesis' QP objective and the
                  best feasible one per state: flags OBJECTIVE / BEST, Engine.objective / best_modes;
                  which constraints bind: flag DUALS on step, Engine.duals / device_duals, dual_rows; under
                  force bounds flag DUALS_FORCE, Engine.force_duals / device_force_duals (48 per robot), under a
                  force task flag DUALS_TASK (the same 48, the same getters)
  Planner         batched motion planner (WbcReferenceMsg producer), see _capi.py
  workloads       synthetic inputs of the BASELINE.json configurations
  sharding        robot shards and the per-step all-gather of the multi-GPU path
  ros_wire        ROS1 wire-byte adapters (libwbc_ros.so)

The WholeBodyController-shaped single-robot shim is C++ (include/wbc_controller.hpp,
libwbc_controller.so), as the reference's class is.

The product path has no CPU fallback: without libwbc_hip.so or a GPU it raises.
"""
from ._capi import (BEST, COLD, DEBUG, DUALS, DUALS_FORCE, DUALS_TASK, DUAL_FORCE_LEN, FUSED, GROUP, NO_X, OBJECTIVE, RESIDENT, SPLIT, STATELESS, TIMED, QP_INFEASIBLE, QP_MAX_ITER, QP_NUMERIC, QP_OK, Engine, WbcError,  # noqa: F401
                    WbcModel, WbcParams, anymal_model, default_params, load_library, model_from_urdf, split_debug, Planner,
                    WbcPlannerParams, ROBOT_PARAM_NAMES, robot_param_table, contact_normal_table,
                    base_body_row, base_body_table, base_body_with_payload, dual_rows, limits_row, limits_table,
                    force_bounds_row, force_bounds_table,
                    force_task_row, force_task_table)

__all__ = ["Engine", "Planner", "WbcPlannerParams", "model_from_urdf", "WbcError", "WbcModel", "WbcParams", "anymal_model", "default_params", "load_library",
           "split_debug", "STATELESS", "DEBUG", "NO_X", "SPLIT", "TIMED", "COLD", "FUSED", "GROUP", "RESIDENT", "OBJECTIVE", "BEST", "DUALS", "DUALS_FORCE", "DUALS_TASK", "DUAL_FORCE_LEN", "QP_OK", "QP_MAX_ITER", "QP_INFEASIBLE", "QP_NUMERIC",
           "ROBOT_PARAM_NAMES", "robot_param_table", "contact_normal_table",
           "base_body_row", "base_body_table", "base_body_with_payload", "dual_rows", "limits_row", "limits_table",
           "force_bounds_row", "force_bounds_table", "force_task_row", "force_task_table"]
