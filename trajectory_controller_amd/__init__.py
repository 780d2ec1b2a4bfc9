"""trajectory_controller_amd -- MI355X-native batched MPC-QP solver behind the
TrajectoryPointController module surface of lms-org/trajectory_controller.

Only the hot path lives here: csrc/ holds the gfx950 HIP kernels and the C ABI
(include/tpc_mpc.h -> lib/libtpc_mpc.so); capi.py / solver.py are the host-side binding;
host/ is the C++ module shim that keeps the LMS surface; autograd.py makes the general-form solve and the closed loop torch
autograd functions (their backward passes are the library's gradient kernels; MpcSolver.polish_batch_general moves a
solved sequence onto the verified optimum, MpcSolver.rollout_polished does so inside every step of the closed loop).  Nothing in this package imports
oracle/ -- that directory is the checker used by tests/ and bench.py only.
"""
from .capi import (ALGO_AUTO, ALGO_GROUP, ALGO_LANE, ALGO_LANE_FMA, ALGO_WAVE, F32, F64, FLAG_BAD_MODEL, FLAG_MAX_ITER, FLAG_NONFINITE,
                   FLAG_NOT_POLISHED,                    TpcMpcError, default_params, load_library)
from .solver import COMPACT_PARAM_NAMES, MpcSolver
from .autograd import CompactWarmStart, compact_general_form, mpc_compact, mpc_compact_exact, mpc_general, mpc_rollout, mpc_rollout_compact

__all__ = ["MpcSolver", "mpc_general", "mpc_compact", "mpc_compact_exact", "CompactWarmStart", "mpc_rollout", "mpc_rollout_compact", "compact_general_form", "COMPACT_PARAM_NAMES", "TpcMpcError", "default_params", "load_library", "ALGO_AUTO", "ALGO_WAVE",
           "ALGO_LANE", "ALGO_LANE_FMA", "ALGO_GROUP", "F64", "F32", "FLAG_NONFINITE", "FLAG_MAX_ITER", "FLAG_BAD_MODEL",
           "FLAG_NOT_POLISHED"]
