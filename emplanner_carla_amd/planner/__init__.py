"""Drop-in for the reference's ``planner`` package (the modules on the EM-Planner hot path, and global routing).

    from emplanner_carla_amd.planner import path_planning, planning_utils      # instead of `from planner import ...`
    from emplanner_carla_amd.planner.global_planning import global_path_planner

Same module-level function names, positional order, keyword names and defaults as reference
planner/path_planning.py, planner/planning_utils.py, planner/global_planning.py and (S-T speed DP only)
planner/speed_planning_test.py; every numeric result is computed by the HIP kernels behind the C-ABI
(batch size 1).  See INTEGRATION.md.
"""
from . import _runtime  # noqa: F401
from . import global_planning, path_planning, planning_utils, speed_planning_test  # noqa: F401

__all__ = ["global_planning", "path_planning", "planning_utils", "speed_planning_test"]
