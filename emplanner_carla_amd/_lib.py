"""ctypes binding of include/emplanner.h (the C-ABI shared library built by build.py).

There is NO fallback: if ``libemplanner.so`` is missing or cannot be loaded, importing a
planner function raises ``RuntimeError``; if no gfx950 GPU is visible, creating a context
raises ``EmpError``.  Nothing in this package computes planner results on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libemplanner.so")


def configure_hw_queues(n: int = 8) -> bool:
    """Lane mode (emp_set_pipeline with n >= 2) wants one hardware queue per stream; the HIP runtime maps all streams of a
    process onto GPU_MAX_HW_QUEUES queues (default 4) and reads the variable ONCE, when it initialises.  Neither the
    library nor this package touches the process environment on its own: a program that owns its process (bench.py does)
    calls this before anything initialises HIP - before the first torch.cuda call and the first Planner.  Returns False,
    and changes nothing, if the variable is already set."""
    if "GPU_MAX_HW_QUEUES" in os.environ:
        return False
    os.environ["GPU_MAX_HW_QUEUES"] = str(int(n))
    return True


def hw_queues() -> int:
    """The queue count the HIP runtime will use / has used, as far as the environment tells."""
    try:
        return int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    except ValueError:
        return 4


ABI_VERSION = 13                   # EMP_ABI_VERSION of include/emplanner.h this binding speaks

EMP_HOST, EMP_DEVICE, EMP_HOST_PINNED = 0, 1, 2
EMP_EDGE_CANONICAL, EMP_EDGE_TILED = 0, 1
EMP_DP_FUSED, EMP_DP_TWO_KERNEL = 0, 1
EMP_PIPELINE_AUTO, EMP_PIPELINE_STAGED, EMP_PIPELINE_MAX = -1, 1, 8

# emp_option (include/emplanner.h; ABI 11: twelve of them): per-context tuning / A-B / test-hook values
OPTIONS = {"path_qp_form": 0, "cartesian_form": 1, "smooth_force_fallback": 2, "edge_block": 3, "edge_form": 4, "sweep_exclusive": 5,
           "edge_after_enrich": 6, "lane_edge_order": 7, "cycle_graph": 8, "sweep_clock_probe": 9, "edge_clock_probe": 10,
           "foreign_streams": 11}
#: the values a fresh context holds (everything else is 0)
OPTION_DEFAULTS = {"edge_after_enrich": 1, "lane_edge_order": 2, "foreign_streams": 1}

ST_DP_INFEASIBLE = 1
ST_S_OUT_OF_RANGE = 2
ST_BOUND_INDEX = 4
ST_QP_FAILED = 8
ST_SMOOTH_FAILED = 16
ST_TRUNCATED = 32


class EmpError(RuntimeError):
    """A C-ABI call returned a negative emp_error."""


class DpParams(C.Structure):
    _fields_ = [("row", C.c_int32), ("col", C.c_int32), ("sample_s", C.c_double), ("sample_l", C.c_double),
                ("sampling_res", C.c_double), ("w_collision", C.c_double), ("w_smooth", C.c_double * 3),
                ("w_ref", C.c_double)]


class QpParams(C.Structure):
    _fields_ = [("ds", C.c_double), ("w_l", C.c_double), ("w_dl", C.c_double), ("w_ddl", C.c_double),
                ("w_dddl", C.c_double), ("w_centre", C.c_double), ("w_end_l", C.c_double),
                ("w_end_dl", C.c_double), ("w_end_ddl", C.c_double), ("host_d1", C.c_double),
                ("host_d2", C.c_double), ("host_w", C.c_double), ("obs_length", C.c_double),
                ("obs_width", C.c_double), ("decimate", C.c_int32), ("midpoint", C.c_int32),
                ("use_qp", C.c_int32), ("reserved", C.c_int32)]


class SmoothParams(C.Structure):
    _fields_ = [("w_smooth", C.c_double), ("w_length", C.c_double), ("w_ref", C.c_double),
                ("x_thre", C.c_double), ("y_thre", C.c_double)]


class MpcParams(C.Structure):
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("Cf", C.c_double), ("Cr", C.c_double), ("m", C.c_double),
                ("Iz", C.c_double), ("q_diag", C.c_double * 4), ("f_diag", C.c_double * 4), ("r", C.c_double)]


class PidParams(C.Structure):
    """emp_pid_params: the gains of Longitudinal_PID_controller (controller.py:622-638)."""
    _fields_ = [("K_P", C.c_double), ("K_I", C.c_double), ("K_D", C.c_double), ("dt", C.c_double),
                ("error_threshold", C.c_double)]


class VehicleParams(C.Structure):
    """emp_vehicle_params: the project's vehicle model (include/emplanner.h states it in full)."""
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("Cf", C.c_double), ("Cr", C.c_double), ("m", C.c_double),
                ("Iz", C.c_double), ("dt", C.c_double), ("steer_gain", C.c_double), ("throttle_accel", C.c_double),
                ("brake_decel", C.c_double), ("drag", C.c_double), ("reserved", C.c_int32)]


class DriveParams(C.Structure):
    """emp_drive_params: the thresholds of the driver's get_actor_from_world / predict_block (test_9.py:48-89, :335, :377)."""
    _fields_ = [("dis_limitation", C.c_double), ("lateral_band", C.c_double), ("behind", C.c_double),
                ("dynamic_speed", C.c_double), ("static_gate", C.c_double), ("pred_ts", C.c_double), ("advance_s", C.c_double),
                ("reserved", C.c_int32)]


class RolloutTimedIO(C.Structure):
    """emp_rollout_timed_io: emp_rollout's arrays, the timed trajectory, the clock and the cursor."""
    _fields_ = [(n, C.c_void_p) for n in (
        "target_path", "n_path", "state", "min_index", "target_speed", "err_in", "n_err_in", "trajectory", "t0", "cursor_in",
        "state_out", "min_index_out", "err_out", "n_err_out", "status", "fail_tick", "cursor_out", "tgt_status",
        "log_state", "log_control", "log_err", "log_index", "log_target")] + [("reserved", C.c_int32)]


TGT_BEFORE, TGT_PAST, TGT_NO_PROFILE, TGT_CAPPED = 1, 2, 4, 8     # EMP_TGT_*
TIMED_POINTS = 401                 # EMP_TIMED_POINTS
DRIVE_MAX_PERIODS = 4096           # EMP_DRIVE_MAX_PERIODS
DRV_TRUNCATED = 1                  # EMP_DRV_TRUNCATED
ROLLOUT_MAX_TICKS = 65536          # EMP_ROLLOUT_MAX_TICKS
PID_BUFFER = 60                    # EMP_PID_BUFFER: the error deque's maxlen (controller.py:637)
MPC_FF_CONTROLS = 8                # EMP_MPC_FF_CONTROLS
EMP_LAT_MPC, EMP_LAT_LQR = 0, 1


class SpeedQpParams(C.Structure):
    """emp_speed_qp_params: keyword arguments of the reference's speed_QP (speed_planning_test.py:410-411)."""
    _fields_ = [("w_cost_s_dot2", C.c_double), ("w_cost_v_ref", C.c_double), ("w_cost_jerk", C.c_double),
                ("reference_speed", C.c_double)]


class SpeedDpParams(C.Structure):
    _fields_ = [("reference_speed", C.c_double), ("w_cost_ref_speed", C.c_double), ("w_cost_accel", C.c_double),
                ("w_cost_obs", C.c_double)]


_vp, _i32, _f64, _u64 = C.c_void_p, C.c_int32, C.c_double, C.c_uint64

ROUTE_MAX_NODES = 4096             # EMP_ROUTE_MAX_NODES
ROUTE_MAX_LENGTH = 1 << 18         # EMP_ROUTE_MAX_LENGTH
ROUTE_UNREACHABLE, ROUTE_TRUNCATED, ROUTE_BAD_QUERY = 1, 2, 4     # EMP_ROUTE_*


class RouteGraph(C.Structure):
    """emp_route_graph: the road graph of global routing (routing.RoadGraph fills it)."""
    _fields_ = [(n, _vp) for n in ("vertex", "succ_off", "succ", "length", "wp_off", "wp")] + \
               [("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("n_wp", C.c_int32), ("reserved", C.c_int32)]


AGENT_BUFFER = 10                  # EMP_AGENT_BUFFER: the agents' two error deques (agents/navigation/controller.py:124, :193)
AGT_DONE = 1                       # EMP_AGT_DONE


class AgentParams(C.Structure):
    """emp_agent_params: the gains and limits of LocalPlanner / VehiclePIDController (local_planner.py:70-79)."""
    _fields_ = [(n, C.c_double) for n in ("lat_K_P", "lat_K_I", "lat_K_D", "lon_K_P", "lon_K_I", "lon_K_D", "dt", "max_throttle",
                                          "max_brake", "max_steer", "base_min_distance")] + [("reserved", C.c_int32)]


class AgentRolloutIO(C.Structure):
    """emp_agent_rollout_io: the path, the vehicle and agent state in and out, the logs."""
    _fields_ = [(n, _vp) for n in (
        "path", "n_path", "state", "target_speed", "head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat",
        "state_out", "head_out", "past_steer_out", "lon_err_out", "n_lon_out", "lat_err_out", "n_lat_out", "status", "done_tick",
        "actors_out", "log_state", "log_control", "log_head")] + [("reserved", C.c_int32)]


TRAFFIC_MAX_WORLD = 64             # EMP_TRAFFIC_MAX_WORLD: agents of a world, and others of a world
BHV_NORMAL, BHV_SLOW, BHV_FOLLOW, BHV_CLEAR, BHV_EMERGENCY, BHV_DONE = range(6)       # EMP_BHV_*: the mode of a tick
BHV_KINDS = {"cautious": 0, "normal": 1, "aggressive": 2}                            # EMP_BHV_CAUTIOUS, _KIND_NORMAL, _AGGRESSIVE


class BehaviorParams(C.Structure):
    """emp_behavior_params: behavior_types.py plus the constants of BehaviorAgent's car-following."""
    _fields_ = [(n, C.c_double) for n in ("max_speed", "speed_lim_dist", "speed_decrease", "safety_time", "min_proximity_threshold",
                                          "braking_distance", "min_speed", "emergency_brake", "up_angle")] + \
               [("look_steps", C.c_int32), ("reserved", C.c_int32)]


class BehaviorIO(C.Structure):
    """emp_behavior_io: the arrays of emp_agent_behave and emp_traffic_rollout."""
    _fields_ = [(n, _vp) for n in (
        "n_world", "path", "n_path", "lane", "state", "forward", "speed_kmh", "speed_limit", "extent", "head", "past_steer", "lon_err",
        "n_lon", "lat_err", "n_lat", "n_other", "other", "other_lane", "head_out", "past_steer_out", "lon_err_out", "n_lon_out",
        "lat_err_out", "n_lat_out", "status", "control", "mode", "blocker", "distance", "ttc", "target_speed_out", "lat_error",
        "lon_command", "state_out", "done_tick", "mode_ticks", "min_gap", "actors_out", "log_state", "log_control", "log_head",
        "log_mode", "log_target")] + [("reserved", C.c_int32)]


HAZARD_MAX = 64                    # EMP_HAZARD_MAX: lights of a world, and walkers of a world
HZ_NONE, HZ_LIGHT, HZ_WALKER, HZ_VEHICLE = range(4)      # EMP_HZ_*: why a tick is EMERGENCY


class HazardParams(C.Structure):
    """emp_hazard_params: the thresholds of BasicAgent._affected_by_traffic_light and pedestrian_avoid_manager."""
    _fields_ = [(n, C.c_double) for n in ("tlight_threshold", "tlight_up_angle", "walker_radius", "walker_up_angle")] + \
               [("reserved", C.c_int32)]


class HazardIO(C.Structure):
    """emp_hazard_io: what emp_agent_behave_hazards and emp_traffic_rollout_hazards add to emp_behavior_io."""
    _fields_ = [(n, _vp) for n in (
        "n_light", "light", "light_lane", "light_cycle", "n_walker", "walker", "walker_lane", "last_light", "last_light_out", "cause",
        "light_hit", "walker_hit", "walker_distance", "cause_ticks", "min_walker_gap", "log_cause")] + [("reserved", C.c_int32)]


WX_ACT_TRUNCATED, WX_NOT_LISTED, WX_NO_WORLD = 1, 2, 4       # EMP_WX_*: bits of emp_world_exchange's wx_status


class WorldExchangeIO(C.Structure):
    """emp_world_exchange_io: both fleets' states in, who sees whom out."""
    _fields_ = [(n, _vp) for n in (
        "n_world", "agent_state", "ego_off", "ego_state", "ego_extent", "global_path", "n_global", "ego_lane", "pre_match_index",
        "actors", "n_act", "other", "other_lane", "n_other", "wx_status")] + [("reserved", C.c_int32)]


class WorldParams(C.Structure):
    """emp_world_params: the traffic's sizes, the agents' clock and the exchange's two settings in emp_world_drive."""
    _fields_ = [(n, C.c_int32) for n in ("W", "max_world", "max_path", "max_other", "max_light", "max_walker", "Ta", "lane_window",
                                         "see_egos", "reserved")] + [("atick0", C.c_int64)]


class WorldIO(C.Structure):
    """emp_world_io: emp_drive_timed_io without actors and n_act, the exchange's ego arrays, the traffic's two structs, the logs."""
    _fields_ = [(n, _vp) for n in (
        "global_path", "n_global", "state", "accel", "pre_match_index", "track", "track_len", "held", "t0", "profile", "cursor",
        "speed_held", "ego_off", "ego_extent", "ego_lane",
        "state_out", "accel_out", "actors_out", "pre_match_index_out", "track_out", "track_len_out", "held_out", "profile_out",
        "cursor_out", "speed_held_out",
        "log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len", "log_speed_status",
        "log_speed_held", "log_tgt_status", "log_cursor", "log_profile")] + \
        [("agents", C.POINTER(BehaviorIO)), ("hazards", C.POINTER(HazardIO))] + \
        [(n, _vp) for n in ("log_wx_status", "log_n_act", "log_agent_state", "log_agent_status", "log_done_tick", "log_mode_ticks",
                            "log_cause_ticks", "log_min_gap", "log_min_walker_gap")] + [("reserved", C.c_int32)]


class CycleIO(C.Structure):
    _fields_ = [(n, _vp) for n in (
        "ref_line", "n_ref", "origin_xy", "start_xy", "start_v", "start_a", "obs_xy", "n_obs",
        "dp_rows", "dp_s", "dp_l", "dp_len", "path_s", "path_l", "path_len", "traj", "traj_len", "status",
        "dyn_dis_speed",
        # the optional front end (ABI 11): the cycle starts from the global path
        "global_path", "n_global", "pre_match_index", "match_index", "ref_status")] + [("max_global", C.c_int32), ("reserved_io", C.c_int32)]


class SpeedIO(C.Structure):
    """emp_speed_io (ABI 13): the speed half of emp_plan_trajectory."""
    _fields_ = [(n, _vp) for n in (
        "dyn_obs", "n_dyn", "start_heading", "plan_start_time", "dyn_pre_match",
        "trajectory", "speed_status", "path_index2s", "st_segments", "dp_speed", "speed_profile")] + [("reserved", C.c_int32)]


class DriveIO(C.Structure):
    """emp_drive_io: the arrays of emp_drive - inputs, the in/out state's outputs, per-period logs."""
    _fields_ = [(n, _vp) for n in (
        "global_path", "n_global", "state", "accel", "actors", "n_act", "pre_match_index", "track", "track_len", "held",
        "state_out", "accel_out", "actors_out", "pre_match_index_out", "track_out", "track_len_out", "held_out",
        "log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len")] + [("reserved", C.c_int32)]


class DriveTimedParams(C.Structure):
    """emp_drive_timed_params: what emp_drive_timed adds to the parameter blocks of emp_drive and emp_plan_trajectory."""
    _fields_ = [("plan_lead", C.c_double), ("reserved", C.c_int32)]


class DriveTimedIO(C.Structure):
    """emp_drive_timed_io: emp_drive_io's arrays under their names, the clock, the profile with its cursor and counter, their logs."""
    _fields_ = [(n, _vp) for n in (
        "global_path", "n_global", "state", "accel", "actors", "n_act", "pre_match_index", "track", "track_len", "held",
        "t0", "profile", "cursor", "speed_held",
        "state_out", "accel_out", "actors_out", "pre_match_index_out", "track_out", "track_len_out", "held_out",
        "profile_out", "cursor_out", "speed_held_out",
        "log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len",
        "log_speed_status", "log_speed_held", "log_tgt_status", "log_cursor", "log_profile")] + [("reserved", C.c_int32)]


# name -> (restype, argtypes); data pointers are void* so numpy arrays and raw device addresses both fit
PROTOTYPES = {
    "emp_abi_version": (C.c_int, []),
    "emp_dp_params_default": (None, [C.POINTER(DpParams)]),
    "emp_qp_params_default": (None, [C.POINTER(QpParams)]),
    "emp_smooth_params_default": (None, [C.POINTER(SmoothParams)]),
    "emp_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "emp_destroy": (None, [_vp]),
    "emp_last_error": (C.c_char_p, [_vp]),
    "emp_synchronize": (C.c_int, [_vp]),
    "emp_stream": (_vp, [_vp]),
    "emp_host_alloc": (C.c_int, [_vp, _u64, C.POINTER(_vp)]),
    "emp_host_free": (C.c_int, [_vp, _vp]),
    "emp_wait_cycle": (C.c_int, [_vp, _i32]),
    "emp_cycle_ticket": (_u64, [_vp]),
    "emp_wait_ticket": (C.c_int, [_vp, _u64]),
    "emp_device_alloc": (C.c_int, [_vp, _u64, C.POINTER(_vp)]),
    "emp_device_free": (C.c_int, [_vp, _vp]),
    "emp_copy_to_device": (C.c_int, [_vp, _vp, _vp, _u64]),
    "emp_copy_to_host": (C.c_int, [_vp, _vp, _vp, _u64]),
    "emp_set_timing": (C.c_int, [_vp, C.c_int]),
    "emp_set_timing_filter": (C.c_int, [_vp, C.c_char_p]),
    "emp_set_pipeline": (C.c_int, [_vp, C.c_int]),
    "emp_result_stream": (_vp, [_vp]),
    "emp_pipeline_depth": (C.c_int, [_vp]),
    "emp_pipeline_form": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "emp_set_fence": (C.c_int, [_vp, C.c_int]),
    "emp_set_option": (C.c_int, [_vp, _i32, _i32]),
    "emp_get_option": (C.c_int, [_vp, _i32, C.POINTER(_i32)]),
    "emp_sweep_clock_mhz": (_f64, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "emp_cycle_graph_replays": (C.c_int64, [_vp]),
    "emp_edge_probe": (C.c_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_i32)]),
    "emp_edge_clock_mhz": (_f64, [_vp]),
    "emp_sweep_probe_spans": (C.c_int, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "emp_pack_records": (C.c_int, [_vp, _i32, _i32, _i32, _i32] + [_vp] * 8 + [C.c_int, C.c_int]),
    "emp_pack_trajectory_records": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 4 + [C.c_int, C.c_int]),
    "emp_kernel_ms": (_f64, [_vp, C.c_char_p]),
    "emp_kernel_launches": (C.c_int, [_vp, C.c_char_p]),
    "emp_kernel_samples": (C.c_int, [_vp, C.c_char_p, _vp, _i32]),
    "emp_edge_tensor_elems": (_u64, [C.POINTER(DpParams), _i32, C.c_int]),
    "emp_dp_edge_costs": (C.c_int, [_vp, C.POINTER(DpParams), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                    C.c_int]),
    "emp_dp_plan": (C.c_int, [_vp, C.POINTER(DpParams), _i32, _i32, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp,
                              C.c_int]),
    "emp_dp_sweep": (C.c_int, [_vp, C.POINTER(DpParams), _i32, _vp, _vp, _vp, _vp, _vp, C.c_int]),
    "emp_dp_enrich": (C.c_int, [_vp, C.POINTER(DpParams), _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, C.c_int]),
    "emp_enrich_nodes": (C.c_int, [_vp, _i32, _i32, _f64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, C.c_int]),
    "emp_frenet_project": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 13 + [C.c_int]),
    "emp_match_projection": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 6 + [C.c_int]),
    "emp_find_match_points": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 8 + [C.c_int]),
    "emp_heading_kappa": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, C.c_int]),
    "emp_lmin_lmax": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 6 + [_f64, _f64, _vp, _vp, _vp, C.c_int]),
    "emp_path_qp": (C.c_int, [_vp, C.POINTER(QpParams), _i32, _i32] + [_vp] * 9 + [C.c_int]),
    "emp_smooth_line": (C.c_int, [_vp, C.POINTER(SmoothParams), _i32, _i32] + [_vp] * 5 + [C.c_int]),
    "emp_frenet_path_to_xy": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 10 + [C.c_int]),
    "emp_plan_cycle": (C.c_int, [_vp, C.POINTER(DpParams), C.POINTER(QpParams), C.POINTER(SmoothParams), _i32, _i32,
                                 _i32, _i32, C.c_int, C.POINTER(CycleIO), C.c_int]),
    "emp_s_map": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, C.c_int]),
    "emp_s_l": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 8 + [C.c_int]),
    "emp_s_l_deri": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 8 + [C.c_int]),
    "emp_proj_point": (C.c_int, [_vp, _i32, _i32] + [_vp] * 8 + [C.c_int]),
    "emp_trajectory_index2s": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, C.c_int]),
    "emp_frenet2cartesian": (C.c_int, [_vp, _i32, _i32, _i32] + [_vp] * 7 + [_i32, C.c_int]),
    "emp_dy_obs_deri": (C.c_int, [_vp, _i32, _vp, _vp, C.c_int]),
    "emp_quintic_coefficients": (C.c_int, [_vp, _i32, _vp, _vp, C.c_int]),
    "emp_obs_cost": (C.c_int, [_vp, _i32, _f64, _f64, _f64, _vp, _vp, C.c_int]),
    "emp_obs_cost_n": (C.c_int, [_vp, _i32, _i32, _f64, _f64, _f64, _vp, _vp, C.c_int]),
    "emp_free_edge_costs": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _f64, C.POINTER(_f64), _f64, _vp, C.c_int]),
    "emp_reference_line": (C.c_int, [_vp, C.POINTER(SmoothParams), _i32, _i32] + [_vp] * 10 + [C.c_int]),
    "emp_mpc_params_default": (None, [C.POINTER(MpcParams)]),
    "emp_mpc_lateral": (C.c_int, [_vp, C.POINTER(MpcParams), _i32, _i32] + [_vp] * 15 + [C.c_int]),
    "emp_lqr_params_default": (None, [C.POINTER(MpcParams)]),
    "emp_lqr_lateral": (C.c_int, [_vp, C.POINTER(MpcParams), _i32, _i32] + [_vp] * 13 + [C.c_int]),
    "emp_pid_params_default": (None, [C.POINTER(PidParams)]),
    "emp_pid_longitudinal": (C.c_int, [_vp, C.POINTER(PidParams), _i32] + [_vp] * 7 + [C.c_int]),
    "emp_mpc_ff_params_default": (None, [C.POINTER(MpcParams)]),
    "emp_mpc_ff_lateral": (C.c_int, [_vp, C.POINTER(MpcParams), _i32, _i32] + [_vp] * 15 + [C.c_int]),
    "emp_vehicle_control": (C.c_int, [_vp, _i32, C.POINTER(MpcParams), C.POINTER(PidParams), _i32, _i32] + [_vp] * 19
                            + [C.c_int]),
    "emp_vehicle_params_default": (None, [C.POINTER(VehicleParams)]),
    "emp_vehicle_step": (C.c_int, [_vp, C.POINTER(VehicleParams), _i32] + [_vp] * 6 + [C.c_int]),
    "emp_rollout": (C.c_int, [_vp, _i32, C.POINTER(MpcParams), C.POINTER(PidParams), C.POINTER(VehicleParams), _i32, _i32]
                    + [_vp] * 7 + [_i32, _i32] + [_vp] * 10 + [C.c_int]),
    "emp_speed_target": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _f64] + [_vp] * 5 + [C.c_int]),
    "emp_rollout_timed": (C.c_int, [_vp, _i32, C.POINTER(MpcParams), C.POINTER(PidParams), C.POINTER(VehicleParams)] + [_i32] * 5
                          + [C.POINTER(RolloutTimedIO), C.c_int]),
    "emp_drive_params_default": (None, [C.POINTER(DriveParams)]),
    "emp_drive_request": (C.c_int, [_vp, C.POINTER(DriveParams), _i32, _i32, _i32, _i32] + [_vp] * 18 + [C.c_int]),
    "emp_drive": (C.c_int, [_vp, C.POINTER(DpParams), C.POINTER(QpParams), C.POINTER(SmoothParams), C.POINTER(DriveParams), _i32,
                            C.POINTER(MpcParams), C.POINTER(PidParams), C.POINTER(VehicleParams)] + [_i32] * 8
                  + [_vp, C.POINTER(DriveIO), C.c_int]),
    "emp_drive_timed_params_default": (None, [C.POINTER(DriveTimedParams)]),
    "emp_drive_request_timed": (C.c_int, [_vp, C.POINTER(DriveParams), _i32, _i32, _i32, _i32] + [_vp] * 5 + [_i32, _f64, _f64]
                                + [_vp] * 17 + [C.c_int]),
    "emp_drive_timed": (C.c_int, [_vp, C.POINTER(DpParams), C.POINTER(QpParams), C.POINTER(SmoothParams), C.POINTER(SpeedDpParams),
                                  C.POINTER(SpeedQpParams), C.POINTER(DriveParams), C.POINTER(DriveTimedParams), _i32,
                                  C.POINTER(MpcParams), C.POINTER(PidParams), C.POINTER(VehicleParams)] + [_i32] * 9
                        + [_vp, C.POINTER(DriveTimedIO), C.c_int]),
    "emp_speed_dp_params_default": (None, [C.POINTER(SpeedDpParams)]),
    "emp_st_graph": (C.c_int, [_vp, _i32, _i32] + [_vp] * 8 + [C.c_int]),
    "emp_speed_dp": (C.c_int, [_vp, C.POINTER(SpeedDpParams), _i32, _i32] + [_vp] * 11 + [C.c_int]),
    "emp_st_edge_costs": (C.c_int, [_vp, C.POINTER(SpeedDpParams), _i32, _i32, _i32] + [_vp] * 7 + [C.c_int]),
    "emp_st_collision_cost": (C.c_int, [_vp, _i32, _f64, _vp, _vp, C.c_int]),
    "emp_speed_start_condition": (C.c_int, [_vp, _i32] + [_vp] * 7 + [C.c_int]),
    "emp_speed_qp_params_default": (None, [C.POINTER(SpeedQpParams)]),
    "emp_speed_convex_space": (C.c_int, [_vp, _i32, _i32, _i32, _f64] + [_vp] * 14 + [C.c_int]),
    "emp_speed_qp": (C.c_int, [_vp, C.POINTER(SpeedQpParams), _i32] + [_vp] * 14 + [C.c_int]),
    "emp_speed_increase_points": (C.c_int, [_vp, _i32] + [_vp] * 9 + [C.c_int]),
    "emp_path_speed_merge": (C.c_int, [_vp, _i32, _i32] + [_vp] * 13 + [C.c_int]),
    "emp_plan_trajectory": (C.c_int, [_vp, C.POINTER(DpParams), C.POINTER(QpParams), C.POINTER(SmoothParams),
                                      C.POINTER(SpeedDpParams), C.POINTER(SpeedQpParams), _i32, _i32, _i32, _i32, _i32,
                                      C.c_int, C.POINTER(CycleIO), C.POINTER(SpeedIO), C.c_int]),
    "emp_route_search": (C.c_int, [_vp, C.POINTER(RouteGraph), _i32, _i32] + [_vp] * 5 + [C.c_int]),
    "emp_route_paths": (C.c_int, [_vp, C.POINTER(RouteGraph), _i32, _i32, _i32] + [_vp] * 10 + [C.c_int]),
    "emp_agent_params_default": (None, [C.POINTER(AgentParams)]),
    "emp_agent_observe": (C.c_int, [_vp, _i32] + [_vp] * 4 + [C.c_int]),
    "emp_agent_control": (C.c_int, [_vp, C.POINTER(AgentParams), _i32, _i32] + [_vp] * 22 + [C.c_int]),
    "emp_agent_rollout": (C.c_int, [_vp, C.POINTER(AgentParams), C.POINTER(VehicleParams), _i32, _i32, _i32, _i32,
                                    C.POINTER(AgentRolloutIO), C.c_int]),
    "emp_behavior_params_default": (None, [C.POINTER(BehaviorParams), _i32]),
    "emp_agent_behave": (C.c_int, [_vp, C.POINTER(AgentParams), C.POINTER(BehaviorParams), _i32, _i32, _i32, _i32, C.c_int64,
                                   C.POINTER(BehaviorIO), C.c_int]),
    "emp_traffic_rollout": (C.c_int, [_vp, C.POINTER(AgentParams), C.POINTER(BehaviorParams), C.POINTER(VehicleParams), _i32, _i32, _i32,
                                      _i32, _i32, _i32, C.c_int64, C.POINTER(BehaviorIO), C.c_int]),
    "emp_hazard_params_default": (None, [C.POINTER(HazardParams)]),
    "emp_agent_behave_hazards": (C.c_int, [_vp, C.POINTER(AgentParams), C.POINTER(BehaviorParams), _i32, _i32, _i32, _i32, C.c_int64,
                                           C.POINTER(BehaviorIO), C.c_int, C.POINTER(HazardParams), _i32, _i32, C.POINTER(HazardIO)]),
    "emp_traffic_rollout_hazards": (C.c_int, [_vp, C.POINTER(AgentParams), C.POINTER(BehaviorParams), C.POINTER(VehicleParams), _i32, _i32,
                                              _i32, _i32, _i32, _i32, C.c_int64, C.POINTER(BehaviorIO), C.c_int, C.POINTER(HazardParams),
                                              _i32, _i32, C.POINTER(HazardIO)]),
    "emp_world_exchange": (C.c_int, [_vp] + [_i32] * 8 + [C.POINTER(WorldExchangeIO), C.c_int]),
    "emp_traffic_rollout_epoch": (C.c_int, [_vp, C.POINTER(AgentParams), C.POINTER(BehaviorParams), C.POINTER(VehicleParams), _i32, _i32,
                                            _i32, _i32, _i32, _i32, C.c_int64, C.POINTER(BehaviorIO), C.c_int, C.POINTER(HazardParams),
                                            _i32, _i32, C.POINTER(HazardIO), C.c_int64]),
    "emp_world_params_default": (None, [C.POINTER(WorldParams)]),
    "emp_world_drive": (C.c_int, [_vp, C.POINTER(DpParams), C.POINTER(QpParams), C.POINTER(SmoothParams), C.POINTER(SpeedDpParams),
                                  C.POINTER(SpeedQpParams), C.POINTER(DriveParams), C.POINTER(DriveTimedParams), _i32,
                                  C.POINTER(MpcParams), C.POINTER(PidParams), C.POINTER(VehicleParams), C.POINTER(AgentParams),
                                  C.POINTER(BehaviorParams), C.POINTER(VehicleParams), C.POINTER(HazardParams), C.POINTER(WorldParams)]
                        + [_i32] * 9 + [_vp, C.POINTER(WorldIO), C.c_int]),
}

_lib = None


def load():
    """Load the shared library once; raise loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (soname libamdhip64.so.7, the
    # same as /opt/rocm's).  If torch is imported AFTER this library, the loader maps a second copy and that
    # copy finds no GPU.  Importing torch first makes our DT_NEEDED resolve to the already-loaded runtime.
    if "torch" not in sys.modules and os.environ.get("EMP_SKIP_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m emplanner_carla_amd.build` "
            "(hipcc, gfx950).  This package has no CPU implementation to fall back to.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)   # AttributeError here means header and library disagree
        fn.restype = res
        fn.argtypes = args
    if lib.emp_abi_version() != ABI_VERSION:
        raise RuntimeError("libemplanner.so ABI version mismatch")
    _lib = lib
    return lib
