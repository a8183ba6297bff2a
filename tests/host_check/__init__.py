"""Builds and loads the CPU logic-check library (g++).  Test tool only - see host_check.cpp."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_check.cpp")
OUT = os.path.join(HERE, "_build", "libhostcheck.so")
CSRC = os.path.join(HERE, "..", "..", "emplanner_carla_amd", "csrc")


def load():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("emp_core.h", "emp_dp_launch.h", "emp_tail_launch.h", "emp_frenet_core.h", "emp_qp_core.h", "emp_st_core.h", "emp_st_backend_core.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", SRC, "-o", OUT],
                       check=True)
    lib = C.CDLL(OUT)
    d, i, p = C.c_double, C.c_int, C.c_void_p
    lib.hc_segment_cost.restype = d
    lib.hc_segment_cost.argtypes = [d, d, d, d, d, d, p, p, i, d, d, d, d, d]
    lib.hc_neighbour_cost.restype = d
    lib.hc_neighbour_cost.argtypes = [d, d, d, d, p, p, i, d, d, d, d, d]
    lib.hc_path_qp.restype = i
    lib.hc_path_qp.argtypes = [i, p, p, d, d, d, p, p, p, p, p]
    lib.hc_path_qp_gi.restype = i
    lib.hc_path_qp_gi.argtypes = [i, p, p, d, d, d, p, p, p, p, p]
    lib.hc_box_qp.restype = i
    lib.hc_box_qp.argtypes = [i, p, i, d, d, d, d, p, p]
    lib.hc_heading_kappa.restype = None
    lib.hc_heading_kappa.argtypes = [p, i, p, p]
    lib.hc_s_map.restype = None
    lib.hc_s_map.argtypes = [p, i, d, d, p]
    lib.hc_dot2.restype = None
    lib.hc_dot2.argtypes = [i, p, p, p]
    lib.hc_match.restype = i
    lib.hc_match.argtypes = [p, i, d, d, i, i, i]
    lib.hc_proj_point.restype = i
    lib.hc_proj_point.argtypes = [p, p, i, d, p, p]
    lib.hc_walk_from_zero.restype = i
    lib.hc_walk_from_zero.argtypes = [p, i, d, p]
    lib.hc_argmin_abs3.restype = None
    lib.hc_argmin_abs3.argtypes = [p, i, p, p, p]
    lib.hc_lmin_lmax.restype = i
    lib.hc_lmin_lmax.argtypes = [p, p, i, p, p, i, d, d, p, p]
    lib.hc_st_edge_cost.restype = d
    lib.hc_st_edge_cost.argtypes = [p, p, i, p, p, p, p, p]
    lib.hc_st_reach.restype = None
    lib.hc_st_reach.argtypes = [i, d, p, p, p, p, p, p]
    lib.hc_st_graph.restype = None
    lib.hc_st_graph.argtypes = [i] + [p] * 8
    lib.hc_st_grid.restype = None
    lib.hc_st_grid.argtypes = [p, p]
    lib.hc_st_terminal.restype = i
    lib.hc_st_terminal.argtypes = [p, p, p]
    lib.hc_stb_convex_space.restype = i
    lib.hc_stb_convex_space.argtypes = [p, p, p, p, i, p, p, p, p, i, d, p, p, p, p]
    lib.hc_stb_speed_qp.restype = i
    lib.hc_stb_speed_qp.argtypes = [p, p, d, d, p, p, p, p, p, p, p, p, p, p]
    lib.hc_stb_increase_points.restype = i
    lib.hc_stb_increase_points.argtypes = [p] * 8
    lib.hc_stb_np_interp.restype = d
    lib.hc_stb_np_interp.argtypes = [p, p, i, d]
    lib.hc_plan_edge.restype = C.c_char_p
    lib.hc_plan_edge.argtypes = [i] * 7 + [p]
    lib.hc_plan_sweep.restype = C.c_char_p
    lib.hc_plan_sweep.argtypes = [i] * 4 + [p]
    lib.hc_plan_fused.restype = C.c_char_p
    lib.hc_plan_fused.argtypes = [i] * 4 + [p]
    lib.hc_plan_enrich.restype = C.c_char_p
    lib.hc_plan_enrich.argtypes = [i] * 5 + [p]
    lib.hc_edge_tensor_elems.restype = C.c_longlong
    lib.hc_edge_tensor_elems.argtypes = [i] * 4
    lib.hc_edge_ring_constants.restype = None
    lib.hc_edge_ring_constants.argtypes = [i, p]
    lib.hc_dp_layout.restype = i
    lib.hc_dp_layout.argtypes = [C.c_char_p, i, i, i, i, i, p]
    for name, n_args in (("project", 2), ("reference_line", 1), ("cycle_qp", 5), ("cycle_cartesian", 5), ("path_qp", 2), ("smooth", 2),
                         ("speed_front", 2), ("speed_dp", 2), ("st_edge_cost", 3), ("speed_qp", 1), ("merge", 2)):
        fn = getattr(lib, "hc_plan_" + name)
        fn.restype = C.c_char_p
        fn.argtypes = [i] * n_args + [p]
    lib.hc_tail_layout.restype = i
    lib.hc_tail_layout.argtypes = [C.c_char_p, i, i, i, p]
    lib.hc_tail_constants.restype = None
    lib.hc_tail_constants.argtypes = [i, i, p]
    return lib
