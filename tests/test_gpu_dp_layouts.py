"""GPU parity at the edges of the DP kernels' LDS layouts (csrc/emp_dp_launch.h: edge_lds, edge_ring_lds, sweep_lds, enrich_lds,
fused_lds) that the other DP tests do not reach: shapes where the per-wavefront arrays are many, idle, or cut short.

Each case is picked through the launch plan (tests/host_check: hc_plan_edge, hc_plan_fused), and what the case is there for is
asserted on the plan first, on the CPU side.  Bar: bit for bit against oracle/exact.py.  The kernels are bit-identical for any
geometry, so a slip in a layout would show here only as a wrong or a faulting read at these shapes - small ones, chosen so.
"""
import numpy as np
import pytest

from oracle import exact as ex
from tests.test_gpu_edge_masks import _live_tiled, _scenes

pytestmark = pytest.mark.gpu

LDS_CU = 160 * 1024
EDGE_FIELDS = ("wide", "ring", "m32", "row_inst", "wpb", "cpc", "grid_x", "grid_y", "block", "lds")


@pytest.fixture(scope="module")
def planner():
    from emplanner_carla_amd.api import Planner
    p = Planner(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def hc():
    from tests import host_check
    return host_check.load()


def _edge_plan(hc, row, col, B, max_obs, tiled, form, block):
    out = np.zeros(len(EDGE_FIELDS), dtype=np.int64)
    assert hc.hc_plan_edge(row, col, B, max_obs, tiled, form, block, out.ctypes.data) is None
    return dict(zip(EDGE_FIELDS, out.tolist()))


def _lockstep_wide_rows(p, case):
    # 32 rows with 254 obstacle slots: the table and the obstacle rows take 131 KB, and the block has sixteen wavefronts for two
    # columns - fourteen of them idle, each with a box array of its own, 64 terms a scene where the slots are 254.  (Under the
    # pinned plans this block is NOT shrunk by the LDS: a wavefront's box terms stop at the mask's 64 bits, 1 KB.)
    assert not p["ring"] and not p["m32"] and p["wpb"] == 16 > case[1] - 1 and p["cpc"] == 16
    assert p["lds"] > 0.9 * LDS_CU and p["lds"] == (15 * 32 * 32 + 2 * 2 * 254 + 15 + 16 * 2 * 64) * 8


def _lockstep_shrunk(p, case):
    # one row: 64 scenes a tile, whose obstacle rows fill the LDS - four wavefronts were asked for, two fit
    assert not p["ring"] and p["wpb"] == 2 < case[8] // 64 and p["lds"] <= LDS_CU < p["lds"] + 64 * 64 * 8


def _ring_idle_wavefronts(p, case):
    # sixteen wavefronts, five columns: eleven never enter the column loop, every one owns its bands, rings and one jerk factor row
    assert p["ring"] and p["m32"] and p["wpb"] == 16 > case[1] - 1 and p["cpc"] == 16 and p["grid_y"] == 1


def _ring_partial_chunk(p, case):
    # 8-byte masks, two wavefronts, two columns a chunk, seven columns: the last chunk has one, its second wavefront none
    assert p["ring"] and not p["m32"] and 32 < case[5] <= 64 and p["wpb"] == 2 and p["cpc"] == 2
    assert (case[1] - 1) % p["cpc"] != 0 and p["grid_y"] * p["cpc"] > case[1] - 1


# (row, col, sample_s, sample_l, n_obs, max_obs, scenes, edge_form, edge_block, what the plan must show)
EDGE_CASES = [
    (32, 3, 5.0, 0.4, 254, 254, 3, 0, 0, _lockstep_wide_rows),
    (1, 4, 5.0, 1.5, 64, 64, 70, 1, 256, _lockstep_shrunk),
    (9, 6, 2.5, 1.5, 8, 8, 45, 0, 1024, _ring_idle_wavefronts),
    (5, 8, 5.0, 1.0, 40, 40, 25, 0, 128, _ring_partial_chunk),
]


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: c[9].__name__.lstrip("_"))
def test_edge_costs_at_the_layouts_edges(planner, hc, case):
    from emplanner_carla_amd import _lib as L
    from emplanner_carla_amd.api import dp_params
    row, col, ss, sl, n_obs, max_obs, B, form, block, check = case
    for tiled in (0, 1):
        check(_edge_plan(hc, row, col, B, max_obs, tiled, form, block), case)
    obs_s, obs_l, nob, start = _scenes(row, col, ss, sl, n_obs, max_obs, B, seed=row * 7919 + col * 31 + max_obs)
    p = dp_params(row=row, col=col, sample_s=ss, sample_l=sl)
    planner.set_option("edge_form", form)
    planner.set_option("edge_block", block)
    try:
        c0, e = planner.dp_edge_costs(p, obs_s, obs_l, nob, start, layout=L.EMP_EDGE_CANONICAL)
        c0t, et = planner.dp_edge_costs(p, obs_s, obs_l, nob, start, layout=L.EMP_EDGE_TILED)
    finally:
        planner.set_option("edge_form", 0)
        planner.set_option("edge_block", 0)
    rc0, re = ex.edge_costs(obs_s, obs_l, nob, start, row, col, ss, sl)
    assert np.array_equal(c0, rc0) and np.array_equal(c0t, rc0), "start edges"
    assert np.array_equal(e, re), f"canonical layout: {(e != re).sum()} of {re.size} edges differ from the exact oracle"
    from emplanner_carla_amd.api import tile_edges
    assert np.array_equal(_live_tiled(et, row, col, B), _live_tiled(tile_edges(re, row), row, col, B)), "tiled layout"
    _, clear = ex.edge_costs(obs_s, obs_l, np.zeros(B, np.int32), start, row, col, ss, sl)
    assert (re != clear).any()                              # not a vacuous comparison: some pair in reach costs something


# (row, col, sample_s, sample_l, n_obs, max_obs, scenes, the chunk size plan_fused must come down to)
FUSED_CASES = [
    (12, 10, 5.0, 1.5, 32, 32, 13, 2),        # halved once; nine columns in chunks of two: the last chunk holds one
    (21, 8, 1.0, 0.6, 16, 16, 7, 1),          # halved twice: one column a chunk, three wavefronts of four idle in the costing
]


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: f"{c[1]}x{c[0]}_nc{c[7]}")
def test_fused_dp_where_the_plan_halves_its_chunk(planner, hc, case):
    from emplanner_carla_amd.api import dp_params
    row, col, ss, sl, n_obs, max_obs, B, nc = case
    f = np.zeros(2, dtype=np.int64)
    assert hc.hc_plan_fused(row, col, B, max_obs, f.ctypes.data) is None
    # twice the columns a chunk would not leave room for three blocks a CU (53 KB each)
    bigger = np.zeros(9, dtype=np.int64)
    assert hc.hc_dp_layout(b"fused", row, col, 64 // row, max_obs, 2 * nc, bigger.ctypes.data) == 9
    assert f[0] == nc < 4 and bigger[-1] > 53 * 1024 and (nc == 1 or f[1] <= 53 * 1024)
    obs_s, obs_l, nob, start = _scenes(row, col, ss, sl, n_obs, max_obs, B, seed=row * 7919 + col * 31 + max_obs)
    nob[1:-1] = np.maximum(nob[1:-1], 1)                # one scene without obstacles (the last: the bypass), the others planned
    p = dp_params(row=row, col=col, sample_s=ss, sample_l=sl)
    rows, min_cost, status = planner.dp_plan(p, obs_s, obs_l, nob, start, mode=0)
    xrows, xfeas, _ = ex.dp_plan(obs_s, obs_l, nob, start, row, col, ss, sl, 2)
    assert np.array_equal(rows, xrows), "DP rows differ from the exact oracle"
    assert np.array_equal((status & 1) == 1, ~xfeas)


@pytest.mark.parametrize("row", [9, 7], ids=["9rows", "generic_rows"])
def test_sweep_and_densification_at_120_columns_one_scene(planner, row):
    """One scene, 120 columns: the sweep's predecessor table is 120 x 64 bytes behind the 64-double front, the densification
    takes its 120 rows through LDS and more segments than a wavefront has lanes.  (The stand-alone calls run the densification
    without the backtrack: enrich_lds's predecessor bytes `bt` are reached through planning cycles only, at 120 columns in
    tests/test_gpu_fullsize.py.)"""
    from emplanner_carla_amd.api import dp_params, max_path_points
    col, ss, sl, res = 120, 2.5, 1.5, 1.0
    # eight obstacles along the 300 m, left and right in turn: a feasible path that changes rows
    rng, k = np.random.default_rng(0), np.arange(8)
    obs_s = (25.0 + 35.0 * k + rng.uniform(-3, 3, 8))[None, :]
    obs_l = (5.0 * (-1.0) ** k + rng.uniform(-1.5, 1.5, 8))[None, :]
    nob, start = np.array([8], np.int32), np.array([[1.25, 0.2, 0.01, -0.003]])
    p = dp_params(row=row, col=col, sample_s=ss, sample_l=sl, sampling_res=res)
    rows, min_cost, status = planner.dp_plan(p, obs_s, obs_l, nob, start, mode=1)
    xrows, xfeas, xpaths = ex.dp_plan(obs_s, obs_l, nob, start, row, col, ss, sl, res)
    assert np.array_equal(rows, xrows), "DP rows differ from the exact oracle"
    assert xfeas.all() and (status == 0).all()
    assert len(np.unique(xrows)) > 1                         # the obstacles move the path: the chain of predecessors is not constant
    ps, pl, ln, st = planner.dp_enrich(p, rows, start, max_path_points(p))
    xs, xl = xpaths[0]
    assert st[0] == 0 and ln[0] == len(xs)
    assert np.array_equal(ps[0, :ln[0]], np.asarray(xs)) and np.array_equal(pl[0, :ln[0]], np.asarray(xl))
