"""The Cartesian tail indexes its passes by TRAJECTORY point (emp_tail_kernels.h, cycle_cartesian_body): point 0 is
the planning start, point q >= 1 path point q - 1, so that the start shares the first pass's trigonometry.  Reached through
plan_cycle like tests/test_gpu_cycle.py::test_path_qp_at_its_size_limits; the lattice's column count sets the output capacity
and with it the instantiation: 21 columns <8, 3> (24 points), 29 columns <8, 4> (32), 60 columns <16, 4> (63).

The trajectory length m is set by where the reference line ends: the path stops at the first point whose s passes s_map[-1]
(path_planning.py:40-41).  The nodes are 1 m apart and the path's s values lie 0.3 m and more from any node's, so no comparison
is decided by a last bit.  m = 15 / 16 (31 / 32 on the 32-lane scenes) are the lines that end at the last point of the first pass
and at the first point of the second.  Path point 0 has the planning start's own s (the densified DP path begins there), so a path
that passes the end of the line at its FIRST point is the scene whose start lies beyond the line: EMP_ST_S_OUT_OF_RANGE.
A scene the path QP has refused and the lanes of scenes that are not there (batches of 1, 3 and 5) share wavefronts with live
scenes.  Everything is compared with oracle/ref_port.plan_cycle on the cut line, and alone against in the batch bit for bit.

The same body runs one scene per wavefront under cartesian_form = 1 (64 lanes per scene: the passes end at 64 points, not at 16 or
32, the scene's ballots are the whole wavefront's): 24 and 32 points reach cycle_cartesian_wave_kernel_narrow, 63
cycle_cartesian_wave_kernel_wide.  Every batch again in that form, bit for bit against the default form."""
import functools

import numpy as np
import pytest

from emplanner_carla_amd import scenes as S
from oracle import ref_port as op
from tests.conftest import assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-6                  # as tests/test_gpu_cycle.py
FULL = None
#: col -> (seed, nodes kept of the reference line, expected outcome: trajectory points, "qp" or "range")
CASES = {
    21: ((306, FULL, 24), (300, 9, 2), (302, FULL, "qp"), (300, 35, 15), (300, 37, 16), (300, 39, 17), (300, 8, "range")),
    29: ((306, FULL, 32), (300, 55, 25), (302, FULL, "qp"), (300, 8, "range")),
    60: ((304, FULL, 63), (300, 67, 31), (300, 69, 32), (300, 71, 33), (300, 8, "range")),
}


@pytest.fixture(scope="module")
def planner():
    from tests.conftest import make_planner
    p = make_planner(0)
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def case(col):
    """Inputs of the lattice's batch (lines cut and NaN behind the cut) and the port's result per scene (None: it raises IndexError)."""
    cfg = S.LatticeConfig(f"tail_{col}x5", row=5, col=col, sample_s=2.0, sample_l=1.0, sampling_res=1, n_obs=4, n_ref=2 * col + 30,
                          ref_ds=1.0)
    b = S.make_batch([c[0] for c in CASES[col]], cfg, start_ahead=S.BENCH_START_AHEAD)
    P = b.ref.shape[1]
    n_ref = np.array([P if c[1] is FULL else c[1] for c in CASES[col]], np.int32)
    ref = b.ref.copy()
    kw = dict(sampling_res=cfg.sampling_res, row=cfg.row, col=cfg.col, sample_s=cfg.sample_s, sample_l=cfg.sample_l)
    want = []
    for i, (_, _, outcome) in enumerate(CASES[col]):
        ref[i, n_ref[i]:] = np.nan
        try:
            w = op.plan_cycle(b.ref[i, :n_ref[i]], b.origin_xy[i], b.start_xy[i], b.start_v[i], b.start_a[i], b.obs_xy[i, :b.n_obs[i]],
                              dp_kwargs=kw, obs_length=cfg.obs_length, obs_width=cfg.obs_width, verbose=False)
        except IndexError:
            w = None
        # the scenes are what the table says they are
        if outcome == "range":
            assert w is None
        elif outcome == "qp":
            assert w["qp_status"] != "optimal"
        else:
            assert w["qp_status"] == "optimal" and w["smooth_status"] == "optimal" and len(w["trajectory"]) == outcome, (col, i)
        want.append(w)
    inputs = dict(ref_line=ref, n_ref=n_ref, origin_xy=b.origin_xy, start_xy=b.start_xy, start_v=b.start_v, start_a=b.start_a,
                  obs_xy=b.obs_xy, n_obs=b.n_obs.astype(np.int32))
    for x in inputs.values():
        x.setflags(write=False)
    return cfg, inputs, want


def _plan(planner, cfg, inputs, idx):
    from emplanner_carla_amd.api import dp_params_from_cfg, qp_params, smooth_params
    idx = list(idx)
    return planner.plan_cycle(dp_params_from_cfg(cfg), qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), smooth_params(),
                              **{k: v[idx] for k, v in inputs.items()})


@pytest.fixture(scope="module")
def hc():
    from tests import host_check
    return host_check.load()


def _cartesian_plan(hc, B, max_ref, max_pts, form):
    """emp_tail_launch.h plan_cycle_cartesian as emp_plan_cycle calls it (stations decimated by two, midpoints, planning start)"""
    fields = ("gp", "r", "wide", "m32", "spw", "grid", "grid_y", "block", "lds")
    out = np.zeros(len(fields), dtype=np.int64)
    err = hc.hc_plan_cycle_cartesian(B, max_ref, max_pts, (max_pts + 1) // 2 + 1, form, out.ctypes.data)
    assert err is None, err
    return dict(zip(fields, out.tolist()))


@pytest.mark.parametrize("col", [21, 29, 60], ids=["rows_8x3", "rows_8x4", "rows_16x4"])
def test_planning_start_is_point_zero_of_the_first_pass(planner, col):
    cfg, inputs, want = case(col)
    N = len(want)
    r = _plan(planner, cfg, inputs, range(N))
    # the trajectory capacity that selects the instantiation (emp_plan_cycle: decimated DP points + midpoint + planning start)
    assert (r.traj.shape[1] - 1 + 1) // 2 + 2 == col + 3
    for i, (_, _, outcome) in enumerate(CASES[col]):
        m = int(r.traj_len[i])
        assert np.all(r.traj[i, m:] == 0.0), f"scene {i}: padding"
        if outcome == "range":
            assert r.status[i] & 2 and m == 0, f"scene {i}: EMP_ST_S_OUT_OF_RANGE expected, status {r.status[i]}"
        elif outcome == "qp":
            assert r.status[i] & 8 and m == 0, f"scene {i}: EMP_ST_QP_FAILED expected, status {r.status[i]}"
        else:
            assert (r.status[i] & ~1) == 0 and m == outcome, f"scene {i}: status {r.status[i]}, {m} points"
            w = np.asarray(want[i]["trajectory"], np.float64)
            assert_rel(r.traj[i, :m, :2], w[:, :2], RTOL, f"scene {i} x, y")
            if m >= 3:                              # (two points: as tests/test_gpu_cycle.py::test_smooth_line_all_kernel_paths)
                assert_rel(r.traj[i, :m, 2], w[:, 2], RTOL, f"scene {i} theta")
    # the same bits alone (three or one scene's worth of lanes idle) and in batches of 3 and 5
    for idx in [[i] for i in range(N)] + [range(3)] + ([range(5)] if N >= 5 else []):
        sub = _plan(planner, cfg, inputs, idx)
        for j, i in enumerate(idx):
            for f in ("traj", "traj_len", "status"):
                assert np.array_equal(getattr(sub, f)[j], getattr(r, f)[i], equal_nan=True), f"scene {i} {f}: batch of {len(idx)} differs"


@pytest.mark.parametrize("col", [21, 29, 60], ids=["narrow_24", "narrow_32", "wide_63"])
def test_one_scene_per_wavefront_gives_the_bits_of_the_default_form(planner, hc, col):
    cfg, inputs, want = case(col)
    N = len(want)
    r = _plan(planner, cfg, inputs, range(N))
    max_ref, max_pts = inputs["ref_line"].shape[1], r.traj.shape[1] - 1
    rows = _cartesian_plan(hc, N, max_ref, max_pts, 0)
    assert (rows["gp"], rows["r"]) == {21: (8, 3), 29: (8, 4), 60: (16, 4)}[col]          # what r came from
    old = planner.get_option("cartesian_form")
    planner.set_option("cartesian_form", 1)
    planner.set_timing(True, only="to_cartesian")
    try:
        for idx in [range(N)] + [[i] for i in range(N)] + [range(3)] + ([range(5)] if N >= 5 else []):
            # which kernel: one launch of the stage, planned as one scene per wavefront, narrow up to 32 points and wide beyond
            p = _cartesian_plan(hc, len(idx), max_ref, max_pts, 1)
            assert (p["r"], p["spw"], p["grid"], p["block"], p["wide"]) == (0, 1, len(idx), 64, int(col == 60)), p
            at = planner.kernel_launches("to_cartesian")
            sub = _plan(planner, cfg, inputs, idx)
            assert planner.kernel_launches("to_cartesian") == at + 1
            for j, i in enumerate(idx):
                for f in ("traj", "traj_len", "status"):
                    assert np.array_equal(getattr(sub, f)[j], getattr(r, f)[i], equal_nan=True), \
                        f"scene {i} {f}: cartesian_form 1 in a batch of {len(idx)} differs from the default form"
    finally:
        planner.set_timing(False)
        planner.set_option("cartesian_form", old)
