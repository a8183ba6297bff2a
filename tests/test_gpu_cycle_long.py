"""emp_plan_cycle above 61 stations, each lattice against oracle/ref_port.plan_cycle scene by scene (in the manner of
test_path_qp_at_its_size_limits): the 16-lane rows form of the path QP up to its limit of 66 stations, the one-scene-per-wavefront
form with the register-resident solver (up to 66) and the LDS-resident one (67 and more) in one batch, the wide Cartesian kernel
on either side of 64 trajectory points (above it the smoother works in LDS), and the 255 DP points / 128 stations / 130
trajectory points that are the most the ABI accepts.

    col   n_ref   DP points   stations   trajectory points
     62     81    123-125     62-63       64-65        rows<16,4>; the Cartesian kernel's 64-point boundary
     65     81    128-131     64-66       66-68        rows<16,4> at its limit
     66     81    130-133     65-67       67-69        max_pts = 132: rows<16,4>, the 133-point scene EMP_ST_TRUNCATED; default: wave<64>
     67     81    132-135     66-68       68-70        wave<64>: register and LDS solver in one batch
     70     91    138-141     69-71       71-73        LDS solver
    127    151    252-255    126-128     128-130       the ABI's maximum

What this file found: trajectories of more than 64 points are smoothed by the LDS-resident interior point (range_qp_solve_wave),
whose stopping rule for the box QP (eps_mu = 1e-13, emp_qp_core.h box_qp_forms) left the points beside a weakly active bound
9.4e-9 m from the certified minimiser - x, y and the heading far inside their tolerance, the curvature, a second difference over
2 m steps, not: trajectory point 3 of seed 404 (|kappa| = 6e-4, so the 1e-9 floor applies) missed the rule by 1.02 (col 65),
1.04 (col 66) and 8.4 (col 127).  The CPU build of the solver (tests/host_check hc_box_qp) showed the same 9.4e-9 m on that
scene's 67 points.  With eps_mu = 1e-16 (and eps_p = 1e-11) both are within 1e-12 m of the oracle, in 7 to 11 iterations.
"""
import functools

import numpy as np
import pytest

from emplanner_carla_amd import scenes as S
from oracle import ref_port as op
from tests.conftest import assert_rel, make_planner

pytestmark = pytest.mark.gpu
RTOL = 1e-6
SEEDS = tuple(range(400, 406))
ST_TRUNCATED = 32
# (col, n_ref, max_pts or None for the default capacity)
LATTICES = [(62, 81, None), (65, 81, None), (66, 81, 132), (66, 81, None), (67, 81, None), (70, 91, None), (127, 151, None)]
COMPARED = {}              # lattice -> stations of every compared scene: each lattice runs once, whichever test asks first


@pytest.fixture(scope="module")
def planner():
    pl = make_planner()
    yield pl
    pl.close()


def lattice(col, n_ref):
    return S.LatticeConfig(f"long_{col}x5", row=5, col=col, sample_s=2.0, sample_l=1.0, sampling_res=1, n_obs=6, n_ref=n_ref)


@functools.lru_cache(maxsize=None)
def port_truth(col, n_ref):
    """plan_cycle of the port for the six scenes: a dict per scene, or "index" where it raises IndexError."""
    cfg = lattice(col, n_ref)
    b = S.make_batch(SEEDS, cfg)
    kw = dict(sampling_res=cfg.sampling_res, row=cfg.row, col=cfg.col, sample_s=cfg.sample_s, sample_l=cfg.sample_l)
    out = []
    for i in range(len(SEEDS)):
        try:
            out.append(op.plan_cycle([tuple(x) for x in b.ref[i]], b.origin_xy[i], b.start_xy[i], b.start_v[i], b.start_a[i],
                                     b.obs_xy[i, :b.n_obs[i]], dp_kwargs=kw, obs_length=cfg.obs_length, obs_width=cfg.obs_width,
                                     verbose=False))
        except IndexError:
            out.append("index")
    return tuple(out)


def compared_stations(planner, col, n_ref, max_pts):
    """Runs and checks one lattice (once); returns the station counts of the scenes that were compared with the port."""
    if (col, n_ref, max_pts) in COMPARED:
        return COMPARED[(col, n_ref, max_pts)]
    from emplanner_carla_amd.api import dp_params_from_cfg, max_path_points, qp_params, smooth_params
    cfg = lattice(col, n_ref)
    b = S.make_batch(SEEDS, cfg)
    B, P = b.ref.shape[:2]
    p = dp_params_from_cfg(cfg)
    assert max_path_points(p) == 2 * col + 1 <= 255
    kwargs = {} if max_pts is None else {"max_pts": max_pts}
    r = planner.plan_cycle(p, qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), smooth_params(), ref_line=b.ref,
                           n_ref=np.full(B, P, np.int32), origin_xy=b.origin_xy, start_xy=b.start_xy, start_v=b.start_v,
                           start_a=b.start_a, obs_xy=b.obs_xy, n_obs=b.n_obs, **kwargs)
    stations, truncated = [], 0
    for i, want in enumerate(port_truth(col, n_ref)):
        assert want != "index", f"scene {i}: the port raises IndexError on a lattice chosen so that it does not"
        assert np.array_equal(r.dp_rows[i], np.asarray(want["dp_rows"], dtype=np.float64)), f"scene {i}: DP rows"
        assert want["qp_status"] == "optimal", f"scene {i}: the port's QP ends {want['qp_status']}"
        if max_pts is not None and len(want["dp_s"]) > max_pts:
            assert r.status[i] & ST_TRUNCATED, f"scene {i}: {len(want['dp_s'])} DP points do not fit {max_pts}: EMP_ST_TRUNCATED"
            truncated += 1
            continue
        assert (r.status[i] & ~1) == 0, f"scene {i}: status {r.status[i]}"
        if want["smooth_status"] != "optimal":          # the dense oracle did not certify its own smoothing: no yardstick
            continue
        m = len(want["path_l"])
        assert r.path_len[i] == m, f"scene {i}: path length {r.path_len[i]}, the port's {m}"
        assert_rel(r.path_l[i, :m], np.asarray(want["path_l"]), RTOL, f"scene {i} path l")
        traj = np.asarray(want["trajectory"], dtype=np.float64)
        t = len(traj)
        assert r.traj_len[i] == t == m + 1, f"scene {i}: trajectory length {r.traj_len[i]}, the port's {t}"
        assert_rel(r.traj[i, :t, :3], traj[:, :3], RTOL, f"scene {i} trajectory")
        assert_rel(r.traj[i, 2:t, 3], traj[2:, 3], RTOL, f"scene {i} curvature")
        stations.append(len(want["qp_l"]))
    print(f"col {col}, max_pts {max_pts}: compared scenes with {stations} stations, {truncated} truncated")
    if max_pts is not None:
        assert truncated == 1 and len(stations) == B - 1 and max(stations) == max_pts // 2
    COMPARED[(col, n_ref, max_pts)] = stations
    return stations


@pytest.mark.parametrize("col,n_ref,max_pts", LATTICES)
def test_long_cycle_vs_port(planner, col, n_ref, max_pts):
    assert len(compared_stations(planner, col, n_ref, max_pts)) >= 5


def test_long_cycle_coverage(planner):
    """None of the lattices passed by skipping, and both sides of the 66 | 67 switch were compared."""
    every = [n for lat in LATTICES for n in compared_stations(planner, *lat)]
    assert sum(n >= 67 for n in every) >= 3 and sum(62 <= n <= 66 for n in every) >= 3
    assert max(every) == 128
