"""The launchers every call of a stage shares (emp_api.hip: dev_speed_*, launch_lateral, dev_path_speed_merge), at the smallest
shapes where sharing them can go wrong:

- the speed DP's heaviest-first ordering inside the trajectory call: B = 513 takes it, B = 512 does not, in the fused call and
  in the stand-alone emp_speed_dp alike, and the fused call still equals the chain bit for bit;
- every stage keeps its timing name, once per call, for both lateral laws;
- the merge kernel beyond the default 48 KB of dynamic LDS (opted in by the launcher), and its refusal beyond 64 KB.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_rollout as TR  # noqa: E402  (fleets and helpers; nothing of these three is collected here)
import test_gpu_timed as TD  # noqa: E402
import test_gpu_trajectory as TT  # noqa: E402

from emplanner_carla_amd import api as A  # noqa: E402
from emplanner_carla_amd import scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SPEED_STAGES = ("speed_front", "speed_dp", "speed_convex_space", "speed_qp", "speed_increase_points", "path_speed_merge",
                "speed_status")


@pytest.fixture(scope="module")
def pl():
    p = A.Planner(0)
    yield p
    p.set_timing(False)
    p.close()


def trajectory_case(B, seed):
    """B scenes of the default 12 x 6 lattice with ragged dynamic obstacles and some empty lines, as
    test_trajectory_equals_cycle_and_chain_bit_for_bit builds its own."""
    cfg = S.CFG_DEFAULT
    b = S.make_batch(range(9000, 9000 + B), cfg)
    cyc = TT.cycle_inputs(b, empty=range(3, B, 41))
    dyn, n = TT.dynamic_obstacles(b, seed)
    p, q, sp = A.dp_params_from_cfg(cfg), A.qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), A.smooth_params()
    return p, q, sp, cyc, TT.speed_inputs(cyc, dyn, n, seed)


def launches(pl, names):
    return {k: pl.kernel_launches(k) for k in names}


def rise(pl, before):
    return {k: pl.kernel_launches(k) - v for k, v in before.items()}


@pytest.mark.parametrize("B, ordered", [(513, 1), (512, 0)])
def test_ordered_speed_dp_inside_the_trajectory_call(pl, B, ordered):
    """513 scenes is the smallest batch whose speed DP is ordered heaviest first: one `speed_dp_order` interval in the trajectory
    call and one in the chain's stand-alone speed_dp, none at 512; either way the call equals the chain bit for bit."""
    p, q, sp, cyc, spd = trajectory_case(B, 3)
    M = A.max_path_points(p)
    pl.set_timing(True)
    try:
        at = launches(pl, ("speed_dp_order", "speed_dp"))
        r = pl.plan_cycle(p, q, sp, speed=spd, **cyc)
        assert rise(pl, at) == {"speed_dp_order": ordered, "speed_dp": 1}
        ref = pl.plan_cycle(p, q, sp, **cyc)
        at = launches(pl, ("speed_dp_order", "speed_dp"))
        TT.check_against_chain(pl, r, spd, M, cyc)
        assert rise(pl, at) == {"speed_dp_order": ordered, "speed_dp": 1}
    finally:
        pl.set_timing(False)
    for f in TT.path_fields(r):
        assert TT.same_bits(getattr(r, f), getattr(ref, f)), f
    st = r.speed.speed_status
    print("speed_status classes", {int(v): int((st == v).sum()) for v in np.unique(st)})
    assert (spd.n_dyn > 0).any() and (spd.n_dyn == 0).any()


def test_one_launch_under_every_speed_stage_name(pl):
    p, q, sp, cyc, spd = trajectory_case(3, 4)
    pl.set_timing(True)
    try:
        at = launches(pl, SPEED_STAGES + ("speed_dp_order",))
        pl.plan_cycle(p, q, sp, speed=spd, **cyc)
        assert rise(pl, at) == {**{k: 1 for k in SPEED_STAGES}, "speed_dp_order": 0}
    finally:
        pl.set_timing(False)


@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_one_launch_under_every_control_name(pl, law):
    """B = 6: two wavefronts of MPC groups (five vehicles each), one LQR wavefront."""
    names = ("rollout", "rollout_timed", "vehicle_control")
    d, prof = TR.fleet(6), TD.profiles(6)
    lat, vpar = TR.laws()[law], A.vehicle_params()
    st = d["state"]
    kmh = 3.6 * np.sqrt(st[:, 5] * st[:, 5] + st[:, 3] * st[:, 3])
    pl.set_timing(True)
    try:
        at = launches(pl, names)
        r = pl.rollout(lat, TR.pid(), vpar, d["path"], d["n"], st, d["mi"], d["target"], d["err"], d["n_err"], 2, lateral=law)
        assert rise(pl, at) == {"rollout": 1, "rollout_timed": 0, "vehicle_control": 0}
        at = launches(pl, names)
        rt = TD.run(pl, law, d, prof, 2)
        assert rise(pl, at) == {"rollout": 0, "rollout_timed": 1, "vehicle_control": 0}
        at = launches(pl, names)
        c = pl.vehicle_control(lat, TR.pid(), d["path"], d["n"], st[:, :5].copy(), st[:, 5].copy(), d["mi"], kmh, d["target"], d["err"],
                               d["n_err"], lateral=law)
        assert rise(pl, at) == {"rollout": 0, "rollout_timed": 0, "vehicle_control": 1}
    finally:
        pl.set_timing(False)
    assert r.status[0] == 0 and rt.status[0] == 0 and c.status[0] == 0          # the good vehicle of the fleet was driven


def merge_rows(P):
    """Two paths of 50 and 64 points (NaN from point 40 / 60 on, as a W-wide row is padded) in rows P wide, the slots beyond
    n_init poisoned; speed samples that run along them."""
    B, D = 2, A.SPEED_DENSE_POINTS
    n = np.array([50, 64], np.int32)
    live = (40, 60)
    rows = np.full((5, B, P), 7.0e300)
    for b in range(B):
        i = np.arange(n[b], dtype=np.float64)
        th = 0.01 * (b + 1) * i
        rows[0, b, :n[b]] = 1.5 * i                                      # path_s
        rows[1, b, :n[b]] = 10.0 * b + 1.5 * i * np.cos(th)             # x
        rows[2, b, :n[b]] = 1.5 * i * np.sin(th)                        # y
        rows[3, b, :n[b]] = th                                          # heading
        rows[4, b, :n[b]] = 0.01 * (b + 1) / 1.5                        # kappa
        rows[:, b, live[b]:n[b]] = NAN
    t = np.tile(np.linspace(0.0, 8.0, D), (B, 1))
    v = np.array([[4.0], [6.5]]) + 0.1 * t
    s = v * t * 0.9
    s[1, 350:] = NAN                                                     # the densifier's padding
    return dict(s=s, s_dot=v, s_dot2=np.full((B, D), 0.1), relative_time=t, current_time=np.array([12.5, 99.0]), path_s=rows[0],
                x_init=rows[1], y_init=rows[2], heading_init=rows[3], kappa_init=rows[4], n_init=n)


def test_merge_beyond_48_kb_of_lds(pl):
    """max_path = 1229 needs 5 * 1229 * 8 = 49 160 B of dynamic LDS, the first width past the 49 152 B a kernel gets without
    opting in; the rows are those of a 64-wide call, so the trajectories are too.  1639 (65 560 B) is past this entry's 64 KB."""
    narrow, st_narrow = pl.path_speed_merge(**merge_rows(64))
    wide, st_wide = pl.path_speed_merge(**merge_rows(1229))
    assert (st_narrow == 0).all() and (st_wide == 0).all()
    assert np.isfinite(narrow[:, :, :350]).all()
    assert TT.same_bits(wide, narrow)
    pl.set_timing(True)
    try:
        at = launches(pl, ("path_speed_merge",))
        with pytest.raises(A.EmpError, match="path too long for the LDS-resident merge kernel"):
            pl.path_speed_merge(**merge_rows(1639))
        assert rise(pl, at) == {"path_speed_merge": 0}
    finally:
        pl.set_timing(False)
