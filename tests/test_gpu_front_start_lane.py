"""The projection kernel's planning start rides in a free lane of the last obstacle group (emp_tail_kernels.h,
frenet_project_wave_kernel): the start is point k behind the k obstacles, lane k & 63 of group k / 64.  Obstacle rows of 63, 64
and 65 slots filled to capacity put it on the last lane of a group, in a group of its own and on the second lane of a second
group; no obstacles at all make it the only group.  Every output is compared with oracle/ref_port.py on the scene's valid
slices - what lies behind the counts is NaN or hostile - and every scene must give the same bits alone and inside a batch.

Planner.frenet_project has no dynamic-obstacle input (only emp_plan_cycle passes one on, with obstacle rows of max_obs + 3
slots: k + 3 > obs_cap cannot be reached through the C ABI), so the virtual obstacles and the obstacle total are checked through
plan_cycle: its DP sees them.  Output padding is not observable through either call (they allocate their outputs)."""
import functools

import numpy as np
import pytest

from emplanner_carla_amd import scenes as S
from oracle import ref_port as op
from tests.conftest import assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-6                  # as tests/test_gpu_cycle.py
MAX_REF = 130
N_REF = (51, 0, 1, 2, 64, 65, 130, 51, 130)          # 65 and 130 take the chunked scan
#: obstacle counts per scene for every row width: capacity first, then 0, 1, 8 and capacity again among other line lengths
N_OBS = {8: (8, 0, 1, 8, 8, 0, 1, 8, 3), 63: (63, 0, 1, 8, 63, 63, 8, 1, 63), 64: (64, 0, 1, 8, 64, 64, 8, 1, 64),
         65: (65, 0, 1, 8, 65, 65, 8, 1, 65)}


@pytest.fixture(scope="module")
def planner():
    from tests.conftest import make_planner
    p = make_planner(0)
    yield p
    p.close()


def _line(rng, n):
    """n nodes 2 m apart on an arc, heading and curvature consistent."""
    kappa = rng.uniform(-0.01, 0.01)
    h = rng.uniform(-3.0, 3.0) + kappa * 2.0 * np.arange(n)
    xy = np.zeros((n, 2))
    xy[0] = rng.uniform(-50.0, 50.0, 2)
    for j in range(1, n):
        xy[j] = xy[j - 1] + 2.0 * np.array([np.cos(h[j - 1]), np.sin(h[j - 1])])
    return np.concatenate([xy, h[:, None], np.full((n, 1), kappa)], axis=1)


def _beside(rng, line, j, lateral):
    x, y, h, _ = line[j]
    along = rng.uniform(-0.9, 0.9)
    return np.array([x + along * np.cos(h) - lateral * np.sin(h), y + along * np.sin(h) + lateral * np.cos(h)])


@functools.lru_cache(maxsize=None)
def scenes(max_obs):
    """Nine scenes (clean, full rows) and their counts; read-only."""
    rng = np.random.default_rng(1000 + max_obs)
    B = len(N_REF)
    ref = np.stack([_line(rng, MAX_REF) for _ in range(B)])
    n_ref, n_obs = np.array(N_REF, np.int32), np.array(N_OBS[max_obs], np.int32)
    origin, start, obs = np.zeros((B, 2)), np.zeros((B, 2)), np.zeros((B, max_obs, 2))
    for b in range(B):
        top = max(int(n_ref[b]) - 1, 0)
        origin[b] = _beside(rng, ref[b], min(3, top), rng.uniform(-0.3, 0.3))
        start[b] = _beside(rng, ref[b], min(10, top), rng.uniform(-0.8, 0.8))
        for j in range(max_obs):
            obs[b, j] = _beside(rng, ref[b], int(rng.integers(0, top + 1)), rng.uniform(-4.0, 4.0))
    v = np.stack([rng.uniform(3.0, 9.0, B), rng.uniform(-1.0, 1.0, B)], axis=1)
    a = rng.uniform(-0.5, 0.5, (B, 2))
    out = dict(ref=ref, n_ref=n_ref, n_obs=n_obs, origin=origin, start=start, obs=obs, v=v, a=a)
    for x in out.values():
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(max_obs):
    """oracle/ref_port.py on the valid slices of every scene; None where the reference raises IndexError (no node to project on)."""
    sc = scenes(max_obs)
    res = []
    for b in range(len(N_REF)):
        nodes = [tuple(r) for r in sc["ref"][b, :sc["n_ref"][b]]]
        pts = [tuple(p) for p in sc["obs"][b, :sc["n_obs"][b]]]
        st = tuple(sc["start"][b])
        try:
            sm = op.cal_s_map_fun(nodes, tuple(sc["origin"][b]))
            os_, ol_ = op.cal_s_l_fun(pts, nodes, sm) if pts else ([], [])
            bs, bl = op.cal_s_l_fun([st], nodes, sm)
            l0, _, _, _, dl0, _, ddl0 = op.cal_s_l_deri_fun([st], [tuple(sc["v"][b])], [tuple(sc["a"][b])], nodes, st)
        except IndexError:
            res.append(None)
            continue
        res.append(dict(s_map=np.asarray(sm, np.float64), obs_s=np.asarray(os_, np.float64), obs_l=np.asarray(ol_, np.float64),
                        begin=np.array([bs[0], bl[0]]), start=np.array([bs[0], l0[0], dl0[0], ddl0[0]])))
    return res


def poisoned(max_obs, poison):
    sc = scenes(max_obs)
    ref, obs = sc["ref"].copy(), sc["obs"].copy()
    for b in range(len(N_REF)):
        nr, k = sc["n_ref"][b], sc["n_obs"][b]
        if poison == "nan":
            ref[b, nr:] = np.nan
            obs[b, k:] = np.nan
        else:                        # nodes on the planning start, heading 1 rad off; obstacles on the origin of the s axis
            ref[b, nr:, :2] = sc["start"][b]
            ref[b, nr:, 2] += 1.0
            ref[b, nr:, 3] = 0.3
            obs[b, k:] = sc["origin"][b]
    return ref, obs


def _project(planner, sc, ref, obs, idx):
    idx = list(idx)
    return planner.frenet_project(ref_line=ref[idx], n_ref=sc["n_ref"][idx], origin_xy=sc["origin"][idx], start_xy=sc["start"][idx],
                                  start_v=sc["v"][idx], start_a=sc["a"][idx], obs_xy=obs[idx], n_obs=sc["n_obs"][idx])


@pytest.mark.parametrize("poison", ["nan", "hostile"])
@pytest.mark.parametrize("max_obs", [8, 63, 64, 65])
def test_start_lane_of_the_obstacle_flush(planner, max_obs, poison):
    sc, want = scenes(max_obs), truth(max_obs)
    ref, obs = poisoned(max_obs, poison)
    B = len(N_REF)
    batch = _project(planner, sc, ref, obs, range(B))
    compared = 0
    for b in range(B):
        nr, k = int(sc["n_ref"][b]), int(sc["n_obs"][b])
        sm, os_, ol_, bsl, start = (x[b] for x in batch)
        valid = (sm[:nr], os_[:k], ol_[:k], bsl, start)
        if want[b] is not None:
            w = want[b]
            assert_rel(valid[0], w["s_map"], RTOL, f"scene {b} s_map")
            assert_rel(valid[1], w["obs_s"], RTOL, f"scene {b} obs_s")
            assert_rel(valid[2], w["obs_l"], RTOL, f"scene {b} obs_l")
            assert_rel(valid[3], w["begin"], RTOL, f"scene {b} begin s, l")
            assert_rel(valid[4], w["start"], RTOL, f"scene {b} start")
            compared += 1
        else:
            assert nr == 0
        alone = _project(planner, sc, ref, obs, [b])
        for got, x in zip(valid, (alone[0][0, :nr], alone[1][0, :k], alone[2][0, :k], alone[3][0], alone[4][0])):
            assert np.array_equal(got, x, equal_nan=True), f"scene {b}: alone and in the batch of {B} differ"
    assert compared == B - 1
    three = _project(planner, sc, ref, obs, range(3))
    for b in range(3):
        nr, k = int(sc["n_ref"][b]), int(sc["n_obs"][b])
        for x, y, n in zip(three, batch, (nr, k, k, 2, 4)):
            assert np.array_equal(x[b, :n], y[b, :n], equal_nan=True), f"scene {b}: batch of 3 and of {B} differ"


@functools.lru_cache(maxsize=None)
def _dyn_case():
    """Six cfg2 scenes; obstacle counts at capacity (k + 3 == obs_cap), 0, 1 and in between; a dynamic obstacle on four of them."""
    cfg = S.CFG2
    b = S.make_batch(range(700, 706), cfg)
    mo = b.obs_xy.shape[1]
    n_obs = np.minimum(np.array([mo, 0, 1, mo, 3, mo], np.int32), b.n_obs.astype(np.int32))
    rng = np.random.default_rng(77)
    dyn = np.stack([rng.uniform(12.0, 35.0, 6), rng.uniform(0.0, 3.0, 6)], axis=1)
    dyn[[2, 4]] = np.nan
    kw = dict(sampling_res=cfg.sampling_res, row=cfg.row, col=cfg.col, sample_s=cfg.sample_s, sample_l=cfg.sample_l)
    want = []
    for i in range(6):
        d = None if np.isnan(dyn[i, 0]) else tuple(dyn[i])
        try:
            want.append(op.plan_cycle(b.ref[i], b.origin_xy[i], b.start_xy[i], b.start_v[i], b.start_a[i], b.obs_xy[i, :n_obs[i]],
                                      dp_kwargs=kw, obs_length=cfg.obs_length, obs_width=cfg.obs_width, verbose=False, dyn_dis_speed=d))
        except (IndexError, np.linalg.LinAlgError):
            want.append(None)
    return cfg, b, n_obs, dyn, want


def test_virtual_obstacles_behind_a_full_obstacle_row(planner):
    from emplanner_carla_amd.api import dp_params_from_cfg, qp_params, smooth_params
    cfg, b, n_obs, dyn, want = _dyn_case()
    obs = b.obs_xy.copy()
    for i in range(6):
        obs[i, n_obs[i]:] = np.nan

    def run(idx):
        idx = list(idx)
        P = b.ref.shape[1]
        return planner.plan_cycle(dp_params_from_cfg(cfg), qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), smooth_params(),
                                  ref_line=b.ref[idx], n_ref=np.full(len(idx), P, np.int32), origin_xy=b.origin_xy[idx],
                                  start_xy=b.start_xy[idx], start_v=b.start_v[idx], start_a=b.start_a[idx], obs_xy=obs[idx],
                                  n_obs=n_obs[idx], dyn_dis_speed=dyn[idx])

    r = run(range(6))
    compared = with_virtual = 0
    for i in range(6):
        alone = run([i])
        for f in ("dp_rows", "traj", "traj_len", "status"):
            assert np.array_equal(getattr(r, f)[i], getattr(alone, f)[0], equal_nan=True), f"scene {i} {f}: alone and in the batch differ"
        w = want[i]
        if w is None:
            continue
        assert np.array_equal(r.dp_rows[i], np.asarray(w["dp_rows"], np.float64)), f"scene {i}: DP rows"
        with_virtual += len(w["obs_s"]) == n_obs[i] + 3
        if w.get("qp_status") == "optimal" and w["smooth_status"] == "optimal":
            m = len(w["trajectory"])
            assert r.traj_len[i] == m
            assert_rel(r.traj[i, :m, :3], np.asarray(w["trajectory"], np.float64)[:, :3], RTOL, f"scene {i} trajectory")
            compared += 1
    assert compared >= 3 and with_virtual >= 3
