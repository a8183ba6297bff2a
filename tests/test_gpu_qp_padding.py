"""The rows form of the path QP (emp_qp_rows.h: eight or four scenes per wavefront) reads its LDS arrays in windows that
reach past a problem's ends and relies on zero padding there instead of a select behind every load.  Padding can go wrong
only through a scene's NEIGHBOURS in the wavefront and through what a scene itself leaves behind, so the truth for every
scene is the same scene planned in a batch of one: the batched result must equal it bit for bit - for partly filled last
wavefronts, for dead groups, and for wavefronts that mix plannable scenes, scenes that are dead before the QP starts and
scenes whose QP is infeasible and iterates to the stall limit, each kind in every group position.

One lattice per instantiation of the kernel: <8, 3> at the benchmark's 21 stations and at its limit of 26, <8, 4> at 27
and 34, <16, 4> at 61.  The kernel is chosen by the station CAPACITY of the call (path points the outputs hold, over the
decimation of 2), so each lattice is planned with outputs of exactly twice its station count; a lattice of `stations - 1`
columns gives scenes of `stations - 1` and of `stations` stations, depending on where the start falls.
"""
from __future__ import annotations

import numpy as np
import pytest

from emplanner_carla_amd import scenes as S

pytestmark = pytest.mark.gpu

OUT = (("status", None), ("path_len", None), ("traj_len", None), ("dp_len", None), ("path_s", "path_len"), ("path_l", "path_len"),
       ("traj", "traj_len"))
PLANNED, DEAD, QP_FAILED = 0, 1, 2
POOL = 96                        # scenes a lattice's mix is drawn from
PER_KIND = 6
SIZES = (1, 7, 8, 9, 17)


def _lattice(stations):
    """lattice, max_pts of the call (None: the lattice's own bound)"""
    if stations == 21:
        return S.CFG2, None                                                 # the benchmark's: 40 columns, every second one a station
    return S.LatticeConfig(f"padding_{stations}x5", row=5, col=stations - 1, sample_s=2.0, sample_l=1.0, sampling_res=1,
                           n_obs=6, n_ref=max(61, stations + 10)), 2 * stations


def _kind(status):
    if status & 8:
        return QP_FAILED
    return PLANNED if (status & ~1) == 0 else DEAD          # (bit 0: the DP met a collision cost - such a scene is still planned)


class Mix:
    """A lattice's scenes, each planned alone once, and batches cut from them."""

    def __init__(self, pl, stations):
        from emplanner_carla_amd.api import dp_params_from_cfg, qp_params, smooth_params
        cfg, max_pts = _lattice(stations)
        self.kwargs = {} if max_pts is None else {"max_pts": max_pts}
        self.pl, self.stations = pl, stations
        self.params = (dp_params_from_cfg(cfg), qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), smooth_params())
        # even seeds: corridor scenes (mostly plannable); odd seeds: the survey's slalom, whose obstacles reach the last
        # stations (bound index out of range) or leave no corridor the QP's fixed start state can reach (infeasible QP)
        b = S.make_batch(range(5000, 5000 + POOL), cfg, per_seed=S.survey_geometry_kwargs)
        B, P = b.ref.shape[:2]
        self.inputs = dict(ref_line=b.ref, n_ref=np.full(B, P, np.int32), origin_xy=b.origin_xy, start_xy=b.start_xy,
                           start_v=b.start_v, start_a=b.start_a, obs_xy=b.obs_xy, n_obs=b.n_obs)
        # every sixteenth scene: its first obstacle on the reference line a metre before the horizon - the bound builder's
        # index runs past the last station (IndexError in the reference, EMP_ST_BOUND_INDEX here) and the QP never starts
        at = 5 + int((cfg.col * cfg.sample_s - 1.0) / cfg.ref_ds)            # (the origin is reference point 5)
        assert at < P
        self.inputs["obs_xy"][3::16, 0] = b.ref[3::16, at, :2]
        pool = self._plan(np.arange(B))
        kinds = np.array([_kind(int(s)) for s in pool["status"]])
        self.pool_kinds = kinds
        self.pool_path_len = pool["path_len"]
        self.by_kind = [np.flatnonzero(kinds == k)[:PER_KIND] for k in (PLANNED, DEAD, QP_FAILED)]
        self.alone = {}

    def _plan(self, idx):
        r = self.pl.plan_cycle(*self.params, **{k: np.ascontiguousarray(v[idx]) for k, v in self.inputs.items()}, **self.kwargs)
        return {name: np.array(getattr(r, name)) for name, _ in OUT}

    def single(self, i):
        if i not in self.alone:
            self.alone[i] = self._plan(np.array([i]))
        return self.alone[i]

    def order(self, B, rot):
        """B scenes, kinds cycling planned / dead / failed from `rot` on: over rot = 0, 1, 2 every group position of every
        wavefront holds every kind."""
        use = [0, 0, 0]
        out = []
        for p in range(B):
            k = (p + rot) % 3
            out.append(int(self.by_kind[k][use[k] % len(self.by_kind[k])]))
            use[k] += 1
        return np.array(out)

    def check(self, idx):
        got = self._plan(idx)
        for pos, i in enumerate(idx):
            want = self.single(int(i))
            for name, length in OUT:
                a, w = got[name][pos], want[name][0]
                if length is not None:
                    n = int(want[length][0])
                    a, w = a[:n], w[:n]
                assert np.array_equal(a, w, equal_nan=True), \
                    f"{self.stations} stations, batch of {len(idx)}, position {pos} (scene {i}, kind {self.pool_kinds[i]}): {name}"


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    p = Planner(0)
    p.set_option("path_qp_form", 0)                  # the rows form at every batch size (include/emplanner.h)
    yield p
    p.close()


_mixes = {}


def _mix(pl, stations):
    if stations not in _mixes:
        _mixes[stations] = Mix(pl, stations)
    return _mixes[stations]


STATIONS = (21, 26, 27, 34, 61)


@pytest.mark.parametrize("stations", STATIONS)
def test_the_mix_holds_all_three_kinds_of_neighbour(pl, stations):
    """What the other tests of this file rely on: plannable scenes at the lattice's full station count, scenes dead before
    the QP, scenes whose QP fails."""
    m = _mix(pl, stations)
    counts = [len(x) for x in m.by_kind]
    print(f"{stations} stations: pool kinds planned/dead/failed = {[(m.pool_kinds == k).sum() for k in range(3)]}")
    assert min(counts) >= 2, f"{stations} stations: planned / dead before the QP / QP failed = {counts}"
    planned = m.by_kind[PLANNED]
    # path points = stations + 1 (midpoints and both ends): no planned scene beyond the instantiation's station count, and some
    # of the chosen ones exactly at it
    assert (m.pool_path_len[m.pool_kinds == PLANNED] <= stations + 1).all()
    assert (m.pool_path_len[planned] == stations + 1).any(), m.pool_path_len[planned]


@pytest.mark.parametrize("stations", STATIONS)
@pytest.mark.parametrize("B", SIZES)
def test_partly_filled_wavefronts_equal_scenes_planned_alone(pl, stations, B):
    m = _mix(pl, stations)
    m.check(m.order(B, 0))


@pytest.mark.parametrize("stations", STATIONS)
@pytest.mark.parametrize("rot", (1, 2))
def test_every_kind_of_neighbour_in_every_group_position(pl, stations, rot):
    m = _mix(pl, stations)
    m.check(m.order(17, rot))


@pytest.mark.parametrize("stations", STATIONS)
def test_a_wavefront_of_failing_scenes_beside_one_plannable(pl, stations):
    """Seven scenes that are dead or fail around ONE plannable scene, in the first and in the last group position."""
    m = _mix(pl, stations)
    others = np.concatenate([m.by_kind[QP_FAILED], m.by_kind[DEAD]])
    others = np.resize(others, 7)
    good = int(m.by_kind[PLANNED][0])
    m.check(np.concatenate([[good], others]))
    m.check(np.concatenate([others, [good]]))
