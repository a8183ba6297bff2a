"""GPU parity: the work-ring edge kernel's reach masks (emp_dp_kernels.h dp_edge_ring_kernel).

The ring kernel finds the obstacles an edge (k -> i) must scan from two masks per lane, A_i = {m : l_i > b_lo[m]} and
B_i = {m : l_i < b_hi[m]}, combined as (A_k | A_i) & (B_k | B_i) with the masks of the scene's lane k.  These cases put
obstacle bands exactly on lattice values (ties on b_lo and on b_hi), obstacles exactly on the lattice rows, and cover every
compiled row count, the generic one, 32 rows (two scenes a wavefront), every mask width, empty and full obstacle rows, one
scene and ragged last tiles.  Bar: the ring form equal bit for bit to the lockstep form (both layouts) and to oracle/exact.py.
"""
import numpy as np
import pytest

from oracle import exact as ex

pytestmark = pytest.mark.gpu

# With dx = 2.5 (the obstacle 2.5 m before the column's first station) the lateral half-width of the reach band is
# sqrt(36.5 - 6.25) = 5.5 exactly, so the band's ends can be placed on lattice values.
DX_TIE, R_TIE = 2.5, 5.5


@pytest.fixture(scope="module")
def planner():
    from emplanner_carla_amd.api import Planner
    p = Planner(0)
    yield p
    p.close()


def _tie(l, r, sign):
    """An obstacle offset ol with fl(ol - r) == l (sign -1: a tie on b_lo) or fl(ol + r) == l (sign +1: on b_hi), or None."""
    c = l - sign * r
    for cand in (c, np.nextafter(c, np.inf), np.nextafter(c, -np.inf)):
        if (cand + sign * r) == l:
            return float(cand)
    return None


def _scenes(row, col, ss, sl, n_obs, max_obs, B, seed):
    rng = np.random.default_rng(seed)
    lat = ex.lattice_l(row, sl)
    start = np.column_stack([rng.integers(0, 20, B) * 0.25, rng.uniform(-0.5, 0.5, B), rng.uniform(-0.05, 0.05, B),
                             rng.uniform(-0.01, 0.01, B)])
    obs_s = rng.uniform(-5.0, col * ss + 5.0, (B, max_obs))          # slots beyond a scene's count keep this noise
    obs_l = rng.uniform(-row * sl, row * sl, (B, max_obs))
    for b in range(B):
        for m in range(max_obs):
            kind = rng.integers(0, 5)
            j = int(rng.integers(1, col)) if col > 1 else 1
            lv = float(lat[rng.integers(0, row)])
            if kind == 0 or kind == 1:            # a band end exactly on a lattice value
                ol = _tie(lv, R_TIE, -1 if kind == 0 else 1)
                if ol is not None:
                    obs_s[b, m] = start[b, 0] + j * ss - DX_TIE
                    obs_l[b, m] = ol
            elif kind == 2:                       # the obstacle exactly on a lattice row, inside a column's span
                obs_s[b, m] = start[b, 0] + j * ss + rng.uniform(0.0, ss)
                obs_l[b, m] = lv
            elif kind == 3:                       # on a lattice row, at the tie distance
                obs_s[b, m] = start[b, 0] + j * ss - DX_TIE
                obs_l[b, m] = lv
    nob = rng.integers(0, n_obs + 1, B).astype(np.int32)
    nob[0] = n_obs
    if B > 1:
        nob[-1] = 0
    return obs_s, obs_l, nob, start


def _live_tiled(x, row, col, B):
    S_ = 64 // row
    t = x.reshape(-1, 64)[:, :S_ * row].reshape(-1, (col - 1) * row, S_, row)
    live = (np.arange(t.shape[0])[:, None] * S_ + np.arange(S_)[None, :]) < B
    return t.transpose(0, 2, 1, 3)[live]


# (row, col, sample_s, sample_l, n_obs, max_obs, scenes)
CASES = [
    (9, 40, 2.5, 1.5, 8, 8, 45),          # the benchmark lattice, ragged last tile (45 = 6 x 7 + 3)
    (9, 12, 2.5, 1.5, 16, 16, 7),         # one full tile, 2-byte masks
    (9, 10, 2.5, 1.5, 0, 8, 9),           # no obstacles at all
    (21, 20, 1.0, 0.6, 16, 16, 11),       # the wide benchmark lattice's row count
    (12, 10, 5.0, 1.5, 32, 32, 13),       # 4-byte masks, every slot used in scene 0
    (5, 20, 5.0, 1.0, 64, 64, 25),        # 64-bit masks, a full 64-slot row
    (7, 11, 4.5, 1.0, 40, 40, 1),         # generic row count, 64-bit mask, one scene
    (3, 6, 7.5, 1.5, 2, 2, 43),           # generic row count, 21 scenes a wavefront
    (32, 5, 5.0, 0.4, 8, 8, 5),           # 32 rows: two scenes a wavefront, ragged
    (32, 4, 5.0, 0.4, 64, 64, 3),         # 32 rows, 64-bit masks
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[1]}x{c[0]}_{c[4]}of{c[5]}obs_B{c[6]}")
def test_ring_reach_masks_match_lockstep_and_oracle(planner, case):
    from emplanner_carla_amd import _lib as L
    from emplanner_carla_amd.api import dp_params
    row, col, ss, sl, n_obs, max_obs, B = case
    obs_s, obs_l, nob, start = _scenes(row, col, ss, sl, n_obs, max_obs, B, seed=row * 7919 + col * 31 + max_obs)
    p = dp_params(row=row, col=col, sample_s=ss, sample_l=sl)
    out = {}
    for form in (0, 1):
        planner.set_option("edge_form", form)
        try:
            out[form] = [planner.dp_edge_costs(p, obs_s, obs_l, nob, start, layout=lay)
                         for lay in (L.EMP_EDGE_CANONICAL, L.EMP_EDGE_TILED)]
        finally:
            planner.set_option("edge_form", 0)
    for lay in (0, 1):
        assert np.array_equal(out[0][lay][0], out[1][lay][0]), "start edges"
        a, b = out[0][lay][1], out[1][lay][1]
        if lay == 1:
            a, b = _live_tiled(a, row, col, B), _live_tiled(b, row, col, B)
        assert np.array_equal(a, b), f"layout {lay}: {(a != b).sum()} of {a.size} edges differ between the two kernels"
    _, re = ex.edge_costs(obs_s, obs_l, nob, start, row, col, ss, sl)
    assert np.array_equal(out[0][0][1], re), "ring form against the exact oracle"
    if n_obs > 0:      # not a vacuous comparison: some pair in reach must cost something
        _, clear = ex.edge_costs(obs_s, obs_l, np.zeros(B, np.int32), start, row, col, ss, sl)
        assert (re != clear).any()
