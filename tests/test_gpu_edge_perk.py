"""GPU parity: the per-source-row block of the work-ring edge kernel (emp_dp_kernels.h dp_edge_ring_kernel, round 9).

For every source row k the kernel fetches the reach masks A_k, B_k of the scene's lane k with ds_bpermute - as ONE word
(A | B << 16) where the call's masks fit 16 bits, fetched one k ahead - classifies the edge's mask with pass & (pass - 1)
and pushes it into one of two rings from two prefix counts.  What can go wrong there: a bit that crosses between the two
halves of the packed word, the wrong form for a mask width, a prefetch that belongs to another k or another scene, a slot
computed from the other ring's count, a round that fires between two k with entries of both.  The cases:

  * max_obs 16, 17, 32, 33 (packed 32-bit, unpacked 32-bit twice, 64-bit masks) x rows 5, 9, 12, 21 and the generic 7, with
    obstacles in slots 0, 15, 16, 31, 32 whose band ends lie exactly on lattice values, so that bit 15 of A and bit 0 of B
    (neighbours in the packed word) differ; ragged last tiles, dead lanes (S * row < 64 for every one of these row counts),
    lattices of 2, 3 and 4 columns;
  * one scene;
  * every obstacle within reach of every edge, scenes with one obstacle beside scenes with many: both rings pass 64 entries
    inside a column and rounds fire between two k;
  * obstacles, none within reach.

Bar: the ring form equal bit for bit to the lockstep form (edge_form = 1) and to oracle/exact.py edge_costs; the tiled layout
everywhere, the canonical one on the cases marked so.
"""
import numpy as np
import pytest

from oracle import exact as ex

pytestmark = pytest.mark.gpu

# With dx = 2.5 (the obstacle 2.5 m before the column's first station) the lateral half-width of the reach band is
# sqrt(36.5 - 6.25) = 5.5 exactly, so the band's ends can be placed on lattice values.
DX_TIE, R_TIE = 2.5, 5.5
SLOTS = (0, 15, 16, 31, 32)


@pytest.fixture(scope="module")
def planner():
    from emplanner_carla_amd.api import Planner
    p = Planner(0)
    yield p
    p.close()


def _tie(l, sign):
    """The obstacle offset ol with fl(ol - 5.5) == l (sign -1: a tie on b_lo) or fl(ol + 5.5) == l (sign +1: on b_hi)."""
    ol = l - sign * R_TIE
    assert ol + sign * R_TIE == l, "the lattice value is not exactly representable as a band end"
    return float(ol)


def _starts(B, rng):
    return np.column_stack([rng.integers(0, 20, B) * 0.25, rng.uniform(-0.5, 0.5, B), rng.uniform(-0.05, 0.05, B),
                            rng.uniform(-0.01, 0.01, B)])


def _slot_scenes(row, col, ss, sl, max_obs, B, seed):
    """Random obstacles around the lattice; in every scene the slots 0, 15, 16, 31, 32 (those the row holds) sit at the tie
    distance in front of one column, band ends on lattice values: b_hi of even slots, b_lo of odd ones."""
    rng = np.random.default_rng(seed)
    lat = ex.lattice_l(row, sl)
    start = _starts(B, rng)
    obs_s = rng.uniform(-5.0, col * ss + 5.0, (B, max_obs))
    obs_l = rng.uniform(-row * sl, row * sl, (B, max_obs))
    nob = rng.integers(0, max_obs + 1, B).astype(np.int32)
    nob[0] = max_obs
    if B > 2:
        nob[1] = max_obs
        nob[-1] = min(max_obs, 16)       # the last scene of the ragged tile: slots 0 and 15
    for b in range(B):
        j = 1 + b % (col - 1)
        for n, m in enumerate(SLOTS):
            if m >= max_obs:
                continue
            lv = float(lat[(1 + 2 * n + b) % row])
            obs_s[b, m] = start[b, 0] + j * ss - DX_TIE
            obs_l[b, m] = _tie(lv, +1 if m % 2 == 0 else -1)
    # what the construction is for: in scene 0's tie column, bit 15 of A and bit 0 of B differ on some row
    b_hi0, b_lo15 = obs_l[0, 0] + R_TIE, obs_l[0, 15] - R_TIE
    assert ((lat > b_lo15) != (lat < b_hi0)).any()
    return obs_s, obs_l, nob, start


def _full_reach_scenes(row, col, ss, sl, max_obs, B, seed):
    """Every obstacle within reach of every edge (dx = 0 in columns 1 and 2, the band wider than the lattice); scenes with one
    obstacle alternate with scenes that use the whole row."""
    rng = np.random.default_rng(seed)
    lat = ex.lattice_l(row, sl)
    assert col <= 3 and np.abs(lat).max() + 0.03 < np.sqrt(36.5)
    start = _starts(B, rng)
    obs_s = np.repeat(start[:, :1] + 2 * ss, max_obs, axis=1)
    obs_l = rng.uniform(-0.02, 0.02, (B, max_obs))
    nob = np.where(np.arange(B) % 2 == 0, 1, max_obs).astype(np.int32)
    return obs_s, obs_l, nob, start


def _out_of_reach_scenes(row, col, ss, sl, max_obs, B, seed):
    rng = np.random.default_rng(seed)
    start = _starts(B, rng)
    obs_s = start[:, :1] - rng.uniform(30.0, 60.0, (B, max_obs))
    obs_l = rng.uniform(-row * sl, row * sl, (B, max_obs))
    obs_s[:, ::2] = start[:, :1] + rng.uniform(0.0, col * ss, (B, (max_obs + 1) // 2))     # beside the lattice, far to the side
    obs_l[:, ::2] = row * sl + rng.uniform(10.0, 20.0, (B, (max_obs + 1) // 2))
    return obs_s, obs_l, np.full(B, max_obs, np.int32), start


def _tiled_to_canonical(x, row, col, B):
    """The tiled tensor's live lanes as (B, col-1, row_i, row_k)."""
    S_ = 64 // row
    t = x.reshape(-1, 64)[:, :S_ * row].reshape(-1, col - 1, row, S_, row)            # tile, j-1, k, scene, i
    live = (np.arange(t.shape[0])[:, None] * S_ + np.arange(S_)[None, :]) < B
    return t.transpose(0, 3, 1, 4, 2)[live]


# (scenes builder, row, col, sample_s, sample_l, max_obs, scenes, canonical layout too)
CASES = []
for _n, _row in enumerate((5, 9, 12, 21, 7)):
    _ss, _sl = {5: (5.0, 1.0), 9: (2.5, 1.5), 12: (5.0, 1.5), 21: (2.5, 0.5), 7: (4.5, 1.0)}[_row]
    for _m, _max_obs in enumerate((16, 17, 32, 33)):
        CASES.append((_slot_scenes, _row, 2 + (_n + _m) % 3, _ss, _sl, _max_obs, 64 // _row + 1 + (_n + _m) % 2, _row == 9))
CASES += [
    (_slot_scenes, 9, 3, 2.5, 1.5, 16, 1, True),            # one scene
    (_slot_scenes, 7, 2, 4.5, 1.0, 33, 1, False),
    (_full_reach_scenes, 9, 3, 2.5, 1.5, 16, 7, True),      # rounds of both rings between two k, packed masks
    (_full_reach_scenes, 9, 3, 2.5, 1.5, 17, 10, False),    # the same with unpacked masks and a ragged tile
    (_full_reach_scenes, 21, 2, 2.5, 0.5, 33, 3, False),    # one column, 64-bit masks
    (_full_reach_scenes, 5, 3, 5.0, 1.0, 8, 13, False),     # one-byte masks, twelve scenes a wavefront and a scene more
    (_out_of_reach_scenes, 9, 3, 2.5, 1.5, 16, 9, False),
    (_out_of_reach_scenes, 12, 2, 5.0, 1.5, 33, 5, False),
]


def _case_id(c):
    return f"{c[0].__name__.strip('_').replace('_scenes', '')}_{c[2]}x{c[1]}_{c[5]}obs_B{c[6]}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_ring_per_k_block_matches_lockstep_and_oracle(planner, case):
    from emplanner_carla_amd import _lib as L
    from emplanner_carla_amd.api import dp_params
    build, row, col, ss, sl, max_obs, B, canonical = case
    obs_s, obs_l, nob, start = build(row, col, ss, sl, max_obs, B, seed=row * 7919 + col * 31 + max_obs)
    p = dp_params(row=row, col=col, sample_s=ss, sample_l=sl)
    layouts = (L.EMP_EDGE_TILED, L.EMP_EDGE_CANONICAL) if canonical else (L.EMP_EDGE_TILED,)
    out = {}
    for form in (0, 1):
        planner.set_option("edge_form", form)
        try:
            out[form] = {lay: planner.dp_edge_costs(p, obs_s, obs_l, nob, start, layout=lay) for lay in layouts}
        finally:
            planner.set_option("edge_form", 0)
    rc0, re = ex.edge_costs(obs_s, obs_l, nob, start, row, col, ss, sl)
    for lay in layouts:
        c0, e = out[0][lay]
        c0_lock, e_lock = out[1][lay]
        if lay == L.EMP_EDGE_TILED:
            e, e_lock = _tiled_to_canonical(e, row, col, B), _tiled_to_canonical(e_lock, row, col, B)
        assert np.array_equal(c0, c0_lock), "start edges"
        assert np.array_equal(e, e_lock), f"layout {lay}: {(e != e_lock).sum()} of {e.size} edges differ between the two kernels"
        assert np.array_equal(e, re), f"layout {lay}: {(e != re).sum()} of {e.size} edges differ from the exact oracle"
    _, clear = ex.edge_costs(obs_s, obs_l, np.zeros(B, np.int32), start, row, col, ss, sl)
    if build is _out_of_reach_scenes:
        assert np.array_equal(re, clear)
    else:
        assert (re != clear).any()
