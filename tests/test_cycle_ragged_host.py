"""What keeps tests/test_gpu_cycle_batch.py from being vacuous, checked on the oracles alone (no GPU, no library): the ragged
batches of tests/cycle_ragged.py really hold the counts the issue is about, their hostile padding really would change the
answer if it were counted, and the port really takes every outcome on them - planned at full length, planned with two or
three trajectory points, IndexError, an infeasible path QP.  Run with -s to see the measured mix per lattice."""
import numpy as np
import pytest

from tests import cycle_ragged as R


@pytest.mark.parametrize("case", list(R.EXACT_CASES))
def test_counts_follow_the_recipe(case):
    cfg, seeds, seed = R.EXACT_CASES[case]
    r = R.ragged_batch(cfg, seeds, seed, "zero")
    B, P, mo = len(r), cfg.n_ref, max(cfg.n_obs, 1)
    assert r.ref.shape == (B, P, 4) and r.obs_xy.shape == (B, mo, 2)
    assert r.n_ref[0] == P and r.n_ref[-1] == P
    assert all((r.n_ref == k).any() for k in (0, 1, 2, 3))
    assert ((r.n_ref >= P - 12) & (r.n_ref <= P)).sum() >= 2 + B // 3 - 1
    assert (r.n_ref >= 0).all() and (r.n_ref <= P).all()
    assert (r.n_obs < mo).all() and (r.n_obs >= 0).all(), "every scene has obstacle padding"
    assert (r.n_obs == 0).sum() >= 3 and r.n_obs[0] == mo - 1
    if cfg.n_obs:
        tiles = [r.n_obs[t:t + 64 // cfg.row] for t in range(0, B, 64 // cfg.row)] if cfg.row <= 32 else [r.n_obs]
        assert any((t == 0).any() and (t > 0).any() for t in tiles), "a bypass scene beside obstacle scenes in one sweep tile"


@pytest.mark.parametrize("case", ["cfg2", "default", "cfg5"])
def test_hostile_obstacles_are_mapped_like_the_generators_own(case):
    """scenes.scene_frenet_to_xy, which places the hostile obstacles, gives every obstacle of the generator its own x, y back."""
    cfg, seeds, seed = R.EXACT_CASES[case]
    b = R.ragged_batch(cfg, seeds, seed, "zero").batch
    for i in range(len(b)):
        for k in range(b.n_obs[i]):
            xy = R.S.scene_frenet_to_xy(int(b.seeds[i]), cfg, b.sl_obs_s[i, k], b.sl_obs_l[i, k])
            assert np.array_equal(xy, b.obs_xy[i, k]), (i, k)


@pytest.mark.parametrize("poison", R.POISONS)
def test_poison_leaves_the_valid_slices_alone(poison):
    cfg, seeds, seed = R.EXACT_CASES["cfg2"]
    r, z = R.ragged_batch(cfg, seeds, seed, poison), R.ragged_batch(cfg, seeds, seed, "zero")
    for i in range(len(r)):
        nr, no = r.n_ref[i], r.n_obs[i]
        assert np.array_equal(r.ref[i, :nr], r.batch.ref[i, :nr]) and np.array_equal(r.obs_xy[i, :no], r.batch.obs_xy[i, :no])
        assert np.array_equal(r.sl_obs_s[i, :no], r.batch.sl_obs_s[i, :no])
        if poison == "nan":
            assert np.isnan(r.ref[i, nr:]).all() and np.isnan(r.obs_xy[i, no:]).all() and np.isnan(r.sl_obs_l[i, no:]).all()
        if poison == "hostile":
            assert (r.ref[i, nr:, :2] == r.batch.start_xy[i]).all() and (r.ref[i, nr:, 3] == 0.3).all()
    assert np.array_equal(r.n_ref, z.n_ref) and np.array_equal(r.n_obs, z.n_obs)


@pytest.mark.parametrize("case", [c for c in R.EXACT_CASES if c != "cfg1"])
def test_hostile_obstacles_would_change_the_dp_if_counted(case):
    """oracle/exact.dp_plan with the padding counted moves dp_rows in at least 80 % of the scenes that have padding and
    n_obs > 0 (measured: 36 of 37 on CFG2, 28 of 28 on the default lattice, 5 of 6 on CFG5) - and in none with the true counts."""
    cfg, seeds, seed = R.EXACT_CASES[case]
    r = R.ragged_batch(cfg, seeds, seed, "hostile")
    obs_s, obs_l, n_obs, start = r.dp_inputs()
    mo = obs_s.shape[1]
    counted, _, _ = R.exact_dp(cfg, obs_s, obs_l, np.full(len(r), mo, np.int32), start)
    true, _, _ = R.exact_dp(cfg, obs_s, obs_l, n_obs, start)
    zero = R.ragged_batch(cfg, seeds, seed, "zero")
    zrows, _, _ = R.exact_dp(cfg, zero.sl_obs_s, zero.sl_obs_l, n_obs, start)
    assert np.array_equal(true, r.clean_rows) and np.array_equal(zrows, r.clean_rows)
    act = (n_obs > 0) & (n_obs < mo)
    moved = (counted != r.clean_rows).any(axis=1)
    print(f"{cfg.name}: hostile padding, if counted, moves dp_rows in {int(moved[act].sum())} of {int(act.sum())} obstacle scenes "
          f"and {int(moved[~act].sum())} of {int((~act).sum())} bypass scenes")
    assert act.sum() >= 5 and moved[act].mean() >= 0.8
    assert moved[n_obs == 0].any(), "a bypass scene that counted its padding would run the DP"


@pytest.mark.parametrize("case", ["cfg2", "default"])
def test_port_outcomes_on_the_ragged_batch(case):
    """The port alone, on each scene's valid slices: at least 60 % planned with QP and smoothing optimal, IndexError for every
    line of at most three nodes, a planned trajectory of at most three points and one at full length (measured: CFG2 18 of 24
    planned, 4 IndexError, 2 infeasible QPs, lengths 2..23; default lattice 37 of 45, 5, 3, lengths 2..27)."""
    cfg, seeds, seed = R.PORT_CASES[case]
    r = R.ragged_batch(cfg, seeds, seed, "zero")
    truth = R.port_truth(cfg, seeds, seed)
    mix, lens = R.outcome_mix(truth)
    print(f"{cfg.name}: {len(r)} scenes, outcomes {mix}, trajectory lengths {lens}")
    assert mix.get("planned", 0) >= 0.6 * len(r)
    short = np.nonzero(r.n_ref <= 3)[0]
    assert len(short) >= 4 and all(truth[i].outcome == "index" for i in short)
    full = {"cfg2": 23, "default": 27}[case]
    assert lens[0] <= 3 and lens[-1] == full
    for t in truth:
        if t.outcome == "planned":
            assert t.out["qp_status"] == "optimal" and t.out["smooth_status"] == "optimal"


def test_port_outcomes_with_virtual_obstacles():
    """The CFG2 batch with a first dynamic obstacle in every other scene: the virtual obstacles change the outcome or the DP
    rows of some of those scenes and of none of the others."""
    cfg, seeds, seed = R.PORT_CASES["cfg2"]
    plain, dyn = R.port_truth(cfg, seeds, seed), R.port_truth(cfg, seeds, seed, 7)
    given = ~np.isnan(R.dyn_dis_speed(len(plain), 7)[:, 0])
    differs = np.array([a.outcome != b.outcome or list(a.out.get("dp_rows", [])) != list(b.out.get("dp_rows", []))
                        for a, b in zip(plain, dyn)])
    print(f"{cfg.name} + dyn_dis_speed: outcomes {R.outcome_mix(dyn)[0]}, {int(differs.sum())} scenes differ from the plain batch")
    assert differs[given].sum() >= 3 and not differs[~given].any()
