"""The inputs of tests/test_gpu_speed_front_batch.py are what tests/speed_front_cases.py says they are (no GPU): no
default-weight comparison hangs on the last bits of a power, the dense scenes fill several list windows, the exact distances
are exact, the poison would change the result if it were read, and every family reaches the code it is named after."""
import numpy as np
import pytest

from oracle import st_speed as st
from tests import host_check
from tests import speed_front_cases as F


@pytest.fixture(scope="module")
def hc():
    return host_check.load()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def test_default_pow_route_is_unchanged_and_kernel_route_is_close():
    rng = np.random.default_rng(1)
    d = np.concatenate([rng.uniform(-2, 2, 20000), F.collision_distances(1000)])
    for w in (10000000, 1.0, 0.0, np.inf, 3.7):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            want = np.where(np.abs(d) < 0.5, np.float64(w), np.where(F.in_band(d), np.power(np.float64(w), (0.5 - d) + 1.0), 0.0))
        assert same_bits(st.exact_collision_cost(w, d), want)
        k = st.exact_collision_cost(w, d, pow_route="kernel")
        fin = np.isfinite(want)
        assert same_bits(k[~fin], want[~fin])
        assert np.all(np.abs(k[fin] - want[fin]) <= 1e-15 * np.abs(want[fin]))
    assert same_bits(st.exact_collision_cost(1.0, d, pow_route="kernel"), st.exact_collision_cost(1.0, d))   # 1 ** y == 1 on both


def test_truth_on_live_slots_equals_truth_on_all_slots():
    """Leaving the absent slots out of the oracle's input changes no bit of any output."""
    for cap, weights in ((16, "default"), (33, "count")):
        _, sets, v0 = F.dp_cases(cap)
        whole = st.exact_speed_dp(*sets, v0, **F.WEIGHTS[weights])
        live = F.truth(cap, weights)
        for k in whole:
            assert same_bits(whole[k], live[k]), (cap, k)


@pytest.mark.parametrize("cap", F.CAPS)
def test_no_near_tie_in_the_default_weight_cases(cap):
    """The two routes to w ** y (np.power; the kernels' exp2 of a double-double logarithm) give the same predecessor, terminal
    node and profile for every scene and costs within 1e-13: no comparison of the GPU test is decided by a power's last bits."""
    _no_near_tie(F.truth(cap, "default"), F.truth(cap, "default", "kernel"), f"capacity {cap}")


def _no_near_tie(a, b, what):
    for k in ("node", "end", "speed_s", "speed_t", "s_dot"):
        bad = [i for i in range(len(a[k])) if not same_bits(a[k][i], b[k][i])]
        assert not bad, f"{k} of scenes {bad} of {what} depends on the route to the power"
    fin = np.isfinite(a["cost"])
    assert same_bits(a["cost"][~fin], b["cost"][~fin])
    assert np.all(np.abs(a["cost"][fin] - b["cost"][fin]) <= 1e-13 * np.abs(a["cost"][fin]))


def test_no_near_tie_in_the_sample_of_the_large_batch_and_behind_the_graph():
    sets, v = F.big_batch()
    assert sets.shape == (4, F.BIG_B, F.BIG_CAP) and F.BIG_B > 512 and F.BIG_CAP > 32
    live = (~np.isnan(sets[0])).sum(axis=1)
    assert live.min() == 0 and live.max() == F.BIG_CAP and len(np.unique(live)) > 10      # a real sort by obstacle count
    assert live[list(F.BIG_SAMPLE)].max() == F.BIG_CAP
    _no_near_tie(F.big_truth(), F.big_truth("kernel"), "the large batch's sample")
    gsets, _ = F.graph_dp_inputs()
    assert np.isinf(gsets).any() and (gsets[1] < gsets[0]).any() and (~np.isnan(gsets[0])).sum() > 100
    _no_near_tie(F.graph_dp_truth("default"), F.graph_dp_truth("default", "kernel"), "the graph's own segments")


@pytest.mark.parametrize("which", ["batch of 96", "64 slots"])
def test_no_near_tie_in_the_older_node_table_comparisons(which):
    """tests/test_gpu_speed.py compares the node tables of these two inputs outright (it used to allow a share of mismatches)."""
    if which == "batch of 96":
        from emplanner_carla_amd import scenes as S
        o = S.make_dynamic_batch(range(200, 296))
        sets, v0 = np.stack(st.exact_generate_st_graph(*o[:4])), o[4]
    else:
        rng = np.random.default_rng(5)
        s_in = rng.uniform(5, 50, (2, 64))
        s_out = s_in + rng.uniform(0, 20, (2, 64))
        t_in = rng.uniform(0, 6, (2, 64))
        t_out = t_in + rng.uniform(1, 6, (2, 64))
        s_in[:, ::3] = np.nan
        sets, v0 = np.stack([s_in, s_out, t_in, t_out]), np.array([3.0, 12.0])
    _no_near_tie(F.oracle_dp(sets, v0), F.oracle_dp(sets, v0, "kernel"), which)


def test_start_speeds_and_families_are_mixed_over_the_capacities():
    seen = set()
    for cap in F.CAPS:
        names, sets, v0 = F.dp_cases(cap)
        assert len(names) == sets.shape[1] == len(v0) and sets.shape[2] == cap
        seen |= {("nan" if np.isnan(v) else v) for v in v0}
        for fam in list(F.SHAPES) + ["live_first", "live_last", "live_alternating", "live_all", "live_none"]:
            assert fam in names
        live = ~np.isnan(sets[0])
        assert live[names.index("live_all")].all() and not live[names.index("live_none")].any()
        assert live[names.index("live_last")].tolist() == [False] * (cap - 1) + [True]
        for k in (31, 32, 63):
            if cap > k:
                name = "live_last" if k == cap - 1 else f"live_{k}"
                assert np.flatnonzero(live[names.index(name)]).tolist() == [k]
    assert {0.0, -3.0, 1e6, np.inf, "nan"} <= seen
    for cap in F.DENSE_CAPS:
        assert "dense" in F.dp_cases(cap)[0]
    # a NaN start: column 0 is NaN, nothing beats +inf afterwards (the reference's strict < from +inf), and the terminal
    # search's <= takes the top right node
    names, sets, v0 = F.dp_cases(16)
    b = int(np.flatnonzero(np.isnan(v0))[0])
    t = F.truth(16, "default")
    assert np.isnan(t["cost"][b, :, 0]).all() and np.isinf(t["cost"][b, :, 1:]).all() and tuple(t["end"][b]) == (0, 15)


def test_axis_aligned_segments_occur_at_both_mask_widths():
    for caps in ((16, 31, 32), (33, 64)):
        ux0 = uy0 = point = False
        for cap in caps:
            names, sets, _ = F.dp_cases(cap)
            s_in, s_out, t_in, t_out = sets[:, names.index("axis")]
            ux0 |= bool(((s_in == s_out) & (t_in != t_out)).any())
            uy0 |= bool(((t_in == t_out) & (s_in != s_out)).any())
            point |= bool(((t_in == t_out) & (s_in == s_out)).any())
        assert ux0 and uy0 and point, caps


@pytest.mark.parametrize("family", list(F.SHAPES))
def test_every_shape_family_has_costly_pairs(family):
    """On its own (without the plain segments beside it) the family puts pairs on the kernel's lists, and its source nodes
    cost something too, except where it is built not to ("exact")."""
    segs = np.array(F.SHAPES[family]()).T
    costly = F.costly_pairs(segs)
    assert costly.any(), family
    per_segment = costly.any(axis=(0, 1, 2, 3))
    print(family, "segments with a costly pair:", per_segment.astype(int).tolist())
    assert per_segment.sum() >= len(per_segment) // 2
    if family == "axis":
        # uy == 0 and ux == 0 cost; the point never does: v3 = 0 makes its distance 0 / 0 = NaN, which no comparison of
        # CalcCollisionCost takes (a kernel that computed a real distance to it would differ from the oracle)
        assert per_segment[:2].all() and not per_segment[2]


def test_the_dense_scenes_fill_more_than_two_list_windows_and_a_lane_straddles_one():
    best = 0
    for cap in F.DENSE_CAPS:
        names, sets, _ = F.dp_cases(cap)
        counts, per_lane = F.list_passes(F.costly_pairs(sets[:, names.index("dense")]))
        print(f"dense scene of {cap} slots: up to {counts.max()} costly pairs in one wavefront pass")
        best = max(best, int(counts.max()))
        if cap >= 33:
            assert counts.max() > 512 and F.straddles(per_lane), cap
    assert best > 512
    # the windows the mutations kStListCap = 64 and = 1024 move: straddled at every size
    names, sets, _ = F.dp_cases(64)
    _, per_lane = F.list_passes(F.costly_pairs(sets[:, names.index("dense")]))
    assert F.straddles(per_lane, 64) and F.straddles(per_lane, 256) and F.straddles(per_lane, 1024)


def test_exact_distances_are_exact_and_their_twins_fall_on_either_side():
    exact = F.SHAPES["exact"]()
    twins = F.SHAPES["ulp"]()
    n = len(F.EXACT_AT)
    for i, (s, off) in enumerate(F.EXACT_AT):
        for t in (0.0, 0.5, 4.0, 8.0):
            if t == 0.0 and s != 0.0:
                continue                                 # only the origin lies at t = 0
            d = float(F.oracle_distance(s, t, *exact[i]))
            assert d == abs(off), (s, off, t, d)
            assert float(st.exact_collision_cost(10000000, d)) == 0.0
            da, db = (float(F.oracle_distance(s, t, *twins[k])) for k in (i, n + i))
            assert min(da, db) < abs(off) < max(da, db), (s, off, da, db)
            assert float(st.exact_collision_cost(10000000, da)) > 0.0 or abs(off) == 1.5
            if abs(off) == 0.5:                           # either side of 0.5 costs; exactly 0.5 does not
                assert float(st.exact_collision_cost(1.0, da)) == 1.0 and float(st.exact_collision_cost(1.0, db)) == 1.0
            else:                                         # only the near side of 1.5 costs
                assert sorted((float(st.exact_collision_cost(1.0, da)), float(st.exact_collision_cost(1.0, db)))) == [0.0, 1.0]
    # and every such segment sits in some scene, on both sides of the mask switch
    for caps in ((16, 31, 32), (33, 64)):
        got = set()
        for cap in caps:
            names, sets, _ = F.dp_cases(cap)
            sc = sets[:, names.index("exact")]
            got |= {float(x) for x in sc[0][(sc[0] == sc[1]) & (sc[2] == 0.0) & (sc[3] == 8.0)]}
        assert got >= {s + o for s, o in F.EXACT_AT}


@pytest.mark.parametrize("cap", F.CAPS)
def test_poison_is_effective(cap):
    """An absent slot's obstacle, made live (its s_in set to its s_out: a stationary obstacle), changes the oracle's result
    of its scene wherever the scene has a finite table; and the poison leaves no absent slot untouched."""
    names, sets, v0 = F.dp_cases(cap)
    p = F.poisoned(cap)
    absent = np.isnan(sets[0])
    assert same_bits(p[:, ~absent], sets[:, ~absent]) and np.isnan(p[0][absent]).all()
    kinds = {"nan": 0, "inf": 0, "hostile": 0}
    kinds["nan"] = int(np.isnan(p[1][absent]).sum())
    kinds["inf"] = int(np.isinf(p[1][absent]).sum())
    kinds["hostile"] = int(np.isfinite(p[1][absent]).sum())
    if absent.sum() >= 3:
        assert min(kinds.values()) > 0, kinds
    t = F.truth(cap, "default")
    done = set()
    for b, j in F.hostile_slots(cap):
        if b in done or not np.isfinite(t["cost"][b]).all():
            continue
        done.add(b)
        live = p[:, b].copy()
        live[0, j] = live[1, j]
        got = F.oracle_dp(live[:, None, :], v0[b:b + 1])
        assert not same_bits(got["cost"][0], t["cost"][b]), f"scene {names[b]}: the poison of slot {j} would go unnoticed"
    assert done or cap == 1 or not F.hostile_slots(cap)


def test_graph_cases_cover_their_branches(hc):
    seen = dict(inside=0, outside=0, reversed=0, kept_t1=0, kept_t8=0, dead=0, inf=0)
    for B, cap in ((64, 1), (64, 16), (150, 65), (150, 200)):
        g = F.graph_cases(B, cap)
        out = st.exact_generate_st_graph(*g)
        first = np.where(np.isnan(g[0]).any(axis=1), np.argmax(np.isnan(g[0]), axis=1), cap)
        assert (first == 0).any() and (first == cap).any() and (cap == 1 or ((first > 0) & (first < cap)).any())
        behind = np.arange(cap)[None, :] >= first[:, None]
        for o in out:
            assert np.isnan(o[behind]).all()
        seen["dead"] += int((behind & np.isfinite(g).all(axis=0) & (np.abs(g[3]) >= 0.3)).sum())   # live-looking data behind the NaN
        s_in, s_out, t_in, t_out = out
        seen["inside"] += int(((t_in == 0.0) & ~np.isnan(s_in)).sum())
        seen["outside"] += int((t_in > 0.0).sum())
        seen["reversed"] += int((s_out < s_in).sum())
        seen["inf"] += int((np.isinf(s_in) | np.isinf(s_out) | np.isinf(t_out)).sum())
        # the host build of st::st_graph agrees bit for bit
        got = [np.zeros((B, cap)) for _ in range(4)]
        for b in range(B):
            ins = [np.ascontiguousarray(g[i, b]) for i in range(4)]
            outs = [np.zeros(cap) for _ in range(4)]
            hc.hc_st_graph(cap, *[a.ctypes.data for a in ins], *[a.ctypes.data for a in outs])
            for i in range(4):
                got[i][b] = outs[i]
        for i in range(4):
            assert same_bits(got[i], out[i]), (B, cap, i)
    assert min(seen[k] for k in ("inside", "outside", "reversed", "dead", "inf")) > 0, seen
    e = F.graph_exact_rows()
    s_in, s_out, t_in, t_out = (o[0] for o in st.exact_generate_st_graph(*e))
    assert (t_in[0], t_out[0]) == (0.0, 4.0) and s_in[0] == 10.0 + 3.0 * 0.0          # t_min == 0: the else branch
    assert np.isnan(s_in[2]) and t_out[3] == 1.0 and t_in[4] == 8.0 and np.isnan(s_in[5])
    assert s_out[6] < s_in[6] and not np.isnan(s_in[7]) and not np.isnan(s_in[8]) and np.isnan(s_in[9])


def test_edge_cases_hold_every_kind():
    for cap in F.EDGE_CAPS:
        E, sets = F.edge_cases(cap)
        assert E.shape == (8, F.N_EDGES, 5) and sets.shape == (4, 8, cap) and F.N_EDGES % 64 != 0
        assert (E[:, :, 4] == E[:, :, 1]).any() and (E[:, :, 4] < E[:, :, 1]).any() and (E[:, :, 3] == E[:, :, 0]).any()
        assert np.isnan(E).any() and np.isinf(E).any() and (np.abs(E[np.isfinite(E)]) > 1e100).any()
        tot, obs = F.oracle_edges(E, sets)
        assert (obs > 0).any(axis=1).sum() >= 6
        if cap >= 32:          # samples exactly 0.5 / 1.5 beside a stationary segment cost nothing; every kind of edge costs somewhere
            for kind in (0, 1, 4, 5, 6, 7):
                assert (obs[:, kind::10] > 0).any(), (cap, kind)


def test_small_entry_point_inputs():
    d = F.collision_distances(1000)
    for x in (0.5, -0.5, 1.5, -1.5, F.up(0.5), F.down(1.5), 0.0):
        assert (d == x).any()
    assert np.isnan(d).any() and np.isinf(d).any()
    for n in F.SMALL_N:
        assert len(F.collision_distances(n)) == n and all(len(a) == n for a in F.start_condition_inputs(n))
    h = F.start_condition_inputs(1000)[4]
    assert {0.0, np.pi / 2, -np.pi, 1e6} <= set(h[np.isfinite(h)].tolist()) and np.isnan(h).any()
