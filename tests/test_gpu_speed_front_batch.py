"""The S-T speed front (emp_st_graph, emp_speed_dp, emp_st_edge_costs, emp_st_collision_cost, emp_speed_start_condition) on
the adversarial segment sets and ragged batches of tests/speed_front_cases.py, against oracle/st_speed.py.

Bars.  With w_cost_obs = 1 the obstacle term is an exact count of the (sample, obstacle) pairs within reach (1 ** y == 1 in
NumPy and on the kernels' route: make_pow_base(1) has a zero logarithm, exp2(0) == 1), so every output equals the oracle's bit
for bit: a dropped, doubled or misattributed pair, a wrong sample slot, < against <= at 0.5 or 1.5 and a wrong tie rule all
show.  With the reference's weights cost is compared at 1e-12 relative (scale 1.0; csrc/emp_st_core.h: pow is the one operation
that is not correctly rounded) and the predecessors, speeds, terminal node and profile are equal outright - the inputs have no
near-tie (tests/test_speed_front_cases_host.py).  Summation order inside one edge's obstacle term cannot be pinned tighter than
that while the device's power and NumPy's differ in the last place."""
import ctypes as C

import numpy as np
import pytest

from oracle import st_speed as st
from tests import batch_check as bc
from tests import speed_front_cases as F
from tests.conftest import make_planner

pytestmark = pytest.mark.gpu

DP_OUTS = ("cost", "s_dot", "node", "end_node", "speed_s", "speed_t")
ORACLE = dict(cost="cost", s_dot="s_dot", node="node", end_node="end", speed_s="speed_s", speed_t="speed_t")


@pytest.fixture(scope="module")
def pl():
    p = make_planner(0)
    yield p
    p.close()


def params(weights="default"):
    from emplanner_carla_amd.api import speed_dp_params
    return speed_dp_params(**F.WEIGHTS[weights])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def bad_rows(a, b):
    return [i for i in range(len(a)) if not same_bits(a[i], b[i])]


def assert_close(got, want, rtol, what, scale=1.0):
    """|got - want| <= rtol max(|want|, scale) where want is finite; the same bits (NaN to NaN) where it is not."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert same_bits(got[~fin], want[~fin]), f"{what}: a non-finite value differs"
    err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), scale)
    worst = float(err.max(initial=0.0))
    print(f"{what}: worst relative error {worst:.3g} (bar {rtol:g})")
    assert not np.isnan(got[fin]).any() and worst <= rtol, f"{what}: {worst:.3g} > {rtol:g}"


def run_dp(pl, sets, v0, weights="default", tables=True):
    r = pl.speed_dp(params(weights), *[np.ascontiguousarray(a) for a in sets], np.ascontiguousarray(v0), tables=tables)
    return {n: bc.to_np(getattr(r, n)) for n in DP_OUTS}


def check_dp_exact(got, want, names, what):
    for n in DP_OUTS:
        bad = bad_rows(got[n], want[ORACLE[n]])
        assert not bad, f"{what}: {n} of scenes {[(b, names[b]) for b in bad[:6]]} differs from the oracle"


def check_dp_default(got, want, names, what):
    for n in ("node", "s_dot", "end_node", "speed_s", "speed_t"):
        bad = bad_rows(got[n], want[ORACLE[n]])
        assert not bad, f"{what}: {n} of scenes {[(b, names[b]) for b in bad[:6]]} differs from the oracle"
    assert_close(got["cost"], want["cost"], 1e-12, f"{what}: cost")


# ---- emp_speed_dp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["count", "ties"])
@pytest.mark.parametrize("cap", F.CAPS)
def test_speed_dp_counts_the_pairs_within_reach_exactly(pl, cap, weights):
    """w_cost_obs = 1: everything bit-equal to the oracle; "ties" (no other weight) makes every cost a small integer, and the
    lowest source row wins each tie as in the reference's ordered strict-< scan.  The poisoned twin equals the clean batch."""
    names, sets, v0 = F.dp_cases(cap)
    got = run_dp(pl, sets, v0, weights)
    check_dp_exact(got, F.truth(cap, weights), names, f"{cap} slots, {weights}")
    twin = run_dp(pl, F.poisoned(cap), v0, weights)
    for n in DP_OUTS:
        assert not bad_rows(twin[n], got[n]), f"{cap} slots, {weights}: {n} changes with what absent slots hold"


@pytest.mark.parametrize("cap", F.CAPS)
def test_speed_dp_default_weights_vs_oracle_and_poisoned_twin(pl, cap):
    names, sets, v0 = F.dp_cases(cap)
    got = run_dp(pl, sets, v0)
    check_dp_default(got, F.truth(cap, "default"), names, f"{cap} slots")
    twin = run_dp(pl, F.poisoned(cap), v0)
    for n in DP_OUTS:
        assert not bad_rows(twin[n], got[n]), f"{cap} slots: {n} changes with what absent slots hold"
    # a NaN start (include/emplanner.h): column 0 NaN, +inf behind it, the top right node, a profile along row 0
    for b in np.flatnonzero(np.isnan(v0)):
        assert np.isnan(got["cost"][b, :, 0]).all() and np.isposinf(got["cost"][b, :, 1:]).all()
        assert tuple(got["end_node"][b]) == (0, 15) and (got["speed_s"][b] == 54.5).all()


def _dp_spec(cap, sets, v0, weights="default", tables=True):
    p = params(weights)
    row = F.hostile_guard_row(cap)
    tab = (st.N_ROWS, st.N_COLS)
    outs = {"cost": (tab, np.float64), "s_dot": (tab, np.float64), "node": (tab, np.int32), "end_node": ((2,), np.int32),
            "speed_s": ((st.N_COLS,), np.float64), "speed_t": ((st.N_COLS,), np.float64)}
    sig = [C.byref(p), "B", cap, "s_in", "s_out", "t_in", "t_out", "v0"] + (["cost", "s_dot", "node"] if tables else [None] * 3) + \
          ["end_node", "speed_s", "speed_t"]
    if not tables:
        outs = {n: outs[n] for n in ("end_node", "speed_s", "speed_t")}
    return dict(fn="emp_speed_dp", sig=sig, keep=p,
                ins={"s_in": (sets[0], row[0]), "s_out": (sets[1], row[1]), "t_in": (sets[2], row[2]), "t_out": (sets[3], row[3]),
                     "v0": (v0, 3.0)}, outs=outs)


@pytest.mark.parametrize("cap", F.CAPS)
def test_speed_dp_batch_invariance_and_guard_rows(pl, cap):
    """Host against device call, reversed, shifted and alone (batch_check.invariant); then the raw call between guard rows of
    finite hostile obstacles (inputs) and sentinels (outputs), with and without the tables, and B = 0."""
    names, sets, v0 = F.dp_cases(cap)

    def call(args, device):
        r = pl.speed_dp(params(), *args)
        if device:
            pl.synchronize()
        return {n: bc.to_np(getattr(r, n)) for n in DP_OUTS}

    full = bc.invariant(call, [np.ascontiguousarray(a) for a in sets] + [np.ascontiguousarray(v0)], f"speed_dp at {cap} slots")
    for tables in (True, False):
        g = bc.Guarded(pl, _dp_spec(cap, F.poisoned(cap), v0, tables=tables))
        got = g.call()
        g.check_guards(f"speed_dp at {cap} slots")
        for n, o in got.items():
            assert not bad_rows(o, full[n]), f"speed_dp at {cap} slots between guard rows (tables={tables}): {n}"
    g = bc.Guarded(pl, _dp_spec(cap, sets, v0), B=0)
    g.call()
    g.check_guards(f"speed_dp at {cap} slots, B = 0")
    empty = pl.speed_dp(params(), *[np.zeros((0, cap))] * 4, np.zeros(0))
    assert empty.cost.shape == (0, 40, 16) and empty.end_node.shape == (0, 2)


def test_speed_dp_heaviest_first_with_64_bit_masks(pl):
    """513 scenes at 40 slots: the launcher's heaviest-first order with the 64-bit instantiation.  Bit-equal to the same scenes
    in two chunks (no ordering below 513), to the oracle on a sample of 8, and with tables=False on device pointers."""
    import torch
    sets, v0 = F.big_batch()
    big = run_dp(pl, sets, v0)
    for sl in (slice(0, 257), slice(257, F.BIG_B)):
        small = run_dp(pl, sets[:, sl], v0[sl])
        for n in DP_OUTS:
            bad = bad_rows(big[n][sl], small[n])
            assert not bad, f"{n} of scenes {[sl.start + b for b in bad[:8]]} differs between the batch of 513 and its chunk"
    pick = list(F.BIG_SAMPLE)
    check_dp_default({n: big[n][pick] for n in DP_OUTS}, F.big_truth(), [f"scene {b}" for b in pick], "sample of the 513")
    dev = pl.speed_dp(params(), *[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in sets],
                      torch.from_numpy(np.ascontiguousarray(v0)).cuda(), tables=False)
    pl.synchronize()
    assert dev.cost is None and dev.s_dot is None and dev.node is None
    for n in ("end_node", "speed_s", "speed_t"):
        assert not bad_rows(bc.to_np(getattr(dev, n)), big[n]), n


# ---- emp_st_graph ---------------------------------------------------------------------------------------------------------
GRAPH_SHAPES = [(B, cap) for B in (64, 150) for cap in (1, 16, 65, 200)]


@pytest.fixture(scope="module")
def hc():
    from tests import host_check
    return host_check.load()


def _host_graph(hc, g):
    B, cap = g.shape[1:]
    out = np.zeros((4, B, cap))
    for b in range(B):
        ins = [np.ascontiguousarray(g[i, b]) for i in range(4)]
        outs = [np.zeros(cap) for _ in range(4)]
        hc.hc_st_graph(cap, *[a.ctypes.data for a in ins], *[a.ctypes.data for a in outs])
        out[:, b] = outs
    return out


@pytest.mark.parametrize("B,cap", GRAPH_SHAPES)
def test_st_graph_vs_oracle_and_host_build(pl, hc, B, cap):
    g = F.graph_cases(B, cap)
    what = f"st_graph B = {B}, {cap} slots"

    def call(args, device):
        r = pl.st_graph(*args)
        if device:
            pl.synchronize()
        return dict(zip(("s_in", "s_out", "t_in", "t_out"), (bc.to_np(x) for x in r)))

    got = bc.invariant(call, [np.ascontiguousarray(a) for a in g], what)
    want = st.exact_generate_st_graph(*g)
    host = _host_graph(hc, g)
    for i, n in enumerate(("s_in", "s_out", "t_in", "t_out")):
        assert not bad_rows(got[n], want[i]), f"{what}: {n} differs from the oracle"
        assert not bad_rows(got[n], host[i]), f"{what}: {n} differs from the host build of st::st_graph"
    first = np.where(np.isnan(g[0]).any(axis=1), np.argmax(np.isnan(g[0]), axis=1), cap)
    behind = np.arange(cap)[None, :] >= first[:, None]
    for n in got:
        assert np.isnan(got[n][behind]).all(), f"{what}: {n} is not NaN from the first NaN s on"
    fill = np.array([20.0, 1.0, 3.0, -0.5])          # a live obstacle in every guard slot
    spec = dict(fn="emp_st_graph", sig=["B", cap, "s", "l", "sd", "ld", "s_in", "s_out", "t_in", "t_out"],
                ins={k: (g[i], fill[i]) for i, k in enumerate(("s", "l", "sd", "ld"))},
                outs={k: ((cap,), np.float64) for k in ("s_in", "s_out", "t_in", "t_out")})
    gd = bc.Guarded(pl, spec)
    raw = gd.call()
    gd.check_guards(what)
    for n in raw:
        assert not bad_rows(raw[n], got[n]), f"{what} between guard rows: {n}"
    g0 = bc.Guarded(pl, spec, B=0)
    g0.call()
    g0.check_guards(what + ", B = 0")


def test_st_graph_threshold_rows(pl):
    e = F.graph_exact_rows()
    got = pl.st_graph(*e)
    want = st.exact_generate_st_graph(*e)
    for i in range(4):
        assert same_bits(got[i], want[i])
    assert got[3][0, 3] == 1.0 and got[2][0, 4] == 8.0 and got[2][0, 0] == 0.0 and got[0][0, 0] == 10.0


@pytest.mark.parametrize("weights", ["count", "default"])
def test_speed_dp_on_the_graphs_own_segments(pl, weights):
    """generate_st_graph's own output (reversed and non-finite segments included) through the speed DP at 16 slots."""
    g = F.graph_cases(*F.GRAPH_DP)
    sets, v0 = F.graph_dp_inputs()
    dev_sets = pl.st_graph(*[np.ascontiguousarray(a) for a in g])
    for i in range(4):
        assert same_bits(dev_sets[i], sets[i])
    got = run_dp(pl, dev_sets, v0, weights)
    names = [f"row {b}" for b in range(len(v0))]
    (check_dp_exact if weights == "count" else check_dp_default)(got, F.graph_dp_truth(weights), names, f"graph output, {weights}")


# ---- emp_st_edge_costs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", F.EDGE_CAPS)
def test_edge_costs_of_arbitrary_edges(pl, cap):
    E, sets = F.edge_cases(cap)
    E, sets = np.ascontiguousarray(E), [np.ascontiguousarray(a) for a in sets]
    what = f"edge costs at {cap} slots"
    tot, obs = pl.st_edge_costs(params("count"), E, *sets)
    wt, wo = F.edge_truth(cap, "count")
    for name, a, b in (("total", tot, wt), ("obs", obs, wo)):
        bad = np.argwhere(~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
        assert not len(bad), f"{what}, w_cost_obs = 1: {name} differs at (scene, edge) {bad[:8].tolist()}"
    tot, obs = pl.st_edge_costs(params(), E, *sets)
    wt, wo = F.edge_truth(cap, "default")
    assert_close(tot, wt, 1e-12, f"{what}: total")
    assert_close(obs, wo, 1e-12, f"{what}: obs")
    # between guard rows: hostile finite obstacles and edges around the batch, sentinels around the outputs
    p = params()
    row = F.hostile_guard_row(cap)
    for n_edges in (F.N_EDGES, 1, 0):
        spec = dict(fn="emp_st_edge_costs", sig=[C.byref(p), "B", n_edges, cap, "edges", "s_in", "s_out", "t_in", "t_out", "total", "obs"],
                    ins={"edges": (E[:, :max(n_edges, 1)] if n_edges else np.zeros((8, 1, 5)), 5.0), "s_in": (sets[0], row[0]),
                         "s_out": (sets[1], row[1]), "t_in": (sets[2], row[2]), "t_out": (sets[3], row[3])},
                    outs={"total": ((max(n_edges, 1),), np.float64), "obs": ((max(n_edges, 1),), np.float64)})
        g = bc.Guarded(pl, spec)
        raw = g.call()
        g.check_guards(f"{what}, {n_edges} edges")
        if n_edges:
            assert same_bits(raw["total"], tot[:, :n_edges]) and same_bits(raw["obs"], obs[:, :n_edges]), (what, n_edges)
        else:
            assert (raw["total"] == bc.F_GUARD).all() and (raw["obs"] == bc.F_GUARD).all(), f"{what}: no edge, yet an output was written"
    g = bc.Guarded(pl, spec, B=0)
    g.call()
    g.check_guards(what + ", B = 0")
    t0, o0 = pl.st_edge_costs(params(), np.zeros((8, 0, 5)), *sets)
    assert t0.shape == (8, 0) and o0.shape == (8, 0)


def test_edge_costs_device_call_and_refusals(pl):
    import torch
    E, sets = F.edge_cases(33)
    host = pl.st_edge_costs(params(), np.ascontiguousarray(E), *[np.ascontiguousarray(a) for a in sets])
    dev = pl.st_edge_costs(params(), torch.from_numpy(np.ascontiguousarray(E)).cuda(),
                           *[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in sets])
    pl.synchronize()
    assert same_bits(bc.to_np(dev[0]), host[0]) and same_bits(bc.to_np(dev[1]), host[1])
    p = params()
    one = np.zeros(8)
    out = np.zeros(8)
    ptr = lambda a: a.ctypes.data
    from emplanner_carla_amd import _lib as L
    for B, n_edges, cap in ((65536, 0, 1), (1, 1, 65)):
        rc = pl._lib.emp_st_edge_costs(pl._h, C.byref(p), B, n_edges, cap, ptr(one), ptr(one), ptr(one), ptr(one), ptr(one), ptr(out),
                                       ptr(out), L.EMP_HOST)
        assert rc != 0, f"B = {B}, max_obs = {cap} was not refused"
    with pytest.raises(Exception):
        pl.st_edge_costs(params(), np.zeros((1, 1, 5)), *[np.zeros((1, 65))] * 4)
    with pytest.raises(Exception):
        pl.speed_dp(params(), *[np.zeros((1, 65))] * 4, np.zeros(1))


# ---- the two small entry points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.SMALL_N)
def test_collision_cost_around_its_thresholds(pl, n):
    import torch
    d = F.collision_distances(n)
    band = F.in_band(d)
    for w in (10000000.0, 1.0, 0.0, np.inf):
        got = pl.st_collision_cost(w, d)
        want = st.exact_collision_cost(w, d)
        assert got.shape == (n,)
        assert same_bits(got[~band], want[~band]), f"base {w}: a cost outside the band differs"
        assert_close(got[band], want[band], 1e-13, f"collision cost, n = {n}, base {w}, in the band")
        if n:       # (an empty torch tensor has a NULL data pointer, which every entry point refuses: n = 0 on device pointers is
            dev = pl.st_collision_cost(w, torch.from_numpy(d).cuda())       # the guarded call below)
            pl.synchronize()
            assert same_bits(bc.to_np(dev), got)
        spec = dict(fn="emp_st_collision_cost", sig=["B", w, "d", "cost"], ins={"d": (d, 0.2)}, outs={"cost": ((), np.float64)})
        g = bc.Guarded(pl, spec, B=n)
        raw = g.call()
        g.check_guards(f"collision cost, n = {n}")
        assert same_bits(raw["cost"], got)


@pytest.mark.parametrize("n", F.SMALL_N)
def test_start_condition_headings(pl, n):
    import torch
    x = F.start_condition_inputs(n)
    s1, s2 = pl.speed_start_condition(*x)
    w1, w2 = F.start_condition_truth(*x)
    assert s1.shape == (n,) and s2.shape == (n,)
    for got, want, ops in ((s1, w1, x[:2]), (s2, w2, x[2:4])):
        want = np.asarray(want, dtype=np.float64)
        assert_close(got, want, 1e-13, f"start condition, n = {n}", scale=float(np.abs(ops).max(initial=1.0)))
    if n:           # (n = 0 on device pointers: the guarded call below)
        dev = pl.speed_start_condition(*[torch.from_numpy(a).cuda() for a in x])
        pl.synchronize()
        assert same_bits(bc.to_np(dev[0]), s1) and same_bits(bc.to_np(dev[1]), s2)
    spec = dict(fn="emp_speed_start_condition", sig=["B", "vx", "vy", "ax", "ay", "h", "s1", "s2"],
                ins={k: (a, 7.0) for k, a in zip(("vx", "vy", "ax", "ay", "h"), x)},
                outs={"s1": ((), np.float64), "s2": ((), np.float64)})
    g = bc.Guarded(pl, spec, B=n)
    raw = g.call()
    g.check_guards(f"start condition, n = {n}")
    assert same_bits(raw["s1"], s1) and same_bits(raw["s2"], s2)
