"""emp_path_qp (path_qp_wave_kernel) on the hard corridors of tests/path_qp_cases.py: below 9 stations, on either side of the
switch between the register-resident solver (n <= 66: one unknown per lane) and the LDS-resident one (n >= 67), up to the 256
stations the call accepts - one ragged call per capacity, feasible and infeasible scenes side by side, NaN beyond every scene's
count.  The yardstick is the dense reference formulation (oracle.ref_port.path_qp_matrices -> oracle.qp_dense), checked on the CPU
by tests/test_path_qp_cases_host.py; a scene the oracle could not certify is compared with nothing and counted.

Pinch family (one station between bounds 1e-6 m apart): compared at 1e-6 of half the host width, the magnitude of the bounds the
solution rests on, and without the stationarity bound.  Measured deviation from the oracle, max over l, dl, ddl and the family's
cases of a size, kernel | CPU interior point (tests/host_check, the same algorithm in another summation order):
    n = 8: 3.9e-16 | 3.9e-16      n = 34: 1.4e-14 | 1.4e-14      n = 35: 1.6e-14 | 1.6e-14      n = 66 (registers): 3.3e-15 | 3.3e-15
    n = 67 (LDS): 1.3e-15 | 1.4e-15      n = 68 (LDS): 1.9e-15 | 2.2e-15      n = 100: 3.2e-15 | 3.2e-15      n = 256: 6.2e-15 | 5.8e-15
(metres, MI355X; on these corridors the iteration has room to converge and both stay eight orders below the bar).  Most
interior-point iterations on the chicane, random, pinch and start-on-a-bound corridors: 0 at n = 4, 9 | 8 | 7 | 8 at n = 5 .. 8,
10 at n = 34 and 35, 13 at n = 66, 67, 68, 100 and 256 (the cap is 60).

The count contract of emp_path_qp and emp_smooth_line, and the smoother's minimum size, are at the end of the file."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import qp_dense
from oracle import ref_port as rp
from tests import batch_check as BC
from tests import path_qp_cases as F
from tests.conftest import assert_rel, make_planner

pytestmark = pytest.mark.gpu

RTOL = 1e-6
MAX_ITER = 60                     # kQpMaxIter of emp_qp_core.h
ST_QP_FAILED, ST_SMOOTH_FAILED = 8, 16      # EMP_ST_* of include/emplanner.h
NAN = np.nan
CAPS = (8, 68, 256)
HARD = ("chicane", "random", "pinch", "bound")


@pytest.fixture(scope="module")
def planner():
    pl = make_planner()
    yield pl
    pl.close()


def qp():
    from emplanner_carla_amd.api import qp_params
    return qp_params()


def batch_names(cap):
    """The scenes of one call: every case of the sizes this capacity is there for, a few of the smaller ones mixed in, the
    infeasible ones spread evenly between the feasible ones.  Names "short<k>" are open corridors of k < 4 stations."""
    cs = F.cases()
    if cap == 8:
        names = [c.name for c in cs.values() if c.n <= 8] + [f"short{k}" for k in range(4)]
    elif cap == 68:
        names = [c.name for c in cs.values() if 34 <= c.n <= 68] + ["random_seed46_n5", "inspect_empty_n7", "pinch_gap_n8", "short3"]
    else:
        names = [c.name for c in cs.values() if c.n >= 100] + \
                [c.name for c in cs.values() if c.n in (66, 67, 68) and c.family in ("chicane", "spline", "pinch")] + \
                ["chicane_narrow_n6", "inspect_start_n4", "offset_start_n4", "short0", "short2"]
    fails = lambda name: name.startswith("short") or cs[name].expectation == "infeasible"
    good, bad = [n for n in names if not fails(n)], [n for n in names if fails(n)]
    step = max(1, len(good) // len(bad))
    out = []
    for i, name in enumerate(good):
        out.append(name)
        if i % step == step - 1 and bad:
            out.append(bad.pop(0))
    return out + bad


def batch_arrays(names, cap):
    B = len(names)
    l_min, l_max = np.full((B, cap), NAN), np.full((B, cap), NAN)
    n_pts, start = np.zeros(B, np.int32), np.zeros((B, 3))
    for b, name in enumerate(names):
        if name.startswith("short"):
            n = int(name[5:])
            l_min[b, :n], l_max[b, :n], start[b] = -F.WIDE, F.WIDE, (0.1, 0.0, 0.0)
        else:
            c = F.cases()[name]
            n = c.n
            l_min[b, :n], l_max[b, :n], start[b] = c.l_min, c.l_max, c.start_l3
        n_pts[b] = n
    return l_min, l_max, n_pts, start


@pytest.mark.parametrize("cap", CAPS)
def test_path_qp_on_the_case_set(planner, cap):
    names = batch_names(cap)
    l_min, l_max, n_pts, start = batch_arrays(names, cap)
    assert n_pts.max() == cap and len(set(n_pts.tolist())) >= 5
    if cap == 68:
        assert (n_pts == 66).any() and (n_pts == 67).any()         # both solver tiers in one launch
    l, dl, ddl, iters, st = planner.path_qp(qp(), l_min, l_max, n_pts, start)
    compared = meant = failed = 0
    worst_iters, pinch_dev = {}, {}
    for b, name in enumerate(names):
        n = int(n_pts[b])
        if name.startswith("short"):
            assert st[b] == ST_QP_FAILED, f"{name}: {n} stations must fail, status {st[b]}"
            failed += 1
            continue
        c = F.cases()[name]
        verdict, x, _ = F.truth(name)
        meant += c.expectation == "feasible"
        if verdict == "uncertified":
            continue
        if verdict == "infeasible":
            assert st[b] == ST_QP_FAILED, f"{name}: infeasible, status {st[b]} after {iters[b]} iterations"
            failed += 1
            continue
        got = np.stack([l[b, :n], dl[b, :n], ddl[b, :n]], axis=1)
        dev = float(np.abs(got - x).max()) if st[b] == 0 else NAN
        print(f"{name}: status {st[b]}, {iters[b]} iterations, max deviation {dev:.2e}")
        assert st[b] == 0, f"{name}: status {st[b]}"
        assert iters[b] <= MAX_ITER, f"{name}: {iters[b]} iterations"
        pinch = c.family == "pinch"
        for k, what in enumerate(("l", "dl", "ddl")):
            assert_rel(got[:, k], x[:, k], RTOL, f"{name}: {what}", scale=F.HALF_W if pinch else None)
        cert = qp_dense.kkt_certificate(*F.matrices(c), got.reshape(-1))
        assert cert["ineq_violation"] < 1e-9 and cert["eq_violation"] < 1e-9, f"{name}: {cert}"
        assert pinch or cert["stationarity"] < 1e-7, f"{name}: {cert}"
        if c.n == 4:
            assert got[3, 0] == 0.0 and iters[b] == 0              # nothing free: the constant forms are checked, nothing is solved
        if c.family in HARD:
            worst_iters[n] = max(worst_iters.get(n, 0), int(iters[b]))
        if pinch:
            pinch_dev[n] = max(pinch_dev.get(n, 0.0), dev)
        compared += 1
    print(f"capacity {cap}: compared {compared} of {meant} feasible scenes, {failed} failing scenes; most iterations on the hard "
          f"corridors per size {worst_iters}; pinch deviation per size {pinch_dev}")
    assert compared >= 0.9 * meant and failed >= 4
    padded = np.arange(cap)[None, :] >= n_pts[:, None]
    for o in (l, dl, ddl):
        assert not o[padded].any(), "an output slot beyond a scene's count was written"


INVARIANT = ("chicane_alt_n66", "chicane_alt_n67", "inspect_empty_n67", "random_seed68_n68", "pinch_gap_n34", "random_seed46_n5",
             "spline_ramp_n66", "pinch_gap_n8", "short3", "random_seed35_n35", "spline_stairs_n68", "offset_start_n4")


def test_path_qp_batch_independence(planner):
    """Bit for bit the same alone, reversed, shifted by one and on the device path: failing scenes beside passing ones, both
    solver tiers (66 | 67 stations) in one batch.  No oracle here."""
    l_min, l_max, n_pts, start = batch_arrays(INVARIANT, 68)
    q = qp()

    def call(args, device):
        out = planner.path_qp(q, *args)
        if device:
            planner.synchronize()
        return dict(zip(("l", "dl", "ddl", "iters", "status"), (BC.to_np(o) for o in out)))

    full = BC.invariant(call, [l_min, l_max, n_pts, start], "emp_path_qp")
    st = full["status"]
    assert (st == 0).sum() >= 6 and (st == ST_QP_FAILED).sum() >= 4 and set(st.tolist()) == {0, ST_QP_FAILED}
    assert st[list(INVARIANT).index("chicane_alt_n66")] == 0 and st[list(INVARIANT).index("chicane_alt_n67")] == 0


# ---------------------------------------------------------------------------------------------------------------------
# count contract (include/emplanner.h: a per-scene count beyond its row's capacity is clamped, never followed)
# ---------------------------------------------------------------------------------------------------------------------
def _ragged_counts(rng, B, cap, lo):
    n = rng.integers(lo, cap + 1, B).astype(np.int32)
    n[1], n[2], n[3] = 0, 1, 3
    n[0] = n[-1] = n[B // 2] = cap            # the wild scenes hold a whole row of data: clamped, they solve it
    return n


@functools.lru_cache(maxsize=None)
def qp_count_spec(cap):
    """Random corridors filling every row to the capacity (so that a clamped count finds a problem), ragged counts, NaN guards."""
    B = 12
    rng = np.random.default_rng(cap)
    l_min, l_max, start = np.empty((B, cap)), np.empty((B, cap)), np.empty((B, 3))
    for b in range(B):
        l_min[b], l_max[b], start[b] = F.random_case(cap, 7000 + 100 * cap + b)
    q = qp()
    row = lambda: ((cap,), np.float64)
    return dict(fn="emp_path_qp", sig=[C.byref(q), "B", cap, "lo", "hi", "n", "s3", "l", "dl", "ddl", "it", "st"], keep=q,
                ins={"lo": (l_min, NAN), "hi": (l_max, NAN), "n": (_ragged_counts(rng, B, cap, 4), 0), "s3": (start, NAN)},
                outs={"l": row(), "dl": row(), "ddl": row(), "it": ((), np.int32), "st": ((), np.int32)}, counts={"n": cap})


@functools.lru_cache(maxsize=None)
def smooth_count_spec(cap):
    from emplanner_carla_amd.api import smooth_params
    B = 12
    rng = np.random.default_rng(100 + cap)
    t = np.arange(cap) * 2.0
    xy = np.stack([np.stack([t * np.cos(0.2 * b) + rng.normal(0, 0.12, cap),
                             t * np.sin(0.2 * b) + 10 * np.sin(t / 35.0) + rng.normal(0, 0.12, cap)], axis=1) for b in range(B)])
    sp = smooth_params()
    return dict(fn="emp_smooth_line", sig=[C.byref(sp), "B", cap, "xy", "n", "out", "it", "st"], keep=sp,
                ins={"xy": (xy, NAN), "n": (_ragged_counts(rng, B, cap, 2), 0)},
                outs={"out": ((cap, 4), np.float64), "it": ((), np.int32), "st": ((), np.int32)}, counts={"n": cap})


@pytest.mark.parametrize("cap", [24, 68])
def test_path_qp_counts_beyond_capacity_are_clamped(planner, cap):
    spec = qp_count_spec(cap)
    B = len(spec["ins"]["n"][0])
    BC.check_count_contract(planner, spec, (B // 2, B // 3), f"emp_path_qp, capacity {cap}")
    g = BC.Guarded(planner, spec)
    wild = np.array(spec["ins"]["n"][0])
    wild[[B // 2, B - 1]] = cap + 3
    wild[B // 3] = -1
    g.set_count("n", wild)
    out = g.call()
    # clamped to the capacity the scene is the row's whole problem - solved, or refused for what the corridor is, as at n = cap
    full = planner.path_qp(spec["keep"], spec["ins"]["lo"][0], spec["ins"]["hi"][0], np.full(B, cap, np.int32), spec["ins"]["s3"][0])
    for b in (B // 2, B - 1):
        assert out["st"][b] == full[4][b] and BC.bits(out["l"][b]) == BC.bits(full[0][b])
    assert (out["st"][[B // 2, B - 1]] == 0).all(), "a count beyond the capacity is the whole row, solved"
    assert out["st"][B // 3] == ST_QP_FAILED and not out["l"][B // 3].any()      # -1 -> 0 stations: below the stage's minimum
    assert (out["st"][[1, 2, 3]] == ST_QP_FAILED).all()                          # 0, 1, 3 stations


@pytest.mark.parametrize("cap", [24, 100])
def test_smooth_line_counts_beyond_capacity_are_clamped(planner, cap):
    spec = smooth_count_spec(cap)
    B = len(spec["ins"]["n"][0])
    BC.check_count_contract(planner, spec, (B // 2, B // 3), f"emp_smooth_line, capacity {cap}")
    g = BC.Guarded(planner, spec)
    wild = np.array(spec["ins"]["n"][0])
    wild[[B // 2, B - 1]] = cap + 3
    wild[B // 3] = -1
    g.set_count("n", wild)
    out = g.call()
    assert (out["st"][[B // 2, B - 1]] == 0).all(), "a count beyond the capacity is the whole row, smoothed"
    want = np.asarray(rp.smooth_reference_line([tuple(p) for p in spec["ins"]["xy"][0][B - 1]]), dtype=np.float64)
    assert_rel(out["out"][B - 1][:, :2], want[:, :2], RTOL, "the clamped last scene")
    assert out["st"][B // 3] == ST_SMOOTH_FAILED and not out["out"][B // 3].any()


def test_smooth_line_minimum_size(planner):
    """m = 0, 1, 2, 3 points against the port: EMP_ST_SMOOTH_FAILED where smooth_reference_line raises, its answer where it has one."""
    from emplanner_carla_amd.api import smooth_params
    rng = np.random.default_rng(9)
    cap = 5
    xy = np.full((4, cap, 2), NAN)
    n_pts = np.arange(4, dtype=np.int32)
    raised = []
    for m in range(4):
        pts = np.stack([np.arange(m) * 2.0 + rng.normal(0, 0.1, m), rng.normal(0, 0.1, m)], axis=1)
        xy[m, :m] = pts
    out, iters, st = planner.smooth_line(smooth_params(), xy, n_pts)
    for m in range(4):
        try:
            want = np.asarray(rp.smooth_reference_line([tuple(p) for p in xy[m, :m]]), dtype=np.float64)
        except (ValueError, IndexError):
            raised.append(m)
            assert st[m] == ST_SMOOTH_FAILED, f"{m} points: the port raises, status {st[m]}"
            assert not out[m].any()
            continue
        assert st[m] == 0, f"{m} points: status {st[m]}"
        assert_rel(out[m, :m, :2], want[:, :2], RTOL, f"{m} points: smoothed xy")
        assert_rel(out[m, :m, 2], want[:, 2], RTOL, f"{m} points: theta")
        assert_rel(out[m, :m, 3], want[:, 3], RTOL, f"{m} points: kappa")
        assert not out[m, m:].any()
    assert raised == [0, 1]
