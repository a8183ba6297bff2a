"""CPU checks of the kernels' scalar building blocks (csrc/emp_core.h, emp_qp_core.h, emp_frenet_core.h).

The headers are plain C++ that hipcc compiles into the kernels; here g++ compiles the same text
into a test-only library (tests/host_check) so the *logic* - the B-spline reformulation of the path
QP, the banded interior point, the Frenet helpers, the edge arithmetic - is compared with the oracle
without a GPU.  This is host-logic coverage, not the GPU parity proof (tests/test_gpu_*.py).
"""
import ctypes as C

import numpy as np
import pytest

from emplanner_carla_amd import scenes as S
from oracle import exact as ex
from oracle import qp_dense
from oracle import ref_port as op
from tests import host_check
from tests.conftest import assert_rel, load_golden

QP_PRM = np.array([2.0, 1000.0, 3000.0, 150.0, 250.0, 3.0, 3.0, 3.0])   # ds, w_l, w_ddl, w_dddl, w_centre, d1, d2, w


@pytest.fixture(scope="module")
def hc():
    return host_check.load()


def _path_qp(hc, l_min, l_max, start3, prm=QP_PRM, solver="ipm"):
    n = len(l_min)
    l_min = np.ascontiguousarray(l_min, dtype=np.float64)
    l_max = np.ascontiguousarray(l_max, dtype=np.float64)
    prm = np.ascontiguousarray(prm, dtype=np.float64)
    out = [np.zeros(n) for _ in range(3)]
    it = C.c_int(0)
    fn = hc.hc_path_qp if solver == "ipm" else hc.hc_path_qp_gi      # interior point / dual active set
    rc = fn(n, l_min.ctypes.data, l_max.ctypes.data, *[float(v) for v in start3], prm.ctypes.data,
                       out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, C.byref(it))
    return rc, out, it.value


@pytest.mark.parametrize("fname", ["cycle_cfg2_40x9_8obs.npz", "cycle_default_6x12_3obs.npz",
                                   "cycle_cfg1_20x5_0obs.npz", "cycle_default_6x12_3obs_t7.npz"])
@pytest.mark.parametrize("solver", ["ipm", "gi"])
def test_bspline_path_qp_matches_reference_formulation(hc, fname, solver):
    """Banded B-spline solvers (interior point, dual active set) == dense solve of the reference's own (H, f, G, h, Aeq, beq)."""
    g = load_golden(fname)
    n_ok = 0
    for i in range(len(g["seeds"])):
        if np.isnan(g["l_min"][i, 0]):
            continue
        nq = int(g["n_qp"][i])
        rc, (l, dl, ddl), iters = _path_qp(hc, g["l_min"][i, :nq], g["l_max"][i, :nq], g["start"][i, 1:], solver=solver)
        if g["status"][i] == 4:
            assert rc != 0, "oracle says infeasible, banded solver must not claim success"
            continue
        assert rc == 0 and iters <= 40
        assert_rel(l, g["qp_l"][i, :nq], 1e-8, "qp_l", scale=1.0)
        assert_rel(dl, g["qp_dl"][i, :nq], 1e-8, "qp_dl", scale=1.0)
        assert_rel(ddl, g["qp_ddl"][i, :nq], 1e-8, "qp_ddl", scale=1.0)
        n_ok += 1
    assert n_ok >= 6


@pytest.mark.parametrize("solver", ["ipm", "gi"])
def test_path_qp_kkt_certificate_on_random_corridors(hc, solver):
    """Certificate against the reference's dense formulation on corridors the goldens do not hold."""
    rng = np.random.default_rng(11)
    checked = 0
    for trial in range(40):
        n = int(rng.integers(8, 60))
        l_min = -10.0 * np.ones(n)
        l_max = 10.0 * np.ones(n)
        for _ in range(int(rng.integers(0, 4))):
            a = int(rng.integers(4, max(5, n - 6)))
            w = int(rng.integers(1, 4))
            if rng.random() < 0.5:
                l_max[a:a + w] = rng.uniform(0.5, 4.0)
            else:
                l_min[a:a + w] = rng.uniform(-4.0, -0.5)
        start3 = (rng.uniform(-0.4, 0.4), rng.uniform(-0.05, 0.05), rng.uniform(-0.01, 0.01))
        rc, (l, dl, ddl), iters = _path_qp(hc, l_min, l_max, start3, solver=solver)
        H, f, G, h, A, b = op.path_qp_matrices(l_min, l_max, *start3)
        ref = qp_dense.solve_qp(H, f, G, h, A, b)
        if ref.status != "optimal":
            assert rc != 0
            continue
        assert rc == 0
        x = np.stack([l, dl, ddl], axis=1).reshape(-1)
        cert = qp_dense.kkt_certificate(H, f, G, h, A, b, x)
        assert cert["stationarity"] < 1e-7 and cert["ineq_violation"] < 1e-9 and cert["eq_violation"] < 1e-9
        assert_rel(x, ref.x, 1e-7, "x vs dense oracle", scale=1.0)
        checked += 1
    assert checked >= 20


@pytest.mark.parametrize("solver", ["ipm", "gi"])
def test_path_qp_rejects_infeasible_and_tiny(hc, solver):
    import functools
    _path_qp_s = functools.partial(_path_qp, solver=solver)
    n = 12
    rc, _, _ = _path_qp_s(hc, 2.0 * np.ones(n), -2.0 * np.ones(n), (0, 0, 0))       # empty corridor
    assert rc == 1
    rc, _, _ = _path_qp_s(hc, -10 * np.ones(n), 10 * np.ones(n), (9.5, 0.0, 0.0))   # pinned start outside
    assert rc == 1
    lmax = 10 * np.ones(n)
    lmax[n - 1] = -5.0                               # pinned end (l = 0) above the last stations' upper bound
    rc, _, _ = _path_qp_s(hc, -10 * np.ones(n), lmax, (0, 0, 0))
    assert rc == 1
    rc, _, _ = _path_qp_s(hc, -10 * np.ones(3), 10 * np.ones(3), (0, 0, 0))         # n < 4: start/end overlap
    assert rc == 2
    rc, (l, dl, ddl), _ = _path_qp_s(hc, -10 * np.ones(4), 10 * np.ones(4), (0.3, 0.01, 0.0))   # n = 4: no freedom
    assert rc == 0 and abs(l[0] - 0.3) < 1e-15 and l[3] == 0.0


def _box_qp(hc, ref, thr=0.2, w=(0.4, 0.3, 0.3)):
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    out = np.zeros(len(ref))
    it = C.c_int(0)
    rc = hc.hc_box_qp(len(ref), ref.ctypes.data, 1, w[0], w[1], w[2], thr, out.ctypes.data, C.byref(it))
    return rc, out, it.value


def test_box_qp_matches_reference_smoothing(hc):
    """x and y solved separately == the reference's joint 2m-variable QP (unique minimiser)."""
    rng = np.random.default_rng(3)
    for m in (2, 3, 5, 23, 51, 130):
        pts = np.cumsum(rng.normal(0, 1.2, (m, 2)), axis=0) + rng.uniform(-300, 300, 2)
        H, f, G, h = op.smooth_qp_matrices([tuple(p) for p in pts])
        ref = qp_dense.solve_qp(H, f, G, h)
        assert ref.status == "optimal"
        for c in range(2):
            rc, x, iters = _box_qp(hc, pts[:, c])
            assert rc == 0 and iters <= 40
            assert_rel(x, ref.x[c::2], 1e-9, f"coordinate {c}, m={m}", scale=1.0)
    # golden: the smoothed trajectory of the reference cycle (x, y columns)
    g = load_golden("cycle_cfg2_40x9_8obs.npz")
    f0 = load_golden("qp_formulation.npz")
    tgt = (-f0["smooth_q"].reshape(-1) / 0.6)          # f = -2 * 0.3 * x_ref
    for c in range(2):
        rc, x, _ = _box_qp(hc, tgt[c::2])
        m = int(g["traj_len"][0])
        assert rc == 0
        assert_rel(x, g["traj"][0, :m, c], 1e-9, "golden trajectory", scale=1.0)


def test_heading_kappa_and_s_map(hc):
    g = load_golden("functions.npz")
    xy = np.ascontiguousarray(g["hk_xy"])
    th = np.zeros(len(xy))
    kp = np.zeros(len(xy))
    hc.hc_heading_kappa(xy.ctypes.data, len(xy), th.ctypes.data, kp.ctypes.data)
    assert_rel(th, g["hk_theta"], 1e-12, "theta", scale=1.0)
    assert_rel(kp, g["hk_kappa"], 1e-9, "kappa", scale=1.0)
    line = np.ascontiguousarray(g["mp_path"][:80])
    sm = np.zeros(80)
    hc.hc_s_map(line.ctypes.data, 80, 7.3, 2.0, sm.ctypes.data)
    assert_rel(sm, g["sm_out"], 1e-12, "s_map", scale=1.0)
    # matching with both early exits (50 on a first run, 5 in windowed mode)
    full = np.ascontiguousarray(g["mp_path"])
    for (x, y), want in zip(g["mp_pts"], g["mp_index"]):
        assert hc.hc_match(full.ctypes.data, len(full), x, y, 0, 1, 50) == want


def test_segment_cost_bit_exact_with_exact_oracle(hc):
    g = load_golden("cycle_default_6x12_3obs.npz")
    cfg = S.CFG_DEFAULT
    for sd in range(4):
        k = int(g["in_n_obs"][sd])
        obs_s = np.ascontiguousarray(g["obs_s"][sd, :k])
        obs_l = np.ascontiguousarray(g["obs_l"][sd, :k])
        c0, e = ex.edge_costs(obs_s[None], obs_l[None], np.array([k]), g["start"][sd:sd + 1], cfg.row, cfg.col,
                              cfg.sample_s, cfg.sample_l)
        ps, pl, pdl, pddl = g["start"][sd]
        for i in range(cfg.row):
            l1 = ((cfg.row + 1) / 2 - 1 - i) * cfg.sample_l
            v = hc.hc_segment_cost(pl, pdl, pddl, l1, ps, cfg.sample_s, obs_s.ctypes.data, obs_l.ctypes.data, k,
                                   1e12, 300.0, 1000.0, 5000.0, 20.0)
            assert v == c0[0, i]
        for (j, i, kk) in ((1, 0, 0), (3, 11, 2), (5, 4, 9)):
            l0 = ((cfg.row + 1) / 2 - 1 - kk) * cfg.sample_l
            l1 = ((cfg.row + 1) / 2 - 1 - i) * cfg.sample_l
            # neighbour edges: the factorised jerk term (emp_core.h neighbour_cost = what the edge kernels tabulate)
            v = hc.hc_neighbour_cost(l0, l1, ps + j * cfg.sample_s, cfg.sample_s, obs_s.ctypes.data,
                                     obs_l.ctypes.data, k, 1e12, 300.0, 1000.0, 5000.0, 20.0)
            assert v == e[0, j - 1, i, kk]
            # ... which is the general form (start edges) to a few units in the last place
            w = hc.hc_segment_cost(l0, 0.0, 0.0, l1, ps + j * cfg.sample_s, cfg.sample_s, obs_s.ctypes.data,
                                   obs_l.ctypes.data, k, 1e12, 300.0, 1000.0, 5000.0, 20.0)
            assert abs(v - w) <= 1e-13 * abs(w)


# ---- S-T speed DP scalar pieces (csrc/emp_st_core.h; reference planner/speed_planning_test.py) ---------------
def test_st_core_grid_graph_and_edges_vs_reference_golden(hc):
    from oracle import st_speed
    g = load_golden("speed.npz")
    ptr = lambda a: a.ctypes.data
    s_rows, t_cols = np.zeros(40), np.zeros(16)
    hc.hc_st_grid(ptr(s_rows), ptr(t_cols))
    np.testing.assert_array_equal(s_rows, g["s_list"][::-1])
    np.testing.assert_array_equal(t_cols, g["t_list"])
    # generate_st_graph: bit-exact against the reference on all 64 obstacle sets
    for b in range(g["graph_in"].shape[1]):
        ins = [np.ascontiguousarray(g["graph_in"][i, b]) for i in range(4)]
        outs = [np.zeros(16) for _ in range(4)]
        hc.hc_st_graph(16, *[ptr(a) for a in ins], *[ptr(a) for a in outs])
        for i in range(4):
            np.testing.assert_array_equal(outs[i], g["graph_out"][i, b])
    # CalcObsCost / CalcDpCost on the reference's edges
    w4 = np.array([50.0, 4000.0, 100.0, 10000000.0])
    for n, b in enumerate(g["edge_sets"]):
        sets = [np.ascontiguousarray(g["graph_out"][i, b]) for i in range(4)]
        for e, want in zip(g["obs_edges"][n], g["obs_cost"][n]):
            edge = np.array([e[0], e[1], 0.0, e[2], e[3]])
            obs = C.c_double(0)
            hc.hc_st_edge_cost(ptr(w4), ptr(edge), 16, *[ptr(a) for a in sets], C.byref(obs))
            assert abs(obs.value - want) <= 1e-12 * max(1.0, abs(want))
        tab = g["dp_s_dot_table"]
        for rc, want in zip(g["dp_idx"][n], g["dp_cost"][n]):
            origin = rc[0] == 0
            edge = np.array([0.0 if origin else g["s_list"][39 - rc[0]], 0.0 if origin else g["t_list"][rc[1]],
                             7.5 if origin else tab[rc[0], rc[1]], g["s_list"][39 - rc[2]], g["t_list"][rc[3]]])
            got = hc.hc_st_edge_cost(ptr(w4), ptr(edge), 16, *[ptr(a) for a in sets], None)
            assert abs(got - want) <= 1e-12 * abs(want)
    # terminal node rule on the reference's own cost tables
    for n in range(len(g["tables_out"])):
        cost = np.ascontiguousarray(g["tables_out"][n][0])
        r, c = C.c_int(-9), C.c_int(-9)
        assert hc.hc_st_terminal(ptr(cost), C.byref(r), C.byref(c)) == 1
        assert (r.value, c.value) == st_speed.terminal_node(cost)


def test_st_core_pruning_is_exact(hc):
    """Obstacle pruning by bounding boxes must not change any bit: compare with the unpruned NumPy statement."""
    from oracle import st_speed
    rng = np.random.default_rng(11)
    ptr = lambda a: a.ctypes.data
    w4 = np.array([50.0, 4000.0, 100.0, 10000000.0])
    worst = 0.0
    for trial in range(600):
        s_in = rng.uniform(0, 55, 16)
        s_out = s_in + rng.uniform(-5, 25, 16)
        t_in = rng.uniform(0, 7, 16)
        t_out = t_in + rng.uniform(0.5, 6, 16)
        s_in[rng.integers(0, 16, 3)] = np.nan
        s0, s1 = rng.uniform(0, 55, 2)
        t0 = rng.choice(np.arange(0, 8, 0.5))
        if trial % 3 == 0:          # put a few segments right next to the edge: the 1.5 .. 1.6 zone matters
            for j in range(0, 16, 4):
                off = rng.uniform(1.3, 1.8) * rng.choice([-1, 1])
                s_in[j], t_in[j] = s0 + off, t0 + rng.uniform(-0.3, 0.3)
                s_out[j], t_out[j] = s_in[j] + rng.uniform(-3, 3), t_in[j] + rng.uniform(0.2, 3)
        edge = np.array([s0, t0, rng.uniform(0, 20), s1, t0 + 0.5])
        obs = C.c_double(0)
        hc.hc_st_edge_cost(ptr(w4), ptr(edge), 16, ptr(s_in), ptr(s_out), ptr(t_in), ptr(t_out), C.byref(obs))
        want = float(st_speed.exact_obs_cost(s0, t0, s1, t0 + 0.5, s_in, s_out, t_in, t_out, 10000000.0))
        worst = max(worst, abs(obs.value - want) / max(1.0, abs(want)))
    assert worst <= 1e-13


def test_st_core_reach_interval_and_flat_pair_cost(hc):
    """The two pieces the round-3 speed DP kernel adds (emp_st_core.h): the branch-free pair cost equals the reference-order
    one bit for bit, and a pair that costs anything lies strictly inside the segment's reach interval at its sample time
    (so skipping everything outside the interval never changes a result).  Points are drawn around the 1.5 m reach, at
    the segment's ends, along it, and against steep, flat, short and degenerate segments."""
    rng = np.random.default_rng(23)
    n = 400000
    s_in = rng.uniform(0, 55, n)
    t_in = rng.uniform(0, 7, n)
    kind = rng.integers(0, 6, n)
    ds = np.where(kind == 0, 0.0, rng.uniform(-30, 30, n))               # stationary in s
    dt = np.where(kind == 1, rng.uniform(1e-9, 1e-3, n), rng.uniform(0.2, 8, n))   # nearly instantaneous
    ds = np.where(kind == 2, rng.uniform(-1e-6, 1e-6, n), ds)
    both = kind == 3                                                      # degenerate: a point
    ds = np.where(both, 0.0, ds)
    dt = np.where(both, 0.0, dt)
    s_out, t_out = s_in + ds, t_in + dt
    # a point at parameter u along the segment, offset by r across it (or beyond an end)
    u = rng.uniform(-0.3, 1.3, n)
    r = np.where(rng.uniform(size=n) < 0.7, rng.uniform(1.3, 1.7, n), rng.uniform(0, 3, n)) * rng.choice([-1.0, 1.0], n)
    L = np.hypot(ds, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        nx, ny = np.where(L > 0, -dt / L, 1.0), np.where(L > 0, ds / L, 0.0)
    pt = np.stack([s_in + u * ds + r * nx, t_in + u * dt + r * ny], axis=1)
    seg = np.ascontiguousarray(np.stack([s_in, t_in, s_out, t_out], axis=1))
    pt = np.ascontiguousarray(pt)
    cost, flat, lohi = np.zeros(n), np.zeros(n), np.zeros((n, 2))
    inside = np.zeros(n, np.int32)
    ptr = lambda a: a.ctypes.data
    hc.hc_st_reach(n, 10000000.0, ptr(seg), ptr(pt), ptr(cost), ptr(flat), ptr(inside), ptr(lohi))
    assert np.array_equal(cost, flat, equal_nan=True), "point_cost_flat differs from point_cost"
    costly = cost != 0.0
    assert costly.sum() > 0.2 * n and (~costly).sum() > 0.2 * n          # both sides of the reach are sampled
    assert inside[costly].all(), "a pair with a cost lies outside its reach interval"
    # and the interval is not vacuous: most free pairs that lie across the segment's band are outside it
    assert (inside[~costly] == 0).mean() > 0.5


# --------------------------------------------------------------------------------------
# S-T speed planning back end: the scalar core the kernels call (emp_st_backend_core.h) against the reference's
# golden vectors and oracle/st_backend.py - no GPU involved
# --------------------------------------------------------------------------------------
def test_stb_core_convex_space_and_interp_vs_reference_golden(hc):
    g = load_golden("speed_backend.npz")
    ptr = lambda a: a.ctypes.data
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    ran = 0
    for b in range(len(g["v0"])):
        n = int(g["path_len"][b])
        outs = [np.zeros(16) for _ in range(4)]
        ins = [c(g[k][b]) for k in ("dp_s", "dp_t", "path_index2s", "path_kappa")]
        sets = [c(g[k][b]) for k in ("s_in", "s_out", "t_in", "t_out")]
        st = hc.hc_stb_convex_space(*[ptr(a) for a in ins], n, *[ptr(a) for a in sets], 16, 0.2 * 9.8, *[ptr(a) for a in outs])
        assert st == [0, 2, 4][int(g["cs_raise"][b])]
        if st == 0:
            np.testing.assert_array_equal(np.stack(outs), g["cs_out"][b])
            ran += 1
    assert ran >= 60
    # numpy.interp, knot hits and clamped ends included
    rng = np.random.default_rng(3)
    xp = np.cumsum(rng.uniform(0.5, 1.5, 40))
    fp = rng.normal(size=40)
    xs = np.concatenate([xp[[0, 7, 39]], rng.uniform(xp[0] - 2, xp[-1] + 2, 500), [np.nan]])
    got = np.array([hc.hc_stb_np_interp(ptr(xp), ptr(fp), 40, float(x)) for x in xs])
    np.testing.assert_array_equal(got, np.interp(xs, xp, fp))


def test_stb_core_speed_qp_and_increase_points(hc):
    from oracle import st_backend as be
    g = load_golden("speed_backend.npz")
    ptr = lambda a: a.ctypes.data
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    w4 = np.array([10.0, 50.0, 500.0, 50.0])
    solved = 0
    for b in np.nonzero(g["qp_code"] >= 0)[0]:
        outs = [np.zeros(17) for _ in range(4)]
        iters = C.c_int(0)
        cs = [c(g["cs_out"][b, k]) for k in range(4)]
        dps, dpt = c(g["dp_s"][b]), c(g["dp_t"][b])         # named: the arrays must outlive the call
        st = hc.hc_stb_speed_qp(ptr(dps), ptr(dpt), float(g["v0"][b]), float(g["qp_a0"][b]),
                                *[ptr(a) for a in cs], ptr(w4), *[ptr(a) for a in outs], C.byref(iters))
        if g["qp_code"][b] == 2:
            assert st == 4
            continue
        if np.isnan(g["prof"][b]).all():                  # the dense oracle found the corridor infeasible
            assert st == 8
            continue
        assert st == 0 and 0 < iters.value < 60
        k = int(g["qp_size"][b])
        assert_rel(np.stack(outs)[:, :k], g["prof"][b][:, :k], 1e-6)
        assert np.isnan(np.stack(outs)[:, k:]).all()
        solved += 1
    assert solved >= 25
    for b in np.nonzero(g["dense_raise"] == 0)[0]:
        prof = [c(g["prof"][b, k]) for k in range(4)]
        outs = [np.zeros(401) for _ in range(4)]
        assert hc.hc_stb_increase_points(*[ptr(a) for a in prof], *[ptr(a) for a in outs]) == 0
        np.testing.assert_array_equal(outs[3], g["dense_out"][b, 3])
        assert_rel(np.stack(outs[:3]), g["dense_out"][b, :3], 1e-12, scale=1.0)


def test_host_logic_under_address_and_undefined_behaviour_sanitizers():
    """SURVEY.md section 5 (sanitizers): the scalar cores the kernels are built from, compiled with g++
    -fsanitize=address,undefined and driven with sizes at and beside every capacity, infeasible QPs, NaN / Inf
    coordinates, repeated points, empty and full obstacle slots (tests/host_check/sanitize_main.cpp).  Any report aborts
    the program (-fno-sanitize-recover)."""
    import os
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_check")
    exe = os.path.join(here, "_build", "sanitize_main")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(here, "host_check.cpp"),
                    os.path.join(here, "sanitize_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    assert "sanitize_main:" in run.stdout


def test_projection_dot_product_rounds_like_numpy(hc):
    """emp_frenet_core.h dot2 = fma(a1, b1, a0 * b0): bit for bit what numpy.dot returns for two 2-vectors on an x86 host
    whose OpenBLAS accumulates with fused multiply-adds (the reference evaluates every projection with np.dot,
    planning_utils.py:107, :443, :507, :546-578).  The fused form itself is checked against libm's fma on any host; numpy
    only where its dot is of that form (another BLAS may round the plain way - that is the reference's host dependence,
    HISTORY.md section 4)."""
    import ctypes
    rng = np.random.default_rng(11)
    n = 20000
    a = np.ascontiguousarray(rng.normal(0, 30, (n, 2)))
    b = np.ascontiguousarray(rng.normal(0, 1, (n, 2)))
    out = np.zeros(n)
    hc.hc_dot2(n, a.ctypes.data, b.ctypes.data, out.ctypes.data)
    libm = ctypes.CDLL("libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    fused = np.array([libm.fma(a[k, 1], b[k, 1], a[k, 0] * b[k, 0]) for k in range(n)])
    np.testing.assert_array_equal(out, fused)
    plain = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
    assert (fused != plain).mean() > 0.1                       # the two forms really differ in the last bit
    dots = np.array([np.dot(a[k], b[k]) for k in range(n)])
    if (dots == plain).all():
        pytest.skip("this host's numpy rounds 2-vector dot products the plain way")
    np.testing.assert_array_equal(out, dots)


# ---- launch geometry of the lattice-DP kernels (csrc/emp_dp_launch.h) --------------------------------------------------
def _dp_plan_row(hc, row, col, B, max_obs, tiled, form, block, messages):
    """One row of tests/golden/dp_launch_plans.npz, recomputed: the inputs, then every plan (refusal as 1 + its index in
    `messages`, the plan's fields zero beside it)."""
    code = lambda m: 0 if m is None else 1 + messages.index(m.decode())
    e, s, f, n = (np.zeros(k, dtype=np.int64) for k in (10, 6, 2, 1))
    out = [row, col, B, max_obs, tiled, form, block]
    out += [code(hc.hc_plan_edge(row, col, B, max_obs, tiled, form, block, e.ctypes.data)), *e]
    out += [code(hc.hc_plan_sweep(row, col, B, max_obs, s.ctypes.data)), *s]
    out += [code(hc.hc_plan_fused(row, col, B, max_obs, f.ctypes.data)), *f]
    for pre in (0, 1):
        out += [code(hc.hc_plan_enrich(row, col, B, max_obs, pre, n.ctypes.data)), n[0]]
    out.append(hc.hc_edge_tensor_elems(row, col, B, tiled))
    return out


def test_dp_launch_plans_match_the_pinned_table(hc):
    """Every launch plan of emp_dp_launch.h (edge-cost, sweep, fused, densification, and the edge tensor's size) on the
    25 920 points of tests/golden/dp_launch_plans.npz: row {1, 5, 9, 12, 21, 32, 33, 64, 1024} x col {1, 2, 9, 21, 40,
    120} x B {1, 7, 64, 4096, 32768} x max_obs {0, 8, 32, 33, 64, 65, 254, 256} x both layouts x edge_form {0, 1} x
    edge_block {0, 128, 256}; all fields compared, refusals with their text.  The table holds what the launchers computed
    inline before the plans existed (commit b1fe952: those lines, unchanged, behind a stub context): the numbers were tuned
    on the GPU, and no parity test notices a slip in them - the kernels are bit-identical for any geometry."""
    g = load_golden("dp_launch_plans.npz")
    plans, messages = g["plans"], [str(m) for m in g["messages"]]
    assert plans.shape == (9 * 6 * 5 * 8 * 2 * 2 * 3, len(g["columns"]))
    got = np.array([_dp_plan_row(hc, *(int(v) for v in p[:7]), messages) for p in plans], dtype=np.int64)
    bad = np.nonzero((got != plans).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size} points differ; first: inputs {plans[bad[0], :7].tolist()} "
                           f"fields {[str(c) for c in g['columns'][got[bad[0]] != plans[bad[0]]]]}")


def test_dp_edge_plan_invariants(hc):
    """What every good edge-cost plan on the pinned grid must satisfy, whatever the tuning: the block fits the LDS and is
    its wavefronts; the chunks are whole wavefront rounds and cover the lattice; the ring form only where its entry code
    holds the scene (64 obstacles, 15 bits of column); and the ring form's LDS is exactly what dp_edge_ring_kernel carves
    up (emp_dp_kernels.h: the pointer arithmetic from `tab` to `f_all`)."""
    g = load_golden("dp_launch_plans.npz")
    LDS = 160 * 1024
    n_ring = n_shrunk = 0
    for row, col, B, max_obs, tiled, form, block in np.unique(g["plans"][:, :7], axis=0).tolist():
        e = np.zeros(10, dtype=np.int64)
        if hc.hc_plan_edge(row, col, B, max_obs, tiled, form, block, e.ctypes.data) is not None:
            continue
        wide, ring, m32, row_inst, wpb, cpc, gx, gy, threads, lds = e.tolist()
        what = f"row {row} col {col} B {B} max_obs {max_obs} tiled {tiled} form {form} block {block}"
        assert wide == (row > 32), what
        assert 0 <= lds <= LDS and threads == 64 * wpb and gx >= 1 and 1 <= gy <= 65535, what
        assert gy * cpc >= col - 1, what
        if wide:
            assert (gx, gy, lds) == (B, max(col - 1, 1), 0) and threads <= 256, what
            continue
        mo = max(max_obs, 1)                                     # make_dp_dev: at least one slot
        S = 64 // row
        assert gx == (B + S - 1) // S and cpc % wpb == 0 and m32 == (mo <= 32), what
        assert row_inst == (row if row in (5, 9, 12, 21) else 0), what
        c = np.zeros(4, dtype=np.int64)
        hc.hc_edge_ring_constants(mo, c.ctypes.data)
        fields, ring_slots, ring_max_col, ring_bytes = c.tolist()
        assert ring_bytes == 2 * ring_slots * 4 + ring_slots * (1 if mo <= 8 else 2 if mo <= 16 else 4 if mo <= 32 else 8)
        if ring:
            assert form == 0 and mo <= 64 and col <= ring_max_col, what
            # dp_edge_ring_kernel: tab [fields][row^2], t_obs_s and t_obs_l [S][max_obs], t_ps [S rounded up to even] doubles;
            # per wavefront the reach bands [2][S][max_obs] doubles, then the two rings, then the jerk factors
            # [columns per wavefront][S] doubles with columns per wavefront = ceil(cols_per_chunk / wavefronts)
            cpw = (cpc + wpb - 1) // wpb
            per_wave = 2 * S * mo * 8 + ring_bytes + cpw * S * 8
            assert lds == (fields * row * row + 2 * S * mo + ((S + 1) & ~1)) * 8 + wpb * per_wave, what
            n_ring += 1
        else:
            # dp_edge_kernel: the table and the obstacles as above, the fields + 5 doubles of the table's tail; per wavefront
            # the box terms [S][min(max_obs, 64)]
            per_wave = S * min(mo, 64) * 8
            assert lds == (fields * row * row + 2 * S * mo + fields) * 8 + wpb * per_wave, what
        if block:
            assert wpb <= block // 64, what                      # overridden: as asked, or shrunk to what the LDS holds
        else:
            assert wpb <= 16, what
        if wpb < (block // 64 if block else 2):                  # shrunk: one more wavefront would not have fitted
            assert lds + per_wave > LDS, what
            n_shrunk += 1
    assert n_ring > 1000 and n_shrunk > 0                        # the grid reaches both (32 rows with 254 obstacle slots shrinks)


def _dp_layout(hc, name, a=0, b=0, c=0, d=0, e=0):
    out = np.zeros(12, dtype=np.int64)
    n = hc.hc_dp_layout(name.encode(), a, b, c, d, e, out.ctypes.data)
    assert n > 0, name
    return out[:n].tolist()


def test_dp_layouts_hold_what_the_kernels_index(hc):
    """The LDS layouts of emp_dp_launch.h against the loops of the six kernels that carve with them, on every good plan of the
    pinned grid: arrays in the struct's order, none overlapping, each aligned to its element and as long as the kernel indexes
    it, `end` equal to the plan's `lds`.  Positions count doubles, but bytes for edge_ring, enrich and fused.  The bounds, read from
    emp_dp_kernels.h (rr = row^2, S = 64 / row scenes a tile, F = kTableFields, T = kTableTail = 10 sample offsets + 2 moments
    + 3 coefficients):
      dp_edge_kernel        tab [f rr + p], f < F, p < rr (the scan's ten samples are fields 0..9); obs_s, obs_l [s max_obs + m],
                            s < S, m < max_obs; smp [t], t < T; box [(wave S + s) w + m], wave < wavefronts, m < w =
                            min(max_obs, mask bits)
      dp_edge_ring_kernel   tab, obs_s, obs_l as above; ps [s], s < S; band [((wave S + s) max_obs + m) 2 + 1]; rings: a wavefront's
                            share is edge_ring_bytes - 32-bit codes [2][kRingSlots], then kRingSlots masks of edge_ring_mask_bytes;
                            f [(wave cpw + t) S + s], t < cpw = ceil(cols_per_chunk / wavefronts)
      dp_sweep_kernel       front [wave 64 + lane]; pre bytes [(wave col + j) 64 + lane], j < col, copied out 16 bytes a lane;
                            the plan launches WPB = 1
      dp_sweep_wide_kernel  cur [i], nxt [i], i < row
      dp_enrich_wave_kernel rows [j] doubles, j < col; with the backtrack bt [j row + r] bytes, r < row
      dp_fused_kernel       tab, smp, obs_s, obs_l as the lockstep kernel; buf [((par nc + jj) row + k) 64 + lane] doubles, par < 2,
                            jj < nc, k < row; front [lane]; pre bytes [j 64 + lane], j < col; ctr [2] 32-bit"""
    g = load_golden("dp_launch_plans.npz")
    T = 10 + 2 + 3
    n_edge = n_ring = n_wide = n_fused = 0
    seen_small = set()
    for row, col, B, max_obs, tiled, form, block in np.unique(g["plans"][:, :7], axis=0).tolist():
        what = f"row {row} col {col} B {B} max_obs {max_obs} tiled {tiled} form {form} block {block}"
        mo = max(max_obs, 1)                                     # make_dp_dev: at least one slot
        S = 64 // row if row <= 32 else 1
        rr = row * row
        c = np.zeros(4, dtype=np.int64)
        hc.hc_edge_ring_constants(mo, c.ctypes.data)
        F, ring_slots, _, ring_bytes = c.tolist()
        mask_bytes = 1 if mo <= 8 else 2 if mo <= 16 else 4 if mo <= 32 else 8
        e = np.zeros(10, dtype=np.int64)
        if hc.hc_plan_edge(row, col, B, max_obs, tiled, form, block, e.ctypes.data) is None and not e[0]:
            _, ring, m32, _, wpb, cpc, _, _, _, lds = e.tolist()
            if ring:
                cpw = (cpc + wpb - 1) // wpb
                pos = _dp_layout(hc, "edge_ring", row, S, mo, wpb, cpw)                       # bytes
                assert ring_bytes == 4 * 2 * ring_slots + mask_bytes * ring_slots, what
                _in_order(pos, [8 * F * rr, 8 * S * mo, 8 * S * mo, 8 * ((S + 1) & ~1), 8 * wpb * S * mo * 2, wpb * ring_bytes,
                                8 * wpb * cpw * S])
                assert S <= (S + 1) & ~1 and all(p % 8 == 0 for p in pos), what                # the doubles, and the ones behind the rings
                # a wavefront's codes at 4 bytes, its masks (behind 2 kRingSlots codes) at their own width
                for wave in range(wpb):
                    at = pos[5] + wave * ring_bytes
                    assert at % 4 == 0 and (at + 4 * 2 * ring_slots) % mask_bytes == 0, what
                assert pos[-1] == lds, what
                n_ring += 1
            else:
                bits = 32 if m32 else 64
                pos = _dp_layout(hc, "edge", row, S, mo, bits, wpb)
                _in_order(pos, [F * rr, S * mo, S * mo, T, wpb * S * min(mo, bits)])
                assert F >= 10 and m32 == (mo <= 32), what      # the scan's ten samples are the table's first fields
                assert 8 * pos[-1] == lds, what
                n_edge += 1
        if (row, col, B, max_obs) in seen_small:
            continue
        seen_small.add((row, col, B, max_obs))
        s = np.zeros(6, dtype=np.int64)
        if hc.hc_plan_sweep(row, col, B, max_obs, s.ctypes.data) is None:
            if row > 32:
                pos = _dp_layout(hc, "sweep_wide", row)
                _in_order(pos, [row, row])
                n_wide += 1
            else:
                assert s[4] == 64, what                          # one wavefront a block: WPB = 1
                pos = _dp_layout(hc, "sweep", 1, col)
                _in_order(pos, [64, col * 64 // 8])
                assert (8 * pos[1]) % 16 == 0, what              # the predecessor table leaves the kernel 16 bytes a lane
                for wpb in (2, 4):                               # the kernel's other block sizes: a wavefront's share is col * 64 bytes
                    _in_order(_dp_layout(hc, "sweep", wpb, col), [wpb * 64, wpb * col * 64 // 8])
            assert 8 * pos[-1] == s[5], what
        for with_pre in (0, 1):
            n = np.zeros(1, dtype=np.int64)
            if hc.hc_plan_enrich(row, col, B, max_obs, with_pre, n.ctypes.data) is None:
                pos = _dp_layout(hc, "enrich", row, col, with_pre)                            # bytes
                _in_order(pos, [8 * col, col * row if with_pre else 0])
                assert pos[0] % 8 == 0 and pos[-1] == n[0], what
        f = np.zeros(2, dtype=np.int64)
        if hc.hc_plan_fused(row, col, B, max_obs, f.ctypes.data) is None:
            nc = int(f[0])
            pos = _dp_layout(hc, "fused", row, col, S, mo, nc)                                # bytes
            _in_order(pos, [8 * F * rr, 8 * T, 8 * S * mo, 8 * S * mo, 8 * 2 * nc * row * 64, 8 * 64, col * 64, 2 * 4])
            assert all(p % 8 == 0 for p in pos[:6]) and pos[7] % 4 == 0 and pos[-1] == f[1], what
            n_fused += 1
    assert n_ring > 1000 and n_edge > 1000 and n_wide > 0 and n_fused > 100


def test_edge_tensor_elems_is_the_size_of_the_tiled_tensor(hc):
    """emp_dp_launch.h edge_tensor_elems against the package's own host-side tiling (api.tile_edges) and the canonical
    shape, on small lattices either side of every scenes-per-wavefront count."""
    from emplanner_carla_amd.api import tile_edges
    for row in (1, 5, 9, 12, 21, 31, 32):
        for col in (2, 3, 6):
            for B in (1, 2, 3, 7, 13, 64, 65):
                canonical = np.zeros((B, col - 1, row, row))
                assert hc.hc_edge_tensor_elems(row, col, B, 1) == tile_edges(canonical, row).size
                assert hc.hc_edge_tensor_elems(row, col, B, 0) == canonical.size
    assert hc.hc_edge_tensor_elems(33, 4, 5, 1) == 5 * 3 * 33 * 33         # beyond 32 rows: canonical whatever is asked


# ---- launch plans and LDS layouts of the other kernels with dynamic LDS (csrc/emp_tail_launch.h) -----------------------------
# per plan: how many inputs lead a row of tests/golden/tail_launch_plans.npz (the hc_plan_* arguments, in order)
TAIL_PLANS = {"project": 2, "reference_line": 1, "cycle_qp": 5, "cycle_cartesian": 5, "path_qp": 2, "smooth": 2, "speed_front": 2,
              "speed_dp": 2, "st_edge_cost": 3, "speed_qp": 1, "merge": 2}
TAIL_FIELDS = ("gp", "r", "wide", "m32", "spw", "grid", "grid_y", "block", "lds")
LDS_CU, LDS_DEFAULT = 160 * 1024, 48 * 1024


def _tail_plan(hc, name, args):
    """(refusal text or None, the plan's fields by name)"""
    out = np.zeros(len(TAIL_FIELDS), dtype=np.int64)
    err = getattr(hc, "hc_plan_" + name)(*args, out.ctypes.data)
    return (None if err is None else err.decode()), dict(zip(TAIL_FIELDS, out.tolist()))


def _tail_layout(hc, name, a=0, b=0, c=0):
    out = np.zeros(24, dtype=np.int64)
    n = hc.hc_tail_layout(name.encode(), a, b, c, out.ctypes.data)
    assert n > 0, name
    return out[:n].tolist()


def _tail_constants(hc, n, max_obs=0):
    out = np.zeros(12, dtype=np.int64)
    hc.hc_tail_constants(n, max_obs, out.ctypes.data)
    return dict(zip(("path_qp_words", "pair_words", "pair_stations", "box_words", "speed_qp_words", "half_wave", "ref_points",
                     "stride_8_3", "stride_8_4", "stride_16_4", "st_list", "st_parts"), out.tolist()))


def test_tail_launch_plans_match_the_pinned_table(hc):
    """Every launch plan of emp_tail_launch.h on the points of tests/golden/tail_launch_plans.npz: max_pts {2, 8, 23 .. 27, 32 ..
    35, 51 .. 53, 64 .. 68, 128, 255, 256} x obstacle slots {1, 8, 32, 33, 64, 65, 253, 256} x max_ref {51, 61, 64, 65, 256, 4096,
    5000} x decimate {1, 2} x midpoint {0, 1} x B {0, 1, 7, 9, 64, 4096} x both values of path_qp_form and cartesian_form, less what an
    entry point rejects before it launches (max_ref < 2; max_pts = 256 in a cycle; more than 64 slots in the speed stages); the
    merge at path lengths either side of its entry point's 64 KB.  Kernel instantiation, grid, block, LDS bytes and refusals with
    their text are compared.  The table holds what the launchers computed inline before the plans existed (commit 429a7cf: those
    lines, unchanged, behind a stub context that records each launch) - a slip in them shows in no parity test at the sizes the
    suite runs, only as an LDS access out of bounds at a capacity nobody runs."""
    g = load_golden("tail_launch_plans.npz")
    messages, fields = [str(m) for m in g["messages"]], [str(f) for f in g["fields"]]
    assert set(TAIL_PLANS) == set(g.files) - {"messages", "fields"}
    assert len(g["cycle_qp"]) == 6 * 21 * 8 * 2 * 2 and len(g["cycle_cartesian"]) == 6 * 21 * 7 * 2 * 2 * 2
    for name, n_in in TAIL_PLANS.items():
        for row in g[name].tolist():
            err, p = _tail_plan(hc, name, row[:n_in])
            got = [0 if err is None else 1 + messages.index(err)] + [p[f] for f in fields[1:]]
            assert got == row[n_in:], f"{name}{tuple(row[:n_in])}: {dict(zip(fields, got))} != {dict(zip(fields, row[n_in:]))}"


def test_tail_plan_invariants(hc):
    """What every plan on the pinned grid must satisfy, whatever the tuning: the LDS bytes are the layout's total times the scenes
    (groups) per block and fit a compute unit, or the plan is refused; the chosen instantiation holds the capacity (GP R + 2
    stations for the rows path QP, 34 for the pair form, GP R points for the rows Cartesian tail, the narrow smoothers up to 32
    points); the grid covers the batch.  The four speed-stage launches had no LDS opt-in before the plans: three stay below
    the default 48 KB over everything their entry points accept (speed_front: max_pts <= 255; st_edge_cost and speed_qp: <= 64
    slots), the speed DP does not from 53 slots on - which is why every plan's launch goes through set_lds."""
    g = load_golden("tail_launch_plans.npz")
    rows_cap = {(8, 3): 24, (8, 4): 32, (16, 4): 64}
    seen = set()
    for name, n_in in TAIL_PLANS.items():
        for row in g[name].tolist():
            args = row[:n_in]
            err, p = _tail_plan(hc, name, args)
            what = f"{name}{tuple(args)}"
            B = args[0]
            if B == 0 or (name == "st_edge_cost" and args[1] == 0):
                # nothing to launch: all zeros, and never refused - but by emp_path_speed_merge, which checks before it stages
                assert not any(p.values()) and (err is None or name == "merge"), what
                continue
            if err is not None:
                continue
            assert 0 < p["lds"] <= LDS_CU and p["spw"] >= 1 and p["block"] % 64 == 0, what
            if name == "st_edge_cost":
                assert p["grid"] * 64 >= args[1] and p["grid_y"] == B, what
            else:
                assert p["grid"] * p["spw"] >= B > (p["grid"] - 1) * p["spw"] and p["grid_y"] == 1, what
            if name == "cycle_qp":
                _, max_pts, mo, dec, form = args
                cap = (max_pts + dec - 1) // dec
                k = _tail_constants(hc, cap, mo)
                if p["r"]:
                    assert form == 0 and (p["gp"], p["r"]) in rows_cap and p["spw"] == 64 // p["gp"], what
                    assert cap <= rows_cap[p["gp"], p["r"]] + 2, what
                    assert all(cap > c + 2 for (gp, r), c in rows_cap.items() if c < rows_cap[p["gp"], p["r"]]), what   # the smallest that holds it
                    assert p["lds"] == p["spw"] * k[f"stride_{p['gp']}_{p['r']}"] * 8, what
                else:
                    assert form == 1 or cap > 66, what
                    assert (p["gp"], p["spw"]) == ((32, 2) if cap <= 34 and form == 1 else (64, 1)), what
                    assert k["pair_stations"] == 34, what
                    assert p["lds"] == p["spw"] * _tail_layout(hc, "cycle_qp", p["gp"] == 32, cap, mo)[-1] * 8, what
                seen.add(("qp", p["gp"], p["r"]))
            elif name == "cycle_cartesian":
                _, max_ref, max_pts, path_cap, form = args
                cap = path_cap + 1
                if p["r"]:
                    assert form == 0 and cap <= rows_cap[p["gp"], p["r"]] and p["spw"] == 32 // p["gp"], what
                    assert all(cap > c for c in rows_cap.values() if c < rows_cap[p["gp"], p["r"]]), what
                    assert p["lds"] == _tail_layout(hc, "cartesian_rows", p["spw"], max_ref, cap)[0] * 8, what
                else:
                    assert (form == 1 or cap > 64) and p["spw"] == 1 and p["wide"] == (cap > 32), what
                    assert p["lds"] == _tail_layout(hc, "cartesian", max_ref, cap)[-1] * 8, what
                seen.add(("cart", p["gp"], p["r"], p["wide"]))
            else:
                layout, largs, groups = {"project": ("project", args[1:], 1), "reference_line": ("ref_line", [], 1),
                                         "path_qp": ("path_qp", args[1:], 1), "smooth": ("smooth", args[1:], 1),
                                         "speed_front": ("speed_front", args[1:], 1), "speed_dp": ("speed_dp", args[1:], 1),
                                         "st_edge_cost": ("st_edge", args[2:], 1), "speed_qp": ("speed_qp", [], 2),
                                         "merge": ("merge", args[1:], 1)}[name]
                total = _tail_layout(hc, layout, *largs)[-1]
                assert p["spw"] == groups, what
                if name == "speed_dp":
                    assert p["lds"] == (total + 7) // 8 * 8 and p["block"] == 320 and p["m32"] == (args[1] <= 32), what     # (bytes)
                else:
                    assert p["lds"] == groups * total * 8 and p["block"] == 64, what
                if name == "smooth":
                    assert p["wide"] == (args[1] > 32), what
                if name == "merge":
                    assert p["lds"] <= 64 * 1024, what
    assert seen >= {("qp", 8, 3), ("qp", 8, 4), ("qp", 16, 4), ("qp", 32, 0), ("qp", 64, 0), ("cart", 8, 3, 0), ("cart", 8, 4, 0),
                    ("cart", 16, 4, 0), ("cart", 0, 0, 0), ("cart", 0, 0, 1)}
    # the speed stages over the whole range of their entry points, not the grid's points alone
    for B in (1, 9, 4096):
        for max_pts in range(2, 256):
            err, p = _tail_plan(hc, "speed_front", [B, max_pts + 2])
            assert err is None and p["lds"] <= LDS_DEFAULT
        for slots in range(1, 65):
            for name, args in (("st_edge_cost", [B, 1000, slots]), ("speed_dp", [B, slots])):
                err, p = _tail_plan(hc, name, args)
                assert err is None and (p["lds"] <= LDS_DEFAULT or (name == "speed_dp" and slots >= 53))
        err, p = _tail_plan(hc, "speed_qp", [B])
        assert err is None and p["lds"] <= LDS_DEFAULT
    assert _tail_plan(hc, "speed_dp", [1, 52])[1]["lds"] <= LDS_DEFAULT < _tail_plan(hc, "speed_dp", [1, 53])[1]["lds"]


def _in_order(pos, sizes):
    """positions (the last one `end`) of arrays of these sizes: in order, none overlapping, nothing behind the last"""
    assert len(pos) == len(sizes) + 1 and pos[0] == 0
    assert [b - a for a, b in zip(pos, pos[1:])] == list(sizes), (pos, sizes)


def test_tail_layouts_hold_what_the_kernels_index(hc):
    """The LDS layouts of emp_tail_launch.h against the loops of the kernels that use them: arrays in order, none overlapping,
    each as long as the kernel indexes it.  The bounds, read from the kernels:
      frenet_project_wave_kernel   all seven arrays at i < P <= max_ref (and entry 0 for an empty line; max_ref >= 2)
      smooth_wave_kernel           smooth_pair_wave binds x and y to BoxRangeQp::words(m, m) doubles each from `qmem`;
                                   heading_kappa_wave writes theta [i], i < m, from `theta` TAKEN AT m <= cap
      reference_line_wave_kernel   gxy [2 lane + 1], lane < 51; then as smooth_wave_kernel with m = 51
      path_qp_wave_kernel          path_qp_group<64> takes path_qp_words(n) doubles, n <= cap
      cycle_qp_body, R == 0        sd, ld [i], i < n <= cap; lmin, lmax [i], i < n; ql [i], i < n; otab [4 k + 3], k < max_obs;
                                   qmem: path_qp_words(n) (one scene per wavefront), path_qp_words_pair() with n <= 34 (two)
      cycle_cartesian_body         sm [i], i < P <= max_ref; txy [2 q + 1], q < cap; th [i], i < m <= cap; qmem 2 words(m, m)
      cycle_cartesian_rows_kernel  the same per scene, px / py [j], j < m <= cap; the fall-back's 2 words(m2, m2) behind the scenes
      stb::speed_qp_kernel         cc [kQp + 2]; the solver's speed_qp_words(17) - 19 doubles; one flag word
      stb::merge_kernel            five arrays at i < width <= max_path
      speed_front_wave_kernel      chord [i], i2s [i], i < W
      st_edge_cost_kernel          seven arrays at j < max_obs
      speed_dp_kernel              see emp_st_kernels.h StLds: [max_obs] x 7, iv [2][max_obs][5][2], node_c [40][max_obs], t_tab
                                   [10], s_tab [40], part_c [8][40], p_cost and p_sdot [2][40], row0 [16], colmask [2][2] 64-bit,
                                   list_s [5][257] doubles, list_c [5][257] 32-bit, part_k [8][40] and t_node [40][16] bytes"""
    for n in (1, 2, 51, 64, 65, 256, 4096):
        _in_order(_tail_layout(hc, "project", n), [n] * 7)
        _in_order(_tail_layout(hc, "merge", n), [n] * 5)
        _in_order(_tail_layout(hc, "speed_front", n), [n] * 2)
    for k in (1, 8, 32, 33, 64):
        _in_order(_tail_layout(hc, "st_edge", k), [k] * 7)
        c = _tail_constants(hc, 4)
        assert (c["st_list"], c["st_parts"]) == (5 * 257, 8)
        pos = _tail_layout(hc, "speed_dp", k)                                                   # bytes
        _in_order(pos, [8 * k] * 7 + [8 * 20 * k, 8 * 40 * k, 80, 320, 8 * 8 * 40, 640, 640, 128, 32, 8 * c["st_list"], 4 * c["st_list"],
                        8 * 40, 40 * 16])
        assert all(p % 8 == 0 for p in pos[:17]) and pos[17] % 4 == 0                          # doubles and codes aligned
    words = lambda m: _tail_constants(hc, m)["box_words"]
    theta_prev = -1
    for cap in range(2, 257):
        c = _tail_constants(hc, cap)
        _in_order(_tail_layout(hc, "smooth", cap), [2 * c["box_words"], cap])
        _in_order(_tail_layout(hc, "path_qp", cap), [c["path_qp_words"]])
        # theta at the scene's own m: never behind theta at the capacity, and its m headings end inside the capacity's total
        q, theta, end = _tail_layout(hc, "smooth", cap)
        assert theta > theta_prev
        theta_prev = theta
        for m in (2, cap // 2 + 1, cap - 1, cap):
            qm, tm, em = _tail_layout(hc, "smooth", m)
            assert tm <= theta and em <= end and words(m) <= words(cap)
        assert _tail_constants(hc, cap - 1)["path_qp_words"] <= c["path_qp_words"]           # a scene with n <= cap stations fits
    assert _tail_layout(hc, "ref_line") == [0, 102, 102 + 2 * words(51), 102 + 2 * words(51) + 51]
    sq = _tail_constants(hc, 4)["speed_qp_words"]
    _in_order(_tail_layout(hc, "speed_qp"), [19, sq - 19, 1])
    for cap in (1, 2, 8, 26, 27, 34, 35, 66, 67, 128, 255):
        for mo in (1, 8, 33, 64, 65, 256, 259):
            c = _tail_constants(hc, cap)
            _in_order(_tail_layout(hc, "cycle_qp", 0, cap, mo), [cap] * 5 + [4 * mo, c["path_qp_words"]])
            if cap <= c["pair_stations"]:
                _in_order(_tail_layout(hc, "cycle_qp", 1, cap, mo), [cap] * 5 + [4 * mo, c["pair_words"]])
    for cap in (3, 24, 25, 32, 33, 64, 65, 129, 257):
        for max_ref in (2, 51, 61, 256, 4096):
            _in_order(_tail_layout(hc, "cartesian", max_ref, cap), [max_ref, 2 * cap, cap, 2 * words(cap)])
            scene = _tail_layout(hc, "cartesian_scene", max_ref, cap)
            _in_order(scene, [max_ref, 2 * cap, cap, cap, cap])
            for spw in (2, 4):
                assert _tail_layout(hc, "cartesian_rows", spw, max_ref, cap) == [spw * scene[-1] + 2 * words(cap)]


def test_path_qp_size_limit_cases_reach_every_launch_class(hc):
    """tests/test_gpu_cycle.py::test_path_qp_at_its_size_limits plans scenes at these (columns, max_pts) with the default
    decimation (2) and midpoints (1): which kernels the plans give each case - asserted here, on the CPU - and that together the
    cases stand on both sides of every capacity at which a plan changes the kernel."""
    from tests.test_gpu_cycle import PATH_QP_LIMIT_CASES, PATH_QP_LIMIT_SEEDS
    want = {(33, None): ((8, 4, 34), (16, 4, 36)), (34, 68): ((8, 4, 34), (16, 4, 36)), (34, None): ((16, 4, 35), (16, 4, 37)),
            (26, 52): ((8, 3, 26), (8, 4, 28)), (26, None): ((8, 4, 27), (8, 4, 29)), (35, None): ((16, 4, 36), (16, 4, 38)),
            (66, 132): ((16, 4, 66), (0, 0, 68)), (66, None): ((64, 0, 67), (0, 0, 69)), (67, None): ((64, 0, 68), (0, 0, 70)),
            (21, None): ((8, 3, 22), (8, 3, 24)), (22, None): ((8, 3, 23), (8, 4, 25))}
    assert {(c, m) for c, m, _ in PATH_QP_LIMIT_CASES} == set(want)
    caps_qp, caps_cart = set(), set()
    for col, max_pts, at_size in PATH_QP_LIMIT_CASES:
        n_seeds = PATH_QP_LIMIT_SEEDS.get((col, max_pts), 16)
        assert at_size == col
        M = max_pts or 2 * col + 1                      # api.max_path_points: sample_s = 2, sampling_res = 1
        stations, points = (M + 1) // 2, (M + 1) // 2 + 2
        for B in (n_seeds, 9):
            err, q = _tail_plan(hc, "cycle_qp", [B, M, 4, 2, 0])
            err2, c = _tail_plan(hc, "cycle_cartesian", [B, 61, M, stations + 1, 0])
            assert err is None and err2 is None
            assert ((q["gp"], q["r"], stations), (c["gp"], c["r"], points)) == want[col, max_pts], (col, max_pts)
            assert q["grid"] == -(-B // q["spw"]) and c["grid"] == -(-B // c["spw"])
        assert B % q["spw"] == 1 % q["spw"] and B % c["spw"] == 1 % c["spw"]       # nine scenes: one in the last wavefront
        caps_qp.add(stations)
        caps_cart.add(points)
    assert caps_qp >= {26, 27, 34, 35, 66, 67} and caps_cart >= {24, 25, 36, 37, 68}
