"""CPU suite of the station lookups' case tables (tests/lookup_cases.py): the tables say what they claim to say before the GPU suite
(tests/test_gpu_lookup_cases.py) relies on them, and the lookups' own text (emp_frenet_core.h, built with g++ by tests/host_check)
returns every label.

- Every case against its construction label: hc_proj_point, hc_walk_from_zero, hc_argmin_abs3, hc_lmin_lmax, hc_heading_kappa and
  oracle/ref_port.py.  Where the port raises IndexError the label is a status case.
- The wave form of the index walk (bisection, running maximum, carry between passes, count from the first station past the end,
  fmin against the end) equals the serial walk on EVERY non-decreasing integer s_map of up to 7 entries and every station of a
  15-value set: counted, not sampled.
- argmin_abs3 equals three argmin_abs calls on every non-decreasing integer station table of up to 9 entries.
- What a NaN station does in either form ("The station lookups")."""
from __future__ import annotations

import itertools
import math

import numpy as np
import pytest

from oracle import ref_port as rp
from tests import lookup_cases as K

NAN, INF = K.NAN, K.INF
REL = 1e-12                     # the port against the labels' own arithmetic: the same libm, the last bit of numpy's array route at most


@pytest.fixture(scope="module")
def hc():
    from tests import host_check
    return host_check.load()


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype)


def hc_proj(hc, line, sm, P, s, pre):
    line, sm = _c(line).reshape(-1), _c(sm)
    if line.size == 0:
        line, sm = np.zeros(4), np.zeros(1)          # (an address to hand over: P = 0 reads nothing)
    idx = np.array([pre], np.int32)
    out = np.zeros(4)
    ok = hc.hc_proj_point(line.ctypes.data, sm.ctypes.data, int(P), float(s), idx.ctypes.data, out.ctypes.data)
    return bool(ok), int(idx[0]), out


def hc_walk0(hc, sm, P, s):
    sm = _c(sm) if P else np.zeros(1)
    off = np.zeros(1, np.int32)
    k = hc.hc_walk_from_zero(sm.ctypes.data, int(P), float(s), off.ctypes.data)
    return int(k), bool(off[0])


def close(a, b, rel=REL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    k = ~np.isnan(a)
    inf = np.isinf(a[k]) | np.isinf(b[k])
    return bool(np.array_equal(a[k][inf], b[k][inf]) and
                np.all(np.abs(a[k][~inf] - b[k][~inf]) <= rel * np.maximum(np.abs(b[k][~inf]), 1.0)))


# ---------------------------------------------------------------------------------------------------------------------------
# a. every table entry against its label
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_walks_return_every_label(hc):
    seen = dict(ok=0, raised=0, zero=0, refused=0)
    for c in K.walk():
        P, line, sm = c["P"], c["line"], c["s_map"]
        if c["pre"] >= 0:                            # (the kernel refuses a negative previous index before the walk)
            ok, idx, out = hc_proj(hc, line, sm, P, c["s"], c["pre"])
            assert ok == c["ok"], c["name"]
            if ok:
                assert idx == c["idx"], (c["name"], idx)
                assert close(out, K.advance(line, sm, c["idx"], c["s"]), 0.0), c["name"]     # the same operations: the same bits
        if c["port"]:
            try:
                with np.errstate(all="ignore"):
                    w = rp.cal_proj_point(c["s"], c["pre"], [tuple(p) for p in line], list(sm))
            except IndexError:
                assert not c["ok"], c["name"]                                # a status case
                seen["raised"] += 1
            else:
                assert c["ok"] and w[4] == c["idx"], (c["name"], w[4])
                assert close(w[:4], K.advance(line, sm, c["idx"], c["s"])), c["name"]
                seen["ok"] += 1
        else:
            assert c["pre"] < 0 and not c["ok"]
            seen["refused"] += 1
        if c["zero"] is not None:
            assert c["pre"] == 0 and hc_walk0(hc, sm, P, c["s"]) == c["zero"], c["name"]
            assert c["zero"][1] == (not c["ok"]), c["name"]                  # off_end is "the serial walk from 0 raises"
            seen["zero"] += 1
    assert sum(seen[k] for k in ("ok", "raised", "refused")) == len(K.walk()) >= 250
    assert seen["raised"] >= 40 and seen["zero"] >= 150 and seen["refused"] == len(K.P_ALL)
    assert {c["P"] for c in K.walk()} == set(K.P_ALL)


def test_the_port_and_the_chained_host_walk_return_every_path_label(hc):
    raised = 0
    for c in K.paths():
        line, sm, P = c["line"], c["s_map"], c["P"]
        want = K.path_points(c)
        try:
            with np.errstate(all="ignore"):
                got = rp.frenet_path_to_xy(c["begin"][0], c["begin"][1], list(c["s"]), list(c["l"]), [tuple(p) for p in line], list(sm))
        except IndexError:
            assert c["status"] == 2 and c["count"] == 0, c["name"]
            raised += 1
        else:
            assert c["status"] == 0 and len(got) == c["count"], (c["name"], len(got))
            assert close(np.array([g[:2] for g in got]).reshape(-1, 2), want), c["name"]
        # the host walk chained as the kernel chains it
        ok, idx, _ = hc_proj(hc, line, sm, P, c["begin"][0], 0)
        assert ok == (c["status"] == 0), c["name"]
        if not ok:
            continue
        assert idx == c["idx0"], c["name"]
        kept = 0
        for s in c["s"]:
            if s > sm[P - 1]:
                break
            ok, idx, _ = hc_proj(hc, line, sm, P, s, idx)
            assert ok and (c["idx"][kept] is None or idx == c["idx"][kept]), (c["name"], kept, idx)
            assert (c["idx"][kept] is None) == math.isnan(s)
            kept += 1
        assert kept + 1 == c["count"], c["name"]
    assert raised == 4 and max(c["count"] for c in K.paths()) == K.PATH_CAP + 1


def f2c_want(c, proj_only):
    """The port on a case, point by point as the library's contract has it: (K, 4) NaN-filled, status."""
    X, Y, H, Kp = (list(c["line"][:, j]) for j in range(4))
    out = np.full((len(c["sl"]), 4), NAN)
    for j, (s, l, dl, ddl) in enumerate(c["sl"]):
        if np.isnan(s):
            return out, 0
        try:
            with np.errstate(all="ignore"):
                if proj_only:
                    out[j] = rp.CalcProjPoint(s, X, Y, H, Kp, list(c["i2s"]))
                else:
                    r = rp.Frenet2Cartesian([s], [l], [dl], [ddl], X, Y, H, Kp, list(c["i2s"]))
                    out[j] = [r[k][0, 0] for k in range(4)]
        except IndexError:
            return out, 2
    return out, 0


def test_the_port_returns_every_frenet2cartesian_label():
    statuses = 0
    for c in K.f2c():
        out, st = f2c_want(c, True)
        assert st == c["status"], c["name"]
        statuses += st == 2
        for j, i in enumerate(c["idx"]):
            if i is None:
                assert np.isnan(out[j]).all(), (c["name"], j)
            elif math.isfinite(c["sl"][j, 0]):
                assert close(out[j], K.advance(c["line"], c["i2s"], i, c["sl"][j, 0])), (c["name"], j)
        full, st2 = f2c_want(c, False)
        fin = np.isfinite(c["sl"][:, 0])                                    # (s = -inf: x is -inf, then NaN with the offset)
        assert st2 == st and np.array_equal(np.isnan(full[fin, 0]), np.isnan(out[fin, 0])), c["name"]
    assert statuses >= 8
    zero = [c for c in K.f2c() if c["name"].endswith("kappa_l_zero")]
    assert len(zero) == 1 and all(1.0 - 0.5 * l == 0.0 for l in zero[0]["sl"][:, 1]) and (zero[0]["line"][:, 3] == 0.5).all()


def test_the_bounds_return_every_label_bit_for_bit(hc):
    statuses = 0
    for c in K.bounds():
        n, k = c["n"], len(c["obs"])
        dps, dpl, os_, ol_ = _c(c["dp_s"]), _c(c["dp_l"]), _c(np.append(c["obs"][:, 0], 0.0)), _c(np.append(c["obs"][:, 1], 0.0))
        # the three indices: one pass against three scans against the labels
        for j, (lo, hi, centre) in enumerate(c["labels"]):
            t = _c([os_[j] - c["length"] / 2.0, os_[j] + c["length"] / 2.0, os_[j]])
            one, three = np.zeros(3, np.int32), np.zeros(3, np.int32)
            hc.hc_argmin_abs3(dps.ctypes.data, n, t.ctypes.data, one.ctypes.data, three.ctypes.data)
            assert tuple(three) == (lo - 2, hi - 2, centre) == tuple(one), (c["name"], j, tuple(one), tuple(three))
        lmin, lmax = np.full(n, NAN), np.full(n, NAN)
        ok = hc.hc_lmin_lmax(dps.ctypes.data, dpl.ctypes.data, n, os_.ctypes.data, ol_.ctypes.data, k, c["length"], K.OBS_WIDTH,
                             lmin.ctypes.data, lmax.ctypes.data)
        assert bool(ok) == (c["status"] == 0), c["name"]
        try:
            wlo, whi = rp.cal_lmin_lmax(list(c["dp_s"]), list(c["dp_l"]), list(c["obs"][:, 0]), list(c["obs"][:, 1]), c["length"], K.OBS_WIDTH)
        except IndexError:
            assert c["status"] == 4, c["name"]
            statuses += 1
            continue
        assert c["status"] == 0, c["name"]
        for got in ((lmin, lmax), (wlo, whi)):
            assert np.array_equal(got[0], c["l_min"]) and np.array_equal(got[1], c["l_max"]), c["name"]
    assert statuses >= 60 and {c["n"] for c in K.bounds()} >= set(K.BOUND_N)
    assert {len(c["obs"]) for c in K.bounds()} >= {0, 1, 2, 8, 9, 64}
    crossed = [c for c in K.bounds() if "opposite" in c["name"]]
    assert crossed and all((c["l_min"] > c["l_max"]).any() for c in crossed)
    assert all(lo > hi >= c["n"] and c["status"] == 0 for c in K.bounds() if "empty_range" in c["name"] for lo, hi, _ in c["labels"])
    for edge in (-1, 0, 1):                      # hi on n - 1 (legal), n and n + 1
        assert any(hi == c["n"] + edge for c in K.bounds() for _, hi, _ in c["labels"])


def test_the_port_and_the_host_heading_agree_on_every_heading_case(hc):
    for c in K.headings():
        xy = _c(c["xy"])
        m = len(xy)
        with np.errstate(all="ignore"):
            wt, wk = (np.array(v, np.float64) for v in rp.cal_heading_kappa([tuple(p) for p in xy]))
        th, kp = np.zeros(m), np.zeros(m)
        hc.hc_heading_kappa(xy.ctypes.data, m, th.ctypes.data, kp.ctypes.data)
        assert close(th, wt) and close(kp, wk), c["name"]
        if c["theta"] is not None:
            assert np.array_equal(wt, np.array(c["theta"])), (c["name"], wt)
    west = next(c for c in K.headings() if c["name"] == "west_dy_sign")
    with np.errstate(all="ignore"):
        wt, wk = (np.array(v) for v in rp.cal_heading_kappa([tuple(p) for p in west["xy"]]))
    assert set(np.abs(wt)) == {math.pi} and (wt > 0).any() and (wt < 0).any()            # the jump between +pi and -pi ...
    assert (np.abs(wk) > 1e-17).any() and np.abs(wk).max() < 1e-15                        # ... leaves sin(+-pi) / 1, not 0, on a straight line
    wob = next(c for c in K.headings() if c["name"] == "west_wobble")
    with np.errstate(all="ignore"):
        wt, wk = (np.array(v) for v in rp.cal_heading_kappa([tuple(p) for p in wob["xy"]]))
        _, ek = (np.array(v) for v in rp.cal_heading_kappa([(-x, y) for x, y in wob["xy"]]))       # the mirror image heads east: no jump
    # a mirror image has the opposite curvature everywhere; where theta jumped the reference's has the SAME sign as the mirror's
    assert np.isfinite(wk).all() and (wt > 3.0).any() and (wt < -3.0).any()
    assert ((np.sign(wk) == np.sign(ek)) & (np.abs(wk) > 1e-2)).sum() >= 3 and ((np.sign(wk) == -np.sign(ek)) & (np.abs(wk) > 1e-2)).sum() >= 3
    rep = next(c for c in K.headings() if c["name"] == "repeated_point")
    with np.errstate(all="ignore"):
        wt, wk = rp.cal_heading_kappa([tuple(p) for p in rep["xy"]])
    assert wt[3] == 0.0 and not np.isfinite(wk[3])


@pytest.mark.parametrize("col", K.CYCLE_COLS)
def test_the_cycle_scenes_are_what_the_table_says(col):
    """tests/lookup_truth.py asserts while it builds: the port plans every live scene to "optimal", the s_map and begin_s are the
    integers of the construction, every kept path station is a knot, the labelled node is SEP away from its neighbours', the
    obstacle's (s, l) is exact, its bound is the labelled index range and that range is active in the QP's answer.  Here: what the
    scenes cover - the station that lands on the end of the line on the last lane of a pass and on the first lane of the next."""
    from tests import lookup_truth as T
    cfg, specs, inputs, labels, want = T.cycle(col)
    SL = K.CYCLE_LANES[col]
    pts = {s["points"] for s in specs}
    assert {SL - 1, SL, SL + 1, col + 3, 2, 3} <= pts, (col, pts)
    assert {s["status"] for s in specs} == {0, 2, 4, 8} and len(specs) == len(want) == 14 + (col in K.CYCLE_L_EQUAL_COLS)
    n = col + 1
    assert {lab[1] for lab in labels if lab} - {2} == {n // 2 + 3, n - 1, n}            # hi: mid-path, on n - 1 (legal) and on n (2: l_equal)
    half = next(s for s in specs if s["half_end"])
    w = want[specs.index(half)]
    assert w["path_s"][half["points"] - 1] - w["s_map"][-1] == 0.5                         # the dropped station: half a unit past the end


# ---------------------------------------------------------------------------------------------------------------------------
# b. the wave form of the walk equals the serial one: exhaustive
# ---------------------------------------------------------------------------------------------------------------------------
STATIONS = tuple(-1.0 + 0.5 * i for i in range(13)) + (INF, -INF)          # -1, -0.5, ..., 5, +inf, -inf


def s_maps(max_len, top):
    for n in range(1, max_len + 1):
        for c in itertools.combinations_with_replacement(range(top + 1), n):
            yield np.array(c, np.float64)


def serial_walk(sm, start, s):
    """The reference's loop (path_planning.py:62-64), None where it raises IndexError."""
    i = start
    while True:
        if i + 1 >= len(sm):
            return None
        if not sm[i + 1] < s:
            return i
        i += 1


def test_bisection_equals_the_serial_walk_on_every_small_s_map(hc):
    pairs = 0
    for sm in s_maps(7, 4):
        P = len(sm)
        line = [(100.0 * i, 0.0, 0.0, 0.0) for i in range(P)]
        for s in STATIONS:
            k, off = hc_walk0(hc, sm, P, s)
            want = serial_walk(sm, 0, s)
            ok, idx, _ = hc_proj(hc, np.array(line), sm, P, s, 0)
            assert off == (want is None) == (not ok), (sm, s)
            assert want is None or k == want == idx, (sm, s, k, want)
            assert want is not None or k == P - 1, (sm, s, k)
            try:
                with np.errstate(all="ignore"):
                    w = rp.cal_proj_point(s, 0, line, list(sm))[4]
            except IndexError:
                w = None
            assert w == want, (sm, s)
            pairs += 1
    assert pairs == 791 * 15


def wave_passes(sm, w_min, begin_i, path_i, SL):
    """The pass logic of cycle_cartesian_body in NumPy, for a batch of paths at once.  w_min[j]: walk_from_zero of
    fmin(STATIONS[j], s_map[-1]); begin_i (N,), path_i (N, n): indices into STATIONS.  Returns idx (N, n + 1) per trajectory point
    (point 0 the start) and count (N,)."""
    st = np.array(STATIONS)
    N, n = path_i.shape
    s_last = sm[-1]
    carry = w_min[begin_i].copy()                    # idx0 (the caller has refused the starts that run off the end)
    count = np.full(N, n)
    stop = np.zeros(N, bool)
    idx = np.zeros((N, n + 1), np.int64)
    for base in range(0, n + 1, SL):
        k = np.zeros((N, SL), np.int64)
        bad = np.zeros((N, SL), bool)
        for sl in range(SL):
            i = base + sl - 1
            if 0 <= i < n:
                live = ~stop
                s = st[path_i[:, i]]
                bad[:, sl] = live & (s > s_last)
                k[:, sl] = np.where(live, w_min[path_i[:, i]], 0)
        any_bad = bad.any(axis=1)
        first_bad = np.where(any_bad, bad.argmax(axis=1) + 1, 0)                      # 1-based lane, 0 if none
        count = np.where(~stop & any_bad, np.minimum(count, base + first_bad - 2), count)
        k = np.maximum.accumulate(k, axis=1)                                          # inclusive running maximum across the lanes
        k = np.maximum(k, carry[:, None])
        carry = k[:, SL - 1]
        for sl in range(SL):
            if base + sl <= n:
                idx[:, base + sl] = k[:, sl]
        stop = stop | any_bad
    return idx, count


def test_the_pass_logic_equals_the_serial_chain_on_every_small_s_map():
    """Every sequence of three path stations from STATIONS on every s_map of the test above, the planning start at the first
    station (the densified path begins at the start): per-point bisection,
    inclusive running maximum, carry, count from the first s > s_last and fmin(s, s_last), in passes of 2 lanes (the carry
    crosses a pass) and of 4 (one pass), against the serial chain - built from the port's own walk, one call per (start index,
    station), and checked against the port's frenet_path_to_xy itself on every 97th path."""
    st = np.array(STATIONS)
    S = len(STATIONS)
    grid = np.array(list(itertools.product(range(S), repeat=3)))                      # three stations, the start on the first
    cases = sampled = 0
    for sm in s_maps(7, 4):
        P = len(sm)
        if P < 2:
            continue                                 # a line of one node: refused before the passes
        line = [(100.0 * i, 0.0, math.pi / 2, 0.0) for i in range(P)]                 # x tells the node
        # the port's walk as a table: T[p, j] = index from p for station j, -1 where it raises
        T = np.full((P, S), -1)
        for p in range(P):
            for j, s in enumerate(STATIONS):
                try:
                    with np.errstate(all="ignore"):
                        T[p, j] = rp.cal_proj_point(s, p, line, list(sm))[4]
                except IndexError:
                    pass
        w_min = np.array([serial_walk(sm, 0, min(s, sm[-1])) for s in STATIONS])       # (fmin(s, s_last) never runs off the end)
        assert all(w is not None for w in w_min)
        begin_ok = T[0, grid[:, 0]] >= 0
        g = grid[begin_ok]
        # serial chain (ref path_planning.py:29-46)
        idx = np.zeros((len(g), 4), np.int64)
        idx[:, 0] = T[0, g[:, 0]]
        alive = np.ones(len(g), bool)
        count = np.zeros(len(g), np.int64)
        for i in range(3):
            alive &= ~(st[g[:, i]] > sm[-1])                                      # :40-41 break
            nxt = T[idx[:, i], g[:, i]]
            assert (nxt[alive] >= 0).all()                                            # a station <= s_map[-1] never raises
            idx[:, i + 1] = np.where(alive, nxt, idx[:, i])
            count += alive
        for SL in (2, 4):
            widx, wcount = wave_passes(sm, w_min, g[:, 0], g, SL)
            assert np.array_equal(wcount, count), (sm, SL)
            kept = np.arange(4)[None, :] <= count[:, None]
            assert np.array_equal(widx[kept], idx[kept]), (sm, SL)
        cases += len(g)
        for r in range(0, len(g), 97):
            with np.errstate(all="ignore"):
                got = rp.frenet_path_to_xy(st[g[r, 0]], 0.0, list(st[g[r]]), [0.0] * 3, line, list(sm))
            assert len(got) == count[r] + 1
            nodes = [int(round(p[0] / 100.0)) for p in got if math.isfinite(p[0])]
            assert nodes == [int(v) for v, p in zip(idx[r], got) if math.isfinite(p[0])], (sm, r)
            sampled += 1
    # every (s_map, three stations) whose start the reference accepts: counted from the tables themselves
    want = sum(int(sum(serial_walk(sm, 0, s) is not None for s in STATIONS)) * S ** 2 for sm in s_maps(7, 4) if len(sm) >= 2)
    assert cases == want and cases > 1_000_000 and sampled > 10_000


# ---------------------------------------------------------------------------------------------------------------------------
# c. one pass of three targets equals three scans
# ---------------------------------------------------------------------------------------------------------------------------
def test_argmin_abs3_equals_three_scans_on_every_small_station_table(hc):
    targets = [-1.0 + 0.5 * i for i in range(11)]                                     # -1 .. 4: the half-integer grid round 0 .. 3
    calls = 0
    for sm in s_maps(9, 3):
        n = len(sm)
        d = np.abs(sm[None, :] - np.array(targets)[:, None])
        first = d.argmin(axis=1)                                                      # numpy: the first minimum
        for a in range(len(targets)):
            tri = [a, (a + 4) % 11, (a + 7) % 11]                                     # every slot sees every target
            t = _c([targets[i] for i in tri])
            one, three = np.zeros(3, np.int32), np.zeros(3, np.int32)
            hc.hc_argmin_abs3(sm.ctypes.data, n, t.ctypes.data, one.ctypes.data, three.ctypes.data)
            assert tuple(one) == tuple(three) == tuple(first[tri]), (sm, t, tuple(one), tuple(three))
            calls += 1
    assert calls == 714 * 11


# ---------------------------------------------------------------------------------------------------------------------------
# d. a NaN station
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_nan_station_moves_the_wave_index_but_no_output(hc):
    """DESIGN.md section 5, "The station lookups": inside the cycle a path station is NaN only when all of them and the planning start's s are (they are
    sums with it).  The wave form then walks every point to the end of the line (fmin(NaN, s_last) = s_last) where the serial walk
    stays at node 0 - and neither index is seen: ds = NaN - s_map[k] makes the point NaN from any finite node."""
    line, acc = K.chord_line(9, 9)
    P = len(line)
    k_wave, off = hc_walk0(hc, acc, P, acc[-1])                              # what fmin(NaN, s_last) hands the bisection
    ok, k_serial, out = hc_proj(hc, line, acc, P, NAN, 0)
    assert (k_wave, off) == (P - 2, False) and ok and k_serial == 0
    for k in range(P):
        assert all(math.isnan(v) for v in K.advance(line, acc, k, NAN)[:3])
    assert np.isnan(out[:3]).all()
    # a NaN node of the reference line: its chords are NaN, and so is every later entry of the s_map (a running sum).  On a
    # finite prefix followed by NaN the predicate `s_map[k + 1] < s` is still true-then-false: bisection and serial walk agree
    pairs = 0
    for sm in s_maps(5, 3):
        for tail in (1, 2):
            bad = np.concatenate([sm, np.full(tail, NAN)])
            for s in STATIONS:
                k, off = hc_walk0(hc, bad, len(bad), s)
                want = serial_walk(bad, 0, s)
                assert want is not None and (k, off) == (want, False), (bad, s)       # (NaN stops the walk: it never runs off the end)
                pairs += 1
    assert pairs == 125 * 2 * 15
