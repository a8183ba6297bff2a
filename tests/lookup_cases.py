"""Hard inputs for the station lookups (NumPy only, deterministic): the four places that find "the node or station that belongs to
this s" (emp_frenet_core.h: proj_point, walk_from_zero, argmin_abs / argmin_abs3 / lmin_lmax; emp_tail_kernels.h:
frenet2cartesian_kernel) and cal_heading_kappa.  Every case carries its expected index (or bound indices) as a label that follows
from how the case was built, not from the port or the library.

Where a decision is exact: a reference line's chords are integer vectors of length 5 (or unit steps for the cycle), so its
cumulative chord length is a sum of exact square roots, every s_map entry is an integer and a station "on a knot" equals the knot
in bits.  "One ulp above" is numpy.nextafter.  Stations of the bound cases are integers 1 apart and obstacle edges sit on the
half-integer grid, so |s_j - t| ties are equal in bits.

Separation: node headings are the centred-difference heading plus a seeded offset of 0.05 to 0.15 rad, curvatures are +-0.01 to
0.03, so extrapolating from node i and from node i + 1 to the same s lands on different points; `separation` measures it and the
builders of every table that goes to an entry point that does not return its index assert at least SEP metres.

  walk()      cal_proj_point: one query per case, with a previous index (the serial form) - and, from index 0, the wave form's bisection
  paths()     frenet_path_to_xy: a planning start and a path of stations
  f2c()       CalcProjPoint / Frenet2Cartesian: scenes of (s, l, dl, ddl) points
  bounds()    cal_lmin_lmax: stations, obstacles, the expected (lo, hi, centre) per obstacle
  headings()  cal_heading_kappa: polylines"""
from __future__ import annotations

import functools
import math

import numpy as np

NAN, INF = float("nan"), float("inf")
SEP = 1e-3                                           # metres between the labelled point and the one from the neighbouring index
P_ALL = (0, 1, 2, 3, 7, 63, 64, 65, 130)
MAX_REF = 130
CHORD = 5.0
VECS = ((5, 0), (4, 3), (3, 4), (0, 5), (4, -3), (3, -4))        # integer chords of length 5


def up(v):
    return float(np.nextafter(v, INF))


def down(v):
    return float(np.nextafter(v, -INF))


# ---------------------------------------------------------------------------------------------------------------------------
# lines
# ---------------------------------------------------------------------------------------------------------------------------
def chord_line(P, seed, repeats=()):
    """P nodes (P, 4) and their cumulative chord length from node 0 (integers): chords drawn from VECS, node `j` of `repeats` at the
    place of node j - 1 (a zero chord: a plateau of the s_map).  Heading: centred difference of the chords plus the node's own
    offset; curvature non-zero."""
    rng = np.random.default_rng(seed)
    xy = np.zeros((P, 2))
    acc = np.zeros(P)
    for i in range(1, P):
        v = (0, 0) if i in repeats else VECS[int(rng.integers(0, len(VECS)))]
        xy[i] = xy[i - 1] + v
        acc[i] = acc[i - 1] + math.sqrt(v[0] * v[0] + v[1] * v[1])
    th = np.zeros(P)
    for i in range(P):
        a, b = max(i - 1, 0), min(i + 1, P - 1)
        th[i] = math.atan2(xy[b, 1] - xy[a, 1], xy[b, 0] - xy[a, 0]) if P >= 2 else 0.0
    th = th + rng.uniform(0.05, 0.15, P) * np.where(np.arange(P) % 2 == 0, 1.0, -1.0) + 0.01 * (np.arange(P) % 7)
    kp = rng.uniform(0.01, 0.03, P) * np.where(np.arange(P) % 3 == 0, -1.0, 1.0)
    return np.column_stack([xy, th, kp]).reshape(P, 4), acc


def advance(line, s_map, idx, s):
    """The reference's extrapolation from node idx to station s (path_planning.py:66-75): x, y, theta, kappa."""
    x, y, th, k = (float(v) for v in line[idx])
    ds = s - float(s_map[idx])
    return (x + ds * math.cos(th), y + ds * math.sin(th), th + k * ds, k)


def offset(pt, l):
    """The point at lateral offset l of a projection (path_planning.py:44-46): x, y."""
    return (pt[0] + l * -math.sin(pt[2]), pt[1] + l * math.cos(pt[2]))


def separation(line, s_map, idx, s, l=0.0):
    """How far the point of station s moves when it is extrapolated from a neighbour of node idx instead (the smaller of the two)."""
    want = offset(advance(line, s_map, idx, s), l)
    out = INF
    for j in (idx - 1, idx + 1):
        if 0 <= j < len(line):
            other = offset(advance(line, s_map, j, s), l)
            out = min(out, math.hypot(other[0] - want[0], other[1] - want[1]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# walk cases: cal_proj_point
# ---------------------------------------------------------------------------------------------------------------------------
def _walk_case(name, P, line, s_map, s, pre, idx, ok, port=True, zero=None):
    """idx / ok: the serial walk's answer from `pre` (ok False: the reference raises IndexError, the library reports
    EMP_ST_S_OUT_OF_RANGE).  zero: (index, off_end) of the walk from 0 where the bisection form applies (a non-decreasing
    s_map without NaN), None otherwise.  port False: the reference's answer is not the contract (a negative previous index wraps
    round in Python; the library refuses it)."""
    return dict(name=f"P{P}_{name}", P=P, line=line, s_map=np.asarray(s_map, np.float64), s=float(s), pre=int(pre), idx=idx, ok=ok,
                port=port, zero=zero, exact=name.startswith("exact_"))


@functools.lru_cache(maxsize=None)
def walk():
    out = []
    for P in P_ALL:
        line, acc = chord_line(P, 100 + P)
        o = P // 3
        sm = acc - (acc[o] if P else 0.0)            # the origin on node o: integers, negative before it
        add = lambda name, s, pre, idx, ok, port=True, zero=None, sm_=None, line_=None: out.append(  # noqa: E731
            _walk_case(name, P, line if line_ is None else line_, sm if sm_ is None else sm_, s, pre, idx, ok, port, zero))
        if P < 2:
            # no index stops the walk: s_map[idx + 1] does not exist
            for name, s in (("zero", 0.0), ("nan", NAN), ("minus_inf", -INF), ("plus_inf", INF)):
                add(name, s, 0, None, False, zero=(0, True))
            add("negative_pre", 0.0, -1, None, False, port=False)
            continue
        last = P - 2                                  # the last index at which the walk can stop
        for tag, i in (("first", 0), ("mid", last // 2), ("last", last)):
            # s on s_map[i + 1]: `s_map[i + 1] < s` is false, the walk stays at i and ds is the whole chord
            add(f"on_knot_{tag}", sm[i + 1], 0, i, True, zero=(i, False))
            # one ulp above: it advances; past s_map[P - 1] no index stops it
            if i + 1 <= last:
                add(f"knot_plus_ulp_{tag}", up(sm[i + 1]), 0, i + 1, True, zero=(i + 1, False))
            else:
                add(f"knot_plus_ulp_{tag}", up(sm[i + 1]), 0, None, False, zero=(P - 1, True))
            add(f"knot_minus_ulp_{tag}", down(sm[i + 1]), 0, i, True, zero=(i, False))
        add("at_first_entry", sm[0], 0, 0, True, zero=(0, False))
        add("below_first_entry", sm[0] - 2.5, 0, 0, True, zero=(0, False))            # negative ds from node 0
        add("at_last_entry", sm[P - 1], 0, last, True, zero=(last, False))
        add("plus_inf", INF, 0, None, False, zero=(P - 1, True))
        add("minus_inf", -INF, 0, 0, True, zero=(0, False))
        add("nan", NAN, 0, 0, True, zero=(0, False))                                  # NaN is never `>` an entry: the walk stays
        # the previous index: the walk never steps back
        i = last // 2
        s = sm[i + 1]                                                                 # answer i from 0
        add("pre_at_answer", s, i, i, True)
        if i + 1 <= last:
            add("pre_beyond_answer", s, i + 1, i + 1, True)
            add("nan_from_mid", NAN, i + 1, i + 1, True)
        add("pre_at_last_stop", s, last, last, True)
        add("pre_at_last_node", s, P - 1, None, False)                                # s_map[P] does not exist, whatever s is
        add("pre_at_last_node_minus_inf", -INF, P - 1, None, False)
        add("negative_pre", s, -1, None, False, port=False)
        add("pre_mid_to_end", sm[P - 1], i, last, True)
        add("pre_mid_past_end", up(sm[P - 1]), i, None, False)
        # plateaus: m equal consecutive entries (repeated nodes) at the front, in the middle and at the end
        for m in (2, 3):
            if P < m + 2:
                continue
            for tag, j in (("front", 0), ("mid", max((P - m) // 2, 1)), ("end", P - m)):
                rep = tuple(range(j + 1, j + m))
                pl, pacc = chord_line(P, 1000 * m + P, repeats=rep)
                v = pacc[j]
                assert all(pacc[k] == v for k in range(j, j + m)) and (j == 0 or pacc[j - 1] < v) and (j + m == P or pacc[j + m] > v)
                stay = max(j - 1, 0)                       # entry j is the first that is not `< v`
                for q, s_ in (("on", v), ("minus_ulp", down(v))):
                    add(f"plateau{m}_{tag}_{q}", s_, 0, stay, True, zero=(stay, False), sm_=pacc, line_=pl)
                if j + m <= P - 1:                         # one ulp above: past every entry of the plateau
                    add(f"plateau{m}_{tag}_plus_ulp", up(v), 0, j + m - 1, True, zero=(j + m - 1, False), sm_=pacc, line_=pl)
                else:
                    add(f"plateau{m}_{tag}_plus_ulp", up(v), 0, None, False, zero=(P - 1, True), sm_=pacc, line_=pl)
        # a NaN entry inside the s_map (serial form only: the bisection needs a monotone predicate): `NaN < s` is false, the walk
        # stops in front of it; started behind it, it goes on
        if P >= 7:
            q = P // 2
            bad = sm.copy()
            bad[q] = NAN
            add("nan_entry_stops", sm[P - 1], 0, q - 1, True, sm_=bad)
            add("nan_entry_behind", sm[q + 2], q, q + 1, True, sm_=bad)
            add("nan_entry_behind_past_end", up(sm[P - 1]), q, None, False, sm_=bad)
        # heading 0 on an axis-aligned line, integer and dyadic ds, dyadic curvature: every product and sum is exact, the device's
        # point is the port's bit for bit (cos 0 = 1 and sin 0 = 0 on both)
        if P in (7, 65):
            ax = np.zeros((P, 4))
            ax[:, 0] = 3.0 * np.arange(P)
            ax[:, 3] = np.where(np.arange(P) % 2 == 0, 0.25, -0.125)
            asm = 3.0 * np.arange(P) - 6.0
            for tag, i in (("first", 0), ("mid", last // 2), ("last", last)):
                add(f"exact_on_knot_{tag}", asm[i + 1], 0, i, True, zero=(i, False), sm_=asm, line_=ax)
                add(f"exact_half_{tag}", asm[i] + 1.5, 0, i, True, zero=(i, False), sm_=asm, line_=ax)
            add("exact_below", asm[0] - 4.0, 0, 0, True, zero=(0, False), sm_=asm, line_=ax)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# path cases: frenet_path_to_xy
# ---------------------------------------------------------------------------------------------------------------------------
PATH_CAP = 12                                            # station capacity M of the path batch (output capacity M + 1)


def _path_case(name, line, sm, begin, stations, idx0, idxs, count, status):
    """idx0: the start's node; idxs: the node of every kept path point (None: its station is NaN, the point is NaN); count: the
    points written (start included); status: 0 or EMP_ST_S_OUT_OF_RANGE (2)."""
    P = len(line)
    n = len(stations)
    rng = np.random.default_rng(len(name) + 31 * n)
    ls = rng.uniform(-2.0, 2.0, n)
    c = dict(name=name, P=P, line=line, s_map=np.asarray(sm, np.float64), begin=(float(begin), 0.75), s=np.asarray(stations, np.float64),
             l=ls, idx0=idx0, idx=tuple(idxs), count=count, status=status)
    assert n <= PATH_CAP and len(idxs) == max(count - 1, 0)
    # separation: the start and every kept finite point
    if count >= 1:
        assert math.isnan(begin) or separation(line, sm, idx0, c["begin"][0], c["begin"][1]) >= SEP, name
        for k, i in enumerate(idxs):
            if i is not None:
                assert separation(line, sm, i, c["s"][k], ls[k]) >= SEP, (name, k)
    return c


def path_points(c):
    """The expected target_xy of a path case from its labels (count rows; NaN where the station is NaN)."""
    out = [offset(advance(c["line"], c["s_map"], c["idx0"], c["begin"][0]), c["begin"][1])] if c["count"] else []
    for k, i in enumerate(c["idx"]):
        out.append((NAN, NAN) if i is None else offset(advance(c["line"], c["s_map"], i, c["s"][k]), c["l"][k]))
    return np.array(out, np.float64).reshape(len(out), 2)


@functools.lru_cache(maxsize=None)
def paths():
    out = []
    for P in (8, 65):
        line, acc = chord_line(P, 200 + P)
        sm = acc - acc[1]                                # the origin on node 1
        end = sm[P - 1]
        k0 = P - 8                                       # the cases live on the last eight nodes: the walk crosses the whole line first
        add = lambda *a: out.append(_path_case(f"P{P}_{a[0]}", line, sm, *a[1:]))      # noqa: E731
        # every station on a knot: station s_map[i] is extrapolated from node i - 1 by the whole chord
        st = [sm[i] for i in range(k0 + 1, P)]
        add("all_on_knots", sm[0], st, 0, [i - 1 for i in range(k0 + 1, P)], len(st) + 1, 0)
        # a station that decreases after an increase: the index stays
        add("decrease", sm[k0], [sm[k0 + 1], sm[k0 + 4], sm[k0 + 2] + 2.5, sm[k0 + 2], sm[k0 + 5]], k0 - 1 if k0 else 0,
            [k0, k0 + 3, k0 + 3, k0 + 3, k0 + 4], 6, 0)
        # a NaN station in the middle: not `>` the end, the walk stays, its point is NaN, later points are unaffected
        add("nan_station", sm[k0 + 1], [sm[k0 + 2], NAN, sm[k0 + 3] + 2.5, NAN, sm[k0 + 5]], k0, [k0 + 1, None, k0 + 3, None, k0 + 4], 6, 0)
        # a station equal to s_map[-1] as the last kept point; the first one to pass it at positions 0, 1 and in the middle
        add("end_kept", sm[k0 + 3], [sm[P - 2], end, up(end), sm[P - 3]], k0 + 2, [P - 3, P - 2], 3, 0)
        add("past_at_0", sm[k0 + 3], [up(end), sm[P - 2]], k0 + 2, [], 1, 0)
        add("past_at_1", sm[k0 + 3], [end, up(end), sm[P - 2]], k0 + 2, [P - 2], 2, 0)
        add("past_in_the_middle", sm[k0 + 1] + 2.5, [sm[k0 + 2], sm[k0 + 3] + 2.5, end + 2.5, sm[k0 + 4]], k0 + 1, [k0 + 1, k0 + 3], 3, 0)
        # the planning start: on the end (kept, node P - 2), one ulp beyond it and far beyond it (IndexError)
        add("begin_on_the_end", end, [end, end], P - 2, [P - 2, P - 2], 3, 0)
        add("begin_ulp_beyond", up(end), [sm[k0 + 2]], None, [], 0, 2)
        add("begin_beyond", end + 40.0, [sm[k0 + 2]], None, [], 0, 2)
        add("begin_nan", NAN, [sm[k0 + 2], sm[k0 + 3]], 0, [k0 + 1, k0 + 2], 3, 0)             # NaN start: node 0, a NaN point
        # the output capacity reached exactly: PATH_CAP stations, all kept
        st = [sm[k0 + 1] + 2.5 * j for j in range(PATH_CAP)]
        add("capacity", sm[k0 + 1], st, k0, [k0 + 1 + (j - 1) // 2 if j else k0 for j in range(PATH_CAP)], PATH_CAP + 1, 0)
        add("no_stations", sm[k0 + 1], [], k0, [], 1, 0)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# CalcProjPoint / Frenet2Cartesian
# ---------------------------------------------------------------------------------------------------------------------------
F2C_CAP = 6


def _f2c_case(name, line, i2s, pts, idxs, status):
    """pts: rows (s, l, dl, ddl); idxs: per point the node CalcProjPoint stops at, None from the point on that ends the scene
    (a NaN s, or a station past the line: status 2)."""
    sl = np.asarray(pts, np.float64).reshape(len(pts), 4)
    assert len(pts) <= F2C_CAP and len(idxs) == len(pts)
    for k, i in enumerate(idxs):
        if i is not None and math.isfinite(sl[k, 0]):
            assert separation(line, i2s, i, sl[k, 0], sl[k, 1]) >= SEP, (name, k)
    return dict(name=name, P=len(line), line=line, i2s=np.asarray(i2s, np.float64), sl=sl, idx=tuple(idxs), status=status)


@functools.lru_cache(maxsize=None)
def f2c():
    out = []
    for P in (3, 7, 65):
        line, acc = chord_line(P, 300 + P)
        sm = acc + 10.0                                   # index2s need not start at 0
        mid = P // 2
        pt = lambda s, l=1.25: (s, l, 0.1, -0.01)          # noqa: E731
        add = lambda *a: out.append(_f2c_case(f"P{P}_{a[0]}", line, sm, *a[1:]))      # noqa: E731
        # s on s_map[idx]: the first entry that is `>= s` is idx itself, ds = 0
        add("on_knots", [pt(sm[1]), pt(sm[mid]), pt(sm[P - 1]), pt(sm[1])], [1, max(mid, 1), P - 1, 1], 0)
        # at or below s_map[1], below s_map[0]: index 1 (the scan starts there), negative ds
        add("below_entry_1", [pt(down(sm[1])), pt(sm[0]), pt(sm[0] - 7.5), pt(-INF)], [1, 1, 1, 1], 0)
        # one ulp above a knot: the next node, ds = -(chord) + ulp
        if P >= 4:
            add("knot_plus_ulp", [pt(up(sm[1])), pt(up(sm[mid]))], [2, mid + 1], 0)
        # one ulp above the last entry: IndexError, status 2, the rest of the scene NaN
        add("past_the_end", [pt(sm[P - 1]), pt(up(sm[P - 1])), pt(sm[1])], [P - 1, None, None], 2)
        add("past_the_end_first", [pt(INF), pt(sm[1])], [None, None], 2)
        # a NaN s ends the scene without a status, as its first point and in the middle
        add("nan_first", [pt(NAN), pt(sm[1])], [None, None], 0)
        add("nan_middle", [pt(sm[1]), pt(NAN), pt(sm[1])], [1, None, None], 0)
        add("no_points", [], [], 0)
    # P = 1 (and an empty line): s_map[1] does not exist
    for P in (0, 1):
        line, acc = chord_line(P, 300 + P)
        out.append(_f2c_case(f"P{P}_any_station", line, acc, [(0.0, 1.0, 0.0, 0.0), (-5.0, 1.0, 0.0, 0.0)], [None, None], 2))
        out.append(_f2c_case(f"P{P}_nan_first", line, acc, [(NAN, 1.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0)], [None, None], 0))
    # 1 - kappa l equal to 0 in bits (kappa = 0.5, l = 2): the divisions are by zero, as in the reference
    line, acc = chord_line(7, 307)
    line = line.copy()
    line[:, 3] = 0.5
    out.append(_f2c_case("P7_one_minus_kappa_l_zero", line, acc, [(acc[2], 2.0, 0.1, -0.01), (acc[3], 2.0, 0.0, 0.0), (acc[4], 2.0, -0.1, 0.0)],
                         [2, 3, 4], 0))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# bound cases: cal_lmin_lmax
# ---------------------------------------------------------------------------------------------------------------------------
OBS_WIDTH = 2.0
BOUND_N = tuple(range(1, 11)) + (32, 33, 34, 64, 65)
BOUND_OBS = 64
BOUND_CAP = 65


def _bound_case(name, dp_s, dp_l, obs, length, labels):
    """obs: rows (s, l); labels: per obstacle (lo, hi, centre) - argmin + 2, argmin + 2, argmin - by construction.  The expected
    bounds and status follow from the labels alone (ref path_planning.py:233-273): IndexError (EMP_ST_BOUND_INDEX, 4) at the first
    obstacle whose range lo..hi is not empty and reaches n."""
    dp_s, dp_l = np.asarray(dp_s, np.float64), np.asarray(dp_l, np.float64)
    n = len(dp_s)
    obs = np.asarray(obs, np.float64).reshape(len(obs), 2)
    assert len(labels) == len(obs) and len(obs) <= BOUND_OBS and n <= BOUND_CAP
    lmin, lmax = np.full(n, -10.0), np.full(n, 10.0)
    status = 0
    for (s, l), (lo, hi, centre) in zip(obs, labels):
        if lo <= hi and hi >= n:
            status = 4
            break
        below = bool(dp_l[centre] < l)                     # NaN obs_l: not below
        for j in range(lo, hi + 1):
            if below:
                lmax[j] = min(lmax[j], l - OBS_WIDTH / 2)
            elif not math.isnan(l):
                lmin[j] = max(lmin[j], l + OBS_WIDTH / 2)   # (max(a, NaN) keeps a)
    return dict(name=name, n=n, dp_s=dp_s, dp_l=dp_l, obs=obs, length=float(length), labels=tuple(labels), status=status,
                l_min=lmin, l_max=lmax)


@functools.lru_cache(maxsize=None)
def bounds():
    out = []
    for n in BOUND_N:
        s0 = 7.0
        st = s0 + np.arange(n)                             # stations 1 apart
        rng = np.random.default_rng(400 + n)
        dl = np.round(rng.uniform(-2.0, 2.0, n) * 4) / 4   # quarters: dp_l == obs_l can be hit exactly
        clip = lambda k: min(max(k, 0), n - 1)              # noqa: E731
        add = lambda name, obs, length, labels, st_=None, dl_=None: out.append(                 # noqa: E731
            _bound_case(f"n{n}_{name}", st if st_ is None else st_, dl if dl_ is None else dl_, obs, length, labels))
        for k in sorted({0, n // 2, max(n - 4, 0), max(n - 3, 0), max(n - 2, 0), n - 1}):
            # front, back and centre each exactly midway between two stations: the first station wins.  centre s0 + k + 0.5, half
            # length 1: front midway between k - 1 and k (k - 1 wins, clipped at 0 where there is no tie), back between k + 1 and k + 2
            c = s0 + k + 0.5
            f, b, m = clip(k - 1), (k + 1 if k + 2 <= n - 1 else n - 1), (k if k + 1 <= n - 1 else n - 1)
            add(f"midway_{k}", [(c, 5.0)], 2.0, [(f + 2, b + 2, m)])
            add(f"midway_{k}_from_the_left", [(c, -5.0)], 2.0, [(f + 2, b + 2, m)])
            # the same three exactly on stations k - 1, k + 1, k
            add(f"on_station_{k}", [(s0 + k, 5.0)], 2.0, [(clip(k - 1) + 2, clip(k + 1) + 2, k)])
        add("before_station_0", [(s0 - 3.0, 5.0)], 2.0, [(2, 2, 0)])
        add("past_the_last_station", [(s0 + n + 3.0, 5.0)], 2.0, [(n + 1, n + 1, n - 1)])
        # dp_l[centre] == obs_l in bits: not `<`, the l_min branch
        k = n // 2
        add("l_equal", [(s0 + k, dl[k])], 2.0, [(clip(k - 1) + 2, clip(k + 1) + 2, k)])
        add("nan_obs_s", [(NAN, 5.0)], 2.0, [(2, 2, 0)])               # no |s_j - NaN| is `<` another: station 0 three times
        add("nan_obs_l", [(s0, NAN)], 2.0, [(2, clip(1) + 2, 0)])
        add("no_obstacle", [], 2.0, [])
        if n >= 3:
            # the last station repeated in the data: a target beyond it finds the first of the two
            rep = st.copy()
            rep[n - 1] = rep[n - 2]
            add("last_station_repeated", [(s0 + n + 3.0, 5.0)], 2.0, [(n, n, n - 2)], st_=rep)
            # lo > hi with hi >= n: decreasing stations turn front and back round; the reference's empty range raises nothing
            dec = st[::-1].copy()
            add("empty_range_past_n", [(s0 + 0.5, 5.0)], 1.0, [(n - 1 + 2, n - 2 + 2, n - 2)], st_=dec)
        if n >= 6:
            k = n - 5
            # two obstacles bound the same stations from the same side in either order, and from opposite sides (l_min > l_max)
            for tag, ls in (("same_side_ab", (4.0, 6.0)), ("same_side_ba", (6.0, 4.0)), ("same_side_left_ab", (-4.0, -6.0)),
                            ("same_side_left_ba", (-6.0, -4.0)), ("opposite", (dl[k] + 0.25, dl[k] - 0.25)), ("opposite_ba", (dl[k] - 0.25, dl[k] + 0.25))):
                add(tag, [(s0 + k, ls[0]), (s0 + k + 0.5, ls[1])], 2.0, [(k - 1 + 2, k + 1 + 2, k), (k - 1 + 2, k + 1 + 2, k)])
            # a legal obstacle, then one whose range reaches n: the status wins
            add("legal_then_index", [(s0 + 1, 5.0), (s0 + n - 1, 5.0)], 2.0, [(2, 4, 1), (n - 2 + 2, n - 1 + 2, n - 1)])
    # obstacle counts 8, 9 and 64 (one per lane of the cycle's groups, and a second round): obstacle j on station j mod (n - 4)
    for n, k in ((12, 8), (12, 9), (65, 64), (34, 64)):
        st = 3.0 + np.arange(n)
        rng = np.random.default_rng(500 + n + k)
        dl = np.round(rng.uniform(-2.0, 2.0, n) * 4) / 4
        obs, lab = [], []
        for j in range(k):
            q = 1 + j % (n - 4)
            obs.append((3.0 + q + (0.5 if j % 2 else 0.0), 5.0 if j % 3 else -5.0))
            lab.append((q - 1 + 2, q + 1 + 2, q))
        out.append(_bound_case(f"n{n}_{k}_obstacles", st, dl, obs, 2.0, lab))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# heading cases: cal_heading_kappa
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def headings():
    """name, xy (m, 2), and `theta`: the headings known from the construction (None: compare with the port alone)."""
    out = []
    add = lambda name, xy, theta=None: out.append(dict(name=name, xy=np.asarray(xy, np.float64).reshape(-1, 2), theta=theta))  # noqa: E731
    # a line heading west whose dy changes sign: theta jumps between -pi and +pi, and the reference's mean of differences gives
    # the curvature there the wrong sign and size (sin of +-pi where the line is straight)
    y = [0.0, -0.0, -0.0, 0.0, 0.0, -0.0, 0.0]
    add("west_dy_sign", [(-float(i), y[i]) for i in range(7)])
    add("west_wobble", [(-2.0 * i, (0.25, -0.25)[i % 2] * (i % 3 != 0)) for i in range(9)])
    add("west_minus_zero", [(-float(i), -0.0) for i in range(5)], [math.pi] * 5)          # (-0.0) - (-0.0) = +0.0: +pi
    add("east_plus_zero", [(float(i), 0.0) for i in range(5)], [0.0] * 5)
    # a repeated point: dx = dy = 0 in the middle of three equal points, theta 0 there and a division by zero
    add("repeated_point", [(0.0, 0.0), (1.0, 1.0), (2.0, 2.0), (2.0, 2.0), (2.0, 2.0), (3.0, 3.0), (4.0, 4.0)])
    add("all_the_same_point", [(1.5, -2.0)] * 4, [0.0] * 4)
    add("two_equal_points", [(1.5, -2.0)] * 2, [0.0] * 2)
    # a reversal of 180 degrees: the centred difference at the turn is zero
    add("reversal", [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (1.0, 0.0), (0.0, 0.0)])
    add("reversal_off_axis", [(0.0, 0.0), (3.0, 4.0), (6.0, 8.0), (3.0, 4.5), (0.0, 1.0)])
    add("m2", [(0.0, 0.0), (3.0, 4.0)], [math.atan2(4.0, 3.0)] * 2)
    add("m3", [(0.0, 0.0), (3.0, 4.0), (7.0, 7.0)])
    for m in (63, 64, 65):
        line, _ = chord_line(m, 600 + m)
        add(f"chords_{m}", line[:, :2])
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# cycle scenes: plan_cycle on lines of unit chords along the x axis
# ---------------------------------------------------------------------------------------------------------------------------
# Node i sits on (i, 0) - the last node half a unit on where a scene asks for it - so the cumulative chord length is i, and with the
# origin on node o and the planning start on node p (dot2(0, 0, c, s) = 0) s_map[i] = i - o and begin_s = p - o in bits.  With
# sample_s = 2 and sampling_res = 1 the decimated QP stations are begin_s + 2 k and the path stations begin_s, begin_s + 1,
# begin_s + 3, ..., begin_s + 2 col - 1, begin_s + 2 col: every one of them on a knot, so every trajectory point's lookup is a tie.
# Node headings are off the axis by 0.05 to 0.15 rad: a station on knot i + 1 extrapolated from node i (the label) is at least
# 0.05 m from node i + 1 itself.  The node an obstacle matches has heading 0 exactly: the obstacle sits on its normal, obs_s is
# the node's s in bits and obs_l the distance (5).
CYCLE_COLS = (21, 29, 60, 66)                         # <8, 3> 24 points, <8, 4> 32, <16, 4> 63; 69 points: the wave kernel, past lane 63
CYCLE_LANES = {21: 16, 29: 16, 60: 32, 66: 64}        # lanes per scene of the default form's passes
CYCLE_OBS_LENGTH, CYCLE_OBS_WIDTH = 4.0, 7.0          # edges s +- 2; l_max = 5 - 3.5 = 1.5 (the pinned end needs l_max - host_w / 2 >= 0)
CYCLE_L_EQUAL_COLS = (21, 29)
CYCLE_ORIGIN = 3                                      # node of the s axis' origin


def cycle_specs(col):
    """Per scene: dict(kind, p = start node, n_ref, half_end, obs_k, obs_node, points = expected trajectory points or None, status bit).
    m trajectory points need the path station begin_s + 2 (m - 2) - 1 ON the end of the line: n_ref = p + 2 (m - 2)."""
    SL, full = CYCLE_LANES[col], col + 3
    out = []
    add = lambda kind, p, n_ref, points, status=0, half_end=False, obs_k=None, off=0.0, obs_node=None: out.append(          # noqa: E731
        dict(kind=kind, p=p, n_ref=n_ref, half_end=half_end, obs_k=obs_k, points=points, status=status, off=off, obs_node=obs_node))
    p = 5
    add("full", p, p + 2 * col + 1, full)                                  # the last station on the last node
    add("full_plus_one", p, p + 2 * col + 2, full)
    for m in sorted({SL - 1, SL, SL + 1, min(2 * SL, full) - 1, min(2 * SL, full)} - {full, full + 1}):
        if 3 <= m < full:
            add(f"cut_{m}", p, p + 2 * (m - 2), m)                        # station m - 2 on the end: kept
    m = SL
    add(f"half_before_{m + 1}", p, p + 2 * (m - 2) + 2, m, half_end=True)   # the end half a unit before the next station: dropped
    add("start_on_last_but_one", p, p + 2, 3)                              # begin_s + 1 is the end: start, path point 0 and 1
    add("start_on_last", p, p + 1, 2)                                      # begin_s is the end: start and path point 0
    # bounds: an obstacle at s = begin_s + 2 k + 1, half length 2: front, back and centre each midway between two decimated
    # stations, lo = (k - 1) + 2, hi = (k + 1) + 2, centre k
    n = col + 1
    add("obs_mid", p, p + 2 * col + 1, full, obs_k=n // 2)
    add("obs_hi_on_n_minus_1", p, p + 2 * col + 1, full, obs_k=n - 4)
    add("obs_hi_on_n", p, p + 2 * col + 1, None, status=4, obs_k=n - 3)
    # dp_l[centre] == obs_l: an obstacle ON a node 10 m behind the start (l = 0 like the start's; too far for the DP to mind): all
    # three targets lie before station 0, so lo = hi = 2 and centre = 0, and `0 < 0` is false: the l_min side.  Only on the two
    # small lattices: the library's dp_l[0] is the start's l = 0 exactly, the reference's is 0 up to the residue of its 6 x 6
    # inverse (+-1e-13, path_planning.py:405-420), whose sign decides the reference's side; on these two it is not negative (the
    # builder in tests/lookup_truth.py asserts it), on the 60- and 66-column lattices it is and the reference bounds the other side
    if col in CYCLE_L_EQUAL_COLS:
        add("obs_l_equal", 14, 14 + 2 * col + 1, full, obs_node=4)
    add("qp_refused", p, p + 2 * col + 1, None, status=8, off=9.0)         # the start 9 m beside the line: no feasible path
    add("out_of_range", 12, 9, None, status=2)                             # the start beyond the line's end
    return out


def cycle_inputs(col):
    """The batch of cycle_specs(col): plan_cycle's arrays (lines NaN behind their count) and, per scene, (lo, hi, centre) of its
    obstacle."""
    specs = cycle_specs(col)
    B, P = len(specs), max(s["n_ref"] for s in specs)
    rng = np.random.default_rng(700 + col)
    ref = np.full((B, P, 4), NAN)
    n_ref = np.array([s["n_ref"] for s in specs], np.int32)
    origin, start, v = np.zeros((B, 2)), np.zeros((B, 2)), np.zeros((B, 2))
    obs = np.full((B, 2, 2), NAN)
    n_obs = np.zeros(B, np.int32)
    labels = []
    for b, s in enumerate(specs):
        n = s["n_ref"]
        x = np.arange(n, dtype=np.float64)
        if s["half_end"]:
            x[n - 1] = x[n - 2] + 0.5
        th = rng.uniform(0.05, 0.15, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        kp = rng.uniform(0.01, 0.03, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
        lab = None
        if s["obs_k"] is not None:
            k = s["obs_k"]
            q = s["p"] + 2 * k + 1
            th[q] = 0.0
            obs[b, 0] = (float(q), 5.0)
            n_obs[b] = 1
            lab = (k - 1 + 2, k + 1 + 2, k)
        if s["obs_node"] is not None:
            obs[b, 0] = (float(s["obs_node"]), 0.0)
            n_obs[b] = 1
            lab = (2, 2, 0)
        labels.append(lab)
        ref[b, :n] = np.column_stack([x, np.zeros(n), th, kp])
        origin[b] = (float(CYCLE_ORIGIN), 0.0)
        start[b] = (float(s["p"]), s["off"])
        hp = th[min(s["p"], n - 1)]
        v[b] = (8.0 * math.cos(hp), 8.0 * math.sin(hp))
    return dict(ref_line=ref, n_ref=n_ref, origin_xy=origin, start_xy=start, start_v=v, start_a=np.zeros((B, 2)), obs_xy=obs,
                n_obs=n_obs), labels
