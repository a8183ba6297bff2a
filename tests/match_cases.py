"""Hard inputs for the nearest-node match scans (NumPy only, deterministic): the serial match_scan (emp_frenet_core.h), the
value-only wave scan for lines of at most 64 nodes and the chunked wave scan (emp_tail_kernels.h) share one rule, the
reference's ordered scan (planning_utils.py:72-92, :123-167, :383-402): only a strict `<` improves, and the scan stops after
`limit` consecutive non-improvements.  A line for a match scan is a list of nodes, so the tables build the distance profile
directly and every case carries its expected index as a label that follows from how it was built, not from any implementation.

Where a decision is exact: the deciding nodes sit on integer lattice points of norm 3, 5, 25 or 65 round the query, the other
nodes at integer distances above 100, so dx*dx + dy*dy is exact, equal distances are equal in bits and unequal ones differ by
at least 1 m.  Half the cases are shifted by a dyadic offset (query and nodes alike), which keeps every difference exact.
Every node has its own heading (0.37 i rad) and a curvature of +-0.05, so that projections on two equally distant nodes differ.

  whole_line()   the scans from node 0 with limit 50, at every line length of P_ALL
  windowed()     find_match_points with is_first_run = 0 (and the front end of the cycle): limit 5, direction by the sign of flag
  window()       global paths for the 51-node window of the reference line (sampling)"""
from __future__ import annotations

import functools
import math

import numpy as np

LIMIT = 50
WINDOW_LIMIT = 5
P_VALUE_ONLY = (51, 52, 63, 64)                      # one node per lane: match_scan_wave64
P_CHUNKED = (65, 113, 114, 115, 128, 129, 130)       # chunks of 64 with a carry: match_scan_wave
P_ALL = P_VALUE_ONLY + P_CHUNKED
MAX_REF = 130
FAMILIES = ("ties", "stop", "hairpin", "nonfinite")
OFFSET = (16.5, -8.25)                               # dyadic: lattice point + offset and their difference are exact
STOP_NODES = (50, 63, 64, 127, 128)                  # lane `limit`, lane 63, lane 0 of the second chunk, node 127, node 128
SEAMS = ((15, 16), (31, 32), (47, 48), (63, 64), (127, 128))      # DPP row seams and chunk seams


@functools.lru_cache(maxsize=None)
def lattice(n):
    """All integer points of norm n, by angle."""
    pts = [(x, y) for x in range(-n, n + 1) for y in range(-n, n + 1) if x * x + y * y == n * n]
    return tuple(sorted(pts, key=lambda p: math.atan2(p[1], p[0])))


def headings(P):
    return 0.37 * np.arange(P)


def curvatures(P):
    return np.where(np.arange(P) % 2 == 0, 0.05, -0.05)


def _line(P, L, special, shifted):
    """P nodes round a query at the origin (shifted: at OFFSET).  Nodes before L come strictly nearer one by one (distance 400 - i),
    nodes behind L are farther than every special node (distance 100 + i); `special` places nodes on given points."""
    xy = np.zeros((P, 2))
    for i in range(P):
        xy[i] = (-(400.0 - i), 0.0) if i < L else (0.0, 100.0 + i)
    for i, p in special.items():
        xy[i] = p
    q = np.zeros(2)
    if shifted:
        xy += OFFSET
        q = q + OFFSET
    nodes = np.concatenate([xy, headings(P)[:, None], curvatures(P)[:, None]], axis=1)
    return nodes, q


def _case(name, family, P, L, special, label, shifted, tied=(), stop=None, others=(), edit=None, query=None):
    nodes, q = _line(P, L, special, shifted)
    if edit:
        for i, col, v in edit:
            nodes[i, col] = v
    if query is not None:
        q = np.array(query, np.float64)
    nodes.setflags(write=False)
    q.setflags(write=False)
    # candidates: the indices another scan could answer - the other tied nodes, the label's neighbours, the node behind the stop
    cand = sorted({i for i in list(tied) + list(others) + [label - 1, label + 1] if 0 <= i < P and i != label})
    return dict(name=f"{name}_P{P}", family=family, kind=name, P=P, nodes=nodes, q=q, label=int(label), tied=tuple(tied), stop=stop,
                candidates=tuple(cand), finite=bool(np.isfinite(nodes[:label + 1, :2]).all() and np.isfinite(q).all()))


def _ring(n, count, start=0):
    pts = lattice(n)
    return [pts[(start + 7 * j) % len(pts)] for j in range(count)]       # stride 7: neighbours in the line are far apart on the ring


def _ties(P, sh):
    out = []
    a = lattice(5)
    out.append(_case("tie2", "ties", P, 5, {5: a[1], 9: a[6]}, 5, sh, tied=(5, 9)))
    out.append(_case("tie3", "ties", P, 5, {5: a[2], 6: a[9], 30: a[4]}, 5, sh, tied=(5, 6, 30)))
    L = min(2, P - (LIMIT + 1))
    idx = list(range(L, L + LIMIT + 1))
    out.append(_case("tie51", "ties", P, L, dict(zip(idx, _ring(65, LIMIT + 1))), L, sh, tied=idx))
    for lo, hi in SEAMS:
        if hi < P:
            out.append(_case(f"seam{lo}_{hi}", "ties", P, lo, {lo: a[3], hi: a[8]}, lo, sh, tied=(lo, hi)))
            if hi + 1 < P:                                                       # three in a row across the seam
                out.append(_case(f"seam3_{lo}_{hi}", "ties", P, lo, {lo: a[0], hi: a[5], hi + 1: a[10]}, lo, sh, tied=(lo, hi, hi + 1)))
    out.append(_case("whole", "ties", P, 0, dict(zip(range(P), _ring(65, P, 3))), 0, sh, tied=range(P)))
    return out


def _stop(P, sh):
    out = []
    far, near, nearest = lattice(65), lattice(25), lattice(5)
    for node in STOP_NODES:
        L = node - LIMIT
        for off in (49, 50, 51):
            if L + off > P - 1:
                continue
            taken = off <= LIMIT
            out.append(_case(f"stop{node}_plus{off}", "stop", P, L, {L: near[4], L + off: nearest[7]}, L + off if taken else L, sh,
                             stop=(L, off, taken), others=(L, L + off)))
        if L + 100 <= P - 1:             # an improvement at L + 49 resets the counter; a nearer node 51 behind that is not seen
            out.append(_case(f"stop{node}_two_stage", "stop", P, L, {L: far[5], L + 49: near[11], L + 100: nearest[2]}, L + 49, sh,
                             stop=(L + 49, 51, False), others=(L, L + 100)))
    L = P - LIMIT                        # P - 1 - L < 50: the scan runs to the end of the line
    out.append(_case("never_stops", "stop", P, L, {L: nearest[5]}, L, sh, stop=(L, LIMIT - 1, None)))
    out.append(_case("last_node_improves", "stop", P, L, {L: near[9], P - 1: nearest[0]}, P - 1, sh, stop=(L, LIMIT - 1, True), others=(L,)))
    return out


def _hairpin(P, sh):
    """Nearest node 8 going out, nearer still to a node more than `limit` behind it: the answer is 8."""
    if P - 1 <= 8 + LIMIT:
        return []
    back = 70 if P > 70 else P - 1
    return [_case("hairpin", "hairpin", P, 8, {8: lattice(5)[8], back: (0, -3)}, 8, sh, stop=(8, back - 8, False), others=(back,))]


def _nonfinite(P, sh):
    nan, inf = float("nan"), float("inf")
    a = lattice(5)
    out = [
        _case("query_nan", "nonfinite", P, 10, {10: a[1]}, 0, sh, query=(nan, 0.0)),
        _case("query_inf", "nonfinite", P, 10, {10: a[1]}, 0, sh, query=(inf, 0.0)),
        _case("nan_before_min", "nonfinite", P, 10, {10: a[4]}, 10, sh, edit=[(4, 0, nan)]),
        _case("nan_at_min", "nonfinite", P, 10, {10: a[4]}, 11, sh, edit=[(10, 0, nan)]),      # passed over: node 11 (111 m) beats node 9
        _case("nan_after_min", "nonfinite", P, 10, {10: a[4]}, 10, sh, edit=[(12, 1, nan)]),
        _case("inf_x_at_min", "nonfinite", P, 10, {10: a[7]}, 11, sh, edit=[(10, 0, inf)]),
        # the first 49 distances NaN: node 49 is the first improvement (49 non-improvements), node 50 the minimum
        _case("nan_first49", "nonfinite", P, 50, {50: a[6]}, 50, sh, edit=[(i, 0, nan) for i in range(49)]),
        # the first 50: the scan has stopped at node 49 with its initial answer, node 0 (a NaN node)
        _case("nan_first50", "nonfinite", P, 50, {50: a[6]}, 0, sh, edit=[(i, 0, nan) for i in range(50)]),
        _case("inf_first50", "nonfinite", P, 50, {50: a[6]}, 0, sh, edit=[(i, 1, inf) for i in range(50)]),
        _case("nan_all", "nonfinite", P, 50, {50: a[6]}, 0, sh, edit=[(i, 0, nan) for i in range(P)]),
    ]
    return out


@functools.lru_cache(maxsize=None)
def whole_line():
    """Every family at every P it can be built at; read-only."""
    out = []
    for P in P_ALL:
        for k, fam in enumerate((_ties, _stop, _hairpin, _nonfinite)):
            out += fam(P, (P + k) % 2 == 1)
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def distances(c):
    """The distances the scan compares, as the reference forms them (planning_utils.py:390)."""
    return np.array([math.sqrt((float(n[0]) - float(c["q"][0])) ** 2 + (float(n[1]) - float(c["q"][1])) ** 2) for n in c["nodes"]])


# ----------------------------------------------------------------------------------------------------------------------
# windowed search: limit 5, forward where flag > 0 and backward otherwise, from pre_match_index `st`
# ----------------------------------------------------------------------------------------------------------------------
WP = 56          # nodes of a windowed line: node i at (2 (i - 20), 0), node 20 at the origin
ST = 20


def _wcase(name, q, label, st=ST, theta_st=0.0, move=None, P=WP, n_ref=None, flag=None):
    nodes = np.concatenate([np.stack([2.0 * (np.arange(P) - ST), np.zeros(P)], axis=1), headings(P)[:, None], curvatures(P)[:, None]], axis=1)
    if 0 <= st < P:
        nodes[st, 2] = theta_st
    for i, p in (move or {}).items():
        nodes[i, :2] = p
    nodes.setflags(write=False)
    n = P if n_ref is None else n_ref
    return dict(name=name, nodes=nodes, n_ref=n, q=np.array(q, np.float64), st=int(st), label=int(label), flag=flag,
                in_range=bool(n >= 1 and 0 <= st < n))


@functools.lru_cache(maxsize=None)
def windowed():
    """label: the match index, -1 where pre_match_index lies outside the line (the reference raises IndexError).  `flag`, where
    given, is the exact value of the dot product that chooses the direction (heading 0 at `st`: flag = q.x - node.x, exactly)."""
    tiny = 5e-324
    nan = float("nan")
    fwd_bait, back_bait = {ST + 1: (0.0, 2.0)}, {ST - 1: (0.0, 2.0)}
    xe = 2.0 * (WP - 1 - ST)                      # x of the last node
    x0 = -2.0 * ST
    out = [
        # the query on the normal through node st: flag = +0.0 exactly, the search walks backward and does not see node st + 1 at 1 m
        _wcase("flag_plus_zero", (0.0, 3.0), ST, move=fwd_bait, flag=0.0),
        # the query on node st, heading in the third quadrant: both products are -0.0.  The library's fma(a1, b1, a0 * b0) sums them
        # to -0.0, NumPy's dot starts from +0.0 and returns +0.0: backward either way, and the distance 0 wins at once
        _wcase("flag_minus_zero", (0.0, 0.0), ST, theta_st=-2.5, move=fwd_bait),
        _wcase("flag_plus_ulp", (tiny, 3.0), ST + 1, move=fwd_bait, flag=tiny),
        _wcase("flag_minus_ulp", (-tiny, 3.0), ST, move=fwd_bait, flag=-tiny),
        _wcase("flag_plus_2m40", (2.0 ** -40, 3.0), ST + 1, move=fwd_bait, flag=2.0 ** -40),
        _wcase("flag_minus_2m40", (-2.0 ** -40, 3.0), ST, move=fwd_bait, flag=-2.0 ** -40),
        _wcase("flag_nan", (1.0, 3.0), ST, theta_st=nan, move=fwd_bait),                    # NaN > 0 is false: backward
        _wcase("flag_positive_ignores_the_back", (1.0, 3.0), ST + 1, move={**fwd_bait, ST - 1: (1.0, 3.5)}, flag=1.0),
        _wcase("flag_negative_ignores_the_front", (-1.0, 3.0), ST - 1, move={**back_bait, ST + 1: (-1.0, 3.5)}, flag=-1.0),
        # either end of the line: one node
        _wcase("backward_from_0", (x0 - 1.0, 1.0), 0, st=0, move={2: (x0 - 1.0, 1.5)}, flag=-1.0),
        _wcase("forward_from_last", (xe + 1.0, 1.0), WP - 1, st=WP - 1, move={WP - 3: (xe + 1.0, 1.5)}, flag=1.0),
        _wcase("forward_to_the_last", (xe, 0.25), WP - 1, st=WP - 3, flag=xe - 2.0 * (WP - 3 - ST)),
        _wcase("backward_to_0", (x0, 0.25), 0, st=2, flag=x0 - 2.0 * (2 - ST)),
        # an improvement after 4 non-improvements is taken, after 5 it is not
        _wcase("forward_after_4", (0.5, 1.0), ST + 5, move={ST + 5: (0.5, 1.5)}, flag=0.5),
        _wcase("forward_after_5", (0.5, 1.0), ST, move={ST + 6: (0.5, 1.5)}, flag=0.5),
        _wcase("backward_after_4", (-0.5, 1.0), ST - 5, move={ST - 5: (-0.5, 1.5)}, flag=-0.5),
        _wcase("backward_after_5", (-0.5, 1.0), ST, move={ST - 6: (-0.5, 1.5)}, flag=-0.5),
        # ties: the first met wins - the lower index forward, the higher index backward
        _wcase("tie_forward", (3.0, 1.0), ST + 1, flag=3.0),
        _wcase("tie_backward", (-3.0, 1.0), ST - 1, flag=-3.0),
        _wcase("tie_forward_at_st", (1.0, 1.0), ST, flag=1.0),
        _wcase("tie_backward_at_st", (-1.0, 1.0), ST, flag=-1.0),
        _wcase("tie_of_three_forward", (3.0, 1.0), ST + 1, move={ST + 4: (2.0, 2.0)}, flag=3.0),
        # non-finite: the query NaN matches node 0 wherever the search started
        _wcase("query_nan", (nan, 1.0), 0),
        _wcase("nan_node_in_the_way", (6.5, 1.0), ST + 3, move={ST + 1: (nan, 0.0)}, flag=6.5),
        # pre_match_index outside [0, P), and an empty line
        _wcase("st_minus_1", (1.0, 1.0), -1, st=-1),
        _wcase("st_equals_P", (1.0, 1.0), -1, st=WP),
        _wcase("st_far_outside", (1.0, 1.0), -1, st=10 ** 6),
        _wcase("st_beyond_a_short_line", (1.0, 1.0), -1, st=30, n_ref=30),
        _wcase("st_last_of_a_short_line", (2.0 * 9 + 0.5, 1.0), 29, st=29, n_ref=30, flag=0.5),       # the padding behind it is not walked
        _wcase("empty_line", (1.0, 1.0), -1, st=0, n_ref=0),
    ]
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------------------
# the 51-node window of the reference line
# ----------------------------------------------------------------------------------------------------------------------
WINDOW_G = (50, 51, 52, 60, 140)
MAX_GLOBAL = 140
REF_POINTS = 51


def global_path(G):
    """G nodes 2 m apart on a gentle S, headings and curvature those of the curve."""
    i = np.arange(G)
    h = 0.3 + 0.25 * np.sin(0.05 * i)
    xy = np.zeros((G, 2))
    xy[1:] = np.cumsum(2.0 * np.stack([np.cos(h[:-1]), np.sin(h[:-1])], axis=1), axis=0)
    xy += (12.0, -7.0)
    kappa = np.gradient(h) / 2.0
    return np.concatenate([xy, h[:, None], kappa[:, None]], axis=1)


def window_start(G, m):
    """First node of the window by the rule of planning_utils.py:244-259: 10 back and 40 forward, shifted at either end."""
    return min(max(m - 10, 0), G - REF_POINTS)


@functools.lru_cache(maxsize=None)
def window():
    """The match is forced to m by putting the query on node m.  label m; first = window start, None where the path is shorter
    than 51 nodes (EMP_ST_S_OUT_OF_RANGE, zero line)."""
    out = []
    for G in WINDOW_G:
        path = global_path(G)
        path.setflags(write=False)
        for m in sorted({0, 9, 10, 11, G - 42, G - 41, G - 40, G - 1}):
            for first_run in (1, 0):
                out.append(dict(name=f"G{G}_m{m}_{'first' if first_run else 'windowed'}", G=G, n_global=G, path=path, q=path[m, :2].copy(), m=m,
                                first_run=first_run, st=m if not first_run else -7, label=m,
                                first=window_start(G, m) if G >= REF_POINTS else None))
    path = global_path(MAX_GLOBAL)
    path.setflags(write=False)
    for m in (0, MAX_GLOBAL - 1):        # a count beyond the row's capacity is clamped to it
        out.append(dict(name=f"clamped_m{m}", G=MAX_GLOBAL, n_global=1000, path=path, q=path[m, :2].copy(), m=m, first_run=0, st=m, label=m,
                        first=window_start(MAX_GLOBAL, m)))
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------------------
# ragged batches: rows padded to the widest line, the padding poisoned
# ----------------------------------------------------------------------------------------------------------------------
def padded(lines, counts, width, poison, queries):
    """[B][width][4]: line b in its first counts[b] slots; behind them NaN, or "hostile": nodes exactly on the scene's query
    with another heading and curvature."""
    B = len(lines)
    out = np.full((B, width, 4), np.nan)
    for b in range(B):
        n = min(int(counts[b]), len(lines[b]), width)
        out[b, :n] = lines[b][:n]
        if poison == "hostile":
            q = np.where(np.isfinite(queries[b]), queries[b], 0.0)
            out[b, n:] = (q[0], q[1], 1.0 + 0.11 * b, 0.3)
    return out
