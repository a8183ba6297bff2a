"""Hard corridors for the path QP (Quadratic_planning), as plain NumPy: what tests/test_path_qp_cases_host.py checks on the CPU
and tests/test_gpu_path_qp_cases.py feeds to emp_path_qp.  A helper module (no fixtures, no hooks).

A case is Case(l_min, l_max, start_l3, expectation, ...): the corridor of n stations, the pinned start state (l, dl, ddl) and what
the construction intends, "feasible" or "infeasible".  The default parameters of api.qp_params() hold throughout: ds = 2,
d1 = d2 = 3, host width 3, so station i is constrained by

    l_min[max(i - 2, 0)] + 1.5  <=  l +- 3 dl  <=  l_max[min(i + 2, n - 1)] - 1.5          (ref path_planning.py:126-139)

and every family below is written in that station space (``corridor`` shifts the ranges onto l_min / l_max).

The yardstick is the dense reference formulation and nothing of the project's solvers: oracle.ref_port.path_qp_matrices ->
oracle.qp_dense.solve_qp, accepted with status "optimal" and a KKT certificate of its own x only (``truth``).  A case is
infeasible by construction (``infeasible_by_inspection``: the start state outside its own range, or a station whose range is
empty) or because the oracle does not end "optimal"; a case meant feasible that the oracle does not certify is "uncertified" and
compared with nothing - the host test keeps those below 10 %.  The seeds of the random family were chosen per size so that the
oracle certifies every one of them, then frozen."""
import collections
import functools

import numpy as np

from oracle import qp_dense
from oracle import ref_port as rp

HALF_W = 1.5                # half the host width: what every bound is tightened by
REACH = 2                   # ceil(d1 / ds) = ceil(d2 / ds): how many stations ahead / behind a corner looks
WIDE = 10.0                 # the open corridor (cal_lmin_lmax's own +-10)
TINY = (4, 5, 6, 7, 8)
SIZES = TINY + (34, 35, 66, 67, 68, 100, 256)
SPLINE_SIZES = (34, 35, 66, 67, 68)          # the dense oracle needs seconds to give up on these at n >= 100
CHICANE_PERIOD = 10         # stations between the starts of two obstacles (one upper, the next lower)
PINCH_GAP = 1e-6
QP_PRM = np.array([2.0, 1000.0, 3000.0, 150.0, 250.0, 3.0, 3.0, 3.0])   # ds, w_l, w_ddl, w_dddl, w_centre, d1, d2, w (api.qp_params())

Case = collections.namedtuple("Case", "l_min l_max start_l3 expectation name family n")


def corridor(lb, ub):
    """Station ranges lb[i] <= l +- 3 dl <= ub[i] -> (l_min, l_max).  Stations 0, 1 share l_min[0] with station 2 and stations
    n-2, n-1 share l_max[n-1] with station n-3: their own entries of lb / ub are not used."""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    n = len(lb)
    l_min, l_max = np.full(n, -WIDE), np.full(n, WIDE)
    l_min[:n - REACH] = lb[REACH:] - HALF_W
    l_max[REACH:] = ub[:n - REACH] + HALF_W
    return l_min, l_max


def station_ranges(l_min, l_max):
    n = len(l_min)
    lb = np.array([l_min[max(i - REACH, 0)] + HALF_W for i in range(n)])
    ub = np.array([l_max[min(i + REACH, n - 1)] - HALF_W for i in range(n)])
    return lb, ub


def open_ranges(n):
    return np.full(n, -WIDE + HALF_W), np.full(n, WIDE - HALF_W)


def infeasible_by_inspection(c):
    """The two rules a reader can apply without solving anything: the pinned start (or the pinned end, l = dl = ddl = 0) outside
    its station's range, or a station whose range is empty."""
    lb, ub = station_ranges(c.l_min, c.l_max)
    if (lb > ub).any():
        return True
    l0, dl0 = c.start_l3[0], c.start_l3[1]
    lo, hi = l0 - 3.0 * abs(dl0), l0 + 3.0 * abs(dl0)
    return bool(hi > ub[0] or lo < lb[0] or 0.0 > ub[-1] or 0.0 < lb[-1])


# ---------------------------------------------------------------------------------------------------------------------
# families (each: n -> list of (suffix, l_min, l_max, start, expectation)); a family returns [] at a size it has no case for
# ---------------------------------------------------------------------------------------------------------------------
def _open(n):
    return [("zero", *corridor(*open_ranges(n)), (0.0, 0.0, 0.0), "feasible")]


def _offset(n):
    return [("start", *corridor(*open_ranges(n)), (0.35, -0.04, 0.008), "feasible")]


def chicane_blocks(n):
    """[(first station, +1 upper bound / -1 lower bound)] of the 3-station obstacles, and the narrowed station."""
    blocks = [(6 + CHICANE_PERIOD * k, 1 if k % 2 == 0 else -1) for k in range(n) if 6 + CHICANE_PERIOD * k + 2 <= n - 7]
    k_mid = max(0, min(len(blocks) - 2, len(blocks) // 2 - 1)) if len(blocks) > 1 else 0
    narrow = blocks[k_mid][0] + 6 if blocks else None
    return blocks, narrow


def _chicane(n):
    """3-station one-sided obstacles at +-0.5 m (station ranges <= -1 / >= +1), alternating every CHICANE_PERIOD stations, and one
    station between two of them whose range is host width + 0.2 m wide."""
    blocks, narrow = chicane_blocks(n)
    if n in TINY:                                        # no room for obstacles: the narrowed station alone, where one is free
        if n < 6:
            return []
        lb, ub = open_ranges(n)
        lb[n // 2], ub[n // 2] = -0.1, 0.1
        return [("narrow", *corridor(lb, ub), (0.35, -0.04, 0.008), "feasible")]
    lb, ub = open_ranges(n)
    for s, side in blocks:
        if side > 0:
            ub[s:s + 3] = -1.0
        else:
            lb[s:s + 3] = 1.0
    lb[narrow], ub[narrow] = -0.1, 0.1
    return [("alt", *corridor(lb, ub), (0.1, 0.01, 0.0), "feasible")]


# frozen: at every size the dense oracle certifies both (at other seeds it ends "unknown": the generator does not look ahead)
RANDOM_SEEDS = {4: (0, 1), 5: (46, 51), 6: (0, 1), 7: (0, 21), 8: (4, 8), 34: (34, 1034), 35: (35, 1035), 66: (66, 1066),
                67: (67, 1067), 68: (68, 1068), 100: (100, 1100), 256: (1256,)}


def random_case(n, seed):
    rng = np.random.default_rng(seed)
    l_min, l_max = np.full(n, -WIDE), np.full(n, WIDE)
    k = int(rng.integers(1, 3)) if n < 12 else int(rng.integers(max(1, n // 16), max(2, n // 8) + 1))
    for _ in range(k):
        a = int(rng.integers(REACH + 1, max(REACH + 2, n - 4)))
        w = 1 if n < 12 else int(rng.integers(1, 4))
        if rng.random() < 0.5:
            l_max[a:a + w] = rng.uniform(0.5, 4.0)
        else:
            l_min[a:a + w] = rng.uniform(-4.0, -0.5)
    start = (rng.uniform(-0.4, 0.4), rng.uniform(-0.05, 0.05), rng.uniform(-0.01, 0.01))
    return l_min, l_max, start


def _random(n):
    return [(f"seed{s}", *random_case(n, s), "feasible") for s in RANDOM_SEEDS[n]]


def _bound(n):
    """The pinned start exactly on its upper bound l_max[2] - 1.5, and 1e-12 inside it."""
    l_min, l_max = corridor(*open_ranges(n))
    l_max[min(REACH, n - 1)] = 2.0
    on = l_max[min(REACH, n - 1)] - HALF_W
    out = [("exact", l_min, l_max, (on, 0.0, 0.0), "feasible")]
    if n <= 100:                                         # (n = 256 costs the oracle ten seconds a case)
        out.append(("inside", l_min.copy(), l_max.copy(), (on - 1e-12, 0.0, 0.0), "feasible"))
    return out


def _endpin(n):
    """l_min[-1] = 2 with the end pinned at l = 0: feasible, the fixed last stations look at other indices."""
    l_min, l_max = corridor(*open_ranges(n))
    l_min[-1] = 2.0
    return [("outside", l_min, l_max, (0.2, 0.0, 0.0), "feasible")]


def _inspect(n):
    """Infeasible at a glance: the start outside its range; a station whose range is empty."""
    l_min, l_max = corridor(*open_ranges(n))
    out = [("start", l_min, l_max, (9.5, 0.0, 0.0), "infeasible")]
    l_min, l_max = l_min.copy(), l_max.copy()
    i = n // 2
    l_min[max(i - REACH, 0)], l_max[min(i + REACH, n - 1)] = 2.0, 1.0
    out.append(("empty", l_min, l_max, (0.0, 0.0, 0.0), "infeasible"))
    return out


def _spline(n):
    """Every station's own range is non-empty, the set has no C2 solution: a tube 0.02 m wide that climbs (or alternates by) 1 m
    per station over 8 stations.  |dl| <= 0.0034 at each of them, so consecutive 2 m steps need l'' = +1.5 then -1.5 at their
    shared station (l1 - l0 = ds dl0 + ds^2 (l0''/3 + l1''/6), dl1 - dl0 = ds (l0'' + l1'') / 2)."""
    if n not in SPLINE_SIZES:
        return []
    out = []
    for name, centre in (("ramp", lambda k: -3.5 + k), ("stairs", lambda k: 2.0 * (k // 2 % 2) - 1.0 + 0.5 * (k % 2))):
        lb, ub = open_ranges(n)
        first = n // 2 - 4
        for k in range(8):
            lb[first + k], ub[first + k] = centre(k) - 0.01, centre(k) + 0.01
        out.append((name, *corridor(lb, ub), (0.0, 0.0, 0.0), "infeasible"))
    return out


def pinch_station(n):
    return n // 2


def _pinch(n):
    """One station whose corridor is host width + 1e-6 m: the solution passes it at l ~ 0 between bounds 1e-6 m apart.  "rest":
    an open corridor otherwise, the path has long settled on l ~ 0 when it gets there and touches neither bound (an interior point
    that has to end with both slacks below 1e-6).  "gap": right behind an obstacle that holds the path at l <= -1, so that it
    arrives with a slope and rests on a bound of either side."""
    if n < 8:
        return []
    p = pinch_station(n)
    out = []
    for name in ("rest", "gap"):
        lb, ub = open_ranges(n)
        if name == "gap" and n >= 34:
            ub[p - 10:p - 6] = -1.0
        lb[p], ub[p] = -PINCH_GAP / 2.0, PINCH_GAP / 2.0
        if name == "gap" or n >= 34:
            out.append((name, *corridor(lb, ub), (0.35, -0.04, 0.008), "feasible"))
    return out


FAMILIES = {"open": _open, "offset": _offset, "chicane": _chicane, "random": _random, "bound": _bound, "endpin": _endpin,
            "inspect": _inspect, "spline": _spline, "pinch": _pinch}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, every family at every size it has cases for."""
    out = {}
    for n in SIZES:
        for fam, make in FAMILIES.items():
            for suffix, l_min, l_max, start, expect in make(n):
                name = f"{fam}_{suffix}_n{n}"
                assert len(l_min) == len(l_max) == n and name not in out
                out[name] = Case(np.asarray(l_min, dtype=np.float64), np.asarray(l_max, dtype=np.float64),
                                 np.asarray(start, dtype=np.float64), expect, name, fam, n)
    return out


def matrices(c):
    return rp.path_qp_matrices(c.l_min, c.l_max, *c.start_l3)


ORACLE_INFEASIBLE_MAX_N = 68       # the oracle is not asked to give up on a larger infeasible problem (seconds each)


@functools.lru_cache(maxsize=None)
def truth(name):
    """(verdict, x, certificate): "feasible" with the oracle's certified x as (n, 3) l, dl, ddl; "infeasible" (by inspection, or the
    oracle did not end "optimal" on a case meant infeasible); "uncertified" (meant feasible, not certified: no yardstick)."""
    c = cases()[name]
    if infeasible_by_inspection(c):
        return "infeasible", None, None
    assert c.expectation == "feasible" or c.n <= ORACLE_INFEASIBLE_MAX_N
    H, f, G, h, A, b = matrices(c)
    try:
        res = qp_dense.solve_qp(H, f, G, h, A, b)
        status = res.status
    except np.linalg.LinAlgError:              # the dense interior point diverged
        status = "diverged"
    if status != "optimal":
        return ("infeasible" if c.expectation == "infeasible" else "uncertified"), None, None
    cert = qp_dense.kkt_certificate(H, f, G, h, A, b, res.x)
    good = cert["stationarity"] < 1e-7 and cert["ineq_violation"] < 1e-9 and cert["eq_violation"] < 1e-9
    if not good:
        return ("infeasible" if c.expectation == "infeasible" else "uncertified"), None, cert
    return "feasible", np.asarray(res.x, dtype=np.float64).reshape(c.n, 3), cert


def active_rows(c, x, tol=1e-7):
    """How many corner rows of the reference's A are active at x, by form: (l + d1 dl at the upper bound, l - d2 dl at the upper
    bound, l + d1 dl at the lower bound, l - d2 dl at the lower bound), free stations only."""
    lb, ub = station_ranges(c.l_min, c.l_max)
    l, dl = x[1:-1, 0], x[1:-1, 1]
    lb, ub = lb[1:-1], ub[1:-1]
    plus, minus = l + 3.0 * dl, l - 3.0 * dl
    return (int((ub - plus <= tol).sum()), int((ub - minus <= tol).sum()), int((plus - lb <= tol).sum()), int((minus - lb <= tol).sum()))
