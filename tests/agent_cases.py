"""Inputs for the agents' law that the CPU suite (tests/test_agent_host.py: the g++ build of csrc/emp_agent_core.h) and the GPU suite
(tests/test_gpu_agents.py) share: hand-built agents on the rule's thresholds, and ragged random batches with NaN in every slot the
rule must not read.  A batch is a dict of the arrays emp_agent_control takes.  Test tool only."""
from __future__ import annotations

import math
import os

import numpy as np

from tests import agent_port as ap

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agents")
KEYS = ("path", "n_path", "state", "forward", "speed_kmh", "target_speed", "head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat")
STATE_OUT = ("head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat")
NAN = math.nan


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def same_bits(got, want, what=""):
    """Equal bit for bit; two NaNs are equal whatever their payload."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    if got.dtype.kind == "f":
        ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    else:
        ok = got == want
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {np.argwhere(~ok)[0]}: {got[~ok][0]!r} against {want[~ok][0]!r}"


def blank(A, max_path):
    """A agents with nothing set: NaN wherever the rule must not look."""
    return dict(path=np.full((A, max_path, 4), NAN), n_path=np.zeros(A, np.int32), state=np.zeros((A, 6)), forward=np.zeros((A, 2)),
                speed_kmh=np.zeros(A), target_speed=np.zeros(A), head=np.zeros(A, np.int32), past_steer=np.zeros(A),
                lon_err=np.full((A, ap.BUFFER), NAN), n_lon=np.zeros(A, np.int32), lat_err=np.full((A, ap.BUFFER), NAN),
                n_lat=np.zeros(A, np.int32))


def _beyond_one(sign):
    """(c, s, wx, wy) with w parallel (sign > 0) or opposite to the unit-ish forward vector, whose rounded quotient lies beyond
    +-1 before the clip."""
    rng = np.random.default_rng(7)
    while True:
        th, r = float(rng.uniform(0, 6.28)), float(rng.uniform(10, 50))
        c, s = math.cos(th), math.sin(th)
        wx, wy = sign * r * c, sign * r * s
        nn = math.sqrt(wx * wx + wy * wy) * math.sqrt((c * c + s * s) + 0.0)
        d = ((wx * c + wy * s) + 0.0) / nn
        if sign * d > 1.0:
            return c, s, wx, wy


EDGE_MAX_PATH = 8


def edge_cases():
    """(batch, names): one agent per case.  The base agent stands at (0, 0) facing +x at 18 km/h, so min_distance = 3 + 0.5 * 5 =
    5.5 exactly, with waypoints on the x axis 20 m and more ahead."""
    cases = []

    def add(name, pts=((20.0, 0.0), (22.0, 0.0), (24.0, 0.0)), xy=(0.0, 0.0), fw=(1.0, 0.0), kmh=18.0, target=20.0, head=0, past=0.0,
            lon=(), lat=(), n_path=None, n_lon=None, n_lat=None):
        cases.append(dict(name=name, pts=pts, xy=xy, fw=fw, kmh=kmh, target=target, head=head, past=past, lon=lon, lat=lat,
                          n_path=len(pts) if n_path is None else n_path, n_lon=len(lon) if n_lon is None else n_lon,
                          n_lat=len(lat) if n_lat is None else n_lat))

    far = ((30.0, 1.0), (32.0, 1.0))
    # the purge threshold: exactly at md, one ulp on either side
    add("dist == md", ((5.5, 0.0),) + far)
    add("dist one ulp below md", ((math.nextafter(5.5, 0.0), 0.0),) + far)
    add("dist one ulp above md", ((math.nextafter(5.5, 9.0), 0.0),) + far)
    add("three purged in one tick", ((1.0, 0.0), (3.0, 0.0), (5.0, 0.0), (7.0, 0.0)))
    # the last waypoint's 1 m rule
    add("last waypoint at 1 m stays", ((1.0, 0.0),))
    add("last waypoint below 1 m goes: DONE", ((math.nextafter(1.0, 0.0), 0.0),))
    add("last waypoint within md but beyond 1 m stays", ((4.0, 0.0), (5.0, 0.0)))
    add("both purged: DONE", ((4.0, 0.0), (0.5, 0.5)), lon=(1.0, 2.0), lat=(0.1,), past=0.3)
    add("no plan: DONE", (), lon=(1.0,), past=-0.2)
    add("head already at the end: DONE", head=3)
    # nn == 0: the reference's one radian
    add("nn == 0 by a zero forward vector", fw=(0.0, 0.0))
    add("nn == 0 on the waypoint (a NaN speed stops the purge)", ((0.0, 0.0), (2.0, 0.0)), kmh=NAN)
    # cross exactly 0: ahead (dot = 0) and behind (dot = +pi, not negated)
    add("straight ahead")
    add("straight behind", ((-20.0, 0.0), (-22.0, 0.0)))
    add("to the right: negated", ((20.0, -3.0), (22.0, -3.0)))
    add("to the left", ((20.0, 3.0), (22.0, 3.0)))
    for sign, what in ((1.0, "above +1"), (-1.0, "below -1")):
        c, s, wx, wy = _beyond_one(sign)
        add("quotient " + what + " before the clip", ((wx, wy), (2 * wx, 2 * wy)), fw=(c, s), kmh=0.0 if sign > 0 else 18.0,
            xy=(0.0, 0.0))
    # rate limit and max_steer
    add("rate limit binds alone (up)", ((0.0, 20.0), (0.0, 22.0)), past=-0.5)
    add("rate limit binds alone (down)", ((0.0, -20.0), (0.0, -22.0)), past=0.5)
    add("max_steer binds alone", ((0.0, 20.0), (0.0, 22.0)), past=0.95)
    add("-max_steer binds alone", ((0.0, -20.0), (0.0, -22.0)), past=-0.95)
    add("both bind", ((0.0, 20.0), (0.0, 22.0)), past=0.75)
    add("both bind (negative)", ((0.0, -20.0), (0.0, -22.0)), past=-0.75)
    add("neither binds", ((20.0, 0.2), (22.0, 0.2)), past=0.0)
    # throttle and brake limits
    add("throttle limited", target=40.0)
    add("throttle unlimited", target=18.5)
    add("brake limited", target=5.0)
    add("brake unlimited", target=17.9)
    add("acc == 0 takes the throttle branch", target=18.0, lon=(), kmh=18.0)
    # deques of 0, 1, 9 and 10 entries
    ramp = tuple(0.01 * (i + 1) * (-1) ** i for i in range(10))
    for n in (0, 1, 9, 10):
        add(f"deques of {n}", ((20.0, 1.0), (22.0, 1.0)), lon=tuple(0.3 + v for v in ramp[:n]), lat=ramp[:n])
    add("deques of 10 and 2", lon=ramp, lat=ramp[:2])
    add("-0.0 entries: the sum starts from +0", target=18.0, lon=(-0.0,), lat=(-0.0,))
    # NaN in each input
    add("NaN x", xy=(NAN, 0.0))
    add("NaN y", xy=(0.0, NAN))
    add("NaN c", fw=(NAN, 0.0))
    add("NaN s", fw=(1.0, NAN))
    add("NaN speed", kmh=NAN)
    add("NaN target", target=NAN)
    add("NaN past_steer", past=NAN)
    add("NaN waypoint x", ((NAN, 0.0), (22.0, 0.0)))
    add("NaN waypoint y behind a purged one", ((1.0, 0.0), (8.0, NAN)))
    add("NaN in the longitudinal deque", lon=(0.1, NAN, 0.2))
    add("NaN in the lateral deque", lat=(0.1, NAN))
    add("infinite pose", xy=(math.inf, 0.0))
    add("infinite waypoint", ((math.inf, 0.0), (22.0, 0.0)))
    # counts out of range are clamped
    add("n_lon = -3, n_lat = 99", lon=ramp, lat=ramp, n_lon=-3, n_lat=99)
    add("n_lon = 99, n_lat = -1", lon=ramp, lat=ramp, n_lon=99, n_lat=-1)
    add("n_path beyond the row", tuple((20.0 + 2 * i, 0.0) for i in range(EDGE_MAX_PATH)), n_path=EDGE_MAX_PATH + 100)
    add("n_path negative: DONE", n_path=-5)
    add("head negative", head=-7)
    add("head beyond n_path: DONE", head=2 ** 30)

    A = len(cases)
    b = blank(A, EDGE_MAX_PATH)
    for a, c in enumerate(cases):
        for i, (px, py) in enumerate(c["pts"]):
            b["path"][a, i, :2] = (px, py)
        b["n_path"][a] = c["n_path"]
        b["state"][a, :2] = c["xy"]
        b["state"][a, 2:] = NAN                       # only x and y are read
        b["forward"][a] = c["fw"]
        b["speed_kmh"][a], b["target_speed"][a], b["head"][a], b["past_steer"][a] = c["kmh"], c["target"], c["head"], c["past"]
        b["lon_err"][a, :len(c["lon"])] = c["lon"]
        b["lat_err"][a, :len(c["lat"])] = c["lat"]
        b["n_lon"][a], b["n_lat"][a] = c["n_lon"], c["n_lat"]
    return b, [c["name"] for c in cases]


def random_batch(A, max_path, seed):
    """A agents at random poses near ragged paths (n_path 0, 1 and 2 among them, and counts beyond the row), mid-run: heads,
    deques of every length, past steers.  Path rows at and past n_path, deque entries at and past the count and the state's
    unread entries hold NaN."""
    rng = np.random.default_rng(seed)
    b = blank(A, max_path)
    for a in range(A):
        n = int(rng.integers(0, max_path + 1)) if a % 7 else (0, 1, 2, max_path, max_path + 3)[(a // 7) % 5]
        m = min(n, max_path)
        th0 = rng.uniform(-3.1, 3.1)
        pts = np.cumsum(2.0 * np.c_[np.cos(th0 + np.linspace(0, 1.0, max(m, 1))), np.sin(th0 + np.linspace(0, 1.0, max(m, 1)))], 0)[:m]
        b["path"][a, :m, :2] = pts + rng.uniform(-50, 50, 2)
        b["n_path"][a] = n
        head = int(rng.integers(0, m + 1)) if m else 0
        at = b["path"][a, min(head, m - 1), :2] if m else np.zeros(2)
        b["state"][a, :2] = at + rng.uniform(-6, 6, 2) * (rng.random() < 0.8)
        b["state"][a, 2:] = NAN
        th = th0 + rng.uniform(-1.5, 1.5)
        b["forward"][a] = (math.cos(th), math.sin(th))
        b["speed_kmh"][a] = rng.uniform(0, 40)
        b["target_speed"][a] = b["speed_kmh"][a] + rng.choice([-8.0, -0.4, 0.3, 6.0])
        b["head"][a] = head if a % 11 else head - 2
        b["past_steer"][a] = rng.uniform(-0.8, 0.8)
        for k, nk in (("lon_err", "n_lon"), ("lat_err", "n_lat")):
            cnt = int(rng.integers(0, ap.BUFFER + 1))
            b[k][a, :cnt] = rng.uniform(-0.5, 0.5, cnt)
            b[nk][a] = cnt
        if a % 3 == 0 and head < m:
            # a steer that neither limit binds: 15 m from the head waypoint (nothing is purged), heading within 0.03 rad of it, an
            # empty lateral deque (cs = lat_K_P * dot) and a past steer within 0.05 of that
            away, delta = rng.uniform(-3.1, 3.1), rng.uniform(-0.03, 0.03)
            b["state"][a, :2] = b["path"][a, head, :2] - 15.0 * np.array([math.cos(away), math.sin(away)])
            b["forward"][a] = (math.cos(away + delta), math.sin(away + delta))
            b["head"][a], b["n_lat"][a] = head, 0
            b["past_steer"][a] = -1.95 * delta + rng.uniform(-0.05, 0.05)
    return b


def bound_mask(prm, b, want):
    """Per agent: True where the steer is decided to the bit whatever acos' last bits were: DONE, a NaN, or the rate limit or
    max_steer binds - the port's steer is then past_steer +- 0.1 or +-max_steer."""
    steer, past = want["control"][:, 1], b["past_steer"]
    with np.errstate(invalid="ignore"):
        return (want["status"] != 0) | np.isnan(steer) | (steer == past + 0.1) | (steer == past - 0.1) | (np.abs(steer) == prm["max_steer"])


def port_control(prm, b):
    return ap.control_batch(prm, *[b[k] for k in KEYS])


def corner_xy():
    """A short corner: 12 points straight, a 12 m-radius right angle (9 points), 8 points straight, 2 m apart: 29 points."""
    import sys
    if os.path.dirname(GOLDEN) not in sys.path:
        sys.path.insert(0, os.path.dirname(GOLDEN))
    import make_golden_agents as mk             # the scenario half: NumPy only
    return mk.polyline([("s", 11), ("a", 12.0, math.pi / 2), ("s", 8)])


def corner_fleet(A, ragged=True):
    """A agents at the start of rotated and translated copies of corner_xy, a little beside it and off its heading, at 2-5 m/s with
    targets of 15-30 km/h: a batch with fresh agent state (`state` complete, forward / speed_kmh unset).  ragged: every fifth agent
    has no plan (DONE from tick 0, between live ones), some have one or two waypoints, one claims more than the row holds."""
    xy0 = corner_xy()
    M = len(xy0)
    b = blank(A, M)
    b["lon_err"][:], b["lat_err"][:] = 0.0, 0.0
    for a in range(A):
        rot = 0.37 * a
        c, s = math.cos(rot), math.sin(rot)
        shift = np.array([(13 * a) % 101 - 50.0, (7 * a) % 53 - 26.0])
        n = M
        if ragged:
            n = 0 if a % 5 == 2 else (1 if a % 17 == 4 else (2 if a % 17 == 9 else (M + 7 if a % 17 == 13 else M)))
        b["path"][a, :min(n, M), :2] = (xy0 @ np.array([[c, s], [-s, c]]) + shift)[:min(n, M)]
        b["n_path"][a] = n
        side = 0.4 * ((a % 3) - 1)
        b["state"][a] = (shift[0] - side * s, shift[1] + side * c, rot + 0.05 * ((a % 5) - 2), 0.0, 0.0, 2.0 + (a % 4))
        b["target_speed"][a] = 15.0 + 5.0 * (a % 4)
    return b
