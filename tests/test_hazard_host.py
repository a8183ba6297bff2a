"""CPU suite of the hazard rule (red lights and pedestrians in front of the car-following law): the Python port
(tests/hazard_port.py) against what the reference's BehaviorAgent did, tick by tick, on the recorded closed loops of
tests/golden/hazards/; the g++ build of csrc/emp_hazard_core.h and of a CPU copy of both kernels
(tests/host_check/hazard_check.cpp) bit for bit against the port on the fixtures, on hand-built threshold cases and on the seeded
ragged batches the GPU suite uses; that build as a sanitized program of its own; the launch plan; the ctypes layouts and
prototypes; the coverage of the seeded batches; and - where the reference tree is present - every fixture regenerated bit for bit."""
from __future__ import annotations

import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from tests import agent_port as ap
from tests import behavior_cases as bc
from tests import behavior_port as bp
from tests import hazard_cases as hc
from tests import hazard_port as hp
from tests.test_behavior_host import NO_SINCOS, assert_same as assert_same_behavior, c_behavior, c_params, c_vehicle, io_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "host_check", "hazard_check.cpp")
NAMES = hc.NAMES
# The steer of the port against the reference's, by the rule of tests/test_agent_host.py (see tests/test_behavior_host.py): the worst
# difference over the hazard fixtures is 5.66e-12; the bar is four times that, and above 1e-6 rad it would be another law.
STEER_MEASURED = 5.66e-12
STEER_BAR = 4 * STEER_MEASURED
STEER_CAP = 1e-6


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hazard_check") / "libhazardcheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall"] + NO_SINCOS + [SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    p, i, q = C.c_void_p, C.c_int, C.c_longlong
    lib.hc_layout.restype = None
    lib.hc_layout.argtypes = [p, p]
    lib.hc_plan.restype = C.c_char_p
    lib.hc_plan.argtypes = [i, i, i, i, i, i, i, i, q, p, p]
    lib.hc_behave.restype = None
    lib.hc_behave.argtypes = [C.POINTER(L.AgentParams), C.POINTER(L.BehaviorParams), C.POINTER(L.HazardParams), i, i, i, i, i, i, q,
                              C.POINTER(L.BehaviorIO), C.POINTER(L.HazardIO)]
    lib.hc_rollout.restype = None
    lib.hc_rollout.argtypes = [C.POINTER(L.AgentParams), C.POINTER(L.BehaviorParams), C.POINTER(L.HazardParams), C.POINTER(L.VehicleParams),
                               i, i, i, i, i, i, i, i, q, C.POINTER(L.BehaviorIO), C.POINTER(L.HazardIO)]
    return lib


def c_hazard(hpp):
    return L.HazardParams(*[float(hpp[k]) for k in hp.FIELDS], 0)


def hazard_io_of(ins, outs):
    """emp_hazard_io over dicts of arrays (an empty array: NULL)."""
    h = L.HazardIO()
    keep = []
    for k, v in ins.items():
        v = np.ascontiguousarray(v)
        keep.append(v)
        setattr(h, k, v.ctypes.data if v.size else None)
    for k, v in outs.items():
        assert v.flags.c_contiguous
        setattr(h, "last_light_out" if k == "last_light" else k, v.ctypes.data)
    h.reserved = 0
    return h, keep


def host_behave(lib, prm, prb, hpp, b, tick0=0, aliased=False):
    """hc_behave on a batch: a dict of its outputs; padding slots keep the 7s they start with (aliased: the inputs' values)."""
    W, N, M = b["lane"].shape
    K, ML, MW = b["other"].shape[1], b["light"].shape[1], b["walker"].shape[1]
    ins = {k: np.ascontiguousarray(b[k]).copy() for k in bc.IN_KEYS}
    hin = {k: np.ascontiguousarray(b[k]).copy() for k in hc.HAZARD_IN}
    o = {k: (ins[k] if aliased else np.full_like(ins[k], 7)) for k in bc.STATE_OUT}
    o.update(status=np.full((W, N), 7, np.int32), control=np.full((W, N, 3), 7.0), mode=np.full((W, N), 7, np.int32),
             blocker=np.full((W, N), 7, np.int32), distance=np.full((W, N), 7.0), ttc=np.full((W, N), 7.0),
             target_speed_out=np.full((W, N), 7.0), lat_error=np.full((W, N), 7.0), lon_command=np.full((W, N), 7.0))
    ho = dict(last_light=hin["last_light"] if aliased else np.full((W, N), 7, np.int32), cause=np.full((W, N), 7, np.int32),
              light_hit=np.full((W, N), 7, np.int32), walker_hit=np.full((W, N), 7, np.int32), walker_distance=np.full((W, N), 7.0))
    io, keep = io_of(ins, o)
    h, keep2 = hazard_io_of(hin, ho)
    lib.hc_behave(C.byref(c_params(prm)), C.byref(c_behavior(prb)), C.byref(c_hazard(hpp)), W, N, M, K, ML, MW, tick0, C.byref(io), C.byref(h))
    return dict(o, **ho)


def sevens(b, aliased=False):
    """What the padding slots of host_behave's outputs hold."""
    f = {k: (b[k] if aliased else np.full_like(b[k], 7)) for k in bc.STATE_OUT + ("last_light",)}
    W, N = b["n_path"].shape
    for k in bc.TICK_OUT + hc.HAZARD_OUT[1:]:
        f[k] = np.full((W, N, 3) if k == "control" else (W, N), 7, np.int32 if k in hc.INT_OUT else np.float64)
    return f


def assert_same(got, want, what, live=None):
    assert_same_behavior(got, want, what, live)
    for k in hc.HAZARD_OUT:
        hc.same_bits(got[k], want[k], f"{what}: {k}")


# ---- the port against the reference ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replays():
    return {n: hc.replay(n) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_port_equals_the_recorded_reference_tick_by_tick(replays, name):
    f, r = replays[name]
    np.testing.assert_array_equal(r["queue"], f["queue"], err_msg=f"{name}: queue lengths")
    np.testing.assert_array_equal(r["target"], f["target"], err_msg=f"{name}: _target_speed after the tick")
    np.testing.assert_array_equal(r["mode"], f["mode"], err_msg=f"{name}: modes")
    np.testing.assert_array_equal(r["cause"], f["cause"], err_msg=f"{name}: causes")
    np.testing.assert_array_equal(r["last_light"], f["last_light"], err_msg=f"{name}: the reference's _last_traffic_light")
    em = r["mode"] == bp.EMERGENCY
    np.testing.assert_array_equal(em, f["emergency"] == 1, err_msg=f"{name}: the ticks on which the reference made an emergency stop")
    np.testing.assert_array_equal(em, r["cause"] != 0)
    hc.same_bits(r["control"][em], f["control"][em], f"{name}: emergency ticks")
    assert not em.any() or (f["control"][em] == (0.0, 0.0, 0.5)).all()
    d = np.abs(r["control"] - f["control"]).reshape(-1, 3).max(0)
    print(f"{name}: worst throttle / steer / brake difference {d[0]:.3g} / {d[1]:.3g} / {d[2]:.3g}")
    assert d[0] <= 1e-12 and d[2] <= 1e-12, f"{name}: throttle {d[0]}, brake {d[2]}"
    assert STEER_BAR <= STEER_CAP and d[1] <= STEER_BAR, f"{name}: steer differs by {d[1]}"


def test_the_steer_bar_is_the_measured_one(replays):
    worst = max(np.abs(r["control"][..., 1] - f["control"][..., 1]).max() for f, r in replays.values())
    print(f"worst steer difference over the hazard fixtures: {worst:.4g}")
    assert STEER_MEASURED / 2 <= worst <= STEER_MEASURED, "the measured figure in this file and in DESIGN.md 3.13 is stale"


def test_fixtures_cover_what_they_are_for():
    fx = {n: hc.fixture(n) for n in NAMES}
    for n, f in fx.items():
        assert f["margin"].min() >= hc.mkh.MIN_MARGIN, n
        np.testing.assert_array_equal(f["cause_ticks"], [[(f["cause"][:, v] == m).sum() for m in (1, 2, 3)] for v in range(f["cause"].shape[1])])
        assert ((f["cause"] != 0) == (f["mode"] == bp.EMERGENCY)).all(), n
    speed = lambda f, v=0: f["seen"][:, v, 4]
    for n in ("red_light", "sticky"):                            # drive, stop, go on green
        f = fx[n]
        red_to = int(f["light_cycle"][0, 2])
        held = f["cause"][:, 0] == hp.HZ_LIGHT
        assert held.any() and not held[red_to:].any() and held[red_to - 1] and speed(f)[red_to - 1] < 1e-6 and speed(f)[-1] > 5.0, n
        assert (f["last_light"][held, 0] == 0).all() and (f["last_light"][~held, 0] == -1).all()
    # red_light stops short of the trigger waypoint: the scan alone would hold it; sticky rolls past it: only last_light holds it
    ahead = lambda f: ((f["light"][0, :2] - f["seen"][:, 0, :2]) * f["seen"][:, 0, 2:4]).sum(1)      # the waypoint along the heading
    assert ahead(fx["red_light"])[fx["red_light"]["cause"][:, 0] == 1].min() > 0.5
    f = fx["sticky"]
    assert (ahead(f)[(f["sticky"][:, 0] == 1)] < 0.0).sum() > 100
    for n in ("green_light", "opposite_light", "other_key_light"):
        f = fx[n]
        assert f["cause_ticks"].sum() == 0 and (f["light_hit"] < 0).all() and (f["last_light"] == -1).all(), n
        d = np.sqrt(((f["light"][0, :2] - f["seen"][:, 0, :2]) ** 2).sum(1))
        assert d.min() < 4.0, f"{n}: the vehicle passes within the light's 5 m"
    assert fx["opposite_light"]["light_lane"][0] == 1 and fx["other_key_light"]["light_lane"][0] == 2
    f = fx["green_light"]                                        # the light is red again once the vehicle is through
    assert hp.is_red(f["light_cycle"][0], 0) and hp.is_red(f["light_cycle"][0], 310) and len(f["mode"]) > 310
    f = fx["walker_crossing"]                                    # detected and ignored, then the emergency, then on
    first = int(np.argmax(f["cause"][:, 0] == hp.HZ_WALKER))
    assert f["ignored"][:first, 0].sum() >= 3 and f["cause_ticks"][0].tolist()[1] > 10 and speed(f)[-1] > 5.0
    assert (f["walker_distance"][:first, 0][f["ignored"][:first, 0] == 1] >= 5.0).all()
    f = fx["walker_outside_radius"]                              # inside the cone and th, beyond 10 m: unseen until the radius
    lost = f["filtered"][:, 0] == 1
    assert lost.sum() >= 3 and (f["walker_hit"][lost, 0] == -1).all() and (f["walker_hit"][int(np.argmax(lost)) + lost.sum():, 0] >= 0).any()
    f = fx["walker_and_leader"]                                  # an ignored walker, then car-following with its two agent ticks
    both = (f["ignored"][:, 0] == 1) & np.isin(f["mode"][:, 0], (bp.SLOW, bp.FOLLOW, bp.CLEAR))
    assert both.sum() >= 5 and f["cause_ticks"][:, 1].sum() == 0
    f = fx["queue_at_light"]                                     # slot 1 leads and is held by the light, slot 0 by the vehicle rule
    assert f["cause_ticks"][1, 0] > 100 and f["cause_ticks"][0, 2] > 100 and f["cause_ticks"][0, 0] == 0
    assert speed(f, 0)[-1] > 1.5 and speed(f, 1)[-1] > 1.5
    sizes = {n: os.path.getsize(os.path.join(GOLDEN, "hazards", n + ".npz")) for n in NAMES}
    biggest = max(os.path.getsize(os.path.join(GOLDEN, "behavior", n + ".npz")) for n in bc.mkb.NAMES)
    assert max(sizes.values()) <= biggest and sum(sizes.values()) < 900 * 1024, sizes


# ---- the core, compiled with g++ ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_core_equals_the_port_on_the_recorded_inputs(lib, name):
    """The fixture as one world, every third tick a call from the port's agent state and sticky light: every output to the bit."""
    f, b0 = hc.fixture_world(name)
    T, V = f["queue"].shape
    prm, prb, hpp = ap.params(), bp.params(), hp.params()
    agents = [ap.Agent() for _ in range(V)]
    last = np.full(V, -1, np.int32)
    for t in range(T):
        b = {k: v.copy() for k, v in b0.items()}
        b["state"][0, :, :2], b["forward"][0], b["speed_kmh"][0] = f["seen"][t, :, :2], f["seen"][t, :, 2:4], f["seen"][t, :, 4]
        packed = ap.pack(agents, np.zeros((V, ap.BUFFER)), np.zeros((V, ap.BUFFER)))
        for k in bc.STATE_OUT:
            b[k][0] = packed[k]
        b["last_light"][0] = last
        want = hc.port_behave(prm, prb, hpp, b, t, fill=sevens(b))
        if t % 3 == 0:
            assert_same(host_behave(lib, prm, prb, hpp, b, t), want, f"{name} tick {t}")
        np.testing.assert_array_equal(want["cause"][0], f["cause"][t], err_msg=f"{name} tick {t}")
        agents = ap.agents_of(*[want[k][0] for k in bc.STATE_OUT])
        last = want["last_light"][0]


def test_core_on_the_threshold_cases(lib):
    b, names, tick0 = hc.edge_cases()
    prm, prb, hpp = ap.params(), bp.params(), hp.params()
    w = dict(zip(names, range(len(names))))
    assert len(w) == len(names)
    res = {}
    for t0 in sorted(set(tick0)):
        want = hc.port_behave(prm, prb, hpp, b, t0, fill=sevens(b))
        assert_same(host_behave(lib, prm, prb, hpp, b, t0), want, f"tick0 {t0}")
        assert_same(host_behave(lib, prm, prb, hpp, b, t0, aliased=True), hc.port_behave(prm, prb, hpp, b, t0, fill=sevens(b, True)),
                    f"tick0 {t0} aliased")
        res[t0] = want
    # what each case is for did happen, at its own tick
    at = lambda name, k: res[tick0[w[name]]][k][w[name], 0]
    cause, lhit, whit, last = (lambda n: at(n, "cause")), (lambda n: at(n, "light_hit")), (lambda n: at(n, "walker_hit")), (lambda n: at(n, "last_light"))
    L_, W_, V_ = hp.HZ_LIGHT, hp.HZ_WALKER, hp.HZ_VEHICLE
    assert cause("light norm == th") == L_ and cause("light norm one ulp above th") == 0 and cause("light norm one ulp below th") == L_
    assert cause("light norm == 0.001") == 0 and cause("light norm one ulp below 0.001") == L_ and cause("light norm one ulp above 0.001 behind") == 0
    assert cause("light angle exactly 0: not seen") == 0 and cause("light angle just above 0") == L_
    assert cause("light angle exactly 90: not seen") == 0 and cause("light angle near 90 inside") == L_ and cause("light angle near 90 outside") == 0
    assert cause("light angle 60.000001: seen") == L_
    assert cause("light dot == 0: not passed over") == L_ and cause("light dot just below 0") == 0 and cause("light dot -0.0: not passed over") == L_
    assert cause("light NaN direction: not passed over") == L_
    assert cause("light on another key") == 0 and cause("light keyed -1") == 0 and cause("light on key_next only") == 0
    assert cause("phase at red_from") == L_ and cause("phase below red_from") == 0 and cause("phase at red_to - 1") == L_ and cause("phase at red_to") == 0
    assert cause("phase wraps: k mod period") == L_ and cause("phase wraps to green") == 0
    assert cause("period 0: never red") == 0 and cause("period below 0: never red") == 0 and cause("red_to beyond the period") == L_
    assert lhit("two lights hit: the first wins") == 0 and lhit("the first light is green: the second is taken") == 1
    for n in ("two lights hit: the first wins", "the first light is green: the second is taken"):
        assert last(n) == lhit(n)
    n = "sticky: held by a red light far behind"
    assert cause(n) == L_ and lhit(n) == 0 and last(n) == 0
    n = "sticky: light 1 holds though light 0 would hit"
    assert lhit(n) == 1 and last(n) == 1
    n = "sticky light went green: the scan finds the other"
    assert lhit(n) == 1 and last(n) == 1
    n = "sticky light went green: nothing else"
    assert cause(n) == 0 and last(n) == -1
    for n in ("last_light == n_light: counts as -1", "last_light far out of range", "last_light -2", "last_light INT_MIN",
              "last_light points past n_light at a poisoned row"):
        assert cause(n) == 0 and last(n) == -1 and at(n, "mode") == bp.NORMAL, n
    n = "DONE: lights and last_light are left alone"
    assert at(n, "mode") == bp.DONE and last(n) == 9999 and cause(n) == 0 and lhit(n) == -1
    assert at("no plan: DONE", "mode") == bp.DONE and last("no plan: DONE") == 0
    assert cause("n_path == 1: ve is (0, 0), the dot is 0") == L_ and cause("head 0: the chord is the first") == L_
    assert cause("head n_path - 1: the chord is the last") == L_
    assert whit("filter == 10: rejected") == -1 and whit("filter just below 10") == 0 and whit("filter just above 10") == -1
    assert whit("walker inside cone and th, outside the radius") == -1
    assert whit("walker norm == th") == 0 and whit("walker norm just above th") == -1 and whit("walker norm just below th") == 0
    assert cause("walker norm one ulp below 0.001") == W_ and whit("walker angle exactly 0: not seen") == -1
    assert whit("walker angle near 60 inside") == 0 and whit("walker angle near 60 outside") == -1 and whit("walker behind") == -1
    n = "walker d == braking_distance: ignored"
    assert whit(n) == 0 and cause(n) == 0 and at(n, "walker_distance") == 5.0 and at(n, "mode") == bp.NORMAL
    assert cause("walker d one ulp below") == W_ and cause("walker d one ulp above") == 0
    n = "two walkers hit: the first wins though the second is nearer"
    assert whit(n) == 0 and cause(n) == 0
    assert whit("the first walker is keyed -1") == 1 and cause("the first walker is keyed -1") == W_ and whit("the first walker is on another lane") == 1
    assert whit("walker on key_next") == 0
    n = "walker walks into range at tick0"
    assert cause(n) == W_ and res[0]["walker_hit"][w[n], 0] == -1
    n = "an ignored walker, then the vehicle rule"
    assert whit(n) == 0 and cause(n) == 0 and at(n, "mode") in (bp.SLOW, bp.FOLLOW, bp.CLEAR) and at(n, "n_lon") == 2
    n = "an ignored walker, then the vehicle emergency"
    assert whit(n) == 0 and cause(n) == V_ and at(n, "blocker") == 0
    n = "a red light comes before a walker"
    assert cause(n) == L_ and whit(n) == -1 and np.isinf(at(n, "walker_distance"))
    assert cause("alone") == 0 and at("alone", "mode") == bp.NORMAL
    # an emergency tick leaves the agent state alone, whatever its cause
    for n in ("light norm == th", "walker d one ulp below"):
        assert tuple(res[0]["control"][w[n], 0]) == (0.0, 0.0, 0.5) and at(n, "n_lon") == 0 and at(n, "head") == 1 and at(n, "target_speed_out") == 60.0
        assert at(n, "blocker") == -1 and np.isinf(at(n, "distance")) and np.isinf(at(n, "ttc"))


@pytest.mark.parametrize("k", range(hc.BATCHES))
def test_core_on_the_seeded_batches(lib, k):
    b, t0 = hc.gpu_batch(k)
    prm, prb, hpp = ap.params(), bp.params(), hp.params()
    live = hc.live_mask(b)
    assert_same(host_behave(lib, prm, prb, hpp, b, t0), hc.port_behave(prm, prb, hpp, b, t0, fill=sevens(b)), f"batch {k}", live)
    assert_same(host_behave(lib, prm, prb, hpp, b, t0, aliased=True), hc.port_behave(prm, prb, hpp, b, t0, fill=sevens(b, True)),
                f"batch {k} aliased")


def test_the_seeded_batches_cover_the_rule():
    """Every (mode, cause) pair that can occur, and the sticky, ignored-walker and filter-rejects branches, at least 20 times each
    over the twelve batches, with at most 1 % of the rows left out for a margin below 1e-9."""
    prm, prb, hpp = ap.params(), bp.params(), hp.params()
    pairs, branch, rows, low = collections.Counter(), collections.Counter(), 0, 0
    for k in range(hc.BATCHES):
        b, t0 = hc.gpu_batch(k)
        assert tuple(np.clip(b["n_world"], 0, 64)) == hc.SIZES and tuple(np.clip(b["n_light"], 0, 64)) == hc.LIGHTS
        assert tuple(np.clip(b["n_walker"], 0, 64)) == hc.WALKERS and (b["n_other"] > 0).any()
        o = hc.port_behave(prm, prb, hpp, b, t0)
        live = hc.live_mask(b)
        ok = live & (o["margin"] >= hc.MIN_MARGIN)
        rows, low = rows + int(live.sum()), low + int((live & ~ok).sum())
        pairs.update(zip(o["mode"][ok].tolist(), o["cause"][ok].tolist()))
        for n in ("sticky", "ignored", "filter"):
            branch[n] += int(o[n][ok].sum())
        branch["scan"] += int(((o["light_hit"] >= 0) & ~o["sticky"] & ok).sum())
    print(sorted(pairs.items()), dict(branch), rows, low)
    can = {(bp.NORMAL, 0), (bp.SLOW, 0), (bp.FOLLOW, 0), (bp.CLEAR, 0), (bp.DONE, 0), (bp.EMERGENCY, hp.HZ_LIGHT), (bp.EMERGENCY, hp.HZ_WALKER),
           (bp.EMERGENCY, hp.HZ_VEHICLE)}
    assert set(pairs) == can and min(pairs.values()) >= 20, pairs
    assert min(branch[n] for n in ("sticky", "ignored", "filter", "scan")) >= 20, branch
    assert low <= rows // 100, (low, rows)


def host_rollout(lib, prm, prb, hpp, vp, b, T, every, tick0=0):
    W, N, M = b["lane"].shape
    K, ML, MW = b["other"].shape[1], b["light"].shape[1], b["walker"].shape[1]
    n_log = (T + every - 1) // every
    ins = {k: np.ascontiguousarray(b[k]).copy() for k in bc.IN_KEYS if k not in ("forward", "speed_kmh")}
    hin = {k: np.ascontiguousarray(b[k]).copy() for k in hc.HAZARD_IN}
    o = {k: np.full_like(ins[k], 7) for k in bc.STATE_OUT}
    o.update(state=np.full((W, N, 6), 7.0), status=np.full((W, N), 7, np.int32), done_tick=np.full((W, N), 7, np.int32),
             mode_ticks=np.full((W, N, 5), 7, np.int32), min_gap=np.full((W, N), 7.0), actors_out=np.full((W, N, 4), 7.0),
             log_state=np.full((n_log, W, N, 6), 7.0), log_control=np.full((n_log, W, N, 3), 7.0), log_head=np.full((n_log, W, N), 7, np.int32),
             log_mode=np.full((n_log, W, N), 7, np.int32), log_target=np.full((n_log, W, N), 7.0))
    ho = dict(last_light=np.full((W, N), 7, np.int32), cause_ticks=np.full((W, N, 3), 7, np.int32), min_walker_gap=np.full((W, N), 7.0),
              log_cause=np.full((n_log, W, N), 7, np.int32))
    io, keep = io_of(ins, o)
    h, keep2 = hazard_io_of(hin, ho)
    lib.hc_rollout(C.byref(c_params(prm)), C.byref(c_behavior(prb)), C.byref(c_hazard(hpp)), C.byref(c_vehicle(vp)), W, N, M, K, ML, MW, T, every,
                   tick0, C.byref(io), C.byref(h))
    return dict(o, **ho)


@pytest.mark.parametrize("name", ("sticky", "walker_crossing", "walker_and_leader", "queue_at_light"))
def test_core_rollout_equals_the_port_loop_and_the_recording(lib, name):
    """The kernel's loop on the CPU against the port's on a fixture's scenario - bit for bit, since libm is the same - and the
    recording itself: the same closed loop."""
    f, b = hc.fixture_world(name)
    T, V = f["queue"].shape
    every = 3
    prm, prb, hpp, vp = ap.params(), bp.params(), hp.params(), ap.vehicle_params()
    got = host_rollout(lib, prm, prb, hpp, vp, b, T, every)
    agents, last = [ap.Agent() for _ in range(V)], [-1] * V
    want = hp.rollout(prm, prb, hpp, vp, hc.world_of(b, 0, V), agents, last, T)
    hc.same_bits(got["state"][0], want["end"], f"{name}: final state")
    hc.same_bits(got["log_state"][:, 0], want["state"][::every], f"{name}: log_state")
    hc.same_bits(got["log_control"][:, 0], want["control"][::every], f"{name}: log_control")
    hc.same_bits(got["log_target"][:, 0], want["target"][::every], f"{name}: log_target")
    for k in ("head", "mode", "cause"):
        np.testing.assert_array_equal(got["log_" + k][:, 0], want[k][::every])
    np.testing.assert_array_equal(got["last_light"][0], last)
    np.testing.assert_array_equal(got["mode_ticks"][0], [[(want["mode"][:, v] == m).sum() for m in range(5)] for v in range(V)])
    np.testing.assert_array_equal(got["cause_ticks"][0], [[(want["cause"][:, v] == m).sum() for m in (1, 2, 3)] for v in range(V)])
    np.testing.assert_array_equal(got["cause_ticks"][0], f["cause_ticks"])
    hc.same_bits(got["min_walker_gap"][0], want["walker_distance"].min(0), f"{name}: min_walker_gap")
    np.testing.assert_array_equal(want["mode"], f["mode"], err_msg=f"{name}: the port's closed loop leaves the recorded modes")
    np.testing.assert_array_equal(want["cause"], f["cause"])
    assert np.abs(want["state"][:, :, :2] - f["seen"][:, :, :2]).max() < 1e-6, f"{name}: the port's closed loop leaves the recorded one"


def test_hazard_check_as_a_program_of_its_own(tmp_path):
    """-DHAZARD_CHECK_MAIN: the self-checking program a sanitizer build runs (here: address and undefined behaviour, on the CPU)."""
    exe = str(tmp_path / "hazard_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DHAZARD_CHECK_MAIN"] + NO_SINCOS + [SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "hazard_check: 0 bad, 0 wrong" in run.stdout, run.stdout + run.stderr[-2000:]


# ---- the launch plan ------------------------------------------------------------------------------------------------------------------
def plan(lib, W, N, K, ML, MW, M, T, every, tick0=0):
    out, offs = np.zeros(6, np.int64), np.zeros(6, np.int64)
    err = lib.hc_plan(W, N, K, ML, MW, M, T, every, tick0, out.ctypes.data, offs.ctypes.data)
    return out.tolist(), offs.tolist(), (err.decode() if err else None)


def test_launch_plan(lib):
    base = 2 * 64 * 11 + 2 * 3 * 64 + 64 + 64 + 5 * 64 + 32                           # the behaviour kernels' layout, in doubles
    offs = [base, base + 4 * 64, base + 4 * 64 + 32, base + 4 * 64 + 32 + 96, base + 4 * 64 + 32 + 96 + 5 * 64, base + 4 * 64 + 32 + 96 + 5 * 64 + 32]
    lds = 8 * offs[-1]
    assert base == 2272 and lds == 24064
    assert plan(lib, 5, 64, 3, 64, 64, 40, 0, 1) == ([5, 64, lds, 160 * 1024 // lds, 0, 0], offs, None)
    assert plan(lib, 512, 8, 0, 4, 8, 40, 100, 7)[0] == [512, 64, lds, 6, 15, 0]
    assert plan(lib, 3, 8, 0, 0, 0, 40, 100, 1)[0] == [3, 64, lds, 6, 100, 0]
    assert plan(lib, 0, 64, 0, 4, 8, 40, 10, 1)[0] == [0, 0, 0, 0, 0, 0]               # an empty batch launches nothing
    for args, word in (((1, 1, 0, -1, 0, 1, 1, 1), "max_light"), ((1, 1, 0, 65, 0, 1, 1, 1), "max_light"), ((1, 1, 0, 0, -1, 1, 1, 1), "max_walker"),
                       ((1, 1, 0, 0, 65, 1, 1, 1), "max_walker"), ((0, 1, 0, 65, 0, 1, 1, 1), "max_light"),
                       # everything plan_behavior refuses
                       ((1, 0, 0, 1, 1, 1, 1, 1), "max_world"), ((1, 65, 0, 1, 1, 1, 1, 1), "max_world"), ((1, 1, -1, 1, 1, 1, 1, 1), "max_other"),
                       ((1, 1, 65, 1, 1, 1, 1, 1), "max_other"), ((1, 1, 0, 1, 1, 0, 1, 1), "max_path"), ((-1, 1, 0, 1, 1, 1, 1, 1), "W < 0"),
                       ((1, 1, 0, 1, 1, 1, 65537, 1), "T outside"), ((1, 1, 0, 1, 1, 1, 5, 0), "log_every"), ((1, 1, 0, 1, 1, 1, 5, 1, -1), "tick0"),
                       ((1, 1, 0, 1, 1, 1, 5, 1, 2 ** 31 - 5), "tick0")):
        got, _, err = plan(lib, *args)
        assert got == [0, 0, 0, 0, 0, 1] and word in err, (args, err)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts(lib):
    p, r = np.zeros(6, np.int64), np.zeros(18, np.int64)
    lib.hc_layout(p.ctypes.data, r.ctypes.data)
    for got, cls, n in ((p, L.HazardParams, 5), (r, L.HazardIO, 17)):
        assert list(got) == [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_] and len(cls._fields_) == n
    assert [n for n, _ in L.HazardParams._fields_] == list(hp.FIELDS) + ["reserved"]


def test_binding_speaks_the_header():
    text = open(os.path.join(ROOT, "include", "emplanner.h")).read()
    assert f"#define EMP_HAZARD_MAX {L.HAZARD_MAX}\n" in text and "#define EMP_ABI_VERSION 13\n" in text and L.ABI_VERSION == 13
    for name, v in (("NONE", hp.HZ_NONE), ("LIGHT", hp.HZ_LIGHT), ("WALKER", hp.HZ_WALKER), ("VEHICLE", hp.HZ_VEHICLE)):
        assert f"#define EMP_HZ_{name} {v}\n" in text and getattr(L, "HZ_" + name) == v
    assert len(L.PROTOTYPES["emp_agent_behave_hazards"][1]) == 14 and len(L.PROTOTYPES["emp_traffic_rollout_hazards"][1]) == 17
    assert L.PROTOTYPES["emp_agent_behave_hazards"][1][:10] == L.PROTOTYPES["emp_agent_behave"][1]
    assert L.PROTOTYPES["emp_traffic_rollout_hazards"][1][:13] == L.PROTOTYPES["emp_traffic_rollout"][1]
    for name in ("emp_hazard_params_default", "emp_agent_behave_hazards", "emp_traffic_rollout_hazards"):
        assert f" {name}(" in text
    from emplanner_carla_amd import api
    p = api.hazard_params()
    assert {k: getattr(p, k) for k in hp.FIELDS} == hp.params() and p.reserved == 0
    assert api.hazard_params(walker_radius=12).walker_radius == 12.0
    with pytest.raises(TypeError):
        api.hazard_params(reserved=1)


# ---- live: the fixtures regenerate ----------------------------------------------------------------------------------------------------
def test_hazard_fixtures_regenerate_bit_for_bit(tmp_path):
    import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("the reference tree is not present")
    env = dict(os.environ, EMP_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_golden_hazards.py")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(GOLDEN, "hazards"))) == sorted(os.listdir(tmp_path / "hazards")) == sorted(n + ".npz" for n in NAMES)
    for name in NAMES:
        want, got = hc.fixture(name), np.load(tmp_path / "hazards" / (name + ".npz"))
        assert sorted(want) == sorted(got.files), name
        for k in want:
            a, b = want[k], got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{name}: {k}"
