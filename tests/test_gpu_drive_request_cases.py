"""GPU suite of emp_drive_request and emp_drive_request_timed on the hard-input table of tests/drive_request_cases.py: actors ON
each of the kernel's seven thresholds and one ulp to either side, up to 64 actors at one computed distance, kept counts at and around
every output capacity (max_obs to 256, max_dyn to 64: the zero-fill loops take several trips), every n_act of interest, NaN and
+-inf in every input field, standstill, signed zeros, reversing and sideways vehicles - against tests/drive_port.py, the project's
own statement of the arithmetic (include/emplanner.h) in Python floats, and against the labels written down in the table.
tests/test_drive_request_cases_host.py checks the table itself on the CPU.

Set EMP_DRIVE_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import drive_port as port  # noqa: E402
import drive_request_cases as D  # noqa: E402
import test_gpu_drive as TD  # noqa: E402  (its fleet, chain and run_drive; nothing of it is collected here)

pytestmark = pytest.mark.gpu

# (max_obs, max_dyn): the smallest, the existing suite's, each side of 64 (one trip of the zero-fill loop or two), three trips
# (130) and the header's limits (256, 64: four trips)
CONFIGS = ((1, 1), (8, 4), (63, 64), (64, 63), (65, 63), (130, 64), (256, 64))
EXACT = ("static_xy", "static_dis", "dyn", "dyn_dis_speed", "origin_xy", "start_a", "actors_next")
COUNTS = ("n_static", "n_dyn", "n_obs", "req_status")
LIBM = ("start_xy", "pred_fi", "start_v")
SHARED = ("static_xy", "n_static", "static_dis", "dyn", "n_dyn", "dyn_dis_speed", "n_obs", "origin_xy", "start_xy", "pred_fi", "start_v",
          "start_a", "req_status", "actors_next")
DT, PLAN_LEAD = 0.01, 0.1
say, to_np, same_bits, up = TD.say, TD.to_np, TD.same_bits, TD.up


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


def api_params(pset):
    from emplanner_carla_amd.api import drive_params
    prm = D.params(pset)
    return drive_params(**{k: prm[k] for k in port.DEFAULTS})


@functools.lru_cache(maxsize=None)
def want_of(pset, max_obs, max_dyn):
    """The port on one parameter set's cases, computed once per shape and left unchanged."""
    _, state, accel, actors, n_act = D.group(pset)
    return port.request_batch(state, accel, actors, n_act, max_obs, max_dyn, D.params(pset))


def eq_nan(a, b):
    """Bit-equal, NaN matching NaN."""
    a, b = np.ascontiguousarray(to_np(a), np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def close_nan(a, b, tol=1e-12):
    """TD.close's bar where the port's value is finite; the same infinity or NaN for NaN where it is not."""
    a, b = to_np(a), np.asarray(b)
    fin = np.isfinite(b)
    with np.errstate(invalid="ignore"):
        ok = np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))
    return bool(np.all(np.where(fin, ok, (a == b) | (np.isnan(a) & np.isnan(b)))))


def worst(a, b):
    a, b = to_np(a), np.asarray(b)
    fin = np.isfinite(b) & np.isfinite(a)
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin])), initial=0.0))


def libm_free(c):
    """fi = 0 and a heading of zero (or no speed at all): every libm argument of the kernel is a zero."""
    _, _, fi, Vy, _, Vx = c["state"]
    wx, wy = port.world_velocity(fi, Vy, Vx)
    return fi == 0.0 and (math.atan2(wy, wx) == 0.0 or (wx == 0.0 and wy == 0.0))


def check_against_port_and_labels(r, pset, max_obs, max_dyn, what):
    cases, state, accel, actors, n_act = D.group(pset)
    want = want_of(pset, max_obs, max_dyn)
    for name in COUNTS:
        assert np.array_equal(to_np(getattr(r, name)), want[name]), f"{what}: {name}"
    for name in EXACT:
        bad = [cases[b]["name"] for b in range(len(cases)) if not eq_nan(to_np(getattr(r, name))[b], want[name][b])]
        assert not bad, f"{what}: {name} of {bad[:6]}"
    w = max(worst(getattr(r, n), want[n]) for n in LIBM)
    say(f"{what}: worst |GPU - port| / max(1, |port|) in start_xy / pred_fi / start_v {w:.3g} (bar 1e-12)")
    for name in LIBM:
        bad = [cases[b]["name"] for b in range(len(cases)) if not close_nan(to_np(getattr(r, name))[b], want[name][b])]
        assert not bad, f"{what}: {name} of {bad[:6]}"
        bad = [c["name"] for b, c in enumerate(cases) if libm_free(c) and not eq_nan(to_np(getattr(r, name))[b], want[name][b])]
        assert not bad, f"{what}: {name} of {bad[:6]} must be bit-equal: every libm argument is zero"
    assert sum(libm_free(c) for c in cases) >= 3
    # the labels, without the port
    sxy, dyn, ns, nd, nobs, status = (to_np(getattr(r, n)) for n in ("static_xy", "dyn", "n_static", "n_dyn", "n_obs", "req_status"))
    for b, c in enumerate(cases):
        if c["label"] is None:
            continue
        ls, ld = c["label"]["static"], c["label"]["dyn"]
        assert ns[b] == min(len(ls), max_obs) and nd[b] == min(len(ld), max_dyn), f"{what}: counts of {c['name']}"
        assert status[b] == (1 if len(ls) > max_obs or len(ld) > max_dyn else 0), f"{what}: req_status of {c['name']}"
        assert same_bits(sxy[b, :ns[b]], c["actors"][ls[:max_obs], :2]), f"{what}: static order of {c['name']}"
        assert same_bits(dyn[b, :nd[b], :2], c["actors"][ld[:max_dyn], :2]), f"{what}: dynamic order of {c['name']}"
        gated = min(c["label"]["n_obs"], max_obs)
        assert nobs[b] == gated, f"{what}: n_obs of {c['name']}"
    # unused slots are +0.0, out to the last one
    idle_s = np.arange(max_obs)[None, :] >= ns[:, None]
    idle_d = np.arange(max_dyn)[None, :] >= nd[:, None]
    for arr, idle in ((sxy, idle_s), (to_np(r.static_dis), idle_s), (dyn, idle_d)):
        v = arr[idle]
        assert not v.any() and not np.signbit(v).any(), f"{what}: an unused slot is not +0.0"


@pytest.mark.parametrize("pset", list(D.PARAM_SETS))
@pytest.mark.parametrize("max_obs,max_dyn", CONFIGS)
def test_request_on_the_case_table(pl, max_obs, max_dyn, pset):
    _, state, accel, actors, n_act = D.group(pset)
    r = pl.drive_request(api_params(pset), state, accel, actors, n_act, max_obs, max_dyn, advance=True)
    check_against_port_and_labels(r, pset, max_obs, max_dyn, f"request {pset} ({max_obs}, {max_dyn})")


@pytest.mark.parametrize("pset", list(D.PARAM_SETS))
def test_request_is_independent_of_the_batch(pl, pset):
    """tests/batch_check.invariant: alone, in the batch, reversed, shifted by one and on the device path - a NaN, 64-way-tied or
    truncated vehicle changes nothing in the other wavefronts of its block (the table alternates hostile and plain vehicles)."""
    import batch_check as bc
    max_obs, max_dyn = 65, 63
    cases, state, accel, actors, n_act = D.group(pset)
    assert len(cases) > 8
    prm = api_params(pset)

    def call(args, device):
        r = pl.drive_request(prm, *args, max_obs, max_dyn, advance=True)
        if device:
            pl.synchronize()
        return {n: to_np(getattr(r, n)) for n in SHARED}

    full = bc.invariant(call, [state, accel, actors, n_act], f"drive_request {pset}")
    want = want_of(pset, max_obs, max_dyn)
    assert np.array_equal(full["n_static"], want["n_static"]) and np.array_equal(full["n_dyn"], want["n_dyn"])


@pytest.mark.parametrize("pset", list(D.PARAM_SETS))
def test_request_in_place_on_device_tensors(pl, pset):
    max_obs, max_dyn = 8, 4
    cases, state, accel, actors, n_act = D.group(pset)
    prm = api_params(pset)
    r = pl.drive_request(prm, state, accel, actors, n_act, max_obs, max_dyn, advance=True)
    dev_actors = up(actors)
    rd = pl.drive_request(prm, up(state), up(accel), dev_actors, up(n_act), max_obs, max_dyn, in_place=True)
    pl.synchronize()
    assert rd.actors_next is dev_actors
    for name in SHARED:
        assert same_bits(getattr(rd, name), getattr(r, name)), name
    after = to_np(dev_actors)
    for b, c in enumerate(cases):                                         # poisoned slots keep their bits
        assert same_bits(after[b, D.live(c["n_act"]):], actors[b, D.live(c["n_act"]):]), c["name"]
    assert any(D.live(c["n_act"]) < D.A for c in cases)


def test_request_between_guard_rows(pl):
    """One raw EMP_DEVICE call with max_obs = 130 on views with a guard row before and after the batch; the guard rows of the
    inputs hold live actors and n_act = 2 ** 30."""
    import batch_check as bc
    pset, max_obs, max_dyn = "default", 130, 64
    _, state, accel, actors, n_act = D.group(pset)
    prm = api_params(pset)
    live_row = np.tile(np.array([3.0, -1.0, 2.0, 0.5]), (D.A, 1))
    outs = dict(static_xy=((max_obs, 2), np.float64), n_static=((), np.int32), static_dis=((max_obs,), np.float64),
                dyn=((max_dyn, 4), np.float64), n_dyn=((), np.int32), dyn_dis_speed=((2,), np.float64), n_obs=((), np.int32),
                origin_xy=((2,), np.float64), start_xy=((2,), np.float64), pred_fi=((), np.float64), start_v=((2,), np.float64),
                start_a=((2,), np.float64), req_status=((), np.int32), actors_next=((D.A, 4), np.float64))
    spec = dict(fn="emp_drive_request", sig=[C.byref(prm), "B", D.A, max_obs, max_dyn, "state", "accel", "actors", "n_act", *outs],
                ins=dict(state=(state, np.array([0.0, 0.0, 0.1, 0.0, 0.0, 5.0])), accel=(accel, 1.0), actors=(actors, live_row),
                         n_act=(n_act, 2 ** 30)),
                outs=outs)
    g = bc.Guarded(pl, spec)
    raw = g.call()
    g.check_guards("drive_request, max_obs 130")
    r = pl.drive_request(prm, state, accel, actors, n_act, max_obs, max_dyn, advance=True)
    for name in SHARED:
        assert same_bits(raw[name], getattr(r, name)), name
    check_against_port_and_labels(r, pset, max_obs, max_dyn, "request between guard rows")


# ---------------------------------------------------------------------------------------------------------------------
# the timed request on the same table
# ---------------------------------------------------------------------------------------------------------------------
T0S = (0.0, -5.0, 1e9, math.nan)
TICKS = (0, 1, 2 ** 31 - 1)


@pytest.mark.parametrize("pset", list(D.PARAM_SETS))
@pytest.mark.parametrize("max_obs,max_dyn", [(8, 4), (65, 63), (256, 64)])
def test_timed_request_on_the_case_table(pl, max_obs, max_dyn, pset):
    cases, state, accel, actors, n_act = D.group(pset)
    B = len(cases)
    prm = api_params(pset)
    want = want_of(pset, max_obs, max_dyn)
    r = pl.drive_request(prm, state, accel, actors, n_act, max_obs, max_dyn, advance=True)
    t0 = np.array([T0S[b % 4] for b in range(B)])
    heading = np.array([math.atan2(*port.world_velocity(c["state"][2], c["state"][3], c["state"][5])[::-1]) for c in cases])
    dyn_obs = np.zeros((B, max_dyn, 4))
    for b in range(B):
        for q, i in enumerate(want["dyn_idx"][b]):
            dyn_obs[b, q] = actors[b, i]                                  # x, y, vx, vy before the advance
    for tick in TICKS:
        rt = pl.drive_request_timed(prm, state, accel, actors, n_act, t0, tick, DT, max_obs, max_dyn, plan_lead=PLAN_LEAD, advance=True)
        for name in SHARED:
            assert same_bits(getattr(rt, name), getattr(r, name)), f"tick {tick}: {name}"
        bad = [cases[b]["name"] for b in range(B) if not eq_nan(rt.dyn_obs[b], dyn_obs[b])]
        assert not bad, f"dyn_obs of {bad[:6]}"
        say(f"timed request {pset} ({max_obs}, {max_dyn}) tick {tick}: worst |GPU - atan2| {worst(rt.start_heading, heading):.3g} (bar 1e-12)")
        assert close_nan(rt.start_heading, heading)
        exact = 0
        for b, c in enumerate(cases):
            wx, wy = port.world_velocity(c["state"][2], c["state"][3], c["state"][5])
            if c["state"][2] == 0.0 and wy == 0.0 and not math.isnan(wx):      # atan2(+-0, wx) is +-0 or +-pi: sign and value exact
                assert eq_nan(rt.start_heading[b], heading[b]), (c["name"], float(rt.start_heading[b]), heading[b])
                exact += 1
        assert exact >= 8 or pset != "default"
        clock = np.array([(float(t) + float(tick) * DT) + PLAN_LEAD for t in t0])
        assert eq_nan(rt.plan_start_time, clock), f"tick {tick}: plan_start_time"
    assert np.isnan(clock[3]) and clock[2] != clock[0]


# ---------------------------------------------------------------------------------------------------------------------
# in the loop: a 64-way tie and an actor on the gate, all 64 slots live
# ---------------------------------------------------------------------------------------------------------------------
def loop_fleet(T, M):
    """TD.fleet(2) with 64 live actors per vehicle, the vehicles on dyadic positions so that the constructed distances are exact.
    Vehicle 0: 64 actors at one identical spot 25 m ahead and 1 m beside, every second one moving: 32 + 32 at one distance each,
    truncated to MAX_OBS and MAX_DYN.  Vehicle 1: a static actor at dis == 30 exactly in period 0 (the gate is open: n_obs =
    n_static), the other 63 slots live but out of the band or the range."""
    f = TD.fleet(2, T, M)
    actors = np.zeros((2, D.A, 4))
    gate_rot = 0.9                                                              # (18, 24) lies 30 m ahead and 0.8 m beside this heading
    f["global_path"][1] = TD.straight(gate_rot, *f["global_path"][1, 0, :2])
    f["state"][1] = [*TD.at(f["global_path"][1, 0], gate_rot, 10.0, -0.2), gate_rot, 0.0, 0.0, f["state"][1, 5]]
    for b in range(2):
        rot = f["global_path"][b, 0, 2]
        f["state"][b, :2] = np.round(f["state"][b, :2] * 8.0) / 8.0
        x, y = f["state"][b, :2]
        c, s = math.cos(rot), math.sin(rot)
        if b == 0:
            spot = D.place(f["state"][b], 25.0, 1.0)
            for i in range(D.A):
                actors[b, i] = spot + ((6.0 * c, 6.0 * s) if i % 2 else (0.0, 0.0))
        else:
            for i in range(D.A):
                actors[b, i] = D.place(f["state"][b], 5.0 + i, 9.0 + 0.25 * i) + ((0.0, 0.0) if i % 3 else (2.0 * c, 2.0 * s))
            actors[b, 17] = (D.off(x, 18.0), D.off(y, 24.0), 0.0, 0.0)          # dis = sqrt(324 + 576) = 30, every step exact
    f["actors"], f["n_act"] = actors, np.array([D.A, 1000], np.int32)
    return f


def test_hard_requests_inside_the_loop(pl):
    law, K, T = "mpc", 2, 2
    assert (TD.MAX_OBS, TD.MAX_DYN) == (4, 2)
    f = loop_fleet(T, TD.params(law)["M"])
    first = port.request_batch(f["state"], f["accel"], f["actors"], f["n_act"], TD.MAX_OBS, TD.MAX_DYN)
    assert first["req_status"][0] == 1 and first["n_static"][0] == 4 and first["n_dyn"][0] == 2 and first["static_idx"][0] == [0, 2, 4, 6]
    assert first["dyn_idx"][0] == [1, 3]
    assert first["static_dis"][1, 0] == 30.0 and first["static_idx"][1][0] == 17 and first["n_obs"][1] == first["n_static"][1] >= 1
    want = TD.chain(pl, law, f, K, T)
    r = TD.run_drive(pl, law, f, K, T)
    for name in r.__dataclass_fields__:
        assert same_bits(getattr(r, name), want[name]), name
    actors, seen = f["actors"].copy(), []
    for k in range(K):
        q = port.request_batch(to_np(r.log_state)[k], None, actors, f["n_act"], TD.MAX_OBS, TD.MAX_DYN)
        seen.append(np.column_stack([q["n_obs"], q["n_dyn"]]))
        actors = np.array([port.advance(actors[b], f["n_act"][b], T * TD.DT) for b in range(2)])
    say(f"in the loop: (n_obs, n_dyn) per period on the port {np.array(seen).tolist()}")
    assert np.array_equal(to_np(r.log_counts), np.array(seen))
    assert same_bits(r.actors, actors)
