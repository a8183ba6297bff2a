"""CPU suite of the car-following law: the Python port (tests/behavior_port.py) against what the reference's BehaviorAgent did, tick
by tick, on the recorded closed loops of tests/golden/behavior/; the g++ build of csrc/emp_behavior_core.h
(tests/host_check/behavior_check.cpp) bit for bit against the port - host acos is libm's, as Python's is - on the fixtures, on
hand-built threshold cases and on ragged random worlds; that build as a sanitized program of its own; the launch plan; the ctypes
layouts and prototypes; and - where the reference tree is present - every fixture regenerated bit for bit."""
from __future__ import annotations

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "host_check", "behavior_check.cpp")
NAMES = bc.mkb.NAMES
# The steer of the port against the reference's, by the rule of tests/test_agent_host.py: acos near 1 turns a last-bit difference of
# its argument (NumPy's dot / norm against scalar arithmetic) into up to about 1e-8 rad.  The worst difference over the fixtures is
# 1.03e-11; the bar is four times that, and above 1e-6 rad it would be another law, not rounding.
STEER_MEASURED = 1.03e-11
STEER_BAR = 4 * STEER_MEASURED
STEER_CAP = 1e-6


# -fno-builtin-sin / -cos: g++ otherwise merges agt::observe's sin(fi) and cos(fi) into one sincos call, whose cosine is not always
# the bit pattern of libm's cos - and libm's sin and cos are what the port (Python's math) calls
NO_SINCOS = ["-fno-builtin-sin", "-fno-builtin-cos"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("behavior_check") / "libbehaviorcheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall"] + NO_SINCOS + [SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    p, i, q = C.c_void_p, C.c_int, C.c_longlong
    lib.bc_layout.restype = None
    lib.bc_layout.argtypes = [p, p]
    lib.bc_plan.restype = C.c_char_p
    lib.bc_plan.argtypes = [i, i, i, i, i, i, q, p]
    lib.bc_behave.restype = None
    lib.bc_behave.argtypes = [C.POINTER(L.AgentParams), C.POINTER(L.BehaviorParams), i, i, i, i, q, C.POINTER(L.BehaviorIO)]
    lib.bc_rollout.restype = None
    lib.bc_rollout.argtypes = [C.POINTER(L.AgentParams), C.POINTER(L.BehaviorParams), C.POINTER(L.VehicleParams), i, i, i, i, i, i, q, C.POINTER(L.BehaviorIO)]
    return lib


def c_params(prm):
    return L.AgentParams(*[float(prm[k]) for k in ap.DEFAULTS], 0)


def c_behavior(prb):
    return L.BehaviorParams(*[float(prb[k]) for k in bp.FIELDS[:-1]], int(prb["look_steps"]), 0)


def c_vehicle(vp):
    return L.VehicleParams(*[float(v) for v in vp], 0)


def io_of(ins, outs):
    """emp_behavior_io over dicts of arrays (the fields of their names; outputs of the agent state are named *_out)."""
    io = L.BehaviorIO()
    keep = []
    for k, v in ins.items():
        v = np.ascontiguousarray(v)
        keep.append(v)
        setattr(io, k, v.ctypes.data if v.size or k in ("n_world",) else None)
    for k, v in outs.items():
        assert v.flags.c_contiguous
        setattr(io, k + "_out" if k in bc.STATE_OUT or k == "state" else k, v.ctypes.data)
    io.reserved = 0
    return io, keep


def host_behave(lib, prm, prb, b, tick0=0, aliased=False):
    """bc_behave on a batch: a dict of its outputs; padding slots keep the 7s they start with (aliased: the inputs' values)."""
    W, N, M = b["lane"].shape
    K = b["other"].shape[1]
    ins = {k: np.ascontiguousarray(b[k]).copy() for k in bc.IN_KEYS}
    o = {k: (ins[k] if aliased else np.full_like(ins[k], 7)) for k in bc.STATE_OUT}
    o.update(status=np.full((W, N), 7, np.int32), control=np.full((W, N, 3), 7.0), mode=np.full((W, N), 7, np.int32),
             blocker=np.full((W, N), 7, np.int32), distance=np.full((W, N), 7.0), ttc=np.full((W, N), 7.0),
             target_speed_out=np.full((W, N), 7.0), lat_error=np.full((W, N), 7.0), lon_command=np.full((W, N), 7.0))
    io, keep = io_of(ins, o)
    lib.bc_behave(C.byref(c_params(prm)), C.byref(c_behavior(prb)), W, N, M, K, tick0, C.byref(io))
    return o


def sevens(b, aliased=False):
    """What the padding slots of host_behave's outputs hold."""
    f = {k: (b[k] if aliased else np.full_like(b[k], 7)) for k in bc.STATE_OUT}
    W, N = b["n_path"].shape
    for k in bc.TICK_OUT:
        f[k] = np.full((W, N, 3) if k == "control" else (W, N), 7, np.int32 if k in bc.INT_OUT else np.float64)
    return f


def assert_same(got, want, what, live=None):
    for k in bc.STATE_OUT + bc.TICK_OUT:
        if k in ("lon_err", "lat_err") and live is not None:          # entries at and past the count pass through: checked where aliased
            n = want["n_" + k[:3]]
            m = (np.arange(ap.BUFFER)[None, None, :] < n[..., None]) | ~live[..., None]
            bc.same_bits(got[k][m], want[k][m], f"{what}: {k}")
        else:
            bc.same_bits(got[k], want[k], f"{what}: {k}")


# ---- the port against the reference ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replays():
    return {n: bc.replay(n) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_port_equals_the_recorded_reference_tick_by_tick(replays, name):
    f, r = replays[name]
    np.testing.assert_array_equal(r["queue"], f["queue"], err_msg=f"{name}: queue lengths")
    np.testing.assert_array_equal(r["target"], f["target"], err_msg=f"{name}: _target_speed after the tick")
    np.testing.assert_array_equal(r["mode"], f["mode"], err_msg=f"{name}: modes")
    em = r["mode"] == bp.EMERGENCY
    bc.same_bits(r["control"][em], f["control"][em], f"{name}: emergency ticks")
    assert not em.any() or (f["control"][em] == (0.0, 0.0, 0.5)).all()
    d = np.abs(r["control"] - f["control"]).reshape(-1, 3).max(0)
    print(f"{name}: worst throttle / steer / brake difference {d[0]:.3g} / {d[1]:.3g} / {d[2]:.3g}")
    assert d[0] <= 1e-12 and d[2] <= 1e-12, f"{name}: throttle {d[0]}, brake {d[2]}"
    assert STEER_BAR <= STEER_CAP and d[1] <= STEER_BAR, f"{name}: steer differs by {d[1]}"


def test_the_steer_bar_is_the_measured_one(replays):
    worst = max(np.abs(r["control"][..., 1] - f["control"][..., 1]).max() for f, r in replays.values())
    print(f"worst steer difference over the fixtures: {worst:.4g}")
    assert STEER_MEASURED / 2 <= worst <= STEER_MEASURED, "the measured figure in this file and in DESIGN.md 3.12 is stale"


def test_fixtures_cover_what_they_are_for(replays):
    ticks = {n: bc.fixture(n)["mode_ticks"] for n in NAMES}
    for n in NAMES:
        f = bc.fixture(n)
        np.testing.assert_array_equal(ticks[n], [[(f["mode"][:, v] == m).sum() for m in range(6)] for v in range(f["mode"].shape[1])])
        assert f["margin"].min() >= bc.mkb.MIN_MARGIN
    # every reacting mode occurs in `follow`; the counts are the recorded ones
    assert ticks["follow"][0].tolist() == [326, 98, 10, 9, 157, 0] and (ticks["follow"][0][1:5] > 0).all()
    assert ticks["follow"][1][0] == 600                                           # the leader sees nobody
    for n in ("collinear", "other_lane"):
        assert ticks[n][:, 1:].sum() == 0, f"{n}: the leader is never detected"
    centre = lambda f: np.sqrt(((f["seen"][:, 0, :2] - f["seen"][:, 1, :2]) ** 2).sum(1))
    assert centre(bc.fixture("collinear")).min() < 1.0                            # driven through, with no reaction on any tick
    assert 4.0 < centre(bc.fixture("follow")).min() < 4.5
    f = bc.fixture("cruise")                                                      # the follower settles at the leader's 40 km/h
    assert abs(f["seen"][-1, 0, 4] - 40.0) < 1.0 and abs(f["seen"][-1, 1, 4] - 40.0) < 1.0 and (np.abs(f["target"][-100:, 0] - 40.0) < 0.1).all()
    f = bc.fixture("stopped_leader")                                              # the pass-through is kept
    assert f["brake_from"][1] == 200 and f["seen"][-1, 1, 4] < 1e-6 and centre(f).min() < 1.0 and ticks["stopped_leader"][0][4] > 0
    f = bc.fixture("merge")                                                       # seen only once head + 5 has crossed the boundary
    first = int(np.argmax(f["mode"][:, 0] != bp.NORMAL))
    head = f["n_path"][0] - f["queue"][:, 0]
    boundary = int(np.argmax(f["lane"][0] == 2))
    assert first > 5 and head[first - 1] + 5 >= boundary > head[first - 2] + 5
    assert centre(f)[:first].max() < f["speed_limit"][0] / 3                       # in range all along: the key alone kept it unseen
    _, r = replays["platoon4"]                                                    # the rear vehicle takes slot 1, though slot 2 is nearer
    f = bc.fixture("platoon4")
    d1 = np.sqrt(((f["seen"][:, 0, :2] - f["seen"][:, 1, :2]) ** 2).sum(1))
    d2 = np.sqrt(((f["seen"][:, 0, :2] - f["seen"][:, 2, :2]) ** 2).sum(1))
    assert ((r["blocker"][:, 0] == 0) & (d2 < d1)).sum() > 100
    assert sum(os.path.getsize(os.path.join(GOLDEN, "behavior", n + ".npz")) for n in NAMES) < 900 * 1024


# ---- the core, compiled with g++ ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_core_equals_the_port_on_the_recorded_inputs(lib, name):
    """Every vehicle of the fixture as a world of its own scene, every third tick a call from the port's agent state: every output to
    the bit."""
    f = bc.fixture(name)
    T, V = f["queue"].shape
    M = f["lane"].shape[1]
    prm, prb = ap.params(), bp.params()
    _, b0 = bc.fixture_world(name)
    head = np.zeros(V, np.int32)
    agents = [ap.Agent() for _ in range(V)]
    for t in range(T):
        b = {k: v.copy() for k, v in b0.items()}
        b["state"][0, :, :2], b["forward"][0], b["speed_kmh"][0] = f["seen"][t, :, :2], f["seen"][t, :, 2:4], f["seen"][t, :, 4]
        packed = ap.pack(agents, np.zeros((V, ap.BUFFER)), np.zeros((V, ap.BUFFER)))
        for k in bc.STATE_OUT:
            b[k][0] = packed[k]
        want = bc.port_behave(prm, prb, b, fill=bc_fill(b))
        if t % 3 == 0:
            assert_same(host_behave(lib, prm, prb, b), want, f"{name} tick {t}")
        agents = ap.agents_of(*[want[k][0] for k in bc.STATE_OUT])
        for i in range(V):                                                         # a vehicle its agent no longer drives keeps the recorded head
            if 0 <= f["brake_from"][i] <= t:
                agents[i].head = int(f["n_path"][i] - f["queue"][t, i])


def bc_fill(b, aliased=False):
    return sevens(b, aliased)


def test_core_on_the_threshold_cases(lib):
    b, names, tick0 = bc.edge_cases()
    prm, prb = ap.params(), bp.params()
    w = dict(zip(names, range(len(names))))
    for t0 in sorted(set(tick0)):
        want = bc.port_behave(prm, prb, b, t0, fill=sevens(b))
        assert_same(host_behave(lib, prm, prb, b, t0), want, f"tick0 {t0}")
        assert_same(host_behave(lib, prm, prb, b, t0, aliased=True), bc.port_behave(prm, prb, b, t0, fill=sevens(b, True)), f"tick0 {t0} aliased")
        mode, blk = want["mode"][:, 0], want["blocker"][:, 0]
        if t0 == 200:
            assert mode[w["an other moves into range at tick0"]] != bp.NORMAL and blk[w["an other moves into range at tick0"]] == 0
            continue
        # what each case is for did happen
        assert mode[w["an other moves into range at tick0"]] == bp.NORMAL
        assert blk[w["norm == th"]] == 0 and blk[w["norm one ulp above th"]] == -1 and blk[w["norm one ulp below th"]] == 0
        assert mode[w["norm == 0.001"]] == bp.NORMAL and mode[w["norm one ulp above 0.001 straight behind"]] == bp.NORMAL
        assert mode[w["norm one ulp below 0.001"]] == bp.EMERGENCY
        assert mode[w["angle exactly 0: not seen"]] == bp.NORMAL and blk[w["angle just above 0"]] == 0
        assert blk[w["angle near 30 inside"]] == 0 and blk[w["angle near 30 outside"]] == -1 and blk[w["behind"]] == -1
        assert mode[w["d == braking_distance"]] != bp.EMERGENCY and mode[w["d one ulp below"]] == bp.EMERGENCY and mode[w["d one ulp above"]] != bp.EMERGENCY
        assert want["ttc"][w["ttc == safety_time"], 0] == 3.0 and mode[w["ttc == safety_time"]] == bp.FOLLOW
        assert mode[w["ttc just below safety_time"]] == bp.SLOW and mode[w["ttc just above safety_time"]] == bp.FOLLOW
        assert want["ttc"][w["ttc == 2 safety_time"], 0] == 6.0 and mode[w["ttc == 2 safety_time"]] == bp.CLEAR
        assert mode[w["ttc just below 2 safety_time"]] == bp.FOLLOW and mode[w["ttc just above 2 safety_time"]] == bp.CLEAR
        a = w["dv clipped to 1: the leader is faster"]
        assert want["ttc"][a, 0] == want["distance"][a, 0]
        assert want["target_speed_out"][w["positive() at 0: vs == speed_decrease"], 0] == 0.0 and want["target_speed_out"][w["positive() below 0"], 0] == 0.0
        assert mode[w["follow below min_speed"]] == bp.FOLLOW and want["target_speed_out"][w["follow below min_speed"], 0] == 5.0
        a = w["two hit: the first wins though the second is nearer"]
        assert blk[a] == 0 and abs(want["distance"][a, 0] - 11.0) < 1e-9
        assert blk[w["the first is keyed -1: the second is taken"]] == 1 and blk[w["the first is on another lane"]] == 1
        assert blk[w["key_next matches"]] == 0 and blk[w["a DONE blocker is still seen"]] == 0 and want["mode"][w["a DONE blocker is still seen"], 1] == bp.DONE
        assert blk[w["a blocker without a plan shows -1"]] == -1
        assert blk[w["an other is hit"]] == 0 and blk[w["an agent comes before an other"]] == 0
        for name in ("the ego is DONE", "the ego has no plan"):
            assert mode[w[name]] == bp.DONE and tuple(want["control"][w[name], 0]) == (0.0, 0.0, 1.0) and want["status"][w[name], 0] == ap.DONE
        assert mode[w["alone"]] == bp.NORMAL and want["target_speed_out"][w["alone"], 0] == 50.0 and np.isinf(want["distance"][w["alone"], 0])
        # an emergency tick leaves the agent state alone
        a = w["d one ulp below"]
        assert tuple(want["control"][a, 0]) == (0.0, 0.0, 0.5) and want["n_lon"][a, 0] == 0 and want["head"][a, 0] == 0 and want["target_speed_out"][a, 0] == 60.0
        # a reacting tick steps the local planner twice
        assert want["n_lon"][w["d one ulp above"], 0] == 2 and want["n_lon"][w["alone"], 0] == 1


@pytest.mark.parametrize("sizes,N,K,M", (((0, 1, 64), 64, 0, 8), ((1, 2, 3, 64, 7), 64, 3, 40), ((5, 17, 2, 9), 17, 64, 13)))
def test_core_on_ragged_worlds_with_poisoned_padding(lib, sizes, N, K, M):
    b = bc.random_worlds(sizes, N, K, M, seed=sum(sizes) * 100 + M)
    prm, prb = ap.params(), bp.params()
    live = bc.live_mask(b)
    for t0 in (0, 37):
        want = bc.port_behave(prm, prb, b, t0, fill=sevens(b))
        assert_same(host_behave(lib, prm, prb, b, t0), want, f"tick0 {t0}", live)
        assert_same(host_behave(lib, prm, prb, b, t0, aliased=True), bc.port_behave(prm, prb, b, t0, fill=sevens(b, True)), f"tick0 {t0} aliased")
    if N == 64 and K:
        seen = [int((want["mode"][live] == m).sum()) for m in range(6)]
        assert min(seen) > 0, f"modes met: {seen}"


def host_rollout(lib, prm, prb, vp, b, T, every, tick0=0):
    W, N, M = b["lane"].shape
    K = b["other"].shape[1]
    n_log = (T + every - 1) // every
    ins = {k: np.ascontiguousarray(b[k]).copy() for k in bc.IN_KEYS if k not in ("forward", "speed_kmh")}
    o = {k: np.full_like(ins[k], 7) for k in bc.STATE_OUT}
    o.update(state=np.full((W, N, 6), 7.0), status=np.full((W, N), 7, np.int32), done_tick=np.full((W, N), 7, np.int32),
             mode_ticks=np.full((W, N, 5), 7, np.int32), min_gap=np.full((W, N), 7.0), actors_out=np.full((W, N, 4), 7.0),
             log_state=np.full((n_log, W, N, 6), 7.0), log_control=np.full((n_log, W, N, 3), 7.0), log_head=np.full((n_log, W, N), 7, np.int32),
             log_mode=np.full((n_log, W, N), 7, np.int32), log_target=np.full((n_log, W, N), 7.0))
    io, keep = io_of(ins, o)
    lib.bc_rollout(C.byref(c_params(prm)), C.byref(c_behavior(prb)), C.byref(c_vehicle(vp)), W, N, M, K, T, every, tick0, C.byref(io))
    return o


@pytest.mark.parametrize("name", ("follow", "platoon4", "merge"))
def test_core_rollout_equals_the_port_loop_and_the_recording(lib, name):
    """The kernel's loop on the CPU against the port's on a fixture's scenario - states, heads, modes, targets, controls bit for
    bit, since libm is the same - and the recording itself: the same closed loop."""
    f, b = bc.fixture_world(name)
    T, V = f["queue"].shape
    T, every = min(T, 300), 3
    prm, prb, vp = ap.params(), bp.params(), ap.vehicle_params()
    got = host_rollout(lib, prm, prb, vp, b, T, every)
    agents = [ap.Agent() for _ in range(V)]
    w = bc.world_of(b, 0, V)
    want = bp.rollout(prm, prb, vp, w, agents, T)
    bc.same_bits(got["state"][0], want["end"], f"{name}: final state")
    bc.same_bits(got["log_state"][:, 0], want["state"][::every], f"{name}: log_state")
    bc.same_bits(got["log_control"][:, 0], want["control"][::every], f"{name}: log_control")
    bc.same_bits(got["log_target"][:, 0], want["target"][::every], f"{name}: log_target")
    np.testing.assert_array_equal(got["log_head"][:, 0], want["head"][::every])
    np.testing.assert_array_equal(got["log_mode"][:, 0], want["mode"][::every])
    np.testing.assert_array_equal(got["mode_ticks"][0], [[(want["mode"][:, v] == m).sum() for m in range(5)] for v in range(V)])
    seen_d = np.where(np.isfinite(want["distance"]), want["distance"], np.inf).min(0)
    bc.same_bits(got["min_gap"][0], seen_d, f"{name}: min_gap")
    np.testing.assert_array_equal(want["mode"], f["mode"][:T], err_msg=f"{name}: the port's closed loop leaves the recorded modes")
    assert np.abs(want["state"][:, :, :2] - f["seen"][:T, :, :2]).max() < 1e-6, f"{name}: the port's closed loop leaves the recorded one"


def test_behavior_check_as_a_program_of_its_own(tmp_path):
    """-DBEHAVIOR_CHECK_MAIN: the self-checking program a sanitizer build runs (here: address and undefined behaviour, on the CPU)."""
    exe = str(tmp_path / "behavior_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DBEHAVIOR_CHECK_MAIN"] + NO_SINCOS + [SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "behavior_check: 0 bad, 0 wrong" in run.stdout, run.stdout + run.stderr[-2000:]


# ---- the launch plan ------------------------------------------------------------------------------------------------------------------
def plan(lib, W, N, K, M, T, every, tick0=0):
    out = np.zeros(6, np.int64)
    err = lib.bc_plan(W, N, K, M, T, every, tick0, out.ctypes.data)
    return out.tolist(), (err.decode() if err else None)


def test_launch_plan(lib):
    lds = 8 * (2 * 64 * 11 + 2 * 3 * 64 + 64 + 64 + 5 * 64 + 32)                   # deques, two published buffers, keys, extents, others
    assert lds == 18176
    assert plan(lib, 5, 64, 3, 40, 0, 1) == ([5, 64, lds, 160 * 1024 // lds, 0, 0], None)
    assert plan(lib, 512, 8, 0, 40, 100, 7) == ([512, 64, lds, 9, 15, 0], None)
    assert plan(lib, 1, 1, 64, 1, 65536, 1, 2 ** 31 - 1 - 65536)[0][4:] == [65536, 0]
    assert plan(lib, 0, 64, 0, 40, 10, 1) == ([0, 0, 0, 0, 0, 0], None)             # an empty batch launches nothing
    for args, word in (((1, 0, 0, 1, 1, 1), "max_world"), ((1, 65, 0, 1, 1, 1), "max_world"), ((1, 1, -1, 1, 1, 1), "max_other"),
                       ((1, 1, 65, 1, 1, 1), "max_other"), ((1, 1, 0, 0, 1, 1), "max_path"), ((-1, 1, 0, 1, 1, 1), "W < 0"),
                       ((1, 1, 0, 1, 65537, 1), "T outside"), ((1, 1, 0, 1, -1, 1), "T outside"), ((1, 1, 0, 1, 5, 0), "log_every"),
                       ((1, 1, 0, 1, 5, 1, -1), "tick0"), ((1, 1, 0, 1, 5, 1, 2 ** 31 - 5), "tick0"), ((0, 0, 0, 1, 1, 1), "max_world")):
        got, err = plan(lib, *args)
        assert got == [0, 0, 0, 0, 0, 1] and word in err, (args, err)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts(lib):
    p, r = np.zeros(12, np.int64), np.zeros(45, np.int64)
    lib.bc_layout(p.ctypes.data, r.ctypes.data)
    for got, cls, n in ((p, L.BehaviorParams, 11), (r, L.BehaviorIO, 44)):
        assert list(got) == [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_] and len(cls._fields_) == n
    assert [n for n, _ in L.BehaviorParams._fields_] == list(bp.FIELDS) + ["reserved"]


def test_binding_speaks_the_header():
    text = open(os.path.join(ROOT, "include", "emplanner.h")).read()
    assert f"#define EMP_TRAFFIC_MAX_WORLD {L.TRAFFIC_MAX_WORLD}\n" in text and "#define EMP_ABI_VERSION 13\n" in text and L.ABI_VERSION == 13
    for name, v in (("NORMAL", bp.NORMAL), ("SLOW", bp.SLOW), ("FOLLOW", bp.FOLLOW), ("CLEAR", bp.CLEAR), ("EMERGENCY", bp.EMERGENCY), ("DONE", bp.DONE)):
        assert f"#define EMP_BHV_{name} {v}\n" in text and getattr(L, "BHV_" + name) == v
    for name, v in (("EMP_BHV_CAUTIOUS", "cautious"), ("EMP_BHV_KIND_NORMAL", "normal"), ("EMP_BHV_AGGRESSIVE", "aggressive")):
        assert f"#define {name} {L.BHV_KINDS[v]}\n" in text
    assert len(L.PROTOTYPES["emp_agent_behave"][1]) == 10 and len(L.PROTOTYPES["emp_traffic_rollout"][1]) == 13
    assert L.PROTOTYPES["emp_behavior_params_default"][0] is None
    for name in ("emp_behavior_params_default", "emp_agent_behave", "emp_traffic_rollout"):
        assert f" {name}(" in text
    assert "reproduced by emp_agent_behave" in text
    from emplanner_carla_amd import api
    for kind in bp.KINDS:
        p = api.behavior_params(kind)
        assert {k: getattr(p, k) for k in bp.FIELDS} == bp.params(kind) and p.reserved == 0
    assert api.behavior_params(up_angle=45, look_steps=3).up_angle == 45.0 and api.behavior_params(look_steps=3).look_steps == 3
    with pytest.raises(ValueError):
        api.behavior_params("reckless")


def test_lane_keys_of_a_route():
    from emplanner_carla_amd import routing
    g = routing.RoadGraph(np.zeros((3, 3)) + np.arange(3)[:, None], [0, 1, 2, 2], [1, 2], [1, 2], [0, 2, 5], np.zeros((5, 3)))
    np.testing.assert_array_equal(g.edge_key, [0, 1])
    g.edge_key = np.array([routing.pack_lane_key(7, -2), routing.pack_lane_key(7, 3)], np.int32)
    r = routing.RouteResult(None, None, None, np.array([[0, 1, 2, 4, 0], [3, 0, 0, 0, 0]], np.int32), None, np.array([4, 1], np.int32))
    k = r.lane_key(g)
    assert k.dtype == np.int32 and k.tolist() == [[7 * 256 + 126] * 2 + [7 * 256 + 131] * 2 + [-1], [7 * 256 + 131] + [-1] * 4]
    with pytest.raises(ValueError):
        routing.pack_lane_key(1, 200)


# ---- live: the fixtures regenerate ----------------------------------------------------------------------------------------------------
def test_behavior_fixtures_regenerate_bit_for_bit(tmp_path):
    import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("the reference tree is not present")
    env = dict(os.environ, EMP_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_golden_behavior.py")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(GOLDEN, "behavior"))) == sorted(os.listdir(tmp_path / "behavior")) == sorted(n + ".npz" for n in NAMES)
    for name in NAMES:
        want, got = bc.fixture(name), np.load(tmp_path / "behavior" / (name + ".npz"))
        assert sorted(want) == sorted(got.files), name
        for k in want:
            a, b = want[k], got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{name}: {k}"
