"""CPU suite of routed traffic: the Python port of the agents' law (tests/agent_port.py) against what the reference's LocalPlanner and
VehiclePIDController did, tick by tick, on the recorded closed loops of tests/golden/agents/; the g++ build of
csrc/emp_agent_core.h (tests/host_check/agent_check.cpp) bit for bit against the port - host acos is libm's, as Python's is - on
the fixtures, on hand-built threshold cases and on ragged random batches; that build as a sanitized program of its own; the ctypes
layout and prototypes; and - where the reference tree is present - every fixture regenerated bit for bit."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from tests import agent_cases as ac
from tests import agent_port as ap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "host_check", "agent_check.cpp")
sys.path.insert(0, GOLDEN)
import make_golden_agents as mk  # noqa: E402

NAMES = mk.NAMES
# The steer of the port against the reference's.  acos near d = 1 turns a last-bit difference in d (NumPy's dot / norm against
# scalar arithmetic) into about 1e-8 rad, so the bar is set by measurement: the worst difference over the fixtures is 1.46e-9
# (corner), the bar four times that.  Above 1e-6 rad it would be another law, not rounding.
STEER_MEASURED = 1.46e-9
STEER_BAR = 4 * STEER_MEASURED
STEER_CAP = 1e-6


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("agent_check") / "libagentcheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    p, i, d = C.c_void_p, C.c_int, C.c_double
    lib.ac_layout.restype = None
    lib.ac_layout.argtypes = [p, p]
    lib.ac_pid.restype = d
    lib.ac_pid.argtypes = [d, d, d, d, d, p, p]
    lib.ac_observe.restype = None
    lib.ac_observe.argtypes = [i] + [p] * 4
    lib.ac_control.restype = None
    lib.ac_control.argtypes = [C.POINTER(L.AgentParams), i, i] + [p] * 22
    lib.ac_rollout.restype = None
    lib.ac_rollout.argtypes = [C.POINTER(L.AgentParams), C.POINTER(L.VehicleParams), i, i, i, i, C.POINTER(L.AgentRolloutIO)]
    return lib


def c_params(prm):
    return L.AgentParams(*[float(prm[k]) for k in ap.DEFAULTS], 0)


def c_vehicle(vp):
    return L.VehicleParams(*[float(v) for v in vp], 0)


def host_control(lib, prm, b, aliased=False):
    """ac_control on a batch: a dict of its outputs (aliased: the agent state is updated where copies of the inputs live)."""
    A, M = b["path"].shape[:2]
    ins = {k: np.ascontiguousarray(b[k]).copy() for k in ac.KEYS}
    o = dict(control=np.full((A, 3), 7.0), status=np.full(A, 7, np.int32), lat_error=np.full(A, 7.0), lon_command=np.full(A, 7.0))
    for k in ac.STATE_OUT:
        o[k] = ins[k] if aliased else np.full_like(ins[k], 7)
    ptr = lambda a: a.ctypes.data
    lib.ac_control(C.byref(c_params(prm)), A, M, *[ptr(ins[k]) for k in ac.KEYS], ptr(o["control"]), ptr(o["status"]),
                   *[ptr(o[k]) for k in ac.STATE_OUT], ptr(o["lat_error"]), ptr(o["lon_command"]))
    return o


ALL_OUT = ("control", "status", "lat_error", "lon_command") + ac.STATE_OUT


# ---- the port against the reference ---------------------------------------------------------------------------------------------------
def replay(name):
    """The port on the recorded inputs of a fixture, with its own agent state: controls (T, 3), queue lengths (T,)."""
    f = ac.fixture(name)
    path = np.c_[f["xy"], np.zeros((len(f["xy"]), 2))]
    prm, ag, n = ap.params(), ap.Agent(), int(f["n_path"])
    ctl, queue = [], []
    for x, y, c, s, kmh in f["seen"]:
        r = ap.tick(prm, path, n, x, y, c, s, kmh, float(f["target_speed"]), ag)
        ctl.append(r["control"])
        queue.append(n - ag.head)
        assert (r["status"] == ap.DONE) == (queue[-1] == 0)
    return f, np.array(ctl).reshape(-1, 3), np.array(queue)


@pytest.mark.parametrize("name", NAMES)
def test_port_equals_the_recorded_reference_tick_by_tick(name):
    f, ctl, queue = replay(name)
    np.testing.assert_array_equal(queue, f["queue"], err_msg=f"{name}: head / DONE")
    d = np.abs(ctl - f["control"]).max(0) if len(ctl) else np.zeros(3)
    print(f"{name}: worst throttle / steer / brake difference {d[0]:.3g} / {d[1]:.3g} / {d[2]:.3g}")
    assert d[0] <= 1e-12 and d[2] <= 1e-12, f"{name}: throttle {d[0]}, brake {d[2]}"
    assert STEER_BAR <= STEER_CAP and d[1] <= STEER_BAR, f"{name}: steer differs by {d[1]}"


def test_the_steer_bar_is_the_measured_one():
    worst = max(np.abs(c[:, 1] - f["control"][:, 1]).max() for f, c, _ in (replay(n) for n in NAMES))
    print(f"worst steer difference over the fixtures: {worst:.4g}")
    assert STEER_MEASURED / 2 <= worst <= STEER_MEASURED, "the measured figure in this file and in DESIGN.md 3.11 is stale"


def test_fixtures_cover_what_they_are_for():
    done_at = {}
    for name in NAMES:
        f = ac.fixture(name)
        q = f["queue"]
        assert (q == 0).any() and f["state_end"][5] == 0.0, f"{name}: the agent does not empty its queue and brake to rest"
        assert (np.diff(q) <= 0).all()
        done_at[name] = int(np.argmax(q == 0))
    assert done_at["empty"] == 0 and int(ac.fixture("empty")["n_path"]) == 0 and int(ac.fixture("one_waypoint")["n_path"]) == 1
    f = ac.fixture("corner")
    live = f["seen"][:done_at["corner"], :2]
    dev = ap.polyline_distance(f["xy"], live).max()
    assert 1.0 < dev < 2.5, f"corner: worst deviation {dev} m (pursuit-style corner cutting at about 5.8 m look-ahead)"
    assert np.abs(f["control"][:, 1]).max() > 0.3 and (f["control"][:, 2] > 0).any() and (f["control"][:, 0] == 0.75).any()
    steer = ac.fixture("behind")["control"][:, 1]
    assert (np.abs(np.diff(steer)).max() <= 0.1 + 1e-15) and np.isclose(np.abs(np.diff(steer)).max(), 0.1)      # the rate limit binds
    assert sum(os.path.getsize(os.path.join(ac.GOLDEN, n + ".npz")) for n in NAMES) < 400 * 1024


# ---- the core, compiled with g++ ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_core_equals_the_port_on_the_recorded_inputs(lib, name):
    """One agent, every tick a call, the agent state carried in place: every output to the bit."""
    f = ac.fixture(name)
    M = max(len(f["xy"]), 1)
    b = ac.blank(1, M)
    b["path"][0, :len(f["xy"]), :2] = f["xy"]
    b["n_path"][0] = int(f["n_path"])
    b["target_speed"][0] = float(f["target_speed"])
    prm, ag = ap.params(), ap.Agent()
    for t, (x, y, c, s, kmh) in enumerate(f["seen"][::1 if len(f["seen"]) < 450 else 2]):
        b["state"][0, :2], b["forward"][0], b["speed_kmh"][0] = (x, y), (c, s), kmh
        r = ap.tick(prm, b["path"][0], b["n_path"][0], x, y, c, s, kmh, b["target_speed"][0], ag)
        o = host_control(lib, prm, b)
        ac.same_bits(o["control"][0], np.array(r["control"]), f"{name} tick {t}: control")
        assert o["status"][0] == r["status"] and o["head"][0] == ag.head and o["n_lon"][0] == len(ag.lon) and o["n_lat"][0] == len(ag.lat)
        ac.same_bits(o["lon_err"][0, :len(ag.lon)], np.array(ag.lon), f"{name} tick {t}: lon deque")
        ac.same_bits(o["lat_err"][0, :len(ag.lat)], np.array(ag.lat), f"{name} tick {t}: lat deque")
        ac.same_bits(o["lat_error"], np.array([r["lat_error"]]), f"{name} tick {t}: lat_error")
        for k in ac.STATE_OUT:
            b[k] = o[k]


def test_core_on_the_threshold_cases(lib):
    b, names = ac.edge_cases()
    prm = ap.params()
    want = ac.port_control(prm, b)
    for aliased in (False, True):
        got = host_control(lib, prm, b, aliased)
        for a, name in enumerate(names):
            for k in ALL_OUT:
                ac.same_bits(got[k][a], want[k][a], f"{name} (aliased {aliased}): {k}")
    w = dict(zip(names, range(len(names))))
    st, ctl, head = want["status"], want["control"], want["head"]
    # what each case is for did happen
    assert head[w["dist == md"]] == 0 and head[w["dist one ulp below md"]] == 1 and head[w["dist one ulp above md"]] == 0
    assert head[w["three purged in one tick"]] == 3 and st[w["three purged in one tick"]] == 0
    assert st[w["last waypoint at 1 m stays"]] == 0 and st[w["last waypoint below 1 m goes: DONE"]] == ap.DONE
    assert head[w["last waypoint within md but beyond 1 m stays"]] == 1 and st[w["both purged: DONE"]] == ap.DONE
    for name in ("both purged: DONE", "no plan: DONE", "head already at the end: DONE", "n_path negative: DONE", "head beyond n_path: DONE"):
        a = w[name]
        assert st[a] == ap.DONE and tuple(ctl[a]) == (0.0, 0.0, 1.0) and want["past_steer"][a] == b["past_steer"][a]
        assert want["n_lon"][a] == min(max(b["n_lon"][a], 0), 10) and want["n_lat"][a] == min(max(b["n_lat"][a], 0), 10)
    assert want["lat_error"][w["nn == 0 by a zero forward vector"]] == 1.0
    assert want["lat_error"][w["nn == 0 on the waypoint (a NaN speed stops the purge)"]] == 1.0
    assert want["lat_error"][w["straight ahead"]] == 0.0 and want["lat_error"][w["straight behind"]] == np.pi
    assert want["lat_error"][w["to the right: negated"]] < 0 < want["lat_error"][w["to the left"]]
    assert want["lat_error"][w["quotient above +1 before the clip"]] == 0.0 and abs(want["lat_error"][w["quotient below -1 before the clip"]]) == np.pi
    assert ctl[w["rate limit binds alone (up)"], 1] == -0.5 + 0.1 and ctl[w["rate limit binds alone (down)"], 1] == 0.5 - 0.1
    assert ctl[w["max_steer binds alone"], 1] == 0.8 and ctl[w["-max_steer binds alone"], 1] == -0.8
    assert ctl[w["both bind"], 1] == 0.8 and ctl[w["both bind (negative)"], 1] == -0.8
    assert 0 < ctl[w["neither binds"], 1] < 0.1
    assert ctl[w["throttle limited"], 0] == 0.75 and 0 < ctl[w["throttle unlimited"], 0] < 0.75
    assert ctl[w["brake limited"], 2] == 0.3 and 0 < ctl[w["brake unlimited"], 2] < 0.3
    assert tuple(ctl[w["acc == 0 takes the throttle branch"]][[0, 2]]) == (0.0, 0.0)
    assert ctl[w["NaN c"], 1] == -0.8 and ctl[w["NaN s"], 1] == -0.8               # Python's max keeps -max_steer against a NaN
    assert ctl[w["NaN past_steer"], 1] == 0.0                                       # a NaN limit compares false: no rate limit
    assert ctl[w["NaN speed"], 0] == 0.0 and np.isnan(ctl[w["NaN speed"], 2]) and np.isnan(ctl[w["NaN target"], 2])
    assert head[w["NaN x"]] == 0 and st[w["NaN x"]] == 0 and head[w["NaN waypoint y behind a purged one"]] == 1
    assert want["n_lon"][w["n_lon = -3, n_lat = 99"]] == 1 and want["n_lat"][w["n_lon = -3, n_lat = 99"]] == 10
    assert head[w["n_path beyond the row"]] == 0 and st[w["n_path beyond the row"]] == 0 and head[w["head negative"]] == 0
    assert [want["n_lon"][w[f"deques of {n}"]] for n in (0, 1, 9, 10)] == [1, 2, 10, 10]


@pytest.mark.parametrize("A,max_path", ((1, 1), (5, 8), (65, 40), (300, 8)))
def test_core_on_ragged_batches_with_poisoned_padding(lib, A, max_path):
    b = ac.random_batch(A, max_path, seed=A * 100 + max_path)
    prm = ap.params()
    want = ac.port_control(prm, b)
    for aliased in (False, True):
        got = host_control(lib, prm, b, aliased)
        for k in ALL_OUT:
            if k in ("lon_err", "lat_err") and not aliased:
                live = np.arange(ap.BUFFER)[None, :] < want["n_" + k[:3]][:, None]
                ac.same_bits(got[k][live], want[k][live], f"{k} (live entries)")
                ac.same_bits(got[k][~live], b[k][~live], f"{k}: entries at and past the count pass through")
            else:
                ac.same_bits(got[k], want[k], f"{k} (aliased {aliased})")
    if A >= 65:
        assert (want["status"] == ap.DONE).any() and (want["status"] == 0).any() and (want["head"] > b["head"]).any()
        assert ac.bound_mask(prm, b, want).any() and not ac.bound_mask(prm, b, want).all()


def test_pid_alone_matches_the_reference_class(lib):
    """agt::pid10 against the port's pid on a long signal through a deque that fills, with both gain sets."""
    rng = np.random.default_rng(3)
    for kp, ki, kd in ((1.95, 0.05, 0.2), (1.0, 0.05, 0.0)):
        buf, n, pybuf = np.full(ap.BUFFER, np.nan), C.c_int(0), []
        for e in rng.uniform(-0.4, 0.4, 40):
            got = lib.ac_pid(kp, ki, kd, 0.05, float(e), buf.ctypes.data, C.byref(n))
            want, pybuf = ap.pid(kp, ki, kd, 0.05, float(e), pybuf)
            assert got == want and n.value == len(pybuf) and list(buf[:n.value]) == pybuf


def test_observe_equals_the_port(lib):
    rng = np.random.default_rng(5)
    state = rng.uniform(-10, 10, (40, 6))
    state[0, 2], state[1, 2], state[2, 2:] = 0.0, -0.0, (np.nan, 1.0, 0.0, 2.0)
    want = ap.observe_batch(state)
    fw, kmh, act = np.zeros((40, 2)), np.zeros(40), np.zeros((40, 4))
    lib.ac_observe(40, state.ctypes.data, fw.ctypes.data, kmh.ctypes.data, act.ctypes.data)
    for got, k in ((fw, "forward"), (kmh, "speed_kmh"), (act, "actors")):
        ac.same_bits(got, want[k], k)
    assert tuple(fw[0]) == (1.0, 0.0) and kmh[0] == 3.6 * np.sqrt((act[0, 2] ** 2 + act[0, 3] ** 2))


def host_rollout(lib, prm, vp, b, T, log_every):
    A, M = b["path"].shape[:2]
    n_log = (T + log_every - 1) // log_every
    keep = {k: np.ascontiguousarray(b[k]).copy() for k in ac.KEYS if k not in ("forward", "speed_kmh")}
    o = dict(state=np.zeros((A, 6)), status=np.zeros(A, np.int32), done_tick=np.zeros(A, np.int32), actors=np.zeros((A, 4)),
             log_state=np.zeros((n_log, A, 6)), log_control=np.zeros((n_log, A, 3)), log_head=np.zeros((n_log, A), np.int32))
    for k in ac.STATE_OUT:
        o[k] = np.zeros_like(keep[k])
    io = L.AgentRolloutIO()
    for k in ("path", "n_path", "state", "target_speed") + ac.STATE_OUT:
        setattr(io, k, keep[k].ctypes.data)
    io.state_out = o["state"].ctypes.data
    for k in ac.STATE_OUT:
        setattr(io, k + "_out", o[k].ctypes.data)
    io.status, io.done_tick, io.actors_out = o["status"].ctypes.data, o["done_tick"].ctypes.data, o["actors"].ctypes.data
    io.log_state, io.log_control, io.log_head = o["log_state"].ctypes.data, o["log_control"].ctypes.data, o["log_head"].ctypes.data
    lib.ac_rollout(C.byref(c_params(prm)), C.byref(c_vehicle(vp)), A, M, T, log_every, C.byref(io))
    return o


def test_core_rollout_equals_the_port_loop(lib):
    """The kernel's loop on the CPU against the port's, on the fixtures' scenarios side by side: states, heads, controls, the first
    DONE tick - bit for bit, since libm is the same."""
    names = [n for n in NAMES]
    scs = [mk.scenario(n) for n in names]
    A, M, T, every = len(names), max(max(len(s["xy"]) for s in scs), 1), 230, 3
    b = ac.blank(A, M)
    b["lon_err"][:], b["lat_err"][:] = 0.0, 0.0
    for a, s in enumerate(scs):
        b["path"][a, :len(s["xy"]), :2] = s["xy"]
        b["n_path"][a], b["state"][a], b["target_speed"][a] = len(s["xy"]), s["state0"], s["target_speed"]
    prm, vp = ap.params(), ap.vehicle_params()
    got = host_rollout(lib, prm, vp, b, T, every)
    for a, name in enumerate(names):
        ag = ap.Agent()
        S, U, H, ST, end = ap.rollout(prm, vp, b["path"][a], b["n_path"][a], b["state"][a], b["target_speed"][a], ag, T)
        ac.same_bits(got["state"][a], end, f"{name}: final state")
        ac.same_bits(got["log_state"][:, a], S[::every], f"{name}: log_state")
        ac.same_bits(got["log_control"][:, a], U[::every], f"{name}: log_control")
        np.testing.assert_array_equal(got["log_head"][:, a], H[::every])
        assert got["done_tick"][a] == (int(np.argmax(ST == ap.DONE)) if (ST == ap.DONE).any() else -1) and got["status"][a] == int(np.bitwise_or.reduce(ST))
        assert got["head"][a] == ag.head and got["past_steer"][a] == ag.past_steer
        ac.same_bits(got["lon_err"][a, :len(ag.lon)], np.array(ag.lon), f"{name}: lon deque")
        ac.same_bits(got["actors"][a], np.array(ap.observe(end)[2]), f"{name}: actors")
        f = ac.fixture(name)                      # and the recording itself, as far as it goes: the same closed loop
        n = min(T, len(f["seen"]))
        assert np.abs(S[:n, :2] - f["seen"][:n, :2]).max() < 1e-6, f"{name}: the port's closed loop leaves the recorded one"
    assert (got["done_tick"] == 0).sum() == 1 and (got["done_tick"] > 0).sum() >= 3 and (got["done_tick"] == -1).any()


def test_agent_check_as_a_program_of_its_own(tmp_path):
    """-DAGENT_CHECK_MAIN: the self-checking program a sanitizer build runs (here: address and undefined behaviour, on the CPU)."""
    exe = str(tmp_path / "agent_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DAGENT_CHECK_MAIN", SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "agent_check: 0 bad, 0 wrong" in run.stdout, run.stdout + run.stderr[-2000:]


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts(lib):
    p, r = np.zeros(13, np.int64), np.zeros(25, np.int64)
    lib.ac_layout(p.ctypes.data, r.ctypes.data)
    for got, cls, n in ((p, L.AgentParams, 12), (r, L.AgentRolloutIO, 24)):
        assert list(got) == [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_] and len(cls._fields_) == n
    assert [n for n, _ in L.AgentParams._fields_] == list(ap.DEFAULTS) + ["reserved"]
    assert [n for n, _ in L.AgentRolloutIO._fields_] == [
        "path", "n_path", "state", "target_speed", "head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat", "state_out", "head_out",
        "past_steer_out", "lon_err_out", "n_lon_out", "lat_err_out", "n_lat_out", "status", "done_tick", "actors_out", "log_state",
        "log_control", "log_head", "reserved"]


def test_binding_speaks_the_header():
    text = open(os.path.join(ROOT, "include", "emplanner.h")).read()
    assert f"#define EMP_AGENT_BUFFER {L.AGENT_BUFFER}\n" in text and f"#define EMP_AGT_DONE {L.AGT_DONE}\n" in text
    assert "#define EMP_ABI_VERSION 13\n" in text and L.ABI_VERSION == 13
    assert (ap.BUFFER, ap.DONE) == (L.AGENT_BUFFER, L.AGT_DONE)
    assert len(L.PROTOTYPES["emp_agent_observe"][1]) == 7 and len(L.PROTOTYPES["emp_agent_control"][1]) == 27
    assert len(L.PROTOTYPES["emp_agent_rollout"][1]) == 9 and L.PROTOTYPES["emp_agent_params_default"][0] is None
    for name in ("emp_agent_params_default", "emp_agent_observe", "emp_agent_control", "emp_agent_rollout"):
        assert f" {name}(" in text
    from emplanner_carla_amd import api
    p = api.agent_params()
    assert [getattr(p, k) for k in ap.DEFAULTS] == list(ap.DEFAULTS.values()) and p.reserved == 0
    vp = api.agent_vehicle_params()
    assert (vp.a, vp.b, vp.Cf, vp.Cr, vp.m, vp.Iz, vp.dt) == ap.VEHICLE_PARA + (0.05,) and ap.vehicle_params()[:7] == ap.VEHICLE_PARA + (0.05,)


# ---- live: the fixtures regenerate ----------------------------------------------------------------------------------------------------
def test_agent_fixtures_regenerate_bit_for_bit(tmp_path):
    import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("the reference tree is not present")
    env = dict(os.environ, EMP_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_golden_agents.py")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert sorted(os.listdir(ac.GOLDEN)) == sorted(os.listdir(tmp_path / "agents")) == sorted(n + ".npz" for n in NAMES)
    for name in NAMES:
        want, got = ac.fixture(name), np.load(tmp_path / "agents" / (name + ".npz"))
        assert sorted(want.files) == sorted(got.files), name
        for k in want.files:
            a, b = want[k], got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{name}: {k}"
