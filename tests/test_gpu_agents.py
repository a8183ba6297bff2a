"""GPU suite of routed traffic.  emp_agent_control against tests/agent_port.py on identical inputs (the forward vector is data):
head, status, the longitudinal side and every steer that a limit binds bit for bit, what acos touches to 1e-12; emp_agent_observe
against the port; emp_agent_rollout against the chain of the 3 T separate calls BIT FOR BIT on every output and log row, and a
rollout cut in two; 64 agents round a corner against the CPU port loop; traffic alternating with emp_drive; hostile arguments in a
child process.

Set EMP_AGENT_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import agent_cases as ac
from tests import agent_port as ap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# One acos of at most a few ulp of pi (4e-16 each), times lat_K_P + lat_K_D / dt + lat_K_I * dt = 5.95, stays under 1e-13.
ACOS_TOL = 1e-12


def say(*a):
    if os.environ.get("EMP_AGENT_PRINT"):
        print(*a, flush=True)


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


def to_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def c_params(prm):
    from emplanner_carla_amd import api
    return api.agent_params(**prm)


def check_control(prm, b, got, want, what):
    """The rule of this file's docstring on one emp_agent_control result (arrays already on the host)."""
    for k in ("head", "status", "n_lon", "n_lat"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    ac.same_bits(got["lon_err"], want["lon_err"], f"{what}: the longitudinal deque, padding included")
    ac.same_bits(got["lon_command"], want["lon_command"], f"{what}: lon_command")
    ac.same_bits(got["control"][:, [0, 2]], want["control"][:, [0, 2]], f"{what}: throttle and brake")
    bound = ac.bound_mask(prm, b, want)
    ac.same_bits(got["control"][bound, 1], want["control"][bound, 1], f"{what}: a steer that a limit binds")
    ac.same_bits(got["past_steer"][bound], want["past_steer"][bound], f"{what}: past_steer where a limit binds")
    free = ~bound
    worst = [0.0]

    def near(g, w, name):
        nan = np.isnan(w)
        assert (np.isnan(g) == nan).all(), f"{what}: {name}: NaN in other places"
        d = np.abs(g[~nan] - w[~nan]).max() if (~nan).any() else 0.0
        worst[0] = max(worst[0], d)
        assert d <= ACOS_TOL, f"{what}: {name} differs by {d}"

    near(got["lat_error"], want["lat_error"], "lat_error")
    near(got["control"][free, 1], want["control"][free, 1], "the unbound steer")
    near(got["past_steer"][free], want["past_steer"][free], "past_steer")
    A = len(want["head"])
    newest = np.zeros((A, ap.BUFFER), bool)
    live = want["status"] == 0
    newest[np.arange(A)[live], want["n_lat"][live] - 1] = True
    ac.same_bits(got["lat_err"][~newest], want["lat_err"][~newest], f"{what}: the lateral deque but its newest entry, padding included")
    near(got["lat_err"][newest], want["lat_err"][newest], "the newest lateral entry")
    return worst[0]


def gpu_control(pl, prm, b, dev=False, in_place=False):
    g = {k: (up(v) if dev else np.array(v, copy=True)) for k, v in b.items()}
    r = pl.agent_control(c_params(prm), *[g[k] for k in ac.KEYS], in_place=in_place)
    pl.synchronize()
    if in_place:
        for k in ac.STATE_OUT:
            assert getattr(r, k) is g[k], k
    out = {k: to_np(getattr(r, k)) for k in ("control", "status", "lat_error", "lon_command") + ac.STATE_OUT}
    for k in ("path", "state", "forward"):                       # inputs stay as they were, poison included
        ac.same_bits(to_np(g[k]), b[k], f"input {k}")
    return out


@pytest.mark.parametrize("max_path", [1, 8, 40])
@pytest.mark.parametrize("A", [1, 5, 64, 65, 4099])
def test_control_matches_the_port(pl, A, max_path):
    """Ragged n_path (0, 1, 2, beyond the row), deques of every length, NaN in every slot the rule must not read: separate outputs
    from host arrays, aliased outputs on device tensors."""
    b = ac.random_batch(A, max_path, seed=1000 * max_path + A)
    prm = ap.params()
    want = ac.port_control(prm, b)
    w1 = check_control(prm, b, gpu_control(pl, prm, b), want, f"A={A} max_path={max_path} host")
    w2 = check_control(prm, b, gpu_control(pl, prm, b, dev=True, in_place=True), want, f"A={A} max_path={max_path} device, in place")
    say(f"control A={A} max_path={max_path}: worst |GPU - port| in what acos touches {max(w1, w2):.3g}")
    if A >= 64 and max_path >= 8:
        bound = ac.bound_mask(prm, b, want)
        assert (want["status"] == ap.DONE).any() and (want["head"] > np.clip(b["head"], 0, None)).any() and bound.any() and (~bound).any()


def test_control_on_the_threshold_cases(pl):
    b, names = ac.edge_cases()
    prm = ap.params()
    want = ac.port_control(prm, b)
    for dev in (False, True):
        got = gpu_control(pl, prm, b, dev=dev, in_place=dev)
        for a, name in enumerate(names):
            one = lambda d: {k: v[a:a + 1] for k, v in d.items()}
            check_control(prm, one(b), one(got), one(want), name)


def test_observe_matches_the_port(pl):
    rng = np.random.default_rng(5)
    state = rng.uniform(-10, 10, (300, 6))
    state[:, 2] = rng.uniform(-7, 7, 300)
    state[0, 2], state[1, 2], state[2, 3] = 0.0, -0.0, 0.0
    want = ap.observe_batch(state)
    for dev in (False, True):
        r = pl.agent_observe(up(state) if dev else state)
        pl.synchronize()
        got = {k: to_np(getattr(r, k)) for k in ("forward", "speed_kmh", "actors")}
        for k in got:
            ac.same_bits(got[k][:2], want[k][:2], f"{k} at fi = 0 and -0.0")
            d = np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
            say(f"observe {k}: worst relative difference {d.max():.3g}")
            assert d.max() <= 1e-12, k
        ac.same_bits(got["actors"][:, :2], state[:, :2], "actors x, y")


# ---- the rollout against the chain -----------------------------------------------------------------------------------------------------
ROLL_OUT = ("state",) + ac.STATE_OUT + ("status", "done_tick", "actors", "log_state", "log_control", "log_head")


def chain(pl, prm, vp, b, T, every):
    """What a user of the three separate calls writes, on device tensors, everything in place."""
    g = {k: up(v) for k, v in b.items() if k not in ("forward", "speed_kmh")}
    A = len(b["head"])
    status, done = np.zeros(A, np.int32), np.full(A, -1, np.int32)
    logs = dict(log_state=[], log_control=[], log_head=[])
    for t in range(T):
        o = pl.agent_observe(g["state"])
        r = pl.agent_control(prm, g["path"], g["n_path"], g["state"], o.forward, o.speed_kmh, g["target_speed"], g["head"],
                             g["past_steer"], g["lon_err"], g["n_lon"], g["lat_err"], g["n_lat"], in_place=True)
        if t % every == 0:
            logs["log_state"].append(g["state"].clone())
            logs["log_control"].append(r.control)
            logs["log_head"].append(g["head"].clone())
        st = to_np(r.status)
        status |= st
        done = np.where((done < 0) & ((st & ap.DONE) != 0), t, done).astype(np.int32)
        pl.vehicle_step(vp, g["state"], r.control, in_place=True)
    out = {k: to_np(g[k]) for k in ("state",) + ac.STATE_OUT}
    out.update({k: np.stack([to_np(x) for x in v]) for k, v in logs.items()})
    out["status"], out["done_tick"] = status, done
    out["actors"] = to_np(pl.agent_observe(g["state"]).actors)
    return out


def run_rollout(pl, prm, vp, b, T, every, dev=True):
    g = {k: (up(v) if dev else np.array(v, copy=True)) for k, v in b.items() if k not in ("forward", "speed_kmh")}
    r = pl.agent_rollout(prm, vp, g["path"], g["n_path"], g["state"], g["target_speed"], g["head"], g["past_steer"], g["lon_err"],
                         g["n_lon"], g["lat_err"], g["n_lat"], T, log_every=every)
    pl.synchronize()
    return {k: to_np(getattr(r, k)) for k in ROLL_OUT}


@pytest.mark.parametrize("A", [1, 65, 4099])
@pytest.mark.parametrize("T", [1, 7, 300])
def test_rollout_equals_the_chain_bit_for_bit(pl, T, A):
    from emplanner_carla_amd import api
    b = ac.corner_fleet(A if A > 1 else 3)
    if A == 1:
        b = {k: v[1:2] for k, v in b.items()}
    prm, vp, every = api.agent_params(), api.agent_vehicle_params(), (1 if T <= 7 else 7)
    want = chain(pl, prm, vp, b, T, every)
    for dev in (True, False):
        got = run_rollout(pl, prm, vp, b, T, every, dev)
        for k in ROLL_OUT:
            ac.same_bits(got[k], want[k], f"{k} (device tensors {dev})")
    if A >= 65:
        assert (got["done_tick"] == 0).sum() >= A // 5 and (got["done_tick"] != 0).sum() > A // 2
        if T == 300:
            assert (got["done_tick"] > 0).any() and (np.abs(got["log_control"][..., 1]) > 0.2).any()


def test_rollout_cut_in_two_resumes_bit_for_bit(pl):
    from emplanner_carla_amd import api
    b = ac.corner_fleet(65)
    prm, vp = api.agent_params(), api.agent_vehicle_params()
    whole = run_rollout(pl, prm, vp, b, 300, 1)
    first = run_rollout(pl, prm, vp, b, 113, 1)
    b2 = dict(b)
    for k in ("state",) + ac.STATE_OUT:
        b2[k] = first[k]
    second = run_rollout(pl, prm, vp, b2, 187, 1)
    for k in ("state", "actors") + ac.STATE_OUT:
        ac.same_bits(second[k], whole[k], k)
    for k in ("log_state", "log_control", "log_head"):
        ac.same_bits(np.concatenate([first[k], second[k]]), whole[k], k)
    np.testing.assert_array_equal(first["status"] | second["status"], whole["status"])
    want = np.where(first["done_tick"] >= 0, first["done_tick"], np.where(second["done_tick"] >= 0, second["done_tick"] + 113, -1))
    np.testing.assert_array_equal(want, whole["done_tick"])
    assert (whole["done_tick"] > 113).any() and (whole["done_tick"] == 0).any()


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------------
def test_sixty_four_agents_round_the_corner_like_the_port(pl):
    """64 agents on rotated and translated copies of the short corner.  The agents' tick is 0.05 s, so the 57 m take about 200
    ticks at 20 km/h: T = 400 lets the slowest one (15 km/h) finish and brake to rest.  Every agent reaches DONE, and its worst
    distance to its polyline is the CPU port loop's to 0.05 m: steering differences of 1e-12 a tick cannot move a car by
    centimetres.  Measured on an MI355X: worst deviation difference and final-state difference - see DESIGN.md 3.11."""
    from emplanner_carla_amd import api
    A, T = 64, 400
    b = ac.corner_fleet(A, ragged=False)
    prm, vp = ap.params(), ap.vehicle_params()
    got = run_rollout(pl, api.agent_params(), api.agent_vehicle_params(), b, T, 1)
    assert (got["status"] == ap.DONE).all() and (got["done_tick"] > 100).all() and (got["head"] == b["n_path"]).all()
    worst_dev = worst_end = 0.0
    for a in range(A):
        S, _, _, ST, end = ap.rollout(prm, vp, b["path"][a], b["n_path"][a], b["state"][a], b["target_speed"][a], ap.Agent(), T)
        assert ST[-1] == ap.DONE
        xy = b["path"][a, :, :2]
        dev_port = ap.polyline_distance(xy, S[:, :2]).max()
        dev_gpu = ap.polyline_distance(xy, got["log_state"][:, a, :2]).max()
        worst_dev = max(worst_dev, abs(dev_gpu - dev_port))
        worst_end = max(worst_end, np.abs(got["state"][a] - end).max())
        assert dev_port > 0.3                        # the corner is cut: the comparison is not one of two zeros
    print(f"64 agents, T = {T}: worst |deviation GPU - deviation port| {worst_dev:.3g} m, worst final-state difference {worst_end:.3g}")
    assert worst_dev <= 0.05


def test_traffic_agents_surface(pl):
    """run_step + vehicle_step, tick by tick, is rollout; set_speed, done and actors."""
    from emplanner_carla_amd import api
    from emplanner_carla_amd.traffic import TrafficAgents
    b = ac.corner_fleet(9)
    one = TrafficAgents(pl, b["path"], b["n_path"], b["state"], b["target_speed"])
    two = TrafficAgents(pl, up(b["path"]), up(b["n_path"]), up(b["state"]), up(b["target_speed"]))
    assert one.vp.dt == 0.05 and one.vp.Cf == -148970.0 and one.state is not b["state"]
    for _ in range(5):
        ctl = one.run_step()
        pl.vehicle_step(one.vp, one.state, ctl, in_place=True)
    r = two.rollout(5, log_every=1)
    pl.synchronize()
    for k in ("state",) + ac.STATE_OUT:
        ac.same_bits(to_np(getattr(two, k)), getattr(one, k), k)
    ac.same_bits(to_np(two.actors()), to_np(r.actors), "actors")
    ac.same_bits(to_np(r.actors), one.actors(), "actors (host)")
    np.testing.assert_array_equal(to_np(two.done()), (to_np(two.status) & ap.DONE) != 0)
    np.testing.assert_array_equal(one.done(), (one.status & ap.DONE) != 0)
    assert one.done()[2] and not one.done()[0] and (to_np(r.done_tick)[b["n_path"] == 0] == 0).all()
    one.set_speed(12.5)
    two.set_speed(np.full(9, 12.5))
    assert (one.target_speed == 12.5).all() and (to_np(two.target_speed) == 12.5).all()
    assert api.agent_vehicle_params.__doc__ and "PHYSICAL" in api.agent_vehicle_params.__doc__


# ---- with the drive ----------------------------------------------------------------------------------------------------------------------
def test_traffic_alternates_with_the_drive(pl):
    """Two periods of drive(K=1) + TrafficAgents.rollout: the actors of period 2 are agent_observe of the agents' state (and the
    rollout's own actors output), and the drive's log_counts are tests/drive_port.py's on those actors."""
    from emplanner_carla_amd import api
    from emplanner_carla_amd.traffic import TrafficAgents
    from tests import drive_port
    from tests import test_gpu_drive as tgd
    B, T, law = 2, 5, "mpc"
    pr = tgd.params(law)
    f = tgd.fleet(B, T, pr["M"])
    # three agents per ego on straight routes: one ahead and moving (dynamic), one ahead and parked (static), one far away
    A = 3
    paths, state = np.zeros((A, 40, 4)), np.zeros((A, 6))
    rot = f["state"][0, 2]
    for a, (ahead, side, v) in enumerate(((30.0, 0.5, 6.0), (22.0, -1.0, 0.0), (400.0, 0.0, 5.0))):
        x0, y0 = tgd.at(f["state"][0, :2], rot, ahead, side)
        paths[a] = tgd.straight(rot, x0, y0, 40)
        state[a] = (x0, y0, rot, 0.0, 0.0, v)
    target = np.array([25.0, 0.0, 20.0])
    traffic = TrafficAgents(pl, up(paths), up(np.full(A, 40, np.int32)), up(state), up(target))
    ticks = round(T * pr["vp"].dt / traffic.vp.dt) or 1                      # the same span of time, at least one agent tick
    g = {k: up(v) for k, v in f.items()}
    seen = []
    for period in range(2):
        actors = traffic.actors()
        ac.same_bits(to_np(actors), to_np(pl.agent_observe(traffic.state).actors), "actors")
        fleet_actors = actors.reshape(1, A, 4).expand(B, A, 4).contiguous()
        n_act = up(np.full(B, A, np.int32))
        r = pl.drive(pr["p"], pr["q"], pr["sp"], api.drive_params(), pr["lat"], pr["pid"], pr["vp"], g["global_path"], g["n_global"],
                     g["state"], g["accel"], fleet_actors, n_act, g["pre_match_index"], g["track"], g["track_len"], g["held"],
                     g["target_speed"], 1, T, tgd.MAX_OBS, tgd.MAX_DYN, lateral=law)
        ro = traffic.rollout(ticks)
        pl.synchronize()
        ac.same_bits(to_np(ro.actors), to_np(pl.agent_observe(traffic.state).actors), "the rollout's actors output")
        want = [drive_port.request(to_np(r.log_state)[0, e], None, to_np(actors), A, tgd.MAX_OBS, tgd.MAX_DYN) for e in range(B)]
        np.testing.assert_array_equal(to_np(r.log_counts)[0], np.array([[w["n_obs"], w["n_dyn"]] for w in want]))
        seen.append(to_np(r.log_counts)[0, 0].tolist())
        for name in ("state", "accel", "pre_match_index", "track", "track_len", "held"):
            g[name] = getattr(r, name)
    say(f"drive with traffic: ego 0 (n_obs, n_dyn) per period {seen}")
    assert seen[0] == [1, 1], "ego 0 should see the parked agent as static and the moving one as dynamic"
    assert to_np(traffic.state)[0, 0] != state[0, 0] and to_np(traffic.head)[0] >= 0


# ---- hostile arguments --------------------------------------------------------------------------------------------------------------------
def test_hostile_arguments_in_a_child_process():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "agent_fuzz_child.py")], capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    assert run.returncode == 0 and "AGENT-FUZZ-OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    last = run.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 60 and int(last[3]) >= 45, last
