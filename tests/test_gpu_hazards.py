"""GPU suite of the hazard rule (red lights and pedestrians in front of the car-following law).  emp_agent_behave_hazards against
tests/hazard_port.py on the seeded batches of tests/hazard_cases.py (the CPU suite asserts what they cover): every integer output,
last_light, the longitudinal side and every distance bit for bit, what acos touches to 1e-12, padding slots untouched; without
lights and walkers both new calls against emp_agent_behave / emp_traffic_rollout bit for bit; emp_traffic_rollout_hazards against
the chain of the 3 T separate calls BIT FOR BIT on every output and log row, and against itself cut in two while a light holds an
agent; four recorded scenarios for 600 ticks in one launch; refused arguments; BehaviorTraffic with set_lights / set_walkers.

Set EMP_AGENT_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import agent_port as ap
from tests import behavior_cases as bc
from tests import behavior_port as bp
from tests import hazard_cases as hc
from tests import hazard_port as hp
from tests.test_gpu_behavior import ACOS_TOL, MARGIN, c_params, others_of, say, to_np, up
from tests.test_gpu_behavior import gpu_behave as behavior_behave, run_rollout as behavior_rollout

pytestmark = pytest.mark.gpu

# Final states of 600 closed-loop ticks, GPU against the CPU port loop.  Measured on an MI355X: FINAL_MEASURED (red_light, sticky,
# walker_crossing, queue_at_light; steering differences of 1e-16 a tick, integrated); the bar is four times that, and above 1e-6 it
# would be another trajectory.
FINAL_MEASURED = 2.2e-12
FINAL_BAR = 4 * FINAL_MEASURED
FINAL_CAP = 1e-6
EMP_OK, EMP_ERR_INVALID = 0, -1        # include/emplanner.h
BEHAVE_OUT = bc.STATE_OUT + ("status", "control", "mode", "blocker", "distance", "ttc", "lat_error", "lon_command") + hc.HAZARD_OUT
ROLL_OUT = ("state",) + bc.STATE_OUT + ("status", "done_tick", "mode_ticks", "min_gap", "actors", "log_state", "log_control", "log_head", "log_mode",
                                        "log_target", "last_light", "cause_ticks", "min_walker_gap", "log_cause")


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


def hparams():
    from emplanner_carla_amd import api
    return api.hazard_params()


def lights_of(g):
    return (g["n_light"], g["light"], g["light_lane"], g["light_cycle"]) if g["light"].shape[1] else None


def walkers_of(g):
    return (g["n_walker"], g["walker"], g["walker_lane"]) if g["walker"].shape[1] else None


def gpu_behave(pl, b, tick0, dev):
    """emp_agent_behave_hazards on host arrays (new outputs) or on device tensors in place."""
    prm, prb, _ = c_params()
    g = {k: (up(v) if dev else np.array(v, copy=True)) for k, v in b.items()}
    r = pl.agent_behave_hazards(prm, prb, hparams(), g["n_world"], g["path"], g["n_path"], g["lane"], g["state"], g["forward"], g["speed_kmh"],
                                g["speed_limit"], g["extent"], *[g[k] for k in bc.STATE_OUT], g["last_light"], lights=lights_of(g),
                                walkers=walkers_of(g), others=others_of(g), tick0=tick0, in_place=dev)
    pl.synchronize()
    out = {k: to_np(getattr(r, k)) for k in BEHAVE_OUT}
    out["target_speed_out"] = to_np(r.target_speed)
    if dev:
        for k in bc.STATE_OUT + ("last_light",):
            assert getattr(r, k) is g[k], k
    for k in ("path", "state", "forward", "lane", "other", "light", "light_cycle", "walker"):      # inputs stay as they were, poison included
        hc.same_bits(to_np(g[k]), b[k], f"input {k}")
    return out


def check_behave(b, got, want, what, dev):
    """The rule of this file's docstring on one result; returns (rows left out, worst difference in what acos touches)."""
    live = hc.live_mask(b)
    keep = live & ~(want["margin"] < MARGIN)
    for k in ("mode", "blocker", "head", "status", "n_lon", "n_lat", "last_light", "cause", "light_hit", "walker_hit"):
        np.testing.assert_array_equal(got[k][keep], want[k][keep], err_msg=f"{what}: {k}")
    for k in ("target_speed_out", "distance", "ttc", "lon_command", "lon_err", "walker_distance"):
        hc.same_bits(got[k][keep], want[k][keep], f"{what}: {k}")
    hc.same_bits(got["control"][keep][:, [0, 2]], want["control"][keep][:, [0, 2]], f"{what}: throttle and brake")
    em = keep & (want["mode"] == bp.EMERGENCY)
    for k in ("control", "past_steer", "lat_err", "lat_error"):
        hc.same_bits(got[k][em], want[k][em], f"{what}: {k} of an emergency row")
    worst = 0.0
    for k in ("lat_error", "past_steer", "lat_err", "control"):
        g, w = got[k][keep], want[k][keep]
        nan = np.isnan(w)
        assert (np.isnan(g) == nan).all(), f"{what}: {k}: NaN in other places"
        d = np.abs(g[~nan] - w[~nan]).max() if (~nan).any() else 0.0
        worst = max(worst, d)
        assert d <= ACOS_TOL, f"{what}: {k} differs by {d}"
    # padding slots: untouched in device memory, 0 in arrays that were staged
    for k in bc.STATE_OUT + bc.TICK_OUT + hc.HAZARD_OUT:
        pad = got[k][~live]
        if dev and k in bc.STATE_OUT + ("last_light",):
            hc.same_bits(pad, b[k][~live], f"{what}: padding of {k}")
        elif not dev:
            assert not pad.size or (pad == 0).all(), f"{what}: padding of {k} (staged)"
    return int((live & ~keep).sum()), worst


def test_behave_hazards_matches_the_port(pl):
    """Twelve batches of five worlds: 1, 2, 3, 64 and 7 agents with 0, 1, 64, 5 and 2 lights, 0, 64, 1, 3 and 9 walkers and up to 3
    others; host arrays, and device tensors updated in place."""
    prm, prb, hpp = ap.params(), bp.params(), hp.params()
    left = rows = 0
    worst = 0.0
    causes = np.zeros(4, int)
    for k in range(hc.BATCHES):
        b, tick0 = hc.gpu_batch(k)
        want = hc.port_behave(prm, prb, hpp, b, tick0)
        live = hc.live_mask(b)
        for dev in (False, True):
            n, w = check_behave(b, gpu_behave(pl, b, tick0, dev), want, f"batch {k} device {dev}", dev)
            worst = max(worst, w)
        left, rows = left + n, rows + int(live.sum())
        causes += np.bincount(want["cause"][live & ~(want["margin"] < MARGIN)], minlength=4)
    say(f"behave_hazards: {rows} rows, {left} left out, causes (none, light, walker, vehicle) {causes.tolist()}, worst |GPU - port| in what "
        f"acos touches {worst:.3g}")
    assert left <= rows // 100 and causes.min() >= 20, (left, rows, causes)


def test_behave_hazards_on_the_threshold_cases(pl):
    b, names, tick0 = hc.edge_cases()
    prm, prb, hpp = ap.params(), bp.params(), hp.params()
    for t0 in sorted(set(tick0)):
        want = hc.port_behave(prm, prb, hpp, b, t0)
        got = gpu_behave(pl, b, t0, True)
        # the cases just inside and outside a cone leave a margin of 1e-6 degrees: only rows on an exact acos tie may differ
        keep = hc.live_mask(b) & ~(want["margin"] < 1e-12)
        for k in ("mode", "cause", "light_hit", "walker_hit", "last_light", "blocker", "status", "head", "n_lon"):
            np.testing.assert_array_equal(got[k][keep], want[k][keep], err_msg=f"tick0 {t0}: {k}")
        for k in ("distance", "ttc", "target_speed_out", "walker_distance"):
            hc.same_bits(got[k][keep], want[k][keep], f"tick0 {t0}: {k}")


# ---- without lights and walkers: the existing calls ---------------------------------------------------------------------------------------
def no_hazards(b, rows):
    """The batch with n_light = n_walker = 0 in every world (rows: keep the poisoned arrays, or none at all)."""
    b = dict(b, n_light=np.zeros_like(b["n_light"]), n_walker=np.zeros_like(b["n_walker"]))
    if not rows:
        b.update(light=b["light"][:, :0], light_lane=b["light_lane"][:, :0], light_cycle=b["light_cycle"][:, :0], walker=b["walker"][:, :0],
                 walker_lane=b["walker_lane"][:, :0])
    return b


@pytest.mark.parametrize("rows", (True, False))
def test_without_hazards_behave_is_emp_agent_behave(pl, rows):
    b, tick0 = hc.gpu_batch(3)
    live = hc.live_mask(b)
    base = {k: v for k, v in b.items() if k not in hc.HAZARD_IN}
    want = behavior_behave(pl, base, tick0, True)
    got = gpu_behave(pl, no_hazards(b, rows), tick0, True)
    for k in want:
        hc.same_bits(got[k][live], want[k][live], k)
    assert set(np.unique(got["cause"][live])) == {hp.HZ_NONE, hp.HZ_VEHICLE}
    np.testing.assert_array_equal(got["cause"][live] == hp.HZ_VEHICLE, want["mode"][live] == bp.EMERGENCY)
    assert (got["light_hit"][live] == -1).all() and (got["walker_hit"][live] == -1).all() and np.isinf(got["walker_distance"][live]).all()
    assert (got["last_light"][live & (want["mode"] != bp.DONE)] == -1).all()


# ---- the rollout ------------------------------------------------------------------------------------------------------------------------
ROLL_SIZES, ROLL_LIGHTS, ROLL_WALKERS, ROLL_TICK0, ROLL_SEED = (2, 64, 5), (3, 64, 5), (4, 9, 64), 3, 4


@pytest.fixture(scope="module")
def traffic_batch():
    """3 worlds of 2, 64 and 5 agents with others, lights whose phase changes inside 120 ticks and walkers that cross."""
    b = bc.random_worlds(ROLL_SIZES, 64, 3, 40, seed=ROLL_SEED)
    return hc.add_hazards(b, ROLL_LIGHTS, ROLL_WALKERS, 64, 64, ROLL_TICK0 + 40, np.random.default_rng(ROLL_SEED))


def chain(pl, b, T, every, tick0=0):
    """3 T launches on device tensors, updated in place: what emp_traffic_rollout_hazards promises to equal."""
    prm, prb, vp = c_params()
    hpp = hparams()
    g = {k: up(v) for k, v in b.items()}
    W, n = b["n_path"].shape
    flat = lambda x: x.reshape((W * n,) + tuple(x.shape[2:]))
    status, done = np.zeros((W, n), np.int32), np.full((W, n), -1, np.int32)
    ticks, gap, causes, wgap = np.zeros((W, n, 5), np.int32), np.full((W, n), np.inf), np.zeros((W, n, 3), np.int32), np.full((W, n), np.inf)
    logs = dict(log_state=[], log_control=[], log_head=[], log_mode=[], log_target=[], log_cause=[])
    for t in range(T):
        o = pl.agent_observe(flat(g["state"]))
        r = pl.agent_behave_hazards(prm, prb, hpp, g["n_world"], g["path"], g["n_path"], g["lane"], g["state"], o.forward.reshape(W, n, 2),
                                    o.speed_kmh.reshape(W, n), g["speed_limit"], g["extent"], *[g[k] for k in bc.STATE_OUT], g["last_light"],
                                    lights=lights_of(g), walkers=walkers_of(g), others=others_of(g), tick0=tick0 + t, in_place=True)
        if t % every == 0:
            logs["log_state"].append(g["state"].clone())
            logs["log_control"].append(r.control)
            logs["log_head"].append(g["head"].clone())
            logs["log_mode"].append(r.mode)
            logs["log_target"].append(r.target_speed)
            logs["log_cause"].append(r.cause)
        st, mode, blk, dist = to_np(r.status), to_np(r.mode), to_np(r.blocker), to_np(r.distance)
        cause, whit, wd = to_np(r.cause), to_np(r.walker_hit), to_np(r.walker_distance)
        status |= st
        done = np.where((done < 0) & ((st & ap.DONE) != 0), t, done).astype(np.int32)
        for m in range(5):
            ticks[..., m] += mode == m
        for m in range(3):
            causes[..., m] += cause == m + 1
        gap = np.where((blk >= 0) & (dist < gap), dist, gap)
        wgap = np.where((whit >= 0) & (wd < wgap), wd, wgap)
        pl.vehicle_step(vp, flat(g["state"]), flat(r.control), in_place=True)
    out = {k: to_np(g[k]) for k in ("state",) + bc.STATE_OUT + ("last_light",)}
    out.update({k: np.stack([to_np(x) for x in v]) for k, v in logs.items()})
    out.update(status=status, done_tick=done, mode_ticks=ticks, min_gap=gap, cause_ticks=causes, min_walker_gap=wgap)
    out["actors"] = to_np(pl.agent_observe(flat(g["state"])).actors).reshape(W, n, 4)
    return out


def run_rollout(pl, b, T, every, tick0=0, dev=True):
    prm, prb, vp = c_params()
    g = {k: (up(v) if dev else np.array(v, copy=True)) for k, v in b.items() if k not in ("forward", "speed_kmh")}
    r = pl.traffic_rollout_hazards(prm, prb, hparams(), vp, g["n_world"], g["path"], g["n_path"], g["lane"], g["state"], g["speed_limit"],
                                   g["extent"], *[g[k] for k in bc.STATE_OUT], g["last_light"], T, lights=lights_of(g), walkers=walkers_of(g),
                                   others=others_of(g), tick0=tick0, log_every=every)
    pl.synchronize()
    return {k: to_np(getattr(r, k)) for k in ROLL_OUT}


def live_only(b, out):
    """The live slots of every output (padding slots of fresh device outputs hold whatever the memory held)."""
    live = hc.live_mask(b)
    return {k: (v[:, live] if k.startswith("log_") else v[live]) for k, v in out.items()}


def test_rollout_equals_the_chain_bit_for_bit(pl, traffic_batch):
    b, T, every = traffic_batch, 120, 7
    want = live_only(b, chain(pl, b, T, every, tick0=ROLL_TICK0))
    for dev in (True, False):
        got = live_only(b, run_rollout(pl, b, T, every, tick0=ROLL_TICK0, dev=dev))
        for k in ROLL_OUT:
            hc.same_bits(got[k], want[k], f"{k} (device tensors {dev})")
    ticks, causes = want["mode_ticks"].sum(0), want["cause_ticks"].sum(0)
    say(f"rollout: mode ticks {ticks.tolist()}, cause ticks (light, walker, vehicle) {causes.tolist()}, finite walker gaps "
        f"{int(np.isfinite(want['min_walker_gap']).sum())}")
    assert (ticks > 0).all() and (causes > 0).all() and np.isfinite(want["min_walker_gap"]).any()
    # lights switch inside the window: some agent is held for a part of it only
    lt = want["cause_ticks"][:, 0]
    assert ((lt > 0) & (lt < T) & (want["done_tick"] < 0)).any()


def test_rollout_cut_in_two_resumes_bit_for_bit(pl, traffic_batch):
    b = traffic_batch
    whole = run_rollout(pl, b, 120, 1, tick0=ROLL_TICK0)
    first = run_rollout(pl, b, 50, 1, tick0=ROLL_TICK0)
    live = hc.live_mask(b)
    assert (first["last_light"][live] >= 0).any(), "no agent is held by a light at the cut"
    b2 = dict(b)
    for k in ("state",) + bc.STATE_OUT + ("last_light",):
        b2[k] = np.where(live.reshape(b["n_path"].shape + (1,) * (first[k].ndim - 2)), first[k], b[k])
    second = run_rollout(pl, b2, 70, 1, tick0=ROLL_TICK0 + 50)
    whole, first, second = live_only(b, whole), live_only(b, first), live_only(b, second)
    for k in ("state", "actors", "last_light") + bc.STATE_OUT:
        hc.same_bits(second[k], whole[k], k)
    for k in ("log_state", "log_control", "log_head", "log_mode", "log_target", "log_cause"):
        hc.same_bits(np.concatenate([first[k], second[k]]), whole[k], k)
    np.testing.assert_array_equal(first["mode_ticks"] + second["mode_ticks"], whole["mode_ticks"])
    np.testing.assert_array_equal(first["cause_ticks"] + second["cause_ticks"], whole["cause_ticks"])
    hc.same_bits(np.minimum(first["min_gap"], second["min_gap"]), whole["min_gap"], "min_gap")
    hc.same_bits(np.minimum(first["min_walker_gap"], second["min_walker_gap"]), whole["min_walker_gap"], "min_walker_gap")


def test_without_hazards_rollout_is_emp_traffic_rollout(pl, traffic_batch):
    b = traffic_batch
    base = {k: v for k, v in b.items() if k not in hc.HAZARD_IN}
    want = live_only(b, behavior_rollout(pl, base, 120, 7, tick0=ROLL_TICK0))
    got = live_only(b, run_rollout(pl, no_hazards(b, True), 120, 7, tick0=ROLL_TICK0))
    for k in want:
        hc.same_bits(got[k], want[k], k)
    assert (got["cause_ticks"][:, :2] == 0).all() and np.isinf(got["min_walker_gap"]).all()
    np.testing.assert_array_equal(got["cause_ticks"][:, 2], want["mode_ticks"][:, bp.EMERGENCY])
    assert set(np.unique(got["log_cause"])) <= {hp.HZ_NONE, hp.HZ_VEHICLE}
    np.testing.assert_array_equal(got["log_cause"] == hp.HZ_VEHICLE, want["log_mode"] == bp.EMERGENCY)


# ---- the scenarios of the fixtures --------------------------------------------------------------------------------------------------------
SCENARIOS = ("red_light", "sticky", "walker_crossing", "queue_at_light")


@pytest.fixture(scope="module")
def port_loops():
    out = {}
    for name in SCENARIOS:
        f, b = hc.fixture_world(name)
        T, V = f["queue"].shape
        out[name] = hp.rollout(ap.params(), bp.params(), hp.params(), ap.vehicle_params(), hc.world_of(b, 0, V), [ap.Agent() for _ in range(V)],
                               [-1] * V, T)
    return out


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario_on_the_device_like_the_recording(pl, port_loops, name):
    """600 ticks in one launch: the mode and cause of every tick are the recording's, the final state is the CPU port loop's to
    FINAL_BAR."""
    f, b = hc.fixture_world(name)
    T, V = f["queue"].shape
    assert T == 600
    got = run_rollout(pl, b, T, 1)
    want = port_loops[name]
    np.testing.assert_array_equal(got["log_mode"][:, 0], f["mode"], err_msg=f"{name}: the recorded modes")
    np.testing.assert_array_equal(got["log_cause"][:, 0], f["cause"], err_msg=f"{name}: the recorded causes")
    np.testing.assert_array_equal(got["log_head"][:, 0], want["head"])
    np.testing.assert_array_equal(got["cause_ticks"][0], f["cause_ticks"])
    np.testing.assert_array_equal(got["last_light"][0], f["last_light"][-1])
    d = np.abs(got["state"][0] - want["end"]).max()
    say(f"{name}: worst final-state difference GPU - port loop {d:.3g}")
    assert FINAL_BAR <= FINAL_CAP and d <= FINAL_BAR, f"{name}: final states differ by {d}"


def test_the_final_state_bar_is_the_measured_one(pl, port_loops):
    worst = 0.0
    for name in SCENARIOS:
        f, b = hc.fixture_world(name)
        worst = max(worst, np.abs(run_rollout(pl, b, 600, 600)["state"][0] - port_loops[name]["end"]).max())
    print(f"worst final-state difference over {SCENARIOS}: {worst:.4g}")
    assert worst <= FINAL_MEASURED, "the measured figure in this file and in DESIGN.md 3.13 is stale"


# ---- refused arguments ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_invalid_and_leave_the_outputs_untouched(pl):
    """Raw calls on host arrays: every refusal of the launch plan, a NULL required pointer, a non-zero reserved and EMP_HOST_PINNED give
    EMP_ERR_INVALID before any launch, and every output still holds its 7s; W == 0 gives EMP_OK."""
    from emplanner_carla_amd import _lib as L
    lib, h = pl._lib, pl._h
    b, tick0 = hc.gpu_batch(0)
    W, N, M = b["lane"].shape
    K, ML, MW, T = b["other"].shape[1], 64, 64, 4
    prm, prb, vp = c_params()
    hpp = hparams()
    ins = {k: np.ascontiguousarray(v) for k, v in b.items()}
    outs = dict(head_out=np.full((W, N), 7, np.int32), past_steer_out=np.full((W, N), 7.0), lon_err_out=np.full((W, N, 10), 7.0),
                n_lon_out=np.full((W, N), 7, np.int32), lat_err_out=np.full((W, N, 10), 7.0), n_lat_out=np.full((W, N), 7, np.int32),
                status=np.full((W, N), 7, np.int32), control=np.full((W, N, 3), 7.0), mode=np.full((W, N), 7, np.int32),
                blocker=np.full((W, N), 7, np.int32), distance=np.full((W, N), 7.0), ttc=np.full((W, N), 7.0), target_speed_out=np.full((W, N), 7.0),
                state_out=np.full((W, N, 6), 7.0), done_tick=np.full((W, N), 7, np.int32), mode_ticks=np.full((W, N, 5), 7, np.int32),
                min_gap=np.full((W, N), 7.0), log_mode=np.full((T, W, N), 7, np.int32))
    houts = dict(last_light_out=np.full((W, N), 7, np.int32), cause=np.full((W, N), 7, np.int32), light_hit=np.full((W, N), 7, np.int32),
                 walker_hit=np.full((W, N), 7, np.int32), walker_distance=np.full((W, N), 7.0), cause_ticks=np.full((W, N, 3), 7, np.int32),
                 min_walker_gap=np.full((W, N), 7.0), log_cause=np.full((T, W, N), 7, np.int32))

    def blocks(io_kw=None, h_kw=None):
        io, hio = L.BehaviorIO(), L.HazardIO()
        for k in bc.IN_KEYS:
            setattr(io, k, ins[k].ctypes.data)
        for k, v in outs.items():
            setattr(io, k, v.ctypes.data)
        for k in hc.HAZARD_IN:
            setattr(hio, k, ins[k].ctypes.data)
        for k, v in houts.items():
            setattr(hio, k, v.ctypes.data)
        for blk, kw in ((io, io_kw), (hio, h_kw)):
            for k, v in (kw or {}).items():
                setattr(blk, k, v)
        return io, hio

    def call(which, w=W, n=N, m=M, k=K, ml=ML, mw=MW, t=T, every=1, t0=tick0, where=L.EMP_HOST, io_kw=None, h_kw=None, hp_=hpp, null_h=False):
        io, hio = blocks(io_kw, h_kw)
        tail = (C.byref(io), where, C.byref(hp_) if hp_ is not None else None, ml, mw, None if null_h else C.byref(hio))
        if which == "behave":
            return lib.emp_agent_behave_hazards(h, C.byref(prm), C.byref(prb), w, n, m, k, t0, *tail)
        return lib.emp_traffic_rollout_hazards(h, C.byref(prm), C.byref(prb), C.byref(vp), w, n, m, k, t, every, t0, *tail)

    bad_hp = type(hpp).from_buffer_copy(hpp)
    bad_hp.reserved = 1
    probes = 0
    for which in ("behave", "rollout"):
        for v in list(outs.values()) + list(houts.values()):
            v[...] = 7
        refused = [dict(ml=-1), dict(ml=65), dict(mw=-1), dict(mw=65), dict(n=0), dict(n=65), dict(k=-1), dict(k=65), dict(m=0), dict(w=-1),
                   dict(t0=-1), dict(where=L.EMP_HOST_PINNED), dict(hp_=None), dict(null_h=True), dict(hp_=bad_hp), dict(h_kw=dict(reserved=1)),
                   dict(io_kw=dict(reserved=1)), dict(w=0, ml=65)]
        required = ("last_light", "last_light_out") + (("cause", "light_hit", "walker_hit", "walker_distance") if which == "behave"
                                                       else ("cause_ticks", "min_walker_gap"))
        refused += [dict(h_kw={k: None}) for k in required + ("n_light", "light", "light_lane", "light_cycle", "n_walker", "walker", "walker_lane")]
        refused += [dict(io_kw={k: None}) for k in ("n_world", "lane", "head_out", "status")]
        if which == "rollout":
            refused += [dict(t=0), dict(t=65537), dict(every=0), dict(t0=2 ** 31 - 3)]
        for kw in refused:
            rc = call(which, **kw)
            assert rc == EMP_ERR_INVALID, (which, kw, rc)
            assert lib.emp_last_error(h), (which, kw)
            probes += 1
        for k, v in list(outs.items()) + list(houts.items()):
            assert (v == 7).all(), f"{which}: a refused call wrote {k}"
        assert call(which, w=0) == EMP_OK
        # no lights or walkers at all needs none of their arrays
        none = {k: None for k in ("n_light", "light", "light_lane", "light_cycle", "n_walker", "walker", "walker_lane")}
        assert call(which, ml=0, mw=0, h_kw=none) == EMP_OK
        assert (outs["status"] != 7).any() and (houts["last_light_out"] != 7).any()  # the accepted calls did run
    assert probes >= 60


# ---- the class --------------------------------------------------------------------------------------------------------------------------------
def test_behavior_traffic_with_lights_and_walkers(pl):
    """set_lights / set_walkers make BehaviorTraffic give the raw calls' results - run_step + vehicle_step tick by tick is rollout, and
    both are the recording's - and without them it gives today's."""
    from emplanner_carla_amd.traffic import BehaviorTraffic
    for name in ("queue_at_light", "walker_crossing"):
        f, b = hc.fixture_world(name)
        V = len(f["n_path"])
        args = lambda conv: [conv(b[k]) for k in ("path", "n_path", "lane", "state")]
        one = BehaviorTraffic(pl, *args(np.array), 60.0)
        two = BehaviorTraffic(pl, *args(up), 60.0)
        plain = BehaviorTraffic(pl, *args(up), 60.0)
        for t, conv in ((one, np.array), (two, up), (plain, up)):
            t.set_speed_limit(conv(b["speed_limit"]))
        for t, conv in ((one, np.array), (two, up)):
            if b["light"].shape[1]:
                t.set_lights(conv(b["light"]), conv(b["light_lane"]), conv(b["light_cycle"]))
            if b["walker"].shape[1]:
                t.set_walkers(conv(b["walker"]), conv(b["walker_lane"]))
        T = 300
        modes, causes = [], []
        for _ in range(T):
            ctl = one.run_step()
            modes.append(one.modes().copy())
            causes.append(np.array(one.causes(), copy=True))
            pl.vehicle_step(one.vp, one.state, ctl.reshape(V, 3), in_place=True)
            one.tick += 1
        r = two.rollout(T, log_every=1)
        raw = run_rollout(pl, b, T, 1)
        pl.synchronize()
        for k in ("state",) + bc.STATE_OUT + ("last_light",):
            hc.same_bits(to_np(getattr(two, k)).reshape(raw[k].shape), raw[k], f"{name}: {k} against the raw call")
            hc.same_bits(to_np(getattr(two, k)), getattr(one, k), f"{name}: {k}, tick by tick")
        np.testing.assert_array_equal(to_np(r.log_cause), np.stack(causes))
        np.testing.assert_array_equal(to_np(r.log_mode), np.stack(modes))
        np.testing.assert_array_equal(np.stack(causes)[:, 0], f["cause"][:T])
        np.testing.assert_array_equal(to_np(r.cause_ticks), raw["cause_ticks"])
        assert two.tick == T and to_np(r.cause_ticks).sum() > 0
        # without lights and walkers: today's call and today's result
        want = behavior_rollout(pl, {k: v for k, v in b.items() if k not in hc.HAZARD_IN}, T, 1)
        r0 = plain.rollout(T, log_every=1)
        assert type(r0).__name__ == "TrafficRolloutResult" and not hasattr(r0, "cause_ticks")
        hc.same_bits(to_np(r0.state), want["state"], f"{name}: plain state")
        np.testing.assert_array_equal(to_np(r0.log_mode), want["log_mode"])
        # taking the hazards away again gives today's behaviour back
        two.set_lights(None)
        two.set_walkers(None)
        assert type(two.rollout(1)).__name__ == "TrafficRolloutResult" and (to_np(two.last_light) == -1).all()
