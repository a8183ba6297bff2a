"""GPU suite of the timed rollout: emp_speed_target against tests/speed_target_port.py, and emp_rollout_timed - T ticks of
[sample the profile, emp_vehicle_control, emp_vehicle_step] in one launch - against the chain of the 3 T stand-alone calls, BIT FOR
BIT on every output and every log row (both lateral laws, ragged batches, profiles of every kind inside one wavefront, resumed and
in-place forms, a failing vehicle, and timed trajectories as plan_cycle(speed=...) leaves them on the device); tracking of a braking
profile against a CPU loop; the refusals, in-process.

Set EMP_ROLLOUT_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speed_target_port as sp  # noqa: E402
import test_gpu_rollout as TR  # noqa: E402  (its fleets and helpers; nothing of it is collected here)
import vehicle_port as vp  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = 0.01
say, to_np, same_bits = TR.say, TR.to_np, TR.same_bits


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


def up(x):
    import torch
    return x if hasattr(x, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# emp_speed_target against the port
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 64, 4099])
def test_speed_target_matches_the_port_bit_for_bit(pl, B):
    """Every vehicle has its own generated case; host arrays, then device tensors with the slots past B poisoned (NaN, huge
    cursors) and the cursor updated in place."""
    import torch
    tick, pad = 37, 7
    c = sp.make_cases(B, 900 + B, tick=tick, dt=DT)
    want = sp.port_batch(c, tick, DT)
    r = pl.speed_target(c["traj"], c["t0"], tick, DT, c["cap"], c["cursor"])
    assert same_bits(r.target_kmh, want[0]) and same_bits(r.cursor, want[1]) and same_bits(r.tgt_status, want[2])
    r0 = pl.speed_target(c["traj"], c["t0"], tick, DT, c["cap"])                    # no cursor: zeros
    w0 = sp.port_batch(c, tick, DT, np.zeros(B, np.int32))
    assert same_bits(r0.target_kmh, w0[0]) and same_bits(r0.cursor, w0[1]) and same_bits(r0.tgt_status, w0[2])

    def grown(x, fill):
        big = np.full((B + pad,) + x.shape[1:], fill, x.dtype)
        big[:B] = x
        return big
    t = dict(traj=up(grown(c["traj"], NAN)), t0=up(grown(c["t0"], NAN)), cap=up(grown(c["cap"], NAN)),
             cursor=up(grown(c["cursor"], 2 ** 30)))
    rd = pl.speed_target(t["traj"][:B], t["t0"][:B], tick, DT, t["cap"][:B], t["cursor"][:B], in_place=True)
    pl.synchronize()
    assert isinstance(rd.target_kmh, torch.Tensor) and rd.cursor.data_ptr() == t["cursor"].data_ptr()
    assert same_bits(rd.target_kmh, want[0]) and same_bits(t["cursor"][:B], want[1]) and same_bits(rd.tgt_status, want[2])
    assert (to_np(t["cursor"][B:]) == 2 ** 30).all() and np.isnan(to_np(t["t0"][B:])).all()


# ---------------------------------------------------------------------------------------------------------------------
# rollout_timed == chain, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def profiles(B, seed=0):
    """A profile case per vehicle of TR.fleet(B), kinds in turn so that every wavefront (5 vehicles with the MPC, 64 with the
    LQR) mixes them: 0 a full ascending profile the clock runs inside; 1 no profile (NaN at sample 0); 2 a single sample;
    3 a row the clock leaves after 30 ticks; 4 a row the clock enters after 3 ticks; 5 a generated case of any kind (rows with
    equal times, backward steps, NaN caps, wild cursors).  Speeds sit around the vehicle's own, caps above and below them."""
    d = TR.fleet(B)
    rng = np.random.default_rng(7000 + 31 * seed + B)
    traj = rng.normal(0.0, 30.0, (B, 7, sp.N))
    t0, cap = np.zeros(B), np.zeros(B)
    cursor = np.zeros(B, np.int32)
    for b in range(B):
        kind = b % 6
        v = d["state"][b, 5]
        base = float(rng.choice([0.0, 0.1, 100.0 + rng.uniform(0, 10)]))
        span = float(rng.uniform(6.0, 9.0))
        time = np.array([(i - 1) * span / 400 for i in range(1, sp.N + 1)]) + base
        speed = v + rng.uniform(-3.0, 1.0) * np.linspace(0.0, 1.0, sp.N)
        t0[b] = base + float(rng.uniform(0.0, 1.0))
        cap[b] = 3.6 * v + float(rng.choice([30.0, 30.0, -2.0]))
        cursor[b] = 0 if kind in (0, 3) else int(rng.choice([0, 0, 3, -4, 400]))
        if b == 0:
            cap[b] = 3.6 * v + 30.0                                    # vehicle 0 follows its profile uncapped
        if kind == 1:
            (speed if b % 2 else time)[0] = NAN
        elif kind == 2:
            (speed if b % 4 == 0 else time)[1] = NAN
        elif kind == 3:
            k = int(rng.integers(20, 60))
            time[k + 1:] = NAN
            t0[b] = time[k] - 0.295
        elif kind == 4:
            t0[b] = time[0] - 0.025
        traj[b, 4], traj[b, 6] = speed, time
        if kind == 5:
            c = sp.make_case(rng, tick=0, dt=DT)
            traj[b], t0[b], cap[b], cursor[b] = c["traj"], c["t0"] - 0.02, c["cap"], c["cursor"]
            if np.isnan(cap[b]) or cap[b] < 5.0:                       # a NaN target is legal but teaches nothing over T ticks
                cap[b] = 3.6 * v + 1.0
    return dict(traj=traj, t0=t0, cap=cap, cursor=cursor)


def chain_timed(pl, law, d, q, T, tick0=0, torch_dev=False, carry=None):
    """T iterations of speed_target -> vehicle_control -> vehicle_step, full logs.  d: TR.fleet's arrays (its `target` is not
    used), q: profiles' arrays.  carry: (state, mi, err, n_err, cursor) to start from instead of d's and q's."""
    from emplanner_carla_amd.api import vehicle_params
    lat, vpar = TR.laws()[law], vehicle_params()
    state, mi, err, n_err, cursor = carry if carry is not None else (d["state"], d["mi"], d["err"], d["n_err"], q["cursor"])
    path, n, traj, t0, cap = d["path"], d["n"], q["traj"], q["t0"], q["cap"]
    st = to_np(state)
    cs = st[:, :5].copy()
    vx = np.array([vp.clamp_vx(v) for v in st[:, 5]])
    kmh = 3.6 * np.sqrt(st[:, 5] * st[:, 5] + st[:, 3] * st[:, 3])
    if torch_dev:
        cs, vx, kmh, state, mi, err, n_err, cursor, path, n, traj, t0, cap = (up(x) for x in (
            cs, vx, kmh, state, mi, err, n_err, cursor, path, n, traj, t0, cap))
    B = len(st)
    status, fail, tgt = np.zeros(B, np.int32), np.full(B, -1, np.int32), np.zeros(B, np.int32)
    logs = dict(state=[], control=[], err=[], index=[], target=[])
    for t in range(T):
        g = pl.speed_target(traj, t0, tick0 + t, DT, cap, cursor)
        c = pl.vehicle_control(lat, TR.pid(), path, n, cs, vx, mi, kmh, g.target_kmh, err, n_err, lateral=law)
        logs["state"].append(to_np(state).copy())
        logs["control"].append(to_np(c.control).copy())
        logs["err"].append(to_np(c.e_rr).copy())
        logs["index"].append(to_np(c.min_index).copy())
        logs["target"].append(to_np(g.target_kmh).copy())
        s_t = to_np(c.status)
        fail = np.where((fail < 0) & (s_t != 0), t, fail).astype(np.int32)
        status |= s_t
        tgt |= to_np(g.tgt_status)
        v = pl.vehicle_step(vpar, state, c.control)
        state, cs, vx, kmh, mi, err, n_err, cursor = v.state, v.ctl_state, v.vx_ctl, v.speed_kmh, c.min_index, c.err, c.n_err, g.cursor
    return dict(state=to_np(state), min_index=to_np(mi), err=to_np(err), n_err=to_np(n_err), status=status, fail_tick=fail,
                cursor=to_np(cursor), tgt_status=tgt, log_state=np.array(logs["state"]), log_control=np.array(logs["control"]),
                log_err=np.array(logs["err"]), log_index=np.array(logs["index"]), log_target=np.array(logs["target"]))


FIELDS = TR.FIELDS + ("cursor", "tgt_status")
LOGS = TR.LOGS + ("log_target",)


def check(r, want, T, every, what, rows=slice(None)):
    for k in FIELDS:
        assert same_bits(getattr(r, k), want[k]), f"{what}: {k}"
    for k in LOGS:
        got = to_np(getattr(r, k))
        assert got.shape[0] == (T + every - 1) // every, f"{what}: rows of {k}"
        assert same_bits(got, want[k][rows][::every]), f"{what}: {k}"


def run(pl, law, d, q, T, tick0=0, every=None, carry=None, in_place=False):
    from emplanner_carla_amd.api import vehicle_params
    state, mi, err, n_err, cursor = carry if carry is not None else (d["state"], d["mi"], d["err"], d["n_err"], q["cursor"])
    return pl.rollout_timed(TR.laws()[law], TR.pid(), vehicle_params(), d["path"], d["n"], state, mi, q["cap"], err, n_err,
                            q["traj"], q["t0"], T, tick0=tick0, cursor=cursor, lateral=law, log_every=every, in_place=in_place)


_CHAINS = {}


def chain_of(pl, law, B, T, tick0):
    if (law, B, T, tick0) not in _CHAINS:
        _CHAINS[law, B, T, tick0] = chain_timed(pl, law, TR.fleet(B), profiles(B), T, tick0)
    return _CHAINS[law, B, T, tick0]


@pytest.mark.parametrize("T", [1, 7, 100])
@pytest.mark.parametrize("B", [1, 5, 6, 64, 65, 333])
@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_rollout_timed_equals_the_chain_bit_for_bit(pl, law, B, T):
    d, q = TR.fleet(B), profiles(B)
    for tick0 in (0, 37):
        want = chain_of(pl, law, B, T, tick0)
        if B >= 6 and T == 100 and tick0 == 0:                   # the mix is there, and seen
            ts = want["tgt_status"]
            assert ts[1] == sp.NO_PROFILE and ts[2] & sp.PAST and not ts[2] & sp.NO_PROFILE
            assert ts[3] & sp.PAST and want["cursor"][3] > q["cursor"][3] and ts[4] & sp.BEFORE and not ts[4] & sp.PAST
            assert ts[0] & ~sp.CAPPED == 0 and want["cursor"][0] > 0
            assert len(np.unique(want["log_target"][:, 0])) > 50        # the target moves tick by tick
        for every in (1, 3):
            r = run(pl, law, d, q, T, tick0, every)
            check(r, want, T, every, f"{law} B={B} T={T} tick0={tick0} every={every}")
    r = run(pl, law, d, q, T, 37)
    assert r.log_state is None and r.log_target is None
    for k in FIELDS:
        assert same_bits(getattr(r, k), want[k]), k


@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_a_resumed_rollout_is_the_single_rollout(pl, law):
    """T = 60 against T = 23 and then T = 37 with tick0 = 23, fed from the first one's outputs."""
    B = 6
    d, q = TR.fleet(B), profiles(B)
    whole = run(pl, law, d, q, 60, 0, 1)
    a = run(pl, law, d, q, 23, 0, 1)
    b = run(pl, law, d, q, 37, 23, 1, carry=(a.state, a.min_index, a.err, a.n_err, a.cursor))
    for k in ("state", "min_index", "err", "n_err", "cursor"):
        assert same_bits(getattr(b, k), getattr(whole, k)), k
    assert same_bits(a.tgt_status | b.tgt_status, whole.tgt_status) and same_bits(a.status | b.status, whole.status)
    for k in LOGS:
        assert same_bits(np.concatenate([getattr(a, k), getattr(b, k)]), getattr(whole, k)), k
    assert (whole.cursor != q["cursor"]).any()


@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_in_place_on_device_tensors_and_poisoned_padding(pl, law):
    """Device tensors with slots past B poisoned; the five state arrays are updated where they live and equal the out-of-place
    result on host arrays."""
    B, pad, T = 65, 9, 30
    d, q = TR.fleet(B), profiles(B)
    clean = run(pl, law, d, q, T, 5, 4)

    def grown(x, fill):
        big = np.full((B + pad,) + x.shape[1:], fill, x.dtype)
        big[:B] = x
        return big
    t = dict(path=up(grown(d["path"], NAN)), n=up(grown(d["n"], 2 ** 30)), state=up(grown(d["state"], NAN)),
             mi=up(grown(d["mi"], 2 ** 30)), err=up(grown(d["err"], NAN)), n_err=up(grown(d["n_err"], -2 ** 30)),
             traj=up(grown(q["traj"], NAN)), t0=up(grown(q["t0"], NAN)), cap=up(grown(q["cap"], NAN)),
             cursor=up(grown(q["cursor"], 2 ** 30)))
    dd = dict(path=t["path"][:B], n=t["n"][:B])
    qq = dict(traj=t["traj"][:B], t0=t["t0"][:B], cap=t["cap"][:B])
    r = run(pl, law, dd, qq, T, 5, 4, carry=(t["state"][:B], t["mi"][:B], t["err"][:B], t["n_err"][:B], t["cursor"][:B]), in_place=True)
    pl.synchronize()
    assert r.state.data_ptr() == t["state"].data_ptr() and r.cursor.data_ptr() == t["cursor"].data_ptr()
    for k in FIELDS + LOGS:
        assert same_bits(getattr(r, k), getattr(clean, k)), k
    for k, name in (("state", "state"), ("mi", "min_index"), ("err", "err"), ("n_err", "n_err"), ("cursor", "cursor")):
        assert same_bits(t[k][:B], getattr(clean, name)), k
    assert np.isnan(to_np(t["state"][B:])).all() and np.isnan(to_np(t["err"][B:])).all()
    assert (to_np(t["mi"][B:]) == 2 ** 30).all() and (to_np(t["cursor"][B:]) == 2 ** 30).all()
    assert (to_np(t["n_err"][B:]) == -2 ** 30).all()


@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_a_vehicle_without_a_path_coasts_and_still_samples(pl, law):
    """n_path = 0: zero controls, PID state kept, no throttle or brake - and the cursor advances and the bits are ORed, exactly as
    the chain does it."""
    B, T = 6, 100
    d = dict(TR.fleet(B))
    q = {k: v.copy() for k, v in profiles(B).items()}
    d["n"] = d["n"].copy()
    d["n"][0] = 0                                               # vehicle 0: the full ascending profile, and now no path
    q["cap"][0] = 3.6 * d["state"][0, 5] - 2.0                  # ... capped from some tick on or throughout
    want = chain_timed(pl, law, d, q, T)
    r = run(pl, law, d, q, T, 0, 1)
    check(r, want, T, 1, f"{law} with a failing vehicle")
    assert r.status[0] == TR.ST_S_OUT_OF_RANGE and r.fail_tick[0] == 0 and not r.log_control[:, 0].any()
    assert same_bits(r.err[0], d["err"][0]) and r.n_err[0] == d["n_err"][0] and r.state[0, 5] == d["state"][0, 5]
    assert r.cursor[0] > 0 and r.tgt_status[0] & sp.CAPPED and not r.tgt_status[0] & sp.NO_PROFILE
    port = [sp.sample(q["traj"][0], q["t0"][0], 0, DT, q["cap"][0], q["cursor"][0])]
    for t in range(1, T):
        port.append(sp.sample(q["traj"][0], q["t0"][0], t, DT, q["cap"][0], port[-1][1]))
    assert same_bits(r.log_target[:, 0], np.array([p[0] for p in port])) and r.cursor[0] == port[-1][1]


def test_timed_trajectories_left_on_the_device(pl):
    """plan_cycle(speed=TrajectoryInputs(...)) with device tensors on the 16 scenes of test_gpu_trajectory's CPU-port test (scene 7
    has a reference line the cycle cannot plan on; that test holds the CPU port of the speed planner, oracle/st_backend.py,
    against these very scenes and requires solved and unsolved ones among them), then rollout_timed on r.traj, r.traj_len,
    r.speed.trajectory with t0 = the plan_start_time passed in, no host copy in between == the chain on the same tensors."""
    from emplanner_carla_amd import api as A
    from emplanner_carla_amd import scenes as S
    from tests import test_gpu_trajectory as TT
    cfg = S.CFG2
    B = 16
    b = S.make_batch(range(9100, 9100 + B), cfg)
    cyc = TT.cycle_inputs(b, empty=(7,))
    dyn, n = TT.dynamic_obstacles(b, 21)
    spd = TT.speed_inputs(cyc, dyn, n, 21)
    dev = {k: up(v) for k, v in cyc.items()}
    t0 = up(spd.plan_start_time)
    ds = A.TrajectoryInputs(spd.dp, spd.qp, up(spd.dyn_obs), up(spd.n_dyn), t0, start_heading=up(spd.start_heading))
    rd = pl.plan_cycle(A.dp_params_from_cfg(cfg), A.qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), A.smooth_params(),
                       speed=ds, **dev)
    pl.synchronize()
    assert rd.speed.trajectory.is_cuda and tuple(rd.speed.trajectory.shape) == (B, 7, sp.N)
    traj, sst = to_np(rd.traj), to_np(rd.speed.speed_status)
    state = np.zeros((B, 6))
    state[:, :3] = traj[:, 0, :3]
    state[:, 5] = np.maximum(np.hypot(b.start_v[:, 0], b.start_v[:, 1]), 3.0)
    d = dict(path=rd.traj, n=rd.traj_len, state=state, mi=np.zeros(B, np.int32), err=np.zeros((B, 60)), n_err=np.zeros(B, np.int32))
    q = dict(traj=rd.speed.trajectory, t0=t0, cap=np.full(B, 50.0), cursor=np.zeros(B, np.int32))
    for law in ("mpc", "lqr"):
        want = chain_timed(pl, law, d, q, 100, torch_dev=True)
        r = run(pl, law, d, dict(q, cap=up(q["cap"])), 100, 0, 10, carry=(up(state), up(d["mi"]), up(d["err"]), up(d["n_err"]), up(q["cursor"])))
        pl.synchronize()
        assert r.state.is_cuda and r.log_target.is_cuda
        check(r, want, 100, 10, f"{law} on planner trajectories")
        ts = want["tgt_status"]
        driven = (sst == 0) & (ts & sp.NO_PROFILE == 0)
        say(f"timed trajectories, {law}: speed_status {sst.tolist()}, tgt_status {ts.tolist()}")
        assert driven.sum() >= 1 and (ts & sp.NO_PROFILE != 0).sum() >= 1
        assert ts[7] & sp.NO_PROFILE and (want["log_target"][:, 7] == 50.0).all()
        assert (want["log_target"][:, driven] <= 50.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# tracking a braking profile against a CPU loop
# ---------------------------------------------------------------------------------------------------------------------
POS_BAR_M = 7.11e-14        # 10 x the largest position drift measured on the MI355X (7.11e-15 m): see the test's docstring
VX_BAR = 0.0                # 10 x the largest Vx difference measured (0: identical in all 32 x 300 logged states and at the end)


@functools.lru_cache(maxsize=None)
def cpu_tracking():
    path, n, state, mi, _ = TR.tracking_fleet()
    prm, traj = vp.params(), sp.braking_profile()
    timed = [sp.closed_loop_mpc_timed(prm, path[b], state[b], int(mi[b]), 50.0, traj, 0.0, TR.TRACK_T) for b in range(TR.TRACK_B)]
    # the constant-target loop on one vehicle of either side: the fleet's vehicles differ in heading and side only, and the
    # longitudinal loop sees neither but through Vy (a CPU tick costs 3 ms; 32 more vehicles would be 27 s more)
    const = [sp.closed_loop_mpc_timed(prm, path[b], state[b], int(mi[b]), 50.0, None, 0.0, TR.TRACK_T) for b in (0, 1)]
    return timed, const


def test_tracking_a_braking_profile_against_the_cpu_loop(pl):
    """oracle/mpc_lateral.py + the sampling rule + the PID rule + the actuation + vehicle_port on TR.tracking_fleet (32 vehicles
    0.5 m beside a straight path at 10 m/s), T = 300, cap 50 km/h, profile: times (i - 1) * 0.02 + 0.1, 10 m/s falling linearly to
    6 m/s over the first 2 s, then constant; t0 = 0.
    On the CPU loop alone: the final Vx differs by more than 1 m/s from the same loop with the constant target 50 km/h, and lies
    within the band the loop itself shows around 6 m/s over its last 50 ticks.  Then GPU against CPU loop: log_target, cursor and
    tgt_status identical; Vx and position drift under the bars (DESIGN "Tracking and the drift bar": 10 x the largest difference
    seen in one run on the MI355X, at most 1e-3 m and 1e-6 m/s).  Measured once over all 32 x 300 logged states: CPU final Vx
    5.999983 m/s against 13.888862 with the constant target, band 2.17e-4 m/s; largest position drift 7.11e-15 m, Vx identical.
    The Vx bar of 0 says what was seen: the longitudinal loop is + - * / and one sqrt on both sides.  Like the untimed tracking
    bar, both sit at rounding level and have to be RE-MEASURED (same rule) when the ROCm or the C library version changes."""
    from emplanner_carla_amd.api import mpc_params, pid_params, vehicle_params
    path, n, state, mi, _ = TR.tracking_fleet()
    B, T = TR.TRACK_B, TR.TRACK_T
    timed, const = cpu_tracking()
    pS = np.array([p[0] for p in timed]).transpose(1, 0, 2)      # (T, B, 6)
    pG = np.array([p[2] for p in timed]).T                       # (T, B)
    final = np.array([p[3][5] for p in timed])
    final_const = np.array([p[3][5] for p in const])
    say(f"timed tracking, CPU: final Vx {final.min():.6f}..{final.max():.6f}, constant target {final_const.min():.6f}..{final_const.max():.6f}")
    assert (np.abs(final[:, None] - final_const[None, :]) > 1.0).all()
    tail = pS[-50:, :, 5]
    band = np.abs(tail - 6.0).max(axis=0)
    say(f"timed tracking, CPU: band around 6 m/s over the last 50 ticks {band.max():.6g}")
    assert (np.abs(final - 6.0) <= band).all() and band.max() < 1.0
    traj = np.repeat(sp.braking_profile()[None], B, 0)
    r = pl.rollout_timed(mpc_params(), pid_params(), vehicle_params(), path, n, state, mi, np.full(B, 50.0), np.zeros((B, 60)),
                         np.zeros(B, np.int32), traj, np.zeros(B), T, lateral="mpc", log_every=1)
    assert (r.status == 0).all() and (r.fail_tick == -1).all()
    assert same_bits(r.log_target, pG)
    assert np.array_equal(r.cursor, [p[4] for p in timed]) and np.array_equal(r.tgt_status, [p[5] for p in timed])
    pos = np.hypot(r.log_state[:, :, 0] - pS[:, :, 0], r.log_state[:, :, 1] - pS[:, :, 1])
    dvx = np.abs(r.log_state[:, :, 5] - pS[:, :, 5])
    say(f"timed tracking: largest GPU-to-port position drift over {T} ticks {pos.max():.3g} m (bar {POS_BAR_M:.3g}); "
        f"Vx {dvx.max():.3g} (bar {VX_BAR:.3g}); final Vx {abs(r.state[:, 5] - final).max():.3g}")
    assert POS_BAR_M <= 1e-3 and VX_BAR <= 1e-6
    assert pos.max() <= POS_BAR_M and dvx.max() <= VX_BAR and np.abs(r.state[:, 5] - final).max() <= VX_BAR


# ---------------------------------------------------------------------------------------------------------------------
# refusals: host-side checks that return before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(pl):
    from emplanner_carla_amd import _lib as L
    from emplanner_carla_amd.api import lqr_params, mpc_params, pid_params, vehicle_params
    B, M = 2, 8
    keep = []

    def ptr(a):
        keep.append(a)
        return a.ctypes.data

    def io(**kw):
        s = L.RolloutTimedIO()
        s.target_path, s.n_path = ptr(np.zeros((B, M, 4))), ptr(np.zeros(B, np.int32))
        s.state, s.min_index, s.target_speed = ptr(np.zeros((B, 6))), ptr(np.zeros(B, np.int32)), ptr(np.zeros(B))
        s.err_in, s.n_err_in = ptr(np.zeros((B, 60))), ptr(np.zeros(B, np.int32))
        s.trajectory, s.t0 = ptr(np.zeros((B, 7, 401))), ptr(np.zeros(B))
        s.state_out, s.min_index_out = ptr(np.zeros((B, 6))), ptr(np.zeros(B, np.int32))
        s.err_out, s.n_err_out = ptr(np.zeros((B, 60))), ptr(np.zeros(B, np.int32))
        s.status, s.fail_tick = ptr(np.zeros(B, np.int32)), ptr(np.zeros(B, np.int32))
        s.cursor_out, s.tgt_status = ptr(np.zeros(B, np.int32)), ptr(np.zeros(B, np.int32))
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    lat, pid, vpar = mpc_params(), pid_params(), vehicle_params()

    def call(T=3, tick0=0, every=1, where=L.EMP_HOST, b=B, law=L.EMP_LAT_MPC, vp_=vpar, **kw):
        rc = pl._lib.emp_rollout_timed(pl._h, law, C.byref(lat), C.byref(pid), C.byref(vp_), b, M, T, tick0, every, C.byref(io(**kw)), where)
        return rc, (pl._lib.emp_last_error(pl._h) or b"").decode()

    INVALID = -1
    for kw, text in ((dict(T=0), "T must be in [1, 65536]"), (dict(T=65537), "T must be in [1, 65536]"),
                     (dict(tick0=-1), "tick0 must be at least 0"), (dict(tick0=2 ** 31 - 3, T=3), "tick0 + T must not exceed INT32_MAX"),
                     (dict(every=0), "log_every must be at least 1"), (dict(reserved=1), "emp_rollout_timed_io.reserved must be 0"),
                     (dict(where=2), "EMP_HOST_PINNED"), (dict(law=2), "lateral must be"),
                     (dict(trajectory=None), "NULL input array"), (dict(t0=None), "NULL input array"),
                     (dict(target_speed=None), "NULL input array"), (dict(state=None), "NULL input array"),
                     (dict(cursor_out=None), "NULL output array"), (dict(tgt_status=None), "NULL output array"),
                     (dict(state_out=None), "NULL output array"), (dict(fail_tick=None), "NULL output array")):
        rc, msg = call(**kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    bad_vp = vehicle_params()
    bad_vp.reserved = 5
    rc, msg = call(vp_=bad_vp)
    assert rc == INVALID and "emp_vehicle_params.reserved must be 0" in msg
    assert call(tick0=2 ** 31 - 4, T=3)[0] == 0                 # tick0 + T == INT32_MAX is the last one accepted
    assert call(b=0)[0] == 0 and call(law=L.EMP_LAT_LQR, b=0)[0] == 0
    # emp_speed_target
    z = lambda *s, dt=np.float64: ptr(np.zeros(s, dt))
    f = pl._lib.emp_speed_target
    good = [pl._h, B, z(B, 7, 401), z(B), 0, 0.01, z(B), None, z(B), z(B, dt=np.int32), z(B, dt=np.int32), L.EMP_HOST]
    assert f(*good) == 0
    for i, text in ((2, "NULL argument"), (3, "NULL argument"), (6, "NULL argument"), (8, "NULL argument"), (9, "NULL argument"),
                    (10, "NULL argument")):
        a = list(good)
        a[i] = None
        assert f(*a) == INVALID and text in pl._lib.emp_last_error(pl._h).decode(), i
    a = list(good)
    a[4] = -1
    assert f(*a) == INVALID and "tick must be at least 0" in pl._lib.emp_last_error(pl._h).decode()
    a = list(good)
    a[11] = 2
    assert f(*a) == INVALID and "EMP_HOST_PINNED" in pl._lib.emp_last_error(pl._h).decode()
    a = list(good)
    a[1] = 0
    assert f(*a) == 0
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        pl.rollout_timed(lqr_params(), pid, vpar, np.zeros((B, M, 4)), np.zeros(B, np.int32), np.zeros((B, 6)), np.zeros(B, np.int32),
                         np.zeros(B), np.zeros((B, 60)), np.zeros(B, np.int32), np.zeros((B, 7, 401)), np.zeros(B), 3, lateral="pid")
