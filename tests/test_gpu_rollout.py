"""GPU suite of the closed loop: emp_vehicle_step against tests/vehicle_port.py, and emp_rollout - T ticks of emp_vehicle_control +
emp_vehicle_step in one launch - against the chain of the 2 T stand-alone calls, BIT FOR BIT on every output and every log row
(both lateral laws, ragged batches with failing vehicles between good ones, aliased and separate outputs, poisoned padding, and
trajectories as plan_cycle leaves them on the device); tracking against a CPU loop built from oracle/mpc_lateral.py, the PID rule
and the port; hostile arguments in a child process.

Set EMP_ROLLOUT_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vehicle_port as vp  # noqa: E402

pytestmark = pytest.mark.gpu

M = 64                      # path slots per vehicle
ST_S_OUT_OF_RANGE = 2
NAN = float("nan")


def say(*a):
    if os.environ.get("EMP_ROLLOUT_PRINT"):
        print(*a, flush=True)


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


def to_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def same_bits(a, b):
    a, b = np.ascontiguousarray(to_np(a)), np.ascontiguousarray(to_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def arc(kappa, n, ds=2.5, rot=0.0, x0=0.0, y0=0.0):
    """n points of an arc of curvature kappa (0: a straight line) at spacing ds: rows x, y, theta, kappa."""
    s = np.arange(n) * ds
    if kappa == 0.0:
        x, y, th = s, np.zeros(n), np.zeros(n)
    else:
        th = s * kappa
        x, y = np.sin(th) / kappa, (1.0 - np.cos(th)) / kappa
    c, sn = math.cos(rot), math.sin(rot)
    return np.column_stack([x0 + x * c - y * sn, y0 + x * sn + y * c, th + rot, np.full(n, kappa)])


# ---------------------------------------------------------------------------------------------------------------------
# emp_vehicle_step against the port
# ---------------------------------------------------------------------------------------------------------------------
def step_inputs(B, seed):
    rng = np.random.default_rng(seed)
    vx = rng.choice([0.0, 0.001, 0.004, 0.5, 5.0, 20.0, 35.0], B) * rng.uniform(0.5, 1.0, B)
    st = np.column_stack([rng.uniform(-100, 100, B), rng.uniform(-100, 100, B), rng.uniform(-4, 4, B), rng.normal(0, 0.5, B),
                          rng.normal(0, 0.3, B), vx])
    ct = np.column_stack([rng.uniform(0, 1, B), rng.uniform(-1, 1, B), rng.choice([0.0, 1.0], B)])
    return st, ct


@pytest.mark.parametrize("B", [1, 5, 64, 4099])
def test_vehicle_step_matches_the_port(pl, B):
    """Vy+, fi_dot+, Vx+ and the clamped Vx bit for bit (+ - * / only); the pose to 1e-12 relative (sin / cos); speed_kmh from
    the port's formula on the GPU's own Vx+, Vy+ bit for bit (sqrt is correctly rounded on both sides)."""
    from emplanner_carla_amd.api import vehicle_params
    st, ct = step_inputs(B, 40 + B)
    for kw in (dict(), dict(drag=0.05, steer_gain=0.6, dt=0.02)):
        prm = vp.params(**kw)
        r = pl.vehicle_step(vehicle_params(**kw), st, ct)
        want = np.array([vp.step(prm, st[i], ct[i]) for i in range(B)])
        assert np.array_equal(r.state[:, 3:], want[:, 3:])
        pose = np.abs(r.state[:, :3] - want[:, :3]) / np.maximum(1.0, np.abs(want[:, :3]))
        say(f"vehicle_step B={B}: worst pose error {pose.max():.3g} (bar 1e-12)")
        assert pose.max() <= 1e-12
        assert np.array_equal(r.ctl_state, r.state[:, :5])
        assert np.array_equal(r.vx_ctl, [vp.clamp_vx(v) for v in want[:, 5]])
        assert np.array_equal(r.speed_kmh, [vp.speed_kmh(want[i, 5], want[i, 3]) for i in range(B)])
        alias = st.copy()
        ra = pl.vehicle_step(vehicle_params(**kw), alias, ct, in_place=True)
        assert ra.state is alias and same_bits(alias, r.state) and same_bits(ra.speed_kmh, r.speed_kmh)


def test_vehicle_step_on_device_tensors_and_poisoned_slots(pl):
    import torch
    from emplanner_carla_amd.api import vehicle_params
    B, pad = 333, 7
    st, ct = step_inputs(B + pad, 9)
    st[B:], ct[B:] = NAN, NAN
    host = pl.vehicle_step(vehicle_params(), st[:B], ct[:B])
    big, bigc = torch.from_numpy(st).cuda(), torch.from_numpy(ct).cuda()
    r = pl.vehicle_step(vehicle_params(), big[:B], bigc[:B], in_place=True)
    pl.synchronize()
    assert same_bits(big[:B], host.state) and same_bits(r.ctl_state, host.ctl_state) and same_bits(r.vx_ctl, host.vx_ctl)
    assert same_bits(r.speed_kmh, host.speed_kmh)
    assert np.isnan(to_np(big[B:])).all()


# ---------------------------------------------------------------------------------------------------------------------
# rollout == chain, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fleet(B, seed=0):
    """Arcs of radius 150-1000 m (either side) at 2.5 m spacing with ragged counts; a vehicle 0.5 m or less beside its path at
    5-15 m/s; PID deques of every length, targets within and beyond the separation threshold.  Failing vehicles sit between
    good ones: vehicle 1 has an empty path (fails every tick), vehicles 3, 13, ... a min_index = n_path (out of range for the
    MPC's window at tick 0; tick 0 writes a valid match and the vehicle recovers), vehicles 4, 14, ... min_index = -7."""
    rng = np.random.default_rng(1000 * seed + B)
    n = rng.integers(20, M + 1, B).astype(np.int32)
    path = np.zeros((B, M, 4))
    state = np.zeros((B, 6))
    mi = np.zeros(B, np.int32)
    for b in range(B):
        k = rng.choice([-1.0, 1.0]) / rng.uniform(150.0, 1000.0)
        path[b] = arc(k, M, rot=rng.uniform(-math.pi, math.pi), x0=rng.uniform(-80, 80), y0=rng.uniform(-80, 80))
        at = int(rng.integers(1, 8))
        p = path[b, at]
        off = rng.uniform(-0.5, 0.5)
        v = rng.uniform(5.0, 15.0)
        state[b] = [p[0] - off * math.sin(p[2]), p[1] + off * math.cos(p[2]), p[2] + rng.normal(0, 0.03), rng.normal(0, 0.1),
                    v * k + rng.normal(0, 0.02), v]
        mi[b] = max(0, at - int(rng.integers(0, 3)))
        if b % 10 == 3:
            mi[b] = n[b]
        if b % 10 == 4:
            mi[b] = -7
    if B > 1:
        n[1] = 0
    target = 3.6 * state[:, 5] + rng.choice([-6.0, -0.4, 0.3, 0.8, 9.0], B)
    n_err = rng.integers(0, 61, B).astype(np.int32)
    err = rng.normal(0, 0.3, (B, 60))
    for b in range(B):
        err[b, n_err[b]:] = 0.0
    return dict(B=B, path=path, n=n, state=state, mi=mi, target=target, err=err, n_err=n_err)


def laws():
    from emplanner_carla_amd.api import lqr_params, mpc_params
    return {"mpc": mpc_params(), "lqr": lqr_params()}


def pid():
    from emplanner_carla_amd.api import pid_params
    return pid_params(K_P=1.15, K_I=0.3, K_D=0.02)         # every term of the PID takes part


def chain(pl, law, d, T, torch_dev=False):
    """T iterations of vehicle_control + vehicle_step, full logs.  Tick 0's controller inputs come from the state by
    emp_vehicle_step's own formulas, evaluated here in binary64 (IEEE *, +, sqrt: the same bits)."""
    from emplanner_carla_amd.api import vehicle_params
    lat, vpar = laws()[law], vehicle_params()
    st = d["state"]
    cs = st[:, :5].copy()
    vx = np.array([vp.clamp_vx(v) for v in st[:, 5]])
    kmh = 3.6 * np.sqrt(st[:, 5] * st[:, 5] + st[:, 3] * st[:, 3])
    state, mi, err, n_err = st.copy(), d["mi"].copy(), d["err"].copy(), d["n_err"].copy()
    path, n, target = d["path"], d["n"], d["target"]
    if torch_dev:
        import torch
        up = lambda x: x if hasattr(x, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x)).cuda()
        cs, vx, kmh, state, mi, err, n_err, path, n, target = (up(x) for x in (cs, vx, kmh, state, mi, err, n_err, path, n, target))
    B = len(st)
    status, fail = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    logs = dict(state=[], control=[], err=[], index=[])
    for t in range(T):
        c = pl.vehicle_control(lat, pid(), path, n, cs, vx, mi, kmh, target, err, n_err, lateral=law)
        logs["state"].append(to_np(state).copy())
        logs["control"].append(to_np(c.control).copy())
        logs["err"].append(to_np(c.e_rr).copy())
        logs["index"].append(to_np(c.min_index).copy())
        s_t = to_np(c.status)
        fail = np.where((fail < 0) & (s_t != 0), t, fail).astype(np.int32)
        status |= s_t
        v = pl.vehicle_step(vpar, state, c.control)
        state, cs, vx, kmh, mi, err, n_err = v.state, v.ctl_state, v.vx_ctl, v.speed_kmh, c.min_index, c.err, c.n_err
    return dict(state=to_np(state), min_index=to_np(mi), err=to_np(err), n_err=to_np(n_err), status=status, fail_tick=fail,
                log_state=np.array(logs["state"]), log_control=np.array(logs["control"]), log_err=np.array(logs["err"]),
                log_index=np.array(logs["index"]))


_CHAINS = {}


def chain_of(pl, law, B, T):
    if (law, B, T) not in _CHAINS:
        _CHAINS[law, B, T] = chain(pl, law, fleet(B), T)
    return _CHAINS[law, B, T]


FIELDS = ("state", "min_index", "err", "n_err", "status", "fail_tick")
LOGS = ("log_state", "log_control", "log_err", "log_index")


def check_against_chain(r, want, T, every, what):
    for k in FIELDS:
        assert same_bits(getattr(r, k), want[k]), f"{what}: {k}"
    for k in LOGS:
        got = to_np(getattr(r, k))
        assert got.shape[0] == (T + every - 1) // every, f"{what}: rows of {k}"
        assert same_bits(got, want[k][::every]), f"{what}: {k}"


@pytest.mark.parametrize("T", [1, 7, 100])
@pytest.mark.parametrize("B", [1, 5, 6, 333])
@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_rollout_equals_the_chain_bit_for_bit(pl, law, B, T):
    from emplanner_carla_amd.api import vehicle_params
    d = fleet(B)
    want = chain_of(pl, law, B, T)
    if B >= 5:                                              # the failing-vehicle rule is exercised, and seen
        assert want["status"][1] == ST_S_OUT_OF_RANGE and want["fail_tick"][1] == 0
        assert not want["log_control"][:, 1].any() and same_bits(want["err"][1], d["err"][1]) and want["n_err"][1] == d["n_err"][1]
        assert want["state"][1, 5] == d["state"][1, 5]                                  # it coasts: no throttle, no brake
        if law == "mpc":
            assert want["status"][3] == ST_S_OUT_OF_RANGE and want["fail_tick"][3] == 0 and want["fail_tick"][4] == 0
            if T > 1:
                assert want["log_control"][1:, 3].any()                                # ... and recovers at tick 1
        assert want["status"][0] == 0 and want["fail_tick"][0] == -1 and want["status"][2] == 0
    for every in (1, 3, T + 1):
        r = pl.rollout(laws()[law], pid(), vehicle_params(), d["path"], d["n"], d["state"], d["mi"], d["target"], d["err"],
                       d["n_err"], T, lateral=law, log_every=every)
        check_against_chain(r, want, T, every, f"{law} B={B} T={T} every={every}")
        # aliased: the four state arrays are updated where they live
        own = {k: d[k].copy() for k in ("state", "mi", "err", "n_err")}
        ra = pl.rollout(laws()[law], pid(), vehicle_params(), d["path"], d["n"], own["state"], own["mi"], d["target"], own["err"],
                        own["n_err"], T, lateral=law, log_every=every, in_place=True)
        assert ra.state is own["state"] and ra.min_index is own["mi"] and ra.err is own["err"] and ra.n_err is own["n_err"]
        check_against_chain(ra, want, T, every, f"{law} B={B} T={T} every={every} in place")
    r = pl.rollout(laws()[law], pid(), vehicle_params(), d["path"], d["n"], d["state"], d["mi"], d["target"], d["err"], d["n_err"], T,
                   lateral=law)
    assert r.log_state is None and r.log_index is None
    for k in FIELDS:
        assert same_bits(getattr(r, k), want[k]), k


@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_rollout_ignores_poisoned_padding(pl, law):
    """Path slots past n_path and vehicle slots past B are poisoned; device tensors, updated in place.  (e_rr of a vehicle with
    an EMPTY path is computed from path slot 0 - emp_vehicle_control's behaviour, stated in the header - so its log_err rows
    are the one thing left out.)"""
    import torch
    from emplanner_carla_amd.api import vehicle_params
    B, pad, T = 333, 9, 30
    d = fleet(B)
    clean = pl.rollout(laws()[law], pid(), vehicle_params(), d["path"], d["n"], d["state"], d["mi"], d["target"], d["err"],
                       d["n_err"], T, lateral=law, log_every=4)

    def grown(x, fill):
        big = np.full((B + pad,) + x.shape[1:], fill, x.dtype)
        big[:B] = x
        return big
    path = grown(d["path"], NAN)
    for b in range(B):
        path[b, d["n"][b]:] = [1e300, -1e300, NAN, NAN]
    big = dict(path=path, n=grown(d["n"], 2 ** 30), state=grown(d["state"], NAN), mi=grown(d["mi"], 2 ** 30),
               target=grown(d["target"], NAN), err=grown(d["err"], NAN), n_err=grown(d["n_err"], -2 ** 30))
    t = {k: torch.from_numpy(v).cuda() for k, v in big.items()}
    r = pl.rollout(laws()[law], pid(), vehicle_params(), t["path"][:B], t["n"][:B], t["state"][:B], t["mi"][:B], t["target"][:B],
                   t["err"][:B], t["n_err"][:B], T, lateral=law, log_every=4, in_place=True)
    pl.synchronize()
    has_path = d["n"] > 0
    for k in FIELDS + LOGS:
        got, want = to_np(getattr(r, k)), to_np(getattr(clean, k))
        if k == "log_err":
            got, want = got[:, has_path], want[:, has_path]
        assert same_bits(got, want), k
    for k in ("state", "err"):
        assert np.isnan(to_np(t[k][B:])).all(), k
    assert (to_np(t["mi"][B:]) == 2 ** 30).all() and (to_np(t["n_err"][B:]) == -2 ** 30).all()


def test_rollout_on_planner_trajectories_left_on_the_device(pl):
    """plan_cycle on 64 scenes with device tensors, then rollout(T = 100) on CycleResult.traj / traj_len as they are (max_path =
    max_pts + 1, no host copy) == the chain on the same device arrays."""
    import torch
    from emplanner_carla_amd import scenes as S
    from emplanner_carla_amd.api import dp_params_from_cfg, qp_params, smooth_params, vehicle_params
    cfg = S.CFG2
    b = S.make_batch(range(7000, 7064), cfg)
    B, P = b.ref.shape[:2]
    host = dict(ref_line=b.ref, n_ref=np.full(B, P, np.int32), origin_xy=b.origin_xy, start_xy=b.start_xy, start_v=b.start_v,
                start_a=b.start_a, obs_xy=b.obs_xy, n_obs=b.n_obs)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    rd = pl.plan_cycle(dp_params_from_cfg(cfg), qp_params(), smooth_params(), **dev)
    pl.synchronize()
    assert hasattr(rd.traj, "data_ptr") and rd.traj.is_cuda and rd.traj.shape[0] == B and rd.traj.shape[2] == 4
    traj, tlen = to_np(rd.traj), to_np(rd.traj_len)
    assert (tlen > 10).mean() > 0.5
    rng = np.random.default_rng(5)
    state = np.zeros((B, 6))
    state[:, :3] = traj[:, 0, :3]
    state[:, 1] += rng.uniform(-0.2, 0.2, B)
    state[:, 5] = rng.uniform(6.0, 12.0, B)
    d = dict(path=rd.traj, n=rd.traj_len, state=state, mi=np.zeros(B, np.int32), target=3.6 * state[:, 5] + 0.5,
             err=np.zeros((B, 60)), n_err=np.zeros(B, np.int32))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for law in ("mpc", "lqr"):
        want = chain(pl, law, d, 100, torch_dev=True)
        r = pl.rollout(laws()[law], pid(), vehicle_params(), rd.traj, rd.traj_len, up(state), up(d["mi"]), up(d["target"]),
                       up(d["err"]), up(d["n_err"]), 100, lateral=law, log_every=10)
        pl.synchronize()
        assert r.state.is_cuda
        check_against_chain(r, want, 100, 10, f"{law} on planner trajectories")
        ok = want["status"] == 0
        say(f"planner trajectories, {law}: {int(ok.sum())} of {B} vehicles ran all 100 ticks clean")
        assert ok.sum() >= B // 2 and np.isfinite(want["state"][ok]).all()


# ---------------------------------------------------------------------------------------------------------------------
# tracking against a CPU loop
# ---------------------------------------------------------------------------------------------------------------------
TRACK_B, TRACK_T = 32, 300
DRIFT_BAR_M = 5.55e-16      # 10 x the largest drift measured on the MI355X (5.55e-17 m): see the tracking test's docstring


def tracking_fleet():
    """32 STRAIGHT paths of every heading, the vehicle 0.5 m to either side at 10 m/s, target 36 km/h.  Straight because of the
    plant, not the kernel: with the controllers' default vehicle_para a radian of wheel angle yields about 0.03 rad/s of yaw
    rate at 10 m/s, so on the issue's 150-1000 m arcs the port's own |e_d| GROWS over 300 ticks (measured on the CPU: 0.5 m ->
    1.1-2.0 m at R = 300 m, 0.5 -> 0.9 m on the outside of R = 1000 m), while on a straight line it falls 0.5 -> 0.451 m."""
    rng = np.random.default_rng(77)
    path = np.zeros((TRACK_B, 120, 4))
    state = np.zeros((TRACK_B, 6))
    for b in range(TRACK_B):
        path[b] = arc(0.0, 120, rot=-math.pi + 2 * math.pi * b / TRACK_B, x0=rng.uniform(-50, 50), y0=rng.uniform(-50, 50))
        p = path[b, 2]
        off = 0.5 if b % 2 == 0 else -0.5
        state[b] = [p[0] - off * math.sin(p[2]), p[1] + off * math.cos(p[2]), p[2], 0.0, 0.0, 10.0]
    return path, np.full(TRACK_B, 120, np.int32), state, np.full(TRACK_B, 2, np.int32), np.full(TRACK_B, 36.0)


def test_tracking_against_the_cpu_loop(pl):
    """oracle/mpc_lateral.py + the PID rule + the actuation + vehicle_port, 32 vehicles 0.5 m beside a straight path at 10 m/s,
    T = 300 - against emp_rollout with full logs.
      - the port's own |e_d| at tick 299 is below its value at tick 0 (0.5 -> 0.451 m; checked on the CPU first), and the GPU
        shows the same decrease;
      - tick 0 meets the per-call bars of the lateral law (steer 1e-6, e_rr 1e-12 with scale 1);
      - later ticks: the GPU-to-port drift in position (the two solve each tick's QP to their own tolerance and integrate the
        difference).  Measured once on the MI355X over all 32 x 300 logged states: largest position drift 5.55e-17 m, largest
        steer difference 4.11e-15, Vx identical; tick 0 steer difference 2.2e-16.  The bar is 10 x the largest drift seen,
        5.55e-16 m (the cap for such a bar is 1e-3 m).  That is below one ulp of most coordinates: the steer differences of
        1e-15 vanish in the model's rounding, so in effect the two loops must agree to the bit except near a zero coordinate -
        a wrong sign or a swapped term moves a vehicle by millimetres within a few ticks.  Because the bar sits below an ulp it
        also holds the device's sin / cos and the host's libm to the same bits along 300 ticks: it was measured with one
        toolchain and HAS TO BE RE-MEASURED (same rule: 10 x the largest drift seen, at most 1e-3 m) when the ROCm or the C
        library version changes - a red result after such a change is first a reason to measure, not a kernel fault."""
    from emplanner_carla_amd.api import mpc_params, pid_params, vehicle_params
    from conftest import assert_rel
    path, n, state, mi, target = tracking_fleet()
    prm = vp.params()
    port = [vp.closed_loop_mpc(prm, path[b], state[b], int(mi[b]), float(target[b]), TRACK_T) for b in range(TRACK_B)]
    pS = np.array([p[0] for p in port]).transpose(1, 0, 2)      # (T, B, 6)
    pU = np.array([p[1] for p in port]).transpose(1, 0, 2)
    pE = np.array([p[2] for p in port]).transpose(1, 0, 2)
    assert (np.abs(pE[-1, :, 0]) < np.abs(pE[0, :, 0])).all(), "the port itself must converge on the chosen inputs"
    r = pl.rollout(mpc_params(), pid_params(), vehicle_params(), path, n, state, mi, target, np.zeros((TRACK_B, 60)),
                   np.zeros(TRACK_B, np.int32), TRACK_T, lateral="mpc", log_every=1)
    assert (r.status == 0).all() and (r.fail_tick == -1).all()
    say(f"tracking: |e_d| tick 0 {np.abs(r.log_err[0, :, 0]).max():.6f}, tick 299 GPU {np.abs(r.log_err[-1, :, 0]).max():.6f} "
        f"port {np.abs(pE[-1, :, 0]).max():.6f}")
    assert (np.abs(r.log_err[-1, :, 0]) < np.abs(r.log_err[0, :, 0])).all()
    assert same_bits(r.log_state[0], state)
    steer0 = np.abs(r.log_control[0, :, 1] - pU[0, :, 1]).max()
    say(f"tracking: tick 0 steer difference {steer0:.3g} (bar 1e-6)")
    assert_rel(r.log_control[0, :, 1], pU[0, :, 1], 1e-6, "steer at tick 0")
    assert_rel(r.log_err[0], pE[0], 1e-12, "e_rr at tick 0", scale=1.0)
    pos = np.hypot(r.log_state[:, :, 0] - pS[:, :, 0], r.log_state[:, :, 1] - pS[:, :, 1])
    say(f"tracking: largest GPU-to-port position drift over {TRACK_T} ticks {pos.max():.3g} m (bar {DRIFT_BAR_M:.3g} m); "
        f"steer {np.abs(r.log_control[:, :, 1] - pU[:, :, 1]).max():.3g}; Vx {np.abs(r.log_state[:, :, 5] - pS[:, :, 5]).max():.3g}")
    assert DRIFT_BAR_M <= 1e-3
    assert pos.max() <= DRIFT_BAR_M


def test_hostile_arguments_in_a_child_process():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rollout_fuzz_child.py")], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    tail = run.stdout[-3000:] + "\n" + run.stderr[-3000:]
    assert run.returncode == 0, f"the fuzz child died with {run.returncode}:\n{tail}"
    assert "ROLLOUT-FUZZ-OK" in run.stdout, tail
    last = run.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 45 and int(last[3]) >= 30, last
