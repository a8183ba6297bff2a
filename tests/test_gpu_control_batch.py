"""The batched controller surface of the C ABI - emp_mpc_lateral, emp_lqr_lateral, emp_mpc_ff_lateral,
emp_pid_longitudinal and emp_vehicle_control (both lateral laws) - on whole batches of ragged vehicles.

The rest of the suite runs the PID one vehicle per call and the fused step on recorded sequences that share one path of
one length, so a wrong vehicle stride, a read of a neighbour's path or buffer, or a walk into padding could not show.
Here:

- B = 64 and B = 151 (MPC: five vehicles per wavefront, both ragged; MPC-ff: eight per wavefront and LQR: 64 per block,
  64 exact and 151 ragged);
- per-vehicle path lengths from 0, 1 and 2 up to the capacity (the capacity at vehicle 0 and at the last vehicle), speeds
  across the classes of the existing tests (MPC's 0.005 floor; LQR speeds slow enough for all 5000 Riccati sweeps);
- every path slot past n_path[b] is poisoned: a point exactly at that vehicle's predicted position with NaN theta and
  kappa, so a search that reaches it picks it and its NaN spreads into the outputs; PID buffer entries past n_err are NaN;
- every vehicle (not a sample) is compared with its oracle: oracle/mpc_lateral.py, oracle/lqr_lateral.py,
  tests/control_port.py, and a plain-Python statement of the PID rule of include/emplanner.h that first reproduces the
  recorded reference steps bit for bit;
- batch invariance with no oracle and no tolerance (tests/batch_check.invariant): batch, alone, reversed, shifted by one,
  host == device;
- the count contract (a count beyond its row is clamped, never followed) with raw emp_* calls on device buffers with a
  guard row before and after the batch.  Counts are capacity + 3 and -1 only, the capacity is 48 and every guard row a
  whole path row, so even a library without the clamp stays inside memory this test allocated.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from tests import control_port as port
from tests.batch_check import Guarded, bits, check_count_contract, invariant, to_np
from tests.conftest import assert_rel, load_golden

pytestmark = pytest.mark.gpu

M = 48                      # path capacity
NB = 60                     # PID buffer (deque maxlen)
BATCHES = (64, 151)
NAN = np.nan
ST_S_OUT_OF_RANGE = 2
MPC_FIELDS = ("steer", "u", "e_rr", "k_r", "min_index", "pre_pro", "H", "f", "iters", "status")
LQR_FIELDS = ("steer", "K", "e_rr", "k_r", "min_index", "pre_pro", "sweeps", "status")
PID_FIELDS = ("command", "err", "n_err")
VC_FIELDS = ("control", "lat_command", "lon_command", "min_index", "e_rr", "k_r", "pre_pro", "err", "n_err", "status")


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    p = Planner(0)
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("control/control.npz")


def para():
    return tuple(float(v) for v in golden()["vehicle_para"])


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _ragged(rng, B, cap, lo):
    """Counts in [lo, cap] with 0, 1 and 2 present and the capacity at vehicle 0 and at the last vehicle."""
    n = rng.integers(lo, cap + 1, B).astype(np.int32)
    n[1], n[2], n[3] = 0, 1, 2
    n[0] = n[-1] = cap
    return n


def predicted(state, vx):
    """The one-step prediction all three lateral laws search the path for (ts = 0.1)."""
    x, y, fi, Vy = state[:, 0], state[:, 1], state[:, 2], state[:, 3]
    return np.stack([x + vx * 0.1 * np.cos(fi) - Vy * 0.1 * np.sin(fi), y + Vy * 0.1 * np.cos(fi) + vx * 0.1 * np.sin(fi)], 1)


@functools.lru_cache(maxsize=None)
def data(B):
    """Ragged paths with poisoned padding.  Failing vehicles sit between good ones: vehicle 1 (empty path), every tenth
    from 4 (min_index = n_path: out of range for MPC) and every tenth from 8 (500 m off its path with min_index = n_path:
    out of range for all three laws)."""
    rng = np.random.default_rng(500 + B)
    n = _ragged(rng, B, M, 3)
    path = np.zeros((B, M, 4))
    state = np.zeros((B, 5))
    mi = np.zeros(B, np.int32)
    vx = rng.choice([0.005, 0.05, 3.0, 9.0, 18.0], B)
    vx[:5] = 0.005, 0.05, 3.0, 9.0, 18.0
    for b in range(B):
        t = np.arange(M) * 2.4
        lx, ly = t, 10.0 * np.sin(t / 40.0 + rng.uniform(0, 3))
        rot = rng.uniform(-math.pi, math.pi)
        x0, y0 = rng.uniform(-80, 80, 2)
        xy = np.stack([x0 + lx * math.cos(rot) - ly * math.sin(rot), y0 + lx * math.sin(rot) + ly * math.cos(rot)], axis=1)
        th = np.unwrap(np.arctan2(np.gradient(xy[:, 1]), np.gradient(xy[:, 0])))
        ka = np.gradient(th) / np.hypot(np.gradient(xy[:, 0]), np.gradient(xy[:, 1]))
        path[b] = np.column_stack([xy, th, ka])
        m = max(int(n[b]), 1)
        at = int(rng.integers(0, m))
        mi[b] = max(0, at - int(rng.integers(0, 3)))
        state[b] = [xy[at, 0] + rng.normal(0, 0.5), xy[at, 1] + rng.normal(0, 0.5), th[at] + rng.normal(0, 0.1),
                    rng.normal(0, 0.3), rng.normal(0, 0.1)]
        if b % 10 == 4 and b < B - 1:
            mi[b] = n[b]
        if b % 10 == 8 and b < B - 1:
            state[b, :2] += 500.0
            mi[b] = n[b]
    pre = predicted(state, vx)
    for b in range(B):
        path[b, n[b]:, :2] = pre[b]
        path[b, n[b]:, 2:] = NAN
    return dict(B=B, path=path, n=n, state=state, vx=vx, mi=mi, pre=pre)


def _fields(r, names):
    return {k: to_np(getattr(r, k)) for k in names}


def _args(d):
    return [d["path"], d["n"], d["state"], d["vx"], d["mi"]]


# ---------------------------------------------------------------------------------------------------------------------
# lateral laws against their oracles, every vehicle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_mpc_lateral_batch(pl, B):
    from emplanner_carla_amd.api import mpc_params
    from oracle import mpc_lateral as mpc
    d = data(B)
    p = mpc_params(vehicle_para=para())
    r = invariant(lambda a, dev: _fields(pl.mpc_lateral(p, *a, qp_matrices=True), MPC_FIELDS), _args(d), "mpc_lateral")
    failed = 0
    for b in range(B):
        n, m0 = int(d["n"][b]), int(d["mi"][b])
        if not (n >= 1 and 0 <= m0 < n):
            assert r["status"][b] == ST_S_OUT_OF_RANGE and r["steer"][b] == 0.0 and not r["u"][b].any(), f"vehicle {b}"
            failed += 1
            continue
        want = mpc.lateral_mpc([tuple(q) for q in d["path"][b, :n]], tuple(d["state"][b]), float(d["vx"][b]), m0, para())
        assert r["status"][b] == 0, f"vehicle {b}: status {r['status'][b]}"
        assert r["min_index"][b] == want["min_index"], f"vehicle {b}: min_index {r['min_index'][b]} vs {want['min_index']}"
        assert_rel(r["e_rr"][b], want["e_rr"], 1e-12, f"e_rr of vehicle {b}", scale=1.0)
        assert_rel(r["u"][b], want["u"], 1e-6, f"u of vehicle {b}")
        assert_rel(r["steer"][b], want["steering"], 1e-6, f"steer of vehicle {b}")
    assert 0 < failed < B // 4


@functools.lru_cache(maxsize=None)
def _riccati(vx):
    from oracle import lqr_lateral as lq
    A, Bm = lq.continuous_model(para(), vx)
    return lq.riccati_gain(A, Bm)


def _lqr_oracle(path, state, vx, mi):
    """oracle/lqr_lateral.lateral_lqr with the Riccati gain (a function of vx alone) computed once per speed."""
    from oracle import lqr_lateral as lq
    K, sweeps = _riccati(vx)
    e_rr, k_r, idx, _, _ = lq.tracking_error(path, state, vx, mi)
    u = -np.dot(K, np.array(e_rr)) + lq.feed_forward(para(), K, k_r, vx)
    return dict(min_index=idx, sweeps=sweeps, steering=float(u[0]))


@pytest.mark.parametrize("B", BATCHES)
def test_lqr_lateral_batch(pl, B):
    from emplanner_carla_amd.api import lqr_params
    d = data(B)
    p = lqr_params(vehicle_para=para())
    r = invariant(lambda a, dev: _fields(pl.lqr_lateral(p, *a), LQR_FIELDS), _args(d), "lqr_lateral")
    failed = 0
    for b in range(B):
        n = int(d["n"][b])
        if b % 10 == 8 and b < B - 1 or n == 0:
            assert r["status"][b] == ST_S_OUT_OF_RANGE and r["steer"][b] == 0.0, f"vehicle {b}"
            failed += 1
            continue
        want = _lqr_oracle([tuple(q) for q in d["path"][b, :n]], tuple(d["state"][b]), float(d["vx"][b]), int(d["mi"][b]))
        assert r["status"][b] == 0, f"vehicle {b}: status {r['status'][b]}"
        assert r["min_index"][b] == want["min_index"] and r["sweeps"][b] == want["sweeps"], f"vehicle {b}"
        assert abs(r["steer"][b] - want["steering"]) <= 1e-6 * max(1.0, abs(want["steering"])), f"steer of vehicle {b}"
    assert 0 < failed < B // 4
    assert (r["sweeps"] == 5000).any() and (r["sweeps"] < 200).any()


@pytest.mark.parametrize("B", BATCHES)
def test_mpc_ff_lateral_batch(pl, B):
    from emplanner_carla_amd.api import mpc_ff_params
    d = data(B)
    p = mpc_ff_params(vehicle_para=para())
    args = _args(d)
    vx = args[3] = d["vx"].copy()
    vx[5::9] = 0.0                                      # no clamp on vx here: 0 and a reversing vehicle
    vx[6::13] = -1.5
    r = invariant(lambda a, dev: _fields(pl.mpc_ff_lateral(p, *a, qp_matrices=True), MPC_FIELDS), args, "mpc_ff_lateral")
    failed = 0
    for b in range(B):
        n = int(d["n"][b])
        w = port.ff_chain(para(), d["path"][b, :n], d["state"][b], float(vx[b]), int(d["mi"][b]))
        if w.get("index_error"):
            assert r["status"][b] == ST_S_OUT_OF_RANGE and r["steer"][b] == 0.0, f"vehicle {b}"
            failed += 1
            continue
        assert r["status"][b] == 0, f"vehicle {b}: status {r['status'][b]}"
        assert int(r["min_index"][b]) == w["min_index"], f"vehicle {b}"
        assert np.abs(r["H"][b] - w["H"]).max() <= 1e-9 * np.abs(w["H"]).max(), f"H of vehicle {b}"
        assert np.abs(r["f"][b] - w["f"]).max() <= 1e-9 * max(1.0, np.abs(w["f"]).max()), f"f of vehicle {b}"
        assert_rel(r["e_rr"][b], w["e_rr"], 1e-12, f"e_rr of vehicle {b}", scale=1.0)
        d_got, d_want = port.determined(r["u"][b]), port.determined(w["u"])
        assert np.abs(d_got - d_want).max() <= 1e-6, f"controls of vehicle {b}"
        assert r["steer"][b] == r["u"][b, 0]
    assert 0 < failed < B // 4


# ---------------------------------------------------------------------------------------------------------------------
# PID
# ---------------------------------------------------------------------------------------------------------------------
def py_pid(kp, ki, kd, dt, thr, speed_kmh, target, buf):
    """The rule include/emplanner.h states for emp_pid_longitudinal, in Python floats: (command, buffer after)."""
    e = target - speed_kmh
    buf = list(buf)
    if len(buf) == NB:
        buf = buf[1:]
    buf.append(e)
    integral = differential = 0.0
    if len(buf) >= 2:
        integral = sum(buf) * dt
        differential = (e - buf[-2]) / dt
    if abs(e) > thr:
        integral = 0.0
        buf = []
    return (kp * e + ki * integral) + kd * differential, buf


def _speed_kmh(v):
    return 3.6 * math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])        # reference :647-649


def _pid_want(gains, speed, target, err, n_err):
    cmd = np.zeros(len(speed))
    out = np.zeros((len(speed), NB))
    nout = np.zeros(len(speed), np.int32)
    for b in range(len(speed)):
        c, buf = py_pid(*gains, float(speed[b]), float(target[b]), [float(v) for v in err[b, :n_err[b]]])
        cmd[b], nout[b] = c, len(buf)
        out[b, :len(buf)] = buf
    return cmd, out, nout


@functools.lru_cache(maxsize=None)
def _recorded_steps():
    """The 4 x 160 recorded PID steps as 640 vehicles, each starting from the buffer recorded before its step (NaN past
    its count)."""
    g = golden()
    S, K = g["pid_command"].shape
    speed = np.array([_speed_kmh(g["pid_vel"][s, k]) for s in range(S) for k in range(K)])
    target = g["pid_target"].reshape(-1).copy()
    err = np.full((S, K, NB), NAN)
    n = np.zeros((S, K), np.int32)
    for s in range(S):
        for k in range(1, K):
            n[s, k] = g["pid_n_err"][s, k - 1]
            err[s, k, :n[s, k]] = g["pid_err"][s, k - 1, :n[s, k]]
    return speed, target, err.reshape(S * K, NB), n.reshape(-1), S, K


def test_pid_recorded_steps_as_one_batch(pl):
    """One 640-vehicle launch per recorded gain set, in order and shuffled: the rows of that gain set's sequence bit-equal
    to the reference's recorded commands and buffers, every row bit-equal to py_pid - which first reproduces all 640
    recorded steps itself."""
    from emplanner_carla_amd.api import pid_params
    g = golden()
    speed, target, err, n, S, K = _recorded_steps()
    for s in range(S):
        gains = tuple(g["pid_gains"][s]) + (1.0,)
        for k in range(K):
            i = s * K + k
            c, buf = py_pid(*gains, speed[i], target[i], [float(v) for v in err[i, :n[i]]])
            assert c == g["pid_command"][s, k] and len(buf) == g["pid_n_err"][s, k], (s, k)
            assert bits(np.array(buf + [0.0] * (NB - len(buf)))) == bits(g["pid_err"][s, k]), (s, k)
    perm = np.random.default_rng(3).permutation(S * K)
    for s in range(S):
        gains = tuple(g["pid_gains"][s]) + (1.0,)
        p = pid_params(*g["pid_gains"][s])
        call = lambda a, dev: _fields(pl.pid_longitudinal(p, *a), PID_FIELDS)
        r = invariant(call, [speed, target, err, n], f"pid_longitudinal gains {s}") if s == 0 else \
            call([speed, target, err, n], False)
        rows = slice(s * K, (s + 1) * K)
        assert bits(r["command"][rows]) == bits(g["pid_command"][s]), f"gain set {s}: commands"
        assert bits(r["err"][rows]) == bits(g["pid_err"][s]), f"gain set {s}: buffers"
        assert bits(r["n_err"][rows]) == bits(g["pid_n_err"][s]), f"gain set {s}: counts"
        want = _pid_want(gains, speed, target, err, n)
        for name, w in zip(PID_FIELDS, want):
            assert bits(r[name]) == bits(w), f"gain set {s}: {name} of the 640-vehicle batch differs from py_pid"
        rs = call([speed[perm], target[perm], err[perm], n[perm]], False)
        for name in PID_FIELDS:
            assert bits(rs[name]) == bits(r[name][perm]), f"gain set {s}: {name} changes when the batch is shuffled"


GAINS = [(1.15, 0.0, 0.0, 0.01, 1.0), (0.8, 0.3, 0.05, 0.05, 1.0), (2.0, 1.0, 0.01, 0.02, 0.5), (0.6, 0.9, 0.3, 0.1, 2.5)]


def _pid_inputs(B, seed=0):
    """Ragged buffers (0 to 60 entries, NaN past the count), errors above and below the separation threshold."""
    rng = np.random.default_rng(700 + B + seed)
    n = _ragged(rng, B, NB, 0)
    err = np.full((B, NB), NAN)
    for b in range(B):
        err[b, :n[b]] = rng.uniform(-0.9, 0.9, n[b])
    speed = rng.uniform(0.0, 80.0, B)
    dev = np.where(rng.random(B) < 0.5, rng.uniform(-0.4, 0.4, B), rng.choice([-1, 1], B) * rng.uniform(1.5, 6.0, B))
    return speed, speed + dev, err, n


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("gi", range(len(GAINS)))
def test_pid_ragged_batch(pl, B, gi):
    from emplanner_carla_amd.api import pid_params
    p = pid_params(*GAINS[gi])
    args = list(_pid_inputs(B, gi))
    r = invariant(lambda a, dev: _fields(pl.pid_longitudinal(p, *a), PID_FIELDS), args, "pid_longitudinal")
    want = _pid_want(GAINS[gi], *args)
    for name, w in zip(PID_FIELDS, want):
        bad = [b for b in range(B) if bits(r[name][b]) != bits(w[b])]
        assert not bad, f"pid_longitudinal {name} of vehicles {bad[:8]} differs from py_pid"
    sep = np.abs(args[1] - args[0]) > GAINS[gi][4]
    assert sep.any() and (~sep).any() and (r["n_err"] == NB).any() and (r["n_err"] == 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# fused vehicle control
# ---------------------------------------------------------------------------------------------------------------------
def _py_actuation(s, acc):
    """Vehicle_control.run_step (reference :705-718) with its limits, Python's own min / max."""
    steering = min(1, s) if s >= 0 else max(-1, s)
    if acc >= 0:
        return float(min(1, acc)), float(steering), 0.0
    return 0.0, float(steering), float(max(1, acc))


def _lat_params(law):
    from emplanner_carla_amd.api import lqr_params, mpc_params
    return mpc_params(vehicle_para=para()) if law == "mpc" else lqr_params(vehicle_para=para())


def _vc_args(B):
    d = data(B)
    speed, target, err, n_err = _pid_inputs(B, 11)
    return _args(d) + [speed, target, err, n_err]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_vehicle_control_batch(pl, B, law):
    import torch
    from emplanner_carla_amd.api import pid_params
    lat_p, pid_p = _lat_params(law), pid_params()
    args = _vc_args(B)
    names = ("target_path", "n_path", "state", "vx", "min_index", "speed_kmh", "target_speed", "err", "n_err")
    call = lambda a, dev: _fields(pl.vehicle_control(lat_p, pid_p, lateral=law, **dict(zip(names, a))), VC_FIELDS)
    r = invariant(call, args, f"vehicle_control {law}")
    # the lateral half: bit for bit the stand-alone entry point on the same inputs
    lat = (pl.mpc_lateral if law == "mpc" else pl.lqr_lateral)(lat_p, *args[:5])
    for name, got in (("steer", r["lat_command"]), ("min_index", r["min_index"]), ("e_rr", r["e_rr"]), ("k_r", r["k_r"]),
                      ("pre_pro", r["pre_pro"]), ("status", r["status"])):
        assert bits(got) == bits(getattr(lat, name)), f"vehicle_control {law}: {name} differs from the stand-alone law"
    pid = pl.pid_longitudinal(pid_p, *args[5:])
    ok = r["status"] == 0
    assert ok.any() and (~ok[1:-1]).sum() >= 3, "failed vehicles between good ones"
    err_in, n_in = args[7], args[8]
    for b in range(B):
        if ok[b]:
            assert bits(r["lon_command"][b]) == bits(pid.command[b]), f"lon_command of vehicle {b}"
            assert bits(r["err"][b]) == bits(pid.err[b]) and r["n_err"][b] == pid.n_err[b], f"PID state of vehicle {b}"
            want = _py_actuation(float(r["lat_command"][b]), float(r["lon_command"][b]))
            assert bits(r["control"][b]) == bits(np.array(want)), f"control of vehicle {b}: {r['control'][b]} vs {want}"
        else:
            assert bits(r["control"][b]) == bits(np.zeros(3)) and bits(r["lon_command"][b:b + 1]) == bits(np.zeros(1)), \
                f"failed vehicle {b}: controls"
            assert bits(r["err"][b]) == bits(err_in[b]) and r["n_err"][b] == n_in[b], f"failed vehicle {b} PID state"
    # device tensors with err_out / n_err_out aliasing err_in / n_err_in
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in args]
    rd = pl.vehicle_control(lat_p, pid_p, lateral=law, in_place=True, **dict(zip(names, t)))
    torch.cuda.synchronize()
    assert rd.err.data_ptr() == t[7].data_ptr() and rd.n_err.data_ptr() == t[8].data_ptr()
    for name in VC_FIELDS:
        assert bits(to_np(getattr(rd, name))) == bits(r[name]), f"vehicle_control {law} in place: {name}"


# ---------------------------------------------------------------------------------------------------------------------
# the count contract on guarded device buffers
# ---------------------------------------------------------------------------------------------------------------------
WILD_B = 151
MID, NEG = WILD_B // 2, WILD_B // 3


def _guard_path(d):
    """A path row whose points all sit at the last vehicle's predicted position (NaN theta, kappa): a search that runs
    past the last vehicle's row into the trailing guard picks them."""
    row = np.empty((M, 4))
    row[:, :2] = d["pre"][-1]
    row[:, 2:] = NAN
    return row


def _wild_mi(d):
    """min_index max_path + 1 at the wild vehicles: without the clamp, MPC's window from there lands past their row."""
    mi = d["mi"].copy()
    mi[[MID, NEG, WILD_B - 1]] = M + 1
    return mi


def _lat_ins(d, mi):
    return {"path": (d["path"], _guard_path(d)), "n": (d["n"], 0), "state": (d["state"], 0.0), "vx": (d["vx"], 1.0),
            "mi": (mi, 0)}


def _spec_mpc(d, p, ff=False):
    nu = 8 if ff else 12
    return dict(fn="emp_mpc_ff_lateral" if ff else "emp_mpc_lateral",
                sig=[C.byref(p), "B", M, "path", "n", "state", "vx", "mi", "steer", "u", "e_rr", "k_r", "mio", "pp", "H", "f",
                     "it", "st"],
                ins=_lat_ins(d, _wild_mi(d)),
                outs={"steer": ((), np.float64), "u": ((nu,), np.float64), "e_rr": ((4,), np.float64),
                      "k_r": ((), np.float64), "mio": ((), np.int32), "pp": ((4,), np.float64), "H": ((nu, nu), np.float64),
                      "f": ((nu,), np.float64), "it": ((), np.int32), "st": ((), np.int32)},
                counts={"n": M})


def _spec_lqr(d, p):
    return dict(fn="emp_lqr_lateral",
                sig=[C.byref(p), "B", M, "path", "n", "state", "vx", "mi", "steer", "K", "e_rr", "k_r", "mio", "pp", "sw", "st"],
                ins=_lat_ins(d, _wild_mi(d)),
                outs={"steer": ((), np.float64), "K": ((4,), np.float64), "e_rr": ((4,), np.float64), "k_r": ((), np.float64),
                      "mio": ((), np.int32), "pp": ((4,), np.float64), "sw": ((), np.int32), "st": ((), np.int32)},
                counts={"n": M})


def _pid_ins(B):
    speed, target, err, n_err = _pid_inputs(B, 11)
    return {"speed": (speed, 0.0), "target": (target, 0.0), "err": (err, NAN), "n_err": (n_err, 0)}


def _spec_pid(d, p):
    return dict(fn="emp_pid_longitudinal", sig=[C.byref(p), "B", "speed", "target", "err", "n_err", "cmd", "eo", "no"],
                ins=_pid_ins(d["B"]), outs={"cmd": ((), np.float64), "eo": ((NB,), np.float64), "no": ((), np.int32)},
                counts={"n_err": NB})


def _spec_vc(d, law, lat_p, pid_p, count):
    """count "n": n_path wild, with the wild vehicles' min_index at max_path + 1 as for emp_mpc_lateral.  count "n_err":
    the PID count wild on vehicles whose lateral law succeeds (a failed vehicle hands its PID state back unchanged)."""
    ins = _lat_ins(d, _wild_mi(d) if count == "n" else d["mi"])
    ins.update(_pid_ins(d["B"]))
    return dict(fn="emp_vehicle_control",
                sig=[law, C.byref(lat_p), C.byref(pid_p), "B", M, "path", "n", "state", "vx", "mi", "speed", "target", "err",
                     "n_err", "ctl", "lat", "lon", "mio", "e_rr", "k_r", "pp", "eo", "no", "st"],
                ins=ins,
                outs={"ctl": ((3,), np.float64), "lat": ((), np.float64), "lon": ((), np.float64), "mio": ((), np.int32),
                      "e_rr": ((4,), np.float64), "k_r": ((), np.float64), "pp": ((4,), np.float64),
                      "eo": ((NB,), np.float64), "no": ((), np.int32), "st": ((), np.int32)},
                counts={"n": M} if count == "n" else {"n_err": NB})


def _specs():
    from emplanner_carla_amd.api import lqr_params, mpc_ff_params, mpc_params, pid_params
    mp, lp, fp, pp = mpc_params(vehicle_para=para()), lqr_params(vehicle_para=para()), mpc_ff_params(vehicle_para=para()), \
        pid_params(0.8, 0.3, 0.05, 0.05)
    return {
        "mpc_lateral": lambda d: _spec_mpc(d, mp),
        "lqr_lateral": lambda d: _spec_lqr(d, lp),
        "mpc_ff_lateral": lambda d: _spec_mpc(d, fp, ff=True),
        "pid_longitudinal": lambda d: _spec_pid(d, pp),
        "vehicle_control_mpc": lambda d: _spec_vc(d, L.EMP_LAT_MPC, mp, pp, "n"),
        "vehicle_control_lqr": lambda d: _spec_vc(d, L.EMP_LAT_LQR, lp, pp, "n"),
        "vehicle_control_mpc_n_err": lambda d: _spec_vc(d, L.EMP_LAT_MPC, mp, pp, "n_err"),
        "vehicle_control_lqr_n_err": lambda d: _spec_vc(d, L.EMP_LAT_LQR, lp, pp, "n_err"),
    }


KERNELS = ("mpc_lateral", "lqr_lateral", "mpc_ff_lateral", "pid_longitudinal", "vehicle_control_mpc", "vehicle_control_lqr",
           "vehicle_control_mpc_n_err", "vehicle_control_lqr_n_err")


@pytest.mark.parametrize("kernel", KERNELS)
def test_counts_beyond_capacity_are_clamped(pl, kernel):
    """n_path (and n_err) at capacity + 3 for a middle and the last vehicle, -1 for another: guard rows unchanged, every
    other vehicle bit-equal to the clean call, the wild vehicles bit-equal to the call with the count clamped."""
    d = data(WILD_B)
    assert d["n"][-1] == M and (d["n"] < M).any()
    spec = _specs()[kernel](d)
    check_count_contract(pl, spec, (MID, NEG), kernel)


def test_empty_batch_writes_nothing(pl):
    for name, spec in _specs().items():
        g = Guarded(pl, spec(data(WILD_B)), B=0)
        g.call()
        g.check_guards(name)
