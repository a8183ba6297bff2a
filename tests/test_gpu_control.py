"""GPU parity of the controller completion (reference controller/controller.py): the feed-forward lateral MPC
(emp_mpc_ff_lateral, :727-990), the longitudinal PID (emp_pid_longitudinal, :614-678) and Vehicle_control.run_step as one
kernel launch (emp_vehicle_control, :680-724), against tests/golden/control/control.npz (the imported reference classes) and
tests/control_port.py; the drop-in classes; hostile arguments in a child process.

Bars: PID commands and buffers bit for bit (csrc/emp_control_core.h keeps the reference's operation order); match index and
k_r exact, e_rr and the predicted / projected points 1e-12; H and f 1e-9 relative; the controls the singular feed-forward QP
determines (u0..u3 and the pair sums u4 + u5, u6 + u7, see include/emplanner.h) 1e-6; the fused kernel's lateral command bit
for bit equal to the stand-alone lateral entry points."""
from __future__ import annotations

import math
import os
import subprocess
import sys
from collections import deque
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests.conftest import load_golden
from tests import control_port as port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_S_OUT_OF_RANGE = 2


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


@pytest.fixture(scope="module")
def g():
    return load_golden(os.path.join("control", "control.npz"))


def _speed_kmh(v):
    return 3.6 * math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])        # reference :647-649


class FakeVehicle:
    def __init__(self, s):
        self.s = [float(v) for v in s]          # x, y, yaw (deg), vx, vy, vz, yaw rate (deg/s)

    def get_location(self):
        return NS(x=self.s[0], y=self.s[1], z=0.0)

    def get_transform(self):
        return NS(rotation=NS(yaw=self.s[2], pitch=0.0, roll=0.0))

    def get_velocity(self):
        return NS(x=self.s[3], y=self.s[4], z=self.s[5])

    def get_angular_velocity(self):
        return NS(x=0.0, y=0.0, z=self.s[6])


def _close(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    d = np.abs(got - want).max(initial=0.0)
    assert d <= tol, f"{what}: off by {d:.3e} (bar {tol:.0e})"


# ---- feed-forward MPC ------------------------------------------------------------------------------------------------
def _ff_call(pl, g):
    from emplanner_carla_amd.api import mpc_ff_params
    return pl.mpc_ff_lateral(mpc_ff_params(vehicle_para=tuple(g["vehicle_para"])), g["ff_path"], g["ff_n"].astype(np.int32),
                             g["ff_state"], g["ff_Vx"], g["ff_min_index_in"].astype(np.int32), qp_matrices=True)


def test_mpc_ff_vs_reference_class(pl, g):
    r = _ff_call(pl, g)
    assert (r.status == 0).all(), r.status
    assert (g["ff_Vx"] == 0).any()
    np.testing.assert_array_equal(r.min_index, g["ff_min_index"])
    np.testing.assert_array_equal(r.k_r, g["ff_k_r"])
    _close(r.e_rr, g["ff_e_rr"], 1e-12, "e_rr")
    _close(r.pre_pro[:, :2], g["ff_pre"], 1e-12, "predicted point")
    _close(r.pre_pro[:, 2:], g["ff_pro"], 1e-12, "projected point")
    for c in range(len(g["ff_n"])):
        assert np.abs(r.H[c] - g["ff_H"][c]).max() <= 1e-9 * np.abs(g["ff_H"][c]).max(), f"H of case {c}"
        assert np.abs(r.f[c] - g["ff_f"][c]).max() <= 1e-9 * max(1.0, np.abs(g["ff_f"][c]).max()), f"f of case {c}"
    _close(port.determined(r.u), port.determined(g["ff_u"]), 1e-6, "u0..u3 and pair sums")
    _close(r.steer, g["ff_steer"], 1e-6, "steer")
    np.testing.assert_array_equal(r.steer, r.u[:, 0])
    assert (np.abs(r.u) <= 1.0 + 1e-12).all()
    # the reference's H is singular along u4 - u5 and u6 - u7 (R_bar covers the first P steps only)
    ev = np.linalg.eigvalsh(g["ff_H"][1])
    assert (np.abs(ev) < 1e-9 * ev.max()).sum() == 2
    # KKT certificate of the box QP on the reference's own (H, f)
    for c in range(len(g["ff_n"])):
        H, f, u = g["ff_H"][c], g["ff_f"][c], r.u[c]
        grad = H @ u + f
        scale = max(1.0, np.abs(f).max())
        free = np.abs(u) < 1.0 - 1e-7
        assert np.abs(grad[free]).max(initial=0.0) <= 1e-6 * scale, f"stationarity of case {c}"
        assert (grad[u >= 1.0 - 1e-7] <= 1e-6 * scale).all() and (grad[u <= -1.0 + 1e-7] >= -1e-6 * scale).all(), c


def test_mpc_ff_batch_vs_port_and_device_tensors(pl, g):
    """300 random vehicles against tests/control_port.py; host and device pointers give identical bits."""
    import torch
    from emplanner_carla_amd.api import mpc_ff_params
    rng = np.random.default_rng(11)
    B, M = 300, 64
    para = tuple(g["vehicle_para"])
    path = np.zeros((B, M, 4))
    n = rng.integers(1, M + 1, B).astype(np.int32)
    state = np.zeros((B, 5))
    vx = np.zeros(B)
    mi = np.zeros(B, np.int32)
    for b in range(B):
        t = np.arange(n[b]) * 2.0
        x0, y0, h0 = rng.uniform(-50, 50, 2).tolist() + [rng.uniform(-math.pi, math.pi)]
        k = rng.normal(0, 0.01)
        th = h0 + k * t
        path[b, :n[b]] = np.column_stack([x0 + np.cumsum(np.cos(th)) * 2.0, y0 + np.cumsum(np.sin(th)) * 2.0, th,
                                          np.full(n[b], k)])
        at = int(rng.integers(0, n[b]))
        state[b] = [path[b, at, 0] + rng.normal(0, 0.5), path[b, at, 1] + rng.normal(0, 0.5), th[at] + rng.normal(0, 0.1),
                    rng.normal(0, 0.3), rng.normal(0, 0.1)]
        vx[b] = 0.0 if b % 50 == 0 else rng.uniform(-2, 30)
        mi[b] = rng.integers(0, n[b])
    p = mpc_ff_params(vehicle_para=para)
    r = pl.mpc_ff_lateral(p, path, n, state, vx, mi, qp_matrices=True)
    assert (r.status == 0).all()
    for b in range(B):
        w = port.ff_chain(para, path[b, :n[b]], state[b], float(vx[b]), int(mi[b]))
        assert int(r.min_index[b]) == w["min_index"], b
        assert np.abs(r.H[b] - w["H"]).max() <= 1e-9 * np.abs(w["H"]).max(), b
        assert np.abs(r.f[b] - w["f"]).max() <= 1e-9 * max(1.0, np.abs(w["f"]).max()), b
        _close(r.e_rr[b], w["e_rr"], 1e-12, f"e_rr {b}")
        _close(port.determined(r.u[b]), port.determined(w["u"]), 1e-6, f"controls {b}")
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rd = pl.mpc_ff_lateral(p, T(path), T(n), T(state), T(vx), T(mi), qp_matrices=True)
    torch.cuda.synchronize()
    for name in ("steer", "u", "e_rr", "k_r", "min_index", "pre_pro", "H", "f", "iters", "status"):
        np.testing.assert_array_equal(getattr(rd, name).cpu().numpy(), getattr(r, name), err_msg=name)


def test_mpc_ff_bad_index_and_empty_batch(pl, g):
    from emplanner_carla_amd.api import mpc_ff_params
    p = mpc_ff_params(vehicle_para=tuple(g["vehicle_para"]))
    path = g["ff_path"][:3].copy()
    n = g["ff_n"][:3].astype(np.int32)
    state = g["ff_state"][:3].copy()
    state[1, :2] += 500.0                        # nothing within 100 m: min_index is used, and it is out of range
    mi = np.array([0, 999, 0], np.int32)
    r = pl.mpc_ff_lateral(p, path, n, state, g["ff_Vx"][:3], mi)
    assert list(r.status) == [0, ST_S_OUT_OF_RANGE, 0] and r.steer[1] == 0.0
    r1 = pl.mpc_ff_lateral(p, path[[0, 2]], n[[0, 2]], state[[0, 2]], g["ff_Vx"][[0, 2]], mi[[0, 2]])
    np.testing.assert_array_equal(r.steer[[0, 2]], r1.steer)
    r0 = pl.mpc_ff_lateral(p, path[:0], n[:0], state[:0], g["ff_Vx"][:0], mi[:0])
    assert r0.steer.shape == (0,)


# ---- PID ---------------------------------------------------------------------------------------------------------------
def test_pid_vs_reference_sequences_host_state(pl, g):
    from emplanner_carla_amd.api import pid_params
    for s in range(g["pid_gains"].shape[0]):
        K_P, K_I, K_D, dt = g["pid_gains"][s]
        p = pid_params(K_P, K_I, K_D, dt)
        err, n = np.zeros((1, 60)), np.zeros(1, np.int32)
        for k in range(g["pid_command"].shape[1]):
            r = pl.pid_longitudinal(p, np.array([_speed_kmh(g["pid_vel"][s, k])]), g["pid_target"][s, k:k + 1], err, n)
            assert r.command[0] == g["pid_command"][s, k], (s, k)
            np.testing.assert_array_equal(r.err[0], g["pid_err"][s, k])
            assert r.n_err[0] == g["pid_n_err"][s, k]
            err, n = r.err, r.n_err


def test_pid_state_on_device_with_aliased_buffers(pl, g):
    """All four sequences at once (one vehicle each, four calls per step), the PID state living in torch device tensors
    updated in place (err_out / n_err_out the same memory as err_in / n_err_in); and the aliased host form."""
    import torch
    from emplanner_carla_amd.api import pid_params
    dev = torch.device("cuda", 0)
    S, K = g["pid_gains"].shape[0], g["pid_command"].shape[1]
    errs = [torch.zeros((1, 60), dtype=torch.float64, device=dev) for _ in range(S)]
    ns = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(S)]
    herr = [np.zeros((1, 60)) for _ in range(S)]
    hn = [np.zeros(1, np.int32) for _ in range(S)]
    cmds = torch.zeros((S, K), dtype=torch.float64, device=dev)
    bufs = torch.zeros((S, K, 60), dtype=torch.float64, device=dev)
    for k in range(K):
        for s in range(S):
            p = pid_params(*g["pid_gains"][s])
            v = np.array([_speed_kmh(g["pid_vel"][s, k])])
            r = pl.pid_longitudinal(p, torch.from_numpy(v).to(dev), torch.from_numpy(g["pid_target"][s, k:k + 1]).to(dev),
                                    errs[s], ns[s], in_place=True)
            assert r.err.data_ptr() == errs[s].data_ptr() and r.n_err.data_ptr() == ns[s].data_ptr()
            cmds[s, k] = r.command[0]
            bufs[s, k] = errs[s][0]
            rh = pl.pid_longitudinal(p, v, g["pid_target"][s, k:k + 1], herr[s], hn[s], in_place=True)
            assert rh.err is herr[s]
            assert rh.command[0] == g["pid_command"][s, k] and hn[s][0] == g["pid_n_err"][s, k]
            np.testing.assert_array_equal(herr[s][0], g["pid_err"][s, k])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cmds.cpu().numpy(), g["pid_command"])
    np.testing.assert_array_equal(bufs.cpu().numpy(), g["pid_err"])
    np.testing.assert_array_equal(np.array([int(n.cpu()[0]) for n in ns]), g["pid_n_err"][:, -1])


# ---- fused vehicle control ---------------------------------------------------------------------------------------------
def _vc_inputs(g, tag):
    K = g[f"vc_{tag}_target"].shape[0]
    path = np.repeat(g[f"vc_{tag}_path"][None], K, axis=0)
    n = np.full(K, int(g[f"vc_{tag}_n"]), np.int32)
    speed = np.array([_speed_kmh(v[3:6]) for v in g[f"vc_{tag}_vehicle"]])
    return dict(target_path=path, n_path=n, state=g[f"vc_{tag}_state"], vx=g[f"vc_{tag}_Vx"],
                min_index=g[f"vc_{tag}_min_index_in"].astype(np.int32), speed_kmh=speed, target_speed=g[f"vc_{tag}_target"],
                err=g[f"vc_{tag}_err_in"], n_err=g[f"vc_{tag}_n_err_in"].astype(np.int32))


def _lat_params(tag, para):
    from emplanner_carla_amd.api import lqr_params, mpc_params
    return mpc_params(vehicle_para=para) if tag == "mpc" else lqr_params(vehicle_para=para)


@pytest.mark.parametrize("tag", ["mpc", "lqr"])
def test_vehicle_control_replays_the_reference_run_step(pl, g, tag):
    """Every recorded step at once (B = steps, each with its own recorded state), one emp_vehicle_control launch."""
    from emplanner_carla_amd.api import pid_params
    para = tuple(g["vehicle_para"])
    a = _vc_inputs(g, tag)
    pl.set_timing(True)
    n0 = pl.kernel_launches("vehicle_control")
    r = pl.vehicle_control(_lat_params(tag, para), pid_params(), lateral=tag, **a)
    assert pl.kernel_launches("vehicle_control") == n0 + 1
    pl.set_timing(False)
    assert (r.status == 0).all() and len(r.status) >= 40
    want = g[f"vc_{tag}_control"]
    np.testing.assert_array_equal(r.control[:, 0], want[:, 0])          # throttle
    np.testing.assert_array_equal(r.control[:, 2], want[:, 2])          # brake
    _close(r.control[:, 1], want[:, 1], 1e-6, "steer")
    np.testing.assert_array_equal(r.err, g[f"vc_{tag}_err"])
    np.testing.assert_array_equal(r.n_err, g[f"vc_{tag}_n_err"])
    np.testing.assert_array_equal(r.min_index, g[f"vc_{tag}_min_index"])
    np.testing.assert_array_equal(r.k_r, g[f"vc_{tag}_k_r"])
    _close(r.e_rr, g[f"vc_{tag}_e_rr"], 1e-9, "e_rr")
    _close(r.pre_pro, g[f"vc_{tag}_pre_pro"], 1e-9, "pre_pro")
    # the lateral half is bit for bit the stand-alone entry point's
    lat = (pl.mpc_lateral if tag == "mpc" else pl.lqr_lateral)(_lat_params(tag, para), a["target_path"], a["n_path"], a["state"],
                                                               a["vx"], a["min_index"])
    for name, got in (("steer", r.lat_command), ("min_index", r.min_index), ("e_rr", r.e_rr), ("k_r", r.k_r),
                      ("pre_pro", r.pre_pro), ("status", r.status)):
        np.testing.assert_array_equal(got, getattr(lat, name), err_msg=name)
    # and the longitudinal half the stand-alone PID's
    pid = pl.pid_longitudinal(pid_params(), a["speed_kmh"], a["target_speed"], a["err"], a["n_err"])
    np.testing.assert_array_equal(r.lon_command, pid.command)


@pytest.mark.parametrize("tag", ["mpc", "lqr"])
def test_vehicle_control_failed_vehicle_keeps_its_pid_state(pl, g, tag):
    import torch
    from emplanner_carla_amd.api import pid_params
    para = tuple(g["vehicle_para"])
    a = {k: np.ascontiguousarray(v[5:8]).copy() for k, v in _vc_inputs(g, tag).items()}
    a["err"][1, :7] = np.arange(7) * 0.25 - 0.5
    a["n_err"][1] = 7
    if tag == "mpc":
        a["min_index"][1] = 999                  # IndexError in the reference
    else:
        a["n_path"][1] = 0                       # an empty path: IndexError
    r = pl.vehicle_control(_lat_params(tag, para), pid_params(), lateral=tag, **a)
    assert r.status[1] == ST_S_OUT_OF_RANGE and r.status[0] == 0 and r.status[2] == 0
    assert (r.control[1] == 0).all() and r.lon_command[1] == 0.0
    np.testing.assert_array_equal(r.err[1], a["err"][1])
    assert r.n_err[1] == 7
    sel = [0, 2]
    r2 = pl.vehicle_control(_lat_params(tag, para), pid_params(), lateral=tag, **{k: v[sel] for k, v in a.items()})
    for name in ("control", "lat_command", "lon_command", "err", "n_err", "min_index", "e_rr"):
        np.testing.assert_array_equal(getattr(r, name)[sel], getattr(r2, name), err_msg=name)
    # device tensors, PID state updated in place: the same bits
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in a.items()}
    rd = pl.vehicle_control(_lat_params(tag, para), pid_params(), lateral=tag, in_place=True, **t)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(t["err"].cpu().numpy(), r.err)
    np.testing.assert_array_equal(t["n_err"].cpu().numpy(), r.n_err)
    np.testing.assert_array_equal(rd.control.cpu().numpy(), r.control)
    # B = 0
    r0 = pl.vehicle_control(_lat_params(tag, para), pid_params(), lateral=tag, **{k: v[:0] for k, v in a.items()})
    assert r0.control.shape == (0, 3)


# ---- drop-ins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,ctype", [("mpc", "MPC_controller"), ("lqr", "LQR_controller")])
def test_dropin_vehicle_control_run_step(pl, g, tag, ctype):
    from emplanner_carla_amd.controller.controller import Vehicle_control
    para = tuple(g["vehicle_para"])
    path = [tuple(r) for r in g[f"vc_{tag}_path"][:int(g[f"vc_{tag}_n"])]]
    veh = FakeVehicle(g[f"vc_{tag}_vehicle"][0])
    vc = Vehicle_control(veh, para, path, controller_type=ctype)
    for k in range(g[f"vc_{tag}_target"].shape[0]):
        veh.s = [float(v) for v in g[f"vc_{tag}_vehicle"][k]]
        vc.Lat_control.min_index = int(g[f"vc_{tag}_min_index_in"][k])
        n = int(g[f"vc_{tag}_n_err_in"][k])
        vc.Lon_control.error_buffer = deque([float(v) for v in g[f"vc_{tag}_err_in"][k, :n]], maxlen=60)
        control = vc.run_step(float(g[f"vc_{tag}_target"][k]))
        want = g[f"vc_{tag}_control"][k]
        assert control.throttle == want[0] and control.brake == want[2], k
        assert abs(control.steer - want[1]) <= 1e-6, k
        assert (control.hand_brake, control.manual_gear_shift, control.gear) == (False, False, 1)
        L = vc.Lat_control
        assert L.min_index == g[f"vc_{tag}_min_index"][k] and L.k_r == g[f"vc_{tag}_k_r"][k]
        _close(L.e_rr, g[f"vc_{tag}_e_rr"][k], 1e-9, "e_rr")
        _close([L.x_pre, L.y_pre, L.x_pro, L.y_pro], g[f"vc_{tag}_pre_pro"][k], 1e-9, "pre_pro")
        m = int(g[f"vc_{tag}_n_err"][k])
        assert list(vc.Lon_control.error_buffer) == [float(v) for v in g[f"vc_{tag}_err"][k, :m]], k
        assert vc.Lon_control.error_buffer.maxlen == 60 and vc.Lon_control.target_speed == g[f"vc_{tag}_target"][k]


def test_dropin_vehicle_control_errors_and_fallback(pl, g):
    from emplanner_carla_amd.controller import controller as cc
    para = tuple(g["vehicle_para"])
    path = [tuple(r) for r in g["vc_mpc_path"][:int(g["vc_mpc_n"])]]
    veh = FakeVehicle(g["vc_mpc_vehicle"][3])
    with pytest.raises(AttributeError):
        cc.Vehicle_control(veh, para, path, controller_type="Stanley").run_step(30)
    vc = cc.Vehicle_control(veh, para, path)
    near = _speed_kmh(veh.s[3:6]) + 0.25         # inside the separation threshold: the buffer keeps its entries
    vc.run_step(near)
    vc.run_step(near)
    before = list(vc.Lon_control.error_buffer)
    assert len(before) == 2
    vc.Lat_control.min_index = 10_000
    with pytest.raises(IndexError):
        vc.run_step(near)
    assert list(vc.Lon_control.error_buffer) == before
    # a user's own lateral controller: _control() and PID_control() separately, the same actuation
    vc.Lat_control = NS(_control=lambda: float("nan"))
    c = vc.run_step(30.0)
    assert c.steer == -1 and c.gear == 1             # max(-1, nan) keeps -1, as the reference's expression does
    vc2 = cc.Vehicle_control(veh, para, path)
    vc2._max_steer = 0.1                         # limits the kernel does not know: the separate path, as the reference
    c = vc2.run_step(30.0)
    assert c.steer <= 0.1


def test_dropin_pid_with_custom_gains(pl, g):
    from emplanner_carla_amd.controller.controller import Longitudinal_PID_controller
    s = 2
    K_P, K_I, K_D, dt = g["pid_gains"][s]
    veh = FakeVehicle([0, 0, 0, 0, 0, 0, 0])
    pid = Longitudinal_PID_controller(veh, K_P=K_P, K_I=K_I, K_D=K_D, dt=dt)
    for k in range(g["pid_command"].shape[1]):
        veh.s[3:6] = [float(v) for v in g["pid_vel"][s, k]]
        assert pid.PID_control(float(g["pid_target"][s, k])) == g["pid_command"][s, k], k
        m = int(g["pid_n_err"][s, k])
        assert list(pid.error_buffer) == [float(v) for v in g["pid_err"][s, k, :m]], k
    pid.K_P = 3.0                                # gains are read at every call
    veh.s[3:6] = [30.0 / 3.6, 0.0, 0.0]
    pid.error_buffer.clear()
    assert pid.PID_control(30.5) == 3.0 * (30.5 - 3.6 * math.sqrt((30.0 / 3.6) ** 2))


def test_dropin_feedforward_mpc(pl, g):
    from emplanner_carla_amd.api import mpc_ff_params
    from emplanner_carla_amd.controller.controller import Lateral_MPC__with_feedforward_controller
    para = tuple(g["vehicle_para"])
    path = [tuple(r) for r in g["vc_mpc_path"][:int(g["vc_mpc_n"])]]
    veh = FakeVehicle(g["vc_mpc_vehicle"][6])
    m = Lateral_MPC__with_feedforward_controller(veh, para, path)
    assert m._vehicle_state is not None and m.min_index == 0
    steer = m.MPC_control()
    arr = np.array(path)[None]
    r = pl.mpc_ff_lateral(mpc_ff_params(vehicle_para=para), arr, np.array([len(path)], np.int32),
                          np.array([m._vehicle_state]), np.array([m._vehicle_Vx]), np.array([0], np.int32))
    assert steer == r.steer[0] and m.min_index == r.min_index[0] and m.k_r == r.k_r[0]
    assert m.e_rr == tuple(r.e_rr[0]) and (m.x_pre, m.y_pre, m.x_pro, m.y_pro) == tuple(r.pre_pro[0])
    w = port.ff_chain(para, np.array(path), m._vehicle_state, m._vehicle_Vx, 0)
    assert abs(steer - w["steer"]) <= 1e-6 and m.min_index == w["min_index"]


def test_control_entry_points_survive_hostile_arguments():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "control_fuzz_child.py")], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    tail = run.stdout[-3000:] + "\n" + run.stderr[-3000:]
    assert run.returncode == 0, f"the fuzz child died with {run.returncode}:\n{tail}"
    assert "CONTROL-FUZZ-OK" in run.stdout, tail
    last = run.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 30 and int(last[3]) >= 25, last
