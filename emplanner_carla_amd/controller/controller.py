"""Drop-in for reference controller/controller.py: Lateral_MPC_controller (:65-337), Lateral_LQR_controller (:374-611),
Longitudinal_PID_controller (:614-678), Vehicle_control (:680-724) and Lateral_MPC__with_feedforward_controller (:727-990).
Line numbers cite the reference file.  ``cal_vehicle_info`` and the speed read of the PID are the only parts that talk to
CARLA: they stay on the host, duck-typed; everything after them is one call of the C-ABI (batch of one vehicle):
``emp_mpc_lateral`` / ``emp_lqr_lateral`` / ``emp_pid_longitudinal`` / ``emp_mpc_ff_lateral``, and for
``Vehicle_control.run_step`` one ``emp_vehicle_control`` (lateral law, PID and actuation in one kernel launch).

The module defines the reference's classes and nothing else public: helpers are module-level functions."""
from __future__ import annotations

import math
import types
from collections import deque

import numpy as np

from ..api import mpc_ff_params, mpc_params, pid_params
from .._lib import PID_BUFFER
from ..planner._runtime import planner
from ..planner.vehicle_state import planar_state


class Lateral_MPC_controller(object):
    def __init__(self, ego_vehicle, vehicle_para, pathway_xy_theta_kappa):
        self._vehicle_state = None
        self._vehicle_para = vehicle_para
        self._vehicle = ego_vehicle
        self._vehicle_Vx = 0
        self._target_path = pathway_xy_theta_kappa
        self._N, self._P, self._n = 6, 2, 4                  # :72-74
        self.k_r = None
        self.e_rr = None
        self.min_index = 0
        self.x_pre = self.y_pre = self.x_pro = self.y_pro = 0

    def cal_vehicle_info(self):
        """:90-113 - the longitudinal speed keeps its sign but never drops below 0.005 in magnitude (the model divides by it)."""
        st = planar_state(self._vehicle)
        self._vehicle_state = (st.x, st.y, st.yaw, st.v_lat, st.yaw_rate)
        self._vehicle_Vx = math.copysign(max(abs(st.v_long), 0.005), st.v_long) if st.v_long != 0 else 0.005

    def _control(self):
        """:313-337 - returns the first control of the horizon (the raw steering command)."""
        self.cal_vehicle_info()
        path = np.asarray([[float(p[0]), float(p[1]), float(p[2]), float(p[3])] for p in self._target_path], dtype=np.float64)
        if not 0 <= self.min_index < len(path):
            raise IndexError("list index out of range")         # what the reference's self._target_path[min_index] does
        res = planner().mpc_lateral(mpc_params(vehicle_para=self._vehicle_para), path[None], np.array([len(path)], np.int32),
                                    np.array([self._vehicle_state], dtype=np.float64), np.array([self._vehicle_Vx]),
                                    np.array([self.min_index], np.int32))
        if int(res.status[0]) != 0:
            raise ValueError("lateral MPC: the box QP did not converge")
        self.min_index = int(res.min_index[0])
        self.e_rr = tuple(float(v) for v in res.e_rr[0])
        self.k_r = float(res.k_r[0])
        self.x_pre, self.y_pre, self.x_pro, self.y_pro = (float(v) for v in res.pre_pro[0])
        return float(res.steer[0])


class Lateral_LQR_controller(object):
    """Drop-in for reference class Lateral_LQR_controller (:374-611): same constructor and ``_control()``."""

    def __init__(self, ego_vehicle, vehicle_para, pathway_xy_theta_kappa):
        self._vehicle_para = vehicle_para
        self._vehicle = ego_vehicle
        self._vehicle_state = None
        self._vehicle_Vx = 0
        self._target_path = pathway_xy_theta_kappa
        self.K = None
        self.k_r = None
        self.e_rr = None
        self.delta_f = None
        self.min_index = 0
        self.x_pre = self.y_pre = self.x_pro = self.y_pro = 0

    def cal_vehicle_info(self):
        """:405-422 - no clamp on the longitudinal speed here (cal_A_B_fun adds 0.0001 instead, :439)."""
        st = planar_state(self._vehicle)
        self._vehicle_state = (st.x, st.y, st.yaw, st.v_lat, st.yaw_rate)
        self._vehicle_Vx = st.v_long

    def _control(self):
        """:585-611 - the raw steering command -K e_rr + delta_f."""
        from ..api import lqr_params
        self.cal_vehicle_info()
        path = np.asarray([[float(p[0]), float(p[1]), float(p[2]), float(p[3])] for p in self._target_path],
                          dtype=np.float64).reshape(-1, 4)
        if len(path) == 0:
            raise IndexError("list index out of range")
        res = planner().lqr_lateral(lqr_params(vehicle_para=self._vehicle_para), path[None], np.array([len(path)], np.int32),
                                    np.array([self._vehicle_state], dtype=np.float64), np.array([self._vehicle_Vx]),
                                    np.array([min(max(self.min_index, 0), len(path) - 1)], np.int32))
        if int(res.status[0]) != 0:
            raise IndexError("list index out of range")
        self.min_index = int(res.min_index[0])
        self.K = np.asarray(res.K[0]).reshape(1, 4)
        self.e_rr = tuple(float(v) for v in res.e_rr[0])
        self.k_r = float(res.k_r[0])
        self.x_pre, self.y_pre, self.x_pro, self.y_pro = (float(v) for v in res.pre_pro[0])
        return float(res.steer[0])


# ---- helpers of the PID / vehicle-control drop-ins (module functions: the module defines only the reference's classes) --
_ST_S_OUT_OF_RANGE = 2          # EMP_ST_S_OUT_OF_RANGE: where the reference raises IndexError


def _path_array(target_path):
    return np.asarray([[float(p[0]), float(p[1]), float(p[2]), float(p[3])] for p in target_path], dtype=np.float64).reshape(-1, 4)


def _speed_kmh(vehicle):
    """:647-649 - the speed the PID compares with its target, in km/h, as the reference computes it."""
    v = vehicle.get_velocity()
    return 3.6 * math.sqrt(v.x * v.x + v.y * v.y + v.z * v.z)


def _pid_gains(lon):
    """The gains as the controller holds them now (users change them between calls)."""
    return pid_params(K_P=lon.K_P, K_I=lon.K_I, K_D=lon.K_D, dt=lon.dt, error_threshold=lon.error_threshold)


def _pid_state(lon):
    """The error deque as emp_pid_longitudinal takes it: (1, 60) oldest first and the entry count."""
    buf = list(lon.error_buffer)[-PID_BUFFER:]
    err = np.zeros((1, PID_BUFFER), np.float64)
    err[0, :len(buf)] = buf
    return err, np.array([len(buf)], np.int32)


def _pid_store(lon, err, n):
    """Write the buffer after the call back into the controller's own deque object."""
    lon.error_buffer.clear()
    lon.error_buffer.extend(float(v) for v in np.asarray(err).reshape(-1)[:int(n)])


_control_type = []


def _vehicle_control(throttle, steer, brake):
    """carla.VehicleControl when carla imports, else a record with the same attributes (run_step, :685-688)."""
    if not _control_type:
        try:
            import carla
            _control_type.append(carla.VehicleControl)
        except ImportError:
            _control_type.append(types.SimpleNamespace)
    control = _control_type[0]()
    control.hand_brake = False
    control.manual_gear_shift = False
    control.gear = 1
    control.steer = steer
    control.throttle = throttle
    control.brake = brake
    return control


def _actuate(vc, current_steering, current_acceleration):
    """:705-718 in Python, with the controller's own limits: the path taken when run_step cannot use the fused kernel."""
    if current_steering >= 0:
        steering = min(vc._max_steer, current_steering)
    else:
        steering = max(vc.min_steer, current_steering)
    if current_acceleration >= 0:
        return min(vc._max_throttle, current_acceleration), steering, 0
    return 0, steering, max(vc._max_brake, current_acceleration)


def _fused_run_step(vc, lat, lon, target_speed):
    """Vehicle_control.run_step as ONE emp_vehicle_control call: the lateral law, the PID step and the actuation."""
    from ..api import lqr_params
    is_mpc = type(lat) is Lateral_MPC_controller
    lat.cal_vehicle_info()
    speed = _speed_kmh(vc._vehicle)
    path = _path_array(lat._target_path)
    if is_mpc:
        if not 0 <= lat.min_index < len(path):
            raise IndexError("list index out of range")
        min_index = lat.min_index
    else:
        if len(path) == 0:
            raise IndexError("list index out of range")
        min_index = min(max(lat.min_index, 0), len(path) - 1)
    err, n_err = _pid_state(lon)
    p_lat = mpc_params(vehicle_para=lat._vehicle_para) if is_mpc else lqr_params(vehicle_para=lat._vehicle_para)
    res = planner().vehicle_control(p_lat, _pid_gains(lon), path[None], np.array([len(path)], np.int32),
                                    np.array([lat._vehicle_state], dtype=np.float64), np.array([lat._vehicle_Vx], np.float64),
                                    np.array([min_index], np.int32), np.array([speed], np.float64),
                                    np.array([target_speed], np.float64), err, n_err, lateral="mpc" if is_mpc else "lqr")
    status = int(res.status[0])
    if status != 0:              # raised before PID_control runs (:700-702): the PID state stays as it was
        if is_mpc and status != _ST_S_OUT_OF_RANGE:
            raise ValueError("lateral MPC: the box QP did not converge")
        raise IndexError("list index out of range")
    lat.min_index = int(res.min_index[0])
    lat.e_rr = tuple(float(v) for v in res.e_rr[0])
    lat.k_r = float(res.k_r[0])
    lat.x_pre, lat.y_pre, lat.x_pro, lat.y_pro = (float(v) for v in res.pre_pro[0])
    lon.target_speed = target_speed
    _pid_store(lon, res.err[0], res.n_err[0])
    throttle, steer, brake = (float(v) for v in res.control[0])
    return _vehicle_control(throttle, steer, brake)


class Longitudinal_PID_controller(object):
    """Drop-in for reference class Longitudinal_PID_controller (:614-678): same constructor, public attributes and
    ``PID_control``; each call is one emp_pid_longitudinal call, bit-exact with the reference."""

    def __init__(self, ego_vehicle, K_P=1.15, K_I=0, K_D=0, dt=0.01):
        self._vehicle = ego_vehicle
        self.K_P = K_P
        self.K_I = K_I
        self.K_D = K_D
        self.dt = dt
        self.target_speed = None
        self.error_buffer = deque(maxlen=60)             # :637
        self.error_threshold = 1                         # :638

    def PID_fun(self):
        """:641-672 - one PID step against the vehicle's current speed."""
        err, n_err = _pid_state(self)
        res = planner().pid_longitudinal(_pid_gains(self), np.array([_speed_kmh(self._vehicle)], np.float64),
                                         np.array([self.target_speed], np.float64), err, n_err, in_place=True)
        _pid_store(self, err[0], n_err[0])
        return float(res.command[0])

    def PID_control(self, target_speed):
        self.target_speed = target_speed
        return self.PID_fun()


class Vehicle_control(object):
    """Drop-in for reference class Vehicle_control (:680-724).  ``run_step`` is one emp_vehicle_control call when
    ``Lat_control`` / ``Lon_control`` are this module's classes and the limits are the reference's; otherwise (a user
    replaced one of them) it calls ``_control()`` and ``PID_control()`` separately, as the reference does."""

    def __init__(self, ego_vehicle, vehicle_para, pathway, controller_type="MPC_controller"):
        self._vehicle = ego_vehicle
        self._max_throttle = 1
        self._max_brake = 1
        self._max_steer = 1
        self.min_steer = -1
        if controller_type == "MPC_controller":
            self.Lat_control = Lateral_MPC_controller(ego_vehicle, vehicle_para, pathway)
        elif controller_type == "LQR_controller":
            self.Lat_control = Lateral_LQR_controller(ego_vehicle, vehicle_para, pathway)
        self.Lon_control = Longitudinal_PID_controller(ego_vehicle)      # default gains (:692)

    def run_step(self, target_speed):
        lat, lon = self.Lat_control, self.Lon_control    # AttributeError for an unknown controller_type, as in the reference
        if (type(lat) in (Lateral_MPC_controller, Lateral_LQR_controller) and type(lon) is Longitudinal_PID_controller
                and (self._max_throttle, self._max_brake, self._max_steer, self.min_steer) == (1, 1, 1, -1)):
            return _fused_run_step(self, lat, lon, target_speed)
        current_steering = lat._control()
        current_acceleration = lon.PID_control(target_speed)
        return _vehicle_control(*_actuate(self, current_steering, current_acceleration))


class Lateral_MPC__with_feedforward_controller(object):
    """Drop-in for reference class Lateral_MPC__with_feedforward_controller (:727-990): same constructor (it reads the
    vehicle, :755-756) and ``MPC_control()``, one emp_mpc_ff_lateral call."""

    def __init__(self, ego_vehicle, vehicle_para, pathway_xy_theta_kappa):
        self._vehicle_state = None
        self._vehicle_para = vehicle_para
        self._vehicle = ego_vehicle
        self._vehicle_Vx = 0
        self._target_path = pathway_xy_theta_kappa
        self._N, self._P, self._n = 4, 2, 4              # :737-739
        self.k_r = None
        self.e_rr = None
        self.min_index = 0
        self.x_pre = self.y_pre = self.x_pro = self.y_pro = 0
        self.cal_vehicle_info()

    def cal_vehicle_info(self):
        """:758-776 - no clamp on the longitudinal speed (the model adds 0.0001 instead, :791)."""
        st = planar_state(self._vehicle)
        self._vehicle_state = (st.x, st.y, st.yaw, st.v_lat, st.yaw_rate)
        self._vehicle_Vx = st.v_long

    def MPC_control(self):
        """:972-990 - the first control of the horizon (the raw steering command)."""
        self.cal_vehicle_info()
        path = _path_array(self._target_path)
        if len(path) == 0:
            raise IndexError("list index out of range")
        res = planner().mpc_ff_lateral(mpc_ff_params(vehicle_para=self._vehicle_para), path[None],
                                       np.array([len(path)], np.int32), np.array([self._vehicle_state], dtype=np.float64),
                                       np.array([self._vehicle_Vx], np.float64), np.array([self.min_index], np.int32))
        status = int(res.status[0])
        if status == _ST_S_OUT_OF_RANGE:
            raise IndexError("list index out of range")
        if status != 0:
            raise ValueError("feed-forward MPC: the box QP did not converge")
        self.min_index = int(res.min_index[0])
        self.e_rr = tuple(float(v) for v in res.e_rr[0])
        self.k_r = float(res.k_r[0])
        self.x_pre, self.y_pre, self.x_pro, self.y_pro = (float(v) for v in res.pre_pro[0])
        return float(res.steer[0])
