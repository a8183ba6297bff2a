"""Routed traffic: a fleet of agents that follow global paths with the reference's LocalPlanner / VehiclePIDController law
(agents/navigation/local_planner.py, controller.py), on the device.

``TrafficAgents`` is the reference's LocalPlanner surface for a fleet: ``run_step()`` gives one tick's controls, ``done()`` says
whose queue is empty, ``set_speed()`` changes the target.  What the reference leaves to CARLA - moving the vehicles - is
``rollout(T)``: T ticks of [observe, control, vehicle model] in one kernel launch.  ``actors()`` is the fleet as rows of
``Planner.drive``'s ``actors``, so traffic and a planning fleet alternate without leaving the device:

    traffic = TrafficAgents(planner, route.global_path, route.n_global, state, 30.0)
    for period in range(K):
        actors = traffic.actors().reshape(1, A, 4).expand(B, A, 4).contiguous()      # every ego sees every agent
        res = planner.drive(..., actors=actors, n_act=n_act, K=1, T=T)
        traffic.rollout(round(T * vp_ego.dt / traffic.vp.dt))                       # the same span of time

Include/emplanner.h states the law and what of the reference is not reproduced."""
from __future__ import annotations

import numpy as np

from . import _lib as L
from . import api


class TrafficAgents:
    """A agents on paths (A, M, 4) / n_path (A,) - ``Planner.route(...)``'s ``global_path`` / ``n_global`` as they are - starting
    from state (A, 6) = x, y, fi, Vy, fi_dot, Vx.  NumPy arrays or torch CUDA tensors, never a mix; everything this object holds is
    of that kind and is updated in place.  target_speed: km/h, a number or (A,)."""

    def __init__(self, planner, paths, n_path, state, target_speed, params=None, vehicle=None, past_steer=None):
        self.planner = planner
        self.params = params if params is not None else api.agent_params()
        self.vp = vehicle if vehicle is not None else api.agent_vehicle_params(dt=self.params.dt)
        self._torch = api._is_torch(paths)
        if self._torch != api._is_torch(state):
            raise ValueError("paths and state must both be torch device tensors or both be host arrays")
        A = int(paths.shape[0])
        if tuple(paths.shape[2:]) != (4,) or tuple(state.shape) != (A, 6):
            raise ValueError("paths must be (A, M, 4) and state (A, 6)")
        self.A = A
        self.paths = self._own(paths, np.float64)
        self.n_path = self._own(n_path, np.int32)
        self.state = self._own(state, np.float64, copy=True)
        self.head = self._zeros((A,), np.int32)
        self.past_steer = self._zeros((A,), np.float64) if past_steer is None else self._own(past_steer, np.float64, copy=True)
        self.lon_err, self.lat_err = self._zeros((A, L.AGENT_BUFFER), np.float64), self._zeros((A, L.AGENT_BUFFER), np.float64)
        self.n_lon, self.n_lat = self._zeros((A,), np.int32), self._zeros((A,), np.int32)
        self.status = self._zeros((A,), np.int32)
        self.target_speed = self._zeros((A,), np.float64)
        self.set_speed(target_speed)

    # ---- arrays of the fleet's kind ---------------------------------------------------------------------------------------------
    def _own(self, x, dtype, copy=False):
        if self._torch:
            import torch
            t = x.to({np.float64: torch.float64, np.int32: torch.int32}[dtype]).contiguous()
            return t.clone() if copy and t.data_ptr() == x.data_ptr() else t
        a = np.ascontiguousarray(x, dtype=dtype)
        return a.copy() if copy and a is x else a

    def _zeros(self, shape, dtype):
        if self._torch:
            import torch
            return torch.zeros(shape, dtype={np.float64: torch.float64, np.int32: torch.int32}[dtype], device=self.paths.device)
        return np.zeros(shape, dtype)

    # ---- the LocalPlanner surface -----------------------------------------------------------------------------------------------
    def set_speed(self, speed):
        """ref LocalPlanner.set_speed: the target in km/h, one number for the fleet or one per agent."""
        if self._torch:
            import torch
            self.target_speed.copy_(torch.as_tensor(speed, dtype=torch.float64).to(self.target_speed.device).expand(self.A))
        else:
            self.target_speed[:] = np.broadcast_to(np.asarray(speed, np.float64), (self.A,))

    def run_step(self):
        """ref LocalPlanner.run_step for every agent: one tick's controls (A, 3) = throttle, steer, brake from the state as it
        is.  The agent state advances; the vehicles do not move (apply the controls with ``Planner.vehicle_step`` on ``state``,
        or use ``rollout``)."""
        obs = self.planner.agent_observe(self.state)
        r = self.planner.agent_control(self.params, self.paths, self.n_path, self.state, obs.forward, obs.speed_kmh, self.target_speed,
                                       self.head, self.past_steer, self.lon_err, self.n_lon, self.lat_err, self.n_lat, in_place=True)
        self.status = r.status
        return r.control

    def rollout(self, T, log_every=None):
        """T ticks of run_step + the vehicle model in one launch; the fleet's state and agent state are updated in place."""
        r = self.planner.agent_rollout(self.params, self.vp, self.paths, self.n_path, self.state, self.target_speed, self.head,
                                       self.past_steer, self.lon_err, self.n_lon, self.lat_err, self.n_lat, T, log_every=log_every,
                                       in_place=True)
        self.status = r.status
        return r

    def actors(self):
        """(A, 4) x, y, world-frame vx, vy: the fleet as rows of ``Planner.drive``'s ``actors``."""
        return self.planner.agent_observe(self.state).actors

    def done(self):
        """ref LocalPlanner.done per agent: (A,) bool, the waypoint queue is empty."""
        return self.head >= self.n_path.clamp(0, int(self.paths.shape[1])) if self._torch else \
            self.head >= np.clip(self.n_path, 0, self.paths.shape[1])
