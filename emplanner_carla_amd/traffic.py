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

``BehaviorTraffic`` is the same fleet with the reference's BehaviorAgent on top: W worlds of up to 64 agents that see the vehicles
of their own world - each other, and ``set_others()``'s, e.g. a planning fleet's egos - and follow, slow down or stop behind them.

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


class BehaviorTraffic(TrafficAgents):
    """W worlds of up to N <= 64 agents with the reference's BehaviorAgent car-following law: paths (W, N, M, 4), n_path (W, N),
    lane (W, N, M) int32 lane keys (``RouteResult.lane_key(graph)`` reshaped), state (W, N, 6), speed_limit km/h (a number, or
    (W, N)), n_world (W,) the live agents of each world (None: all N), extent (W, N) half extents in metres (a number: all alike;
    2.4 is a mid-size car's).  Arrays of one kind, as for ``TrafficAgents``.  The target speed is the law's own: it follows from the
    speed limit and the vehicle ahead."""

    def __init__(self, planner, paths, n_path, lane, state, speed_limit, n_world=None, extent=2.4, params=None, behavior=None,
                 vehicle=None):
        W, N = int(paths.shape[0]), int(paths.shape[1])
        if tuple(paths.shape[3:]) != (4,) or tuple(state.shape) != (W, N, 6) or tuple(lane.shape) != tuple(paths.shape[:3]):
            raise ValueError("paths must be (W, N, M, 4), lane (W, N, M) and state (W, N, 6)")
        if not 1 <= N <= L.TRAFFIC_MAX_WORLD:
            raise ValueError(f"a world holds 1 to {L.TRAFFIC_MAX_WORLD} agents, not {N}")
        self.W, self.N = W, N
        flat = lambda x: x.reshape((W * N,) + tuple(x.shape[2:]))
        super().__init__(planner, flat(paths), flat(n_path), flat(state), 0.0, params=params, vehicle=vehicle)
        self.behavior = behavior if behavior is not None else api.behavior_params()
        self.lane = self._own(lane, np.int32)
        self.speed_limit, self.extent = self._zeros((W, N), np.float64), self._zeros((W, N), np.float64)
        self.n_world = self._zeros((W,), np.int32)
        self._fill(self.n_world, N if n_world is None else n_world)
        self._fill(self.extent, extent)
        self.set_speed_limit(speed_limit)
        self.others = None
        self.tick = 0                  # ticks done: the clock of the others
        self.mode = self._zeros((W, N), np.int32)
        self.target_speed = self._zeros((W, N), np.float64)
        self.lights = self.walkers = None
        self.hazard = None             # emp_hazard_params, made when lights or walkers are first used
        self.last_light = self._zeros((W, N), np.int32)       # the light that holds each agent (_last_traffic_light), -1 for none
        self._fill(self.last_light, -1)
        self.cause = self._zeros((W, N), np.int32)

    def _fill(self, dst, value):
        if self._torch:
            import torch
            dst.copy_(torch.as_tensor(value, dtype=dst.dtype).to(dst.device).expand(dst.shape))
        else:
            dst[...] = np.broadcast_to(np.asarray(value, dst.dtype), dst.shape)

    def _world(self, x):
        return x.reshape((self.W, self.N) + tuple(x.shape[1:]))

    def _state_args(self):
        v = self._world
        return (v(self.head), v(self.past_steer), v(self.lon_err), v(self.n_lon), v(self.lat_err), v(self.n_lat))

    def _adopt(self, r):
        self.status = r.status.reshape(self.A)

    # ---- the BehaviorAgent surface ----------------------------------------------------------------------------------------------
    def set_speed(self, speed):
        """The law sets its own target from the speed limit: use ``set_speed_limit``."""
        if hasattr(self, "speed_limit"):
            raise AttributeError("BehaviorTraffic takes its target from the speed limit: use set_speed_limit")

    def set_speed_limit(self, limit):
        """What get_speed_limit returns, km/h: one number, or (W, N)."""
        self._fill(self.speed_limit, limit)

    def set_others(self, other=None, other_lane=None, n_other=None):
        """Vehicles the fleet does not drive: other (W, K, 5) = x, y, world-frame vx, vy, half extent (the first four columns are a
        row of ``Planner.drive``'s actors), other_lane (W, K) their lane keys, n_other (W,) (None: all K).  Their positions are
        those at the fleet's current tick: the clock restarts here.  None removes them."""
        if other is None:
            self.others = None
            return
        W, K = int(other.shape[0]), int(other.shape[1])
        if W != self.W or tuple(other.shape[2:]) != (5,) or not K <= L.TRAFFIC_MAX_WORLD:
            raise ValueError(f"other must be (W, K, 5) with K <= {L.TRAFFIC_MAX_WORLD}")
        n = self._zeros((W,), np.int32)
        self._fill(n, K if n_other is None else n_other)
        self.others = (n, self._own(other, np.float64), self._own(other_lane, np.int32))
        self.tick = 0

    def set_lights(self, light=None, light_lane=None, light_cycle=None, n_light=None):
        """Traffic lights: light (W, L, 4) = x, y, dx, dy, the location and forward vector of the lane waypoint under each light's
        trigger volume; light_lane (W, L) that waypoint's lane key (a light that governs several keys is listed once per key);
        light_cycle (W, L, 3) int32 = period, red_from, red_to in ticks: red while red_from <= tick mod period < red_to, on the
        fleet's clock ``tick``.  n_light (W,) (None: all L).  No agent is held by a light afterwards.  None removes them."""
        self._fill(self.last_light, -1)
        if light is None:
            self.lights = None
            return
        W, K = int(light.shape[0]), int(light.shape[1])
        if W != self.W or tuple(light.shape[2:]) != (4,) or not K <= L.HAZARD_MAX:
            raise ValueError(f"light must be (W, L, 4) with L <= {L.HAZARD_MAX}")
        n = self._zeros((W,), np.int32)
        self._fill(n, K if n_light is None else n_light)
        self.lights = (n, self._own(light, np.float64), self._own(light_lane, np.int32), self._own(light_cycle, np.int32))

    def set_walkers(self, walker=None, walker_lane=None, n_walker=None):
        """Pedestrians: walker (W, K, 5) = x, y, world-frame vx, vy, half extent, as they stand at the fleet's tick 0 (they move by
        the clock ``tick``, as the others do); walker_lane (W, K) their lane keys; n_walker (W,) (None: all K).  None removes them."""
        if walker is None:
            self.walkers = None
            return
        W, K = int(walker.shape[0]), int(walker.shape[1])
        if W != self.W or tuple(walker.shape[2:]) != (5,) or not K <= L.HAZARD_MAX:
            raise ValueError(f"walker must be (W, K, 5) with K <= {L.HAZARD_MAX}")
        n = self._zeros((W,), np.int32)
        self._fill(n, K if n_walker is None else n_walker)
        self.walkers = (n, self._own(walker, np.float64), self._own(walker_lane, np.int32))

    def _hazards(self):
        return self.lights is not None or self.walkers is not None

    def causes(self):
        """(W, N) int32 EMP_HZ_* of the last ``run_step``: why an agent made an emergency stop (light, walker, vehicle), 0 where it
        made none.  (A rollout reports ``cause_ticks`` and ``log_cause`` instead.)  Without lights and walkers: EMP_HZ_VEHICLE where
        the mode is EMERGENCY."""
        if self._hazards():
            return self.cause
        return (self.mode == L.BHV_EMERGENCY) * L.HZ_VEHICLE

    def _hazard_params(self):
        if self.hazard is None:
            self.hazard = api.hazard_params()
        return self.hazard

    def run_step(self):
        """ref BehaviorAgent.run_step for every agent: one tick's controls (W, N, 3).  The agent state advances, the vehicles do
        not move, the others' clock stands."""
        v = self._world
        obs = self.planner.agent_observe(self.state)
        if self._hazards():
            r = self.planner.agent_behave_hazards(self.params, self.behavior, self._hazard_params(), self.n_world, v(self.paths),
                                                  v(self.n_path), self.lane, v(self.state), v(obs.forward), v(obs.speed_kmh),
                                                  self.speed_limit, self.extent, *self._state_args(), self.last_light,
                                                  lights=self.lights, walkers=self.walkers,
                                                  others=self.others, tick0=self.tick, in_place=True)
            self._adopt(r)
            self.mode, self.target_speed, self.cause = r.mode, r.target_speed, r.cause
            return r.control
        r = self.planner.agent_behave(self.params, self.behavior, self.n_world, v(self.paths), v(self.n_path), self.lane, v(self.state),
                                      v(obs.forward), v(obs.speed_kmh), self.speed_limit, self.extent, *self._state_args(),
                                      others=self.others, tick0=self.tick, in_place=True)
        self._adopt(r)
        self.mode, self.target_speed = r.mode, r.target_speed
        return r.control

    def rollout(self, T, log_every=None):
        """T ticks of run_step + the vehicle model in one launch; state, agent state and the others' clock advance."""
        v = self._world
        if self._hazards():
            r = self.planner.traffic_rollout_hazards(self.params, self.behavior, self._hazard_params(), self.vp, self.n_world, v(self.paths),
                                                     v(self.n_path), self.lane, v(self.state), self.speed_limit, self.extent,
                                                     *self._state_args(), self.last_light, T, lights=self.lights, walkers=self.walkers,
                                                     others=self.others, tick0=self.tick, log_every=log_every, in_place=True)
            self._adopt(r)
            self.tick += int(T)
            return r
        r = self.planner.traffic_rollout(self.params, self.behavior, self.vp, self.n_world, v(self.paths), v(self.n_path), self.lane,
                                         v(self.state), self.speed_limit, self.extent, *self._state_args(), T, others=self.others,
                                         tick0=self.tick, log_every=log_every, in_place=True)
        self._adopt(r)
        self.tick += int(T)
        return r

    def modes(self):
        """(W, N) int32 EMP_BHV_* of the last ``run_step`` (a rollout reports ``mode_ticks`` and ``log_mode`` instead)."""
        return self.mode

    def actors(self):
        """(W, N, 4) x, y, world-frame vx, vy; rows of padding slots are observations of whatever their state holds."""
        return self._world(super().actors())

    def done(self):
        return self._world(super().done())


class World:
    """A planning fleet and a ``BehaviorTraffic`` in the same W worlds, driven together by ``Planner.world_drive``: world w holds
    the traffic's agents of that world and the egos ego_off[w] <= b < ego_off[w + 1] (ego_off (W + 1,), non-decreasing; an ego
    outside every range is in no world).  ``params`` are ``drive_timed``'s nine parameter blocks in its order (p, q, sp, sdp, sqp,
    dp, lat, pid, vp).  The ego arrays - global_path (B, G, 4), n_global (B,), ego_lane (B, G) (``RouteResult.lane_key(graph)``),
    state (B, 6), target_speed (B,) km/h, t0 (B,) (None: zeros), ego_extent (a number, or (B,)) - are of the traffic's kind (NumPy
    or torch CUDA); what changes is held here and updated in place.  ``drive(K)`` runs K periods of T ego ticks and
    Ta = round(T * vp.dt / traffic.params.dt) agent ticks and advances both clocks: ``tick`` here, ``traffic.tick`` there - the
    traffic's clock is never reset, so its lights keep their phase.  ``traffic.set_others`` is not used: the egos are exchanged
    every period."""

    def __init__(self, planner, traffic: BehaviorTraffic, params, global_path, n_global, ego_lane, state, target_speed, ego_off, T,
                 max_obs, max_act=None, max_other=None, max_dyn=8, ego_extent=2.4, t0=None, see_egos=False, lane_window=50,
                 lateral="mpc", tp=None, max_pts=None):
        if len(params) != 9:
            raise ValueError("params: drive_timed's nine parameter blocks (p, q, sp, sdp, sqp, dp, lat, pid, vp)")
        self.planner, self.traffic, self.params = planner, traffic, tuple(params)
        tr = traffic
        if api._is_torch(state) != tr._torch:
            raise ValueError("the egos' arrays and the traffic's must both be torch device tensors or both be host arrays")
        B, G = int(global_path.shape[0]), int(global_path.shape[1])
        self.B, self.T = B, int(T)
        vp = self.params[8]
        self.Ta = max(1, round(self.T * vp.dt / tr.params.dt))
        if abs(self.T * vp.dt - self.Ta * tr.params.dt) > 1e-9:
            raise ValueError(f"T * vp.dt = {self.T * vp.dt} s is no whole number of agent ticks of {tr.params.dt} s")
        self.max_obs, self.max_dyn, self.max_pts = int(max_obs), int(max_dyn), (int(max_pts) if max_pts else api.max_path_points(self.params[0]))
        self.max_act = int(max_act) if max_act is not None else min(64, tr.N + (B if see_egos else 0))
        self.max_other = int(max_other) if max_other is not None else min(64, max(B, 1))
        self.see_egos, self.lane_window, self.lateral, self.tp = bool(see_egos), int(lane_window), lateral, tp
        own, zeros = tr._own, tr._zeros
        self.global_path, self.n_global, self.ego_lane = own(global_path, np.float64), own(n_global, np.int32), own(ego_lane, np.int32)
        self.ego_off = own(ego_off, np.int32)
        self.state = own(state, np.float64, copy=True)
        self.target_speed = zeros((B,), np.float64)
        tr._fill(self.target_speed, target_speed)
        self.ego_extent = zeros((B,), np.float64)
        tr._fill(self.ego_extent, ego_extent)
        self.t0 = zeros((B,), np.float64) if t0 is None else own(t0, np.float64)
        self.accel = zeros((B, 2), np.float64)
        self.pre_match_index, self.track_len = zeros((B,), np.int32), zeros((B,), np.int32)
        self.track = zeros((B, self.max_pts + 1, 4), np.float64)
        self.held, self.cursor, self.speed_held = zeros((B,), np.int32), zeros((B,), np.int32), zeros((B,), np.int32)
        self.profile = zeros((B, 7, L.TIMED_POINTS), np.float64)
        tr._fill(self.profile, float("nan"))                  # no profile yet: the cap is tracked until a plan is adopted
        self.tick = 0                                          # ego ticks done

    def drive(self, K, logs=True):
        """K periods in one call -> ``WorldDriveResult``; both fleets' state and both clocks advance."""
        tr, v = self.traffic, self.traffic._world
        r = self.planner.world_drive(
            *self.params, tr.params, tr.behavior, tr._hazard_params(), tr.vp, self.global_path, self.n_global, self.state, self.accel,
            self.pre_match_index, self.track, self.track_len, self.held, self.t0, self.profile, self.cursor, self.speed_held,
            self.target_speed, self.ego_off, self.ego_extent, self.ego_lane, tr.n_world, v(tr.paths), v(tr.n_path), tr.lane,
            v(tr.state), tr.speed_limit, tr.extent, *tr._state_args(), tr.last_light, K, self.T, self.Ta, self.max_obs, self.max_act,
            self.max_other, max_dyn=self.max_dyn, tick0=self.tick, atick0=tr.tick, lights=tr.lights, walkers=tr.walkers,
            see_egos=self.see_egos, lane_window=self.lane_window, tp=self.tp, max_pts=self.max_pts, lateral=self.lateral, logs=logs,
            in_place=True)
        tr.status = r.traffic.status.reshape(tr.A)
        self.tick += int(K) * self.T
        tr.tick += int(K) * self.Ta
        return r
