"""Child process of tests/test_gpu_world.py: raw ctypes calls of emp_world_exchange, emp_traffic_rollout_epoch and emp_world_drive
with host pointers and hostile arguments - ego offsets that decrease or leave [0, B], periods of different length, the agents' clock
out of range, other_tick0 < 0 and > tick0, NULL for every required array and struct in turn, reserved != 0 in each struct,
EMP_HOST_PINNED, the sizes out of range.  Each must return EMP_ERR_INVALID with a message and launch nothing (the context's launch
counters stay at 0); then the empty batches, which must be accepted, and clean calls.  Refusals only: nothing here is meant to
fault.  Prints one line per probe and, last, 'WORLD-FUZZ-OK <probes> probes <errors> errors'."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import world_port as wp  # noqa: E402
from emplanner_carla_amd import _lib as L  # noqa: E402

lib = L.load()
h = C.c_void_p()
assert lib.emp_create(0, C.byref(h)) == 0
ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
probes = errors = 0
KERNELS = (b"world_exchange", b"traffic_rollout_hazards", b"drive_request_timed", b"drive_adopt_timed", b"rollout_timed", b"drive_accel",
           b"project", b"speed_front")
INT32_MAX = 2 ** 31 - 1


def launches():
    return sum(lib.emp_kernel_launches(h, k) for k in KERNELS)


def expect(rc, what, ok=False):
    global probes, errors
    probes += 1
    msg = lib.emp_last_error(h)
    if ok:
        assert rc == 0, f"{what}: rejected (rc {rc}: {msg.decode() if msg else ''})"
    else:
        assert rc == -1, f"{what}: rc {rc}, EMP_ERR_INVALID expected"
        assert msg, f"{what}: error without a message"
        assert launches() == 0, f"{what}: a kernel was launched"
        errors += 1
    print(f"{what}: rc {rc} {msg.decode()[:70] if rc < 0 and msg else ''}")


W, NW, MP, B, G, A, MO, MD, M, K, T, N, KO = 2, 2, 40, 3, 80, 4, 4, 2, 60, 2, 3, L.TIMED_POINTS, 2
dp, qp, sp, sdp, sqp = L.DpParams(), L.QpParams(), L.SmoothParams(), L.SpeedDpParams(), L.SpeedQpParams()
lib.emp_dp_params_default(C.byref(dp))
lib.emp_qp_params_default(C.byref(qp))
lib.emp_smooth_params_default(C.byref(sp))
lib.emp_speed_dp_params_default(C.byref(sdp))
lib.emp_speed_qp_params_default(C.byref(sqp))
drv, tp, mp, pid, vp = L.DriveParams(), L.DriveTimedParams(), L.MpcParams(), L.PidParams(), L.VehicleParams()
lib.emp_drive_params_default(C.byref(drv))
lib.emp_drive_timed_params_default(C.byref(tp))
lib.emp_mpc_params_default(C.byref(mp))
lib.emp_pid_params_default(C.byref(pid))
lib.emp_vehicle_params_default(C.byref(vp))
ap, bp, hp, avp = L.AgentParams(), L.BehaviorParams(), L.HazardParams(), L.VehicleParams()
lib.emp_agent_params_default(C.byref(ap))
lib.emp_behavior_params_default(C.byref(bp), 1)
lib.emp_hazard_params_default(C.byref(hp))
lib.emp_vehicle_params_default(C.byref(avp))
ap.dt = avp.dt = vp.dt                                         # Ta = T covers the same span of time
wdef = L.WorldParams()
lib.emp_world_params_default(C.byref(wdef))
assert (wdef.lane_window, wdef.see_egos, wdef.Ta, wdef.atick0, wdef.reserved) == (50, 0, 1, 0, 0)
lib.emp_world_params_default(None)                             # a NULL block is ignored

gp = np.zeros((B, G, 4))
gp[:, :, 0] = np.arange(G) * 2.0
gp[:, :, 1] = 100.0 * np.arange(B)[:, None]
e = dict(global_path=gp, n_global=np.full(B, G, np.int32),
         state=np.column_stack([np.full(B, 10.0), 100.0 * np.arange(B) + 0.2, np.zeros(B), np.zeros(B), np.zeros(B), np.full(B, 8.0)]),
         accel=np.zeros((B, 2)), pre_match_index=np.full(B, 5, np.int32), track=np.zeros((B, M + 1, 4)), track_len=np.zeros(B, np.int32),
         held=np.zeros(B, np.int32), t0=np.array([0.0, 10.0, 20.5]), profile=np.full((B, 7, N), np.nan), cursor=np.zeros(B, np.int32),
         speed_held=np.zeros(B, np.int32), target=np.full(B, 30.0), ego_off=np.array([0, 2, 3], np.int32), ego_extent=np.full(B, 2.0),
         ego_lane=np.tile(np.arange(B, dtype=np.int32)[:, None], (1, G)))
EGO_IN = ("global_path", "n_global", "state", "accel", "pre_match_index", "track", "track_len", "held", "t0", "profile", "cursor",
          "speed_held", "ego_off", "ego_extent", "ego_lane")
EGO_OUT = dict(state_out=(B, 6), accel_out=(B, 2), actors_out=(B, A, 4), pre_match_index_out=(B,), track_out=(B, M + 1, 4),
               track_len_out=(B,), held_out=(B,), profile_out=(B, 7, N), cursor_out=(B,), speed_held_out=(B,))
LOGS = dict(log_state=(K, B, 6), log_plan_status=(K, B), log_roll_status=(K, B), log_held=(K, B), log_counts=(K, B, 2),
            log_traj=(K, B, M + 1, 4), log_traj_len=(K, B), log_speed_status=(K, B), log_speed_held=(K, B), log_tgt_status=(K, B),
            log_cursor=(K, B), log_wx_status=(K, B), log_n_act=(K, B), log_agent_state=(K, W, NW, 6), log_agent_status=(K, W, NW),
            log_done_tick=(K, W, NW), log_mode_ticks=(K, W, NW, 5), log_cause_ticks=(K, W, NW, 3), log_min_gap=(K, W, NW),
            log_min_walker_gap=(K, W, NW))
FLOAT = {"state_out", "accel_out", "actors_out", "track_out", "profile_out", "log_state", "log_traj", "log_agent_state", "log_min_gap",
         "log_min_walker_gap"}
for name, shape in {**EGO_OUT, **LOGS}.items():
    e[name] = np.zeros(shape, np.float64 if name in FLOAT else np.int32)
# the traffic: an agent 30 m ahead of each ego on its road, at 6 m/s
t = wp.traffic_of([[(40.0, 0.5, 0.0, 6.0, 25.0, 0), (40.0, 100.5, 0.0, 6.0, 25.0, 1)], [(40.0, 200.5, 0.0, 6.0, 25.0, 2)]], NW, MP)
AGENT_IN = ("n_world", "path", "n_path", "lane", "state", "speed_limit", "extent", "head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat")
AGENT_OUT = dict(head_out="head", past_steer_out="past_steer", lon_err_out="lon_err", n_lon_out="n_lon", lat_err_out="lat_err",
                 n_lat_out="n_lat", state_out="state")
t.update({k: np.zeros_like(t[v]) for k, v in AGENT_OUT.items()})
t.update(status=np.zeros((W, NW), np.int32), done_tick=np.zeros((W, NW), np.int32), mode_ticks=np.zeros((W, NW, 5), np.int32),
         min_gap=np.zeros((W, NW)), actors_out=np.zeros((W, NW, 4)), last_light_out=np.zeros((W, NW), np.int32),
         cause_ticks=np.zeros((W, NW, 3), np.int32), min_walker_gap=np.zeros((W, NW)),
         n_other=np.zeros(W, np.int32), other=np.zeros((W, KO, 5)), other_lane=np.zeros((W, KO), np.int32))
AGENT_REQUIRED = AGENT_IN + tuple(AGENT_OUT) + ("status", "done_tick", "mode_ticks", "min_gap")
HAZARD_REQUIRED = ("last_light", "last_light_out", "cause_ticks", "min_walker_gap")


def traffic_structs(others=False, reserved=0, hreserved=0, **kw):
    arrays = dict(t)
    arrays.update(kw)
    io, hz = L.BehaviorIO(), L.HazardIO()
    for name in AGENT_REQUIRED + ("actors_out",) + (("n_other", "other", "other_lane") if others else ()):
        setattr(io, name, ptr(arrays[name]))
    for name in HAZARD_REQUIRED:
        setattr(hz, name, ptr(arrays[name]))
    for name in ("log_state", "log_cause"):
        if name in kw:
            setattr(io if name == "log_state" else hz, name, ptr(kw[name]))
    io.reserved, hz.reserved = reserved, hreserved
    return io, hz


def world(ctx=h, d=C.byref(drv), a_=C.byref(ap), b_=C.byref(bp), av=C.byref(avp), hp_=C.byref(hp), law=L.EMP_LAT_MPC, b=B, mo=MO, m=M, ma=A,
          md=MD, k=K, tt=T, tick0=0, where=L.EMP_HOST, reserved=0, target=True, w=W, nw=NW, mp_=MP, ko=KO, ml=0, mw=0, ta=T, window=50,
          see=0, wreserved=0, atick0=0, agents=True, hazards=True, wparams=True, treserved=0, hreserved=0, tkw=None, **kw):
    arrays = dict(e)
    arrays.update(kw)
    io = L.WorldIO()
    for name in EGO_IN + tuple(EGO_OUT) + tuple(LOGS):
        setattr(io, name, ptr(arrays[name]))
    tio, hz = traffic_structs(reserved=treserved, hreserved=hreserved, **(tkw or {}))
    io.agents = C.pointer(tio) if agents else None
    io.hazards = C.pointer(hz) if hazards else None
    io.reserved = reserved
    wp_ = L.WorldParams(w, nw, mp_, ko, ml, mw, ta, window, see, wreserved, atick0)
    return lib.emp_world_drive(ctx, C.byref(dp), C.byref(qp), C.byref(sp), C.byref(sdp), C.byref(sqp), d, C.byref(tp), law, C.byref(mp),
                               C.byref(pid), C.byref(vp), a_, b_, av, hp_, C.byref(wp_) if wparams else None, b, G, mo, m, ma, md, k, tt,
                               tick0, ptr(e["target"]) if target else None, C.byref(io), where)


x = dict(actors=np.zeros((B, A, 4)), n_act=np.zeros(B, np.int32), other=np.zeros((W, KO, 5)), other_lane=np.zeros((W, KO), np.int32),
         n_other=np.zeros(W, np.int32), wx_status=np.zeros(B, np.int32))
X_IN = dict(n_world=t["n_world"], agent_state=t["state"], ego_off=e["ego_off"], ego_state=e["state"], ego_extent=e["ego_extent"],
            global_path=e["global_path"], n_global=e["n_global"], ego_lane=e["ego_lane"], pre_match_index=e["pre_match_index"])


def exchange(ctx=h, w=W, nw=NW, b=B, g=G, ma=A, ko=KO, window=50, see=0, where=L.EMP_HOST, reserved=0, io=True, **kw):
    arrays = dict(X_IN, **x)
    arrays.update(kw)
    s = L.WorldExchangeIO()
    for name in arrays:
        setattr(s, name, ptr(arrays[name]))
    s.reserved = reserved
    return lib.emp_world_exchange(ctx, w, nw, b, g, ma, ko, window, see, C.byref(s) if io else None, where)


def epoch(tick0=40, other_tick0=40, tt=4, **kw):
    io, hz = traffic_structs(others=True, **kw)
    return lib.emp_traffic_rollout_epoch(h, C.byref(ap), C.byref(bp), C.byref(avp), W, NW, MP, KO, tt, 1, tick0, C.byref(io), L.EMP_HOST,
                                         C.byref(hp), 0, 0, C.byref(hz), other_tick0)


off = lambda *v: np.array(v, np.int32)
assert lib.emp_set_timing(h, 1) == 0                           # launches are counted from here on
# ---- emp_world_exchange
for bad in (off(0, 3, 2), off(-1, 2, 3), off(0, 2, 4), off(1, 0, 3), off(0, INT32_MAX, 3), off(0, 2, -2 ** 31)):
    expect(exchange(ego_off=bad), f"exchange: ego_off = {bad.tolist()}")
expect(exchange(io=False), "exchange: NULL struct")
expect(exchange(reserved=1), "exchange: reserved = 1")
expect(exchange(where=L.EMP_HOST_PINNED), "exchange: EMP_HOST_PINNED")
for kw in (dict(w=-1), dict(b=-1), dict(nw=0), dict(nw=65), dict(g=0), dict(ma=0), dict(ma=65), dict(ko=-1), dict(ko=65), dict(window=-1),
           dict(see=2), dict(see=-1)):
    expect(exchange(**kw), f"exchange: {kw}")
for name in tuple(X_IN) + tuple(x):
    expect(exchange(**{name: None}), f"exchange: NULL {name}")
# ---- emp_traffic_rollout_epoch
expect(epoch(other_tick0=41), "epoch: other_tick0 = tick0 + 1")
expect(epoch(other_tick0=-1), "epoch: other_tick0 = -1")
expect(epoch(tick0=0, other_tick0=1), "epoch: other_tick0 = 1 at tick0 = 0")
expect(epoch(other_tick0=2 ** 40), "epoch: other_tick0 = 2^40")
expect(epoch(tick0=-1, other_tick0=-1), "epoch: tick0 = -1")
expect(epoch(reserved=1), "epoch: emp_behavior_io.reserved = 1")
expect(epoch(hreserved=1), "epoch: emp_hazard_io.reserved = 1")
expect(epoch(state=None), "epoch: NULL state")
expect(epoch(cause_ticks=None), "epoch: NULL cause_ticks")
# ---- emp_world_drive
for bad in (off(0, 3, 2), off(-1, 2, 3), off(0, 2, 4), off(2, 1, 3)):
    expect(world(ego_off=bad), f"world_drive: ego_off = {bad.tolist()}")
expect(world(ta=T + 1), "world_drive: Ta = T + 1 at equal tick lengths")
expect(world(ta=1), "world_drive: Ta = 1 against T = 3")
expect(world(ta=0), "world_drive: Ta = 0")
expect(world(atick0=-1), "world_drive: atick0 = -1")
expect(world(atick0=INT32_MAX - K * T + 1), "world_drive: atick0 + K * Ta = INT32_MAX + 1")
expect(world(tick0=-1), "world_drive: tick0 = -1")
expect(world(tick0=INT32_MAX - K * T + 1), "world_drive: tick0 + K * T = INT32_MAX + 1")
expect(world(d=None), "world_drive: NULL drive params")
expect(world(a_=None), "world_drive: NULL agent params")
expect(world(b_=None), "world_drive: NULL behavior params")
expect(world(av=None), "world_drive: NULL agent vehicle params")
expect(world(hp_=None), "world_drive: NULL hazard params")
expect(world(wparams=False), "world_drive: NULL world params")
expect(world(agents=False), "world_drive: NULL emp_behavior_io")
expect(world(hazards=False), "world_drive: NULL emp_hazard_io")
expect(world(reserved=7), "world_drive: emp_world_io.reserved = 7")
expect(world(wreserved=1), "world_drive: emp_world_params.reserved = 1")
expect(world(treserved=1), "world_drive: emp_behavior_io.reserved = 1")
expect(world(hreserved=1), "world_drive: emp_hazard_io.reserved = 1")
expect(world(where=L.EMP_HOST_PINNED), "world_drive: EMP_HOST_PINNED")
expect(world(law=2), "world_drive: lateral = 2")
expect(world(tkw=dict(log_state=np.zeros((T, W, NW, 6)))), "world_drive: a tick log of emp_behavior_io")
for kw in (dict(k=0), dict(k=L.DRIVE_MAX_PERIODS + 1), dict(tt=0, ta=0), dict(ma=0), dict(ma=65), dict(md=0), dict(mo=254), dict(m=256),
           dict(b=-1), dict(w=-1), dict(nw=0), dict(nw=65), dict(mp_=0), dict(ko=65), dict(ml=65), dict(mw=-1), dict(window=-1), dict(see=2)):
    expect(world(**kw), f"world_drive: {kw}")
expect(world(target=False), "world_drive: NULL target_speed")
for name in tuple(k_ for k_ in EGO_IN if k_ != "accel") + tuple(EGO_OUT):
    expect(world(**{name: None}), f"world_drive: NULL {name}")
for name in AGENT_REQUIRED + HAZARD_REQUIRED:
    expect(world(tkw={name: None}), f"world_drive: NULL traffic {name}")
assert launches() == 0
# ---- accepted
expect(exchange(w=0), "exchange: W = 0", ok=True)
expect(exchange(b=0, ego_off=off(0, 0, 0)), "exchange: B = 0", ok=True)
assert launches() == 0
expect(exchange(see=1), "exchange: clean", ok=True)
assert x["n_act"].tolist() == [3, 3, 1] and x["n_other"].tolist() == [2, 1] and x["other_lane"].tolist() == [[0, 1], [2, -1]]
assert not x["wx_status"].any() and np.array_equal(x["other"][0, 0], [10.0, 0.2, 8.0, 0.0, 2.0])
expect(exchange(ko=0, other=None, other_lane=None, n_other=None), "exchange: max_other = 0 without its arrays", ok=True)
assert (x["wx_status"] == L.WX_NOT_LISTED).all()
expect(epoch(), "epoch: clean", ok=True)
expect(world(w=0), "world_drive: W = 0", ok=True)
expect(world(b=0, ego_off=off(0, 0, 0)), "world_drive: B = 0", ok=True)
expect(world(), "world_drive: clean", ok=True)
clean = {k_: e[k_].copy() for k_ in tuple(EGO_OUT) + tuple(LOGS)}
assert (e["log_n_act"] == [2, 2, 1]).all() and not e["log_wx_status"].any()
assert (e["log_counts"][:, :, 1] == 1).all(), "each ego's agent is its dynamic actor"
assert np.array_equal(e["log_agent_state"][0], t["state"]) and np.isfinite(e["state_out"]).all() and np.isfinite(t["state_out"]).all()
assert lib.emp_kernel_launches(h, b"world_exchange") == K + 2 and lib.emp_kernel_launches(h, b"traffic_rollout_hazards") == K + 1
assert lib.emp_kernel_launches(h, b"drive_request_timed") == K and lib.emp_kernel_launches(h, b"rollout_timed") == K
expect(world(accel=None, **{k_: None for k_ in LOGS}), "world_drive: optional pointers NULL", ok=True)
for k_ in clean:
    e[k_][...] = 0
expect(world(), "world_drive: clean again", ok=True)
for k_ in clean:
    assert np.array_equal(e[k_], clean[k_], equal_nan=True), k_
lib.emp_destroy(h)
print(f"WORLD-FUZZ-OK {probes} probes {errors} errors")
