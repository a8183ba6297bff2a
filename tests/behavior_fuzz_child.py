"""Child process of tests/test_gpu_behavior.py: raw ctypes calls of emp_agent_behave and emp_traffic_rollout with host pointers and
arguments the header says are refused BEFORE any launch - a NULL context or parameter block, max_world 0 and 65, max_other -1 and 65,
max_path 0, W < 0, T = 0 and above EMP_ROLLOUT_MAX_TICKS, log_every = 0, tick0 < 0, reserved != 0 in each block, EMP_HOST_PINNED,
NULL for every required pointer in turn, others asked for without their arrays; then NULL for every optional pointer and W = 0,
which must be accepted.  Contract (include/emplanner.h): a call returns EMP_OK or a negative emp_error with a message, never
crashes, and a clean call afterwards still yields the clean answer.  Prints one line per probe and, last,
'BEHAVIOR-FUZZ-OK <probes> probes <errors> errors'."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emplanner_carla_amd import _lib as L  # noqa: E402

lib = L.load()
h = C.c_void_p()
assert lib.emp_create(0, C.byref(h)) == 0
probes = errors = 0


def expect(rc, what, ok=False, ctx=True):
    global probes, errors
    probes += 1
    msg = lib.emp_last_error(h)
    if ok:
        assert rc == 0, f"{what}: rejected (rc {rc}: {msg.decode() if msg else ''})"
    else:
        assert rc < 0, f"{what}: accepted (rc {rc})"
        assert msg or not ctx, f"{what}: error {rc} without a message"
        errors += 1
    print(f"{what}: rc {rc} {msg.decode()[:70] if rc < 0 and msg else ''}")


W, N, M, K, T = 2, 3, 12, 2, 6
A = W * N
arr = dict(
    n_world=np.array([3, 2], np.int32), path=np.zeros((W, N, M, 4)), n_path=np.full((W, N), M, np.int32), lane=np.ones((W, N, M), np.int32),
    state=np.zeros((W, N, 6)), forward=np.zeros((W, N, 2)), speed_kmh=np.full((W, N), 18.0), speed_limit=np.full((W, N), 60.0),
    extent=np.full((W, N), 2.0), head=np.zeros((W, N), np.int32), past_steer=np.zeros((W, N)), lon_err=np.zeros((W, N, 10)),
    n_lon=np.zeros((W, N), np.int32), lat_err=np.zeros((W, N, 10)), n_lat=np.zeros((W, N), np.int32), n_other=np.array([1, 0], np.int32),
    other=np.zeros((W, K, 5)), other_lane=np.ones((W, K), np.int32))
arr["path"][..., 0] = 6.0 + 2.0 * np.arange(M)
arr["path"][..., 0] += 9.0 * np.arange(N)[None, :, None]                        # three in a row, 9 m apart, slightly staggered
arr["path"][..., 1] = 0.4 * np.arange(N)[None, :, None]
arr["state"][..., 0], arr["state"][..., 1], arr["state"][..., 5] = 9.0 * np.arange(N), 0.4 * np.arange(N), 5.0
arr["forward"][..., 0] = 1.0
arr["other"][0, 0] = (30.0, 1.0, 0.0, 0.0, 2.0)
out = dict(
    head_out=np.zeros((W, N), np.int32), past_steer_out=np.zeros((W, N)), lon_err_out=np.zeros((W, N, 10)), n_lon_out=np.zeros((W, N), np.int32),
    lat_err_out=np.zeros((W, N, 10)), n_lat_out=np.zeros((W, N), np.int32), status=np.zeros((W, N), np.int32), control=np.zeros((W, N, 3)),
    mode=np.zeros((W, N), np.int32), blocker=np.zeros((W, N), np.int32), distance=np.zeros((W, N)), ttc=np.zeros((W, N)),
    target_speed_out=np.zeros((W, N)), lat_error=np.zeros((W, N)), lon_command=np.zeros((W, N)), state_out=np.zeros((W, N, 6)),
    done_tick=np.zeros((W, N), np.int32), mode_ticks=np.zeros((W, N, 5), np.int32), min_gap=np.zeros((W, N)), actors_out=np.zeros((W, N, 4)),
    log_state=np.zeros((T, W, N, 6)), log_control=np.zeros((T, W, N, 3)), log_head=np.zeros((T, W, N), np.int32),
    log_mode=np.zeros((T, W, N), np.int32), log_target=np.zeros((T, W, N)))
prm, bp, vp = L.AgentParams(), L.BehaviorParams(), L.VehicleParams()
lib.emp_agent_params_default(C.byref(prm))
lib.emp_behavior_params_default(C.byref(bp), L.BHV_KINDS["normal"])
lib.emp_behavior_params_default(None, 1)                       # a NULL block is ignored
assert (bp.max_speed, bp.braking_distance, bp.min_speed, bp.emergency_brake, bp.up_angle, bp.look_steps, bp.reserved) == (50.0, 5.0, 5.0, 0.5, 30.0, 5, 0)
lib.emp_vehicle_params_default(C.byref(vp))
vp.Cf, vp.Cr, vp.m, vp.dt = -148970.0, -82204.0, 1412.0, 0.05


def bad(block):
    b = type(block).from_buffer_copy(block)
    b.reserved = 1
    return b


def io_of(**kw):
    io = L.BehaviorIO()
    d = dict(arr, **out)
    d.update(kw)
    for k, v in d.items():
        setattr(io, k, None if v is None else v.ctypes.data)
    io.reserved = 0
    return io


BEHAVE_REQUIRED = ("n_world", "path", "n_path", "lane", "state", "forward", "speed_kmh", "speed_limit", "extent", "head", "past_steer", "lon_err",
                   "n_lon", "lat_err", "n_lat", "head_out", "past_steer_out", "lon_err_out", "n_lon_out", "lat_err_out", "n_lat_out", "status",
                   "control", "mode", "blocker", "distance", "ttc", "target_speed_out")
ROLLOUT_REQUIRED = tuple(k for k in BEHAVE_REQUIRED if k not in ("forward", "speed_kmh", "control", "mode", "blocker", "distance", "ttc",
                                                                 "target_speed_out")) + ("state_out", "done_tick", "mode_ticks", "min_gap")


def behave(ctx=h, p=prm, b=bp, w=W, n=N, m=M, k=K, tick0=0, io=None, where=L.EMP_HOST):
    io = io or io_of()
    return lib.emp_agent_behave(ctx, C.byref(p) if p else None, C.byref(b) if b else None, w, n, m, k, tick0, C.byref(io) if io != "null" else None, where)


def rollout(ctx=h, p=prm, b=bp, v=vp, w=W, n=N, m=M, k=K, t=T, every=1, tick0=0, io=None, where=L.EMP_HOST):
    io = io or io_of()
    return lib.emp_traffic_rollout(ctx, C.byref(p) if p else None, C.byref(b) if b else None, C.byref(v) if v else None, w, n, m, k, t, every,
                                   tick0, C.byref(io) if io != "null" else None, where)


def snapshot():
    return {k: v.copy() for k, v in out.items()}


expect(behave(), "behave: clean", ok=True)
clean_b = snapshot()
assert clean_b["mode"][0, 0] != 0 and clean_b["blocker"][0, 0] == 0 and clean_b["mode"][1, 1] == 0, clean_b["mode"]
expect(rollout(), "rollout: clean", ok=True)
clean_r = snapshot()
assert (clean_r["mode_ticks"].sum(-1)[[0, 0, 0, 1, 1], [0, 1, 2, 0, 1]] == T).all() and clean_r["mode_ticks"][0, 0, 1:].sum() > 0

for name, call in (("behave", behave), ("rollout", rollout)):
    expect(call(ctx=None), f"{name}: NULL context", ctx=False)
    expect(call(p=None), f"{name}: NULL agent params")
    expect(call(b=None), f"{name}: NULL behaviour params")
    expect(call(io="null"), f"{name}: NULL io")
    expect(call(p=bad(prm)), f"{name}: agent params reserved")
    expect(call(b=bad(bp)), f"{name}: behaviour params reserved")
    io = io_of()
    io.reserved = 1
    expect(call(io=io), f"{name}: io reserved")
    for kw, what in ((dict(n=0), "max_world 0"), (dict(n=65), "max_world 65"), (dict(k=-1), "max_other -1"), (dict(k=65), "max_other 65"),
                     (dict(m=0), "max_path 0"), (dict(w=-1), "W -1"), (dict(tick0=-1), "tick0 -1"), (dict(where=L.EMP_HOST_PINNED), "EMP_HOST_PINNED")):
        expect(call(**kw), f"{name}: {what}")
    for k in (BEHAVE_REQUIRED if name == "behave" else ROLLOUT_REQUIRED):
        expect(call(io=io_of(**{k: None})), f"{name}: NULL {k}")
    for k in ("n_other", "other", "other_lane"):
        expect(call(io=io_of(**{k: None})), f"{name}: others without {k}")
    expect(call(k=0, io=io_of(n_other=None, other=None, other_lane=None)), f"{name}: no others at all", ok=True)
    expect(call(w=0), f"{name}: W = 0", ok=True)
    expect(call(w=0, n=0), f"{name}: W = 0 does not excuse max_world 0")
expect(rollout(v=None), "rollout: NULL vehicle params")
expect(rollout(v=bad(vp)), "rollout: vehicle params reserved")
expect(rollout(t=0), "rollout: T 0")
expect(rollout(t=65537), "rollout: T 65537")
expect(rollout(every=0), "rollout: log_every 0")
expect(rollout(tick0=2 ** 31 - 3), "rollout: tick0 + T beyond int32")
expect(behave(io=io_of(lat_error=None, lon_command=None)), "behave: no optional outputs", ok=True)
expect(rollout(io=io_of(actors_out=None, log_state=None, log_control=None, log_head=None, log_mode=None, log_target=None)),
       "rollout: no optional outputs", ok=True)

# a clean call afterwards still yields the clean answer
expect(behave(), "behave: clean again", ok=True)
for k in ("control", "mode", "blocker", "distance", "ttc", "target_speed_out", "head_out", "lon_err_out"):
    assert np.array_equal(out[k], clean_b[k], equal_nan=True), k
expect(rollout(), "rollout: clean again", ok=True)
for k in ("state_out", "mode_ticks", "min_gap", "log_mode", "log_state", "done_tick"):
    assert np.array_equal(out[k], clean_r[k], equal_nan=True), k
lib.emp_destroy(h)
print(f"BEHAVIOR-FUZZ-OK {probes} probes {errors} errors")
