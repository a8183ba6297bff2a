"""Child process of tests/test_gpu_drive_timed.py: raw ctypes calls of emp_drive_request_timed and emp_drive_timed with host
pointers and hostile arguments - NULL for every required pointer and struct in turn, tick / tick0 < 0, tick0 + K * T beyond
INT32_MAX, K and T out of range, the sizes out of range, reserved != 0 in each of the three structs, EMP_HOST_PINNED, an unknown
lateral law, speed weights the speed planner refuses.  Each must return EMP_ERR_INVALID with a message and launch nothing (the
context's launch counters stay at 0); then optional pointers NULL and B = 0, which must be accepted, and a clean call that still
yields the clean answer.  Refusals only: nothing here is meant to fault.  Prints one line per probe and, last,
'DRIVE-TIMED-FUZZ-OK <probes> probes <errors> errors'."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emplanner_carla_amd import _lib as L  # noqa: E402

lib = L.load()
h = C.c_void_p()
assert lib.emp_create(0, C.byref(h)) == 0
ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
probes = errors = 0
KERNELS = (b"drive_request_timed", b"drive_adopt_timed", b"rollout_timed", b"drive_accel", b"project", b"speed_front", b"drive_request")
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


B, G, A, MO, MD, M, K, T, N = 3, 80, 4, 4, 2, 60, 2, 3, L.TIMED_POINTS
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
assert (tp.plan_lead, tp.reserved) == (0.1, 0)
lib.emp_drive_timed_params_default(None)                       # a NULL block is ignored
bad_drv, bad_tp, bad_sdp, bad_sqp = L.DriveParams(), L.DriveTimedParams(), L.SpeedDpParams(), L.SpeedQpParams()
nan_tp = L.DriveTimedParams()
lib.emp_drive_params_default(C.byref(bad_drv))
bad_drv.reserved = 1
lib.emp_drive_timed_params_default(C.byref(bad_tp))
bad_tp.reserved = 1
lib.emp_drive_timed_params_default(C.byref(nan_tp))
nan_tp.plan_lead = float("nan")
lib.emp_speed_dp_params_default(C.byref(bad_sdp))
bad_sdp.w_cost_obs = -1.0
lib.emp_speed_qp_params_default(C.byref(bad_sqp))
bad_sqp.w_cost_v_ref = 0.0

gp = np.zeros((B, G, 4))
gp[:, :, 0] = np.arange(G) * 2.0
a = dict(global_path=gp, n_global=np.full(B, G, np.int32),
         state=np.column_stack([np.full(B, 10.0), np.array([0.2, -0.1, 0.0]), np.zeros(B), np.zeros(B), np.zeros(B), np.full(B, 8.0)]),
         accel=np.zeros((B, 2)), actors=np.zeros((B, A, 4)), n_act=np.array([0, 1, 2], np.int32),
         pre_match_index=np.full(B, 5, np.int32), track=np.zeros((B, M + 1, 4)), track_len=np.zeros(B, np.int32),
         held=np.zeros(B, np.int32), t0=np.array([0.0, 10.0, 20.5]), profile=np.full((B, 7, N), np.nan), cursor=np.zeros(B, np.int32),
         speed_held=np.zeros(B, np.int32), target=np.full(B, 30.0))
a["actors"][:, 0] = (35.0, 1.0, 0.0, 0.0)
a["actors"][:, 1] = (30.0, -1.0, 6.0, 0.0)
OUT_SHAPES = dict(state_out=(B, 6), accel_out=(B, 2), actors_out=(B, A, 4), pre_match_index_out=(B,), track_out=(B, M + 1, 4),
                  track_len_out=(B,), held_out=(B,), profile_out=(B, 7, N), cursor_out=(B,), speed_held_out=(B,))
LOG_SHAPES = dict(log_state=(K, B, 6), log_plan_status=(K, B), log_roll_status=(K, B), log_held=(K, B), log_counts=(K, B, 2),
                  log_traj=(K, B, M + 1, 4), log_traj_len=(K, B), log_speed_status=(K, B), log_speed_held=(K, B), log_tgt_status=(K, B),
                  log_cursor=(K, B), log_profile=(K, B, 7, N))
INT = {"pre_match_index_out", "track_len_out", "held_out", "cursor_out", "speed_held_out", "log_plan_status", "log_roll_status", "log_held",
       "log_counts", "log_traj_len", "log_speed_status", "log_speed_held", "log_tgt_status", "log_cursor"}
for name, shape in {**OUT_SHAPES, **LOG_SHAPES}.items():
    a[name] = np.zeros(shape, np.int32 if name in INT else np.float64)
INS = ("global_path", "n_global", "state", "accel", "actors", "n_act", "pre_match_index", "track", "track_len", "held", "t0", "profile",
       "cursor", "speed_held")


def drive(ctx=h, d=C.byref(drv), t_=C.byref(tp), sd=C.byref(sdp), sq=C.byref(sqp), law=L.EMP_LAT_MPC, b=B, mo=MO, m=M, ma=A, md=MD, k=K, t=T,
          tick0=0, where=L.EMP_HOST, reserved=0, target=True, v=C.byref(vp), **kw):
    arrays = dict(a)
    arrays.update(kw)
    io = L.DriveTimedIO()
    for name in INS + tuple(OUT_SHAPES) + tuple(LOG_SHAPES):
        setattr(io, name, ptr(arrays[name]))
    io.reserved = reserved
    return lib.emp_drive_timed(ctx, C.byref(dp), C.byref(qp), C.byref(sp), sd, sq, d, t_, law, C.byref(mp), C.byref(pid), v, b, G, mo, m, ma,
                               md, k, t, tick0, ptr(a["target"]) if target else None, C.byref(io), where)


rq = dict(static_xy=np.zeros((B, MO, 2)), n_static=np.zeros(B, np.int32), static_dis=np.zeros((B, MO)), dyn=np.zeros((B, MD, 4)),
          n_dyn=np.zeros(B, np.int32), dyn_dis_speed=np.zeros((B, 2)), n_obs=np.zeros(B, np.int32), origin_xy=np.zeros((B, 2)),
          start_xy=np.zeros((B, 2)), pred_fi=np.zeros(B), start_v=np.zeros((B, 2)), start_a=np.zeros((B, 2)),
          req_status=np.zeros(B, np.int32), actors_next=np.zeros((B, A, 4)), dyn_obs=np.zeros((B, MD, 4)), start_heading=np.zeros(B),
          plan_start_time=np.zeros(B))
RQ_IN = ("state", "accel", "actors", "n_act", "t0")


def request(ctx=h, d=C.byref(drv), b=B, ma=A, mo=MO, md=MD, tick=4, dt=0.01, lead=0.1, where=L.EMP_HOST, **kw):
    arrays = dict(a, **rq)
    arrays.update(kw)
    return lib.emp_drive_request_timed(ctx, d, b, ma, mo, md, *(ptr(arrays[k]) for k in RQ_IN), tick, dt, lead,
                                       *(ptr(arrays[k]) for k in rq), where)


assert lib.emp_set_timing(h, 1) == 0                           # launches are counted from here on
# ---- emp_drive_request_timed
expect(request(d=None), "request_timed: NULL params")
expect(request(d=C.byref(bad_drv)), "request_timed: reserved = 1")
expect(request(b=-1), "request_timed: B = -1")
expect(request(tick=-1), "request_timed: tick = -1")
for dt_ in (0.0, -0.01, float("nan"), float("inf")):
    expect(request(dt=dt_), f"request_timed: dt = {dt_}")
for lead_ in (float("nan"), float("-inf")):
    expect(request(lead=lead_), f"request_timed: plan_lead = {lead_}")
for ma in (0, 65):
    expect(request(ma=ma), f"request_timed: max_act = {ma}")
for mo in (0, 257):
    expect(request(mo=mo), f"request_timed: max_obs = {mo}")
for md in (0, 65):
    expect(request(md=md), f"request_timed: max_dyn = {md}")
expect(request(where=L.EMP_HOST_PINNED), "request_timed: EMP_HOST_PINNED")
for k_ in ("state", "actors", "n_act", "t0") + tuple(k for k in rq if k != "actors_next"):
    expect(request(**{k_: None}), f"request_timed: NULL {k_}")
# ---- emp_drive_timed
expect(drive(d=None), "drive_timed: NULL drive params")
expect(drive(t_=None), "drive_timed: NULL timed params")
expect(drive(sd=None), "drive_timed: NULL speed DP params")
expect(drive(sq=None), "drive_timed: NULL speed QP params")
expect(drive(v=None), "drive_timed: NULL vehicle params")
expect(drive(d=C.byref(bad_drv)), "drive_timed: emp_drive_params.reserved = 1")
expect(drive(t_=C.byref(bad_tp)), "drive_timed: emp_drive_timed_params.reserved = 1")
expect(drive(t_=C.byref(nan_tp)), "drive_timed: plan_lead = nan")
expect(drive(reserved=7), "drive_timed: emp_drive_timed_io.reserved = 7")
expect(drive(sd=C.byref(bad_sdp)), "drive_timed: w_cost_obs = -1")
expect(drive(sq=C.byref(bad_sqp)), "drive_timed: w_cost_v_ref = 0")
expect(drive(where=L.EMP_HOST_PINNED), "drive_timed: EMP_HOST_PINNED")
expect(drive(law=2), "drive_timed: lateral = 2")
expect(drive(tick0=-1), "drive_timed: tick0 = -1")
expect(drive(tick0=INT32_MAX - K * T + 1), "drive_timed: tick0 + K * T = INT32_MAX + 1")
expect(drive(tick0=INT32_MAX), "drive_timed: tick0 = INT32_MAX")
for k_ in (0, -1, L.DRIVE_MAX_PERIODS + 1):
    expect(drive(k=k_), f"drive_timed: K = {k_}")
for t_n in (0, L.ROLLOUT_MAX_TICKS + 1):
    expect(drive(t=t_n), f"drive_timed: T = {t_n}")
for ma in (0, 65):
    expect(drive(ma=ma), f"drive_timed: max_act = {ma}")
expect(drive(mo=254), "drive_timed: max_obs = 254")
for md in (0, 65):
    expect(drive(md=md), f"drive_timed: max_dyn = {md}")
expect(drive(m=256), "drive_timed: max_pts = 256")
expect(drive(b=-1), "drive_timed: B = -1")
expect(drive(target=False), "drive_timed: NULL target_speed")
for k_ in tuple(k for k in INS if k != "accel") + tuple(OUT_SHAPES):
    expect(drive(**{k_: None}), f"drive_timed: NULL {k_}")
assert launches() == 0
# ---- accepted
expect(request(), "request_timed: clean", ok=True)
assert list(rq["n_static"]) == [0, 1, 1] and list(rq["n_dyn"]) == [0, 0, 1]
assert np.array_equal(rq["plan_start_time"], (a["t0"] + 4.0 * 0.01) + 0.1) and np.array_equal(rq["dyn_obs"][2, 0], a["actors"][2, 1])
expect(request(accel=None, actors_next=None), "request_timed: optional pointers NULL", ok=True)
expect(request(b=0), "request_timed: B = 0", ok=True)
expect(drive(tick0=INT32_MAX - K * T), "drive_timed: the last clock that fits", ok=True)
expect(drive(), "drive_timed: clean", ok=True)
clean = {k: a[k].copy() for k in tuple(OUT_SHAPES) + tuple(LOG_SHAPES)}
assert ((a["log_plan_status"] & ~1) == 0).all() and (a["log_held"] == 0).all() and (a["track_len_out"] > 10).all()
assert np.array_equal(a["log_state"][0], a["state"]) and np.isfinite(a["state_out"]).all()
assert lib.emp_kernel_launches(h, b"drive_request_timed") == 2 * K + 2 and lib.emp_kernel_launches(h, b"drive_adopt_timed") == 2 * K
assert lib.emp_kernel_launches(h, b"rollout_timed") == 2 * K and lib.emp_kernel_launches(h, b"drive_accel") == 2 * K
assert lib.emp_kernel_launches(h, b"drive_request") == 0 and lib.emp_kernel_launches(h, b"speed_front") == 2 * K
expect(drive(accel=None, **{k: None for k in LOG_SHAPES}), "drive_timed: optional pointers NULL", ok=True)
expect(drive(b=0), "drive_timed: B = 0", ok=True)
for k_ in clean:
    a[k_][...] = 0
expect(drive(), "drive_timed: clean again", ok=True)
for k_ in clean:
    assert np.array_equal(a[k_], clean[k_], equal_nan=True), k_
lib.emp_destroy(h)
print(f"DRIVE-TIMED-FUZZ-OK {probes} probes {errors} errors")
