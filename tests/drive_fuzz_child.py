"""Child process of tests/test_gpu_drive.py: raw ctypes calls of emp_drive_request and emp_drive with host pointers and hostile
arguments - NULL for every required pointer in turn, K = 0 and above EMP_DRIVE_MAX_PERIODS, T = 0, max_act = 0 and 65, max_obs and
max_dyn out of range, reserved != 0 in either struct, EMP_HOST_PINNED, an unknown lateral law.  Each must return EMP_ERR_INVALID
with a message and launch nothing (the context's launch counters stay at 0); then optional pointers NULL and B = 0, which must be
accepted, and a clean call that still yields the clean answer.  Prints one line per probe and, last,
'DRIVE-FUZZ-OK <probes> probes <errors> errors'."""
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
KERNELS = (b"drive_request", b"drive_adopt", b"rollout", b"drive_accel", b"project")


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


B, G, A, MO, MD, M, K, T = 3, 80, 4, 4, 2, 60, 2, 3
dp, qp, sp = L.DpParams(), L.QpParams(), L.SmoothParams()
lib.emp_dp_params_default(C.byref(dp))
lib.emp_qp_params_default(C.byref(qp))
lib.emp_smooth_params_default(C.byref(sp))
drv, mp, pid, vp = L.DriveParams(), L.MpcParams(), L.PidParams(), L.VehicleParams()
lib.emp_drive_params_default(C.byref(drv))
lib.emp_mpc_params_default(C.byref(mp))
lib.emp_pid_params_default(C.byref(pid))
lib.emp_vehicle_params_default(C.byref(vp))
assert (drv.dis_limitation, drv.lateral_band, drv.behind, drv.dynamic_speed, drv.static_gate, drv.pred_ts, drv.advance_s,
        drv.reserved) == (50.0, 5.0, -10.0, 1.0, 30.0, 0.2, 0.0, 0)
lib.emp_drive_params_default(None)                             # a NULL block is ignored
bad_drv = L.DriveParams()
lib.emp_drive_params_default(C.byref(bad_drv))
bad_drv.reserved = 1

gp = np.zeros((B, G, 4))
gp[:, :, 0] = np.arange(G) * 2.0
a = dict(global_path=gp, n_global=np.full(B, G, np.int32),
         state=np.column_stack([np.full(B, 10.0), np.array([0.2, -0.1, 0.0]), np.zeros(B), np.zeros(B), np.zeros(B), np.full(B, 8.0)]),
         accel=np.zeros((B, 2)), actors=np.zeros((B, A, 4)), n_act=np.array([0, 1, 2], np.int32),
         pre_match_index=np.full(B, 5, np.int32), track=np.zeros((B, M + 1, 4)), track_len=np.zeros(B, np.int32),
         held=np.zeros(B, np.int32), target=np.full(B, 30.0))
a["actors"][:, 0] = (35.0, 1.0, 0.0, 0.0)
a["actors"][:, 1] = (30.0, -1.0, 6.0, 0.0)
OUT_SHAPES = dict(state_out=(B, 6), accel_out=(B, 2), actors_out=(B, A, 4), pre_match_index_out=(B,), track_out=(B, M + 1, 4),
                  track_len_out=(B,), held_out=(B,))
LOG_SHAPES = dict(log_state=(K, B, 6), log_plan_status=(K, B), log_roll_status=(K, B), log_held=(K, B), log_counts=(K, B, 2),
                  log_traj=(K, B, M + 1, 4), log_traj_len=(K, B))
INT = {"pre_match_index_out", "track_len_out", "held_out", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj_len"}
for name, shape in {**OUT_SHAPES, **LOG_SHAPES}.items():
    a[name] = np.zeros(shape, np.int32 if name in INT else np.float64)
INS = ("global_path", "n_global", "state", "accel", "actors", "n_act", "pre_match_index", "track", "track_len", "held")


def drive(ctx=h, d=C.byref(drv), law=L.EMP_LAT_MPC, b=B, mo=MO, m=M, ma=A, md=MD, k=K, t=T, where=L.EMP_HOST, reserved=0, target=True,
          v=C.byref(vp), **kw):
    arrays = dict(a)
    arrays.update(kw)
    io = L.DriveIO()
    for name in INS + tuple(OUT_SHAPES) + tuple(LOG_SHAPES):
        setattr(io, name, ptr(arrays[name]))
    io.reserved = reserved
    return lib.emp_drive(ctx, C.byref(dp), C.byref(qp), C.byref(sp), d, law, C.byref(mp), C.byref(pid), v, b, G, mo, m, ma, md, k, t,
                         ptr(a["target"]) if target else None, C.byref(io), where)


rq = dict(static_xy=np.zeros((B, MO, 2)), n_static=np.zeros(B, np.int32), static_dis=np.zeros((B, MO)), dyn=np.zeros((B, MD, 4)),
          n_dyn=np.zeros(B, np.int32), dyn_dis_speed=np.zeros((B, 2)), n_obs=np.zeros(B, np.int32), origin_xy=np.zeros((B, 2)),
          start_xy=np.zeros((B, 2)), pred_fi=np.zeros(B), start_v=np.zeros((B, 2)), start_a=np.zeros((B, 2)),
          req_status=np.zeros(B, np.int32), actors_next=np.zeros((B, A, 4)))
RQ_IN = ("state", "accel", "actors", "n_act")


def request(ctx=h, d=C.byref(drv), b=B, ma=A, mo=MO, md=MD, where=L.EMP_HOST, **kw):
    arrays = dict(a, **rq)
    arrays.update(kw)
    return lib.emp_drive_request(ctx, d, b, ma, mo, md, *(ptr(arrays[k]) for k in RQ_IN + tuple(rq)), where)


assert lib.emp_set_timing(h, 1) == 0                           # launches are counted from here on
# ---- emp_drive_request
expect(request(d=None), "request: NULL params")
expect(request(d=C.byref(bad_drv)), "request: reserved = 1")
expect(request(b=-1), "request: B = -1")
for ma in (0, 65):
    expect(request(ma=ma), f"request: max_act = {ma}")
for mo in (0, 257):
    expect(request(mo=mo), f"request: max_obs = {mo}")
for md in (0, 65):
    expect(request(md=md), f"request: max_dyn = {md}")
expect(request(where=L.EMP_HOST_PINNED), "request: EMP_HOST_PINNED")
for k_ in ("state", "actors", "n_act") + tuple(k for k in rq if k != "actors_next"):
    expect(request(**{k_: None}), f"request: NULL {k_}")
# ---- emp_drive
expect(drive(d=None), "drive: NULL drive params")
expect(drive(v=None), "drive: NULL vehicle params")
expect(drive(d=C.byref(bad_drv)), "drive: emp_drive_params.reserved = 1")
expect(drive(reserved=7), "drive: emp_drive_io.reserved = 7")
expect(drive(where=L.EMP_HOST_PINNED), "drive: EMP_HOST_PINNED")
expect(drive(law=2), "drive: lateral = 2")
for k_ in (0, -1, L.DRIVE_MAX_PERIODS + 1):
    expect(drive(k=k_), f"drive: K = {k_}")
for t_ in (0, L.ROLLOUT_MAX_TICKS + 1):
    expect(drive(t=t_), f"drive: T = {t_}")
for ma in (0, 65):
    expect(drive(ma=ma), f"drive: max_act = {ma}")
expect(drive(mo=254), "drive: max_obs = 254")
expect(drive(md=65), "drive: max_dyn = 65")
expect(drive(m=256), "drive: max_pts = 256")
expect(drive(b=-1), "drive: B = -1")
expect(drive(target=False), "drive: NULL target_speed")
for k_ in tuple(k for k in INS if k != "accel") + tuple(OUT_SHAPES):
    expect(drive(**{k_: None}), f"drive: NULL {k_}")
assert launches() == 0
# ---- accepted
expect(request(), "request: clean", ok=True)
assert list(rq["n_static"]) == [0, 1, 1] and list(rq["n_dyn"]) == [0, 0, 1] and list(rq["n_obs"]) == [0, 1, 1]
expect(request(accel=None, actors_next=None), "request: optional pointers NULL", ok=True)
expect(request(b=0), "request: B = 0", ok=True)
expect(drive(), "drive: clean", ok=True)
clean = {k: a[k].copy() for k in tuple(OUT_SHAPES) + tuple(LOG_SHAPES)}
assert ((a["log_plan_status"] & ~1) == 0).all() and (a["log_held"] == 0).all() and (a["track_len_out"] > 10).all()
assert np.array_equal(a["log_state"][0], a["state"]) and np.isfinite(a["state_out"]).all()
assert lib.emp_kernel_launches(h, b"drive_request") == K + 2 and lib.emp_kernel_launches(h, b"drive_adopt") == K
assert lib.emp_kernel_launches(h, b"rollout") == K and lib.emp_kernel_launches(h, b"drive_accel") == K
expect(drive(accel=None, **{k: None for k in LOG_SHAPES}), "drive: optional pointers NULL", ok=True)
expect(drive(b=0), "drive: B = 0", ok=True)
for k_ in clean:
    a[k_][...] = 0
expect(drive(), "drive: clean again", ok=True)
for k_ in clean:
    assert np.array_equal(a[k_], clean[k_]), k_
lib.emp_destroy(h)
print(f"DRIVE-FUZZ-OK {probes} probes {errors} errors")
