"""Child process of tests/test_gpu_control.py: raw ctypes calls of the three controller entry points of ABI 12
(emp_pid_longitudinal, emp_mpc_ff_lateral, emp_vehicle_control) with host pointers and hostile arguments - a NULL context
or parameter block, negative batches, NULL where a pointer is required and where it is optional, an unknown lateral law,
max_path 0, B = 0.  Contract (include/emplanner.h): a call returns EMP_OK or a negative emp_error with a message, never
crashes, and a clean call afterwards still yields the clean answer.  Prints one line per probe and, last,
'CONTROL-FUZZ-OK <probes> probes <errors> errors'."""
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


def expect(rc, what, ok=False, ctx=True):
    """ctx=False: the probe passed no context, so there is no context to hold the message."""
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


B, M = 4, 16
rng = np.random.default_rng(3)
path = np.zeros((B, M, 4))
path[:, :, 0] = np.arange(M) * 2.0
n_path = np.full(B, M, np.int32)
state = np.column_stack([rng.normal(0, 0.3, B), rng.normal(0, 0.3, B), rng.normal(0, 0.05, B), np.zeros(B), np.zeros(B)])
vx = np.full(B, 5.0)
mi = np.zeros(B, np.int32)
speed = np.full(B, 20.0)
target = np.full(B, 20.5)
err_in = np.zeros((B, 60))
n_in = np.zeros(B, np.int32)

pid = L.PidParams()
lib.emp_pid_params_default(C.byref(pid))
assert (pid.K_P, pid.K_I, pid.K_D, pid.dt, pid.error_threshold) == (1.15, 0.0, 0.0, 0.01, 1.0)
mp = L.MpcParams()
lib.emp_mpc_ff_params_default(C.byref(mp))
assert list(mp.q_diag) == [200.0, 1.0, 1.0, 1.0] and list(mp.f_diag) == [10.0] * 4 and mp.r == 1.0
lib.emp_mpc_params_default(C.byref(mp))

# ---- emp_pid_longitudinal
cmd, err_out, n_out = np.zeros(B), np.zeros((B, 60)), np.zeros(B, np.int32)


def pid_call(ctx=h, p=C.byref(pid), b=B, **kw):
    a = dict(speed=speed, target=target, err_in=err_in, n_in=n_in, cmd=cmd, err_out=err_out, n_out=n_out)
    a.update(kw)
    return lib.emp_pid_longitudinal(ctx, p, b, *(ptr(a[k]) for k in ("speed", "target", "err_in", "n_in", "cmd", "err_out",
                                                                      "n_out")), L.EMP_HOST)


expect(pid_call(ctx=None), "pid: NULL ctx", ctx=False)
expect(pid_call(p=None), "pid: NULL params")
expect(pid_call(b=-1), "pid: B = -1")
expect(pid_call(b=-(1 << 30)), "pid: B = -2^30")
for k in ("speed", "target", "err_in", "n_in", "cmd", "err_out", "n_out"):
    expect(pid_call(**{k: None}), f"pid: NULL {k}")
expect(pid_call(b=0), "pid: B = 0", ok=True)
expect(pid_call(), "pid: clean", ok=True)
assert np.array_equal(cmd, np.full(B, 1.15 * 0.5)) and (n_out == 1).all()

# ---- emp_mpc_ff_lateral
steer, u, e, k_r, mo, pp, H, f, it, st = (np.zeros(B), np.zeros((B, 8)), np.zeros((B, 4)), np.zeros(B), np.zeros(B, np.int32),
                                          np.zeros((B, 4)), np.zeros((B, 8, 8)), np.zeros((B, 8)), np.zeros(B, np.int32),
                                          np.zeros(B, np.int32))


def ff_call(ctx=h, p=C.byref(mp), b=B, m=M, **kw):
    a = dict(path=path, n_path=n_path, state=state, vx=vx, mi=mi, steer=steer, u=u, e=e, k_r=k_r, mo=mo, pp=pp, H=H, f=f, it=it,
             st=st)
    a.update(kw)
    return lib.emp_mpc_ff_lateral(ctx, p, b, m, *(ptr(a[k]) for k in ("path", "n_path", "state", "vx", "mi", "steer", "u", "e",
                                                                      "k_r", "mo", "pp", "H", "f", "it", "st")), L.EMP_HOST)


expect(ff_call(ctx=None), "ff: NULL ctx", ctx=False)
expect(ff_call(p=None), "ff: NULL params")
expect(ff_call(b=-1), "ff: B = -1")
expect(ff_call(m=0), "ff: max_path = 0")
expect(ff_call(m=-4), "ff: max_path = -4")
for k in ("path", "n_path", "state", "vx", "mi", "steer", "mo", "st"):
    expect(ff_call(**{k: None}), f"ff: NULL {k}")
expect(ff_call(u=None, e=None, k_r=None, pp=None, H=None, f=None, it=None), "ff: optional outputs NULL", ok=True)
expect(ff_call(b=0), "ff: B = 0", ok=True)
expect(ff_call(), "ff: clean", ok=True)
assert (st == 0).all() and np.array_equal(steer, u[:, 0])

# ---- emp_vehicle_control
control, lat_c, lon_c = np.zeros((B, 3)), np.zeros(B), np.zeros(B)


def vc_call(ctx=h, law=L.EMP_LAT_MPC, lat=C.byref(mp), pp_=C.byref(pid), b=B, m=M, **kw):
    a = dict(path=path, n_path=n_path, state=state, vx=vx, mi=mi, speed=speed, target=target, err_in=err_in, n_in=n_in,
             control=control, lat_c=lat_c, lon_c=lon_c, mo=mo, e=e, k_r=k_r, pp=pp, err_out=err_out, n_out=n_out, st=st)
    a.update(kw)
    names = ("path", "n_path", "state", "vx", "mi", "speed", "target", "err_in", "n_in", "control", "lat_c", "lon_c", "mo", "e",
             "k_r", "pp", "err_out", "n_out", "st")
    return lib.emp_vehicle_control(ctx, law, lat, pp_, b, m, *(ptr(a[k]) for k in names), L.EMP_HOST)


expect(vc_call(ctx=None), "vc: NULL ctx", ctx=False)
expect(vc_call(law=2), "vc: lateral 2")
expect(vc_call(law=-1), "vc: lateral -1")
expect(vc_call(lat=None), "vc: NULL lateral params")
expect(vc_call(pp_=None), "vc: NULL pid params")
expect(vc_call(b=-1), "vc: B = -1")
expect(vc_call(m=0), "vc: max_path = 0")
for k in ("path", "n_path", "state", "vx", "mi", "speed", "target", "err_in", "n_in", "control", "mo", "err_out", "n_out", "st"):
    expect(vc_call(**{k: None}), f"vc: NULL {k}")
for law in (L.EMP_LAT_MPC, L.EMP_LAT_LQR):
    expect(vc_call(law=law, lat_c=None, lon_c=None, e=None, k_r=None, pp=None), f"vc {law}: optional outputs NULL", ok=True)
    expect(vc_call(law=law, b=0), f"vc {law}: B = 0", ok=True)
    expect(vc_call(law=law), f"vc {law}: clean", ok=True)
    assert (st == 0).all() and (n_out == 1).all() and np.array_equal(lon_c, np.full(B, 1.15 * 0.5))
lib.emp_destroy(h)
print(f"CONTROL-FUZZ-OK {probes} probes {errors} errors")
