"""Child process of tests/test_gpu_rollout.py: raw ctypes calls of emp_vehicle_step and emp_rollout with host pointers and hostile
arguments - a NULL context or parameter block, T = 0 and T above EMP_ROLLOUT_MAX_TICKS, log_every = 0, reserved != 0, an unknown
lateral law, max_path 0, a negative batch, NULL for every required pointer in turn; then NULL for every optional pointer and
B = 0, which must be accepted.  Contract (include/emplanner.h): a call returns EMP_OK or a negative emp_error with a message,
never crashes, and a clean call afterwards still yields the clean answer.  Prints one line per probe and, last,
'ROLLOUT-FUZZ-OK <probes> probes <errors> errors'."""
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


B, M, T = 4, 32, 5
rng = np.random.default_rng(11)
path = np.zeros((B, M, 4))
path[:, :, 0] = np.arange(M) * 2.5
n_path = np.full(B, M, np.int32)
state = np.column_stack([rng.normal(3, 0.3, B), rng.normal(0, 0.3, B), rng.normal(0, 0.02, B), np.zeros(B), np.zeros(B),
                         np.full(B, 8.0)])
pid = L.PidParams()
lib.emp_pid_params_default(C.byref(pid))
mp = L.MpcParams()
lib.emp_mpc_params_default(C.byref(mp))
vp = L.VehicleParams()
lib.emp_vehicle_params_default(C.byref(vp))
assert (vp.a, vp.b, vp.Cf, vp.Cr, vp.m, vp.Iz) == (mp.a, mp.b, mp.Cf, mp.Cr, mp.m, mp.Iz)
assert (vp.dt, vp.steer_gain, vp.throttle_accel, vp.brake_decel, vp.drag, vp.reserved) == (0.01, 1.0, 3.0, 6.0, 0.0, 0)
bad_vp = L.VehicleParams()
lib.emp_vehicle_params_default(C.byref(bad_vp))
bad_vp.reserved = 1
lib.emp_vehicle_params_default(None)                           # a NULL block is ignored

# ---- emp_vehicle_step
control = np.column_stack([np.full(B, 0.5), rng.uniform(-0.2, 0.2, B), np.zeros(B)])
vs = dict(state=state.copy(), control=control, out=np.zeros((B, 6)), cs=np.zeros((B, 5)), vx=np.zeros(B), kmh=np.zeros(B))


def vs_call(ctx=h, p=C.byref(vp), b=B, **kw):
    a = dict(vs)
    a.update(kw)
    return lib.emp_vehicle_step(ctx, p, b, *(ptr(a[k]) for k in ("state", "control", "out", "cs", "vx", "kmh")), L.EMP_HOST)


expect(vs_call(), "vehicle_step: clean", ok=True)
clean_step = vs["out"].copy()
assert (clean_step[:, 5] == 8.0 + 0.01 * 1.5).all()
expect(vs_call(ctx=None), "vehicle_step: NULL ctx", ctx=False)
expect(vs_call(p=None), "vehicle_step: NULL params")
expect(vs_call(p=C.byref(bad_vp)), "vehicle_step: reserved = 1")
expect(vs_call(b=-1), "vehicle_step: B = -1")
for k in ("state", "control", "out"):
    expect(vs_call(**{k: None}), f"vehicle_step: NULL {k}")
for k in ("cs", "vx", "kmh"):
    expect(vs_call(**{k: None}), f"vehicle_step: optional {k} NULL", ok=True)
expect(vs_call(b=0), "vehicle_step: B = 0", ok=True)
vs["out"][:] = 0
expect(vs_call(), "vehicle_step: clean again", ok=True)
assert np.array_equal(vs["out"], clean_step)

# ---- emp_rollout
n_log = T
ro = dict(path=path, n_path=n_path, state=state.copy(), mi=np.zeros(B, np.int32), target=np.full(B, 29.0), err=np.zeros((B, 60)),
          n_err=np.zeros(B, np.int32), so=np.zeros((B, 6)), mo=np.zeros(B, np.int32), eo=np.zeros((B, 60)), no=np.zeros(B, np.int32),
          st=np.zeros(B, np.int32), ft=np.zeros(B, np.int32), ls=np.zeros((n_log, B, 6)), lc=np.zeros((n_log, B, 3)),
          le=np.zeros((n_log, B, 4)), li=np.zeros((n_log, B), np.int32))
INS = ("path", "n_path", "state", "mi", "target", "err", "n_err")
OUTS = ("so", "mo", "eo", "no", "st", "ft")
LOGS = ("ls", "lc", "le", "li")


def ro_call(ctx=h, law=L.EMP_LAT_MPC, lat=C.byref(mp), pp=C.byref(pid), v=C.byref(vp), b=B, m=M, t=T, every=1, **kw):
    a = dict(ro)
    a.update(kw)
    return lib.emp_rollout(ctx, law, lat, pp, v, b, m, *(ptr(a[k]) for k in INS), t, every, *(ptr(a[k]) for k in OUTS + LOGS),
                           L.EMP_HOST)


clean = {}
for law in (L.EMP_LAT_MPC, L.EMP_LAT_LQR):
    expect(ro_call(law=law), f"rollout: clean (law {law})", ok=True)
    assert (ro["st"] == 0).all() and (ro["ft"] == -1).all() and np.isfinite(ro["so"]).all()
    assert np.array_equal(ro["ls"][0], state)
    clean[law] = {k: ro[k].copy() for k in OUTS + LOGS}
expect(ro_call(ctx=None), "rollout: NULL ctx", ctx=False)
expect(ro_call(law=2), "rollout: lateral = 2")
expect(ro_call(law=-1), "rollout: lateral = -1")
expect(ro_call(lat=None), "rollout: NULL lateral params")
expect(ro_call(pp=None), "rollout: NULL PID params")
expect(ro_call(v=None), "rollout: NULL vehicle params")
expect(ro_call(v=C.byref(bad_vp)), "rollout: reserved = 1")
expect(ro_call(t=0), "rollout: T = 0")
expect(ro_call(t=-3), "rollout: T = -3")
expect(ro_call(t=L.ROLLOUT_MAX_TICKS + 1), "rollout: T above the limit")
expect(ro_call(t=2 ** 31 - 1), "rollout: T = INT32_MAX")
expect(ro_call(every=0), "rollout: log_every = 0")
expect(ro_call(every=-1), "rollout: log_every = -1")
expect(ro_call(b=-1), "rollout: B = -1")
expect(ro_call(m=0), "rollout: max_path = 0")
for k in INS + OUTS:
    expect(ro_call(**{k: None}), f"rollout: NULL {k}")
for k in LOGS:
    expect(ro_call(**{k: None}), f"rollout: optional {k} NULL", ok=True)
expect(ro_call(ls=None, lc=None, le=None, li=None, every=T + 1), "rollout: no logs at all", ok=True)
expect(ro_call(b=0), "rollout: B = 0", ok=True)
for law in (L.EMP_LAT_MPC, L.EMP_LAT_LQR):
    for k in OUTS + LOGS:
        ro[k][...] = 0
    expect(ro_call(law=law), f"rollout: clean again (law {law})", ok=True)
    for k in OUTS + LOGS:
        assert np.array_equal(ro[k], clean[law][k]), k
lib.emp_destroy(h)
print(f"ROLLOUT-FUZZ-OK {probes} probes {errors} errors")
