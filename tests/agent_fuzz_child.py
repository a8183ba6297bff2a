"""Child process of tests/test_gpu_agents.py: raw ctypes calls of emp_agent_observe, emp_agent_control and emp_agent_rollout with
host pointers and hostile arguments - a NULL context or parameter block, T = 0 and T above EMP_ROLLOUT_MAX_TICKS, log_every = 0,
reserved != 0 in each of the three blocks, max_path 0, a negative batch, EMP_HOST_PINNED, NULL for every required pointer in turn;
then NULL for every optional pointer and A = 0, which must be accepted.  Contract (include/emplanner.h): a call returns EMP_OK or a
negative emp_error with a message, never crashes, and a clean call afterwards still yields the clean answer.  Prints one line per
probe and, last, 'AGENT-FUZZ-OK <probes> probes <errors> errors'."""
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


A, M, T = 5, 12, 6
path = np.zeros((A, M, 4))
path[:, :, 0] = 4.0 + np.arange(M) * 2.0
path[:, :, 1] = np.arange(A)[:, None] * 0.3
n_path = np.array([M, M, 0, 1, M + 9], np.int32)
state = np.column_stack([np.zeros(A), np.zeros(A), np.linspace(-0.2, 0.2, A), np.zeros(A), np.zeros(A), np.full(A, 4.0)])
target = np.full(A, 20.0)
prm = L.AgentParams()
lib.emp_agent_params_default(C.byref(prm))
assert (prm.lat_K_P, prm.lat_K_I, prm.lat_K_D, prm.lon_K_P, prm.lon_K_I, prm.lon_K_D) == (1.95, 0.05, 0.2, 1.0, 0.05, 0.0)
assert (prm.dt, prm.max_throttle, prm.max_brake, prm.max_steer, prm.base_min_distance, prm.reserved) == (0.05, 0.75, 0.3, 0.8, 3.0, 0)
lib.emp_agent_params_default(None)                             # a NULL block is ignored
bad_prm = L.AgentParams()
lib.emp_agent_params_default(C.byref(bad_prm))
bad_prm.reserved = 1
vp = L.VehicleParams()
lib.emp_vehicle_params_default(C.byref(vp))
vp.Cf, vp.Cr, vp.m, vp.dt = -148970.0, -82204.0, 1412.0, 0.05
bad_vp = L.VehicleParams.from_buffer_copy(vp)
bad_vp.reserved = 1

# ---- emp_agent_observe
ob = dict(state=state, fw=np.zeros((A, 2)), kmh=np.zeros(A), act=np.zeros((A, 4)))


def ob_call(ctx=h, a=A, where=L.EMP_HOST, **kw):
    d = dict(ob)
    d.update(kw)
    return lib.emp_agent_observe(ctx, a, *(ptr(d[k]) for k in ("state", "fw", "kmh", "act")), where)


expect(ob_call(), "observe: clean", ok=True)
clean_ob = {k: ob[k].copy() for k in ("fw", "kmh", "act")}
assert np.allclose(ob["kmh"], 14.4) and np.array_equal(ob["act"][:, :2], state[:, :2])
expect(ob_call(ctx=None), "observe: NULL ctx", ctx=False)
expect(ob_call(a=-1), "observe: A = -1")
expect(ob_call(state=None), "observe: NULL state")
expect(ob_call(fw=None, kmh=None, act=None), "observe: no output at all")
expect(ob_call(where=L.EMP_HOST_PINNED), "observe: EMP_HOST_PINNED")
expect(ob_call(where=7), "observe: where = 7")
for k in ("fw", "kmh", "act"):
    expect(ob_call(**{k: None}), f"observe: optional {k} NULL", ok=True)
expect(ob_call(fw=None, kmh=None), "observe: actors only", ok=True)
expect(ob_call(a=0), "observe: A = 0", ok=True)

# ---- emp_agent_control
st_in = dict(head=np.zeros(A, np.int32), past=np.zeros(A), lon=np.zeros((A, 10)), n_lon=np.zeros(A, np.int32), lat=np.zeros((A, 10)),
             n_lat=np.zeros(A, np.int32))
co = dict(path=path, n_path=n_path, state=state, fw=clean_ob["fw"], kmh=clean_ob["kmh"], target=target, **st_in,
          ctl=np.zeros((A, 3)), status=np.zeros(A, np.int32), head_o=np.zeros(A, np.int32), past_o=np.zeros(A), lon_o=np.zeros((A, 10)),
          n_lon_o=np.zeros(A, np.int32), lat_o=np.zeros((A, 10)), n_lat_o=np.zeros(A, np.int32), le=np.zeros(A), lc=np.zeros(A))
CO_INS = ("path", "n_path", "state", "fw", "kmh", "target", "head", "past", "lon", "n_lon", "lat", "n_lat")
CO_OUTS = ("ctl", "status", "head_o", "past_o", "lon_o", "n_lon_o", "lat_o", "n_lat_o")
CO_OPT = ("le", "lc")


def co_call(ctx=h, p=C.byref(prm), a=A, m=M, where=L.EMP_HOST, **kw):
    d = dict(co)
    d.update(kw)
    return lib.emp_agent_control(ctx, p, a, m, *(ptr(d[k]) for k in CO_INS + CO_OUTS + CO_OPT), where)


expect(co_call(), "control: clean", ok=True)
assert list(co["status"]) == [0, 0, 1, 0, 0] and (co["ctl"][2] == (0.0, 0.0, 1.0)).all() and list(co["n_lon_o"]) == [1, 1, 0, 1, 1]
clean_co = {k: co[k].copy() for k in CO_OUTS + CO_OPT}
expect(co_call(ctx=None), "control: NULL ctx", ctx=False)
expect(co_call(p=None), "control: NULL params")
expect(co_call(p=C.byref(bad_prm)), "control: reserved = 1")
expect(co_call(a=-1), "control: A = -1")
expect(co_call(m=0), "control: max_path = 0")
expect(co_call(where=L.EMP_HOST_PINNED), "control: EMP_HOST_PINNED")
for k in CO_INS + CO_OUTS:
    expect(co_call(**{k: None}), f"control: NULL {k}")
for k in CO_OPT:
    expect(co_call(**{k: None}), f"control: optional {k} NULL", ok=True)
expect(co_call(a=0), "control: A = 0", ok=True)
for k in CO_OUTS + CO_OPT:
    co[k][...] = 0
expect(co_call(), "control: clean again", ok=True)
for k in CO_OUTS + CO_OPT:
    assert np.array_equal(co[k], clean_co[k]), k

# ---- emp_agent_rollout
ro = dict(path=path, n_path=n_path, state=state, target_speed=target, head=st_in["head"], past_steer=st_in["past"], lon_err=st_in["lon"],
          n_lon=st_in["n_lon"], lat_err=st_in["lat"], n_lat=st_in["n_lat"], state_out=np.zeros((A, 6)), head_out=np.zeros(A, np.int32),
          past_steer_out=np.zeros(A), lon_err_out=np.zeros((A, 10)), n_lon_out=np.zeros(A, np.int32), lat_err_out=np.zeros((A, 10)),
          n_lat_out=np.zeros(A, np.int32), status=np.zeros(A, np.int32), done_tick=np.zeros(A, np.int32), actors_out=np.zeros((A, 4)),
          log_state=np.zeros((T, A, 6)), log_control=np.zeros((T, A, 3)), log_head=np.zeros((T, A), np.int32))
RO_REQ = ("path", "n_path", "state", "target_speed", "head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat", "state_out", "head_out",
          "past_steer_out", "lon_err_out", "n_lon_out", "lat_err_out", "n_lat_out", "status", "done_tick")
RO_OPT = ("actors_out", "log_state", "log_control", "log_head")
RO_OUTS = RO_REQ[10:] + RO_OPT


def ro_call(ctx=h, p=C.byref(prm), v=C.byref(vp), a=A, m=M, t=T, every=1, where=L.EMP_HOST, io=True, reserved=0, **kw):
    d = dict(ro)
    d.update(kw)
    s = L.AgentRolloutIO()
    for k in RO_REQ + RO_OPT:
        setattr(s, k, ptr(d[k]))
    s.reserved = reserved
    return lib.emp_agent_rollout(ctx, p, v, a, m, t, every, C.byref(s) if io else None, where)


expect(ro_call(), "rollout: clean", ok=True)
assert list(ro["done_tick"]) == [-1, -1, 0, -1, -1] and np.array_equal(ro["log_state"][0], state) and np.isfinite(ro["state_out"]).all()
assert np.array_equal(ro["log_control"][0], clean_co["ctl"]) and np.array_equal(ro["log_head"][0], clean_co["head_o"])
clean_ro = {k: ro[k].copy() for k in RO_OUTS}
expect(ro_call(ctx=None), "rollout: NULL ctx", ctx=False)
expect(ro_call(p=None), "rollout: NULL agent params")
expect(ro_call(v=None), "rollout: NULL vehicle params")
expect(ro_call(io=False), "rollout: NULL io")
expect(ro_call(p=C.byref(bad_prm)), "rollout: agent params reserved = 1")
expect(ro_call(v=C.byref(bad_vp)), "rollout: vehicle params reserved = 1")
expect(ro_call(reserved=1), "rollout: io reserved = 1")
expect(ro_call(t=0), "rollout: T = 0")
expect(ro_call(t=-3), "rollout: T = -3")
expect(ro_call(t=L.ROLLOUT_MAX_TICKS + 1), "rollout: T above the limit")
expect(ro_call(t=2 ** 31 - 1), "rollout: T = INT32_MAX")
expect(ro_call(every=0), "rollout: log_every = 0")
expect(ro_call(every=-1), "rollout: log_every = -1")
expect(ro_call(a=-1), "rollout: A = -1")
expect(ro_call(m=0), "rollout: max_path = 0")
expect(ro_call(where=L.EMP_HOST_PINNED), "rollout: EMP_HOST_PINNED")
for k in RO_REQ:
    expect(ro_call(**{k: None}), f"rollout: NULL {k}")
for k in RO_OPT:
    expect(ro_call(**{k: None}), f"rollout: optional {k} NULL", ok=True)
expect(ro_call(actors_out=None, log_state=None, log_control=None, log_head=None, every=T + 1), "rollout: no optional output at all", ok=True)
expect(ro_call(a=0), "rollout: A = 0", ok=True)
for k in RO_OUTS:
    ro[k][...] = 0
expect(ro_call(), "rollout: clean again", ok=True)
for k in RO_OUTS:
    assert np.array_equal(ro[k], clean_ro[k]), k
lib.emp_destroy(h)
print(f"AGENT-FUZZ-OK {probes} probes {errors} errors")
