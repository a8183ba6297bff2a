"""CPU suite of the timed fleet loop (emp_drive_request_timed, emp_drive_timed): the header declares the calls, the two structs and
the clock rule, the library exports them and the ABI is still 13; the ctypes layouts equal the C structs (a g++ sizeof / offsetof
probe); the clock rule's split identity on integers and doubles, in Python and in the host-compiled plan_drive_clock, with its
refusals; tests/drive_timed_port.py - the request's timed extras and the adopt rule in Python floats - on the recorded request
fixture and on hand-made adoptions; and the GPU suite's tracking scenario and its speed-refused vehicle through the CPU oracle
alone, period by period."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emplanner.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "drive", "drive_request.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import drive_port as port  # noqa: E402
import drive_timed_port as tport  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is needed to compile the host programs")

BASE_IN = ["global_path", "n_global", "state", "accel", "actors", "n_act", "pre_match_index", "track", "track_len", "held"]
BASE_OUT = ["state_out", "accel_out", "actors_out", "pre_match_index_out", "track_out", "track_len_out", "held_out"]
BASE_LOG = ["log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len"]
TIMED_IO_FIELDS = (BASE_IN + ["t0", "profile", "cursor", "speed_held"] + BASE_OUT + ["profile_out", "cursor_out", "speed_held_out"]
                   + BASE_LOG + ["log_speed_status", "log_speed_held", "log_tgt_status", "log_cursor", "log_profile", "reserved"])
NEW_SYMBOLS = ("emp_drive_timed_params_default", "emp_drive_request_timed", "emp_drive_timed")


def test_header_declares_and_the_library_exports_the_timed_loop():
    text = open(HEADER).read()
    assert re.search(r"#define EMP_ABI_VERSION 13\b", text)                      # additions do not bump the version
    for struct in ("emp_drive_timed_params", "emp_drive_timed_io"):
        assert f"typedef struct {struct}" in text and f"}} {struct};" in text
    assert re.search(r"void emp_drive_timed_params_default\(", text)
    assert re.search(r"int emp_drive_request_timed\(", text) and re.search(r"int emp_drive_timed\(", text)
    # the clock rule and the contract are stated, the latter in capitals like the others
    assert "tick_k = tick0 + k * T" in text and "(t0 + (double)tick_k * dt) + plan_lead" in text
    assert "EVERY OUTPUT AND LOG EQUALS, BIT FOR BIT" in text and "EMP_TGT_NO_PROFILE" in text and "22 456 B" in text
    assert "emp_drive_timed below is the loop with the speed planner in it" in text          # emp_drive's comment points here
    from emplanner_carla_amd import _lib, build
    assert _lib.ABI_VERSION == 13
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["emp_drive_request_timed"][1]) == 32 and len(_lib.PROTOTYPES["emp_drive_timed"][1]) == 24
    lib = C.CDLL(build.build(verbose=False))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is declared but not exported"


@needs_gxx
def test_ctypes_layouts_match_the_c_structs(tmp_path):
    from emplanner_carla_amd import _lib
    pairs = (("emp_drive_timed_params", _lib.DriveTimedParams, ["plan_lead", "reserved"]),
             ("emp_drive_timed_io", _lib.DriveTimedIO, TIMED_IO_FIELDS))
    body = ""
    for cname, cls, fields in pairs:
        assert [n for n, _ in cls._fields_] == fields
        body += f'    std::printf("{cname}.sizeof %zu\\n", sizeof({cname}));\n'
        body += "".join(f'    std::printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));\n' for f in fields)
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "emplanner.h"\nint main() {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
               if line)
    for cname, cls, fields in pairs:
        assert int(got[f"{cname}.sizeof"]) == C.sizeof(cls)
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_python_surface_and_defaults():
    from emplanner_carla_amd import api
    tp = api.drive_timed_params()
    assert (tp.plan_lead, tp.reserved) == (0.1, 0) and tport.PLAN_LEAD == 0.1
    for name in ("drive_request_timed", "drive_timed"):
        assert callable(getattr(api.Planner, name))
    base_r, base_q = list(api.DriveResult.__dataclass_fields__), list(api.DriveRequest.__dataclass_fields__)
    assert list(api.TimedDriveResult.__dataclass_fields__) == base_r + [
        "profile", "cursor", "speed_held", "log_speed_status", "log_speed_held", "log_tgt_status", "log_cursor", "log_profile"]
    assert list(api.TimedDriveRequest.__dataclass_fields__) == base_q + ["dyn_obs", "start_heading", "plan_start_time"]


# ---------------------------------------------------------------------------------------------------------------------
# the clock
# ---------------------------------------------------------------------------------------------------------------------
CLOCKS = [(0, 3, 5), (0, 1, 1), (7, 4, 20), (123456, 5, 65536), (2 ** 31 - 1 - 12, 3, 4), (2 ** 31 - 2, 1, 1)]
REFUSED = [(-1, 3, 5), (2 ** 31 - 1, 1, 1), (2 ** 31 - 1 - 11, 3, 4), (0, 4096, 2 ** 20), (0, 0, 5), (0, 3, 0), (-2 ** 31, 1, 1)]


def test_the_clock_splits_on_integers_and_doubles():
    """Nothing accumulates: period k of a K-period run and period k - K1 of the run that resumes it at tick0 + K1 * T have the
    same tick, hence the same doubles t0 + (double)tick * dt and (that) + plan_lead.  The accumulating form the rule avoids,
    clock += T * dt, does NOT split: shown on the same numbers."""
    dt, t0 = 0.01, 1234.5678
    for tick0, K, T in CLOCKS:
        assert tport.clock_refusal(tick0, K, T) is None
        whole = [tport.period_tick(tick0, k, T) for k in range(K)]
        for K1 in range(1, K):
            resumed = [tport.period_tick(tick0, k, T) for k in range(K1)] + \
                      [tport.period_tick(tick0 + K1 * T, k, T) for k in range(K - K1)]
            assert resumed == whole
            a = [(tport.clock(t0, t, dt), tport.plan_start_time(t0, t, dt)) for t in whole]
            b = [(tport.clock(t0, t, dt), tport.plan_start_time(t0, t, dt)) for t in resumed]
            assert a == b
        assert whole[-1] + T <= tport.INT32_MAX
    for tick0, K, T in REFUSED:
        assert tport.clock_refusal(tick0, K, T) is not None, (tick0, K, T)
    # each operation rounded separately: the product first
    assert tport.plan_start_time(0.3, 7, 0.01, 0.1) == (0.3 + 7.0 * 0.01) + 0.1
    # an accumulated clock drifts from the rule's within a few hundred periods
    acc, drift = t0, 0.0
    for k in range(1, 400):
        acc += 5 * dt
        drift = max(drift, abs(acc - tport.clock(t0, 5 * k, dt)))
    assert drift > 0.0


@needs_gxx
def test_host_compiled_clock_and_refusals(tmp_path):
    out = str(tmp_path / "libdriveclock.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
                    os.path.join(ROOT, "tests", "host_check", "drive_clock_check.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.dcc_clock.restype = C.c_int
    lib.dcc_clock.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_int]
    lib.dcc_times.restype = None
    lib.dcc_times.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]
    for tick0, K, T in CLOCKS:
        end, ticks = C.c_longlong(), (C.c_int * 8)()
        assert lib.dcc_clock(tick0, K, T, C.byref(end), ticks, 8) == 0, (tick0, K, T)
        assert end.value == tick0 + K * T
        assert list(ticks)[:K] == [tport.period_tick(tick0, k, T) for k in range(K)]
        for K1 in range(1, K):                                   # the resumed call's plan starts where the first one ends
            e1, t2 = C.c_longlong(), (C.c_int * 8)()
            assert lib.dcc_clock(tick0, K1, T, C.byref(e1), ticks, 8) == 0
            assert lib.dcc_clock(int(e1.value), K - K1, T, C.byref(end), t2, 8) == 0
            assert list(t2)[:K - K1] == [tport.period_tick(tick0, k, T) for k in range(K1, K)] and end.value == tick0 + K * T
    for tick0, K, T in REFUSED:
        end, ticks = C.c_longlong(), (C.c_int * 8)()
        assert lib.dcc_clock(tick0, K, T, C.byref(end), ticks, 8) == 1, (tick0, K, T)
    o = (C.c_double * 2)()
    for t0, tick, dt, lead in ((0.0, 0, 0.01, 0.1), (1234.5678, 2 ** 31 - 1, 0.01, 0.1), (-3.25, 77, 0.013, 0.0), (1e9, 5, 1e-3, 0.25)):
        lib.dcc_times(t0, tick, dt, lead, o)
        assert o[0] == tport.clock(t0, tick, dt) and o[1] == tport.plan_start_time(t0, tick, dt, lead)


# ---------------------------------------------------------------------------------------------------------------------
# the port: the request's extras, the adopt rule
# ---------------------------------------------------------------------------------------------------------------------
def test_request_extras_on_the_recorded_scenes():
    fx = dict(np.load(FIXTURE))
    hit_trunc = hit_none = 0
    for k in range(len(fx["n_act"])):
        st, acts, n = fx["state"][k], fx["actors"][k], fx["n_act"][k]
        for md in (1, 8):
            r = tport.request_timed(st, None, acts, n, 4, md, 2.5, 40, 0.01)
            base = port.request(st, None, acts, n, 4, md)
            for name in base:                                     # everything shared is drive_port's
                assert np.array_equal(np.asarray(r[name]), np.asarray(base[name]), equal_nan=True), name
            nd = r["n_dyn"]
            assert r["dyn_idx"] == list(fx["dyn_idx"][k, :int(fx["n_dyn"][k])])[:md]      # the reference's order
            for q, i in enumerate(r["dyn_idx"]):
                assert np.array_equal(r["dyn_obs"][q], acts[i])
                assert np.array_equal(r["dyn_obs"][q, :2], r["dyn"][q, :2])               # the same rows as dyn
                assert math.sqrt((acts[i, 2] * acts[i, 2] + acts[i, 3] * acts[i, 3]) + 0.0) == r["dyn"][q, 3]
            assert not r["dyn_obs"][nd:].any()
            assert r["plan_start_time"] == (2.5 + 40.0 * 0.01) + 0.1
            assert r["start_heading"] == math.atan2(r["start_v"][1], r["start_v"][0])
            hit_trunc += int(fx["n_dyn"][k]) > md
            hit_none += nd == 0
    assert hit_trunc >= 5 and hit_none >= 5


def test_adopt_rule():
    B, rows = 5, 6
    rng = np.random.default_rng(1)
    traj, track = rng.normal(size=(B, rows, 4)), rng.normal(size=(B, rows, 4))
    trajectory, profile = rng.normal(size=(B, 7, 401)), np.full((B, 7, 401), np.nan)
    profile[3] = rng.normal(size=(7, 401))
    status = np.array([0, 1, 8, 0, 0], np.int32)               # vehicle 2: path QP failed
    ref_status = np.array([0, 0, 0, 0, 1], np.int32)           # vehicle 4: the front end refused
    speed_status = np.array([0, 0, 0, 8, 0], np.int32)         # vehicle 3: speed QP failed
    traj_len = np.array([4, 6, 5, 3, 2], np.int32)
    r = tport.adopt(traj, traj_len, status, ref_status, trajectory, speed_status, track, np.full(B, 2, np.int32),
                    np.array([0, 3, 1, 0, 2], np.int32), profile, np.array([5, 6, 7, 8, 9], np.int32), np.array([0, 0, 4, 1, 2], np.int32))
    assert list(r["held"]) == [0, 0, 2, 0, 3] and list(r["track_len"]) == [4, 6, 2, 3, 2]
    assert list(r["speed_held"]) == [0, 0, 5, 2, 3] and list(r["cursor"]) == [0, 0, 7, 8, 9]
    for b in (0, 1):
        assert np.array_equal(r["profile"][b], trajectory[b])
        assert np.array_equal(r["track"][b, :traj_len[b]], traj[b, :traj_len[b]]) and np.array_equal(r["track"][b, traj_len[b]:], track[b, traj_len[b]:])
    assert np.array_equal(r["track"][3, :3], traj[3, :3]) and np.array_equal(r["profile"][3], profile[3])      # track taken, profile held
    for b in (2, 4):
        assert np.array_equal(r["track"][b], track[b]) and np.isnan(r["profile"][b]).all()                     # both held


# ---------------------------------------------------------------------------------------------------------------------
# the tracking scenario through the oracle alone
# ---------------------------------------------------------------------------------------------------------------------
def test_tracking_scenario_plans_in_every_period_on_the_cpu_oracle():
    """tests/test_gpu_drive_timed.py's closed-loop fleet (straight paths, 10 m/s, cap 50 km/h, a dynamic actor at 3 m/s 20 m ahead)
    through oracle/ref_port, st_speed, st_backend, tests/speed_target_port.py, oracle/mpc_lateral.py and tests/vehicle_port.py
    alone, in every period: the path is valid and speed_status == 0 for every vehicle-period, so the GPU comparison compares plans,
    not refusals; the timed vehicles slow down, the untimed ones speed up - the margin the GPU test takes."""
    from emplanner_carla_amd import api
    M = api.max_path_points(api.dp_params())
    cpu = tport.loop_on_the_cpu(M)
    for b in range(tport.LOOP_B):
        for k, period in enumerate(cpu[True][b]):
            assert period["path_ok"] and period["speed_status"] == 0, (b, k, period["qp_status"], period["speed_status"])
            assert period["n_dyn"] == 1 and period["speed_held"] == 0 and not (period["tgt_bits"] & 4)
            assert period["targets"].max() < 40.0                              # the profile, not the 50 km/h cap
        vt = [p["state"][5] for p in cpu[True][b]]
        vu = [p["state"][5] for p in cpu[False][b]]
        assert all(p["path_ok"] for p in cpu[False][b])
        assert vt[0] < 10.0 and all(x > y for x, y in zip(vt, vt[1:])), vt        # slower every period
        assert vu[0] > 10.0 and all(x < y for x, y in zip(vu, vu[1:])), vu        # the untimed loop accelerates towards its cap
        assert vu[-1] - vt[-1] > 1.0, (vu, vt)


def test_the_blocked_vehicle_fails_the_speed_stage_on_the_cpu_oracle():
    """The hold test's input: the path plans (qp 'optimal'), the speed QP does not (EMP_STB_QP_FAILED), in every period."""
    from emplanner_carla_amd import api
    M = api.max_path_points(api.dp_params())
    b = 1
    g = tport.blocked(tport.timed_fleet(4, 5, M), b)
    log = tport.oracle_loop(g["global_path"][b], g["state"][b], g["actors"][b], g["n_act"][b], g["pre_match_index"][b],
                            g["target_speed"][b], g["t0"][b], 3, 5, tport.MAX_OBS, tport.MAX_DYN, M + 2)
    assert [(p["path_ok"], p["speed_status"]) for p in log] == [(True, tport.STB_QP_FAILED)] * 3
    assert all(p["tgt_bits"] == 4 and (p["targets"] == g["target_speed"][b]).all() for p in log)     # no profile: the cap
