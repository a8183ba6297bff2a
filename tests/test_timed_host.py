"""CPU suite of the timed rollout (emp_speed_target, emp_rollout_timed): the header declares the two calls, the struct and the four
bits, the binding lists both prototypes, the ctypes RolloutTimedIO has the C layout (a g++ probe prints sizeof / offsetof), and
the sampling rule of csrc/emp_control_core.h - compiled with g++ -ffp-contract=off - equals tests/speed_target_port.py BIT FOR
BIT (target, cursor, bits) on 2000 generated cases.  The invariants at the end follow from the rule's definition alone."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emplanner.h")
SRC = os.path.join(ROOT, "tests", "host_check", "speed_target_check.cpp")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speed_target_port as sp  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is needed to compile the host programs")

IO_FIELDS = ["target_path", "n_path", "state", "min_index", "target_speed", "err_in", "n_err_in", "trajectory", "t0", "cursor_in",
             "state_out", "min_index_out", "err_out", "n_err_out", "status", "fail_tick", "cursor_out", "tgt_status",
             "log_state", "log_control", "log_err", "log_index", "log_target", "reserved"]


def test_header_declares_the_timed_rollout():
    text = open(HEADER).read()
    assert re.search(r"#define EMP_ABI_VERSION 13\b", text)                      # additions do not bump the version
    for name, value in (("EMP_TGT_BEFORE", 1), ("EMP_TGT_PAST", 2), ("EMP_TGT_NO_PROFILE", 4), ("EMP_TGT_CAPPED", 8),
                        ("EMP_TIMED_POINTS", 401)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert "typedef struct emp_rollout_timed_io" in text and "} emp_rollout_timed_io;" in text
    assert re.search(r"int emp_speed_target\(", text) and re.search(r"int emp_rollout_timed\(", text)
    assert "THE SAMPLING RULE IS THIS PROJECT'S DEFINITION, NOT THE REFERENCE'S" in text
    # every array of emp_rollout is a member of the struct
    decl = text[text.index("int emp_rollout("):]
    decl = decl[:decl.index(");")]
    body = text[text.index("typedef struct emp_rollout_timed_io"):text.index("} emp_rollout_timed_io;")]
    for arg in re.findall(r"\*\s*(\w+)", decl):
        if arg not in ("ctx", "lat", "pid", "vp"):
            assert re.search(rf"\*\s*{arg};", body), arg


def test_binding_lists_both_calls_and_the_constants():
    from emplanner_carla_amd import _lib, api
    assert _lib.ABI_VERSION == 13
    assert len(_lib.PROTOTYPES["emp_speed_target"][1]) == 12 and len(_lib.PROTOTYPES["emp_rollout_timed"][1]) == 12
    assert (_lib.TGT_BEFORE, _lib.TGT_PAST, _lib.TGT_NO_PROFILE, _lib.TGT_CAPPED, _lib.TIMED_POINTS) == (1, 2, 4, 8, 401)
    assert (sp.BEFORE, sp.PAST, sp.NO_PROFILE, sp.CAPPED, sp.N) == (1, 2, 4, 8, 401)
    for name in ("speed_target", "rollout_timed"):
        assert callable(getattr(api.Planner, name))
    assert list(api.TimedRolloutResult.__dataclass_fields__) == list(api.RolloutResult.__dataclass_fields__) + [
        "cursor", "tgt_status", "log_target"]


@needs_gxx
def test_rollout_timed_io_ctypes_layout_matches_the_c_struct(tmp_path):
    from emplanner_carla_amd import _lib
    assert [name for name, _ in _lib.RolloutTimedIO._fields_] == IO_FIELDS
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "emplanner.h"\nint main() {\n'
                   '    std::printf("sizeof %zu\\n", sizeof(emp_rollout_timed_io));\n'
                   + "".join(f'    std::printf("{f} %zu\\n", offsetof(emp_rollout_timed_io, {f}));\n' for f in IO_FIELDS)
                   + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
               if line)
    assert int(got["sizeof"]) == C.sizeof(_lib.RolloutTimedIO)
    for f in IO_FIELDS:
        assert int(got[f]) == getattr(_lib.RolloutTimedIO, f).offset, f


@pytest.fixture(scope="module")
def stc(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is needed to compile the host programs")
    out = str(tmp_path_factory.mktemp("speed_target_check") / "libspeedtargetcheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.stc_sample.restype = None
    lib.stc_sample.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 5
    lib.stc_count.restype = C.c_int
    lib.stc_count.argtypes = [C.c_void_p]
    return lib


def core_batch(stc, c, tick, dt, cursor=None):
    n = len(c["t0"])
    traj, t0, cap = (np.ascontiguousarray(c[k], np.float64) for k in ("traj", "t0", "cap"))
    cur = np.ascontiguousarray(c["cursor"] if cursor is None else cursor, np.int32)
    tg, co, bits = np.full(n, -7.0), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    stc.stc_sample(n, traj.ctypes.data, t0.ctypes.data, tick, dt, cap.ctypes.data, cur.ctypes.data, tg.ctypes.data, co.ctypes.data,
                   bits.ctypes.data)
    return tg, co, bits


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_core_equals_the_port_on_2000_cases_bit_for_bit(stc):
    """1000 cases at tick 0 (t0 is the clock: 'exactly on a sample' is exact) and 1000 at tick 37 with dt = 0.01 (the clock goes
    through the rounded product and sum).  The generator's coverage is asserted, not assumed."""
    seen_bits, seen_nv = set(), set()
    for seed, tick in ((11, 0), (12, 37)):
        c = sp.make_cases(1000, seed, tick=tick)
        want = sp.port_batch(c, tick, 0.01)
        got = core_batch(stc, c, tick, 0.01)
        for g, w, what in zip(got, want, ("target", "cursor", "bits")):
            assert same_bits(g, w), f"tick {tick}: {what}"
        seen_bits |= set(int(b) for b in want[2])
        nv = [sp.profile_count(list(t[4]), list(t[6])) for t in c["traj"]]
        assert nv == [stc.stc_count(np.ascontiguousarray(t).ctypes.data) for t in c["traj"]]
        seen_nv |= set(nv)
        if tick == 0:
            # the clock placements: before, on a sample, between, on the last sample, past, NaN; and the cursor / cap cases
            for i in range(len(nv)):
                if c["where"][i] == "on_last" and nv[i] > 0:
                    assert c["t0"][i] == c["traj"][i, 6, nv[i] - 1] and want[2][i] & sp.PAST
                if (c["where"][i] == "on_sample" and 1 < nv[i] and c["kind"][i] == "full" and not want[2][i] & sp.PAST
                        and c["cursor"][i] <= 0):                               # (a cursor beyond the bracket never walks back)
                    assert c["traj"][i, 6, want[1][i]] == c["t0"][i]             # the bracket starts at the sample hit
            assert any(np.isnan(c["cap"])) and any(np.isnan(c["t0"]))
            inside = [i for i in range(len(nv)) if want[2][i] & 7 == 0]
            assert any(c["cursor"][i] < 0 for i in inside) and any(c["cursor"][i] > nv[i] - 2 for i in inside)
            assert {"equal_times", "backwards", "nan_speed", "nan_time"} <= set(c["kind"][i] for i in inside)
    assert {0, 1, 2, 3, 400, 401} <= seen_nv
    assert {0, sp.BEFORE, sp.PAST, sp.NO_PROFILE, sp.CAPPED, sp.BEFORE | sp.CAPPED, sp.PAST | sp.CAPPED} <= seen_bits


def ascending_case(seed):
    rng = np.random.default_rng(seed)
    c = sp.make_case(rng, kind="full", where="between")
    return c


def test_any_cursor_at_or_below_the_bracket_gives_the_same_result(stc):
    rng = np.random.default_rng(3)
    for seed in range(20):
        c = ascending_case(seed)
        speed, time = list(c["traj"][4]), list(c["traj"][6])
        cap = float("nan")
        t, j, bits = sp.speed_target(speed, time, sp.N, c["t0"], cap, 0)
        assert bits == 0 and time[j] <= c["t0"] < time[j + 1]
        lo, hi = sorted((speed[j], speed[j + 1]))
        assert 3.6 * lo <= t <= 3.6 * hi                                         # between the bracket's two speeds
        cursors = np.array([0, j, -9] + list(rng.integers(0, j + 1, 13)), np.int32)
        batch = dict(traj=np.repeat(c["traj"][None], len(cursors), 0), t0=np.full(len(cursors), c["t0"]),
                     cap=np.full(len(cursors), cap), cursor=cursors)
        tg, co, b = core_batch(stc, batch, 0, 0.01)
        assert (co == j).all() and (b == 0).all() and same_bits(tg, np.full(len(cursors), t))


def test_a_resumed_sequence_gives_the_single_sequence_bit_for_bit(stc):
    """Ticks 0 .. T - 1 with the cursor carried along, against ticks 0 .. T1 - 1 and then tick0 = T1 from the first part's cursor -
    on rows the clock enters, crosses and leaves."""
    c = sp.make_cases(64, 5)
    finite = np.isfinite(c["t0"])
    c["t0"] = np.where(finite, c["t0"] - 0.3, c["t0"])
    T, T1, dt = 90, 31, 0.01

    def run(ticks, cursor):
        out = []
        for t in ticks:
            tg, cursor, bits = core_batch(stc, c, t, dt, cursor)
            out.append((tg, cursor.copy(), bits))
        return out, cursor
    whole, _ = run(range(T), c["cursor"])
    first, cur = run(range(T1), c["cursor"])
    second, _ = run(range(T1, T), cur)
    for a, b in zip(whole, first + second):
        assert all(same_bits(x, y) for x, y in zip(a, b))
    cur = c["cursor"]
    for t in range(T):                                                           # and the port walks the same way
        tg, cur, bits = sp.port_batch(c, t, dt, cur)
        assert same_bits(tg, whole[t][0]) and same_bits(cur, whole[t][1]) and same_bits(bits, whole[t][2])
    assert (whole[-1][1] != whole[0][1]).any()                                   # cursors did advance on some rows
