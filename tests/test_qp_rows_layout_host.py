"""CPU check of the LDS layout of the path QP's rows form (csrc/emp_qp_core.h, PathQpRowsLayout), compiled with g++
(tests/host_check/qp_rows_layout_check.cpp): for every (GP, R) the kernel is instantiated with, the bytes the launcher asks for
against the kernel's own carve-up, the arrays against each other, and every window the solver reads against the padding
that path_qp_group_rows writes - no window may leave its group's region or meet a double that is neither the problem's own
nor padded."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "qp_rows_layout_check.cpp")
FORMS = [(8, 3), (8, 4), (16, 4)]
NAMES = ("C", "cc", "P", "q", "u", "dua", "rhs", "c", "lo", "hi", "tmp", "wgt", "words", "result", "path", "obstacles", "stride",
         "max_stations")


@pytest.fixture(scope="module")
def ql(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("qp_rows_layout") / "libqprowslayout.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.ql_offsets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.ql_wave_bytes.restype = C.c_longlong
    lib.ql_wave_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.ql_replay.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong]
    return lib


def _offsets(ql, gp, r, max_obs):
    out = np.zeros(len(NAMES), np.int64)
    assert ql.ql_offsets(gp, r, max_obs, out.ctypes.data) == 0
    return dict(zip(NAMES, (int(x) for x in out)))


@pytest.mark.parametrize("gp,r", FORMS)
@pytest.mark.parametrize("max_obs", [0, 1, 8, 24, 25, 32, 33, 64, 65, 200])
def test_launcher_bytes_cover_the_kernels_carve_up(ql, gp, r, max_obs):
    o = _offsets(ql, gp, r, max_obs)
    cap = gp * r
    assert o["C"] == cap and o["max_stations"] == cap + 2
    # arrays in order, none overlapping, guards of the documented widths between them
    assert o["P"] - (o["cc"] + cap + 4) == 12                      # three Hessian rows above row 0
    assert o["q"] == o["P"] + 4 * cap
    assert o["u"] - (o["q"] + cap) == 3 and o["dua"] - (o["u"] + cap) == 3 and o["rhs"] - (o["dua"] + cap) == 2
    assert o["c"] == o["rhs"] + cap and o["lo"] == o["c"] + 2 * cap and o["hi"] == o["lo"] + 2 * cap and o["tmp"] == o["hi"] + 2 * cap
    assert o["wgt"] - (o["tmp"] + 2 * cap) == 4 and o["words"] - (o["wgt"] + 2 * cap) == 4
    # the arrays of the kernel around the solver fit into the solver arrays they borrow
    assert o["result"] + o["max_stations"] <= o["rhs"] + cap
    assert o["path"] + 4 * o["max_stations"] <= o["words"]
    obstacle_end = o["obstacles"] + 4 * max_obs
    assert obstacle_end <= (o["q"] if max_obs <= cap else o["stride"])
    # an odd stride (the groups of a wavefront walk across the LDS banks), and the launcher's bytes are the groups' strides
    assert o["stride"] % 2 == 1 and o["stride"] >= max(o["words"], obstacle_end)
    assert ql.ql_wave_bytes(gp, r, max_obs) == (64 // gp) * o["stride"] * 8
    assert ql.ql_wave_bytes(gp, r, max_obs) <= 160 * 1024            # one CU's LDS


@pytest.mark.parametrize("gp,r", FORMS)
def test_every_window_stays_in_its_group_and_meets_padding_outside_the_problem(ql, gp, r):
    cap = gp * r
    for max_obs in (8, cap + 1):
        wave = ql.ql_wave_bytes(gp, r, max_obs)
        for n in [0, 4, 5, 6, 7, 21, cap - 1, cap, cap + 1, cap + 2]:       # stations of a scene; 0: a group without a problem
            N, ns = max(n - 4, 0), max(n - 2, 0) if n else 0
            assert ql.ql_replay(gp, r, max_obs, N, ns, wave) == 0, (max_obs, n)
    # the check itself: a wavefront two doubles short (the odd stride leaves one spare) loses the last guard entry
    wave = ql.ql_wave_bytes(gp, r, 8)
    assert ql.ql_replay(gp, r, 8, cap - 2, cap, wave - 16) != 0
