"""CPU suite of the ABI 13 trajectory call (emp_plan_trajectory): the header declares it and emp_speed_io, the ctypes
SpeedIO has the C layout (a tiny C++ program compiled with g++ prints sizeof / offsetof), and the test_10 request packer
feeds fields 6 and 7 of the first dynamic obstacle to the path half - on a stub planner, no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emplanner.h")


def test_header_declares_abi_13_and_the_trajectory_call():
    text = open(HEADER).read()
    assert re.search(r"#define EMP_ABI_VERSION 13\b", text)
    assert "typedef struct emp_speed_io" in text and "} emp_speed_io;" in text
    assert re.search(r"int emp_plan_trajectory\(", text)
    from emplanner_carla_amd import _lib
    assert _lib.ABI_VERSION == 13
    assert "emp_plan_trajectory" in _lib.PROTOTYPES


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is needed to compile the layout probe")
def test_speed_io_ctypes_layout_matches_the_c_struct(tmp_path):
    from emplanner_carla_amd import _lib
    fields = [name for name, _ in _lib.SpeedIO._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "emplanner.h"\nint main() {\n'
                   '    std::printf("sizeof %zu\\n", sizeof(emp_speed_io));\n'
                   + "".join(f'    std::printf("{f} %zu\\n", offsetof(emp_speed_io, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
               if line)
    assert int(got["sizeof"]) == ctypes.sizeof(_lib.SpeedIO)
    for f in fields:
        assert int(got[f]) == getattr(_lib.SpeedIO, f).offset, f


def _test10_request(seed, n_dyn):
    rng = np.random.default_rng(seed)
    path = [(float(i * 2.0), float(0.01 * i), 0.005, 0.0) for i in range(120)]
    static = [(40.0, 1.0, 12.0)]
    dynamic = [tuple(float(x) for x in rng.normal(size=6)) + (float(20 + j), float(3 + j)) for j in range(n_dyn)]
    return (static, dynamic, (10.0, 0.0), (12.0, 0.1), (5.0, 0.5), (0.2, -0.1), path, [7], 100.0 + seed)


class _StubPlanner:
    """Records what plan_trajectory_requests hands to plan_cycle and answers with planned-looking arrays."""

    def plan_cycle(self, p, q, sp, ref_line, n_ref, max_pts=None, **kw):
        from emplanner_carla_amd.api import CycleResult, TrajectoryResult
        self.kw = kw
        B = len(kw["n_global"])
        traj = np.zeros((B, max_pts + 1, 4))
        speed = TrajectoryResult(trajectory=np.arange(B * 7 * 401, dtype=np.float64).reshape(B, 7, 401),
                                 speed_status=np.array([0, 4, 0][:B], np.int32))
        return CycleResult(dp_rows=None, dp_s=None, dp_l=None, dp_len=None, path_s=np.zeros((B, max_pts)),
                           path_l=np.zeros((B, max_pts)), path_len=np.full(B, 3, np.int32), traj=traj,
                           traj_len=np.full(B, 5, np.int32), status=np.array([0, 0, 8][:B], np.int32),
                           match_index=np.array([11, 12, 13][:B], np.int32), ref_status=np.zeros(B, np.int32), speed=speed)


def test_trajectory_request_packing_takes_dynamic_fields_6_and_7():
    from emplanner_carla_amd import service
    reqs = [_test10_request(0, 2), _test10_request(1, 0), _test10_request(2, 3)]
    a = service.pack_trajectory_requests(reqs)
    # the path half's (dis, speed) of the first dynamic obstacle: fields 6 and 7 (test_10.py:136 reads them as 2 and 3)
    assert np.array_equal(a["dyn"][0], [20.0, 3.0]) and np.isnan(a["dyn"][1]).all() and np.array_equal(a["dyn"][2], [20.0, 3.0])
    assert a["dyn_obs"].shape == (3, 3, 4) and a["n_dyn"].tolist() == [2, 0, 3]
    assert np.array_equal(a["dyn_obs"][2], np.asarray([o[:4] for o in reqs[2][1]]))
    assert a["plan_start_time"].tolist() == [100.0 + 0.1, 101.0 + 0.1, 102.0 + 0.1]
    assert np.allclose(a["start_heading"], np.arctan2(0.5, 5.0))
    # the same path arrays as the test_9 packer on the re-shaped requests
    a9 = service.pack_requests([service.as_test9_request(r) for r in reqs])
    for k, v in a9.items():
        assert np.array_equal(a[k], v, equal_nan=True), k
    assert service.as_test9_request(reqs[0])[1] == [(o[0], o[1], o[6], o[7]) for o in reqs[0][1]]
    with pytest.raises(ValueError):
        service.pack_trajectory_requests([_test10_request(3, 65)])

    stub = _StubPlanner()
    out = service.plan_trajectory_requests(stub, reqs)
    kw = stub.kw
    assert np.array_equal(kw["dyn_dis_speed"], a["dyn"], equal_nan=True)
    assert np.array_equal(kw["speed"].dyn_obs, a["dyn_obs"]) and kw["speed"].intermediates is False
    assert np.array_equal(kw["speed"].plan_start_time, a["plan_start_time"])
    assert kw["pre_match_index"].tolist() == [7, 7, 7]
    reply, lists, status, speed_status = out[0]
    assert reply[1] == [11] and len(reply[0]) == 5 and len(reply[2]) == 3        # the global-path match index
    assert len(lists) == 7 and lists[6][0] == 6 * 401.0 and speed_status == 0
    assert out[1][1] is None and out[1][3] == 4 and out[1][0] is not None          # speed status set: no trajectory lists
    assert out[2][0] is None and out[2][1] is None and out[2][2] == 8              # the path refused: no reply, no trajectory


def test_speed_with_slot_is_refused_before_any_call():
    from emplanner_carla_amd import api
    pl = api.Planner.__new__(api.Planner)           # no context: the refusal comes first
    speed = api.TrajectoryInputs(api.speed_dp_params(), api.speed_qp_params(), np.zeros((1, 1, 4)), np.zeros(1, np.int32),
                                 np.zeros(1))
    with pytest.raises(ValueError, match="slot"):
        pl.plan_cycle(None, None, None, None, None, None, None, None, None, None, None, slot=object(), speed=speed)
