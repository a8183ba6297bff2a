"""CPU suite of the fleet loop (emp_drive_request, emp_drive): the header declares the calls and both structs and the ABI is
still 13; the ctypes layouts equal the C structs (a g++ sizeof / offsetof probe); tests/drive_port.py - the request in Python
floats, written from the header's formulas - reproduces what the reference's own get_actor_from_world and predict_block recorded
in tests/golden/drive/drive_request.npz: kept indices and order exactly, dis and speed bit for bit, the prediction to 1e-12
relative (scale 1: libm enters); the fixture regenerates bit for bit where the reference is present; truncation, which the
reference does not have, is the first max_obs of the port's uncapped list; plan_drive_request covers every vehicle."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "drive", "drive_request.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import drive_port as port  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is needed to compile the host programs")

DRIVE_PARAMS_FIELDS = ["dis_limitation", "lateral_band", "behind", "dynamic_speed", "static_gate", "pred_ts", "advance_s", "reserved"]
DRIVE_IO_FIELDS = ["global_path", "n_global", "state", "accel", "actors", "n_act", "pre_match_index", "track", "track_len", "held",
                   "state_out", "accel_out", "actors_out", "pre_match_index_out", "track_out", "track_len_out", "held_out",
                   "log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len", "reserved"]


def test_header_declares_the_fleet_loop():
    text = open(HEADER).read()
    assert re.search(r"#define EMP_ABI_VERSION 13\b", text)                      # additions do not bump the version
    for struct in ("emp_drive_params", "emp_drive_io"):
        assert f"typedef struct {struct}" in text and f"}} {struct};" in text
    assert re.search(r"void emp_drive_params_default\(", text)
    assert re.search(r"int emp_drive_request\(", text) and re.search(r"int emp_drive\(", text)
    assert re.search(r"#define EMP_DRIVE_MAX_PERIODS 4096\b", text) and re.search(r"#define EMP_DRV_TRUNCATED 1\b", text)
    from emplanner_carla_amd import _lib
    assert _lib.ABI_VERSION == 13 and _lib.DRIVE_MAX_PERIODS == 4096 and _lib.DRV_TRUNCATED == 1
    for name in ("emp_drive_params_default", "emp_drive_request", "emp_drive"):
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["emp_drive_request"][1]) == 25 and len(_lib.PROTOTYPES["emp_drive"][1]) == 20


@needs_gxx
def test_ctypes_layouts_match_the_c_structs(tmp_path):
    from emplanner_carla_amd import _lib
    pairs = (("emp_drive_params", _lib.DriveParams, DRIVE_PARAMS_FIELDS), ("emp_drive_io", _lib.DriveIO, DRIVE_IO_FIELDS))
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
    p = api.drive_params()
    assert (p.dis_limitation, p.lateral_band, p.behind, p.dynamic_speed, p.static_gate, p.pred_ts, p.advance_s, p.reserved) == \
        (50.0, 5.0, -10.0, 1.0, 30.0, 0.2, 0.0, 0)
    assert tuple(port.DEFAULTS[k] for k in DRIVE_PARAMS_FIELDS[:-1]) == (50.0, 5.0, -10.0, 1.0, 30.0, 0.2, 0.0)
    for name in ("drive_request", "drive"):
        assert callable(getattr(api.Planner, name))
    assert [f for f in api.DriveResult.__dataclass_fields__] == [
        "state", "accel", "actors", "pre_match_index", "track", "track_len", "held", "log_state", "log_plan_status",
        "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len"]
    assert [f for f in api.DriveRequest.__dataclass_fields__] == [
        "static_xy", "n_static", "static_dis", "dyn", "n_dyn", "dyn_dis_speed", "n_obs", "origin_xy", "start_xy", "pred_fi",
        "start_v", "start_a", "req_status", "actors_next"]
    # the drop-in modules keep the reference's surface
    import emplanner_carla_amd.planner.planning_utils as pu
    assert not hasattr(pu, "drive") and not hasattr(pu, "drive_request")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def test_fixture_covers_the_cases_and_keeps_its_margins(fx):
    n_act = fx["n_act"]
    assert 90 <= len(n_act) <= 100
    for n in (0, 1, 63, 64):
        assert (n_act == n).any(), n
    margin = float(fx["margin"])
    seen = dict(all_static=False, all_dynamic=False, behind=False, outside=False, beyond=False, gate=False, dup=False, still=False)
    for k in range(len(n_act)):
        st, n = fx["state"][k], int(n_act[k])
        m = np.array([port.measure(st, fx["actors"][k, i]) for i in range(n)]).reshape(n, 4)
        for col, thresholds in ((0, (50.0, 30.0)), (1, (5.0, -5.0)), (2, (-10.0,)), (3, (1.0,))):
            for t in thresholds:
                assert n == 0 or np.min(np.abs(m[:, col] - t)) >= margin, (k, col, t)
        ns, nd = int(fx["n_static"][k]), int(fx["n_dyn"][k])
        seen["all_static"] |= ns > 1 and nd == 0
        seen["all_dynamic"] |= nd > 1 and ns == 0
        seen["behind"] |= n > 0 and bool((m[:, 2] < -10.0).any())
        seen["outside"] |= n > 0 and bool((np.abs(m[:, 1]) > 5.0).any())
        seen["beyond"] |= n > 0 and bool((m[:, 0] > 50.0).any())
        seen["gate"] |= ns > 0 and fx["static_dis"][k, 0] > 30.0
        d = np.concatenate([fx["static_dis"][k, :ns], fx["dyn_dis"][k, :nd]])
        seen["dup"] |= len(np.unique(d)) < len(d)
        seen["still"] |= st[5] == 0.0 and st[3] == 0.0 and n > 1 and bool((m[:, 2] == 0.0).all())
        # ties on dis are exact duplicates only
        pos = fx["actors"][k, :n, :2]
        for i in range(n):
            for j in range(i + 1, n):
                if m[i, 0] == m[j, 0]:
                    assert np.array_equal(pos[i], pos[j]), (k, i, j)
    assert all(seen.values()), seen


def test_port_reproduces_the_reference(fx):
    for k in range(len(fx["n_act"])):
        st = fx["state"][k]
        statics, dynamics = port.perceive(st, fx["actors"][k], fx["n_act"][k])
        ns, nd = int(fx["n_static"][k]), int(fx["n_dyn"][k])
        assert [i for i, _ in statics] == list(fx["static_idx"][k, :ns]), k             # indices and order: exact
        assert [i for i, _, _ in dynamics] == list(fx["dyn_idx"][k, :nd]), k
        assert np.array_equal([d for _, d in statics], fx["static_dis"][k, :ns]), k     # dis, speed: bit for bit
        assert np.array_equal([d for _, d, _ in dynamics], fx["dyn_dis"][k, :nd]), k
        assert np.array_equal([s for _, _, s in dynamics], fx["dyn_speed"][k, :nd]), k
        got, want = np.array(port.predict(st, float(fx["pred_ts"]))), fx["pred"][k]
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), (k, got, want)


def test_truncation_is_the_head_of_the_uncapped_list(fx):
    """The reference has no cap: the capped request is the first max_obs (max_dyn) of the port's uncapped lists."""
    hit = 0
    for k in range(len(fx["n_act"])):
        st, acts, n = fx["state"][k], fx["actors"][k], fx["n_act"][k]
        statics, dynamics = port.perceive(st, acts, n)
        for mo, md in ((1, 8), (8, 2)):
            r = port.request(st, None, acts, n, mo, md)
            assert r["static_idx"] == [i for i, _ in statics][:mo] and r["dyn_idx"] == [i for i, _, _ in dynamics][:md]
            assert r["n_static"] == min(len(statics), mo) and r["n_dyn"] == min(len(dynamics), md)
            assert r["req_status"] == (port.TRUNCATED if len(statics) > mo or len(dynamics) > md else 0)
            assert np.array_equal(r["static_dis"][:r["n_static"]], [d for _, d in statics][:mo])
            assert not r["static_dis"][r["n_static"]:].any() and not r["static_xy"][r["n_static"]:].any()
            assert r["n_obs"] == (r["n_static"] if statics and statics[0][1] <= 30.0 else 0)
            hit += len(statics) > mo
    assert hit >= 10


def test_request_fixture_regenerates_from_the_reference_bit_for_bit(tmp_path):
    """As tests/test_reference_live.py for the fixture this file reads (that file's generator list is a yardstick)."""
    sys.path.insert(0, GOLDEN)
    import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("the reference tree is not present (fixture regeneration runs only where it is)")
    env = dict(os.environ, EMP_GOLDEN_OUT=str(tmp_path), EMP_SKIP_TORCH_PRELOAD="1", OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    p = subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_golden_drive.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    want = np.load(FIXTURE)
    got = np.load(os.path.join(str(tmp_path), "drive_request.npz"))
    assert sorted(want.files) == sorted(got.files)
    for k in want.files:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, k
        assert np.array_equal(want[k], got[k], equal_nan=True), k


@needs_gxx
def test_launch_plan_covers_the_fleet(tmp_path):
    out = str(tmp_path / "libdriveplan.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", os.path.join(ROOT, "tests", "host_check", "drive_plan_check.cpp"),
                    "-o", out], check=True)
    lib = C.CDLL(out)
    lib.dpc_plan.restype = None
    lib.dpc_plan.argtypes = [C.c_int, C.POINTER(C.c_int)]
    blocks = set()
    for B in (0, 1, 63, 64, 65, 70, 32768):
        o = (C.c_int * 4)()
        lib.dpc_plan(B, o)
        wpb, grid, block, refused = list(o)
        assert not refused
        assert wpb >= 1 and block == 64 * wpb and block <= 256                  # the kernels' __launch_bounds__
        assert grid * wpb >= B and (grid - 1) * wpb < max(B, 1), (B, wpb, grid)   # covers B, no idle block
        blocks.add(block)
    assert blocks == {64, 256}                                                  # every block size the plan may choose was seen
    o = (C.c_int * 4)()
    lib.dpc_plan(-1, o)
    assert o[3] == 1


def test_the_reference_path_follows_the_last_bits_of_its_start():
    """Why tests/test_gpu_drive.py compares the loop with the CPU port stage by stage and not end to end.  The reference sizes
    every densified DP segment with int(end_s - start_s) (path_planning.py:405, :423; oracle/ref_port.enrich_DP_s_l), and with
    the driver's sample_s = 15 that is int((s0 + 15 (i + 1)) - (s0 + 15 i)) = int(15 -+ 1 ulp): 8 samples or 7, by the last
    bits of the planning start's s0.  Here the predicted location of one scene (a straight path, a static actor 25 m ahead) moves
    by multiples of 1e-13 m: the DP rows never change, the start's s moves by less than 1e-11 - and the path's stations, and
    with them the trajectory, jump by a whole 2 m sample."""
    import math
    sys.path.insert(0, ROOT)
    from oracle import ref_port
    rot, n = 0.3, 80
    d = np.arange(n) * 2.0
    path = [(5.0 + t * math.cos(rot), -3.0 + t * math.sin(rot), rot, 0.0) for t in d]
    at = lambda ahead, side: (5.0 + ahead * math.cos(rot) - side * math.sin(rot), -3.0 + ahead * math.sin(rot) + side * math.cos(rot))
    state = [*at(10.37, 0.2), rot, 0.0, 0.0, 8.13]
    actor = [*at(35.37, 1.2), 0.0, 0.0]
    statics, _ = port.perceive(state, [actor], 1)
    px, py, _ = port.predict(state, 0.2)
    seen = []
    for k in range(12):
        req = ([(actor[0], actor[1], statics[0][1])], [], (state[0], state[1]), (px + k * 1e-13, py - k * 1e-13),
               port.world_velocity(state[2], state[3], state[5]), (0.0, 0.0), path, [5])
        traj, _, path_s, _, out = ref_port.motion_planning_body(req)
        seen.append((out["begin_s"], list(out["dp_rows"]), np.array(out["dp_s"]), np.array(traj)))
    assert all(r == seen[0][1] for _, r, _, _ in seen)                          # one and the same DP decision
    assert max(abs(b - seen[0][0]) for b, _, _, _ in seen) < 1e-11              # one and the same start, to 1e-11 m
    counts = {len(s_) for _, _, s_, _ in seen}
    shift = max(np.abs(s_[:40] - seen[0][2][:40]).max() for _, _, s_, _ in seen)
    moved = max(np.abs(t[:20, :2] - seen[0][3][:20, :2]).max() for _, _, _, t in seen)
    assert shift >= 1.99, f"stations moved by {shift}"                          # a whole sample
    assert moved >= 0.5, f"trajectory moved by {moved}"                         # metres, from 1e-13 m
    # the arithmetic behind it, alone
    node = lambda s0, i: s0 if i == 0 else s0 + i * 15            # the segment ends as DP_algorithm forms them (ref_port :176)
    widths = {int(node(b, i + 1) - node(b, i)) for b, _, _, _ in seen for i in range(6)}
    assert widths == {14, 15} and len(counts) > 1, (widths, counts)
