"""CPU suite of the shared world (emp_world_exchange, emp_traffic_rollout_epoch, emp_world_drive): the header declares the calls and
the ABI is still 13; the ctypes layouts equal the C structs (a g++ sizeof / offsetof probe); the g++ build of csrc/emp_world_core.h
(tests/host_check/world_check.cpp) against the NumPy port (tests/world_port.py) bit for bit - keys, counts, status and the gather
order - on seeded and on hand-built cases, the match also as 64 lanes and the kernel's butterfly make it; that build under the
address and undefined-behaviour sanitizers as a program of its own; the launch plan, the offsets rule and the two clocks as pure
host code."""
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
SRC = os.path.join(ROOT, "tests", "host_check", "world_check.cpp")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import world_port as wp  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is needed to compile the host programs")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is needed to compile the host programs")
    out = str(tmp_path_factory.mktemp("world_check") / "libworldcheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    p, i, q, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.wc_exchange.restype = None
    lib.wc_exchange.argtypes = [i] * 8 + [p] * 16
    lib.wc_match64.restype = i
    lib.wc_match64.argtypes = [i, i, i, p, p, p, p]
    lib.wc_plan.restype = C.c_char_p
    lib.wc_plan.argtypes = [i] * 8 + [p]
    lib.wc_ego_off.restype = C.c_char_p
    lib.wc_ego_off.argtypes = [p, i, i]
    lib.wc_epoch.restype = C.c_char_p
    lib.wc_epoch.argtypes = [q, q]
    lib.wc_clock.restype = C.c_char_p
    lib.wc_clock.argtypes = [i, i, d, i, d, q, p, i]
    return lib


def host_exchange(lib, c, agent_rows, ego_rows, max_act, max_other, see_egos=0, lane_window=50):
    """wc_exchange on a case: every output starts as 7s, so a slot the rule leaves alone shows."""
    W, N = c["agent_state"].shape[:2]
    B, G = c["global_path"].shape[:2]
    ins = [np.ascontiguousarray(c[k], dt) for k, dt in (("n_world", np.int32), ("ego_off", np.int32), ("ego_state", np.float64),
                                                        ("ego_extent", np.float64), ("global_path", np.float64), ("n_global", np.int32),
                                                        ("ego_lane", np.int32), ("pre_match_index", np.int32))]
    ins += [np.ascontiguousarray(agent_rows, np.float64), np.ascontiguousarray(ego_rows, np.float64)]
    o = dict(actors=np.full((B, max_act, 4), 7.0), n_act=np.full(B, 7, np.int32), other=np.full((W, max_other, 5), 7.0),
             other_lane=np.full((W, max_other), 7, np.int32), n_other=np.full(W, 7, np.int32), wx_status=np.full(B, 7, np.int32))
    lib.wc_exchange(W, B, N, G, max_act, max_other, lane_window, see_egos, *[x.ctypes.data for x in ins],
                    *[(o[k].ctypes.data if o[k].size else None) for k in wp.OUT])
    return o


def port_exchange(c, agent_rows, ego_rows, **kw):
    """The port on a case; with max_other == 0 the call does not touch n_other, which keeps host_exchange's 7s."""
    r = wp.exchange(c["n_world"], c["ego_off"], c["ego_state"], c["ego_extent"], c["global_path"], c["n_global"], c["ego_lane"],
                    c["pre_match_index"], agent_rows, ego_rows, **kw)
    if kw["max_other"] == 0:
        r["n_other"][:] = 7
    return r


def match64(lib, c, b, lane_window):
    G = c["global_path"].shape[1]
    a = [np.ascontiguousarray(c[k], dt) for k, dt in (("ego_state", np.float64), ("global_path", np.float64), ("n_global", np.int32),
                                                      ("pre_match_index", np.int32))]
    return lib.wc_match64(G, lane_window, b, *[x.ctypes.data for x in a])


# ---- the header and the binding -----------------------------------------------------------------------------------------------------
def test_header_declares_the_world_calls():
    text = open(HEADER).read()
    assert re.search(r"#define EMP_ABI_VERSION 13\b", text)                      # additions do not bump the version
    for struct in ("emp_world_exchange_io", "emp_world_params", "emp_world_io"):
        assert f"typedef struct {struct}" in text and f"}} {struct};" in text
    for name in ("emp_world_exchange", "emp_traffic_rollout_epoch", "emp_world_drive"):
        assert re.search(rf"int {name}\(", text), name
    assert re.search(r"void emp_world_params_default\(", text)
    from emplanner_carla_amd import _lib
    for name, v in (("ACT_TRUNCATED", wp.ACT_TRUNCATED), ("NOT_LISTED", wp.NOT_LISTED), ("NO_WORLD", wp.NO_WORLD)):
        assert f"#define EMP_WX_{name} {v}\n" in text and getattr(_lib, "WX_" + name) == v
    assert _lib.ABI_VERSION == 13
    assert len(_lib.PROTOTYPES["emp_world_exchange"][1]) == 11 and len(_lib.PROTOTYPES["emp_world_drive"][1]) == 29
    # the epoch call is the hazards call with one more argument
    assert _lib.PROTOTYPES["emp_traffic_rollout_epoch"][1][:17] == _lib.PROTOTYPES["emp_traffic_rollout_hazards"][1]
    assert _lib.PROTOTYPES["emp_traffic_rollout_epoch"][1][17:] == [C.c_int64]


@needs_gxx
def test_ctypes_layouts_match_the_c_structs(tmp_path):
    from emplanner_carla_amd import _lib
    pairs = (("emp_world_exchange_io", _lib.WorldExchangeIO), ("emp_world_params", _lib.WorldParams), ("emp_world_io", _lib.WorldIO))
    body = ""
    for cname, cls in pairs:
        body += f'    std::printf("{cname}.sizeof %zu\\n", sizeof({cname}));\n'
        body += "".join(f'    std::printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));\n' for f, _ in cls._fields_)
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "emplanner.h"\nint main() {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if line)
    for cname, cls in pairs:
        assert int(got[f"{cname}.sizeof"]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    # emp_world_io is emp_drive_timed_io without actors and n_act, then the exchange's three, in that order
    timed = [n for n, _ in _lib.DriveTimedIO._fields_ if n not in ("actors", "n_act", "reserved")]
    world = [n for n, _ in _lib.WorldIO._fields_]
    ins = timed[:timed.index("state_out")]
    assert world[:len(ins) + 3] == ins + ["ego_off", "ego_extent", "ego_lane"]
    assert world[len(ins) + 3:len(timed) + 3] == timed[len(ins):]


def test_python_surface():
    from emplanner_carla_amd import api, traffic
    for name in ("world_exchange", "traffic_rollout_epoch", "world_drive"):
        assert callable(getattr(api.Planner, name)), name
    assert list(api.WorldExchangeResult.__dataclass_fields__) == list(wp.OUT)
    assert list(api.WorldDriveResult.__dataclass_fields__)[:2] == ["egos", "traffic"]
    assert callable(traffic.World.drive)


# ---- the core, compiled with g++, against the port ----------------------------------------------------------------------------------
@pytest.mark.parametrize("see_egos", [0, 1])
@pytest.mark.parametrize("seed", range(6))
def test_core_equals_the_port_on_seeded_cases(lib, seed, see_egos):
    c = wp.seeded(seed, W=4, N=5, per_world=(0, 1, 3, 2), outside=2) if seed % 2 else wp.seeded(seed)
    rng = np.random.default_rng(100 + seed)
    W, N = c["agent_state"].shape[:2]
    B = len(c["ego_state"])
    agent_rows, ego_rows = wp.rows_of(rng, (W, N)), wp.rows_of(rng, (B,))
    for max_act, max_other, window in ((8, 4, 50), (3, 2, 2), (1, 0, 0), (64, 64, 5)):
        kw = dict(max_act=max_act, max_other=max_other, see_egos=see_egos, lane_window=window)
        got, want = host_exchange(lib, c, agent_rows, ego_rows, **kw), port_exchange(c, agent_rows, ego_rows, **kw)
        for k in wp.OUT:
            assert wp.same_bits(got[k], want[k]), (seed, kw, k)
        for b in range(B):
            if want["match"][b] >= 0:
                assert match64(lib, c, b, window) == want["match"][b], (seed, b, window)


@pytest.mark.parametrize("name", sorted(wp.hand_built()))
def test_core_and_port_on_the_hand_built_cases(lib, name):
    c, settings, expect = wp.hand_built()[name]
    kw = dict(wp.SETTINGS, **settings)
    rng = np.random.default_rng(5)
    W, N = c["agent_state"].shape[:2]
    B = len(c["ego_state"])
    agent_rows, ego_rows = wp.rows_of(rng, (W, N)), wp.rows_of(rng, (B,))
    got, want = host_exchange(lib, c, agent_rows, ego_rows, **kw), port_exchange(c, agent_rows, ego_rows, **kw)
    for k in wp.OUT:
        assert wp.same_bits(got[k], want[k]), (name, k)
    # ... and what the case is for did happen
    if "match" in expect:
        assert want["match"][0] == expect["match"], (name, want["match"])
        assert match64(lib, c, 0, kw["lane_window"]) == expect["match"]
        key = expect.get("key", None if expect["match"] < 0 else int(c["ego_lane"][0, expect["match"]]))
        assert got["other_lane"][0, 0] == key and got["n_other"][0] == 1
        assert wp.same_bits(got["other"][0, 0], np.append(ego_rows[0], c["ego_extent"][0]))
    for k, field in (("n_act", "n_act"), ("status", "wx_status"), ("n_other", "n_other")):
        if k in expect:
            assert got[field].tolist() == expect[k], (name, k, got[field])
    # slots at and past the counts are written: rows 0, key -1
    for b in range(B):
        assert not got["actors"][b, got["n_act"][b]:].any()
    for w in range(W):
        assert not got["other"][w, got["n_other"][w]:].any() and (got["other_lane"][w, got["n_other"][w]:] == -1).all()


def test_the_gather_order(lib):
    """Agents in slot order, then the world's other egos in index order without the ego itself; rows past max_act dropped."""
    c, _, _ = wp.hand_built()["max_act smaller than agents plus egos"]
    rng = np.random.default_rng(9)
    agent_rows, ego_rows = wp.rows_of(rng, (1, 3)), wp.rows_of(rng, (3,))
    got = host_exchange(lib, c, agent_rows, ego_rows, max_act=8, max_other=3, see_egos=1)
    for b, others in ((0, [1, 2]), (1, [0, 2]), (2, [0, 1])):
        assert wp.same_bits(got["actors"][b, :3], agent_rows[0]) and wp.same_bits(got["actors"][b, 3:5], ego_rows[others])
        assert got["n_act"][b] == 5 and not got["actors"][b, 5:].any()
    cut = host_exchange(lib, c, agent_rows, ego_rows, max_act=4, max_other=3, see_egos=1)
    assert wp.same_bits(cut["actors"], got["actors"][:, :4])
    blind = host_exchange(lib, c, agent_rows, ego_rows, max_act=8, max_other=3, see_egos=0)
    assert blind["n_act"].tolist() == [3, 3, 3] and wp.same_bits(blind["other"], got["other"])      # seen all the same


def test_clamped_offsets_stay_inside_the_arrays(lib):
    """Offsets no host check saw (EMP_DEVICE): clamped as the header says, and the port agrees."""
    c = wp.seeded(3)
    B = len(c["ego_state"])
    rng = np.random.default_rng(4)
    agent_rows, ego_rows = wp.rows_of(rng, (3, 4)), wp.rows_of(rng, (B,))
    for off in ([-5, 2, 1, 99], [3, 3, 3, 3], [2 ** 31 - 1, -2 ** 31, 0, 2], [0, 0, 0, 0]):
        c["ego_off"] = np.array(off, np.int32)
        kw = dict(max_act=5, max_other=3, see_egos=1)
        got, want = host_exchange(lib, c, agent_rows, ego_rows, **kw), port_exchange(c, agent_rows, ego_rows, **kw)
        for k in ("n_other", "other", "other_lane"):
            assert wp.same_bits(got[k], want[k]), (off, k)
        assert (got["n_other"] >= 0).all() and (got["n_other"] <= 3).all()


@needs_gxx
def test_world_check_under_the_sanitizers(tmp_path):
    """The core on the seeded and hand-built cases as a program of its own, built with the address and undefined-behaviour
    sanitizers (on the CPU): its outputs are written to files the test compares with the port."""
    main = tmp_path / "main.cpp"
    main.write_text('#include <cstdio>\n#include <cstdlib>\n#include <vector>\n#include "' + SRC + '"\n' + r'''
template <class T> std::vector<T> rd(std::FILE* f, size_t n) { std::vector<T> v(n ? n : 1); if (n && std::fread(v.data(), sizeof(T), n, f) != n) std::abort(); return v; }
int main(int argc, char** argv) {
    std::FILE* f = std::fopen(argv[1], "rb");
    int h[9];
    if (!f || std::fread(h, sizeof(int), 9, f) != 9) return 2;
    const size_t W = h[0], B = h[1], N = h[2], G = h[3], A = h[4], K = h[5];
    auto n_world = rd<int>(f, W); auto off = rd<int>(f, W + 1); auto st = rd<double>(f, B * 6); auto ext = rd<double>(f, B);
    auto gp = rd<double>(f, B * G * 4); auto ng = rd<int>(f, B); auto lane = rd<int>(f, B * G); auto pre = rd<int>(f, B);
    auto ar = rd<double>(f, W * N * 4); auto er = rd<double>(f, B * 4);
    std::fclose(f);
    std::vector<double> actors(B * A * 4 + 1, 7.0), other(W * K * 5 + 1, 7.0);
    std::vector<int> n_act(B + 1, 7), okey(W * K + 1, 7), n_other(W + 1, 7), status(B + 1, 7);
    wc_exchange(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], n_world.data(), off.data(), st.data(), ext.data(), gp.data(), ng.data(),
                lane.data(), pre.data(), ar.data(), er.data(), actors.data(), n_act.data(), K ? other.data() : nullptr,
                K ? okey.data() : nullptr, K ? n_other.data() : nullptr, status.data());
    for (size_t b = 0; b < B; ++b) if (ng[b] > 0 && wc_match64(h[3], h[6], (int)b, st.data(), gp.data(), ng.data(), pre.data()) == -2) return 3;
    std::FILE* o = std::fopen(argv[2], "wb");
    std::fwrite(actors.data(), sizeof(double), B * A * 4, o); std::fwrite(n_act.data(), sizeof(int), B, o);
    std::fwrite(other.data(), sizeof(double), W * K * 5, o); std::fwrite(okey.data(), sizeof(int), W * K, o);
    std::fwrite(n_other.data(), sizeof(int), W, o); std::fwrite(status.data(), sizeof(int), B, o);
    std::fclose(o);
    return 0;
}
''')
    exe = str(tmp_path / "world_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(main), "-o", exe], check=True)
    cases = [(wp.seeded(s), dict(max_act=3, max_other=2, see_egos=s % 2, lane_window=4)) for s in range(3)]
    cases += [(c, dict(wp.SETTINGS, **st)) for c, st, _ in wp.hand_built().values()]
    bad = wp.seeded(8)
    bad["ego_off"] = np.array([2 ** 31 - 1, -7, 2, 99], np.int32)
    cases.append((bad, dict(max_act=64, max_other=0, see_egos=1, lane_window=2 ** 31 - 1)))
    for n, (c, kw) in enumerate(cases):
        W, N = c["agent_state"].shape[:2]
        B, G = c["global_path"].shape[:2]
        rng = np.random.default_rng(n)
        agent_rows, ego_rows = wp.rows_of(rng, (W, N)), wp.rows_of(rng, (B,))
        blob = np.array([W, B, N, G, kw["max_act"], kw["max_other"], kw["lane_window"], kw["see_egos"], 0], np.int32).tobytes()
        for k, dt in (("n_world", np.int32), ("ego_off", np.int32), ("ego_state", np.float64), ("ego_extent", np.float64),
                      ("global_path", np.float64), ("n_global", np.int32), ("ego_lane", np.int32), ("pre_match_index", np.int32)):
            blob += np.ascontiguousarray(c[k], dt).tobytes()
        blob += agent_rows.tobytes() + ego_rows.tobytes()
        (tmp_path / "in.bin").write_bytes(blob)
        run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, (n, run.stderr[-2000:])
        want = port_exchange(c, agent_rows, ego_rows, **kw)
        expect = b"".join(np.ascontiguousarray(want[k]).tobytes() for k in wp.OUT)
        assert (tmp_path / "out.bin").read_bytes() == expect, n


# ---- the launch plan and the argument rules -----------------------------------------------------------------------------------------
def plan(lib, *args):
    out = np.zeros(5, np.int32)
    err = lib.wc_plan(*args, out.ctypes.data)
    return out.tolist(), (err.decode() if err else None)


def test_launch_plan(lib):
    #            W, B, max_world, max_global, max_act, max_other, lane_window, see_egos
    assert plan(lib, 3, 5, 4, 80, 8, 4, 50, 0) == ([4, 64, 3, 1, 0], None)
    assert plan(lib, 512, 4096, 64, 80, 64, 64, 50, 1) == ([512 + 64, 64, 512, 64, 0], None)
    assert plan(lib, 1, 64, 1, 1, 1, 0, 0, 0)[0] == [2, 64, 1, 1, 0] and plan(lib, 1, 65, 1, 1, 1, 0, 0, 0)[0] == [3, 64, 1, 2, 0]
    for args in ((0, 5, 4, 80, 8, 4, 50, 0), (3, 0, 4, 80, 8, 4, 50, 0)):               # an empty batch launches nothing
        assert plan(lib, *args) == ([0, 0, 0, 0, 0], None)
    for args, word in (((-1, 5, 4, 80, 8, 4, 50, 0), "W < 0"), ((3, -1, 4, 80, 8, 4, 50, 0), "B < 0"), ((3, 5, 0, 80, 8, 4, 50, 0), "max_world"),
                       ((3, 5, 65, 80, 8, 4, 50, 0), "max_world"), ((3, 5, 4, 0, 8, 4, 50, 0), "max_global"), ((3, 5, 4, 80, 0, 4, 50, 0), "max_act"),
                       ((3, 5, 4, 80, 65, 4, 50, 0), "max_act"), ((3, 5, 4, 80, 8, -1, 50, 0), "max_other"), ((3, 5, 4, 80, 8, 65, 50, 0), "max_other"),
                       ((3, 5, 4, 80, 8, 4, -1, 0), "lane_window"), ((3, 5, 4, 80, 8, 4, 50, 2), "see_egos"), ((3, 5, 4, 80, 8, 4, 50, -1), "see_egos"),
                       ((0, 5, 4, 80, 65, 4, 50, 0), "max_act")):                        # sizes are refused before the empty batch is let through
        got, err = plan(lib, *args)
        assert got == [0, 0, 0, 0, 1] and word in err, (args, err)


def test_ego_offsets_rule(lib):
    def ok(off, W, B):
        a = np.array(off, np.int32)
        return lib.wc_ego_off(a.ctypes.data, W, B) is None
    assert ok([0, 0, 1, 4], 3, 5) and ok([0, 5], 1, 5) and ok([5, 5], 1, 5) and ok([0], 0, 5) and ok([2, 2, 2], 2, 2)
    assert not ok([0, 2, 1, 4], 3, 5) and not ok([-1, 0, 1, 4], 3, 5) and not ok([0, 0, 1, 6], 3, 5) and not ok([1], 0, 0)
    assert not ok([0, -2 ** 31, 1], 2, 5) and not ok([2 ** 31 - 1, 2 ** 31 - 1], 1, 5)


def test_the_two_clocks(lib):
    assert lib.wc_epoch(37, 37) is None and lib.wc_epoch(37, 0) is None and lib.wc_epoch(0, 0) is None
    for tick0, other in ((37, 38), (0, 1), (5, -1), (2 ** 40, 2 ** 40 + 1)):
        assert b"other_tick0" in lib.wc_epoch(tick0, other)

    def clock(K, T, dt, Ta, adt, atick0):
        ticks = np.zeros(4, np.int64)
        err = lib.wc_clock(K, T, dt, Ta, adt, atick0, ticks.ctypes.data, 4)
        return (err.decode() if err else None), ticks[:min(K, 4)].tolist()
    assert clock(3, 5, 0.01, 5, 0.01, 0) == (None, [0, 5, 10])
    assert clock(3, 5, 0.01, 2, 0.025, 37) == (None, [37, 39, 41])                    # dt_agent = 2.5 * vp.dt, T = 5, Ta = 2
    assert clock(2, 20, 0.01, 4, 0.05, 2 ** 31 - 1 - 8) == (None, [2 ** 31 - 9, 2 ** 31 - 5])
    assert clock(1, 5, 0.01, 1, 0.05 + 5e-10, 0)[0] is None                          # inside 1e-9
    for args, word in (((3, 5, 0.01, 5, 0.02, 0), "periods differ"), ((3, 5, 0.01, 4, 0.01, 0), "periods differ"),
                       ((1, 5, 0.01, 1, 0.05 + 3e-9, 0), "periods differ"), ((3, 5, float("nan"), 5, 0.01, 0), "periods differ"),
                       ((3, 5, 0.01, 0, 0.01, 0), "Ta < 1"), ((3, 5, 0.01, 5, 0.01, -1), "atick0"),
                       ((2, 20, 0.01, 4, 0.05, 2 ** 31 - 8), "INT32_MAX")):
        err, _ = clock(*args)
        assert err is not None and word in err, (args, err)
