"""Bit-identity of two builds of the library on whole planning cycles (development aid for changes that must not change a bit:
storage layouts, launch geometry): python tools/lib_equal.py A.so B.so [cfg2|cfg5|stationsNN] [scenes].  Each library plans the same scenes in
a child process of its own; every output array must be equal bit for bit (padding beyond each scene's length excluded).
Two more targets feed both libraries committed fixtures instead of planning cycles: `speed` (tests/golden/speed_backend.npz
through the speed planner's QP stage - the fixture holds that stage's inputs, not a scene for Planner.speed_plan) and
`control` (tests/golden/control/control.npz through mpc_lateral, mpc_ff_lateral and lqr_lateral).  `tail` runs the stand-alone
Frenet entry points (frenet_path_to_xy, frenet2cartesian, proj_point, match_projection, heading_kappa, smooth_line,
reference_line) on the ragged hostile batch of tests/cycle_ragged.py."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("dp_rows", "dp_s", "dp_l", "dp_len", "path_s", "path_l", "path_len", "traj", "traj_len", "status")


def fixture_child(name, out):
    """every output of the speed QP or of the three lateral controllers on the committed fixture"""
    from emplanner_carla_amd import api
    g = np.load(os.path.join(ROOT, "tests", "golden", "speed_backend.npz" if name == "speed" else os.path.join("control", "control.npz")))
    pl = api.Planner(0)
    res = {}
    if name == "speed":
        sel = np.nonzero(g["qp_code"] >= 0)[0]
        cs = g["cs_out"][sel]
        r = pl.speed_qp(api.speed_qp_params(), g["v0"][sel], g["qp_a0"][sel], g["dp_s"][sel], g["dp_t"][sel], cs[:, 0], cs[:, 1], cs[:, 2],
                        cs[:, 3])
        res = {f"speed_qp_{i}": np.asarray(a) for i, a in enumerate(r)}
    else:
        para = tuple(float(v) for v in g["vehicle_para"])
        args = (g["ff_path"], g["ff_n"].astype(np.int32), g["ff_state"], g["ff_Vx"], g["ff_min_index_in"].astype(np.int32))
        for law, prm, kw in (("mpc_lateral", api.mpc_params, dict(qp_matrices=True)), ("mpc_ff_lateral", api.mpc_ff_params, dict(qp_matrices=True)),
                             ("lqr_lateral", api.lqr_params, {})):
            r = getattr(pl, law)(prm(vehicle_para=para), *args, **kw)
            for k, v in vars(r).items():
                if isinstance(v, np.ndarray):
                    res[f"{law}_{k}"] = v
    pl.close()
    assert res, "no outputs"
    np.savez(out, **res)


def tail_child(out):
    """every output of the stand-alone entry points that share the Cartesian tail's helpers (emp_frenet_core.h point transform and
    centred difference, heading_kappa_lanes, find_match_one), on the ragged hostile batch of tests/cycle_ragged.py"""
    from emplanner_carla_amd import api
    from tests import cycle_ragged as CR
    cfg, seeds, seed = CR.EXACT_CASES["cfg2"]
    r = CR.ragged_batch(cfg, seeds, seed, "hostile")
    b, B, P = r.batch, len(r), r.ref.shape[1]
    rng = np.random.default_rng(7)
    pl = api.Planner(0)
    sp = api.smooth_params()
    res = {}

    def keep(name, outs):
        for i, a in enumerate(outs):
            res[f"{name}_{i}"] = np.array(a)

    sm = pl.s_map(r.ref, r.n_ref, b.origin_xy)
    # a path of M stations from each scene's planning start, 1.3 m apart: it runs past the end of the shorter lines
    M = 30
    n_pts = rng.integers(0, M + 1, B).astype(np.int32)
    n_pts[[0, B - 1]] = M
    path_s = b.sl_start[:, :1] + 0.4 + 1.3 * np.arange(M)[None, :]
    path_l = b.sl_start[:, 1:2] + 0.8 * np.sin(0.3 * np.arange(M)[None, :] + np.arange(B)[:, None])
    txy, n_out, st = pl.frenet_path_to_xy(r.ref, sm, r.n_ref, np.ascontiguousarray(b.sl_start[:, :2]), path_s, path_l, n_pts)
    keep("frenet_path_to_xy", (txy, n_out, st))
    sl = np.stack([path_s, path_l, 0.05 * np.cos(path_s), 0.01 * np.sin(path_s)], axis=2)
    for proj_only in (False, True):
        keep(f"frenet2cartesian_{int(proj_only)}", pl.frenet2cartesian(r.ref, sm, r.n_ref, sl, n_pts, proj_only=proj_only))
    keep("proj_point", pl.proj_point(r.ref, sm, r.n_ref, np.ascontiguousarray(path_s[:, 3]), np.zeros(B, np.int32)))
    keep("match_projection", pl.match_projection(r.ref, r.n_ref, r.obs_xy, r.n_obs))
    keep("heading_kappa", pl.heading_kappa(txy, n_out))
    for cap in (30, P):                         # row capacities of at most 32 points and of more: smooth_wave_kernel<false> / <true>
        keep(f"smooth_line_{cap}", pl.smooth_line(sp, np.ascontiguousarray(r.ref[:, :cap, :2]), np.minimum(r.n_ref, cap).astype(np.int32)))
    first = pl.reference_line(sp, r.ref, r.n_ref, b.start_xy, np.zeros(B, np.int32), is_first_run=np.ones(B, np.int32))
    keep("reference_line_first", first)
    pre = (np.asarray(first[2]) + np.where(np.arange(B) % 2 == 0, -2, 2)).clip(0, P - 1).astype(np.int32)   # windowed, both directions
    keep("reference_line_windowed", pl.reference_line(sp, r.ref, r.n_ref, b.start_xy, pre, is_first_run=np.zeros(B, np.int32)))
    pl.close()
    np.savez(out, **res)


def child(lib, cfg_name, scenes, out):
    sys.path.insert(0, ROOT)
    from emplanner_carla_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    if cfg_name in ("speed", "control"):
        return fixture_child(cfg_name, out)
    if cfg_name == "tail":
        return tail_child(out)
    from emplanner_carla_amd import scenes as S
    from emplanner_carla_amd.api import Planner, dp_params_from_cfg, qp_params, smooth_params
    extra = {}
    if cfg_name.startswith("stations"):     # stationsNN: a small lattice whose scenes have NN - 1 or NN path-QP stations, planned with
        st = int(cfg_name[8:])               # outputs of 2 NN points - the path QP's kernel is chosen by that capacity (27-34: <8, 4>)
        cfg = S.LatticeConfig(f"stations_{st}x5", row=5, col=st - 1, sample_s=2.0, sample_l=1.0, sampling_res=1, n_obs=6,
                              n_ref=max(61, st + 10))
        extra = {"max_pts": 2 * st}
    else:
        cfg = {"cfg2": S.CFG2, "cfg5": S.CFG5, "default": S.CFG_DEFAULT}[cfg_name]
    res = {}
    pl = Planner(0)
    for tag, kw in (("bench", dict(start_ahead=S.BENCH_START_AHEAD)), ("tight", dict(per_seed=S.survey_geometry_kwargs))):
        b = S.make_batch(range(scenes), cfg, **kw)
        B, P = b.ref.shape[:2]
        r = pl.plan_cycle(dp_params_from_cfg(cfg), qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), smooth_params(),
                          ref_line=b.ref, n_ref=np.full(B, P, np.int32), origin_xy=b.origin_xy, start_xy=b.start_xy, start_v=b.start_v,
                          start_a=b.start_a, obs_xy=b.obs_xy, n_obs=b.n_obs, **extra)
        for k in OUT:
            a = np.array(getattr(r, k))
            for arr, ln in (("dp_s", "dp_len"), ("dp_l", "dp_len"), ("path_s", "path_len"), ("path_l", "path_len"), ("traj", "traj_len")):
                if k == arr:
                    a[np.arange(a.shape[1])[None, :] >= np.asarray(getattr(r, ln))[:, None]] = 0.0
            res[f"{tag}_{k}"] = a
    pl.close()
    np.savez(out, **res)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
        sys.exit(0)
    a, b = sys.argv[1], sys.argv[2]
    pos = [x for x in sys.argv[3:] if not x.startswith("--")]
    cfg = pos[0] if len(pos) > 0 else "cfg2"
    n = int(pos[1]) if len(pos) > 1 else 4096
    outs = []
    for k, lib in enumerate((a, b)):
        out = f"/tmp/lib_equal_{k}.npz"
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, cfg, str(n), out], check=True)
        outs.append(np.load(out))
    bad = [k for k in outs[0].files if not np.array_equal(outs[0][k], outs[1][k], equal_nan=True)]
    if cfg in ("speed", "control", "tail"):
        what = "stand-alone entry points on the ragged hostile batch" if cfg == "tail" else "fixture"
        print(f"{cfg} {what}, {len(outs[0].files)} arrays: {'BIT-IDENTICAL' if not bad else 'DIFFERENT: ' + ', '.join(bad)} ({a} vs {b})")
        sys.exit(1 if bad else 0)
    ok = ((outs[0]["bench_status"] & ~1) == 0).mean()
    if "--diff" in sys.argv:            # builds that may differ by rounding (solver arithmetic): how far apart, scene statuses first
        for tag in ("bench", "tight"):
            sa, sb = outs[0][f"{tag}_status"], outs[1][f"{tag}_status"]
            both = ((sa & ~1) == 0) & ((sb & ~1) == 0)
            print(f"  {tag}: status differs on {(sa != sb).sum()} of {len(sa)} scenes; planned by both {both.sum()}")
            for k in ("dp_rows", "dp_s", "dp_l", "path_s", "path_l", "traj"):
                x, y = outs[0][f"{tag}_{k}"][both], outs[1][f"{tag}_{k}"][both]
                d = np.abs(x - y)
                print(f"    {k:8s} max |a-b| {d.max():.3e}   max |a-b| / max(|b|, 1) {(d / np.maximum(np.abs(y), 1.0)).max():.3e}")
    print(f"{cfg} {n} scenes x 2 geometries: {'BIT-IDENTICAL' if not bad else 'DIFFERENT: ' + ', '.join(bad)} ({a} vs {b}; planned {ok:.3f})")
    sys.exit(1 if bad else 0)
