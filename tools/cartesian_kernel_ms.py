"""The Cartesian tail alone (`to_cartesian`, HIP events around the launch, 4096 scenes) with one build of the library, in the four
shapes that reach its four kinds of kernel: configs[2] (rows <8, 3>), configs[4] (rows <16, 4>), configs[2] under cartesian_form = 1
(narrow) and a 66-column lattice planned with 134-point outputs (69 trajectory points: wide).  Ten timed cycles per shape behind two
untimed ones; one line per shape.  Usage: python tools/cartesian_kernel_ms.py LIB.so TAG (profiles/cartesian_body/README.md)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from emplanner_carla_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
tag = sys.argv[2]
from emplanner_carla_amd import scenes as S
from emplanner_carla_amd.api import Planner, dp_params_from_cfg, qp_params, smooth_params
WIDE = S.LatticeConfig("stations_67x5", row=5, col=66, sample_s=2.0, sample_l=1.0, sampling_res=1, n_obs=6, n_ref=77)
SHAPES = (("cfg2_rows_8x3", S.CFG2, 0, {}), ("cfg5_rows_16x4", S.CFG5, 0, {}), ("cfg2_narrow", S.CFG2, 1, {}),
          ("wide_69pts", WIDE, 0, {"max_pts": 134}))
pl = Planner(0)
for shape, cfg, form, extra in SHAPES:
    b = S.make_batch(range(4096), cfg, start_ahead=S.BENCH_START_AHEAD)
    d = dict(ref_line=b.ref, n_ref=np.full(b.ref.shape[0], b.ref.shape[1], np.int32), origin_xy=b.origin_xy, start_xy=b.start_xy,
             start_v=b.start_v, start_a=b.start_a, obs_xy=b.obs_xy, n_obs=b.n_obs.astype(np.int32))
    pl.set_option("cartesian_form", form)
    args = (dp_params_from_cfg(cfg), qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), smooth_params())
    for _ in range(2):
        r = pl.plan_cycle(*args, **d, **extra)
    pl.set_timing(True, only="to_cartesian")
    for _ in range(10):
        r = pl.plan_cycle(*args, **d, **extra)
    us = pl.kernel_samples("to_cartesian") * 1e3
    pl.set_timing(False)
    ok = float(((np.asarray(r.status) & ~1) == 0).mean())
    print(f"{tag} {os.path.basename(sys.argv[1])} {shape} to_cartesian_us median {np.median(us):.2f} min {us.min():.2f} max {us.max():.2f} n {len(us)} planned {ok:.3f} traj_pts {r.traj.shape[1]}", flush=True)
pl.set_option("cartesian_form", 0)
pl.close()
