"""What oracle/ref_port.py says about the cycle scenes of tests/lookup_cases.py, computed once per column count and shared by the
CPU and GPU suites: the port's plan_cycle per scene (None: it raises IndexError), with the conditions a scene must meet to test
anything asserted here - every lookup a tie, the labelled node separated from its neighbours, every obstacle's bound active."""
from __future__ import annotations

import functools
import math

import numpy as np

from emplanner_carla_amd import scenes as S
from oracle import ref_port as rp
from tests import lookup_cases as K

ACTIVE = 1e-3               # metres the port's path_l must move when an obstacle's index range moves by one station


def cfg_of(col):
    return S.LatticeConfig(f"lookup_{col}x5", row=5, col=col, sample_s=2.0, sample_l=1.0, sampling_res=1, n_obs=2, n_ref=2 * col + 8,
                           ref_ds=1.0, obs_length=K.CYCLE_OBS_LENGTH, obs_width=K.CYCLE_OBS_WIDTH)


def _port(cfg, inputs, b, **kw):
    n, k = inputs["n_ref"][b], inputs["n_obs"][b]
    dp = dict(sampling_res=cfg.sampling_res, row=cfg.row, col=cfg.col, sample_s=cfg.sample_s, sample_l=cfg.sample_l)
    return rp.plan_cycle(inputs["ref_line"][b, :n], inputs["origin_xy"][b], inputs["start_xy"][b], inputs["start_v"][b],
                         inputs["start_a"][b], inputs["obs_xy"][b, :k], dp_kwargs=dp, obs_length=cfg.obs_length,
                         obs_width=cfg.obs_width, verbose=False, **kw)


@functools.lru_cache(maxsize=None)
def cycle(col):
    cfg = cfg_of(col)
    specs = K.cycle_specs(col)
    inputs, labels = K.cycle_inputs(col)
    want = []
    for b, (s, lab) in enumerate(zip(specs, labels)):
        try:
            with np.errstate(all="ignore"):
                w = _port(cfg, inputs, b)
        except IndexError:
            w = None
        name = f"col {col} scene {b} ({s['kind']})"
        if s["status"] == 2:
            assert w is None, name
            want.append(None)
            continue
        if s["status"] == 4:
            assert w is None, name                        # cal_lmin_lmax raises
            want.append(None)
            continue
        assert w is not None, name
        if s["status"] == 8:
            assert w["qp_status"] != "optimal", name
            want.append(w)
            continue
        assert w["qp_status"] == "optimal" and w["smooth_status"] == "optimal" and len(w["trajectory"]) == s["points"], \
            (name, w["qp_status"], w["smooth_status"], len(w["trajectory"]))
        # every lookup a tie in bits: the s_map is i - origin, the start on its node, every kept path station on a knot
        n, p = s["n_ref"], s["p"]
        sm = np.asarray(w["s_map"])
        x = inputs["ref_line"][b, :n, 0]
        assert np.array_equal(sm, x - K.CYCLE_ORIGIN) and w["begin_s"] == p - K.CYCLE_ORIGIN and w["begin_l"] == 0.0, name
        kept = np.asarray(w["path_s"][:s["points"] - 1])
        assert np.isin(kept, sm).all() and (len(w["path_s"]) == s["points"] - 1 or w["path_s"][s["points"] - 1] > sm[-1]), name
        # separation: the labelled node (station on knot i + 1: node i; the start on node p: node p - 1) against its neighbours
        line = inputs["ref_line"][b, :n]
        for st, l in zip([w["begin_s"]] + list(kept), [w["begin_l"]] + list(w["path_l"][:len(kept)])):
            i = int(np.flatnonzero(sm == st)[0]) - 1
            assert i >= 0 and K.separation(line, sm, i, st, l) >= K.SEP, (name, st)
        # the port's target_xy is the labelled one
        t = np.array([q[:2] for q in w["target_xy"]])
        lab_xy = [K.offset(K.advance(line, sm, int(np.flatnonzero(sm == st)[0]) - 1, st), l)
                  for st, l in zip([w["begin_s"]] + list(kept), [w["begin_l"]] + list(w["path_l"][:len(kept)]))]
        assert np.abs(t - np.array(lab_xy)).max() <= 1e-12, name
        if lab is not None:
            # the obstacle's Frenet position is exact, its bound is the labelled range and that range is active in the QP's answer
            lo, hi, centre = lab
            if s["obs_k"] is not None:
                assert w["obs_s"][0] == w["begin_s"] + 2 * s["obs_k"] + 1 and w["obs_l"][0] == 5.0, (name, w["obs_s"], w["obs_l"])
                side, free, value = "l_max", 10.0, 5.0 - cfg.obs_width / 2
            else:                                         # on a node behind the start: l = 0 like dp_l[0], the l_min side
                assert w["obs_s"][0] == s["obs_node"] - K.CYCLE_ORIGIN and w["obs_l"][0] == 0.0 and 0.0 <= w["dp_l"][centre] < 1e-12, \
                    (name, w["dp_l"][centre])          # (the residue of the reference's inverse: see cycle_specs)
                side, free, value = "l_min", -10.0, cfg.obs_width / 2
            other = "l_min" if side == "l_max" else "l_max"
            bound = np.flatnonzero(np.asarray(w[side]) != free)
            assert np.array_equal(bound, np.arange(lo, hi + 1)) and (np.asarray(w[other]) == -free).all(), (name, bound)
            assert (np.asarray(w[side])[bound] == value).all(), name
            for shift in (-1, 1):
                if hi + shift >= len(w[side]):
                    continue                              # the moved range reaches n: it shows as EMP_ST_BOUND_INDEX, not in path_l
                moved_b = {side: np.full(len(w[side]), free), other: np.asarray(w[other])}
                moved_b[side][lo + shift:hi + shift + 1] = value
                ql, _, _, status = rp.Quadratic_planning(moved_b["l_min"], moved_b["l_max"], w["start_l"], w["start_dl"], w["start_ddl"],
                                                         _return_status=True)
                moved = np.abs(np.asarray(ql) - np.asarray(w["qp_l"])).max()
                assert status == "optimal" and moved > ACTIVE, (name, shift, status, moved)
        want.append(w)
    for v in inputs.values():
        v.setflags(write=False)
    return cfg, specs, inputs, labels, want
