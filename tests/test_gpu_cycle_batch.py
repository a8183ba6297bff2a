"""emp_plan_cycle (and the DP entry points it stands on) on ragged batches: per-scene n_ref and n_obs, every slot beyond them
poisoned (tests/cycle_ragged.py), several scenes with different counts in every wavefront.

- dp_plan / dp_enrich against oracle/exact.py, bit for bit, both DP modes and both edge forms;
- plan_cycle against oracle/ref_port.plan_cycle on each scene's valid slices alone: outcome, DP rows, lengths, path and
  trajectory (1e-6), both path-QP forms, with and without virtual obstacles; the wide lattice stage by stage;
- the padding does not matter: zero, NaN and hostile padding give the same bits, and so do the kernel forms that are
  bit-identical on full batches;
- batch invariance (host / device, reversed, shifted, each scene alone), the count contract behind guard rows, the front end
  on ragged global paths and plan_trajectory on the same batch.

tests/test_cycle_ragged_host.py checks on the oracles alone that these batches can tell a read past a count from none."""
import dataclasses

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from emplanner_carla_amd import api as A
from emplanner_carla_amd import scenes as S
from oracle import ref_port as op
from tests import batch_check as BC
from tests import cycle_ragged as R
from tests.conftest import assert_dp_l_vs_reference, assert_rel, make_planner

pytestmark = pytest.mark.gpu

RTOL = 1e-6
FIELDS = BC.CYCLE_OUTS
PADDED = (("dp_s", "dp_len"), ("dp_l", "dp_len"), ("path_s", "path_len"), ("path_l", "path_len"), ("traj", "traj_len"))
CFG5_CASE = (S.CFG5, range(70, 82), 14)          # 12 scenes of the 120 x 21 lattice: <16, 4> path QP, the wide Cartesian kernel


@pytest.fixture(scope="module")
def planner():
    pl = make_planner()
    yield pl
    pl.close()


class options:
    """Planner options for the length of a with-block."""

    def __init__(self, pl, **kw):
        self.pl, self.kw = pl, kw

    def __enter__(self):
        self.old = {k: self.pl.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            self.pl.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.pl.set_option(k, v)


def params(cfg):
    return A.dp_params_from_cfg(cfg), A.qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), A.smooth_params()


def plan(pl, cfg, inputs, **kw):
    p, q, sp = params(cfg)
    r = pl.plan_cycle(p, q, sp, **inputs, **kw)
    pl.synchronize()
    return {f: BC.to_np(getattr(r, f)) for f in FIELDS}


def planned(out):
    return (out["status"] & ~1) == 0


def up_to_lengths(out, refused_too=True):
    """The specified part of a cycle's outputs: status, dp_rows and the lengths of every scene, and the padded arrays up to their
    lengths (beyond: zeroed here) - of a refused scene as well (include/emplanner.h says what its lengths are).
    refused_too=False (the batch-invariance runs): for a scene the cycle refuses, status, dp_rows and the lengths only."""
    res = {f: np.array(out[f]) for f in FIELDS}
    ok = planned(out)
    for arr, ln in PADDED:
        a = res[arr]
        n = out[ln] if refused_too else np.where(ok, out[ln], 0)
        a[np.arange(a.shape[1])[None, :] >= n[:, None]] = 0.0
    return res


def assert_same_bits(a, b, what, fields=FIELDS):
    for f in fields:
        if BC.bits(a[f]) != BC.bits(b[f]):
            x, y = np.asarray(a[f]).reshape(len(a[f]), -1), np.asarray(b[f]).reshape(len(b[f]), -1)
            bad = np.nonzero([BC.bits(u) != BC.bits(v) for u, v in zip(x, y)])[0]
            raise AssertionError(f"{what}: {f} differs in scenes {bad[:8].tolist()} (status {a['status'][bad[:8]].tolist()} vs "
                                 f"{b['status'][bad[:8]].tolist()})")


# ---------------------------------------------------------------------------------------------------------------------
# the DP entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.EXACT_CASES))
def test_dp_plan_and_enrich_on_ragged_obstacles_with_hostile_padding(planner, case):
    """dp_rows, feasibility and the densified paths equal oracle/exact.py on the true counts bit for bit - with obstacles on
    each scene's own clean path right behind its count - in the two-kernel and the fused DP and in both edge forms; scenes on
    the n_obs == 0 bypass sit beside obstacle scenes in the same sweep tile."""
    cfg, seeds, seed = R.EXACT_CASES[case]
    r = R.ragged_batch(cfg, seeds, seed, "hostile")
    obs_s, obs_l, n_obs, start = r.dp_inputs()
    xrows, xfeas, xpaths = R.exact_dp(cfg, obs_s, obs_l, n_obs, start)
    assert np.array_equal(xrows, r.clean_rows)
    p = A.dp_params_from_cfg(cfg)
    M = A.max_path_points(p)
    per_tile = max(64 // cfg.row, 1)
    for edge_form in (0, 1):
        for mode in (L.EMP_DP_TWO_KERNEL, L.EMP_DP_FUSED):
            what = f"{cfg.name}, edge_form {edge_form}, mode {mode}"
            with options(planner, edge_form=edge_form):
                rows, _, status = planner.dp_plan(p, obs_s, obs_l, n_obs, start, mode=mode)
            bad = np.nonzero((rows != xrows).any(axis=1))[0]
            assert not len(bad), f"{what}: dp_rows of scenes {bad.tolist()} (n_obs {n_obs[bad].tolist()}) differ from the oracle"
            assert np.array_equal((status & 1) == 1, ~xfeas), what
            byp = np.nonzero(n_obs == 0)[0]
            assert (rows[byp] == (cfg.row + 1) / 2 - 1).all()
            if cfg.n_obs:
                mixed = [t for t in range(0, len(r), per_tile) if (n_obs[t:t + per_tile] == 0).any() and (n_obs[t:t + per_tile] > 0).any()]
                assert mixed, "no tile holds a bypass scene beside an obstacle scene"
            ps, pl_, ln, st = planner.dp_enrich(p, rows, start, M)
            assert (st == 0).all()
            for b in range(len(r)):
                xs, xl = xpaths[b]
                assert ln[b] == len(xs), f"{what}: scene {b} point count"
                assert np.array_equal(ps[b, :ln[b]], np.asarray(xs)) and np.array_equal(pl_[b, :ln[b]], np.asarray(xl)), \
                    f"{what}: densified path of scene {b}"


# ---------------------------------------------------------------------------------------------------------------------
# the cycle against the port
# ---------------------------------------------------------------------------------------------------------------------
def check_against_port(out, truth, what):
    stats = dict(planned=0, index=0, qp=0, smooth=0, short=0, headings=0)
    for i, t in enumerate(truth):
        w, st = f"{what}, scene {i}", int(out["status"][i])
        stats[t.outcome] += 1
        assert (t.outcome == "planned") == ((st & ~1) == 0), f"{w}: the port's outcome is {t.outcome}, status {st}"
        if t.outcome == "index":
            assert st & (2 | 4), f"{w}: the port raises IndexError, status {st}"
        if t.outcome == "qp":
            assert st & 8, f"{w}: the port's path QP is not optimal, status {st}"
        if "dp_rows" in t.out:
            assert bool(st & 1) == (not t.out["dp_feasible"]), f"{w}: DP feasibility"
            assert np.array_equal(out["dp_rows"][i], np.asarray(t.out["dp_rows"], dtype=np.float64)), f"{w}: dp_rows"
            k = len(t.out["dp_s"])                        # the DP path of refused scenes too: the start state behind it is
            assert out["dp_len"][i] == k, f"{w}: dp_len"   # projected on the last nodes before the count
            assert_rel(out["dp_s"][i, :k], np.asarray(t.out["dp_s"], dtype=np.float64), RTOL, f"{w} dp_s")
            assert_dp_l_vs_reference(out["dp_l"][i, :k], np.asarray(t.out["dp_l"], dtype=np.float64), f"{w} dp_l")
        if out["traj_len"][i] == 0:
            assert not (st & ~1) == 0
        if t.outcome != "planned":
            assert out["traj_len"][i] == 0, f"{w}: a refused scene has no trajectory"
            continue
        n, m = len(t.out["path_s"]), len(t.out["trajectory"])
        assert out["path_len"][i] == n and out["traj_len"][i] == m, f"{w}: lengths"
        stats["short"] += m <= 3
        assert_rel(out["path_s"][i, :n], np.asarray(t.out["path_s"]), RTOL, f"{w} path_s")
        assert_rel(out["path_l"][i, :n], np.asarray(t.out["path_l"]), RTOL, f"{w} path_l")
        want = np.asarray(t.out["trajectory"], dtype=np.float64)
        assert_rel(out["traj"][i, :m, :2], want[:, :2], RTOL, f"{w} x, y")
        # A two-point trajectory is the planning start twice (path_s[0] IS the start's s, path_l[0] its l; the next station lies
        # beyond a line that ends within 2 m): the port's own two points are 3e-14 m apart (measured, CFG2 scene 15 and default
        # scene 15) and its heading is atan2 of that rounding noise, 0 / 0 on the default lattice.  A heading is compared where
        # the points it is taken from are further apart than the 1e-6 their coordinates are compared to.
        if m > 2 or np.hypot(*(want[1, :2] - want[0, :2])) > RTOL * np.abs(want[:, :2]).max():
            assert_rel(out["traj"][i, :m, 2], want[:, 2], RTOL, f"{w} theta")
            assert_rel(out["traj"][i, 2:m, 3], want[2:, 3], RTOL, f"{w} kappa")
            stats["headings"] += 1
    return stats


@pytest.mark.parametrize("form", [0, 1], ids=["qp_rows", "qp_pair"])
@pytest.mark.parametrize("case", list(R.PORT_CASES))
def test_cycle_vs_port_on_each_scenes_valid_slices(planner, case, form):
    cfg, seeds, seed = R.PORT_CASES[case]
    r = R.ragged_batch(cfg, seeds, seed, "hostile")
    with options(planner, path_qp_form=form):
        out = plan(planner, cfg, r.cycle_inputs())
    stats = check_against_port(out, R.port_truth(cfg, seeds, seed), f"{cfg.name}, path_qp_form {form}")
    print(cfg.name, stats)
    assert stats["planned"] >= 0.6 * len(r) and stats["index"] >= 4 and (case == "limits34" or stats["short"] >= 1)
    assert stats["headings"] >= stats["planned"] - 1, "at most the one two-point trajectory goes without a heading check"


@pytest.mark.parametrize("form", [0, 1], ids=["qp_rows", "qp_pair"])
def test_cycle_vs_port_with_virtual_obstacles_behind_the_count(planner, form):
    """dyn_dis_speed for every other scene: the three virtual obstacles are appended at index n_obs[b], exactly where the
    hostile padding of obs_xy starts."""
    cfg, seeds, seed = R.PORT_CASES["cfg2"]
    r = R.ragged_batch(cfg, seeds, seed, "hostile")
    dyn = R.dyn_dis_speed(len(r), 7)
    with options(planner, path_qp_form=form):
        out = plan(planner, cfg, r.cycle_inputs(), dyn_dis_speed=dyn)
        plain = plan(planner, cfg, r.cycle_inputs())
    stats = check_against_port(out, R.port_truth(cfg, seeds, seed, 7), f"{cfg.name} + dyn, path_qp_form {form}")
    assert stats["planned"] >= 0.5 * len(r)
    none = np.isnan(dyn[:, 0])
    assert_same_bits({f: v[none] for f, v in out.items()}, {f: v[none] for f, v in plain.items()}, "scenes without a dynamic obstacle")


def test_cycle_on_the_wide_lattice_stage_by_stage(planner):
    """12 ragged CFG5 scenes: the DP against oracle/exact.py on the projected obstacles, the stages behind it against the port
    fed with the GPU's DP path (as test_full_cycle_on_the_wide_lattice_stage_by_stage, whose docstring says why)."""
    cfg, seeds, seed = CFG5_CASE
    r = R.ragged_batch(cfg, seeds, seed, "hostile")
    inp = r.cycle_inputs()
    out = plan(planner, cfg, inp)
    sm, os_, ol_, bsl, start = planner.frenet_project(**inp)
    live = np.nonzero(r.n_ref >= 1)[0]
    xrows, xfeas, xpaths = R.exact_dp(cfg, os_[live], ol_[live], r.n_obs[live], start[live])
    checked = 0
    for k, i in enumerate(live):
        w = f"scene {i} (n_ref {r.n_ref[i]}, n_obs {r.n_obs[i]})"
        assert np.array_equal(out["dp_rows"][i], xrows[k]), f"{w}: dp_rows"
        assert bool(out["status"][i] & 1) == (not xfeas[k]), w
        n = int(out["dp_len"][i])
        assert n == len(xpaths[k][0]) and np.array_equal(out["dp_l"][i, :n], np.asarray(xpaths[k][1])), f"{w}: DP path"
        ds, dl = list(out["dp_s"][i, :n:2]), list(out["dp_l"][i, :n:2])
        no, nr = int(r.n_obs[i]), int(r.n_ref[i])
        try:
            l_min, l_max = op.cal_lmin_lmax(ds, dl, list(os_[i, :no]), list(ol_[i, :no]), cfg.obs_length, cfg.obs_width)
        except IndexError:
            assert out["status"][i] & 4, w
            continue
        try:
            ql, _, _, status = op.Quadratic_planning(l_min, l_max, start[i, 1], start[i, 2], start[i, 3], _return_status=True)
        except np.linalg.LinAlgError:
            status = "diverged"
        if status == "diverged":
            assert out["status"][i] & 8, w
            continue
        if status != "optimal":
            # the dense oracle could not certify its own answer: no yardstick for the values.  A path the library did plan still
            # lies inside the port's bounds: its points are the stations' midpoints (and the two end stations), the QP's tolerance wide
            if not out["status"][i] & 8:
                lo, hi = np.asarray(l_min), np.asarray(l_max)
                lo = np.concatenate([lo[:1], (lo[1:] + lo[:-1]) / 2, lo[-1:]])
                hi = np.concatenate([hi[:1], (hi[1:] + hi[:-1]) / 2, hi[-1:]])
                m = len(lo)
                assert out["path_len"][i] == m, w
                assert (out["path_l"][i, 1:m] >= lo[1:] - 1e-6).all() and (out["path_l"][i, 1:m] <= hi[1:] + 1e-6).all(), w
            continue
        assert not out["status"][i] & (4 | 8 | 32), f"{w}: status {out['status'][i]}"
        path_s = [ds[0]] + [(ds[j] + ds[j - 1]) / 2 for j in range(1, len(ql))] + [ds[-1]]
        path_l = [ql[0]] + [(ql[j] + ql[j - 1]) / 2 for j in range(1, len(ql))] + [ql[-1]]
        m = len(path_s)
        assert out["path_len"][i] == m
        assert_rel(out["path_l"][i, :m], np.asarray(path_l), RTOL, f"{w} path l")
        try:
            want = np.asarray(op.frenet_2_x_y_theta_kappa(bsl[i, 0], bsl[i, 1], path_s, path_l, [tuple(x) for x in r.ref[i, :nr]],
                                                          list(sm[i, :nr])), dtype=np.float64)
        except IndexError:
            assert out["status"][i] & 2 and out["traj_len"][i] == 0, w
            continue
        t = len(want)
        assert (out["status"][i] & ~1) == 0 and out["traj_len"][i] == t, f"{w}: status {out['status'][i]}"
        assert_rel(out["traj"][i, :t, :3], want[:, :3], RTOL, f"{w} trajectory")
        assert_rel(out["traj"][i, 2:t, 3], want[2:, 3], RTOL, f"{w} curvature")
        checked += 1
    dead = np.nonzero(r.n_ref < 1)[0]
    assert len(dead) and (out["status"][dead] & 2).all() and (out["traj_len"][dead] == 0).all()
    assert checked >= 3


# ---------------------------------------------------------------------------------------------------------------------
# nothing beyond a count is read
# ---------------------------------------------------------------------------------------------------------------------
ALL_CASES = dict(R.PORT_CASES, cfg5=CFG5_CASE, cfg1=R.EXACT_CASES["cfg1"])


@pytest.mark.parametrize("case", list(ALL_CASES))
def test_poison_does_not_matter(planner, case):
    """Zero, NaN and hostile padding: the same bits in status, dp_rows and the lengths, and in the padded outputs up to their
    lengths - in the default form and in every form that is bit-identical to it on full batches."""
    cfg, seeds, seed = ALL_CASES[case]
    outs = {poison: up_to_lengths(plan(planner, cfg, R.ragged_batch(cfg, seeds, seed, poison).cycle_inputs())) for poison in R.POISONS}
    for poison in ("nan", "hostile"):
        assert_same_bits(outs[poison], outs["zero"], f"{cfg.name}: {poison} vs zero padding")
    hostile = R.ragged_batch(cfg, seeds, seed, "hostile").cycle_inputs()
    for name, kw, opt in (("cartesian_form", {}, dict(cartesian_form=1 - planner.get_option("cartesian_form"))),
                          ("edge_form", {}, dict(edge_form=1 - planner.get_option("edge_form"))),
                          ("fused DP", dict(mode=L.EMP_DP_FUSED), {})):
        with options(planner, **opt):
            other = up_to_lengths(plan(planner, cfg, hostile, **kw))
        assert_same_bits(other, outs["hostile"], f"{cfg.name}: {name} vs the default form")


@pytest.mark.parametrize("form", [0, 1], ids=["qp_rows", "qp_pair"])
def test_batch_invariance_on_the_hostile_batch(planner, form):
    cfg, seeds, seed = R.PORT_CASES["cfg2"]
    inp = R.ragged_batch(cfg, seeds, seed, "hostile").cycle_inputs()
    names = list(inp)
    p, q, sp = params(cfg)

    def call(args, device):
        r = planner.plan_cycle(p, q, sp, **dict(zip(names, args)))
        planner.synchronize()
        return up_to_lengths({f: BC.to_np(getattr(r, f)) for f in FIELDS}, refused_too=False)

    with options(planner, path_qp_form=form):
        full = BC.invariant(call, [inp[k] for k in names], f"plan_cycle, path_qp_form {form}")
    assert planned(full).sum() >= 14 and (~planned(full)).sum() >= 4


@pytest.mark.parametrize("case,mode", [("cfg2", L.EMP_DP_TWO_KERNEL), ("default", L.EMP_DP_TWO_KERNEL), ("default", L.EMP_DP_FUSED)],
                         ids=["cfg2", "default", "default_fused"])
def test_count_contract_behind_guard_rows(planner, case, mode):
    """n_ref and n_obs at capacity + 3 (a middle scene and the last scene) and at -1, on device tensors with a guard row before and
    after the batch: no guard row of an output is written, the other scenes keep their bits, the wild scenes equal the call with
    their counts clamped, and a B = 0 call writes nothing.  The input guard rows are hostile too (nodes on the last scene's start,
    an obstacle on its path), and three items past a row stay inside them.  On the default lattice the bypass row is 5.5: a scene
    with n_obs = -1 that ran the DP instead of taking the bypass cannot give the bits of n_obs = 0."""
    cfg, seeds, seed = R.PORT_CASES[case]
    r = R.ragged_batch(cfg, seeds, seed, "hostile")
    inp = r.cycle_inputs()
    p, q, sp = params(cfg)
    B, M = len(r), A.max_path_points(p)
    node = np.array([*r.batch.start_xy[-1], 1.0, 0.3])
    fills = dict(ref_line=np.tile(node, (cfg.n_ref, 1)), obs_xy=np.tile(r.obs_xy[-1, -1], (r.obs_xy.shape[1], 1)),
                 n_ref=cfg.n_ref, n_obs=r.obs_xy.shape[1])
    g = BC.GuardedCycle(planner, p, q, sp, inp, fills, M, mode=mode)
    clean = g.call()
    g.check_guards("plan_cycle clean")
    assert_same_bits(up_to_lengths(clean), up_to_lengths(plan(planner, cfg, inp, mode=mode)), "guarded call vs Planner.plan_cycle")
    mid, neg = B // 2, 3
    wild_ix = [mid, neg, B - 1]
    others = np.setdiff1d(np.arange(B), wild_ix)
    for cname, cap in (("n_ref", cfg.n_ref), ("n_obs", r.obs_xy.shape[1])):
        base = np.array(inp[cname], dtype=np.int32)
        wild = base.copy()
        wild[[mid, B - 1]] = cap + 3
        wild[neg] = -1
        g.set_count(cname, wild)
        got = g.call()
        g.check_guards(f"plan_cycle with {cname} wild")
        g.set_count(cname, np.clip(wild, 0, cap))
        clamped = g.call()
        g.set_count(cname, base)
        sel = lambda o, ix: {f: v[ix] for f, v in o.items()}
        assert_same_bits(sel(got, others), sel(clean, others), f"{cname} beyond the capacity changed another scene")
        assert_same_bits(sel(got, wild_ix), sel(clamped, wild_ix), f"wild {cname} vs the clamped count")
    g0 = BC.GuardedCycle(planner, p, q, sp, inp, fills, M, mode=mode, B=0)
    g0.call()
    g0.check_guards("plan_cycle with B = 0")


WIDE41 = S.LatticeConfig("wide_41", row=41, col=4, sample_s=5.7, sample_l=13.0 / 41, sampling_res=2, n_obs=5, n_ref=40)


@pytest.mark.parametrize("cfg", [S.CFG2, S.CFG_DEFAULT, S.CFG5, WIDE41], ids=lambda c: c.name)
def test_negative_n_obs_takes_the_bypass_in_every_dp_kernel(planner, cfg):
    """A count below 0 is clamped to 0, and 0 is the reference's no-obstacle bypass (path_planning.py:362-363): dp_plan with
    n_obs = -1 and -7 gives the bits of n_obs = 0 - the centre row, 5.5 and 20 on the even lattices - in the tiled sweep, the
    fused kernel and the wide sweep of lattices beyond 32 rows, beside scenes that run the DP."""
    b = S.make_batch(range(900, 912), cfg)
    p = A.dp_params_from_cfg(cfg)
    neg = np.array(b.n_obs, dtype=np.int32)
    neg[[1, 6]] = -1
    neg[10] = -7
    for mode in (L.EMP_DP_TWO_KERNEL, L.EMP_DP_FUSED):
        got = planner.dp_plan(p, b.sl_obs_s, b.sl_obs_l, neg, b.sl_start, mode=mode)
        want = planner.dp_plan(p, b.sl_obs_s, b.sl_obs_l, np.maximum(neg, 0), b.sl_start, mode=mode)
        for name, x, y in zip(("rows", "min_cost", "status"), got, want):
            assert BC.bits(x) == BC.bits(y), f"{cfg.name}, mode {mode}: {name} with a negative n_obs differs from n_obs = 0"
        assert (got[0][[1, 6, 10]] == (cfg.row + 1) / 2 - 1).all() and (got[0] != (cfg.row + 1) / 2 - 1).any()


# ---------------------------------------------------------------------------------------------------------------------
# the front end and the trajectory call on the same kind of batch
# ---------------------------------------------------------------------------------------------------------------------
def test_front_end_on_ragged_global_paths(planner):
    """The cycle from the global path with ragged n_global (some below the 51 nodes the front end needs, some cut inside the
    sampling window) and ragged n_obs: hostile padding behind both counts gives the bits of zeroed padding, and the fused call
    equals reference_line followed by plan_cycle."""
    G, at = 120, 20
    cfg = dataclasses.replace(S.CFG2, name="cfg2_global", n_ref=G)
    b = S.make_batch(range(800, 824), cfg, origin_index=at)
    B = len(b)
    rng = np.random.default_rng(31)
    n_global = rng.integers(at + 2, G + 1, B).astype(np.int32)
    n_global[[0, B - 1]] = G
    n_global[[2, 5]] = (40, 50)
    n_global[7:12] = rng.integers(80, G + 1, 5)
    _, n_obs = R.ragged_counts(cfg, B, 32)
    pre = np.full(B, at - 2, np.int32)
    p, q, sp = params(S.CFG2)
    M = A.max_path_points(p)

    def inputs(hostile):
        gp, obs = b.ref.copy(), b.obs_xy.copy()
        for i in range(B):
            gp[i, n_global[i]:] = (*b.start_xy[i], b.ref[i, at, 2] + 1.0, 0.3) if hostile else 0.0
            obs[i, n_obs[i]:] = b.ref[i, at + 9, :2] if hostile else 0.0        # on the centre line, 18 m ahead
        return gp, obs

    def fused(gp, obs):
        r = planner.plan_cycle(p, q, sp, None, None, max_pts=M, origin_xy=b.origin_xy, start_xy=b.start_xy, start_v=b.start_v,
                               start_a=b.start_a, obs_xy=obs, n_obs=n_obs, global_path=gp, n_global=n_global, pre_match_index=pre)
        planner.synchronize()
        out = {f: BC.to_np(getattr(r, f)) for f in FIELDS}
        return out, r.match_index, r.ref_status

    (h, hm, hs), (z, zm, zs) = fused(*inputs(True)), fused(*inputs(False))
    assert np.array_equal(hm, zm) and np.array_equal(hs, zs)
    assert_same_bits(up_to_lengths(h), up_to_lengths(z), "front end: hostile vs zeroed padding")
    assert (hs[n_global < 51] != 0).all() and (hs == 0).sum() >= 8 and planned(h)[hs == 0].sum() >= 5
    gp, obs = inputs(True)
    ref, n_ref, match, _, st_ref = planner.reference_line(sp, gp, n_global, b.start_xy, pre)
    two = planner.plan_cycle(p, q, sp, max_pts=M, ref_line=ref, n_ref=np.where(st_ref == 0, n_ref, 2).astype(np.int32),
                             origin_xy=b.origin_xy, start_xy=b.start_xy, start_v=b.start_v, start_a=b.start_a, obs_xy=obs, n_obs=n_obs)
    assert np.array_equal(match, hm) and np.array_equal(st_ref, hs)
    assert_same_bits(h, {f: BC.to_np(getattr(two, f)) for f in FIELDS}, "front end: one call vs two")


def test_plan_trajectory_on_the_ragged_hostile_batch(planner):
    """emp_plan_trajectory: the path fields are plan_cycle's bits, the speed half equals the chain of stand-alone calls."""
    from tests.test_gpu_trajectory import check_against_chain, dynamic_obstacles, speed_inputs
    cfg, seeds, seed = R.PORT_CASES["cfg2"]
    r = R.ragged_batch(cfg, seeds, seed, "hostile")
    cyc = r.cycle_inputs()
    dyn, n = dynamic_obstacles(r.batch, 5)
    p, q, sp = params(cfg)
    spd = speed_inputs(cyc, dyn, n, 5)
    res = planner.plan_cycle(p, q, sp, speed=spd, **cyc)
    ref = plan(planner, cfg, cyc)
    assert_same_bits({f: BC.to_np(getattr(res, f)) for f in FIELDS}, ref, "plan_trajectory vs plan_cycle")
    check_against_chain(planner, res, spd, A.max_path_points(p), cyc)
    assert (res.speed.speed_status == 0).any()
