"""emp_speed_qp (speed_qp_kernel<32>: two 32-lane scenes per wavefront, range_qp_solve_wave_fast) on the hard corridors of
tests/speed_qp_cases.py: standstill and v0 = 60, a0 on and outside [-6, 4], walls, speed caps, chased lower bounds, tubes down to
width 0, crossing bounds, 2 to 15 DP columns and the by-rule sizes 0, 1 and 16 - one ragged call, infeasible and by-rule scenes
spread between the feasible ones so that the two scenes of a wavefront differ, poison (crossed bounds or NaN) in every column the
reference never reads.  The yardstick is the dense formulation (oracle.st_backend.speed_qp at the nominal, widened and tightened
bounds: tests/speed_qp_cases.truth), checked on the CPU scalar build by tests/test_speed_qp_cases_host.py.

Measured on the MI355X, kernel | CPU scalar build (speed_qp_solve_scalar, tests/host_check: the same interior point with its own
stop-rule clauses and summation order).  Labels: 174 feasible, 62 infeasible, 42 borderline (15 %), 6 by rule; borderline cases
reported solved: 29 | 29.  Worst deviation from the oracle over s, s_dot, s_dot2 and the feasible cases of a family (m, m/s, m/s^2):
    open 1.5e-9 | 1.5e-9    wall 2.1e-10 | 3.6e-10    cap 1.2e-9 | 1.3e-9    chase 3.4e-10 | 3.4e-10    sandwich 3.1e-10 | 2.6e-10
    tube 7.7e-13 | 4.2e-13    huge 3.2e-11 | 2.6e-11    (the largest at 15 columns, where s reaches hundreds of metres)
Most iterations on a solved scene:
    open 19 | 19    wall 23 | 24    cap 15 | 14    chase 14 | 14    sandwich 15 | 15    tube 20 | 20    halt 13 | 13    huge 12 | 12
Failed scenes: the kernel reports iters = 0 for every scene it fails (asserted below), so their cost is not visible through the
call; the scalar build gives up after at most open 16, wall 16, cap 25, chase 16, cross 18 iterations.  The kernel passes
iter_cap = 1000 to range_qp_solve_wave_fast, but qp_stop_rule ends at kQpMaxIter = 60 whatever the cap says: no scene, solved or
failed, can run 1000 passes, none reported more than 23, none reached 60.  No decided infeasible case came back solved.
Non-finite inputs: status 8, NaN outputs, iters 0 | 0 for all six kinds (mu is NaN at the first stop test).

Non-finite inputs, batch invariance and the stages downstream of a standstill (increase_points, path_speed_merge on a profile
whose s plateaus) follow the case-set test."""
import collections
import functools

import numpy as np
import pytest

from emplanner_carla_amd import api as A
from oracle import st_backend as be
from tests import speed_qp_cases as F
from tests.batch_check import bits, invariant, to_np
from tests.conftest import assert_rel, make_planner
from tests.test_gpu_speed_backend_batch import _code
from tests.test_speed_qp_cases_host import NONFINITE, nonfinite

pytestmark = pytest.mark.gpu

RTOL = 1e-6                       # the bar of test_speed_qp_batch
MAX_ITER = 60                     # kQpMaxIter: qp_stop_rule ends at it whatever iter_cap the kernel passes (1000)
QP = ("qp_s", "qp_s_dot", "qp_s_dot2", "relative_time", "iters", "status")
BY_RULE = {0: A.STB_NO_PROFILE, 1: A.STB_QP_FAILED, 16: A.STB_INDEX}
NAN = np.nan


@pytest.fixture(scope="module")
def planner():
    pl = make_planner()
    yield pl
    pl.close()


def run(pl, args):
    return dict(zip(QP, (to_np(o) for o in pl.speed_qp(A.speed_qp_params(), *args))))


def batch_names():
    """Every case, the ones that fail (infeasible, by rule) spread evenly between the ones that solve or may solve; an odd count,
    so that the last wavefront holds one scene."""
    fails = lambda n: F.truth(n)[0] in ("infeasible", "rule")
    names = list(F.cases())
    good, bad = [n for n in names if not fails(n)], [n for n in names if fails(n)]
    step = max(1, len(good) // len(bad))
    out = []
    for i, name in enumerate(good):
        out.append(name)
        if i % step == step - 1 and bad:
            out.append(bad.pop(0))
    out += bad
    if len(out) % 2 == 0:
        out.append(out[len(out) // 2])
    return out


def consistent(r, b, k):
    """A scene's outputs match its own status: solved with finite values on stations 0 .. k-1 and NaN behind, or failed with NaN
    everywhere and no iterations reported."""
    got = np.stack([r[c][b] for c in QP[:4]])
    if r["status"][b] == 0:
        return bool(np.isfinite(got[:, :k]).all() and np.isnan(got[:, k:]).all() and r["iters"][b] > 0)
    return bool(np.isnan(got).all() and r["iters"][b] == 0)


def check_solved_scene(r, b, c):
    """What holds for every scene reported solved, with or without an oracle: the time grid, the NaN tail, every used bound and
    the monotonicity of s within 1e-6 max(1, |bound|)."""
    k, dt = c.k, c.dp_t[c.k - 1] / (c.k - 1)
    assert consistent(r, b, k), f"{c.name}: outputs do not match status 0"
    np.testing.assert_array_equal(r["relative_time"][b, :k], np.arange(k) * dt, err_msg=c.name)
    assert 0 < r["iters"][b] <= MAX_ITER, f"{c.name}: {r['iters'][b]} iterations"
    s, v, a = (r[q][b, :k] for q in QP[:3])
    assert max(abs(s[0]), abs(v[0] - c.v0), abs(a[0] - c.a0)) <= 1e-9 * max(1.0, c.v0), f"{c.name}: the pinned start"
    slack = lambda bound: RTOL * np.maximum(1.0, np.abs(np.where(np.isfinite(bound), bound, 1.0)))
    n = k - 1
    for what, x, lo, hi in (("s", s[1:], c.s_lb[:n], c.s_ub[:n]), ("s_dot", v[1:], c.sd_lb[:n], c.sd_ub[:n]),
                            ("s_dot2", a[1:], np.full(n, F.A_MIN), np.full(n, F.A_MAX))):
        assert (x >= lo - slack(lo)).all() and (x <= hi + slack(hi)).all(), f"{c.name}: {what} leaves its bounds"
    assert (np.diff(s) >= -RTOL * np.maximum(1.0, np.abs(s[1:]))).all(), f"{c.name}: s decreases"


def test_speed_qp_on_the_case_set(planner):
    names = batch_names()
    B = len(names)
    assert B % 2 == 1 and B >= len(F.cases())
    r = run(planner, F.arrays(names))
    dev, most = collections.defaultdict(float), collections.defaultdict(int)
    tally, borderline_solved = collections.Counter(), 0
    differ = sum(F.truth(names[b])[0] != F.truth(names[b + 1])[0] for b in range(0, B - 1, 2))
    for b, name in enumerate(names):
        c = F.cases()[name]
        label, x = F.truth(name)
        st, it = int(r["status"][b]), int(r["iters"][b])
        tally[label] += 1
        if label == "rule":
            assert st == BY_RULE[c.k] and consistent(r, b, 0), f"{name}: status {st}"
            continue
        assert st in (0, A.STB_QP_FAILED) and consistent(r, b, c.k), f"{name}: status {st}, {it} iterations, outputs do not match"
        if label == "infeasible":
            assert st == A.STB_QP_FAILED, f"{name}: infeasible, reported solved after {it} iterations"
            continue
        if label == "feasible":
            assert st == 0, f"{name}: feasible, status {st}"
        if st != 0:
            continue
        check_solved_scene(r, b, c)
        most[c.family] = max(most[c.family], it)
        if label == "borderline":
            borderline_solved += names.index(name) == b          # (the scene that makes the count odd is a second copy)
            continue
        got = np.stack([r[q][b, :c.k] for q in QP[:3]], axis=1)
        dev[c.family] = max(dev[c.family], float(np.abs(got - x).max()))
        for j, what in enumerate(QP[:3]):
            assert_rel(got[:, j], x[:, j], RTOL, f"{name}: {what}")
        if c.family == "huge":                            # clamped at kSpeedBig: the open corridor's answer, bit for bit
            twin = names.index(f"open_a0_v{c.v0:g}_k{c.k}")
            assert all(bits(r[q][b]) == bits(r[q][twin]) for q in QP[:5]), f"{name}: differs from the open corridor"
    n_borderline = sum(F.truth(n)[0] == "borderline" for n in set(names))
    print(f"{B} scenes, labels {dict(tally)}, {differ} of {B // 2} wavefronts pair two labels; borderline cases solved: "
          f"{borderline_solved} of {n_borderline}")
    print("worst deviation from the oracle per family: " + ", ".join(f"{f} {d:.1e}" for f, d in dev.items()))
    print("most iterations on solved scenes per family: " + ", ".join(f"{f} {i}" for f, i in most.items()))
    at_cap = [names[b] for b in range(B) if r["iters"][b] >= MAX_ITER]
    print(f"scenes at the cap of {MAX_ITER} iterations: {at_cap}")
    assert differ >= B // 6 and tally["feasible"] >= 150 and tally["infeasible"] >= 50


@functools.lru_cache(maxsize=None)
def invariant_names():
    """65 cases: round-robin over (family, label), so that every family and every label of every family is there."""
    groups = collections.defaultdict(list)
    for n, c in F.cases().items():
        groups[c.family, F.truth(n)[0]].append(n)
    groups["rule", "rule"].sort(key=lambda n: (F.cases()[n].v0, F.cases()[n].k))         # 0, 1 and 16 columns first
    out, depth = [], 0
    while len(out) < 65:
        out += [g[depth] for g in groups.values() if depth < len(g)]
        depth += 1
    return tuple(out[:65])


def test_speed_qp_batch_independence(planner):
    """Bit for bit the same alone, reversed, shifted by one and on the device path: hard, infeasible and by-rule scenes beside easy
    ones in the wavefront.  No oracle here."""
    names = invariant_names()
    cs = [F.cases()[n] for n in names]
    assert {c.family for c in cs} == set(F.FAMILIES) | {"rule"}
    assert {F.truth(n)[0] for n in names} == {"feasible", "infeasible", "borderline", "rule"}
    calls = []
    full = invariant(lambda a, dev: calls.append(dev) or run(planner, a), F.arrays(names), "emp_speed_qp")
    assert len(calls) == len(names) + 4 and sum(calls) == 1          # the batch, on the device, reversed, shifted, each scene alone
    st = full["status"]
    assert (st == 0).sum() >= 25 and (st == A.STB_QP_FAILED).sum() >= 15
    assert set(st.tolist()) == {0, A.STB_QP_FAILED, A.STB_NO_PROFILE, A.STB_INDEX}


def open_name(k):
    return f"open_a0_v{F.V0S[F.SIZES.index(k) % 5]:g}_k{k}"


def test_speed_qp_refuses_non_finite_inputs(planner):
    """One scene of a wavefront with a non-finite input: all four bound arrays NaN (what a raised convex space hands over beside a
    valid DP profile), one used s_lb or s_dot_ub NaN, v0 NaN or +inf, dp_t[k-1] NaN.  It fails with NaN outputs and every other
    scene of the call is bit-identical to the call with the open corridor in that slot.  No oracle: there is no such problem."""
    base, bad = [], {}
    for i, kind in enumerate(NONFINITE):
        for j, k in enumerate((2, 5, 15)):
            name, partner = open_name(k), open_name((15, 2, 5)[j])
            pair = [name, partner] if (i + j) % 2 == 0 else [partner, name]       # the bad scene in either half of the wavefront
            bad[len(base) + pair.index(name)] = kind
            base += pair
    fields = ("v0", "a0", "dp_s", "dp_t", "s_lb", "s_ub", "sd_lb", "sd_ub")
    clean = F.arrays(base)
    dirty = [x.copy() for x in clean]
    for b, kind in bad.items():
        for f, value in nonfinite(F.cases()[base[b]], kind).items():
            dirty[fields.index(f)][b] = value
    want, got = run(planner, clean), run(planner, dirty)
    assert (want["status"] == 0).all()
    iters = collections.defaultdict(int)
    for b, name in enumerate(base):
        if b in bad:
            st = got["status"][b]
            iters[bad[b]] = max(iters[bad[b]], int(got["iters"][b]))
            assert st == A.STB_QP_FAILED and all(np.isnan(got[q][b]).all() for q in QP[:4]), \
                f"{bad[b]} in {name} (scene {b}): status {st}, {got['iters'][b]} iterations"
        else:
            assert all(bits(got[q][b]) == bits(want[q][b]) for q in QP), f"{name} (scene {b}) changes beside a non-finite scene"
    print(f"iterations reported for the non-finite scenes: {dict(iters)}")


DENSE = ("s", "s_dot", "s_dot2", "relative_time", "status")


def test_downstream_of_a_standstill(planner):
    """increase_points and path_speed_merge on the kernel's own profiles of the wall and halt cases: s_dot reaches 0, s plateaus
    (tests/test_gpu_speed_backend_batch.py's profiles keep v >= 0.2, so s always rises strictly there)."""
    names = F.names_of("wall") + F.names_of("halt")
    q = run(planner, F.arrays(names))
    keep = np.nonzero(q["status"] == 0)[0]
    names = [names[b] for b in keep]
    prof = [np.ascontiguousarray(q[c][keep]) for c in QP[:4]]
    B = len(names)
    still = [b for b in range(B) if np.nanmin(prof[1][b]) < 1e-6]
    flat = [b for b in range(B) if (np.abs(np.diff(prof[0][b, :F.cases()[names[b]].k])) < 1e-6).any()]
    print(f"{B} solved wall and halt profiles, {len(still)} reach s_dot < 1e-6, {len(flat)} hold a step of s below 1e-6 m")
    assert B >= 40 and len(still) >= 12 and len(flat) >= 12
    d = dict(zip(DENSE, (to_np(o) for o in planner.speed_increase_points(*prof))))
    for b in range(B):
        want = np.stack(be.port_increase_points(*(p[b] for p in prof)))
        assert d["status"][b] == 0, f"{names[b]}: status {d['status'][b]}"
        assert bits(d["relative_time"][b]) == bits(want[3]), f"sample times of {names[b]}"
        got = np.stack([d[c][b] for c in DENSE[:3]])
        assert np.array_equal(np.isnan(got), np.isnan(want[:3])), f"NaN pattern of {names[b]}"
        fin = ~np.isnan(want[:3])
        assert_rel(got[fin], want[:3][fin], 1e-12, f"samples of {names[b]}", scale=1.0)
    W, n_valid = 81, 80                                                  # a straight path of 80 points, 2 m apart, NaN behind
    ps = np.tile(2.0 * np.arange(W), (B, 1))
    px, py = ps * np.cos(0.3), ps * np.sin(0.3)
    ph, pk = np.full((B, W), 0.3), np.zeros((B, W))
    for x in (px, py, ph, pk):
        x[:, n_valid:] = NAN
    now = np.linspace(0.0, 50.0, B)
    n_init = np.full(B, W, np.int32)
    dense = [d[c] for c in DENSE[:4]]
    traj, st = (to_np(o) for o in planner.path_speed_merge(*dense, now, ps, px, py, ph, pk, n_init))
    for b in range(B):
        want, code = _code(be.port_path_speed_merge, *(x[b] for x in dense), float(now[b]), ps[b], px[b], py[b], ph[b], pk[b])
        assert st[b] == code, f"{names[b]}: status {st[b]}, the port {code}"
        if code == 0:
            assert bits(traj[b]) == bits(np.stack(want)), f"merge of {names[b]} (bit-exact expected)"
