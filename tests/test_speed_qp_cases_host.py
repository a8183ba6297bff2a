"""The corridors of tests/speed_qp_cases.py are what they say they are (no GPU): every size, family and start speed is there, the
columns the reference never reads are poisoned, the dense oracle's label agrees with what the construction decides on its own, and
the scalar build of the speed QP (speed_qp_solve_scalar through tests/host_check) agrees with the oracle in status and values.
What tests/test_gpu_speed_qp_cases.py then asks of speed_qp_kernel is asked of the scalar code first."""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import host_check
from tests import speed_qp_cases as F
from tests.conftest import assert_rel

RTOL = 1e-6                # the bar of test_speed_qp_batch
MAX_ITER = 60              # kQpMaxIter of emp_qp_core.h
ST_QP_FAILED = 8           # kStbQpFailed
BY_RULE = {0: 64, 1: 8, 16: 4}         # kStbNoProfile, kStbQpFailed (dt = T / 0), kStbIndex


@pytest.fixture(scope="module")
def hc():
    return host_check.load()


def solve(hc, c, **changed):
    """speed_qp_solve_scalar on case c (fields replaced by ``changed``) -> status, [17][3] s, s_dot, s_dot2, relative_time, iters."""
    get = lambda f: np.ascontiguousarray(changed.get(f, getattr(c, f)), dtype=np.float64)
    ins = [get(f) for f in ("dp_s", "dp_t", "s_lb", "s_ub", "sd_lb", "sd_ub")]
    outs = [np.zeros(17) for _ in range(4)]
    it = C.c_int(-1)
    st = hc.hc_stb_speed_qp(ins[0].ctypes.data, ins[1].ctypes.data, float(changed.get("v0", c.v0)), float(changed.get("a0", c.a0)),
                            *[a.ctypes.data for a in ins[2:]], F.W4.ctypes.data, *[o.ctypes.data for o in outs], C.byref(it))
    return st, np.stack(outs[:3], axis=1), outs[3], it.value


def test_the_case_set_covers_what_it_names():
    cs = F.cases()
    assert 250 <= len(cs) <= 320
    assert {c.k for c in cs.values()} == set(F.SIZES) | set(F.RULE_SIZES)
    assert {c.family for c in cs.values()} == set(F.FAMILIES) | {"rule"}
    assert {c.v0 for c in cs.values()} == set(F.V0S)
    for k in F.SIZES:
        assert {c.family for c in cs.values() if c.k == k} == set(F.FAMILIES), k
        assert {c.v0 for c in cs.values() if c.k == k} == set(F.V0S), k
    for fam in F.FAMILIES:
        assert {c.k for c in cs.values() if c.family == fam} == set(F.SIZES), fam
        assert fam == "halt" or len({c.v0 for c in cs.values() if c.family == fam}) >= 4, fam
    assert {c.a0 for c in cs.values() if c.family == "open"} == set(F.OPEN_A0)
    crossed = nan = 0
    for c in cs.values():
        k, n = c.k, F.used(c.k)
        bounds = (c.s_lb, c.s_ub, c.sd_lb, c.sd_ub)
        assert all(len(x) == F.N_DP for x in bounds + (c.dp_s, c.dp_t))
        np.testing.assert_array_equal(c.dp_t[:k], 0.5 * (np.arange(k) + 1.0))
        assert np.isnan(c.dp_t[k:]).all() and np.isnan(c.dp_s[k:]).all() and np.isfinite(c.dp_s[:k]).all(), c.name
        assert not any(np.isnan(x[:n]).any() for x in bounds) and (c.sd_lb[:n] == 0.0).all(), c.name
        if np.isnan(c.s_lb[n:]).all():                   # the columns behind the used ones: NaN, or crossed bounds
            assert all(np.isnan(x[n:]).all() for x in bounds), c.name
            nan += 1
        else:
            assert (c.s_lb[n:] > c.s_ub[n:]).all() and (c.sd_lb[n:] > c.sd_ub[n:]).all(), c.name
            crossed += 1
        if c.k in F.RULE_SIZES:
            continue
        t = F.times(k)
        assert abs(F.dt_of(k) - c.dp_t[k - 1] / (k - 1)) < 1e-15 and F.dt_of(k) != 0.5
        if c.family in ("open", "halt", "wall", "cap"):
            assert (c.s_lb[:n] == -np.inf).all()
        if c.family == "wall":
            w = F.wall_column(k)
            assert 0 <= w < n and (c.s_ub[:w] == np.inf).all() and (c.s_ub[w:n] == c.s_ub[w]).all() and 0.5 <= c.s_ub[w] < np.inf
        if c.family == "cross":
            g = c.s_lb[:n] - c.s_ub[:n]
            assert (g > 0).sum() == 1 and g[F.cross_column(k)] > 0
        if c.family == "halt":
            assert c.v0 == 0.0 and c.s_ub[n - 1] == 0.0
        if c.family == "huge":
            assert (c.s_ub[:n] == F.HUGE).all() and (c.s_lb[:n] == -F.HUGE).all() and (c.sd_ub[:n] == F.HUGE).all()
            assert f"open_a0_v{c.v0:g}_k{k}" in cs, c.name
        if c.family in ("tube", "sandwich"):
            np.testing.assert_allclose((c.s_lb[:n] + c.s_ub[:n]) / 2.0, c.v0 * t, rtol=0, atol=1e-12)
        if c.family in ("tube", "halt") and "w0.02" not in c.name:
            assert c.design == "borderline", c.name
    assert crossed >= 100 and nan >= 100
    assert cs["open_a-6_v0_k2"].design == "infeasible" and cs["open_a-6_v0_k15"].design == "infeasible"   # by dynamics
    assert all(cs[n].design == "infeasible" for n in F.names_of("cross") if "g0.001" in n)               # by inspection
    assert all(cs[n].design == "infeasible" for n in F.names_of("chase") if "g6" in n)                    # needs s_dot2 > 4


def test_the_oracle_agrees_with_the_design():
    """Where the construction decides, the oracle's label is the design.  At most 5 % of those cases may come out borderline; no
    family and no size loses all its decided cases; every size has a feasible and an infeasible case."""
    cs = F.cases()
    decided = [c for c in cs.values() if c.family in F.DECIDED_BY_DESIGN and c.design != "borderline"]
    assert len(decided) >= 0.85 * sum(c.family in F.DECIDED_BY_DESIGN for c in cs.values())
    blurred = 0
    kept_family, kept_size, labels = collections.Counter(), collections.Counter(), collections.defaultdict(set)
    for c in cs.values():
        label = F.truth(c.name)[0]
        labels[c.k].add(label)
        if c not in decided:
            continue
        if label == "borderline":
            blurred += 1
            continue
        assert label == c.design, f"{c.name}: built {c.design}, the oracle says {label}"
        kept_family[c.family] += 1
        kept_size[c.k] += 1
    tally = collections.Counter(F.truth(n)[0] for n in cs)
    print(f"labels: {dict(tally)}; decided by design {len(decided)}, of which the oracle calls {blurred} borderline")
    assert blurred <= 0.05 * len(decided)
    assert all(kept_family[f] >= 1 for f in F.DECIDED_BY_DESIGN) and all(kept_size[k] >= 1 for k in F.SIZES)
    for k in F.SIZES:
        assert {"feasible", "infeasible"} <= labels[k], k
    for k in F.RULE_SIZES:
        assert labels[k] == {"rule"}


@pytest.mark.parametrize("k", F.SIZES + F.RULE_SIZES)
def test_scalar_solver_against_the_labels(hc, k):
    worst, most = collections.defaultdict(float), collections.defaultdict(int)
    for c in (c for c in F.cases().values() if c.k == k):
        label, x = F.truth(c.name)
        st, got, rel_t, iters = solve(hc, c)
        failed_clean = st == ST_QP_FAILED and np.isnan(got).all() and np.isnan(rel_t).all()
        if label == "rule":
            assert st == BY_RULE[k] and np.isnan(got).all() and iters == 0, f"{c.name}: status {st}"
            continue
        if label == "infeasible":
            assert failed_clean, f"{c.name}: infeasible, status {st} after {iters} iterations"
            most[c.family, "failed"] = max(most[c.family, "failed"], iters)
            continue
        solved_clean = st == 0 and np.isfinite(got[:k]).all() and np.isnan(got[k:]).all()
        if label == "borderline":
            assert failed_clean or solved_clean, f"{c.name}: status {st} with outputs that do not match it"
            most[c.family, "solved" if st == 0 else "failed"] = max(most[c.family, "solved" if st == 0 else "failed"], iters)
            continue
        assert solved_clean and 0 < iters <= MAX_ITER, f"{c.name}: feasible, status {st} after {iters} iterations"
        np.testing.assert_array_equal(rel_t[:k], np.arange(k) * (c.dp_t[k - 1] / (k - 1)))
        for j, what in enumerate(("qp_s", "qp_s_dot", "qp_s_dot2")):
            assert_rel(got[:k, j], x[:, j], RTOL, f"{c.name}: {what}")
        worst[c.family] = max(worst[c.family], float(np.abs(got[:k] - x).max()))
        most[c.family, "solved"] = max(most[c.family, "solved"], iters)
        if c.family == "huge":                            # clamped at kSpeedBig: the open corridor's answer, bit for bit
            twin = F.cases()[f"open_a0_v{c.v0:g}_k{k}"]
            assert solve(hc, twin)[1].tobytes() == got.tobytes(), c.name
    print(f"k = {k}: worst deviation per family {dict(worst)}; most iterations {dict(most)}")


NONFINITE = ("all_bounds", "s_lb", "sd_ub", "v0_nan", "v0_inf", "dp_t")


def nonfinite(c, kind):
    """Case c with one non-finite input, as keyword arguments for ``solve`` (and for the GPU test's batch rows)."""
    nan16 = np.full(F.N_DP, np.nan)
    col = (c.k - 1) // 2
    one = lambda a: np.where(np.arange(F.N_DP) == col, np.nan, a)
    dp_t = c.dp_t.copy()
    dp_t[c.k - 1] = np.nan
    return {"all_bounds": dict(s_lb=nan16, s_ub=nan16, sd_lb=nan16, sd_ub=nan16), "s_lb": dict(s_lb=one(c.s_lb)),
            "sd_ub": dict(sd_ub=one(c.sd_ub)), "v0_nan": dict(v0=np.nan), "v0_inf": dict(v0=np.inf), "dp_t": dict(dp_t=dp_t)}[kind]


@pytest.mark.parametrize("kind", NONFINITE)
def test_scalar_solver_refuses_non_finite_inputs(hc, kind):
    """A raised convex space hands all-NaN bounds to the QP beside a valid DP profile; ``lo > hi + 1e-9`` is false for NaN."""
    for k in (2, 5, 15):
        c = F.cases()[f"open_a0_v{F.V0S[F.SIZES.index(k) % 5]:g}_k{k}"]
        assert F.truth(c.name)[0] == "feasible" and solve(hc, c)[0] == 0
        st, got, rel_t, iters = solve(hc, c, **nonfinite(c, kind))
        print(f"{kind}, k = {k}: status {st} after {iters} iterations")
        assert st == ST_QP_FAILED and np.isnan(got).all() and np.isnan(rel_t).all(), f"{kind}, k = {k}: status {st}"
        assert iters == 0, f"{kind}, k = {k}: {iters} iterations on a problem that holds a NaN"
