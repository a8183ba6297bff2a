"""The corridors of tests/path_qp_cases.py are what they say they are (no GPU): the dense reference formulation classifies every
case as its construction intends, certifies its own answer, and the two CPU builds of the project's banded solver (interior point,
dual active set: tests/host_check) agree with it in return code and values.  What tests/test_gpu_path_qp_cases.py then asks of the
kernels is asked of the scalar code first."""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import host_check
from tests import path_qp_cases as F
from tests.conftest import assert_rel

RTOL = 1e-6
MAX_ITER = 60              # kQpMaxIter of emp_qp_core.h: the interior point's cap


@pytest.fixture(scope="module")
def hc():
    return host_check.load()


def solve(hc, c, solver):
    n = c.n
    l_min, l_max = np.ascontiguousarray(c.l_min), np.ascontiguousarray(c.l_max)
    out = [np.zeros(n) for _ in range(3)]
    it = C.c_int(0)
    fn = hc.hc_path_qp if solver == "ipm" else hc.hc_path_qp_gi
    rc = fn(n, l_min.ctypes.data, l_max.ctypes.data, *[float(v) for v in c.start_l3], F.QP_PRM.ctypes.data, out[0].ctypes.data,
            out[1].ctypes.data, out[2].ctypes.data, C.byref(it))
    return rc, np.stack(out, axis=1), it.value


def test_the_case_set_covers_what_it_names():
    cs = F.cases()
    assert {c.n for c in cs.values()} == set(F.SIZES)
    assert {c.family for c in cs.values()} == set(F.FAMILIES)
    for n in F.SIZES:
        fams = {c.family for c in cs.values() if c.n == n}
        assert {"open", "offset", "random", "bound", "endpin", "inspect"} <= fams, n
        assert ("chicane" in fams) == (n >= 6) and ("pinch" in fams) == (n >= 8) and ("spline" in fams) == (n in F.SPLINE_SIZES)
    for c in cs.values():
        lb, ub = F.station_ranges(c.l_min, c.l_max)
        assert np.isfinite(c.l_min).all() and np.isfinite(c.l_max).all()
        assert F.infeasible_by_inspection(c) == (c.family == "inspect"), c.name
        if c.family == "spline":                       # nothing to see: every station's own range is open, the ends are inside
            assert (ub - lb >= 0.02 - 1e-12).all() and c.expectation == "infeasible"
        if c.family == "pinch":
            p = F.pinch_station(c.n)
            assert abs((ub[p] - lb[p]) - F.PINCH_GAP) < 1e-12 and (np.delete(ub - lb, p) > 1.0).all()
        if c.family == "bound":
            assert c.start_l3[0] == ub[0] if "exact" in c.name else 0.0 < ub[0] - c.start_l3[0] < 2e-12
        if c.family == "endpin":
            assert c.l_min[-1] == 2.0 and lb[-1] < 0.0


@pytest.mark.parametrize("n", F.SIZES)
def test_oracle_and_cpu_solvers_agree_on_every_case(hc, n):
    for c in (c for c in F.cases().values() if c.n == n):
        verdict, x, cert = F.truth(c.name)
        if verdict == "uncertified":                   # counted by the summary test below
            continue
        assert verdict == c.expectation, f"{c.name}: the oracle says {verdict}"
        for solver in ("ipm", "gi"):
            rc, got, iters = solve(hc, c, solver)
            if verdict == "infeasible":
                assert rc != 0, f"{c.name}, {solver}: infeasible, the solver claims success"
                continue
            assert rc == 0, f"{c.name}, {solver}: rc {rc} after {iters} iterations"
            assert solver == "gi" or iters <= MAX_ITER        # (the active-set method counts constraint changes, one a step)
            scale = F.HALF_W if c.family == "pinch" else None
            for k, what in enumerate(("l", "dl", "ddl")):
                assert_rel(got[:, k], x[:, k], RTOL, f"{c.name}, {solver}: {what}", scale=scale)
        if c.family == "chicane" and n not in F.TINY:
            up_plus, up_minus, lo_plus, lo_minus = F.active_rows(c, x)
            blocks, _ = F.chicane_blocks(n)
            assert min(up_plus, up_minus, lo_plus, lo_minus) >= 1 and up_plus + up_minus + lo_plus + lo_minus >= 2 * len(blocks), \
                f"{c.name}: active rows {(up_plus, up_minus, lo_plus, lo_minus)}"


def test_the_oracle_certifies_the_feasible_cases():
    """At most 10 % of the cases built to be feasible may go without a certified answer; no size and no family loses all."""
    by_size, by_family = collections.Counter(), collections.Counter()
    total_size, total_family = collections.Counter(), collections.Counter()
    for c in F.cases().values():
        if c.expectation != "feasible":
            continue
        ok = F.truth(c.name)[0] == "feasible"
        total_size[c.n] += 1
        total_family[c.family] += 1
        by_size[c.n] += ok
        by_family[c.family] += ok
    print("certified per size:  ", {n: f"{by_size[n]}/{total_size[n]}" for n in total_size})
    print("certified per family:", {f: f"{by_family[f]}/{total_family[f]}" for f in total_family})
    good, total = sum(by_size.values()), sum(total_size.values())
    print(f"certified: {good} of {total} feasible-by-design cases")
    assert total - good <= 0.1 * total
    assert all(by_size[n] >= 1 for n in total_size) and all(by_family[f] >= 1 for f in total_family)
