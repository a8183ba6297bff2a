"""The tables of tests/lateral_cases.py are what they say they are (no GPU): every family, speed and parameter set is there, the
padding is poisoned, and the oracles' labels (tests/lateral_oracle.py) meet the conditions that keep tests/test_gpu_lateral_cases.py
honest - nearly every finite case is decided, every count of saturated controls occurs, no Riccati iteration ends within an ulp
of its threshold, and every tie resolves to the index the construction names."""
import collections

import numpy as np
import pytest

from tests import lateral_cases as F
from tests import lateral_oracle as O

FAMILIES = {"saturate", "speed", "singular", "wrap", "ties", "nonfinite"}
# finite inputs, non-finite model: Vx + 0.0001 == 0 divides the error model by zero (the reference raises ZeroDivisionError)
ZERO_MODEL_VELOCITY = "speed_v-0.0001"


def _all(law):
    return [(c, O.label(law, pset, i)) for pset, cs in F.table(law).items() for i, c in enumerate(cs)]


@pytest.mark.parametrize("law", F.LAWS)
def test_the_tables_cover_what_they_name(law):
    tab = F.table(law)
    assert tuple(tab) == F.PSETS
    cases = [c for cs in tab.values() for c in cs]
    assert 200 <= len(cases) <= 300
    assert len({(c.pset, c.name) for c in cases}) == len(cases)
    assert {c.family for c in cases} == FAMILIES
    for pset, cs in tab.items():
        assert {c.pset for c in cs} == {pset}
        assert {"saturate", "speed", "singular"} <= {c.family for c in cs}, pset
        assert {c.vx for c in cs if c.family == "speed"} >= {0.005, 9.0, 60.0, -0.005}, pset
    for pset in ("ref", "phys"):
        sat = [c for c in tab[pset] if c.family == "saturate"]
        assert len(sat) >= len(F.OFFSETS) * len(F.HEADINGS) * 2
        for shape in ("line", "arc"):
            assert {c.name.rsplit("_h", 1)[0] for c in sat if shape in c.name} == {f"saturate_{shape}_d{o:g}" for o in F.OFFSETS}
        assert {c.vx for c in tab[pset] if c.family == "speed"} == set(F.MPC_SPEEDS if law == "mpc" else F.GUARDED_SPEEDS)
    assert (law == "mpc") == any(c.name.startswith("ties_window") for c in cases)
    nonfinite = [c for c in cases if c.family == "nonfinite"]
    assert len(nonfinite) == 3 * (5 + 1 + 4)
    for c in cases:
        assert c.path.shape == (F.CAP, 4) and 1 <= c.n_path <= F.CAP and c.state.shape == (5,)
        assert np.isnan(c.path[c.n_path:, 2:]).all(), c.name
        if F.inputs_finite(c):
            np.testing.assert_array_equal(c.path[c.n_path:, :2], np.tile(F.predicted(c.state, c.vx), (F.CAP - c.n_path, 1)))
        assert (c.family == "nonfinite") == (not F.inputs_finite(c)), c.name
    for c in cases:
        if c.name == "singular_exact":
            py, k = c.path[c.min_index, 1], c.path[c.min_index, 3]
            assert 1.0 - k * (c.state[1] - py) == 0.0 and c.state[2] == 0.0 and c.state[3] == 0.0
        if c.name in ("singular_below", "singular_above"):
            assert abs(1.0 - c.path[0, 3] * c.state[1]) < 1e-10 and 1.0 - c.path[0, 3] * c.state[1] != 0.0


@pytest.mark.parametrize("law", F.LAWS)
def test_nearly_every_finite_case_is_decided(law):
    """Every finite case outside ``singular`` is decided but the one whose model velocity is exactly 0; undecided finite cases are at
    most 5 % of the table; a non-finite input leaves a case decided only where it is the x or y of a path point, which no law's
    match can select."""
    rows = _all(law)
    tally = collections.Counter((c.family, "decided" if l["decided"] else "undecided") for c, l in rows)
    print(f"{law}: {len(rows)} cases, {dict(sorted(tally.items()))}")
    undecided_finite = 0
    for c, l in rows:
        if c.family == "nonfinite":
            skipped_point = c.name.startswith(("nonfinite_path_x_", "nonfinite_path_y_"))
            assert l["decided"] == skipped_point, f"{c.pset} {c.name}: decided {l['decided']}"
            assert not skipped_point or l["min_index"] == F.NONFINITE_AT + 1, c.name      # the next point, 0.6 m nearer than the last
            continue
        if c.name == ZERO_MODEL_VELOCITY and law != "mpc":
            assert not l["decided"] and l.get("raised") == "ZeroDivisionError", c.name
        elif c.family != "singular":
            assert l["decided"], f"{c.pset} {c.name}: {l.get('raised')} {l.get('qp_status')}"
        undecided_finite += not l["decided"]
    assert undecided_finite <= 0.05 * len(rows), f"{undecided_finite} of {len(rows)}"
    for pset, cs in F.table(law).items():
        ls = O.labels(law, pset)
        for i, c in enumerate(cs):
            if c.family in ("nonfinite", "singular"):            # between two ordinary cases
                for j in (i - 1, i + 1):
                    assert cs[j].family not in ("nonfinite", "singular") and ls[j]["decided"], f"{pset} {c.name}"


def test_every_count_of_saturated_controls_occurs():
    """0, 2, .. 12 of the MPC's 12 controls at a bound each occur among the decided cases.  With r at its default, all 12 occur only
    with the physical tuple - outside ``singular``, whose e_fi_dot of 1e10 beside the singular point saturates anything.  (With
    r = 1e-3 or less the reference tuple's H is 2 r I to within rounding and any error saturates all 12.)"""
    seen = collections.defaultdict(set)
    for c, l in _all("mpc"):
        if l["decided"]:
            seen[l["n_bound"]].add((c.pset, c.family))
    print({k: len(v) for k, v in sorted(seen.items())})
    assert set(seen) >= {0, 2, 4, 6, 8, 10, 12}
    full = {(p, f) for p, f in seen[12] if p in F.DEFAULT_R and f != "singular"}
    assert full and all(p.startswith("phys") for p, _ in full), full
    assert max(l["n_bound"] for c, l in _all("mpc") if l["decided"] and c.pset == "ref" and c.family != "singular") == 10


def test_no_riccati_iteration_ends_on_the_threshold():
    """max|dP| at the last sweep and at the one before differs from 0.1 by more than 1e-6 relative in every LQR case, so rounding
    cannot move the sweep count; both ends of the sweep range occur."""
    sweeps = set()
    for c, l in _all("lqr"):
        if "last_deltas" not in l or not np.isfinite(c.vx):      # (a non-finite model has no sweep count to protect)
            continue
        for d in l["last_deltas"]:
            assert abs(d - 0.1) > 1e-6 * 0.1, f"{c.pset} {c.name}: max|dP| {l['last_deltas']}"
        if l["decided"]:
            sweeps.add(l["sweeps"])
    assert min(sweeps) < 10 and max(sweeps) == 5000 and len(sweeps) >= 10


@pytest.mark.parametrize("law", F.LAWS)
def test_ties_resolve_to_the_lowest_index(law):
    ties = [(c, l) for c, l in _all(law) if c.family == "ties"]
    assert len(ties) >= 8
    for c, l in ties:
        assert c.expect_index is not None and l["decided"] and l["min_index"] == c.expect_index, \
            f"{c.name}: the oracle matches {l['min_index']}, the construction says {c.expect_index}"
    by = {c.name: c for c, _ in ties}
    px, py = F.predicted(by["ties_pair_5_8"].state, by["ties_pair_5_8"].vx)
    for name, (lo, hi) in (("ties_pair_5_8", (5, 8)), ("ties_pair_2_5", (2, 5)), ("ties_pair_4_12", (4, 12))):
        d = (by[name].path[:by[name].n_path, 0] - px) ** 2 + (by[name].path[:by[name].n_path, 1] - py) ** 2
        assert d[lo] == d[hi] == 25.0 and (np.delete(d, [lo, hi]) > 25.0).all()
    c = by["ties_exactly_100m"]
    d = (c.path[:c.n_path, 0] - px) ** 2 + (c.path[:c.n_path, 1] - py) ** 2
    assert d.min() == 10000.0 and d.argmin() != c.expect_index
    c = by["ties_standstill"]
    assert (c.path[:c.n_path] == c.path[0]).all() and c.n_path > 8
