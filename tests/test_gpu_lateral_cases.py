"""emp_mpc_lateral, emp_mpc_ff_lateral and emp_lqr_lateral on the hard inputs of tests/lateral_cases.py: saturated, stiff
(the vehicle tuple in its physical order: eigenvalues of H from 2 to 5e5; r down to 1e-6; q_diag x 1e4), singular
(1 - k_r e_d == 0), wrapped headings, exact ties of the match, non-finite inputs.  One call per law and parameter set, under
tests/batch_check.invariant: every vehicle bit-equal alone, in the batch, reversed, shifted by one, host and device - so a
failing or slow vehicle changes nothing in its wavefront neighbours.

A case the oracles decide (tests/lateral_oracle.py) must come back with status 0, the oracle's match, e_rr to 1e-12, H and f to
1e-9, and controls that are judged on the ORACLE's H, f and minimiser, never on the kernel's own matrices: inside the box, the
gradient's sign right at every active bound, the objective within GAP of the oracle's and the controls within DIST of its
minimiser.  The reference-tuple sets keep the suite's 1e-6 on u.  The other bounds are ten times what an MI355X measured (the
margin covers one build's fast_rcp rounding against the next's), with two floors that come from the number format alone:

  ROUND   64 ulp of the objective's terms: J = u'Hu / 2 + f'u is evaluated here in float64 from 12 x 12 + 12 products, twice;
  1e-12   on a distance: the oracle polishes its own minimiser with a dense solve and is itself good to a few thousand ulp of 1.

and, for the MPC, under the ceiling |u - u*| <= sqrt(2 (gap + ROUND) / lambda_min(H)) that strong convexity gives: the bound
stays tied to the conditioning of the problem.  (The feed-forward law's H is singular by construction; there the distance is
taken on what the problem determines, control_port.determined.)  Measured worst distance | objective gap relative to its terms:

  MPC   ref 9.2e-13 | 1.6e-14   phys 6.4e-12 | 1.5e-16   ref_r1e-3 3.9e-13 | 1.1e-16   ref_r1e-6 1.2e-9 | 3.7e-14
        phys_r1e-3 7.2e-9 | 7.3e-17   phys_r1e-6 9.4e-6 | 8.4e-17   ref_q1e4 5.4e-16 | 0   phys_q1e4 5.7e-8 | 6.8e-17
  FF    ref 1.3e-9 | 4.9e-13   phys 3.5e-11 | 1.3e-16   ref_r1e-3 4.6e-9 | 3.1e-13   ref_r1e-6 6.6e-11 | 3.5e-13
        phys_r1e-3 1.8e-9 | 1.4e-14   phys_r1e-6 8.0e-7 | 1.5e-14   ref_q1e4 2.1e-11 | 4.1e-16   phys_q1e4 1.5e-7 | 1.9e-16

The physical tuple's gaps sit at the rounding of their own evaluation; the reference tuple's, whose objectives are of order 1, show
what the solver leaves: 24 rows x eps_mu = 1e-13 of complementarity.  LQR: sweeps equal to the oracle's (from 6 to all 5000), K
against the oracle's relative to its largest gain and steer relative to max(1, |steer|) within ten times MEASURED_LQR (worst
1.0e-12 and 1.8e-12, "ref_r1e-6"; the suite's bar on steer is 1e-6), over the same 1e-12 floor: the kernel sums its 4 x 4
products in another order than NumPy's matmul, for up to 5000 sweeps.

Undecided and non-finite cases are pinned to what include/emplanner.h states: the two MPCs fail them (EMP_ST_QP_FAILED or
EMP_ST_S_OUT_OF_RANGE, steer 0, u all zero); the LQR, which has no QP to fail, answers status 0 with the IEEE result of the
reference's expression and the finite model's own K and sweeps - or, where the model itself is not finite, EMP_ST_QP_FAILED, steer 0,
K all NaN after one sweep.  No case may hold its wavefront: iters <= 60, sweeps <= 5000.

A further test per fused law sends the reference-tuple table through emp_vehicle_control with ragged PID buffers."""
import functools

import numpy as np
import pytest

from tests import control_port as port
from tests import lateral_cases as F
from tests import lateral_oracle as O
from tests.batch_check import bits, invariant, to_np
from tests.conftest import assert_rel

pytestmark = pytest.mark.gpu

ST_S_OUT_OF_RANGE, ST_QP_FAILED = 2, 8
MAX_ITERS, MAX_SWEEPS = 60, 5000
NB = 60                                             # PID buffer
ROUND = 64 * 2.0 ** -52
DIST_FLOOR = 1e-12
MPC_FIELDS = ("steer", "u", "e_rr", "k_r", "min_index", "pre_pro", "H", "f", "iters", "status")
LQR_FIELDS = ("steer", "K", "e_rr", "k_r", "min_index", "pre_pro", "sweeps", "status")

# what an MI355X measured, per parameter set: the worst |u - u_oracle| (feed-forward: over control_port.determined) and the
# worst J(u) - J(u_oracle) relative to the objective's terms
MEASURED = {
    "mpc": {"ref": (9.2e-13, 1.6e-14), "phys": (6.4e-12, 1.5e-16), "ref_r1e-3": (3.9e-13, 1.1e-16), "ref_r1e-6": (1.2e-9, 3.7e-14),
            "phys_r1e-3": (7.2e-9, 7.3e-17), "phys_r1e-6": (9.4e-6, 8.4e-17), "ref_q1e4": (5.4e-16, 0.0),
            "phys_q1e4": (5.7e-8, 6.8e-17)},
    "ff": {"ref": (1.3e-9, 4.9e-13), "phys": (3.5e-11, 1.3e-16), "ref_r1e-3": (4.6e-9, 3.1e-13), "ref_r1e-6": (6.6e-11, 3.5e-13),
           "phys_r1e-3": (1.8e-9, 1.4e-14), "phys_r1e-6": (8.0e-7, 1.5e-14), "ref_q1e4": (2.1e-11, 4.1e-16),
           "phys_q1e4": (1.5e-7, 1.9e-16)},
}
# LQR: the worst |K - K_oracle| / max|K_oracle| and |steer - steer_oracle| / max(1, |steer_oracle|)
MEASURED_LQR = {"ref": (2.1e-13, 2.1e-13), "phys": (2.3e-13, 8.2e-14), "ref_r1e-3": (2.3e-13, 4.7e-13), "ref_r1e-6": (1.0e-12, 1.8e-12),
                "phys_r1e-3": (3.1e-13, 2.8e-14), "phys_r1e-6": (8.9e-13, 5.4e-15), "ref_q1e4": (2.5e-13, 7.1e-13),
                "phys_q1e4": (2.9e-13, 2.0e-14)}


def lqr_bounds(pset):
    """(K, steer): ten times the measured value over the same floor as a distance, steer never above the suite's 1e-6."""
    k, s = MEASURED_LQR[pset]
    return max(10.0 * k, DIST_FLOOR), min(1e-6, max(10.0 * s, DIST_FLOOR))


def dist_bound(law, pset):
    return 1e-6 if pset == "ref" else max(10.0 * MEASURED[law][pset][0], DIST_FLOOR)


def gap_bound(law, pset):
    return max(10.0 * MEASURED[law][pset][1], ROUND)


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    p = Planner(0)
    yield p
    p.close()


def lat_params(law, pset):
    from emplanner_carla_amd.api import mpc_params
    para, q, f, r = F.params(law, pset)
    return mpc_params(vehicle_para=para, q_diag=q, f_diag=f, r=r)


def _fields(r, names):
    return {k: to_np(getattr(r, k)) for k in names}


def run(pl, law, pset):
    p = lat_params(law, pset)
    if law == "lqr":
        call = lambda a, dev: _fields(pl.lqr_lateral(p, *a), LQR_FIELDS)
    else:
        fn = pl.mpc_lateral if law == "mpc" else pl.mpc_ff_lateral
        call = lambda a, dev: _fields(fn(p, *a, qp_matrices=True), MPC_FIELDS)
    return invariant(call, F.batch(F.table(law)[pset]), f"{law} {pset}")


def terms(H, f, u):
    """What the objective is a sum of: the scale of its rounding."""
    return float(0.5 * np.abs(u) @ np.abs(H) @ np.abs(u) + np.abs(f) @ np.abs(u))


def judge_controls(law, c, l, u):
    """The controls of a decided case on the oracle's H, f and minimiser -> (distance, gap relative to the terms)."""
    H, f, u0 = l["H"], l["f"], l["u"]
    who = f"{law} {c.pset} {c.name}"
    assert (np.abs(u) <= 1.0 + 1e-9).all(), f"{who}: outside the box by {np.abs(u).max() - 1.0:.3e}"
    grad = H @ u + f
    scale = max(1.0, np.abs(f).max())
    free = np.abs(u) < 1.0 - 1e-7
    assert np.abs(grad[free]).max(initial=0.0) <= 1e-6 * scale, f"{who}: gradient on the free controls"
    assert (grad[u >= 1.0 - 1e-7] <= 1e-6 * scale).all() and (grad[u <= -1.0 + 1e-7] >= -1e-6 * scale).all(), \
        f"{who}: the gradient points into the box at an active bound"
    mag = max(terms(H, f, u0), 1.0)
    gap = O.objective(H, f, u) - O.objective(H, f, u0)
    assert gap <= gap_bound(law, c.pset) * mag, f"{who}: objective {gap:.3e} above the oracle's (terms {mag:.3e})"
    if law == "ff":
        dist = float(np.abs(port.determined(u) - port.determined(u0)).max())
    else:
        dist = float(np.abs(u - u0).max())
        ceiling = np.sqrt(2.0 * (max(gap, 0.0) + ROUND * mag) / l["lam_min"])
        assert np.linalg.norm(u - u0) <= ceiling, f"{who}: |u - u*| {np.linalg.norm(u - u0):.3e} above the ceiling {ceiling:.3e}"
    assert dist <= dist_bound(law, c.pset), f"{who}: controls {dist:.3e} from the oracle's"
    return dist, gap / mag


@pytest.mark.parametrize("pset", F.PSETS)
@pytest.mark.parametrize("law", ["mpc", "ff"])
def test_mpc_laws_on_hard_cases(pl, law, pset):
    cs, ls = F.table(law)[pset], O.labels(law, pset)
    r = run(pl, law, pset)
    assert (r["iters"] <= MAX_ITERS).all() and (r["iters"] >= 0).all()
    worst_dist = worst_gap = 0.0
    judged = 0
    for b, (c, l) in enumerate(zip(cs, ls)):
        who = f"{law} {pset} {c.name}"
        if not l["decided"]:
            assert r["status"][b] in (ST_QP_FAILED, ST_S_OUT_OF_RANGE), f"{who}: status {r['status'][b]}"
            assert bits(r["steer"][b:b + 1]) == bits(np.zeros(1)) and bits(r["u"][b]) == bits(np.zeros_like(r["u"][b])), \
                f"{who}: a failed vehicle with controls {r['u'][b]}"
            continue
        assert r["status"][b] == 0, f"{who}: status {r['status'][b]} after {r['iters'][b]} iterations"
        assert r["min_index"][b] == l["min_index"], f"{who}: match {r['min_index'][b]}, the oracle's {l['min_index']}"
        assert c.expect_index is None or r["min_index"][b] == c.expect_index, who
        assert_rel(r["e_rr"][b], l["e_rr"], 1e-12, f"e_rr of {who}", scale=1.0)
        assert np.abs(r["H"][b] - l["H"]).max() <= 1e-9 * np.abs(l["H"]).max(), f"H of {who}"
        assert np.abs(r["f"][b] - l["f"]).max() <= 1e-9 * max(1.0, np.abs(l["f"]).max()), f"f of {who}"
        assert r["steer"][b] == r["u"][b, 0]
        dist, gap = judge_controls(law, c, l, r["u"][b])
        worst_dist, worst_gap = max(worst_dist, dist), max(worst_gap, gap)
        judged += 1
    print(f"{law} {pset}: {judged} of {len(cs)} judged; worst distance {worst_dist:.3e} (bound {dist_bound(law, pset):.1e}), "
          f"worst gap / terms {worst_gap:.3e} (bound {gap_bound(law, pset):.1e}), most iterations {r['iters'].max()}")
    assert judged == sum(l["decided"] for l in ls) >= 0.7 * len(cs)


def model_is_finite(c):
    """The LQR's model divides by Vx + 0.0001."""
    return not np.isnan(c.vx) and c.vx + 0.0001 != 0.0            # (+-inf: every quotient is 0)


@pytest.mark.parametrize("pset", F.PSETS)
def test_lqr_on_hard_cases(pl, pset):
    cs, ls = F.table("lqr")[pset], O.labels("lqr", pset)
    r = run(pl, "lqr", pset)
    assert (r["sweeps"] <= MAX_SWEEPS).all() and (r["sweeps"] >= 1).all()
    worst_k = worst_steer = 0.0
    judged = 0
    for b, (c, l) in enumerate(zip(cs, ls)):
        who = f"lqr {pset} {c.name}"
        if not model_is_finite(c):
            assert not l["decided"]
            assert r["status"][b] == ST_QP_FAILED and bits(r["steer"][b:b + 1]) == bits(np.zeros(1)), f"{who}: status {r['status'][b]}"
            assert r["sweeps"][b] == 1 and np.isnan(r["K"][b]).all(), f"{who}: {r['sweeps'][b]} sweeps, K {r['K'][b]}"
            continue
        assert r["status"][b] == 0, f"{who}: status {r['status'][b]}"
        K, sweeps, _ = O.riccati(pset, c.vx)                  # a function of the parameters and vx alone
        K = np.asarray(K).reshape(-1)
        assert r["sweeps"][b] == sweeps, f"{who}: {r['sweeps'][b]} sweeps, the oracle's {sweeps}"
        k_err = float(np.abs(r["K"][b] - K).max() / np.abs(K).max())
        assert k_err <= lqr_bounds(pset)[0], f"{who}: K off by {k_err:.3e} of its largest entry"
        worst_k = max(worst_k, k_err)
        if not l["decided"]:
            assert not np.isfinite(r["steer"][b]), f"{who}: steer {r['steer'][b]} from a non-finite tracking error"
            continue
        assert r["min_index"][b] == l["min_index"], f"{who}: match {r['min_index'][b]}, the oracle's {l['min_index']}"
        assert c.expect_index is None or r["min_index"][b] == c.expect_index, who
        assert_rel(r["e_rr"][b], l["e_rr"], 1e-12, f"e_rr of {who}", scale=1.0)
        s_err = abs(r["steer"][b] - l["steer"]) / max(1.0, abs(l["steer"]))
        assert s_err <= lqr_bounds(pset)[1], f"{who}: steer off by {s_err:.3e}"
        worst_steer = max(worst_steer, s_err)
        judged += 1
    print(f"lqr {pset}: {judged} of {len(cs)} judged; worst K {worst_k:.3e}, worst steer {worst_steer:.3e}, sweeps "
          f"{r['sweeps'].min()} .. {r['sweeps'].max()}")
    assert judged == sum(l["decided"] for l in ls) >= 0.7 * len(cs)
    assert (r["sweeps"] == MAX_SWEEPS).any()


# ---------------------------------------------------------------------------------------------------------------------
# the fused step
# ---------------------------------------------------------------------------------------------------------------------
def _py_actuation(s, acc):
    """Vehicle_control.run_step's limits with Python's own min / max (they keep their first argument against NaN)."""
    steering = min(1, s) if s >= 0 else max(-1, s)
    if acc >= 0:
        return float(min(1, acc)), float(steering), 0.0
    return 0.0, float(steering), float(max(1, acc))


@functools.lru_cache(maxsize=None)
def _pid_inputs(B):
    """Ragged buffers (0 to 60 entries, NaN past the count), errors on both sides of the separation threshold."""
    rng = np.random.default_rng(900 + B)
    n = rng.integers(0, NB + 1, B).astype(np.int32)
    n[0], n[1], n[-1] = NB, 0, NB
    err = np.full((B, NB), np.nan)
    for b in range(B):
        err[b, :n[b]] = rng.uniform(-0.9, 0.9, n[b])
    speed = rng.uniform(0.0, 80.0, B)
    dev = np.where(rng.random(B) < 0.5, rng.uniform(-0.4, 0.4, B), rng.choice([-1, 1], B) * rng.uniform(1.5, 6.0, B))
    return speed, speed + dev, err, n


@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_vehicle_control_on_hard_cases(pl, law):
    """The reference-tuple table, decided and failing cases alike, through emp_vehicle_control: lat_command bit-identical to the
    stand-alone steer, a failed vehicle with zero controls and its PID state untouched, a non-finite LQR command actuated as the
    header says (NaN and -inf: full lock -1, +inf: +1)."""
    from emplanner_carla_amd.api import pid_params
    cs = F.table(law)["ref"]
    lat_p, pid_p = lat_params(law, "ref"), pid_params()
    a = F.batch(cs)
    B = len(cs)
    speed, target, err, n_err = _pid_inputs(B)
    r = pl.vehicle_control(lat_p, pid_p, *a, speed, target, err, n_err, lateral=law)
    lat = (pl.mpc_lateral if law == "mpc" else pl.lqr_lateral)(lat_p, *a)
    pid = pl.pid_longitudinal(pid_p, speed, target, err, n_err)
    for name, got in (("steer", r.lat_command), ("min_index", r.min_index), ("e_rr", r.e_rr), ("k_r", r.k_r),
                      ("pre_pro", r.pre_pro), ("status", r.status)):
        assert bits(got) == bits(getattr(lat, name)), f"vehicle_control {law}: {name} differs from the stand-alone law"
    ok = r.status == 0
    assert ok.sum() >= 0.7 * B and (~ok).sum() >= 2
    odd = 0
    for b in range(B):
        who = f"vehicle_control {law} {cs[b].name}"
        if not ok[b]:
            assert bits(r.control[b]) == bits(np.zeros(3)) and bits(r.lon_command[b:b + 1]) == bits(np.zeros(1)), f"{who}: controls"
            assert bits(r.err[b]) == bits(err[b]) and r.n_err[b] == n_err[b], f"{who}: PID state of a failed vehicle"
            continue
        assert bits(r.lon_command[b:b + 1]) == bits(pid.command[b:b + 1]), f"{who}: lon_command"
        assert bits(r.err[b]) == bits(pid.err[b]) and r.n_err[b] == pid.n_err[b], f"{who}: PID state"
        want = _py_actuation(float(r.lat_command[b]), float(r.lon_command[b]))
        assert bits(r.control[b]) == bits(np.array(want)), f"{who}: control {r.control[b]}, by the header {want}"
        if not np.isfinite(r.lat_command[b]):
            assert r.control[b, 1] == (1.0 if r.lat_command[b] == np.inf else -1.0), who
            odd += 1
    assert (odd >= 20) if law == "lqr" else (odd == 0)
