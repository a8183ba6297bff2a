"""GPU suite of the vehicle model on hard input: emp_vehicle_step on the table of tests/vehicle_cases.py (speeds at rest, on the
0.005 clamp, reversing, infinite and NaN; controls out of range and non-finite; NaN in every state field) against
tests/vehicle_port.py - Vy+, fi_dot+, Vx+, vx_ctl and speed_kmh bit for bit with NaN matching NaN, the pose to 1e-12 where finite -
and under tests/batch_check.invariant; and emp_rollout on a fleet that brakes to rest, with a reversing and a NaN-speed vehicle
between good ones, against the chain of the separate calls (tests/test_gpu_rollout.chain) bit for bit.
tests/test_vehicle_cases_host.py runs the same table through the g++ build of the same core.

The LQR rollout is the test that found the sign of the NaN PID error to differ between emp_rollout and the chain (0xfff8... against
0x7ff8..., measured on the MI355X; nothing else differed): ctl::pid_step now stores a NaN error as the quiet NaN, DESIGN.md 3.9.

Set EMP_ROLLOUT_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_rollout as TR  # noqa: E402  (its chain and helpers; nothing of it is collected here)
import vehicle_cases as V  # noqa: E402
import vehicle_port as vp  # noqa: E402

pytestmark = pytest.mark.gpu
say, to_np = TR.say, TR.to_np


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


@pytest.mark.parametrize("pset", list(V.PARAM_SETS))
def test_vehicle_step_on_the_case_table(pl, pset):
    import batch_check as bc
    from emplanner_carla_amd.api import vehicle_params
    kw = V.PARAM_SETS[pset]
    prm, par = vp.params(**kw), vehicle_params(**kw)
    state, control = V.arrays()

    def call(args, device):
        r = pl.vehicle_step(par, *args)
        if device:
            pl.synchronize()
        return dict(state=to_np(r.state), ctl_state=to_np(r.ctl_state), vx_ctl=to_np(r.vx_ctl), speed_kmh=to_np(r.speed_kmh))

    got = bc.invariant(call, [state, control], f"vehicle_step {pset}")
    want = np.array([vp.step(prm, state[i], control[i]) for i in range(len(state))])
    fin = np.isfinite(want[:, :3])
    with np.errstate(invalid="ignore"):
        pose = np.abs(got["state"][:, :3] - want[:, :3]) / np.maximum(1.0, np.abs(want[:, :3]))
    say(f"vehicle_step {pset}: worst pose error where finite {pose[fin].max():.3g} (bar 1e-12)")
    for b, c in enumerate(V.table()):
        what = (pset, c["name"])
        assert V.eq_nan(got["state"][b, 3:], want[b, 3:]), (what, got["state"][b], want[b])        # Vy+, fi_dot+, Vx+
        assert (pose[b][fin[b]] <= 1e-12).all(), (what, got["state"][b], want[b])
        assert V.eq_nan(got["state"][b, :3][~fin[b]], want[b, :3][~fin[b]]), (what, got["state"][b], want[b])
        assert V.eq_nan(got["vx_ctl"][b], vp.clamp_vx(want[b, 5])) and V.eq_nan(got["speed_kmh"][b], vp.speed_kmh(want[b, 5], want[b, 3])), what
        assert V.eq_nan(got["ctl_state"][b], got["state"][b, :5]), what
    vx = got["state"][:, 5]
    assert not np.isnan(vx).any() and (vx >= 0.0).all() and not np.signbit(vx[vx == 0.0]).any()   # no reversing, no -0.0, a NaN speed steps to 0
    if pset == "stop":
        b = [c["name"] for c in V.table()].index("v_exactly_zero")
        assert vx[b] == 0.0 and state[b, 5] == 0.5


# ---------------------------------------------------------------------------------------------------------------------
# emp_rollout: braking to rest, a reversing and a NaN-speed vehicle between good ones
# ---------------------------------------------------------------------------------------------------------------------
def resting_fleet(speeds):
    """Straight paths of several headings, the vehicle 0.2 m beside its third point at the given Vx, target 0 km/h: the PID's first
    command is the full brake."""
    B = len(speeds)
    path, state = np.zeros((B, TR.M, 4)), np.zeros((B, 6))
    for b in range(B):
        path[b] = TR.arc(0.0, TR.M, rot=-2.0 + 0.9 * b, x0=10.0 * b, y0=-5.0 * b)
        p = path[b, 2]
        state[b] = [p[0] - 0.2 * math.sin(p[2]), p[1] + 0.2 * math.cos(p[2]), p[2] + 0.01, 0.02, 0.0, speeds[b]]
    return dict(B=B, path=path, n=np.full(B, TR.M, np.int32), state=state, mi=np.full(B, 2, np.int32), target=np.zeros(B),
                err=np.zeros((B, 60)), n_err=np.zeros(B, np.int32))


@pytest.mark.parametrize("law,T,speeds", [("mpc", 12, (0.3, 0.05, -2.0, 0.3, math.nan, 0.3)), ("lqr", 6, (0.3, -2.0, math.nan))])
def test_rollout_to_rest_equals_the_chain_bit_for_bit(pl, law, T, speeds):
    """A fleet of 6 is one wavefront's five vehicles and one more (MPC); a short run of three vehicles for LQR, whose creeping
    vehicles cost up to 5000 Riccati sweeps a tick (csrc/emp_rollout_kernels.h)."""
    from emplanner_carla_amd.api import vehicle_params
    d = resting_fleet(speeds)
    want = TR.chain(pl, law, d, T)
    r = pl.rollout(TR.laws()[law], TR.pid(), vehicle_params(), d["path"], d["n"], d["state"], d["mi"], d["target"], d["err"], d["n_err"], T,
                   lateral=law, log_every=1)
    TR.check_against_chain(r, want, T, 1, f"{law} to rest")
    vx = np.concatenate([to_np(r.log_state)[:, :, 5], to_np(r.state)[None, :, 5]])      # before each tick, and after the last
    say(f"rollout to rest {law}: Vx per tick {vx.T.tolist()}")
    after = vx[1:]
    assert not np.isnan(after).any() and (after >= 0.0).all() and not np.signbit(after[after == 0.0]).any()   # no reversing, no -0.0, no NaN
    slow, rev, bad = [b for b, v in enumerate(speeds) if v == 0.05], speeds.index(-2.0), [b for b, v in enumerate(speeds) if math.isnan(v)][0]
    # one tick of the full brake (0.06 m/s) takes a 0.05 m/s vehicle through zero; the model does not reverse; a NaN speed steps to 0
    assert (vx[1, slow] == 0.0).all() and vx[1, rev] == 0.0 and vx[1, bad] == 0.0
    good = [b for b, v in enumerate(speeds) if v == 0.3]
    assert (vx[1, good] < 0.3).all() and np.isfinite(to_np(r.state)[good]).all()
