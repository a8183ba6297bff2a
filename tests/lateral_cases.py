"""Hard inputs for the three lateral laws (emp_mpc_lateral, emp_mpc_ff_lateral, emp_lqr_lateral), as plain NumPy: what
tests/test_lateral_cases_host.py labels on the CPU and tests/test_gpu_lateral_cases.py feeds to the kernels.  A helper module (no
fixtures, no hooks).

A case is Case(name, family, pset, path, n_path, state, vx, min_index, expect_index): one vehicle with its path row [CAP][4], the
count of valid points, state = x, y, fi, Vy, fi_dot, the law's vx and the previous match.  expect_index is the match the
construction decides without a solver (``ties``), None elsewhere.  Every path slot past n_path is poisoned: a point at the
vehicle's predicted position with NaN theta and kappa, so a search that reaches it picks it and its NaN shows in the outputs.

Parameters are per call, so ``table(law)`` returns {pset: [Case, ...]} in call order.  The parameter sets (PSETS): the vehicle tuple
in the order the reference's drivers pass it ("ref": (a, b, Cf, Cr, m, Iz) = (1.015, 1.895, 1412, -148970, -82204, 1537), which
makes H nearly 2 I) and in its physical order ("phys": Cf = -148970, Cr = -82204, m = 1412: eigenvalues of H from 2 to 5e5), each
with the law's default weights, with r = 1e-3 and 1e-6, and with q_diag x 1e4.

Families: saturate (lateral offsets and heading errors from small to absurd, straight and curved), speed (creeping, reversing,
fast; for the two laws that guard their divisions with Vx + 0.0001 also 0, 1e-6 and the -0.0001 that makes the guarded velocity
exactly 0), singular (1 - k_r e_d exactly 0 in binary, and 1e-9 m to either side), wrap (yaw a whole number of turns from the
path's heading, headings that straddle +-pi), ties (exactly equidistant path points, a standstill path of identical points, a
point at exactly 100 m, one- and two-point paths, the match at the last index, the MPC's 50-point window) and nonfinite (NaN and
+-inf in turn in every state entry, in vx and in every field of the matched path point, each between two ordinary cases).  The
two default-weight sets carry the whole saturate grid; everything whose point is the matching or the error model rather than
the weights sits in "ref" only; the six other sets carry a cut of saturate, speed and singular."""
import collections
import functools
import math

import numpy as np

NAN = np.nan
CAP = 64                                 # path capacity of every call
LAWS = ("mpc", "ff", "lqr")
TS = 0.1                                 # the prediction step of all three laws

REF = (1.015, 1.895, 1412.0, -148970.0, -82204.0, 1537.0)       # as the reference's drivers pass it
PHYS = (1.015, 1.895, -148970.0, -82204.0, 1412.0, 1537.0)      # what the names (a, b, Cf, Cr, m, Iz) say

DEFAULT_WEIGHTS = {                      # q_diag, f_diag, r: api.mpc_params / mpc_ff_params / lqr_params
    "mpc": ((250.0, 1.0, 50.0, 1.0), (1.0, 1.0, 1.0, 1.0), 1.0),
    "ff": ((200.0, 1.0, 1.0, 1.0), (10.0, 10.0, 10.0, 10.0), 1.0),
    "lqr": ((200.0, 1.0, 50.0, 1.0), (1.0, 1.0, 1.0, 1.0), 1.0),
}
PSETS = ("ref", "phys", "ref_r1e-3", "ref_r1e-6", "phys_r1e-3", "phys_r1e-6", "ref_q1e4", "phys_q1e4")
DEFAULT_R = ("ref", "phys", "ref_q1e4", "phys_q1e4")             # the sets whose r is the default 1

OFFSETS = (0.05, 0.5, 3.0, 20.0, 90.0)
HEADINGS = (0.0, 0.1, math.pi / 2, 3.0)
KAPPA = 0.05
MPC_SPEEDS = (0.005, 0.05, 1.0, 9.0, 30.0, 60.0, -0.005)
GUARDED_SPEEDS = MPC_SPEEDS + (0.0, 1e-6, -1.5, -0.0001)
SING_KAPPA, SING_OFFSET = 0.0625, 16.0                           # 1 - 0.0625 * 16 == 0 exactly
WINDOW = 50                                                      # the MPC's match window

Case = collections.namedtuple("Case", "name family pset path n_path state vx min_index expect_index")


def params(law, pset):
    """(vehicle_para, q_diag, f_diag, r) of a parameter set."""
    q, f, r = DEFAULT_WEIGHTS[law]
    tup, _, mod = pset.partition("_")
    if mod.startswith("r"):
        r = float(mod[1:])
    elif mod == "q1e4":
        q = tuple(v * 1e4 for v in q)
    return (REF if tup == "ref" else PHYS), q, f, r


def predicted(state, vx):
    """The pose all three laws search the path for, in the laws' own order of operations."""
    x, y, fi, Vy = (float(v) for v in state[:4])
    with np.errstate(all="ignore"):
        c, s = np.cos(fi), np.sin(fi)
        return x + vx * TS * c - Vy * TS * s, y + Vy * TS * c + vx * TS * s


# ---------------------------------------------------------------------------------------------------------------------
# paths: (n, 4) x, y, theta, kappa
# ---------------------------------------------------------------------------------------------------------------------
def straight(n, step=1.0, x0=0.0, y0=0.0, kappa=0.0):
    p = np.zeros((n, 4))
    p[:, 0] = x0 + step * np.arange(n)
    p[:, 1] = y0
    p[:, 3] = kappa
    return p


def arc(n, kappa=KAPPA, step=1.0):
    """A left turn of curvature kappa from the origin, heading +x at its start."""
    th = kappa * step * np.arange(n)
    return np.column_stack([np.sin(th) / kappa, (1.0 - np.cos(th)) / kappa, th, np.full(n, kappa)])


def west(n):
    """Heading -x with theta alternately just below +pi and just above -pi."""
    p = np.zeros((n, 4))
    p[:, 0] = -1.0 * np.arange(n)
    p[:, 2] = np.where(np.arange(n) % 2 == 0, math.pi - 1e-3, -math.pi + 1e-3)
    return p


def beside(path, at, offset, heading, vx, Vy=0.0, fi_dot=0.0):
    """The state whose PREDICTED pose lies ``offset`` to the left of path point ``at`` with yaw theta + heading."""
    px, py, th, _ = path[at]
    fi = th + heading - fi_dot * TS
    X, Y = px - offset * math.sin(th), py + offset * math.cos(th)
    c, s = math.cos(fi), math.sin(fi)
    return np.array([X - (vx * TS * c - Vy * TS * s), Y - (Vy * TS * c + vx * TS * s), fi, Vy, fi_dot])


def _case(name, family, pset, path, state, vx, mi, n=None, expect=None):
    n = len(path) if n is None else n
    row = np.zeros((CAP, 4))
    row[:len(path)] = path
    row[n:, :2] = predicted(state, vx)
    row[n:, 2:] = NAN
    return Case(name, family, pset, row, n, np.asarray(state, dtype=np.float64), float(vx), int(mi), expect)


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------
def _saturate(law, pset, cut):
    """offsets x headings x {straight, curved}; on the curve the vehicle is outside it (inside, 20 m is its centre).  cut: every
    fourth case of the grid, which still spans every offset and heading."""
    out = []
    k = 0
    for shape, path in (("line", straight(48)), ("arc", arc(48))):
        for off in OFFSETS:
            for hd in HEADINGS:
                k += 1
                if cut and k % 4 != (1 if shape == "line" else 2):
                    continue
                side = 1.0 if shape == "line" else -1.0
                at = 20 + (k % 5)
                st = beside(path, at, side * off, hd if k % 2 else -hd, 9.0, Vy=0.2 * ((k % 3) - 1), fi_dot=0.05 * ((k % 4) - 1.5))
                out.append(_case(f"saturate_{shape}_d{off:g}_h{hd:.3g}", "saturate", pset, path, st, 9.0, max(0, at - (k % 3))))
    # nearly all and nearly none of the controls at a bound: the errors between the grid's
    for j, (off, hd) in enumerate(((0.0, 0.0), (0.2, 0.02), (1.0, 0.3), (1.5, -0.4), (6.0, 1.0), (0.3, -0.25))):
        if cut and j % 3:
            continue
        path = straight(48)
        out.append(_case(f"saturate_mid_d{off:g}_h{hd:g}", "saturate", pset, path, beside(path, 22, off, hd, 9.0), 9.0, 20))
    return out


def _speed(law, pset, cut):
    speeds = MPC_SPEEDS if law == "mpc" else GUARDED_SPEEDS
    out = []
    for j, v in enumerate(speeds):
        if cut and abs(v) not in (0.005, 9.0, 60.0):
            continue
        path = arc(48) if j % 2 else straight(48)
        st = beside(path, 18 + j, 0.4 if j % 2 else -0.3, 0.08, v, Vy=0.1, fi_dot=-0.05)
        out.append(_case(f"speed_v{v:g}", "speed", pset, path, st, v, 16 + j))
    return out


def _singular(law, pset, cut):
    """theta = fi = 0 and Vy = 0, vx = 10: the prediction, e_d = y - py and 1 - k_r e_d are exact in binary."""
    out = []
    for tag, dy in (("exact", 0.0), ("below", -1e-9), ("above", 1e-9)):
        path = straight(40, kappa=SING_KAPPA)
        st = np.array([path[12, 0] - 1.0, SING_OFFSET + dy, 0.0, 0.0, 0.0])
        out.append(_case(f"singular_{tag}", "singular", pset, path, st, 10.0, 10))
    return out


def _wrap(law, pset):
    out = []
    path = arc(48)
    for k in (1, -1, 3, -3):
        st = beside(path, 21, -0.3, 2.0 * math.pi * k, 9.0, Vy=0.1)
        out.append(_case(f"wrap_turns{k:+d}", "wrap", pset, path, st, 9.0, 19))
    path = west(40)
    for at, hd in ((14, 0.05), (15, -0.05)):
        out.append(_case(f"wrap_west_at{at}", "wrap", pset, path, beside(path, at, 0.4, hd, 9.0), 9.0, at - 2))
    return out


def _ties(law, pset):
    """fi = 0, Vy = 0, vx = 10 and integer coordinates: the predicted pose is (x + 1, y) exactly and so is every squared distance."""
    out = []
    vx = 10.0
    still = 0.005 if law == "mpc" else 0.0
    far = lambda n: straight(n, x0=-20.0, y0=60.0)                  # every point more than 60 m away, all distinct
    st = np.array([9.0, 0.0, 0.0, 0.0, 0.0])                        # predicted (10, 0)
    # a standstill trajectory: every point the same
    p = np.tile(np.array([[3.0, 1.0, 0.2, 0.01]]), (20, 1))
    out.append(_case("ties_standstill", "ties", pset, p, np.array([2.5, 0.5, 0.1, 0.0, 0.0]), still, 0, expect=0))
    # two points at squared distance 25, the rest farther: (lower index, higher index); 5 / 8 puts the HIGHER index on the FF
    # search's lower lane, 2 / 5 the lower index on the lower lane, 4 / 12 both on one lane
    for lo, hi in ((5, 8), (2, 5), (4, 12)):
        p = far(30)
        p[lo, :2] = 10.0 - 3.0, 4.0
        p[hi, :2] = 10.0 + 5.0, 0.0
        out.append(_case(f"ties_pair_{lo}_{hi}", "ties", pset, p, st, vx, 0, expect=lo))
    # the only point within reach at exactly 100 m: strict < keeps the fallback
    p = straight(30, x0=200.0, y0=300.0)
    p[7, :2] = 10.0 + 60.0, 80.0
    out.append(_case("ties_exactly_100m", "ties", pset, p, st, vx, 3, expect=3))
    out.append(_case("ties_one_point", "ties", pset, np.array([[10.0, 1.0, 0.0, 0.0]]), st, vx, 0, expect=0))
    out.append(_case("ties_two_points", "ties", pset, np.array([[9.0, 1.0, 0.0, 0.0], [11.0, 1.0, 0.0, 0.0]]), st, vx, 0, expect=0))
    p = straight(40, x0=-29.0, y0=1.0)                              # the last point at (10, 1)
    out.append(_case("ties_last_index", "ties", pset, p, st, vx, 0 if law != "mpc" else 10, expect=39))
    if law == "mpc":
        p = straight(CAP, x0=-45.0, y0=1.0)                         # point 55 at (10, 1)
        out.append(_case("ties_window_49", "ties", pset, p, st, vx, 55 - (WINDOW - 1), n=CAP, expect=55))
        out.append(_case("ties_window_50", "ties", pset, p, st, vx, 55 - WINDOW, n=CAP, expect=54))
    return out


NONFINITE_VALUES = (("nan", NAN), ("pinf", np.inf), ("ninf", -np.inf))
NONFINITE_AT = 17                                                   # the base case's matched point


def _nonfinite_base(pset):
    """0.3 m past its matched point, so that with this point passed over the next one is nearest by 0.6 m, not by rounding."""
    path = straight(40)
    state = beside(path, NONFINITE_AT, 0.5, 0.1, 9.0, Vy=0.1, fi_dot=0.02)
    path[:, 0] -= 0.3
    return path, state, 9.0, NONFINITE_AT - 1


def _nonfinite(law, pset):
    out = []
    for tag, v in NONFINITE_VALUES:
        for j in range(5):
            path, st, vx, mi = _nonfinite_base(pset)
            pre = predicted(st, vx)
            st[j] = v
            c = _case(f"nonfinite_state{j}_{tag}", "nonfinite", pset, path, st, vx, mi, n=36)
            c.path[36:, :2] = pre                                   # the poison stays where the sound vehicle would look
            out.append(c)
        path, st, vx, mi = _nonfinite_base(pset)
        c = _case(f"nonfinite_vx_{tag}", "nonfinite", pset, path, st, v, mi, n=36)
        c.path[36:, :2] = predicted(st, vx)
        out.append(c)
        for f, fname in enumerate(("x", "y", "theta", "kappa")):
            path, st, vx, mi = _nonfinite_base(pset)
            path[NONFINITE_AT, f] = v
            out.append(_case(f"nonfinite_path_{fname}_{tag}", "nonfinite", pset, path, st, vx, mi, n=36))
    return out


def _interleave(ordinary, special):
    """Every special case between two ordinary ones."""
    assert len(ordinary) > len(special)
    out = []
    for i, c in enumerate(ordinary):
        out.append(c)
        if i < len(special):
            out.append(special[i])
    return out


@functools.lru_cache(maxsize=None)
def table(law):
    """{pset: [Case, ...]} in call order for one law."""
    assert law in LAWS
    out = {}
    for pset in PSETS:
        cut = pset not in ("ref", "phys")
        ordinary = _saturate(law, pset, cut) + _speed(law, pset, cut)
        if pset == "ref":
            ordinary += _wrap(law, pset) + _ties(law, pset)
            special = _singular(law, pset, cut) + _nonfinite(law, pset)
        else:
            special = _singular(law, pset, cut)
        out[pset] = _interleave(ordinary, special)
    return out


def batch(cases):
    """The arrays of one call: path [B][CAP][4], n_path, state [B][5], vx, min_index."""
    return [np.stack([c.path for c in cases]), np.array([c.n_path for c in cases], np.int32), np.stack([c.state for c in cases]),
            np.array([c.vx for c in cases]), np.array([c.min_index for c in cases], np.int32)]


def inputs_finite(c):
    return bool(np.isfinite(c.state).all() and np.isfinite(c.vx) and np.isfinite(c.path[:c.n_path]).all())
