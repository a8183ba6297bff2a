"""Hard corridors for the S-T speed QP (speed_QP, oracle/st_backend.py), as plain NumPy: what tests/test_speed_qp_cases_host.py
checks on the CPU and tests/test_gpu_speed_qp_cases.py feeds to emp_speed_qp.  A helper module (no fixtures, no hooks).

A case is Case(name, family, k, v0, a0, dp_s, dp_t, s_lb, s_ub, sd_lb, sd_ub, design): k valid DP columns (NaN behind them), the
pinned start (0, v0, a0) and the four bound arrays [16].  The reference's geometry, which every family below respects:

    dp_t[j] = 0.5 (j + 1) for j < k;   qp_size = k;   dt = dp_t[k-1] / (k-1)   (NOT 0.5);
    station i = 1 .. k-1 sits at time i dt and is bounded by DP column i-1;   -6 <= s_dot2_i <= 4;   s_i >= s_{i-1}

so columns k-1 .. 15 are never read.  They are poisoned, alternately with crossed bounds (s_lb > s_ub) and with NaN: a kernel or
an oracle that read them would show it.  On the used columns s_dot_lb = 0, as generate_convex_space sets it.

``design`` is what the construction can decide WITHOUT a solver (``design_of``), from the spline recurrences
s_{i+1} = s_i + dt s_dot_i + dt^2 (a_i / 3 + a_{i+1} / 6), s_dot_{i+1} = s_dot_i + dt (a_i + a_{i+1}) / 2 alone:
  "feasible"    one of a few thousand two-phase acceleration profiles (a_1..a_m = A, the rest B) meets every row with 1e-3 to spare;
  "infeasible"  a row contradicts, by more than 1e-3, the envelope of ALL profiles (a = 4 throughout from above, a = -6 throughout
                from below, s_i between the largest lower bound before it and the smallest upper bound behind it);
  "borderline"  neither: the tube, halt, and straddling cross cases by intent, a cap or a wall the two certificates cannot
                separate.  Nothing is claimed about these and nothing compares them with the oracle's label.

The yardstick is ``truth``: oracle.st_backend.speed_qp (the dense formulation, nothing of the project's solvers) at the nominal
bounds, at bounds widened by 1e-6 and at bounds tightened by 1e-6.  "feasible" if all three end optimal, "infeasible" if none
does, "borderline" otherwise; the sizes k = 0, 1, 16 are decided by rule (EMP_STB_NO_PROFILE, _QP_FAILED, _INDEX) and "rule" here."""
import collections
import functools

import numpy as np

from oracle import st_backend as be

NAN = np.nan
N_DP = 16
SIZES = (2, 3, 4, 5, 8, 15)             # 2: one free coefficient, no monotonicity row; 4: the first full band; 15: the largest
RULE_SIZES = (0, 1, 16)                 # no profile | dt = T / 0 | no NaN tail: the reference's IndexError
V0S = (0.0, 3.0, 12.0, 30.0, 60.0)      # standstill .. above the reference speed of 50 m/s
A_MIN, A_MAX = -6.0, 4.0
HUGE = 1.4e5                            # sqrt(0.2 g / 1e-10): the curvature bound of a straight, beyond the kernel's kSpeedBig
EPS = 1e-6                              # how far truth() widens and tightens the bounds
MARGIN = 1e-3                           # what a certificate of design_of must have to spare
W4 = np.array([10.0, 50.0, 500.0, 50.0])    # w_s_dot2, w_v_ref, w_jerk, v_ref (api.speed_qp_params(), the oracle's defaults)

Case = collections.namedtuple("Case", "name family k v0 a0 dp_s dp_t s_lb s_ub sd_lb sd_ub design")


def dt_of(k):
    return 0.5 * k / (k - 1)


def times(k):
    """Time of the station that column c bounds, c = 0 .. k-2."""
    return (np.arange(k - 1) + 1.0) * dt_of(k)


def used(k):
    return max(k - 1, 0) if k < N_DP else 0


def open_bounds(k):
    """s free, 0 <= s_dot on the used columns; everything behind them is filled in by ``cases`` (poison)."""
    n = used(k)
    s_lb, s_ub, sd_lb, sd_ub = np.full(N_DP, -np.inf), np.full(N_DP, np.inf), np.full(N_DP, -np.inf), np.full(N_DP, np.inf)
    sd_lb[:n] = 0.0
    return s_lb, s_ub, sd_lb, sd_ub


def wall_column(k):
    return min(k // 2, k - 2)


def _pick(i, j, count, step=2):
    """count start speeds for size index i and variant index j: a rotation, so that every speed meets every family and size class."""
    return [V0S[(i + j + step * n) % len(V0S)] for n in range(count)]


# ---------------------------------------------------------------------------------------------------------------------
# families: (size index i, k) -> [(suffix, v0, a0, (s_lb, s_ub, sd_lb, sd_ub))]
# ---------------------------------------------------------------------------------------------------------------------
OPEN_A0 = (0.0, 4.0, -6.0, 8.0, -9.0, -1.5)    # on and outside [-6, 4]: the start is pinned, not bounded


def _open(i, k):
    out = []
    for j, a0 in enumerate(OPEN_A0):
        # a0 = -1.5 from standstill: s_dot_1 >= 0 asks for a_1 >= 1.5, s_1 = dt^2 (a0 / 3 + a_1 / 6) >= 0 for a_1 >= 3 - the one
        # place where the row s_1 >= s_0 = 0 decides the answer (the jerk cost holds a_1 below 3 without it)
        v0s = [0.0] if a0 == -1.5 else _pick(i, 0 if a0 == 0.0 else j, 2)
        if a0 in (-6.0, -9.0) and 0.0 not in v0s:
            v0s.append(0.0)                        # s_dot_1 = dt (a0 + a_1) / 2 < 0 whatever a_1 <= 4 is: infeasible by dynamics
        out += [(f"a{a0:g}", v0, a0, open_bounds(k)) for v0 in v0s]
    return out


WALL_F = (2.0, 1.05, 0.5)


def _wall(i, k):
    """s <= d from column k // 2 on, d = f (v0^2 / 12 + v0 dt) + 0.5: f times the stopping distance at -6 m/s^2 plus one step."""
    out, dt = [], dt_of(k)
    for j, f in enumerate(WALL_F):
        for v0 in _pick(i, j + 1, 3):
            b = open_bounds(k)
            b[1][wall_column(k):k - 1] = f * (v0 * v0 / 12.0 + v0 * dt) + 0.5
            out.append((f"f{f:g}", v0, 0.0, b))
    return out


def _cap(i, k):
    """s_dot <= v0 + 1 (loose), v0 - 2 (reachable where 3 dt > 2), v0 - 6 dt - 1 (beyond -6 m/s^2), floored at 0."""
    out, dt = [], dt_of(k)
    for j, name in enumerate(("loose", "reach", "beyond")):
        for v0 in _pick(i, j + 2, 2):
            b = open_bounds(k)
            b[3][:k - 1] = max(0.0, (v0 + 1.0, v0 - 2.0, v0 - 6.0 * dt - 1.0)[j])
            out.append((name, v0, 0.0, b))
    return out


CHASE_G = (1.0, 3.5, 6.0)


def _chase(i, k):
    """s >= v0 t + 0.4 g t^2: a lower bound that pulls away at 0.8 g m/s^2 (g = 6: more than s_dot2 <= 4 gives)."""
    out, t = [], times(k)
    for j, g in enumerate(CHASE_G):
        for v0 in _pick(i, j + 3, 2):
            b = open_bounds(k)
            b[0][:k - 1] = v0 * t + 0.4 * g * t * t
            out.append((f"g{g:g}", v0, 0.0, b))
    return out


def _sandwich(i, k):
    """s_lb and s_ub ramps 2 m apart around the constant-speed profile: the speed cost pushes to one of them (upper below the
    reference speed, lower at v0 = 60), the monotonicity rows to the other at v0 = 0."""
    out, t = [], times(k)
    for v0 in _pick(i, 4, 3):
        b = open_bounds(k)
        b[0][:k - 1], b[1][:k - 1] = v0 * t - 1.0, v0 * t + 1.0
        out.append(("w2", v0, 0.0, b))
    return out


TUBE_W = (2e-2, 2e-6, 0.0)


def _tube(i, k):
    out, t = [], times(k)
    for j, w in enumerate(TUBE_W):
        for v0 in _pick(i, j, 1):
            b = open_bounds(k)
            b[0][:k - 1], b[1][:k - 1] = v0 * t - w / 2.0, v0 * t + w / 2.0
            out.append((f"w{w:g}", v0, 0.0, b))
    return out


CROSS_G = (1e-3, 1e-10, 1e-8)             # the kernel's own test is lo > hi + 1e-9


def cross_column(k):
    return (k - 1) // 2


def _cross(i, k):
    out, t = [], times(k)
    for j, g in enumerate(CROSS_G):
        for v0 in _pick(i, j + 1, 1):
            b = open_bounds(k)
            c = cross_column(k)
            b[1][c] = v0 * t[c]
            b[0][c] = b[1][c] + g
            out.append((f"g{g:g}", v0, 0.0, b))
    return out


def _halt(i, k):
    """v0 = 0 with s_ub = 0: the only feasible profile stands still (no interior)."""
    out = []
    for name, first in (("all", 0), ("late", wall_column(k))):
        b = open_bounds(k)
        b[1][first:k - 1] = 0.0
        out.append((name, 0.0, 0.0, b))
    return out


def _huge(i, k):
    """Finite bounds of +-1.4e5 where ``open`` has infinite ones (same start speeds as open_a0): the answer is open's."""
    out = []
    for v0 in _pick(i, 0, 2):
        b = open_bounds(k)
        n = k - 1
        b[0][:n], b[1][:n], b[3][:n] = -HUGE, HUGE, HUGE
        out.append(("b", v0, 0.0, b))
    return out


FAMILIES = {"open": _open, "wall": _wall, "cap": _cap, "chase": _chase, "sandwich": _sandwich, "tube": _tube, "cross": _cross,
            "halt": _halt, "huge": _huge}
DECIDED_BY_DESIGN = ("open", "wall", "cap", "chase", "sandwich", "huge", "cross")     # where design_of decides, the oracle must agree


# ---------------------------------------------------------------------------------------------------------------------
# what the construction decides without a solver
# ---------------------------------------------------------------------------------------------------------------------
def profile(v0, a0, dt, nodes):
    """nodes [C][k-1] = a_1 .. a_{k-1} -> s, s_dot, a [C][k] of the piecewise-linear-acceleration spline from (0, v0, a0)."""
    nodes = np.atleast_2d(np.asarray(nodes, dtype=np.float64))
    C, n = nodes.shape
    a = np.concatenate([np.full((C, 1), a0), nodes], axis=1)
    s, v = np.zeros((C, n + 1)), np.full((C, n + 1), float(v0))
    for i in range(n):
        s[:, i + 1] = s[:, i] + dt * v[:, i] + dt * dt * (a[:, i] / 3.0 + a[:, i + 1] / 6.0)
        v[:, i + 1] = v[:, i] + dt * (a[:, i] + a[:, i + 1]) / 2.0
    return s, v, a


def station_bounds(k, s_lb, s_ub, sd_lb, sd_ub):
    n = k - 1
    return s_lb[:n], s_ub[:n], sd_lb[:n], sd_ub[:n]


def slack(k, bounds, s, v, a):
    """The smallest slack over every row of the problem, per profile [C]: bounds of stations 1 .. k-1, -6 <= a <= 4, s_i >= s_{i-1}."""
    lo, hi, vlo, vhi = station_bounds(k, *bounds)
    rows = [s[:, 1:] - lo, hi - s[:, 1:], v[:, 1:] - vlo, vhi - v[:, 1:], a[:, 1:] - A_MIN, A_MAX - a[:, 1:], s[:, 1:] - s[:, :-1]]
    return np.min(np.concatenate(rows, axis=1), axis=1)


def _candidates(k, v0, a0):
    """Two-phase profiles: a_1 .. a_m = A, a_{m+1} .. = B.  A from a grid and from the values that end phase one at a small speed
    (a stop at a wall: brake, then creep); B from a grid that holds 0."""
    dt, n = dt_of(k), k - 1
    grid_a, grid_b = np.linspace(A_MIN, A_MAX, 41), np.linspace(A_MIN, A_MAX, 11)
    out = []
    for m in range(1, n + 1):
        stop = (np.array([0.002, 0.01, 0.05, 0.2, 1.0]) - v0 - dt * a0 / 2.0) / (m * dt)
        As = np.concatenate([grid_a, stop[(stop >= A_MIN) & (stop <= A_MAX)]])
        Bs = grid_b if m < n else grid_b[:1]
        A, B = np.meshgrid(As, Bs, indexing="ij")
        nodes = np.repeat(B.reshape(-1, 1), n, axis=1)
        nodes[:, :m] = A.reshape(-1, 1)
        out.append(nodes)
    return np.concatenate(out)


def design_of(k, v0, a0, bounds):
    if k in RULE_SIZES:
        return "rule"
    dt = dt_of(k)
    if slack(k, bounds, *profile(v0, a0, dt, _candidates(k, v0, a0))).max() >= MARGIN:
        return "feasible"
    lo, hi, vlo, vhi = station_bounds(k, *bounds)
    if (lo > hi + MARGIN / 10.0).any() or (vlo > vhi + MARGIN / 10.0).any():           # by inspection: an empty box
        return "infeasible"
    (s_up, v_up, _), (s_dn, v_dn, _) = (profile(v0, a0, dt, np.full((1, k - 1), a)) for a in (A_MAX, A_MIN))
    s_min = np.maximum.accumulate(np.maximum(np.maximum(s_dn[0], 0.0), np.concatenate([[0.0], lo])))[1:]   # s_i >= s_j, j <= i
    s_max = np.minimum(s_up[0, 1:], np.minimum.accumulate(hi[::-1])[::-1])                                  # s_i <= s_j, j >= i
    gap = max((s_min - s_max).max(), (np.maximum(vlo, v_dn[0, 1:]) - np.minimum(vhi, v_up[0, 1:])).max())
    return "infeasible" if gap > MARGIN else "borderline"


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: every family at every size, and the by-rule sizes 0, 1 and 16."""
    raw = []
    for i, k in enumerate(SIZES):
        for fam, make in FAMILIES.items():
            raw += [(f"{fam}_{suffix}_v{v0:g}_k{k}", fam, k, v0, a0, b) for suffix, v0, a0, b in make(i, k)]
    for k in RULE_SIZES:
        raw += [(f"rule_v{v0:g}_k{k}", "rule", k, v0, 0.0, open_bounds(k)) for v0 in (3.0, 12.0)]
    out = {}
    for idx, (name, fam, k, v0, a0, b) in enumerate(raw):
        assert name not in out, name
        dp_t = np.full(N_DP, NAN)
        dp_t[:k] = 0.5 * (np.arange(k) + 1.0)
        dp_s = np.where(np.isnan(dp_t), NAN, v0 * dp_t)
        b = [np.array(x, dtype=np.float64) for x in b]
        for x, crossed in zip(b, (5.0, -5.0, 3.0, -3.0)):             # columns the reference never reads
            x[used(k):] = crossed if idx % 2 == 0 else NAN
        out[name] = Case(name, fam, k, float(v0), float(a0), dp_s, dp_t, *b, design_of(k, v0, a0, b))
    return out


def names_of(family=None, k=None):
    return [c.name for c in cases().values() if family in (None, c.family) and k in (None, c.k)]


def _oracle(c, shift):
    s_lb, s_ub, sd_lb, sd_ub = c.s_lb - shift, c.s_ub + shift, c.sd_lb - shift, c.sd_ub + shift
    out, res, F = be.speed_qp(c.v0, c.a0, c.dp_s, c.dp_t, s_lb, s_ub, sd_lb, sd_ub)
    if res is None or res.status != "optimal":
        return None
    return np.stack(out[:3], axis=1)[:c.k]


@functools.lru_cache(maxsize=None)
def truth(name):
    """(label, x): "feasible" | "infeasible" | "borderline" | "rule", and the oracle's minimiser at the nominal bounds as
    [k][3] = s, s_dot, s_dot2 (None where it has none)."""
    c = cases()[name]
    if c.k in RULE_SIZES:
        return "rule", None
    n = c.k - 1
    narrow = min((c.s_ub[:n] - c.s_lb[:n]).min(), (c.sd_ub[:n] - c.sd_lb[:n]).min()) < 4.0 * EPS
    nominal = _oracle(c, 0.0)
    wide = _oracle(c, EPS)
    tight = None if narrow else _oracle(c, -EPS)
    found = [x is not None for x in (nominal, wide, tight)]
    return ("feasible" if all(found) else "borderline" if any(found) else "infeasible"), nominal


def arrays(names):
    """The batch of ``names``: v0, a0 [B] and dp_s, dp_t, s_lb, s_ub, sd_lb, sd_ub [B][16]."""
    cs = [cases()[n] for n in names]
    return [np.array([c.v0 for c in cs]), np.array([c.a0 for c in cs])] + \
           [np.stack([getattr(c, f) for c in cs]) for f in ("dp_s", "dp_t", "s_lb", "s_ub", "sd_lb", "sd_ub")]
