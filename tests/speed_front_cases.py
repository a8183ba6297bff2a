"""Adversarial inputs of the S-T speed front (emp_st_graph, emp_speed_dp, emp_st_edge_costs, emp_st_collision_cost,
emp_speed_start_condition) and their oracle truth (tests/test_speed_front_cases_host.py, tests/test_gpu_speed_front_batch.py).
A plain helper module (no fixtures, no hooks).

What feeds speed_dp_kernel elsewhere in the suite is generate_st_graph output of forward-moving obstacles.  ``dp_cases``
hands it segment sets directly, at the capacities around its 32 / 64-bit mask switch (``CAPS``):

  family       segments
  "axis"       t_in == t_out (the uy == 0 branch of st::reach_interval), s_in == s_out (ux == 0), a point (NaN frame), and
               segments whose ds or dt is 1e-9
  "reversed"   s_out < s_in, t_out < t_in, both
  "early"      wholly / partly at negative time (where sample 0 of the edges from the origin lies), through the origin (0, 0)
  "outside"    beyond the grid (s > 54.5, t > 8): within 1.5 of its border and far from it
  "exact"      stationary segments at exactly 0.5 and 1.5 from grid rows and from the origin (no cost in the reference)
  "ulp"        the same segments one ulp to either side (both sides of 0.5 cost, only the near side of 1.5)
  "live_*"     slot patterns: only slot 0 / the last / 31 / 32 / 63, alternating, every slot, none
  "nonfinite"  live slots (s_in not NaN) with s_out = inf / NaN, t_in = NaN, t_out = inf, s_in = +inf
  "dense"      many long overlapping segments: pair lists of several windows (kStListCap) per wavefront pass

Every scene has a poisoned twin (``poisoned``): the slots whose s_in is NaN carry NaN, +-inf or an obstacle on the scene's
own best path in their other three arrays.  The truth is oracle/st_speed.exact_speed_dp, computed once per process and
weight set on the live slots of each scene (``truth``): an absent slot adds an exact +0.0 to a sum of non-negative terms
that starts at +0.0, so leaving it out changes no bit (checked on the CPU in the host test).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import st_speed as st

NAN, INF = np.nan, np.inf
CAPS = (1, 16, 31, 32, 33, 64)
#: weight sets of the comparisons: "count" makes the obstacle term an exact count of pairs within reach (1 ** y == 1),
#: "ties" leaves nothing but that count (every cost a small integer, ties everywhere), "default" is the reference's
WEIGHTS = {"count": dict(w_cost_obs=1.0), "ties": dict(w_cost_obs=1.0, w_cost_ref_speed=0.0, w_cost_accel=0.0), "default": {}}
STARTS = (5.0, 0.0, -3.0, 12.0, 1e6, 8.0, INF, 20.0, NAN, 2.5, 15.0, 7.5)
S_LIST, T_LIST = st.grid()
S_ROW = S_LIST[::-1].copy()

up = lambda x: float(np.nextafter(x, INF))
down = lambda x: float(np.nextafter(x, -INF))


def _axis():
    return [(12.0, 19.0, 2.25, 2.25),              # t_in == t_out: uy == 0
            (22.0, 22.0, 0.5, 6.0),                # s_in == s_out: ux == 0
            (8.5, 8.5, 3.0, 3.0),                  # a point: NaN frame
            (30.0, 30.0 + 1e-9, 1.0, 5.0), (40.0, 47.0, 4.0, 4.0 + 1e-9), (3.0, 3.0 + 1e-9, 1.5, 1.5 + 1e-9),
            (26.5, 14.5, 5.5, 5.5)]                # uy == 0, reversed in s


def _reversed():
    return [(25.0, 11.0, 1.0, 6.0), (6.0, 21.0, 7.0, 2.0), (38.0, 19.0, 6.5, 0.75), (4.0, 0.5, 3.0, 0.25)]


def _early():
    return [(3.0, 9.0, -3.0, -1.0), (1.0, 14.0, -1.0, 2.5), (-4.0, 6.0, -2.0, 3.0), (-2.0, 2.0, -0.5, 0.5),
            (0.75, 0.75, -0.25, -0.25), (2.0, 0.25, -0.1, 0.6)]


def _outside():
    return [(55.5, 55.5, 0.0, 8.0), (50.0, 58.0, 8.5, 9.25), (30.0, 45.0, 9.4, 9.4), (56.25, 70.0, 2.0, 7.0),
            (200.0, 300.0, 1.0, 5.0), (10.0, 30.0, 40.0, 50.0), (-30.0, -2.0, 1.0, 7.0), (53.0, 57.0, 7.0, 9.0)]


#: (grid s, offset): a stationary obstacle at s + offset over t = 0 .. 8 is exactly |offset| from that row's nodes in every
#: column; s = 0 is both row 39 and the DP origin (sample 1 of the edges with source row 0)
EXACT_AT = ((10.5, 0.5), (10.5, 1.5), (22.0, -0.5), (22.0, -1.5), (0.0, 0.5), (0.0, 1.5), (3.0, -1.5), (47.0, 0.5), (34.5, -0.5),
            (0.0, -0.5), (0.0, -1.5), (6.5, 1.5))


def _exact():
    return [(s + o, s + o, 0.0, 8.0) for s, o in EXACT_AT]


def _ulp():
    out = []
    for i, (s, o) in enumerate(EXACT_AT):
        x = (up if i % 2 == 0 else down)(s + o)
        out.append((x, x, 0.0, 8.0))
    for i, (s, o) in enumerate(EXACT_AT):
        x = (down if i % 2 == 0 else up)(s + o)
        out.append((x, x, 0.0, 8.0))
    return out


def _nonfinite():
    return [(14.0, INF, 1.0, 4.0), (20.0, NAN, 2.0, 5.0), (9.0, 18.0, NAN, 3.0), (5.0, 16.0, 0.5, INF), (INF, 12.0, 1.0, 3.0),
            (INF, 27.5, 2.0, 2.0), (11.0, -INF, 3.0, 3.5), (17.5, 17.5, -INF, 2.0), (INF, INF, 1.0, 2.0), (7.0, 8.0, INF, INF)]


def _plain(rng, n):
    s_in = rng.uniform(2.0, 45.0, n)
    t_in = rng.uniform(0.0, 5.0, n)
    return [tuple(v) for v in np.stack([s_in, s_in + rng.uniform(2.0, 20.0, n), t_in, t_in + rng.uniform(1.0, 4.0, n)], 1)]


def _dense(rng, n):
    s_in = rng.uniform(0.0, 30.0, n)
    t_in = rng.uniform(-1.0, 3.0, n)
    return [tuple(v) for v in np.stack([s_in, s_in + rng.uniform(5.0, 30.0, n), t_in, t_in + rng.uniform(3.0, 8.0, n)], 1)]


SHAPES = {"axis": _axis, "reversed": _reversed, "early": _early, "outside": _outside, "exact": _exact, "ulp": _ulp,
          "nonfinite": _nonfinite}
DENSE_CAPS = (16, 33, 64)


def _place(cap, segs, rng, turn, extra=2):
    """The family's segments spread over the capacity's slots (the last slot taken whenever there are two or more), up to
    ``extra`` plain segments in between, NaN elsewhere.  A capacity with fewer slots than segments takes those from ``turn``
    on, so that the capacities share the variants out between them."""
    a = np.full((4, cap), NAN)
    k = min(len(segs), cap)
    segs = [segs[(turn + i) % len(segs)] for i in range(k)]
    at = np.unique(np.round(np.linspace(0, cap - 1, k)).astype(int)) if k > 1 else np.array([0 if turn % 2 == 0 else cap - 1])
    for slot, seg in zip(at, segs):
        a[:, slot] = seg
    free = np.setdiff1d(np.arange(cap), at)
    for slot, seg in zip(rng.permutation(free)[:extra], _plain(rng, extra)):
        a[:, slot] = seg
    return a


def _patterns(cap):
    pats = {"live_first": [0], "live_last": [cap - 1], "live_alternating": list(range(1, cap, 2)) or [0],
            "live_all": list(range(cap)), "live_none": []}
    for k in (31, 32, 63):
        if cap > k and k != cap - 1:
            pats[f"live_{k}"] = [k]
    return pats


@functools.lru_cache(maxsize=None)
def dp_cases(cap, seed=0):
    """(names, sets [4][B][cap] = s_in, s_out, t_in, t_out, start speeds [B]) of capacity ``cap``.  Cached: read-only."""
    rng = np.random.default_rng(1000 * seed + cap)
    turn = CAPS.index(cap) if cap in CAPS else cap
    names, scenes = [], []
    for name, make in SHAPES.items():
        names.append(name)
        scenes.append(_place(cap, make(), rng, turn))
    for name, live in _patterns(cap).items():
        a = np.full((4, cap), NAN)
        segs = _plain(rng, cap)
        for slot in live:
            a[:, slot] = segs[slot]
        names.append(name)
        scenes.append(a)
    if cap in DENSE_CAPS:
        names.append("dense")
        scenes.append(np.array(_dense(rng, cap)).T.copy())
    sets = np.ascontiguousarray(np.stack(scenes, axis=1))
    B = len(names)
    v0 = np.array([STARTS[(i + turn) % len(STARTS)] for i in range(B)])
    for i, n in enumerate(names):                      # the shape families keep a start that leaves the table finite
        if n in ("exact", "ulp", "dense", "axis") and not np.isfinite(v0[i]) or (n in ("exact", "ulp", "dense") and v0[i] > 1e3):
            v0[i] = 6.0 + i
    sets.setflags(write=False)
    v0.setflags(write=False)
    return tuple(names), sets, v0


def squeeze(sets_b):
    """The live slots of one scene [4][cap], in order (one NaN slot if none is live)."""
    live = ~np.isnan(sets_b[0])
    return sets_b[:, live] if live.any() else np.full((4, 1), NAN)


def oracle_dp(sets, v0, pow_route=None, **weights):
    """exact_speed_dp scene by scene on the live slots: dict of stacked arrays."""
    outs = [st.exact_speed_dp(*[x[None] for x in squeeze(sets[:, b])], v0[b:b + 1], pow_route=pow_route, **weights)
            for b in range(sets.shape[1])]
    if not outs:
        outs = [st.exact_speed_dp(*np.full((4, 0, 1), NAN), np.zeros(0), **weights)]
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


@functools.lru_cache(maxsize=None)
def truth(cap, weights="default", pow_route=None, seed=0):
    _, sets, v0 = dp_cases(cap, seed)
    out = oracle_dp(sets, v0, pow_route, **WEIGHTS[weights])
    for a in out.values():
        a.setflags(write=False)
    return out


def best_path_point(t, col=3):
    """(s, t) of every scene's best path in column ``col`` (or its terminal column if that comes first); (10.5, 2.0) where the
    scene has no path."""
    s = np.full(len(t["end"]), 10.5)
    tt = np.full(len(t["end"]), 2.0)
    for b, (r, c) in enumerate(t["end"]):
        if r >= 0:
            c = min(int(c), col)
            s[b], tt[b] = t["speed_s"][b, c], t["speed_t"][b, c]
    return s, tt


@functools.lru_cache(maxsize=None)
def poisoned(cap, seed=0):
    """dp_cases' sets with the other three arrays of every absent slot (s_in NaN) filled, by turns: NaN; +inf / -inf; a
    stationary obstacle across the scene's own default-weight best path (live, it would sit on a node of that path)."""
    _, sets, _ = dp_cases(cap, seed)
    ps, pt = best_path_point(truth(cap, "default", None, seed))
    out = sets.copy()
    for b in range(sets.shape[1]):
        for j in np.flatnonzero(np.isnan(sets[0, b])):
            kind = (j + b) % 3
            if kind == 0:
                out[1:, b, j] = NAN
            elif kind == 1:
                out[1:, b, j] = (INF, -INF, INF) if j % 2 else (-INF, INF, -INF)
            else:
                out[1:, b, j] = (ps[b], pt[b] - 0.25, pt[b] + 0.25)
    out.setflags(write=False)
    return out


def hostile_slots(cap, seed=0):
    """[(scene, slot)] of the absent slots that ``poisoned`` fills with an obstacle on the path."""
    _, sets, _ = dp_cases(cap, seed)
    return [(b, int(j)) for b in range(sets.shape[1]) for j in np.flatnonzero(np.isnan(sets[0, b])) if (j + b) % 3 == 2]


def hostile_guard_row(cap):
    """A finite obstacle row for the guard rows around a batch: segments across the middle of the grid."""
    j = np.arange(cap, dtype=np.float64)
    return np.stack([4.0 + 0.7 * j, 9.0 + 0.7 * j, 0.25 + 0.1 * j, 3.0 + 0.1 * j])


# ---- beyond 512 scenes (the launcher runs the heaviest scenes first), with 64-bit masks ------------------------------------
BIG_B, BIG_CAP = 513, 40
#: the scenes of ``big_batch`` compared with the oracle: the two dense scenes (33 slots; the first 40 of 64), their perturbed
#: copies, four others and the last scene
BIG_SAMPLE = (13, 28, 42, 57, 130, 260, 390, 512)


@functools.lru_cache(maxsize=None)
def big_batch(seed=5):
    """(sets [4][513][40], start speeds): the scenes of dp_cases(33) and dp_cases(64) - their live segments, the first 40 of
    them, in random slots - and then copies of them with every finite value moved by N(0, 0.25).  0 .. 40 live slots."""
    rng = np.random.default_rng(seed)
    pool = []
    for cap in (33, 64):
        _, sets, v0 = dp_cases(cap)
        pool += [(sets[:, b][:, ~np.isnan(sets[0, b])][:, :BIG_CAP], v0[b]) for b in range(sets.shape[1])]
    out = np.full((4, BIG_B, BIG_CAP), NAN)
    v = np.zeros(BIG_B)
    for b in range(BIG_B):
        seg, v[b] = pool[b % len(pool)]
        if b >= len(pool):
            seg = np.where(np.isfinite(seg), seg + rng.normal(0.0, 0.25, seg.shape), seg)
            if np.isfinite(v[b]):
                v[b] += rng.uniform(-1.0, 1.0)
        out[:, b, np.sort(rng.choice(BIG_CAP, seg.shape[1], replace=False))] = seg
    out.setflags(write=False)
    v.setflags(write=False)
    return out, v


@functools.lru_cache(maxsize=None)
def big_truth(pow_route=None):
    sets, v = big_batch()
    pick = list(BIG_SAMPLE)
    return oracle_dp(sets[:, pick], v[pick], pow_route)


# ---- the kernel's pair lists, counted on the CPU --------------------------------------------------------------------------
def oracle_distance(s, t, s_in, s_out, t_in, t_out):
    """Distance of the point (s, t) from a segment by the oracle's expressions (oracle/st_speed.exact_pair_costs)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        v1x, v1y = s_in - s, t_in - t
        v2x, v2y = s_out - s, t_out - t
        v3x, v3y = v2x - v1x, v2y - v1y
        p = v1x * v3x + v1y * v3y
        q = v2x * v3x + v2y * v3y
        d11 = v1x * v1x + v1y * v1y
        d22 = v2x * v2x + v2y * v2y
        ends = np.sqrt(np.where(d22 < d11, d22, d11))
        perp = np.abs(v1x * v3y - v1y * v3x) / np.sqrt(v3x * v3x + v3y * v3y)
        return np.where(((p > 0) & (q > 0)) | ((p < 0) & (q < 0)), ends, perp)


def costly_pairs(sets_b, w_cost_obs=10000000):
    """Costly (sample, obstacle) pairs of every edge of one scene that go through speed_dp_kernel's pair lists: bool
    [16 columns][40 destination rows j][40 source rows k][4 samples (0, 2, 3, 4)][n_obs].  Sample 1 is the source node (the
    kernel takes it from its node table, not from a list).  Column 0 has only the edges from the origin, k == 0."""
    o = squeeze(sets_b)[:, None, None, :]
    out = np.zeros((st.N_COLS, st.N_ROWS, st.N_ROWS, 4, o.shape[-1]), bool)
    for c in range(st.N_COLS):
        s0 = np.broadcast_to(S_ROW[None, :], (st.N_ROWS, st.N_ROWS)).copy()
        t0 = np.full((st.N_ROWS, st.N_ROWS), T_LIST[c - 1] if c else 0.0)
        s0[:, 0] = 0.0
        t0[:, 0] = 0.0
        s1 = np.broadcast_to(S_ROW[:, None], (st.N_ROWS, st.N_ROWS))
        pairs = st.exact_pair_costs(s0, t0, s1, T_LIST[c], *o, w_cost_obs)       # [5][j][k][n_obs]
        out[c] = np.moveaxis(pairs[[0, 2, 3, 4]] != 0.0, 0, 2)
        if c == 0:
            out[c, :, 1:] = False
    return out


def list_passes(costly):
    """Per (column, pass, wavefront) of speed_dp_kernel, from ``costly_pairs``: the number of costly pairs, and whether some
    lane's run of pairs crosses a multiple of ``window`` in the wavefront's list.  The lane mapping is the kernel's
    (csrc/emp_st_kernels.h, "Mapping: lane = (kb, j) ..."): thread tid has destination row j = tid % 40, takes the source rows
    tid / 40 + 8 i in its passes i = 0 .. 4 and belongs to wavefront tid / 64; a lane's pairs follow those of the lower lanes
    of its wavefront.  Every costly pair lies inside its reach interval (tests/test_host_logic.py), so these counts are lower
    bounds of the kernel's list lengths.  Returns (counts [16][5][5], per-lane counts [16][5][320])."""
    tid = np.arange(320)
    j, kb = tid % 40, tid // 40
    per_lane = np.zeros((st.N_COLS, 5, 320), np.int64)
    n = costly.sum(axis=(3, 4))                         # [c][j][k]
    for i in range(5):
        per_lane[:, i] = n[:, j, kb + 8 * i]
    return per_lane.reshape(st.N_COLS, 5, 5, 64).sum(axis=3), per_lane


def straddles(per_lane, window=256):
    """True if, in some wavefront pass, a lane's pairs begin before a multiple of ``window`` and end after it."""
    x = per_lane.reshape(-1, 64)
    end = np.cumsum(x, axis=1)
    begin = end - x
    return bool(((begin // window) != ((end - 1) // window))[x > 0].any())


# ---- emp_st_graph ---------------------------------------------------------------------------------------------------------
L_DOTS = (0.0, 0.3, -0.3, 0.29999999999999993, -0.29999999999999993, NAN, INF, -INF, 1.0, -1.0, 0.5, -2.0, 4.0, 0.31)


@functools.lru_cache(maxsize=None)
def graph_cases(B, cap, seed=0):
    """obs_s, obs_l, obs_s_dot, obs_l_dot [4][B][cap]: rows whose first NaN s sits at slot 0, in the middle or nowhere, with
    finite data, inf and NaN behind it; l_dot around the 0.3 threshold and non-finite; l = +-2 exactly (t_min == 0: the else
    branch); t_max == 1 and t_min == 8 exactly (both kept); negative s_dot (reversed segments); s, l, s_dot = +-inf."""
    rng = np.random.default_rng(7000 + 10 * B + cap + seed)
    s = rng.uniform(0.0, 50.0, (B, cap))
    l = rng.uniform(-6.0, 6.0, (B, cap))
    sd = rng.uniform(-6.0, 12.0, (B, cap))
    ld = rng.choice(np.array(L_DOTS), (B, cap))
    ld = np.where(rng.uniform(size=(B, cap)) < 0.4, np.where(l > 0, -1.0, 1.0) * rng.uniform(0.3, 3.0, (B, cap)), ld)
    kind = rng.integers(0, 10, (B, cap))
    l = np.where(kind == 0, 2.0, np.where(kind == 1, -2.0, l))                    # t_min == 0 or t_max == 0 exactly
    # l_dot = +-1, +-0.5, +-2 and l a multiple of 0.5 keep every quotient exact: t_min / t_max land on 0, 1 and 8 themselves
    ex = kind == 2
    l = np.where(ex, rng.choice(np.array([1.0, -1.0, 3.0, -3.0, 6.0, -6.0, 10.0, -10.0, 2.5, -2.5]), (B, cap)), l)
    ld = np.where(ex, rng.choice(np.array([1.0, -1.0, 0.5, -0.5, 2.0, -2.0]), (B, cap)), ld)
    for arr, k in ((s, 3), (l, 4), (sd, 5)):
        arr[kind == k] = rng.choice(np.array([INF, -INF]), int((kind == k).sum()))
    # the first NaN s: a third of the rows at slot 0 (where there is more than one row), a third in the middle, a third nowhere
    for b in range(B):
        where = b % 3
        if where == 2:
            continue
        cut = 0 if where == 0 else int(rng.integers(0, cap))
        s[b, cut] = NAN
        behind = slice(cut + 1, cap)
        mode = (b // 3) % 3
        if mode == 1:                                   # live-looking data stays behind the first NaN
            for arr in (s, l, sd, ld):
                arr[b, behind] = rng.choice(np.array([INF, -INF, NAN]), cap - cut - 1)
        elif mode == 2:
            s[b, behind] = np.where(rng.uniform(size=cap - cut - 1) < 0.5, NAN, s[b, behind])
    out = np.ascontiguousarray(np.stack([s, l, sd, ld]))
    out.setflags(write=False)
    return out


GRAPH_DP = (64, 16)


@functools.lru_cache(maxsize=None)
def graph_dp_inputs():
    """generate_st_graph's own output on graph_cases(64, 16) as the speed DP's input: (sets [4][64][16], start speeds)."""
    sets = np.ascontiguousarray(np.stack(st.exact_generate_st_graph(*graph_cases(*GRAPH_DP))))
    finite = [v for v in STARTS if np.isfinite(v) and abs(v) < 1e3]
    v0 = np.array([finite[b % len(finite)] for b in range(sets.shape[1])])
    return sets, v0


@functools.lru_cache(maxsize=None)
def graph_dp_truth(weights="default", pow_route=None):
    return oracle_dp(*graph_dp_inputs(), pow_route, **WEIGHTS[weights])


def graph_exact_rows():
    """Hand-built slots (one row of 12): (s, l, s_dot, l_dot) whose t_min / t_max hit the thresholds exactly."""
    rows = [(10.0, 2.0, 3.0, -1.0),      # b1 = -2 + 2 = 0, b2 = 2 + 2 = 4: t_min == 0 -> else branch
            (10.0, -2.0, 3.0, 1.0),      # b1 = 2 + 2 = 4, b2 = 0
            (10.0, -2.0, -3.0, -1.0),    # t_max == 0: dropped (t_max < 1)
            (10.0, 1.0, 2.0, 1.0),       # t_zero = -1: b1 = 1, b2 = -3: t_max == 1.0 exactly, kept, inside
            (10.0, 10.0, 2.0, -1.0),     # t_zero = 10: b1 = 8, b2 = 12: t_min == 8.0 exactly, kept
            (10.0, 10.5, 2.0, -1.0),     # t_min = 8.5: dropped
            (30.0, 0.0, -4.0, 0.5),      # reversed segment: s_dot < 0
            (30.0, 0.0, -4.0, 0.3), (30.0, 0.0, -4.0, -0.3), (30.0, 0.0, 4.0, 0.29999999999999993),
            (5.0, 0.0, 1.0, INF), (5.0, 1.0, 1.0, NAN)]
    return np.ascontiguousarray(np.array(rows).T[:, None, :])


# ---- emp_st_edge_costs ----------------------------------------------------------------------------------------------------
EDGE_CAPS = (1, 32, 33, 64)
N_EDGES = 200


@functools.lru_cache(maxsize=None)
def edge_cases(cap, seed=0):
    """(edges [8][200][5] = s0, t0, v0, s1, t1; sets [4][8][cap]) against eight of dp_cases' segment sets."""
    names, sets, v0 = dp_cases(cap, seed)
    want = ["axis", "reversed", "early", "outside", "exact", "ulp", "nonfinite", "dense" if "dense" in names else "live_all"]
    pick = [names.index(n) for n in want]
    sets = np.ascontiguousarray(sets[:, pick])
    rng = np.random.default_rng(9000 + cap + seed)
    E = np.zeros((len(pick), N_EDGES, 5))
    for b in range(len(pick)):
        live = squeeze(sets[:, b])
        seg = live[:, rng.integers(0, live.shape[1], N_EDGES)]          # a segment of the scene per edge: s_in, s_out, t_in, t_out
        seg = np.where(np.isfinite(seg), seg, 10.0)
        for e in range(N_EDGES):
            kind = e % 10
            c = int(rng.integers(1, 16))
            si, so, ti, to = seg[:, e]
            if kind == 0:                                               # a grid edge
                row = (S_ROW[rng.integers(0, 40)], T_LIST[c - 1], rng.uniform(0, 20), S_ROW[rng.integers(0, 40)], T_LIST[c])
            elif kind == 1:                                             # an edge from the origin
                row = (0.0, 0.0, v0[pick[b]] if np.isfinite(v0[pick[b]]) else 4.0, S_ROW[rng.integers(0, 40)], T_LIST[c - 1])
            elif kind == 2:                                             # t1 == t0: division by zero
                row = (si, T_LIST[c], 3.0, si + rng.uniform(-2, 2), T_LIST[c])
            elif kind == 3:                                             # t1 < t0
                row = (S_ROW[rng.integers(0, 40)], T_LIST[c], 5.0, S_ROW[rng.integers(0, 40)], T_LIST[c - 1])
            elif kind == 4:                                             # s1 == s0
                s = si + rng.uniform(-2, 2)
                row = (s, ti + rng.uniform(-1, 1), 0.0, s, ti + rng.uniform(1, 2))
            elif kind == 5:                                             # exactly along the segment
                row = (si, ti, 2.0, so, to)
            elif kind == 6:                                             # samples 0.5 / 1.5 beside a stationary segment (exact in "exact")
                off = (0.5, -0.5, 1.5, -1.5)[(e // 10) % 4]
                row = (si - off, T_LIST[c - 1], 0.0, si - off, T_LIST[c])
            elif kind == 7:                                             # near the segment, at random
                row = (si + rng.uniform(-2, 2), ti + rng.uniform(-1, 1), rng.uniform(0, 10), so + rng.uniform(-2, 2), to + rng.uniform(-1, 1))
            elif kind == 8:                                             # huge coordinates
                row = (rng.choice([1e150, -1e150, 1e300, 1e9]), rng.uniform(0, 8), 1.0, rng.choice([1e150, 3.0, -1e300]), rng.choice([1e200, 4.0]))
            else:                                                       # non-finite coordinates, one member at a time
                row = [si, ti, 1.0, so, to + 0.5]
                row[(e // 10) % 5] = (INF, -INF, NAN)[(e // 50) % 3]
            E[b, e] = row
    E.setflags(write=False)
    sets.setflags(write=False)
    return E, sets


def oracle_edges(E, sets, **weights):
    """exact_edge_cost(..., with_parts=True) of edge_cases' edges, scene by scene on the live slots: total, obs [B][n_edges]."""
    tot, obs = np.zeros(E.shape[:2]), np.zeros(E.shape[:2])
    for b in range(E.shape[0]):
        o = squeeze(sets[:, b])[:, None, :]
        e = E[b]
        with np.errstate(over="ignore"):
            tot[b], obs[b] = st.exact_edge_cost(e[:, 0], e[:, 1], e[:, 2], e[:, 3], e[:, 4], *o, with_parts=True, **weights)
    return tot, obs


@functools.lru_cache(maxsize=None)
def edge_truth(cap, weights="default"):
    out = oracle_edges(*edge_cases(cap), **WEIGHTS[weights])
    for a in out:
        a.setflags(write=False)
    return out


# ---- the two small entry points -------------------------------------------------------------------------------------------
SMALL_N = (0, 1, 63, 64, 65, 1000)


def collision_distances(n):
    edge = []
    for x in (0.5, 1.5):
        edge += [x, -x, up(x), down(x), -up(x), -down(x)]
    edge += [0.0, -0.0, NAN, INF, -INF, 1e-300, 1.0, -1.0, 0.75, -1.25, 2.0, -7.0, 1e300]
    rng = np.random.default_rng(31)
    d = rng.uniform(-2.5, 2.5, max(n, 1))
    k = min(n, len(edge))
    d[:k] = edge[:k]
    if n > len(edge):
        d[-len(edge):] = edge[::-1]
    return d[:n].copy()


def in_band(d):
    a = np.abs(d)
    return (0.5 < a) & (a < 1.5)


def start_condition_inputs(n):
    rng = np.random.default_rng(32)
    m = max(n, 1)
    v = rng.uniform(-20, 20, (4, m))
    h = rng.uniform(-np.pi, np.pi, m)
    special = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1e6, NAN, -0.0, 1e-300, 3.0]
    k = min(m, len(special))
    h[:k] = special[:k]
    if m > len(special):
        h[-len(special):] = special
    return [np.ascontiguousarray(a[:n]) for a in (*v, h)]


def start_condition_truth(vx, vy, ax, ay, h):
    ld = np.longdouble
    c, s = np.cos(ld(1) * h.astype(ld)), np.sin(h.astype(ld))
    return c * vx + s * vy, c * ax + s * ay
