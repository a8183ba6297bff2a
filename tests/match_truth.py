"""What oracle/ref_port.py answers on the tables of tests/match_cases.py, computed once and shared by the CPU and the GPU suite
of the match scans: the Frenet outputs of a whole-line case in every role of the projection (origin of the s axis, planning
start, obstacle), the same outputs with the match FORCED to another index (for the margins the CPU suite checks), and the
reference line of every window case."""
from __future__ import annotations

import functools
import math
import struct

import numpy as np

from oracle import ref_port as op
from tests import match_cases as M

#: role of the case's query in a projection scene, and the width of the scene's obstacle row (filled to capacity)
ROLES = (("origin", 8), ("start", 8), ("obs_slot0", 8), ("obs_slot64", 65), ("obs_last", 63))
START_V, START_A = (5.0, 0.7), (0.3, -0.2)


def node_list(nodes):
    return [tuple(float(v) for v in r) for r in nodes]


def chord_sums(nodes):
    """The running chord length of cal_s_map_fun (planning_utils.py:461-466), before the origin is subtracted."""
    acc = [0.0]
    for i in range(1, len(nodes)):
        acc.append(math.sqrt((nodes[i][0] - nodes[i - 1][0]) ** 2 + (nodes[i][1] - nodes[i - 1][1]) ** 2) + acc[-1])
    return acc


def scene(c, role):
    """The projection scene in which `role` takes the case's query; every other point sits on the labelled node (distance 0: its match
    is that node whatever the scan does on a tie or at a stop, unless the node is NaN)."""
    benign = np.array(c["nodes"][c["label"], :2])
    q = np.array(c["q"])
    mo = dict(ROLES)[role]
    obs = np.tile(benign, (mo, 1))
    if role.startswith("obs"):
        obs[{"obs_slot0": 0, "obs_slot64": 64, "obs_last": mo - 1}[role]] = q
    return dict(origin=q if role == "origin" else benign, start=q if role == "start" else benign, obs=obs, n_obs=mo)


def _key(p):
    return struct.pack("<2d", float(p[0]), float(p[1]))


def _s_l(nodes, sm, pts):
    """cal_s_l_fun on pts; a point's s depends on its own match and its l on the first point's (planning_utils.py:413), so equal
    points are evaluated once.  Where a projection is infinite (an infinite coordinate) the reference's math.sin raises
    ValueError for the whole list; IEEE arithmetic, and the library, answer NaN for that point's l and go on: the other points
    are then evaluated one by one, by the same formulas (:414-424, :439-443, :499-507)."""
    first, seen, s_out, l_out = tuple(pts[0]), {}, [], []
    for p in pts:
        k = _key(p)
        if k not in seen:
            try:
                s, l = op.cal_s_l_fun([first, tuple(p)], nodes, sm)
                seen[k] = (s[1], l[1])
            except ValueError:
                match, _ = op.match_projection_points([first, tuple(p)], nodes)
                px, py, theta, _ = op._project_on(nodes[match[0]], p[0], p[1])
                l = float("nan")
                if math.isfinite(theta):
                    l = np.dot(np.array([p[0], p[1]]) - np.array([px, py]), np.array([-math.sin(theta), math.cos(theta)]))
                seen[k] = (op.cal_projection_s_fun(nodes, [match[1]], [tuple(p)], sm)[0], l)
        s_out.append(seen[k][0])
        l_out.append(seen[k][1])
    return np.array(s_out, np.float64), np.array(l_out, np.float64)


def project(nodes, origin, start, obs):
    """The five outputs of emp_frenet_project from the port (test_9.py:113-177)."""
    with np.errstate(all="ignore"):
        sm = op.cal_s_map_fun(nodes, tuple(origin))
        obs_s, obs_l = _s_l(nodes, sm, [tuple(p) for p in obs])
        st = tuple(float(v) for v in start)
        bs, bl = _s_l(nodes, sm, [st])
        try:
            l0, _, _, _, dl0, _, ddl0 = op.cal_s_l_deri_fun([st], [START_V], [START_A], nodes, st)
        except ValueError:
            l0 = dl0 = ddl0 = [float("nan")]
    return dict(s_map=np.asarray(sm, np.float64), obs_s=obs_s, obs_l=obs_l, begin=np.array([bs[0], bl[0]], np.float64),
                start=np.array([bs[0], l0[0], dl0[0], ddl0[0]], np.float64))


@functools.lru_cache(maxsize=None)
def projection_truth(role):
    """project() for every whole-line case with the query in `role`; read-only."""
    out = []
    for c in M.whole_line():
        sc = scene(c, role)
        out.append(project(node_list(c["nodes"]), sc["origin"], sc["start"], sc["obs"]))
    return tuple(out)


def forced(c, idx):
    """What the port computes from the case's query when the match is `idx` instead of what the scan finds: the s_map with the query
    as origin, and (s, l) of the query as an obstacle or planning start when the origin sits on the labelled node, as in scene()."""
    nodes = node_list(c["nodes"])
    q = tuple(float(v) for v in c["q"])
    acc = chord_sums(nodes)
    with np.errstate(all="ignore"):
        s0 = op.cal_projection_s_fun(nodes, [idx], [q], acc)[0]           # the query as origin of the s axis
        sm = list(np.array(acc) - acc[c["label"]])           # the origin on the labelled node projects on it with ds = 0
        s = op.cal_projection_s_fun(nodes, [idx], [q], sm)[0]
        pr = op._project_on(nodes[idx], q[0], q[1])
        l = float(np.dot(np.array(q) - np.array(pr[:2]), np.array([-math.sin(pr[2]), math.cos(pr[2])])))
    return dict(s_map=np.array(acc) - s0, s=float(s), l=l)


@functools.lru_cache(maxsize=None)
def window_truth():
    """Per window case: (status, n_ref, ref_line [51][4]) - smooth_reference_line(sampling(label, nodes)), or the zero line of a path
    shorter than 51 nodes.  Cases that share a path and a window share the line."""
    lines, out = {}, []
    for c in M.window():
        if c["first"] is None:
            out.append((2, 0, np.zeros((M.REF_POINTS, 4))))
            continue
        key = (c["G"], c["first"])
        if key not in lines:
            win = op.sampling(c["label"], node_list(c["path"]))
            line, status = op.smooth_reference_line([(n[0], n[1]) for n in win], _return_status=True)
            assert status == "optimal", (c["name"], status)
            lines[key] = np.array(line, np.float64)
        out.append((0, M.REF_POINTS, lines[key]))
    return tuple(out)
