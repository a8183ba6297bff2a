"""NumPy port of the reference's feed-forward lateral MPC (controller/controller.py class
Lateral_MPC__with_feedforward_controller, :727-990) from explicit inputs, for the batch tests of emp_mpc_ff_lateral.  The box QP
is solved by oracle/qp_dense.py (the same solver the fixtures' stub cvxopt uses).  Test tool only: the package never imports it."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import qp_dense  # noqa: E402

N, P, NX = 4, 2, 4                       # :737-739
TS = 0.1


def ff_chain(vehicle_para, path, state, Vx, min_index, q_diag=(200.0, 1.0, 1.0, 1.0), f_diag=(10.0,) * 4, r=1.0):
    """One vehicle: path (n, 4), state (x, y, fi, Vy, fi_dot), unclamped Vx.  Returns a dict with H, f, u, steer, e_rr, k_r,
    min_index, pre_pro, or {"index_error": True} where the reference raises IndexError."""
    a, b, Cf, Cr, m, Iz = (float(v) for v in vehicle_para)
    x, y, fi, Vy, fi_dot = (float(v) for v in state)
    Vg = Vx + 0.0001                                        # :791
    A = np.zeros((4, 4))
    A[0][1] = 1
    A[1][1] = (Cf + Cr) / (m * Vg)
    A[1][2] = -(Cf + Cr) / m
    A[1][3] = (a * Cf - b * Cr) / (m * Vg)
    A[2][3] = 1
    A[3][1] = (a * Cf - b * Cr) / (Iz * Vg)
    A[3][2] = -(a * Cf - b * Cr) / Iz
    A[3][3] = (a * a * Cf + b * b * Cr) / (Iz * Vg)
    B = np.zeros((4, 1))
    B[1][0] = -Cf / m
    B[3][0] = -a * Cf / Iz
    C = np.zeros((4, 1))
    C[1][0] = (a * Cf + b * Cr) / (m * Vg) - Vg
    C[3][0] = (a ** 2 * Cf + b ** 2 * Cr) / (Iz * Vg)
    # prediction and match (:827-912): the whole path, strict <, min_index as the fallback
    x = x + Vx * TS * math.cos(fi) - Vy * TS * math.sin(fi)
    y = y + Vy * TS * math.cos(fi) + Vx * TS * math.sin(fi)
    fi = fi + fi_dot * TS
    min_d = 10000
    for i in range(len(path)):
        d = (path[i][0] - x) ** 2 + (path[i][1] - y) ** 2
        if d < min_d:
            min_d = d
            min_index = i
    if not 0 <= min_index < len(path):
        return {"index_error": True}
    px, py, pth, pk = (float(v) for v in path[min_index])
    tor = np.array([math.cos(pth), math.sin(pth)])
    nor = np.array([-math.sin(pth), math.cos(pth)])
    dv = np.array([x - px, y - py])
    e_d, e_s = float(nor @ dv), float(tor @ dv)
    pro = np.array([px, py]) + e_s * tor
    theta_r = pth + pk * e_s
    e_d_dot = Vy * math.cos(fi - theta_r) + Vx * math.sin(fi - theta_r)
    e_fi = fi - theta_r
    S_dot = (Vx * math.cos(fi - theta_r) - Vy * math.sin(fi - theta_r)) / (1 - pk * e_d)
    e_fi_dot = fi_dot - pk * S_dot
    e_rr = np.array([e_d, e_d_dot, e_fi, e_fi_dot])
    # discretisation (:811-822)
    temp = np.linalg.inv(np.eye(4) - (TS * A) / 2)
    A_bar = temp @ (np.eye(4) + (TS * A) / 2)
    B_bar = temp @ B * TS
    C_bar = temp @ C * TS * pk * Vx
    # condensed problem (:924-948)
    M = np.zeros(((N + 1) * NX, NX))
    Cm = np.zeros(((N + 1) * NX, N * P))
    M[0:NX] = np.eye(NX)
    for i in range(1, N + 1):
        M[i * NX:(i + 1) * NX] = A_bar @ M[(i - 1) * NX:i * NX]
    Cm[NX:2 * NX, 0:P] = B_bar
    for i in range(2, N + 1):
        Cm[i * NX:(i + 1) * NX, (i - 1) * P:i * P] = B_bar
        for j in range(i - 2, -1, -1):
            Cm[i * NX:(i + 1) * NX, j * P:(j + 1) * P] = A_bar @ Cm[i * NX:(i + 1) * NX, (j + 1) * P:(j + 2) * P]
    Cc = np.zeros(((N + 1) * NX, 1))
    for i in range(1, N + 1):
        Cc[NX * i:NX * (i + 1)] = A_bar @ Cc[NX * (i - 1):NX * i] + C_bar
    Q_bar = np.zeros(((N + 1) * NX, (N + 1) * NX))
    for i in range(N):
        Q_bar[i * NX:(i + 1) * NX, i * NX:(i + 1) * NX] = np.diag(q_diag)
    Q_bar[N * NX:, N * NX:] = np.diag(f_diag)
    R_bar = np.zeros((N * P, N * P))
    for i in range(P):
        R_bar[i * P:(i + 1) * P, i * P:(i + 1) * P] = np.eye(P) * r
    E = M.T @ Q_bar @ Cm
    H = 2 * (Cm.T @ Q_bar @ Cm + R_bar)
    f = (2 * E.T @ e_rr.reshape(NX, 1) + 2 * Cm.T @ Q_bar.T @ Cc).reshape(-1)
    G = np.concatenate((np.identity(N * P), -np.identity(N * P)))
    h = np.ones(2 * N * P)
    try:
        res = qp_dense.solve_qp(H, f, G, h)
    except np.linalg.LinAlgError:                           # singular reduced Hessian in the polish: the IPM point
        res = qp_dense.solve_qp(H, f, G, h, do_polish=False)
    return {"H": H, "f": f, "u": res.x, "steer": float(res.x[0]), "e_rr": e_rr, "k_r": pk, "min_index": min_index,
            "pre_pro": np.array([x, y, pro[0], pro[1]]), "qp_status": res.status}


def determined(u):
    """The part of a solution the singular QP determines: u0..u3 and the pair sums u4 + u5, u6 + u7."""
    u = np.asarray(u, dtype=np.float64)
    return np.concatenate([u[..., :4], u[..., 4:5] + u[..., 5:6], u[..., 6:7] + u[..., 7:8]], axis=-1)
