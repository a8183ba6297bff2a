"""Labels for tests/lateral_cases.py from the oracles alone: oracle/mpc_lateral.py with oracle/qp_dense.py (MPC),
tests/control_port.ff_chain (feed-forward MPC) and oracle/lqr_lateral.py (LQR).  Nothing of the package is imported.  A helper
module (no fixtures, no hooks); labels are computed once per process.

``label(law, pset, i)`` returns a dict.  ``decided`` is True when the oracle's e_rr and (H, f) (LQR: K and steer) are finite and,
for the two MPCs, qp_dense ends ``optimal`` and kkt_certificate confirms its point (stationarity and violation below CERT).
Finite outputs mean finite inputs with one exception, which the host test pins by name: a path point whose x or y is NaN or
+-inf is at no distance ``<`` anything, so every law, the reference included, passes over it and matches its finite neighbour.
A decided case carries min_index, e_rr, and H, f, u, n_bound (controls at a bound), lam_min (smallest
eigenvalue of H) or K, sweeps, steer, last_deltas (max|dP| at the sweep before the last and at the last)."""
import functools

import numpy as np

from oracle import lqr_lateral as lq
from oracle import mpc_lateral as mpc
from oracle import qp_dense
from tests import control_port as port
from tests import lateral_cases as F

CERT = 1e-8                 # solve_qp's own bar for "optimal"
AT_BOUND = 1e-7             # the active-set tolerance of qp_dense


def _certified(H, f, u, status):
    n = len(f)
    G = np.concatenate((np.identity(n), -np.identity(n)))
    cert = qp_dense.kkt_certificate(H, f, G, np.ones(2 * n), None, None, u)
    return status == "optimal" and cert["stationarity"] < CERT and cert["ineq_violation"] < CERT


def _mpc(c):
    para, q, fd, r = F.params("mpc", c.pset)
    path = c.path[:c.n_path]
    A, B, C = mpc.continuous_model(para, c.vx)
    e_rr, k_r, idx, _, _ = mpc.tracking_error(path, tuple(c.state), c.vx, c.min_index)
    Ab, Bb, Cb = mpc.discretise(A, B, C, k_r, c.vx)
    H, f = mpc.condensed_qp(Ab, Bb, Cb, e_rr, Q=np.diag(q), R=r, F=np.diag(fd))
    out = dict(min_index=idx, e_rr=np.array(e_rr, dtype=np.float64), H=H, f=f.reshape(-1))
    if not (np.isfinite(out["e_rr"]).all() and np.isfinite(H).all() and np.isfinite(f).all()):
        return out
    u, res = mpc.solve_box_qp(H, f)
    out.update(u=np.asarray(u).reshape(-1), qp_status=res.status)
    return out


def _ff(c):
    para, q, fd, r = F.params("ff", c.pset)
    return port.ff_chain(para, c.path[:c.n_path], c.state, c.vx, c.min_index, q_diag=q, f_diag=fd, r=r)


@functools.lru_cache(maxsize=None)
def riccati(pset, vx):
    """oracle.lqr_lateral.riccati_gain, which is checked to return the same K and sweeps, with max|dP| of every sweep kept."""
    para, q, _, r = F.params("lqr", pset)
    with np.errstate(all="ignore"):
        Ac, Bc = lq.continuous_model(para, vx)
        K, sweeps = lq.riccati_gain(Ac, Bc, Q=np.diag(q), R=r)
        Q = np.diag(q)
        P = P_pre = Q
        temp = np.linalg.inv(np.eye(4) - (lq.TS * Ac) / 2)
        A = temp @ (np.eye(4) + (lq.TS * Ac) / 2)
        B = temp @ Bc * lq.TS
        deltas = []
        for _ in range(lq.MAX_ITR):
            P = A.T @ P @ A - (A.T @ P @ B) @ np.linalg.inv(r + B.T @ P @ B) @ (B.T @ P @ A) + Q
            deltas.append(float(abs(P - P_pre).max()))
            if deltas[-1] < lq.EPS:
                break
            P_pre = P
    assert len(deltas) == sweeps, (pset, vx)
    return K, sweeps, tuple(deltas[-2:]) if len(deltas) > 1 else (np.inf, deltas[-1])


def _lqr(c):
    para = F.params("lqr", c.pset)[0]
    K, sweeps, last = riccati(c.pset, c.vx)
    e_rr, k_r, idx, _, _ = lq.tracking_error(c.path[:c.n_path], tuple(c.state), c.vx, c.min_index)
    steer = -np.dot(K, np.array(e_rr)) + lq.feed_forward(para, K, k_r, c.vx)
    return dict(min_index=idx, e_rr=np.array(e_rr, dtype=np.float64), K=np.asarray(K).reshape(-1), sweeps=sweeps,
                steer=float(steer[0]), last_deltas=last)


@functools.lru_cache(maxsize=None)
def label(law, pset, i):
    c = F.table(law)[pset][i]
    out = dict(decided=False, finite_inputs=F.inputs_finite(c))
    try:
        with np.errstate(all="ignore"):
            out.update({"mpc": _mpc, "ff": _ff, "lqr": _lqr}[law](c))
    except (ZeroDivisionError, IndexError, np.linalg.LinAlgError, ValueError, OverflowError) as e:
        out["raised"] = type(e).__name__                   # where the reference itself raises: nothing to compare with
        return out
    if out.get("index_error"):
        return out
    if law == "lqr":
        out["decided"] = bool(np.isfinite(out["e_rr"]).all() and np.isfinite(out["K"]).all() and np.isfinite(out["steer"]))
        return out
    if "u" not in out or not (np.isfinite(out["e_rr"]).all() and np.isfinite(out["H"]).all() and np.isfinite(out["f"]).all()):
        return out
    out["decided"] = bool(_certified(out["H"], out["f"], out["u"], out["qp_status"]))
    out["n_bound"] = int((np.abs(out["u"]) >= 1.0 - AT_BOUND).sum())
    out["lam_min"] = float(np.linalg.eigvalsh((out["H"] + out["H"].T) / 2.0).min())
    return out


def labels(law, pset):
    return [label(law, pset, i) for i in range(len(F.table(law)[pset]))]


def objective(H, f, u):
    return float(0.5 * u @ H @ u + f @ u)
