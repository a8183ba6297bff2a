// emp_smooth_rows.h - the smoothing QP (ref smooth_reference_line, planning_utils.py:262-361) with EIGHT problems per
// wavefront: the x and the y problem of four polylines (device only).
//
// Same idea as emp_qp_rows.h: a problem takes a group of GP = 8 lanes (16 for polylines of up to 64 points: four problems
// per wavefront) and every lane owns R CONSECUTIVE coordinates (GP = 8: R = 3 up to 24 points, R = 4 up to 32), so a sweep
// of the pentadiagonal Cholesky factorisation / substitution serves eight problems where the half-wave form of
// emp_qp_wave.h (box_qp_active_set_lanes<32>) serves two.  Same algorithm - the primal-dual active-set iteration - and the
// same operation order per coordinate, so the fixed point it stops at is the same KKT point: the trajectories of the
// benchmark batch come out bit-identical.  The sweeps are band_chol_rows / band_solve_rows of emp_qp_rows.h at half
// bandwidth 2; this header holds the active-set iteration alone.
#pragma once

#include "emp_qp_rows.h"

namespace emp {

#pragma clang fp contract(fast)      // see emp_qp_wave.h

// One box QP per group of GP lanes (8 or 16) by the primal-dual active-set iteration (box_qp_active_set_lanes, same arithmetic per
// coordinate): ref[r] = the lane's reference coordinates j = gl * R + r (anything for j >= m), box ref +- thr.
// Every lane of the wavefront must call it.  Returns (per group) 0 settled (x holds the minimiser), -1 classification
// still changing after kBoxAsMaxIter rounds (the caller falls back to the interior point), 2 bad input.
template <int GP, int R>
__device__ inline int box_qp_active_set_rows(const double (&ref)[R], int m, const SmoothQpParams& prm, double (&x)[R],
                                             int* iters_out) {
    const int gl = (threadIdx.x & 63) & (GP - 1), base = gl * R;
    const bool valid = m >= 2 && m <= GP * R && prm.thr > 0.0;
    *iters_out = 0;
    bool has[R];
    double Prow[R][3], Plow[R][3], q[R], lo[R], hi[R];
    int code[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = base + r;
        has[r] = valid && j < m;
#pragma unroll
        for (int d = 0; d < 3; ++d) Prow[r][d] = has[r] ? smooth_hess_entry(j, d, m, prm) : 0.0;      // ref planning_utils.py:313-344
        q[r] = has[r] ? -2.0 * prm.w_ref * ref[r] : 0.0;      // ref :346
        lo[r] = ref[r] - prm.thr;                           // ref :308-311
        hi[r] = ref[r] + prm.thr;
        x[r] = ref[r];
        code[r] = 0;                                        // 0 free, 1 fixed at hi, 2 fixed at lo
    }
    rows_column_entries<R, 2>(Prow, Plow, gl == 0);        // P[j-1][j], P[j-2][j]
    const double c = 2.0 * (6.0 * prm.w_smooth + 2.0 * prm.w_length + prm.w_ref);   // the Hessian's interior diagonal
    int state = valid ? 1 : 0, iters = 0;                  // 1 running, 0 done, -1 gave up
    const int steps = oct_wave_max<GP>(valid ? (m + R - 1) / R : 0);
    const bool g_first = gl == 0, g_last = gl == GP - 1;
    // value i of the lane's row window [-2, R + 1]: own rows, the left neighbour's last two, the right neighbour's first two
    auto window = [&](const double (&v)[R], double (&w)[R + 4]) {
        const double p2 = lane_up1(v[R - 2]), p1 = lane_up1(v[R - 1]), n0 = lane_dn1(v[0]), n1 = lane_dn1(v[1]);
        w[0] = g_first ? 0.0 : p2;
        w[1] = g_first ? 0.0 : p1;
#pragma unroll
        for (int r = 0; r < R; ++r) w[2 + r] = v[r];
        w[R + 2] = g_last ? 0.0 : n0;
        w[R + 3] = g_last ? 0.0 : n1;
    };
    while (__any(state == 1)) {
        const bool go = state == 1;
        bool act[R];
        double af[R], ab[R], afw[R + 4], abw[R + 4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            act[r] = go && has[r] && code[r] != 0;
            const double bnd = (code[r] == 1) ? hi[r] : lo[r];
            af[r] = act[r] ? 1.0 : 0.0;
            ab[r] = act[r] ? bnd : 0.0;
        }
        window(af, afw);
        window(ab, abw);
        double fa[R][3], flow[R][3], frinv[R], rhs[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            fa[r][0] = act[r] ? 1.0 : ((go && has[r]) ? Prow[r][0] : 0.0);
            fa[r][1] = (go && !act[r] && afw[r + 3] == 0.0) ? Prow[r][1] : 0.0;
            fa[r][2] = (go && !act[r] && afw[r + 4] == 0.0) ? Prow[r][2] : 0.0;
            const double free_rhs = -q[r] - (((Prow[r][1] * abw[r + 3] + Prow[r][2] * abw[r + 4]) + Plow[r][1] * abw[r + 1]) + Plow[r][2] * abw[r]);
            rhs[r] = act[r] ? ab[r] : ((go && has[r]) ? free_rhs : 0.0);
        }
        const bool okf = band_chol_rows<GP, R, 2>(fa, frinv, flow, m, gl, go, steps);
        band_solve_rows<R, 2>(fa, frinv, flow, rhs, steps);
        double xs[R], xw[R + 4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (go && has[r]) x[r] = rhs[r];
            xs[r] = (go && has[r]) ? x[r] : 0.0;
        }
        if (go) ++iters;
        window(xs, xw);
        // gradient of the full problem at x and the new classification
        bool changed_here = false;
        int ncode[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double g = (q[r] + Prow[r][0] * xs[r]) + (((Prow[r][1] * xw[r + 3] + Prow[r][2] * xw[r + 4]) + Plow[r][1] * xw[r + 1]) + Plow[r][2] * xw[r]);
            const double lam = -g;
            int nc = 0;
            if (lam + c * (xs[r] - hi[r]) > 0.0) nc = 1;
            else if (lam + c * (xs[r] - lo[r]) < 0.0) nc = 2;
            if (!(go && has[r])) nc = code[r];
            ncode[r] = nc;
            changed_here = changed_here || (nc != code[r]);
        }
        const bool changed = oct_any<GP>(changed_here);
        if (go) {
#pragma unroll
            for (int r = 0; r < R; ++r) code[r] = ncode[r];
            if (!okf) state = -1;
            else if (!changed) state = 0;
            else if (iters >= kBoxAsMaxIter) state = -1;
        }
    }
    *iters_out = iters;
    return valid ? state : 2;
}

#pragma clang fp contract(off)

}  // namespace emp
