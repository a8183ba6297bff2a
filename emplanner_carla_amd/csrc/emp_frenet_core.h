// emp_frenet_core.h - Cartesian <-> Frenet helpers of the reference's planning_utils.py, scalar form.
// Tolerance contract (not bit-exact): device sin/cos/atan2 differ from libm in the last ulp; tests
// compare at 1e-6 relative.  "ref:" cites the reference (paths relative to the reference tree).
#pragma once

#include "emp_core.h"

#if !defined(__HIPCC__)
#include <algorithm>
#endif

namespace emp {

#if !defined(__HIPCC__)
using std::max;      // the device compiler declares min / max itself
using std::min;
#endif

struct Node {
    double x, y, theta, kappa;
};
EMP_HD Node node_at(const double* line, int i) { return Node{line[4 * i], line[4 * i + 1], line[4 * i + 2], line[4 * i + 3]}; }

// ref: match_projection_points scan, planning_utils.py:383-402 - strict minimum from index `first`,
// stepping `step` (+1/-1), stop after `limit` consecutive non-improvements.
EMP_HD int match_scan(const double* line, int n_ref, double x, double y, int first, int step, int limit) {
    int match = 0, worse = 0;
    double best = __builtin_inf();
    for (int i = first; i >= 0 && i < n_ref; i += step) {
        const double dx = line[4 * i] - x, dy = line[4 * i + 1] - y;
        const double d = sqrt(dx * dx + dy * dy);
        if (d < best) {
            best = d;
            match = i;
            worse = 0;
        } else if (++worse >= limit) {
            break;
        }
    }
    return match;
}

// numpy.dot of two 2-vectors, as the reference evaluates every projection (planning_utils.py:107, :173, :417, :443, :507,
// :546-578, :799-800).  On an x86 host numpy hands it to OpenBLAS' ddot kernel, which accumulates with fused
// multiply-adds: the result is fma(a1, b1, a0 * b0) - one rounding of the second product fewer than a0*b0 + a1*b1,
// different in the last bit a quarter of the time (checked against numpy 2.2 / OpenBLAS 0.3.29 on 200 000 random
// pairs: identical every time).  That bit decides ties the reference cannot see: a planning start that projects exactly
// onto a node of the reference line (the synthetic scenes put it there) lands on one side or the other of
// `s_map[idx + 1] < s` (path_planning.py:63) by the rounding of this sum.  Evaluating it the way the reference's host
// does took the full-cycle mismatches of a 2048-scene sweep (tools/parity_sweep.py) from two scenes, first trajectory point
// 0.45 mm off, to one - whose tie is decided by the last bit of cos / sin instead.
EMP_HD double dot2(double a0, double a1, double b0, double b1) { return __builtin_fma(a1, b1, a0 * b0); }

// sin and cos of one angle.  The device compiler does not share the argument reduction between a sin(x) and a cos(x) of the
// same x (two reductions, 302 vector instructions); sincos(x) does (one, 155), and returns the same bits as the two calls
// (tools/sincos_bits_test.hip: 2^30 operands over every exponent, 0 differing).  Host builds keep the separate calls: the host
// checks under tests/host_check compare against values computed that way.
EMP_HD void sincos_pair(double x, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(x, s, c);
#else
    *s = sin(x);
    *c = cos(x);
#endif
}

// node m advanced by ds along its tangent, (c, s) = cos / sin of m.theta (ref planning_utils.py:419-424, path_planning.py:66-75)
EMP_HD Node node_advanced(const Node& m, double ds, double c, double s) {
    return Node{m.x + ds * c, m.y + ds * s, m.theta + m.kappa * ds, m.kappa};
}
// the point at offset l along the normal of (x, y), (c, s) = cos / sin of the heading there (ref path_planning.py:32-34, :44-46)
EMP_HD void normal_offset(double x, double y, double l, double c, double s, double* ox, double* oy) {
    *ox = x + l * (-s);
    *oy = y + l * c;
}

// ref: planning_utils.py:414-424 - projection on the tangent line of a matched node, cos / sin of its heading supplied (the
// projection kernel evaluates them once per node and scene)
EMP_HD Node project_on_cs(const Node& m, double c, double s, double x, double y) {
    return node_advanced(m, dot2(x - m.x, y - m.y, c, s), c, s);
}
EMP_HD Node project_on(const Node& m, double x, double y) {
    double c, s;
    sincos_pair(m.theta, &s, &c);
    return project_on_cs(m, c, s, x, y);
}
EMP_HD double projection_s_cs(const Node& m, double c, double s, double s_at_m, double x, double y) {
    return s_at_m + dot2(x - m.x, y - m.y, c, s);
}

// ref: cal_projection_s_fun, planning_utils.py:439-443
EMP_HD double projection_s(const Node& m, double s_at_m, double x, double y) {
    double c, sn;
    sincos_pair(m.theta, &sn, &c);
    return s_at_m + dot2(x - m.x, y - m.y, c, sn);
}

// ref: cal_s_l_fun tail, planning_utils.py:499-507
EMP_HD double lateral_offset(const Node& proj, double x, double y) {
    double c, s;
    sincos_pair(proj.theta, &s, &c);
    return dot2(x - proj.x, y - proj.y, -s, c);
}
// the same with cos / sin of the projection's heading supplied (the planning start forms them once for this and frenet_state_cs)
EMP_HD double lateral_offset_cs(const Node& proj, double c, double s, double x, double y) {
    return dot2(x - proj.x, y - proj.y, -s, c);
}

// ref: cal_s_map_fun, planning_utils.py:448-472.  s_map has n_ref entries.
EMP_HD void s_map_build(const double* line, int n_ref, double ox, double oy, double* s_map) {
    const int m0 = match_scan(line, n_ref, ox, oy, 0, 1, 50);
    double acc = 0.0;
    s_map[0] = 0.0;
    for (int i = 1; i < n_ref; ++i) {
        const double dx = line[4 * i] - line[4 * (i - 1)], dy = line[4 * i + 1] - line[4 * (i - 1) + 1];
        acc = sqrt(dx * dx + dy * dy) + acc;
        s_map[i] = acc;
    }
    const double s0 = projection_s(node_at(line, m0), s_map[m0], ox, oy);
    for (int i = 0; i < n_ref; ++i) s_map[i] = s_map[i] - s0;
}

// ref: cal_s_l_deri_fun, planning_utils.py:538-586 for one point.  (px, py) is the position used for l
// (the reference passes origin_xy there, :542); proj is the projection of the point itself.
struct FrenetState {
    double l, l_dot, s_dot, l_ddot, dl_ds, s_ddot, ddl_ds;
};
// (c, s) = cos / sin of proj.theta
EMP_HD FrenetState frenet_state_cs(const Node& proj, double c, double s, double px, double py, double vx, double vy, double ax,
                                   double ay) {
    FrenetState o;
    const double k = proj.kappa;
    o.l = dot2(px - proj.x, py - proj.y, -s, c);
    o.l_dot = dot2(vx, vy, -s, c);
    o.s_dot = dot2(vx, vy, c, s) / (1.0 - k * o.l);
    o.l_ddot = dot2(ax, ay, -s, c) - k * (1.0 - k * o.l) * (o.s_dot * o.s_dot);
    o.dl_ds = (fabs(o.s_dot) < 1e-6) ? 0.0 : o.l_dot / o.s_dot;
    o.s_ddot = (dot2(ax, ay, c, s) + 2.0 * (o.s_dot * o.s_dot * k * o.dl_ds) + o.s_dot * o.s_dot * 0.0 * o.l) / (1.0 - k * o.l);
    o.ddl_ds = (fabs(o.s_dot) < 1e-6) ? 0.0 : (o.l_ddot - o.dl_ds * o.s_ddot) / (o.s_dot * o.s_dot);
    return o;
}
EMP_HD FrenetState frenet_state(const Node& proj, double px, double py, double vx, double vy, double ax, double ay) {
    double c, s;
    sincos_pair(proj.theta, &s, &c);
    return frenet_state_cs(proj, c, s, px, py, vx, vy, ax, ay);
}

// ref: cal_proj_point, path_planning.py:52-75 - monotone walk; returns false where the reference would
// raise IndexError (s beyond the last s_map entry).
EMP_HD bool proj_point(const double* line, const double* s_map, int n_ref, double s, int* idx, Node* out) {
    int i = *idx;
    while (true) {
        if (i + 1 >= n_ref) return false;
        if (!(s_map[i + 1] < s)) break;
        ++i;
    }
    const Node m = node_at(line, i);
    const double ds = s - s_map[i];
    double c, sn;
    sincos_pair(m.theta, &sn, &c);
    *out = node_advanced(m, ds, c, sn);
    *idx = i;
    return true;
}

// ---------------------------------------------------------------------------------------------
// The station lookups the kernels of emp_tail_kernels.h share, here so that the CPU checks (tests/host_check) run the same text.
// ---------------------------------------------------------------------------------------------
// monotone index walk of cal_proj_point from index 0 (ref path_planning.py:62-64: `while s_map[idx + 1] < s: idx += 1`);
// *off_end when it runs past the end.  s_map is a cumulative chord length, i.e. non-decreasing, so the walk's stopping
// index is found by bisection (6 LDS round trips instead of up to P).
EMP_HD int walk_from_zero(const double* sm, int P, double s, bool* off_end) {
    int lo = 0, hi = P - 1;                       // answer in [0, P-1]; P-1 = "no index stops the walk"
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sm[mid + 1] < s) lo = mid + 1;
        else hi = mid;
    }
    *off_end = lo + 1 >= P;
    return lo;
}

// ref: cal_lmin_lmax, path_planning.py:222-273.  lmin_lmax returns false where the reference raises IndexError.
EMP_HD int argmin_abs(const double* s, int stride, int n, double target) {
    int best = 0;
    double bv = fabs(s[0] - target);
    for (int j = 1; j < n; ++j) {
        const double v = fabs(s[j * stride] - target);
        if (v < bv) {
            bv = v;
            best = j;
        }
    }
    return best;
}

// The three scans of one obstacle (ref path_planning.py:240, :241, :257) in ONE pass over the stations, four stations a step: the
// same comparisons in the same order per target as three argmin_abs calls (strict '<': the first minimum), but the stations are
// read once and four LDS reads are in flight at a time - the three separate loops were 3 n dependent LDS round trips of a wavefront
// that has its SIMD to itself (round 6: 4 us of the path-QP kernel's 30 us set-up).  n >= 1.
EMP_HD void argmin_abs3(const double* s, int n, double t0, double t1, double t2, int* i0, int* i1, int* i2) {
    const double f = s[0];
    double b0 = fabs(f - t0), b1 = fabs(f - t1), b2 = fabs(f - t2);
    int k0 = 0, k1 = 0, k2 = 0;
    for (int j0 = 1; j0 < n; j0 += 4) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = s[min(j0 + u, n - 1)];      // past the end: the last station again (never a strict improvement)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u;
            const double a0 = fabs(v[u] - t0), a1 = fabs(v[u] - t1), a2 = fabs(v[u] - t2);
            if (a0 < b0) { b0 = a0; k0 = j; }
            if (a1 < b1) { b1 = a1; k1 = j; }
            if (a2 < b2) { b2 = a2; k2 = j; }
        }
    }
    *i0 = min(k0, n - 1);      // (k never exceeds n - 1: a repeated last station is not strictly below itself; the clamp costs nothing)
    *i1 = min(k1, n - 1);
    *i2 = min(k2, n - 1);
}

EMP_HD bool lmin_lmax(const double* dp_s, const double* dp_l, int stride, int n, const double* obs_s,
                                 const double* obs_l, int n_obs, double obs_length, double obs_width, double* l_min,
                                 double* l_max) {
    for (int j = 0; j < n; ++j) {
        l_min[j] = -10.0;                                                          // ref :233-234
        l_max[j] = 10.0;
    }
    for (int k = 0; k < n_obs; ++k) {
        const int lo = argmin_abs(dp_s, stride, n, obs_s[k] - obs_length / 2.0) + 2;   // ref :240
        const int hi = argmin_abs(dp_s, stride, n, obs_s[k] + obs_length / 2.0) + 2;   // ref :241
        const int centre = argmin_abs(dp_s, stride, n, obs_s[k]);                      // ref :257
        const bool below = dp_l[centre * stride] < obs_l[k];                           // ref :263
        for (int j = lo; j <= hi; ++j) {
            if (j >= n) return false;                                                  // IndexError in the reference
            if (below) l_max[j] = fmin(l_max[j], obs_l[k] - obs_width / 2.0);
            else l_min[j] = fmax(l_min[j], obs_l[k] + obs_width / 2.0);
        }
    }
    return true;
}

// Centred difference of v[0..m) (stride `stride`) at i: the mean of the forward differences on either side, the ends replicated
// (ref planning_utils.py:193-203 and :213-222).  Needs m >= 2.
EMP_HD double centred_diff(const double* v, int stride, int i, int m) {
    const int a = (i - 1 > 0) ? i - 1 : 0, b = (i < m - 2) ? i : m - 2;
    return ((v[(a + 1) * stride] - v[a * stride]) + (v[(b + 1) * stride] - v[b * stride])) / 2.0;
}

// ref: cal_heading_kappa, planning_utils.py:185-228.  xy interleaved [m][stride]; needs m >= 2.
EMP_HD void heading_kappa(const double* xy, int stride, int m, double* theta, int tstride, double* kappa, int kstride) {
    for (int i = 0; i < m; ++i) {
        const double dx = centred_diff(xy, stride, i, m), dy = centred_diff(xy + 1, stride, i, m);
        theta[i * tstride] = atan2(dy, dx);
    }
    for (int i = 0; i < m; ++i) {
        const double dx = centred_diff(xy, stride, i, m), dy = centred_diff(xy + 1, stride, i, m);
        kappa[i * kstride] = sin(centred_diff(theta, tstride, i, m)) / sqrt(dx * dx + dy * dy);
    }
}

}  // namespace emp
