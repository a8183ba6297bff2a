// emp_mpc_kernels.h - batched lateral MPC controller (the controller input side).
// ref: controller/controller.py class Lateral_MPC_controller, :65-337 - `_control` from explicit inputs (the
// reference reads x, y, yaw, velocities from a live carla.Vehicle in cal_vehicle_info, :90-113).
//
// Mapping: one vehicle per GROUP of 12 lanes - lane r owns control r of the condensed problem (N = 6 steps x P = 2
// controls per step, :72-73) - and five vehicles per wavefront.  The small per-vehicle algebra (4x4 model,
// bilinear discretisation, 50-point nearest-point window, powers of A_bar) is computed redundantly by the 12
// lanes of a group; lane r then builds row r of the dense 12 x 12 Hessian and the box QP (|u| <= 1, :300-304) is
// solved by the same Mehrotra interior point as the planner's QPs with a dense Cholesky whose pivot rows travel
// by ds_bpermute inside the group.
#pragma once

#include <hip/hip_runtime.h>

#include "emp_qp_wave.h"          // closes its `fp contract(fast)` region at its end
#include "emp_tail_kernels.h"   // status bits
#include "emp_control_core.h"   // PID step and actuation of the fused vehicle-control kernels

namespace emp {
namespace mpc {

constexpr int kN = 6, kP = 2, kNu = kN * kP;     // ref :72-73
constexpr int kGroupsPerWave = 5;
constexpr int kWindow = 50;                      // ref :204
constexpr double kTs = 0.1;                      // ref :159 and _control's cal_error_k_fun(ts=0.1), :333

struct Params {
    double a, b, Cf, Cr, m, Iz;                  // vehicle_para (ref test_9.py:316)
    double q[4], f[4], r;                        // Q, F diagonals and R (ref :321-328)
};

struct V4 { double v[4]; };
struct M4 { double a[4][4]; };

__device__ __forceinline__ V4 matvec(const M4& A, const V4& x) {
    V4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) y.v[i] = ((A.a[i][0] * x.v[0] + A.a[i][1] * x.v[1]) + A.a[i][2] * x.v[2]) + A.a[i][3] * x.v[3];
    return y;
}

// inverse of a 4 x 4 matrix by Gauss-Jordan with partial pivoting (the reference calls np.linalg.inv, :161)
__device__ inline bool inverse4(const M4& A, M4* out) {
    double w[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[i][j] = A.a[i][j];
            w[i][4 + j] = (i == j) ? 1.0 : 0.0;
        }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        double best = fabs(w[c][c]);
#pragma unroll
        for (int r = c + 1; r < 4; ++r)
            if (fabs(w[r][c]) > best) {
                best = fabs(w[r][c]);
                piv = r;
            }
        if (!(best > 0.0)) {
            // singular or non-finite: NaN, not whatever *out held - the callers still form A_bar, H, f and K from it for the outputs
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) out->a[i][j] = __builtin_nan("");
            return false;
        }
#pragma unroll
        for (int r = c + 1; r < 4; ++r)
            if (r == piv) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const double t = w[c][j];
                    w[c][j] = w[r][j];
                    w[r][j] = t;
                }
            }
        const double inv = 1.0 / w[c][c];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[c][j] *= inv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double m = w[r][c];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[r][j] -= m * w[c][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out->a[i][j] = w[i][4 + j];
    return true;
}

// value of lane `k` of MY group (the group whose first lane is group_base)
__device__ __forceinline__ double grp_bcast(double v, int group_base, int k) {
    union { double d; int i[2]; } a, r;
    a.d = v;
    const int src = (group_base + k) << 2;
    r.i[0] = __builtin_amdgcn_ds_bpermute(src, a.i[0]);
    r.i[1] = __builtin_amdgcn_ds_bpermute(src, a.i[1]);
    return r.d;
}
__device__ __forceinline__ int grp_bcast_int(int v, int group_base, int k) {
    return __builtin_amdgcn_ds_bpermute((group_base + k) << 2, v);
}
// over the NU lanes of MY group, in lane order
template <int NU, class Op>
__device__ __forceinline__ double grp_reduce(double v, int group_base, Op op) {
    double acc = grp_bcast(v, group_base, 0);
#pragma unroll
    for (int k = 1; k < NU; ++k) acc = op(acc, grp_bcast(v, group_base, k));
    return acc;
}

// Dense box QP  min 1/2 u'Hu + f'u, -1 <= u <= 1  on one group of NU lanes: lane r holds row r of H (h[]) and f_r.
// Same interior point as smooth_pair_lanes (emp_qp_wave.h; stopping rule: qp_stop_rule, emp_qp_core.h): G = I, so a row IS its
// unknown.  H may be singular (the feed-forward law's is): M = H + diag(wu + wl) stays positive definite as the weights are.
// Returns 0 ok / 2 failed (group-uniform); u_out = this lane's control.
template <int NU>
__device__ inline int box_qp_full(const double (&h)[NU], double f_r, int r, int gb, bool live, double* u_out, int* iters_out) {
    const double eps_p = 1e-10, eps_mu = 1e-13, eps_d_rel = 1e-10;
    const double lo = -1.0, hi = 1.0;
    double u = 0.0, su = 1.0, sl = 1.0, zu = 1.0, zl = 1.0;          // slacks of the centre of the box are already 1
    const double qscale = fmax(1.0, grp_reduce<NU>(fabs(f_r), gb, [](double a, double b) { return fmax(a, b); }));
    int state = live ? 1 : 0, iters = 0;
    bool acceptable = false;
    const int rows = 2 * NU;
    while (__any(state == 1)) {
        const bool run = state == 1;
        const double rpu = u - hi + su, rpl = lo - u + sl;
        const double isu = fast_rcp(su), isl = fast_rcp(sl), izu = fast_rcp(zu), izl = fast_rcp(zl);
        const double wu = zu * isu, wl = zl * isl;
        double hu = 0.0;
#pragma unroll
        for (int c = 0; c < NU; ++c) hu = __builtin_fma(h[c], grp_bcast(u, gb, c), hu);
        const double rd = (hu + f_r) + (zu - zl);
        const double rd_max = grp_reduce<NU>(fabs(rd), gb, [](double a, double b) { return fmax(a, b); });
        const double rp_max = grp_reduce<NU>(fmax(fabs(rpu), fabs(rpl)), gb, [](double a, double b) { return fmax(a, b); });
        const double zmax = grp_reduce<NU>(fmax(zu, zl), gb, [](double a, double b) { return fmax(a, b); });
        const double mu = grp_reduce<NU>(su * zu + sl * zl, gb, [](double a, double b) { return a + b; }) / (double)rows;
        if (run)
            state = qp_stop_rule<false, false>(rd_max, rp_max, mu, zmax, qscale, 0.0, iters, kQpMaxIter, eps_d_rel, eps_p, eps_mu,
                                               acceptable).state;
        const bool go = state == 1;
        // ---- dense Cholesky of M = H + diag(wu + wl): lane r keeps row r; after step k its entry k is L[r][k]
        // (r > k) and lane k's entries j > k are U[k][j] = L[j][k]
        double a[NU], rinv = 1.0;
#pragma unroll
        for (int c = 0; c < NU; ++c) a[c] = go ? h[c] : ((c == r) ? 1.0 : 0.0);
#pragma unroll
        for (int c = 0; c < NU; ++c)
            if (c == r && go) a[c] += wu + wl;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < NU; ++k) {
            double rowk[NU];
#pragma unroll
            for (int j = k; j < NU; ++j) rowk[j] = grp_bcast(a[j], gb, k);
            const double piv = rowk[k];
            if (!(piv > 0.0)) bad = true;
            const double rs = fast_rsqrt(piv > 0.0 ? piv : 1.0);
            const double lik = a[k] * rs;                       // column-k entry of my row, scaled (symmetry: = U[k][r])
#pragma unroll
            for (int j = k + 1; j < NU; ++j) {
                const double ukj = rowk[j] * rs;
                if (r > k) a[j] = __builtin_fma(-lik, ukj, a[j]);
                else if (r == k) a[j] = ukj;
            }
            if (r >= k) a[k] = (r == k) ? piv * rs : lik;
            if (r == k) rinv = rs;
        }
        if (go && bad) state = acceptable ? 0 : 2;
        const bool go2 = state == 1;
        auto solve = [&](double b) {
#pragma unroll
            for (int k = 0; k < NU; ++k) {                     // L y = b
                const double yk = grp_bcast(b * rinv, gb, k);
                if (r == k) b = yk;
                else if (r > k) b = __builtin_fma(-a[k], yk, b);
            }
#pragma unroll
            for (int k = NU - 1; k >= 0; --k) {                // L' x = y
                const double xk = grp_bcast(b * rinv, gb, k);
                if (r == k) b = xk;
                else if (r < k) b = __builtin_fma(-a[k], xk, b);
            }
            return b;
        };
        const double dua = solve(go2 ? -rd - ((wu * rpu - zu) - (wl * rpl - zl)) : 0.0);
        const double dsua = -rpu - dua, dsla = -rpl + dua;
        const double dzua = -zu - wu * dsua, dzla = -zl - wl * dsla;
        double ratio = go2 ? fmax(fmax(-dsua * isu, -dsla * isl), fmax(-dzua * izu, -dzla * izl)) : 0.0;
        ratio = grp_reduce<NU>(ratio, gb, [](double x, double y) { return fmax(x, y); });
        const double a_aff = (ratio > 1.0) ? fast_rcp(ratio) : 1.0;
        double mu_aff = go2 ? (su + a_aff * dsua) * (zu + a_aff * dzua) + (sl + a_aff * dsla) * (zl + a_aff * dzla) : 0.0;
        mu_aff = grp_reduce<NU>(mu_aff, gb, [](double x, double y) { return x + y; }) / (double)rows;
        double sigma = (mu > 0.0) ? mu_aff * fast_rcp(mu) : 0.0;
        sigma = sigma * sigma * sigma;
        const double rcu = su * zu + dsua * dzua - sigma * mu, rcl = sl * zl + dsla * dzla - sigma * mu;
        const double du = solve(go2 ? -rd - ((zu * rpu - rcu) * isu - (zl * rpl - rcl) * isl) : 0.0);
        const double dsu = -rpu - du, dsl = -rpl + du;
        const double dzu = -(rcu + zu * dsu) * isu, dzl = -(rcl + zl * dsl) * isl;
        ratio = go2 ? fmax(fmax(-dsu * isu, -dsl * isl), fmax(-dzu * izu, -dzl * izl)) : 0.0;
        ratio = grp_reduce<NU>(ratio, gb, [](double x, double y) { return fmax(x, y); });
        const double tau = qp_step_fraction(mu);
        const double alpha = (ratio > tau) ? tau * fast_rcp(ratio) : 1.0;
        if (go2) {
            su += alpha * dsu;
            sl += alpha * dsl;
            zu += alpha * dzu;
            zl += alpha * dzl;
            u += alpha * du;
            ++iters;
        }
    }
    *u_out = u;
    *iters_out = iters;
    return state;
}

// The longitudinal half of Vehicle_control.run_step (ref :680-724) that the fused vehicle-control kernels append to a lateral
// law (emp_vehicle_control): the PID step and the actuation, for vehicle b whose lateral law gave `lat` with status `lat_status`.
// A vehicle the lateral law failed on gets zero controls and its PID state back unchanged (the reference raises in _control()
// before PID_control runs, :700-702).  err_out / n_err_out may be the memory of err_in / n_err_in.
struct CtlIO {
    ctl::PidParams pid;
    const double* speed_kmh;       // [B]
    const double* target_speed;    // [B]
    const double* err_in;          // [B][60]
    const int* n_err_in;           // [B]
    double* control;               // [B][3] throttle, steer, brake
    double* lon_command;           // [B] or null
    double* err_out;               // [B][60]
    int* n_err_out;                // [B]
};

__device__ inline void control_epilogue(const CtlIO& io, int b, int lat_status, double lat) {
    const double* ein = io.err_in + (size_t)b * ctl::kPidBuffer;
    double* eout = io.err_out + (size_t)b * ctl::kPidBuffer;
    double* c3 = io.control + 3 * (size_t)b;
    if (lat_status == 0) {
        int n = 0;
        const double acc = ctl::pid_step(io.pid, io.speed_kmh[b], io.target_speed[b], ein, io.n_err_in[b], eout, &n);
        io.n_err_out[b] = n;
        if (io.lon_command) io.lon_command[b] = acc;
        ctl::actuate(lat, acc, &c3[0], &c3[1], &c3[2]);
    } else {
        const int n = io.n_err_in[b];
        for (int i = 0; i < ctl::kPidBuffer; ++i) eout[i] = ein[i];
        io.n_err_out[b] = n;
        if (io.lon_command) io.lon_command[b] = 0.0;
        c3[0] = c3[1] = c3[2] = 0.0;
    }
}

// What one evaluation of a lateral law leaves in registers: the kernels below write it out, the rollout kernels feed it to the
// vehicle model.
struct LatResult {
    double steer;                  // the command; 0 where status != 0
    V4 e_rr;
    double pk;                     // k_r
    double pre[4];                 // predicted x, y and projected x, y
    int idx, iters, status;        // match index, QP iterations / Riccati sweeps, status bits
};

// ---- what the three lateral laws (mpc_lateral_core, lqr::lqr_lateral_core, mpcff::mpc_ff_lateral_core) share.  Each core reads
// top to bottom as: model, predict, match, error, discretise, problem or Riccati, solve, outputs.

// continuous error model of cal_A_B_C_fun (ref :115-148, :424-455, :778-809).  V is the velocity that divides: the clamped Vx
// for the MPC, Vx + 0.0001 for the other two.  The LQR has no Cc.
__device__ __forceinline__ void error_model(const Params& prm, double V, M4* A_out, V4* Bc, V4* Cc) {
    M4 A;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) A.a[i][j] = 0.0;
    A.a[0][1] = 1.0;
    A.a[1][1] = (prm.Cf + prm.Cr) / (prm.m * V);
    A.a[1][2] = -(prm.Cf + prm.Cr) / prm.m;
    A.a[1][3] = (prm.a * prm.Cf - prm.b * prm.Cr) / (prm.m * V);
    A.a[2][3] = 1.0;
    A.a[3][1] = (prm.a * prm.Cf - prm.b * prm.Cr) / (prm.Iz * V);
    A.a[3][2] = -(prm.a * prm.Cf - prm.b * prm.Cr) / prm.Iz;
    A.a[3][3] = (prm.a * prm.a * prm.Cf + prm.b * prm.b * prm.Cr) / (prm.Iz * V);
    *A_out = A;
    *Bc = V4{{0.0, -prm.Cf / prm.m, 0.0, -prm.a * prm.Cf / prm.Iz}};
    *Cc = V4{{0.0, (prm.a * prm.Cf + prm.b * prm.Cr) / (prm.m * V) - V, 0.0,
              (prm.a * prm.a * prm.Cf + prm.b * prm.b * prm.Cr) / (prm.Iz * V)}};
}

// the pose kTs ahead (cal_error_k_fun(ts = 0.1), ref :170-180): always with the law's own Vx, never the guarded one
__device__ __forceinline__ void predict_pose(double Vx, double Vy, double fi_dot, double* x, double* y, double* fi) {
    const double c = cos(*fi), s = sin(*fi);
    const double xn = *x + Vx * kTs * c - Vy * kTs * s;
    const double yn = *y + Vy * kTs * c + Vx * kTs * s;
    *x = xn;
    *y = yn;
    *fi = *fi + fi_dot * kTs;
}

// tracking error of the predicted pose (x, y, fi) at path point idx (ref :226-251): o's e_rr, pk, pre and idx.
// raw_e_fi: e_fi is the angle fi - theta_r itself (the feed-forward law, ref :889), not its sine.
__device__ __forceinline__ void tracking_error(const double* __restrict__ path, int idx, double x, double y, double fi, double Vx,
                                               double Vy, double fi_dot, bool raw_e_fi, LatResult* o) {
    const double px = path[4 * idx], py = path[4 * idx + 1], pth = path[4 * idx + 2], pk = path[4 * idx + 3];
    const double ct = cos(pth), st = sin(pth);
    const double dvx = x - px, dvy = y - py;
    const double e_d = -st * dvx + ct * dvy;
    const double e_s = ct * dvx + st * dvy;
    const double theta_r = pth + pk * e_s;
    const double cd = cos(fi - theta_r), sd = sin(fi - theta_r);
    const double e_d_dot = Vy * cd + Vx * sd;
    const double e_fi = raw_e_fi ? fi - theta_r : sd;
    const double S_dot = (Vx * cd - Vy * sd) / (1.0 - pk * e_d);
    const double e_fi_dot = fi_dot - pk * S_dot;
    o->e_rr = V4{{e_d, e_d_dot, e_fi, e_fi_dot}};
    o->pk = pk;
    o->pre[0] = x;
    o->pre[1] = y;
    o->pre[2] = px + e_s * ct;
    o->pre[3] = py + e_s * st;
    o->idx = idx;
}

// bilinear discretisation (ref :159-165): A_bar = inv (I + kTs A / 2), B_bar = inv Bc kTs with inv = (I - kTs A / 2)^-1.
// Returns false where that inverse does not exist.
__device__ __forceinline__ bool discretise(const M4& A, const V4& Bc, M4* inv_out, M4* Ab_out, V4* Bb_out) {
    M4 lhs, rhs, inv;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double e = (i == j) ? 1.0 : 0.0;
            lhs.a[i][j] = e - (kTs * A.a[i][j]) / 2.0;
            rhs.a[i][j] = e + (kTs * A.a[i][j]) / 2.0;
        }
    const bool inv_ok = inverse4(lhs, &inv);
    M4 Ab;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            Ab.a[i][j] = ((inv.a[i][0] * rhs.a[0][j] + inv.a[i][1] * rhs.a[1][j]) + inv.a[i][2] * rhs.a[2][j]) + inv.a[i][3] * rhs.a[3][j];
    V4 Bb = matvec(inv, Bc);
#pragma unroll
    for (int i = 0; i < 4; ++i) Bb.v[i] = Bb.v[i] * kTs;
    *inv_out = inv;
    *Ab_out = Ab;
    *Bb_out = Bb;
    return inv_ok;
}
// ... and the MPCs' C_bar = inv Cc kTs k_r Vx (ref :164, :821), with discretise's inv
__device__ __forceinline__ V4 discretise_offset(const M4& inv, const V4& Cc, double pk, double Vx) {
    V4 Cb = matvec(inv, Cc);
#pragma unroll
    for (int i = 0; i < 4; ++i) Cb.v[i] = Cb.v[i] * kTs * pk * Vx;
    return Cb;
}

// condensed problem of N steps x P controls per step (ref :262-298, :924-948) for the lane that owns control r: row r of H and
// f_r, with g_t = A_bar^t B_bar and the free response w_i = A_bar^i e_rr + Cc_i.  R_bar regularises controls 0 .. n_reg - 1.
template <int N, int P>
__device__ __forceinline__ void condensed_row(const Params& prm, const M4& Ab, const V4& Bb, const V4& Cb, const V4& e_rr, int r,
                                              int n_reg, double (&h)[N * P], double* f_r_out) {
    V4 g[N];
    g[0] = Bb;
#pragma unroll
    for (int t = 1; t < N; ++t) g[t] = matvec(Ab, g[t - 1]);
    V4 w[N + 1];
    {
        V4 me = e_rr, cc{{0.0, 0.0, 0.0, 0.0}};
        w[0] = me;
#pragma unroll
        for (int i = 1; i <= N; ++i) {
            me = matvec(Ab, me);
            cc = matvec(Ab, cc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                cc.v[q] += Cb.v[q];
                w[i].v[q] = cc.v[q] + me.v[q];
            }
        }
    }
    const int jr = r / P;
    double f_r = 0.0;
#pragma unroll
    for (int c = 0; c < N * P; ++c) {
        const int jc = c / P;
        double acc = 0.0;
#pragma unroll
        for (int i = 1; i <= N; ++i) {
            // block row i of C holds A_bar^(i-1-j) B_bar in the P columns of step j < i (ref :268-273)
            if (i - 1 - jr < 0 || i - 1 - jc < 0) continue;
            const double* wt = (i == N) ? prm.f : prm.q;
            const V4& ga = g[(i - 1 - jr) < 0 ? 0 : (i - 1 - jr)];
            const V4& gc = g[i - 1 - jc];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc += ga.v[q] * wt[q] * gc.v[q];
        }
        if (c == r && c < n_reg) acc += prm.r;
        h[c] = 2.0 * acc;
    }
#pragma unroll
    for (int i = 1; i <= N; ++i) {
        if (i - 1 - jr < 0) continue;
        const double* wt = (i == N) ? prm.f : prm.q;
        const V4& ga = g[(i - 1 - jr) < 0 ? 0 : (i - 1 - jr)];
#pragma unroll
        for (int q = 0; q < 4; ++q) f_r += ga.v[q] * wt[q] * w[i].v[q];
    }
    *f_r_out = 2.0 * f_r;
}

// ref: Lateral_MPC_controller._control (:313-337) for the vehicle of MY 12-lane group (lane r of the group at lane gb), from its
// state in registers: the body of mpc_lateral_kernel and of a tick of mpc_rollout_kernel.  `path` is the vehicle's row, np_ its
// clamped count, idx the previous match.  h, *f_r_out, *u_out: row r of H, f_r and control r (lane-local); *o is group-uniform.
__device__ __forceinline__ void mpc_lateral_core(const Params& prm, const double* __restrict__ path, int np_, double x, double y,
                                                 double fi, double Vy, double fi_dot, double Vx, int idx, bool live, int r, int gb,
                                                 double (&h)[kNu], double* f_r_out, double* u_out, LatResult* o) {
    M4 A, inv, Ab;
    V4 Bc, Cc, Bb;
    error_model(prm, Vx, &A, &Bc, &Cc);
    predict_pose(Vx, Vy, fi_dot, &x, &y, &fi);
    // ---- match (ref :201-224): a 50-point window from the previous index
    bool bad_index = live && (np_ < 1 || idx < 0 || idx >= np_);   // the reference raises IndexError at :224
    if (bad_index || !live) idx = 0;                               // (an idle group follows no index at all)
    {
        double min_d = 10000.0;                                     // squared metres (ref :201): farther than 100 m
        const int first = idx, last = min(first + kWindow, np_);    // keeps the previous match
        for (int i = first; i < last; ++i) {
            const double dx = path[4 * i] - x, dy = path[4 * i + 1] - y;
            const double d = dx * dx + dy * dy;
            if (d < min_d) {
                min_d = d;
                idx = i;
            }
        }
    }
    tracking_error(path, idx, x, y, fi, Vx, Vy, fi_dot, false, o);
    const bool inv_ok = discretise(A, Bc, &inv, &Ab, &Bb);
    const V4 Cb = discretise_offset(inv, Cc, o->pk, Vx);
    double f_r;
    condensed_row<kN, kP>(prm, Ab, Bb, Cb, o->e_rr, r, kNu, h, &f_r);
    // ---- box QP (ref :300-311) and outputs
    const bool solvable = live && !bad_index && inv_ok;
    double u = 0.0;
    int it = 0;
    const int rc = box_qp_full<kNu>(h, f_r, r, gb, solvable, &u, &it);
    const bool ok = solvable && rc == 0;
    *f_r_out = f_r;
    *u_out = ok ? u : 0.0;
    o->steer = grp_bcast(ok ? u : 0.0, gb, 0);                    // ref :311: res['x'][0]
    o->iters = it;
    o->status = bad_index ? kStSOutOfRange : ((!inv_ok || rc != 0) ? kStQpFailed : 0);
}

// ref: Lateral_MPC_controller._control (:313-337) for B vehicles; grid = ceil(B / 5), block = 64.  kFused: then the longitudinal
// half of Vehicle_control.run_step (control_epilogue) on the lane that holds u[0] - emp_vehicle_control in one launch; the
// lateral arithmetic is the same in both instantiations.
template <bool kFused>
__global__ __launch_bounds__(64) void mpc_lateral_kernel(int B, int max_path, Params prm, const double* __restrict__ target_path,
                                                         const int* __restrict__ n_path, const double* __restrict__ state,
                                                         const double* __restrict__ vx, const int* __restrict__ min_index_in,
                                                         double* __restrict__ steer, double* __restrict__ u_out,
                                                         double* __restrict__ e_rr_out, double* __restrict__ k_r_out,
                                                         int* __restrict__ min_index_out, double* __restrict__ pre_pro,
                                                         double* __restrict__ H_out, double* __restrict__ f_out,
                                                         int* __restrict__ iters_out, int* __restrict__ status, CtlIO io) {
    const int lane = threadIdx.x & 63;
    const int grp = lane / kNu, r = lane - grp * kNu;
    const int gb = grp * kNu;
    const int b = blockIdx.x * kGroupsPerWave + grp;
    const bool live = grp < kGroupsPerWave && b < B;
    const int bb = live ? b : 0;
    double h[kNu], f_r, u;
    LatResult o;
    // vehicle state: what cal_vehicle_info provides (ref :90-113); a count beyond the path's row is clamped, never followed
    mpc_lateral_core(prm, target_path + (size_t)bb * max_path * 4, min(max(n_path[bb], 0), max_path), state[5 * bb],
                     state[5 * bb + 1], state[5 * bb + 2], state[5 * bb + 3], state[5 * bb + 4], vx[bb], min_index_in[bb], live, r, gb,
                     h, &f_r, &u, &o);
    if (live) {
        if (H_out)
#pragma unroll
            for (int c = 0; c < kNu; ++c) H_out[((size_t)b * kNu + r) * kNu + c] = h[c];
        if (f_out) f_out[(size_t)b * kNu + r] = f_r;
        if (u_out) u_out[(size_t)b * kNu + r] = u;
        if (r == 0) {
            steer[b] = o.steer;
            if (e_rr_out)
#pragma unroll
                for (int q = 0; q < 4; ++q) e_rr_out[4 * b + q] = o.e_rr.v[q];
            if (k_r_out) k_r_out[b] = o.pk;
            min_index_out[b] = o.idx;
            if (pre_pro)
#pragma unroll
                for (int q = 0; q < 4; ++q) pre_pro[4 * b + q] = o.pre[q];
            if (iters_out) iters_out[b] = o.iters;
            status[b] = o.status;
            if constexpr (kFused) control_epilogue(io, b, o.status, o.steer);
        }
    }
}

}  // namespace mpc

// ---------------------------------------------------------------------------------------------
// Lateral LQR controller, ref controller/controller.py class Lateral_LQR_controller (:374-611): `_control` from
// explicit inputs.  One vehicle per lane: the 4 x 4 algebra lives in registers and the Riccati iteration
// (:470-481: until max|dP| < 0.1, at most 5000 sweeps - a slowly creeping vehicle needs all of them) is a private
// loop; lanes of a wavefront simply run as long as their slowest vehicle.  Products are associated as NumPy
// evaluates the reference's expression (left to right).
// ---------------------------------------------------------------------------------------------
namespace lqr {

using mpc::M4;
using mpc::V4;

__device__ __forceinline__ M4 matmul(const M4& A, const M4& B) {
    M4 C;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            C.a[i][j] = ((A.a[i][0] * B.a[0][j] + A.a[i][1] * B.a[1][j]) + A.a[i][2] * B.a[2][j]) + A.a[i][3] * B.a[3][j];
    return C;
}

// ref: Lateral_LQR_controller._control (:374-611) for ONE vehicle from its state in registers: the body of lqr_lateral_kernel and
// of a tick of lqr_rollout_kernel.  `path` is the vehicle's row, np_ its clamped count, idx the fallback match.
__device__ __forceinline__ void lqr_lateral_core(const mpc::Params& prm, const double* __restrict__ path, int np_, double x, double y,
                                                 double fi, double Vy, double fi_dot, double Vx, int idx, V4* K_out,
                                                 mpc::LatResult* o) {
    // ---- model (ref :424-455: Vx + 0.0001 guards the divisions), discretisation and Riccati iteration (ref :466-481)
    M4 A, inv, Ad;
    V4 Bc, Cc, Bd;
    mpc::error_model(prm, Vx + 0.0001, &A, &Bc, &Cc);
    const bool inv_ok = mpc::discretise(A, Bc, &inv, &Ad, &Bd);
    M4 AT;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) AT.a[i][j] = Ad.a[j][i];
    M4 P, Ppre;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) P.a[i][j] = Ppre.a[i][j] = (i == j) ? prm.q[i] : 0.0;
    int sweeps = 0;
    for (int it = 0; it < 5000; ++it) {
        const M4 ATP = matmul(AT, P);
        const M4 ATPA = matmul(ATP, Ad);
        const V4 ATPB = mpc::matvec(ATP, Bd);
        V4 BTP;                                             // B' P (row vector)
#pragma unroll
        for (int j = 0; j < 4; ++j) BTP.v[j] = ((Bd.v[0] * P.a[0][j] + Bd.v[1] * P.a[1][j]) + Bd.v[2] * P.a[2][j]) + Bd.v[3] * P.a[3][j];
        V4 BTPA;
#pragma unroll
        for (int j = 0; j < 4; ++j) BTPA.v[j] = ((BTP.v[0] * Ad.a[0][j] + BTP.v[1] * Ad.a[1][j]) + BTP.v[2] * Ad.a[2][j]) + BTP.v[3] * Ad.a[3][j];
        const double BTPB = ((BTP.v[0] * Bd.v[0] + BTP.v[1] * Bd.v[1]) + BTP.v[2] * Bd.v[2]) + BTP.v[3] * Bd.v[3];
        const double g = 1.0 / (prm.r + BTPB);
        double delta = 0.0;
        M4 Pn;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Pn.a[i][j] = (ATPA.a[i][j] - (ATPB.v[i] * g) * BTPA.v[j]) + ((i == j) ? prm.q[i] : 0.0);
                delta = fmax(delta, fabs(Pn.a[i][j] - Ppre.a[i][j]));
            }
        P = Pn;
        sweeps = it + 1;
        if (delta < 0.1) break;
        Ppre = Pn;
    }
    V4 K;
    {
        V4 BTP;
#pragma unroll
        for (int j = 0; j < 4; ++j) BTP.v[j] = ((Bd.v[0] * P.a[0][j] + Bd.v[1] * P.a[1][j]) + Bd.v[2] * P.a[2][j]) + Bd.v[3] * P.a[3][j];
        const double BTPB = ((BTP.v[0] * Bd.v[0] + BTP.v[1] * Bd.v[1]) + BTP.v[2] * Bd.v[2]) + BTP.v[3] * Bd.v[3];
        const double g = 1.0 / (BTPB + prm.r);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            K.v[j] = g * (((BTP.v[0] * Ad.a[0][j] + BTP.v[1] * Ad.a[1][j]) + BTP.v[2] * Ad.a[2][j]) + BTP.v[3] * Ad.a[3][j]);
    }
    mpc::predict_pose(Vx, Vy, fi_dot, &x, &y, &fi);
    // ---- match (ref :519-535): the nearest point of the whole path
    {
        double min_d = 10000.0;
        for (int i = 0; i < np_; ++i) {
            const double dx = path[4 * i] - x, dy = path[4 * i + 1] - y;
            const double d = dx * dx + dy * dy;
            if (d < min_d) {
                min_d = d;
                idx = i;
            }
        }
    }
    const bool bad_index = np_ < 1 || idx < 0 || idx >= np_;          // IndexError in the reference
    if (bad_index) idx = 0;
    mpc::tracking_error(path, idx, x, y, fi, Vx, Vy, fi_dot, false, o);
    // ---- feed-forward (ref :569-583) and control (ref :606)
    const V4& e = o->e_rr;
    const double K3 = K.v[2];
    double delta_f = o->pk * (prm.a + prm.b - prm.b * K3 -
                              (prm.b / prm.Cf + prm.a * K3 / prm.Cr - prm.a / prm.Cr) * (prm.m * Vx * Vx) / (prm.a + prm.b));
    delta_f = delta_f * 3.141592653589793 / 180.0;
    const double u = -(((K.v[0] * e.v[0] + K.v[1] * e.v[1]) + K.v[2] * e.v[2]) + K.v[3] * e.v[3]) + delta_f;
    const bool ok = inv_ok && !bad_index;
    o->steer = ok ? u : 0.0;
    *K_out = K;
    o->iters = sweeps;
    o->status = bad_index ? kStSOutOfRange : (inv_ok ? 0 : kStQpFailed);
}

// kFused: as mpc_lateral_kernel<true> - one vehicle per lane, so every lane runs its own epilogue.
template <bool kFused>
__global__ void lqr_lateral_kernel(int B, int max_path, mpc::Params prm, const double* __restrict__ target_path,
                                   const int* __restrict__ n_path, const double* __restrict__ state,
                                   const double* __restrict__ vx, const int* __restrict__ min_index_in,
                                   double* __restrict__ steer, double* __restrict__ K_out, double* __restrict__ e_rr_out,
                                   double* __restrict__ k_r_out, int* __restrict__ min_index_out,
                                   double* __restrict__ pre_pro, int* __restrict__ sweeps_out, int* __restrict__ status,
                                   mpc::CtlIO io) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    V4 K;
    mpc::LatResult o;
    // a count beyond the path's row is clamped, never followed
    lqr_lateral_core(prm, target_path + (size_t)b * max_path * 4, min(max(n_path[b], 0), max_path), state[5 * b], state[5 * b + 1],
                     state[5 * b + 2], state[5 * b + 3], state[5 * b + 4], vx[b], min_index_in[b], &K, &o);
    steer[b] = o.steer;
    if (K_out)
#pragma unroll
        for (int j = 0; j < 4; ++j) K_out[4 * b + j] = K.v[j];
    if (e_rr_out)
#pragma unroll
        for (int q = 0; q < 4; ++q) e_rr_out[4 * b + q] = o.e_rr.v[q];
    if (k_r_out) k_r_out[b] = o.pk;
    min_index_out[b] = o.idx;
    if (pre_pro)
#pragma unroll
        for (int q = 0; q < 4; ++q) pre_pro[4 * b + q] = o.pre[q];
    if (sweeps_out) sweeps_out[b] = o.iters;
    status[b] = o.status;
    if constexpr (kFused) mpc::control_epilogue(io, b, o.status, o.steer);
}

}  // namespace lqr

// ---------------------------------------------------------------------------------------------
// Lateral MPC with feed-forward, ref controller/controller.py class Lateral_MPC__with_feedforward_controller (:727-990):
// MPC_control from explicit inputs.  Differences from Lateral_MPC_controller: N = 4 steps x P = 2 controls (:737-739); no
// clamp on Vx (:758-776) but Vx + 0.0001 in the model, its C terms included (:789-809); C_bar with k_r x the RAW Vx (:821);
// e_fi = fi - theta_r, not its sine (:889); the match search covers the whole path (:850-866, min_index is only the fallback);
// Q_bar's first block is Q as well (:934-936, multiplied by C's zero block row); and R_bar regularises only the first P steps'
// controls (`for i in range(P)`, :939-940).  With two controls per step sharing one column of C, H then has a 2-D null space
// along u4 - u5 and u6 - u7: the box barrier still gives the interior point a unique iterate, and u0..u3 and the pair sums
// u4 + u5, u6 + u7 are what the problem determines.
//
// Mapping: one vehicle per GROUP of 8 lanes (lane r owns control r), eight vehicles per wavefront - no idle lane.  The
// nearest-point search is spread over the group's lanes (lane r scans points r, r + 8, ...) and reduced to the smallest
// distance, lowest index on ties (the reference's strict < keeps the first minimum).
// ---------------------------------------------------------------------------------------------
namespace mpcff {

using mpc::M4;
using mpc::V4;
using mpc::grp_bcast;
using mpc::grp_bcast_int;

constexpr int kN = 4, kP = 2, kNu = kN * kP;     // ref :737-739
constexpr int kGroupsPerWave = 64 / kNu;
constexpr int kRegularised = kP * kP;            // R_bar's blocks i < P (ref :939-940): controls 0..3

// ref: Lateral_MPC__with_feedforward_controller.MPC_control (:972-990) for the vehicle of MY 8-lane group (lane r of the group at
// lane gb), from its state in registers (cal_vehicle_info, ref :758-776: no clamp on Vx): the body of mpc_ff_lateral_kernel.
// Arguments as mpc_lateral_core's, idx being only the fallback match.  h, *f_r_out, *u_out: row r of H, f_r and control r
// (lane-local).  *o is group-uniform but for o->steer, which like *u_out is this lane's control: the command, control 0, on the
// group's lane 0, the lane that stores it.  No caller reads it on another lane, so it is not broadcast as mpc_lateral_core's is.
__device__ __forceinline__ void mpc_ff_lateral_core(const mpc::Params& prm, const double* __restrict__ path, int np_, double x,
                                                    double y, double fi, double Vy, double fi_dot, double Vx, int idx, bool live,
                                                    int r, int gb, double (&h)[kNu], double* f_r_out, double* u_out,
                                                    mpc::LatResult* o) {
    M4 A, inv, Ab;
    V4 Bc, Cc, Bb;
    mpc::error_model(prm, Vx + 0.0001, &A, &Bc, &Cc);             // ref :778-809: guarded everywhere, the C terms included
    mpc::predict_pose(Vx, Vy, fi_dot, &x, &y, &fi);                // with the raw Vx
    // ---- match (ref :850-866): the whole path, lane r scanning points r, r + 8, ...
    {
        double best = 10000.0;                                      // squared metres (ref :851)
        int best_i = -1;
        for (int i = r; i < np_; i += kNu) {
            const double dx = path[4 * i] - x, dy = path[4 * i + 1] - y;
            const double d = dx * dx + dy * dy;
            if (d < best) {
                best = d;
                best_i = i;
            }
        }
        double g_best = 10000.0;
        int g_i = -1;
#pragma unroll
        for (int k = 0; k < kNu; ++k) {
            const double dk = grp_bcast(best, gb, k);
            const int ik = grp_bcast_int(best_i, gb, k);
            if (ik >= 0 && (dk < g_best || (dk == g_best && ik < g_i))) {
                g_best = dk;
                g_i = ik;
            }
        }
        if (g_i >= 0) idx = g_i;
    }
    const bool bad_index = live && (np_ < 1 || idx < 0 || idx >= np_);  // IndexError in the reference
    if (bad_index || !live) idx = 0;
    mpc::tracking_error(path, idx, x, y, fi, Vx, Vy, fi_dot, true, o);
    const bool inv_ok = mpc::discretise(A, Bc, &inv, &Ab, &Bb);
    const V4 Cb = mpc::discretise_offset(inv, Cc, o->pk, Vx);      // ref :821: k_r x the RAW Vx
    double f_r;
    mpc::condensed_row<kN, kP>(prm, Ab, Bb, Cb, o->e_rr, r, kRegularised, h, &f_r);
    // ---- box QP (ref :950-970) and outputs
    const bool solvable = live && !bad_index && inv_ok;
    double u = 0.0;
    int it = 0;
    const int rc = mpc::box_qp_full<kNu>(h, f_r, r, gb, solvable, &u, &it);
    const bool ok = solvable && rc == 0;
    *f_r_out = f_r;
    *u_out = ok ? u : 0.0;
    o->steer = ok ? u : 0.0;                                      // ref :990: res['x'][0], on lane 0
    o->iters = it;
    o->status = bad_index ? kStSOutOfRange : ((!inv_ok || rc != 0) ? kStQpFailed : 0);
}

// ref: Lateral_MPC__with_feedforward_controller.MPC_control (:972-990) for B vehicles; grid = ceil(B / 8), block = 64.
__global__ __launch_bounds__(64) void mpc_ff_lateral_kernel(int B, int max_path, mpc::Params prm, const double* __restrict__ target_path,
                                                            const int* __restrict__ n_path, const double* __restrict__ state,
                                                            const double* __restrict__ vx, const int* __restrict__ min_index_in,
                                                            double* __restrict__ steer, double* __restrict__ u_out,
                                                            double* __restrict__ e_rr_out, double* __restrict__ k_r_out,
                                                            int* __restrict__ min_index_out, double* __restrict__ pre_pro,
                                                            double* __restrict__ H_out, double* __restrict__ f_out,
                                                            int* __restrict__ iters_out, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int grp = lane / kNu, r = lane - grp * kNu;
    const int gb = grp * kNu;
    const int b = blockIdx.x * kGroupsPerWave + grp;
    const bool live = b < B;
    const int bb = live ? b : 0;
    double h[kNu], f_r, u;
    mpc::LatResult o;
    // a count beyond the path's row is clamped, never followed
    mpc_ff_lateral_core(prm, target_path + (size_t)bb * max_path * 4, min(max(n_path[bb], 0), max_path), state[5 * bb],
                        state[5 * bb + 1], state[5 * bb + 2], state[5 * bb + 3], state[5 * bb + 4], vx[bb], min_index_in[bb], live, r,
                        gb, h, &f_r, &u, &o);
    if (live) {
        if (H_out)
#pragma unroll
            for (int c = 0; c < kNu; ++c) H_out[((size_t)b * kNu + r) * kNu + c] = h[c];
        if (f_out) f_out[(size_t)b * kNu + r] = f_r;
        if (u_out) u_out[(size_t)b * kNu + r] = u;
        if (r == 0) {
            steer[b] = o.steer;
            if (e_rr_out)
#pragma unroll
                for (int q = 0; q < 4; ++q) e_rr_out[4 * b + q] = o.e_rr.v[q];
            if (k_r_out) k_r_out[b] = o.pk;
            min_index_out[b] = o.idx;
            if (pre_pro)
#pragma unroll
                for (int q = 0; q < 4; ++q) pre_pro[4 * b + q] = o.pre[q];
            if (iters_out) iters_out[b] = o.iters;
            status[b] = o.status;
        }
    }
}

}  // namespace mpcff
}  // namespace emp
