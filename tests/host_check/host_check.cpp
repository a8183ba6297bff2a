// host_check.cpp - runs the scalar building blocks of csrc/*.h on the CPU for the `-m "not gpu"` suite.
// TEST TOOL ONLY: compiled with g++ into tests/host_check/_build/, loaded by tests/test_host_logic.py,
// never by the package.  It lets kernel *logic* (banded QP, Frenet helpers, edge arithmetic) be checked
// against the oracle without a GPU; GPU parity proper is tests/test_gpu_*.py through the C-ABI.
#include "../../emplanner_carla_amd/csrc/emp_core.h"
#include "../../emplanner_carla_amd/csrc/emp_dp_launch.h"
#include "../../emplanner_carla_amd/csrc/emp_frenet_core.h"
#include "../../emplanner_carla_amd/csrc/emp_qp_core.h"
#include "../../emplanner_carla_amd/csrc/emp_st_core.h"
#include "../../emplanner_carla_amd/csrc/emp_st_backend_core.h"
#include "../../emplanner_carla_amd/csrc/emp_tail_launch.h"

#include <initializer_list>
#include <string_view>

using namespace emp;

extern "C" {

double hc_segment_cost(double l0, double dl0, double ddl0, double l1, double s0, double sample_s, const double* obs_s,
                       const double* obs_l, int n_obs, double w_coll, double w0, double w1, double w2, double w_ref) {
    const Quintic q = quintic_shifted(l0, dl0, ddl0, l1, sample_s);
    return segment_cost(q, s0, sample_s, obs_s, obs_l, n_obs, w_coll, w0, w1, w2, w_ref);
}

double hc_neighbour_cost(double l0, double l1, double s0, double sample_s, const double* obs_s, const double* obs_l, int n_obs,
                         double w_coll, double w0, double w1, double w2, double w_ref) {
    return neighbour_cost(l0, l1, s0, sample_s, obs_s, obs_l, n_obs, w_coll, w0, w1, w2, w_ref);
}

int hc_path_qp(int n, const double* l_min, const double* l_max, double l0, double dl0, double ddl0, const double* prm8,
               double* out_l, double* out_dl, double* out_ddl, int* iters) {
    static double mem[path_qp_words(256)];
    if (n > 256) return 2;
    PathQpParams p{prm8[0], prm8[1], prm8[2], prm8[3], prm8[4], prm8[5], prm8[6], prm8[7]};
    return path_qp_solve_scalar(mem, l_min, l_max, n, l0, dl0, ddl0, p, out_l, out_dl, out_ddl, iters);
}

int hc_path_qp_gi(int n, const double* l_min, const double* l_max, double l0, double dl0, double ddl0, const double* prm8,
                  double* out_l, double* out_dl, double* out_ddl, int* iters) {
    static double mem[path_qp_words(256)];
    static double work[gi_words(256)];
    if (n > 256) return 2;
    PathQpParams p{prm8[0], prm8[1], prm8[2], prm8[3], prm8[4], prm8[5], prm8[6], prm8[7]};
    return path_qp_solve_scalar(mem, l_min, l_max, n, l0, dl0, ddl0, p, out_l, out_dl, out_ddl, iters, work);
}

int hc_box_qp(int m, const double* ref, int stride, double w_smooth, double w_length, double w_ref, double thr,
              double* out, int* iters) {
    static double mem[BoxRangeQp::words(256, 256)];
    *iters = 0;
    if (m > 256 || m < 2) return 2;
    BoxRangeQp Q;
    Q.bind(mem, m, m);
    SmoothQpParams p{w_smooth, w_length, w_ref, thr};
    int rc = box_qp_setup(Q, ref, stride, m, p);
    if (rc) return rc;
    rc = Q.solve_scalar();
    *iters = Q.iters;
    for (int i = 0; i < m; ++i) out[i] = Q.u[i];
    return rc;
}

void hc_heading_kappa(const double* xy, int m, double* theta, double* kappa) { heading_kappa(xy, 2, m, theta, 1, kappa, 1); }

void hc_s_map(const double* line, int n_ref, double ox, double oy, double* s_map) { s_map_build(line, n_ref, ox, oy, s_map); }

void hc_dot2(int n, const double* a, const double* b, double* out) {     // a, b: [n][2]
    for (int i = 0; i < n; ++i) out[i] = dot2(a[2 * i], a[2 * i + 1], b[2 * i], b[2 * i + 1]);
}

int hc_match(const double* line, int n_ref, double x, double y, int first, int step, int limit) {
    return match_scan(line, n_ref, x, y, first, step, limit);
}

// ---- the station lookups (emp_frenet_core.h): the text the kernels of emp_tail_kernels.h run ------
// cal_proj_point: out[4] = x, y, theta, kappa; *idx in: the previous index, out: the walk's; returns 1 where the walk stops in range
int hc_proj_point(const double* line, const double* s_map, int n_ref, double s, int* idx, double* out) {
    Node pr{0, 0, 0, 0};
    const bool ok = proj_point(line, s_map, n_ref, s, idx, &pr);
    out[0] = pr.x; out[1] = pr.y; out[2] = pr.theta; out[3] = pr.kappa;
    return ok ? 1 : 0;
}

int hc_walk_from_zero(const double* s_map, int n_ref, double s, int* off_end) {
    bool off = false;
    const int k = walk_from_zero(s_map, n_ref, s, &off);
    *off_end = off ? 1 : 0;
    return k;
}

// one pass over the stations (one[3]) next to three argmin_abs calls (three[3]), targets t[3]
void hc_argmin_abs3(const double* s, int n, const double* t, int* one, int* three) {
    argmin_abs3(s, n, t[0], t[1], t[2], &one[0], &one[1], &one[2]);
    for (int k = 0; k < 3; ++k) three[k] = argmin_abs(s, 1, n, t[k]);
}

int hc_lmin_lmax(const double* dp_s, const double* dp_l, int n, const double* obs_s, const double* obs_l, int n_obs,
                 double obs_length, double obs_width, double* l_min, double* l_max) {
    return lmin_lmax(dp_s, dp_l, 1, n, obs_s, obs_l, n_obs, obs_length, obs_width, l_min, l_max) ? 1 : 0;
}

// ---- S-T speed DP scalar pieces (emp_st_core.h) ---------------------------------------------------
double hc_st_edge_cost(const double* w4, const double* edge5, int n_obs, const double* s_in, const double* s_out,
                       const double* t_in, const double* t_out, double* obs) {
    const st::Weights w{w4[0], w4[1], w4[2], st::make_pow_base(w4[3])};
    double ux[st::kMaxObs], uy[st::kMaxObs], len[st::kMaxObs];
    for (int j = 0; j < n_obs; ++j) st::obs_frame(s_in[j], t_in[j], s_out[j], t_out[j], &ux[j], &uy[j], &len[j]);
    const st::ObsSet set{n_obs, s_in, s_out, t_in, t_out, ux, uy, len};
    return st::edge_cost(w, edge5[0], edge5[1], edge5[2], edge5[3], edge5[4], set, obs);
}

// speed DP kernel, round 3: the branch-free pair cost against the reference-order one, and whether the sample lies inside
// the segment's reach interval at its time (it must whenever the pair costs anything)
void hc_st_reach(int n, double w_obs, const double* seg4, const double* pt2, double* cost, double* cost_flat, int* inside,
                 double* lo_hi) {
    const st::PowBase w = st::make_pow_base(w_obs);
    for (int i = 0; i < n; ++i) {
        const double s_in = seg4[4 * i], t_in = seg4[4 * i + 1], s_out = seg4[4 * i + 2], t_out = seg4[4 * i + 3];
        const double s = pt2[2 * i], t = pt2[2 * i + 1];
        cost[i] = st::point_cost(w, s, t, s_in, t_in, s_out, t_out);
        cost_flat[i] = st::point_cost_flat(w, s, t, s_in, t_in, s_out, t_out);
        double ux, uy, len, lo, hi;
        st::obs_frame(s_in, t_in, s_out, t_out, &ux, &uy, &len);
        st::reach_interval(t, s_in, t_in, ux, uy, len, &lo, &hi);
        inside[i] = s > lo && s < hi;
        lo_hi[2 * i] = lo;
        lo_hi[2 * i + 1] = hi;
    }
}

void hc_st_graph(int n, const double* s, const double* l, const double* sd, const double* ld, double* s_in, double* s_out,
                 double* t_in, double* t_out) {
    st::st_graph(n, s, l, sd, ld, s_in, s_out, t_in, t_out);
}

void hc_st_grid(double* s_rows, double* t_cols) {
    for (int r = 0; r < st::kRows; ++r) s_rows[r] = st::s_of_row(r);
    for (int c = 0; c < st::kCols; ++c) t_cols[c] = st::t_of_col(c);
}

int hc_st_terminal(const double* cost, int* row, int* col) {
    return st::terminal_node([&](int r, int c) { return cost[r * st::kCols + c]; }, row, col) ? 1 : 0;
}


// ---- S-T speed planning back end (emp_st_backend_core.h) ------------------------------------
int hc_stb_convex_space(const double* dp_s, const double* dp_t, const double* idx2s, const double* kappa, int path_len,
                        const double* s_in, const double* s_out, const double* t_in, const double* t_out, int n_slots,
                        double max_lat, double* s_lb, double* s_ub, double* sd_lb, double* sd_ub) {
    return stb::convex_space(dp_s, dp_t, idx2s, kappa, path_len, s_in, s_out, t_in, t_out, n_slots, max_lat, s_lb, s_ub,
                             sd_lb, sd_ub);
}

int hc_stb_speed_qp(const double* dp_s, const double* dp_t, double v0, double a0, const double* s_lb, const double* s_ub,
                    const double* sd_lb, const double* sd_ub, const double* w4, double* qs, double* qv, double* qa,
                    double* qt, int* iters) {
    static double mem[stb::speed_qp_words(stb::kQp)];
    const stb::SpeedQpParams prm{w4[0], w4[1], w4[2], w4[3]};
    return stb::speed_qp_solve_scalar(mem, dp_s, dp_t, v0, a0, s_lb, s_ub, sd_lb, sd_ub, prm, qs, qv, qa, qt, iters);
}

// increase_points with the kernel's structure: match per sample, running maximum as the sticky interval
int hc_stb_increase_points(const double* qs, const double* qv, const double* qa, const double* qt, double* s, double* v,
                           double* a, double* t) {
    const int t_end = stb::dense_t_end(qt);
    if (t_end >= stb::kQp || t_end < 0) return t_end < 0 ? stb::kStbNoProfile : stb::kStbIndex;
    const double dt = qt[t_end] / (double)(stb::kDense - 1);
    int tmp = 0;
    for (int i = 0; i < stb::kDense; ++i) {
        const double cur = (double)(i - 1) * dt;
        const int m = stb::dense_match(qt, t_end, cur);
        if (m > tmp) tmp = m;
        stb::dense_sample(qs, qv, qa, qt, tmp, cur, &s[i], &v[i], &a[i]);
        t[i] = cur;
    }
    return 0;
}

double hc_stb_np_interp(const double* xp, const double* fp, int n, double x) {
    return stb::np_interp_at(xp, fp, n, (x != x) ? 0 : stb::np_interp_index(xp, n, x), x);
}

// ---- launch geometry of the lattice-DP kernels (emp_dp_launch.h) --------------------------------
// Each writes its plan into `out` (zeros when the plan is refused) and returns the refusal text, or NULL.
static DpDev hc_dp_dev(int row, int col, int B, int max_obs) {      // as emp_api.hip make_dp_dev
    DpDev d{};
    d.row = row;
    d.col = col;
    d.S = dp_tiling(row, B).S;
    d.tiles = dp_tiling(row, B).tiles;
    d.B = B;
    d.max_obs = max_obs > 0 ? max_obs : 1;
    return d;
}

const char* hc_plan_edge(int row, int col, int B, int max_obs, int tiled, int edge_form, int edge_block, long long* out) {
    const EdgePlan p = plan_edge(hc_dp_dev(row, col, B, max_obs), tiled != 0, edge_form, edge_block, 0);
    const long long v[10] = {p.wide, p.ring, p.m32, p.row_inst, p.wpb, p.cols_per_chunk, p.grid_x, p.grid_y, p.block, (long long)p.lds};
    for (int i = 0; i < 10; ++i) out[i] = p.error ? 0 : v[i];
    return p.error;
}

const char* hc_plan_sweep(int row, int col, int B, int max_obs, long long* out) {
    const SweepPlan p = plan_sweep(hc_dp_dev(row, col, B, max_obs));
    const long long v[6] = {p.row_inst, p.pd, p.nt, p.grid, p.block, (long long)p.lds};
    for (int i = 0; i < 6; ++i) out[i] = p.error ? 0 : v[i];
    return p.error;
}

const char* hc_plan_fused(int row, int col, int B, int max_obs, long long* out) {
    const FusedPlan p = plan_fused(hc_dp_dev(row, col, B, max_obs));
    out[0] = p.error ? 0 : p.nc;
    out[1] = p.error ? 0 : (long long)p.lds;
    return p.error;
}

const char* hc_plan_enrich(int row, int col, int B, int max_obs, int with_pre, long long* out) {
    const EnrichPlan p = plan_enrich(hc_dp_dev(row, col, B, max_obs), with_pre != 0);
    out[0] = p.error ? 0 : (long long)p.lds;
    return p.error;
}

long long hc_edge_tensor_elems(int row, int col, int B, int tiled) { return (long long)edge_tensor_elems(row, col, B, tiled != 0); }

// the constants the ring kernel's LDS carve-up is made of: kTableFields, kRingSlots, kRingMaxCol, then edge_ring_bytes(max_obs)
void hc_edge_ring_constants(int max_obs, long long* out) {
    out[0] = kTableFields;
    out[1] = kRingSlots;
    out[2] = kRingMaxCol;
    out[3] = edge_ring_bytes(max_obs);
}

// A DP kernel's LDS layout: its positions counted from 0, in the struct's order, `end` last; returns how many.  a .. e are the
// layout function's own arguments, in its order.  Doubles, but bytes for "edge_ring", "enrich" and "fused".
int hc_dp_layout(const char* name, int a, int b, int c, int d, int e, long long* out) {
    const LdsCount z = 0;
    const std::string_view n(name);
    int k = 0;
    auto put = [&](std::initializer_list<LdsCount> v) {
        for (LdsCount x : v) out[k++] = (long long)x;
        return k;
    };
    if (n == "edge") { const auto L = edge_lds(z, a, b, c, d, e); return put({L.tab, L.obs_s, L.obs_l, L.smp, L.box, L.end}); }
    if (n == "edge_ring") { const auto L = edge_ring_lds(z, a, b, c, d, e); return put({L.tab, L.obs_s, L.obs_l, L.ps, L.band, L.rings, L.f, L.end}); }
    if (n == "sweep") { const auto L = sweep_lds(z, a, b); return put({L.front, L.pre, L.end}); }
    if (n == "sweep_wide") { const auto L = sweep_wide_lds(z, a); return put({L.cur, L.nxt, L.end}); }
    if (n == "enrich") { const auto L = enrich_lds(z, a, b, c != 0); return put({L.rows, L.bt, L.end}); }
    if (n == "fused") { const auto L = fused_lds(z, a, b, c, d, e); return put({L.tab, L.smp, L.obs_s, L.obs_l, L.buf, L.front, L.pre, L.ctr, L.end}); }
    return 0;
}

// ---- launch plans and LDS layouts of every other kernel with dynamic LDS (emp_tail_launch.h) -------------------------------
// A plan: its nine fields into `out` (zeros when refused), the refusal text or NULL returned.
static const char* hc_put(const TailPlan& p, long long* out) {
    const long long v[9] = {p.gp, p.r, p.wide, p.m32, p.spw, p.grid, p.grid_y, p.block, (long long)p.lds};
    for (int i = 0; i < 9; ++i) out[i] = p.error ? 0 : v[i];
    return p.error;
}
const char* hc_plan_project(int B, int max_ref, long long* out) { return hc_put(plan_project(B, max_ref), out); }
const char* hc_plan_reference_line(int B, long long* out) { return hc_put(plan_reference_line(B), out); }
const char* hc_plan_cycle_qp(int B, int max_pts, int max_obs, int decimate, int form, long long* out) {
    return hc_put(plan_cycle_qp(B, max_pts, max_obs, decimate, form, 0), out);
}
const char* hc_plan_cycle_cartesian(int B, int max_ref, int max_pts, int path_cap, int form, long long* out) {
    return hc_put(plan_cycle_cartesian(B, max_ref, max_pts, path_cap, form), out);
}
const char* hc_plan_path_qp(int B, int max_pts, long long* out) { return hc_put(plan_path_qp(B, max_pts), out); }
const char* hc_plan_smooth(int B, int max_pts, long long* out) { return hc_put(plan_smooth(B, max_pts), out); }
const char* hc_plan_speed_front(int B, int W, long long* out) { return hc_put(plan_speed_front(B, W), out); }
const char* hc_plan_speed_dp(int B, int max_obs, long long* out) { return hc_put(plan_speed_dp(B, max_obs), out); }
const char* hc_plan_st_edge_cost(int B, int n_edges, int max_obs, long long* out) {
    return hc_put(plan_st_edge_cost(B, n_edges, max_obs), out);
}
const char* hc_plan_speed_qp(int B, long long* out) { return hc_put(plan_speed_qp(B), out); }
const char* hc_plan_merge(int B, int max_path, long long* out) { return hc_put(plan_merge(B, max_path), out); }

// A layout: its positions counted from 0, in the struct's order, `end` last; returns how many.  a, b, c are the layout
// function's own arguments, in its order.
int hc_tail_layout(const char* name, int a, int b, int c, long long* out) {
    const LdsCount z = 0;
    const std::string_view n(name);
    int k = 0;
    auto put = [&](std::initializer_list<LdsCount> v) {
        for (LdsCount x : v) out[k++] = (long long)x;
        return k;
    };
    if (n == "project") { const auto L = project_lds(z, a); return put({L.lx, L.ly, L.lth, L.lk, L.sm, L.lcos, L.lsin, L.end}); }
    if (n == "smooth") { const auto L = smooth_lds(z, a); return put({L.qmem, L.theta, L.end}); }
    if (n == "ref_line") { const auto L = ref_line_lds(z); return put({L.gxy, L.smooth.qmem, L.smooth.theta, L.end}); }
    if (n == "path_qp") { const auto L = path_qp_lds(z, a); return put({L.qmem, L.end}); }
    if (n == "cycle_qp") { const auto L = cycle_qp_lds(z, a != 0, b, c); return put({L.sd, L.ld, L.lmin, L.lmax, L.ql, L.otab, L.qmem, L.end}); }
    if (n == "cartesian") { const auto L = cartesian_lds(z, a, b); return put({L.sm, L.txy, L.th, L.qmem, L.end}); }
    if (n == "cartesian_scene") { const auto L = cartesian_scene_lds(z, a, b); return put({L.sm, L.txy, L.th, L.px, L.py, L.end}); }
    if (n == "cartesian_rows") return put({cartesian_rows_words(a, b, c)});
    if (n == "speed_qp") { const auto L = speed_qp_lds(z); return put({L.cc, L.qmem, L.flag, L.end}); }
    if (n == "merge") { const auto L = merge_lds(z, a); return put({L.ps, L.px, L.py, L.ph, L.pk, L.end}); }
    if (n == "speed_front") { const auto L = speed_front_lds(z, a); return put({L.chord, L.i2s, L.end}); }
    if (n == "st_edge") { const auto L = st_edge_lds(z, a); return put({L.s_in, L.s_out, L.t_in, L.t_out, L.ux, L.uy, L.len, L.end}); }
    if (n == "speed_dp") {
        const auto L = speed_dp_lds(z, a);
        return put({L.o_s_in, L.o_s_out, L.o_t_in, L.o_t_out, L.o_ux, L.o_uy, L.o_len, L.iv, L.node_c, L.t_tab, L.s_tab, L.part_c, L.p_cost,
                    L.p_sdot, L.row0, L.colmask, L.list_s, L.list_c, L.part_k, L.t_node, L.end});
    }
    return 0;
}

// what the layouts are made of: the solvers' storage for n stations / points, and the rows path QP's stride and capacity
void hc_tail_constants(int n, int max_obs, long long* out) {
    out[0] = path_qp_words(n);
    out[1] = path_qp_words_pair();
    out[2] = kPathQpPairStations;
    out[3] = BoxRangeQp::words(n, n);
    out[4] = stb::speed_qp_words(stb::kQp);
    out[5] = kHalfWave;
    out[6] = kRefLinePoints;
    out[7] = PathQpRowsLayout<8, 3>::stride(max_obs);
    out[8] = PathQpRowsLayout<8, 4>::stride(max_obs);
    out[9] = PathQpRowsLayout<16, 4>::stride(max_obs);
    out[10] = kStWaves * (kStListCap + 1);
    out[11] = kStParts;
}

}  // extern "C"
