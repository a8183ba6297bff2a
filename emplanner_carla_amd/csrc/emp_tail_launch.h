// emp_tail_launch.h - what host and device agree on about every kernel outside the lattice DP that takes dynamic LDS (projection,
// reference line, path QP, Cartesian tail, the S-T speed stages): the carve-up of that LDS as a struct of offsets, and the launch
// of the kernel - which instantiation, scenes per wavefront, grid, LDS bytes - as pure host arithmetic.  As emp_dp_launch.h: no
// HIP types, readable by a plain C++17 compiler (tests/host_check runs every layout and plan on the CPU;
// tests/golden/tail_launch_plans.npz pins the plans).  The kernels carve their LDS with the layout, emp_api.hip's launchers size
// it with the plan's `lds`, which is the same layout's `total`: one sum, not two.
//
// A slip here shows in no parity test at the benchmark's sizes - only as an LDS access out of bounds at a capacity nobody runs.
#pragma once

#include <stddef.h>

#include "emp_dp_launch.h"
#include "emp_qp_core.h"
#include "emp_st_backend_core.h"
#include "emp_st_core.h"

namespace emp {

constexpr int kRefLinePoints = 51;      // nodes of a cycle's reference line (ref planning_utils.py:231-259: 10 back, 40 forward)
constexpr int kHalfWave = 32;           // the half-wave smoothers take x on lanes 0-31, y on lanes 32-63, one point per lane up to here

// speed_dp_kernel's block (emp_st_kernels.h): 320 lanes = 8 partial minima for each of the 40 destination rows
constexpr int kStBlock = 320;
constexpr int kStWaves = kStBlock / 64;
constexpr int kStParts = kStBlock / st::kRows;
constexpr int kStListCap = 256;         // pair-list entries per wavefront (a longer list is processed in windows)

// ---- layouts ------------------------------------------------------------------------------------------------------------------
// Each is a struct of positions, and ONE function that walks the arrays in order from `at`.  The position type P is the
// kernel's own pointer on the device - the function then IS the kernel's carve-up, the same chain of pointer additions the kernels
// used to spell out - and a plain count from 0 on the host (LdsCount: doubles, or bytes for SpeedDpLds), where `end` is the total
// the launch asks for.
using LdsCount = size_t;

template <class P>
struct ProjectLds {      // frenet_project_wave_kernel: the reference line's x, y, heading, curvature, s_map, cos, sin [max_ref] each
    P lx, ly, lth, lk, sm, lcos, lsin, end;
};
template <class P>
EMP_HD ProjectLds<P> project_lds(P at, int max_ref) {
    ProjectLds<P> L;
    L.lx = at;   at += max_ref;
    L.ly = at;   at += max_ref;
    L.lth = at;  at += max_ref;
    L.lk = at;   at += max_ref;
    L.sm = at;   at += max_ref;
    L.lcos = at; at += max_ref;
    L.lsin = at; at += max_ref;
    L.end = at;
    return L;
}

// smooth_wave_kernel, and the tail of every kernel that smooths a polyline on the whole wavefront: the x and the y problem
// (smooth_pair_wave, emp_qp_wave.h), then the headings heading_kappa_lanes<64> exchanges.  The kernels take `theta` at the scene's
// OWN point count m <= cap (the solver binds its arrays to m): BoxRangeQp::words grows with m, so theta(m) + m <= end(cap).
template <class P>
struct SmoothLds {
    P qmem, theta, end;
};
template <class P>
EMP_HD SmoothLds<P> smooth_lds(P at, int m) {
    SmoothLds<P> L;
    L.qmem = at;  at += 2 * BoxRangeQp::words(m, m);
    L.theta = at; at += m;
    L.end = at;
    return L;
}

template <class P>
struct RefLineLds {      // reference_line_wave_kernel: the gathered nodes [51][2], then a SmoothLds of 51 points
    P gxy;
    SmoothLds<P> smooth;
    P end;
};
template <class P>
EMP_HD RefLineLds<P> ref_line_lds(P at) {
    RefLineLds<P> L;
    L.gxy = at; at += 2 * kRefLinePoints;
    L.smooth = smooth_lds(at, kRefLinePoints);
    L.end = L.smooth.end;
    return L;
}

template <class P>
struct PathQpLds {       // path_qp_wave_kernel: the solver's storage alone
    P qmem, end;
};
template <class P>
EMP_HD PathQpLds<P> path_qp_lds(P at, int cap) {
    return {at, at + path_qp_words(cap)};
}

// cycle_qp_body without the rows solver (R == 0), per group: decimated s, DP l, bounds and result [cap] each, the obstacle table
// [max_obs][4], then the solver's storage - path_qp_words_pair() for two scenes per wavefront (G = 32), path_qp_words(cap) for one
template <class P>
struct CycleQpLds {
    P sd, ld, lmin, lmax, ql, otab, qmem, end;
};
template <class P>
EMP_HD CycleQpLds<P> cycle_qp_lds(P at, bool pair, int cap, int max_obs) {
    CycleQpLds<P> L;
    L.sd = at;   at += cap;
    L.ld = at;   at += cap;
    L.lmin = at; at += cap;
    L.lmax = at; at += cap;
    L.ql = at;   at += cap;
    L.otab = at; at += 4 * max_obs;
    L.qmem = at; at += pair ? path_qp_words_pair() : path_qp_words(cap);
    L.end = at;
    return L;
}

// cycle_cartesian_body<64, 0, WIDE> (one scene per wavefront): s_map [max_ref], trajectory x, y interleaved [cap][2], headings
// [cap], the two smoothing problems (the headings live in `th`, not behind the solver)
template <class P>
struct CartesianLds {
    P sm, txy, th, qmem, end;
};
template <class P>
EMP_HD CartesianLds<P> cartesian_lds(P at, int max_ref, int cap) {
    CartesianLds<P> L;
    L.sm = at;   at += max_ref;
    L.txy = at;  at += 2 * cap;
    L.th = at;   at += cap;
    L.qmem = at; at += 2 * BoxRangeQp::words(cap, cap);
    L.end = at;
    return L;
}

// cycle_cartesian_body<2 GP, R, .> (cycle_cartesian_rows_kernel): a scene's share (as above, then the smoothed x and y [cap] each, no solver) ...
template <class P>
struct CartesianSceneLds {
    P sm, txy, th, px, py, end;
};
template <class P>
EMP_HD CartesianSceneLds<P> cartesian_scene_lds(P at, int max_ref, int cap) {
    CartesianSceneLds<P> L;
    L.sm = at;  at += max_ref;
    L.txy = at; at += 2 * cap;
    L.th = at;  at += cap;
    L.px = at;  at += cap;
    L.py = at;  at += cap;
    L.end = at;
    return L;
}
// ... and the wavefront's: `spw` shares, then the whole-wavefront fall-back's two smoothing problems
EMP_HD LdsCount cartesian_rows_words(int spw, int max_ref, int cap) {
    return (LdsCount)spw * cartesian_scene_lds(LdsCount(0), max_ref, cap).end + 2 * BoxRangeQp::words(cap, cap);
}

template <class P>
struct SpeedQpLds {      // stb::speed_qp_kernel, per group: coefficient slots, the solver's arrays, the set-up's flag word
    P cc, qmem, flag, end;
};
template <class P>
EMP_HD SpeedQpLds<P> speed_qp_lds(P at) {
    SpeedQpLds<P> L;
    L.cc = at;   at += stb::kQp + 2;
    L.qmem = at; at += stb::speed_qp_words(stb::kQp) - (stb::kQp + 2);
    L.flag = at; at += 1;
    L.end = at;
    return L;
}

template <class P>
struct MergeLds {        // stb::merge_kernel: the path's s, x, y, heading, curvature [max_path] each
    P ps, px, py, ph, pk, end;
};
template <class P>
EMP_HD MergeLds<P> merge_lds(P at, int max_path) {
    MergeLds<P> L;
    L.ps = at; at += max_path;
    L.px = at; at += max_path;
    L.py = at; at += max_path;
    L.ph = at; at += max_path;
    L.pk = at; at += max_path;
    L.end = at;
    return L;
}

template <class P>
struct SpeedFrontLds {   // speed_front_wave_kernel: chords and trajectory_index2s [W] each
    P chord, i2s, end;
};
template <class P>
EMP_HD SpeedFrontLds<P> speed_front_lds(P at, int W) {
    return {at, at + W, at + W + W};
}

template <class P>
struct StEdgeLds {       // st_edge_cost_kernel: the scene's obstacle segments and their frames [max_obs] each
    P s_in, s_out, t_in, t_out, ux, uy, len, end;
};
template <class P>
EMP_HD StEdgeLds<P> st_edge_lds(P at, int max_obs) {
    StEdgeLds<P> L;
    L.s_in = at;  at += max_obs;
    L.s_out = at; at += max_obs;
    L.t_in = at;  at += max_obs;
    L.t_out = at; at += max_obs;
    L.ux = at;    at += max_obs;
    L.uy = at;    at += max_obs;
    L.len = at;   at += max_obs;
    L.end = at;
    return L;
}

// speed_dp_kernel, in BYTES (P: a byte pointer, or a count of bytes): doubles, then 32-bit codes, then bytes.  What the arrays
// hold: emp_st_kernels.h StLds, which types these positions.
template <class P>
struct SpeedDpLds {
    P o_s_in, o_s_out, o_t_in, o_t_out, o_ux, o_uy, o_len;      // [max_obs] doubles each
    P iv;               // [2][max_obs][5][2] doubles
    P node_c;           // [40][max_obs]
    P t_tab;            // [10]
    P s_tab;            // [40]
    P part_c;           // [8][40]
    P p_cost, p_sdot;   // [2][40] each
    P row0;             // [16]
    P colmask;          // [2][2] 64-bit masks
    P list_s;           // [waves][cap + 1] doubles
    P list_c;           // [waves][cap + 1] 32-bit codes
    P part_k;           // [8][40] bytes
    P t_node;           // [40][16] bytes
    P end;              // (the launch rounds it up to whole doubles)
};
template <class P>
EMP_HD SpeedDpLds<P> speed_dp_lds(P at, int max_obs) {
    SpeedDpLds<P> L;
    constexpr int kList = kStWaves * (kStListCap + 1);
    L.o_s_in = at;  at += max_obs * 8;
    L.o_s_out = at; at += max_obs * 8;
    L.o_t_in = at;  at += max_obs * 8;
    L.o_t_out = at; at += max_obs * 8;
    L.o_ux = at;    at += max_obs * 8;
    L.o_uy = at;    at += max_obs * 8;
    L.o_len = at;   at += max_obs * 8;
    L.iv = at;      at += 2 * st::kStSamples * 2 * max_obs * 8;
    L.node_c = at;  at += st::kRows * max_obs * 8;
    L.t_tab = at;   at += 2 * st::kStSamples * 8;
    L.s_tab = at;   at += st::kRows * 8;
    L.part_c = at;  at += kStParts * st::kRows * 8;
    L.p_cost = at;  at += 2 * st::kRows * 8;
    L.p_sdot = at;  at += 2 * st::kRows * 8;
    L.row0 = at;    at += st::kCols * 8;
    L.colmask = at; at += 2 * 2 * 8;
    L.list_s = at;  at += kList * 8;
    L.list_c = at;  at += kList * 4;
    L.part_k = at;  at += kStParts * st::kRows;
    L.t_node = at;  at += st::kRows * st::kCols;
    L.end = at;
    return L;
}

// ---- plans -----------------------------------------------------------------------------------------------------------------------
// One struct for all of them.  An empty batch launches nothing: its plan is all zeros and never refused.
struct TailPlan {
    int gp = 0, r = 0;          // the kernel's instantiation where it has several: lanes per group (problem), stations per lane (0:
                                // the one-row-per-lane solvers)
    bool wide = false;          // ... and more than kHalfWave points: the WIDE instantiation of the half-wave smoothers
    bool m32 = false;           // speed_dp_kernel: every obstacle slot fits a 32-bit mask
    int spw = 0;                // scenes per wavefront (per block, for speed_dp_kernel)
    int grid = 0, grid_y = 0, block = 0;
    size_t lds = 0;             // dynamic LDS bytes
    const char* error = nullptr;
};

constexpr const char* kQpTooLarge = "problem too large for the LDS-resident QP solver";
constexpr const char* kProjectTooLong = "reference line too long for the LDS-resident projection kernel";
constexpr const char* kMergeTooLong = "path too long for the LDS-resident merge kernel";
constexpr const char* kSpeedTooLarge = "speed planner's working set too large for the LDS";
constexpr size_t kMergeLdsBytes = 64 * 1024;        // emp_path_speed_merge's own limit, below a compute unit's LDS

// `spw` scenes per 64-lane block, `words` doubles of LDS; refused with `too_large` beyond `limit`
static inline TailPlan tail_plan(int B, int spw, LdsCount words, const char* too_large, size_t limit = kLdsBytes) {
    TailPlan p;
    p.spw = spw;
    p.grid = (int)(((long long)B + spw - 1) / spw);
    p.grid_y = 1;
    p.block = 64;
    p.lds = words * sizeof(double);
    if (p.lds > limit) p.error = too_large;
    return p;
}

static inline TailPlan plan_project(int B, int max_ref) {
    if (B == 0) return {};
    return tail_plan(B, 1, project_lds(LdsCount(0), max_ref).end, kProjectTooLong);
}

static inline TailPlan plan_reference_line(int B) {
    if (B == 0) return {};
    return tail_plan(B, 1, ref_line_lds(LdsCount(0)).end, kQpTooLarge);
}

static inline TailPlan plan_path_qp(int B, int max_pts) {
    if (B == 0) return {};
    return tail_plan(B, 1, path_qp_lds(LdsCount(0), max_pts).end, kQpTooLarge);
}

static inline TailPlan plan_smooth(int B, int max_pts) {
    if (B == 0) return {};
    TailPlan p = tail_plan(B, 1, smooth_lds(LdsCount(0), max_pts).end, kQpTooLarge);
    p.wide = max_pts > kHalfWave;
    return p;
}

// The path QP of a cycle.  path_qp_form 0 (default): the rows kernels (emp_qp_rows.h) - the smallest of <8, 3>, <8, 4>, <16, 4>
// whose GP R + 2 stations hold the scene, eight (four) scenes per wavefront.  path_qp_form 1 (EMP_OPT_PATH_QP_FORM, emp_set_option)
// selects the kernels of rounds 1-2 (two scenes per wavefront up to 34 stations, one beyond): an interior-point iteration
// of that kernel is 2500 instructions against 3000, for the slower of two scenes instead of eight - the form for a caller
// who plans a handful of scenes and counts microseconds.  The two associate their sums differently (~2e-9) and only the
// rows solver restores its last acceptable iterate on a fallback exit, so the choice is the CALLER's and never follows
// the batch size (round 3 switched below 1024 scenes: a 512-scene shard then differed from its slice of a 4096-scene call).
// Beyond the largest rows kernel either form is one scene per wavefront.  lds_pad: development, extra (unused) LDS per rows wavefront.
template <int GP, int R>
static inline bool qp_rows_holds(int B, int cap, int max_obs, size_t lds_pad, TailPlan* p) {
    using L = PathQpRowsLayout<GP, R>;
    if (cap > L::max_stations) return false;
    // the kernel's own carve-up (PathQpRowsLayout, emp_qp_core.h: stride(max_obs) doubles between two groups)
    *p = tail_plan(B, 64 / GP, (size_t)(64 / GP) * L::stride(max_obs), kQpTooLarge);
    p->lds += lds_pad;
    if (p->lds > kLdsBytes) p->error = kQpTooLarge;
    p->gp = GP;
    p->r = R;
    return true;
}
static inline TailPlan plan_cycle_qp(int B, int max_pts, int max_obs, int decimate, int path_qp_form, size_t lds_pad) {
    if (B == 0) return {};
    const int cap = (max_pts + decimate - 1) / decimate;          // most stations a scene can have
    TailPlan p;
    if (path_qp_form != 1 && (qp_rows_holds<8, 3>(B, cap, max_obs, lds_pad, &p) || qp_rows_holds<8, 4>(B, cap, max_obs, lds_pad, &p) ||
                              qp_rows_holds<16, 4>(B, cap, max_obs, lds_pad, &p)))
        return p;
    const bool pair = path_qp_form == 1 && cap <= kPathQpPairStations;
    p = tail_plan(B, pair ? 2 : 1, (pair ? 2 : 1) * cycle_qp_lds(LdsCount(0), pair, cap, max_obs).end, kQpTooLarge);
    p.gp = pair ? 32 : 64;
    return p;
}

// The Cartesian tail of a cycle; cap = path_cap + 1 trajectory points (planning start + path points).  cartesian_form 0 (default):
// cycle_cartesian_rows_kernel, the smallest of <8, 3>, <8, 4>, <16, 4> whose GP R points hold the trajectory - a scene takes
// 2 GP lanes, so four (two) per wavefront.  EMP_OPT_CARTESIAN_FORM = 1 (A/B runs), and anything longer, takes the
// one-scene-per-wavefront kernels cycle_cartesian_wave_kernel_narrow / _wide: the same cycle_cartesian_body on 64 lanes per scene
// (bit-identical results).  (max_pts: the kernels' row stride, no part of the plan.)
template <int GP, int R>
static inline bool cartesian_rows_holds(int B, int max_ref, int cap, TailPlan* p) {
    if (cap > GP * R) return false;
    const int spw = 64 / (2 * GP);
    *p = tail_plan(B, spw, cartesian_rows_words(spw, max_ref, cap), kQpTooLarge);
    p->gp = GP;
    p->r = R;
    return true;
}
static inline TailPlan plan_cycle_cartesian(int B, int max_ref, int /*max_pts*/, int path_cap, int cartesian_form) {
    if (B == 0) return {};
    const int cap = path_cap + 1;
    TailPlan p;
    if (cartesian_form != 1 && (cartesian_rows_holds<8, 3>(B, max_ref, cap, &p) || cartesian_rows_holds<8, 4>(B, max_ref, cap, &p) ||
                                cartesian_rows_holds<16, 4>(B, max_ref, cap, &p)))
        return p;
    p = tail_plan(B, 1, cartesian_lds(LdsCount(0), max_ref, cap).end, kQpTooLarge);
    p.wide = cap > kHalfWave;
    return p;
}

// ---- the S-T speed stages.  Their entry points bound every capacity (64 obstacle slots, 255 path points): none is ever refused,
// and all but the speed DP (55 088 bytes at 64 slots) stay below the 48 KB a kernel gets without opting in (emp_api.hip set_lds) ---------------------------------------------------
static inline TailPlan plan_speed_front(int B, int W) {
    if (B == 0) return {};
    return tail_plan(B, 1, speed_front_lds(LdsCount(0), W).end, kSpeedTooLarge);
}

static inline TailPlan plan_speed_dp(int B, int max_obs) {       // one block of kStBlock lanes per scene
    if (B == 0) return {};
    TailPlan p = tail_plan(B, 1, (speed_dp_lds(LdsCount(0), max_obs).end + 7) / 8, kSpeedTooLarge);      // (bytes to whole doubles)
    p.block = kStBlock;
    p.m32 = max_obs <= 32;
    return p;
}

static inline TailPlan plan_st_edge_cost(int B, int n_edges, int max_obs) {       // one edge per lane, blockIdx.y = scene
    if (B == 0 || n_edges == 0) return {};
    TailPlan p = tail_plan(B, 1, st_edge_lds(LdsCount(0), max_obs).end, kSpeedTooLarge);
    p.grid = (int)(((long long)n_edges + 63) / 64);
    p.grid_y = B;
    return p;
}

static inline TailPlan plan_speed_qp(int B) {                    // two scenes per wavefront, 32 lanes each
    if (B == 0) return {};
    TailPlan p = tail_plan(B, 2, 2 * speed_qp_lds(LdsCount(0)).end, kSpeedTooLarge);
    p.gp = 32;
    return p;
}

// (refused before the empty batch is let through: emp_path_speed_merge checks its sizes before it stages anything)
static inline TailPlan plan_merge(int B, int max_path) {
    const TailPlan p = tail_plan(B, 1, merge_lds(LdsCount(0), max_path).end, kMergeTooLong, kMergeLdsBytes);
    return p.error || B ? p : TailPlan{};
}

}  // namespace emp
