// emp_tail_kernels.h - everything of one planning cycle around the DP: Cartesian->Frenet projection,
// QP bounds, path QP, midpoint re-interleave, Frenet->Cartesian, smoothing QP, heading/curvature.
//
// Mapping: the kernels of emp_plan_cycle run one scene per wavefront (or per half wavefront) with the reference
// line, the path and the QP state in LDS / registers; the stand-alone per-function kernels of the utilities keep
// the simple one-scene-per-lane form.  "ref:" cites the reference (paths relative to the reference tree).
#pragma once

#include <hip/hip_runtime.h>

#include "emp_core.h"
#include "emp_frenet_core.h"
#include "emp_qp_core.h"
#include "emp_qp_wave.h"
#include "emp_qp_rows.h"
#include "emp_smooth_rows.h"
#include "emp_tail_launch.h"

namespace emp {

// status bits (mirror include/emplanner.h)
constexpr int kStDpInfeasible = 1, kStSOutOfRange = 2, kStBoundIndex = 4, kStQpFailed = 8, kStSmoothFailed = 16,
              kStTruncated = 32;

struct QpDev {
    PathQpParams qp;
    double obs_length, obs_width;
    int decimate, midpoint, use_qp;
    int debug_stage;   // development only: cut the QP kernel short after stage N (0 = run everything)
};

// ---------------------------------------------------------------------------------------------
// ref: test_9.py:113-177 - s_map, obstacle (s, l), planning-start (s, l) and (l, dl/ds, d2l/ds2)
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Wave-parallel form of the cycle front (one wavefront per scene, one reference-line node per lane).
// The reference's nearest-node scan (planning_utils.py:383-402) is an ordered scan with an early exit after
// 50 consecutive non-improvements; in parallel that is: L_i = first index achieving min(d_0..d_i) (a prefix
// minimum that keeps the FIRST occurrence, because only a strict '<' counts as an improvement), stop at the first
// i with i - L_i >= 50, answer L_i there (or L_{P-1} if the scan never stops early).  A distance that is not `< inf` (NaN, +inf) never
// improves and counts from node 0 on: until the first improvement L_i is "-1", so a line whose first 50 distances are all such
// stops at node 49 with the scan's initial answer, node 0 (tests/match_cases.py holds the ties, stop boundaries and non-finite
// lines that pin all of this against the serial match_scan).
// ---------------------------------------------------------------------------------------------
// Inclusive prefix minimum of (d, index) over the 64 lanes, the EARLIER lane winning ties, by DPP moves (no LDS
// traffic, no address arithmetic): Hillis-Steele inside each row of 16 lanes (row_shr:1, 2, 4, 8; a lane without a
// source keeps +inf), then the row totals travel on with row_bcast:15 (into rows 1 and 3) and row_bcast:31 (into
// rows 2 and 3).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void prefix_min_step(double& d, int& li) {
    union { double f; int w[2]; } a, r, inf;
    a.f = d;
    inf.f = __builtin_inf();
    r.w[0] = __builtin_amdgcn_update_dpp(inf.w[0], a.w[0], CTRL, ROW_MASK, 0xF, false);
    r.w[1] = __builtin_amdgcn_update_dpp(inf.w[1], a.w[1], CTRL, ROW_MASK, 0xF, false);
    const int oi = __builtin_amdgcn_update_dpp(0, li, CTRL, ROW_MASK, 0xF, false);
    if (!(d < r.f)) {                  // the value from the earlier lanes wins unless mine is strictly smaller;
        d = r.f;                       // a lane without a source sees +inf and keeps its own unless that is +inf (the caller
                                       // hands in no NaN: it would win this comparison and travel down the prefix)
        li = oi;
    }
}
__device__ __forceinline__ void prefix_min_first(double& d, int& li) {
    prefix_min_step<0x111, 0xF>(d, li);   // row_shr:1
    prefix_min_step<0x112, 0xF>(d, li);   // row_shr:2
    prefix_min_step<0x114, 0xF>(d, li);   // row_shr:4
    prefix_min_step<0x118, 0xF>(d, li);   // row_shr:8
    prefix_min_step<0x142, 0xA>(d, li);   // row_bcast:15 -> rows 1, 3
    prefix_min_step<0x143, 0xC>(d, li);   // row_bcast:31 -> rows 2, 3
}

// One step of a value-only inclusive prefix minimum (lanes without a source, or outside the row mask, see +inf)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double prefix_fmin_step(double v) {
    union { double f; int w[2]; } a, r, inf;
    a.f = v;
    inf.f = __builtin_inf();
    r.w[0] = __builtin_amdgcn_update_dpp(inf.w[0], a.w[0], CTRL, ROW_MASK, 0xF, false);
    r.w[1] = __builtin_amdgcn_update_dpp(inf.w[1], a.w[1], CTRL, ROW_MASK, 0xF, false);
    return __builtin_fmin(v, r.f);
}

// The scan for lines of at most 64 nodes (one node per lane; the cycle's 51- and 61-node lines), without carrying the index
// through the prefix: with pm_i = min(d_0..d_i), the first occurrence L_i of pm_i satisfies i - L_i >= limit exactly when
// pm_i == pm_{i-limit} (no strict improvement among the last `limit` nodes), so the stopping node i* is the first lane where
// that holds and the answer is the first lane j <= i* with d_j == pm_{i*} - or, if the scan never stops, the first lane that
// attains the overall minimum.  Half the instructions of the indexed prefix (round 3).
__device__ inline int match_scan_wave64(const double* lx, const double* ly, int P, double x, double y, int limit) {
    const int lane = threadIdx.x & 63;
    double d = __builtin_inf();
    if (lane < P) {
        const double dx = lx[lane] - x, dy = ly[lane] - y;
        d = sqrt(dx * dx + dy * dy);
    }
    // A distance that is not `< inf` (NaN, or +inf itself) is a non-improvement from node 0 on: where none of the first `limit`
    // nodes improves, the ordered scan has stopped at node limit - 1 with its initial answer, node 0.  The prefix below cannot
    // see that stop (pm is +inf there, and a finite node `limit` differs from it).
    if (P >= limit && !__ballot(lane < limit && d < __builtin_inf())) return 0;   // uniform
    double pm = d;
    pm = prefix_fmin_step<0x111, 0xF>(pm);   // row_shr:1
    pm = prefix_fmin_step<0x112, 0xF>(pm);   // row_shr:2
    pm = prefix_fmin_step<0x114, 0xF>(pm);   // row_shr:4
    pm = prefix_fmin_step<0x118, 0xF>(pm);   // row_shr:8
    pm = prefix_fmin_step<0x142, 0xA>(pm);   // row_bcast:15 -> rows 1, 3
    pm = prefix_fmin_step<0x143, 0xC>(pm);   // row_bcast:31 -> rows 2, 3
    const double back = __shfl(pm, lane >= limit ? lane - limit : 0, 64);
    const unsigned long long stop = __ballot(lane < P && lane >= limit && pm == back);
    const int last = stop ? __builtin_ffsll((long long)stop) - 1 : P - 1;          // the node at which the scan ends
    const double target = __shfl(pm, last, 64);
    const unsigned long long hit = __ballot(lane <= last && d == target);
    return hit ? __builtin_ffsll((long long)hit) - 1 : 0;                           // (no finite distance at all: node 0)
}

__device__ inline int match_scan_wave(const double* lx, const double* ly, int P, double x, double y, int limit) {
    if (P <= 64 && limit >= 1) return match_scan_wave64(lx, ly, P, x, y, limit);   // uniform
    const int lane = threadIdx.x & 63;
    double cd = __builtin_inf();     // carry: prefix minimum and its first index over the previous chunks
    int ci = -1;                     // -1: nothing has improved yet.  The ordered scan counts non-improvements from node 0, so
                                     // it stops at node limit - 1 where no distance so far was `< inf` (NaN, +inf): answer 0
    for (int base = 0; base < P; base += 64) {
        const int i = base + lane;
        double d = __builtin_inf();
        int li = i;
        if (i < P) {
            const double dx = lx[i] - x, dy = ly[i] - y;
            d = sqrt(dx * dx + dy * dy);
            // A NaN distance is passed over like +inf: it is never `<` another.  As NaN it would travel down the prefix instead -
            // `!(d < NaN)` hands a later lane the NaN in place of its own strictly smaller distance.
            if (!(d < __builtin_inf())) d = __builtin_inf();
        }
        prefix_min_first(d, li);                           // inclusive prefix-min keeping the earlier index on ties
        if (!(d < cd)) {                                   // fold the carry (earlier) in
            d = cd;
            li = ci;
        }
        const unsigned long long stop = __ballot(i < P && i - li >= limit);
        if (stop) {
            const int first = __builtin_ffsll((long long)stop) - 1;
            return max(__shfl(li, first, 64), 0);
        }
        const int last = min(63, P - 1 - base);
        cd = __shfl(d, last, 64);
        ci = __shfl(li, last, 64);
    }
    return max(ci, 0);
}

// dynamic LDS: ProjectLds (emp_tail_launch.h)
__global__ __launch_bounds__(64) void frenet_project_wave_kernel(
    int B, int max_ref, int max_obs, const double* __restrict__ ref_line, const int* __restrict__ n_ref,
    const double* __restrict__ origin_xy, const double* __restrict__ start_xy, const double* __restrict__ start_v,
    const double* __restrict__ start_a, const double* __restrict__ obs_xy, const int* __restrict__ n_obs,
    double* __restrict__ s_map, double* __restrict__ obs_s, double* __restrict__ obs_l, double* __restrict__ begin_sl,
    double* __restrict__ start, int obs_cap, const double* __restrict__ dyn, int* __restrict__ n_obs_out) {
    __builtin_amdgcn_s_setprio(EMP_PRIO_FRONT);
    // obs_xy rows hold max_obs slots, obs_s / obs_l rows obs_cap >= max_obs (+3 when `dyn` is given: the virtual
    // obstacles of test_9.py:137-169 are appended behind the projected ones and n_obs_out gets the total)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const ProjectLds<double*> L = project_lds(lds, max_ref);
    double *lx = L.lx, *ly = L.ly, *lth = L.lth, *lk = L.lk, *sm = L.sm;
    double *lcos = L.lcos, *lsin = L.lsin;              // cos / sin of every node's heading: each node one lane, once per
                                                        // scene - the ten projections below read them instead of calling
    const double* line = ref_line + (size_t)b * max_ref * 4;   // cos / sin again (half of this kernel's instructions were those calls)
    const int P = min(max(n_ref[b], 0), max_ref);       // clamped to the row's capacity
    // Every coordinate the ten match scans below start from is fetched HERE, next to the reference line: one round trip
    // to memory for the whole kernel.  Loaded where they are used - one obstacle per scan, each scan behind the previous
    // one - they cost a dependent trip each: a third of the kernel's 30 us, on the queue that is the step's critical path.
    const int k = n_obs ? min(max(n_obs[b], 0), max_obs) : 0;   // clamped to the row's capacity
    const double ox = origin_xy[2 * b], oy = origin_xy[2 * b + 1];
    const double px = start_xy[2 * b], py = start_xy[2 * b + 1];
    double obx = 0.0, oby = 0.0;                        // obstacle `lane` of the first 64 (the rest are loaded in the loop)
    if (lane < k) {
        obx = obs_xy[((size_t)b * max_obs + lane) * 2];
        oby = obs_xy[((size_t)b * max_obs + lane) * 2 + 1];
    }
    for (int i = lane; i < P; i += 64) {
        lx[i] = line[4 * i];
        ly[i] = line[4 * i + 1];
        const double th = line[4 * i + 2];
        lth[i] = th;
        lk[i] = line[4 * i + 3];
        double sn, cs;
        sincos_pair(th, &sn, &cs);
        lcos[i] = cs;
        lsin[i] = sn;
    }
    // An empty line (the reference raises IndexError; the Cartesian tail refuses the scene): every scan below answers node 0,
    // which nothing has loaded.  It reads as a node at the origin with heading 0, so that the scene's Frenet outputs - and the
    // DP the cycle runs on them - are the same bits in any batch, not what an earlier kernel left in LDS.
    if (P == 0 && lane == 0) {
        lx[0] = ly[0] = lth[0] = lk[0] = sm[0] = lsin[0] = 0.0;
        lcos[0] = 1.0;
    }
    __syncthreads();
    // cumulative chord length (ref planning_utils.py:461-466).  The chords are computed one per lane, but the
    // running sum is formed strictly left to right like the reference's loop: the planning-start s inherits its
    // last bits, and with an integer sample_s those bits decide int(end_s - start_s), i.e. the number of
    // densified points (path_planning.py:405).
    double carry = 0.0;
    for (int base = 0; base < P; base += 64) {
        const int i = base + lane;
        double d = 0.0;
        if (i >= 1 && i < P) {
            const double dx = lx[i] - lx[i - 1], dy = ly[i] - ly[i - 1];
            d = sqrt(dx * dx + dy * dy);
        }
        // s_i = chord_i + s_{i-1}, one add per point in the reference's order.  As a lane-shift sweep (emp_qp_wave.h): every
        // lane adds its chord to its left neighbour's CURRENT sum at every step, lanes 0..k are final after step k - three
        // vector instructions per step where the loop over readlane'd chords took fourteen (a quarter of this kernel).
        const int cnt = min(64, P - base);
        if (lane == 0) d = (base >= 1) ? d + carry : 0.0;            // the chunk's first point continues the previous chunk
        double mine = d;
        for (int k = 1; k < cnt; ++k) mine = d + lane_up1(mine);     // lane 0: neighbour reads 0, d + 0.0 == d bit for bit
        carry = __shfl(mine, cnt - 1, 64);
        if (i < P) sm[i] = mine;
    }
    __syncthreads();
    auto node = [&](int i) { return Node{lx[i], ly[i], lth[i], lk[i]}; };
    // origin of the s axis (ref :457-471)
    const int m0 = match_scan_wave(lx, ly, P, ox, oy, 50);
    const double s0 = projection_s_cs(node(m0), lcos[m0], lsin[m0], sm[m0], ox, oy);
    __syncthreads();
    for (int i = lane; i < P; i += 64) {
        const double v = sm[i] - s0;
        sm[i] = v;
        s_map[(size_t)b * max_ref + i] = v;
    }
    __syncthreads();
    // obstacles (ref test_9.py:122) and the planning start (ref test_9.py:134 and :172-177): matches one after the other (each
    // scan is wave-parallel, and none depends on another), then one point per lane for the projection arithmetic.  The start is
    // point k behind the k obstacles: it takes the free lane k & 63 of the last group, so that its trigonometry is the pass the
    // obstacles run anyway (as lane 0 of a pass of its own it cost the wavefront a second one).  Where k is a multiple of 64 no lane
    // is free and the start is a group by itself (k == 0: the only one).  An obstacle's l uses the FIRST obstacle's match
    // (quirk :413); the start uses its own match for s and l.
    // the start's outputs (one lane): ref test_9.py:134 and :172-177
    auto planning_start = [&](double bs, double l, const Node& proj, double pc, double psn) {
        if (begin_sl) {
            begin_sl[2 * b] = bs;
            begin_sl[2 * b + 1] = l;
        }
        const FrenetState fs = frenet_state_cs(proj, pc, psn, px, py, start_v[2 * b], start_v[2 * b + 1], start_a[2 * b], start_a[2 * b + 1]);
        start[4 * b + 0] = bs;
        start[4 * b + 1] = fs.l;
        start[4 * b + 2] = fs.dl_ds;
        start[4 * b + 3] = fs.ddl_ds;
        // ref test_9.py:137-169: the FIRST dynamic obstacle (distance Dis, speed V_obs) becomes three obstacles on
        // the centre line covering the stretch where it and the ego meet, unless they part beyond s = 80 m
        int total = k;
        if (dyn && !isnan(dyn[2 * b]) && k + 3 <= obs_cap) {
            const double Len_vehicle = 2.910, Len_obs = 3.0;
            const double Dis = dyn[2 * b], V_obs = dyn[2 * b + 1];
            const double vx = start_v[2 * b], vy = start_v[2 * b + 1];
            const double V_ego = sqrt(vx * vx + vy * vy);
            const double delta_v = V_ego - V_obs;
            const double meet_t = ((Dis - Len_vehicle / 2.0) - Len_obs / 2.0) / delta_v;
            const double delta_t = (Len_vehicle + Len_obs) / delta_v;
            const double leave_t = meet_t + delta_t;
            const double meet_s = ((bs + Dis) + V_obs * meet_t) - Len_obs / 2.0;
            const double leave_s = ((bs + Dis) + V_obs * leave_t) + Len_obs / 2.0;
            const double delta_s = leave_s - meet_s;
            const double obs_pos = meet_s + delta_s / 2.0;
            if (leave_s < 80.0) {
                double* os = obs_s + (size_t)b * obs_cap + k;
                double* ol = obs_l + (size_t)b * obs_cap + k;
                os[0] = meet_s - 10.0;
                os[1] = obs_pos;
                os[2] = leave_s;
                ol[0] = ol[1] = ol[2] = 0.0;
                total = k + 3;
            }
        }
        if (n_obs_out) n_obs_out[b] = total;
    };
    const int ms = match_scan_wave(lx, ly, P, px, py, 50);
    int my_match = 0, first_match = 0;
    for (int j = 0; j <= k; ++j) {
        if (j < k) {
            if (j >= 64 && (j & 63) == 0 && (j & ~63) + lane < k) {   // the next 64 obstacles (rows of more than 64 slots)
                obx = obs_xy[((size_t)b * max_obs + (j & ~63) + lane) * 2];
                oby = obs_xy[((size_t)b * max_obs + (j & ~63) + lane) * 2 + 1];
            }
            const double x = __shfl(obx, j & 63, 64), y = __shfl(oby, j & 63, 64);
            const int mj = match_scan_wave(lx, ly, P, x, y, 50);
            if (j == 0) first_match = mj;
            if ((j & 63) == lane) my_match = mj;
        }
        if ((j & 63) != 63 && j != k) continue;             // (uniform) flush a full set of lanes, or the last set with the start
        const int jj = (j & ~63) + lane;
        const bool is_start = jj == k;
        if (jj <= j) {
            const int m_s = is_start ? ms : my_match, m_l = is_start ? ms : first_match;
            const double x = is_start ? px : obx, y = is_start ? py : oby;
            const double bs = projection_s_cs(node(m_s), lcos[m_s], lsin[m_s], sm[m_s], x, y);
            const Node proj = project_on_cs(node(m_l), lcos[m_l], lsin[m_l], x, y);
            double pc, psn;
            sincos_pair(proj.theta, &psn, &pc);
            const double l = lateral_offset_cs(proj, pc, psn, x, y);
            if (!is_start) {
                obs_s[(size_t)b * obs_cap + jj] = bs;
                obs_l[(size_t)b * obs_cap + jj] = l;
            } else {
                planning_start(bs, l, proj, pc, psn);
            }
        }
    }
}

// ref: find_match_points (planning_utils.py:72-92 unwindowed, :123-167 windowed from pre_match_index `st`, which the caller
// has checked to lie in [0, P)) / match_projection_points (:383-402): the match index of one point
__device__ inline int find_match_one(const double* line, int P, double x, double y, bool windowed, int st) {
    if (!windowed) return match_scan(line, P, x, y, 0, 1, 50);
    const Node pm = node_at(line, st);
    const double flag = dot2(x - pm.x, y - pm.y, cos(pm.theta), sin(pm.theta));   // ref :139 np.dot
    return match_scan(line, P, x, y, st, flag > 0.0 ? 1 : -1, 5);
}

// ref: match_projection_points (mode 0) / find_match_points (mode 1), one lane per scene, points in order
__global__ void match_points_kernel(int B, int max_ref, int max_pts, const double* __restrict__ ref_line,
                                    const int* __restrict__ n_ref, const double* __restrict__ xy,
                                    const int* __restrict__ n_pts, const int* __restrict__ is_first_run,
                                    const int* __restrict__ pre_match_index, int* __restrict__ match_index,
                                    double* __restrict__ proj, int windowed_api) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* line = ref_line + (size_t)b * max_ref * 4;
    const int P = min(max(n_ref[b], 0), max_ref);       // clamped to the row's capacity
    const int k = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    int m_first = 0;
    // The windowed search starts at pre_match_index: the reference indexes the path with it (planning_utils.py:123)
    // and raises IndexError past the end; an index outside [0, P) - or an empty path - yields match_index = -1 for
    // every point of the scene (the drop-in turns that into IndexError) and touches no node.
    const bool windowed = windowed_api && !is_first_run[b];
    if (P < 1 || (windowed && (pre_match_index[b] < 0 || pre_match_index[b] >= P))) {
        for (int j = 0; j < k; ++j) {
            match_index[(size_t)b * max_pts + j] = -1;
            double* o = proj + ((size_t)b * max_pts + j) * 4;
            o[0] = o[1] = o[2] = o[3] = __builtin_nan("");
        }
        return;
    }
    for (int j = 0; j < k; ++j) {
        const double x = xy[((size_t)b * max_pts + j) * 2], y = xy[((size_t)b * max_pts + j) * 2 + 1];
        const int m = find_match_one(line, P, x, y, windowed, windowed ? pre_match_index[b] : 0);
        if (j == 0) m_first = m;
        match_index[(size_t)b * max_pts + j] = m;
        const Node pr = project_on(node_at(line, m_first), x, y);                  // quirk: first point's match (:103/:169/:413)
        double* o = proj + ((size_t)b * max_pts + j) * 4;
        o[0] = pr.x;
        o[1] = pr.y;
        o[2] = pr.theta;
        o[3] = pr.kappa;
    }
}

__global__ void heading_kappa_kernel(int B, int max_pts, const double* __restrict__ xy, const int* __restrict__ n_pts,
                                     double* __restrict__ theta, double* __restrict__ kappa) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int m = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    if (m < 2) return;
    heading_kappa(xy + (size_t)b * max_pts * 2, 2, m, theta + (size_t)b * max_pts, 1, kappa + (size_t)b * max_pts, 1);
}

// ---------------------------------------------------------------------------------------------
// ref: cal_lmin_lmax, path_planning.py:222-273.  returns false where the reference raises IndexError.
// ---------------------------------------------------------------------------------------------
// argmin_abs, argmin_abs3 and lmin_lmax: emp_frenet_core.h (shared with the CPU checks)
__global__ void lmin_lmax_kernel(int B, int max_pts, int max_obs, const double* __restrict__ dp_s,
                                 const double* __restrict__ dp_l, const int* __restrict__ n_pts,
                                 const double* __restrict__ obs_s, const double* __restrict__ obs_l,
                                 const int* __restrict__ n_obs, double obs_length, double obs_width,
                                 double* __restrict__ l_min, double* __restrict__ l_max, int* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    const bool ok = lmin_lmax(dp_s + (size_t)b * max_pts, dp_l + (size_t)b * max_pts, 1, n,
                              obs_s + (size_t)b * max_obs, obs_l + (size_t)b * max_obs, min(max(n_obs[b], 0), max_obs), obs_length,
                              obs_width, l_min + (size_t)b * max_pts, l_max + (size_t)b * max_pts);
    status[b] = ok ? 0 : kStBoundIndex;
}

// ---------------------------------------------------------------------------------------------
// heading / curvature of a scene's m points held in LDS (px, py), one point per lane of the scene's SL (ref planning_utils.py:185-228)
// th: LDS scratch [m].  out[i*ostride + 0..3] = x, y, theta, kappa.  Contains a barrier: whole wavefront calls (m = 0: no point).
// ---------------------------------------------------------------------------------------------
template <int SL>
__device__ __forceinline__ void heading_kappa_lanes(const double* px, const double* py, int m, double* th, double* out,
                                                    int ostride) {
    const int sl = threadIdx.x & (SL - 1);
    for (int i = sl; i < m; i += SL) {
        const double dx = centred_diff(px, 1, i, m), dy = centred_diff(py, 1, i, m);
        th[i] = atan2(dy, dx);
    }
    __syncthreads();
    for (int i = sl; i < m; i += SL) {
        const double dx = centred_diff(px, 1, i, m), dy = centred_diff(py, 1, i, m);
        double* o = out + (size_t)i * ostride;
        o[0] = px[i];
        o[1] = py[i];
        o[2] = th[i];
        o[3] = sin(centred_diff(th, 1, i, m)) / sqrt(dx * dx + dy * dy);
    }
}

// ---------------------------------------------------------------------------------------------
// ref: Quadratic_planning, path_planning.py:78-219 (stand-alone stage): one wavefront per scene
// dynamic LDS: PathQpLds (emp_tail_launch.h)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void path_qp_wave_kernel(int B, int max_pts, int cap, QpDev Q,
                                                          const double* __restrict__ l_min,
                                                          const double* __restrict__ l_max,
                                                          const int* __restrict__ n_pts,
                                                          const double* __restrict__ start_l3,
                                                          double* __restrict__ qp_l, double* __restrict__ qp_dl,
                                                          double* __restrict__ qp_ddl, int* __restrict__ iters,
                                                          int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x;
    const size_t o = (size_t)b * max_pts;
    const int n = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    int it = 0;
    int rc = 2;
    const bool fits = n <= cap;                         // (fewer than 4 stations: path_qp_setup_group refuses, EMP_ST_QP_FAILED)
    rc = path_qp_group<64>(path_qp_lds(lds, cap).qmem, l_min + o, l_max + o, n, start_l3[3 * b], start_l3[3 * b + 1], start_l3[3 * b + 2], Q.qp,
                           qp_l + o, qp_dl + o, qp_ddl + o, &it, fits);
    if ((threadIdx.x & 63) == 0) {
        if (iters) iters[b] = it;
        status[b] = rc ? kStQpFailed : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// ref: smooth_reference_line, planning_utils.py:262-361 (stand-alone stage): one wavefront per polyline,
// x on lanes 0-31, y on lanes 32-63, then heading / curvature one point per lane.
// dynamic LDS: SmoothLds of cap points (emp_tail_launch.h); the headings sit behind the solver arrays of the scene's own m points
// ---------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(64) void smooth_wave_kernel(int B, int max_pts, int cap, SmoothQpParams sx,
                                                         SmoothQpParams sy, const double* __restrict__ xy,
                                                         const int* __restrict__ n_pts, double* __restrict__ out,
                                                         int* __restrict__ iters, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x;
    const int m = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    int it = 0, rc = 2;
    double *px = nullptr, *py = nullptr;
    if (m <= cap) rc = smooth_pair_wave<WIDE>(smooth_lds(lds, m).qmem, xy + (size_t)b * max_pts * 2, 2, m, sx, sy, &px, &py, &it);
    if (rc == 0) heading_kappa_lanes<64>(px, py, m, smooth_lds(lds, m).theta, out + (size_t)b * max_pts * 4, 4);
    if ((threadIdx.x & 63) == 0) {
        if (iters) iters[b] = it;
        status[b] = rc ? kStSmoothFailed : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// Front end of one planning cycle (ref test_9.py:99-110): find_match_points for the predicted location on the
// GLOBAL path (planning_utils.py:49-182: windowed from the previous match unless is_first_run) -> sampling
// (:231-259: 10 nodes back, 40 forward, shifted at either end of the path, 51 nodes) -> smooth_reference_line
// (:262-361) -> the reference line of the cycle.  One wavefront per scene.
// dynamic LDS: RefLineLds (emp_tail_launch.h)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void reference_line_wave_kernel(int B, int max_global, SmoothQpParams sx, SmoothQpParams sy,
                                                                 const double* __restrict__ global_path,
                                                                 const int* __restrict__ n_global,
                                                                 const double* __restrict__ pred_xy,
                                                                 const int* __restrict__ is_first_run,
                                                                 const int* __restrict__ pre_match_index,
                                                                 double* __restrict__ ref_line, int* __restrict__ n_ref,
                                                                 int* __restrict__ match_index, int* __restrict__ iters,
                                                                 int* __restrict__ status, int n_ref_on_fail = 0) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const double* line = global_path + (size_t)b * max_global * 4;
    const int P = min(n_global[b], max_global);          // a count beyond the row's capacity is clamped, never followed
    const RefLineLds<double*> L = ref_line_lds(lds);
    double* gxy = L.gxy;                                 // [51][2]
    double* qmem = L.smooth.qmem;
    double* out = ref_line + (size_t)b * kRefLinePoints * 4;
    int m = 0, first = 0, fail = 0;
    if (lane == 0) {
        const double x = pred_xy[2 * b], y = pred_xy[2 * b + 1];
        const int st = pre_match_index[b];
        if (P < 1 || ((!is_first_run || !is_first_run[b]) && (st < 0 || st >= P))) {
            fail = kStSOutOfRange;                       // the reference raises IndexError
        } else {
            m = find_match_one(line, P, x, y, !(is_first_run && is_first_run[b]), st);
        }
        // sampling (ref :244-259): the arguments are overwritten with 10 back / 40 forward
        int back = 10, fwd = 40;
        if (m < back) {
            back = m;
            fwd = 50 - back;
        }
        if (P - m - 1 < fwd) {
            fwd = P - m - 1;
            back = 50 - fwd;
        }
        first = m - back;
        if (!fail && (first < 0 || m + fwd + 1 > P)) fail = kStSOutOfRange;   // path shorter than 51 nodes: the
                                                                              // reference's slice wraps around
    }
    m = __shfl(m, 0, 64);
    first = __shfl(first, 0, 64);
    fail = __shfl(fail, 0, 64);
    int it = 0;
    if (!fail) {
        if (lane < kRefLinePoints) {
            gxy[2 * lane] = line[4 * (first + lane)];
            gxy[2 * lane + 1] = line[4 * (first + lane) + 1];
        }
        __syncthreads();
        double *px = nullptr, *py = nullptr;
        const int rc = smooth_pair_wave<true>(qmem, gxy, 2, kRefLinePoints, sx, sy, &px, &py, &it);
        if (rc) fail = kStSmoothFailed;
        else heading_kappa_lanes<64>(px, py, kRefLinePoints, L.smooth.theta, out, 4);
    }
    if (fail)
        for (int i = lane; i < kRefLinePoints * 4; i += 64) out[i] = 0.0;
    if (lane == 0) {
        n_ref[b] = fail ? n_ref_on_fail : kRefLinePoints;       // (the fused cycle hands a failed line on as two zero nodes)
        match_index[b] = m;
        if (iters) iters[b] = it;
        status[b] = fail;
    }
}

// ---------------------------------------------------------------------------------------------
// ref: frenet_2_x_y_theta_kappa without its smoothing call, path_planning.py:29-46
// ---------------------------------------------------------------------------------------------
__device__ inline int frenet_path_to_xy(const double* line, const double* s_map, int P, double begin_s, double begin_l,
                                        const double* path_s, const double* path_l, int n, double* target_xy,
                                        int cap, bool* s_error, bool* trunc) {
    *s_error = false;
    *trunc = false;
    int idx = 0, m = 0;
    Node pr;
    if (!proj_point(line, s_map, P, begin_s, &idx, &pr)) {                        // ref :31
        *s_error = true;
        return 0;
    }
    double pc, psn;
    sincos_pair(pr.theta, &psn, &pc);
    normal_offset(pr.x, pr.y, begin_l, pc, psn, &target_xy[0], &target_xy[1]);    // ref :32-34
    m = 1;
    for (int i = 0; i < n; ++i) {
        const double s = path_s[i];
        if (s > s_map[P - 1]) break;                                               // ref :40-41
        if (!proj_point(line, s_map, P, s, &idx, &pr)) {                           // ref :42 (IndexError)
            *s_error = true;
            return m;
        }
        if (m >= cap) {
            *trunc = true;
            break;
        }
        sincos_pair(pr.theta, &psn, &pc);
        normal_offset(pr.x, pr.y, path_l[i], pc, psn, &target_xy[2 * m], &target_xy[2 * m + 1]);   // ref :44-46
        ++m;
    }
    return m;
}

__global__ void path_to_xy_kernel(int B, int max_ref, int max_pts, const double* __restrict__ ref_line,
                                  const double* __restrict__ s_map, const int* __restrict__ n_ref,
                                  const double* __restrict__ begin_sl, const double* __restrict__ path_s,
                                  const double* __restrict__ path_l, const int* __restrict__ n_pts,
                                  double* __restrict__ target_xy, int* __restrict__ n_out, int* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int P = min(max(n_ref[b], 0), max_ref);       // clamped to the row's capacity
    const int n = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    bool s_err, trunc;
    const int m = frenet_path_to_xy(ref_line + (size_t)b * max_ref * 4, s_map + (size_t)b * max_ref, P,
                                    begin_sl[2 * b], begin_sl[2 * b + 1], path_s + (size_t)b * max_pts,
                                    path_l + (size_t)b * max_pts, n, target_xy + (size_t)b * (max_pts + 1) * 2,
                                    max_pts + 1, &s_err, &trunc);
    n_out[b] = m;
    status[b] = (s_err ? kStSOutOfRange : 0) | (trunc ? kStTruncated : 0);
}

// ---------------------------------------------------------------------------------------------
// One cycle, middle part (ref test_9.py:187-210): decimate -> bounds -> path QP -> midpoints.
// One scene per GROUP of G lanes (G = 32: two scenes per wavefront when cap <= 34 stations, else G = 64).
// dynamic LDS, per group: CycleQpLds (emp_tail_launch.h)
// ---------------------------------------------------------------------------------------------
// R > 0: eight scenes per wavefront (G = 8), R stations per lane (emp_qp_rows.h; cap <= 8 R + 2 stations).
// doubles of LDS per group (scene)
template <int G, int R = 0>
__host__ __device__ constexpr int cycle_qp_group_words(int cap, int max_obs) {
    // Rows form: an ODD number of doubles.  The eight (four) groups of a wavefront read the same offsets of their own slices in
    // every LDS instruction; with a stride that is a multiple of 32 doubles they would all sit on the same banks (468 doubles at
    // R = 3: the station and Hessian arrays at 2-4 times their conflict-free cost, 14.5 % of the kernel's wavefront cycles in
    // SQ_LDS_BANK_CONFLICT, profiles/r06a_sq.csv) - an odd stride walks the groups across the banks.
    if (R > 0) return PathQpRowsLayout<(R > 0 ? G : 8), (R > 0 ? R : 3)>::stride(max_obs);
    return cycle_qp_lds(0, G == 32, cap, max_obs).end;
}
template <int G, int R = 0>
__device__ __forceinline__ void cycle_qp_body(int B, int max_pts, int max_obs, int cap, const QpDev& Q,
                                                           const double* __restrict__ dp_s,
                                                           const double* __restrict__ dp_l,
                                                           const int* __restrict__ dp_len,
                                                           const double* __restrict__ obs_s,
                                                           const double* __restrict__ obs_l,
                                                           const int* __restrict__ n_obs,
                                                           const double* __restrict__ start,
                                                           double* __restrict__ path_s, double* __restrict__ path_l,
                                                           int* __restrict__ path_len, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double lds_all[];
    __builtin_amdgcn_s_setprio(EMP_PRIO_BACK);     // wavefront priority of the back stage, see emp_context.h
    constexpr int GPW = 64 / G;                                   // groups (scenes) per wavefront
    const int lane = threadIdx.x & 63, grp = lane / G, gl = lane & (G - 1);
    const int b = blockIdx.x * GPW + grp;
    const bool present = b < B;
    static_assert(R == 0 || G == 8 || G == 16, "the rows solver runs on groups of 8 or 16 lanes");
    const int per_group = cycle_qp_group_words<G, R>(cap, max_obs);
    double* lds = lds_all + (size_t)grp * per_group;
    const size_t o = (size_t)(present ? b : 0) * max_pts;
    double* sd = lds;                 // decimated station s   [cap]  (rows form: see below)
    double *ld, *lmin, *lmax, *ql, *otab, *qmem;
    if constexpr (R > 0) {
        // Rows form (round 5): a path-QP wavefront's LDS - eight scenes - is what bounds how many edge-cost blocks of the NEXT
        // batch fit on its CU (measured: +1.2 us per staged step for every KB a QP wavefront holds, profiles/r05_edge/README.md 8).
        // The arrays that are dead once the QP is set up live inside solver arrays that are not written before its first
        // iteration (PathQpRowsLayout, emp_qp_core.h): sd, ld, lmin, lmax from tmp on (the station abscissae are re-read from
        // device memory for the midpoints at the end), the QP's result ql - written after the last iteration - in dua .. rhs, the
        // obstacle table in P.  Same values, same arithmetic; 5 cap + 4 max_obs doubles per scene less.  The solver's zero
        // padding is written behind the set-up, when these are dead (path_qp_group_rows).
        using L = PathQpRowsLayout<G, R>;
        qmem = lds;
        ql = qmem + L::result;
        sd = qmem + L::path;
        ld = sd + cap;
        lmin = ld + cap;
        lmax = lmin + cap;
        // the obstacle table is dead before the QP is set up: it lives where the Hessian band P will be written (4 C doubles),
        // or behind the group's other arrays when the obstacle rows are wider than that
        otab = qmem + (max_obs <= L::C ? L::obstacles : L::words);
    } else {
        const CycleQpLds<double*> L = cycle_qp_lds(lds, G == 32, cap, max_obs);
        ld = L.ld;                    // decimated DP l        [cap]
        lmin = L.lmin;                // [cap]
        lmax = L.lmax;                // [cap]
        ql = L.ql;                    // QP result l           [cap]
        otab = L.otab;                // per obstacle: lo, hi, below, bound   [4*max_obs]
        qmem = L.qmem;
    }
#ifdef EMP_QP_PROBE_EMPTY
    if (Q.debug_stage == 4) return;                 // development timing: the launch alone (tools/qp_phase_probe.py)
#endif
    const int ne = present ? dp_len[b] : 0;
    const int dec = Q.decimate > 0 ? Q.decimate : 1;
    const int n = (ne + dec - 1) / dec;                                            // len(x[::dec])
    const int st = present ? status[b] : 0;
    int fail = 0;                      // status bits this kernel adds; once set the group idles through the barriers
    if (present && (n > cap || n + (Q.midpoint ? 1 : 0) > max_pts || n < 1)) fail = kStTruncated;
    bool live = present && !fail;
    for (int i = gl; i < (live ? n : 0); i += G) {
        sd[i] = dp_s[o + (size_t)i * dec];
        ld[i] = dp_l[o + (size_t)i * dec];
    }
    __syncthreads();
#ifdef EMP_QP_PROBE_EMPTY
    if (Q.debug_stage == 5) return;                 // ... behind the loads of the DP path
#endif
    if (Q.use_qp) {
        // ---- cal_lmin_lmax (ref path_planning.py:222-273): one obstacle per lane finds its index range,
        // then one station per lane folds the (commutative) min / max over the obstacles covering it
        const int nob = live ? min(max(n_obs[b], 0), max_obs) : 0;
        bool bad = false;
        for (int k = gl; k < nob; k += G) {
            const double os = obs_s[(size_t)b * max_obs + k], ol = obs_l[(size_t)b * max_obs + k];
            int lo, hi, centre;                                                    // ref :240, :241, :257
            argmin_abs3(sd, n, os - Q.obs_length / 2.0, os + Q.obs_length / 2.0, os, &lo, &hi, &centre);
            lo += 2;
            hi += 2;
            const bool below = ld[centre] < ol;                                    // ref :263
            otab[4 * k + 0] = (double)lo;
            otab[4 * k + 1] = (double)hi;
            otab[4 * k + 2] = below ? 1.0 : 0.0;
            otab[4 * k + 3] = below ? ol - Q.obs_width / 2.0 : ol + Q.obs_width / 2.0;
            if (lo <= hi && hi >= n) bad = true;                                   // IndexError in the reference
        }
        if (group_any<G>(bad) && live) {
            fail = kStBoundIndex;
            live = false;
        }
        __syncthreads();
        {
            // obstacle by obstacle (its four table entries read ONCE, the same for every lane), each lane folding it into its own
            // stations gl, gl + G, ...: the same fmin / fmax in the same obstacle order per station as the station-outer loop this
            // replaces, with nob LDS round trips instead of (stations per lane) x nob
            constexpr int T = R > 0 ? R + 1 : (G == 64 ? 4 : 2);                  // stations a lane can own (cap <= G R + 2; 34 / 32; 255 / 64)
            const int nn = live ? n : 0;
            double a[T], c[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                a[t] = -10.0;                                                      // ref :233-234
                c[t] = 10.0;
            }
            for (int k = 0; k < nob; ++k) {
                const double klo = otab[4 * k], khi = otab[4 * k + 1], kbelow = otab[4 * k + 2], kb = otab[4 * k + 3];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const double j = (double)(gl + G * t);
                    if (j >= klo && j <= khi) {
                        if (kbelow != 0.0) c[t] = fmin(c[t], kb);
                        else a[t] = fmax(a[t], kb);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int j = gl + G * t;
                if (j < nn) {
                    lmin[j] = a[t];
                    lmax[j] = c[t];
                }
            }
            for (int j = gl + G * T; j < nn; j += G) {                            // (no launch gives a lane more stations than T: kept for safety)
                double aj = -10.0, cj = 10.0;
                for (int k = 0; k < nob; ++k) {
                    if ((double)j >= otab[4 * k] && (double)j <= otab[4 * k + 1]) {
                        if (otab[4 * k + 2] != 0.0) cj = fmin(cj, otab[4 * k + 3]);
                        else aj = fmax(aj, otab[4 * k + 3]);
                    }
                }
                lmin[j] = aj;
                lmax[j] = cj;
            }
        }
        __syncthreads();
        if (Q.debug_stage == 1) live = false;
        int it = 0;
        const int sb = present ? b : 0;
        int rc;
        if constexpr (R > 0)
            rc = path_qp_group_rows<G, R>(qmem, lmin, lmax, n, start[4 * sb + 1], start[4 * sb + 2], start[4 * sb + 3], Q.qp, ql, &it,
                                       live, Q.debug_stage);
        else
            rc = path_qp_group<G>(qmem, lmin, lmax, n, start[4 * sb + 1], start[4 * sb + 2], start[4 * sb + 3], Q.qp,
                                  ql, nullptr, nullptr, &it, live, Q.debug_stage);
        if (live && rc) {
            fail = kStQpFailed;
            live = false;
        }
    } else {
        for (int i = gl; i < (live ? n : 0); i += G) ql[i] = ld[i];
        __syncthreads();
    }
    if (present) {
        double* ps = path_s + o;
        double* pl = path_l + o;
        int plen = 0;
        // station abscissa i: from LDS, or - rows form, where the solver has overwritten it - from the DP path again (the same
        // number: sd[i] IS dp_s[i dec]).  The choice is made at COMPILE time (round 6): as a run-time select between a device and an
        // LDS address it compiled to one flat load behind a select of two pointers, and builds of this kernel that differed only
        // in where an unrelated value was loaded read that address wrong (an aperture violation, or midpoints of the wrong stations).
        auto sd_at = [&](int i) {
            if constexpr (R > 0) return dp_s[o + (size_t)i * dec];
            else return sd[i];
        };
        if (live) {
            if (Q.midpoint) {                                                      // ref test_9.py:204-210
                for (int i = gl; i <= n; i += G) {
                    if (i == 0) {
                        ps[0] = sd_at(0);
                        pl[0] = ql[0];
                    } else if (i == n) {
                        ps[n] = sd_at(n - 1);
                        pl[n] = ql[n - 1];
                    } else {
                        ps[i] = (sd_at(i) + sd_at(i - 1)) / 2.0;
                        pl[i] = (ql[i] + ql[i - 1]) / 2.0;
                    }
                }
                plen = n + 1;
            } else {
                for (int i = gl; i < n; i += G) {
                    ps[i] = sd_at(i);
                    pl[i] = ql[i];
                }
                plen = n;
            }
        }
        for (int i = plen + gl; i < max_pts; i += G) {                           // padding reads as 0
            ps[i] = 0.0;
            pl[i] = 0.0;
        }
        if (gl == 0) {
            path_len[b] = plen;
            status[b] = st | fail;
        }
    }
}

#define EMP_CYCLE_QP_PARAMS                                                                                         \
    int B, int max_pts, int max_obs, int cap, QpDev Q, const double *__restrict__ dp_s, const double *__restrict__ dp_l, \
        const int *__restrict__ dp_len, const double *__restrict__ obs_s, const double *__restrict__ obs_l,           \
        const int *__restrict__ n_obs, const double *__restrict__ start, double *__restrict__ path_s,                  \
        double *__restrict__ path_l, int *__restrict__ path_len, int *__restrict__ status
#define EMP_CYCLE_QP_ARGS B, max_pts, max_obs, cap, Q, dp_s, dp_l, dp_len, obs_s, obs_l, n_obs, start, path_s, path_l, path_len, status
template <int G>
__global__ __launch_bounds__(64) void cycle_qp_wave_kernel(EMP_CYCLE_QP_PARAMS) {
    cycle_qp_body<G>(EMP_CYCLE_QP_ARGS);
}
// 64 / GP scenes per wavefront on groups of GP lanes, R stations per lane (emp_qp_rows.h): a quarter (GP = 8) of the
// wavefronts of the two-per-wavefront kernel, each as long as before.
// (Round 5, measured and not kept: amdgpu_waves_per_eu(2, 2) - 256 registers and 224 bytes of scratch per lane instead of 256 + 74
// accumulation registers as spill space - so that two edge-cost wavefronts fit beside a path-QP wavefront on its SIMD instead of
// one: the kernel alone 137 -> 157 us, the staged step 0.241 -> 0.250 ms.)
template <int GP, int R>
__global__ __launch_bounds__(64) void cycle_qp_rows_kernel(EMP_CYCLE_QP_PARAMS) {
    cycle_qp_body<GP, R>(EMP_CYCLE_QP_ARGS);
}
#undef EMP_CYCLE_QP_PARAMS
#undef EMP_CYCLE_QP_ARGS

// walk_from_zero, the bisection form of cal_proj_point's index walk from 0: emp_frenet_core.h (shared with the CPU checks)

// ---------------------------------------------------------------------------------------------
// One cycle, last part (ref path_planning.py:15-49): Frenet->Cartesian one point per lane, x / y smoothing, heading / curvature
// one point per lane.  One scene per SL lanes, 64 / SL scenes per wavefront:
//   R == 0 (SL = 64): one scene per wavefront, smoothing on the two half-waves (smooth_pair_wave<WIDE>; WIDE == false, cap <= 32,
//     compiles the half-wave register path only, which fits four wavefronts per SIMD).  dynamic LDS: CartesianLds.
//   R > 0 (SL = 2 GP = 16 or 32): the x and the y smoothing problem on the scene's two GP-lane groups with R points per lane
//     (emp_smooth_rows.h; trajectories of at most GP R points: <8, 3> the benchmark's 23, <8, 4> up to 32, <16, 4> up to 64, BASELINE
//     configs[4]'s 63).  What the one-scene form spends per scene on 23 of 64 lanes (trigonometry) and on sweeps for two problems
//     (smoothing) is shared by four scenes here.  A problem whose active-set classification does not settle (none on any test or
//     benchmark scene) is solved by the whole wavefront with the half-wave solvers, one scene at a time.  dynamic LDS: a
//     CartesianSceneLds per scene, then the fall-back solver's storage (emp_tail_launch.h cartesian_rows_words).
// The reference walks the s_map index monotonically from the previous point (:42-43); that equals a running maximum of
// independent walks from index 0 (walk_from_zero, emp_frenet_core.h) under two preconditions: a non-decreasing s_map - what
// cal_s_map_fun produces; a NaN node leaves a NaN suffix, on which the walk's predicate is still true-then-false - and finite
// path stations - a NaN station exists only with a NaN planning start, which the bounds or the path QP have retired before this
// kernel.  The argument, the exhaustive CPU check of it and the tie cases are DESIGN.md section 5, "The station lookups".
// ---------------------------------------------------------------------------------------------
#define EMP_CARTESIAN_PARAMS                                                                                                       \
    int B, int max_ref, int max_pts, int cap, SmoothQpParams sx, SmoothQpParams sy, const double *__restrict__ ref_line,            \
        const double *__restrict__ s_map, const int *__restrict__ n_ref, const double *__restrict__ begin_sl,                       \
        const double *__restrict__ path_s, const double *__restrict__ path_l, const int *__restrict__ path_len,                     \
        double *__restrict__ traj, int *__restrict__ traj_len, int *__restrict__ status
#define EMP_CARTESIAN_ARGS B, max_ref, max_pts, cap, sx, sy, ref_line, s_map, n_ref, begin_sl, path_s, path_l, path_len, traj, traj_len, status
template <int SL, int R, bool WIDE>
__device__ __forceinline__ void cycle_cartesian_body(EMP_CARTESIAN_PARAMS, int force_fallback) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __builtin_amdgcn_s_setprio(EMP_PRIO_CART);          // as in the path QP kernel
    constexpr int GP = SL / 2, SPW = 64 / SL;     // lanes per smoothing problem, scenes per wavefront
    static_assert(R > 0 ? (SL == 16 || SL == 32) : SL == 64, "rows smoother: 16 or 32 lanes per scene; else the whole wavefront");
    const int lane = threadIdx.x & 63, sc = lane / SL, sl = lane & (SL - 1);
    const int b = blockIdx.x * SPW + sc;
    const bool present = b < B;
    const size_t bb = present ? (size_t)b : 0;
    const int per_scene = cartesian_scene_lds(0, max_ref, cap).end;
    double *sm, *txy, *th, *px, *py, *qmem;
    if constexpr (R > 0) {
        const CartesianSceneLds<double*> L = cartesian_scene_lds(lds + (size_t)sc * per_scene, max_ref, cap);
        sm = L.sm;                                   // [max_ref]
        txy = L.txy;                                 // [cap][2] interleaved x, y
        th = L.th;                                   // [cap]
        px = L.px;                                   // [cap] smoothed x
        py = L.py;                                   // [cap] smoothed y
        qmem = lds + (size_t)SPW * per_scene;        // the fall-back solver's storage (whole wavefront)
    } else {
        const CartesianLds<double*> L = cartesian_lds(lds, max_ref, cap);
        sm = L.sm;
        txy = L.txy;
        th = L.th;
        qmem = L.qmem;                               // the two smoothing problems; px, py: where the solver leaves its results
        px = py = nullptr;
    }
    const int st = present ? status[bb] : 0;
    int add = 0;                                 // status bits this kernel adds (scene-uniform)
    bool alive = present && !(st & (kStQpFailed | kStBoundIndex | kStTruncated));
    const double* line = ref_line + bb * max_ref * 4;
    const int P = present ? min(max(n_ref[bb], 0), max_ref) : 0;     // clamped to the row's capacity
    const int n = alive ? path_len[bb] : 0;
    for (int i = sl; i < P; i += SL) sm[i] = s_map[bb * max_ref + i];
    __syncthreads();
    // planning start (ref :31-34).  Checked for a scene the path QP has refused as well: the reference ignores its solver's
    // status (path_planning.py:211-218) and raises IndexError here all the same
    bool off = false;
    const double bs = present ? begin_sl[2 * bb] : 0.0, bl = alive ? begin_sl[2 * bb + 1] : 0.0;
    const int idx0 = walk_from_zero(sm, P, bs, &off);
    if (present && (off || P < 2)) {
        add = kStSOutOfRange;
        alive = false;
    }
    // trajectory points, one per lane in passes of SL: point q = 0 is the planning start (s = bs, l = bl, node idx0), point
    // q >= 1 is path point i = q - 1 (the start rides in the first pass: it used to cost a trigonometry pass of its own in front
    // of this loop).  count = leading path points with s <= s_map[-1] (ref :40-41), index = running max of walks (:42-43) from
    // idx0 on - the start's lane enters the maximum with 0, i.e. not at all.
    const double s_last = alive ? sm[P - 1] : 0.0;
    int carry = idx0, count = alive ? n : 0;
    bool stop = !alive;
    int qmax = 0;
#pragma unroll
    for (int g = 0; g < SPW; ++g) qmax = max(qmax, __builtin_amdgcn_readlane(alive ? n + 1 : 0, SL * g));
    constexpr unsigned long long kSceneMask = ~0ull >> (64 - SL);
    for (int base = 0; base < qmax; base += SL) {
        const int q = base + sl, i = q - 1;
        const bool is0 = alive && q == 0;
        const bool in = !stop && i >= 0 && i < n;
        const double s = in ? path_s[bb * max_pts + i] : 0.0;
        const unsigned long long bad = (__ballot(in && s > s_last) >> (SL * sc)) & kSceneMask;
        const int first_bad = SL == 64 ? __builtin_ffsll((long long)bad) : __builtin_ffs((int)bad);   // 1-based lane of the scene, 0 if none
        if (!stop && first_bad) count = min(count, base + first_bad - 2);              // (lane first_bad - 1 holds path point base + first_bad - 2)
        bool o2 = false;
        int k = in ? walk_from_zero(sm, P, fmin(s, s_last), &o2) : 0;
        for (int d = 1; d < SL; d <<= 1) {                 // inclusive running maximum across the scene's lanes
            const int v = __shfl_up(k, d, SL);
            if (sl >= d) k = max(k, v);
        }
        k = max(k, carry);
        carry = __shfl(k, SL - 1, SL);
        if (is0 || (in && i < count && i + 1 < cap)) {
            const Node mm = node_at(line, k);
            const double ds = (is0 ? bs : s) - sm[k], l = is0 ? bl : path_l[bb * max_pts + i];
            double mc, msn, pc, psn;
            sincos_pair(mm.theta, &msn, &mc);
            const Node pr = node_advanced(mm, ds, mc, msn);
            sincos_pair(pr.theta, &psn, &pc);
            normal_offset(pr.x, pr.y, l, pc, psn, &txy[2 * q], &txy[2 * q + 1]);     // ref :32-34 and :44-46
        }
        if (first_bad) stop = true;
    }
    int m = count + 1;
    __syncthreads();
    if (alive && (m > cap || m > max_pts + 1 || (R > 0 && m > GP * R))) {
        add = kStTruncated;
        alive = false;
    }
    if (alive && m < 2) {
        add = kStSmoothFailed;
        alive = false;
    }
    if constexpr (R > 0) {
        // smoothing (ref planning_utils.py:262-361): x on the scene's first GP lanes, y on the other GP, R points per lane
        const int grp = sl / GP, gl = sl & (GP - 1);
        double ref[R], u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = gl * R + r;
            const double v = txy[2 * (j < cap ? j : 0) + grp];
            ref[r] = (alive && j < m) ? v : 0.0;
        }
        int it = 0;
        int rc = box_qp_active_set_rows<GP, R>(ref, alive ? m : 0, grp ? sy : sx, u, &it);
        if (force_fallback && rc == 0) rc = -1;          // test hook (EMP_SMOOTH_FORCE_FALLBACK=1): every scene takes the fall-back
        const unsigned long long unsettled = __ballot(alive && rc < 0), wrong = __ballot(alive && rc > 0);
        const bool need_fb = ((unsettled >> (SL * sc)) & kSceneMask) != 0ull;
        if (((wrong >> (SL * sc)) & kSceneMask) != 0ull) {
            add = kStSmoothFailed;
            alive = false;
        }
        if (alive && !need_fb) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = gl * R + r;
                if (j < m) (grp ? py : px)[j] = u[r];
            }
        }
        __syncthreads();
        if (unsettled != 0ull) {             // wave-uniform; never taken on the test and benchmark scenes
            for (int s2 = 0; s2 < SPW; ++s2) {
                if (((unsettled >> (SL * s2)) & kSceneMask) == 0ull) continue;
                const int m2 = __builtin_amdgcn_readlane(m, SL * s2);
                const CartesianSceneLds<double*> L2 = cartesian_scene_lds(lds + (size_t)s2 * per_scene, max_ref, cap);
                double *qx = nullptr, *qy = nullptr;
                int it2 = 0;
                const int rc2 = smooth_pair_wave<WIDE>(qmem, L2.txy, 2, m2, sx, sy, &qx, &qy, &it2);
                if (rc2 == 0) {
                    for (int i = lane; i < m2; i += 64) {
                        L2.px[i] = qx[i];
                        L2.py[i] = qy[i];
                    }
                } else if (sc == s2) {
                    add = kStSmoothFailed;
                    alive = false;
                }
                __syncthreads();
            }
        }
    } else {
        // smoothing on the two half-waves (alive is wave-uniform: the scene is the wavefront)
        int it = 0;
        if (alive && smooth_pair_wave<WIDE>(qmem, txy, 2, m, sx, sy, &px, &py, &it)) {
            add = kStSmoothFailed;
            alive = false;
        }
    }
    double* out_rows = traj + bb * (max_pts + 1) * 4;
    const int mm = alive ? m : 0;
    heading_kappa_lanes<SL>(px, py, mm, th, out_rows, 4);
    if (present) {
        for (int i = mm * 4 + sl; i < (max_pts + 1) * 4; i += SL) out_rows[i] = 0.0;       // padding reads as 0
        if (sl == 0) {
            traj_len[bb] = mm;
            if (add) status[bb] = st | add;
        }
    }
}

__global__ __launch_bounds__(64) void cycle_cartesian_wave_kernel_wide(EMP_CARTESIAN_PARAMS) {
    cycle_cartesian_body<64, 0, true>(EMP_CARTESIAN_ARGS, 0);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void cycle_cartesian_wave_kernel_narrow(EMP_CARTESIAN_PARAMS) {
    cycle_cartesian_body<64, 0, false>(EMP_CARTESIAN_ARGS, 0);
}
template <int GP, int R>
__global__ __launch_bounds__(64) void cycle_cartesian_rows_kernel(EMP_CARTESIAN_PARAMS, int force_fallback) {
    cycle_cartesian_body<2 * GP, R, (GP * R > kHalfWave)>(EMP_CARTESIAN_ARGS, force_fallback);
}
#undef EMP_CARTESIAN_PARAMS
#undef EMP_CARTESIAN_ARGS

// ---------------------------------------------------------------------------------------------
// stand-alone forms of the projection helpers (one lane per scene, points in order)
// ---------------------------------------------------------------------------------------------
// ref: cal_s_map_fun, planning_utils.py:448-472
__global__ void s_map_kernel(int B, int max_ref, const double* __restrict__ ref_line, const int* __restrict__ n_ref,
                             const double* __restrict__ origin_xy, double* __restrict__ s_map) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int P = min(max(n_ref[b], 0), max_ref);       // a count beyond the row's capacity is clamped, never followed
    if (P < 1) return;                                  // an empty line has no s_map (the reference raises IndexError)
    s_map_build(ref_line + (size_t)b * max_ref * 4, P, origin_xy[2 * b], origin_xy[2 * b + 1], s_map + (size_t)b * max_ref);
}

// ref: cal_s_l_fun, planning_utils.py:496-507, for one point matched at `m`, its l on the FIRST point's match `m_first` (quirk :413);
// an index outside [0, P) gives NaN.  l may be null.
__device__ inline void s_l_point(const double* line, const double* sm, int P, int m, int m_first, double x, double y, double* s,
                                 double* l) {
    const double qnan = __builtin_nan("");
    const bool ok = m >= 0 && m < P, ok_first = m_first >= 0 && m_first < P;
    *s = ok ? projection_s(node_at(line, m), sm[m], x, y) : qnan;
    if (l) *l = (ok && ok_first) ? lateral_offset(project_on(node_at(line, m_first), x, y), x, y) : qnan;
}

// ref: cal_s_l_fun, planning_utils.py:475-509 (mode 0) and cal_projection_s_fun, :429-445 (mode 1: the caller
// supplies the match indices and only s is produced).  A match index outside [0, P) is not followed: that point's s and
// l are NaN (l also where the scene's first index is out of range: every l projects on the first point's match); an
// empty line (P = 0, where the reference raises IndexError) gives NaN for every point.
__global__ void s_l_kernel(int B, int max_ref, int max_pts, const double* __restrict__ ref_line,
                           const double* __restrict__ s_map, const int* __restrict__ n_ref,
                           const double* __restrict__ xy, const int* __restrict__ n_pts,
                           const int* __restrict__ match_in, double* __restrict__ out_s, double* __restrict__ out_l) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* line = ref_line + (size_t)b * max_ref * 4;
    const double* sm = s_map + (size_t)b * max_ref;
    const int P = min(max(n_ref[b], 0), max_ref);       // clamped to the row's capacity
    const int k = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    int m_first = 0;
    for (int j = 0; j < k; ++j) {
        const size_t o = (size_t)b * max_pts + j;
        const double x = xy[o * 2], y = xy[o * 2 + 1];
        const int m = match_in ? match_in[o] : match_scan(line, P, x, y, 0, 1, 50);
        if (j == 0) m_first = m;
        double s, l;
        s_l_point(line, sm, P, m, m_first, x, y, &s, out_l ? &l : nullptr);
        out_s[o] = s;
        if (out_l) out_l[o] = l;
    }
}

// ref: cal_s_l_deri_fun, planning_utils.py:512-588: out [B][max_pts][7] = l, dl/dt, ds/dt, d2l/dt2, dl/ds, d2s/dt2, d2l/ds2
__global__ void s_l_deri_kernel(int B, int max_ref, int max_pts, const double* __restrict__ ref_line,
                                const int* __restrict__ n_ref, const double* __restrict__ xy,
                                const double* __restrict__ vxy, const double* __restrict__ axy,
                                const int* __restrict__ n_pts, const double* __restrict__ origin_xy,
                                double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* line = ref_line + (size_t)b * max_ref * 4;
    const int P = min(max(n_ref[b], 0), max_ref);       // clamped to the row's capacity
    const int k = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    int m_first = 0;
    for (int j = 0; j < k; ++j) {
        const size_t o = (size_t)b * max_pts + j;
        double* r = out + o * 7;
        if (P < 1) {                                    // empty line: the reference raises IndexError; no node is read
            r[0] = r[1] = r[2] = r[3] = r[4] = r[5] = r[6] = __builtin_nan("");
            continue;
        }
        const double x = xy[o * 2], y = xy[o * 2 + 1];
        const int m = match_scan(line, P, x, y, 0, 1, 50);
        if (j == 0) m_first = m;
        const Node proj = project_on(node_at(line, m_first), x, y);
        const FrenetState f = frenet_state(proj, origin_xy[2 * b], origin_xy[2 * b + 1], vxy[o * 2], vxy[o * 2 + 1],
                                           axy[o * 2], axy[o * 2 + 1]);
        r[0] = f.l; r[1] = f.l_dot; r[2] = f.s_dot; r[3] = f.l_ddot; r[4] = f.dl_ds; r[5] = f.s_ddot; r[6] = f.ddl_ds;
    }
}

// ref: cal_proj_point, path_planning.py:52-75: one query per lane; out [n][4], idx_out [n]; status 2 = IndexError
__global__ void proj_point_kernel(int n, int max_ref, const double* __restrict__ ref_line,
                                  const double* __restrict__ s_map, const int* __restrict__ n_ref,
                                  const double* __restrict__ s, const int* __restrict__ pre_idx,
                                  double* __restrict__ out, int* __restrict__ idx_out, int* __restrict__ status) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int P = min(max(n_ref[t], 0), max_ref);       // a count beyond the row's capacity is clamped, never followed
    int idx = pre_idx[t];
    Node pr{0, 0, 0, 0};
    const bool ok = idx >= 0 && proj_point(ref_line + (size_t)t * max_ref * 4, s_map + (size_t)t * max_ref, P, s[t], &idx, &pr);
    out[4 * t] = pr.x; out[4 * t + 1] = pr.y; out[4 * t + 2] = pr.theta; out[4 * t + 3] = pr.kappa;
    idx_out[t] = idx;
    status[t] = ok ? 0 : kStSOutOfRange;
}

// ref: trajectory_index2s, planning_utils.py:776: one chord (the caller sums them left to right)
__device__ inline double chord_length(double x0, double y0, double x1, double y1) {
    const double dx = x1 - x0, dy = y1 - y0;
    return sqrt(dx * dx + dy * dy);
}

// ref: trajectory_index2s, planning_utils.py:758-780: cumulative chord length until the first NaN x
__global__ void index2s_kernel(int B, int max_pts, const double* __restrict__ x, const double* __restrict__ y,
                               const int* __restrict__ n_pts, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const size_t o = (size_t)b * max_pts;
    const int n = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    double acc = 0.0;
    for (int i = 0; i < n; ++i) out[o + i] = 0.0;
    for (int i = 1; i < n; ++i) {
        if (x[o + i] != x[o + i]) break;
        acc += chord_length(x[o + i - 1], y[o + i - 1], x[o + i], y[o + i]);
        out[o + i] = acc;
    }
}

// ref: CalcProjPoint (planning_utils.py:736-755) + Frenet2Cartesian (:706-733): per point, NaN s stops the scene.
// line [B][max_ref][4], index2s [B][max_ref]; sl [B][max_pts][4] = s, l, dl, ddl -> out [B][max_pts][4] (NaN-filled)
__global__ void frenet2cartesian_kernel(int B, int max_ref, int max_pts, const double* __restrict__ ref_line,
                                        const double* __restrict__ index2s, const int* __restrict__ n_ref,
                                        const double* __restrict__ sl, const int* __restrict__ n_pts,
                                        double* __restrict__ out, int* __restrict__ status, int proj_only) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* line = ref_line + (size_t)b * max_ref * 4;
    const double* sm = index2s + (size_t)b * max_ref;
    const int P = min(max(n_ref[b], 0), max_ref);       // clamped to the row's capacity
    const int k = min(max(n_pts[b], 0), max_pts);       // a count beyond the row's capacity is clamped, never followed
    const double qnan = __builtin_nan("");
    int st = 0;
    bool stopped = false;
    for (int j = 0; j < k; ++j) {
        const double* v = sl + ((size_t)b * max_pts + j) * 4;
        double* o = out + ((size_t)b * max_pts + j) * 4;
        o[0] = o[1] = o[2] = o[3] = qnan;
        if (stopped || v[0] != v[0]) {                      // ref :718-719 break at the first NaN s
            stopped = true;
            continue;
        }
        int idx = 1;                                         // ref :742-744 starts at 1, first s_map[idx] >= s
        while (idx < P && sm[idx] < v[0]) ++idx;
        if (idx >= P) {
            st = kStSOutOfRange;                             // IndexError in the reference
            stopped = true;
            continue;
        }
        const Node m = node_at(line, idx);
        const double ds = v[0] - sm[idx];
        double mc, msn;
        sincos_pair(m.theta, &msn, &mc);
        const Node pr = node_advanced(m, ds, mc, msn);
        const double ph = pr.theta, pk = pr.kappa;
        if (proj_only) {
            o[0] = pr.x; o[1] = pr.y; o[2] = ph; o[3] = pk;
            continue;
        }
        const double l = v[1], dl = v[2], ddl = v[3];
        double pc, psn;
        sincos_pair(ph, &psn, &pc);
        normal_offset(pr.x, pr.y, l, pc, psn, &o[0], &o[1]);
        const double hd = ph + atan(dl / (1.0 - pk * l));                                   // ref :727
        const double dth = hd - ph;
        o[2] = hd;
        o[3] = ((ddl + pk * dl * tan(dth)) * (cos(dth) * cos(dth)) / (1.0 - pk * l) + pk) * cos(dth) / (1.0 - pk * l);
    }
    status[b] = st;
}

// ref: cal_dy_obs_deri, planning_utils.py:795-806 for one obstacle: l, velocity, projected heading and kappa -> s_dot, l_dot, dl/ds
__device__ inline void dy_obs_deri_one(double l, double vx, double vy, double hd, double k, double* s_dot_out, double* l_dot_out,
                                       double* dl_out) {
    const double l_dot = dot2(vx, vy, -sin(hd), cos(hd));                 // np.dot, :799-800
    const double s_dot = dot2(vx, vy, cos(hd), sin(hd)) / (1.0 - k * l);
    *s_dot_out = s_dot;
    *l_dot_out = l_dot;
    *dl_out = (fabs(s_dot) < 1e-6) ? 0.0 : l_dot / s_dot;
}

// ref: cal_dy_obs_deri, planning_utils.py:783-808: in [n][5] = l, vx, vy, heading, kappa -> out [n][3] = s_dot, l_dot, dl
__global__ void dy_obs_deri_kernel(int n, const double* __restrict__ in, double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    dy_obs_deri_one(in[5 * t], in[5 * t + 1], in[5 * t + 2], in[5 * t + 3], in[5 * t + 4], &out[3 * t], &out[3 * t + 1], &out[3 * t + 2]);
}

// small utilities ---------------------------------------------------------------------------------
// ref: cal_quintic_coefficient, planning_utils.py:671-703 - returns ABSOLUTE-s coefficients c0..c5 like the
// reference, computed from the closed form in the shifted coordinate (binomial re-expansion about s0).
__global__ void quintic_kernel(int n, const double* __restrict__ bc, double* __restrict__ coeff) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double* v = bc + 8 * t;
    const double l0 = v[0], dl0 = v[1], ddl0 = v[2], l1 = v[3], dl1 = v[4], ddl1 = v[5], s0 = v[6], T = v[7] - v[6];
    const double h = l1 - l0, T2 = T * T, T3 = T2 * T, T4 = T3 * T, T5 = T4 * T;
    double a[6];
    a[0] = l0;
    a[1] = dl0;
    a[2] = 0.5 * ddl0;
    a[3] = (20.0 * h - (8.0 * dl1 + 12.0 * dl0) * T - (3.0 * ddl0 - ddl1) * T2) / (2.0 * T3);
    a[4] = (-30.0 * h + (14.0 * dl1 + 16.0 * dl0) * T + (3.0 * ddl0 - 2.0 * ddl1) * T2) / (2.0 * T4);
    a[5] = (12.0 * h - 6.0 * (dl1 + dl0) * T - (ddl0 - ddl1) * T2) / (2.0 * T5);
    // p(s) = sum a_k (s - s0)^k  ->  sum c_j s^j  by repeated synthetic "shift" (Horner form in (s - s0))
    double c[6] = {a[5], 0, 0, 0, 0, 0};
    int deg = 0;
    for (int k = 4; k >= 0; --k) {               // c(s) <- c(s) * (s - s0) + a_k
        ++deg;
        for (int j = deg; j >= 1; --j) c[j] = c[j - 1] - s0 * c[j];
        c[0] = a[k] - s0 * c[0];                 // (descending j reads the not-yet-updated c[j-1])
    }
    for (int j = 0; j < 6; ++j) coeff[6 * t + j] = c[j];
}

// ref: cal_obs_cost, path_planning.py:588-609
__global__ void obs_cost_kernel(int n, int samples, double w, double danger, double safe, const double* __restrict__ sq,
                                double* __restrict__ cost) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double d2a = danger * danger, d2b = safe * safe;
    double c = 0.0;
    for (int i = 0; i < samples; ++i) {               // the reference loops over whatever it is handed (:601)
        const double v = sq[(size_t)samples * t + i];
        if (v <= d2a) {
            c = c + w;
            break;
        } else if (d2a < v && v < d2b) {
            c = c + kSoftGain / v;
        }
    }
    cost[t] = c;
}

// ref: cal_start_cost (path_planning.py:435-514) / cal_neighbor_cost (:517-585) for FREE edges: edges [n][8] = start s, l, dl, ddl,
// span (end s - start s), end l, sample_s, (unused).  The quintic ends at `end s` (the reference's cal_quintic_coefficient call, :475 / :553) while
// the ten samples step by sample_s / 10 from the start (:492-493 / :565-566) - the two coincide on the lattice and need not
// for a caller of the drop-in functions.  Obstacles per edge: obs_s, obs_l [n][max_obs], n_obs [n].
__global__ void free_edge_cost_kernel(int n, int max_obs, const double* __restrict__ edges, const double* __restrict__ obs_s,
                                      const double* __restrict__ obs_l, const int* __restrict__ n_obs, double w_coll, double w0,
                                      double w1, double w2, double w_ref, double* __restrict__ cost) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double* e = edges + (size_t)t * 8;
    const Quintic q = quintic_shifted(e[1], e[2], e[3], e[5], e[4]);
    const int k = max_obs > 0 ? min(max(n_obs[t], 0), max_obs) : 0;
    cost[t] = segment_cost(q, e[0], e[6], obs_s + (size_t)t * max_obs, obs_l + (size_t)t * max_obs, k, w_coll, w0, w1, w2, w_ref);
}

}  // namespace emp
