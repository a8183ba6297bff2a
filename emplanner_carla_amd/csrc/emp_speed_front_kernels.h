// emp_speed_front_kernels.h - the front of emp_plan_trajectory's speed half (reference test_10.py:233-292): the glue between a
// planned path and the S-T speed planner, one wavefront per scene.  The arithmetic is the stand-alone kernels' own device
// functions (index2s_kernel, match_points_kernel, s_l_kernel, dy_obs_deri_kernel, st_start_condition_kernel, st_graph_kernel),
// so every value equals the chain of those entry points bit for bit.
//
//   speed_front_wave_kernel  lanes over the trajectory points: the W-wide rows and the chords of trajectory_index2s (summed
//                            left to right by one lane, index2s_kernel's order); lanes over the dynamic obstacles (<= 64):
//                            find_match_points, cal_s_l_fun, cal_dy_obs_deri, generate_st_graph
//   speed_status_kernel      speed_status = the OR of the back-end stages' EMP_STB_* bits, or the front's IndexError alone
#pragma once

#include <hip/hip_runtime.h>

#include "emp_st_backend_core.h"
#include "emp_st_kernels.h"
#include "emp_tail_kernels.h"

namespace emp {

// dynamic LDS: SpeedFrontLds (emp_tail_launch.h).  traj [B][max_pts + 1][4] and traj_len [B] are emp_plan_cycle's outputs; W = max_pts + 2.
// Outputs: rows [4][B][W] = x, y, heading, kappa (NaN from traj_len on), index2s [B][W], s_dot0 / s_dot20 [B] (the speed
// planner's start condition), seg [4][B][max_dyn] = s_in, s_out, t_in, t_out, merge_width [B] (W, or 0 for a scene whose
// obstacle match leaves the trajectory: path_speed_merge then NaN-fills it), front_status [B] (EMP_STB_INDEX or 0).
__global__ __launch_bounds__(64) void speed_front_wave_kernel(
    int B, int max_pts, int W, int max_dyn, const double* __restrict__ traj, const int* __restrict__ traj_len,
    const double* __restrict__ start_v, const double* __restrict__ start_a, const double* __restrict__ heading,
    const double* __restrict__ dyn_obs, const int* __restrict__ n_dyn, const int* __restrict__ dyn_pre_match,
    double* __restrict__ rows, double* __restrict__ index2s, double* __restrict__ s_dot0, double* __restrict__ s_dot20,
    double* __restrict__ seg, int* __restrict__ merge_width, int* __restrict__ front_status) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const SpeedFrontLds<double*> L = speed_front_lds(lds, W);
    double* chord = L.chord;         // [W] chord i = |point i - point i-1|
    double* i2s = L.i2s;             // [W] trajectory_index2s of the scene
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int cap = max_pts + 1;
    const double* line = traj + (size_t)b * cap * 4;
    const int P = min(max(traj_len[b], 0), cap);          // a count beyond the row's capacity is clamped, never followed
    const double qnan = __builtin_nan("");
    const size_t plane = (size_t)B * W, ro = (size_t)b * W;

    // 1. the rows handed to the reference's MATLAB-style functions: x, y, heading, kappa, NaN behind the valid points
    int first_nan = W;               // index2s_kernel's loop (i >= 1) stops at the first NaN x
    for (int base = 0; base < W; base += 64) {
        const int i = base + lane;
        double x = qnan, y = qnan, h = qnan, k = qnan;
        if (i < P) {
            x = line[4 * i];
            y = line[4 * i + 1];
            h = line[4 * i + 2];
            k = line[4 * i + 3];
        }
        if (i < W) {
            rows[ro + i] = x;
            rows[plane + ro + i] = y;
            rows[2 * plane + ro + i] = h;
            rows[3 * plane + ro + i] = k;
            chord[i] = (i >= 1 && i < P) ? chord_length(line[4 * (i - 1)], line[4 * (i - 1) + 1], x, y) : 0.0;
        }
        const unsigned long long m = __ballot(i >= 1 && i < W && x != x);
        if (m && first_nan == W) first_nan = base + __builtin_ffsll((long long)m) - 1;
    }
    __syncthreads();
    // 2. trajectory_index2s: the chords summed left to right (a prefix scan would reassociate the sum), 0 from the first NaN on
    if (lane == 0) {
        double acc = 0.0;
        i2s[0] = 0.0;
        for (int i = 1; i < W; ++i) {
            if (i < first_nan) acc += chord[i];
            i2s[i] = i < first_nan ? acc : 0.0;
        }
        // 3. calc_speed_planning_start_condition
        speed_start_condition(start_v[2 * b], start_v[2 * b + 1], start_a[2 * b], start_a[2 * b + 1], heading[b], &s_dot0[b],
                              &s_dot20[b]);
    }
    __syncthreads();
    for (int i = lane; i < W; i += 64) index2s[ro + i] = i2s[i];

    // 4.-7. the dynamic obstacles, one per lane.  find_match_points (is_first_run = False) indexes the trajectory with
    // pre_match_index first: outside [0, traj_len) the reference raises IndexError (planning_utils.py:132) - no obstacle then
    // no loop, no error
    const int k = min(max(n_dyn[b], 0), max_dyn);
    const int pre = dyn_pre_match ? dyn_pre_match[b] : 0;
    const bool index_error = k > 0 && (P < 1 || pre < 0 || pre >= P);
    const bool mine = lane < k && !index_error;
    double ox = 0.0, oy = 0.0, ovx = 0.0, ovy = 0.0;
    if (mine) {
        const double* o = dyn_obs + ((size_t)b * max_dyn + lane) * 4;
        ox = o[0];
        oy = o[1];
        ovx = o[2];
        ovy = o[3];
    }
    int m_match = 0, m_sl = 0;
    if (mine) {
        m_match = find_match_one(line, P, ox, oy, true, pre);          // find_match_points' own match
        m_sl = match_scan(line, P, ox, oy, 0, 1, 50);                  // cal_s_l_fun matches again, from the start
    }
    const int first_match = __shfl(m_match, 0, 64), first_sl = __shfl(m_sl, 0, 64);
    double os = qnan, ol = qnan, osd = qnan, old = qnan;
    if (mine) {
        // every projected node is taken at the FIRST obstacle's match (planning_utils.py:169)
        const Node pr = project_on(node_at(line, first_match), ox, oy);
        s_l_point(line, i2s, P, m_sl, first_sl, ox, oy, &os, &ol);     // s_map = the trajectory's index2s
        double dl;
        dy_obs_deri_one(ol, ovx, ovy, pr.theta, pr.kappa, &osd, &old, &dl);
    }
    // cal_dy_obs_deri stops at the first NaN l (planning_utils.py:794-795): NaN from there on
    const unsigned long long lnan = __ballot(lane < k && !(ol == ol));
    if (lnan && lane >= __builtin_ffsll((long long)lnan) - 1) osd = old = qnan;
    // generate_st_graph: slots at or beyond n_dyn are NaN in all four inputs; the scan stops at the first NaN s
    const unsigned long long snan = __ballot(lane < max_dyn && !(os == os));
    const int first_empty = snan ? __builtin_ffsll((long long)snan) - 1 : 64;
    double si = qnan, so = qnan, ti = qnan, to = qnan;
    if (lane < first_empty) st::st_graph_slot(os, ol, osd, old, &si, &so, &ti, &to);
    if (lane < max_dyn) {
        const size_t sp = (size_t)B * max_dyn, so_ = (size_t)b * max_dyn + lane;
        seg[so_] = si;
        seg[sp + so_] = so;
        seg[2 * sp + so_] = ti;
        seg[3 * sp + so_] = to;
    }
    if (lane == 0) {
        merge_width[b] = index_error ? 0 : W;
        front_status[b] = index_error ? stb::kStbIndex : 0;
    }
}

// speed_status: a scene whose obstacle match raised keeps EMP_STB_INDEX alone (the reference never reaches the later stages);
// every other scene gets the OR of convex space, speed QP, densification and merge
__global__ void speed_status_kernel(int B, const int* __restrict__ front, const int* __restrict__ convex, const int* __restrict__ qp,
                                    const int* __restrict__ dense, const int* __restrict__ merge, int* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    status[b] = front[b] ? front[b] : (convex[b] | qp[b] | dense[b] | merge[b]);
}

}  // namespace emp
