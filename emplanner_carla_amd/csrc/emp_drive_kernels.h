// emp_drive_kernels.h - what the reference's DRIVER does between two planning requests (test_9.py:336-436), on the device:
//   drive_request_kernel  get_actor_from_world (test_9.py:48-89), predict_block (planning_utils.py:591-614), the planner's gate on
//                         the nearest static obstacle (test_9.py:116) and the first dynamic obstacle's (dis, speed): fleet state
//                         and a list of actors in, the inputs of emp_plan_cycle out
//   drive_adopt_kernel    adopt a valid plan as the track the controller follows, or hold the previous one and count
//   drive_accel_kernel    the world-frame acceleration over the period's last tick, the next request's start_a
// emp_drive (emp_api.hip) strings them together with the cycle and the rollout kernel, K periods without a host round trip.
// emp_drive_timed is the same loop with the speed planner in it: the request and the adopt kernel take a policy, as
// mpc_rollout_kernel<TG> does - NoClock / NoSpeed are emp_drive's kernels, statement for statement; Clock adds the speed planner's
// inputs to the request, Speed the profile (the period's timed trajectory), its cursor and its counter to the adoption.
//
// Arithmetic contract as in emp_control_core.h: written order, separately rounded binary64 operations (-ffp-contract=off), IEEE
// `/` and sqrt; libm enters through sin, cos and atan2 only.  include/emplanner.h states the formulas in order; tests/drive_port.py
// is the same in Python floats.
#pragma once

#include "emp_control_core.h"

namespace emp {
namespace drive {

struct Params {
    double dis_limitation, lateral_band, behind, dynamic_speed, static_gate, pred_ts, advance_s;
};

// world-frame velocity of a vehicle from its body-frame components: c = cos fi, s = sin fi
struct World {
    double wx, wy;
};
EMP_HD World world_velocity(double c, double s, double Vy, double Vx) { return World{Vx * c - Vy * s, Vx * s + Vy * c}; }

struct RequestIO {
    const double* state;        // [B][6] x, y, fi, Vy, fi_dot, Vx
    const double* accel;        // [B][2] or null (zeros)
    const double* actors;       // [B][max_act][4] x, y, vx, vy
    const int* n_act;           // [B]
    double* static_xy;          // [B][max_obs][2]
    int* n_static;              // [B]
    double* static_dis;         // [B][max_obs]
    double* dyn;                // [B][max_dyn][4] x, y, dis, speed
    int* n_dyn;                 // [B]
    double* dyn_dis_speed;      // [B][2]
    int* n_obs;                 // [B]
    double* origin_xy;          // [B][2]
    double* start_xy;           // [B][2]
    double* pred_fi;            // [B]
    double* start_v;            // [B][2]
    double* start_a;            // [B][2]
    int* req_status;            // [B]
    double* actors_next;        // [B][max_act][4] or null; may be `actors`
    double* log_state;          // [B][6] or null: emp_drive's row of this period
    int* log_counts;            // [B][2] or null: n_obs, n_dyn
};

// What emp_drive_request_timed and emp_drive_timed add to the request: the speed planner's inputs (emp_speed_io), which only this
// kernel can give - it holds each dynamic actor's (x, y, vx, vy) and its rank in registers, and the actors advance in place.
struct NoClock {
    static constexpr bool kTimed = false;
};
struct Clock {
    static constexpr bool kTimed = true;
    const double* t0;           // [B] the vehicle's clock at tick 0
    int tick;                   // the period's first tick
    double dt, plan_lead;
    double* dyn_obs;            // [B][max_dyn][4] x, y, vx, vy of the kept dynamics in dyn's order, before the advance; idle slots 0
    double* start_heading;      // [B] atan2(wy, wx): the value beta is made of
    double* plan_start_time;    // [B] (t0 + (double)tick * dt) + plan_lead
};

// One wavefront per vehicle, one actor per lane (max_act <= 64); grid and block from plan_drive_request (emp_dp_launch.h).
// Each class (static, dynamic) is ordered by (dis, actor index): a lane's rank is the number of same-class lanes that come
// before it, counted in a wave-uniform loop over the set bits of the class masks - no atomics, no per-lane branches.  A lane
// reads its actor before it writes it, so actors_next may be actors.
template <typename TM>
__global__ __launch_bounds__(256) void drive_request_kernel(int B, int max_act, int max_obs, int max_dyn, Params prm, RequestIO io, TM tm) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (b >= B) return;                                            // (the whole wavefront)
    const double* st = io.state + 6 * (size_t)b;
    const double x = st[0], y = st[1], fi = st[2], Vy = st[3], fi_dot = st[4], Vx = st[5];
    const double c = cos(fi), s = sin(fi);
    const World w = world_velocity(c, s, Vy, Vx);
    const int n = min(max(io.n_act[b], 0), max_act);
    const bool has = lane < n;
    const size_t slot = (size_t)b * max_act + lane;
    double ax = 0.0, ay = 0.0, avx = 0.0, avy = 0.0;
    if (has) {                                                     // slots at or beyond n_act are never read
        const double* a = io.actors + 4 * slot;
        ax = a[0]; ay = a[1]; avx = a[2]; avy = a[3];
    }
    // ref test_9.py:62-84
    const double dx = x - ax, dy = y - ay;
    const double dis = sqrt((dx * dx + dy * dy) + 0.0);
    const double v1x = ax - x, v1y = ay - y;
    const double lat = v1x * (-s) + v1y * c;
    const double along = v1x * w.wx + v1y * w.wy;
    const double speed = sqrt((avx * avx + avy * avy) + 0.0);
    const bool kept = has && dis < prm.dis_limitation && -prm.lateral_band < lat && lat < prm.lateral_band && along > prm.behind;
    const bool is_dyn = kept && speed > prm.dynamic_speed;
    const bool is_stat = kept && !is_dyn;
    const unsigned long long mask_s = __ballot(is_stat), mask_d = __ballot(is_dyn);
    int rank = 0;
    for (unsigned long long m = mask_s | mask_d; m; m &= m - 1) {
        const int j = __ffsll((long long)m) - 1;
        const double dj = __shfl(dis, j);
        const bool j_dyn = (mask_d >> j) & 1ull;
        rank += (int)((j_dyn == is_dyn) & ((dj < dis) | ((dj == dis) & (j < lane))));
    }
    const int kept_s = __popcll(mask_s), kept_d = __popcll(mask_d);
    const int ns = min(kept_s, max_obs), nd = min(kept_d, max_dyn);
    if (is_stat && rank < max_obs) {
        const size_t o = (size_t)b * max_obs + rank;
        io.static_xy[2 * o] = ax;
        io.static_xy[2 * o + 1] = ay;
        io.static_dis[o] = dis;
    }
    if (is_dyn && rank < max_dyn) {
        double* o = io.dyn + 4 * ((size_t)b * max_dyn + rank);
        o[0] = ax; o[1] = ay; o[2] = dis; o[3] = speed;
        if constexpr (TM::kTimed) {
            double* v = tm.dyn_obs + 4 * ((size_t)b * max_dyn + rank);
            v[0] = ax; v[1] = ay; v[2] = avx; v[3] = avy;
        }
    }
    for (int q = ns + lane; q < max_obs; q += 64) {                // unused slots are 0: every output is determined
        const size_t o = (size_t)b * max_obs + q;
        io.static_xy[2 * o] = 0.0;
        io.static_xy[2 * o + 1] = 0.0;
        io.static_dis[o] = 0.0;
    }
    for (int q = nd + lane; q < max_dyn; q += 64) {
        double* o = io.dyn + 4 * ((size_t)b * max_dyn + q);
        o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
        if constexpr (TM::kTimed) {
            double* v = tm.dyn_obs + 4 * ((size_t)b * max_dyn + q);
            v[0] = 0.0; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0;
        }
    }
    if (io.actors_next) {
        double* o = io.actors_next + 4 * slot;
        if (has) {
            o[0] = ax + avx * prm.advance_s;
            o[1] = ay + avy * prm.advance_s;
            o[2] = avx;
            o[3] = avy;
        } else if (lane < max_act && io.actors_next != io.actors) {
            const double* a = io.actors + 4 * slot;
            o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
        }
    }
    if (io.log_state && lane < 6) io.log_state[6 * (size_t)b + lane] = st[lane];
    // the nearest of each class, to every lane
    const unsigned long long first_s = __ballot(is_stat && rank == 0), first_d = __ballot(is_dyn && rank == 0);
    const int ls = first_s ? __ffsll((long long)first_s) - 1 : 0, ld = first_d ? __ffsll((long long)first_d) - 1 : 0;
    const double s_dis0 = __shfl(dis, ls), d_dis0 = __shfl(dis, ld), d_speed0 = __shfl(speed, ld);
    if (lane != 0) return;
    // ref planning_utils.py:599-612 (products left to right)
    const double V = sqrt((w.wx * w.wx + w.wy * w.wy) + 0.0);
    const double heading = atan2(w.wy, w.wx);
    const double beta = heading - fi;
    const double V_y = V * sin(beta), V_x = V * cos(beta);
    const double ts = prm.pred_ts;
    io.n_static[b] = ns;
    io.n_dyn[b] = nd;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    io.dyn_dis_speed[2 * (size_t)b] = kept_d > 0 ? d_dis0 : nan;
    io.dyn_dis_speed[2 * (size_t)b + 1] = kept_d > 0 ? d_speed0 : nan;
    const int n_obs = (ns > 0 && s_dis0 <= prm.static_gate) ? ns : 0;          // ref test_9.py:116
    io.n_obs[b] = n_obs;
    io.origin_xy[2 * (size_t)b] = x;
    io.origin_xy[2 * (size_t)b + 1] = y;
    io.start_xy[2 * (size_t)b] = (x + V_x * ts * c) - V_y * ts * s;
    io.start_xy[2 * (size_t)b + 1] = (y + V_y * ts * c) + V_x * ts * s;
    io.pred_fi[b] = fi + fi_dot * ts;
    io.start_v[2 * (size_t)b] = w.wx;
    io.start_v[2 * (size_t)b + 1] = w.wy;
    io.start_a[2 * (size_t)b] = io.accel ? io.accel[2 * (size_t)b] : 0.0;
    io.start_a[2 * (size_t)b + 1] = io.accel ? io.accel[2 * (size_t)b + 1] : 0.0;
    io.req_status[b] = (kept_s > max_obs || kept_d > max_dyn) ? 1 : 0;           // EMP_DRV_TRUNCATED
    if (io.log_counts) {
        io.log_counts[2 * (size_t)b] = n_obs;
        io.log_counts[2 * (size_t)b + 1] = nd;
    }
    if constexpr (TM::kTimed) {
        tm.start_heading[b] = heading;                                           // ref test_10.py:247
        tm.plan_start_time[b] = (tm.t0[b] + (double)tm.tick * tm.dt) + tm.plan_lead;      // :325; nothing accumulates over periods
    }
}

struct AdoptIO {
    const double* traj;         // [B][max_pts + 1][4] the cycle's
    const int* traj_len;        // [B]
    const int* status;          // [B]
    const int* ref_status;      // [B]
    const int* match_index;     // [B]
    const double* track_in;     // [B][max_pts + 1][4]
    const int* track_len_in;    // [B]
    const int* held_in;         // [B]
    double* track_out;          // each output may be its input: an element is read by the lane that writes it
    int* track_len_out;
    int* held_out;
    int* pre_match_out;         // [B] the next period's pre_match_index
    int* log_plan_status;       // [B] or null: status | ref_status
    int* log_held;              // [B] or null
    double* log_traj;           // [B][max_pts + 1][4] or null
    int* log_traj_len;          // [B] or null
};

// What emp_drive_timed adds to the adoption: the period's timed trajectory becomes the profile the PID follows when the path is
// valid AND speed_status == 0 (cursor 0, speed_held 0); otherwise the profile and its cursor stay - still on the absolute clock, so
// the sampling rule goes on reading it - and speed_held counts.  The track is adopted or held by its own rule, independently.
constexpr int kProfile = 7 * ctl::kTimedPoints;      // doubles of one vehicle's profile: 22 456 B
struct NoSpeed {
    static constexpr bool kTimed = false;
};
struct Speed {
    static constexpr bool kTimed = true;
    const double* trajectory;   // [B][7][401] the period's
    const int* speed_status;    // [B]
    const double* profile_in;   // [B][7][401]
    const int* cursor_in;       // [B]
    const int* speed_held_in;   // [B]
    double* profile_out;        // each output may be its input: an element is read by the lane that writes it
    int* cursor_out;
    int* speed_held_out;
    int* log_speed_status;      // [B] or null
    int* log_speed_held;        // [B] or null
    int* log_cursor;            // [B] or null: the cursor the period's ticks start from
    double* log_profile;        // [B][7][401] or null: the period's trajectory, adopted or not
};

// One wavefront per vehicle, rows copied by lanes (consecutive lanes, consecutive doubles).  A plan is valid when ref_status == 0
// and status has no bit but EMP_ST_DP_INFEASIBLE (service.py's rule): its first traj_len rows become the track and held is 0;
// otherwise the track stays and held counts the periods it has been held.
template <typename TS>
__global__ __launch_bounds__(256) void drive_adopt_kernel(int B, int max_pts, AdoptIO io, TS ts) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (b >= B) return;
    const int st = io.status[b], rs = io.ref_status[b];
    const bool valid = rs == 0 && (st & ~1) == 0;
    const int tl = min(max(io.traj_len[b], 0), max_pts + 1);
    const int row = (max_pts + 1) * 4;
    const size_t base = (size_t)b * row;
    const bool moved = io.track_out != io.track_in;
    for (int i = lane; i < row; i += 64) {
        const double t = io.traj[base + i];
        if (io.log_traj) io.log_traj[base + i] = t;
        const bool take = valid && i < 4 * tl;
        if (take) io.track_out[base + i] = t;
        else if (moved) io.track_out[base + i] = io.track_in[base + i];
    }
    if constexpr (TS::kTimed) {
        const bool adopt = valid && ts.speed_status[b] == 0;
        const bool read = adopt || ts.log_profile != nullptr, kept = !adopt && ts.profile_out != ts.profile_in;
        const size_t pb = (size_t)b * kProfile;
        if (read || kept) {                                        // (a profile held in place without a log: nothing moves)
            for (int i = lane; i < kProfile; i += 64) {
                const double t = read ? ts.trajectory[pb + i] : 0.0;
                if (ts.log_profile) ts.log_profile[pb + i] = t;
                if (adopt) ts.profile_out[pb + i] = t;
                else if (kept) ts.profile_out[pb + i] = ts.profile_in[pb + i];
            }
        }
        if (lane == 0) {
            const int sheld = adopt ? 0 : ts.speed_held_in[b] + 1, cur = adopt ? 0 : ts.cursor_in[b];
            ts.cursor_out[b] = cur;
            ts.speed_held_out[b] = sheld;
            if (ts.log_speed_status) ts.log_speed_status[b] = ts.speed_status[b];
            if (ts.log_speed_held) ts.log_speed_held[b] = sheld;
            if (ts.log_cursor) ts.log_cursor[b] = cur;
        }
    }
    if (lane != 0) return;
    const int held = valid ? 0 : io.held_in[b] + 1;
    io.track_len_out[b] = valid ? tl : io.track_len_in[b];
    io.held_out[b] = held;
    io.pre_match_out[b] = io.match_index[b];
    if (io.log_plan_status) io.log_plan_status[b] = st | rs;
    if (io.log_held) io.log_held[b] = held;
    if (io.log_traj_len) io.log_traj_len[b] = io.traj_len[b];
}

// One vehicle per lane: accel = (w(state_end) - w(state_prev)) / dt with the request kernel's w; state_prev is the state the
// controller saw at the period's last tick.
__global__ __launch_bounds__(256) void drive_accel_kernel(int B, double dt, const double* __restrict__ state_end,
                                                          const double* __restrict__ state_prev, double* __restrict__ accel) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* e = state_end + 6 * (size_t)b;
    const double* p = state_prev + 6 * (size_t)b;
    const World we = world_velocity(cos(e[2]), sin(e[2]), e[3], e[5]);
    const World wp = world_velocity(cos(p[2]), sin(p[2]), p[3], p[5]);
    accel[2 * (size_t)b] = (we.wx - wp.wx) / dt;
    accel[2 * (size_t)b + 1] = (we.wy - wp.wy) / dt;
}

}  // namespace drive
}  // namespace emp
