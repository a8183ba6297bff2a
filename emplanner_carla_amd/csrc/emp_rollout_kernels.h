// emp_rollout_kernels.h - the vehicle model on the device (emp_vehicle_step) and the closed loop in ONE launch (emp_rollout):
// T ticks of [lateral law + PID + actuation] (emp_vehicle_control) followed by the vehicle model (emp_vehicle_step); and the same
// loop with the PID's target sampled every tick from a timed trajectory (emp_speed_target, emp_rollout_timed).
//
// The model is the project's own (csrc/emp_control_core.h: ctl::vehicle_step) - the reference's plant is CARLA (its main loop,
// test_9.py:336-436, calls Controller.run_step 100 times per planning cycle against the simulator).
//
// Contract: every output equals, bit for bit, T iterations of the two stand-alone calls on the same arrays.  That holds because
// a tick calls the very functions the stand-alone kernels call (mpc_lateral_core / lqr_lateral_core, ctl::pid_step, ctl::actuate,
// ctl::vehicle_step), the library is compiled without contraction or fast-math, and what travels through HBM between the
// stand-alone calls travels through registers here unchanged.
//
// Mappings are those of the lateral kernels: 12 lanes per vehicle and 5 vehicles per wavefront (MPC), one vehicle per lane (LQR).
// The state lives in registers for the whole rollout; the PID deque lives in LDS (5 x 60 doubles per wavefront for MPC, 64 rows
// for LQR), is summed oldest to newest by the same ctl::pid_step, and goes back to HBM once at the end; the path window is
// re-read every tick (it stays in L2); logs are plain vector stores.
//
// Cost note (LQR): the Riccati loop takes up to 5000 sweeps for a creeping vehicle (ref controller.py:470-481) and a wavefront
// runs as long as its slowest lane - per TICK here, so a fleet with one vehicle below ~1 m/s pays T x 5000 sweeps.
#pragma once

#include "emp_mpc_kernels.h"

namespace emp {
namespace rollout {

struct IO {
    ctl::PidParams pid;
    ctl::VehicleParams vp;
    int T, log_every;
    const double* state_in;        // [B][6]
    const int* min_index_in;       // [B]
    const double* target_speed;    // [B]
    const double* err_in;          // [B][60]
    const int* n_err_in;           // [B]
    double* state_out;             // [B][6]; each output may be the memory of its input: a vehicle's inputs are all read
    int* min_index_out;            // [B]     before its first output is written, and no vehicle reads another's
    double* err_out;               // [B][60]
    int* n_err_out;                // [B]
    int* status;                   // [B]
    int* fail_tick;                // [B]
    double* log_state;             // [n_log][B][6] or null
    double* log_control;           // [n_log][B][3] or null
    double* log_err;               // [n_log][B][4] or null
    int* log_index;                // [n_log][B] or null
};

// What emp_rollout_timed adds to IO: the timed trajectory whose speed / time rows give every tick's PID target (ctl::speed_target,
// the rule of include/emplanner.h), with target_speed as the cap.  emp_rollout's instantiations take NoProfile and are the kernels
// they were: every timed statement sits behind `if constexpr (Tgt::kTimed)`.
struct NoProfile {
    static constexpr bool kTimed = false;
};
struct Profile {
    static constexpr bool kTimed = true;
    const double* trajectory;      // [B][7][401]; rows 4 (speed, m/s) and 6 (time, s) are read
    const double* t0;              // [B]
    const int* cursor_in;          // [B] or null (zeros)
    int tick0;
    int* cursor_out;               // [B] (may be cursor_in)
    int* tgt_status;               // [B] OR of the ticks' EMP_TGT_* bits
    double* log_target;            // [n_log][B] or null
};
constexpr int kTrajRows = 7, kSpeedRow = 4, kTimeRow = 6;

__device__ __forceinline__ const double* profile_row(const double* trajectory, int b, int row) {
    return trajectory + ((size_t)b * kTrajRows + row) * ctl::kTimedPoints;
}

// control_epilogue (emp_mpc_kernels.h) on PID state that stays on chip: the deque `e` (60 doubles in LDS, updated in place as
// ctl::pid_step allows) and its count in a register.  A failing vehicle: zero controls, PID state untouched.
__device__ __forceinline__ void control_tick(const ctl::PidParams& pid, double speed_kmh, double target, double* e, int* n,
                                             int lat_status, double lat, double (&c3)[3]) {
    if (lat_status == 0) {
        int nn = 0;
        const double acc = ctl::pid_step(pid, speed_kmh, target, e, *n, e, &nn);
        *n = nn;
        ctl::actuate(lat, acc, &c3[0], &c3[1], &c3[2]);
    } else {
        c3[0] = c3[1] = c3[2] = 0.0;
    }
}

// rows of tick t for vehicle b: the state the controller saw, its controls, e_rr and the match it found
__device__ __forceinline__ void write_log(const IO& io, int B, int b, int t, const ctl::VehicleState& s, const double (&c3)[3],
                                          const mpc::LatResult& o) {
    if (t % io.log_every != 0) return;
    const size_t row = (size_t)(t / io.log_every) * B + b;
    if (io.log_state) {
        double* p = io.log_state + 6 * row;
        p[0] = s.x; p[1] = s.y; p[2] = s.fi; p[3] = s.Vy; p[4] = s.fi_dot; p[5] = s.Vx;
    }
    if (io.log_control) {
        double* p = io.log_control + 3 * row;
        p[0] = c3[0]; p[1] = c3[1]; p[2] = c3[2];
    }
    if (io.log_err)
#pragma unroll
        for (int q = 0; q < 4; ++q) io.log_err[4 * row + q] = o.e_rr.v[q];
    if (io.log_index) io.log_index[row] = o.idx;
}

__device__ __forceinline__ void write_final(const IO& io, int b, const ctl::VehicleState& s, int idx, const double* e, int n,
                                            int status, int fail_tick) {
    double* p = io.state_out + 6 * (size_t)b;
    p[0] = s.x; p[1] = s.y; p[2] = s.fi; p[3] = s.Vy; p[4] = s.fi_dot; p[5] = s.Vx;
    io.min_index_out[b] = idx;
    double* eo = io.err_out + (size_t)b * ctl::kPidBuffer;
    for (int i = 0; i < ctl::kPidBuffer; ++i) eo[i] = e[i];
    io.n_err_out[b] = n;
    io.status[b] = status;
    io.fail_tick[b] = fail_tick;
}

__device__ __forceinline__ ctl::VehicleState load_state(const double* state, int b) {
    const double* p = state + 6 * (size_t)b;
    return ctl::VehicleState{p[0], p[1], p[2], p[3], p[4], p[5]};
}

// grid = ceil(B / 5), block = 64 (mpc_lateral_kernel's).  The 12 lanes of a group carry the vehicle's state redundantly and step
// it with the same arithmetic; the group's lane 0 owns the PID deque and hands the three controls to the others.
template <class Tgt>
__global__ __launch_bounds__(64) void mpc_rollout_kernel(int B, int max_path, mpc::Params prm, const double* __restrict__ target_path,
                                                         const int* __restrict__ n_path, IO io, Tgt tg) {
    __shared__ double pid_err[mpc::kGroupsPerWave][ctl::kPidBuffer];
    const int lane = threadIdx.x & 63;
    const int grp = lane / mpc::kNu, r = lane - grp * mpc::kNu;
    const int gb = grp * mpc::kNu;
    const int b = blockIdx.x * mpc::kGroupsPerWave + grp;
    const bool live = grp < mpc::kGroupsPerWave && b < B;
    const int bb = live ? b : 0;                                   // an idle group shadows vehicle 0 and writes nothing
    const bool owner = live && r == 0;
    const double* path = target_path + (size_t)bb * max_path * 4;
    const int np_ = min(max(n_path[bb], 0), max_path);             // a count beyond the row is clamped, never followed
    ctl::VehicleState s = load_state(io.state_in, bb);
    int idx = io.min_index_in[bb];
    double target = io.target_speed[bb];                           // timed: the cap, and every tick's target on the owner lane
    int n_err = io.n_err_in[bb];
    double* e = pid_err[owner ? grp : 0];
    if (owner)
        for (int i = 0; i < ctl::kPidBuffer; ++i) e[i] = io.err_in[(size_t)b * ctl::kPidBuffer + i];
    // timed: the group's 12 lanes scan the two rows strided for the first NaN; the owner lane keeps the profile's state
    const double *p_speed = nullptr, *p_time = nullptr;
    double cap = 0.0, t0 = 0.0;
    int n_v = 0, cursor = 0, tgt_bits = 0;
    if constexpr (Tgt::kTimed) {
        p_speed = profile_row(tg.trajectory, bb, kSpeedRow);
        p_time = profile_row(tg.trajectory, bb, kTimeRow);
        int first = ctl::kTimedPoints;
        for (int i = r; i < ctl::kTimedPoints; i += mpc::kNu) {
            const double tv = p_time[i], sv = p_speed[i];
            if ((tv != tv || sv != sv) && first == ctl::kTimedPoints) first = i;
        }
        n_v = first;
#pragma unroll
        for (int k = 0; k < mpc::kNu; ++k) n_v = min(n_v, mpc::grp_bcast_int(first, gb, k));
        cap = target;
        t0 = tg.t0[bb];
        cursor = tg.cursor_in ? tg.cursor_in[bb] : 0;
    }
    int status = 0, fail_tick = -1;
    for (int t = 0; t < io.T; ++t) {
        double h[mpc::kNu], f_r, u;
        mpc::LatResult o;
        mpc::mpc_lateral_core(prm, path, np_, s.x, s.y, s.fi, s.Vy, s.fi_dot, ctl::clamp_vx(s.Vx), idx, live, r, gb, h, &f_r, &u, &o);
        double c3[3] = {0.0, 0.0, 0.0};
        if constexpr (Tgt::kTimed)
            if (owner) {
                int bits = 0;
                target = ctl::speed_target(p_speed, p_time, n_v, ctl::tick_clock(t0, tg.tick0 + t, io.vp.dt), cap, &cursor, &bits);
                tgt_bits |= bits;
                if (tg.log_target && t % io.log_every == 0) tg.log_target[(size_t)(t / io.log_every) * B + b] = target;
            }
        if (owner) control_tick(io.pid, ctl::speed_kmh_of(s.Vx, s.Vy), target, e, &n_err, o.status, o.steer, c3);
#pragma unroll
        for (int k = 0; k < 3; ++k) c3[k] = mpc::grp_bcast(c3[k], gb, 0);
        if (owner) write_log(io, B, b, t, s, c3, o);
        if (o.status != 0 && fail_tick < 0) fail_tick = t;
        status |= o.status;
        idx = o.idx;
        s = ctl::vehicle_step(io.vp, s, c3[0], c3[1], c3[2]);
    }
    if (owner) write_final(io, b, s, idx, e, n_err, status, fail_tick);
    if constexpr (Tgt::kTimed)
        if (owner) {
            tg.cursor_out[b] = cursor;
            tg.tgt_status[b] = tgt_bits;
        }
}

// grid = ceil(B / 64), block = 64 (lqr_lateral_kernel's): one vehicle per lane.  A deque row is 61 doubles apart from the next,
// so that the 64 lanes' accesses to entry i fall on distinct LDS banks.
constexpr int kPidStride = ctl::kPidBuffer + 1;

template <class Tgt>
__global__ __launch_bounds__(64) void lqr_rollout_kernel(int B, int max_path, mpc::Params prm, const double* __restrict__ target_path,
                                                         const int* __restrict__ n_path, IO io, Tgt tg) {
    __shared__ double pid_err[64 * kPidStride];
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* path = target_path + (size_t)b * max_path * 4;
    const int np_ = min(max(n_path[b], 0), max_path);              // a count beyond the row is clamped, never followed
    ctl::VehicleState s = load_state(io.state_in, b);
    int idx = io.min_index_in[b];
    double target = io.target_speed[b];                            // timed: the cap, and every tick's target
    int n_err = io.n_err_in[b];
    double* e = pid_err + threadIdx.x * kPidStride;
    for (int i = 0; i < ctl::kPidBuffer; ++i) e[i] = io.err_in[(size_t)b * ctl::kPidBuffer + i];
    // timed: each lane scans its own two rows (uncoalesced, once per rollout against T Riccati iterations)
    const double *p_speed = nullptr, *p_time = nullptr;
    double cap = 0.0, t0 = 0.0;
    int n_v = 0, cursor = 0, tgt_bits = 0;
    if constexpr (Tgt::kTimed) {
        p_speed = profile_row(tg.trajectory, b, kSpeedRow);
        p_time = profile_row(tg.trajectory, b, kTimeRow);
        n_v = ctl::profile_count(p_speed, p_time);
        cap = target;
        t0 = tg.t0[b];
        cursor = tg.cursor_in ? tg.cursor_in[b] : 0;
    }
    int status = 0, fail_tick = -1;
    for (int t = 0; t < io.T; ++t) {
        mpc::V4 K;
        mpc::LatResult o;
        lqr::lqr_lateral_core(prm, path, np_, s.x, s.y, s.fi, s.Vy, s.fi_dot, ctl::clamp_vx(s.Vx), idx, &K, &o);
        if constexpr (Tgt::kTimed) {
            int bits = 0;
            target = ctl::speed_target(p_speed, p_time, n_v, ctl::tick_clock(t0, tg.tick0 + t, io.vp.dt), cap, &cursor, &bits);
            tgt_bits |= bits;
            if (tg.log_target && t % io.log_every == 0) tg.log_target[(size_t)(t / io.log_every) * B + b] = target;
        }
        double c3[3];
        control_tick(io.pid, ctl::speed_kmh_of(s.Vx, s.Vy), target, e, &n_err, o.status, o.steer, c3);
        write_log(io, B, b, t, s, c3, o);
        if (o.status != 0 && fail_tick < 0) fail_tick = t;
        status |= o.status;
        idx = o.idx;
        s = ctl::vehicle_step(io.vp, s, c3[0], c3[1], c3[2]);
    }
    write_final(io, b, s, idx, e, n_err, status, fail_tick);
    if constexpr (Tgt::kTimed) {
        tg.cursor_out[b] = cursor;
        tg.tgt_status[b] = tgt_bits;
    }
}

// emp_speed_target: one tick's sampling, one vehicle per lane.  cursor_out may be cursor_in (a lane reads its own before it writes).
__global__ __launch_bounds__(256) void speed_target_kernel(int B, const double* __restrict__ trajectory, const double* __restrict__ t0,
                                                           int tick, double dt, const double* __restrict__ cap, const int* cursor_in,
                                                           double* __restrict__ target_kmh, int* cursor_out,
                                                           int* __restrict__ tgt_status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* p_speed = profile_row(trajectory, b, kSpeedRow);
    const double* p_time = profile_row(trajectory, b, kTimeRow);
    int cursor = cursor_in ? cursor_in[b] : 0, bits = 0;
    target_kmh[b] = ctl::speed_target(p_speed, p_time, ctl::profile_count(p_speed, p_time), ctl::tick_clock(t0[b], tick, dt), cap[b],
                                      &cursor, &bits);
    cursor_out[b] = cursor;
    tgt_status[b] = bits;
}

// emp_vehicle_step: one vehicle per lane.  state_out may be state_in (a lane reads its six values before it writes them).
__global__ __launch_bounds__(256) void vehicle_step_kernel(int B, ctl::VehicleParams p, const double* state_in,
                                                           const double* __restrict__ control, double* state_out,
                                                           double* __restrict__ ctl_state, double* __restrict__ vx_ctl,
                                                           double* __restrict__ speed_kmh) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const ctl::VehicleState n = ctl::vehicle_step(p, load_state(state_in, b), control[3 * (size_t)b], control[3 * (size_t)b + 1],
                                                  control[3 * (size_t)b + 2]);
    double* o = state_out + 6 * (size_t)b;
    o[0] = n.x; o[1] = n.y; o[2] = n.fi; o[3] = n.Vy; o[4] = n.fi_dot; o[5] = n.Vx;
    if (ctl_state) {
        double* c = ctl_state + 5 * (size_t)b;
        c[0] = n.x; c[1] = n.y; c[2] = n.fi; c[3] = n.Vy; c[4] = n.fi_dot;
    }
    if (vx_ctl) vx_ctl[b] = ctl::clamp_vx(n.Vx);
    if (speed_kmh) speed_kmh[b] = ctl::speed_kmh_of(n.Vx, n.Vy);
}

}  // namespace rollout
}  // namespace emp
