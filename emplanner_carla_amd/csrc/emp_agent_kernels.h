// emp_agent_kernels.h - routed traffic on the device: the reference's LocalPlanner / VehiclePIDController pair (emp_agent_core.h)
// for a fleet of agents, one agent per lane.
//   agent_observe_kernel  what the CARLA getters return for a vehicle of the project's model (emp_agent_observe)
//   agent_control_kernel  one tick of the law (emp_agent_control)
//   agent_rollout_kernel  T ticks of [observe, control, ctl::vehicle_step] in ONE launch (emp_agent_rollout)
//
// Contract of the rollout: every output equals, bit for bit, T iterations of the three stand-alone calls on the same arrays.  A
// tick calls the very functions the stand-alone kernels call (agt::observe, agt::tick, ctl::vehicle_step), the library is compiled
// without contraction or fast-math, and what travels through HBM between the stand-alone calls travels through registers here.
//
// The state and the head waypoint live in registers for the whole rollout; the two deques live in lane-private LDS rows 11 doubles
// apart (rollout::kPidStride's idea: the 32 lanes of a ds_read_b64 group fall on distinct banks) and go back to HBM once at the
// end.  A path row is read only when `head` moves (about once per 30 ticks at 2 m spacing; the rows are scattered per lane).  No
// lane waits for another: there is no barrier, and a DONE lane runs the vehicle model only.
#pragma once

#include <hip/hip_runtime.h>

#include "emp_agent_core.h"
#include "emp_control_core.h"

namespace emp {
namespace agt {

constexpr int kStride = kBuffer + 1;

__device__ __forceinline__ void store_actor(double* actors, int a, double x, double y, const Obs& o) {
    double* p = actors + 4 * (size_t)a;
    p[0] = x; p[1] = y; p[2] = o.wx; p[3] = o.wy;
}

// emp_agent_observe.  Each output may be null.
__global__ __launch_bounds__(256) void agent_observe_kernel(int A, const double* __restrict__ state, double* __restrict__ forward,
                                                            double* __restrict__ speed_kmh, double* __restrict__ actors) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const double* st = state + 6 * (size_t)a;
    const Obs o = observe(st[2], st[3], st[5]);
    if (forward) {
        forward[2 * (size_t)a] = o.c;
        forward[2 * (size_t)a + 1] = o.s;
    }
    if (speed_kmh) speed_kmh[a] = o.kmh;
    if (actors) store_actor(actors, a, st[0], st[1], o);
}

// The agent state of a call: inputs and outputs, each output possibly the memory of its input (a lane reads all of its inputs
// before it writes, and no lane reads another's).
struct StateIO {
    const int* head_in;            // [A]
    const double* past_in;         // [A]
    const double* lon_in;          // [A][10]
    const int* n_lon_in;           // [A]
    const double* lat_in;          // [A][10]
    const int* n_lat_in;           // [A]
    int* head_out;
    double* past_out;
    double* lon_out;
    int* n_lon_out;
    double* lat_out;
    int* n_lat_out;
};

// the agent of lane `a`, its two deques copied to lon / lat (kBuffer doubles each: registers or an LDS row)
__device__ __forceinline__ Agent load_agent(const StateIO& io, int a, int n_path, double* lon, double* lat) {
    Agent g;
    g.head = clampi(io.head_in[a], 0, n_path);
    g.n_lon = clampi(io.n_lon_in[a], 0, kBuffer);
    g.n_lat = clampi(io.n_lat_in[a], 0, kBuffer);
    g.past_steer = io.past_in[a];
    g.lon = lon;
    g.lat = lat;
    g.at = -1;
    g.px = g.py = 0.0;
#pragma unroll
    for (int i = 0; i < kBuffer; ++i) {
        lon[i] = io.lon_in[(size_t)a * kBuffer + i];
        lat[i] = io.lat_in[(size_t)a * kBuffer + i];
    }
    return g;
}

__device__ __forceinline__ void store_agent(const StateIO& io, int a, const Agent& g) {
    io.head_out[a] = g.head;
    io.past_out[a] = g.past_steer;
    io.n_lon_out[a] = g.n_lon;
    io.n_lat_out[a] = g.n_lat;
#pragma unroll
    for (int i = 0; i < kBuffer; ++i) {
        io.lon_out[(size_t)a * kBuffer + i] = g.lon[i];
        io.lat_out[(size_t)a * kBuffer + i] = g.lat[i];
    }
}

// emp_agent_control: the deques pass through registers (agt::pid10 indexes them with constants).
__global__ __launch_bounds__(64) void agent_control_kernel(int A, int max_path, Params prm, const double* __restrict__ path,
                                                           const int* __restrict__ n_path, const double* __restrict__ state,
                                                           const double* __restrict__ forward, const double* __restrict__ speed_kmh,
                                                           const double* __restrict__ target_speed, StateIO io,
                                                           double* __restrict__ control, int* __restrict__ status,
                                                           double* __restrict__ lat_error, double* __restrict__ lon_command) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const int np_ = clampi(n_path[a], 0, max_path);                // a count beyond the row is clamped, never followed
    double lon[kBuffer], lat[kBuffer];
    Agent g = load_agent(io, a, np_, lon, lat);
    const Tick k = tick(prm, path + (size_t)a * max_path * 4, np_, state[6 * (size_t)a], state[6 * (size_t)a + 1], forward[2 * (size_t)a],
                        forward[2 * (size_t)a + 1], speed_kmh[a], target_speed[a], g);
    store_agent(io, a, g);
    double* c3 = control + 3 * (size_t)a;
    c3[0] = k.throttle; c3[1] = k.steer; c3[2] = k.brake;
    status[a] = k.status;
    if (lat_error) lat_error[a] = k.lat_error;
    if (lon_command) lon_command[a] = k.lon_command;
}

struct RolloutIO {
    int T, log_every;
    const double* state_in;        // [A][6]
    const double* target_speed;    // [A]
    StateIO st;
    double* state_out;             // [A][6] (may be state_in)
    int* status;                   // [A] OR of the ticks' statuses
    int* done_tick;                // [A] first DONE tick, -1 if none
    double* actors_out;            // [A][4] or null: observe of the final state
    double* log_state;             // [n_log][A][6] or null
    double* log_control;           // [n_log][A][3] or null
    int* log_head;                 // [n_log][A] or null
};

// emp_agent_rollout: grid = ceil(A / 64), block = 64.
__global__ __launch_bounds__(64) void agent_rollout_kernel(int A, int max_path, Params prm, ctl::VehicleParams vp,
                                                           const double* __restrict__ path_all, const int* __restrict__ n_path,
                                                           RolloutIO io) {
    __shared__ double deque_lds[2 * 64 * kStride];
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const double* path = path_all + (size_t)a * max_path * 4;
    const int np_ = clampi(n_path[a], 0, max_path);
    Agent g = load_agent(io.st, a, np_, deque_lds + threadIdx.x * kStride, deque_lds + (64 + threadIdx.x) * kStride);
    const double* p = io.state_in + 6 * (size_t)a;
    ctl::VehicleState s{p[0], p[1], p[2], p[3], p[4], p[5]};
    const double target = io.target_speed[a];
    int status = 0, done_tick = -1;
    for (int t = 0; t < io.T; ++t) {
        const Obs o = observe(s.fi, s.Vy, s.Vx);
        const Tick k = tick(prm, path, np_, s.x, s.y, o.c, o.s, o.kmh, target, g);
        if (t % io.log_every == 0) {
            const size_t row = (size_t)(t / io.log_every) * A + a;
            if (io.log_state) {
                double* q = io.log_state + 6 * row;
                q[0] = s.x; q[1] = s.y; q[2] = s.fi; q[3] = s.Vy; q[4] = s.fi_dot; q[5] = s.Vx;
            }
            if (io.log_control) {
                double* q = io.log_control + 3 * row;
                q[0] = k.throttle; q[1] = k.steer; q[2] = k.brake;
            }
            if (io.log_head) io.log_head[row] = g.head;
        }
        if ((k.status & kDone) && done_tick < 0) done_tick = t;
        status |= k.status;
        s = ctl::vehicle_step(vp, s, k.throttle, k.steer, k.brake);
    }
    double* q = io.state_out + 6 * (size_t)a;
    q[0] = s.x; q[1] = s.y; q[2] = s.fi; q[3] = s.Vy; q[4] = s.fi_dot; q[5] = s.Vx;
    store_agent(io.st, a, g);
    io.status[a] = status;
    io.done_tick[a] = done_tick;
    if (io.actors_out) store_actor(io.actors_out, a, s.x, s.y, observe(s.fi, s.Vy, s.Vx));
}

}  // namespace agt
}  // namespace emp
