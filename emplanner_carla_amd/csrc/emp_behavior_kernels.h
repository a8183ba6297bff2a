// emp_behavior_kernels.h - traffic that reacts to traffic: the car-following law of the reference's BehaviorAgent
// (emp_behavior_core.h) for W worlds of up to 64 agents, one world per 64-lane block, one agent per lane.
//   agent_behave_kernel     one tick of the law (emp_agent_behave)
//   traffic_rollout_kernel  T ticks of [observe, behave, ctl::vehicle_step] in ONE launch (emp_traffic_rollout)
//
// Contract of the rollout: every output equals, bit for bit, T iterations of emp_agent_observe, emp_agent_behave and
// emp_vehicle_step on the same arrays.  A tick calls the very functions the stand-alone kernels call (agt::observe, bhv::behave,
// ctl::vehicle_step), and what travels through HBM between the stand-alone calls travels through registers and LDS here.
//
// A tick is synchronous: every lane publishes what the others may see of it (x, y, km/h, its lane key) to LDS, the block meets
// at ONE barrier, and every lane scans its world from LDS (all lanes read the same address: a broadcast).  The published rows are
// double-buffered: a lane that runs ahead writes tick t + 1 into the other buffer while a slower lane still reads tick t, and
// cannot reach tick t + 2 before that lane has passed the barrier of tick t + 1.  NO LANE LEAVES BEFORE THE TICK LOOP ENDS:
// padding lanes (slot >= n_world) and DONE lanes meet every barrier; the trip count T and the barrier are uniform per block, and
// the barrier stands outside every lane-dependent branch.  (emp_behavior_launch.h has the LDS layout.)
#pragma once

#include <hip/hip_runtime.h>

#include "emp_agent_kernels.h"
#include "emp_behavior_core.h"
#include "emp_behavior_launch.h"
#include "emp_control_core.h"

namespace emp {
namespace bhv {

struct WorldIO {
    int max_world, max_path, max_other;
    long long tick0;
    long long other_tick0;         // the tick index the others' rows were taken at (the rollouts; 0 but for emp_traffic_rollout_epoch)
    const int* n_world;            // [W]
    const double* path;            // [A][max_path][4], A = W * max_world
    const int* n_path;             // [A]
    const int* lane;               // [A][max_path]
    const double* state;           // [A][6]
    const double* forward;         // [A][2]  (behave)
    const double* speed_kmh;       // [A]     (behave)
    const double* speed_limit;     // [A]
    const double* extent;          // [A]
    agt::StateIO st;
    const int* n_other;            // [W] or null
    const double* other;           // [W][max_other][5] or null
    const int* other_lane;         // [W][max_other] or null
    // one tick
    double* control;               // [A][3]
    int* status;                   // [A]
    int* mode;                     // [A]
    int* blocker;                  // [A]
    double* distance;              // [A]
    double* ttc;                   // [A]
    double* target_out;            // [A]
    double* lat_error;             // [A] or null
    double* lon_command;           // [A] or null
    // the rollout
    int T, log_every;
    double* state_out;             // [A][6]
    int* done_tick;                // [A]
    double* actors_out;            // [A][4] or null
    int* mode_ticks;               // [A][5]
    double* min_gap;               // [A]
    double* log_state;             // [n_log][A][6] or null
    double* log_control;           // [n_log][A][3] or null
    int* log_head;                 // [n_log][A] or null
    int* log_mode;                 // [n_log][A] or null
    double* log_target;            // [n_log][A] or null
};

// What a block keeps in LDS (emp_behavior_launch.h).
struct Lds {
    double* lon;
    double* lat;
    double* ext;
    double* other;
    int* okey;
    double* base;
    __device__ __forceinline__ double* pub(int buf) const { return base + kOffPub + buf * kPubDoubles; }
    __device__ __forceinline__ int* key(int buf) const { return reinterpret_cast<int*>(base + kOffKey) + buf * kLanes; }
};

__device__ __forceinline__ Lds carve(double* base, int lane) {
    Lds l;
    l.base = base;
    l.lon = base + kOffDeque + lane * kDequeStride;
    l.lat = base + kOffDeque + (kLanes + lane) * kDequeStride;
    l.ext = base + kOffExtent;
    l.other = base + kOffOther;
    l.okey = reinterpret_cast<int*>(base + kOffOtherKey);
    return l;
}

// The world of this block: its counts, and its others and extents copied to LDS (read after the first barrier of the tick loop).
struct World {
    int nw, no, a;
    bool live;
};
__device__ __forceinline__ World stage_world(const WorldIO& io, const Lds& l, int lane) {
    World w;
    const int b = blockIdx.x;
    w.nw = agt::clampi(io.n_world[b], 0, io.max_world);
    w.no = (io.max_other > 0 && io.n_other) ? agt::clampi(io.n_other[b], 0, io.max_other) : 0;
    w.live = lane < w.nw;                                  // nw <= max_world <= 64: a live lane's slot exists
    w.a = b * io.max_world + (w.live ? lane : 0);
    if (w.live) l.ext[lane] = io.extent[w.a];
    if (lane < w.no) {
        const double* r = io.other + ((size_t)b * io.max_other + lane) * 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) l.other[5 * lane + i] = r[i];
        l.okey[lane] = io.other_lane[(size_t)b * io.max_other + lane];
    }
    return w;
}

__device__ __forceinline__ void publish(const Lds& l, int buf, int lane, double x, double y, double kmh, int key) {
    double* p = l.pub(buf);
    p[lane] = x;
    p[kLanes + lane] = y;
    p[2 * kLanes + lane] = kmh;
    l.key(buf)[lane] = key;
}

__device__ __forceinline__ Scene scene(const Lds& l, int buf, int lane, const World& w, double tau) {
    const double* p = l.pub(buf);
    return Scene{lane, w.nw, w.no, p, p + kLanes, p + 2 * kLanes, l.ext, l.key(buf), l.other, l.okey, tau};
}

// emp_agent_behave: grid = W, block = 64.
__global__ __launch_bounds__(64) void agent_behave_kernel(agt::Params ap, Params bp, WorldIO io) {
    __shared__ double lds[kLdsDoubles];
    const int lane = threadIdx.x;
    const Lds l = carve(lds, lane);
    const World w = stage_world(io, l, lane);
    const int a = w.a;
    const int np_ = w.live ? agt::clampi(io.n_path[a], 0, io.max_path) : 0;
    const int* lrow = io.lane + (size_t)a * io.max_path;
    agt::Agent g{};
    double x = 0.0, y = 0.0, kmh = 0.0;
    if (w.live) {
        g = agt::load_agent(io.st, a, np_, l.lon, l.lat);
        x = io.state[6 * (size_t)a];
        y = io.state[6 * (size_t)a + 1];
        kmh = io.speed_kmh[a];
        publish(l, 0, lane, x, y, kmh, shown_key(lrow, np_, g.head));
    }
    __syncthreads();                                       // every lane of the block, live or not
    if (!w.live) return;
    const Scene sc = scene(l, 0, lane, w, (double)io.tick0 * ap.dt);
    const Out o = behave(ap, bp, io.path + (size_t)a * io.max_path * 4, lrow, np_, x, y, io.forward[2 * (size_t)a],
                         io.forward[2 * (size_t)a + 1], kmh, io.speed_limit[a], l.ext[lane], sc, g);
    agt::store_agent(io.st, a, g);
    double* c3 = io.control + 3 * (size_t)a;
    c3[0] = o.k.throttle; c3[1] = o.k.steer; c3[2] = o.k.brake;
    io.status[a] = o.k.status;
    io.mode[a] = o.mode;
    io.blocker[a] = o.blocker;
    io.distance[a] = o.distance;
    io.ttc[a] = o.ttc;
    io.target_out[a] = o.target;
    if (io.lat_error) io.lat_error[a] = o.k.lat_error;
    if (io.lon_command) io.lon_command[a] = o.k.lon_command;
}

// emp_traffic_rollout: grid = W, block = 64.
__global__ __launch_bounds__(64) void traffic_rollout_kernel(agt::Params ap, Params bp, ctl::VehicleParams vp, int A, WorldIO io) {
    __shared__ double lds[kLdsDoubles];
    const int lane = threadIdx.x;
    const Lds l = carve(lds, lane);
    const World w = stage_world(io, l, lane);
    const int a = w.a;
    const int np_ = w.live ? agt::clampi(io.n_path[a], 0, io.max_path) : 0;
    const double* path = io.path + (size_t)a * io.max_path * 4;
    const int* lrow = io.lane + (size_t)a * io.max_path;
    agt::Agent g{};
    ctl::VehicleState s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double limit = 0.0, extent = 0.0;
    if (w.live) {
        g = agt::load_agent(io.st, a, np_, l.lon, l.lat);
        const double* p = io.state + 6 * (size_t)a;
        s = ctl::VehicleState{p[0], p[1], p[2], p[3], p[4], p[5]};
        limit = io.speed_limit[a];
        extent = io.extent[a];
    }
    int status = 0, done_tick = -1, key_at = -1, key_val = -1;
    int ticks[kCountedModes] = {0, 0, 0, 0, 0};
    double min_gap = infinity();
    const int T = io.T;                                    // uniform: every lane runs every tick and meets every barrier
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        agt::Obs o{};
        if (w.live) {
            o = agt::observe(s.fi, s.Vy, s.Vx);
            int key = -1;
            if (np_ > 0) {                                 // shown_key, its row read again only when head has moved
                const int at = g.head - 1 < 0 ? 0 : g.head - 1;
                if (at != key_at) {
                    key_val = lrow[at];
                    key_at = at;
                }
                key = key_val;
            }
            publish(l, buf, lane, s.x, s.y, o.kmh, key);
        }
        __syncthreads();
        if (w.live) {
            const Scene sc = scene(l, buf, lane, w, (double)(io.tick0 + t - io.other_tick0) * ap.dt);
            const Out r = behave(ap, bp, path, lrow, np_, s.x, s.y, o.c, o.s, o.kmh, limit, extent, sc, g);
            if (t % io.log_every == 0) {
                const size_t row = (size_t)(t / io.log_every) * A + a;
                if (io.log_state) {
                    double* q = io.log_state + 6 * row;
                    q[0] = s.x; q[1] = s.y; q[2] = s.fi; q[3] = s.Vy; q[4] = s.fi_dot; q[5] = s.Vx;
                }
                if (io.log_control) {
                    double* q = io.log_control + 3 * row;
                    q[0] = r.k.throttle; q[1] = r.k.steer; q[2] = r.k.brake;
                }
                if (io.log_head) io.log_head[row] = g.head;
                if (io.log_mode) io.log_mode[row] = r.mode;
                if (io.log_target) io.log_target[row] = r.target;
            }
            if ((r.k.status & agt::kDone) && done_tick < 0) done_tick = t;
            status |= r.k.status;
#pragma unroll
            for (int m = 0; m < kCountedModes; ++m) ticks[m] += r.mode == m ? 1 : 0;
            if (r.blocker >= 0 && r.distance < min_gap) min_gap = r.distance;
            s = ctl::vehicle_step(vp, s, r.k.throttle, r.k.steer, r.k.brake);
        }
    }
    if (!w.live) return;
    double* q = io.state_out + 6 * (size_t)a;
    q[0] = s.x; q[1] = s.y; q[2] = s.fi; q[3] = s.Vy; q[4] = s.fi_dot; q[5] = s.Vx;
    agt::store_agent(io.st, a, g);
    io.status[a] = status;
    io.done_tick[a] = done_tick;
#pragma unroll
    for (int m = 0; m < kCountedModes; ++m) io.mode_ticks[kCountedModes * (size_t)a + m] = ticks[m];
    io.min_gap[a] = min_gap;
    if (io.actors_out) agt::store_actor(io.actors_out, a, s.x, s.y, agt::observe(s.fi, s.Vy, s.Vx));
}

}  // namespace bhv
}  // namespace emp
