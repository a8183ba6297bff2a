// emp_hazard_kernels.h - traffic that stops for red lights and pedestrians: emp_hazard_core.h for W worlds of up to 64 agents, one
// world per 64-lane block, one agent per lane, built on the behaviour kernels' parts (emp_behavior_kernels.h).
//   agent_behave_hazards_kernel     one tick of the rule (emp_agent_behave_hazards)
//   traffic_rollout_hazards_kernel  T ticks of [observe, behave with hazards, ctl::vehicle_step] in ONE launch
//
// Contract of the rollout: every output equals, bit for bit, T iterations of emp_agent_observe, emp_agent_behave_hazards and
// emp_vehicle_step on the same arrays.  Lane q copies light q and walker q to LDS once, before the first barrier of the tick loop;
// nobody writes them afterwards, and every lane reads the same address at the same time (a broadcast).  The tick keeps the ONE
// barrier of traffic_rollout_kernel, outside every lane-dependent branch: padding, DONE and emergency lanes meet it.  The sticky
// light lives in a register across ticks.  (emp_hazard_launch.h has the LDS layout.)
#pragma once

#include <hip/hip_runtime.h>

#include "emp_behavior_kernels.h"
#include "emp_hazard_core.h"
#include "emp_hazard_launch.h"

namespace emp {
namespace hz {

struct HazardIO {
    int max_light, max_walker;
    const int* n_light;            // [W] or null
    const double* light;           // [W][max_light][4] or null
    const int* light_lane;         // [W][max_light] or null
    const int* light_cycle;        // [W][max_light][3] or null
    const int* n_walker;           // [W] or null
    const double* walker;          // [W][max_walker][5] or null
    const int* walker_lane;        // [W][max_walker] or null
    const int* last_light;         // [A]
    int* last_light_out;           // [A]
    // one tick
    int* cause;                    // [A]
    int* light_hit;                // [A]
    int* walker_hit;               // [A]
    double* walker_distance;       // [A]
    // the rollout
    int* cause_ticks;              // [A][3]
    double* min_walker_gap;        // [A]
    int* log_cause;                // [n_log][A] or null
};

// The lights and walkers of this block's world, copied to LDS (read after the first barrier).
__device__ __forceinline__ Scene stage_hazards(const HazardIO& h, double* base, int lane) {
    const int b = blockIdx.x;
    Scene sc;
    sc.n_light = (h.max_light > 0 && h.n_light) ? agt::clampi(h.n_light[b], 0, h.max_light) : 0;
    sc.n_walker = (h.max_walker > 0 && h.n_walker) ? agt::clampi(h.n_walker[b], 0, h.max_walker) : 0;
    double* light = base + kOffLight;
    int* lkey = reinterpret_cast<int*>(base + kOffLightKey);
    int* lcycle = reinterpret_cast<int*>(base + kOffLightCycle);
    double* walker = base + kOffWalker;
    int* wkey = reinterpret_cast<int*>(base + kOffWalkerKey);
    if (lane < sc.n_light) {                               // n_light <= max_light <= 64: the row exists
        const size_t q = (size_t)b * h.max_light + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) light[4 * lane + i] = h.light[4 * q + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) lcycle[3 * lane + i] = h.light_cycle[3 * q + i];
        lkey[lane] = h.light_lane[q];
    }
    if (lane < sc.n_walker) {
        const size_t q = (size_t)b * h.max_walker + lane;
#pragma unroll
        for (int i = 0; i < 5; ++i) walker[5 * lane + i] = h.walker[5 * q + i];
        wkey[lane] = h.walker_lane[q];
    }
    sc.light = light;
    sc.light_key = lkey;
    sc.light_cycle = lcycle;
    sc.walker = walker;
    sc.walker_key = wkey;
    sc.k = 0;
    sc.tau = 0.0;
    return sc;
}

// emp_agent_behave_hazards: grid = W, block = 64.
__global__ __launch_bounds__(64) void agent_behave_hazards_kernel(agt::Params ap, bhv::Params bp, Params hp, bhv::WorldIO io, HazardIO h) {
    __shared__ double lds[kLdsDoubles];
    const int lane = threadIdx.x;
    const bhv::Lds l = bhv::carve(lds, lane);
    const bhv::World w = bhv::stage_world(io, l, lane);
    Scene hs = stage_hazards(h, lds, lane);
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
        bhv::publish(l, 0, lane, x, y, kmh, bhv::shown_key(lrow, np_, g.head));
    }
    __syncthreads();                                       // every lane of the block, live or not
    if (!w.live) return;
    hs.k = io.tick0;
    hs.tau = (double)io.tick0 * ap.dt;
    const bhv::Scene sc = bhv::scene(l, 0, lane, w, hs.tau);
    int last = h.last_light[a];
    const Out o = behave(ap, bp, hp, io.path + (size_t)a * io.max_path * 4, lrow, np_, x, y, io.forward[2 * (size_t)a],
                         io.forward[2 * (size_t)a + 1], kmh, io.speed_limit[a], l.ext[lane], sc, hs, g, last);
    agt::store_agent(io.st, a, g);
    double* c3 = io.control + 3 * (size_t)a;
    c3[0] = o.b.k.throttle; c3[1] = o.b.k.steer; c3[2] = o.b.k.brake;
    io.status[a] = o.b.k.status;
    io.mode[a] = o.b.mode;
    io.blocker[a] = o.b.blocker;
    io.distance[a] = o.b.distance;
    io.ttc[a] = o.b.ttc;
    io.target_out[a] = o.b.target;
    if (io.lat_error) io.lat_error[a] = o.b.k.lat_error;
    if (io.lon_command) io.lon_command[a] = o.b.k.lon_command;
    h.last_light_out[a] = last;
    h.cause[a] = o.cause;
    h.light_hit[a] = o.light_hit;
    h.walker_hit[a] = o.walker_hit;
    h.walker_distance[a] = o.walker_distance;
}

// emp_traffic_rollout_hazards: grid = W, block = 64.
__global__ __launch_bounds__(64) void traffic_rollout_hazards_kernel(agt::Params ap, bhv::Params bp, Params hp, ctl::VehicleParams vp, int A,
                                                                     bhv::WorldIO io, HazardIO h) {
    __shared__ double lds[kLdsDoubles];
    const int lane = threadIdx.x;
    const bhv::Lds l = bhv::carve(lds, lane);
    const bhv::World w = bhv::stage_world(io, l, lane);
    Scene hs = stage_hazards(h, lds, lane);
    const int a = w.a;
    const int np_ = w.live ? agt::clampi(io.n_path[a], 0, io.max_path) : 0;
    const double* path = io.path + (size_t)a * io.max_path * 4;
    const int* lrow = io.lane + (size_t)a * io.max_path;
    agt::Agent g{};
    ctl::VehicleState s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double limit = 0.0, extent = 0.0;
    int last = -1;
    if (w.live) {
        g = agt::load_agent(io.st, a, np_, l.lon, l.lat);
        const double* p = io.state + 6 * (size_t)a;
        s = ctl::VehicleState{p[0], p[1], p[2], p[3], p[4], p[5]};
        limit = io.speed_limit[a];
        extent = io.extent[a];
        last = h.last_light[a];
    }
    int status = 0, done_tick = -1, key_at = -1, key_val = -1;
    int ticks[bhv::kCountedModes] = {0, 0, 0, 0, 0};
    int causes[kCountedCauses] = {0, 0, 0};
    double min_gap = bhv::infinity(), min_walker = bhv::infinity();
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
            bhv::publish(l, buf, lane, s.x, s.y, o.kmh, key);
        }
        __syncthreads();
        if (w.live) {
            hs.k = io.tick0 + t;
            hs.tau = (double)hs.k * ap.dt;
            // the others move from the tick their rows were taken at; lights and walkers stay on k
            const bhv::Scene sc = bhv::scene(l, buf, lane, w, (double)(hs.k - io.other_tick0) * ap.dt);
            const Out r = behave(ap, bp, hp, path, lrow, np_, s.x, s.y, o.c, o.s, o.kmh, limit, extent, sc, hs, g, last);
            if (t % io.log_every == 0) {
                const size_t row = (size_t)(t / io.log_every) * A + a;
                if (io.log_state) {
                    double* q = io.log_state + 6 * row;
                    q[0] = s.x; q[1] = s.y; q[2] = s.fi; q[3] = s.Vy; q[4] = s.fi_dot; q[5] = s.Vx;
                }
                if (io.log_control) {
                    double* q = io.log_control + 3 * row;
                    q[0] = r.b.k.throttle; q[1] = r.b.k.steer; q[2] = r.b.k.brake;
                }
                if (io.log_head) io.log_head[row] = g.head;
                if (io.log_mode) io.log_mode[row] = r.b.mode;
                if (io.log_target) io.log_target[row] = r.b.target;
                if (h.log_cause) h.log_cause[row] = r.cause;
            }
            if ((r.b.k.status & agt::kDone) && done_tick < 0) done_tick = t;
            status |= r.b.k.status;
#pragma unroll
            for (int m = 0; m < bhv::kCountedModes; ++m) ticks[m] += r.b.mode == m ? 1 : 0;
#pragma unroll
            for (int m = 0; m < kCountedCauses; ++m) causes[m] += r.cause == m + 1 ? 1 : 0;
            if (r.b.blocker >= 0 && r.b.distance < min_gap) min_gap = r.b.distance;
            if (r.walker_hit >= 0 && r.walker_distance < min_walker) min_walker = r.walker_distance;
            s = ctl::vehicle_step(vp, s, r.b.k.throttle, r.b.k.steer, r.b.k.brake);
        }
    }
    if (!w.live) return;
    double* q = io.state_out + 6 * (size_t)a;
    q[0] = s.x; q[1] = s.y; q[2] = s.fi; q[3] = s.Vy; q[4] = s.fi_dot; q[5] = s.Vx;
    agt::store_agent(io.st, a, g);
    io.status[a] = status;
    io.done_tick[a] = done_tick;
#pragma unroll
    for (int m = 0; m < bhv::kCountedModes; ++m) io.mode_ticks[bhv::kCountedModes * (size_t)a + m] = ticks[m];
    io.min_gap[a] = min_gap;
    if (io.actors_out) agt::store_actor(io.actors_out, a, s.x, s.y, agt::observe(s.fi, s.Vy, s.Vx));
    h.last_light_out[a] = last;
#pragma unroll
    for (int m = 0; m < kCountedCauses; ++m) h.cause_ticks[kCountedCauses * (size_t)a + m] = causes[m];
    h.min_walker_gap[a] = min_walker;
}

}  // namespace hz
}  // namespace emp
