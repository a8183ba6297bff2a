// emp_behavior_launch.h - the launch of the behaviour kernels (emp_behavior_kernels.h) as pure host arithmetic: as
// emp_route_launch.h, no HIP types, readable by a plain C++17 compiler (tests/host_check/behavior_check.cpp runs it on the CPU).
// One world per 64-lane block, one agent per lane.  The block's LDS, in doubles from its start:
//   deque    2 x 64 rows of 11: the two error deques of each lane (emp_agent_rollout's rows: stride 11 keeps the 32 lanes of a
//            ds_read_b64 group on distinct banks)
//   pub      2 buffers of x[64], y[64], km/h[64]: what each lane shows the others at the start of a tick, double-buffered so that
//            one barrier a tick suffices
//   key      2 buffers of 64 int32 lane keys
//   extent   64: loaded once
//   other    64 rows of 5, and 64 int32 keys: loaded once
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "emp_behavior_core.h"
#include "emp_dp_launch.h"        // kLdsBytes

namespace emp {
namespace bhv {

constexpr int kLanes = 64;
constexpr int kDequeStride = agt::kBuffer + 1;
constexpr int kOffDeque = 0;
constexpr int kOffPub = kOffDeque + 2 * kLanes * kDequeStride;       // 1408
constexpr int kPubDoubles = 3 * kLanes;                              // one buffer
constexpr int kOffKey = kOffPub + 2 * kPubDoubles;                   // 1792
constexpr int kOffExtent = kOffKey + 2 * kLanes / 2;                 // 1856
constexpr int kOffOther = kOffExtent + kLanes;                       // 1920
constexpr int kOffOtherKey = kOffOther + 5 * kMaxWorld;              // 2240
constexpr int kLdsDoubles = kOffOtherKey + kMaxWorld / 2;            // 2272
constexpr int kMaxTicks = 65536;                                     // EMP_ROLLOUT_MAX_TICKS

struct BehaviorPlan {
    int grid = 0, block = 0;
    size_t lds = 0;             // static LDS bytes of a block
    int blocks_per_cu = 0;      // what the LDS lets a compute unit hold (one wavefront a block; the registers may hold fewer)
    size_t n_log = 0;           // log rows of a rollout: ceil(T / log_every)
    const char* error = nullptr;
};

constexpr const char* kBadWorld = "max_world outside [1, EMP_TRAFFIC_MAX_WORLD]";
constexpr const char* kBadOther = "max_other outside [0, EMP_TRAFFIC_MAX_WORLD]";
constexpr const char* kBadPath = "max_path < 1 or W < 0";
constexpr const char* kBadTicks = "T outside [1, EMP_ROLLOUT_MAX_TICKS], log_every < 1, tick0 < 0 or tick0 + T > INT32_MAX";

// T == 0 plans the single tick of emp_agent_behave (log_every is not looked at).  The sizes are refused before the empty batch is
// let through.
static inline BehaviorPlan plan_behavior(int W, int max_world, int max_other, int max_path, int T, int log_every, int64_t tick0) {
    BehaviorPlan p;
    if (max_world < 1 || max_world > kMaxWorld) p.error = kBadWorld;
    else if (max_other < 0 || max_other > kMaxWorld) p.error = kBadOther;
    else if (max_path < 1 || W < 0) p.error = kBadPath;
    else if (T < 0 || T > kMaxTicks || (T > 0 && log_every < 1) || tick0 < 0 || tick0 + T > INT32_MAX) p.error = kBadTicks;
    if (p.error || W == 0) return p;
    p.grid = W;
    p.block = kLanes;
    p.lds = sizeof(double) * kLdsDoubles;
    const size_t fit = kLdsBytes / p.lds;
    p.blocks_per_cu = fit < 32 ? (int)fit : 32;
    p.n_log = T > 0 ? ((size_t)T + (size_t)log_every - 1) / (size_t)log_every : 0;
    return p;
}

}  // namespace bhv
}  // namespace emp
