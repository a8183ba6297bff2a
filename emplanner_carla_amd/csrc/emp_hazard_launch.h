// emp_hazard_launch.h - the launch of the hazard kernels (emp_hazard_kernels.h) as pure host arithmetic: as emp_behavior_launch.h, no
// HIP types, readable by a plain C++17 compiler (tests/host_check/hazard_check.cpp runs it on the CPU).  One world per 64-lane
// block, one agent per lane.  The block's LDS is the behaviour kernels' layout (emp_behavior_launch.h), followed, in doubles from
// the block's start, by what lane q stages once before the first barrier and nobody writes afterwards:
//   light    64 rows of 4: x, y, dx, dy of the trigger waypoint
//   lkey     64 int32 lane keys
//   lcycle   64 rows of 3 int32: period, red_from, red_to
//   walker   64 rows of 5: x, y, vx, vy, half extent
//   wkey     64 int32 lane keys
#pragma once

#include "emp_behavior_launch.h"
#include "emp_hazard_core.h"

namespace emp {
namespace hz {

constexpr int kOffLight = bhv::kLdsDoubles;                          // 2272
constexpr int kOffLightKey = kOffLight + 4 * kMaxLight;              // 2528
constexpr int kOffLightCycle = kOffLightKey + kMaxLight / 2;         // 2560
constexpr int kOffWalker = kOffLightCycle + 3 * kMaxLight / 2;       // 2656
constexpr int kOffWalkerKey = kOffWalker + 5 * kMaxWalker;           // 2976
constexpr int kLdsDoubles = kOffWalkerKey + kMaxWalker / 2;          // 3008

constexpr const char* kBadLight = "max_light outside [0, EMP_HAZARD_MAX]";
constexpr const char* kBadWalker = "max_walker outside [0, EMP_HAZARD_MAX]";

// Everything plan_behavior refuses, then the two row counts.  T == 0 plans the single tick of emp_agent_behave_hazards.
static inline bhv::BehaviorPlan plan_hazards(int W, int max_world, int max_other, int max_light, int max_walker, int max_path, int T,
                                             int log_every, int64_t tick0) {
    bhv::BehaviorPlan p = bhv::plan_behavior(W, max_world, max_other, max_path, T, log_every, tick0);
    if (!p.error) {
        if (max_light < 0 || max_light > kMaxLight) p.error = kBadLight;
        else if (max_walker < 0 || max_walker > kMaxWalker) p.error = kBadWalker;
    }
    if (p.error) return bhv::BehaviorPlan{0, 0, 0, 0, 0, p.error};
    if (W == 0) return p;
    p.lds = sizeof(double) * kLdsDoubles;
    const size_t fit = kLdsBytes / p.lds;
    p.blocks_per_cu = fit < 32 ? (int)fit : 32;
    return p;
}

}  // namespace hz
}  // namespace emp
