// emp_route_launch.h - the launch of route_kernel (emp_route_kernels.h) as pure host arithmetic: as emp_dp_launch.h and
// emp_tail_launch.h, no HIP types, readable by a plain C++17 compiler (tests/host_check/route_check.cpp runs it on the CPU).
// One query per 64-lane block; the dynamic LDS is the per-node search state (route::state_lds), 24 bytes a node.
#pragma once

#include <stddef.h>

#include "emp_dp_launch.h"        // kLdsBytes
#include "emp_route_core.h"

namespace emp {

constexpr int kWavesPerCu = 32;

struct RoutePlan {
    int grid = 0, block = 0;
    size_t lds = 0;             // dynamic LDS bytes of a block
    int waves_per_cu = 0;       // how many blocks (one wavefront each) the LDS lets a compute unit hold, at most kWavesPerCu (the
                                // kernel's registers may hold fewer: this is host arithmetic and knows only the LDS)
    const char* error = nullptr;
};

constexpr const char* kRouteTooManyNodes = "route graph: n_nodes outside [1, EMP_ROUTE_MAX_NODES]";
constexpr const char* kRouteBadCapacity = "max_route < 2 or max_global < 1";

// (the sizes are refused before the empty batch is let through, as plan_merge)
static inline RoutePlan plan_route(int B, int n_nodes, int max_route, int max_global) {
    RoutePlan p;
    if (n_nodes < 1 || n_nodes > route::kMaxNodes) p.error = kRouteTooManyNodes;
    else if (max_route < 2 || max_global < 1) p.error = kRouteBadCapacity;
    if (p.error || B <= 0) return p;
    p.grid = B;
    p.block = 64;
    p.lds = route::state_lds(size_t(0), n_nodes).end;
    const size_t fit = kLdsBytes / p.lds;
    p.waves_per_cu = fit < (size_t)kWavesPerCu ? (int)fit : kWavesPerCu;
    return p;
}

}  // namespace emp
