// emp_world_kernels.h - world_exchange_kernel: who sees whom at the start of a period (emp_world_core.h), one world per 64-lane
// block, then one block per 64 egos for the egos in no world.
//
// A world's block observes its live agents once (lane = slot, agt::observe: the function emp_agent_observe calls, so the rows are
// that call's bit for bit) and keeps the rows in LDS; every ego of the world then gathers them, lane = row.  An ego's own row is
// observed again wherever it is listed - a world has a handful of egos and the function is deterministic.  The lane key an ego
// shows is a windowed nearest match: the lanes stride the window and reduce on (d2, index) with the butterfly of
// emp_route_kernels.h.  One barrier, outside every lane-dependent branch; a block writes only its own world's rows and its own
// egos', so no block waits for another.
#pragma once

#include <hip/hip_runtime.h>

#include "emp_agent_core.h"
#include "emp_world_core.h"

namespace emp {
namespace wx {

struct Wave64 {
    static constexpr int kLanes = 64;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ void argmin(double& d, int& idx) const {
        for (int off = 32; off; off >>= 1) {
            const double od = __shfl_xor(d, off);
            const int oi = __shfl_xor(idx, off);
            if (before(od, oi, d, idx)) {
                d = od;
                idx = oi;
            }
        }
        // the order is total on real indices, so every lane holds the same winner already; lane 0's copy makes that unconditional
        d = __shfl(d, 0);
        idx = __shfl(idx, 0);
    }
};

struct DeviceRows {
    const double* agent_rows;      // LDS: [64][4], the world's live agents
    const double* ego_state;       // [B][6]
    __device__ __forceinline__ void agent(int slot, double* v) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = agent_rows[4 * slot + i];
    }
    __device__ __forceinline__ void ego(int b, double* v) const {
        const double* st = ego_state + 6 * (size_t)b;
        const agt::Obs o = agt::observe(st[2], st[3], st[5]);
        v[0] = st[0]; v[1] = st[1]; v[2] = o.wx; v[3] = o.wy;
    }
};

// emp_world_exchange: grid = W + ceil(B / 64), block = 64.
__global__ __launch_bounds__(64) void world_exchange_kernel(Sizes z, const double* __restrict__ agent_state, In in, Out out) {
    __shared__ double rows[4 * kMaxRows];
    const int lane = (int)threadIdx.x, w = (int)blockIdx.x;
    if (w >= z.W) {                                        // (uniform: a whole block)
        const int b = (w - z.W) * kMaxRows + lane;
        if (b < z.B) exchange_no_world(z, in, out, b);
        return;
    }
    const int nw = clampi(in.n_world[w], 0, z.max_world);
    if (lane < nw) {                                       // nw <= max_world <= 64: the slot exists
        const double* st = agent_state + 6 * ((size_t)w * z.max_world + lane);
        const agt::Obs o = agt::observe(st[2], st[3], st[5]);
        rows[4 * lane] = st[0]; rows[4 * lane + 1] = st[1]; rows[4 * lane + 2] = o.wx; rows[4 * lane + 3] = o.wy;
    }
    __syncthreads();
    exchange_world(z, in, out, w, Wave64{}, DeviceRows{rows, in.ego_state});
}

}  // namespace wx
}  // namespace emp
