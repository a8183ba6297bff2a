// emp_route_kernels.h - route_kernel: one routing query per wavefront (a block of 64 lanes), the search state of its N nodes in
// LDS.  The procedure is emp_route_core.h's, compiled here with the 64-lane collectives below; the graph's arrays are read-only and
// shared by every query of the launch, so they stay in cache.
#pragma once

#include <hip/hip_runtime.h>

#include "emp_route_core.h"

namespace emp {
namespace route {

// The lanes of a block of exactly 64 threads.  sync() is the block's barrier: every lane of the wavefront reaches it together
// (emp_route_core.h keeps control flow uniform), and it orders the lanes' LDS and global stores before the loads behind it.
struct Wave64 {
    static constexpr int kLanes = 64;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void argmin(double& f, int& key, int& idx) const {
        for (int off = 32; off; off >>= 1) {
            const double of = __shfl_xor(f, off);
            const int ok = __shfl_xor(key, off), oi = __shfl_xor(idx, off);
            if (before(of, ok, oi, f, key, idx)) {
                f = of;
                key = ok;
                idx = oi;
            }
        }
        // keys are distinct among candidates, so every lane holds the same winner already; lane 0's copy makes that unconditional
        f = __shfl(f, 0);
        key = __shfl(key, 0);
        idx = __shfl(idx, 0);
    }
    __device__ __forceinline__ int prefix(bool flag, int* total) const {
        const unsigned long long mask = __ballot(flag);
        *total = __popcll(mask);
        return __popcll(mask & ((1ull << threadIdx.x) - 1ull));
    }
    __device__ __forceinline__ bool any(bool flag) const { return __ballot(flag) != 0ull; }
};

// origin_wp == nullptr: A* only (wp_index, global_path, n_global unused).  The outputs are zero on entry.
__global__ __launch_bounds__(64) void route_kernel(Graph G, int B, int max_route, int max_global, const int* __restrict__ start_node,
                                                   const int* __restrict__ end_edge, const double* __restrict__ origin_wp,
                                                   const double* __restrict__ dest_wp, int* route, int* route_len, int* wp_index,
                                                   double* global_path, int* n_global, int* status) {
    extern __shared__ double route_lds[];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    const StateLds<char*> L = state_lds((char*)route_lds, G.n_nodes);
    const State S = {(double*)L.h, (int*)L.g, (int*)L.parent, (int*)L.stamp, (int*)L.state};
    Query q = {start_node[b], end_edge[b], nullptr, nullptr};
    Result r = {route + (size_t)b * max_route, max_route, {nullptr, nullptr, max_global}, 0, 0, 0};
    if (origin_wp) {
        q.origin_wp = origin_wp + 3 * (size_t)b;
        q.dest_wp = dest_wp + 3 * (size_t)b;
        r.path.wp_index = wp_index + (size_t)b * max_global;
        r.path.global_path = global_path + (size_t)b * max_global * 4;
    }
    run_query(G, S, q, r, Wave64{});
    if (threadIdx.x == 0) {
        route_len[b] = r.route_len;
        status[b] = r.status;
        if (origin_wp) n_global[b] = r.n_global;
    }
}

}  // namespace route
}  // namespace emp
