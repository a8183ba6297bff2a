// emp_api.hip - C-ABI of the MI355X EM-Planner hot path (see include/emplanner.h).
// One translation unit: kernels are header-only templates, this file owns launches and staging.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <tuple>

#include "emp_context.h"
#ifndef EMP_QP_LDS_PAD
#define EMP_QP_LDS_PAD 0       // development: the same for a path-QP wavefront
#endif
#ifndef EMP_EDGE_LDS_PAD
#define EMP_EDGE_LDS_PAD 0     // development: extra (unused) dynamic LDS per edge-cost block, to measure what LDS room is worth
#endif
#include "emp_dp_kernels.h"
#include "emp_st_kernels.h"
#include "emp_st_backend_kernels.h"
#include "emp_tail_kernels.h"
#include "emp_mpc_kernels.h"
#include "emp_rollout_kernels.h"
#include "emp_speed_front_kernels.h"
#include "emp_drive_kernels.h"
#include "emp_route_kernels.h"
#include "emp_route_launch.h"
#include "emp_agent_kernels.h"
#include "emp_behavior_kernels.h"
#include "emp_hazard_kernels.h"
#include "emp_world_kernels.h"

namespace emp {
thread_local std::string g_create_error;

// Asked by every launch of this file before it is issued: none while the call's Stage still takes inputs (packed inputs may not
// have been sent yet - emp_context.h Stage::ready()).
static int launch_gate(emp_ctx* ctx) {
    if (ctx->stage_open) return fail(ctx, EMP_ERR_INVALID, "internal: kernel launch before Stage::ready() (packed inputs may be unsent)");
    return EMP_OK;
}

// A plain launch on the context's stream: nothing for an empty grid; timed under `name` unless that is null.
template <typename K, typename... A>
static int launch(emp_ctx* ctx, const char* name, K kern, dim3 grid, dim3 block, size_t lds, A... args) {
    if ((size_t)grid.x * grid.y * grid.z == 0) return EMP_OK;
    if (const int rc = launch_gate(ctx)) return rc;
    KernelTimer t(ctx, name);
    hipLaunchKernelGGL(kern, grid, block, lds, ctx->stream, args...);
    EMP_LAUNCH_CHECK(ctx);
    return EMP_OK;
}

// Dynamic LDS of a kernel: refused with the caller's own text beyond a compute unit's 160 KB, opted in beyond the default 48 KB.
template <typename K>
static int set_lds(emp_ctx* ctx, K kernel, size_t bytes, const char* too_large) {
    EMP_REQUIRE(ctx, bytes <= 160 * 1024, too_large);
    if (bytes > 48 * 1024)
        EMP_HIP(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return EMP_OK;
}

// The scheduling of one emp_plan_cycle call between its launchers (stand-alone entry points pass nullptr: none of it).
struct CycleSched {
    // STAGED: the event the front stage's LAST kernel (the sweep) is asked to signal when it completes (hipExtLaunchKernelGGL's
    // stop event: no marker packet behind the kernel); the sweep's launcher reports the event it did attach - its own timing
    // event when the kernel is being timed, else front_stop
    hipEvent_t front_stop = nullptr, front_attached = nullptr;
    // what the next sweep (EMP_OPT_SWEEP_EXCLUSIVE: the previous call's back stage) and the next edge-cost launch
    // (EMP_OPT_EDGE_AFTER_ENRICH) wait for on their stream; each is consumed by the launch that waits
    hipEvent_t sweep_wait = nullptr, edge_wait = nullptr;
    // The planning cycle leaves the DP backtrack to the densification kernel (dp_sweep_kernel, BT == false): the caller offers
    // the two buffers, the sweep's launcher sets bt_deferred when it used them (compiled row counts only).
    unsigned char* bt_pre = nullptr;
    int* bt_term = nullptr;
    bool bt_deferred = false;
    // STAGED: an event the next densification / path-QP launch is asked to signal from its own dispatch (hipExtLaunchKernelGGL's
    // stop event) instead of a marker packet behind it - a marker idles the back queue ~6 us, twice per step; `stop_attached`
    // says whether the launcher did (it does not while the kernel carries timing events)
    hipEvent_t attach_stop = nullptr;
    bool stop_attached = false;
};

static int make_dp_dev(emp_ctx* ctx, const emp_dp_params* p, int B, int max_obs, DpDev* d) {
    EMP_REQUIRE(ctx, p != nullptr, "dp params are NULL");
    EMP_REQUIRE(ctx, p->row >= 1 && p->row <= kMaxWideRow, "row must be in [1, 1024]");
    EMP_REQUIRE(ctx, p->col >= 1 && p->col <= 255 * 16, "col must be in [1, 4080]");
    EMP_REQUIRE(ctx, B >= 0, "negative batch");
    EMP_REQUIRE(ctx, max_obs >= 0 && max_obs <= 256, "max_obs must be in [0, 256]");
    EMP_REQUIRE(ctx, p->sample_s > 0 && p->sample_l > 0 && p->sampling_res > 0, "sample_s, sample_l, sampling_res must be > 0");
    d->row = p->row;
    d->col = p->col;
    d->S = dp_tiling(p->row, B).S;
    d->tiles = dp_tiling(p->row, B).tiles;
    d->B = B;
    d->max_obs = max_obs > 0 ? max_obs : 1;
    d->sample_s = p->sample_s;
    d->sample_l = p->sample_l;
    d->res = p->sampling_res;
    d->w_coll = p->w_collision;
    d->w0 = p->w_smooth[0];
    d->w1 = p->w_smooth[1];
    d->w2 = p->w_smooth[2];
    d->w_ref = p->w_ref;
    return EMP_OK;
}

// elements of the edge tensor the DP kernels exchange between themselves: tiled up to 32 rows, canonical beyond (emp_dp_launch.h)
static size_t tiled_elems(const DpDev& d) { return edge_tensor_elems(d.row, d.col, d.B, true); }
// a plan emp_dp_launch.h or emp_tail_launch.h refused, as the call's error
static int plan_refused(emp_ctx* ctx, const char* error) { return error ? fail(ctx, EMP_ERR_INVALID, error) : EMP_OK; }
// A kernel launched as emp_tail_launch.h plans it: refused with the plan's text, else opted in to its LDS and launched on its grid.
template <typename K, typename... A>
static int launch_plan(emp_ctx* ctx, const char* name, const TailPlan& p, K kern, A... args) {
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    if (const int rc = set_lds(ctx, kern, p.lds, "internal: a launch plan beyond the LDS")) return rc;
    return launch(ctx, name, kern, dim3(p.grid, p.grid_y), dim3(p.block), p.lds, args...);
}

// ---- device-level stage launchers (all pointers are device memory; nothing synchronises) -----
// pair table of the lattice (emp_dp_kernels.h dp_pair_table_kernel): rebuilt only when the lattice parameters change,
// stream-ordered before its first use
static int dp_pair_table(emp_ctx* ctx, const DpDev& d, const double** out) {
    const double key[8] = {(double)d.row, d.sample_s, d.sample_l, d.w0, d.w1, d.w_ref, d.w2, 0.0};
    const size_t tab_bytes = ((size_t)kTableFields * d.row * d.row + kTableTail) * sizeof(double);
    emp_ctx::PairTable& pt = ctx->pair_tables[ctx->active_lane];
    emp_ctx::Buf& tb = pt.buf;
    if (tb.bytes < tab_bytes) {
        const int grc = grow_buffer(ctx, tb, tab_bytes);
        if (grc) return grc;
        pt.valid = false;
    }
    if (!pt.valid || memcmp(key, pt.key, sizeof(key)) != 0) {
        if (const int rc = launch(ctx, nullptr, dp_pair_table_kernel, dim3(1), dim3(256), 0, d, (double*)tb.p)) return rc;
        ++ctx->alloc_gen;                 // (a captured cycle graph does not carry this launch: EMP_OPT_CYCLE_GRAPH)
        memcpy(pt.key, key, sizeof(key));
        pt.valid = true;
    }
    *out = (const double*)tb.p;
    return EMP_OK;
}

// The tiled edge-cost kernels of one layout and mask width, by the plan's row_inst
struct EdgeKernels {
    decltype(&dp_edge_ring_kernel<true>) ring;
    decltype(&dp_edge_kernel<true>) lockstep;
};
template <bool TILED, typename MASK>
static EdgeKernels edge_kernels(int row_inst) {
    switch (row_inst) {
        case 5: return {dp_edge_ring_kernel<TILED, 5, MASK>, dp_edge_kernel<TILED, 5, MASK>};
        case 9: return {dp_edge_ring_kernel<TILED, 9, MASK>, dp_edge_kernel<TILED, 9, MASK>};
        case 12: return {dp_edge_ring_kernel<TILED, 12, MASK>, dp_edge_kernel<TILED, 12, MASK>};
        case 21: return {dp_edge_ring_kernel<TILED, 21, MASK>, dp_edge_kernel<TILED, 21, MASK>};
        default: return {dp_edge_ring_kernel<TILED, 0, MASK>, dp_edge_kernel<TILED, 0, MASK>};
    }
}

// Edge costs: plan (emp_dp_launch.h plan_edge), pick the kernel, wait, one launch, signal.
static int dev_dp_edge(emp_ctx* ctx, const DpDev& d, const double* obs_s, const double* obs_l, const int* n_obs,
                       const double* start, double* start_cost, double* edge, bool tiled, CycleSched* cs) {
    if (d.B == 0) return EMP_OK;
    const EdgePlan p = plan_edge(d, tiled, ctx->opt[EMP_OPT_EDGE_FORM], ctx->opt[EMP_OPT_EDGE_BLOCK], EMP_EDGE_LDS_PAD);
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    const dim3 grid(p.grid_x, p.grid_y), block(p.block);
    const double* pair_tab = nullptr;
    if (const int rc = dp_pair_table(ctx, d, &pair_tab)) return rc;
    if (p.wide)
        return launch(ctx, "dp_edge", dp_edge_wide_kernel, grid, block, 0, d, pair_tab, obs_s, obs_l, n_obs, start, start_cost, edge);
    using M32 = unsigned int;
    using M64 = unsigned long long;
    const EdgeKernels k = tiled ? (p.m32 ? edge_kernels<true, M32>(p.row_inst) : edge_kernels<true, M64>(p.row_inst))
                                : (p.m32 ? edge_kernels<false, M32>(p.row_inst) : edge_kernels<false, M64>(p.row_inst));
    if (const int rc = p.ring ? set_lds(ctx, k.ring, p.lds, "edge-cost block too large for the LDS")
                              : set_lds(ctx, k.lockstep, p.lds, "edge-cost block too large for the LDS"))
        return rc;
    // EMP_OPT_EDGE_AFTER_ENRICH (staged pipeline): the edge kernel starts behind the previous call's densification kernel,
    // so that the path QP that follows it on the back queue is dispatched BEFORE this kernel's sixteen-wavefront blocks
    // take the compute units (emp_plan_cycle)
    if (cs && cs->edge_wait) {
        EMP_HIP(ctx, hipStreamWaitEvent(ctx->stream, cs->edge_wait, 0));
        cs->edge_wait = nullptr;
    }
    // EMP_OPT_EDGE_CLOCK_PROBE (measurement, ring form): two reference ticks per wavefront of this launch
    const bool probed = p.ring && ctx->opt[EMP_OPT_EDGE_CLOCK_PROBE];
    if (probed) {
        const size_t waves_total = (size_t)grid.x * grid.y * p.wpb;
        const int grc = grow_buffer(ctx, ctx->edge_probe, waves_total * 4 * sizeof(unsigned long long));
        if (grc) return grc;
        if (const int rc = ctx->edge_probe_done.ensure(ctx, hipEventDisableTiming)) return rc;
        ctx->edge_probe_waves = (long)waves_total;
    }
    // EMP_OPT_LANE_EDGE_ORDER (lane mode): this edge kernel starts when the previous call's, on another lane, is done - the
    // lanes' FP64-bound kernels take turns instead of running two or three at a time, and the HBM-bound sweep behind each of them
    // has one of them beside it, not two (measured: include/emplanner.h).  Pure ordering: results do not depend on it.
    // A probed launch takes no part in it: neither the wait nor the record.
    const int leo = ctx->opt[EMP_OPT_LANE_EDGE_ORDER];
    const bool ordered = !probed && ctx->pipe_mode >= 2 && ctx->active_lane >= 0 && (leo == 1 || (leo == 2 && d.B >= 8192));
    if (ordered && ctx->lane_edge_done) EMP_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->lane_edge_done, 0));
    if (const int rc = launch_gate(ctx)) return rc;
    {
        KernelTimer t(ctx, "dp_edge");       // (open until the lane's event is recorded)
        if (p.ring) {
            hipLaunchKernelGGL(k.ring, grid, block, p.lds, ctx->stream, d, pair_tab, obs_s, obs_l, n_obs, start, start_cost, edge,
                               p.cols_per_chunk, probed ? (unsigned long long*)ctx->edge_probe.p : nullptr);
        } else {
            hipLaunchKernelGGL(k.lockstep, grid, block, p.lds, ctx->stream, d, pair_tab, obs_s, obs_l, n_obs, start, start_cost, edge,
                               p.cols_per_chunk);
        }
        EMP_LAUNCH_CHECK(ctx);
        if (ordered) {
            emp_ctx::Lane& ln = ctx->lanes[ctx->active_lane];
            if (const int rc = ln.ev_edge.ensure(ctx, hipEventDisableTiming)) return rc;
            ctx->lane_edge_done = ln.ev_edge;
            EMP_HIP(ctx, hipEventRecord(ctx->lane_edge_done, ctx->stream));
        }
    }
    if (probed) EMP_HIP(ctx, hipEventRecord(ctx->edge_probe_done, ctx->stream));      // behind the kernel (and its timing event)
    return EMP_OK;
}

// What a sweep launch carries besides its plan: the dispatch's events and dp_sweep_kernel's arguments.
struct SweepCall {
    hipEvent_t start, stop;
    bool defer;       // the backtrack is left to the densification kernel (BT == false), which reads bt_pre / bt_term
    const DpDev& d;
    const double *start_cost, *edge;
    const int* n_obs;
    double *rows, *min_cost;
    int* status;
    unsigned char* bt_pre;
    int* bt_term;
    unsigned long long* probe;
};

// The one launch of dp_sweep_kernel<R, PD, 1, NT, BT>.  A stream capture records plain launches only; otherwise the dispatch
// itself stamps c.start and signals c.stop (hipExtLaunchKernelGGL: no marker packets around the roofline kernel).
template <int R, int PD, bool NT>
static int launch_sweep(emp_ctx* ctx, const SweepPlan& p, const SweepCall& c) {
    if (p.row_inst != R || p.pd != PD || p.nt != NT) return fail(ctx, EMP_ERR_INVALID, "internal: sweep instantiation differs from its plan");
    const auto kern = c.defer ? dp_sweep_kernel<R, PD, 1, NT, false> : dp_sweep_kernel<R, PD, 1, NT, true>;
    if (const int rc = set_lds(ctx, kern, p.lds, "too many columns for the predecessor table in LDS")) return rc;
    if (const int rc = launch_gate(ctx)) return rc;
    if (ctx->cycle_graph.capturing) {
        hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.block), p.lds, ctx->stream, c.d, c.start_cost, c.edge, c.n_obs, c.rows, c.min_cost,
                           c.status, c.bt_pre, c.bt_term, c.probe);
    } else {
        hipExtLaunchKernelGGL(kern, dim3(p.grid), dim3(p.block), p.lds, ctx->stream, c.start, c.stop, 0, c.d, c.start_cost, c.edge, c.n_obs,
                              c.rows, c.min_cost, c.status, c.bt_pre, c.bt_term, c.probe);
    }
    return EMP_OK;
}

static int dev_dp_sweep(emp_ctx* ctx, const DpDev& d, const double* start_cost, const double* edge,
                        const int* n_obs, double* rows, double* min_cost, int* status, CycleSched* cs) {
    if (d.B == 0) return EMP_OK;
    const SweepPlan p = plan_sweep(d);
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    if (dp_wide(d)) {          // more than 32 rows: one block per scene, predecessors in device memory
        emp_ctx::Buf& pre = ctx->named["dp_wide_pre_" + std::to_string(ctx->active_lane)];
        const int grc = grow_buffer(ctx, pre, (size_t)d.B * d.col * d.row * sizeof(unsigned short));
        if (grc) return grc;
        return launch(ctx, "dp_sweep", dp_sweep_wide_kernel, dim3(p.grid), dim3(p.block), p.lds, d, start_cost, edge, n_obs,
                      (unsigned short*)pre.p, rows, min_cost, status);
    }
    // EMP_OPT_SWEEP_EXCLUSIVE (staged pipeline): the sweep starts once the previous call's back stage is done
    if (cs && cs->sweep_wait) {
        EMP_HIP(ctx, hipStreamWaitEvent(ctx->stream, cs->sweep_wait, 0));
        cs->sweep_wait = nullptr;
    }
    // EMP_OPT_SWEEP_CLOCK_PROBE: four ticks per wavefront (emp_dp_kernels.h), read by emp_sweep_clock_mhz
    unsigned long long* probe = nullptr;
    if (ctx->opt[EMP_OPT_SWEEP_CLOCK_PROBE]) {
        if (ctx->clock_probe_tiles != d.tiles) ctx->probe_launches = 0;       // another batch size: the ring starts over
        const int grc = grow_buffer(ctx, ctx->clock_probe, (size_t)emp_ctx::kProbeSlots * d.tiles * 4 * sizeof(unsigned long long));
        if (grc) return grc;
        probe = (unsigned long long*)ctx->clock_probe.p + (size_t)(ctx->probe_launches % emp_ctx::kProbeSlots) * d.tiles * 4;
        ctx->clock_probe_tiles = d.tiles;
        ctx->probe_launches++;
    }
    KernelTimer t(ctx, "dp_sweep", true);   // the roofline kernel: events stamped by the dispatch itself
    const hipEvent_t stop_ev = t.stop ? t.stop : cs ? cs->front_stop : nullptr;
    // the caller's two buffers are used by the compiled row counts only
    const bool defer = p.row_inst > 0 && cs && cs->bt_pre && cs->bt_term;
    const SweepCall c{t.start, stop_ev, defer, d, start_cost, edge, n_obs, rows, min_cost, status,
                      defer ? cs->bt_pre : nullptr, defer ? cs->bt_term : nullptr, probe};
    int lrc;
    switch (p.row_inst) {          // the plan's (row_inst, pd, nt) become template arguments here
        case 5: lrc = p.nt ? launch_sweep<5, 2, true>(ctx, p, c) : launch_sweep<5, 2, false>(ctx, p, c); break;
        case 9: lrc = p.nt ? launch_sweep<9, 2, true>(ctx, p, c) : launch_sweep<9, 3, false>(ctx, p, c); break;
        case 12: lrc = p.nt ? launch_sweep<12, 2, true>(ctx, p, c) : launch_sweep<12, 2, false>(ctx, p, c); break;
        case 21: lrc = p.nt ? launch_sweep<21, 3, true>(ctx, p, c) : launch_sweep<21, 3, false>(ctx, p, c); break;
        default: lrc = launch_sweep<0, 1, false>(ctx, p, c); break;
    }
    if (lrc) return lrc;
    if (cs) {
        cs->front_attached = stop_ev;
        cs->bt_deferred = defer;
    }
    EMP_LAUNCH_CHECK(ctx);
    if (probe) {
        if (const int rc = ctx->clock_probe_done.ensure(ctx, hipEventDisableTiming)) return rc;
        EMP_HIP(ctx, hipEventRecord(ctx->clock_probe_done, ctx->stream));
    }
    return EMP_OK;
}

// A launch that signals cs->attach_stop from its own dispatch when the caller offered one and the kernel carries no timing
// events (CycleSched); else a plain launch.
template <typename K, typename... A>
static int launch_attaching(emp_ctx* ctx, CycleSched* cs, bool timed, K kern, dim3 grid, dim3 block, size_t lds, A... args) {
    if (const int rc = launch_gate(ctx)) return rc;
    if (cs && cs->attach_stop && !timed) {
        hipExtLaunchKernelGGL(kern, grid, block, lds, ctx->stream, nullptr, cs->attach_stop, 0, args...);
        cs->stop_attached = true;
    } else {
        hipLaunchKernelGGL(kern, grid, block, lds, ctx->stream, args...);
    }
    EMP_LAUNCH_CHECK(ctx);
    return EMP_OK;
}

static int dev_dp_enrich(emp_ctx* ctx, const DpDev& d, const double* rows, const double* start, int max_pts,
                         double* path_s, double* path_l, int* path_len, int* status, int or_status, CycleSched* cs,
                         const unsigned char* pre = nullptr, const int* term = nullptr, const int* n_obs = nullptr,
                         double* rows_out = nullptr) {
    if (d.B == 0) return EMP_OK;
    const EnrichPlan p = plan_enrich(d, pre != nullptr);
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    if (const int rc = set_lds(ctx, dp_enrich_wave_kernel, p.lds, "too many columns for the densification kernel's predecessor table in LDS")) return rc;
    KernelTimer t(ctx, "dp_enrich");
    return launch_attaching(ctx, cs, t.stop != nullptr, dp_enrich_wave_kernel, dim3(d.B), dim3(64), p.lds, d, rows, start, max_pts, path_s,
                            path_l, path_len, status, or_status, pre, term, n_obs, rows_out);
}

// DP_algorithm up to the backtrack.  `edge_scratch` may be NULL: taken from the named scratch.
// The edge tensor (and the start costs behind it) of the current call.  One per stream that runs DP kernels (the main
// stream, and every lane in LANES mode): the sweep of one call may still read its tensor while the edge kernel of the
// next call, on another lane, writes its own.
static int dp_edge_tensor(emp_ctx* ctx, const DpDev& d, double** edge, double** start_cost) {
    const size_t need = (tiled_elems(d) + (size_t)d.B * d.row) * sizeof(double);
    emp_ctx::Buf& sc = ctx->named["dp_edge_tensor_" + std::to_string(ctx->active_lane)];
    const int grc = grow_buffer(ctx, sc, need);
    if (grc) return grc;
    *edge = (double*)sc.p;
    *start_cost = *edge + tiled_elems(d);
    return EMP_OK;
}

// EMP_DP_FUSED: one kernel, edge costs staged in LDS and swept in place (emp_dp_kernels.h dp_fused_kernel)
static int dev_dp_fused(emp_ctx* ctx, const DpDev& d, const double* obs_s, const double* obs_l, const int* n_obs,
                        const double* start, double* rows, double* min_cost, int* status) {
    if (d.B == 0) return EMP_OK;
    const FusedPlan p = plan_fused(d);
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    const double* pair_tab = nullptr;
    if (const int rc = dp_pair_table(ctx, d, &pair_tab)) return rc;
    const int r = dp_row_inst(d.row);
    const auto kern = r == 5 ? dp_fused_kernel<5> : r == 9 ? dp_fused_kernel<9> : r == 12 ? dp_fused_kernel<12> : r == 21 ? dp_fused_kernel<21> : dp_fused_kernel<0>;
    KernelTimer t(ctx, "dp_fused");
    if (const int rc = set_lds(ctx, kern, p.lds, "lattice too wide for the fused DP kernel's LDS working set")) return rc;
    if (const int rc = launch_gate(ctx)) return rc;
    hipLaunchKernelGGL(kern, dim3(d.tiles), dim3(256), p.lds, ctx->stream, d, pair_tab, obs_s, obs_l, n_obs, start, rows, min_cost, status, p.nc);
    EMP_LAUNCH_CHECK(ctx);
    return EMP_OK;
}

// DP_algorithm up to the backtrack, in either form.
static int dev_dp_plan(emp_ctx* ctx, const DpDev& d, const double* obs_s, const double* obs_l, const int* n_obs,
                       const double* start, emp_dp_mode mode, double* rows, double* min_cost, int* status, CycleSched* cs) {
    if (d.B == 0) return EMP_OK;
    // the single-kernel form lives on the tiled layout: lattices wider than 32 rows take the two-kernel form either way
    if (mode == EMP_DP_FUSED && !dp_wide(d)) return dev_dp_fused(ctx, d, obs_s, obs_l, n_obs, start, rows, min_cost, status);
    double *edge, *start_cost;
    int rc = dp_edge_tensor(ctx, d, &edge, &start_cost);
    if (rc) return rc;
    if ((rc = dev_dp_edge(ctx, d, obs_s, obs_l, n_obs, start, start_cost, edge, true, cs))) return rc;
    return dev_dp_sweep(ctx, d, start_cost, edge, n_obs, rows, min_cost, status, cs);
}

}  // namespace emp

using namespace emp;

// The preamble of a staged entry point, behind its argument checks: the context's device, then the call's Stage.
#define EMP_STAGE(st, ...)                       \
    EMP_HIP(ctx, hipSetDevice(ctx->device));    \
    Stage st(ctx, __VA_ARGS__)

// A launch on the stream that carries a record-packing call (the main stream, or the result stream of the pipelined cycle),
// with its timing events there.
template <typename K, typename... A>
static int launch_on(emp_ctx* ctx, hipStream_t stream, const char* name, K kern, dim3 grid, dim3 block, A... args) {
    const hipStream_t saved = ctx->stream;
    ctx->stream = stream;
    const int rc = launch(ctx, name, kern, grid, block, 0, args...);
    ctx->stream = saved;
    return rc;
}

extern "C" {

int emp_abi_version(void) { return EMP_ABI_VERSION; }

void emp_dp_params_default(emp_dp_params* p) {
    // ref: path_planning.py:276-279
    p->row = 12;
    p->col = 6;
    p->sample_s = 15.0;
    p->sample_l = 1.5;
    p->sampling_res = 2.0;
    p->w_collision = 1e12;
    p->w_smooth[0] = 300.0;
    p->w_smooth[1] = 1000.0;
    p->w_smooth[2] = 5000.0;
    p->w_ref = 20.0;
}

void emp_qp_params_default(emp_qp_params* q) {
    // ref: path_planning.py:78-81, test_9.py:187-192
    q->ds = 2.0;
    q->w_l = 1000.0;
    q->w_dl = 10000.0;
    q->w_ddl = 3000.0;
    q->w_dddl = 150.0;
    q->w_centre = 250.0;
    q->w_end_l = q->w_end_dl = q->w_end_ddl = 40.0;
    q->host_d1 = q->host_d2 = q->host_w = 3.0;
    q->obs_length = q->obs_width = 5.0;
    q->decimate = 2;
    q->midpoint = 1;
    q->use_qp = 1;
    q->reserved = 0;
}

void emp_smooth_params_default(emp_smooth_params* s) {
    // ref: planning_utils.py:262-264
    s->w_smooth = 0.4;
    s->w_length = 0.3;
    s->w_ref = 0.3;
    s->x_thre = 0.2;
    s->y_thre = 0.2;
}

int emp_create(int device_id, emp_ctx** out) {
    if (!out) return fail(nullptr, EMP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, EMP_ERR_NO_DEVICE,
                    std::string("no HIP device visible: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0"));
    if (device_id < 0 || device_id >= n) return fail(nullptr, EMP_ERR_INVALID, "device_id out of range");
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(nullptr, EMP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return fail(nullptr, EMP_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, EMP_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    emp_ctx* c = new emp_ctx();
    c->device = device_id;
    c->cu_count = prop.multiProcessorCount;
    if (const int rc = c->main_stream.ensure(nullptr, hipStreamNonBlocking)) {
        delete c;
        return rc;
    }
    c->stream = c->main_stream;
    *out = c;
    return EMP_OK;
}

void emp_destroy(emp_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)sync_all(ctx);        // the owners release without synchronising
    delete ctx;
}

const char* emp_last_error(const emp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int emp_synchronize(emp_ctx* ctx) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_HIP(ctx, (hipError_t)sync_all(ctx));
    return EMP_OK;
}

void* emp_stream(emp_ctx* ctx) { return ctx ? (void*)ctx->main_stream : nullptr; }

void* emp_result_stream(emp_ctx* ctx) {
    if (!ctx) return nullptr;
    return (void*)ctx->result_stream();
}

// one thread per record slot; consecutive threads write consecutive doubles
__global__ __launch_bounds__(256) void pack_records_kernel(int B, int col, int max_pts, int cap, const int* __restrict__ status,
                                                           const int* __restrict__ traj_len,
                                                           const int* __restrict__ path_len,
                                                           const double* __restrict__ dp_rows,
                                                           const double* __restrict__ path_s,
                                                           const double* __restrict__ path_l,
                                                           const double* __restrict__ traj, double* __restrict__ rec) {
    const int width = 3 + col + 2 * cap + 4 * (cap + 1);
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * width) return;
    const int b = (int)(idx / width);
    int c = (int)(idx - (size_t)b * width);
    double v;
    if (c < 3) {
        v = (double)(c == 0 ? status[b] : c == 1 ? traj_len[b] : path_len[b]);
    } else if ((c -= 3) < col) {
        v = dp_rows[(size_t)b * col + c];
    } else if ((c -= col) < cap) {
        v = path_s[(size_t)b * max_pts + c];
    } else if ((c -= cap) < cap) {
        v = path_l[(size_t)b * max_pts + c];
    } else {
        v = traj[(size_t)b * (max_pts + 1) * 4 + (c - cap)];
    }
    rec[idx] = v;
}

int emp_pack_records(emp_ctx* ctx, int32_t B, int32_t col, int32_t max_pts, int32_t path_cap, const int32_t* status,
                     const int32_t* traj_len, const int32_t* path_len, const double* dp_rows, const double* path_s,
                     const double* path_l, const double* traj, double* rec, int on_result_stream, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && col >= 1 && max_pts >= 1 && path_cap >= 1 && path_cap <= max_pts, "bad sizes");
    EMP_REQUIRE(ctx, status && traj_len && path_len && dp_rows && path_s && path_l && traj && rec, "NULL array");
    const bool on_rs = on_result_stream && ctx->pipelined() && where == EMP_DEVICE;
    EMP_STAGE(st, where, on_rs);             // on the result stream the launch is ordered behind the cycle by the stream itself
    const size_t width = 3 + (size_t)col + 2 * (size_t)path_cap + 4 * ((size_t)path_cap + 1);
    const int* d_st = st.in(status, (size_t)B);
    const int* d_tl = st.in(traj_len, (size_t)B);
    const int* d_pl = st.in(path_len, (size_t)B);
    const double* d_rows = st.in(dp_rows, (size_t)B * col);
    const double* d_ps = st.in(path_s, (size_t)B * max_pts);
    const double* d_pll = st.in(path_l, (size_t)B * max_pts);
    const double* d_traj = st.in(traj, (size_t)B * (max_pts + 1) * 4);
    // the kernel writes every slot of rec: no zero fill (it would be queued on ctx->stream, unordered with a launch on
    // the result stream)
    double* d_rec = st.out(rec, (size_t)B * width, false);
    if (const int rc = st.ready()) return rc;
    const size_t total = (size_t)B * width;
    if (const int rc = launch_on(ctx, on_rs ? ctx->result_stream() : ctx->stream, "pack_records", pack_records_kernel,
                                 dim3((unsigned)((total + 255) / 256)), dim3(256), B, col, max_pts, path_cap, d_st, d_tl, d_pl, d_rows,
                                 d_ps, d_pll, d_traj, d_rec))
        return rc;
    return st.finish();
}

// trajectory-only record: status, traj_len, traj [cap + 1][4]
__global__ __launch_bounds__(256) void pack_trajectory_records_kernel(int B, int max_pts, int cap, const int* __restrict__ status,
                                                                      const int* __restrict__ traj_len,
                                                                      const double* __restrict__ traj,
                                                                      double* __restrict__ rec) {
    const int width = 2 + 4 * (cap + 1);
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * width) return;
    const int b = (int)(idx / width);
    const int c = (int)(idx - (size_t)b * width);
    rec[idx] = c == 0 ? (double)status[b] : c == 1 ? (double)traj_len[b] : traj[(size_t)b * (max_pts + 1) * 4 + (c - 2)];
}

int emp_pack_trajectory_records(emp_ctx* ctx, int32_t B, int32_t max_pts, int32_t path_cap, const int32_t* status,
                                const int32_t* traj_len, const double* traj, double* rec, int on_result_stream,
                                emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_pts >= 1 && path_cap >= 1 && path_cap <= max_pts, "bad sizes");
    EMP_REQUIRE(ctx, status && traj_len && traj && rec, "NULL array");
    const bool on_rs = on_result_stream && ctx->pipelined() && where == EMP_DEVICE;
    EMP_STAGE(st, where, on_rs);
    const size_t width = 2 + 4 * ((size_t)path_cap + 1);
    const int* d_st = st.in(status, (size_t)B);
    const int* d_tl = st.in(traj_len, (size_t)B);
    const double* d_traj = st.in(traj, (size_t)B * (max_pts + 1) * 4);
    double* d_rec = st.out(rec, (size_t)B * width, false);      // every slot is written by the kernel
    if (const int rc = st.ready()) return rc;
    const size_t total = (size_t)B * width;
    if (const int rc = launch_on(ctx, on_rs ? ctx->result_stream() : ctx->stream, "pack_records", pack_trajectory_records_kernel,
                                 dim3((unsigned)((total + 255) / 256)), dim3(256), B, max_pts, path_cap, d_st, d_tl, d_traj, d_rec))
        return rc;
    return st.finish();
}

int emp_set_pipeline(emp_ctx* ctx, int mode) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, mode <= EMP_PIPELINE_MAX && mode >= EMP_PIPELINE_AUTO, "mode: EMP_PIPELINE_AUTO, 0, EMP_PIPELINE_STAGED or 2..EMP_PIPELINE_MAX lanes");
    EMP_HIP(ctx, hipSetDevice(ctx->device));
    EMP_HIP(ctx, (hipError_t)sync_all(ctx));
    if (mode == EMP_PIPELINE_AUTO) {
        // Three lanes are the fastest form - when every stream of the process has a hardware queue of its own.  The HIP runtime
        // maps all streams onto GPU_MAX_HW_QUEUES queues (default 4), read once when it initialised: three lane streams, the main
        // stream, the copy / d2h streams of the page-locked path if this context has them, and the streams the REST of the
        // process brings (EMP_OPT_FOREIGN_STREAMS: the caller's own, a gather stream, RCCL's) must fit - otherwise lanes share
        // queues, serialise and run slower than the staged form, which needs two.  (The one environment variable the library reads:
        // it is the only place the queue count can be had from.)
        const char* env = getenv("GPU_MAX_HW_QUEUES");
        int queues = env ? atoi(env) : 4;
        if (queues < 1) queues = 4;
        const int owned = 1 + (ctx->copy_stream ? 1 : 0) + (ctx->d2h_stream ? 1 : 0);
        const int foreign = ctx->opt[EMP_OPT_FOREIGN_STREAMS];
        mode = (queues >= 3 + owned + foreign) ? 3 : EMP_PIPELINE_STAGED;
        ctx->auto_queues = queues;
        ctx->auto_streams = owned + foreign;
    }
    const int m = mode;
    const int need = m == EMP_PIPELINE_STAGED ? emp_ctx::kStagedPools : m;
    // Streams the new mode does not use go away (everything was drained above): a stream holds a share of one of the process's
    // few hardware queues, and a staged pipeline set up while three lane streams of an earlier mode were still alive found its
    // front and back stage on one queue - 0.43 ms a step instead of 0.22 (bench.py's staged legs behind the three-lane headline)
    for (size_t i = 0; i < ctx->lanes.size(); ++i)
        if (m == EMP_PIPELINE_STAGED || (int)i >= m) EMP_HIP(ctx, ctx->lanes[i].stream.reset());
    if (m != EMP_PIPELINE_STAGED) EMP_HIP(ctx, ctx->back_stream.reset());
    if ((int)ctx->lanes.size() < need) ctx->lanes.resize(need);
    for (int i = 0; i < need; ++i) {
        emp_ctx::Lane& ln = ctx->lanes[i];
        int rc = EMP_OK;
        if (m != EMP_PIPELINE_STAGED && (rc = ln.stream.ensure(ctx, hipStreamNonBlocking))) return rc;
        for (emp::Event* ev : {&ln.ev_in, &ln.ev_front, &ln.ev_tail, &ln.ev_done, &ln.ev_qp, &ln.ev_enrich})
            if ((rc = ev->ensure(ctx, hipEventDisableTiming))) return rc;
    }
    if (m == EMP_PIPELINE_STAGED) {
        // the back stage's kernels are short chains of dependent instructions on few wavefronts: their queue gets the
        // higher priority, so that they are dispatched (and, with s_setprio in the kernels, issued) ahead of the front
        // stage's bulk work they overlap with.  (Until round 6 an option confined this stream to a CU mask: never a gain.)
        if (const int rc = ctx->back_stream.ensure(ctx, hipStreamNonBlocking, true)) return rc;
    }
    for (auto& ln : ctx->lanes) ln.done_valid = ln.qp_valid = ln.enrich_valid = false;       // everything was drained above
    ctx->lane_edge_done = nullptr;
    ctx->pipe_mode = m;
    ctx->lane = 0;
    return EMP_OK;
}

int emp_pipeline_form(emp_ctx* ctx, int32_t* hw_queues, int32_t* other_streams) {
    if (!ctx) return EMP_ERR_INVALID;
    if (hw_queues) *hw_queues = ctx->auto_queues;
    if (other_streams) *other_streams = ctx->auto_streams;
    return ctx->pipe_mode;
}

int emp_pipeline_depth(emp_ctx* ctx) {
    if (!ctx) return EMP_ERR_INVALID;
    return ctx->pipe_mode == 0 ? 1 : ctx->lanes_in_use();
}

int emp_set_fence(emp_ctx* ctx, int enabled) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    ctx->fence = enabled != 0;
    return EMP_OK;
}

int emp_set_option(emp_ctx* ctx, int32_t option, int32_t value) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, option >= 0 && option < EMP_OPT_COUNT, "unknown option");
    bool ok = false;
    switch (option) {
        case EMP_OPT_PATH_QP_FORM:
        case EMP_OPT_CARTESIAN_FORM:
        case EMP_OPT_SMOOTH_FORCE_FALLBACK:
        case EMP_OPT_EDGE_AFTER_ENRICH:
        case EMP_OPT_EDGE_FORM:
        case EMP_OPT_EDGE_CLOCK_PROBE:
        case EMP_OPT_CYCLE_GRAPH:
        case EMP_OPT_SWEEP_CLOCK_PROBE: ok = value == 0 || value == 1; break;
        case EMP_OPT_LANE_EDGE_ORDER:
        case EMP_OPT_SWEEP_EXCLUSIVE: ok = value >= 0 && value <= 2; break;
        case EMP_OPT_EDGE_BLOCK: ok = value == 0 || (value >= 64 && value <= 1024 && value % 64 == 0); break;
        case EMP_OPT_FOREIGN_STREAMS: ok = value >= 0 && value <= 64; break;
    }
    EMP_REQUIRE(ctx, ok, "option value out of range (include/emplanner.h, emp_option)");
    ctx->opt[option] = value;
    if (option == EMP_OPT_SWEEP_CLOCK_PROBE) ctx->probe_launches = 0;      // the statistics start over
    return EMP_OK;
}

int emp_get_option(emp_ctx* ctx, int32_t option, int32_t* value) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, option >= 0 && option < EMP_OPT_COUNT && value, "unknown option or NULL value");
    *value = ctx->opt[option];
    return EMP_OK;
}

double emp_sweep_clock_mhz(emp_ctx* ctx, double* mean_wave_us, double* max_wave_us) {
    if (!ctx || !ctx->clock_probe.p || !ctx->clock_probe_done || ctx->clock_probe_tiles <= 0 || ctx->probe_launches <= 0) return -1.0;
    if (hipEventSynchronize(ctx->clock_probe_done) != hipSuccess) return -1.0;
    const long slots = ctx->probe_launches < emp_ctx::kProbeSlots ? ctx->probe_launches : emp_ctx::kProbeSlots;
    const size_t waves = (size_t)slots * ctx->clock_probe_tiles;
    std::vector<unsigned long long> h(waves * 4);
    if (hipMemcpy(h.data(), ctx->clock_probe.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
        return -1.0;
    double ticks_c = 0.0, ticks_r = 0.0, longest = 0.0;
    for (size_t t = 0; t < waves; ++t) {
        const double dc = (double)(h[4 * t + 1] - h[4 * t + 0]), dr = (double)(h[4 * t + 3] - h[4 * t + 2]);
        ticks_c += dc;
        ticks_r += dr;
        if (dr > longest) longest = dr;
    }
    if (ticks_r <= 0.0) return -1.0;
    if (mean_wave_us) *mean_wave_us = ticks_r / (double)waves / 100.0;      // 100 MHz reference
    if (max_wave_us) *max_wave_us = longest / 100.0;
    return ticks_c / ticks_r * 100.0;
}

int emp_edge_probe(emp_ctx* ctx, double* mean_wave_us, double* span_us, double* mean_resident_waves, int32_t* waves) {
    if (!ctx || !ctx->edge_probe.p || !ctx->edge_probe_done || ctx->edge_probe_waves <= 0) return EMP_ERR_INVALID;
    if (hipEventSynchronize(ctx->edge_probe_done) != hipSuccess) return EMP_ERR_HIP;
    std::vector<unsigned long long> h((size_t)ctx->edge_probe_waves * 4);
    if (hipMemcpy(h.data(), ctx->edge_probe.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return EMP_ERR_HIP;
    unsigned long long first = ~0ull, last = 0;
    double sum = 0.0;
    for (long w = 0; w < ctx->edge_probe_waves; ++w) {
        first = std::min(first, h[4 * w]);
        last = std::max(last, h[4 * w + 1]);
        sum += (double)(h[4 * w + 1] - h[4 * w]);
    }
    const double span = (double)(last - first);
    if (mean_wave_us) *mean_wave_us = sum / (double)ctx->edge_probe_waves / 100.0;      // 100 MHz reference
    if (span_us) *span_us = span / 100.0;
    if (mean_resident_waves) *mean_resident_waves = span > 0 ? sum / span : 0.0;
    if (waves) *waves = (int32_t)ctx->edge_probe_waves;
    return EMP_OK;
}

double emp_edge_clock_mhz(emp_ctx* ctx) {
    if (!ctx || !ctx->edge_probe.p || !ctx->edge_probe_done || ctx->edge_probe_waves <= 0) return -1.0;
    if (hipEventSynchronize(ctx->edge_probe_done) != hipSuccess) return -1.0;
    std::vector<unsigned long long> h((size_t)ctx->edge_probe_waves * 4);
    if (hipMemcpy(h.data(), ctx->edge_probe.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    double ticks_c = 0.0, ticks_r = 0.0;
    for (long w = 0; w < ctx->edge_probe_waves; ++w) {
        ticks_r += (double)(h[4 * w + 1] - h[4 * w]);
        ticks_c += (double)(h[4 * w + 3] - h[4 * w + 2]);
    }
    return ticks_r > 0.0 ? ticks_c / ticks_r * 100.0 : -1.0;          // 100 MHz reference
}

int emp_sweep_probe_spans(emp_ctx* ctx, double* start_spread_us, double* first_start_to_last_end_us) {
    if (!ctx || !ctx->clock_probe.p || !ctx->clock_probe_done || ctx->clock_probe_tiles <= 0 || ctx->probe_launches <= 0) return EMP_ERR_INVALID;
    if (hipEventSynchronize(ctx->clock_probe_done) != hipSuccess) return EMP_ERR_HIP;
    const long slots = ctx->probe_launches < emp_ctx::kProbeSlots ? ctx->probe_launches : emp_ctx::kProbeSlots;
    const size_t tiles = (size_t)ctx->clock_probe_tiles;
    std::vector<unsigned long long> h((size_t)slots * tiles * 4);
    if (hipMemcpy(h.data(), ctx->clock_probe.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return EMP_ERR_HIP;
    double spread = 0.0, span = 0.0;
    for (long sl = 0; sl < slots; ++sl) {
        unsigned long long first = ~0ull, last_start = 0, last_end = 0;
        for (size_t t = 0; t < tiles; ++t) {
            const unsigned long long* o = &h[((size_t)sl * tiles + t) * 4];
            if (o[2] < first) first = o[2];
            if (o[2] > last_start) last_start = o[2];
            if (o[3] > last_end) last_end = o[3];
        }
        spread += (double)(last_start - first);
        span += (double)(last_end - first);
    }
    if (start_spread_us) *start_spread_us = spread / (double)slots / 100.0;
    if (first_start_to_last_end_us) *first_start_to_last_end_us = span / (double)slots / 100.0;
    return EMP_OK;
}

int emp_device_alloc(emp_ctx* ctx, uint64_t bytes, void** out) {
    EMP_REQUIRE(ctx, ctx && out, "NULL argument");
    EMP_HIP(ctx, hipSetDevice(ctx->device));
    EMP_HIP(ctx, hipMalloc(out, bytes ? bytes : 8));
    return EMP_OK;
}
int emp_device_free(emp_ctx* ctx, void* ptr) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_HIP(ctx, (hipError_t)sync_all(ctx));
    EMP_HIP(ctx, hipFree(ptr));
    return EMP_OK;
}
int emp_copy_to_device(emp_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    EMP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return EMP_OK;
}
int emp_copy_to_host(emp_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    EMP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return EMP_OK;
}

int emp_set_timing(emp_ctx* ctx, int enabled) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    ctx->timing = enabled != 0;
    if (ctx->timing)
        for (auto& kv : ctx->events) kv.second.used = 0;   // restart the statistics
    return EMP_OK;
}

int emp_set_timing_filter(emp_ctx* ctx, const char* kernel) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    ctx->timing_filter = kernel ? kernel : "";
    return EMP_OK;
}

int emp_kernel_launches(emp_ctx* ctx, const char* kernel) {
    if (!ctx || !kernel) return 0;
    auto it = ctx->events.find(kernel);
    return it == ctx->events.end() ? 0 : (int)it->second.used;
}

double emp_kernel_ms(emp_ctx* ctx, const char* kernel) {
    if (!ctx || !kernel) return -1.0;
    auto it = ctx->events.find(kernel);
    if (it == ctx->events.end() || it->second.used == 0) return -1.0;
    double total = 0.0;
    for (size_t i = 0; i < it->second.used; ++i) {
        auto& pr = it->second.pairs[i];
        if (hipEventSynchronize(pr.second) != hipSuccess) return -1.0;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) != hipSuccess) return -1.0;
        total += (double)ms;
    }
    return total / (double)it->second.used;
}

int emp_kernel_samples(emp_ctx* ctx, const char* kernel, double* ms, int32_t cap) {
    if (!ctx || !kernel || (cap > 0 && !ms) || cap < 0) return -1;
    auto it = ctx->events.find(kernel);
    if (it == ctx->events.end()) return 0;
    const size_t n = it->second.used;
    for (size_t i = 0; i < n && i < (size_t)cap; ++i) {
        auto& pr = it->second.pairs[i];
        float v = 0.f;
        if (hipEventSynchronize(pr.second) != hipSuccess || hipEventElapsedTime(&v, pr.first, pr.second) != hipSuccess) return -1;
        ms[i] = (double)v;
    }
    return (int)n;
}

// ---- DP ----------------------------------------------------------------------------------
uint64_t emp_edge_tensor_elems(const emp_dp_params* p, int32_t B, emp_edge_layout layout) {
    if (!p || p->row < 1 || p->row > emp::kMaxWideRow || p->col < 1 || B < 0) return 0;
    return (uint64_t)emp::edge_tensor_elems(p->row, p->col, B, layout != EMP_EDGE_CANONICAL);
}

int emp_dp_edge_costs(emp_ctx* ctx, const emp_dp_params* p, int32_t B, int32_t max_obs, const double* obs_s,
                      const double* obs_l, const int32_t* n_obs, const double* start, double* start_cost,
                      double* edge, emp_edge_layout layout, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    DpDev d;
    if (const int rc = make_dp_dev(ctx, p, B, max_obs, &d)) return rc;
    EMP_REQUIRE(ctx, n_obs && start && edge, "n_obs, start and edge are required");
    EMP_REQUIRE(ctx, max_obs == 0 || (obs_s && obs_l), "obs_s / obs_l are required when max_obs > 0");
    EMP_STAGE(st, where);
    const double* d_os = st.in(obs_s, (size_t)B * max_obs);
    const double* d_ol = st.in(obs_l, (size_t)B * max_obs);
    const int* d_n = st.in(n_obs, (size_t)B);
    const double* d_start = st.in(start, (size_t)B * 4);
    double* d_c0 = st.out(start_cost, (size_t)B * d.row);
    double* d_e = st.out(edge, (size_t)emp_edge_tensor_elems(p, B, layout), layout == EMP_EDGE_TILED);  // canonical: fully written
    if (max_obs == 0) d_os = d_ol = st.tmp<double>(1);   // kernels index [b * max_obs + m] only for m < n_obs == 0
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_dp_edge(ctx, d, d_os, d_ol, d_n, d_start, d_c0, d_e, layout == EMP_EDGE_TILED, nullptr)) return rc;
    return st.finish();
}

int emp_dp_sweep(emp_ctx* ctx, const emp_dp_params* p, int32_t B, const double* start_cost, const double* edge,
                 double* rows, double* min_cost, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    DpDev d;
    if (const int rc = make_dp_dev(ctx, p, B, 0, &d)) return rc;
    EMP_REQUIRE(ctx, start_cost && edge && rows && status, "start_cost, edge, rows and status are required");
    EMP_STAGE(st, where);
    const double* d_c0 = st.in(start_cost, (size_t)B * d.row);
    const double* d_e = st.in(edge, tiled_elems(d));
    double* d_rows = st.out(rows, (size_t)B * d.col);
    double* d_min = st.out(min_cost, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_dp_sweep(ctx, d, d_c0, d_e, nullptr, d_rows, d_min, d_st, nullptr)) return rc;
    return st.finish();
}

int emp_dp_plan(emp_ctx* ctx, const emp_dp_params* p, int32_t B, int32_t max_obs, const double* obs_s,
                const double* obs_l, const int32_t* n_obs, const double* start, emp_dp_mode mode, double* rows,
                double* min_cost, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    DpDev d;
    if (const int rc = make_dp_dev(ctx, p, B, max_obs, &d)) return rc;
    EMP_REQUIRE(ctx, n_obs && start && rows && status, "n_obs, start, rows and status are required");
    EMP_REQUIRE(ctx, max_obs == 0 || (obs_s && obs_l), "obs_s / obs_l are required when max_obs > 0");
    EMP_STAGE(st, where);
    const double* d_os = st.in(obs_s, (size_t)B * max_obs);
    const double* d_ol = st.in(obs_l, (size_t)B * max_obs);
    const int* d_n = st.in(n_obs, (size_t)B);
    const double* d_start = st.in(start, (size_t)B * 4);
    double* d_rows = st.out(rows, (size_t)B * d.col);
    double* d_min = st.out(min_cost, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (max_obs == 0) d_os = d_ol = st.tmp<double>(1);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_dp_plan(ctx, d, d_os, d_ol, d_n, d_start, mode, d_rows, d_min, d_st, nullptr)) return rc;
    return st.finish();
}

int emp_dp_enrich(emp_ctx* ctx, const emp_dp_params* p, int32_t B, const double* rows, const double* start,
                  int32_t max_pts, double* path_s, double* path_l, int32_t* path_len, int32_t* status,
                  emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    DpDev d;
    if (const int rc = make_dp_dev(ctx, p, B, 0, &d)) return rc;
    EMP_REQUIRE(ctx, rows && start && path_s && path_l && path_len && status, "NULL argument");
    EMP_REQUIRE(ctx, max_pts >= 1, "max_pts must be >= 1");
    EMP_STAGE(st, where);
    const double* d_rows = st.in(rows, (size_t)B * d.col);
    const double* d_start = st.in(start, (size_t)B * 4);
    double* d_ps = st.out(path_s, (size_t)B * max_pts);
    double* d_pl = st.out(path_l, (size_t)B * max_pts);
    int* d_len = st.out(path_len, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_dp_enrich(ctx, d, d_rows, d_start, max_pts, d_ps, d_pl, d_len, d_st, 0, nullptr)) return rc;
    return st.finish();
}

}  // extern "C"


// =============================================================================================
// Frenet / QP stages and the whole cycle
// =============================================================================================
namespace emp {

// emp_qp_params.reserved: 0 in every build that ships.  A development build (-DEMP_DEV_HOOKS) reads it as the QP kernels'
// debug stage (cut the solve short / cap its iterations for timing experiments, tools/qp_sensitivity_probe.py); a product
// build refuses it, so that an uninitialised struct can never mask a failed solve.
static bool qp_reserved_ok(const emp_qp_params* q) { return EMP_DEV_HOOKS || q->reserved == 0; }

static QpDev make_qp_dev(const emp_qp_params* q) {
    QpDev d;
    d.qp = PathQpParams{q->ds, q->w_l, q->w_ddl, q->w_dddl, q->w_centre, q->host_d1, q->host_d2, q->host_w};
    d.obs_length = q->obs_length;
    d.obs_width = q->obs_width;
    d.decimate = q->decimate > 0 ? q->decimate : 1;
    d.midpoint = q->midpoint;
    d.use_qp = q->use_qp;
    d.debug_stage = EMP_DEV_HOOKS ? q->reserved : 0;
    return d;
}

static inline dim3 grid1(int n, int block) { return dim3((unsigned)((n + block - 1) / block)); }
// one 64-lane block per wavefront of `per_wave` vehicle groups (the lateral MPCs' mapping)
static inline dim3 grid_groups(int B, int per_wave) { return grid1(B, per_wave); }

static int dev_project(emp_ctx* ctx, int B, int max_ref, int max_obs, const double* ref_line, const int* n_ref,
                       const double* origin_xy, const double* start_xy, const double* start_v, const double* start_a,
                       const double* obs_xy, const int* n_obs, double* s_map, double* obs_s, double* obs_l,
                       double* begin_sl, double* start, int obs_cap = -1, const double* dyn = nullptr,
                       int* n_obs_out = nullptr) {
    return launch_plan(ctx, "project", plan_project(B, max_ref), frenet_project_wave_kernel, B, max_ref, max_obs, ref_line, n_ref,
                       origin_xy, start_xy, start_v, start_a, obs_xy, n_obs, s_map, obs_s, obs_l, begin_sl, start,
                       obs_cap < 0 ? max_obs : obs_cap, dyn, n_obs_out);
}

// smooth_reference_line, one wavefront per scene (emp_reference_line, and the front end of emp_plan_cycle)
template <typename... A>
static int dev_reference_line(emp_ctx* ctx, const emp_smooth_params* sp, int B, int max_global, A... args) {
    const SmoothQpParams sx{sp->w_smooth, sp->w_length, sp->w_ref, sp->x_thre};
    const SmoothQpParams sy{sp->w_smooth, sp->w_length, sp->w_ref, sp->y_thre};
    return launch_plan(ctx, "reference_line", plan_reference_line(B), reference_line_wave_kernel, B, max_global, sx, sy, args...);
}

static int dev_cycle_qp(emp_ctx* ctx, int B, int max_pts, int max_obs, const QpDev& Q, const double* dp_s,
                        const double* dp_l, const int* dp_len, const double* obs_s, const double* obs_l,
                        const int* n_obs, const double* start, double* path_s, double* path_l, int* path_len,
                        int* status, CycleSched* cs) {
    if (B == 0) return EMP_OK;
    // which kernel, how many scenes per wavefront and why: emp_tail_launch.h plan_cycle_qp
    const TailPlan p = plan_cycle_qp(B, max_pts, max_obs, Q.decimate, ctx->opt[EMP_OPT_PATH_QP_FORM], EMP_QP_LDS_PAD);
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    const int cap = (max_pts + Q.decimate - 1) / Q.decimate;          // most stations a scene can have
    auto kern = p.r == 0 ? (p.gp == 32 ? cycle_qp_wave_kernel<32> : cycle_qp_wave_kernel<64>)
                         : p.gp == 16 ? cycle_qp_rows_kernel<16, 4> : p.r == 3 ? cycle_qp_rows_kernel<8, 3> : cycle_qp_rows_kernel<8, 4>;
    KernelTimer t(ctx, "path_qp");
    if (const int rc = set_lds(ctx, kern, p.lds, kQpTooLarge)) return rc;
    return launch_attaching(ctx, cs, t.stop != nullptr, kern, dim3(p.grid), dim3(p.block), p.lds, B, max_pts, max_obs, cap, Q, dp_s,
                            dp_l, dp_len, obs_s, obs_l, n_obs, start, path_s, path_l, path_len, status);
}

static int dev_cycle_cartesian(emp_ctx* ctx, int B, int max_ref, int max_pts, int path_cap, const emp_smooth_params* sp,
                               const double* ref_line, const double* s_map, const int* n_ref, const double* begin_sl,
                               const double* path_s, const double* path_l, const int* path_len, double* traj,
                               int* traj_len, int* status) {
    if (B == 0) return EMP_OK;
    const SmoothQpParams sx{sp->w_smooth, sp->w_length, sp->w_ref, sp->x_thre};
    const SmoothQpParams sy{sp->w_smooth, sp->w_length, sp->w_ref, sp->y_thre};
    const int cap = path_cap + 1;                                        // trajectory = planning start + path points
    // which kernel and how many scenes per wavefront: emp_tail_launch.h plan_cycle_cartesian
    const TailPlan p = plan_cycle_cartesian(B, max_ref, max_pts, path_cap, ctx->opt[EMP_OPT_CARTESIAN_FORM]);
    auto go = [&](auto kern, auto... hook) {
        return launch_plan(ctx, "to_cartesian", p, kern, B, max_ref, max_pts, cap, sx, sy, ref_line, s_map, n_ref, begin_sl, path_s, path_l,
                           path_len, traj, traj_len, status, hook...);
    };
    if (p.r == 0) return go(p.wide ? cycle_cartesian_wave_kernel_wide : cycle_cartesian_wave_kernel_narrow);
    return go(p.gp == 16 ? cycle_cartesian_rows_kernel<16, 4> : p.r == 3 ? cycle_cartesian_rows_kernel<8, 3> : cycle_cartesian_rows_kernel<8, 4>,
              ctx->opt[EMP_OPT_SMOOTH_FORCE_FALLBACK] ? 1 : 0);                                      // (the rows smoother's test hook)
}

// ---- emp_plan_cycle's pipeline lane and cycle graph -------------------------------------------------------------------
// Pipelined modes (device pointers only; emp_context.h).  LANES: the whole call runs on the next lane - its stream stands in
// for ctx->stream and its pool for ctx->pool - behind whatever the caller has ordered on the main stream so far.  STAGED: the
// call takes the pool of the next lane once the back stage that used it last is done; its front stage runs on the main
// stream, its back stage on the back stream.
// EMP_HOST_PINNED: the caller's arrays are page-locked; the call is pipelined like a device-pointer call, its inputs arrive
// over the copy stream and its outputs leave over the d2h stream (emp_context.h Stage: async_host).
// Outside pipelined mode (mode 0) a CycleLane orders nothing; done() still sends a pinned call's outputs home.
class CycleLane {
  public:
    CycleLane(emp_ctx* c, int m, bool p) : ctx(c), mode(m), pinned(p) {}
    ~CycleLane() {          // the main stream and pool stand in for the call's again
        if (!ln) return;
        ctx->stream = ctx->main_stream;
        std::swap(ctx->pool, ln->pool);
        ctx->active_lane = -1;
    }

    // The pinned path's streams and events, then the next lane is taken over and ordered.
    int begin() {
        if (pinned) {
            if (const int rc = ctx->copy_stream.ensure(ctx, hipStreamNonBlocking)) return rc;
            if (const int rc = ctx->d2h_stream.ensure(ctx, hipStreamNonBlocking)) return rc;
            if (const int rc = ctx->ev_h2d.ensure(ctx, hipEventDisableTiming)) return rc;
            if (const int rc = ctx->ev_host_last.ensure(ctx, hipEventDisableTiming)) return rc;
        }
        if (!mode) return EMP_OK;
        ctx->lane = (ctx->lane + 1) % ctx->lanes_in_use();
        ++ctx->cycle_calls;
        ln = &ctx->lanes[ctx->lane];                  // (ln->ticket changes below, after the host-side wait for the lane's previous call)
        std::swap(ctx->pool, ln->pool);
        if (staged()) {
            // the pool's previous user is four calls back: a host-side wait (emp_context.h, kStagedPools)
            if (ln->done_valid) EMP_HIP(ctx, hipEventSynchronize(ln->ev_done));
            if (ln->host_valid) EMP_HIP(ctx, hipEventSynchronize(ln->ev_host));   // ... and its outputs have left the pool
        } else {
            ctx->active_lane = ctx->lane;
            ctx->stream = ln->stream;
            if (ln->host_valid) EMP_HIP(ctx, hipEventSynchronize(ln->ev_host));
            // The lane's previous occupant (call k - n) and whatever its caller queued behind it on the lane's stream (record
            // packing) must be done before anything ordered on the main stream from here on may touch memory they use: the
            // caller keeps a call's outputs alive only until this call is issued, and the NEXT call runs on another lane.
            if (ln->done_valid) {
                EMP_HIP(ctx, hipEventRecord(ln->ev_tail, ctx->stream));
                EMP_HIP(ctx, hipStreamWaitEvent(ctx->main_stream, ln->ev_tail, 0));
            }
            EMP_HIP(ctx, hipEventRecord(ln->ev_in, ctx->main_stream));
            EMP_HIP(ctx, hipStreamWaitEvent(ctx->stream, ln->ev_in, 0));
        }
        // Only now - the previous occupant's outputs are in its caller's arrays - does the lane stop answering for the previous
        // ticket: emp_wait_ticket(T) on another thread either still finds the lane under T with its event valid and waits for
        // the same event, or finds no lane under T, which now MEANS that this thread has waited for T already (the advisor's
        // round-5 finding: the ticket used to change before the wait, and a waiter in that window returned at once).
        ln->host_valid = false;
        ln->ticket = ctx->cycle_calls;
        // A pinned call's inputs go into the lane's pool over the copy stream.  If the lane's previous occupant was an EMP_DEVICE
        // cycle there has been no host-side wait for it: the copy stream waits for its kernels instead.
        if (pinned && !staged() && ln->done_valid) EMP_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ln->ev_done, 0));
        return EMP_OK;
    }

    // STAGED: what the front stage's launches signal and wait for (CycleSched).  `two_kernel`: the edge-cost kernel runs.
    void front_waits(CycleSched& cs, bool two_kernel) const {
        if (!staged()) return;
        cs.front_stop = ln->ev_front;
        // the previous call's back stage: its lane is the one before ours
        const emp_ctx::Lane& prev = ctx->lanes[(ctx->lane + ctx->lanes_in_use() - 1) % ctx->lanes_in_use()];
        // (EMP_OPT_SWEEP_EXCLUSIVE = 2: only its densification and path QP - the sweep runs beside the Cartesian tail)
        if (ctx->opt[EMP_OPT_SWEEP_EXCLUSIVE] == 2 && prev.qp_valid) cs.sweep_wait = prev.ev_qp;
        if (ctx->opt[EMP_OPT_SWEEP_EXCLUSIVE] == 1 && prev.done_valid) cs.sweep_wait = prev.ev_done;
        if (ctx->opt[EMP_OPT_EDGE_AFTER_ENRICH] && two_kernel && prev.enrich_valid) cs.edge_wait = prev.ev_enrich;
    }

    // STAGED, behind the sweep: the back stage (short kernels that last as long as their slowest scene) goes to the back stream.
    int to_back(const CycleSched& cs) {
        if (!staged()) return EMP_OK;
        // EMP_OPT_SWEEP_EXCLUSIVE: a marker behind the sweep on the front stream.  Measured, not understood: which of two
        // regimes the two queues settle in depends on it.  With it the kernels keep the durations of the overlapped step (edge
        // 198 us, path QP 140, Cartesian 70, sweep 19) and the step takes 0.264 ms (mode 2) / 0.277 (mode 1); without it the
        // edge kernel runs at its stand-alone 147 us, starves the path QP beside it (250 us) and the step takes 0.32 - 0.35 ms
        // (profiles/r04_sweep/README.md).  The clock probe's event did the same by accident, which is how this was found.
        if (ctx->opt[EMP_OPT_SWEEP_EXCLUSIVE]) {
            if (const int rc = ctx->sweep_marker.ensure(ctx, hipEventDisableTiming)) return rc;
            EMP_HIP(ctx, hipEventRecord(ctx->sweep_marker, ctx->stream));
        }
        // behind the sweep's own completion event where the launch attached one (a marker packet behind the sweep costs the
        // front queue ~5 us per step), else behind an event recorded here
        hipEvent_t front_done = cs.front_attached;
        if (!front_done) {
            EMP_HIP(ctx, hipEventRecord(ln->ev_front, ctx->stream));
            front_done = ln->ev_front;
        }
        EMP_HIP(ctx, hipStreamWaitEvent(ctx->back_stream, front_done, 0));
        ctx->stream = ctx->back_stream;        // ~CycleLane puts the main stream back
        return EMP_OK;
    }

    // STAGED: a back-stage kernel (`launch`) signals the lane's event `ev` for the NEXT call's front stage when `want`, and
    // the lane's `valid` flag says whether it does.  The dispatch itself signals it where possible (CycleSched::attach_stop):
    // a marker packet behind each idled the back queue ~6 us, and with the edge kernel's round-4 diet the back queue is what
    // bounds the step.  Where the launch could not attach it, the event is recorded behind the kernel.
    template <typename F>
    int signal(CycleSched& cs, bool want, emp::Event emp_ctx::Lane::*ev, bool emp_ctx::Lane::*valid, F launch) {
        want = want && staged();
        cs.attach_stop = want ? (hipEvent_t)(ln->*ev) : nullptr;
        cs.stop_attached = false;
        if (const int rc = launch()) return rc;
        if (want && !cs.stop_attached) EMP_HIP(ctx, hipEventRecord(ln->*ev, ctx->stream));
        if (staged()) ln->*valid = want;
        return EMP_OK;
    }

    // The end of the cycle: the lane's ev_done, then a pinned call's outputs go home on the d2h stream behind the cycle's last
    // kernel.  Pipelined, nobody waits here (emp_wait_cycle, emp_synchronize, or the call that takes this pool over); not
    // pipelined, the pool is the next call's, so the host waits.
    int done(Stage& st) {
        if (ln) {
            EMP_HIP(ctx, hipEventRecord(ln->ev_done, ctx->stream));
            ln->done_valid = true;
        }
        if (!st.async_host()) return EMP_OK;
        if (ln) {
            if (const int rc = ln->ev_host.ensure(ctx, hipEventDisableTiming)) return rc;
            if (const int rc = st.finish_async(ln->ev_done, ln->ev_host)) return rc;
            ln->host_valid = true;
            return EMP_OK;
        }
        EMP_HIP(ctx, hipEventRecord(ctx->ev_h2d, ctx->stream));
        if (const int rc = st.finish_async(ctx->ev_h2d, ctx->ev_host_last)) return rc;
        EMP_HIP(ctx, hipEventSynchronize(ctx->ev_host_last));
        return EMP_OK;
    }

  private:
    bool staged() const { return mode == EMP_PIPELINE_STAGED; }
    emp_ctx* ctx;
    int mode;
    bool pinned;
    emp_ctx::Lane* ln = nullptr;       // the lane of this call (pipelined)
};

// EMP_OPT_CYCLE_GRAPH: one batch at a time on device pointers - the third consecutive call with one signature is captured,
// the following ones are one hipGraphLaunch.  The signature is everything a launch argument is made of; the context's
// allocation count says whether a temporary or a lattice table moved or changed since the capture.
class CycleCapture {
  public:
    explicit CycleCapture(emp_ctx* c) : ctx(c) {}
    ~CycleCapture() {
        if (!active) return;            // (an early return inside the captured region: end the capture, keep nothing)
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(ctx->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        ctx->cycle_graph.capturing = false;
    }

    // A call that may use the graph replays it (and sets *replayed: that was the call's work) or, at its signature's third
    // call in a row, begins a capture; any other call drops the graph.
    int begin(int pmode, emp_mem where, int B, int max_ref, int max_obs, int max_pts, emp_dp_mode mode, const emp_dp_params* p,
              const emp_qp_params* q, const emp_smooth_params* sp, const emp_cycle_io* io, bool* replayed) {
        emp_ctx::CycleGraph& g = ctx->cycle_graph;
        if (ctx->opt[EMP_OPT_CYCLE_GRAPH] != 1 || pmode != 0 || where != EMP_DEVICE || B <= 0 || ctx->timing ||
            ctx->opt[EMP_OPT_SWEEP_CLOCK_PROBE] || ctx->opt[EMP_OPT_EDGE_CLOCK_PROBE]) {
            if (g.exec) g.seen = 0;         // (a graph is dropped: its signature starts over)
            (void)g.exec.reset();
            return EMP_OK;
        }
        std::vector<unsigned long long> key;
        auto add = [&](const void* ptr, size_t bytes) {
            const unsigned char* b8 = (const unsigned char*)ptr;
            for (size_t o = 0; o < bytes; o += 8) {
                unsigned long long w = 0;
                memcpy(&w, b8 + o, std::min<size_t>(8, bytes - o));
                key.push_back(w);
            }
        };
        const long long sizes[5] = {B, max_ref, max_obs, max_pts, (long long)mode};
        add(sizes, sizeof(sizes));
        add(p, sizeof(*p));
        add(q, sizeof(*q));
        add(sp, sizeof(*sp));
        add(io, sizeof(*io));
        add(ctx->opt, sizeof(ctx->opt));
        if (g.exec && key == g.key && ctx->alloc_gen == g.gen) {
            EMP_HIP(ctx, hipGraphLaunch(g.exec, ctx->stream));
            ++g.replays;
            *replayed = true;
            return EMP_OK;
        }
        (void)g.exec.reset();               // another signature, or the buffers moved: the graph is stale
        g.seen = (key == g.seen_key) ? g.seen + 1 : 1;
        g.seen_key = key;
        if (g.seen >= 3) {                  // the two calls before this one allocated and built whatever this signature needs
            g.gen = ctx->alloc_gen;
            EMP_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
            active = g.capturing = true;
        }
        return EMP_OK;
    }

    // The capture (if any) ends: the graph is kept unless the context's buffers changed inside it, and launched - the captured
    // launches have not run yet: this is the call's work.
    int end() {
        if (!active) return EMP_OK;
        emp_ctx::CycleGraph& g = ctx->cycle_graph;
        active = g.capturing = false;
        hipGraph_t graph = nullptr;
        EMP_HIP(ctx, hipStreamEndCapture(ctx->stream, &graph));
        emp::GraphExec exec;
        const hipError_t ie = hipGraphInstantiate(&exec.h, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        EMP_HIP(ctx, ie);
        if (ctx->alloc_gen != g.gen) {      // something was allocated or rebuilt inside the capture after all
            g.seen = 0;
            return emp::fail(ctx, EMP_ERR_HIP, "EMP_OPT_CYCLE_GRAPH: the context's buffers changed inside a capture");
        }
        g.exec = std::move(exec);
        g.key = g.seen_key;
        EMP_HIP(ctx, hipGraphLaunch(g.exec, ctx->stream));
        return EMP_OK;
    }

  private:
    emp_ctx* ctx;
    bool active = false;
};

}  // namespace emp

extern "C" {

int emp_frenet_project(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_obs, const double* ref_line,
                       const int32_t* n_ref, const double* origin_xy, const double* start_xy, const double* start_v,
                       const double* start_a, const double* obs_xy, const int32_t* n_obs, double* s_map, double* obs_s,
                       double* obs_l, double* begin_sl, double* start, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_ref >= 2 && max_obs >= 0, "bad sizes");
    EMP_REQUIRE(ctx, ref_line && n_ref && origin_xy && start_xy && start_v && start_a && s_map && start, "NULL argument");
    EMP_REQUIRE(ctx, max_obs == 0 || (obs_xy && n_obs && obs_s && obs_l), "obstacle arrays required when max_obs > 0");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)B * max_ref * 4);
    const int* d_nr = st.in(n_ref, (size_t)B);
    const double* d_o = st.in(origin_xy, (size_t)B * 2);
    const double* d_sxy = st.in(start_xy, (size_t)B * 2);
    const double* d_v = st.in(start_v, (size_t)B * 2);
    const double* d_a = st.in(start_a, (size_t)B * 2);
    const double* d_oxy = st.in(obs_xy, (size_t)B * max_obs * 2);
    const int* d_no = st.in(max_obs ? n_obs : nullptr, (size_t)B);
    double* d_sm = st.out(s_map, (size_t)B * max_ref);
    double* d_os = st.out(obs_s, (size_t)B * max_obs);
    double* d_ol = st.out(obs_l, (size_t)B * max_obs);
    double* d_bsl = st.out(begin_sl, (size_t)B * 2);
    double* d_start = st.out(start, (size_t)B * 4);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_project(ctx, B, max_ref, max_obs, d_ref, d_nr, d_o, d_sxy, d_v, d_a, d_oxy, d_no, d_sm, d_os, d_ol, d_bsl,
                                   d_start))
        return rc;
    return st.finish();
}

static int match_common(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                        const int32_t* n_ref, const double* xy, const int32_t* n_pts, const int32_t* is_first_run,
                        const int32_t* pre_match_index, int32_t* match_index, double* proj, emp_mem where, int windowed) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_ref >= 1 && max_pts >= 1, "bad sizes");
    EMP_REQUIRE(ctx, ref_line && n_ref && xy && n_pts && match_index && proj, "NULL argument");
    EMP_REQUIRE(ctx, !windowed || (is_first_run && pre_match_index), "is_first_run / pre_match_index required");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)B * max_ref * 4);
    const int* d_nr = st.in(n_ref, (size_t)B);
    const double* d_xy = st.in(xy, (size_t)B * max_pts * 2);
    const int* d_np = st.in(n_pts, (size_t)B);
    const int* d_first = st.in(is_first_run, (size_t)B);
    const int* d_pre = st.in(pre_match_index, (size_t)B);
    int* d_mi = st.out(match_index, (size_t)B * max_pts);
    double* d_pr = st.out(proj, (size_t)B * max_pts * 4);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "match", match_points_kernel, grid1(B, 64), dim3(64), 0, B, max_ref, max_pts, d_ref, d_nr, d_xy,
                              d_np, d_first, d_pre, d_mi, d_pr, windowed))
        return rc;
    return st.finish();
}

int emp_match_projection(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                         const int32_t* n_ref, const double* xy, const int32_t* n_pts, int32_t* match_index,
                         double* proj, emp_mem where) {
    return match_common(ctx, B, max_ref, max_pts, ref_line, n_ref, xy, n_pts, nullptr, nullptr, match_index, proj, where, 0);
}

int emp_find_match_points(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                          const int32_t* n_ref, const double* xy, const int32_t* n_pts, const int32_t* is_first_run,
                          const int32_t* pre_match_index, int32_t* match_index, double* proj, emp_mem where) {
    return match_common(ctx, B, max_ref, max_pts, ref_line, n_ref, xy, n_pts, is_first_run, pre_match_index,
                        match_index, proj, where, 1);
}

int emp_heading_kappa(emp_ctx* ctx, int32_t B, int32_t max_pts, const double* xy, const int32_t* n_pts, double* theta,
                      double* kappa, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_pts >= 2 && xy && n_pts && theta && kappa, "bad argument");
    EMP_STAGE(st, where);
    const double* d_xy = st.in(xy, (size_t)B * max_pts * 2);
    const int* d_np = st.in(n_pts, (size_t)B);
    double* d_t = st.out(theta, (size_t)B * max_pts);
    double* d_k = st.out(kappa, (size_t)B * max_pts);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "heading", heading_kappa_kernel, grid1(B, 64), dim3(64), 0, B, max_pts, d_xy, d_np, d_t, d_k))
        return rc;
    return st.finish();
}

int emp_lmin_lmax(emp_ctx* ctx, int32_t B, int32_t max_pts, int32_t max_obs, const double* dp_s, const double* dp_l,
                  const int32_t* n_pts, const double* obs_s, const double* obs_l, const int32_t* n_obs,
                  double obs_length, double obs_width, double* l_min, double* l_max, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_pts >= 1 && max_obs >= 0, "bad sizes");
    EMP_REQUIRE(ctx, dp_s && dp_l && n_pts && n_obs && l_min && l_max && status, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_s = st.in(dp_s, (size_t)B * max_pts);
    const double* d_l = st.in(dp_l, (size_t)B * max_pts);
    const int* d_np = st.in(n_pts, (size_t)B);
    const double* d_os = st.in(obs_s, (size_t)B * max_obs);
    const double* d_ol = st.in(obs_l, (size_t)B * max_obs);
    const int* d_no = st.in(n_obs, (size_t)B);
    double* d_lo = st.out(l_min, (size_t)B * max_pts);
    double* d_hi = st.out(l_max, (size_t)B * max_pts);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "lmin_lmax", lmin_lmax_kernel, grid1(B, 64), dim3(64), 0, B, max_pts, max_obs, d_s, d_l, d_np,
                              d_os, d_ol, d_no, obs_length, obs_width, d_lo, d_hi, d_st))
        return rc;
    return st.finish();
}

int emp_path_qp(emp_ctx* ctx, const emp_qp_params* q, int32_t B, int32_t max_pts, const double* l_min,
                const double* l_max, const int32_t* n_pts, const double* start_l3, double* qp_l, double* qp_dl,
                double* qp_ddl, int32_t* iters, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, q && B >= 0 && max_pts >= 1 && max_pts <= 256, "bad sizes (max_pts must be in [1, 256])");
    EMP_REQUIRE(ctx, qp_reserved_ok(q), "emp_qp_params.reserved must be 0 (start from emp_qp_params_default)");
    EMP_REQUIRE(ctx, l_min && l_max && n_pts && start_l3 && qp_l && qp_dl && qp_ddl && status, "NULL argument");
    EMP_REQUIRE(ctx, q->ds > 0, "ds must be > 0");
    EMP_STAGE(st, where);
    const double* d_lo = st.in(l_min, (size_t)B * max_pts);
    const double* d_hi = st.in(l_max, (size_t)B * max_pts);
    const int* d_np = st.in(n_pts, (size_t)B);
    const double* d_s3 = st.in(start_l3, (size_t)B * 3);
    double* d_l = st.out(qp_l, (size_t)B * max_pts);
    double* d_dl = st.out(qp_dl, (size_t)B * max_pts);
    double* d_ddl = st.out(qp_ddl, (size_t)B * max_pts);
    int* d_it = st.out(iters, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch_plan(ctx, "path_qp", plan_path_qp(B, max_pts), path_qp_wave_kernel, B, max_pts, max_pts, make_qp_dev(q), d_lo,
                                   d_hi, d_np, d_s3, d_l, d_dl, d_ddl, d_it, d_st))
        return rc;
    return st.finish();
}

int emp_smooth_line(emp_ctx* ctx, const emp_smooth_params* sp, int32_t B, int32_t max_pts, const double* xy,
                    const int32_t* n_pts, double* out, int32_t* iters, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, sp && B >= 0 && max_pts >= 2 && max_pts <= 256, "bad sizes (max_pts must be in [2, 256])");
    EMP_REQUIRE(ctx, xy && n_pts && out && status, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_xy = st.in(xy, (size_t)B * max_pts * 2);
    const int* d_np = st.in(n_pts, (size_t)B);
    double* d_out = st.out(out, (size_t)B * max_pts * 4);
    int* d_it = st.out(iters, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    const SmoothQpParams sx{sp->w_smooth, sp->w_length, sp->w_ref, sp->x_thre};
    const SmoothQpParams sy{sp->w_smooth, sp->w_length, sp->w_ref, sp->y_thre};
    const TailPlan plan = plan_smooth(B, max_pts);
    if (const int rc = launch_plan(ctx, "smooth", plan, plan.wide ? smooth_wave_kernel<true> : smooth_wave_kernel<false>, B, max_pts, max_pts,
                                   sx, sy, d_xy, d_np, d_out, d_it, d_st))
        return rc;
    return st.finish();
}

int emp_reference_line(emp_ctx* ctx, const emp_smooth_params* sp, int32_t B, int32_t max_global,
                       const double* global_path, const int32_t* n_global, const double* pred_xy,
                       const int32_t* is_first_run, const int32_t* pre_match_index, double* ref_line, int32_t* n_ref,
                       int32_t* match_index, int32_t* iters, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, sp && B >= 0 && max_global >= 1, "bad sizes");
    EMP_REQUIRE(ctx, global_path && n_global && pred_xy && pre_match_index && ref_line && n_ref && match_index && status,
                "NULL argument");
    EMP_STAGE(st, where);
    const double* d_g = st.in(global_path, (size_t)B * max_global * 4);
    const int* d_ng = st.in(n_global, (size_t)B);
    const double* d_xy = st.in(pred_xy, (size_t)B * 2);
    const int* d_first = st.in(is_first_run, (size_t)B);
    const int* d_pre = st.in(pre_match_index, (size_t)B);
    double* d_ref = st.out(ref_line, (size_t)B * kRefLinePoints * 4, false);
    int* d_nr = st.out(n_ref, (size_t)B, false);
    int* d_m = st.out(match_index, (size_t)B, false);
    int* d_it = st.out(iters, (size_t)B, false);
    int* d_st = st.out(status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_reference_line(ctx, sp, B, max_global, d_g, d_ng, d_xy, d_first, d_pre, d_ref, d_nr, d_m, d_it, d_st, 0))
        return rc;
    return st.finish();
}

int emp_frenet_path_to_xy(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                          const double* s_map, const int32_t* n_ref, const double* begin_sl, const double* path_s,
                          const double* path_l, const int32_t* n_pts, double* target_xy, int32_t* n_out,
                          int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_ref >= 2 && max_pts >= 1, "bad sizes");
    EMP_REQUIRE(ctx, ref_line && s_map && n_ref && begin_sl && path_s && path_l && n_pts && target_xy && n_out && status,
                "NULL argument");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)B * max_ref * 4);
    const double* d_sm = st.in(s_map, (size_t)B * max_ref);
    const int* d_nr = st.in(n_ref, (size_t)B);
    const double* d_b = st.in(begin_sl, (size_t)B * 2);
    const double* d_ps = st.in(path_s, (size_t)B * max_pts);
    const double* d_pl = st.in(path_l, (size_t)B * max_pts);
    const int* d_np = st.in(n_pts, (size_t)B);
    double* d_t = st.out(target_xy, (size_t)B * (max_pts + 1) * 2);
    int* d_no = st.out(n_out, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "path_to_xy", path_to_xy_kernel, grid1(B, 64), dim3(64), 0, B, max_ref, max_pts, d_ref, d_sm,
                              d_nr, d_b, d_ps, d_pl, d_np, d_t, d_no, d_st))
        return rc;
    return st.finish();
}

}  // extern "C"

namespace emp {
// The speed half of emp_plan_trajectory (ref test_10.py:233-340): its arrays are staged with the cycle's, and run() launches it
// on the cycle's stream - the lane's in lane mode, the back stream in staged mode - behind the Cartesian tail, with the lane's
// temporaries.  Member bodies after the S-T entry points (make_st_dev).
struct SpeedHalf {
    const emp_speed_dp_params* dp;
    const emp_speed_qp_params* qp;
    const emp_speed_io* io;
    int max_dyn;
    const double *dyn = nullptr, *heading = nullptr, *t0 = nullptr;
    const int *n_dyn = nullptr, *pre = nullptr;
    double *traj = nullptr, *i2s = nullptr, *seg = nullptr, *dp_speed = nullptr, *profile = nullptr;
    int* status = nullptr;
    void ins(Stage& st, int B);
    void outs(Stage& st, int B, int max_pts);
    int run(emp_ctx* ctx, Stage& st, int B, int max_pts, const double* d_traj, const int* d_tlen, const double* d_v,
            const double* d_a);
};
}  // namespace emp

// emp_plan_cycle's body; with `speed` (emp_plan_trajectory) the speed half runs behind the Cartesian tail, before the lane is done;
// `plain` (emp_drive, emp_drive_timed): EMP_OPT_CYCLE_GRAPH is neither used nor touched
static int plan_cycle_impl(emp_ctx* ctx, const emp_dp_params* p, const emp_qp_params* q, const emp_smooth_params* sp, int32_t B,
                           int32_t max_ref, int32_t max_obs, int32_t max_pts, emp_dp_mode mode, const emp_cycle_io* io,
                           emp_mem where, SpeedHalf* speed, bool plain = false) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, p && q && sp && io, "NULL parameter struct");
    EMP_REQUIRE(ctx, qp_reserved_ok(q), "emp_qp_params.reserved must be 0 (start from emp_qp_params_default)");
    // with a dynamic obstacle per scene (test_9.py:137-169) up to three virtual obstacles join the projected ones
    const bool has_dyn = io->dyn_dis_speed != nullptr;
    const int obs_cap = max_obs + (has_dyn ? 3 : 0);
    DpDev d;
    int rc = make_dp_dev(ctx, p, B, obs_cap, &d);
    if (rc) return rc;
    EMP_REQUIRE(ctx, max_ref >= 2 && max_pts >= 2 && max_pts <= 255, "max_ref >= 2 and 2 <= max_pts <= 255 required");
    // the optional front end (ABI 11): find_match_points on the global path, sampling, smooth_reference_line in front of the cycle
    const bool front = io->global_path != nullptr;
    EMP_REQUIRE(ctx, (front || (io->ref_line && io->n_ref)) && io->origin_xy && io->start_xy && io->start_v && io->start_a,
                "cycle inputs missing");
    EMP_REQUIRE(ctx, !front || (io->n_global && io->pre_match_index && io->match_index && io->ref_status && io->max_global >= 1 &&
                                max_ref == kRefLinePoints),
                "front end: n_global, pre_match_index, match_index, ref_status, max_global >= 1 and max_ref == EMP_REF_LINE_POINTS");
    EMP_REQUIRE(ctx, max_obs == 0 || (io->obs_xy && io->n_obs), "obstacle inputs missing");
    EMP_REQUIRE(ctx, io->traj && io->traj_len && io->status, "traj, traj_len and status are required outputs");
    EMP_REQUIRE(ctx, q->ds > 0, "ds must be > 0");
    EMP_HIP(ctx, hipSetDevice(ctx->device));
    const bool pinned = where == EMP_HOST_PINNED;
    const int pmode = ((where == EMP_DEVICE || pinned) && B > 0) ? ctx->pipe_mode : 0;
    CycleLane lane(ctx, pmode, pinned);
    if ((rc = lane.begin())) return rc;
    CycleCapture graph(ctx);
    bool replayed = false;
    // (the trajectory call is never captured: plain launches)
    if (!speed && !plain && ((rc = graph.begin(pmode, where, B, max_ref, max_obs, max_pts, mode, p, q, sp, io, &replayed)) || replayed)) return rc;
    // (the slot form of in() / out(): with EMP_HOST_PINNED the device pointers are known only at inputs_ready() / outputs_ready())
    Stage st(ctx, where, pmode != 0, pinned);
    const double *d_ref = nullptr, *d_o, *d_sxy, *d_v, *d_a, *d_oxy, *d_dyn, *d_glob = nullptr;
    const int *d_nr = nullptr, *d_no, *d_nglob = nullptr, *d_prem = nullptr;
    if (front) {
        st.in(io->global_path, (size_t)B * io->max_global * 4, &d_glob);
        st.in(io->n_global, (size_t)B, &d_nglob);
        st.in(io->pre_match_index, (size_t)B, &d_prem);
    } else {
        st.in(io->ref_line, (size_t)B * max_ref * 4, &d_ref);
        st.in(io->n_ref, (size_t)B, &d_nr);
    }
    st.in(io->origin_xy, (size_t)B * 2, &d_o);
    st.in(io->start_xy, (size_t)B * 2, &d_sxy);
    st.in(io->start_v, (size_t)B * 2, &d_v);
    st.in(io->start_a, (size_t)B * 2, &d_a);
    st.in(io->obs_xy, (size_t)B * max_obs * 2, &d_oxy);
    st.in(io->n_obs, (size_t)B, &d_no);
    st.in(io->dyn_dis_speed, (size_t)B * 2, &d_dyn);
    if (speed) speed->ins(st, B);
    st.inputs_ready();
    // outputs (optional ones fall back to device temporaries); no memsets: every kernel of the cycle writes its
    // rows completely, padding included
    double *d_rows, *d_dps, *d_dpl, *d_ps, *d_pl, *d_traj;
    int *d_dplen, *d_plen, *d_tlen, *d_st, *d_match = nullptr, *d_rst = nullptr;
    st.out_or_tmp(io->dp_rows, (size_t)B * d.col, &d_rows);
    st.out_or_tmp(io->dp_s, (size_t)B * max_pts, &d_dps);
    st.out_or_tmp(io->dp_l, (size_t)B * max_pts, &d_dpl);
    st.out_or_tmp(io->dp_len, (size_t)B, &d_dplen);
    st.out_or_tmp(io->path_s, (size_t)B * max_pts, &d_ps);
    st.out_or_tmp(io->path_l, (size_t)B * max_pts, &d_pl);
    st.out_or_tmp(io->path_len, (size_t)B, &d_plen);
    st.out(io->traj, (size_t)B * (max_pts + 1) * 4, &d_traj, false);
    st.out(io->traj_len, (size_t)B, &d_tlen, false);
    st.out(io->status, (size_t)B, &d_st, false);
    if (front) {
        st.out(io->match_index, (size_t)B, &d_match, false);
        st.out(io->ref_status, (size_t)B, &d_rst, false);
    }
    if (speed) speed->outs(st, B, max_pts);
    st.outputs_ready();
    // intermediates
    const int mo = obs_cap > 0 ? obs_cap : 1;
    double* d_sm = st.tmp<double>((size_t)B * max_ref);
    double* d_os = st.tmp<double>((size_t)B * mo);
    double* d_ol = st.tmp<double>((size_t)B * mo);
    double* d_bsl = st.tmp<double>((size_t)B * 2);
    double* d_start = st.tmp<double>((size_t)B * 4);
    if (max_obs == 0) d_no = st.tmp<int>((size_t)B, true);
    int* d_ntot = has_dyn ? st.tmp<int>((size_t)B) : nullptr;
    double* d_ref_w = front ? st.tmp<double>((size_t)B * kRefLinePoints * 4) : nullptr;
    int* d_nr_w = front ? st.tmp<int>((size_t)B) : nullptr;
    if ((rc = st.ready())) return rc;
    if (B == 0) return st.finish();
    if (front) {          // ref test_9.py:99-110, one wavefront per scene; the predicted location is the planning start
        if ((rc = dev_reference_line(ctx, sp, B, (int)io->max_global, d_glob, d_nglob, d_sxy, (const int*)nullptr, d_prem, d_ref_w,
                                     d_nr_w, d_match, (int*)nullptr, d_rst, 2)))
            return rc;
        d_ref = d_ref_w;
        d_nr = d_nr_w;
    }
    if ((rc = dev_project(ctx, B, max_ref, max_obs, d_ref, d_nr, d_o, d_sxy, d_v, d_a, d_oxy, d_no, d_sm, d_os, d_ol,
                          d_bsl, d_start, mo, d_dyn, d_ntot)))
        return rc;
    if (has_dyn) d_no = d_ntot;                            // downstream stages see the projected + virtual obstacles
    CycleSched cs;
    const bool two_kernel = mode == EMP_DP_TWO_KERNEL && !dp_wide(d);
    // the sweep may leave the backtrack to the densification kernel (emp_dp_kernels.h, BT == false): two temporaries for it
    if (two_kernel) {
        cs.bt_pre = st.tmp<unsigned char>((size_t)d.tiles * d.col * 64);
        cs.bt_term = st.tmp<int>((size_t)B);
        if ((rc = st.ready())) return rc;        // (staged behind the projection launch: checked here)
    }
    lane.front_waits(cs, two_kernel);
    if ((rc = dev_dp_plan(ctx, d, d_os, d_ol, d_no, d_start, mode, d_rows, nullptr, d_st, &cs))) return rc;
    const QpDev Q = make_qp_dev(q);
    if ((rc = lane.to_back(cs))) return rc;
    auto enrich = [&] {
        return dev_dp_enrich(ctx, d, d_rows, d_start, max_pts, d_dps, d_dpl, d_dplen, d_st, 1, &cs, cs.bt_deferred ? cs.bt_pre : nullptr,
                             cs.bt_deferred ? cs.bt_term : nullptr, d_no, d_rows);
    };
    auto path_qp = [&] {
        return dev_cycle_qp(ctx, B, max_pts, mo, Q, d_dps, d_dpl, d_dplen, d_os, d_ol, d_no, d_start, d_ps, d_pl, d_plen, d_st, &cs);
    };
    if ((rc = lane.signal(cs, ctx->opt[EMP_OPT_EDGE_AFTER_ENRICH] != 0, &emp_ctx::Lane::ev_enrich, &emp_ctx::Lane::enrich_valid, enrich))) return rc;
    if ((rc = lane.signal(cs, true, &emp_ctx::Lane::ev_qp, &emp_ctx::Lane::qp_valid, path_qp))) return rc;
    const int path_cap = (max_pts + Q.decimate - 1) / Q.decimate + (Q.midpoint ? 1 : 0);
    if ((rc = dev_cycle_cartesian(ctx, B, max_ref, max_pts, path_cap, sp, d_ref, d_sm, d_nr, d_bsl, d_ps, d_pl, d_plen,
                                  d_traj, d_tlen, d_st)))
        return rc;
    if (speed && (rc = speed->run(ctx, st, B, max_pts, d_traj, d_tlen, d_v, d_a))) return rc;
    if ((rc = lane.done(st))) return rc;
    if (st.async_host()) return EMP_OK;            // (finish_async has sent the outputs)
    if ((rc = graph.end())) return rc;
    return st.finish();
}

extern "C" {

int emp_plan_cycle(emp_ctx* ctx, const emp_dp_params* p, const emp_qp_params* q, const emp_smooth_params* sp, int32_t B,
                   int32_t max_ref, int32_t max_obs, int32_t max_pts, emp_dp_mode mode, const emp_cycle_io* io,
                   emp_mem where) {
    return plan_cycle_impl(ctx, p, q, sp, B, max_ref, max_obs, max_pts, mode, io, where, nullptr);
}

int64_t emp_cycle_graph_replays(emp_ctx* ctx) { return ctx ? (int64_t)ctx->cycle_graph.replays : -1; }

uint64_t emp_cycle_ticket(emp_ctx* ctx) { return ctx ? ctx->cycle_calls : 0; }

int emp_wait_cycle(emp_ctx* ctx, int32_t calls_back) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    if (!ctx->pipelined()) return EMP_OK;                       // a non-pipelined call returned with its outputs in place
    const int n = ctx->lanes_in_use();
    EMP_REQUIRE(ctx, calls_back >= 0 && calls_back < n, "calls_back beyond the pipeline depth");
    emp_ctx::Lane& ln = ctx->lanes[((ctx->lane - calls_back) % n + n) % n];
    if (ln.host_valid) EMP_HIP(ctx, hipEventSynchronize(ln.ev_host));
    return EMP_OK;
}

int emp_wait_ticket(emp_ctx* ctx, uint64_t ticket) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    // Reads two atomics per lane (emp_context.h Lane).  The lane's event exists since the call that got the ticket; a call
    // that takes the lane over waits - on the host - for that same event BEFORE it changes the lane's ticket, so a ticket that no
    // lane holds any more has been waited for already.  (A waiter that read the old ticket just before it changed waits for the
    // event as re-recorded by the new call: longer than needed, never shorter.)
    for (auto& ln : ctx->lanes)
        if (ln.ticket == ticket && ln.host_valid && ln.ev_host) {
            const hipError_t e = hipEventSynchronize(ln.ev_host);
            if (e != hipSuccess) return EMP_ERR_HIP;       // (no ctx->err write: another thread may be inside a call)
            break;
        }
    return EMP_OK;
}

int emp_host_alloc(emp_ctx* ctx, uint64_t bytes, void** out) {
    EMP_REQUIRE(ctx, ctx && out, "NULL argument");
    EMP_HIP(ctx, hipSetDevice(ctx->device));
    emp_ctx::HostBlock hb;
    if (const int rc = hb.ensure(ctx, bytes ? bytes : 8)) return rc;
    *out = hb.p;
    ctx->pinned.push_back(std::move(hb));
    return EMP_OK;
}
int emp_host_free(emp_ctx* ctx, void* ptr) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    auto it = std::find_if(ctx->pinned.begin(), ctx->pinned.end(), [&](const emp_ctx::HostBlock& a) { return a.p == ptr; });
    EMP_REQUIRE(ctx, it != ctx->pinned.end(), "not an emp_host_alloc pointer of this context");
    EMP_HIP(ctx, (hipError_t)sync_all(ctx));
    EMP_HIP(ctx, it->reset());
    ctx->pinned.erase(it);
    return EMP_OK;
}

int emp_quintic_coefficients(emp_ctx* ctx, int32_t n, const double* bc, double* coeff, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, n >= 0 && bc && coeff, "bad argument");
    EMP_STAGE(st, where);
    const double* d_bc = st.in(bc, (size_t)n * 8);
    double* d_c = st.out(coeff, (size_t)n * 6);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, quintic_kernel, grid1(n, 64), dim3(64), 0, n, d_bc, d_c)) return rc;
    return st.finish();
}

int emp_obs_cost_n(emp_ctx* ctx, int32_t n, int32_t samples, double w_collision, double danger_dis, double safe_dis,
                   const double* square_d, double* cost, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, n >= 0 && samples >= 0 && cost && (square_d || (size_t)n * samples == 0), "bad argument");
    EMP_STAGE(st, where);
    const double* d_sq = st.in(square_d, (size_t)n * samples);
    double* d_c = st.out(cost, (size_t)n);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, obs_cost_kernel, grid1(n, 64), dim3(64), 0, n, samples, w_collision, danger_dis,
                              safe_dis, d_sq, d_c))
        return rc;
    return st.finish();
}

int emp_obs_cost(emp_ctx* ctx, int32_t n, double w_collision, double danger_dis, double safe_dis, const double* square_d,
                 double* cost, emp_mem where) {
    return emp_obs_cost_n(ctx, n, kSamples, w_collision, danger_dis, safe_dis, square_d, cost, where);
}

int emp_free_edge_costs(emp_ctx* ctx, int32_t n, int32_t max_obs, const double* edges, const double* obs_s, const double* obs_l,
                        const int32_t* n_obs, double w_collision, const double* w_smooth3, double w_ref, double* cost, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, n >= 0 && max_obs >= 0 && edges && w_smooth3 && cost, "bad argument");
    EMP_REQUIRE(ctx, max_obs == 0 || (obs_s && obs_l && n_obs), "obs_s / obs_l / n_obs are required when max_obs > 0");
    const double w0 = w_smooth3[0], w1 = w_smooth3[1], w2 = w_smooth3[2];      // host memory, like the parameter structs
    EMP_STAGE(st, where);
    const double* d_e = st.in(edges, (size_t)n * 8);
    const double* d_os = st.in(obs_s, (size_t)n * max_obs);
    const double* d_ol = st.in(obs_l, (size_t)n * max_obs);
    const int* d_n = st.in(n_obs, (size_t)n);
    double* d_c = st.out(cost, (size_t)n);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, free_edge_cost_kernel, grid1(n, 64), dim3(64), 0, n, max_obs, d_e, d_os, d_ol, d_n,
                              w_collision, w0, w1, w2, w_ref, d_c))
        return rc;
    return st.finish();
}

}  // extern "C"

// ---- stand-alone projection helpers and the utilities beside the path ---------------------------
extern "C" {

int emp_s_map(emp_ctx* ctx, int32_t B, int32_t max_ref, const double* ref_line, const int32_t* n_ref,
              const double* origin_xy, double* s_map, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_ref >= 1 && ref_line && n_ref && origin_xy && s_map, "bad argument");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)B * max_ref * 4);
    const int* d_nr = st.in(n_ref, (size_t)B);
    const double* d_o = st.in(origin_xy, (size_t)B * 2);
    double* d_sm = st.out(s_map, (size_t)B * max_ref);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, s_map_kernel, grid1(B, 64), dim3(64), 0, B, max_ref, d_ref, d_nr, d_o, d_sm)) return rc;
    return st.finish();
}

int emp_s_l(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line, const double* s_map,
            const int32_t* n_ref, const double* xy, const int32_t* n_pts, const int32_t* match_index, double* s,
            double* l, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_ref >= 1 && max_pts >= 1 && ref_line && s_map && n_ref && xy && n_pts && s,
                "bad argument");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)B * max_ref * 4);
    const double* d_sm = st.in(s_map, (size_t)B * max_ref);
    const int* d_nr = st.in(n_ref, (size_t)B);
    const double* d_xy = st.in(xy, (size_t)B * max_pts * 2);
    const int* d_np = st.in(n_pts, (size_t)B);
    const int* d_mi = st.in(match_index, (size_t)B * max_pts);
    double* d_s = st.out(s, (size_t)B * max_pts);
    double* d_l = st.out(l, (size_t)B * max_pts);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, s_l_kernel, grid1(B, 64), dim3(64), 0, B, max_ref, max_pts, d_ref, d_sm, d_nr, d_xy,
                              d_np, d_mi, d_s, d_l))
        return rc;
    return st.finish();
}

int emp_s_l_deri(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                 const int32_t* n_ref, const double* xy, const double* v_xy, const double* a_xy, const int32_t* n_pts,
                 const double* origin_xy, double* out, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_ref >= 1 && max_pts >= 1 && ref_line && n_ref && xy && v_xy && a_xy && n_pts &&
                         origin_xy && out, "bad argument");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)B * max_ref * 4);
    const int* d_nr = st.in(n_ref, (size_t)B);
    const double* d_xy = st.in(xy, (size_t)B * max_pts * 2);
    const double* d_v = st.in(v_xy, (size_t)B * max_pts * 2);
    const double* d_a = st.in(a_xy, (size_t)B * max_pts * 2);
    const int* d_np = st.in(n_pts, (size_t)B);
    const double* d_o = st.in(origin_xy, (size_t)B * 2);
    double* d_out = st.out(out, (size_t)B * max_pts * 7);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, s_l_deri_kernel, grid1(B, 64), dim3(64), 0, B, max_ref, max_pts, d_ref, d_nr, d_xy, d_v,
                              d_a, d_np, d_o, d_out))
        return rc;
    return st.finish();
}

int emp_proj_point(emp_ctx* ctx, int32_t n, int32_t max_ref, const double* ref_line, const double* s_map,
                   const int32_t* n_ref, const double* s, const int32_t* pre_match_index, double* out, int32_t* index,
                   int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, n >= 0 && max_ref >= 1 && ref_line && s_map && n_ref && s && pre_match_index && out && index &&
                         status, "bad argument");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)n * max_ref * 4);
    const double* d_sm = st.in(s_map, (size_t)n * max_ref);
    const int* d_nr = st.in(n_ref, (size_t)n);
    const double* d_s = st.in(s, (size_t)n);
    const int* d_pre = st.in(pre_match_index, (size_t)n);
    double* d_out = st.out(out, (size_t)n * 4);
    int* d_idx = st.out(index, (size_t)n);
    int* d_st = st.out(status, (size_t)n);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, proj_point_kernel, grid1(n, 64), dim3(64), 0, n, max_ref, d_ref, d_sm, d_nr, d_s, d_pre,
                              d_out, d_idx, d_st))
        return rc;
    return st.finish();
}

int emp_trajectory_index2s(emp_ctx* ctx, int32_t B, int32_t max_pts, const double* x, const double* y,
                           const int32_t* n_pts, double* index2s, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_pts >= 1 && x && y && n_pts && index2s, "bad argument");
    EMP_STAGE(st, where);
    const double* d_x = st.in(x, (size_t)B * max_pts);
    const double* d_y = st.in(y, (size_t)B * max_pts);
    const int* d_np = st.in(n_pts, (size_t)B);
    double* d_o = st.out(index2s, (size_t)B * max_pts);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, index2s_kernel, grid1(B, 64), dim3(64), 0, B, max_pts, d_x, d_y, d_np, d_o)) return rc;
    return st.finish();
}

int emp_frenet2cartesian(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                         const double* index2s, const int32_t* n_ref, const double* sl, const int32_t* n_pts,
                         double* out, int32_t* status, int32_t proj_only, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_ref >= 2 && max_pts >= 1 && ref_line && index2s && n_ref && sl && n_pts && out &&
                         status, "bad argument");
    EMP_STAGE(st, where);
    const double* d_ref = st.in(ref_line, (size_t)B * max_ref * 4);
    const double* d_i2s = st.in(index2s, (size_t)B * max_ref);
    const int* d_nr = st.in(n_ref, (size_t)B);
    const double* d_sl = st.in(sl, (size_t)B * max_pts * 4);
    const int* d_np = st.in(n_pts, (size_t)B);
    double* d_out = st.out(out, (size_t)B * max_pts * 4);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, frenet2cartesian_kernel, grid1(B, 64), dim3(64), 0, B, max_ref, max_pts, d_ref, d_i2s,
                              d_nr, d_sl, d_np, d_out, d_st, proj_only))
        return rc;
    return st.finish();
}

int emp_dy_obs_deri(emp_ctx* ctx, int32_t n, const double* in, double* out, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, n >= 0 && in && out, "bad argument");
    EMP_STAGE(st, where);
    const double* d_in = st.in(in, (size_t)n * 5);
    double* d_out = st.out(out, (size_t)n * 3);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, dy_obs_deri_kernel, grid1(n, 64), dim3(64), 0, n, d_in, d_out)) return rc;
    return st.finish();
}

}  // extern "C"

extern "C" int emp_enrich_nodes(emp_ctx* ctx, int32_t B, int32_t max_nodes, double resolution, const double* node_s,
                                const double* node_l, const int32_t* n_nodes, const double* start, int32_t max_pts,
                                double* path_s, double* path_l, int32_t* path_len, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_nodes >= 1 && max_pts >= 1 && resolution > 0, "bad sizes");
    EMP_REQUIRE(ctx, node_s && node_l && n_nodes && start && path_s && path_l && path_len && status, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_ns = st.in(node_s, (size_t)B * max_nodes);
    const double* d_nl = st.in(node_l, (size_t)B * max_nodes);
    const int* d_nn = st.in(n_nodes, (size_t)B);
    const double* d_start = st.in(start, (size_t)B * 4);
    double* d_ps = st.out(path_s, (size_t)B * max_pts);
    double* d_pl = st.out(path_l, (size_t)B * max_pts);
    int* d_len = st.out(path_len, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, enrich_nodes_kernel, grid1(B, 64), dim3(64), 0, B, max_nodes, resolution, d_ns, d_nl,
                              d_nn, d_start, max_pts, d_ps, d_pl, d_len, d_st))
        return rc;
    return st.finish();
}

// ---- S-T speed DP (reference planner/speed_planning_test.py) ------------------------------------
extern "C" {

void emp_speed_dp_params_default(emp_speed_dp_params* p) {
    if (!p) return;
    p->reference_speed = 50.0;
    p->w_cost_ref_speed = 4000.0;
    p->w_cost_accel = 100.0;
    p->w_cost_obs = 10000000.0;
}

static emp::StDev make_st_dev(const emp_speed_dp_params* p, int B, int max_obs) {
    emp::StDev d;
    d.B = B;
    d.max_obs = max_obs;
    d.w.v_ref = p->reference_speed;
    d.w.w_ref = p->w_cost_ref_speed;
    d.w.w_acc = p->w_cost_accel;
    d.w.w_obs = emp::st::make_pow_base(p->w_cost_obs);
    return d;
}

// ---- device-level launchers of the speed stages (as dev_project: device pointers, nothing of the caller's checked, no sync) ----
// The speed DP takes its heaviest scenes first (emp_st_kernels.h: st_count_kernel) beyond this many: pointless while every block
// is resident at once.  The caller stages the ordering's temporaries before its Stage::ready().
constexpr int kStOrderAbove = 512;
struct StOrderTmp {
    int* order = nullptr;
    unsigned char* key = nullptr;
    int* hist = nullptr;
};
static StOrderTmp st_order_tmp(Stage& st, int B) {
    if (B <= kStOrderAbove) return {};
    int* order = st.tmp<int>((size_t)B);
    unsigned char* key = st.tmp<unsigned char>((size_t)B);
    return {order, key, st.tmp<int>(2 * (size_t)kStKeys, true)};
}

static int dev_speed_dp(emp_ctx* ctx, const emp_speed_dp_params* p, int B, int max_obs, const double* s_in, const double* s_out,
                        const double* t_in, const double* t_out, const double* v_start, double* cost, double* s_dot, int* node,
                        int* end_node, double* speed_s, double* speed_t, const StOrderTmp& o) {
    if (o.order) {           // two launches, one timing interval
        if (const int rc = launch_gate(ctx)) return rc;
        KernelTimer t(ctx, "speed_dp_order");
        hipLaunchKernelGGL(st_count_kernel, grid1(B, 256), dim3(256), 0, ctx->stream, B, max_obs, s_in, o.key, o.hist);
        hipLaunchKernelGGL(st_scatter_kernel, grid1(B, 256), dim3(256), 0, ctx->stream, B, o.key, o.hist, o.hist + kStKeys, o.order);
        EMP_LAUNCH_CHECK(ctx);
    }
    const TailPlan plan = plan_speed_dp(B, max_obs);
    return launch_plan(ctx, "speed_dp", plan, plan.m32 ? speed_dp_kernel<uint32_t> : speed_dp_kernel<uint64_t>, make_st_dev(p, B, max_obs),
                       s_in, s_out, t_in, t_out, v_start, cost, s_dot, node, end_node, speed_s, speed_t, (const int*)o.order);
}

constexpr double kDefaultMaxLateralAccel = 0.2 * 9.8;       // ref: generate_convex_space's default, speed_planning_test.py:309
static int dev_speed_convex_space(emp_ctx* ctx, int B, int n_slots, int max_path, double max_lateral_accel, const double* dp_s,
                                  const double* dp_t, const double* index2s, const double* kappa, const int* path_len,
                                  const double* s_in, const double* s_out, const double* t_in, const double* t_out, double* s_lb,
                                  double* s_ub, double* sd_lb, double* sd_ub, int* status) {
    return launch(ctx, "speed_convex_space", stb::convex_space_kernel, grid1(B, 64), dim3(64), 0, B, n_slots, max_path,
                  max_lateral_accel, dp_s, dp_t, index2s, kappa, path_len, s_in, s_out, t_in, t_out, s_lb, s_ub, sd_lb, sd_ub, status);
}

static int dev_speed_qp(emp_ctx* ctx, const emp_speed_qp_params* p, int B, const double* v0, const double* a0, const double* dp_s,
                        const double* dp_t, const double* s_lb, const double* s_ub, const double* sd_lb, const double* sd_ub,
                        double* qs, double* qv, double* qa, double* qt, int* iters, int* status) {
    const stb::SpeedQpParams prm{p->w_cost_s_dot2, p->w_cost_v_ref, p->w_cost_jerk, p->reference_speed};
    return launch_plan(ctx, "speed_qp", plan_speed_qp(B), stb::speed_qp_kernel<32>, B, prm, v0, a0, dp_s, dp_t, s_lb, s_ub, sd_lb, sd_ub,
                       qs, qv, qa, qt, iters, status);
}

static int dev_speed_increase_points(emp_ctx* ctx, int B, const double* qs, const double* qv, const double* qa, const double* qt,
                                     double* s, double* v, double* a, double* t, int* status) {
    return launch(ctx, "speed_increase_points", stb::densify_kernel, dim3(B), dim3(64), 0, B, qs, qv, qa, qt, s, v, a, t, status);
}

static int dev_path_speed_merge(emp_ctx* ctx, int B, int max_path, const double* s, const double* v, const double* a, const double* t,
                                const double* now, const double* path_s, const double* x, const double* y, const double* heading,
                                const double* kappa, const int* n_init, double* trajectory, int* status) {
    return launch_plan(ctx, "path_speed_merge", plan_merge(B, max_path), stb::merge_kernel, B, max_path, s, v, a, t, now, path_s, x, y,
                       heading, kappa, n_init, trajectory, status);
}

int emp_st_graph(emp_ctx* ctx, int32_t B, int32_t max_obs, const double* obs_s, const double* obs_l,
                 const double* obs_s_dot, const double* obs_l_dot, double* s_in, double* s_out, double* t_in,
                 double* t_out, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_obs >= 1, "bad sizes");
    EMP_REQUIRE(ctx, obs_s && obs_l && obs_s_dot && obs_l_dot && s_in && s_out && t_in && t_out, "NULL argument");
    EMP_STAGE(st, where);
    const size_t n = (size_t)B * max_obs;
    const double* d_s = st.in(obs_s, n);
    const double* d_l = st.in(obs_l, n);
    const double* d_sd = st.in(obs_s_dot, n);
    const double* d_ld = st.in(obs_l_dot, n);
    double* d_si = st.out(s_in, n, false);
    double* d_so = st.out(s_out, n, false);
    double* d_ti = st.out(t_in, n, false);
    double* d_to = st.out(t_out, n, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "st_graph", st_graph_kernel, grid1(B, 64), dim3(64), 0, B, max_obs, d_s, d_l, d_sd, d_ld, d_si,
                              d_so, d_ti, d_to))
        return rc;
    return st.finish();
}

int emp_speed_dp(emp_ctx* ctx, const emp_speed_dp_params* p, int32_t B, int32_t max_obs, const double* s_in,
                 const double* s_out, const double* t_in, const double* t_out, const double* plan_start_s_dot,
                 double* cost, double* s_dot, int32_t* node, int32_t* end_node, double* speed_s, double* speed_t,
                 emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, p != nullptr, "speed dp params are NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_obs >= 1 && max_obs <= st::kMaxObs, "bad sizes (max_obs must be in [1, 64])");
    EMP_REQUIRE(ctx, s_in && s_out && t_in && t_out && plan_start_s_dot && end_node && speed_s && speed_t, "NULL argument");
    // ref :281 w_cost_obs ** (1.5 - d): complex for a negative base, and the reference fails on its next comparison
    EMP_REQUIRE(ctx, !(p->w_cost_obs < 0.0), "w_cost_obs must not be negative");
    EMP_STAGE(st, where);
    const size_t n = (size_t)B * max_obs, nt = (size_t)B * emp::st::kRows * emp::st::kCols;
    const double* d_si = st.in(s_in, n);
    const double* d_so = st.in(s_out, n);
    const double* d_ti = st.in(t_in, n);
    const double* d_to = st.in(t_out, n);
    const double* d_v = st.in(plan_start_s_dot, (size_t)B);
    double* d_c = st.out(cost, nt, false);
    double* d_sd = st.out(s_dot, nt, false);
    int* d_n = st.out(node, nt, false);
    int* d_e = st.out(end_node, (size_t)B * 2, false);
    double* d_ss = st.out(speed_s, (size_t)B * emp::st::kCols, false);
    double* d_tt = st.out(speed_t, (size_t)B * emp::st::kCols, false);
    const StOrderTmp order = st_order_tmp(st, B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_speed_dp(ctx, p, B, max_obs, d_si, d_so, d_ti, d_to, d_v, d_c, d_sd, d_n, d_e, d_ss, d_tt, order)) return rc;
    return st.finish();
}

int emp_st_edge_costs(emp_ctx* ctx, const emp_speed_dp_params* p, int32_t B, int32_t n_edges, int32_t max_obs,
                      const double* edges, const double* s_in, const double* s_out, const double* t_in,
                      const double* t_out, double* total, double* obs, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, p != nullptr, "speed dp params are NULL");
    EMP_REQUIRE(ctx, B >= 0 && B <= 65535 && n_edges >= 0 && max_obs >= 1 && max_obs <= st::kMaxObs,
                "bad sizes (B <= 65535, max_obs in [1, 64])");
    EMP_REQUIRE(ctx, edges && s_in && s_out && t_in && t_out && total, "NULL argument");
    EMP_STAGE(st, where);
    const size_t n = (size_t)B * max_obs, ne = (size_t)B * n_edges;
    const double* d_e = st.in(edges, ne * 5);
    const double* d_si = st.in(s_in, n);
    const double* d_so = st.in(s_out, n);
    const double* d_ti = st.in(t_in, n);
    const double* d_to = st.in(t_out, n);
    double* d_t = st.out(total, ne, false);
    double* d_o = st.out(obs, ne, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch_plan(ctx, nullptr, plan_st_edge_cost(B, n_edges, max_obs), st_edge_cost_kernel, make_st_dev(p, B, max_obs),
                                   n_edges, d_e, d_si, d_so, d_ti, d_to, d_t, d_o))
        return rc;
    return st.finish();
}

int emp_st_collision_cost(emp_ctx* ctx, int32_t n, double w_cost_obs, const double* min_dis, double* cost, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, n >= 0 && min_dis && cost, "bad argument");
    EMP_STAGE(st, where);
    const double* d_d = st.in(min_dis, (size_t)n);
    double* d_c = st.out(cost, (size_t)n, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, st_collision_cost_kernel, grid1(n, 64), dim3(64), 0, n, emp::st::make_pow_base(w_cost_obs),
                              d_d, d_c))
        return rc;
    return st.finish();
}

int emp_speed_start_condition(emp_ctx* ctx, int32_t n, const double* vx, const double* vy, const double* ax, const double* ay,
                              const double* heading, double* s_dot, double* s_dot2, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, n >= 0 && vx && vy && ax && ay && heading && s_dot && s_dot2, "bad argument");
    EMP_STAGE(st, where);
    const double* d_vx = st.in(vx, (size_t)n);
    const double* d_vy = st.in(vy, (size_t)n);
    const double* d_ax = st.in(ax, (size_t)n);
    const double* d_ay = st.in(ay, (size_t)n);
    const double* d_h = st.in(heading, (size_t)n);
    double* d_s1 = st.out(s_dot, (size_t)n, false);
    double* d_s2 = st.out(s_dot2, (size_t)n, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, nullptr, st_start_condition_kernel, grid1(n, 64), dim3(64), 0, n, d_vx, d_vy, d_ax, d_ay, d_h,
                              d_s1, d_s2))
        return rc;
    return st.finish();
}

// ---- S-T speed planning back end (reference speed_planning_test.py:308-620) ---------------------
void emp_speed_qp_params_default(emp_speed_qp_params* p) {
    if (!p) return;
    // ref: speed_QP keyword defaults, speed_planning_test.py:410-411
    p->w_cost_s_dot2 = 10.0;
    p->w_cost_v_ref = 50.0;
    p->w_cost_jerk = 500.0;
    p->reference_speed = 50.0;
}

int emp_speed_convex_space(emp_ctx* ctx, int32_t B, int32_t n_slots, int32_t max_path, double max_lateral_accel,
                           const double* dp_speed_s, const double* dp_speed_t, const double* path_index2s,
                           const double* path_kappa, const int32_t* path_len, const double* s_in, const double* s_out,
                           const double* t_in, const double* t_out, double* s_lb, double* s_ub, double* s_dot_lb,
                           double* s_dot_ub, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && n_slots >= 1 && max_path >= 1, "bad sizes");
    EMP_REQUIRE(ctx, dp_speed_s && dp_speed_t && path_index2s && path_kappa && path_len && s_in && s_out && t_in && t_out &&
                         s_lb && s_ub && s_dot_lb && s_dot_ub && status, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_ds = st.in(dp_speed_s, (size_t)B * stb::kDp);
    const double* d_dt = st.in(dp_speed_t, (size_t)B * stb::kDp);
    const double* d_i2s = st.in(path_index2s, (size_t)B * max_path);
    const double* d_k = st.in(path_kappa, (size_t)B * max_path);
    const int* d_pl = st.in(path_len, (size_t)B);
    const double* d_si = st.in(s_in, (size_t)B * n_slots);
    const double* d_so = st.in(s_out, (size_t)B * n_slots);
    const double* d_ti = st.in(t_in, (size_t)B * n_slots);
    const double* d_to = st.in(t_out, (size_t)B * n_slots);
    double* d_lb = st.out(s_lb, (size_t)B * stb::kDp, false);
    double* d_ub = st.out(s_ub, (size_t)B * stb::kDp, false);
    double* d_vlb = st.out(s_dot_lb, (size_t)B * stb::kDp, false);
    double* d_vub = st.out(s_dot_ub, (size_t)B * stb::kDp, false);
    int* d_st = st.out(status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_speed_convex_space(ctx, B, n_slots, max_path, max_lateral_accel, d_ds, d_dt, d_i2s, d_k, d_pl, d_si, d_so,
                                              d_ti, d_to, d_lb, d_ub, d_vlb, d_vub, d_st))
        return rc;
    return st.finish();
}

int emp_speed_qp(emp_ctx* ctx, const emp_speed_qp_params* p, int32_t B, const double* plan_start_s_dot,
                 const double* plan_start_s_dot2, const double* dp_speed_s, const double* dp_speed_t, const double* s_lb,
                 const double* s_ub, const double* s_dot_lb, const double* s_dot_ub, double* qp_s, double* qp_s_dot,
                 double* qp_s_dot2, double* relative_time, int32_t* iters, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, p != nullptr && B >= 0, "bad argument");
    EMP_REQUIRE(ctx, plan_start_s_dot && plan_start_s_dot2 && dp_speed_s && dp_speed_t && s_lb && s_ub && s_dot_lb && s_dot_ub &&
                         qp_s && qp_s_dot && qp_s_dot2 && relative_time && status, "NULL argument");
    EMP_REQUIRE(ctx, p->w_cost_s_dot2 > 0 && p->w_cost_v_ref > 0 && p->w_cost_jerk >= 0, "weights must be positive");
    EMP_STAGE(st, where);
    const double* d_v0 = st.in(plan_start_s_dot, (size_t)B);
    const double* d_a0 = st.in(plan_start_s_dot2, (size_t)B);
    const double* d_ds = st.in(dp_speed_s, (size_t)B * stb::kDp);
    const double* d_dt = st.in(dp_speed_t, (size_t)B * stb::kDp);
    const double* d_lb = st.in(s_lb, (size_t)B * stb::kDp);
    const double* d_ub = st.in(s_ub, (size_t)B * stb::kDp);
    const double* d_vlb = st.in(s_dot_lb, (size_t)B * stb::kDp);
    const double* d_vub = st.in(s_dot_ub, (size_t)B * stb::kDp);
    double* d_qs = st.out(qp_s, (size_t)B * stb::kQp, false);
    double* d_qv = st.out(qp_s_dot, (size_t)B * stb::kQp, false);
    double* d_qa = st.out(qp_s_dot2, (size_t)B * stb::kQp, false);
    double* d_qt = st.out(relative_time, (size_t)B * stb::kQp, false);
    int* d_it = st.out(iters, (size_t)B, false);
    int* d_st = st.out(status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_speed_qp(ctx, p, B, d_v0, d_a0, d_ds, d_dt, d_lb, d_ub, d_vlb, d_vub, d_qs, d_qv, d_qa, d_qt, d_it, d_st))
        return rc;
    return st.finish();
}

int emp_speed_increase_points(emp_ctx* ctx, int32_t B, const double* s_init, const double* s_dot_init,
                              const double* s_dot2_init, const double* relative_time_init, double* s, double* s_dot,
                              double* s_dot2, double* relative_time, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && s_init && s_dot_init && s_dot2_init && relative_time_init && s && s_dot && s_dot2 &&
                         relative_time && status, "bad argument");
    EMP_STAGE(st, where);
    const double* d_qs = st.in(s_init, (size_t)B * stb::kQp);
    const double* d_qv = st.in(s_dot_init, (size_t)B * stb::kQp);
    const double* d_qa = st.in(s_dot2_init, (size_t)B * stb::kQp);
    const double* d_qt = st.in(relative_time_init, (size_t)B * stb::kQp);
    double* d_s = st.out(s, (size_t)B * stb::kDense, false);
    double* d_v = st.out(s_dot, (size_t)B * stb::kDense, false);
    double* d_a = st.out(s_dot2, (size_t)B * stb::kDense, false);
    double* d_t = st.out(relative_time, (size_t)B * stb::kDense, false);
    int* d_st = st.out(status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_speed_increase_points(ctx, B, d_qs, d_qv, d_qa, d_qt, d_s, d_v, d_a, d_t, d_st)) return rc;
    return st.finish();
}

int emp_path_speed_merge(emp_ctx* ctx, int32_t B, int32_t max_path, const double* s, const double* s_dot,
                         const double* s_dot2, const double* relative_time, const double* current_time,
                         const double* path_s, const double* x_init, const double* y_init, const double* heading_init,
                         const double* kappa_init, const int32_t* n_init, double* trajectory, int32_t* status,
                         emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B >= 0 && max_path >= 1, "bad sizes");
    EMP_REQUIRE(ctx, s && s_dot && s_dot2 && relative_time && current_time && path_s && x_init && y_init && heading_init &&
                         kappa_init && n_init && trajectory && status, "NULL argument");
    if (const int rc = plan_refused(ctx, plan_merge(B, max_path).error)) return rc;      // (kMergeLdsBytes) before anything is staged
    EMP_STAGE(st, where);
    const double* d_s = st.in(s, (size_t)B * stb::kDense);
    const double* d_v = st.in(s_dot, (size_t)B * stb::kDense);
    const double* d_a = st.in(s_dot2, (size_t)B * stb::kDense);
    const double* d_t = st.in(relative_time, (size_t)B * stb::kDense);
    const double* d_now = st.in(current_time, (size_t)B);
    const double* d_ps = st.in(path_s, (size_t)B * max_path);
    const double* d_x = st.in(x_init, (size_t)B * max_path);
    const double* d_y = st.in(y_init, (size_t)B * max_path);
    const double* d_h = st.in(heading_init, (size_t)B * max_path);
    const double* d_k = st.in(kappa_init, (size_t)B * max_path);
    const int* d_n = st.in(n_init, (size_t)B);
    double* d_out = st.out(trajectory, (size_t)B * 7 * stb::kDense, false);
    int* d_st = st.out(status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = dev_path_speed_merge(ctx, B, max_path, d_s, d_v, d_a, d_t, d_now, d_ps, d_x, d_y, d_h, d_k, d_n, d_out, d_st))
        return rc;
    return st.finish();
}

}  // extern "C"

// ---- path cycle + S-T speed planner in one call (reference test_10.py:99-340) ---------------------
namespace emp {

void SpeedHalf::ins(Stage& st, int B) {
    dyn = st.in(io->dyn_obs, (size_t)B * max_dyn * 4);
    n_dyn = st.in(io->n_dyn, (size_t)B);
    heading = st.in(io->start_heading, (size_t)B);
    t0 = st.in(io->plan_start_time, (size_t)B);
    pre = st.in(io->dyn_pre_match, (size_t)B);
}

void SpeedHalf::outs(Stage& st, int B, int max_pts) {
    const size_t W = (size_t)max_pts + 2;
    traj = st.out(io->trajectory, (size_t)B * 7 * stb::kDense, false);
    status = st.out(io->speed_status, (size_t)B, false);
    st.out_or_tmp(io->path_index2s, (size_t)B * W, &i2s);
    st.out_or_tmp(io->st_segments, (size_t)B * 4 * max_dyn, &seg);
    st.out_or_tmp(io->dp_speed, (size_t)B * 2 * stb::kDp, &dp_speed);
    st.out_or_tmp(io->speed_profile, (size_t)B * 4 * stb::kQp, &profile);
}

int SpeedHalf::run(emp_ctx* ctx, Stage& st, int B, int max_pts, const double* d_traj, const int* d_tlen, const double* d_v,
                   const double* d_a) {
    const int W = max_pts + 2;
    const size_t nb = (size_t)B, bw = nb * W;
    double* rows = st.tmp<double>(4 * bw);
    double* v0 = st.tmp<double>(nb);
    double* a0 = st.tmp<double>(nb);
    int* width = st.tmp<int>(nb);
    int* st_front = st.tmp<int>(nb);
    int* end_node = st.tmp<int>(2 * nb);
    double* cs = st.tmp<double>(4 * nb * stb::kDp);
    int* st_cs = st.tmp<int>(nb);
    double* qp4 = profile;
    int* st_qp = st.tmp<int>(nb);
    double* dense = st.tmp<double>(4 * nb * stb::kDense);
    int* st_dense = st.tmp<int>(nb);
    int* st_merge = st.tmp<int>(nb);
    const StOrderTmp order = st_order_tmp(st, B);
    if (const int rc = st.ready()) return rc;          // (temporaries staged behind the cycle's launches: checked here)
    const size_t sp = nb * max_dyn, n16 = nb * stb::kDp, n17 = nb * stb::kQp, n401 = nb * stb::kDense;
    const double *si = seg, *so = seg + sp, *ti = seg + 2 * sp, *to = seg + 3 * sp;
    double *ds = dp_speed, *dt = dp_speed + n16;
    const double* kappa = rows + 3 * bw;
    int rc;
    if ((rc = launch_plan(ctx, "speed_front", plan_speed_front(B, W), speed_front_wave_kernel, B, max_pts, W, max_dyn, d_traj, d_tlen,
                          d_v, d_a, heading, dyn, n_dyn, pre, rows, i2s, v0, a0, seg, width, st_front)))
        return rc;
    if ((rc = dev_speed_dp(ctx, dp, B, max_dyn, si, so, ti, to, v0, nullptr, nullptr, nullptr, end_node, ds, dt, order))) return rc;
    // generate_convex_space on the W-wide rows; path_len = merge width: W, or 0 for a scene that already raised
    if ((rc = dev_speed_convex_space(ctx, B, max_dyn, W, kDefaultMaxLateralAccel, ds, dt, i2s, kappa, width, si, so, ti, to, cs,
                                     cs + n16, cs + 2 * n16, cs + 3 * n16, st_cs)))
        return rc;
    if ((rc = dev_speed_qp(ctx, qp, B, v0, a0, ds, dt, cs, cs + n16, cs + 2 * n16, cs + 3 * n16, qp4, qp4 + n17, qp4 + 2 * n17,
                           qp4 + 3 * n17, nullptr, st_qp)))
        return rc;
    if ((rc = dev_speed_increase_points(ctx, B, qp4, qp4 + n17, qp4 + 2 * n17, qp4 + 3 * n17, dense, dense + n401, dense + 2 * n401,
                                        dense + 3 * n401, st_dense)))
        return rc;
    if ((rc = dev_path_speed_merge(ctx, B, W, dense, dense + n401, dense + 2 * n401, dense + 3 * n401, t0, i2s, rows, rows + bw,
                                   rows + 2 * bw, kappa, width, traj, st_merge)))
        return rc;
    return launch(ctx, "speed_status", speed_status_kernel, grid1(B, 64), dim3(64), 0, B, (const int*)st_front, (const int*)st_cs,
                  (const int*)st_qp, (const int*)st_dense, (const int*)st_merge, status);
}

}  // namespace emp

// the speed planner's parameter checks, behind the caller's own for NULL structs (emp_plan_trajectory, emp_drive_timed)
static int speed_params_ok(emp_ctx* ctx, const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp) {
    EMP_REQUIRE(ctx, !(sdp->w_cost_obs < 0.0), "w_cost_obs must not be negative");
    EMP_REQUIRE(ctx, sqp->w_cost_s_dot2 > 0 && sqp->w_cost_v_ref > 0 && sqp->w_cost_jerk >= 0, "speed QP weights must be positive");
    return EMP_OK;
}

extern "C" int emp_plan_trajectory(emp_ctx* ctx, const emp_dp_params* p, const emp_qp_params* q, const emp_smooth_params* sp,
                                   const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp, int32_t B, int32_t max_ref,
                                   int32_t max_obs, int32_t max_pts, int32_t max_dyn, emp_dp_mode mode, const emp_cycle_io* io,
                                   const emp_speed_io* sio, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, sdp && sqp && sio, "NULL speed parameter struct or emp_speed_io");
    EMP_REQUIRE(ctx, sio->reserved == 0, "emp_speed_io.reserved must be 0");
    EMP_REQUIRE(ctx, max_dyn >= 1 && max_dyn <= st::kMaxObs, "max_dyn must be in [1, 64] (the speed DP's obstacle slots)");
    EMP_REQUIRE(ctx, where != EMP_HOST_PINNED, "emp_plan_trajectory does not take EMP_HOST_PINNED arrays (HostRing slots carry the "
                                               "cycle's layout only): use EMP_HOST or EMP_DEVICE");
    EMP_REQUIRE(ctx, sio->dyn_obs && sio->n_dyn && sio->start_heading && sio->plan_start_time,
                "dyn_obs, n_dyn, start_heading and plan_start_time are required inputs");
    EMP_REQUIRE(ctx, sio->trajectory && sio->speed_status, "trajectory and speed_status are required outputs");
    if (const int rc = speed_params_ok(ctx, sdp, sqp)) return rc;
    SpeedHalf speed{sdp, sqp, sio, (int)max_dyn};
    return plan_cycle_impl(ctx, p, q, sp, B, max_ref, max_obs, max_pts, mode, io, where, &speed);
}

// ---- lateral MPC controller (reference controller/controller.py:65-337) -------------------------
extern "C" {

void emp_mpc_params_default(emp_mpc_params* p) {
    if (!p) return;
    // the driver's tuple (1.015, 2.910 - 1.015, 1412, -148970, -82204, 1537) (ref test_9.py:316) as the controller
    // unpacks it: (a, b, Cf, Cr, m, Iz) = vehicle_para (ref controller.py:132)
    p->a = 1.015;
    p->b = 2.910 - 1.015;
    p->Cf = 1412.0;
    p->Cr = -148970.0;
    p->m = -82204.0;
    p->Iz = 1537.0;
    const double q[4] = {250.0, 1.0, 50.0, 1.0};
    for (int i = 0; i < 4; ++i) {
        p->q_diag[i] = q[i];
        p->f_diag[i] = 1.0;
    }
    p->r = 1.0;
}

static mpc::Params mpc_params(const emp_mpc_params* p) {
    mpc::Params prm;
    prm.a = p->a; prm.b = p->b; prm.Cf = p->Cf; prm.Cr = p->Cr; prm.m = p->m; prm.Iz = p->Iz;
    for (int i = 0; i < 4; ++i) {
        prm.q[i] = p->q_diag[i];
        prm.f[i] = p->f_diag[i];
    }
    prm.r = p->r;
    return prm;
}

}  // extern "C"

// The one launch of a lateral law chosen at run time (emp_vehicle_control, the rollouts, emp_drive), timed under `name`: the MPC
// kernel with kGroupsPerWave vehicle groups per wavefront or the LQR kernel with one vehicle per lane, each with its argument list.
template <typename KM, typename KL, typename... AM, typename... AL>
static int launch_lateral(emp_ctx* ctx, const char* name, int lateral, int B, KM mpc_kern, KL lqr_kern, const std::tuple<AM...>& mpc_args,
                          const std::tuple<AL...>& lqr_args) {
    const auto go = [&](auto kern, dim3 grid, const auto& args) {
        return std::apply([&](auto... a) { return launch(ctx, name, kern, grid, dim3(64), 0, a...); }, args);
    };
    return lateral == EMP_LAT_MPC ? go(mpc_kern, grid_groups(B, mpc::kGroupsPerWave), mpc_args) : go(lqr_kern, grid1(B, 64), lqr_args);
}

// Stage and launch a stand-alone lateral law (emp_mpc_lateral, emp_mpc_ff_lateral, emp_lqr_lateral): one vehicle per group of `lanes`
// lanes, 64 / lanes groups per wavefront.  `gain` is the law's own [B][n_gain] output (the MPCs' controls u, the LQR's K) and `iters`
// its count (QP iterations, Riccati sweeps); HF: the kernel also writes the condensed problem, H [n_gain x n_gain] and f [n_gain].
// `tail`: what the kernel takes after status (the fused epilogue's CtlIO, or nothing).
template <bool HF, typename K, typename... Tail>
static int stage_lateral(emp_ctx* ctx, const char* name, K kern, int lanes, int n_gain, const emp_mpc_params* p, int B, int max_path,
                         const double* target_path, const int32_t* n_path, const double* state, const double* vx,
                         const int32_t* min_index, double* steer, double* gain, double* e_rr, double* k_r, int32_t* min_index_out,
                         double* pre_pro, double* H, double* f, int32_t* iters, int32_t* status, emp_mem where, Tail... tail) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, p && B >= 0 && max_path >= 1, "bad sizes");
    EMP_REQUIRE(ctx, target_path && n_path && state && vx && min_index && steer && min_index_out && status, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_path = st.in(target_path, (size_t)B * max_path * 4);
    const int* d_np = st.in(n_path, (size_t)B);
    const double* d_state = st.in(state, (size_t)B * 5);
    const double* d_vx = st.in(vx, (size_t)B);
    const int* d_mi = st.in(min_index, (size_t)B);
    double* d_steer = st.out(steer, (size_t)B, false);
    double* d_g = st.out(gain, (size_t)B * n_gain, false);
    double* d_e = st.out(e_rr, (size_t)B * 4, false);
    double* d_k = st.out(k_r, (size_t)B, false);
    int* d_mo = st.out(min_index_out, (size_t)B, false);
    double* d_pp = st.out(pre_pro, (size_t)B * 4, false);
    double* d_H = st.out(H, (size_t)B * n_gain * n_gain, false);
    double* d_f = st.out(f, (size_t)B * n_gain, false);
    int* d_it = st.out(iters, (size_t)B, false);
    int* d_st = st.out(status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    const auto go = [&](auto... rest) {
        return launch(ctx, name, kern, grid_groups(B, 64 / lanes), dim3(64), 0, B, max_path, mpc_params(p), d_path, d_np, d_state, d_vx,
                      d_mi, d_steer, d_g, d_e, d_k, d_mo, d_pp, rest...);
    };
    int rc;
    if constexpr (HF) rc = go(d_H, d_f, d_it, d_st, tail...);
    else rc = go(d_it, d_st, tail...);
    return rc ? rc : st.finish();
}

extern "C" {

int emp_mpc_lateral(emp_ctx* ctx, const emp_mpc_params* p, int32_t B, int32_t max_path, const double* target_path,
                    const int32_t* n_path, const double* state, const double* vx, const int32_t* min_index,
                    double* steer, double* u, double* e_rr, double* k_r, int32_t* min_index_out, double* pre_pro,
                    double* H, double* f, int32_t* iters, int32_t* status, emp_mem where) {
    return stage_lateral<true>(ctx, "mpc_lateral", mpc::mpc_lateral_kernel<false>, mpc::kNu, mpc::kNu, p, B, max_path, target_path, n_path,
                               state, vx, min_index, steer, u, e_rr, k_r, min_index_out, pre_pro, H, f, iters, status, where, mpc::CtlIO{});
}

void emp_lqr_params_default(emp_mpc_params* p) {
    if (!p) return;
    emp_mpc_params_default(p);
    p->q_diag[0] = 200.0;                                    // ref controller.py:593-597
}

int emp_lqr_lateral(emp_ctx* ctx, const emp_mpc_params* p, int32_t B, int32_t max_path, const double* target_path,
                    const int32_t* n_path, const double* state, const double* vx, const int32_t* min_index,
                    double* steer, double* K, double* e_rr, double* k_r, int32_t* min_index_out, double* pre_pro,
                    int32_t* sweeps, int32_t* status, emp_mem where) {
    return stage_lateral<false>(ctx, "lqr_lateral", lqr::lqr_lateral_kernel<false>, 1, 4, p, B, max_path, target_path, n_path, state, vx,
                                min_index, steer, K, e_rr, k_r, min_index_out, pre_pro, nullptr, nullptr, sweeps, status, where,
                                mpc::CtlIO{});
}

}  // extern "C"

// ---- longitudinal PID, feed-forward MPC, fused vehicle control (reference controller/controller.py:614-990) ----------
namespace {

// ref: Longitudinal_PID_controller.PID_control for B vehicles, one per lane
__global__ __launch_bounds__(256) void pid_longitudinal_kernel(int B, ctl::PidParams p, const double* __restrict__ speed_kmh,
                                                               const double* __restrict__ target_speed, const double* err_in,
                                                               const int* n_err_in, double* __restrict__ command, double* err_out,
                                                               int* n_err_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = 0;
    command[b] = ctl::pid_step(p, speed_kmh[b], target_speed[b], err_in + (size_t)b * ctl::kPidBuffer, n_err_in[b],
                               err_out + (size_t)b * ctl::kPidBuffer, &n);
    n_err_out[b] = n;
}

ctl::PidParams pid_params(const emp_pid_params* p) { return ctl::PidParams{p->K_P, p->K_I, p->K_D, p->dt, p->error_threshold}; }

}  // namespace

extern "C" {

void emp_pid_params_default(emp_pid_params* p) {
    if (!p) return;
    p->K_P = 1.15;                                          // ref controller.py:622
    p->K_I = 0.0;
    p->K_D = 0.0;
    p->dt = 0.01;
    p->error_threshold = 1.0;                               // ref :638
}

int emp_pid_longitudinal(emp_ctx* ctx, const emp_pid_params* p, int32_t B, const double* speed_kmh, const double* target_speed,
                         const double* err_in, const int32_t* n_err_in, double* command, double* err_out, int32_t* n_err_out,
                         emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, p && B >= 0, "bad sizes");
    EMP_REQUIRE(ctx, speed_kmh && target_speed && err_in && n_err_in && command && err_out && n_err_out, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_v = st.in(speed_kmh, (size_t)B);
    const double* d_t = st.in(target_speed, (size_t)B);
    const double* d_ei = st.in(err_in, (size_t)B * ctl::kPidBuffer);
    const int* d_ni = st.in(n_err_in, (size_t)B);
    double* d_c = st.out(command, (size_t)B, false);
    double* d_eo = st.out(err_out, (size_t)B * ctl::kPidBuffer, false);
    int* d_no = st.out(n_err_out, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "pid_longitudinal", pid_longitudinal_kernel, grid1(B, 256), dim3(256), 0, B, pid_params(p), d_v, d_t,
                              d_ei, d_ni, d_c, d_eo, d_no))
        return rc;
    return st.finish();
}

void emp_mpc_ff_params_default(emp_mpc_params* p) {
    if (!p) return;
    emp_mpc_params_default(p);                              // vehicle_para as there
    const double q[4] = {200.0, 1.0, 1.0, 1.0};             // ref controller.py:974-979
    for (int i = 0; i < 4; ++i) {
        p->q_diag[i] = q[i];
        p->f_diag[i] = 10.0;
    }
    p->r = 1.0;
}

int emp_mpc_ff_lateral(emp_ctx* ctx, const emp_mpc_params* p, int32_t B, int32_t max_path, const double* target_path,
                       const int32_t* n_path, const double* state, const double* vx, const int32_t* min_index,
                       double* steer, double* u, double* e_rr, double* k_r, int32_t* min_index_out, double* pre_pro,
                       double* H, double* f, int32_t* iters, int32_t* status, emp_mem where) {
    return stage_lateral<true>(ctx, "mpc_ff_lateral", mpcff::mpc_ff_lateral_kernel, mpcff::kNu, mpcff::kNu, p, B, max_path, target_path,
                               n_path, state, vx, min_index, steer, u, e_rr, k_r, min_index_out, pre_pro, H, f, iters, status, where);
}

int emp_vehicle_control(emp_ctx* ctx, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid, int32_t B,
                        int32_t max_path, const double* target_path, const int32_t* n_path, const double* state,
                        const double* vx, const int32_t* min_index, const double* speed_kmh, const double* target_speed,
                        const double* err_in, const int32_t* n_err_in, double* control, double* lat_command,
                        double* lon_command, int32_t* min_index_out, double* e_rr, double* k_r, double* pre_pro,
                        double* err_out, int32_t* n_err_out, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, lateral == EMP_LAT_MPC || lateral == EMP_LAT_LQR, "lateral must be EMP_LAT_MPC or EMP_LAT_LQR");
    EMP_REQUIRE(ctx, lat && pid && B >= 0 && max_path >= 1, "bad sizes");
    EMP_REQUIRE(ctx, target_path && n_path && state && vx && min_index && speed_kmh && target_speed && err_in && n_err_in &&
                         control && min_index_out && err_out && n_err_out && status,
                "NULL argument");
    EMP_STAGE(st, where);
    const double* d_path = st.in(target_path, (size_t)B * max_path * 4);
    const int* d_np = st.in(n_path, (size_t)B);
    const double* d_state = st.in(state, (size_t)B * 5);
    const double* d_vx = st.in(vx, (size_t)B);
    const int* d_mi = st.in(min_index, (size_t)B);
    mpc::CtlIO io{pid_params(pid), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    io.speed_kmh = st.in(speed_kmh, (size_t)B);
    io.target_speed = st.in(target_speed, (size_t)B);
    io.err_in = st.in(err_in, (size_t)B * ctl::kPidBuffer);
    io.n_err_in = st.in(n_err_in, (size_t)B);
    io.control = st.out(control, (size_t)B * 3, false);
    io.lon_command = st.out(lon_command, (size_t)B, false);
    io.err_out = st.out(err_out, (size_t)B * ctl::kPidBuffer, false);
    io.n_err_out = st.out(n_err_out, (size_t)B, false);
    double* d_lat = lat_command ? st.out(lat_command, (size_t)B, false) : st.tmp<double>((size_t)B);
    double* d_e = st.out(e_rr, (size_t)B * 4, false);
    double* d_k = st.out(k_r, (size_t)B, false);
    int* d_mo = st.out(min_index_out, (size_t)B, false);
    double* d_pp = st.out(pre_pro, (size_t)B * 4, false);
    int* d_st = st.out(status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    const mpc::Params prm = mpc_params(lat);
    double* const no_d = nullptr;                 // the stand-alone laws' own outputs: none here
    int* const no_i = nullptr;
    if (const int rc = launch_lateral(
            ctx, "vehicle_control", lateral, B, mpc::mpc_lateral_kernel<true>, lqr::lqr_lateral_kernel<true>,
            std::make_tuple(B, max_path, prm, d_path, d_np, d_state, d_vx, d_mi, d_lat, no_d, d_e, d_k, d_mo, d_pp, no_d, no_d, no_i, d_st, io),
            std::make_tuple(B, max_path, prm, d_path, d_np, d_state, d_vx, d_mi, d_lat, no_d, d_e, d_k, d_mo, d_pp, no_i, d_st, io)))
        return rc;
    return st.finish();
}

}  // extern "C"

// ---- the vehicle model and the closed-loop rollout (the project's own plant: the reference's is CARLA) ---------------------
namespace {

ctl::VehicleParams vehicle_params(const emp_vehicle_params* p) {
    return ctl::VehicleParams{p->a, p->b, p->Cf, p->Cr, p->m, p->Iz, p->dt, p->steer_gain, p->throttle_accel, p->brake_decel, p->drag};
}

// the one launch of a rollout: `tg` is rollout::NoProfile (emp_rollout, every period of emp_drive) or the rollout::Profile whose
// target emp_rollout_timed and every period of emp_drive_timed sample every tick
template <typename TG>
int launch_rollout(emp_ctx* ctx, const char* name, int lateral, const emp_mpc_params* lat, int B, int max_path, const double* d_path,
                   const int* d_np, const rollout::IO& io, const TG& tg) {
    const auto args = std::make_tuple(B, max_path, mpc_params(lat), d_path, d_np, io, tg);
    return launch_lateral(ctx, name, lateral, B, rollout::mpc_rollout_kernel<TG>, rollout::lqr_rollout_kernel<TG>, args, args);
}

// the checks every rollout shares, behind the caller's own for NULL structs (emp_drive derives its log_every)
int rollout_args_ok(emp_ctx* ctx, int lateral, const emp_vehicle_params* vp, int T, int log_every) {
    EMP_REQUIRE(ctx, lateral == EMP_LAT_MPC || lateral == EMP_LAT_LQR, "lateral must be EMP_LAT_MPC or EMP_LAT_LQR");
    EMP_REQUIRE(ctx, vp->reserved == 0, "emp_vehicle_params.reserved must be 0");
    EMP_REQUIRE(ctx, T >= 1 && T <= EMP_ROLLOUT_MAX_TICKS, "T must be in [1, 65536]");
    EMP_REQUIRE(ctx, log_every >= 1, "log_every must be at least 1");
    return EMP_OK;
}
size_t rollout_log_rows(int T, int log_every) { return ((size_t)T + (size_t)log_every - 1) / (size_t)log_every; }

// The caller's arrays of a rollout (emp_rollout's positional arguments, emp_rollout_timed_io's members): 7 inputs, 6 outputs, 4 logs.
struct RolloutArrays {
    const double *target_path, *state, *target_speed, *err_in;
    const int32_t *n_path, *min_index, *n_err_in;
    double *state_out, *err_out, *log_state, *log_control, *log_err;
    int32_t *min_index_out, *n_err_out, *status, *fail_tick, *log_index;
};

// ... staged into the kernels' rollout::IO: inputs, outputs, logs; the timed rollout's own (`timed` into `tg`) behind the inputs and last
struct RolloutDev {
    const double* path;
    const int* n_path;
    rollout::IO io;
};
RolloutDev stage_rollout(Stage& st, const RolloutArrays& a, const emp_pid_params* pid, const emp_vehicle_params* vp, int B, int max_path,
                         int T, int log_every, const emp_rollout_timed_io* timed = nullptr, rollout::Profile* tg = nullptr) {
    const size_t nB = (size_t)B, n_log = rollout_log_rows(T, log_every);
    RolloutDev d{st.in(a.target_path, nB * max_path * 4), st.in(a.n_path, nB), {pid_params(pid), vehicle_params(vp), T, log_every}};
    rollout::IO& io = d.io;
    io.state_in = st.in(a.state, nB * 6);
    io.min_index_in = st.in(a.min_index, nB);
    io.target_speed = st.in(a.target_speed, nB);
    io.err_in = st.in(a.err_in, nB * ctl::kPidBuffer);
    io.n_err_in = st.in(a.n_err_in, nB);
    if (timed) {
        tg->trajectory = st.in(timed->trajectory, nB * rollout::kTrajRows * EMP_TIMED_POINTS);
        tg->t0 = st.in(timed->t0, nB);
        tg->cursor_in = st.in(timed->cursor_in, nB);
    }
    io.state_out = st.out(a.state_out, nB * 6, false);
    io.min_index_out = st.out(a.min_index_out, nB, false);
    io.err_out = st.out(a.err_out, nB * ctl::kPidBuffer, false);
    io.n_err_out = st.out(a.n_err_out, nB, false);
    io.status = st.out(a.status, nB, false);
    io.fail_tick = st.out(a.fail_tick, nB, false);
    io.log_state = st.out(a.log_state, n_log * nB * 6, false);
    io.log_control = st.out(a.log_control, n_log * nB * 3, false);
    io.log_err = st.out(a.log_err, n_log * nB * 4, false);
    io.log_index = st.out(a.log_index, n_log * nB, false);
    if (timed) {
        tg->cursor_out = st.out(timed->cursor_out, nB, false);
        tg->tgt_status = st.out(timed->tgt_status, nB, false);
        tg->log_target = st.out(timed->log_target, n_log * nB, false);
    }
    return d;
}

}  // namespace

extern "C" {

void emp_vehicle_params_default(emp_vehicle_params* p) {
    if (!p) return;
    emp_mpc_params vp;
    emp_mpc_params_default(&vp);                            // vehicle_para as the controllers take it
    p->a = vp.a; p->b = vp.b; p->Cf = vp.Cf; p->Cr = vp.Cr; p->m = vp.m; p->Iz = vp.Iz;
    p->dt = 0.01;                                           // the PID's (ref controller.py:622)
    p->steer_gain = 1.0;
    p->throttle_accel = 3.0;
    p->brake_decel = 6.0;
    p->drag = 0.0;
    p->reserved = 0;
}

int emp_vehicle_step(emp_ctx* ctx, const emp_vehicle_params* vp, int32_t B, const double* state, const double* control,
                     double* state_out, double* ctl_state, double* vx_ctl, double* speed_kmh, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, vp && B >= 0, "bad sizes");
    EMP_REQUIRE(ctx, vp->reserved == 0, "emp_vehicle_params.reserved must be 0");
    EMP_REQUIRE(ctx, state && control && state_out, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_state = st.in(state, (size_t)B * 6);
    const double* d_ctl = st.in(control, (size_t)B * 3);
    double* d_out = st.out(state_out, (size_t)B * 6, false);
    double* d_cs = st.out(ctl_state, (size_t)B * 5, false);
    double* d_vx = st.out(vx_ctl, (size_t)B, false);
    double* d_kmh = st.out(speed_kmh, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "vehicle_step", rollout::vehicle_step_kernel, grid1(B, 256), dim3(256), 0, B, vehicle_params(vp),
                              d_state, d_ctl, d_out, d_cs, d_vx, d_kmh))
        return rc;
    return st.finish();
}

int emp_rollout(emp_ctx* ctx, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid, const emp_vehicle_params* vp,
                int32_t B, int32_t max_path, const double* target_path, const int32_t* n_path, const double* state,
                const int32_t* min_index, const double* target_speed, const double* err_in, const int32_t* n_err_in, int32_t T,
                int32_t log_every, double* state_out, int32_t* min_index_out, double* err_out, int32_t* n_err_out, int32_t* status,
                int32_t* fail_tick, double* log_state, double* log_control, double* log_err, int32_t* log_index, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, lat && pid && vp && B >= 0 && max_path >= 1, "bad sizes");
    if (const int rc = rollout_args_ok(ctx, lateral, vp, T, log_every)) return rc;
    EMP_REQUIRE(ctx, target_path && n_path && state && min_index && target_speed && err_in && n_err_in && state_out &&
                         min_index_out && err_out && n_err_out && status && fail_tick,
                "NULL argument");
    const RolloutArrays a{target_path, state, target_speed, err_in, n_path, min_index, n_err_in, state_out, err_out, log_state,
                          log_control, log_err, min_index_out, n_err_out, status, fail_tick, log_index};
    EMP_STAGE(st, where);
    const RolloutDev d = stage_rollout(st, a, pid, vp, B, max_path, T, log_every);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch_rollout(ctx, "rollout", lateral, lat, B, max_path, d.path, d.n_path, d.io, rollout::NoProfile{})) return rc;
    return st.finish();
}

int emp_speed_target(emp_ctx* ctx, int32_t B, const double* trajectory, const double* t0, int32_t tick, double dt, const double* cap,
                     const int32_t* cursor_in, double* target_kmh, int32_t* cursor_out, int32_t* tgt_status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "emp_speed_target takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, B >= 0, "bad sizes");
    EMP_REQUIRE(ctx, tick >= 0, "tick must be at least 0");
    EMP_REQUIRE(ctx, trajectory && t0 && cap && target_kmh && cursor_out && tgt_status, "NULL argument");
    EMP_STAGE(st, where);
    const double* d_tr = st.in(trajectory, (size_t)B * rollout::kTrajRows * EMP_TIMED_POINTS);
    const double* d_t0 = st.in(t0, (size_t)B);
    const double* d_cap = st.in(cap, (size_t)B);
    const int* d_ci = st.in(cursor_in, (size_t)B);
    double* d_tg = st.out(target_kmh, (size_t)B, false);
    int* d_co = st.out(cursor_out, (size_t)B, false);
    int* d_ts = st.out(tgt_status, (size_t)B, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "speed_target", rollout::speed_target_kernel, grid1(B, 256), dim3(256), 0, B, d_tr, d_t0, (int)tick, dt,
                              d_cap, d_ci, d_tg, d_co, d_ts))
        return rc;
    return st.finish();
}

int emp_rollout_timed(emp_ctx* ctx, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid, const emp_vehicle_params* vp,
                      int32_t B, int32_t max_path, int32_t T, int32_t tick0, int32_t log_every, const emp_rollout_timed_io* a,
                      emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "emp_rollout_timed takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, lat && pid && vp && a, "NULL parameter struct");
    EMP_REQUIRE(ctx, B >= 0 && max_path >= 1, "bad sizes");
    if (const int rc = rollout_args_ok(ctx, lateral, vp, T, log_every)) return rc;
    EMP_REQUIRE(ctx, a->reserved == 0, "emp_rollout_timed_io.reserved must be 0");
    EMP_REQUIRE(ctx, tick0 >= 0, "tick0 must be at least 0");
    EMP_REQUIRE(ctx, (int64_t)tick0 + (int64_t)T <= (int64_t)INT32_MAX, "tick0 + T must not exceed INT32_MAX");
    EMP_REQUIRE(ctx, a->target_path && a->n_path && a->state && a->min_index && a->target_speed && a->err_in && a->n_err_in &&
                         a->trajectory && a->t0,
                "NULL input array");
    EMP_REQUIRE(ctx, a->state_out && a->min_index_out && a->err_out && a->n_err_out && a->status && a->fail_tick && a->cursor_out &&
                         a->tgt_status,
                "NULL output array");
    const RolloutArrays ra{a->target_path, a->state, a->target_speed, a->err_in, a->n_path, a->min_index, a->n_err_in, a->state_out,
                           a->err_out, a->log_state, a->log_control, a->log_err, a->min_index_out, a->n_err_out, a->status, a->fail_tick,
                           a->log_index};
    EMP_STAGE(st, where);
    rollout::Profile tg{};
    tg.tick0 = tick0;
    const RolloutDev d = stage_rollout(st, ra, pid, vp, B, max_path, T, log_every, a, &tg);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch_rollout(ctx, "rollout_timed", lateral, lat, B, max_path, d.path, d.n_path, d.io, tg)) return rc;
    return st.finish();
}

}  // extern "C"

// ---- the fleet loop (reference driver test_9.py:336-436): request, plan, adopt, T ticks - K periods, nothing leaves the device ----
namespace {

drive::Params drive_params(const emp_drive_params* p, double advance_s) {
    return drive::Params{p->dis_limitation, p->lateral_band, p->behind, p->dynamic_speed, p->static_gate, p->pred_ts, advance_s};
}

// the one launch of a request: `tm` is drive::NoClock (emp_drive_request, every period of emp_drive) or the drive::Clock whose
// extras the speed planner takes (emp_drive_request_timed, every period of emp_drive_timed)
template <typename TM>
int launch_drive_request(emp_ctx* ctx, int B, int max_act, int max_obs, int max_dyn, const drive::Params& prm, const drive::RequestIO& io,
                         const TM& tm) {
    const DriveRequestPlan p = plan_drive_request(B);
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    return launch(ctx, TM::kTimed ? "drive_request_timed" : "drive_request", drive::drive_request_kernel<TM>, dim3(p.grid), dim3(p.block), 0,
                  B, max_act, max_obs, max_dyn, prm, io, tm);
}

// ... and of an adoption: drive::NoSpeed (emp_drive) or the drive::Speed that carries the profile (emp_drive_timed)
template <typename TS>
int launch_drive_adopt(emp_ctx* ctx, int B, int max_pts, const drive::AdoptIO& io, const TS& ts) {
    const DriveRequestPlan p = plan_drive_request(B);
    if (const int rc = plan_refused(ctx, p.error)) return rc;
    return launch(ctx, TS::kTimed ? "drive_adopt_timed" : "drive_adopt", drive::drive_adopt_kernel<TS>, dim3(p.grid), dim3(p.block), 0, B,
                  max_pts, io, ts);
}

// While emp_drive stages its arrays the context's pool is the drive pool; while its periods run, the pipeline setting is off.
// Both are put back however the call ends.
struct DriveScope {
    emp_ctx* ctx;
    int pipe_mode;
    bool own_pool = false;
    explicit DriveScope(emp_ctx* c) : ctx(c), pipe_mode(c->pipe_mode) { swap_pool(); }
    ~DriveScope() {
        ctx->pipe_mode = pipe_mode;
        if (own_pool) swap_pool();
    }
    void swap_pool() {
        std::swap(ctx->pool, ctx->drive_pool);
        own_pool = !own_pool;
    }
};

// The caller's arrays of a request: emp_drive_request's positional arguments.
struct RequestArrays {
    const double *state, *accel, *actors;
    const int32_t* n_act;
    double *static_xy, *static_dis, *dyn, *dyn_dis_speed, *origin_xy, *start_xy, *pred_fi, *start_v, *start_a, *actors_next;
    int32_t *n_static, *n_dyn, *n_obs, *req_status;
};

// emp_drive_request's body; `ck` (emp_drive_request_timed) holds the CALLER's pointers of the timed extras and is staged with the rest
int drive_request_impl(emp_ctx* ctx, const emp_drive_params* p, int B, int max_act, int max_obs, int max_dyn, const RequestArrays& a,
                       emp_mem where, const drive::Clock* ck) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, p && B >= 0, "bad sizes");
    EMP_REQUIRE(ctx, p->reserved == 0, "emp_drive_params.reserved must be 0");
    EMP_REQUIRE(ctx, max_act >= 1 && max_act <= 64, "max_act must be in [1, 64]");
    EMP_REQUIRE(ctx, max_obs >= 1 && max_obs <= 256 && max_dyn >= 1 && max_dyn <= 64, "max_obs must be in [1, 256], max_dyn in [1, 64]");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "EMP_HOST_PINNED is emp_plan_cycle's");
    EMP_REQUIRE(ctx, a.state && a.actors && a.n_act && a.static_xy && a.n_static && a.static_dis && a.dyn && a.n_dyn && a.dyn_dis_speed &&
                         a.n_obs && a.origin_xy && a.start_xy && a.pred_fi && a.start_v && a.start_a && a.req_status,
                "NULL argument");
    if (ck) {
        EMP_REQUIRE(ctx, ck->tick >= 0, "tick must be at least 0");
        EMP_REQUIRE(ctx, std::isfinite(ck->dt) && ck->dt > 0.0, "dt must be finite and positive");
        EMP_REQUIRE(ctx, std::isfinite(ck->plan_lead), "plan_lead must be finite");
        EMP_REQUIRE(ctx, ck->t0 && ck->dyn_obs && ck->start_heading && ck->plan_start_time, "NULL argument");
    }
    EMP_STAGE(st, where);
    drive::RequestIO io{};
    io.state = st.in(a.state, (size_t)B * 6);
    io.accel = st.in(a.accel, (size_t)B * 2);
    io.actors = st.in(a.actors, (size_t)B * max_act * 4);
    io.n_act = st.in(a.n_act, (size_t)B);
    drive::Clock dck{};
    if (ck) {
        dck = *ck;
        dck.t0 = st.in(ck->t0, (size_t)B);
    }
    io.static_xy = st.out(a.static_xy, (size_t)B * max_obs * 2, false);
    io.n_static = st.out(a.n_static, (size_t)B, false);
    io.static_dis = st.out(a.static_dis, (size_t)B * max_obs, false);
    io.dyn = st.out(a.dyn, (size_t)B * max_dyn * 4, false);
    io.n_dyn = st.out(a.n_dyn, (size_t)B, false);
    io.dyn_dis_speed = st.out(a.dyn_dis_speed, (size_t)B * 2, false);
    io.n_obs = st.out(a.n_obs, (size_t)B, false);
    io.origin_xy = st.out(a.origin_xy, (size_t)B * 2, false);
    io.start_xy = st.out(a.start_xy, (size_t)B * 2, false);
    io.pred_fi = st.out(a.pred_fi, (size_t)B, false);
    io.start_v = st.out(a.start_v, (size_t)B * 2, false);
    io.start_a = st.out(a.start_a, (size_t)B * 2, false);
    io.req_status = st.out(a.req_status, (size_t)B, false);
    io.actors_next = st.out(a.actors_next, (size_t)B * max_act * 4, false);
    if (ck) {
        dck.dyn_obs = st.out(ck->dyn_obs, (size_t)B * max_dyn * 4, false);
        dck.start_heading = st.out(ck->start_heading, (size_t)B, false);
        dck.plan_start_time = st.out(ck->plan_start_time, (size_t)B, false);
    }
    if (const int rc = st.ready()) return rc;
    const drive::Params prm = drive_params(p, p->advance_s);
    if (const int rc = ck ? launch_drive_request(ctx, B, max_act, max_obs, max_dyn, prm, io, dck)
                          : launch_drive_request(ctx, B, max_act, max_obs, max_dyn, prm, io, drive::NoClock{}))
        return rc;
    return st.finish();
}

// What emp_drive_timed adds to emp_drive: the speed planner's parameters, the clock, and the arrays emp_drive_io does not have.
struct DriveTimed {
    const emp_speed_dp_params* sdp;
    const emp_speed_qp_params* sqp;
    double plan_lead;
    DriveClockPlan clock;
    const emp_drive_timed_io* io;
};

// What emp_world_drive puts around each period of the loop below (its body is with the traffic calls): the exchange in front,
// whose actors and n_act the period's request reads in place of the caller's, and the agents' ticks behind.  The arrays are staged
// with the drive's own, inputs among its inputs and outputs among its outputs.
struct DriveWorld {
    const double* actors = nullptr;             // [B][max_act][4] on the device: the period's exchanged rows
    const int* n_act = nullptr;                 // [B]
    virtual void stage_in(Stage& st) = 0;
    virtual void stage_out(Stage& st, size_t nK) = 0;
    virtual int exchange(int k, const double* global_path, const int* n_global, const double* state, const int* pre_match_index) = 0;
    virtual int traffic(int k) = 0;
    virtual ~DriveWorld() {}
};

// emp_drive's body behind its own checks of ctx, NULL structs and `where`; with `tm` emp_drive_timed's: the same periods with the
// timed request, the speed half behind the cycle, the profile adopted beside the track, the timed rollout; with `wd` as well
// emp_world_drive's: the same periods again, between the exchange and the agents' ticks
int drive_impl(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth, const emp_drive_params* drv,
               int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid, const emp_vehicle_params* vp, int32_t B,
               int32_t max_global, int32_t max_obs, int32_t max_pts, int32_t max_act, int32_t max_dyn, int32_t K, int32_t T,
               const double* target_speed, const emp_drive_io* io, emp_mem where, const DriveTimed* tm, DriveWorld* wd = nullptr) {
    EMP_REQUIRE(ctx, B >= 0 && max_global >= 1, "bad sizes");
    EMP_REQUIRE(ctx, K >= 1 && K <= EMP_DRIVE_MAX_PERIODS, "K must be in [1, 4096]");
    EMP_REQUIRE(ctx, max_act >= 1 && max_act <= 64, "max_act must be in [1, 64]");
    EMP_REQUIRE(ctx, max_obs >= 1 && max_obs <= 253 && max_dyn >= 1 && max_dyn <= 64, "max_obs must be in [1, 253], max_dyn in [1, 64]");
    EMP_REQUIRE(ctx, max_pts >= 2 && max_pts <= 255, "2 <= max_pts <= 255 required");
    EMP_REQUIRE(ctx, qp->ds > 0, "ds must be > 0");
    EMP_REQUIRE(ctx, target_speed && io->global_path && io->n_global && io->state && (wd || (io->actors && io->n_act)) && io->pre_match_index &&
                         io->track && io->track_len && io->held,
                "NULL input array");
    EMP_REQUIRE(ctx, io->state_out && io->accel_out && io->actors_out && io->pre_match_index_out && io->track_out && io->track_len_out &&
                         io->held_out,
                "NULL output array");
    if (tm) {
        if (const int rc = plan_refused(ctx, tm->clock.error)) return rc;
        if (const int rc = speed_params_ok(ctx, tm->sdp, tm->sqp)) return rc;
        EMP_REQUIRE(ctx, tm->io->t0 && tm->io->profile && tm->io->cursor && tm->io->speed_held, "NULL input array");
        EMP_REQUIRE(ctx, tm->io->profile_out && tm->io->cursor_out && tm->io->speed_held_out, "NULL output array");
    }
    {   // the lattice parameters are checked here, before anything is staged or launched, by the cycle's own rule; the DpDev
        // is not kept (plan_cycle_impl makes its own every period).  max_obs + 3: the cycle adds up to three virtual obstacles
        // for the dynamic one and holds 256 in all, hence this call's limit of 253 against emp_drive_request's 256
        DpDev d;
        if (const int rc = make_dp_dev(ctx, dp, B, max_obs + 3, &d)) return rc;
    }
    EMP_HIP(ctx, hipSetDevice(ctx->device));
    DriveScope scope(ctx);
    Stage st(ctx, where);                       // (with a pipeline set: the main stream waits for the cycles in flight)
    const size_t nB = (size_t)B, row = (size_t)(max_pts + 1) * 4, nK = (size_t)K, prof = (size_t)drive::kProfile;
    const double* d_glob = st.in(io->global_path, nB * max_global * 4);
    const int* d_nglob = st.in(io->n_global, nB);
    const double* d_state = st.in(io->state, nB * 6);
    const double* d_accel = st.in(io->accel, nB * 2);
    const double* d_actors = wd ? nullptr : st.in(io->actors, nB * max_act * 4);
    const int* d_nact = wd ? nullptr : st.in(io->n_act, nB);
    const int* d_prem = st.in(io->pre_match_index, nB);
    const double* d_track = st.in(io->track, nB * row);
    const int* d_tlen = st.in(io->track_len, nB);
    const int* d_held = st.in(io->held, nB);
    const double* d_target = st.in(target_speed, nB);
    const double* d_t0 = tm ? st.in(tm->io->t0, nB) : nullptr;
    const double* d_prof = tm ? st.in(tm->io->profile, nB * prof) : nullptr;
    const int* d_cur = tm ? st.in(tm->io->cursor, nB) : nullptr;
    const int* d_sheld = tm ? st.in(tm->io->speed_held, nB) : nullptr;
    if (wd) wd->stage_in(st);
    double* o_state = st.out(io->state_out, nB * 6, false);
    double* o_accel = st.out(io->accel_out, nB * 2, false);
    double* o_actors = st.out(io->actors_out, nB * max_act * 4, false);
    int* o_prem = st.out(io->pre_match_index_out, nB, false);
    double* o_track = st.out(io->track_out, nB * row, false);
    int* o_tlen = st.out(io->track_len_out, nB, false);
    int* o_held = st.out(io->held_out, nB, false);
    double* l_state = st.out(io->log_state, nK * nB * 6, false);
    int* l_plan = st.out(io->log_plan_status, nK * nB, false);
    int* l_roll = st.out(io->log_roll_status, nK * nB, false);
    int* l_held = st.out(io->log_held, nK * nB, false);
    int* l_counts = st.out(io->log_counts, nK * nB * 2, false);
    double* l_traj = st.out(io->log_traj, nK * nB * row, false);
    int* l_tlen = st.out(io->log_traj_len, nK * nB, false);
    double *o_prof = nullptr, *l_prof = nullptr;
    int *o_cur = nullptr, *o_sheld = nullptr, *l_sst = nullptr, *l_sheld = nullptr, *l_tgt = nullptr, *l_cur = nullptr;
    if (tm) {
        o_prof = st.out(tm->io->profile_out, nB * prof, false);
        o_cur = st.out(tm->io->cursor_out, nB, false);
        o_sheld = st.out(tm->io->speed_held_out, nB, false);
        l_sst = st.out(tm->io->log_speed_status, nK * nB, false);
        l_sheld = st.out(tm->io->log_speed_held, nK * nB, false);
        l_tgt = st.out(tm->io->log_tgt_status, nK * nB, false);
        l_cur = st.out(tm->io->log_cursor, nK * nB, false);
        l_prof = st.out(tm->io->log_profile, nK * nB * prof, false);
    }
    if (wd) wd->stage_out(st, nK);
    // the request's outputs, the cycle's, the rollout's: temporaries of the drive pool, the same for every period
    drive::RequestIO rq{};
    rq.n_act = d_nact;
    rq.static_xy = st.tmp<double>(nB * max_obs * 2);
    rq.n_static = st.tmp<int>(nB);
    rq.static_dis = st.tmp<double>(nB * max_obs);
    rq.dyn = st.tmp<double>(nB * max_dyn * 4);
    rq.n_dyn = st.tmp<int>(nB);
    rq.dyn_dis_speed = st.tmp<double>(nB * 2);
    rq.n_obs = st.tmp<int>(nB);
    rq.origin_xy = st.tmp<double>(nB * 2);
    rq.start_xy = st.tmp<double>(nB * 2);
    rq.pred_fi = st.tmp<double>(nB);
    rq.start_v = st.tmp<double>(nB * 2);
    rq.start_a = st.tmp<double>(nB * 2);
    rq.req_status = st.tmp<int>(nB);
    rq.actors_next = o_actors;
    emp_cycle_io cio{};
    cio.global_path = d_glob;
    cio.n_global = d_nglob;
    cio.max_global = max_global;
    cio.origin_xy = rq.origin_xy;
    cio.start_xy = rq.start_xy;
    cio.start_v = rq.start_v;
    cio.start_a = rq.start_a;
    cio.obs_xy = rq.static_xy;
    cio.n_obs = rq.n_obs;
    cio.dyn_dis_speed = rq.dyn_dis_speed;
    cio.traj = st.tmp<double>(nB * row);
    cio.traj_len = st.tmp<int>(nB);
    cio.status = st.tmp<int>(nB);
    cio.match_index = st.tmp<int>(nB);
    cio.ref_status = st.tmp<int>(nB);
    drive::AdoptIO ad{};
    ad.traj = cio.traj;
    ad.traj_len = cio.traj_len;
    ad.status = cio.status;
    ad.ref_status = cio.ref_status;
    ad.match_index = cio.match_index;
    ad.track_out = o_track;
    ad.track_len_out = o_tlen;
    ad.held_out = o_held;
    ad.pre_match_out = o_prem;
    // the timed loop's own: the request's extras are the speed half's inputs, its trajectory the adoption's
    drive::Clock ck{};
    emp_speed_io sio{};
    drive::Speed sp{};
    int* t_tgt = nullptr;
    if (tm) {
        ck.t0 = d_t0;
        ck.dt = vp->dt;
        ck.plan_lead = tm->plan_lead;
        ck.dyn_obs = st.tmp<double>(nB * max_dyn * 4);
        ck.start_heading = st.tmp<double>(nB);
        ck.plan_start_time = st.tmp<double>(nB);
        sio.dyn_obs = ck.dyn_obs;
        sio.n_dyn = rq.n_dyn;
        sio.start_heading = ck.start_heading;
        sio.plan_start_time = ck.plan_start_time;
        sio.trajectory = st.tmp<double>(nB * prof);
        sio.speed_status = st.tmp<int>(nB);
        sp.trajectory = sio.trajectory;
        sp.speed_status = sio.speed_status;
        sp.profile_out = o_prof;
        sp.cursor_out = o_cur;
        sp.speed_held_out = o_sheld;
        t_tgt = st.tmp<int>(nB);
    }
    // the rollout: a new controller every period (min_index 0, an empty PID deque); its tick-(T - 1) log row feeds the acceleration
    const int log_every = std::max(T - 1, 1);
    const size_t n_log = rollout_log_rows(T, log_every);
    rollout::IO ro{pid_params(pid), vehicle_params(vp), T, log_every};
    ro.min_index_in = st.tmp<int>(nB, true);
    ro.target_speed = d_target;
    ro.err_in = st.tmp<double>(nB * ctl::kPidBuffer, true);
    ro.n_err_in = st.tmp<int>(nB, true);
    ro.state_out = o_state;
    ro.min_index_out = st.tmp<int>(nB);
    ro.err_out = st.tmp<double>(nB * ctl::kPidBuffer);
    ro.n_err_out = st.tmp<int>(nB);
    int* t_roll = st.tmp<int>(nB);
    ro.fail_tick = st.tmp<int>(nB);
    ro.log_state = st.tmp<double>(n_log * nB * 6);
    const double* last_seen = ro.log_state + (T == 1 ? 0 : 1) * nB * 6;
    if (const int rc = st.ready()) return rc;
    if (B == 0) return st.finish();
    scope.swap_pool();                          // the cycles recycle the context's pool as ever
    ctx->pipe_mode = 0;                         // ... and run one batch at a time on the main stream
    const drive::Params prm = drive_params(drv, (double)T * vp->dt);
    for (int k = 0; k < K; ++k) {
        const size_t kB = (size_t)k * nB;
        rq.state = k ? o_state : d_state;
        rq.accel = k ? o_accel : d_accel;
        rq.actors = k ? o_actors : d_actors;
        if (wd) {
            if (const int rc = wd->exchange(k, d_glob, d_nglob, rq.state, k ? o_prem : d_prem)) return rc;
            rq.actors = wd->actors;
            rq.n_act = wd->n_act;
        }
        rq.log_state = l_state ? l_state + kB * 6 : nullptr;
        rq.log_counts = l_counts ? l_counts + kB * 2 : nullptr;
        ck.tick = tm ? tm->clock.tick(k) : 0;
        if (const int rc = tm ? launch_drive_request(ctx, B, max_act, max_obs, max_dyn, prm, rq, ck)
                              : launch_drive_request(ctx, B, max_act, max_obs, max_dyn, prm, rq, drive::NoClock{}))
            return rc;
        cio.pre_match_index = k ? o_prem : d_prem;
        if (tm) {
            SpeedHalf speed{tm->sdp, tm->sqp, &sio, (int)max_dyn};
            if (const int rc = plan_cycle_impl(ctx, dp, qp, smooth, B, kRefLinePoints, max_obs, max_pts, EMP_DP_TWO_KERNEL, &cio, EMP_DEVICE,
                                               &speed, true))
                return rc;
        } else if (const int rc = plan_cycle_impl(ctx, dp, qp, smooth, B, kRefLinePoints, max_obs, max_pts, EMP_DP_TWO_KERNEL, &cio,
                                                  EMP_DEVICE, nullptr, true))
            return rc;
        ad.track_in = k ? o_track : d_track;
        ad.track_len_in = k ? o_tlen : d_tlen;
        ad.held_in = k ? o_held : d_held;
        ad.log_plan_status = l_plan ? l_plan + kB : nullptr;
        ad.log_held = l_held ? l_held + kB : nullptr;
        ad.log_traj = l_traj ? l_traj + kB * row : nullptr;
        ad.log_traj_len = l_tlen ? l_tlen + kB : nullptr;
        ro.state_in = rq.state;
        ro.status = l_roll ? l_roll + kB : t_roll;
        if (tm) {
            sp.profile_in = k ? o_prof : d_prof;
            sp.cursor_in = k ? o_cur : d_cur;
            sp.speed_held_in = k ? o_sheld : d_sheld;
            sp.log_speed_status = l_sst ? l_sst + kB : nullptr;
            sp.log_speed_held = l_sheld ? l_sheld + kB : nullptr;
            sp.log_cursor = l_cur ? l_cur + kB : nullptr;
            sp.log_profile = l_prof ? l_prof + kB * prof : nullptr;
            if (const int rc = launch_drive_adopt(ctx, B, max_pts, ad, sp)) return rc;
            // on the adopted track and profile, from the carried cursor, on the clock of this period's first tick
            const rollout::Profile tg{o_prof, d_t0, o_cur, ck.tick, o_cur, l_tgt ? l_tgt + kB : t_tgt, nullptr};
            if (const int rc = launch_rollout(ctx, "rollout_timed", lateral, lat, B, max_pts + 1, o_track, o_tlen, ro, tg)) return rc;
        } else {
            if (const int rc = launch_drive_adopt(ctx, B, max_pts, ad, drive::NoSpeed{})) return rc;
            if (const int rc = launch_rollout(ctx, "rollout", lateral, lat, B, max_pts + 1, o_track, o_tlen, ro, rollout::NoProfile{})) return rc;
        }
        if (const int rc = launch(ctx, "drive_accel", drive::drive_accel_kernel, grid1(B, 256), dim3(256), 0, B, vp->dt, (const double*)o_state,
                                  last_seen, o_accel))
            return rc;
        if (wd)
            if (const int rc = wd->traffic(k)) return rc;
    }
    ctx->pipe_mode = scope.pipe_mode;
    return st.finish();
}

// emp_drive_timed behind its own checks; with `wd` emp_world_drive's (io->actors and io->n_act are then not looked at)
int drive_timed_impl(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth,
                     const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp, const emp_drive_params* drv,
                     const emp_drive_timed_params* tp, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid,
                     const emp_vehicle_params* vp, int32_t B, int32_t max_global, int32_t max_obs, int32_t max_pts, int32_t max_act,
                     int32_t max_dyn, int32_t K, int32_t T, int32_t tick0, const double* target_speed, const emp_drive_timed_io* io,
                     emp_mem where, DriveWorld* wd) {
    // emp_drive's arrays under their names
    emp_drive_io base{};
    base.global_path = io->global_path;
    base.n_global = io->n_global;
    base.state = io->state;
    base.accel = io->accel;
    base.actors = io->actors;
    base.n_act = io->n_act;
    base.pre_match_index = io->pre_match_index;
    base.track = io->track;
    base.track_len = io->track_len;
    base.held = io->held;
    base.state_out = io->state_out;
    base.accel_out = io->accel_out;
    base.actors_out = io->actors_out;
    base.pre_match_index_out = io->pre_match_index_out;
    base.track_out = io->track_out;
    base.track_len_out = io->track_len_out;
    base.held_out = io->held_out;
    base.log_state = io->log_state;
    base.log_plan_status = io->log_plan_status;
    base.log_roll_status = io->log_roll_status;
    base.log_held = io->log_held;
    base.log_counts = io->log_counts;
    base.log_traj = io->log_traj;
    base.log_traj_len = io->log_traj_len;
    const DriveTimed tm{sdp, sqp, tp->plan_lead, plan_drive_clock(tick0, K, T), io};
    return drive_impl(ctx, dp, qp, smooth, drv, lateral, lat, pid, vp, B, max_global, max_obs, max_pts, max_act, max_dyn, K, T, target_speed,
                      &base, where, &tm, wd);
}

}  // namespace

extern "C" {

void emp_drive_params_default(emp_drive_params* p) {
    if (!p) return;
    p->dis_limitation = 50.0;       // ref test_9.py:377
    p->lateral_band = 5.0;          // :77
    p->behind = -10.0;              // :78
    p->dynamic_speed = 1.0;         // :81
    p->static_gate = 30.0;          // :116
    p->pred_ts = 0.2;               // :335
    p->advance_s = 0.0;
    p->reserved = 0;
}

void emp_drive_timed_params_default(emp_drive_timed_params* p) {
    if (!p) return;
    p->plan_lead = 0.1;             // ref test_10.py:325 (cur_time + 0.1)
    p->reserved = 0;
}

int emp_drive_request(emp_ctx* ctx, const emp_drive_params* p, int32_t B, int32_t max_act, int32_t max_obs, int32_t max_dyn,
                      const double* state, const double* accel, const double* actors, const int32_t* n_act, double* static_xy,
                      int32_t* n_static, double* static_dis, double* dyn, int32_t* n_dyn, double* dyn_dis_speed, int32_t* n_obs,
                      double* origin_xy, double* start_xy, double* pred_fi, double* start_v, double* start_a,
                      int32_t* req_status, double* actors_next, emp_mem where) {
    const RequestArrays a{state, accel, actors, n_act, static_xy, static_dis, dyn, dyn_dis_speed, origin_xy, start_xy, pred_fi, start_v,
                          start_a, actors_next, n_static, n_dyn, n_obs, req_status};
    return drive_request_impl(ctx, p, B, max_act, max_obs, max_dyn, a, where, nullptr);
}

int emp_drive_request_timed(emp_ctx* ctx, const emp_drive_params* p, int32_t B, int32_t max_act, int32_t max_obs, int32_t max_dyn,
                            const double* state, const double* accel, const double* actors, const int32_t* n_act, const double* t0,
                            int32_t tick, double dt, double plan_lead, double* static_xy, int32_t* n_static, double* static_dis,
                            double* dyn, int32_t* n_dyn, double* dyn_dis_speed, int32_t* n_obs, double* origin_xy, double* start_xy,
                            double* pred_fi, double* start_v, double* start_a, int32_t* req_status, double* actors_next,
                            double* dyn_obs, double* start_heading, double* plan_start_time, emp_mem where) {
    const RequestArrays a{state, accel, actors, n_act, static_xy, static_dis, dyn, dyn_dis_speed, origin_xy, start_xy, pred_fi, start_v,
                          start_a, actors_next, n_static, n_dyn, n_obs, req_status};
    const drive::Clock ck{t0, tick, dt, plan_lead, dyn_obs, start_heading, plan_start_time};
    return drive_request_impl(ctx, p, B, max_act, max_obs, max_dyn, a, where, &ck);
}

int emp_drive(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth,
              const emp_drive_params* drv, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid,
              const emp_vehicle_params* vp, int32_t B, int32_t max_global, int32_t max_obs, int32_t max_pts, int32_t max_act,
              int32_t max_dyn, int32_t K, int32_t T, const double* target_speed, const emp_drive_io* io, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, dp && qp && smooth && drv && lat && pid && vp && io, "NULL parameter struct");
    EMP_REQUIRE(ctx, drv->reserved == 0, "emp_drive_params.reserved must be 0");
    EMP_REQUIRE(ctx, io->reserved == 0, "emp_drive_io.reserved must be 0");
    if (const int rc = rollout_args_ok(ctx, lateral, vp, T, 1)) return rc;
    EMP_REQUIRE(ctx, qp_reserved_ok(qp), "emp_qp_params.reserved must be 0 (start from emp_qp_params_default)");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "emp_drive takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    return drive_impl(ctx, dp, qp, smooth, drv, lateral, lat, pid, vp, B, max_global, max_obs, max_pts, max_act, max_dyn, K, T, target_speed,
                      io, where, nullptr);
}

int emp_drive_timed(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth,
                    const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp, const emp_drive_params* drv,
                    const emp_drive_timed_params* tp, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid,
                    const emp_vehicle_params* vp, int32_t B, int32_t max_global, int32_t max_obs, int32_t max_pts, int32_t max_act,
                    int32_t max_dyn, int32_t K, int32_t T, int32_t tick0, const double* target_speed, const emp_drive_timed_io* io,
                    emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, dp && qp && smooth && sdp && sqp && drv && tp && lat && pid && vp && io, "NULL parameter struct");
    EMP_REQUIRE(ctx, drv->reserved == 0, "emp_drive_params.reserved must be 0");
    EMP_REQUIRE(ctx, tp->reserved == 0, "emp_drive_timed_params.reserved must be 0");
    EMP_REQUIRE(ctx, std::isfinite(tp->plan_lead), "emp_drive_timed_params.plan_lead must be finite");
    EMP_REQUIRE(ctx, io->reserved == 0, "emp_drive_timed_io.reserved must be 0");
    if (const int rc = rollout_args_ok(ctx, lateral, vp, T, 1)) return rc;
    EMP_REQUIRE(ctx, qp_reserved_ok(qp), "emp_qp_params.reserved must be 0 (start from emp_qp_params_default)");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE,
                "emp_drive_timed takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    return drive_timed_impl(ctx, dp, qp, smooth, sdp, sqp, drv, tp, lateral, lat, pid, vp, B, max_global, max_obs, max_pts, max_act, max_dyn, K, T,
                            tick0, target_speed, io, where, nullptr);
}

}  // extern "C"

// ---- global routing (emp_route_core.h, emp_route_kernels.h; the launch: emp_route_launch.h) -------------------------------------
// origin_wp == nullptr: emp_route_search, A* only
static int route_impl(emp_ctx* ctx, const emp_route_graph* g, int32_t B, int32_t max_route, int32_t max_global, const int32_t* start_node,
                      const int32_t* end_edge, const double* origin_wp, const double* dest_wp, int32_t* route, int32_t* route_len,
                      int32_t* wp_index, double* global_path, int32_t* n_global, int32_t* status, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, g != nullptr && g->reserved == 0, "route graph: NULL, or reserved != 0");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "routing takes EMP_HOST or EMP_DEVICE arrays");
    const RoutePlan plan = plan_route(B, g->n_nodes, max_route, max_global);
    if (const int rc = plan_refused(ctx, plan.error)) return rc;
    EMP_REQUIRE(ctx, B >= 0 && g->n_edges >= 0 && g->n_wp >= 0, "bad sizes");
    EMP_REQUIRE(ctx, g->vertex && g->succ_off && g->succ && g->length && g->wp_off && g->wp, "route graph: NULL array");
    if (B == 0) return EMP_OK;
    EMP_REQUIRE(ctx, start_node && end_edge && route && route_len && status, "NULL argument");
    const route::Graph host = {g->vertex, g->succ_off, g->succ, g->length, g->wp_off, g->wp, g->n_nodes, g->n_edges, g->n_wp};
    if (where == EMP_HOST)
        if (const char* err = route::graph_error(host)) return fail(ctx, EMP_ERR_INVALID, err);
    EMP_STAGE(st, where);
    route::Graph d = host;
    d.vertex = st.in(g->vertex, (size_t)g->n_nodes * 3);
    d.succ_off = st.in(g->succ_off, (size_t)g->n_nodes + 1);
    d.succ = st.in(g->succ, (size_t)g->n_edges);
    d.length = st.in(g->length, (size_t)g->n_edges);
    d.wp_off = st.in(g->wp_off, (size_t)g->n_edges + 1);
    d.wp = st.in(g->wp, (size_t)g->n_wp * 3);
    const int* d_start = st.in(start_node, (size_t)B);
    const int* d_end = st.in(end_edge, (size_t)B);
    const double* d_origin = st.in(origin_wp, (size_t)B * 3);
    const double* d_dest = st.in(dest_wp, (size_t)B * 3);
    int* d_route = st.out(route, (size_t)B * max_route);
    int* d_len = st.out(route_len, (size_t)B);
    int* d_wpi = st.out(wp_index, (size_t)B * max_global);
    double* d_gp = st.out(global_path, (size_t)B * max_global * 4);
    int* d_ng = st.out(n_global, (size_t)B);
    int* d_st = st.out(status, (size_t)B);
    if (const int rc = st.ready()) return rc;
    if (const int rc = set_lds(ctx, route::route_kernel, plan.lds, kRouteTooManyNodes)) return rc;
    if (const int rc = launch(ctx, "route", route::route_kernel, dim3(plan.grid), dim3(plan.block), plan.lds, d, (int)B, (int)max_route,
                              (int)max_global, d_start, d_end, d_origin, d_dest, d_route, d_len, d_wpi, d_gp, d_ng, d_st))
        return rc;
    return st.finish();
}

extern "C" {

int emp_route_search(emp_ctx* ctx, const emp_route_graph* graph, int32_t B, int32_t max_route, const int32_t* start_node,
                     const int32_t* end_edge, int32_t* route, int32_t* route_len, int32_t* status, emp_mem where) {
    return route_impl(ctx, graph, B, max_route, 1, start_node, end_edge, nullptr, nullptr, route, route_len, nullptr, nullptr, nullptr,
                      status, where);
}

int emp_route_paths(emp_ctx* ctx, const emp_route_graph* graph, int32_t B, int32_t max_route, int32_t max_global,
                    const int32_t* start_node, const int32_t* end_edge, const double* origin_wp, const double* dest_wp,
                    int32_t* route, int32_t* route_len, int32_t* wp_index, double* global_path, int32_t* n_global, int32_t* status,
                    emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, B == 0 || (origin_wp && dest_wp && wp_index && global_path && n_global), "NULL argument");
    return route_impl(ctx, graph, B, max_route, max_global, start_node, end_edge, origin_wp, dest_wp, route, route_len, wp_index,
                      global_path, n_global, status, where);
}

}  // extern "C"

// ---- routed traffic: the agents' local planner and PID pair (emp_agent_core.h, emp_agent_kernels.h) -----------------------------
namespace {

agt::Params agent_params(const emp_agent_params* p) {
    return agt::Params{p->lat_K_P, p->lat_K_I, p->lat_K_D, p->lon_K_P, p->lon_K_I, p->lon_K_D, p->dt, p->max_throttle, p->max_brake,
                       p->max_steer, p->base_min_distance};
}

// The caller's arrays of the agent state: six inputs and the six outputs of their names.
struct AgentArrays {
    const int32_t *head, *n_lon, *n_lat;
    const double *past_steer, *lon_err, *lat_err;
    int32_t *head_out, *n_lon_out, *n_lat_out;
    double *past_steer_out, *lon_err_out, *lat_err_out;
    bool complete() const {
        return head && n_lon && n_lat && past_steer && lon_err && lat_err && head_out && n_lon_out && n_lat_out && past_steer_out &&
               lon_err_out && lat_err_out;
    }
};
void stage_agent_in(Stage& st, const AgentArrays& a, size_t nA, agt::StateIO* io) {
    io->head_in = st.in(a.head, nA);
    io->past_in = st.in(a.past_steer, nA);
    io->lon_in = st.in(a.lon_err, nA * agt::kBuffer);
    io->n_lon_in = st.in(a.n_lon, nA);
    io->lat_in = st.in(a.lat_err, nA * agt::kBuffer);
    io->n_lat_in = st.in(a.n_lat, nA);
}
void stage_agent_out(Stage& st, const AgentArrays& a, size_t nA, agt::StateIO* io) {
    io->head_out = st.out(a.head_out, nA, false);
    io->past_out = st.out(a.past_steer_out, nA, false);
    io->lon_out = st.out(a.lon_err_out, nA * agt::kBuffer, false);
    io->n_lon_out = st.out(a.n_lon_out, nA, false);
    io->lat_out = st.out(a.lat_err_out, nA * agt::kBuffer, false);
    io->n_lat_out = st.out(a.n_lat_out, nA, false);
}

}  // namespace

extern "C" {

void emp_agent_params_default(emp_agent_params* p) {
    if (!p) return;
    p->lat_K_P = 1.95; p->lat_K_I = 0.05; p->lat_K_D = 0.2;     // ref local_planner.py:73
    p->lon_K_P = 1.0; p->lon_K_I = 0.05; p->lon_K_D = 0.0;      // :74
    p->dt = 1.0 / 20.0;                                         // :70
    p->max_throttle = 0.75;                                     // :75-77
    p->max_brake = 0.3;
    p->max_steer = 0.8;
    p->base_min_distance = 3.0;                                 // :79
    p->reserved = 0;
}

int emp_agent_observe(emp_ctx* ctx, int32_t A, const double* state, double* forward, double* speed_kmh, double* actors, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "emp_agent_observe takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, A >= 0, "bad sizes");
    EMP_REQUIRE(ctx, state && (forward || speed_kmh || actors), "NULL argument (state, and at least one output)");
    EMP_STAGE(st, where);
    const double* d_state = st.in(state, (size_t)A * 6);
    double* d_fw = st.out(forward, (size_t)A * 2, false);
    double* d_kmh = st.out(speed_kmh, (size_t)A, false);
    double* d_act = st.out(actors, (size_t)A * 4, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "agent_observe", agt::agent_observe_kernel, grid1(A, 256), dim3(256), 0, (int)A, d_state, d_fw, d_kmh, d_act))
        return rc;
    return st.finish();
}

int emp_agent_control(emp_ctx* ctx, const emp_agent_params* p, int32_t A, int32_t max_path, const double* path, const int32_t* n_path,
                      const double* state, const double* forward, const double* speed_kmh, const double* target_speed,
                      const int32_t* head, const double* past_steer, const double* lon_err, const int32_t* n_lon,
                      const double* lat_err, const int32_t* n_lat, double* control, int32_t* status, int32_t* head_out,
                      double* past_steer_out, double* lon_err_out, int32_t* n_lon_out, double* lat_err_out, int32_t* n_lat_out,
                      double* lat_error, double* lon_command, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "emp_agent_control takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, p && A >= 0 && max_path >= 1, "bad sizes");
    EMP_REQUIRE(ctx, p->reserved == 0, "emp_agent_params.reserved must be 0");
    const AgentArrays aa{head, n_lon, n_lat, past_steer, lon_err, lat_err, head_out, n_lon_out, n_lat_out, past_steer_out, lon_err_out, lat_err_out};
    EMP_REQUIRE(ctx, path && n_path && state && forward && speed_kmh && target_speed && control && status && aa.complete(), "NULL argument");
    const size_t nA = (size_t)A;
    EMP_STAGE(st, where);
    const double* d_path = st.in(path, nA * max_path * 4);
    const int* d_np = st.in(n_path, nA);
    const double* d_state = st.in(state, nA * 6);
    const double* d_fw = st.in(forward, nA * 2);
    const double* d_kmh = st.in(speed_kmh, nA);
    const double* d_tgt = st.in(target_speed, nA);
    agt::StateIO sio{};
    stage_agent_in(st, aa, nA, &sio);
    double* d_ctl = st.out(control, nA * 3, false);
    int* d_st = st.out(status, nA, false);
    stage_agent_out(st, aa, nA, &sio);
    double* d_le = st.out(lat_error, nA, false);
    double* d_lc = st.out(lon_command, nA, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "agent_control", agt::agent_control_kernel, grid1(A, 64), dim3(64), 0, (int)A, (int)max_path, agent_params(p),
                              d_path, d_np, d_state, d_fw, d_kmh, d_tgt, sio, d_ctl, d_st, d_le, d_lc))
        return rc;
    return st.finish();
}

int emp_agent_rollout(emp_ctx* ctx, const emp_agent_params* p, const emp_vehicle_params* vp, int32_t A, int32_t max_path, int32_t T,
                      int32_t log_every, const emp_agent_rollout_io* a, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "emp_agent_rollout takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, p && vp && a, "NULL parameter struct");
    EMP_REQUIRE(ctx, A >= 0 && max_path >= 1, "bad sizes");
    EMP_REQUIRE(ctx, p->reserved == 0, "emp_agent_params.reserved must be 0");
    EMP_REQUIRE(ctx, vp->reserved == 0, "emp_vehicle_params.reserved must be 0");
    EMP_REQUIRE(ctx, a->reserved == 0, "emp_agent_rollout_io.reserved must be 0");
    EMP_REQUIRE(ctx, T >= 1 && T <= EMP_ROLLOUT_MAX_TICKS, "T must be in [1, 65536]");
    EMP_REQUIRE(ctx, log_every >= 1, "log_every must be at least 1");
    const AgentArrays aa{a->head, a->n_lon, a->n_lat, a->past_steer, a->lon_err, a->lat_err, a->head_out, a->n_lon_out, a->n_lat_out,
                         a->past_steer_out, a->lon_err_out, a->lat_err_out};
    EMP_REQUIRE(ctx, a->path && a->n_path && a->state && a->target_speed && a->state_out && a->status && a->done_tick && aa.complete(),
                "NULL array");
    const size_t nA = (size_t)A, n_log = rollout_log_rows(T, log_every);
    EMP_STAGE(st, where);
    const double* d_path = st.in(a->path, nA * max_path * 4);
    const int* d_np = st.in(a->n_path, nA);
    agt::RolloutIO io{};
    io.T = T;
    io.log_every = log_every;
    io.state_in = st.in(a->state, nA * 6);
    io.target_speed = st.in(a->target_speed, nA);
    stage_agent_in(st, aa, nA, &io.st);
    io.state_out = st.out(a->state_out, nA * 6, false);
    stage_agent_out(st, aa, nA, &io.st);
    io.status = st.out(a->status, nA, false);
    io.done_tick = st.out(a->done_tick, nA, false);
    io.actors_out = st.out(a->actors_out, nA * 4, false);
    io.log_state = st.out(a->log_state, n_log * nA * 6, false);
    io.log_control = st.out(a->log_control, n_log * nA * 3, false);
    io.log_head = st.out(a->log_head, n_log * nA, false);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "agent_rollout", agt::agent_rollout_kernel, grid1(A, 64), dim3(64), 0, (int)A, (int)max_path, agent_params(p),
                              vehicle_params(vp), d_path, d_np, io))
        return rc;
    return st.finish();
}

}  // extern "C"

// ---- traffic that reacts to traffic: BehaviorAgent's car-following (emp_behavior_core.h, emp_behavior_kernels.h) ----------------
namespace {

bhv::Params behavior_params(const emp_behavior_params* p) {
    return bhv::Params{p->max_speed, p->speed_lim_dist, p->speed_decrease, p->safety_time, p->min_proximity_threshold, p->braking_distance,
                       p->min_speed, p->emergency_brake, p->up_angle, (int)p->look_steps};
}

AgentArrays behavior_agent_arrays(const emp_behavior_io* a) {
    return AgentArrays{a->head, a->n_lon, a->n_lat, a->past_steer, a->lon_err, a->lat_err, a->head_out, a->n_lon_out, a->n_lat_out,
                       a->past_steer_out, a->lon_err_out, a->lat_err_out};
}

// what both calls refuse, and the arrays both stage: the world, the agents' inputs and state.  A padding slot is never written in
// the caller's device memory (EMP_DEVICE); staged outputs (EMP_HOST) are copied back whole, their padding slots as 0.
int behavior_checks(emp_ctx* ctx, const char* who, const emp_agent_params* p, const emp_behavior_params* bp, const emp_behavior_io* a,
                    int max_other, emp_mem where, const bhv::BehaviorPlan& plan) {
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "the behaviour calls take EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, p && bp && a, "NULL parameter struct");
    (void)who;
    EMP_REQUIRE(ctx, plan.error == nullptr, plan.error);
    EMP_REQUIRE(ctx, p->reserved == 0, "emp_agent_params.reserved must be 0");
    EMP_REQUIRE(ctx, bp->reserved == 0, "emp_behavior_params.reserved must be 0");
    EMP_REQUIRE(ctx, a->reserved == 0, "emp_behavior_io.reserved must be 0");
    EMP_REQUIRE(ctx, a->n_world && a->path && a->n_path && a->lane && a->state && a->speed_limit && a->extent && a->status &&
                         behavior_agent_arrays(a).complete(), "NULL array");
    EMP_REQUIRE(ctx, max_other == 0 || (a->n_other && a->other && a->other_lane), "max_other > 0 needs n_other, other and other_lane");
    return EMP_OK;
}

void stage_world(Stage& st, const emp_behavior_io* a, size_t W, size_t max_world, size_t max_path, size_t max_other, int64_t tick0,
                 bhv::WorldIO* io) {
    const size_t nA = W * max_world;
    io->max_world = (int)max_world;
    io->max_path = (int)max_path;
    io->max_other = (int)max_other;
    io->tick0 = (long long)tick0;
    io->n_world = st.in(a->n_world, W);
    io->path = st.in(a->path, nA * max_path * 4);
    io->n_path = st.in(a->n_path, nA);
    io->lane = st.in(a->lane, nA * max_path);
    io->state = st.in(a->state, nA * 6);
    io->speed_limit = st.in(a->speed_limit, nA);
    io->extent = st.in(a->extent, nA);
    if (max_other > 0) {
        io->n_other = st.in(a->n_other, W);
        io->other = st.in(a->other, W * max_other * 5);
        io->other_lane = st.in(a->other_lane, W * max_other);
    }
    stage_agent_in(st, behavior_agent_arrays(a), nA, &io->st);
}

void stage_behavior_state_out(Stage& st, const emp_behavior_io* a, size_t nA, bool z, bhv::WorldIO* io) {
    io->st.head_out = st.out(a->head_out, nA, z);
    io->st.past_out = st.out(a->past_steer_out, nA, z);
    io->st.lon_out = st.out(a->lon_err_out, nA * agt::kBuffer, z);
    io->st.n_lon_out = st.out(a->n_lon_out, nA, z);
    io->st.lat_out = st.out(a->lat_err_out, nA * agt::kBuffer, z);
    io->st.n_lat_out = st.out(a->n_lat_out, nA, z);
    io->status = st.out(a->status, nA, z);
}

}  // namespace

extern "C" {

void emp_behavior_params_default(emp_behavior_params* p, int32_t kind) {
    if (!p) return;
    // ref behavior_types.py: Cautious, Normal, Aggressive
    if (kind == EMP_BHV_CAUTIOUS) {
        p->max_speed = 40.0; p->speed_lim_dist = 6.0; p->speed_decrease = 12.0; p->safety_time = 3.0;
        p->min_proximity_threshold = 12.0; p->braking_distance = 6.0;
    } else if (kind == EMP_BHV_AGGRESSIVE) {
        p->max_speed = 70.0; p->speed_lim_dist = 1.0; p->speed_decrease = 8.0; p->safety_time = 3.0;
        p->min_proximity_threshold = 8.0; p->braking_distance = 4.0;
    } else {
        p->max_speed = 50.0; p->speed_lim_dist = 3.0; p->speed_decrease = 10.0; p->safety_time = 3.0;
        p->min_proximity_threshold = 10.0; p->braking_distance = 5.0;
    }
    p->min_speed = 5.0;                                         // behavior_agent.py:51
    p->emergency_brake = 0.5;                                   // basic_agent.py:50
    p->up_angle = 30.0;                                         // behavior_agent.py:215
    p->look_steps = 5;                                          // :128
    p->reserved = 0;
}

int emp_agent_behave(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, int32_t W, int32_t max_world,
                     int32_t max_path, int32_t max_other, int64_t tick0, const emp_behavior_io* a, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    const bhv::BehaviorPlan plan = bhv::plan_behavior(W, max_world, max_other, max_path, 0, 1, tick0);
    if (const int rc = behavior_checks(ctx, "emp_agent_behave", p, bp, a, max_other, where, plan)) return rc;
    EMP_REQUIRE(ctx, a->forward && a->speed_kmh && a->control && a->mode && a->blocker && a->distance && a->ttc && a->target_speed_out,
                "NULL array");
    if (W == 0) return EMP_OK;
    const size_t nA = (size_t)W * max_world;
    EMP_STAGE(st, where);
    const bool z = where == EMP_HOST;          // staged outputs start from 0; the caller's device memory is never filled
    bhv::WorldIO io{};
    stage_world(st, a, (size_t)W, (size_t)max_world, (size_t)max_path, (size_t)max_other, tick0, &io);
    io.forward = st.in(a->forward, nA * 2);
    io.speed_kmh = st.in(a->speed_kmh, nA);
    stage_behavior_state_out(st, a, nA, z, &io);
    io.control = st.out(a->control, nA * 3, z);
    io.mode = st.out(a->mode, nA, z);
    io.blocker = st.out(a->blocker, nA, z);
    io.distance = st.out(a->distance, nA, z);
    io.ttc = st.out(a->ttc, nA, z);
    io.target_out = st.out(a->target_speed_out, nA, z);
    io.lat_error = st.out(a->lat_error, nA, z);
    io.lon_command = st.out(a->lon_command, nA, z);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "agent_behave", bhv::agent_behave_kernel, dim3(plan.grid), dim3(plan.block), 0, agent_params(p),
                              behavior_params(bp), io))
        return rc;
    return st.finish();
}

int emp_traffic_rollout(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp, int32_t W,
                        int32_t max_world, int32_t max_path, int32_t max_other, int32_t T, int32_t log_every, int64_t tick0,
                        const emp_behavior_io* a, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, T >= 1, "T must be in [1, 65536]");
    const bhv::BehaviorPlan plan = bhv::plan_behavior(W, max_world, max_other, max_path, T, log_every, tick0);
    if (const int rc = behavior_checks(ctx, "emp_traffic_rollout", p, bp, a, max_other, where, plan)) return rc;
    EMP_REQUIRE(ctx, vp != nullptr, "NULL parameter struct");
    EMP_REQUIRE(ctx, vp->reserved == 0, "emp_vehicle_params.reserved must be 0");
    EMP_REQUIRE(ctx, a->state_out && a->done_tick && a->mode_ticks && a->min_gap, "NULL array");
    if (W == 0) return EMP_OK;
    const size_t nA = (size_t)W * max_world, n_log = plan.n_log;
    EMP_STAGE(st, where);
    const bool z = where == EMP_HOST;          // staged outputs start from 0; the caller's device memory is never filled
    bhv::WorldIO io{};
    stage_world(st, a, (size_t)W, (size_t)max_world, (size_t)max_path, (size_t)max_other, tick0, &io);
    io.T = T;
    io.log_every = log_every;
    stage_behavior_state_out(st, a, nA, z, &io);
    io.state_out = st.out(a->state_out, nA * 6, z);
    io.done_tick = st.out(a->done_tick, nA, z);
    io.mode_ticks = st.out(a->mode_ticks, nA * bhv::kCountedModes, z);
    io.min_gap = st.out(a->min_gap, nA, z);
    io.actors_out = st.out(a->actors_out, nA * 4, z);
    io.log_state = st.out(a->log_state, n_log * nA * 6, z);
    io.log_control = st.out(a->log_control, n_log * nA * 3, z);
    io.log_head = st.out(a->log_head, n_log * nA, z);
    io.log_mode = st.out(a->log_mode, n_log * nA, z);
    io.log_target = st.out(a->log_target, n_log * nA, z);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "traffic_rollout", bhv::traffic_rollout_kernel, dim3(plan.grid), dim3(plan.block), 0, agent_params(p),
                              behavior_params(bp), vehicle_params(vp), (int)nA, io))
        return rc;
    return st.finish();
}

}  // extern "C"

// ---- traffic that stops for red lights and pedestrians (emp_hazard_core.h, emp_hazard_kernels.h) ------------------------------------
namespace {

hz::Params hazard_params(const emp_hazard_params* p) {
    return hz::Params{p->tlight_threshold, p->tlight_up_angle, p->walker_radius, p->walker_up_angle};
}

// what both hazard calls refuse beyond behavior_checks
int hazard_checks(emp_ctx* ctx, const emp_hazard_params* hp, const emp_hazard_io* h, int max_light, int max_walker) {
    EMP_REQUIRE(ctx, hp && h, "NULL parameter struct");
    EMP_REQUIRE(ctx, hp->reserved == 0, "emp_hazard_params.reserved must be 0");
    EMP_REQUIRE(ctx, h->reserved == 0, "emp_hazard_io.reserved must be 0");
    EMP_REQUIRE(ctx, h->last_light && h->last_light_out, "NULL array");
    EMP_REQUIRE(ctx, max_light == 0 || (h->n_light && h->light && h->light_lane && h->light_cycle),
                "max_light > 0 needs n_light, light, light_lane and light_cycle");
    EMP_REQUIRE(ctx, max_walker == 0 || (h->n_walker && h->walker && h->walker_lane), "max_walker > 0 needs n_walker, walker and walker_lane");
    return EMP_OK;
}

void stage_hazards(Stage& st, const emp_hazard_io* h, size_t W, size_t nA, size_t max_light, size_t max_walker, bool z, hz::HazardIO* io) {
    io->max_light = (int)max_light;
    io->max_walker = (int)max_walker;
    if (max_light > 0) {
        io->n_light = st.in(h->n_light, W);
        io->light = st.in(h->light, W * max_light * 4);
        io->light_lane = st.in(h->light_lane, W * max_light);
        io->light_cycle = st.in(h->light_cycle, W * max_light * 3);
    }
    if (max_walker > 0) {
        io->n_walker = st.in(h->n_walker, W);
        io->walker = st.in(h->walker, W * max_walker * 5);
        io->walker_lane = st.in(h->walker_lane, W * max_walker);
    }
    io->last_light = st.in(h->last_light, nA);
    io->last_light_out = st.out(h->last_light_out, nA, z);
}

}  // namespace

extern "C" {

void emp_hazard_params_default(emp_hazard_params* p) {
    if (!p) return;
    p->tlight_threshold = 5.0;                                  // basic_agent.py:47
    p->tlight_up_angle = 90.0;                                  // :245
    p->walker_radius = 10.0;                                    // behavior_agent.py:239
    p->walker_up_angle = 60.0;                                  // :249
    p->reserved = 0;
}

int emp_agent_behave_hazards(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, int32_t W, int32_t max_world,
                             int32_t max_path, int32_t max_other, int64_t tick0, const emp_behavior_io* a, emp_mem where,
                             const emp_hazard_params* hp, int32_t max_light, int32_t max_walker, const emp_hazard_io* h) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    const bhv::BehaviorPlan plan = hz::plan_hazards(W, max_world, max_other, max_light, max_walker, max_path, 0, 1, tick0);
    if (const int rc = behavior_checks(ctx, "emp_agent_behave_hazards", p, bp, a, max_other, where, plan)) return rc;
    EMP_REQUIRE(ctx, a->forward && a->speed_kmh && a->control && a->mode && a->blocker && a->distance && a->ttc && a->target_speed_out,
                "NULL array");
    if (const int rc = hazard_checks(ctx, hp, h, max_light, max_walker)) return rc;
    EMP_REQUIRE(ctx, h->cause && h->light_hit && h->walker_hit && h->walker_distance, "NULL array");
    if (W == 0) return EMP_OK;
    const size_t nA = (size_t)W * max_world;
    EMP_STAGE(st, where);
    const bool z = where == EMP_HOST;          // staged outputs start from 0; the caller's device memory is never filled
    bhv::WorldIO io{};
    hz::HazardIO hio{};
    stage_world(st, a, (size_t)W, (size_t)max_world, (size_t)max_path, (size_t)max_other, tick0, &io);
    io.forward = st.in(a->forward, nA * 2);
    io.speed_kmh = st.in(a->speed_kmh, nA);
    stage_behavior_state_out(st, a, nA, z, &io);
    io.control = st.out(a->control, nA * 3, z);
    io.mode = st.out(a->mode, nA, z);
    io.blocker = st.out(a->blocker, nA, z);
    io.distance = st.out(a->distance, nA, z);
    io.ttc = st.out(a->ttc, nA, z);
    io.target_out = st.out(a->target_speed_out, nA, z);
    io.lat_error = st.out(a->lat_error, nA, z);
    io.lon_command = st.out(a->lon_command, nA, z);
    stage_hazards(st, h, (size_t)W, nA, (size_t)max_light, (size_t)max_walker, z, &hio);
    hio.cause = st.out(h->cause, nA, z);
    hio.light_hit = st.out(h->light_hit, nA, z);
    hio.walker_hit = st.out(h->walker_hit, nA, z);
    hio.walker_distance = st.out(h->walker_distance, nA, z);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch(ctx, "agent_behave_hazards", hz::agent_behave_hazards_kernel, dim3(plan.grid), dim3(plan.block), 0,
                              agent_params(p), behavior_params(bp), hazard_params(hp), io, hio))
        return rc;
    return st.finish();
}

}  // extern "C"

namespace {

// what emp_traffic_rollout_hazards refuses (emp_traffic_rollout_epoch and emp_world_drive with it)
int traffic_hazards_checks(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp,
                           const emp_behavior_io* a, int max_other, emp_mem where, const bhv::BehaviorPlan& plan, const emp_hazard_params* hp,
                           int max_light, int max_walker, const emp_hazard_io* h) {
    if (const int rc = behavior_checks(ctx, "emp_traffic_rollout_hazards", p, bp, a, max_other, where, plan)) return rc;
    EMP_REQUIRE(ctx, vp != nullptr, "NULL parameter struct");
    EMP_REQUIRE(ctx, vp->reserved == 0, "emp_vehicle_params.reserved must be 0");
    EMP_REQUIRE(ctx, a->state_out && a->done_tick && a->mode_ticks && a->min_gap, "NULL array");
    if (const int rc = hazard_checks(ctx, hp, h, max_light, max_walker)) return rc;
    EMP_REQUIRE(ctx, h->cause_ticks && h->min_walker_gap, "NULL array");
    return EMP_OK;
}

// ... and the arrays it stages, but for its logs
void stage_traffic_hazards(Stage& st, const emp_behavior_io* a, const emp_hazard_io* h, size_t W, size_t max_world, size_t max_path,
                           size_t max_other, size_t max_light, size_t max_walker, int64_t tick0, bool z, bhv::WorldIO* io, hz::HazardIO* hio) {
    const size_t nA = W * max_world;
    stage_world(st, a, W, max_world, max_path, max_other, tick0, io);
    stage_behavior_state_out(st, a, nA, z, io);
    io->state_out = st.out(a->state_out, nA * 6, z);
    io->done_tick = st.out(a->done_tick, nA, z);
    io->mode_ticks = st.out(a->mode_ticks, nA * bhv::kCountedModes, z);
    io->min_gap = st.out(a->min_gap, nA, z);
    io->actors_out = st.out(a->actors_out, nA * 4, z);
    stage_hazards(st, h, W, nA, max_light, max_walker, z, hio);
    hio->cause_ticks = st.out(h->cause_ticks, nA * hz::kCountedCauses, z);
    hio->min_walker_gap = st.out(h->min_walker_gap, nA, z);
}

int launch_traffic_hazards(emp_ctx* ctx, const bhv::BehaviorPlan& plan, const emp_agent_params* p, const emp_behavior_params* bp,
                           const emp_hazard_params* hp, const emp_vehicle_params* vp, size_t nA, const bhv::WorldIO& io,
                           const hz::HazardIO& hio) {
    return launch(ctx, "traffic_rollout_hazards", hz::traffic_rollout_hazards_kernel, dim3(plan.grid), dim3(plan.block), 0, agent_params(p),
                  behavior_params(bp), hazard_params(hp), vehicle_params(vp), (int)nA, io, hio);
}

// emp_traffic_rollout_hazards is other_tick0 == 0
int traffic_rollout_hazards_impl(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp,
                                 int32_t W, int32_t max_world, int32_t max_path, int32_t max_other, int32_t T, int32_t log_every,
                                 int64_t tick0, const emp_behavior_io* a, emp_mem where, const emp_hazard_params* hp, int32_t max_light,
                                 int32_t max_walker, const emp_hazard_io* h, int64_t other_tick0) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, T >= 1, "T must be in [1, 65536]");
    const bhv::BehaviorPlan plan = hz::plan_hazards(W, max_world, max_other, max_light, max_walker, max_path, T, log_every, tick0);
    if (const int rc = traffic_hazards_checks(ctx, p, bp, vp, a, max_other, where, plan, hp, max_light, max_walker, h)) return rc;
    if (const int rc = plan_refused(ctx, wx::epoch_error(tick0, other_tick0))) return rc;
    if (W == 0) return EMP_OK;
    const size_t nA = (size_t)W * max_world, n_log = plan.n_log;
    EMP_STAGE(st, where);
    const bool z = where == EMP_HOST;          // staged outputs start from 0; the caller's device memory is never filled
    bhv::WorldIO io{};
    hz::HazardIO hio{};
    stage_traffic_hazards(st, a, h, (size_t)W, (size_t)max_world, (size_t)max_path, (size_t)max_other, (size_t)max_light, (size_t)max_walker,
                          tick0, z, &io, &hio);
    io.other_tick0 = (long long)other_tick0;
    io.T = T;
    io.log_every = log_every;
    io.log_state = st.out(a->log_state, n_log * nA * 6, z);
    io.log_control = st.out(a->log_control, n_log * nA * 3, z);
    io.log_head = st.out(a->log_head, n_log * nA, z);
    io.log_mode = st.out(a->log_mode, n_log * nA, z);
    io.log_target = st.out(a->log_target, n_log * nA, z);
    hio.log_cause = st.out(h->log_cause, n_log * nA, z);
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch_traffic_hazards(ctx, plan, p, bp, hp, vp, nA, io, hio)) return rc;
    return st.finish();
}

}  // namespace

extern "C" {

int emp_traffic_rollout_hazards(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp,
                                int32_t W, int32_t max_world, int32_t max_path, int32_t max_other, int32_t T, int32_t log_every,
                                int64_t tick0, const emp_behavior_io* a, emp_mem where, const emp_hazard_params* hp, int32_t max_light,
                                int32_t max_walker, const emp_hazard_io* h) {
    return traffic_rollout_hazards_impl(ctx, p, bp, vp, W, max_world, max_path, max_other, T, log_every, tick0, a, where, hp, max_light,
                                        max_walker, h, 0);
}

int emp_traffic_rollout_epoch(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp,
                              int32_t W, int32_t max_world, int32_t max_path, int32_t max_other, int32_t T, int32_t log_every,
                              int64_t tick0, const emp_behavior_io* a, emp_mem where, const emp_hazard_params* hp, int32_t max_light,
                              int32_t max_walker, const emp_hazard_io* h, int64_t other_tick0) {
    return traffic_rollout_hazards_impl(ctx, p, bp, vp, W, max_world, max_path, max_other, T, log_every, tick0, a, where, hp, max_light,
                                        max_walker, h, other_tick0);
}

}  // extern "C"

// ---- one world for a planning fleet and reacting traffic (emp_world_core.h, emp_world_kernels.h) -----------------------------------
namespace {

wx::Sizes exchange_sizes(int W, int max_world, int B, int max_global, int max_act, int max_other, int lane_window, int see_egos) {
    return wx::Sizes{W, B, max_world, max_global, max_act, max_other, lane_window, see_egos};
}

int launch_exchange(emp_ctx* ctx, const wx::ExchangePlan& plan, const wx::Sizes& z, const double* agent_state, const wx::In& in,
                    const wx::Out& out) {
    return launch(ctx, "world_exchange", wx::world_exchange_kernel, dim3(plan.grid), dim3(plan.block), 0, z, agent_state, in, out);
}

// emp_world_drive's periods around drive_impl's: the arrays of the traffic and of the exchange, staged once, and the two launches
struct WorldPeriods : DriveWorld {
    emp_ctx* ctx;
    const emp_agent_params* p;
    const emp_behavior_params* bp;
    const emp_vehicle_params* avp;
    const emp_hazard_params* hp;
    const emp_world_params* wp;
    const emp_world_io* w;
    wx::Sizes z;
    wx::ExchangePlan xplan;
    bhv::BehaviorPlan tplan;
    wx::WorldClockPlan clock;
    bool host;
    size_t nA = 0, nB = 0;
    bhv::WorldIO io{};
    hz::HazardIO hio{};
    const int* d_off = nullptr;
    const double* d_extent = nullptr;
    const int* d_elane = nullptr;
    double *x_actors = nullptr, *x_other = nullptr, *l_astate = nullptr, *l_gap = nullptr, *l_wgap = nullptr;
    int *x_nact = nullptr, *x_status = nullptr, *x_okey = nullptr, *x_nother = nullptr;
    int *l_wx = nullptr, *l_nact = nullptr, *l_status = nullptr, *l_done = nullptr, *l_modes = nullptr, *l_causes = nullptr;

    void stage_in(Stage& st) override {
        d_off = st.in(w->ego_off, (size_t)z.W + 1);
        d_extent = st.in(w->ego_extent, nB);
        d_elane = st.in(w->ego_lane, nB * z.max_global);
    }
    void stage_out(Stage& st, size_t nK) override {
        // the others are the exchange's: emp_behavior_io's are not read
        stage_traffic_hazards(st, w->agents, w->hazards, (size_t)z.W, (size_t)z.max_world, (size_t)wp->max_path, 0, (size_t)wp->max_light,
                              (size_t)wp->max_walker, clock.atick0, host, &io, &hio);
        io.T = io.log_every = clock.Ta;
        x_actors = st.tmp<double>(nB * z.max_act * 4);
        x_nact = st.tmp<int>(nB);
        x_status = st.tmp<int>(nB);
        if (z.max_other > 0) {
            x_other = st.tmp<double>((size_t)z.W * z.max_other * 5);
            x_okey = st.tmp<int>((size_t)z.W * z.max_other);
            x_nother = st.tmp<int>((size_t)z.W);
        }
        io.max_other = z.max_other;
        io.n_other = x_nother;
        io.other = x_other;
        io.other_lane = x_okey;
        l_wx = st.out(w->log_wx_status, nK * nB, false);
        l_nact = st.out(w->log_n_act, nK * nB, false);
        l_astate = st.out(w->log_agent_state, nK * nA * 6, false);
        l_status = st.out(w->log_agent_status, nK * nA, false);
        l_done = st.out(w->log_done_tick, nK * nA, false);
        l_modes = st.out(w->log_mode_ticks, nK * nA * bhv::kCountedModes, false);
        l_causes = st.out(w->log_cause_ticks, nK * nA * hz::kCountedCauses, false);
        l_gap = st.out(w->log_min_gap, nK * nA, false);
        l_wgap = st.out(w->log_min_walker_gap, nK * nA, false);
    }
    // a log row is the period's output array as it stands
    template <typename T>
    int keep(T* log, int k, const T* src, size_t n) {
        if (!log) return EMP_OK;
        EMP_HIP(ctx, hipMemcpyAsync(log + (size_t)k * n, src, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        return EMP_OK;
    }
    int exchange(int k, const double* global_path, const int* n_global, const double* state, const int* pre_match_index) override {
        if (k) {                                           // the agents go on from where the last period left them
            io.state = io.state_out;
            io.st.head_in = io.st.head_out;
            io.st.past_in = io.st.past_out;
            io.st.lon_in = io.st.lon_out;
            io.st.n_lon_in = io.st.n_lon_out;
            io.st.lat_in = io.st.lat_out;
            io.st.n_lat_in = io.st.n_lat_out;
            hio.last_light = hio.last_light_out;
        }
        const wx::In in{io.n_world, d_off, state, d_extent, global_path, n_global, d_elane, pre_match_index};
        int* nact = l_nact ? l_nact + (size_t)k * nB : x_nact;
        const wx::Out out{x_actors, nact, x_other, x_okey, x_nother, l_wx ? l_wx + (size_t)k * nB : x_status};
        actors = x_actors;
        n_act = nact;
        return launch_exchange(ctx, xplan, z, io.state, in, out);
    }
    int traffic(int k) override {
        if (const int rc = keep(l_astate, k, io.state, nA * 6)) return rc;
        io.tick0 = io.other_tick0 = (long long)clock.tick(k);
        if (const int rc = launch_traffic_hazards(ctx, tplan, p, bp, hp, avp, nA, io, hio)) return rc;
        if (const int rc = keep(l_status, k, (const int*)io.status, nA)) return rc;
        if (const int rc = keep(l_done, k, (const int*)io.done_tick, nA)) return rc;
        if (const int rc = keep(l_modes, k, (const int*)io.mode_ticks, nA * bhv::kCountedModes)) return rc;
        if (const int rc = keep(l_causes, k, (const int*)hio.cause_ticks, nA * hz::kCountedCauses)) return rc;
        if (const int rc = keep(l_gap, k, (const double*)io.min_gap, nA)) return rc;
        return keep(l_wgap, k, (const double*)hio.min_walker_gap, nA);
    }
};

}  // namespace

extern "C" {

void emp_world_params_default(emp_world_params* p) {
    if (!p) return;
    p->W = 0;
    p->max_world = 1;
    p->max_path = 1;
    p->max_other = 0;
    p->max_light = p->max_walker = 0;
    p->Ta = 1;
    p->lane_window = 50;
    p->see_egos = 0;
    p->reserved = 0;
    p->atick0 = 0;
}

int emp_world_exchange(emp_ctx* ctx, int32_t W, int32_t max_world, int32_t B, int32_t max_global, int32_t max_act, int32_t max_other,
                       int32_t lane_window, int32_t see_egos, const emp_world_exchange_io* a, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE, "emp_world_exchange takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, a != nullptr, "NULL parameter struct");
    EMP_REQUIRE(ctx, a->reserved == 0, "emp_world_exchange_io.reserved must be 0");
    const wx::ExchangePlan plan = wx::plan_exchange(W, B, max_world, max_global, max_act, max_other, lane_window, see_egos);
    if (const int rc = plan_refused(ctx, plan.error)) return rc;
    EMP_REQUIRE(ctx, a->n_world && a->agent_state && a->ego_off && a->ego_state && a->ego_extent && a->global_path && a->n_global &&
                         a->ego_lane && a->pre_match_index && a->actors && a->n_act && a->wx_status,
                "NULL array");
    EMP_REQUIRE(ctx, max_other == 0 || (a->other && a->other_lane && a->n_other), "max_other > 0 needs other, other_lane and n_other");
    if (where == EMP_HOST)
        if (const int rc = plan_refused(ctx, wx::ego_off_error(a->ego_off, W, B))) return rc;
    if (W == 0 || B == 0) return EMP_OK;
    const size_t nA = (size_t)W * max_world, nB = (size_t)B;
    EMP_STAGE(st, where);
    const double* d_agents = st.in(a->agent_state, nA * 6);
    wx::In in{};
    in.n_world = st.in(a->n_world, (size_t)W);
    in.ego_off = st.in(a->ego_off, (size_t)W + 1);
    in.ego_state = st.in(a->ego_state, nB * 6);
    in.ego_extent = st.in(a->ego_extent, nB);
    in.global_path = st.in(a->global_path, nB * max_global * 4);
    in.n_global = st.in(a->n_global, nB);
    in.ego_lane = st.in(a->ego_lane, nB * max_global);
    in.pre_match_index = st.in(a->pre_match_index, nB);
    wx::Out out{};
    out.actors = st.out(a->actors, nB * max_act * 4, false);
    out.n_act = st.out(a->n_act, nB, false);
    out.wx_status = st.out(a->wx_status, nB, false);
    if (max_other > 0) {
        out.other = st.out(a->other, (size_t)W * max_other * 5, false);
        out.other_lane = st.out(a->other_lane, (size_t)W * max_other, false);
        out.n_other = st.out(a->n_other, (size_t)W, false);
    }
    if (const int rc = st.ready()) return rc;
    if (const int rc = launch_exchange(ctx, plan, exchange_sizes(W, max_world, B, max_global, max_act, max_other, lane_window, see_egos),
                                       d_agents, in, out))
        return rc;
    return st.finish();
}

int emp_world_drive(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth,
                    const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp, const emp_drive_params* drv,
                    const emp_drive_timed_params* tp, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid,
                    const emp_vehicle_params* vp, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* avp,
                    const emp_hazard_params* hp, const emp_world_params* wp, int32_t B, int32_t max_global, int32_t max_obs,
                    int32_t max_pts, int32_t max_act, int32_t max_dyn, int32_t K, int32_t T, int32_t tick0, const double* target_speed,
                    const emp_world_io* io, emp_mem where) {
    EMP_REQUIRE(ctx, ctx != nullptr, "ctx is NULL");
    EMP_REQUIRE(ctx, dp && qp && smooth && sdp && sqp && drv && tp && lat && pid && vp && p && bp && avp && hp && wp && io,
                "NULL parameter struct");
    EMP_REQUIRE(ctx, io->agents && io->hazards, "NULL parameter struct");
    EMP_REQUIRE(ctx, drv->reserved == 0, "emp_drive_params.reserved must be 0");
    EMP_REQUIRE(ctx, tp->reserved == 0, "emp_drive_timed_params.reserved must be 0");
    EMP_REQUIRE(ctx, std::isfinite(tp->plan_lead), "emp_drive_timed_params.plan_lead must be finite");
    EMP_REQUIRE(ctx, wp->reserved == 0, "emp_world_params.reserved must be 0");
    EMP_REQUIRE(ctx, io->reserved == 0, "emp_world_io.reserved must be 0");
    if (const int rc = rollout_args_ok(ctx, lateral, vp, T, 1)) return rc;
    EMP_REQUIRE(ctx, qp_reserved_ok(qp), "emp_qp_params.reserved must be 0 (start from emp_qp_params_default)");
    EMP_REQUIRE(ctx, where == EMP_HOST || where == EMP_DEVICE,
                "emp_world_drive takes EMP_HOST or EMP_DEVICE arrays (EMP_HOST_PINNED is emp_plan_cycle's)");
    EMP_REQUIRE(ctx, K >= 1 && K <= EMP_DRIVE_MAX_PERIODS, "K must be in [1, 4096]");
    // the exchange's rules, the traffic's, the two clocks'
    WorldPeriods wd;
    wd.xplan = wx::plan_exchange(wp->W, B, wp->max_world, max_global, max_act, wp->max_other, wp->lane_window, wp->see_egos);
    if (const int rc = plan_refused(ctx, wd.xplan.error)) return rc;
    wd.clock = wx::plan_world_clock(K, T, vp->dt, wp->Ta, p->dt, wp->atick0);
    if (const int rc = plan_refused(ctx, wd.clock.error)) return rc;
    wd.tplan = hz::plan_hazards(wp->W, wp->max_world, wp->max_other, wp->max_light, wp->max_walker, wp->max_path, wp->Ta, wp->Ta,
                                wd.clock.tick(K - 1));
    if (const int rc = traffic_hazards_checks(ctx, p, bp, avp, io->agents, 0, where, wd.tplan, hp, wp->max_light, wp->max_walker, io->hazards))
        return rc;
    EMP_REQUIRE(ctx, !io->agents->log_state && !io->agents->log_control && !io->agents->log_head && !io->agents->log_mode &&
                         !io->agents->log_target && !io->hazards->log_cause,
                "emp_world_drive keeps no tick logs: the log_* arrays of emp_behavior_io and emp_hazard_io must be NULL");
    EMP_REQUIRE(ctx, io->ego_off && io->ego_extent && io->ego_lane, "NULL input array");
    if (where == EMP_HOST)
        if (const int rc = plan_refused(ctx, wx::ego_off_error(io->ego_off, wp->W, B))) return rc;
    // emp_drive_timed's arrays under their names
    emp_drive_timed_io tio{};
    tio.global_path = io->global_path;
    tio.n_global = io->n_global;
    tio.state = io->state;
    tio.accel = io->accel;
    tio.pre_match_index = io->pre_match_index;
    tio.track = io->track;
    tio.track_len = io->track_len;
    tio.held = io->held;
    tio.t0 = io->t0;
    tio.profile = io->profile;
    tio.cursor = io->cursor;
    tio.speed_held = io->speed_held;
    tio.state_out = io->state_out;
    tio.accel_out = io->accel_out;
    tio.actors_out = io->actors_out;
    tio.pre_match_index_out = io->pre_match_index_out;
    tio.track_out = io->track_out;
    tio.track_len_out = io->track_len_out;
    tio.held_out = io->held_out;
    tio.profile_out = io->profile_out;
    tio.cursor_out = io->cursor_out;
    tio.speed_held_out = io->speed_held_out;
    tio.log_state = io->log_state;
    tio.log_plan_status = io->log_plan_status;
    tio.log_roll_status = io->log_roll_status;
    tio.log_held = io->log_held;
    tio.log_counts = io->log_counts;
    tio.log_traj = io->log_traj;
    tio.log_traj_len = io->log_traj_len;
    tio.log_speed_status = io->log_speed_status;
    tio.log_speed_held = io->log_speed_held;
    tio.log_tgt_status = io->log_tgt_status;
    tio.log_cursor = io->log_cursor;
    tio.log_profile = io->log_profile;
    if (B == 0 || wp->W == 0) {                            // nothing runs; emp_drive_timed's own refusals still hold
        if (const int rc = plan_refused(ctx, plan_drive_clock(tick0, K, T).error)) return rc;
        return EMP_OK;
    }
    wd.ctx = ctx;
    wd.p = p;
    wd.bp = bp;
    wd.avp = avp;
    wd.hp = hp;
    wd.wp = wp;
    wd.w = io;
    wd.z = exchange_sizes(wp->W, wp->max_world, B, max_global, max_act, wp->max_other, wp->lane_window, wp->see_egos);
    wd.host = where == EMP_HOST;
    wd.nA = (size_t)wp->W * wp->max_world;
    wd.nB = (size_t)B;
    return drive_timed_impl(ctx, dp, qp, smooth, sdp, sqp, drv, tp, lateral, lat, pid, vp, B, max_global, max_obs, max_pts, max_act, max_dyn, K, T,
                            tick0, target_speed, &tio, where, &wd);
}

}  // extern "C"
