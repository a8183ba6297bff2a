// emp_context.h - context object behind the C-ABI: device, stream, scratch pool, host staging, timing.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/emplanner.h"

// an atomic that a std::vector element may hold (movable: the move is a plain load / store, made only while no other thread
// can be looking - emp_set_pipeline resizing the lanes)
template <typename T>
struct Shared {
    std::atomic<T> v;
    Shared(T x = T()) : v(x) {}
    Shared(Shared&& o) noexcept : v(o.v.load()) {}
    Shared& operator=(T x) { v.store(x, std::memory_order_release); return *this; }
    operator T() const { return v.load(std::memory_order_acquire); }
};

struct emp_ctx;

namespace emp {

// Owners of the context's HIP resources: move-only, one handle each, released by the destructor.  A destructor never
// synchronises: what releases a resource that queued work may still use drains first (emp_destroy, grow_buffer).
template <typename H, hipError_t (*Release)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { (void)reset(); }
    operator H() const { return h; }
    hipError_t reset() {
        const hipError_t e = h ? Release(h) : hipSuccess;
        h = nullptr;
        return e;
    }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    int ensure(emp_ctx* ctx, unsigned flags);                               // created on first use
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    int ensure(emp_ctx* ctx, unsigned flags, bool high_priority = false);   // created on first use
};
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

// device memory (hipMalloc) or, kHost, page-locked host memory (hipHostMalloc), and its size
template <bool kHost>
struct Mem {
    void* p = nullptr;
    size_t bytes = 0;
    Mem() = default;
    Mem(Mem&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Mem& operator=(Mem&& o) noexcept {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~Mem() { (void)reset(); }
    hipError_t reset() {
        const hipError_t e = !p ? hipSuccess : kHost ? hipHostFree(p) : hipFree(p);
        p = nullptr;
        bytes = 0;
        return e;
    }
    int ensure(emp_ctx* ctx, size_t n);                                     // n bytes, allocated on first use
};

}  // namespace emp

struct emp_ctx {
    using Buf = emp::Mem<false>;
    using HostBlock = emp::Mem<true>;
    int device = 0;
    emp::Stream main_stream;            // the first owner: released last
    // the stream the launchers issue to: the main stream, or what stands in for it during a call (a lane's stream, the back
    // stream, the result stream)
    hipStream_t stream = nullptr;
    std::string err;
    // grow-only pool of device buffers, handed out in call order and recycled by the next call
    std::vector<Buf> pool;
    size_t cursor = 0;
    // emp_drive's own pool: its staged arrays and temporaries live through the K cycles of the call, each of which recycles `pool`
    std::vector<Buf> drive_pool;
    // persistent named scratch (survives across the staged buffers of one call)
    std::map<std::string, Buf> named;
    std::string timing_filter;   // non-empty: only this kernel name is bracketed by events
    // the pair table of the edge-cost kernel and the lattice parameters it was built for (emp_api.hip: dp_pair_table);
    // one per stream that runs edge kernels (key: active_lane), so that a rebuild never races a reader on another stream
    struct PairTable {
        Buf buf;
        double key[8] = {0};
        bool valid = false;
    };
    std::map<int, PairTable> pair_tables;
    // per-kernel timing
    bool timing = false;
    struct Ev {
        std::vector<std::pair<emp::Event, emp::Event>> pairs;   // one pair per launch since timing was enabled
        size_t used = 0;
    };
    std::map<std::string, Ev> events;
    int cu_count = 0;
    // Several batches in flight (emp_set_pipeline), two forms.
    // STAGED (mode 1, two batches): a cycle is a front stage (projection, edge costs, sweep) on `stream` and a back stage
    // (densified DP path, path QP, Cartesian tail) on `back_stream`; the back stage of call k overlaps the front stage of
    // call k+1.  The two calls in flight alternate between lanes[0] and lanes[1], of which only the pool of temporaries
    // and the events are used.  The front stages are serial, so one edge tensor serves every call (it stays in the
    // Infinity Cache) and the sweep overlaps nothing but the tail of the back stage before it.
    // LANES (mode n >= 2, n batches): call k runs WHOLE on the stream of lanes[k mod n], with that lane's pool, edge
    // tensor and pair table, behind everything queued on `stream` when it was issued; the dispatcher overlaps the kernels
    // of n consecutive cycles wherever it finds room.
    // ev_in: recorded on `stream` by a LANES call, its lane waits for it.  ev_front: end of a STAGED front stage.
    // ev_tail: LANES, the lane stream's tail when the lane is taken again - the main stream waits for it, so that memory
    // the caller releases once call k + n is issued is not handed to a call on ANOTHER lane while call k, or a consumer
    // queued behind it on the lane, still runs (the lanes are ordered behind the main stream, not against each other).
    // ev_done: end of the lane's latest cycle - what the next user of the lane's pool and every other entry point wait for.
    struct Lane {
        emp::Stream stream;
        emp::Event ev_in, ev_front, ev_done, ev_tail;
        emp::Event ev_host;             // EMP_HOST_PINNED cycles: the lane's latest cycle's outputs have reached the caller's host arrays
        // `ticket` and `host_valid` are the two fields emp_wait_ticket reads from ANOTHER thread while a call is in progress:
        // atomics, and a call that takes the lane over changes them only AFTER its own host-side wait for the previous
        // occupant's outputs (emp_plan_cycle) - until then the lane still answers for the previous ticket
        Shared<bool> host_valid{false};
        Shared<uint64_t> ticket{0};     // emp_cycle_ticket of the lane's latest cycle
        emp::Event ev_qp;               // STAGED: end of the cycle's path QP on the back stream (EMP_OPT_SWEEP_EXCLUSIVE = 2)
        emp::Event ev_enrich;           // STAGED: end of the cycle's densification kernel on the back stream (EMP_OPT_EDGE_AFTER_ENRICH)
        emp::Event ev_edge;             // LANES: end of the cycle's edge-cost kernel (EMP_OPT_LANE_EDGE_ORDER)
        bool done_valid = false, qp_valid = false, enrich_valid = false;
        std::vector<Buf> pool;
    };
    std::vector<Lane> lanes;            // created on demand, kept until emp_destroy
    emp::Stream back_stream;            // STAGED: the back stages (highest queue priority)
    // EMP_HOST_PINNED (emp_plan_cycle): inputs go host -> device on copy_stream while the previous call computes, outputs device ->
    // host on d2h_stream behind the cycle's last kernel - neither ever sits on a queue that carries kernels.  Created on first use.
    emp::Stream copy_stream, d2h_stream;
    emp::Event ev_h2d;                  // the latest call's inputs have arrived
    emp::Event ev_host_last;            // non-pipelined pinned call: outputs have reached the host
    std::vector<HostBlock> pinned;      // emp_host_alloc allocations still alive
    // Small EMP_HOST calls (round 6): ONE page-locked arena and one device arena per direction.  The arrays of a synchronous call
    // with host pointers are packed into the input arena by the host and cross PCIe as one copy; the outputs come back as one
    // copy and are unpacked by the host (Stage).  A copy command costs 4-14 us whatever its size and a call of the reference's
    // function surface has three to twenty small arrays: emp_lmin_lmax went from 100 to ~60 us (profiles/r06_call_cost_probe.txt).
    static constexpr size_t kArena = 256 * 1024, kArenaArray = 64 * 1024;
    HostBlock arena_h_in, arena_h_out;  // kArena bytes each
    Buf arena_d_in, arena_d_out;
    bool arena_failed = false;          // an allocation failed once: the per-array path from then on
    bool stage_open = false;            // a Stage is in its input phase: kernel launches are refused until its ready()
    int pipe_mode = 0;                  // 0 off, 1 STAGED, n >= 2 LANES with n lanes
    int lane = 0;                       // lane of the latest pipelined cycle call
    uint64_t cycle_calls = 0;           // pipelined emp_plan_cycle calls issued so far (emp_cycle_ticket)
    int active_lane = -1;               // LANES: the lane whose stream and pool stand in for `stream` / `pool` right now
    bool fence = true;                  // emp_set_fence: other entry points wait for the cycles in flight
    // emp_set_option (include/emplanner.h): per-context tuning / A-B / test-hook values; the library reads no environment
    int32_t opt[EMP_OPT_COUNT] = {0, 0, 0, 0, 0, 0, /* EDGE_AFTER_ENRICH */ 1, /* LANE_EDGE_ORDER */ 2, 0, 0, 0, /* FOREIGN_STREAMS */ 1};
    int auto_queues = 0, auto_streams = 0;   // what the latest emp_set_pipeline(EMP_PIPELINE_AUTO) saw (emp_pipeline_form)
    // EMP_OPT_CYCLE_GRAPH (emp_api.hip CycleCapture): the launches of one emp_plan_cycle call as an executable graph, the call
    // signature it belongs to, how often that signature has been seen in a row, and the allocation count it was captured under
    struct CycleGraph {
        emp::GraphExec exec;
        std::vector<unsigned long long> key, seen_key;
        int seen = 0;
        long long replays = 0;
        unsigned long long gen = 0;
        bool capturing = false;         // launchers avoid what a stream capture cannot record (hipExtLaunchKernelGGL)
    } cycle_graph;
    unsigned long long alloc_gen = 0;   // buffers (grow_buffer) and pair tables made so far
    hipEvent_t lane_edge_done = nullptr; // EMP_OPT_LANE_EDGE_ORDER: recorded behind the latest edge-cost launch of a lane-mode call (a lane's ev_edge)
    emp::Event sweep_marker;            // EMP_OPT_SWEEP_EXCLUSIVE: recorded on the front stream behind the sweep (emp_api.hip)
    // EMP_OPT_SWEEP_CLOCK_PROBE: a ring of kProbeSlots launches x [tiles][4] ticks (shader-clock begin / end, reference
    // begin / end); probe_launches counts the launches recorded since the option was last switched on
    static constexpr int kProbeSlots = 32;
    Buf clock_probe;
    Buf edge_probe;                     // EMP_OPT_EDGE_CLOCK_PROBE: [wavefronts of the latest edge launch][2] reference ticks
    long edge_probe_waves = 0;
    emp::Event edge_probe_done;
    int clock_probe_tiles = 0;
    long probe_launches = 0;
    emp::Event clock_probe_done;
    bool pipelined() const { return pipe_mode != 0; }
    // STAGED rotates kStagedPools pools of temporaries although only two calls overlap on the GPU: call k reuses the pool
    // of call k - 4 and the HOST waits for that call's back stage (long finished unless the host runs more than four
    // calls ahead, which this also bounds) - no barrier packet on the queue of the front stages.  With two pools the
    // stream had to wait for call k - 2 on the GPU: a cross-queue dependency in front of every projection kernel, ~11 us
    // of the command processor's time per 0.29 ms step on the queue that is the step's critical path.
    static constexpr int kStagedPools = 4;
    int lanes_in_use() const { return pipe_mode == 1 ? kStagedPools : pipe_mode; }
    hipStream_t result_stream() const {
        return pipe_mode == 0 ? main_stream.h : pipe_mode == 1 ? back_stream.h : lanes[lane].stream.h;
    }
};

namespace emp {

extern thread_local std::string g_create_error;

inline int fail(emp_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

// the error of a failed HIP call (`what`: the call's text), or EMP_OK
inline int hip_error(emp_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return EMP_OK;
    (void)hipGetLastError();    // the runtime keeps the error for the next hipGetLastError(): without this, the launch check
                                // of the NEXT call would report this call's failure
    return fail(ctx, e == hipErrorOutOfMemory ? EMP_ERR_NOMEM : EMP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define EMP_HIP(ctx, call)                                                                         \
    do {                                                                                           \
        if (const int rc_ = emp::hip_error((ctx), (call), #call)) return rc_;                      \
    } while (0)

#define EMP_REQUIRE(ctx, cond, msg)                                                               \
    do {                                                                                           \
        if (!(cond)) return emp::fail((ctx), EMP_ERR_INVALID, std::string(msg));                   \
    } while (0)

inline int Event::ensure(emp_ctx* ctx, unsigned flags) {
    return h ? EMP_OK : hip_error(ctx, hipEventCreateWithFlags(&h, flags), "hipEventCreateWithFlags");
}

// high_priority: the device's highest stream priority (the STAGED back stream)
inline int Stream::ensure(emp_ctx* ctx, unsigned flags, bool high_priority) {
    if (h) return EMP_OK;
    if (!high_priority) return hip_error(ctx, hipStreamCreateWithFlags(&h, flags), "hipStreamCreateWithFlags");
    int prio_low = 0, prio_high = 0;
    EMP_HIP(ctx, hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    return hip_error(ctx, hipStreamCreateWithPriority(&h, flags, prio_high), "hipStreamCreateWithPriority");
}

template <bool kHost>
inline int Mem<kHost>::ensure(emp_ctx* ctx, size_t n) {
    if (p) return EMP_OK;
    const hipError_t e = kHost ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
    if (const int rc = hip_error(ctx, e, kHost ? "hipHostMalloc" : "hipMalloc")) return rc;
    bytes = n;
    return EMP_OK;
}

// Waits for everything queued on the context's streams (the main one and every lane).
inline int sync_all(emp_ctx* ctx) {
    hipError_t e = hipStreamSynchronize(ctx->main_stream);
    for (auto& ln : ctx->lanes) {
        const hipError_t e2 = ln.stream ? hipStreamSynchronize(ln.stream) : hipSuccess;
        if (e == hipSuccess) e = e2;
    }
    for (hipStream_t st : {ctx->back_stream.h, ctx->copy_stream.h, ctx->d2h_stream.h}) {
        if (!st) continue;
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
    }
    return (int)e;
}

// Grow-only device buffer with 25 % headroom.  A buffer is replaced only once nothing queued on any of the context's
// streams can still touch it (hipFree's own implicit synchronisation is not relied upon).
inline int grow_buffer(emp_ctx* ctx, emp_ctx::Buf& b, size_t bytes) {
    if (b.bytes >= bytes) return EMP_OK;
    if (b.p) {
        EMP_HIP(ctx, (hipError_t)sync_all(ctx));
        EMP_HIP(ctx, b.reset());
    }
    if (const int rc = b.ensure(ctx, bytes + bytes / 4)) return rc;
    ++ctx->alloc_gen;
    return EMP_OK;
}

// device scratch from the per-call pool
inline int pool_get(emp_ctx* ctx, size_t bytes, void** out) {
    if (bytes == 0) bytes = 8;
    if (ctx->cursor == ctx->pool.size()) ctx->pool.push_back({});
    emp_ctx::Buf& b = ctx->pool[ctx->cursor++];
    const int rc = grow_buffer(ctx, b, bytes);
    if (rc) return rc;
    *out = b.p;
    return EMP_OK;
}

// (inside Stage: keeps the first failure of a HIP call, true when it succeeded)
#define EMP_KEEP(call) keep(emp::hip_error(ctx_, (call), #call))

// Staging of one call's arguments.  For EMP_DEVICE pointers pass through; for EMP_HOST inputs are copied to the device and
// outputs are copied back in finish().  A call stages its inputs, then its outputs and temporaries, then calls ready(): the one
// check in front of its first launch.  Every staging call does nothing once one has failed; ready() returns that first failure,
// sends the packed inputs still on the host and ends the input phase.  Until then the context refuses kernel launches
// (emp_api.hip: launch_gate), and after it in() is refused.
class Stage {
  public:
    // in_cycle: the pipelined emp_plan_cycle (and a launch placed on its lane) orders itself; every OTHER call in
    // pipelined mode first lets the main stream wait for the cycles still in flight, so that it may consume a cycle's
    // outputs as before
    // async_host (emp_plan_cycle with EMP_HOST_PINNED): the caller's arrays are page-locked (emp_host_alloc) - inputs are copied
    // on ctx->copy_stream (inputs_ready() orders the compute stream behind them), outputs on ctx->d2h_stream behind `after`
    // (finish_async), and nothing blocks the host
    Stage(emp_ctx* c, emp_mem where, bool in_cycle = false, bool async_host = false)
        : ctx_(c), dev_(where == EMP_DEVICE), async_(async_host && where != EMP_DEVICE) {
        c->cursor = 0;
        c->stage_open = true;
        arena_ = !dev_ && !async_ && where == EMP_HOST && !c->cycle_graph.capturing;
        if (!in_cycle && c->pipelined() && c->fence)
            for (auto& ln : c->lanes)
                if (ln.done_valid) (void)hipStreamWaitEvent(c->stream, ln.ev_done, 0);
    }
    ~Stage() { ctx_->stage_open = false; }
    Stage(const Stage&) = delete;
    Stage& operator=(const Stage&) = delete;

    // The device copy of an input (null for a null host pointer).  async_host: the device pointers are known only once every
    // input is (inputs_ready() fills *slot then) - emp_plan_cycle's form with a slot.
    template <typename T>
    const T* in(const T* host, size_t n) { return (const T*)stage_in(host, n * sizeof(T), nullptr); }
    template <typename T>
    void in(const T* host, size_t n, const T** slot) { *slot = (const T*)stage_in(host, n * sizeof(T), (void**)slot); }
    // Outputs are zero-filled on the context's stream before the kernels run, so padding beyond a scene's length reads as 0 in
    // both memory spaces (pass zero=false for arrays the kernels fully overwrite).  async_host: outputs_ready() fills *slot.
    template <typename T>
    T* out(T* host, size_t n, bool zero = true) { return (T*)stage_out(host, n * sizeof(T), zero, nullptr); }
    template <typename T>
    void out(T* host, size_t n, T** slot, bool zero) { *slot = (T*)stage_out(host, n * sizeof(T), zero, (void**)slot); }
    // device-only temporary
    template <typename T>
    T* tmp(size_t n, bool zero = false) {
        if (!flush_inputs()) return nullptr;
        void* v = get(n * sizeof(T));
        if (v && zero && n) EMP_KEEP(hipMemsetAsync(v, 0, n * sizeof(T), ctx_->stream));
        return rc_ ? nullptr : (T*)v;
    }
    // an optional output (not zero-filled): the caller's array, or a device temporary where the caller passed none
    template <typename T>
    void out_or_tmp(T* host, size_t n, T** slot) {
        out(host, n, slot, false);
        if (!*slot) *slot = tmp<T>(n);
    }
    // async_host: every input of the call is known.  Arrays that lie side by side in host memory (a HostRing slot is ONE
    // page-locked block: api.py) get one device block at the same offsets and cross PCIe as ONE copy - a copy command costs
    // 10-20 us of host and engine time whatever its size, and a call has nine inputs; others are copied one by one.  Then the
    // compute stream waits for the copy stream.
    void inputs_ready() {
        if (!async_ || rc_ || !place(ins_, true)) return;
        if (EMP_KEEP(hipEventRecord(ctx_->ev_h2d, ctx_->copy_stream))) EMP_KEEP(hipStreamWaitEvent(ctx_->stream, ctx_->ev_h2d, 0));
    }
    // async_host: every output of the call is known - device buffers for them, one block where the host arrays are one block
    void outputs_ready() {
        if (async_ && !rc_) place(backs_, false);
    }
    // The check in front of the call's first launch (see above).  A temporary staged after it (emp_plan_cycle) is checked by
    // calling it again.
    int ready() {
        flush_inputs();
        open_ = ctx_->stage_open = false;
        return rc_;
    }
    // async_host: copy the outputs back on the d2h stream once `after` (the cycle's completion event) has fired, then signal `done`
    int finish_async(hipEvent_t after, hipEvent_t done) {
        EMP_HIP(ctx_, hipStreamWaitEvent(ctx_->d2h_stream, after, 0));
        if (block_out_.bytes) {
            EMP_HIP(ctx_, hipMemcpyAsync(block_out_.host, block_out_.dev, block_out_.bytes, hipMemcpyDeviceToHost, ctx_->d2h_stream));
        } else {
            for (auto& b : backs_)
                if (b.bytes) EMP_HIP(ctx_, hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, ctx_->d2h_stream));
        }
        EMP_HIP(ctx_, hipEventRecord(done, ctx_->d2h_stream));
        return EMP_OK;
    }
    bool async_host() const { return async_; }
    int finish() {
        if (rc_) return rc_;
        for (auto& b : backs_)
            if (b.bytes) EMP_HIP(ctx_, hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, ctx_->stream));
        if (out_used_) EMP_HIP(ctx_, hipMemcpyAsync(ctx_->arena_h_out.p, ctx_->arena_d_out.p, out_used_, hipMemcpyDeviceToHost, ctx_->stream));
        if (!dev_) EMP_HIP(ctx_, hipStreamSynchronize(ctx_->stream));
        for (size_t i = 0; i < arena_backs_.size(); ++i)
            if (arena_backs_[i].bytes) memcpy(arena_backs_[i].host, (char*)ctx_->arena_h_out.p + arena_offs_[i], arena_backs_[i].bytes);
        return EMP_OK;
    }

  private:
    struct Back {
        void* host;
        void* dev;
        size_t bytes;
        void** slot;       // async_host: where the device pointer goes once it is known
    };
    static constexpr uintptr_t kPending = 8;     // non-null placeholder of a deferred pointer (never dereferenced)
    // keeps the first failure of the call; true when `rc` is none
    bool keep(int rc) {
        if (rc) rc_ = rc;
        return rc == EMP_OK;
    }
    bool refuse(const char* msg) { return keep(emp::fail(ctx_, EMP_ERR_INVALID, msg)); }
    void* get(size_t bytes) {
        void* d = nullptr;
        return keep(pool_get(ctx_, bytes, &d)) ? d : nullptr;
    }
    // deferred (async_host): the device pointer is written to *slot by place()
    void* defer(std::vector<Back>& v, void* host, size_t bytes, void** slot) {
        if (!slot) {
            refuse("internal: an EMP_HOST_PINNED array was staged without a slot");
            return nullptr;
        }
        v.push_back({host, nullptr, bytes, slot});
        return (void*)kPending;
    }
    const void* stage_in(const void* host, size_t bytes, void** slot) {
        if (rc_ || !host) return nullptr;
        if (!open_) {
            refuse("internal: Stage::in() after ready()");
            return nullptr;
        }
        if (dev_) return host;
        if (async_) return defer(ins_, (void*)host, bytes, slot);
        if (arena_ && arena_take(bytes, &in_used_)) {      // packed: one copy for all small inputs (flush_inputs)
            const size_t off = in_used_ - arena_round(bytes);
            if (bytes) memcpy((char*)ctx_->arena_h_in.p + off, host, bytes);
            return (char*)ctx_->arena_d_in.p + off;
        }
        void* d = get(bytes);
        if (d && bytes) EMP_KEEP(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, ctx_->stream));
        return rc_ ? nullptr : d;
    }
    void* stage_out(void* host, size_t bytes, bool zero, void** slot) {
        if (!flush_inputs() || !host) return nullptr;
        if (async_) return defer(backs_, host, bytes, slot);
        void* d = host;
        if (!dev_) {
            if (arena_ && arena_take(bytes, &out_used_)) {       // packed: one zero fill, one copy back (finish)
                const size_t off = out_used_ - arena_round(bytes);
                if (!out_zeroed_) {      // the whole output arena once per call instead of a memset per array
                    if (!EMP_KEEP(hipMemsetAsync(ctx_->arena_d_out.p, 0, emp_ctx::kArena, ctx_->stream))) return nullptr;
                    out_zeroed_ = true;
                }
                arena_backs_.push_back({host, nullptr, bytes, nullptr});
                arena_offs_.push_back(off);
                return (char*)ctx_->arena_d_out.p + off;
            }
            if (!(d = get(bytes))) return nullptr;
            backs_.push_back({host, d, bytes, nullptr});
        }
        if (zero && bytes && !EMP_KEEP(hipMemsetAsync(d, 0, bytes, ctx_->stream))) return nullptr;
        return d;
    }
    // The packed inputs gathered so far go to the device: ONE copy on the context's stream, issued by the first out() or tmp()
    // and by ready().  False once the call has failed.
    bool flush_inputs() {
        if (!rc_ && in_used_ > in_sent_) {
            if (!EMP_KEEP(hipMemcpyAsync((char*)ctx_->arena_d_in.p + in_sent_, (char*)ctx_->arena_h_in.p + in_sent_, in_used_ - in_sent_,
                                         hipMemcpyHostToDevice, ctx_->stream)))
                return false;
            in_sent_ = in_used_;
        }
        return rc_ == EMP_OK;
    }
    // device memory for a call's arrays (async_host).  ONE device block with the host offsets - and one PCIe copy per direction -
    // only where that provably touches nothing but the call's own arrays: all of them inside ONE emp_host_alloc allocation of
    // this context, with at most kBlockGap bytes (alignment padding) between neighbours.  Outputs moved as a block overwrite
    // that padding (include/emplanner.h, EMP_HOST_PINNED).  Everything else - arrays allocated one by one, a smaller batch at
    // the head of a bigger slot, foreign data carved between two outputs - is copied array by array.
    static constexpr size_t kBlockGap = 512;
    bool one_block(const std::vector<Back>& v, uintptr_t* lo_out, size_t* span_out) const {
        if (v.size() < 2) return false;
        std::vector<std::pair<uintptr_t, size_t>> a;
        for (auto& b : v)
            if (b.bytes) a.push_back({(uintptr_t)b.host, b.bytes});
        if (a.size() < 2) return false;
        std::sort(a.begin(), a.end());
        const uintptr_t lo = a.front().first;
        uintptr_t end = lo;
        for (auto& x : a) {
            if (x.first < end || x.first - end > kBlockGap) return false;      // overlapping, or more than padding in between
            end = x.first + x.second;
        }
        for (auto& al : ctx_->pinned)
            if (lo >= (uintptr_t)al.p && end <= (uintptr_t)al.p + al.bytes) {
                *lo_out = lo;
                *span_out = end - lo;
                return true;
            }
        return false;
    }
    bool place(std::vector<Back>& v, bool inputs) {
        if (v.empty()) return true;
        uintptr_t lo = 0;
        size_t span = 0;
        if (one_block(v, &lo, &span)) {
            void* d = get(span);
            if (!d) return false;
            for (auto& b : v) {
                b.dev = b.bytes ? (char*)d + ((uintptr_t)b.host - lo) : d;
                *b.slot = b.dev;
            }
            if (inputs) return EMP_KEEP(hipMemcpyAsync(d, (void*)lo, span, hipMemcpyHostToDevice, ctx_->copy_stream));
            block_out_ = {(void*)lo, d, span, nullptr};
            return true;
        }
        for (auto& b : v) {
            void* d = get(b.bytes);
            if (!d) return false;
            b.dev = d;
            *b.slot = d;
            if (inputs && b.bytes && !EMP_KEEP(hipMemcpyAsync(d, b.host, b.bytes, hipMemcpyHostToDevice, ctx_->copy_stream)))
                return false;
        }
        return true;
    }
    static size_t arena_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    // room for `bytes` in an arena whose fill mark is *used?  Creates the four arenas on first use; false = take the per-array path
    // (an array of more than kArenaArray bytes - a host memcpy of that size costs more than the copy command it saves - or a full
    // arena, or an arena that could not be allocated: what was allocated stays with the context, unused)
    bool arena_take(size_t bytes, size_t* used) {
        if (bytes > emp_ctx::kArenaArray || *used + arena_round(bytes) > emp_ctx::kArena || ctx_->arena_failed) return false;
        if (ctx_->arena_h_in.ensure(ctx_, emp_ctx::kArena) || ctx_->arena_h_out.ensure(ctx_, emp_ctx::kArena) ||
            ctx_->arena_d_in.ensure(ctx_, emp_ctx::kArena) || ctx_->arena_d_out.ensure(ctx_, emp_ctx::kArena)) {
            ctx_->arena_failed = true;
            return false;
        }
        *used += arena_round(bytes);
        return true;
    }
    emp_ctx* ctx_;
    int rc_ = EMP_OK;                            // the call's first failure
    bool dev_, async_, arena_ = false, out_zeroed_ = false, open_ = true;
    size_t in_used_ = 0, in_sent_ = 0, out_used_ = 0;
    std::vector<Back> arena_backs_;
    std::vector<size_t> arena_offs_;
    std::vector<Back> backs_, ins_;
    Back block_out_ = {nullptr, nullptr, 0, nullptr};
};
#undef EMP_KEEP

// RAII kernel timer: when ctx->timing is on, brackets a launch with a fresh HIP event pair on the context's
// stream (none for a null name: a kernel that is never timed).  emp_kernel_ms() later averages all pairs recorded since
// timing was (re-)enabled.
struct KernelTimer {
    emp_ctx* ctx;
    hipEvent_t start = nullptr, stop = nullptr;
    bool attached = false;   // the launcher hands start / stop to hipExtLaunchKernelGGL itself
    // attach = true: the events are NOT recorded on the stream here; the caller passes them to
    // hipExtLaunchKernelGGL, which stamps the kernel's own begin and end (no extra stream packets, and the
    // interval excludes the wait between the record and the kernel's start)
    KernelTimer(emp_ctx* c, const char* name, bool attach = false) : ctx(c), attached(attach) {
        if (!c->timing || !name) return;
        if (!c->timing_filter.empty() && c->timing_filter != name) return;
        emp_ctx::Ev& e = c->events[name];
        if (e.used == e.pairs.size()) {
            std::pair<Event, Event> pr;
            if (hipEventCreate(&pr.first.h) != hipSuccess || hipEventCreate(&pr.second.h) != hipSuccess) return;
            e.pairs.push_back(std::move(pr));
        }
        auto& pr = e.pairs[e.used++];
        start = pr.first;
        stop = pr.second;
        if (!attached) (void)hipEventRecord(start, c->stream);
    }
    ~KernelTimer() {
        if (stop && !attached) (void)hipEventRecord(stop, ctx->stream);
    }
};

#define EMP_LAUNCH_CHECK(ctx)                                                                      \
    do {                                                                                           \
        hipError_t e_ = hipGetLastError();                                                         \
        if (e_ != hipSuccess)                                                                      \
            return emp::fail((ctx), EMP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

}  // namespace emp
