/*
 * emplanner.h - C-ABI of the MI355X-native EM-Planner path-planning hot path.
 *
 * The reference (6Lackiu/EMplanner_Carla) is pure Python: its "plugin interface" for this
 * path is the module-level function surface of planner/path_planning.py and
 * planner/planning_utils.py.  Each entry point below is the batched, device-resident form of
 * one (or a chain) of those functions; the Python package `emplanner_carla_amd.planner` binds
 * them with ctypes and re-exposes the reference's names and signatures.
 * "ref:" comments cite the reference function an entry point replaces (paths relative to the
 * reference tree).
 *
 * Conventions
 *   - plain C, POD only; all floating point is IEEE-754 binary64, all indices int32.
 *   - every array is batch-major and padded: [B][max_x]... with a per-scene length array.
 *   - per-scene counts beyond their row's capacity are clamped to [0, max_x], never followed.
 *   - `where` tells whether the DATA pointers of the call are host (EMP_HOST: the library
 *     stages them through its own device buffers) or device (EMP_DEVICE: used in place; e.g.
 *     torch tensors' data_ptr()).  Parameter structs are always host memory.
 *   - functions return EMP_OK or a negative emp_error; emp_last_error() gives the text.
 *     Per-scene problems never fail a call: they are reported in `status[b]` (bit mask).
 *   - a context owns one device, its HIP stream (more streams once emp_set_pipeline is used) and its
 *     scratch buffers; calls on one context are serialised by the caller.  HIP is initialised lazily in emp_create(), so a
 *     forked planning process (ref: test_9.py:225-227 runs the planner in a child process)
 *     must create its context after the fork.
 */
#ifndef EMPLANNER_H
#define EMPLANNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 13 (migration from 12): adds emp_speed_io and emp_plan_trajectory - the path cycle and the S-T speed planner in one call.
 * Nothing of ABI 12 changed: a caller that does not use the new entry point only updates its version check. */
#define EMP_ABI_VERSION 13

typedef struct emp_ctx emp_ctx;

typedef enum emp_error {
    EMP_OK = 0,
    EMP_ERR_INVALID = -1,   /* bad argument (null pointer, size out of supported range) */
    EMP_ERR_HIP = -2,       /* a HIP runtime call failed; see emp_last_error */
    EMP_ERR_NO_DEVICE = -3, /* no gfx950 device visible */
    EMP_ERR_NOMEM = -4
} emp_error;

/* Where the arrays of a call live.  EMP_HOST: ordinary host memory - the call copies in, computes, copies out and returns when
 * the outputs are there (arrays of up to 64 KB, 256 KB a direction and call, are packed into one page-locked block and cross PCIe
 * as ONE copy per direction: a call of the reference's function surface - three to twenty small arrays - costs 50 us instead of
 * 65-100).  EMP_DEVICE: device memory, used in place; the call returns at once (stream-ordered).
 * EMP_HOST_PINNED (ABI 10): page-locked host memory from emp_host_alloc.  Every entry point accepts it like EMP_HOST;
 * emp_plan_cycle additionally overlaps it (see there): inputs cross PCIe on a copy stream while the previous call computes,
 * outputs come back on a stream of their own, and with a pipeline set the call does not wait for them - emp_wait_cycle does.
 * Layout contract of an EMP_HOST_PINNED cycle: the arrays may be any page-locked memory.  Arrays of one direction that lie inside
 * ONE emp_host_alloc allocation of this context with at most 512 bytes between neighbours (alignment padding) cross PCIe as one
 * copy; for outputs that copy also writes the padding bytes between them (contents unspecified) - nothing else is ever written.
 * Any other layout (arrays allocated one by one, a smaller batch at the head of a larger slot, other data carved between two
 * outputs) is copied array by array.  Within one pipeline do not alternate EMP_DEVICE and EMP_HOST_PINNED cycles faster than the
 * pipeline depth unless the device-pointer call's inputs may be read late (the library orders the copies, not the caller's writes). */
typedef enum emp_mem { EMP_HOST = 0, EMP_DEVICE = 1, EMP_HOST_PINNED = 2 } emp_mem;

/* per-scene status bits */
enum {
    EMP_ST_DP_INFEASIBLE = 1,  /* min terminal cost > w_collision: ref prints its banner, path_planning.py:351 */
    EMP_ST_S_OUT_OF_RANGE = 2, /* cal_proj_point walked past the s_map: ref raises IndexError, path_planning.py:63 */
    EMP_ST_BOUND_INDEX = 4,    /* cal_lmin_lmax index >= n: ref raises IndexError, path_planning.py:267/272 */
    EMP_ST_QP_FAILED = 8,      /* path QP infeasible / not converged (ref ignores cvxopt's status, :211-218) */
    EMP_ST_SMOOTH_FAILED = 16, /* smoothing QP not converged */
    EMP_ST_TRUNCATED = 32      /* an output did not fit the caller's max_* capacity */
};

/* ref: keyword arguments of DP_algorithm, path_planning.py:276-279 (defaults in emp_dp_params_default) */
typedef struct emp_dp_params {
    int32_t row;            /* lateral samples  (ref default 12) */
    int32_t col;            /* longitudinal stations (ref default 6) */
    double sample_s;        /* 15  */
    double sample_l;        /* 1.5 */
    double sampling_res;    /* 2: densification step of enrich_DP_s_l */
    double w_collision;     /* 1e12 */
    double w_smooth[3];     /* 300, 1000, 5000 */
    double w_ref;           /* 20 */
} emp_dp_params;

/* ref: keyword arguments of Quadratic_planning, path_planning.py:78-81, and of cal_lmin_lmax :222 */
typedef struct emp_qp_params {
    double ds;              /* dp_sampling_res = 2 (the QP's fixed station spacing, :108) */
    double w_l, w_dl, w_ddl, w_dddl, w_centre;          /* 1000, 10000 (unused by the ref, :193), 3000, 150, 250 */
    double w_end_l, w_end_dl, w_end_ddl;                /* 40, 40, 40 */
    double host_d1, host_d2, host_w;                    /* 3, 3, 3 */
    double obs_length, obs_width;                       /* 5, 5 (ref: test_9.py:192) */
    int32_t decimate;       /* 2 (test_9.py:187) or 1 (test_7.py) */
    int32_t midpoint;       /* 1: re-interleave midpoints (test_9.py:204-210); 0: none (test_7.py) */
    int32_t use_qp;         /* 1; 0 skips the QP (test_5.py / test_6.py form) */
    int32_t reserved;       /* MUST be 0 (emp_qp_params_default sets it): every entry point that takes the struct refuses
                             * anything else with EMP_ERR_INVALID, so that a caller who did not initialise the struct finds
                             * out at once */
} emp_qp_params;

/* ref: keyword arguments of smooth_reference_line, planning_utils.py:262-264 */
typedef struct emp_smooth_params {
    double w_smooth, w_length, w_ref;                   /* 0.4, 0.3, 0.3 */
    double x_thre, y_thre;                              /* 0.2, 0.2 */
} emp_smooth_params;

/* ref: keyword arguments of speed_DP, speed_planning_test.py:101-102 */
typedef struct emp_speed_dp_params {
    double reference_speed;                             /* 50 */
    double w_cost_ref_speed, w_cost_accel, w_cost_obs;  /* 4000, 100, 1e7 */
} emp_speed_dp_params;

void emp_dp_params_default(emp_dp_params* p);
void emp_speed_dp_params_default(emp_speed_dp_params* p);
void emp_qp_params_default(emp_qp_params* p);
void emp_smooth_params_default(emp_smooth_params* p);

/* ---- context ------------------------------------------------------------------------- */
int emp_abi_version(void);
int emp_create(int device_id, emp_ctx** out);
void emp_destroy(emp_ctx* ctx);
const char* emp_last_error(const emp_ctx* ctx); /* ctx may be NULL: error of the last failed emp_create */
int emp_synchronize(emp_ctx* ctx);
/* the context's HIP stream (hipStream_t) so callers can order their own work after ours */
void* emp_stream(emp_ctx* ctx);
/* device memory helpers for callers without a HIP binding (ctypes hosts) */
/* Page-locked host memory for EMP_HOST_PINNED calls (hipHostMalloc); freed by emp_host_free or emp_destroy. */
int emp_host_alloc(emp_ctx* ctx, uint64_t bytes, void** out);
int emp_host_free(emp_ctx* ctx, void* ptr);
/* EMP_HOST_PINNED cycles: block until the outputs of the emp_plan_cycle call issued `calls_back` calls ago (0 = the latest)
 * are in the caller's host arrays.  calls_back < emp_pipeline_depth(); EMP_ERR_INVALID beyond (that call's arrays were already
 * waited for when its pool was taken over).  A call that was not an EMP_HOST_PINNED cycle has nothing to wait for: EMP_OK. */
int emp_wait_cycle(emp_ctx* ctx, int32_t calls_back);
/* The number of pipelined emp_plan_cycle calls issued on this context so far: the ticket of the latest one.  A caller that keeps
 * the ticket of a call finds it again as calls_back = emp_cycle_ticket() - ticket. */
uint64_t emp_cycle_ticket(emp_ctx* ctx);
/* Block until the host outputs of the EMP_HOST_PINNED cycle that got `ticket` are in place; a ticket older than the pipeline
 * depth has been waited for by the call that took its pool over: EMP_OK at once.  The ONE entry point that may be called from
 * another thread while a call on this context is in progress (a server thread waits for its batch while another submits): a pool
 * keeps answering for its ticket until the call that takes it over has itself waited for that ticket's outputs.  Not beside
 * emp_set_pipeline or emp_destroy. */
int emp_wait_ticket(emp_ctx* ctx, uint64_t ticket);
int emp_device_alloc(emp_ctx* ctx, uint64_t bytes, void** out);
int emp_device_free(emp_ctx* ctx, void* ptr);
int emp_copy_to_device(emp_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int emp_copy_to_host(emp_ctx* ctx, void* dst, const void* src, uint64_t bytes);
/* Per-kernel timing with HIP events on the context's stream.  emp_set_timing(ctx, 1) (re)starts the
 * statistics; every launch of a named kernel ("project", "dp_edge", "dp_sweep", "dp_enrich", "path_qp",
 * "to_cartesian", "heading", ...) is then bracketed by an event pair.  emp_kernel_ms returns the MEAN
 * duration in milliseconds over the launches recorded since (it synchronises on their events), or a
 * negative value if there were none; emp_kernel_launches returns how many were recorded. */
int emp_set_timing(emp_ctx* ctx, int enabled);
/* Restrict the event pairs to ONE named kernel (NULL or "" = every kernel again).  An event pair costs a few
 * microseconds of stream time per launch, so a benchmark that needs the live duration of one kernel should not
 * pay for bracketing the others. */
int emp_set_timing_filter(emp_ctx* ctx, const char* kernel);

/* Several batches in flight: CONSECUTIVE emp_plan_cycle calls with device pointers overlap on the GPU (off by default).
 * The kernels of a cycle are bound by different things - FP64 issue (edge costs), HBM (sweep), the latency of the slowest
 * scene's chain of dependent instructions (projection, path QP, Cartesian tail, the chip mostly idle) - so one batch at a
 * time leaves issue slots empty.  mode:
 *   0                      off: one cycle at a time on emp_stream().
 *   EMP_PIPELINE_STAGED    two batches: the back stage (densified DP path, path QP, Cartesian tail) of call k runs on a
 *                          second stream while the front stage (projection, edge costs, sweep) of call k+1 runs on
 *                          emp_stream().  The front stages stay serial, so the sweep runs next to nothing but the end
 *                          of a back stage and keeps its share of the HBM roofline (0.26 ms per 4096-scene step, sweep
 *                          21 us).  A call may wait ON THE HOST for the call four back (emp_pipeline_depth).
 *   n = 2..EMP_PIPELINE_MAX  n batches on n lanes (a stream and a pool of temporaries each; ABI version 7): call k runs
 *                          whole on lane k mod n, behind everything queued on emp_stream() when it is issued, and the
 *                          dispatcher overlaps the kernels of n consecutive cycles.  Highest throughput (n = 3: 0.258 ms
 *                          per step) at the price of every kernel's own duration (the sweep: 40 us).  Wants as many
 *                          hardware queues as streams (n lanes + emp_stream()): the HIP runtime maps a process's streams
 *                          onto GPU_MAX_HW_QUEUES queues (default 4) and reads the variable when it initialises, so the
 *                          HOST PROGRAM exports e.g. GPU_MAX_HW_QUEUES=8 before it first touches HIP - the library does
 *                          not change the environment.  With fewer queues lanes share one and serialise (3 lanes on 4
 *                          queues beside torch's stream: slower than 2); beyond 7 lanes they share in any case.
 *   EMP_PIPELINE_AUTO      (ABI version 11) the library picks what this PROCESS can sustain: three lanes when every stream has a
 *                          hardware queue of its own - GPU_MAX_HW_QUEUES (the value the HIP runtime was started with; default
 *                          4; the one environment variable the library reads) >= 3 lanes + emp_stream() + this context's copy /
 *                          d2h streams (EMP_HOST_PINNED cycles) + EMP_OPT_FOREIGN_STREAMS (the streams the rest of the process
 *                          uses: default 1, the caller's own; add a gather stream, RCCL's) - else EMP_PIPELINE_STAGED (two
 *                          queues).  emp_pipeline_form reports the choice.  Measured on 4 queues (HIP's default): three lanes
 *                          0.272-0.274 ms per 4096-scene step against the staged form's 0.202-0.207; on 12: 0.187-0.191 against the same
 *                          (profiles/r06_bench_queues*.json; tests/test_gpu_fullsize.py).
 * Consequences for the caller: the outputs of a call are complete on emp_result_stream() - in lane mode the lane of the
 * LATEST emp_plan_cycle call, so ask after every call - and emp_synchronize waits for every stream; each call in flight
 * needs its OWN output buffers, and its inputs must stay unchanged until it is done.  Every other entry point first
 * lets emp_stream() wait for the cycles in flight.  Results are bit-identical to the unpipelined call. */
#define EMP_PIPELINE_AUTO (-1)
#define EMP_PIPELINE_STAGED 1
#define EMP_PIPELINE_MAX 8
int emp_set_pipeline(emp_ctx* ctx, int mode);
/* The pipeline form in force: 0 off, EMP_PIPELINE_STAGED, or the number of lanes; negative: ctx is NULL.  After an
 * emp_set_pipeline(EMP_PIPELINE_AUTO), optionally (pointers may be NULL) the hardware-queue count it saw and the streams it counted
 * beside the lanes (0 / 0 when the latest mode was set explicitly). */
int emp_pipeline_form(emp_ctx* ctx, int32_t* hw_queues, int32_t* other_streams);
void* emp_result_stream(emp_ctx* ctx);
/* How many consecutive emp_plan_cycle calls may have work in flight in the current mode (ABI version 8): the output buffers
 * of call k may be reused once call k + emp_pipeline_depth() has been ISSUED.  1 when the pipeline is off, n in lane mode,
 * 4 in staged mode: two batches overlap there, but the pools of temporaries rotate over four calls and emp_plan_cycle
 * waits ON THE HOST for the call four back (a call that finished long ago unless the host runs further ahead than that,
 * which it then may not) - a stream-side wait for the pool's previous user cost ~11 us of every 0.29 ms step. */
int emp_pipeline_depth(emp_ctx* ctx);
/* The fence of the pipelined modes (on by default): every entry point other than a pipelined emp_plan_cycle first lets
 * emp_stream() wait for the cycles in flight, so that it may read their outputs.  Switched off, such calls are queued on
 * emp_stream() at once and overlap the cycles in flight - for work that does not depend on them (the S-T speed planner of
 * the same scenes: bench.py --config cfg5); what must be ordered, the caller orders with emp_result_stream().  Their
 * temporaries are the main stream's own, so consecutive unfenced calls are still serial among themselves. */
int emp_set_fence(emp_ctx* ctx, int enabled);

/* ---- options (ABI version 9; renumbered in version 11: twelve of them) -------------------------------------------------------
 * The library reads no EMP_* environment variable.  Everything that used to be an environment switch of the development
 * builds is a per-context option here, set by the host program before the calls it should affect (a change takes effect
 * at the next call; EMP_OPT_FOREIGN_STREAMS at the next emp_set_pipeline(EMP_PIPELINE_AUTO)).  Retired in version 11, each with the
 * number that retired it: EMP_OPT_SWEEP_MARKER (always on with EMP_OPT_SWEEP_EXCLUSIVE: 0.264 against 0.32-0.35 ms per step without),
 * EMP_OPT_ENRICH_ON_FRONT (0.4 % slower, never a default), EMP_OPT_BACK_STREAM_CUS (a CU mask on the back stage never gained),
 * EMP_OPT_FUSED_COLUMNS / EMP_OPT_EDGE_COLS_PER_WAVE / EMP_OPT_SWEEP_VARIANT (the auto rules are the measured optima: HISTORY.md 3.2,
 * profiles/r05_edge/README.md), EMP_OPT_ST_ORDER (heaviest scenes first: 3 % on configs[4], never slower).  Unknown options and values out of range are
 * EMP_ERR_INVALID.  "result-affecting" options change WHICH kernel computes a stage: the two forms of a stage solve the
 * same problem with the same stopping rule but associate sums differently (path QP: ~2e-9 relative; Cartesian tail: bit
 * identical) - so they are never chosen from the batch size: a scene's result does not depend on how many scenes share
 * its call or its GPU (a rank's shard equals its slice of the one-GPU result, emplanner_carla_amd/dist.py).
 *
 *   option                          default  kind             meaning
 *   EMP_OPT_PATH_QP_FORM            0        result-affecting 0: eight scenes per wavefront (emp_qp_rows.h; up to 66 stations,
 *                                                             beyond that the one-per-wavefront kernel whatever is set);
 *                                                             1: the two-scenes-per-wavefront kernel of rounds 1-2
 *                                                             (emp_qp_wave.h: ~17 % fewer instructions on a scene's own
 *                                                             critical path - for a caller that plans a handful of scenes
 *                                                             and wants the last 10 us of latency)
 *   EMP_OPT_CARTESIAN_FORM          0        A/B (bit-ident.) 0: four scenes per wavefront; 1: one scene per wavefront
 *   EMP_OPT_SMOOTH_FORCE_FALLBACK   0        test hook        1: every smoothing QP of the Cartesian tail takes its
 *                                                             projected-gradient fallback (tests/test_gpu_fullsize.py)
 *   EMP_OPT_EDGE_BLOCK              0        tuning           threads per block of the edge-cost kernel (multiple of 64 up
 *                                                             to 1024); 0: from the lattice's LDS footprint
 *   EMP_OPT_EDGE_FORM               0        A/B (bit-ident.) edge-cost kernel of the tiled lattices (<= 32 rows): 0 = work-ring
 *                                                             form (edges with obstacles in reach are queued per wavefront and
 *                                                             scanned one edge per lane: 0.93 active lanes of a scan at 40 x 9
 *                                                             with 8 obstacles), 1 = the lockstep form of rounds 1-4 (0.49);
 *                                                             obstacle rows wider than 64 slots always take the lockstep form
 *   EMP_OPT_LANE_EDGE_ORDER         2        pipeline order   lane mode (emp_set_pipeline(n >= 2)): 1 = the edge-cost kernel of a call starts
 *                                                             when the previous call's - on another lane - is done, so that at most
 *                                                             one of them runs at a time and the sweep that follows one has a single
 *                                                             edge kernel beside it instead of two (one stream-side wait per call);
 *                                                             2 (default since ABI 11) = 1 for calls of 8192 scenes and more, where
 *                                                             one edge kernel fills the chip by itself (32 768 scenes of the 40 x 9
 *                                                             lattice: 1.47 -> 1.36 ms per step, the sweep at 0.53 of the HBM peak
 *                                                             instead of 0.31; 8192: 2 %); 0 = lanes are never ordered among each
 *                                                             other.  NOT for smaller calls: the order bounds the step from below by
 *                                                             the edge kernel's own duration (4096 scenes with every obstacle beside
 *                                                             the same columns: 0.18 -> 0.23 ms per step; 1024 scenes 0.116 -> 0.121)
 *   EMP_OPT_CYCLE_GRAPH             0        tuning           1: emp_plan_cycle on device pointers, one batch at a time (no pipeline): the
 *                                                             THIRD consecutive call with the same sizes, parameters, options and
 *                                                             pointers captures its six launches into a hipGraph, every further one
 *                                                             replays it with one hipGraphLaunch (the callers that plan one scene or a
 *                                                             few per call over and over, BASELINE configs[1]: launch latency is a
 *                                                             fifth of such a cycle).  Same kernels, same arguments: same bits.  Any
 *                                                             change of an argument, of an option or of the context's buffers drops
 *                                                             the graph; emp_set_timing and the clock probes bypass it
 *   EMP_OPT_EDGE_CLOCK_PROBE        0        measurement      1: every launch of the work-ring edge kernel records, per wavefront,
 *                                                             the 100 MHz reference counter at its first and last instruction
 *                                                             and the shader clock there (emp_edge_probe, emp_edge_clock_mhz read
 *                                                             the latest launch)
 *   EMP_OPT_SWEEP_EXCLUSIVE         0        tuning           staged pipeline, what the HBM-bound sweep of call k may run beside:
 *                                                             0 (default since round 5) = no wait: the fastest step.  With the
 *                                                             work-ring edge kernel the sweep of call k starts after call k-1's
 *                                                             path QP by itself and overlaps its Cartesian tail: 0.66-0.67 of
 *                                                             the HBM peak at 4096 scenes, 0.227 ms per step;
 *                                                             2 = it waits (stream-side) for call k-1's densification and
 *                                                             path QP: 0.70-0.72 at +6 % step time (0.241 ms) - the two
 *                                                             barrier packets, not any waiting, are what the 6 % buy;
 *                                                             1 = it waits for the whole back stage of call k-1 (0.259 ms)
 *   EMP_OPT_EDGE_AFTER_ENRICH       1        tuning           staged pipeline: 1 (default) = the edge-cost kernel of call k waits
 *                                                             (stream-side) for the densification kernel of call k-1, so that
 *                                                             the path QP behind it is dispatched BEFORE the edge kernel's
 *                                                             sixteen-wavefront blocks take the compute units.  Whichever of
 *                                                             the two starts first keeps the chip: QP first = edge 195 us, QP
 *                                                             140 us side by side; edge first = edge 147 us with the QP starved
 *                                                             to 255 us behind it, a 0.32-0.34 ms step.  Without the wait the
 *                                                             order is a race that the N > 1 step (record packing on the back
 *                                                             queue) loses: 0.305 -> 0.270 ms there, +1 % on the plain step
 *   EMP_OPT_FOREIGN_STREAMS         1        pipeline order   streams of the process OUTSIDE this context that carry GPU work while it
 *                                                             plans (the caller's own stream, a gather stream, RCCL's): what
 *                                                             emp_set_pipeline(EMP_PIPELINE_AUTO) counts beside its own
 *   EMP_OPT_SWEEP_CLOCK_PROBE       0        measurement      1: every sweep launch also records, per wavefront, the shader
 *                                                             clock ticks and the 100 MHz reference ticks it ran for
 *                                                             (emp_sweep_clock_mhz reads their ratio)                       */
typedef enum emp_option {
    EMP_OPT_PATH_QP_FORM = 0,
    EMP_OPT_CARTESIAN_FORM = 1,
    EMP_OPT_SMOOTH_FORCE_FALLBACK = 2,
    EMP_OPT_EDGE_BLOCK = 3,
    EMP_OPT_EDGE_FORM = 4,
    EMP_OPT_SWEEP_EXCLUSIVE = 5,
    EMP_OPT_EDGE_AFTER_ENRICH = 6,
    EMP_OPT_LANE_EDGE_ORDER = 7,
    EMP_OPT_CYCLE_GRAPH = 8,
    EMP_OPT_SWEEP_CLOCK_PROBE = 9,
    EMP_OPT_EDGE_CLOCK_PROBE = 10,
    EMP_OPT_FOREIGN_STREAMS = 11,
    EMP_OPT_COUNT = 12
} emp_option;
int emp_set_option(emp_ctx* ctx, int32_t option, int32_t value);
int emp_get_option(emp_ctx* ctx, int32_t option, int32_t* value);
/* With EMP_OPT_SWEEP_CLOCK_PROBE on: the shader clock the sweep launches ran at since the option was last switched on (the
 * latest 32 of them), in MHz: the ratio of shader-clock ticks to 100 MHz reference ticks between a wavefront's first and
 * last instruction, summed over all their wavefronts (synchronises on the latest launch); optionally (may be NULL) the mean
 * and the longest time a wavefront was resident, in microseconds.  Negative when nothing was recorded. */
double emp_sweep_clock_mhz(emp_ctx* ctx, double* mean_wave_us, double* max_wave_us);
/* With EMP_OPT_EDGE_CLOCK_PROBE on: the latest edge-cost launch - mean time a wavefront was resident (us), time from the first
 * wavefront's start to the last one's end (us), mean number of wavefronts resident at once (their ratio x count), wavefronts.
 * Synchronises on that launch.  Any out pointer may be NULL. */
int emp_edge_probe(emp_ctx* ctx, double* mean_wave_us, double* span_us, double* mean_resident_waves, int32_t* waves);
/* The same probe: the shader clock the latest edge-cost launch ran at, in MHz (shader-clock ticks over 100 MHz reference ticks,
 * summed over its wavefronts) - the clock the chip holds under the FP64-issue-bound kernel that is most of the step, which is what
 * a vector-issue roofline of the step must be priced at (bench.py roofline_step).  Negative when nothing was recorded. */
double emp_edge_clock_mhz(emp_ctx* ctx);
/* EMP_OPT_CYCLE_GRAPH: how many emp_plan_cycle calls of this context were served by replaying a captured graph (-1: ctx is NULL). */
int64_t emp_cycle_graph_replays(emp_ctx* ctx);
/* The same probe, per launch and averaged over the recorded launches (100 MHz reference ticks, which all wavefronts share):
 * how long after the launch's first wavefront its last wavefront started, and the time from the first wavefront's first
 * instruction to the last wavefront's last - what is left of the launch's event-measured duration is dispatch and
 * completion overhead outside any wavefront. */
int emp_sweep_probe_spans(emp_ctx* ctx, double* start_spread_us, double* first_start_to_last_end_us);

/* One fixed-stride record per scene for the multi-GPU gather (no reference counterpart: the reference plans one scene
 * per process; this is the result exchange of the batched form, emplanner_carla_amd/dist.py):
 *   rec [B][3 + col + 2*path_cap + 4*(path_cap+1)] doubles = status, traj_len, path_len, dp_rows [col],
 *   path_s [path_cap], path_l [path_cap], traj [path_cap+1][4]
 * from the outputs of emp_plan_cycle (arrays with max_pts / max_pts+1 entries per scene, path_cap <= max_pts of them
 * kept).  One launch; on_result_stream != 0 queues it on emp_result_stream(), behind the cycle that produced them. */
int emp_pack_records(emp_ctx* ctx, int32_t B, int32_t col, int32_t max_pts, int32_t path_cap, const int32_t* status,
                     const int32_t* traj_len, const int32_t* path_len, const double* dp_rows, const double* path_s,
                     const double* path_l, const double* traj, double* rec, int on_result_stream, emp_mem where);
/* The same for a consumer that only drives the controller (ref: controller/controller.py:66-71 takes the list of
 * (x, y, theta, kappa) and nothing else): rec [B][2 + 4*(path_cap+1)] doubles = status, traj_len, traj [path_cap+1][4]
 * - 94 instead of 179 doubles per scene on the 40x9 lattice (ABI version 6). */
int emp_pack_trajectory_records(emp_ctx* ctx, int32_t B, int32_t max_pts, int32_t path_cap, const int32_t* status,
                                const int32_t* traj_len, const double* traj, double* rec, int on_result_stream,
                                emp_mem where);
double emp_kernel_ms(emp_ctx* ctx, const char* kernel);
int emp_kernel_launches(emp_ctx* ctx, const char* kernel);
/* The individual durations behind emp_kernel_ms, in launch order: writes min(recorded, cap) values (milliseconds) to `ms`
 * and returns how many were recorded (negative on error). */
int emp_kernel_samples(emp_ctx* ctx, const char* kernel, double* ms, int32_t cap);

/* ---- S-L lattice DP ------------------------------------------------------------------ */
/* Layout of the materialised edge-cost tensor (two-kernel DP mode):
 *   EMP_EDGE_CANONICAL  edge[b][j-1][i][k]  k fastest: cost of row k (column j-1) -> row i (column j)
 *   EMP_EDGE_TILED      the layout the sweep kernel streams: scenes are grouped in tiles of
 *                       S = 64 / row scenes and stored [tile][j-1][k][s][i] so that one wavefront
 *                       reads 64 consecutive doubles per source row k
 * `row` may be anything in [1, 1024] (ref path_planning.py:276-279 takes any; :301-346).  Up to 32 rows the DP runs on the
 * tiled kernels; wider lattices take a generic pair of kernels (one block per scene, pair table in device memory) whose
 * tensor is the CANONICAL one whichever layout is asked for (emp_edge_tensor_elems says so), and EMP_DP_FUSED falls back
 * to the two-kernel form there.  Same arithmetic, bit for bit.  Measured (profiles/r04_wide_lattice.json, 1024 scenes, 40
 * columns): the wide edge kernel costs 0.014-0.021 ns per lattice edge against 0.013 on the 21-row tiled lattice, the wide
 * sweep 0.003-0.007 against 0.0016 (2.0-2.6 TB/s of algorithmic bytes; 0.6 TB/s at exactly 33 rows) - a 48-row lattice is
 * 1.3x the per-edge cost of the 21-row one, so the wide pair stays generic.
 * THE CAP: row > 1024 is refused with EMP_ERR_INVALID (ABI 10; 256 until ABI 9: predecessor indices of the wide sweep are
 * 16-bit now).  The reference itself takes any row count; at 1024 rows the pair table alone is 126 MB and one scene of 6
 * columns 5.2 M edges - what bounds the cap is memory per scene, not the kernels.                                        */
typedef enum emp_edge_layout { EMP_EDGE_CANONICAL = 0, EMP_EDGE_TILED = 1 } emp_edge_layout;
uint64_t emp_edge_tensor_elems(const emp_dp_params* p, int32_t B, emp_edge_layout layout);

/* ref: cal_start_cost (path_planning.py:435-514) for every row and cal_neighbor_cost (:517-585)
 * for every (column, row, row) of every scene.
 *   obs_s, obs_l [B][max_obs], n_obs [B], start [B][4] = plan_start s, l, dl, ddl
 *   start_cost [B][row]   (without the +10000 lane penalty, like the ref's function)
 *   edge       emp_edge_tensor_elems(p, B, layout) doubles                                  */
int emp_dp_edge_costs(emp_ctx* ctx, const emp_dp_params* p, int32_t B, int32_t max_obs,
                      const double* obs_s, const double* obs_l, const int32_t* n_obs, const double* start,
                      double* start_cost, double* edge, emp_edge_layout layout, emp_mem where);

typedef enum emp_dp_mode {
    EMP_DP_FUSED = 0,      /* one kernel, one block per tile of 64 / row scenes: the edge costs of four columns at a time are
                            * staged in LDS and swept in place; no HBM edge tensor (8 E bytes per scene neither written nor
                            * read).  Bit-identical results; slower than the two-kernel form at every measured batch size
                            * (0.264 against 0.181 ms per 4096 scenes 40x9, 1.42 against 1.35 ms per 32768: one block per
                            * tile leaves a CU with 8-12 wavefronts) - the form for callers who cannot afford the tensor. */
    EMP_DP_TWO_KERNEL = 1  /* edge-cost kernel writes the tiled tensor to HBM, sweep kernel streams it (the measured
                            * default of the Python layer and of bench.py) */
} emp_dp_mode;

/* ref: DP_algorithm (path_planning.py:276-375) up to and including the backtrack, batched.
 *   rows   [B][col] float64: chosen lattice row per column (float because the ref's no-obstacle
 *          bypass yields (row+1)/2-1, which is x.5 for even `row`, :363)
 *   min_cost [B] (may be NULL): minimum of the last cost column (+inf in the bypass)
 *   status [B]: EMP_ST_DP_INFEASIBLE or 0                                                    */
int emp_dp_plan(emp_ctx* ctx, const emp_dp_params* p, int32_t B, int32_t max_obs,
                const double* obs_s, const double* obs_l, const int32_t* n_obs, const double* start,
                emp_dp_mode mode, double* rows, double* min_cost, int32_t* status, emp_mem where);

/* min-plus sweep + backtrack on caller-provided costs (ref: path_planning.py:301-361), for tests
 * and for the HBM-roofline measurement.  start_cost [B][row], edge in EMP_EDGE_TILED layout (canonical beyond 32 rows). */
int emp_dp_sweep(emp_ctx* ctx, const emp_dp_params* p, int32_t B, const double* start_cost, const double* edge,
                 double* rows, double* min_cost, int32_t* status, emp_mem where);

/* ref: enrich_DP_s_l (path_planning.py:378-432) after the row->(s,l) mapping of :366-370.
 *   rows [B][col] -> path_s, path_l [B][max_pts], path_len [B]; status gets EMP_ST_TRUNCATED  */
int emp_dp_enrich(emp_ctx* ctx, const emp_dp_params* p, int32_t B, const double* rows, const double* start,
                  int32_t max_pts, double* path_s, double* path_l, int32_t* path_len, int32_t* status,
                  emp_mem where);

/* ref: enrich_DP_s_l (path_planning.py:378-432) exactly as the reference function takes it: arbitrary node
 * lists node_s, node_l [B][max_nodes] with n_nodes [B], start [B][4], resolution -> path_s, path_l, path_len */
int emp_enrich_nodes(emp_ctx* ctx, int32_t B, int32_t max_nodes, double resolution, const double* node_s,
                     const double* node_l, const int32_t* n_nodes, const double* start, int32_t max_pts,
                     double* path_s, double* path_l, int32_t* path_len, int32_t* status, emp_mem where);

/* ---- Cartesian <-> Frenet ------------------------------------------------------------ */
/* ref: cal_s_map_fun (planning_utils.py:448-472), cal_s_l_fun (:475-509) for the obstacles and the
 * planning start, cal_s_l_deri_fun (:512-588) for the planning start - the front half of one
 * motion_planning cycle (test_9.py:113-177).
 *   ref_line [B][max_ref][4] x,y,theta,kappa; n_ref [B]
 *   origin_xy, start_xy, start_v, start_a [B][2]; obs_xy [B][max_obs][2]; n_obs [B]
 *   s_map [B][max_ref]; obs_s, obs_l [B][max_obs]; begin_sl [B][2] = s,l of start_xy;
 *   start [B][4] = s, l, dl/ds, d2l/ds2 (the DP's plan_start_*)                               */
int emp_frenet_project(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_obs,
                       const double* ref_line, const int32_t* n_ref,
                       const double* origin_xy, const double* start_xy, const double* start_v,
                       const double* start_a, const double* obs_xy, const int32_t* n_obs,
                       double* s_map, double* obs_s, double* obs_l, double* begin_sl, double* start,
                       emp_mem where);

/* ref: cal_s_map_fun (planning_utils.py:448-472) alone: s_map [B][max_ref] */
int emp_s_map(emp_ctx* ctx, int32_t B, int32_t max_ref, const double* ref_line, const int32_t* n_ref,
              const double* origin_xy, double* s_map, emp_mem where);

/* ref: cal_s_l_fun (planning_utils.py:475-509) with a caller-supplied s_map: xy [B][max_pts][2] -> s, l [B][max_pts].
 * With match_index != NULL and l == NULL it is cal_projection_s_fun (:429-445): s from the given match indices.  A match
 * index outside [0, n_ref) is not followed: that point's s (and l) are NaN.  n_ref = 0 gives NaN for every point. */
int emp_s_l(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line, const double* s_map,
            const int32_t* n_ref, const double* xy, const int32_t* n_pts, const int32_t* match_index,
            double* s, double* l, emp_mem where);

/* ref: cal_s_l_deri_fun (planning_utils.py:512-588): xy, v_xy, a_xy [B][max_pts][2], origin_xy [B][2]
 * -> out [B][max_pts][7] = l, dl/dt, ds/dt, d2l/dt2, dl/ds, d2s/dt2, d2l/ds2 (NaN rows where n_ref = 0) */
int emp_s_l_deri(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                 const int32_t* n_ref, const double* xy, const double* v_xy, const double* a_xy,
                 const int32_t* n_pts, const double* origin_xy, double* out, emp_mem where);

/* The station lookups: which node (or station) belongs to an s.  The comparisons are the reference's, and where they are decided
 * by equality the answers are these (tests/lookup_cases.py holds every one of them with ties that are equal in bits):
 *   emp_proj_point, emp_frenet_path_to_xy, emp_plan_cycle (cal_proj_point: `while s_map[i + 1] < s: i += 1` from the previous
 *     index, never backwards):
 *       s on the knot s_map[i + 1]   the walk stays at node i (ds is the whole chord); one ulp above, it is node i + 1.  On a plateau
 *                                    of equal entries (repeated nodes) s on or below the value stays in front of the plateau, one
 *                                    ulp above passes all of it.
 *       s on the end s_map[n - 1]    node n - 2, in range; a path station there is KEPT (the path stops at the first s > s_map[n - 1]),
 *                                    one ulp above it is EMP_ST_S_OUT_OF_RANGE for emp_proj_point and for a planning start, and the
 *                                    end of the path for a path station.  s below s_map[0]: node 0, ds negative.
 *       s = NaN                      no comparison holds: the walk stays at the previous index, the point is NaN, status 0; in a path
 *                                    the station is not past the end, its point is NaN and later points are unaffected.
 *                                    s = -inf: as NaN, with an infinite point.  s = +inf: past the end.
 *       a NaN entry of the s_map     stops the walk in front of it (emp_proj_point, emp_frenet_path_to_xy).
 *       pre_match_index              n_ref - 1 or more: EMP_ST_S_OUT_OF_RANGE (s_map[i + 1] does not exist); negative: refused the
 *                                    same way (the reference's index wraps round).  n_ref < 2: always EMP_ST_S_OUT_OF_RANGE.
 *     emp_plan_cycle finds the indices by bisection with a running maximum; that equals the walk for a non-decreasing s_map and
 *     finite stations, which is what it is given: a NaN node makes every later s_map entry NaN (a suffix, on which the bisection still
 *     equals the walk), and a NaN planning start, origin or node in front of the start retires the scene with a status bit and
 *     traj_len 0 before the stations are looked up ("The station lookups").
 *   emp_frenet2cartesian (CalcProjPoint: from index 1, the first index2s[i] >= s): s on index2s[i] is node i with ds = 0; s at or
 *     below index2s[1] - below index2s[0] too - is node 1 with ds <= 0; one ulp above index2s[n - 1], and every s where n_ref < 2, is
 *     EMP_ST_S_OUT_OF_RANGE with that point and the rest of the scene NaN; a NaN s ends the scene the same way without a status.
 *   emp_lmin_lmax, emp_plan_cycle (cal_lmin_lmax: numpy.argmin of |s_j - t|): of equally near stations the FIRST wins, so an
 *     obstacle edge midway between stations j and j + 1 takes j, also where the last station is repeated; a NaN obs_s takes station 0
 *     three times; dp_l[centre] == obs_l is "not below" (the l_min side), and so is a NaN obs_l, which bounds nothing.  An index range
 *     lo..hi that is not empty and reaches n is EMP_ST_BOUND_INDEX; an empty one (lo > hi) is not, wherever it lies. */
/* ref: cal_proj_point (path_planning.py:52-75; twin cal_proj_point_1, planning_utils.py:647-668): n independent
 * queries, each against its own line: s [n], pre_match_index [n] -> out [n][4] x,y,theta,kappa, index [n],
 * status [n] (EMP_ST_S_OUT_OF_RANGE where the reference raises IndexError) */
int emp_proj_point(emp_ctx* ctx, int32_t n, int32_t max_ref, const double* ref_line, const double* s_map,
                   const int32_t* n_ref, const double* s, const int32_t* pre_match_index, double* out,
                   int32_t* index, int32_t* status, emp_mem where);

/* ref: match_projection_points (planning_utils.py:364-426): [B][max_pts] points against one line per scene.
 * The match rule, here and in every entry point that projects on a line (emp_frenet_project, emp_s_map, emp_s_l, emp_s_l_deri,
 * emp_reference_line, emp_plan_cycle): the reference's ordered scan - only a strict `<` improves (the first of equal distances
 * wins), and the scan stops after 50 consecutive non-improvements (5 in the windowed search), so a nearer node behind that is
 * never seen.  A distance that is not finite (a NaN or infinite node or query coordinate) is never `<` another: such a node is
 * passed over and counts as a non-improvement from node 0 on, so a line whose first 50 distances are not finite - or a query that
 * is not finite - matches node 0 (in the windowed search too, wherever it started), and the projection on a NaN node is NaN. */
int emp_match_projection(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts,
                         const double* ref_line, const int32_t* n_ref, const double* xy, const int32_t* n_pts,
                         int32_t* match_index, double* proj, emp_mem where);

/* ref: find_match_points (planning_utils.py:49-182) */
int emp_find_match_points(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts,
                          const double* ref_line, const int32_t* n_ref, const double* xy, const int32_t* n_pts,
                          const int32_t* is_first_run, const int32_t* pre_match_index,
                          int32_t* match_index, double* proj, emp_mem where);

/* ref: cal_heading_kappa (planning_utils.py:185-228): xy [B][max_pts][2] -> theta, kappa [B][max_pts] */
int emp_heading_kappa(emp_ctx* ctx, int32_t B, int32_t max_pts, const double* xy, const int32_t* n_pts,
                      double* theta, double* kappa, emp_mem where);

/* ---- QP stages ----------------------------------------------------------------------- */
/* ref: cal_lmin_lmax (path_planning.py:222-273): station bounds from the (decimated) DP path */
int emp_lmin_lmax(emp_ctx* ctx, int32_t B, int32_t max_pts, int32_t max_obs,
                  const double* dp_s, const double* dp_l, const int32_t* n_pts,
                  const double* obs_s, const double* obs_l, const int32_t* n_obs,
                  double obs_length, double obs_width, double* l_min, double* l_max, int32_t* status,
                  emp_mem where);

/* ref: Quadratic_planning (path_planning.py:78-219).  l_min, l_max [B][max_pts], n_pts [B],
 * start_l3 [B][3] = plan_start l, dl, ddl -> qp_l, qp_dl, qp_ddl [B][max_pts]; status EMP_ST_QP_FAILED.
 * n_pts[b] is clamped to [0, max_pts] like every per-scene count; a scene with fewer than 4 stations after the clamp (the pinned
 * start and end overlap: the reference has no answer) reports EMP_ST_QP_FAILED and nothing is computed for it. */
int emp_path_qp(emp_ctx* ctx, const emp_qp_params* q, int32_t B, int32_t max_pts,
                const double* l_min, const double* l_max, const int32_t* n_pts, const double* start_l3,
                double* qp_l, double* qp_dl, double* qp_ddl, int32_t* iters, int32_t* status, emp_mem where);

/* ref: smooth_reference_line (planning_utils.py:262-361): box-QP smoothing + heading/kappa.
 * xy [B][max_pts][2] -> out [B][max_pts][4] = x, y, theta, kappa; status EMP_ST_SMOOTH_FAILED.
 * n_pts[b] is clamped to [0, max_pts] like every per-scene count; a polyline of fewer than 2 points after the clamp (the
 * reference raises on it) reports EMP_ST_SMOOTH_FAILED and nothing is computed for it. */
int emp_smooth_line(emp_ctx* ctx, const emp_smooth_params* sp, int32_t B, int32_t max_pts,
                    const double* xy, const int32_t* n_pts, double* out, int32_t* iters, int32_t* status,
                    emp_mem where);

/* ref: cal_proj_point (path_planning.py:52-75) chained over a path as frenet_2_x_y_theta_kappa does
 * (:29-46), WITHOUT the smoothing: target_xy [B][max_pts+1][2] (first = the planning start), n_out [B] */
int emp_frenet_path_to_xy(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts,
                          const double* ref_line, const double* s_map, const int32_t* n_ref,
                          const double* begin_sl, const double* path_s, const double* path_l,
                          const int32_t* n_pts, double* target_xy, int32_t* n_out, int32_t* status,
                          emp_mem where);

/* ---- one whole planning cycle -------------------------------------------------------- */
/* ref: the body of motion_planning, test_9.py:113-218 (reference line already smoothed):
 * projection -> DP -> decimate -> bounds -> path QP -> midpoints -> Frenet->Cartesian -> smoothing
 * -> heading/kappa.  Inputs as emp_frenet_project.  Outputs (any may be NULL except traj/traj_len/status):
 *   dp_rows [B][col]; dp_s, dp_l [B][max_pts], dp_len [B]      (DP_algorithm's return)
 *   path_s, path_l [B][max_pts], path_len [B]                   (what test_9.py:220 sends back)
 *   traj [B][max_pts+1][4] x,y,theta,kappa, traj_len [B]        (the controller's input)
 *   status [B] bit mask
 * The counts are per scene: slots at or beyond n_ref[b], n_obs[b] and n_global[b] are never read, whatever they hold (NaN
 * included), and a scene's outputs are the same bits in any batch, beside any neighbours and alone.  A count outside
 * [0, capacity] is clamped (Conventions): n_obs[b] < 0 takes the no-obstacle bypass like 0.  A line of fewer than two nodes, or
 * one that ends before the planning start, is refused with EMP_ST_S_OUT_OF_RANGE (the reference raises IndexError) - also
 * when the path QP has refused the scene already; the DP of an empty line runs on a start state of zeros.
 * A refused scene ((status & ~EMP_ST_DP_INFEASIBLE) != 0) has traj_len 0 and an all-zero traj row; dp_rows, dp_s, dp_l and dp_len
 * are the DP's as for any scene; path_len is 0 (path_s, path_l all zero) when the bounds, the path QP or a capacity refused it
 * (EMP_ST_BOUND_INDEX, EMP_ST_QP_FAILED, EMP_ST_TRUNCATED) and the path QP's result otherwise.  path_s, path_l and traj read
 * as 0 beyond their lengths.  A trajectory of two points is the planning start twice (the line ends before the path's
 * second station): its x, y are specified, its heading and curvature are not (the reference takes them from the rounding
 * error between the two points).                                                                */
typedef struct emp_cycle_io {
    /* inputs */
    const double* ref_line; const int32_t* n_ref;
    const double* origin_xy; const double* start_xy; const double* start_v; const double* start_a;
    const double* obs_xy; const int32_t* n_obs;
    /* outputs */
    double* dp_rows; double* dp_s; double* dp_l; int32_t* dp_len;
    double* path_s; double* path_l; int32_t* path_len;
    double* traj; int32_t* traj_len;
    int32_t* status;
    /* optional input (ABI 2): [B][2] = distance and speed of the FIRST dynamic obstacle of each scene, NaN distance =
     * none.  ref test_9.py:137-169: it becomes three virtual static obstacles on the centre line (meet_s - 10, the
     * middle of the encounter, leave_s) unless the encounter ends beyond s = 80 m.  NULL: no dynamic obstacles. */
    const double* dyn_dis_speed;
    /* optional front end (ABI 11): the cycle starts from the GLOBAL path, as the reference's planning loop does (test_9.py:99-110:
     * find_match_points for the predicted location = start_xy, sampling, smooth_reference_line) - emp_reference_line and this
     * call as ONE call, the 51-point reference line never leaving the device.  global_path [B][max_global][4], n_global [B],
     * pre_match_index [B] in; match_index [B] (the next request's pre_match_index) and ref_status [B] (emp_reference_line's status:
     * OR it into `status`) out.  Then ref_line / n_ref are ignored and max_ref must be EMP_REF_LINE_POINTS.  A scene whose
     * reference line fails runs the cycle on an empty line, exactly as with n_ref = 2 handed to the two-call form.
     * global_path NULL: no front end (the other five fields are ignored). */
    const double* global_path; const int32_t* n_global; const int32_t* pre_match_index;
    int32_t* match_index; int32_t* ref_status;
    int32_t max_global; int32_t reserved_io;      /* reserved_io: 0 */
} emp_cycle_io;

int emp_plan_cycle(emp_ctx* ctx, const emp_dp_params* p, const emp_qp_params* q, const emp_smooth_params* sp,
                   int32_t B, int32_t max_ref, int32_t max_obs, int32_t max_pts, emp_dp_mode mode,
                   const emp_cycle_io* io, emp_mem where);

/* ---- scalar utilities of the reference that sit beside the path ----------------------- */
/* ref: cal_quintic_coefficient (planning_utils.py:671-703): bc [n][8] -> coeff [n][6] (absolute-s basis) */
int emp_quintic_coefficients(emp_ctx* ctx, int32_t n, const double* bc, double* coeff, emp_mem where);
/* ref: cal_obs_cost (path_planning.py:588-609): square_d [n][10] -> cost [n] */
int emp_obs_cost(emp_ctx* ctx, int32_t n, double w_collision, double danger_dis, double safe_dis,
                 const double* square_d, double* cost, emp_mem where);
/* ... for any number of samples per row (ABI 10; the reference loops over whatever it is handed, :601): square_d [n][samples] */
int emp_obs_cost_n(emp_ctx* ctx, int32_t n, int32_t samples, double w_collision, double danger_dis, double safe_dis,
                   const double* square_d, double* cost, emp_mem where);
/* ref: cal_start_cost (path_planning.py:435-514) and cal_neighbor_cost (:517-585) for n FREE edges (ABI 10): edges [n][8] =
 * start s, l, dl, ddl, span, end l, sample_s, 0.  The quintic runs from the start state to (end l, 0, 0) at start s + span (:475 /
 * :553) while the ten samples step by sample_s / 10 from the start (:492-493 / :565-566): on the lattice span = sample_s, a
 * caller of the drop-in functions may pass anything.  Obstacles per edge: obs_s, obs_l [n][max_obs], n_obs [n];
 * w_smooth3 [3] in HOST memory.  cost [n]. */
int emp_free_edge_costs(emp_ctx* ctx, int32_t n, int32_t max_obs, const double* edges, const double* obs_s, const double* obs_l,
                        const int32_t* n_obs, double w_collision, const double* w_smooth3, double w_ref, double* cost, emp_mem where);

/* ref: trajectory_index2s (planning_utils.py:758-780): x, y [B][max_pts] -> cumulative chord length [B][max_pts] */
int emp_trajectory_index2s(emp_ctx* ctx, int32_t B, int32_t max_pts, const double* x, const double* y,
                           const int32_t* n_pts, double* index2s, emp_mem where);
/* ref: Frenet2Cartesian (planning_utils.py:706-733; proj_only = 0) and CalcProjPoint (:736-755; proj_only = 1):
 * sl [B][max_pts][4] = s, l, dl, ddl -> out [B][max_pts][4] = x, y, heading, kappa (NaN from the first NaN s on) */
int emp_frenet2cartesian(emp_ctx* ctx, int32_t B, int32_t max_ref, int32_t max_pts, const double* ref_line,
                         const double* index2s, const int32_t* n_ref, const double* sl, const int32_t* n_pts,
                         double* out, int32_t* status, int32_t proj_only, emp_mem where);
/* ref: cal_dy_obs_deri (planning_utils.py:783-808): in [n][5] = l, vx, vy, heading, kappa -> out [n][3] */
int emp_dy_obs_deri(emp_ctx* ctx, int32_t n, const double* in, double* out, emp_mem where);

/* ---- front end of the cycle ----------------------------------
 * ref: motion_planning, test_9.py:99-110: find_match_points (planning_utils.py:49-182) for the predicted
 * location on the GLOBAL path [B][max_global][4] (x, y, heading, kappa; windowed search from pre_match_index
 * unless is_first_run) -> sampling (:231-259; 10 nodes back / 40 forward, shifted at the ends of the path) ->
 * smooth_reference_line (:262-361).  ref_line [B][EMP_REF_LINE_POINTS][4] is what emp_plan_cycle takes;
 * match_index [B] is the next cycle's pre_match_index.  status: EMP_ST_S_OUT_OF_RANGE where the reference raises
 * IndexError or slices past the path (fewer than 51 nodes), EMP_ST_SMOOTH_FAILED for the QP.
 * is_first_run and iters may be NULL. */
#define EMP_REF_LINE_POINTS 51
int emp_reference_line(emp_ctx* ctx, const emp_smooth_params* sp, int32_t B, int32_t max_global,
                       const double* global_path, const int32_t* n_global, const double* pred_xy,
                       const int32_t* is_first_run, const int32_t* pre_match_index, double* ref_line, int32_t* n_ref,
                       int32_t* match_index, int32_t* iters, int32_t* status, emp_mem where);

/* ---- lateral MPC controller ------------------------------------
 * ref: controller/controller.py class Lateral_MPC_controller (:65-337), `_control` from explicit inputs: the reference
 * reads the vehicle state from a live carla.Vehicle (cal_vehicle_info, :90-113); here the caller supplies
 * state [B][5] = x, y, yaw fi (rad), lateral velocity Vy, yaw rate fi_dot (rad/s) and vx [B] (the caller applies the
 * reference's |Vx| >= 0.005 clamp, :107-110).  target_path [B][max_path][4] = x, y, theta, kappa is the planner's
 * trajectory; min_index [B] the previous match (the search window is 50 points from it, :204).  n_path [B] is clamped to
 * [0, max_path] (the convention above): a count beyond the row never reads the next vehicle's path.  The same holds for
 * emp_lqr_lateral, emp_mpc_ff_lateral and emp_vehicle_control.
 * Chain: cal_A_B_C_fun (:115-148) -> cal_error_k_fun(ts = 0.1) (:170-251) -> cal_coefficient_of_discretion_fun (:151-168)
 * -> cal_control_para_fun (:253-311): condensed MPC with N = 6 steps x P = 2 controls, box |u| <= 1.
 * steer [B] = first control (res['x'][0]); optional outputs (NULL to skip): u [B][12], e_rr [B][4], k_r [B],
 * pre_pro [B][4] = predicted x, y and projected x, y, H [B][12][12] and f [B][12] of the QP, iters [B].
 * status: EMP_ST_S_OUT_OF_RANGE for a bad min_index / empty path (IndexError in the reference), EMP_ST_QP_FAILED.
 * Non-finite and singular input: a vehicle with NaN or +-inf in a state entry, in vx or in theta or kappa of its matched path
 * point, or exactly at its path's centre of curvature (1 - k_r e_d == 0, which divides e_fi_dot by zero), gets
 * EMP_ST_QP_FAILED (EMP_ST_S_OUT_OF_RANGE where the index rule above fires first), steer 0 and u all zero after at most one
 * iteration; H and f are written as computed (NaN where the input reaches them).  The other vehicles of the call are unaffected, bit for bit.  A path
 * point whose x or y is not finite is at no distance `<` another's: the match passes over it, as the reference's does, and
 * the vehicle is answered from the nearest finite point.  No vehicle takes more than 60 iterations. */
typedef struct emp_mpc_params {
    double a, b, Cf, Cr, m, Iz;            /* (a, b, Cf, Cr, m, Iz) = vehicle_para (controller.py:132); the drivers pass
                                            * (1.015, 1.895, 1412, -148970, -82204, 1537) (test_9.py:316) in THIS order */
    double q_diag[4], f_diag[4], r;        /* controller.py:321-328: (250, 1, 50, 1), (1, 1, 1, 1), 1 */
} emp_mpc_params;
void emp_mpc_params_default(emp_mpc_params* p);
int emp_mpc_lateral(emp_ctx* ctx, const emp_mpc_params* p, int32_t B, int32_t max_path, const double* target_path,
                    const int32_t* n_path, const double* state, const double* vx, const int32_t* min_index,
                    double* steer, double* u, double* e_rr, double* k_r, int32_t* min_index_out, double* pre_pro,
                    double* H, double* f, int32_t* iters, int32_t* status, emp_mem where);

/* ref: controller/controller.py class Lateral_LQR_controller (:374-611), `_control` from explicit inputs (same inputs as
 * emp_mpc_lateral; min_index is only the fallback when no path point lies within 100 m: the search covers the whole
 * path, :518).  Chain: cal_A_B_fun (:424-455) -> LQR_fun (:457-486: bilinear discretisation, Riccati iteration until
 * max|dP| < 0.1 or 5000 sweeps) -> cal_error_k_fun(ts = 0.1) (:488-567) -> forward_control_fun (:569-583) ->
 * steer = -K e_rr + delta_f (:606; the raw command, not clipped).  p->q_diag / p->r are Q and R (:592-598: (200, 1, 50,
 * 1), 1; emp_lqr_params_default sets them), p->f_diag is unused.  Optional outputs (NULL to skip): K [B][4],
 * e_rr [B][4], k_r [B], pre_pro [B][4], sweeps [B] (Riccati sweeps performed).
 * Non-finite and singular input.  This law has no QP to fail.  With a finite model - vx finite, or +-inf, which only zeroes the
 * model's quotients - a vehicle with NaN or +-inf in a state entry, in vx or in theta or kappa of its matched path point, or
 * with 1 - k_r e_d == 0, gets status 0 and the IEEE result of the reference's expression: steer NaN (+-inf at the singular
 * point), with the K and the sweeps of its model; emp_vehicle_control then actuates NaN as full lock -1 (see there).  A pose
 * that is not finite matches nothing and keeps min_index; a path point whose x or y is not finite is passed over as in
 * emp_mpc_lateral.  Where the model itself is not finite - vx NaN, or vx + 0.0001 == 0 - the discretisation has no inverse:
 * EMP_ST_QP_FAILED, steer 0, K all NaN, and sweeps = 1, because the loop's NaN-dropping fmax sees max|dP| = 0 (the reference
 * raises ZeroDivisionError for the zero velocity and spins all 5000 sweeps on NaN).  No vehicle holds its wavefront longer than
 * the 5000 sweeps a creeping one needs. */
void emp_lqr_params_default(emp_mpc_params* p);
int emp_lqr_lateral(emp_ctx* ctx, const emp_mpc_params* p, int32_t B, int32_t max_path, const double* target_path,
                    const int32_t* n_path, const double* state, const double* vx, const int32_t* min_index,
                    double* steer, double* K, double* e_rr, double* k_r, int32_t* min_index_out, double* pre_pro,
                    int32_t* sweeps, int32_t* status, emp_mem where);

/* ---- longitudinal PID, feed-forward MPC and the fused vehicle-control step (ABI 12) -------------------------------
 * ref: controller/controller.py classes Longitudinal_PID_controller (:614-678), Vehicle_control (:680-724) and
 * Lateral_MPC__with_feedforward_controller (:727-990).
 *
 * emp_pid_longitudinal: PID_control(target_speed) (:641-678) for B vehicles, bit-exact with the reference.  speed_kmh [B] is
 * 3.6 * sqrt(x*x + y*y + z*z) of the vehicle's velocity, computed by the caller as the reference does (:647-649);
 * target_speed [B].  The deque of the last errors is err [B][EMP_PID_BUFFER], oldest first, with n_err [B] entries (a count
 * outside [0, EMP_PID_BUFFER] is clamped).  The error is appended before the separation test; with fewer than 2 entries the
 * integral and derivative are 0; |error| > error_threshold sets the integral to 0 and clears the buffer (the derivative term
 * stays).  command [B] = K_P e + K_I integral + K_D derivative.  err_out / n_err_out receive the buffer after the call (entries at
 * and past n_err_out are 0) and MAY be the same arrays as err_in / n_err_in: with EMP_DEVICE a fleet keeps its PID state on
 * the device across steps.  dt = 0 gives IEEE inf / NaN where the reference raises ZeroDivisionError.  A NaN error (a NaN speed or
 * target) enters the buffer as the quiet NaN 0x7ff8000000000000 whatever the sign of the NaN it came from, so that every call
 * that runs this rule (emp_vehicle_control, emp_rollout, emp_drive and their timed forms) stores the same bits. */
#define EMP_PID_BUFFER 60
typedef struct emp_pid_params {
    double K_P, K_I, K_D, dt, error_threshold;     /* controller.py:622, :638: 1.15, 0, 0, 0.01, 1 */
} emp_pid_params;
void emp_pid_params_default(emp_pid_params* p);
int emp_pid_longitudinal(emp_ctx* ctx, const emp_pid_params* p, int32_t B, const double* speed_kmh, const double* target_speed,
                         const double* err_in, const int32_t* n_err_in, double* command, double* err_out, int32_t* n_err_out,
                         emp_mem where);

/* emp_mpc_ff_lateral: Lateral_MPC__with_feedforward_controller.MPC_control (:972-990) for B vehicles; inputs and status as
 * emp_mpc_lateral, except that vx [B] is NOT clamped (cal_vehicle_info, :758-776) and min_index is only the fallback when
 * no path point lies within 100 m (the search covers the whole path, :850-866).  N = 4 steps x P = 2 controls, ts = 0.1;
 * the model uses Vx + 0.0001 (its C terms too), C_bar k_r times the raw Vx (:821), e_fi = fi - theta_r.  R_bar regularises
 * only the first P steps' controls (:939-940), so H has a 2-D null space along u4 - u5 and u6 - u7: u0..u3 and the pair sums
 * u4 + u5, u6 + u7 are determined, the split of a pair is the interior point's.  p->q_diag / f_diag / r are Q, F, R
 * (emp_mpc_ff_params_default: (200, 1, 1, 1), (10, 10, 10, 10), 1; :974-979).  steer [B] = u[0] (:990); optional outputs (NULL to
 * skip): u [B][8], e_rr [B][4], k_r [B], pre_pro [B][4], H [B][8][8], f [B][8], iters [B].
 * Non-finite and singular input is answered as by emp_mpc_lateral (EMP_ST_QP_FAILED, steer 0, u all zero), and so is
 * vx + 0.0001 == 0, which divides this law's model by zero.  Path points at exactly the same distance from the predicted pose -
 * a standstill trajectory is a run of identical points - match at the lowest index, as the reference's strict `<` does. */
#define EMP_MPC_FF_CONTROLS 8
void emp_mpc_ff_params_default(emp_mpc_params* p);
int emp_mpc_ff_lateral(emp_ctx* ctx, const emp_mpc_params* p, int32_t B, int32_t max_path, const double* target_path,
                       const int32_t* n_path, const double* state, const double* vx, const int32_t* min_index,
                       double* steer, double* u, double* e_rr, double* k_r, int32_t* min_index_out, double* pre_pro,
                       double* H, double* f, int32_t* iters, int32_t* status, emp_mem where);

/* emp_vehicle_control: Vehicle_control.run_step(target_speed) (:680-724) for B vehicles in ONE kernel launch: the lateral law
 * (lateral = EMP_LAT_MPC: emp_mpc_lateral, EMP_LAT_LQR: emp_lqr_lateral, with `lat` as their params and the same inputs),
 * then emp_pid_longitudinal with `pid`, then the actuation: steer = min(1, s) if s >= 0 else max(-1, s); acc >= 0: throttle
 * min(1, acc), brake 0; else throttle 0, brake max(1, acc) = 1 (the reference's expression, kept).  Python's min / max keep
 * their first argument against NaN: a NaN steering command gives -1, a NaN acceleration throttle 0 and brake 1.
 * control [B][3] = throttle, steer, brake; lat_command [B] is the raw lateral output, bit-identical to the stand-alone entry
 * point's steer on the same inputs; lon_command [B] the PID command; min_index_out, e_rr [B][4], k_r, pre_pro [B][4] as there.
 * A vehicle whose lateral status is non-zero gets zero controls, lon_command 0, and err_out / n_err_out = err_in / n_err_in
 * unchanged (the reference raises in _control() before PID_control runs, :700-702).  err_out / n_err_out may alias err_in /
 * n_err_in.  Optional outputs (NULL to skip): lat_command, lon_command, e_rr, k_r, pre_pro. */
typedef enum emp_lateral_law { EMP_LAT_MPC = 0, EMP_LAT_LQR = 1 } emp_lateral_law;
int emp_vehicle_control(emp_ctx* ctx, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid, int32_t B,
                        int32_t max_path, const double* target_path, const int32_t* n_path, const double* state,
                        const double* vx, const int32_t* min_index, const double* speed_kmh, const double* target_speed,
                        const double* err_in, const int32_t* n_err_in, double* control, double* lat_command,
                        double* lon_command, int32_t* min_index_out, double* e_rr, double* k_r, double* pre_pro,
                        double* err_out, int32_t* n_err_out, int32_t* status, emp_mem where);

/* ---- the vehicle model and the closed-loop rollout ------------------------------------------------------------------
 * THE MODEL IS THIS PROJECT'S DEFINITION, NOT THE REFERENCE'S.  The reference has no vehicle model: its main loop
 * (test_9.py:336-436) runs Vehicle_control.run_step 100 times per planning cycle against CARLA's physics.  Ours is the dynamic
 * bicycle model that the controllers' own cal_A_B_C_fun (controller.py:115-148) linearises, stepped with the bilinear rule the
 * controllers discretise it with (:159-165).  New with ABI 13's library; adding functions does not change EMP_ABI_VERSION.
 *
 * emp_vehicle_step: one tick of B vehicles.  state [B][6] = x, y, fi, Vy, fi_dot, Vx (pose; body-frame lateral velocity, yaw
 * rate and longitudinal velocity); control [B][3] = throttle, steer, brake, as emp_vehicle_control writes them.  In this order,
 * every operation rounded separately (no contraction), `/` IEEE division:
 *   delta = steer_gain * steer;   ax = (throttle_accel * throttle - brake_decel * brake) - drag * Vx
 *   Vxc = Vx with the reference's sign-preserving clamp |Vxc| >= 0.005 (controller.py:106-109)
 *   a11 = (Cf + Cr) / (m * Vxc)                 a12 = (a * Cf - b * Cr) / (m * Vxc) - Vxc
 *   a21 = (a * Cf - b * Cr) / (Iz * Vxc)        a22 = (a * a * Cf + b * b * Cr) / (Iz * Vxc)
 *   bv1 = -Cf / m,  bv2 = -a * Cf / Iz,  h = dt / 2,  mij = h * aij
 *   the lateral pair z = (Vy, fi_dot) solves (I - h A) z+ = (I + h A) z + dt * bv * delta by Cramer's rule:
 *     l11 = 1 - m11, l12 = -m12, l21 = -m21, l22 = 1 - m22
 *     r1 = ((1 + m11) * Vy + m12 * fi_dot) + (dt * bv1) * delta;   r2 = (m21 * Vy + (1 + m22) * fi_dot) + (dt * bv2) * delta
 *     det = l11 * l22 - l12 * l21;   Vy+ = (r1 * l22 - l12 * r2) / det;   fi_dot+ = (l11 * r2 - l21 * r1) / det
 *   (the rule is A-stable: no speed makes the step blow up where the continuous model decays)
 *   the pose steps from the OLD values: x+ = x + dt * (Vx * cos fi - Vy * sin fi), y+ = y + dt * (Vx * sin fi + Vy * cos fi),
 *   fi+ = fi + dt * fi_dot;   Vx+ = max(Vx + dt * ax, 0): the model does not reverse.
 *   Vx+ is `v > 0 ? v : 0` with v = Vx + dt * ax: never negative, never -0.0 (v = 0 exactly gives +0.0), and a NaN v steps to 0 -
 *   a NaN Vx, a NaN throttle or brake, and an infinite Vx too (drag * inf is NaN with drag = 0, and inf - inf otherwise).  The speed
 *   recovers from a NaN within the tick; x+ and y+, which use the OLD Vx, are NaN and stay so.  A NaN steer reaches Vy+ and fi_dot+
 *   only, a NaN in x, y or fi only the pose.  The clamp keeps the sign of a Vx < 0 only: -0.0 and every |Vx| < 0.005 that is not
 *   negative give Vxc = +0.005.  Controls are not clipped: values outside [0, 1] and [-1, 1] enter ax and delta as they are.
 * Optional outputs (NULL to skip) are the next emp_vehicle_control call's inputs, so a chain of calls never leaves the device:
 * ctl_state [B][5] = x, y, fi, Vy, fi_dot; vx_ctl [B] = the clamped Vx+; speed_kmh [B] = 3.6 * sqrt(Vx+ * Vx+ + Vy+ * Vy+).
 * state_out may alias state.  vp->reserved must be 0.
 * With the controllers' default vehicle_para (the reference drivers' tuple, unpacked in the controllers' order) a radian of wheel
 * angle yields about 0.03 rad/s of yaw rate at 10 m/s: this plant follows straight and very gently curved paths only. */
typedef struct emp_vehicle_params {
    double a, b, Cf, Cr, m, Iz;            /* as emp_mpc_params (the controllers' defaults) */
    double dt;                             /* tick, 0.01 s: the PID's */
    double steer_gain;                     /* wheel angle [rad] per unit steer, 1.0: the MPC treats u as the wheel angle */
    double throttle_accel, brake_decel;    /* m/s^2 per unit throttle / brake: 3.0, 6.0 */
    double drag;                           /* 1/s, 0.0 */
    int32_t reserved;                      /* must be 0 */
} emp_vehicle_params;
void emp_vehicle_params_default(emp_vehicle_params* p);
int emp_vehicle_step(emp_ctx* ctx, const emp_vehicle_params* vp, int32_t B, const double* state, const double* control,
                     double* state_out, double* ctl_state, double* vx_ctl, double* speed_kmh, emp_mem where);

/* emp_rollout: T closed-loop ticks of B vehicles in ONE kernel launch.  Tick t is exactly emp_vehicle_control (lateral law
 * `lateral` with `lat`, PID `pid`) on (ctl_state, vx_ctl, speed_kmh, min_index, PID state), followed by emp_vehicle_step with `vp`
 * on its controls; the next tick takes emp_vehicle_step's ctl_state / vx_ctl / speed_kmh, emp_vehicle_control's min_index_out and
 * err_out / n_err_out.  Tick 0's ctl_state, vx_ctl and speed_kmh come from state [B][6] by emp_vehicle_step's own formulas (the
 * first five values, the clamp, 3.6 * sqrt(Vx * Vx + Vy * Vy)).  There are no special cases: a vehicle whose lateral status is
 * non-zero in a tick gets zero controls, keeps its PID state and coasts through that tick (emp_vehicle_control's rule), and
 * takes part in the next tick like any other (its min_index_out may have become valid).  EVERY OUTPUT EQUALS, BIT FOR BIT, T
 * iterations of the two stand-alone calls on the same arrays.
 * Inputs as emp_vehicle_control (target_path [B][max_path][4], n_path [B] clamped to [0, max_path], min_index [B],
 * target_speed [B], err_in [B][EMP_PID_BUFFER], n_err_in [B]); T in [1, EMP_ROLLOUT_MAX_TICKS], log_every >= 1.
 * Outputs: state_out [B][6], min_index_out [B], err_out / n_err_out (each may alias its input); status [B] = OR of the ticks'
 * lateral statuses; fail_tick [B] = first tick with a non-zero status, -1 if none.  Optional logs (NULL to skip) have
 * n_log = ceil(T / log_every) rows, tick-major; tick t is logged when t % log_every == 0: log_state [n_log][B][6] (the state the
 * controller saw), log_control [n_log][B][3], log_err [n_log][B][4] (e_rr), log_index [n_log][B] (the tick's min_index_out).
 * As in emp_vehicle_control, e_rr of a tick whose status is non-zero is computed from path slot 0 whatever n_path says.
 * Cost: EMP_LAT_LQR's Riccati iteration may take 5000 sweeps for a creeping vehicle (controller.py:470-481), a wavefront runs
 * as long as its slowest lane, and the rollout multiplies that by T: keep LQR fleets moving. */
#define EMP_ROLLOUT_MAX_TICKS 65536
int emp_rollout(emp_ctx* ctx, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid, const emp_vehicle_params* vp,
                int32_t B, int32_t max_path, const double* target_path, const int32_t* n_path, const double* state,
                const int32_t* min_index, const double* target_speed, const double* err_in, const int32_t* n_err_in, int32_t T,
                int32_t log_every, double* state_out, int32_t* min_index_out, double* err_out, int32_t* n_err_out, int32_t* status,
                int32_t* fail_tick, double* log_state, double* log_control, double* log_err, int32_t* log_index, emp_mem where);

/* ---- the timed rollout: the PID follows the speed planner's profile, tick by tick ------------------------------------------
 * THE SAMPLING RULE IS THIS PROJECT'S DEFINITION, NOT THE REFERENCE'S.  The reference densifies its speed plan to 401 points
 * "because control runs 10x as often as planning" (speed_planning_test.py:517) and then drives with a constant ref_speed
 * (test_10.py:554): it never closes this loop.  New with ABI 13's library; adding functions does not change EMP_ABI_VERSION.
 *
 * trajectory [B][7][EMP_TIMED_POINTS] is emp_plan_trajectory's (x, y, heading, kappa, speed, accel, time); only two rows are read:
 * speed = trajectory[b][4][.] in m/s and time = trajectory[b][6][.] in s, on the clock base the caller chose with
 * plan_start_time.  t0 [B] is the vehicle's clock at tick 0, cap [B] (emp_rollout_timed: target_speed [B]) a speed in km/h: the
 * road limit (the reference's ref_speed), and the target where there is no profile.  cursor [B] is the bracket the last tick used.
 *
 * The rule, per vehicle; every operation is rounded separately (no contraction), `/` is IEEE division:
 *   n_v = the largest n in [0, 401] such that for all i < n neither time[i] nor speed[i] is NaN (x != x)
 *   clock = t0 + (double)tick * dt              (the product is rounded, then the sum)
 *   if n_v == 0 or clock is NaN:  target = cap, bits = EMP_TGT_NO_PROFILE; the cursor is unchanged (0 if n_v == 0); nothing else
 *     applies (no cap test)
 *   else if clock < time[0]:          v = speed[0],        bit EMP_TGT_BEFORE;  the cursor is unchanged
 *   else if clock >= time[n_v - 1]:   v = speed[n_v - 1],  bit EMP_TGT_PAST;    the cursor is unchanged
 *   else (n_v >= 2):  j = the incoming cursor clamped to [0, n_v - 2];  while (j + 1 <= n_v - 2 && time[j + 1] <= clock) ++j;
 *     d = time[j + 1] - time[j];  if d > 0: w = (clock - time[j]) / d, v = speed[j] + w * (speed[j + 1] - speed[j]); else v = speed[j];
 *     the outgoing cursor is j
 *   target = 3.6 * v;  if target > cap: target = cap, bit EMP_TGT_CAPPED (a NaN cap compares false: no cap)
 * "Unchanged" means the incoming value as it is, not clamped.  The rule is defined by this text for any row, ascending or not; on
 * the planner's ascending rows (increase_points: (i - 1) * T / 400) the cursor makes the common tick three loads and at most one
 * step: the clock moves dt = 0.01 s per tick against about 0.02 s per sample.
 *
 * emp_speed_target: one tick's sampling for B vehicles.  cursor_in may be NULL (zeros); cursor_out may alias cursor_in; tick >= 0.
 * target_kmh [B], cursor_out [B], tgt_status [B] = this tick's bits.
 *
 * emp_rollout_timed: emp_rollout with the constant target replaced by the rule, in ONE kernel launch, for both laws: tick t uses
 * clock = t0 + (double)(tick0 + t) * vp->dt and the cursor tick t - 1 left (tick 0: cursor_in).  The target and the cursor are
 * computed on every tick whatever the tick's lateral status.  EVERY OUTPUT EQUALS, BIT FOR BIT, T iterations of
 * emp_speed_target(tick0 + t, dt = vp->dt) -> emp_vehicle_control(target_speed = target_kmh) -> emp_vehicle_step on the same arrays,
 * so a rollout cut in two (T1 ticks, then tick0 = T1 on the first one's outputs) resumes bit for bit.
 * emp_rollout_timed_io holds emp_rollout's arrays under their names (target_speed [B] is the cap), and
 *   inputs:  trajectory, t0 [B], cursor_in [B] (NULL = zeros)
 *   outputs: cursor_out [B], tgt_status [B] = OR of the ticks' bits (both required); log_target [n_log][B] (optional): the km/h
 *            target of each logged tick, rows as log_state
 * Each output may alias the input of its name.  reserved must be 0.  The lateral path stays target_path / n_path (the cycle's traj /
 * traj_len): the trajectory's x / y / heading / kappa rows are not read.
 * Refused (EMP_ERR_INVALID): T outside [1, EMP_ROLLOUT_MAX_TICKS], tick0 < 0, tick0 + T > INT32_MAX, log_every < 1, reserved != 0,
 * a NULL required pointer, EMP_HOST_PINNED.  B == 0: EMP_OK.  With a pipeline set both calls fence like every non-cycle entry
 * point.  Cost: as emp_rollout, plus one scan of the two rows per vehicle and three loads per tick. */
#define EMP_TGT_BEFORE 1
#define EMP_TGT_PAST 2
#define EMP_TGT_NO_PROFILE 4
#define EMP_TGT_CAPPED 8
#define EMP_TIMED_POINTS 401
int emp_speed_target(emp_ctx* ctx, int32_t B, const double* trajectory, const double* t0, int32_t tick, double dt, const double* cap,
                     const int32_t* cursor_in, double* target_kmh, int32_t* cursor_out, int32_t* tgt_status, emp_mem where);
typedef struct emp_rollout_timed_io {
    const double* target_path;             /* [B][max_path][4] */
    const int32_t* n_path;                 /* [B] */
    const double* state;                   /* [B][6] */
    const int32_t* min_index;              /* [B] */
    const double* target_speed;            /* [B] km/h: the cap */
    const double* err_in;                  /* [B][EMP_PID_BUFFER] */
    const int32_t* n_err_in;               /* [B] */
    const double* trajectory;              /* [B][7][EMP_TIMED_POINTS] */
    const double* t0;                      /* [B] */
    const int32_t* cursor_in;              /* [B] or NULL */
    double* state_out;
    int32_t* min_index_out;
    double* err_out;
    int32_t* n_err_out;
    int32_t* status;
    int32_t* fail_tick;
    int32_t* cursor_out;
    int32_t* tgt_status;
    double* log_state;                     /* optional logs */
    double* log_control;
    double* log_err;
    int32_t* log_index;
    double* log_target;
    int32_t reserved;                      /* must be 0 */
} emp_rollout_timed_io;
int emp_rollout_timed(emp_ctx* ctx, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid, const emp_vehicle_params* vp,
                      int32_t B, int32_t max_path, int32_t T, int32_t tick0, int32_t log_every, const emp_rollout_timed_io* io,
                      emp_mem where);

/* ---- S-T speed DP (BASELINE config 5; reference planner/speed_planning_test.py) ----------------
 * The S-T grid is hard-coded in the reference (40 non-uniform s samples :114, 16 t samples :116); tables are
 * [B][EMP_ST_ROWS][EMP_ST_COLS], row 0 = largest s (CalcSTCoordinate, :287-305).  Obstacle slots hold NaN when
 * absent (:43-46, :255); max_obs <= 64. */
#define EMP_ST_ROWS 40
#define EMP_ST_COLS 16

/* ref: generate_st_graph (speed_planning_test.py:38-98): dynamic obstacles [B][max_obs] (s, l, s_dot, l_dot; the scan
 * stops at the first NaN s) -> S-T segments s_in, s_out, t_in, t_out [B][max_obs], NaN = ignored */
int emp_st_graph(emp_ctx* ctx, int32_t B, int32_t max_obs, const double* obs_s, const double* obs_l,
                 const double* obs_s_dot, const double* obs_l_dot, double* s_in, double* s_out, double* t_in,
                 double* t_out, emp_mem where);

/* ref: speed_DP (speed_planning_test.py:101-188): forward sweep over the 40 x 16 grid with state-dependent edges
 * (CalcDpCost :191-231: source row 0 means "the DP origin", acceleration from the speed stored at the source node),
 * terminal node = last <=-minimum over the right column then the top row (:158-172), backtrack (:178-186).
 * The reference raises IndexError in its backtrack (float row index) and aliases its two output arrays (:156);
 * here the predecessor is an integer and speed_s / speed_t [B][16] are separate (NaN after the terminal column).
 * cost, s_dot [B][40][16] doubles and node [B][40][16] int32 are the reference's dp_st_cost / dp_st_s_dot /
 * dp_st_node; each may be NULL.  end_node [B][2] = (row, col) of the terminal node, (-1, -1) if every cost is NaN.
 * A NaN plan_start_s_dot does not get there: column 0 of cost is NaN, and since the sweep keeps a candidate only if it is
 * < the +inf it starts from (:138-152), every later column stays +inf with s_dot 0 and node 0; the terminal search's <=
 * then ends on (0, 15) and the profile runs along row 0.  A +-inf start leaves the whole table +inf in the same way.
 * A slot is absent iff its s_in is NaN, and then its s_out, t_in and t_out are never looked at.  A live slot may hold
 * anything: its cost is the reference's arithmetic on those values, where a NaN distance (a NaN member, a point segment
 * with s_in == s_out and t_in == t_out, inf - inf) costs nothing and an infinite s_out / t_out leaves the distance to the
 * finite end.
 * A negative w_cost_obs is refused (EMP_ERR_ARG): w ** (1.5 - d) (:281) is complex there and the reference fails on its
 * next comparison.  Scenes are independent; the order in which the library runs them (heaviest first) shows in nothing. */
int emp_speed_dp(emp_ctx* ctx, const emp_speed_dp_params* p, int32_t B, int32_t max_obs, const double* s_in,
                 const double* s_out, const double* t_in, const double* t_out, const double* plan_start_s_dot,
                 double* cost, double* s_dot, int32_t* node, int32_t* end_node, double* speed_s, double* speed_t,
                 emp_mem where);

/* ref: CalcDpCost (:191-231) / CalcObsCost (:234-271) for arbitrary edges: edges [B][n_edges][5] =
 * s_start, t_start, s_dot_start, s_end, t_end against scene b's obstacles -> total [B][n_edges] and (optional)
 * the obstacle term alone */
int emp_st_edge_costs(emp_ctx* ctx, const emp_speed_dp_params* p, int32_t B, int32_t n_edges, int32_t max_obs,
                      const double* edges, const double* s_in, const double* s_out, const double* t_in,
                      const double* t_out, double* total, double* obs, emp_mem where);

/* ref: CalcCollisionCost (:274-284): n distances -> n costs */
int emp_st_collision_cost(emp_ctx* ctx, int32_t n, double w_cost_obs, const double* min_dis, double* cost, emp_mem where);

/* ref: calc_speed_planning_start_condition (:23-35), called by the driver at test_10.py:249: the planning start's velocity and
 * acceleration (Cartesian) projected on the path tangent at the start's heading, n scenes -> s_dot [n], s_dot2 [n] */
int emp_speed_start_condition(emp_ctx* ctx, int32_t n, const double* vx, const double* vy, const double* ax, const double* ay,
                              const double* heading, double* s_dot, double* s_dot2, emp_mem where);

/* ---- S-T speed planning back end (reference planner/speed_planning_test.py:308-620) ----
 * Status bits of these four entry points (per scene; the arrays of a flagged scene are NaN): */
#define EMP_STB_RANGE 2       /* scipy interp1d bounds error / np.interp on an empty path (ValueError in the reference) */
#define EMP_STB_INDEX 4       /* IndexError in the reference (s_ub[16], dp_speed_s[16], a trajectory without NaN padding) */
#define EMP_STB_QP_FAILED 8   /* speed QP infeasible or not converged */
#define EMP_STB_NO_PROFILE 64 /* the profile / trajectory starts with NaN: nothing to work on */
#define EMP_SPEED_DP_COLS 16
#define EMP_SPEED_QP_POINTS 17
#define EMP_SPEED_DENSE_POINTS 401

/* ref: keyword arguments of speed_QP, speed_planning_test.py:410-411 */
typedef struct emp_speed_qp_params {
    double w_cost_s_dot2, w_cost_v_ref, w_cost_jerk;    /* 10, 50, 500 */
    double reference_speed;                             /* 50 */
} emp_speed_qp_params;
void emp_speed_qp_params_default(emp_speed_qp_params* p);

/* ref: generate_convex_space (:308-407).  dp_speed_s / dp_speed_t [B][16] (NaN behind the terminal column, as
 * emp_speed_dp returns them); path_index2s / path_kappa [B][max_path] with path_len[b] entries handed to the
 * reference (ascending; a zero-padded tail is recognised as in :326-330); obstacle S-T segments [B][n_slots], NaN =
 * empty.  Outputs s_lb, s_ub, s_dot_lb, s_dot_ub [B][16] (+-inf where unbounded). */
int emp_speed_convex_space(emp_ctx* ctx, int32_t B, int32_t n_slots, int32_t max_path, double max_lateral_accel,
                           const double* dp_speed_s, const double* dp_speed_t, const double* path_index2s,
                           const double* path_kappa, const int32_t* path_len, const double* s_in, const double* s_out,
                           const double* t_in, const double* t_out, double* s_lb, double* s_ub, double* s_dot_lb,
                           double* s_dot_ub, int32_t* status, emp_mem where);

/* ref: speed_QP (:410-511).  The reference's call cannot run (untransposed equality matrix, bounds never passed,
 * ub aliased to lb); this solves the problem it states: piecewise-linear acceleration through qp_size = (valid DP
 * columns) time stations dt = T / (qp_size - 1) apart, station 0 pinned to (0, plan_start_s_dot, plan_start_s_dot2),
 * station i >= 1 bounded by column i-1 of the convex space and -6 <= s_dot2 <= 4, s non-decreasing, cost
 * sum w_a s_dot2^2 + w_v (s_dot - v_ref)^2 + w_j (s_dot2_{i+1} - s_dot2_i)^2.  Outputs [B][17], NaN behind the last
 * station.  A DP profile without NaN tail is EMP_STB_INDEX, as in the reference (:435). */
int emp_speed_qp(emp_ctx* ctx, const emp_speed_qp_params* p, int32_t B, const double* plan_start_s_dot,
                 const double* plan_start_s_dot2, const double* dp_speed_s, const double* dp_speed_t, const double* s_lb,
                 const double* s_ub, const double* s_dot_lb, const double* s_dot_ub, double* qp_s, double* qp_s_dot,
                 double* qp_s_dot2, double* relative_time, int32_t* iters, int32_t* status, emp_mem where);

/* ref: increase_points (:514-566): [B][17] profiles -> [B][401] samples (the first sample lies at -dt and the last
 * interval extrapolates the one before it, as in the reference) */
int emp_speed_increase_points(emp_ctx* ctx, int32_t B, const double* s_init, const double* s_dot_init,
                              const double* s_dot2_init, const double* relative_time_init, double* s, double* s_dot,
                              double* s_dot2, double* relative_time, int32_t* status, emp_mem where);

/* ref: path_speed_merge (:569-620): speed samples [B][401] x path arrays [B][max_path] (n_init[b] entries as handed to
 * the reference, NaN behind the valid points) -> trajectory [B][7][401] = x, y, heading, kappa, speed, accel, time */
int emp_path_speed_merge(emp_ctx* ctx, int32_t B, int32_t max_path, const double* s, const double* s_dot,
                         const double* s_dot2, const double* relative_time, const double* current_time,
                         const double* path_s, const double* x_init, const double* y_init, const double* heading_init,
                         const double* kappa_init, const int32_t* n_init, double* trajectory, int32_t* status,
                         emp_mem where);

/* ---- path cycle + S-T speed planner in one call (ABI 13) ---------------------------------------------------------------
 * ref: motion_planning of test_10.py:99-340 - the reference's most complete planning loop: plan the path (emp_plan_cycle exactly:
 * every emp_cycle_io output, the front end included, equals emp_plan_cycle's bit for bit), project the DYNAMIC obstacles onto the
 * planned trajectory, run the speed planner; the result is a timed trajectory.  Per scene, on the device, no host round trip:
 *   1. rows x, y, heading, kappa of width W = max_pts + 2 from traj / traj_len, NaN from traj_len on (the reference's
 *      trajectory_index2s and path_speed_merge are MATLAB transliterations that need a NaN behind the valid points: W
 *      guarantees one)
 *   2. trajectory_index2s on those rows (the chords summed left to right, as emp_trajectory_index2s)
 *   3. calc_speed_planning_start_condition(start_v, start_a, start_heading)
 *   4. find_match_points(dyn xy, traj[:traj_len], is_first_run = False, dyn_pre_match); every projected node is taken at the
 *      FIRST obstacle's match (planning_utils.py:169)
 *   5. cal_s_l_fun(dyn xy, traj[:traj_len], s_map = path_index2s)
 *   6. cal_dy_obs_deri with the projected heading and kappa (it stops at the first NaN l)
 *   7. generate_st_graph; slots at or beyond n_dyn are NaN in all four inputs
 *   8. speed_DP, generate_convex_space (path = the W-wide rows, max_lateral_accel = 0.2 * 9.8, the reference's default),
 *      speed_QP, increase_points, path_speed_merge(current_time = plan_start_time)
 * Steps 1-7 are one wavefront per scene (speed_front_wave_kernel); 8 are the kernels of the stand-alone entry points with their
 * launch configurations - the values equal the chain emp_trajectory_index2s -> emp_speed_start_condition -> emp_find_match_points
 * -> emp_s_l -> emp_dy_obs_deri -> emp_st_graph -> emp_speed_dp -> emp_speed_convex_space -> emp_speed_qp ->
 * emp_speed_increase_points -> emp_path_speed_merge on the same arrays, bit for bit.
 * Statuses stay separate: io->status keeps the path's EMP_ST_* bits, speed_status takes the OR of the speed stages' EMP_STB_* bits
 * (the two sets overlap: 2, 4 and 8 mean different things).  The speed half runs for every scene whatever its path status.  A
 * scene with n_dyn > 0 whose obstacle match cannot start inside [0, traj_len) (dyn_pre_match outside it, or an empty trajectory:
 * the reference's IndexError, planning_utils.py:132) gets speed_status = EMP_STB_INDEX alone and an all-NaN trajectory; its
 * st_segments are NaN and its dp_speed is the DP of that empty graph.  With n_dyn == 0 the match loop never runs: no error.
 * Decisions pinned on test_10's defects:
 *   - :136 unpacks the 8-tuples its driver sends (:521) as 4-tuples: the path half's io->dyn_dis_speed is the caller's, and the
 *     request packer (service.plan_trajectory_requests) takes fields 6 and 7 (dis, speed) of the first dynamic obstacle
 *   - :234-238 and :244 use undefined or chained-assigned names: the trajectory arrays are the columns of the cycle's traj
 *   - :268-271 hand the GLOBAL path's match index to a search on the ~60-point local trajectory, an IndexError in every cycle
 *     with a dynamic obstacle once the vehicle is more than a trajectory's length of nodes along its path: dyn_pre_match makes
 *     the index explicit (NULL = 0, the Python default; the global index reproduces the reference literally)
 *   - :350 replies with the obstacles' match list where test_9 sends the global-path match index, which the driver feeds back as
 *     the next pre_match_index on the global path: the reply carries the global-path match index, as plan_requests does
 *   - the last of the 401 samples takes the arrays' last slots (speed_planning_test.py:608-611), NaN when padded: kept
 * Limits: 1 <= max_dyn <= 64 (the speed DP's), and the emp_plan_cycle limits.  EMP_HOST_PINNED is refused (HostRing slots carry
 * the cycle's layout only); with EMP_OPT_CYCLE_GRAPH set the call is not captured and runs as plain launches.  B == 0: EMP_OK.
 * Pipelined, the speed half runs on the call's lane (staged: its back stream) behind the Cartesian tail: its outputs are complete
 * on emp_result_stream() like the path's. */
typedef struct emp_speed_io {
    /* inputs */
    const double* dyn_obs;          /* [B][max_dyn][4] x, y, vx, vy of the dynamic obstacles (test_10.py:258-265) */
    const int32_t* n_dyn;           /* [B] (clamped to [0, max_dyn]) */
    const double* start_heading;    /* [B] plan_start_heading (test_10.py:247: atan2(vy, vx) of start_v, computed by the caller) */
    const double* plan_start_time;  /* [B] the merge's current_time (test_10.py:325: cur_time + 0.1, added by the caller) */
    const int32_t* dyn_pre_match;   /* [B] pre_match_index of the obstacles' find_match_points on the trajectory; NULL = 0 */
    /* outputs */
    double* trajectory;             /* [B][7][401] x, y, heading, kappa, speed, accel, time  (required) */
    int32_t* speed_status;          /* [B] EMP_STB_* bits (required) */
    double* path_index2s;           /* [B][max_pts + 2] trajectory_index2s of the rows, optional */
    double* st_segments;            /* [4][B][max_dyn] s_in, s_out, t_in, t_out (plane-major, as emp_speed_dp takes them), optional */
    double* dp_speed;               /* [2][B][16] speed_s, speed_t of the speed DP, optional */
    double* speed_profile;          /* [4][B][17] qp_s, qp_s_dot, qp_s_dot2, relative_time of the speed QP, optional */
    int32_t reserved;               /* must be 0 */
} emp_speed_io;

int emp_plan_trajectory(emp_ctx* ctx, const emp_dp_params* p, const emp_qp_params* q, const emp_smooth_params* sp,
                        const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp, int32_t B, int32_t max_ref,
                        int32_t max_obs, int32_t max_pts, int32_t max_dyn, emp_dp_mode mode, const emp_cycle_io* io,
                        const emp_speed_io* sio, emp_mem where);

/* ---- the fleet loop: perceive, predict, plan, adopt, track - K periods on the device (additions: the ABI stays 13) -----------
 * ref: the driver's main loop, test_9.py:336-436.  emp_drive_request is what the driver does between two planning requests:
 * get_actor_from_world (test_9.py:48-89), predict_block (planning_utils.py:591-614), the planner's gate on the nearest static
 * obstacle (test_9.py:116) and the first dynamic obstacle's (dis, speed).  One wavefront per vehicle, one actor per lane.
 * Arithmetic, per vehicle with state = x, y, fi, Vy, fi_dot, Vx (emp_vehicle_step's; fi in radians - the reference's degrees-to-
 * radians factor is the caller's), every operation rounded separately, IEEE division and sqrt, c = cos fi, s = sin fi:
 *   wx = Vx c - Vy s,  wy = Vx s + Vy c                               the ego's world-frame velocity
 * per actor (x_a, y_a, vx_a, vy_a in the world frame, z = 0):
 *   dis   = sqrt((x - x_a)^2 + (y - y_a)^2 + 0)
 *   v1    = (x_a - x, y_a - y)
 *   lat   = v1x (-s) + v1y c
 *   along = v1x wx + v1y wy
 *   speed = sqrt(vx_a^2 + vy_a^2 + 0)
 *   kept    when dis < dis_limitation and -lateral_band < lat < lateral_band and along > behind  (NaN compares false: dropped)
 *   dynamic when kept and speed > dynamic_speed, else static
 * Each class is ordered by dis ascending, equal dis in actor-index order (Python's stable list.sort).  Then
 *   n_obs = n_static if n_static > 0 and static_dis[0] <= static_gate, else 0          (the cycle's static count, test_9.py:116)
 *   dyn_dis_speed = the first dynamic's (dis, speed), (NaN, NaN) without one            (the cycle's io->dyn_dis_speed)
 *   V = sqrt(wx^2 + wy^2 + 0),  beta = atan2(wy, wx) - fi,  V_y = V sin beta,  V_x = V cos beta,  ts = pred_ts
 *   start_xy = (x + V_x ts c - V_y ts s,  y + V_y ts c + V_x ts s)                     products left to right, as the Python
 *   pred_fi = fi + fi_dot ts,  origin_xy = (x, y),  start_v = (wx, wy),  start_a = accel (NULL: zeros)
 *   actors_next = (x_a + vx_a advance_s, y_a + vy_a advance_s, vx_a, vy_a): the product rounded, then the sum; slots at or
 *                 beyond n_act copied unchanged; optional, may be `actors`
 * n_act is clamped to [0, max_act] and slots at or beyond it are never read.  Unused output slots are 0.  static_xy / static_dis
 * hold the max_obs nearest statics and dyn the max_dyn nearest dynamics; req_status is EMP_DRV_TRUNCATED when more were kept.
 * On a threshold, tied and non-finite (each follows from the formulas above; tests/test_gpu_drive_request_cases.py pins them):
 *   - `<` and `>` are strict and the gate is `<=`: an actor AT dis_limitation, AT +-lateral_band or AT `behind` is dropped, a
 *     speed AT dynamic_speed is static, a nearest static AT static_gate opens the gate.
 *   - actors of one class with bit-equal dis come out in actor-index order, a truncated list keeps the lowest indices, and the two
 *     classes are ranked separately: an equal dis in the other class moves nothing.
 *   - NaN compares false.  An actor with a NaN or infinite x_a or y_a is dropped.  A kept actor with a NaN vx_a or vy_a is STATIC
 *     (speed > dynamic_speed is false; its actors_next position is NaN); an infinite velocity makes it dynamic with speed = inf,
 *     and its advance is inf * advance_s.
 *   - a NaN or infinite ego x or y keeps nothing (n_static = n_dyn = n_obs = 0, dyn_dis_speed = NaN) and origin_xy / start_xy carry
 *     it: the prediction is not finite.  A NaN fi, Vy or Vx, and an infinite fi, make `along` NaN: nothing is kept, start_xy and
 *     start_v (and start_heading) are NaN.  A NaN fi_dot reaches pred_fi only; a NaN accel reaches start_a only.
 *   - zeros keep their signs and atan2 follows C Annex F: at fi = 0, Vy = +0 a speed Vx = -0.0 gives w = (-0, +0), start_heading =
 *     pi and beta = pi; V = 0, so start_xy = (x, y).  A vehicle at rest (Vx = Vy = +0) has start_heading = +0, along = 0 for every
 *     actor (all of them are "in front") and start_xy = (x, y).
 * Limits: 1 <= max_act <= 64, 1 <= max_obs <= 256, 1 <= max_dyn <= 64. */
#define EMP_DRV_TRUNCATED 1
#define EMP_DRIVE_MAX_PERIODS 4096

typedef struct emp_drive_params {
    double dis_limitation;      /* 50  (test_9.py:377) */
    double lateral_band;        /* 5   (:77) */
    double behind;              /* -10 (:78) */
    double dynamic_speed;       /* 1   (:81) */
    double static_gate;         /* 30  (:116) */
    double pred_ts;             /* 0.2 (:335) */
    double advance_s;           /* seconds the actors move per call; 0.  emp_drive uses the double product T * dt instead */
    int32_t reserved;           /* must be 0 */
} emp_drive_params;
void emp_drive_params_default(emp_drive_params* p);

/* state [B][6], accel [B][2] or NULL, actors [B][max_act][4], n_act [B] -> static_xy [B][max_obs][2], n_static [B],
 * static_dis [B][max_obs], dyn [B][max_dyn][4] = x, y, dis, speed, n_dyn [B], dyn_dis_speed [B][2], n_obs [B], origin_xy [B][2],
 * start_xy [B][2], pred_fi [B], start_v [B][2], start_a [B][2], req_status [B]; actors_next [B][max_act][4] or NULL. */
int emp_drive_request(emp_ctx* ctx, const emp_drive_params* p, int32_t B, int32_t max_act, int32_t max_obs, int32_t max_dyn,
                      const double* state, const double* accel, const double* actors, const int32_t* n_act, double* static_xy,
                      int32_t* n_static, double* static_dis, double* dyn, int32_t* n_dyn, double* dyn_dis_speed, int32_t* n_obs,
                      double* origin_xy, double* start_xy, double* pred_fi, double* start_v, double* start_a,
                      int32_t* req_status, double* actors_next, emp_mem where);

/* emp_drive: K periods of [request, plan, adopt, T ticks] on emp_stream(), stream-ordered, without a host synchronisation or a
 * copy between them (the host waits only where emp_plan_cycle itself does).  Period k:
 *   1. the request above on state / accel / actors, advance_s = T * vp->dt (actors move in place)
 *   2. emp_plan_cycle exactly as it runs with io->global_path set (EMP_DP_TWO_KERNEL, one batch at a time) on the request's
 *      arrays: obs_xy = static_xy, n_obs, dyn_dis_speed, origin_xy, start_xy, start_v, start_a; pre_match_index of period k + 1 is
 *      this period's match_index
 *   3. adopt: a plan is valid when ref_status == 0 and (status & ~EMP_ST_DP_INFEASIBLE) == 0 (the service's rule).  Valid: its
 *      traj[0..traj_len) becomes the track, track_len = traj_len, held = 0.  Otherwise track / track_len stay and held += 1 (the
 *      service's "previous" policy; the counter is the report).  A vehicle that never had a valid plan has track_len == 0: the
 *      rollout flags it and it coasts
 *   4. emp_rollout's kernel, unchanged: T ticks on track / track_len, min_index = 0 and an empty PID deque (the reference builds a
 *      new Vehicle_control every period, test_9.py:415), the caller's target_speed [B]
 *   5. accel = (w(state after the period) - w(state the controller saw at tick T - 1)) / vp->dt, w as above, in a trailing
 *      one-lane-per-vehicle kernel
 * In/out arrays: each *_out may be the memory of its input.  Logs are optional (NULL), one row per period.
 * Decisions pinned on the reference:
 *   - the reference tracks the reply to the PREVIOUS request (a blocking recv sits right behind the send, test_9.py:390-395); here
 *     the plan of period k drives period k.  The one-period lag is the reference's way of hiding a 0.3 s planner: not reproduced
 *   - the reference's plant is CARLA; ours is emp_vehicle_step, and its caveat stands: gentle paths only
 *   - the speed planner (emp_plan_trajectory) is not part of THIS loop: target_speed is the caller's constant, as test_9.py:420.
 *     emp_drive_timed below is the loop with the speed planner in it and the PID on its profile
 * Limits: 1 <= K <= EMP_DRIVE_MAX_PERIODS, T as emp_rollout, max_obs <= 253, the emp_plan_cycle and emp_drive_request limits.
 * B == 0: EMP_OK.  EMP_HOST_PINNED is refused.  With a pipeline set the call fences like every non-cycle entry point, runs its
 * periods one at a time and leaves the setting as it found it; EMP_OPT_CYCLE_GRAPH is ignored (plain launches).  With
 * lateral = EMP_LAT_LQR keep the fleet at 5 m/s and above (emp_rollout's cost note). */
typedef struct emp_drive_io {
    /* inputs */
    const double* global_path;      /* [B][max_global][4] */
    const int32_t* n_global;        /* [B] */
    const double* state;            /* [B][6] */
    const double* accel;            /* [B][2] world-frame acceleration, NULL = zeros */
    const double* actors;           /* [B][max_act][4] */
    const int32_t* n_act;           /* [B] */
    const int32_t* pre_match_index; /* [B] */
    const double* track;            /* [B][max_pts + 1][4] */
    const int32_t* track_len;       /* [B] */
    const int32_t* held;            /* [B] */
    /* outputs (required; each may alias the input of its name) */
    double* state_out;
    double* accel_out;
    double* actors_out;
    int32_t* pre_match_index_out;
    double* track_out;
    int32_t* track_len_out;
    int32_t* held_out;
    /* per-period logs, NULL to skip */
    double* log_state;              /* [K][B][6] state at the start of the period */
    int32_t* log_plan_status;       /* [K][B] status | ref_status */
    int32_t* log_roll_status;       /* [K][B] */
    int32_t* log_held;              /* [K][B] */
    int32_t* log_counts;            /* [K][B][2] n_obs, n_dyn */
    double* log_traj;               /* [K][B][max_pts + 1][4] the period's plan, adopted or not */
    int32_t* log_traj_len;          /* [K][B] */
    int32_t reserved;               /* must be 0 */
} emp_drive_io;

int emp_drive(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth,
              const emp_drive_params* drive_params, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid,
              const emp_vehicle_params* vp, int32_t B, int32_t max_global, int32_t max_obs, int32_t max_pts, int32_t max_act,
              int32_t max_dyn, int32_t K, int32_t T, const double* target_speed, const emp_drive_io* io, emp_mem where);

/* ---- the timed fleet loop: the speed planner and profile tracking inside the drive (additions: the ABI stays 13) -------------
 * ref: the reference's most complete loop, test_10.py - emp_drive with emp_plan_trajectory in place of emp_plan_cycle and
 * emp_rollout_timed in place of emp_rollout, so a fleet driven on the device slows down for a vehicle ahead.
 *
 * THE CLOCK (the one new rule).  emp_drive_timed takes t0 [B] (seconds, per vehicle) and a scalar tick0 >= 0: emp_rollout_timed's
 * convention, continued over periods.  With dt = vp->dt:
 *   tick_k = tick0 + k * T                                           period k's first tick (integer arithmetic)
 *   the rollout of period k is emp_rollout_timed's kernel with t0 and tick0 = tick_k: tick t of it samples the profile at
 *     clock = t0 + (double)(tick_k + t) * dt                         a function of the tick NUMBER, as in emp_rollout_timed
 *   plan_start_time of period k = (t0 + (double)tick_k * dt) + plan_lead        the product rounded, then each sum
 * plan_lead is emp_drive_timed_params' field, 0.1 by default (test_10.py:325: cur_time + 0.1).  NOTHING ACCUMULATES: a run of K
 * periods equals a run of K1 periods followed by a run of K - K1 periods with tick0 + K1 * T on the first run's outputs, BIT FOR
 * BIT.  Refused (EMP_ERR_INVALID): tick0 < 0, and tick0 + K * T > INT32_MAX.
 *
 * emp_drive_request_timed: emp_drive_request with the speed planner's inputs (emp_speed_io) beside the cycle's, from the same
 * kernel text - the request holds each dynamic actor's (x, y, vx, vy) and its rank in registers, and no later kernel can recover
 * them once the actors have advanced in place.  Every output it shares with emp_drive_request equals that call's bit for bit, and
 *   dyn_obs [B][max_dyn][4]  = x, y, vx, vy of the kept dynamic actors in dyn's order (dis ascending, ties in actor-index
 *                              order), positions BEFORE the advance; slots at or beyond n_dyn are 0
 *   start_heading [B]        = atan2(wy, wx): the value beta is made of, not a second evaluation (test_10.py:247)
 *   plan_start_time [B]      = (t0 + (double)tick * dt) + plan_lead
 * t0 [B], dyn_obs, start_heading and plan_start_time are required; tick >= 0, dt finite and > 0, plan_lead finite (also in
 * emp_drive_timed_params), else EMP_ERR_INVALID. */
int emp_drive_request_timed(emp_ctx* ctx, const emp_drive_params* p, int32_t B, int32_t max_act, int32_t max_obs, int32_t max_dyn,
                            const double* state, const double* accel, const double* actors, const int32_t* n_act, const double* t0,
                            int32_t tick, double dt, double plan_lead, double* static_xy, int32_t* n_static, double* static_dis,
                            double* dyn, int32_t* n_dyn, double* dyn_dis_speed, int32_t* n_obs, double* origin_xy, double* start_xy,
                            double* pred_fi, double* start_v, double* start_a, int32_t* req_status, double* actors_next,
                            double* dyn_obs, double* start_heading, double* plan_start_time, emp_mem where);

/* emp_drive_timed: K periods of [timed request, path and speed plan, adopt, T timed ticks, acceleration] on emp_stream(), stream-
 * ordered, without a host synchronisation or a copy between them.  Period k:
 *   1. emp_drive_request_timed at tick_k on state / accel / actors, advance_s = T * vp->dt (actors move in place)
 *   2. emp_plan_trajectory exactly as it runs with io->global_path set (EMP_DP_TWO_KERNEL, one batch at a time): the path half as
 *      in emp_drive; the speed half on the request's dyn_obs, n_dyn, start_heading and plan_start_time, dyn_pre_match = NULL
 *   3. adopt.  The TRACK by emp_drive's rule: valid when ref_status == 0 and (status & ~EMP_ST_DP_INFEASIBLE) == 0.  The PROFILE
 *      when the path is valid AND speed_status == 0: the 7 x 401 doubles of the period's trajectory become profile_out,
 *      cursor = 0, speed_held = 0.  Otherwise the profile and the cursor stay as they are and speed_held += 1; the track is adopted
 *      or held by its own rule, independently.  A held profile is still on the absolute clock, so the sampling rule goes on
 *      reading it; when the clock passes its end the rule holds its last speed and reports EMP_TGT_PAST.  A VEHICLE THAT NEVER HAD
 *      A PROFILE carries the caller's initial one - all NaN is the natural start: the rule then gives it the cap (target_speed) and
 *      sets EMP_TGT_NO_PROFILE
 *   4. emp_rollout_timed's kernel: T ticks on the adopted track and profile with t0, the carried cursor and tick0 = tick_k; a new
 *      controller every period (min_index 0, an empty PID deque), as in emp_drive.  target_speed [B] is the cap, in km/h
 *   5. accel as in emp_drive (the same kernel)
 * EVERY OUTPUT AND LOG EQUALS, BIT FOR BIT, K iterations of emp_drive_request_timed -> emp_plan_trajectory (io->global_path set)
 * -> the adopt rule of 3 -> emp_rollout_timed(tick0 = tick_k) -> the acceleration formula, on the same arrays.
 * emp_drive_timed_io holds emp_drive_io's fields under their names, and
 *   inputs:  t0 [B]; profile [B][7][EMP_TIMED_POINTS]; cursor [B]; speed_held [B]                                  (all required)
 *   outputs: profile_out, cursor_out, speed_held_out (required; each may alias the input of its name: an element is read by the
 *            lane that writes it)
 *   logs, one row per period, NULL to skip: log_speed_status [K][B] the period's speed_status; log_speed_held [K][B];
 *            log_tgt_status [K][B] the OR of the period's ticks' EMP_TGT_* bits; log_cursor [K][B] the cursor the period's ticks
 *            START from (0 for a profile adopted in that period); log_profile [K][B][7][401] the period's timed trajectory, adopted
 *            or not - 22 456 B per vehicle per period: 736 MB for one period of 32768 vehicles
 * Limits: emp_drive's, emp_plan_trajectory's (1 <= max_dyn <= 64) and emp_rollout_timed's, and the clock's above.  EMP_HOST_PINNED
 * is refused; EMP_OPT_CYCLE_GRAPH is ignored (plain launches); with a pipeline set the call fences like every non-cycle entry point,
 * runs its periods one at a time and leaves the setting as it found it.  B == 0: EMP_OK.  reserved must be 0 in both structs.
 * Memory: the call keeps one timed trajectory per vehicle (22 456 B) beside emp_drive's temporaries. */
typedef struct emp_drive_timed_params {
    double plan_lead;               /* 0.1 (test_10.py:325): plan_start_time = clock at the period's first tick + plan_lead */
    int32_t reserved;               /* must be 0 */
} emp_drive_timed_params;
void emp_drive_timed_params_default(emp_drive_timed_params* p);

typedef struct emp_drive_timed_io {
    /* inputs: emp_drive_io's */
    const double* global_path;      /* [B][max_global][4] */
    const int32_t* n_global;        /* [B] */
    const double* state;            /* [B][6] */
    const double* accel;            /* [B][2] world-frame acceleration, NULL = zeros */
    const double* actors;           /* [B][max_act][4] */
    const int32_t* n_act;           /* [B] */
    const int32_t* pre_match_index; /* [B] */
    const double* track;            /* [B][max_pts + 1][4] */
    const int32_t* track_len;       /* [B] */
    const int32_t* held;            /* [B] */
    /* ... and the timed loop's */
    const double* t0;               /* [B] the vehicle's clock at tick 0, seconds */
    const double* profile;          /* [B][7][EMP_TIMED_POINTS] the timed trajectory being followed; all NaN = none yet */
    const int32_t* cursor;          /* [B] the sampling rule's bracket */
    const int32_t* speed_held;      /* [B] */
    /* outputs (required; each may alias the input of its name) */
    double* state_out;
    double* accel_out;
    double* actors_out;
    int32_t* pre_match_index_out;
    double* track_out;
    int32_t* track_len_out;
    int32_t* held_out;
    double* profile_out;
    int32_t* cursor_out;
    int32_t* speed_held_out;
    /* per-period logs, NULL to skip: emp_drive_io's */
    double* log_state;              /* [K][B][6] state at the start of the period */
    int32_t* log_plan_status;       /* [K][B] status | ref_status */
    int32_t* log_roll_status;       /* [K][B] */
    int32_t* log_held;              /* [K][B] */
    int32_t* log_counts;            /* [K][B][2] n_obs, n_dyn */
    double* log_traj;               /* [K][B][max_pts + 1][4] the period's plan, adopted or not */
    int32_t* log_traj_len;          /* [K][B] */
    /* ... and the timed loop's */
    int32_t* log_speed_status;      /* [K][B] EMP_STB_* bits of the period's speed plan */
    int32_t* log_speed_held;        /* [K][B] */
    int32_t* log_tgt_status;        /* [K][B] OR of the period's ticks' EMP_TGT_* bits */
    int32_t* log_cursor;            /* [K][B] the cursor the period's ticks start from */
    double* log_profile;            /* [K][B][7][EMP_TIMED_POINTS] the period's timed trajectory, adopted or not */
    int32_t reserved;               /* must be 0 */
} emp_drive_timed_io;

int emp_drive_timed(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth,
                    const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp, const emp_drive_params* drive_params,
                    const emp_drive_timed_params* timed_params, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid,
                    const emp_vehicle_params* vp, int32_t B, int32_t max_global, int32_t max_obs, int32_t max_pts, int32_t max_act,
                    int32_t max_dyn, int32_t K, int32_t T, int32_t tick0, const double* target_speed, const emp_drive_timed_io* io,
                    emp_mem where);

/* ---- global routing: B queries over one road graph, routes expanded to global paths (additions: the ABI stays 13) -------------
 * ref: planner/global_planning.py - _A_star (:168-214), _route_search (:153-166), search_path_way (:234-272) - and
 * planning_utils.py waypoint_list_2_target_path (:29-46).  The PROCEDURE is the contract, not "a shortest path": the edge cost is
 * a waypoint count, the heuristic a distance in metres (it over-estimates at the driver's 2 m resolution), and closed nodes are
 * never reopened, so any other search order returns other routes.  One wavefront per query runs the reference's pop-and-relax
 * loop; the lanes share the arg-min of a pop and the successors of the popped node.
 *
 * The graph (emp_route_graph, all arrays contiguous, shared by every query):
 *   vertex [N][3]    the reference's 2-decimal rounded entry / exit positions, in node-id order (_build_graph's ids)
 *   succ_off [N+1], succ [E]   CSR successor lists in the order DiGraph.successors yields them (first add_edge of a pair)
 *                    a list names no node twice (one edge per (u, v), as in a DiGraph): the lanes of a wavefront relax the successors
 *                    of a node side by side.  REQUIRED of EMP_DEVICE graphs too, where it cannot be checked: a repeated successor
 *                    is memory-safe there, but which of its two edges sets g, parent and stamp is undefined
 *   length [E]       edge costs, len(path) + 1;  0 <= length <= 2^18
 *   wp_off [E+1], wp [W][3]    per edge: the entry waypoint, the path waypoints, the exit waypoint (at least 2)
 * An edge id e is a position in succ; its ends are n_end (the node whose list holds e) and n_exit = succ[e].
 *
 * A query: start_node, end_edge, origin_wp [3], dest_wp [3] (the CARLA look-ups _find_location_edge / get_waypoint are the host's).
 * Arithmetic, every operation rounded separately, IEEE sqrt:
 *   dist(p, q) = sqrt(((dx dx) + (dy dy)) + (dz dz))
 *   h(n) = dist(vertex[n], vertex[n_end]),  f(n) = (double) g[n] + h(n)      g int32; a NaN f orders as +inf
 * Per node: NEW, OPEN or CLOSED, g, parent, stamp (the order of its FIRST insertion into the open set; an update keeps it).
 *   start_node is OPEN with g = 0, parent = -1, stamp = 0.  Then, at most N times (each pop closes a node):
 *     c = the OPEN node with the smallest f, equal f: the smallest stamp (Python's min over a dict).  None: EMP_ROUTE_UNREACHABLE
 *     c == n_end: close it, stop
 *     for every successor suc of c in CSR order, len its edge's length:
 *       CLOSED: skipped;  OPEN: g[c] + len < g[suc] (integers) sets g and parent;  NEW: OPEN, g[c] + len, parent c, the next stamp
 *     close c
 *   route = the parents back from n_end, reversed, then n_exit;  route_len = its length (>= 2)
 * Expansion (emp_route_paths).  The edge of (u, v) is the first e in u's list with succ[e] == v; closest(p, list) is the first
 * index with the strictly smallest dist (a NaN or infinite distance never wins; none: the reference's -1, read as Python reads
 * it - list[-1:] on the first edge is its exit waypoint alone, L[:0] on the last edge is nothing):
 *   first edge (route[0], route[1]): its waypoints from closest(origin_wp, all of them) onwards
 *   each further edge but the last, only when route_len > 3: its waypoints without the entry
 *   last edge (route[-2], route[-1]): L = its waypoints without the entry, k = closest(dest_wp, L); L[0..k] when k != 0
 * (kept quirks: a two-node route emits its one edge twice; the first edge is the one A* left start_node by, not the origin's own).
 * wp_index [B][max_global] are positions in wp, global_path [B][max_global][4] = x, y, theta, kappa of those waypoints with theta
 * and kappa bit for bit what emp_heading_kappa gives on the same xy (none below 2 points), n_global [B] the count.
 * status [B]: 0, or EMP_ROUTE_UNREACHABLE (route_len = n_global = 0), or EMP_ROUTE_BAD_QUERY (start_node outside [0, N), end_edge
 * outside [0, E), or - EMP_DEVICE only, where the graph cannot be checked - an offset or successor index out of range met on the
 * way: never followed, route_len = n_global = 0), or EMP_ROUTE_TRUNCATED (route_len > max_route or n_global > max_global: the
 * counts are the true lengths, only the capacity is written; a truncated route is still expanded in full).  Unused slots are 0.
 * With EMP_HOST the graph is checked first (finite values, monotone offsets, indices in range, no repeated successor, the limits above): a violation is
 * EMP_ERR_INVALID.  Refused as well: N > EMP_ROUTE_MAX_NODES, N < 1, max_route < 2, max_global < 1, reserved != 0,
 * EMP_HOST_PINNED.  B == 0: EMP_OK. */
#define EMP_ROUTE_MAX_NODES 4096
#define EMP_ROUTE_MAX_LENGTH (1 << 18)
#define EMP_ROUTE_UNREACHABLE 1
#define EMP_ROUTE_TRUNCATED 2
#define EMP_ROUTE_BAD_QUERY 4

typedef struct emp_route_graph {
    const double* vertex;           /* [n_nodes][3] */
    const int32_t* succ_off;        /* [n_nodes + 1] */
    const int32_t* succ;            /* [n_edges] */
    const int32_t* length;          /* [n_edges] */
    const int32_t* wp_off;          /* [n_edges + 1] */
    const double* wp;               /* [n_wp][3] */
    int32_t n_nodes, n_edges, n_wp;
    int32_t reserved;               /* must be 0 */
} emp_route_graph;

/* A* only: start_node [B], end_edge [B] -> route [B][max_route], route_len [B], status [B]. */
int emp_route_search(emp_ctx* ctx, const emp_route_graph* graph, int32_t B, int32_t max_route, const int32_t* start_node,
                     const int32_t* end_edge, int32_t* route, int32_t* route_len, int32_t* status, emp_mem where);

/* ... and the expansion: origin_wp [B][3], dest_wp [B][3] -> wp_index, global_path, n_global as above.  global_path / n_global are
 * what emp_reference_line, emp_plan_cycle (io->global_path) and emp_drive take. */
int emp_route_paths(emp_ctx* ctx, const emp_route_graph* graph, int32_t B, int32_t max_route, int32_t max_global,
                    const int32_t* start_node, const int32_t* end_edge, const double* origin_wp, const double* dest_wp,
                    int32_t* route, int32_t* route_len, int32_t* wp_index, double* global_path, int32_t* n_global, int32_t* status,
                    emp_mem where);

/* ---- routed traffic: the agents' local planner and PID pair (new with ABI 13's library; EMP_ABI_VERSION is unchanged) --------
 * ref: the dynamic obstacle of the reference's drivers is a BehaviorAgent on a route (test_9.py:288-291), stepped once per control
 * tick (test_9.py:344).  With no hazard in sight that step is LocalPlanner.run_step (agents/navigation/local_planner.py:208-260)
 * and VehiclePIDController.run_step (agents/navigation/controller.py:54-92).  NOT reproduced: offset != 0; random waypoint
 * creation (_stop_waypoint_creation is always true after set_global_plan); BehaviorAgent's traffic-light and pedestrian
 * branches (they need CARLA's map queries); CARLA's float32 Location and its z coordinate.  The target speed is the
 * caller's, as set_target_speed(30.0) is in the driver.  BehaviorAgent's car-following branch and its speed-limit target are
 * reproduced by emp_agent_behave (the section after this one).
 *
 * The rule, per agent; every operation is rounded separately (no contraction), `/` and sqrt are IEEE, clip(v) = min(max(v, -1), 1)
 * in NumPy's form (a NaN passes through).  It reads the pose x, y and the forward vector (c, s), speed_kmh and target_speed (both
 * km/h), the path [max_path][4] in emp_route_paths' global_path layout (only x and y are read) and n_path (clamped to
 * [0, max_path]).  It keeps head (int32, clamped to [0, n_path] on entry), past_steer, and two deques of EMP_AGENT_BUFFER doubles,
 * oldest first, with counts n_lon and n_lat (clamped to [0, 10]).  Deque entries at and past the count are never read and come
 * out as they went in.  One tick:
 *   1. purge.  min_distance = base_min_distance + 0.5 * (speed_kmh / 3.6).  While head < n_path: (px, py) = path[head],
 *      md = (n_path - head == 1) ? 1 : min_distance; if sqrt((x - px) * (x - px) + (y - py) * (y - py)) < md then ++head, else stop
 *      (a NaN distance compares false and stops the purge).
 *   2. empty queue.  head == n_path (n_path == 0 included): control = (0, 0, 1), status EMP_AGT_DONE, lat_error = lon_command = 0;
 *      past_steer and both deques stay as they are (the reference does not call the controller).
 *   3. longitudinal PID.  e = target_speed - speed_kmh is appended; a full deque drops its oldest entry.  With at least 2 entries
 *      de = (e[-1] - e[-2]) / dt and ie = (the sum from +0, oldest first) * dt; with fewer, both are 0.
 *      acc = clip((lon_K_P * e + lon_K_D * de) + lon_K_I * ie).
 *   4. lateral PID and actuation.  (wx, wy) = (px - x, py - y) for path[head];  nn = sqrt(wx * wx + wy * wy) * sqrt((c * c + s * s) + 0).
 *      nn == 0: dot = 1 (the reference's own value, one radian: kept).  Otherwise dot = acos(clip(((wx * c + wy * s) + 0) / nn)).
 *      If c * wy - s * wx < 0 then dot = -dot.  dot is appended; de, ie and cs = clip(...) as in step 3 with the lat_ gains.
 *      Rate limit: cs > past_steer + 0.1 gives past_steer + 0.1; else cs < past_steer - 0.1 gives past_steer - 0.1.
 *      steer = cs >= 0 ? min(max_steer, cs) : max(-max_steer, cs).
 *      acc >= 0: throttle = min(acc, max_throttle), brake = 0; otherwise throttle = 0, brake = min(|acc|, max_brake).
 *      min / max are Python's: they keep their FIRST argument unless the second is strictly smaller / larger, so a NaN cs gives
 *      steer = -max_steer, and a NaN acc throttle 0 and a NaN brake.  past_steer = steer.
 *   A NaN enters a deque as the quiet NaN 0x7ff8000000000000.  acos is the one libm call of the law: outputs that depend on it
 *   (lat_error, the newest lateral entry, a steer that neither limit binds) may differ from another libm's by its last bits times
 *   about 6 (lat_K_P + lat_K_D / dt + lat_K_I * dt); every other output is determined to the bit.
 *
 * emp_agent_observe stands in for the CARLA getters, from state [A][6] = x, y, fi, Vy, fi_dot, Vx (emp_vehicle_step's):
 *   (c, s) = (cos fi, sin fi), as emp_drive_request takes them;  (wx, wy) = (Vx * c - Vy * s, Vx * s + Vy * c);
 *   forward [A][2] = c, s;  speed_kmh [A] = 3.6 * sqrt((wx * wx + wy * wy) + 0) (get_speed);  actors [A][4] = x, y, wx, wy: the
 *   row emp_drive and emp_drive_timed take as an actor.  Each output is optional (NULL), at least one is required.
 *   It exists so that the law's acos argument is made of data the caller can see: emp_agent_control takes (c, s) as data.
 *
 * emp_agent_control: one tick of the rule for A agents, one kernel.  Inputs: path [A][max_path][4], n_path [A], state [A][6] (x and
 * y are read), forward [A][2], speed_kmh [A], target_speed [A], head [A], past_steer [A], lon_err [A][10], n_lon [A],
 * lat_err [A][10], n_lat [A].  Outputs: control [A][3] = throttle, steer, brake; status [A]; head_out, past_steer_out, lon_err_out,
 * n_lon_out, lat_err_out, n_lat_out (each may alias its input); optional lat_error [A] (the signed dot) and lon_command [A] (acc).
 *
 * emp_agent_rollout: T ticks in ONE launch.  Tick t is emp_agent_observe, then emp_agent_control, then emp_vehicle_step(vp) on its
 * controls.  EVERY OUTPUT EQUALS, BIT FOR BIT, T iterations of those three calls on the same arrays, so a rollout cut in two
 * resumes bit for bit.  A DONE agent keeps braking: its vehicle is stepped with (0, 0, 1) like any other.  T in
 * [1, EMP_ROLLOUT_MAX_TICKS], log_every >= 1.  emp_agent_rollout_io: the inputs of emp_agent_control without forward and speed_kmh;
 * outputs state_out [A][6] and the agent state (each may alias its input), status [A] (the OR over ticks), done_tick [A] (the first
 * DONE tick, -1 if none), optional actors_out [A][4] (observe of the final state) and optional logs of n_log = ceil(T / log_every)
 * rows, tick t logged when t % log_every == 0: log_state [n_log][A][6] (the state the tick saw), log_control [n_log][A][3],
 * log_head [n_log][A] (head after the tick's purge).
 * Use emp_vehicle_params with the tuple in physical order (a, b, Cf, Cr, m, Iz) = (1.015, 1.895, -148970, -82204, 1412, 1537) for a
 * vehicle that takes corners: emp_vehicle_params_default keeps the controllers' unpacking order, whose plant barely yaws.
 * Refused (EMP_ERR_INVALID): a NULL required pointer, max_path < 1, A < 0, T outside its range, log_every < 1, reserved != 0,
 * EMP_HOST_PINNED.  A == 0: EMP_OK.  With a pipeline set the three calls fence like every non-cycle entry point. */
#define EMP_AGENT_BUFFER 10
#define EMP_AGT_DONE 1
typedef struct emp_agent_params {
    double lat_K_P, lat_K_I, lat_K_D;      /* 1.95, 0.05, 0.2 (local_planner.py:73) */
    double lon_K_P, lon_K_I, lon_K_D;      /* 1.0, 0.05, 0.0 (:74) */
    double dt;                             /* 0.05 (:70) */
    double max_throttle, max_brake, max_steer; /* 0.75, 0.3, 0.8 (:75-77) */
    double base_min_distance;              /* 3.0 (:79) */
    int32_t reserved;                      /* must be 0 */
} emp_agent_params;
void emp_agent_params_default(emp_agent_params* p);
int emp_agent_observe(emp_ctx* ctx, int32_t A, const double* state, double* forward, double* speed_kmh, double* actors, emp_mem where);
int emp_agent_control(emp_ctx* ctx, const emp_agent_params* p, int32_t A, int32_t max_path, const double* path, const int32_t* n_path,
                      const double* state, const double* forward, const double* speed_kmh, const double* target_speed,
                      const int32_t* head, const double* past_steer, const double* lon_err, const int32_t* n_lon,
                      const double* lat_err, const int32_t* n_lat, double* control, int32_t* status, int32_t* head_out,
                      double* past_steer_out, double* lon_err_out, int32_t* n_lon_out, double* lat_err_out, int32_t* n_lat_out,
                      double* lat_error, double* lon_command, emp_mem where);
typedef struct emp_agent_rollout_io {
    const double* path;                    /* [A][max_path][4] */
    const int32_t* n_path;                 /* [A] */
    const double* state;                   /* [A][6] */
    const double* target_speed;            /* [A] km/h */
    const int32_t* head;                   /* [A] */
    const double* past_steer;              /* [A] */
    const double* lon_err;                 /* [A][EMP_AGENT_BUFFER] */
    const int32_t* n_lon;                  /* [A] */
    const double* lat_err;                 /* [A][EMP_AGENT_BUFFER] */
    const int32_t* n_lat;                  /* [A] */
    double* state_out;
    int32_t* head_out;
    double* past_steer_out;
    double* lon_err_out;
    int32_t* n_lon_out;
    double* lat_err_out;
    int32_t* n_lat_out;
    int32_t* status;
    int32_t* done_tick;
    double* actors_out;                    /* optional */
    double* log_state;                     /* optional logs */
    double* log_control;
    int32_t* log_head;
    int32_t reserved;                      /* must be 0 */
} emp_agent_rollout_io;
int emp_agent_rollout(emp_ctx* ctx, const emp_agent_params* p, const emp_vehicle_params* vp, int32_t A, int32_t max_path, int32_t T,
                      int32_t log_every, const emp_agent_rollout_io* io, emp_mem where);

/* ---- traffic that reacts to traffic: BehaviorAgent's car-following (new with ABI 13's library; EMP_ABI_VERSION is unchanged) ----
 * ref: BehaviorAgent.run_step (agents/navigation/behavior_agent.py:296-362) for the "normal", "cautious" and "aggressive" agents of
 * behavior_types.py: the target speed from the speed limit (_update_information, :65-82), the vehicle-ahead detector
 * (_vehicle_obstacle_detected, :84-138, with is_within_distance, agents/tools/misc.py:66-103), the time-to-collision rule
 * (car_following_manager, :253-294) and the emergency stop (:364-375), on top of the local planner and PID pair of the section
 * above, whose rule (one "agent tick" below) is called unchanged.
 * NOT reproduced: traffic lights and pedestrians (the section after this one puts them in front of this rule: emp_agent_behave_hazards);
 * tailgating and lane changes (the law is that of a road whose markings allow none:
 * _tailgating then only looks behind); the junction branch (:347-352: it needs RoadOptions the router does not produce);
 * BasicAgent.run_step; per-road speed limits (the limit is per agent and constant over a call).
 * Stand-ins for CARLA's map: map.get_waypoint(location) compares (road_id, lane_id); here every path waypoint carries an int32
 * lane key, lane [max_path] beside the path, and a vehicle IS ON the key of the waypoint behind its queue's head:
 * lane[max(head - 1, 0)] with head as at the start of the tick, -1 (never matches) if it has no plan.  That holds for the ego
 * (key_cur) and for every other agent.  A key below 0 never matches.  The 45 m pre-filter round the ego's lane waypoint (:201-202) is
 * not a step of its own: the detector's own range is max(min_proximity_threshold, speed_limit / 3), so the filter cannot decide
 * anything while speed_limit / 3 plus the agent's offset from its lane centre stays below 45 m (a limit under about 130 km/h).
 *
 * Worlds.  Agents are laid out [W][max_world]; world w holds n_world[w] agents (clamped to [0, max_world]), max_world <=
 * EMP_TRAFFIC_MAX_WORLD.  Agents see only their own world.  Padding slots are never read and never written (EMP_HOST arrays are staged:
 * an output array comes back whole, its padding slots as 0).  A world may also hold
 * n_other[w] (clamped to [0, max_other], max_other <= 64) vehicles that the call does not drive: other [W][max_other][5] = x, y,
 * world-frame vx, vy, half extent, and other_lane [W][max_other] their keys.  The first four columns are emp_drive's actor row.
 * At tick t of a call an other stands at x + vx * ((tick0 + t) * dt), y + vy * ((tick0 + t) * dt) with emp_agent_params.dt: nothing
 * accumulates (emp_drive_timed's clock rule).  Its km/h is 3.6 * sqrt((vx * vx + vy * vy) + 0).
 * Per agent: the arrays of emp_agent_control without target_speed; speed_limit in km/h (get_speed_limit); extent, the half extent
 * max(bounding_box.extent.x, .y); lane [max_path].
 *
 * One tick for agent i; every other vehicle is read as it stood at the start of the tick (the reference steps its agents one after
 * another between two world ticks).  Rounding as in the section above; min([..]) and max(a, b) are Python's (the first argument
 * is kept unless a later one is strictly smaller / larger).
 *   1. head == n_path after the clamps: the DONE tick of the agent tick (control (0, 0, 1), status EMP_AGT_DONE), mode
 *      EMP_BHV_DONE, target_speed_out = speed_limit.  (The reference raises here.)  A DONE agent stays visible to the others.
 *   2. th = max(min_proximity_threshold, speed_limit / 3);  key_cur = lane[max(head - 1, 0)];
 *      key_next = lane[min(head + look_steps, n_path - 1)] (get_incoming_waypoint_and_direction(steps=5)).
 *   3. Scan the candidates in order: the world's agents by slot without i, then the others by index.  THE FIRST HIT WINS, not the
 *      nearest.  A candidate whose key is below 0, or equals neither key_cur nor key_next, is passed over.  tv = (xj - xi, yj - yi),
 *      norm = sqrt(tvx * tvx + tvy * tvy).  norm < 0.001: a hit.  norm > th: no hit.  Otherwise
 *      angle = acos(clip((c * tvx + s * tvy) / norm)) * (180 / pi), a hit if and only if 0 < angle < up_angle, with (c, s)
 *      emp_agent_observe's forward vector.  The lower bound is strict as in the reference: a vehicle exactly ahead (angle 0) is not seen.
 *   4. No hit: mode NORMAL, target = min([max_speed, speed_limit - speed_lim_dist]), one agent tick with that target.
 *   5. Hit on j: d = (sqrt((dx * dx + dy * dy) + 0) + 2^-52) - extent_j - extent_i with (dx, dy) = (xi - xj, yi - yj).
 *      d < braking_distance: mode EMERGENCY, control = (0, 0, emergency_brake) (throttle, steer, brake: a fresh control, steer 0);
 *      head, both deques and past_steer stay as they were, lat_error = lon_command = 0, target_speed_out = speed_limit.
 *      Otherwise vs = j's km/h, dv = max(1, (kmh_i - vs) / 3.6), ttc = d / dv, and
 *        safety_time > ttc > 0:                 mode SLOW,   target = min([positive(vs - speed_decrease), max_speed, speed_limit - speed_lim_dist])
 *        2 * safety_time > ttc >= safety_time:  mode FOLLOW, target = min([max(min_speed, vs), max_speed, speed_limit - speed_lim_dist])
 *        otherwise:                             mode CLEAR,  the target of step 4;
 *      then TWO agent ticks with that target on the same observation, the second one's control returned: the reference steps its
 *      local planner in car_following_manager (:275, :284, :292) and once more at the end of run_step (:360).  The second purge finds
 *      nothing to do; both deques take the tick's error twice and the steering rate limit applies twice.
 *   Outputs of a tick beside the agent tick's: mode, blocker (position in the scan order, -1 if none), distance (d) and ttc (+inf
 *   where the rule does not compute them), target_speed_out (what the reference's local planner then holds).  distance and ttc need
 *   no libm call; acos decides a hit only within its last bits of 0 and up_angle.
 *
 * emp_agent_behave: one tick for W worlds, one kernel.  forward [A][2] and speed_kmh [A] are data, as for emp_agent_control
 * (A = W * max_world).  emp_traffic_rollout: T ticks in ONE launch; tick t is emp_agent_observe, emp_agent_behave (tick0 + t),
 * emp_vehicle_step.  EVERY OUTPUT AND LOG ROW EQUALS, BIT FOR BIT, T iterations of those three calls; a rollout cut in two, with
 * tick0 advanced, resumes bit for bit.  Logs as emp_agent_rollout's plus log_mode and log_target; mode_ticks [A][5] counts the ticks
 * spent in NORMAL, SLOW, FOLLOW, CLEAR, EMERGENCY; min_gap [A] is the smallest d seen, +inf if none.  status is the OR over ticks.
 * emp_behavior_io serves both calls; a field the call does not use is not looked at.  Each agent-state output may alias its input.
 *   emp_agent_behave uses: n_world, path, n_path, lane, state, forward, speed_kmh, speed_limit, extent, the agent state in and out,
 *     control, status, mode, blocker, distance, ttc, target_speed_out; optional n_other / other / other_lane (all three, or
 *     max_other == 0), lat_error, lon_command.
 *   emp_traffic_rollout uses: the same inputs without forward and speed_kmh; state_out (may alias state), the agent state out,
 *     status, done_tick, mode_ticks, min_gap; optional actors_out and the five logs.
 * Refused before any launch (EMP_ERR_INVALID): a NULL required pointer, max_world outside [1, 64], max_other outside [0, 64],
 * max_path < 1, W < 0, T outside [1, EMP_ROLLOUT_MAX_TICKS], log_every < 1, tick0 < 0, reserved != 0, EMP_HOST_PINNED.  W == 0: EMP_OK. */
#define EMP_TRAFFIC_MAX_WORLD 64
#define EMP_BHV_NORMAL 0
#define EMP_BHV_SLOW 1
#define EMP_BHV_FOLLOW 2
#define EMP_BHV_CLEAR 3
#define EMP_BHV_EMERGENCY 4
#define EMP_BHV_DONE 5
#define EMP_BHV_CAUTIOUS 0
#define EMP_BHV_KIND_NORMAL 1
#define EMP_BHV_AGGRESSIVE 2
typedef struct emp_behavior_params {
    double max_speed, speed_lim_dist, speed_decrease, safety_time, min_proximity_threshold, braking_distance; /* behavior_types.py */
    double min_speed;                      /* 5 (BehaviorAgent._min_speed) */
    double emergency_brake;                /* 0.5 (BasicAgent._max_brake) */
    double up_angle;                       /* 30 degrees */
    int32_t look_steps;                    /* 5 */
    int32_t reserved;                      /* must be 0 */
} emp_behavior_params;
/* kind: EMP_BHV_CAUTIOUS, EMP_BHV_KIND_NORMAL or EMP_BHV_AGGRESSIVE (anything else: normal) */
void emp_behavior_params_default(emp_behavior_params* p, int32_t kind);
typedef struct emp_behavior_io {
    const int32_t* n_world;                /* [W] */
    const double* path;                    /* [A][max_path][4], A = W * max_world */
    const int32_t* n_path;                 /* [A] */
    const int32_t* lane;                   /* [A][max_path] */
    const double* state;                   /* [A][6] */
    const double* forward;                 /* [A][2] (behave) */
    const double* speed_kmh;               /* [A] (behave) */
    const double* speed_limit;             /* [A] km/h */
    const double* extent;                  /* [A] */
    const int32_t* head;                   /* the agent state, as emp_agent_rollout_io's */
    const double* past_steer;
    const double* lon_err;
    const int32_t* n_lon;
    const double* lat_err;
    const int32_t* n_lat;
    const int32_t* n_other;                /* [W] */
    const double* other;                   /* [W][max_other][5] */
    const int32_t* other_lane;             /* [W][max_other] */
    int32_t* head_out;
    double* past_steer_out;
    double* lon_err_out;
    int32_t* n_lon_out;
    double* lat_err_out;
    int32_t* n_lat_out;
    int32_t* status;                       /* [A] */
    double* control;                       /* [A][3] (behave) */
    int32_t* mode;                         /* [A] (behave) */
    int32_t* blocker;                      /* [A] (behave) */
    double* distance;                      /* [A] (behave) */
    double* ttc;                           /* [A] (behave) */
    double* target_speed_out;              /* [A] (behave) */
    double* lat_error;                     /* [A] optional (behave) */
    double* lon_command;                   /* [A] optional (behave) */
    double* state_out;                     /* [A][6] (rollout) */
    int32_t* done_tick;                    /* [A] (rollout) */
    int32_t* mode_ticks;                   /* [A][5] (rollout) */
    double* min_gap;                       /* [A] (rollout) */
    double* actors_out;                    /* [A][4] optional (rollout) */
    double* log_state;                     /* optional logs (rollout) */
    double* log_control;
    int32_t* log_head;
    int32_t* log_mode;
    double* log_target;
    int32_t reserved;                      /* must be 0 */
} emp_behavior_io;
int emp_agent_behave(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, int32_t W, int32_t max_world,
                     int32_t max_path, int32_t max_other, int64_t tick0, const emp_behavior_io* io, emp_mem where);
int emp_traffic_rollout(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp, int32_t W,
                        int32_t max_world, int32_t max_path, int32_t max_other, int32_t T, int32_t log_every, int64_t tick0,
                        const emp_behavior_io* io, emp_mem where);

/* ---- traffic that stops for red lights and pedestrians (new with ABI 13's library; EMP_ABI_VERSION is unchanged) ----------------
 * ref: the two checks BehaviorAgent.run_step runs before car-following on every tick (agents/navigation/behavior_agent.py:312-328):
 * red lights (traffic_light_manager, :140-148 -> BasicAgent._affected_by_traffic_light, agents/navigation/basic_agent.py:201-249,
 * with its sticky _last_traffic_light) and pedestrians (pedestrian_avoid_manager, :225-251), in front of the rule of the section
 * above, which is called unchanged.  emp_agent_behave and emp_traffic_rollout stay what they are; these calls are theirs plus
 * lights and walkers.
 * NOT reproduced: the lane-change variants of the walker detector (:241-246); ignore_traffic_lights; stop signs; and, as before,
 * the junction branch, tailgating and lane changes.
 * Stand-ins for CARLA's map, beside those of the section above: the ego's lane waypoint (map.get_waypoint(ego location)) has the
 * key key_cur = lane[max(head - 1, 0)], the location path[max(head - 1, 0)] x, y, and a forward vector ve that is the chord
 * path[i0 + 1] - path[i0], i0 = min(max(head - 1, 0), n_path - 2); (0, 0) if n_path == 1.  Only the sign of a dot product with ve is
 * used, so it is not normalised.
 *
 * Worlds as above.  A world also holds
 *   n_light[w] lights (clamped to [0, max_light], max_light <= EMP_HAZARD_MAX): light [W][max_light][4] = x, y, dx, dy, the location
 *     and forward vector of the map waypoint under the light's trigger volume (get_waypoint(get_trafficlight_trigger_location(l)));
 *     light_lane [W][max_light] that waypoint's key (the reference compares road_id only; a light that governs several lane keys is
 *     listed once per key); light_cycle [W][max_light][3] = period, red_from, red_to in ticks.  The light IS RED at tick index k iff
 *     period >= 1 and red_from <= (k mod period) < red_to, in int64 arithmetic: nothing accumulates;
 *   n_walker[w] walkers (clamped to [0, max_walker], max_walker <= EMP_HAZARD_MAX): walker [W][max_walker][5] = x, y, world-frame
 *     vx, vy, half extent, walker_lane [W][max_walker] their keys.  At tick index k a walker stands at x + vx * (k * dt),
 *     y + vy * (k * dt): the clock rule of `other`.
 * Per agent: last_light [A] int32 in and out, the index of the light that holds the agent (_last_traffic_light), -1 for none; any
 * value outside [0, n_light) counts as -1.
 *
 * One tick for agent i at tick index k = tick0 + t.  Rounding as in the section above; libm enters through acos only.
 *   0. head == n_path after the clamps: the DONE tick of the section above.  (The reference raises there, before it looks at a
 *      light.)  last_light_out = last_light as given, cause 0, light_hit = walker_hit = -1, walker_distance = +inf.
 *   1. Red lights.  If last_light >= 0 and that light is red at k: AFFECTED by it, no geometry is looked at.  If it is not red:
 *      last_light = -1.  Then scan the lights in index order, THE FIRST HIT WINS.  A light is passed over if its key is below 0 or
 *      differs from key_cur (key_next plays no part); if ve.x * dx + ve.y * dy < 0; if it is not red at k.  Otherwise it is a hit iff
 *      is_within_distance(light waypoint, vehicle, tlight_threshold, [0, tlight_up_angle]): tv = (x - xi, y - yi),
 *      norm = sqrt(tvx * tvx + tvy * tvy); norm < 0.001: a hit; norm > tlight_threshold: no hit; otherwise
 *      angle = acos(clip((c * tvx + s * tvy) / norm)) * (180 / pi), a hit iff 0 < angle < tlight_up_angle.  A hit sets last_light.
 *      AFFECTED is emergency_stop(): mode EMERGENCY, cause EMP_HZ_LIGHT, control (0, 0, emergency_brake); head, both deques and
 *      past_steer stay, lat_error = lon_command = 0, target_speed_out = speed_limit, distance = ttc = +inf, blocker = -1.
 *      light_hit is the light's index (the sticky one too), -1 if none.
 *   2. Walkers, in index order, THE FIRST HIT WINS.  A walker at (wx, wy) (the clock rule) is a hit iff all of
 *      (a) sqrt((ex * ex + ey * ey) + 0) < walker_radius with (ex, ey) = (wx - px, wy - py), (px, py) the ego's lane waypoint
 *          (:238-239).  Unlike the 45 m vehicle filter this one decides: the detector's own range is
 *          max(min_proximity_threshold, speed_limit / 3) >= walker_radius for the three behaviours;
 *      (b) its key is >= 0 and equals key_cur or key_next;
 *      (c) the `within` of step 3 above with th = max(min_proximity_threshold, speed_limit / 3), tv = (wx - xi, wy - yi) and the
 *          cone 0 < angle < walker_up_angle.
 *      On a hit d = (sqrt((dx * dx + dy * dy) + 0) + 2^-52) - extent_walker - extent_i with (dx, dy) = (xi - wx, yi - wy);
 *      walker_hit and walker_distance = d are reported.  d < braking_distance: emergency_stop() as in step 1, cause EMP_HZ_WALKER.
 *      Otherwise the walker is IGNORED, as in the reference: the tick goes on as if no walker were there.
 *   3. Vehicles: the rule of the section above, unchanged.  Its EMERGENCY has cause EMP_HZ_VEHICLE; every other mode has cause 0.
 *
 * emp_agent_behave_hazards / emp_traffic_rollout_hazards take the arguments of emp_agent_behave / emp_traffic_rollout, then the
 * hazard parameters, max_light, max_walker and emp_hazard_io, which serves both calls.  Everything the counterparts return comes
 * back as they define it.  The rollout: tick t is emp_agent_observe, emp_agent_behave_hazards (tick0 + t), emp_vehicle_step; EVERY
 * OUTPUT AND LOG ROW EQUALS, BIT FOR BIT, T iterations of those three calls, and a rollout cut in two, with tick0 advanced and
 * last_light carried, resumes bit for bit.  cause_ticks [A][3] counts the EMERGENCY ticks by light, walker and vehicle;
 * min_walker_gap [A] is the smallest walker_distance seen (ignored walkers too), +inf if none; log_cause is laid out as log_mode.
 *   emp_agent_behave_hazards uses: last_light, last_light_out (may alias), cause, light_hit, walker_hit, walker_distance; optional
 *     n_light / light / light_lane / light_cycle (all four, or max_light == 0), n_walker / walker / walker_lane (all three, or
 *     max_walker == 0).
 *   emp_traffic_rollout_hazards uses: last_light, last_light_out, cause_ticks, min_walker_gap; optional lights and walkers as
 *     above, log_cause.
 * Refused before any launch (EMP_ERR_INVALID): everything the counterpart refuses; max_light or max_walker outside
 * [0, EMP_HAZARD_MAX]; a NULL required pointer; reserved != 0.  W == 0: EMP_OK. */
#define EMP_HAZARD_MAX 64
#define EMP_HZ_NONE 0
#define EMP_HZ_LIGHT 1
#define EMP_HZ_WALKER 2
#define EMP_HZ_VEHICLE 3
typedef struct emp_hazard_params {
    double tlight_threshold;               /* 5 m (BasicAgent._base_tlight_threshold) */
    double tlight_up_angle;                /* 90 degrees */
    double walker_radius;                  /* 10 m */
    double walker_up_angle;                /* 60 degrees */
    int32_t reserved;                      /* must be 0 */
} emp_hazard_params;
void emp_hazard_params_default(emp_hazard_params* p);
typedef struct emp_hazard_io {
    const int32_t* n_light;                /* [W] */
    const double* light;                   /* [W][max_light][4] */
    const int32_t* light_lane;             /* [W][max_light] */
    const int32_t* light_cycle;            /* [W][max_light][3] */
    const int32_t* n_walker;               /* [W] */
    const double* walker;                  /* [W][max_walker][5] */
    const int32_t* walker_lane;            /* [W][max_walker] */
    const int32_t* last_light;             /* [A] */
    int32_t* last_light_out;               /* [A] */
    int32_t* cause;                        /* [A] (behave) */
    int32_t* light_hit;                    /* [A] (behave) */
    int32_t* walker_hit;                   /* [A] (behave) */
    double* walker_distance;               /* [A] (behave) */
    int32_t* cause_ticks;                  /* [A][3] (rollout) */
    double* min_walker_gap;                /* [A] (rollout) */
    int32_t* log_cause;                    /* optional log (rollout) */
    int32_t reserved;                      /* must be 0 */
} emp_hazard_io;
int emp_agent_behave_hazards(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, int32_t W, int32_t max_world,
                             int32_t max_path, int32_t max_other, int64_t tick0, const emp_behavior_io* io, emp_mem where,
                             const emp_hazard_params* hp, int32_t max_light, int32_t max_walker, const emp_hazard_io* hio);
int emp_traffic_rollout_hazards(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp,
                                int32_t W, int32_t max_world, int32_t max_path, int32_t max_other, int32_t T, int32_t log_every,
                                int64_t tick0, const emp_behavior_io* io, emp_mem where, const emp_hazard_params* hp, int32_t max_light,
                                int32_t max_walker, const emp_hazard_io* hio);

/* ---- one world for a planning fleet and reacting traffic (new with ABI 13's library; EMP_ABI_VERSION is unchanged) ---------------
 * The reference has no counterpart: CARLA's world tick couples its vehicles.  Here the two fleets of the sections above - the egos
 * of emp_drive_timed and the agents of emp_traffic_rollout_hazards - are put in W worlds, and K periods of both run in ONE call.
 * Nothing above changes: emp_traffic_rollout and emp_traffic_rollout_hazards are emp_traffic_rollout_epoch with other_tick0 = 0.
 *
 * WORLDS.  World w holds the agents of slots [w * max_world, w * max_world + n_world[w]) (as above) and the egos
 * b in [ego_off[w], ego_off[w + 1]): ego_off [W + 1] int32, non-decreasing, inside [0, B].  EMP_HOST offsets that are not are
 * refused; EMP_DEVICE offsets are clamped in the kernel (e0 = clamp(ego_off[w], 0, B), e1 = clamp(ego_off[w + 1], e0, B); no world:
 * b < clamp(ego_off[0]) or b >= clamp(ego_off[W])), which keeps every access inside the arrays and promises nothing else.  An ego in
 * no world sees nothing, and nobody sees it.
 *
 * emp_world_exchange: who sees whom, from the states of both fleets (one kernel, one 64-lane block per world).
 *   actors [B][max_act][4], n_act [B]: for ego b of world w the rows emp_agent_observe gives for the world's live agents, in slot
 *     order; with see_egos == 1 the world's other egos follow in index order, without b itself.  The rows come from the device
 *     function emp_agent_observe uses: they equal its output BIT FOR BIT.  n_act = min(rows, max_act); rows past max_act are dropped
 *     and EMP_WX_ACT_TRUNCATED is set; slots at and past n_act are written as 0.  An ego in no world: n_act 0, all rows 0,
 *     EMP_WX_NO_WORLD.
 *   other [W][max_other][5], other_lane [W][max_other], n_other [W]: emp_behavior_io's others of world w - for its egos in index
 *     order the ego's observe row and ego_extent[b], and the lane key it shows.  n_other = min(egos, max_other); an ego past
 *     max_other is not listed and EMP_WX_NOT_LISTED is set on it; slots at and past n_other are written as 0 with key -1.
 *     max_other == 0: the three arrays are not touched (they may be NULL) and every ego of a world is EMP_WX_NOT_LISTED.
 *   wx_status [B]: the OR of the EMP_WX_* bits.
 * THE LANE KEY an ego shows is a windowed nearest match on its global path: n = n_global[b] clamped to [0, max_global];
 * lo = clamp(pre_match_index[b], 0, n - 1), hi = min(lo + lane_window, n - 1); d2_i = (dx * dx) + (dy * dy) with
 * (dx, dy) = (global_path[b][i] x - x_b, ... y - y_b), every operation rounded on its own; i* = the LOWEST index with the smallest
 * d2 in [lo, hi]; a NaN d2 never wins, and if all are NaN i* = lo.  The key is ego_lane[b][i*] (ego_lane [B][max_global] int32:
 * the lane key of each global waypoint); n == 0: -1.
 * Refused (EMP_ERR_INVALID) before any launch: a NULL required pointer (everything but other / other_lane / n_other with
 * max_other == 0); W < 0, B < 0, max_global < 1, max_world outside [1, EMP_TRAFFIC_MAX_WORLD], max_act outside [1, 64], max_other
 * outside [0, 64], lane_window < 0, see_egos not 0 or 1; reserved != 0; EMP_HOST_PINNED; bad EMP_HOST offsets.  W == 0 or B == 0:
 * EMP_OK, nothing is written.
 *
 * emp_traffic_rollout_epoch: emp_traffic_rollout_hazards with one more argument, other_tick0.  At tick index k = tick0 + t an
 * other stands at x + vx * ((double)(k - other_tick0) * dt) (the subtraction in int64): `other` holds the rows as they were at
 * tick other_tick0.  Lights and walkers stay on k.  Everything else is that call, from the same kernel; other_tick0 == 0 IS that
 * call, bit for bit.  Refused beyond what it refuses: other_tick0 < 0 or other_tick0 > tick0.
 *
 * emp_world_drive: K periods on emp_stream(), stream-ordered, without a host synchronisation or a copy to the host between them.
 * Period k, with tick_k = tick0 + k * T (emp_drive_timed's clock) and a_k = atick0 + k * Ta (int64, the agents' clock):
 *   1. emp_world_exchange on the egos' and the agents' states, with the pre_match_index the period starts from
 *   2. the period of emp_drive_timed (its steps 1-5, the same code) on the exchanged actors and n_act at tick_k
 *   3. emp_traffic_rollout_epoch: Ta ticks at tick0 = a_k with the exchanged others, other_tick0 = a_k, log_every = Ta
 * 2 and 3 both read the snapshot of 1: inside a period each fleet sees the other move straight, the rule both calls have.
 * EVERY OUTPUT AND LOG EQUALS, BIT FOR BIT, K iterations of the three public calls and the adopt rule on the same arrays, and a
 * call cut in two resumes bit for bit with tick0 advanced by k * T and atick0 by k * Ta.
 * emp_world_io holds
 *   the egos: emp_drive_timed_io's fields without actors and n_act (actors_out stays: the last period's exchanged rows, advanced
 *     as emp_drive_request_timed leaves them), and the exchange's ego_off, ego_extent, ego_lane;
 *   the traffic: agents (emp_behavior_io) and hazards (emp_hazard_io) exactly as emp_traffic_rollout_hazards takes them - state in
 *     and out, last_light included, each output possibly the memory of its input - but for n_other / other / other_lane, which are
 *     not read (the exchange makes them), and the five log_* arrays of emp_behavior_io and log_cause, which must be NULL.  status,
 *     done_tick, mode_ticks, min_gap, actors_out, cause_ticks, min_walker_gap come back as the LAST period's;
 *   per-period logs, NULL to skip, each row that period's call output: log_wx_status [K][B], log_n_act [K][B], log_agent_state
 *     [K][A][6] (the state at the period's start), log_agent_status [K][A], log_done_tick [K][A], log_mode_ticks [K][A][5],
 *     log_cause_ticks [K][A][3], log_min_gap [K][A], log_min_walker_gap [K][A], A = W * max_world.  A log row is a copy of the
 *     call's output array, padding slots included.
 * Everything runs on the one stream: no second stream, no graph capture.  Refused before any launch: what the three calls refuse;
 * the agents' clock (Ta < 1, atick0 < 0, atick0 + K * Ta > INT32_MAX); periods of different length,
 * |T * vp->dt - Ta * agent_params->dt| > 1e-9.  B == 0 or W == 0: EMP_OK, nothing runs. */
#define EMP_WX_ACT_TRUNCATED 1
#define EMP_WX_NOT_LISTED 2
#define EMP_WX_NO_WORLD 4
typedef struct emp_world_exchange_io {
    const int32_t* n_world;                /* [W] */
    const double* agent_state;             /* [W * max_world][6] */
    const int32_t* ego_off;                /* [W + 1] */
    const double* ego_state;               /* [B][6] */
    const double* ego_extent;              /* [B] */
    const double* global_path;             /* [B][max_global][4] */
    const int32_t* n_global;               /* [B] */
    const int32_t* ego_lane;               /* [B][max_global] */
    const int32_t* pre_match_index;        /* [B] */
    double* actors;                        /* [B][max_act][4] */
    int32_t* n_act;                        /* [B] */
    double* other;                         /* [W][max_other][5] */
    int32_t* other_lane;                   /* [W][max_other] */
    int32_t* n_other;                      /* [W] */
    int32_t* wx_status;                    /* [B] */
    int32_t reserved;                      /* must be 0 */
} emp_world_exchange_io;
int emp_world_exchange(emp_ctx* ctx, int32_t W, int32_t max_world, int32_t B, int32_t max_global, int32_t max_act, int32_t max_other,
                       int32_t lane_window, int32_t see_egos, const emp_world_exchange_io* io, emp_mem where);
int emp_traffic_rollout_epoch(emp_ctx* ctx, const emp_agent_params* p, const emp_behavior_params* bp, const emp_vehicle_params* vp,
                              int32_t W, int32_t max_world, int32_t max_path, int32_t max_other, int32_t T, int32_t log_every,
                              int64_t tick0, const emp_behavior_io* io, emp_mem where, const emp_hazard_params* hp, int32_t max_light,
                              int32_t max_walker, const emp_hazard_io* hio, int64_t other_tick0);

typedef struct emp_world_params {
    int32_t W, max_world, max_path, max_other, max_light, max_walker;      /* the traffic's sizes */
    int32_t Ta;                            /* agent ticks per period */
    int32_t lane_window;                   /* 50 */
    int32_t see_egos;                      /* 0 or 1 */
    int32_t reserved;                      /* must be 0 */
    int64_t atick0;                        /* the agents' tick index at the call's first period */
} emp_world_params;
void emp_world_params_default(emp_world_params* p);
typedef struct emp_world_io {
    /* the egos: emp_drive_timed_io's inputs without actors and n_act */
    const double* global_path;
    const int32_t* n_global;
    const double* state;
    const double* accel;
    const int32_t* pre_match_index;
    const double* track;
    const int32_t* track_len;
    const int32_t* held;
    const double* t0;
    const double* profile;
    const int32_t* cursor;
    const int32_t* speed_held;
    /* ... and the exchange's */
    const int32_t* ego_off;                /* [W + 1] */
    const double* ego_extent;              /* [B] */
    const int32_t* ego_lane;               /* [B][max_global] */
    /* the egos' outputs (required; each may alias the input of its name) */
    double* state_out;
    double* accel_out;
    double* actors_out;                    /* [B][max_act][4] */
    int32_t* pre_match_index_out;
    double* track_out;
    int32_t* track_len_out;
    int32_t* held_out;
    double* profile_out;
    int32_t* cursor_out;
    int32_t* speed_held_out;
    /* the egos' per-period logs, NULL to skip: emp_drive_timed_io's */
    double* log_state;
    int32_t* log_plan_status;
    int32_t* log_roll_status;
    int32_t* log_held;
    int32_t* log_counts;
    double* log_traj;
    int32_t* log_traj_len;
    int32_t* log_speed_status;
    int32_t* log_speed_held;
    int32_t* log_tgt_status;
    int32_t* log_cursor;
    double* log_profile;
    /* the traffic, as emp_traffic_rollout_hazards takes it */
    const emp_behavior_io* agents;
    const emp_hazard_io* hazards;
    /* the world's per-period logs, NULL to skip */
    int32_t* log_wx_status;                /* [K][B] */
    int32_t* log_n_act;                    /* [K][B] */
    double* log_agent_state;               /* [K][A][6] */
    int32_t* log_agent_status;             /* [K][A] */
    int32_t* log_done_tick;                /* [K][A] */
    int32_t* log_mode_ticks;               /* [K][A][5] */
    int32_t* log_cause_ticks;              /* [K][A][3] */
    double* log_min_gap;                   /* [K][A] */
    double* log_min_walker_gap;            /* [K][A] */
    int32_t reserved;                      /* must be 0 */
} emp_world_io;
int emp_world_drive(emp_ctx* ctx, const emp_dp_params* dp, const emp_qp_params* qp, const emp_smooth_params* smooth,
                    const emp_speed_dp_params* sdp, const emp_speed_qp_params* sqp, const emp_drive_params* drive_params,
                    const emp_drive_timed_params* timed_params, int32_t lateral, const emp_mpc_params* lat, const emp_pid_params* pid,
                    const emp_vehicle_params* vp, const emp_agent_params* agent_params, const emp_behavior_params* behavior_params,
                    const emp_vehicle_params* agent_vp, const emp_hazard_params* hazard_params, const emp_world_params* world,
                    int32_t B, int32_t max_global, int32_t max_obs, int32_t max_pts, int32_t max_act, int32_t max_dyn, int32_t K,
                    int32_t T, int32_t tick0, const double* target_speed, const emp_world_io* io, emp_mem where);

#ifdef __cplusplus
}
#endif
#endif /* EMPLANNER_H */
