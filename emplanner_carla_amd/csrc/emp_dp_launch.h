// emp_dp_launch.h - what host and device agree on about the lattice-DP kernels, and the launch geometry of those kernels
// as pure host arithmetic: no HIP types, readable by a plain C++17 compiler (tests/host_check runs every plan_* on the CPU;
// tests/golden/dp_launch_plans.npz pins their results).  emp_dp_kernels.h includes it; emp_api.hip's launchers call it.
//
// Every number the plan_* functions produce was tuned on the GPU (the comments quote the step times).  The kernels are
// bit-identical for any geometry, so a slip here shows only as a slower step or a refused launch: change it with the
// golden table in hand.
#pragma once

#include <stddef.h>

#include <algorithm>

#include "emp_core.h"

namespace emp {

struct DpDev {
    int row, col;
    int S;       // scenes per wavefront tile = 64 / row
    int tiles;   // ceil(B / S)
    int B;
    int max_obs;
    double sample_s, sample_l, res;
    double w_coll, w0, w1, w2, w_ref;
};

// Pair-table fields behind the kSamples lateral samples (round 5: the three quintic coefficients gave way to ONE jerk
// weight - see kF_JERK - which takes the table from 17 to 15 fields: 53 instead of 60 KB of LDS at 21 rows)
constexpr int kF_JERK = kSamples + 0;     // w2 (h h), h = l_cur - l_pre: the quirked jerk term of the edge is this times F(s0)
constexpr int kF_BASE = kSamples + 1;     // w0 sum dl^2 + w1 sum ddl^2
constexpr int kF_REF = kSamples + 2;      // w_ref sum l^2
constexpr int kF_LLO = kSamples + 3;      // min(l_pre, l_cur)
constexpr int kF_LHI = kSamples + 4;      // max(l_pre, l_cur)
constexpr int kTableFields = kSamples + 5;
// behind the fields: the kSamples sample offsets t_n, their two moments (emp_core.h sample_moments) and the UNIT quintic's
// a3, a4, a5 (the coefficients of the neighbour edge with h = 1)
constexpr int kUnitQuintic = 3;
constexpr int kTableTail = kSamples + kSampleMoments + kUnitQuintic;

// Capacity: a ring never holds more than 63 left-over + 64 pushed entries = 127 < kRingSlots.
constexpr int kRingSlots = 128;

// Per wavefront, in LDS: code[2][kRingSlots] (32 bits an entry: column j << 17 | source row k << 12 | obstacle m << 6 | owner
// lane - the one-obstacle ring's entry IS its obstacle, it has no mask) and, for the several-obstacle ring only, one mask per
// slot as wide as the scene's obstacle count needs (1, 2, 4 or 8 bytes: ascending bit = ascending m).  The edge's smoothness
// term is recomputed by the lane that pops the entry.  LDS is what decides how many edge blocks sit beside the previous batch's
// path-QP wavefronts in the staged step (allocated in 1280-byte granules, 128 a CU): the 40 x 9 lattice's two-wavefront block
// is 14.4 KB = 12 granules, six of them fit beside two path-QP wavefronts (profiles/r05_edge/README.md 8).
EMP_HD constexpr int edge_ring_mask_bytes(int max_obs) { return max_obs <= 8 ? 1 : max_obs <= 16 ? 2 : max_obs <= 32 ? 4 : 8; }
EMP_HD constexpr int edge_ring_bytes(int max_obs) { return 2 * kRingSlots * 4 + kRingSlots * edge_ring_mask_bytes(max_obs); }
// the code's fields: 32 rows (5 bits of k), 64 obstacles, 64 lanes, columns below 2^15
constexpr int kRingMaxCol = 32767;

constexpr int kMaxTiledRow = 32;       // the tiled kernels (scenes packed into wavefronts, pair table in LDS) up to here
constexpr int kMaxWideRow = 1024;      // (round 5: predecessors of the wide sweep are 16-bit; until round 4 a byte, 256 rows.  The pair
                                       // table is 15 row^2 doubles - 126 MB at 1024 rows - and the tensor (col - 1) row^2 doubles per scene)

// ---- layouts ------------------------------------------------------------------------------------------------------------
// The dynamic LDS of every DP kernel, as in emp_tail_launch.h: a struct of positions, and ONE function that walks the arrays in
// order from `at`.  The position type P is the kernel's own pointer on the device - the function then IS the kernel's carve-up -
// and a plain count from 0 on the host (LdsCount), where `end` is the total the launch asks for: one sum, not two.  The
// layouts of doubles alone count DOUBLES (edge_lds, sweep_lds - 64 predecessor bytes a column are 8 - and sweep_wide_lds); those
// that also hold bytes or 32-bit words count BYTES, as emp_tail_launch.h's SpeedDpLds does (edge_ring_lds: the rings;
// enrich_lds: col * row predecessor bytes; fused_lds: predecessor bytes and counters).  What varies per wavefront is an
// argument (`waves`, `cpw`, `wpb`); a wavefront's own share of such an array is index arithmetic from its base, in the kernel.
using LdsCount = size_t;

// the lockstep kernel's box terms per scene: one per obstacle slot inside the kernel's reach mask (MASK: 32 or 64 bits)
EMP_HD constexpr int edge_box_width(int max_obs, int mask_bits) { return max_obs < mask_bits ? max_obs : mask_bits; }

template <class P>
struct EdgeLds {         // dp_edge_kernel
    P tab;               // [kTableFields][row^2], pair index = k * row + i
    P obs_s, obs_l;      // [S][max_obs] each
    P smp;               // [kTableTail] sample offsets t_n, sum t_n, sum t_n^2, unit quintic
    P box;               // [waves][S][edge_box_width] longitudinal box terms of the column a wavefront works on.  Keep it the LAST
                         // array: dp_edge_kernel asks for the layout of ONE wavefront (see there), right for everything up to `box`
    P end;
};
template <class P>
EMP_HD EdgeLds<P> edge_lds(P at, int row, int S, int max_obs, int mask_bits, int waves) {
    EdgeLds<P> L;
    L.tab = at;   at += kTableFields * row * row;
    L.obs_s = at; at += S * max_obs;
    L.obs_l = at; at += S * max_obs;
    L.smp = at;   at += kTableTail;
    L.box = at;   at += (size_t)waves * S * edge_box_width(max_obs, mask_bits);
    L.end = at;
    return L;
}

template <class P>
struct EdgeRingLds {     // dp_edge_ring_kernel, in BYTES
    P tab;               // [kTableFields][row^2] doubles
    P obs_s, obs_l;      // [S][max_obs] doubles each
    P ps;                // [S rounded up to even] doubles: plan_start_s of the tile's scenes
    P band;              // [waves][S][max_obs][2] doubles: lateral reach band (lo, hi) of each obstacle in the wavefront's column
    P rings;             // [waves] of edge_ring_bytes(max_obs) bytes: code [2][kRingSlots], then a mask per slot
    P f;                 // [waves][cpw][S] doubles: the jerk factor F of each of a wavefront's cpw columns
    P end;
};
template <class P>
EMP_HD EdgeRingLds<P> edge_ring_lds(P at, int row, int S, int max_obs, int waves, int cpw) {
    EdgeRingLds<P> L;
    L.tab = at;   at += kTableFields * row * row * 8;
    L.obs_s = at; at += S * max_obs * 8;
    L.obs_l = at; at += S * max_obs * 8;
    L.ps = at;    at += ((S + 1) & ~1) * 8;
    L.band = at;  at += (size_t)waves * 2 * S * max_obs * 8;
    L.rings = at; at += (size_t)waves * edge_ring_bytes(max_obs);
    L.f = at;     at += (size_t)waves * cpw * S * 8;
    L.end = at;
    return L;
}

template <class P>
struct SweepLds {        // dp_sweep_kernel<ROW, PD, WPB, ., .>
    P front;             // [wpb][64] the cost front of the previous column
    P pre;               // [wpb][col][64] predecessor BYTES: 8 doubles a column
    P end;
};
template <class P>
EMP_HD SweepLds<P> sweep_lds(P at, int wpb, int col) {
    SweepLds<P> L;
    L.front = at; at += wpb * 64;
    L.pre = at;   at += (size_t)wpb * col * 8;
    L.end = at;
    return L;
}

template <class P>
struct SweepWideLds {    // dp_sweep_wide_kernel: the cost front of the previous column and the one being built, [row] each
    P cur, nxt, end;
};
template <class P>
EMP_HD SweepWideLds<P> sweep_wide_lds(P at, int row) {
    return {at, at + row, at + row + row};
}

template <class P>
struct EnrichLds {       // dp_enrich_wave_kernel, in BYTES (P: a byte pointer, or a count of bytes)
    P rows;              // [col] doubles: the scene's rows
    P bt;                // [col][row] predecessor bytes, where the kernel does the backtrack (with_pre)
    P end;
};
template <class P>
EMP_HD EnrichLds<P> enrich_lds(P at, int row, int col, bool with_pre) {
    EnrichLds<P> L;
    L.rows = at; at += (size_t)col * 8;
    L.bt = at;   at += with_pre ? (size_t)col * row : 0;
    L.end = at;
    return L;
}

template <class P>
struct FusedLds {        // dp_fused_kernel, in BYTES
    P tab;               // [kTableFields][row^2] doubles
    P smp;               // [kTableTail] doubles
    P obs_s, obs_l;      // [S][max_obs] doubles each
    P buf;               // [2][nc][row][64] doubles: the edge costs of two column chunks
    P front;             // [64] doubles: cost front of the previous column
    P pre;               // [col][64] predecessor bytes
    P ctr;               // [2] 32-bit column counters, one per buffer
    P end;
};
template <class P>
EMP_HD FusedLds<P> fused_lds(P at, int row, int col, int S, int max_obs, int nc) {
    FusedLds<P> L;
    L.tab = at;   at += kTableFields * row * row * 8;
    L.smp = at;   at += kTableTail * 8;
    L.obs_s = at; at += S * max_obs * 8;
    L.obs_l = at; at += S * max_obs * 8;
    L.buf = at;   at += 2 * nc * row * 64 * 8;
    L.front = at; at += 64 * 8;
    L.pre = at;   at += col * 64;
    L.ctr = at;   at += 2 * 4;
    L.end = at;
    return L;
}

// ---- tiling -------------------------------------------------------------------------------------------------------------
struct DpTiling {
    int S, tiles;
};
inline DpTiling dp_tiling(int row, int B) {
    const int S = row <= kMaxTiledRow ? 64 / row : 1;      // wider lattices: one scene per block, canonical edge tensor
    return {S, (int)(((long long)B + S - 1) / S)};
}
inline bool dp_wide(const DpDev& d) { return d.row > kMaxTiledRow; }
// elements of the edge tensor the DP kernels exchange: tiled up to 32 rows, canonical [B][col-1][row][row] beyond (and
// wherever the caller asks for the canonical layout)
inline size_t edge_tensor_elems(int row, int col, int B, bool tiled) {
    if (!tiled || row > kMaxTiledRow) return (size_t)B * (size_t)(col - 1) * row * row;
    return (size_t)dp_tiling(row, B).tiles * (size_t)(col - 1) * row * 64;
}
// the benchmark lattices' row counts are compiled in (emp_dp_kernels.h: dp_edge_column<ROW>, dp_sweep_kernel<ROW>,
// dp_fused_kernel<ROW>); any other takes the generic instantiation 0 - the same operations either way
inline int dp_row_inst(int row) { return row == 5 || row == 9 || row == 12 || row == 21 ? row : 0; }

constexpr size_t kLdsBytes = 160 * 1024;                 // LDS of a compute unit, and the most one block may ask for
constexpr size_t kInfinityCacheBytes = (size_t)256 << 20;

// ---- edge costs ---------------------------------------------------------------------------------------------------------
struct EdgePlan {
    bool wide = false;          // dp_edge_wide_kernel: everything below but the grid and the block is unused
    bool ring = false;          // dp_edge_ring_kernel, else dp_edge_kernel
    bool m32 = false;           // every obstacle of a row fits a 32-bit reach mask
    int row_inst = 0;           // the kernels' ROW argument: 0, 5, 9, 12 or 21
    int wpb = 0;                // wavefronts per block
    int cols_per_chunk = 0;     // columns one block takes: the kernels' argument
    int grid_x = 0, grid_y = 0, block = 0;
    size_t lds = 0;             // dynamic LDS bytes
    const char* error = nullptr;
};

// opt_edge_form, opt_edge_block: the context's EMP_OPT_EDGE_FORM and EMP_OPT_EDGE_BLOCK; lds_pad: development, extra (unused)
// dynamic LDS per block
static inline EdgePlan plan_edge(const DpDev& d, bool tiled, int opt_edge_form, int opt_edge_block, size_t lds_pad) {
    EdgePlan p;
    if (dp_wide(d)) {          // more than 32 rows: generic kernel, canonical tensor whatever `tiled` says (emp_dp_kernels.h)
        p.wide = true;
        if (!(d.B <= 0x7fffffff && d.col - 1 <= 65535)) p.error = "batch or lattice too large for the wide-row edge kernel's grid";
        p.grid_x = d.B;
        p.grid_y = d.col > 1 ? d.col - 1 : 1;
        p.block = std::min(((d.row + 63) / 64) * 64, 256);
        p.wpb = p.block / 64;
        p.cols_per_chunk = 1;
        return p;
    }
    // per block: pair table, the tile's obstacles, sample offsets; per wavefront: the longitudinal box terms of its column
    // ([S][mask width] doubles, emp_dp_kernels.h: box_dx2)
    // EMP_OPT_EDGE_FORM: 0 (default) the work-ring kernel (emp_dp_kernels.h dp_edge_ring_kernel: edges with obstacles in reach are
    // queued per wavefront and scanned one entry per lane), 1 the lockstep kernel of rounds 1-4 - bit-identical tensors.  The ring
    // form needs every obstacle of a row inside one 64-bit mask and the column index inside 15 bits; anything else is lockstep.
    const bool ring = opt_edge_form == 0 && d.max_obs <= 64 && d.col <= kRingMaxCol;
    p.ring = ring;
    p.m32 = d.max_obs <= 32;
    p.row_inst = dp_row_inst(d.row);
    // the LDS of a block of w wavefronts: the kernel's own layout.  (cpw, ring form only: the columns a wavefront takes, which
    // follow from the block size - the rules that choose the block size price kEdgeRingMaxCpw, the most a wavefront is ever given)
    constexpr int kEdgeRingMaxCpw = 4;
    const auto lds_of = [&](int w, int cpw) {
        return (ring ? edge_ring_lds(LdsCount(0), d.row, d.S, d.max_obs, w, cpw).end
                     : edge_lds(LdsCount(0), d.row, d.S, d.max_obs, p.m32 ? 32 : 64, w).end * sizeof(double)) + lds_pad;
    };
    size_t lds = lds_of(2, kEdgeRingMaxCpw);      // the block-size rule below prices a two-wavefront block; the launch its own
    if (lds > kLdsBytes) {
        p.error = "lattice too wide for the LDS pair table";
        return p;
    }
    int ncol = d.col - 1;
    int chunks = 1;
    // Block size: as many wavefronts per block as it takes to fill a CU's twenty wavefront slots (five per SIMD) with the
    // blocks its LDS holds - and no more, because a block needs a free slot on as many SIMDs as it has wavefronts at the same
    // moment: beside the previous batch's path-QP wavefronts (staged pipeline) a two-wavefront block of the 40 x 9 lattice
    // (12 KB of LDS: 13 blocks per CU) finds room where a four-wavefront block does not (step 0.322 -> 0.289 ms), while the
    // 120 x 21 lattice's 60 KB table allows two blocks per CU, which therefore carry ten wavefronts each.
    // EMP_OPT_EDGE_BLOCK (emp_set_option) overrides it.
    int wpb = 4;
    if (!ring) {
        const int blocks_per_cu = (int)(kLdsBytes / (lds > 0 ? lds : 1));
        wpb = (20 + blocks_per_cu - 1) / (blocks_per_cu > 0 ? blocks_per_cu : 1);
        if (wpb < 2) wpb = 2;
        if (wpb > 16) wpb = 16;
    } else {
        // the ring form's wavefronts carry ~3 KB of LDS each: the smallest block that puts sixteen wavefronts on a CU (or as many
        // as the LDS allows).  Small blocks matter in the staged step, where a block must find all its slots free at once beside
        // the previous batch's path-QP wavefronts: at 40 x 9 two-wavefront blocks give 0.241 ms per step, three 0.258, four 0.266,
        // eight 0.293 - although ALONE the kernel is fastest with four (profiles/r05_edge/README.md)
        // (LDS is allocated in 1280-byte granules, 128 of them a CU)
        auto blocks_per_cu = [](size_t l) { return (size_t)128 / ((l + 1279) / 1280); };
        int best = 0;
        for (int w = 2; w <= 16; ++w) {
            const size_t l = lds_of(w, kEdgeRingMaxCpw);
            if (l > kLdsBytes) break;
            best = std::max(best, (int)std::min<size_t>(blocks_per_cu(l) * w, 20));
        }
        for (int w = 2; w <= 16; ++w) {
            const size_t l = lds_of(w, kEdgeRingMaxCpw);
            if (l > kLdsBytes) break;
            if ((int)std::min<size_t>(blocks_per_cu(l) * w, 20) >= std::min(best, 16)) {
                wpb = w;
                break;
            }
        }
    }
    // (a tensor beyond the 256 MiB Infinity Cache - 32768 scenes of the 40 x 9 lattice - keeps four wavefronts per block: the
    // faster front stage otherwise leaves the sweep, which then streams from DRAM for 150 us, beside the previous batch's
    // path QP: 0.75 of the roofline against 0.61)
    if (tiled && edge_tensor_elems(d.row, d.col, d.B, true) * sizeof(double) > kInfinityCacheBytes && wpb < 4) wpb = 4;
    if (opt_edge_block) wpb = opt_edge_block / 64;
    // (the rule above prices a two-wavefront block; a wide table with wide obstacle rows - 32 rows, 254+ obstacle slots: one block
    // of sixteen wavefronts per CU - may not hold sixteen per-wavefront scratch areas: fewer wavefronts, not a refusal)
    while (wpb > 1 && lds_of(wpb, kEdgeRingMaxCpw) > kLdsBytes) --wpb;
    lds = lds_of(wpb, kEdgeRingMaxCpw);
    if (lds > kLdsBytes) {
        p.error = "edge-cost block too large for the LDS";
        return p;
    }
    // each of the block's wavefronts takes whole columns: two per wavefront, or one while that leaves the chip short of blocks
    // (a single scene: 29 us with one column per wavefront, 44 with two); chunk sizes multiples of the wavefront count
    if (ncol > 0) {
        int cpw = ((long long)d.tiles * ((ncol + 2 * wpb - 1) / (2 * wpb)) >= 1024) ? 2 : 1;
        // (ring form: a wavefront drains its rings once, at the end of its columns - four columns per wavefront while that
        // still leaves several thousand blocks: 120 x 21 at 4096 scenes 2.18 -> 2.01 ms)
        if (ring && (long long)d.tiles * ((ncol + 4 * wpb - 1) / (4 * wpb)) >= 4096) cpw = 4;
        chunks = (ncol + cpw * wpb - 1) / (cpw * wpb);
        if (chunks < 1) chunks = 1;
    }
    int cols_per_chunk = ncol > 0 ? (ncol + chunks - 1) / chunks : 1;
    cols_per_chunk = cols_per_chunk >= wpb ? (cols_per_chunk / wpb) * wpb : wpb;
    chunks = ncol > 0 ? (ncol + cols_per_chunk - 1) / cols_per_chunk : 1;
    // the launch's LDS: the ring form's jerk-factor table holds the columns a wavefront really takes, as the kernel counts them
    lds = lds_of(wpb, (cols_per_chunk + wpb - 1) / wpb);
    if (lds > kLdsBytes) {
        p.error = "edge-cost block too large for the LDS";
        return p;
    }
    p.wpb = wpb;
    p.cols_per_chunk = cols_per_chunk;
    p.grid_x = d.tiles;
    p.grid_y = chunks;
    p.block = wpb * 64;
    p.lds = lds;
    return p;
}

// ---- min-plus sweep -----------------------------------------------------------------------------------------------------
struct SweepPlan {
    int row_inst = 0;           // dp_sweep_kernel's ROW: 0, 5, 9, 12 or 21 (0 too for dp_sweep_wide_kernel, beyond 32 rows)
    int pd = 0;                 // its ring depth PD: columns in flight per wavefront
    bool nt = false;            // nontemporal loads of the edge tensor
    int grid = 0, block = 0;
    size_t lds = 0;
    const char* error = nullptr;
};

static inline SweepPlan plan_sweep(const DpDev& d) {
    SweepPlan p;
    if (dp_wide(d)) {          // more than 32 rows: one block per scene, predecessors in device memory
        p.grid = d.B;
        p.block = std::min(((d.row + 63) / 64) * 64, 256);
        p.lds = sweep_wide_lds(LdsCount(0), d.row).end * sizeof(double);
        return p;
    }
    // Ring depth PD (columns in flight per wavefront), measured at 4096 scenes: 2 is best for rows 5..12 (row 9:
    // 20.4 us against 23.2 at PD = 8, 21.4 at PD = 1), 3 for the 21-row lattice; nontemporal loads change nothing.
    // Load policy, measured on the 40x9 lattice (sweep alone, TB/s of algorithmic bytes; plain / nontemporal): 4096 scenes
    // (105 MB tensor) 5.45 / 4.74, 8192 (226 MB) 6.47 / 6.21, 12288 (331 MB) 5.04 / 6.45, 16384 4.47 / 6.40, 32768 (883 MB)
    // 4.52 / 6.03.  A tensor that fits the 256 MiB Infinity Cache is still there when the sweep follows the edge kernel
    // that wrote it, and plain loads hit it; a larger one streams from HBM, where plain loads also drag every line through
    // the cache hierarchy they will never hit again: nontemporal from 256 MiB on (compiled row counts only).
    p.row_inst = dp_row_inst(d.row);
    p.nt = p.row_inst != 0 && edge_tensor_elems(d.row, d.col, d.B, true) * sizeof(double) > kInfinityCacheBytes;
    switch (p.row_inst) {
        case 5: p.pd = 2; break;
        case 9:
            // (round 5: three columns in flight instead of two.  Alone the two are within noise of each other - 0.72-0.77 of the
            // peak either way; beside the previous batch's Cartesian tail, where the sweep runs since EMP_OPT_SWEEP_EXCLUSIVE
            // defaults to 0, the deeper ring holds 0.67-0.68 where the shallow one holds 0.65: six A/B pairs, tools/step_ab.sh)
            // (ring depths 4 and 8 and the other load policy were option values until round 6: HISTORY.md 3.2 has their numbers)
            p.pd = p.nt ? 2 : 3;         // from DRAM (32768 scenes) the shallow ring keeps 0.697 against 0.692
            break;
        case 12: p.pd = 2; break;
        case 21: p.pd = 3; break;
        default: p.pd = 1; break;
    }
    p.grid = d.tiles;          // one wavefront a block
    p.block = 64;
    p.lds = sweep_lds(LdsCount(0), 1, d.col).end * sizeof(double);      // WPB = 1: the front [64], the predecessor bytes [col][64]
    if (p.lds > kLdsBytes) p.error = "too many columns for the predecessor table in LDS";
    return p;
}

// ---- EMP_DP_FUSED and the densification ---------------------------------------------------------------------------------
struct FusedPlan {
    int nc = 0;                 // columns per chunk: the kernel's argument
    size_t lds = 0;
    const char* error = nullptr;
};

static inline FusedPlan plan_fused(const DpDev& d) {
    FusedPlan p;
    // columns per chunk: 4 (one per wavefront) while two buffers of them leave room for three blocks per CU, fewer on wide
    // lattices whose pair table fills the LDS
    p.nc = 4;
    const auto lds_of = [&](int nc) { return fused_lds(LdsCount(0), d.row, d.col, d.S, d.max_obs, nc).end; };      // (bytes)
    while (p.nc > 1 && lds_of(p.nc) > 53 * 1024) p.nc /= 2;
    p.lds = lds_of(p.nc);
    if (p.lds > kLdsBytes) p.error = "lattice too wide for the fused DP kernel's LDS working set";
    return p;
}

struct EnrichPlan {
    size_t lds = 0;
    const char* error = nullptr;
};

static inline EnrichPlan plan_enrich(const DpDev& d, bool with_pre) {
    EnrichPlan p;
    p.lds = enrich_lds(LdsCount(0), d.row, d.col, with_pre).end;      // (bytes)
    if (p.lds > kLdsBytes) p.error = "too many columns for the densification kernel's predecessor table in LDS";
    return p;
}

// ---- the fleet loop's wave-per-vehicle kernels (emp_drive_kernels.h: drive_request_kernel, drive_adopt_kernel) --------------
struct DriveRequestPlan {
    int wpb = 0;                // wavefronts (vehicles) per block
    int grid = 0, block = 0;
    const char* error = nullptr;
};

// One wavefront per vehicle: a block per vehicle while the fleet is smaller than a wavefront's worth of vehicles (the few
// wavefronts spread over the compute units), four to a block from there on.  Not tuned: the kernels take microseconds either way.
static inline DriveRequestPlan plan_drive_request(int B) {
    DriveRequestPlan p;
    if (B < 0) {
        p.error = "negative batch";
        return p;
    }
    p.wpb = B >= 64 ? 4 : 1;
    p.block = 64 * p.wpb;
    p.grid = (int)(((long long)B + p.wpb - 1) / p.wpb);
    return p;
}

// The clock of emp_drive_timed (include/emplanner.h): period k starts at tick tick0 + k * T, a function of the tick number like
// emp_rollout_timed's own clock, so a run cut in two resumes bit for bit.  Refused: a negative tick0 and a last tick beyond int32.
struct DriveClockPlan {
    long long end = 0;          // tick0 + K * T: the first tick behind the call, the tick0 of a call that resumes it
    const char* error = nullptr;
    int tick0 = 0, T = 0;
    int tick(int k) const { return (int)((long long)tick0 + (long long)k * T); }
};

static inline DriveClockPlan plan_drive_clock(int tick0, int K, int T) {
    DriveClockPlan p;
    p.tick0 = tick0;
    p.T = T;
    if (K < 1 || T < 1) {
        p.error = "K and T must be at least 1";
        return p;
    }
    if (tick0 < 0) {
        p.error = "tick0 must be at least 0";
        return p;
    }
    p.end = (long long)tick0 + (long long)K * (long long)T;
    if (p.end > 2147483647ll) p.error = "tick0 + K * T must not exceed INT32_MAX";
    return p;
}

}  // namespace emp
