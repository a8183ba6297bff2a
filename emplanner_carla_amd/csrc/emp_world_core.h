// emp_world_core.h - who sees whom when a planning fleet and BehaviorAgent traffic share a world (emp_world_exchange), as plain
// functions that hipcc (emp_world_kernels.h) and g++ (tests/host_check/world_check.cpp) both compile, and the launch plan and
// argument rules of the three world calls as pure host arithmetic.  include/emplanner.h states the rule; tests/world_port.py is the
// same in NumPy.
//
// Nothing here does floating-point arithmetic but d2 below: (dx * dx) + (dy * dy), each operation rounded on its own
// (-ffp-contract=off).  An actor row comes from the caller's `rows` (the kernel: agt::observe, the very function emp_agent_observe
// calls; the host check: rows passed in as data), so libm plays no part in this file.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "emp_core.h"      // EMP_HD

namespace emp {
namespace wx {

constexpr int kActTruncated = 1;               // EMP_WX_ACT_TRUNCATED
constexpr int kNotListed = 2;                  // EMP_WX_NOT_LISTED
constexpr int kNoWorld = 4;                    // EMP_WX_NO_WORLD
constexpr int kMaxRows = 64;                   // max_act, max_other, max_world: a block's 64 lanes
constexpr int kNoIndex = 2147483647;           // a lane without a candidate in the window

struct Sizes {
    int W, B, max_world, max_global, max_act, max_other, lane_window, see_egos;
};
struct In {
    const int* n_world;            // [W]
    const int* ego_off;            // [W + 1]
    const double* ego_state;       // [B][6]
    const double* ego_extent;      // [B]
    const double* global_path;     // [B][max_global][4]
    const int* n_global;           // [B]
    const int* ego_lane;           // [B][max_global]
    const int* pre_match_index;    // [B]
};
struct Out {
    double* actors;                // [B][max_act][4]
    int* n_act;                    // [B]
    double* other;                 // [W][max_other][5] (null with max_other == 0)
    int* other_lane;               // [W][max_other]
    int* n_other;                  // [W]
    int* wx_status;                // [B]
};

EMP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The egos of world w: [e0, e1).  Offsets the host could not check (EMP_DEVICE) are clamped, so every index is inside [0, B].
struct Range {
    int e0, e1;
};
EMP_HD Range world_egos(const int* ego_off, int w, int B) {
    Range r;
    r.e0 = clampi(ego_off[w], 0, B);
    r.e1 = clampi(ego_off[w + 1], r.e0, B);
    return r;
}
// Non-decreasing offsets make the worlds' ranges one interval: ego b is in no world iff it lies outside [ego_off[0], ego_off[W]).
EMP_HD bool in_no_world(const int* ego_off, int W, int B, int b) { return b < clampi(ego_off[0], 0, B) || b >= clampi(ego_off[W], 0, B); }

// The order of the windowed nearest match on the pair (d2, index): a number comes before a NaN, the smaller d2 before the larger,
// the lower index on a tie (and among NaNs, so an all-NaN window gives its first index).
EMP_HD bool before(double da, int ia, double db, int ib) {
    const bool na = da != da, nb = db != db;
    if (na != nb) return nb;
    if (!na && da != db) return da < db;
    return ia < ib;
}

EMP_HD double d2(double px, double py, double x, double y) {
    const double dx = px - x, dy = py - y;
    return (dx * dx) + (dy * dy);
}

// The window [lo, hi] of ego b's match; n == 0: none.
struct Window {
    int n, lo, hi;
};
EMP_HD Window window(int n_global, int max_global, int pre_match_index, int lane_window) {
    Window w;
    w.n = clampi(n_global, 0, max_global);
    w.lo = w.hi = 0;
    if (w.n == 0) return w;
    w.lo = clampi(pre_match_index, 0, w.n - 1);
    w.hi = (w.n - 1 - w.lo < lane_window) ? w.n - 1 : w.lo + lane_window;
    return w;
}

// One lane's share of the window of ego b: the first of its indices (w.lo + lane, + kLanes, ...) in the order above, kNoIndex
// with a NaN where it has none.
EMP_HD void scan_window(const Sizes& z, const In& in, int b, const Window& w, int lane, int lanes, double* best, int* at) {
    const double x = in.ego_state[6 * (size_t)b], y = in.ego_state[6 * (size_t)b + 1];
    const double* gp = in.global_path + (size_t)b * z.max_global * 4;
    *best = __builtin_nan("");
    *at = kNoIndex;
    for (int i = w.lo + lane; i <= w.hi; i += lanes) {
        const double d = d2(gp[4 * (size_t)i], gp[4 * (size_t)i + 1], x, y);
        if (before(d, i, *best, *at)) {
            *best = d;
            *at = i;
        }
    }
}

// The lane key ego b shows: the lanes stride the window, then reduce on (d2, index).  Every lane returns the key.
template <class WV>
EMP_HD int lane_key(const Sizes& z, const In& in, int b, const WV& wv) {
    const Window w = window(in.n_global[b], z.max_global, in.pre_match_index[b], z.lane_window);
    if (w.n == 0) return -1;
    double best;
    int at;
    scan_window(z, in, b, w, wv.lane(), WV::kLanes, &best, &at);
    wv.argmin(best, at);                       // lane 0 holds index lo at least: the winner is a real index
    return in.ego_lane[(size_t)b * z.max_global + at];
}

// Where row r of ego b's actors comes from: the world's live agents in slot order, then (see_egos) its other egos in index order.
constexpr int kSrcNone = 0, kSrcAgent = 1, kSrcEgo = 2;
struct Src {
    int kind, index;               // kSrcAgent: the slot in the world; kSrcEgo: the ego's index b
};
EMP_HD Src actor_source(int r, int nw, const Range& e, int b, int see_egos) {
    Src s = {kSrcNone, 0};
    if (r < nw) {
        s.kind = kSrcAgent;
        s.index = r;
    } else if (see_egos) {
        int j = e.e0 + (r - nw);
        if (j >= b) ++j;                       // without the ego itself
        if (j < e.e1) {
            s.kind = kSrcEgo;
            s.index = j;
        }
    }
    return s;
}
EMP_HD int actor_total(int nw, const Range& e, int see_egos) { return nw + ((see_egos && e.e1 > e.e0) ? e.e1 - e.e0 - 1 : 0); }

// World w's share of the exchange, by the lanes of `wv` together (a block of the kernel, or the one lane of the host check).
// rows.agent(slot, v) / rows.ego(b, v) give the four doubles of emp_agent_observe's actor row of an agent of this world / of ego b.
template <class WV, class ROWS>
EMP_HD void exchange_world(const Sizes& z, const In& in, const Out& out, int w, const WV& wv, const ROWS& rows) {
    const int lane = wv.lane();
    const int nw = clampi(in.n_world[w], 0, z.max_world);
    const Range e = world_egos(in.ego_off, w, z.B);
    const int total = actor_total(nw, e, z.see_egos);
    const int n_act = total < z.max_act ? total : z.max_act;
    for (int b = e.e0; b < e.e1; ++b) {
        for (int r = lane; r < z.max_act; r += WV::kLanes) {
            double v[4] = {0.0, 0.0, 0.0, 0.0};
            const Src s = actor_source(r, nw, e, b, z.see_egos);
            if (s.kind == kSrcAgent) rows.agent(s.index, v);
            else if (s.kind == kSrcEgo) rows.ego(s.index, v);
            double* q = out.actors + ((size_t)b * z.max_act + r) * 4;
            q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3];
        }
        if (lane == 0) {
            out.n_act[b] = n_act;
            out.wx_status[b] = (total > z.max_act ? kActTruncated : 0) | (b - e.e0 >= z.max_other ? kNotListed : 0);
        }
    }
    if (z.max_other <= 0 || !out.other) return;
    const int E = e.e1 - e.e0, no = E < z.max_other ? E : z.max_other;
    for (int j = 0; j < no; ++j) {                         // uniform: every lane takes part in every ego's reduction
        const int b = e.e0 + j;
        const int key = lane_key(z, in, b, wv);
        if (lane == 0) {
            double v[4];
            rows.ego(b, v);
            double* q = out.other + ((size_t)w * z.max_other + j) * 5;
            q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3]; q[4] = in.ego_extent[b];
            out.other_lane[(size_t)w * z.max_other + j] = key;
        }
    }
    for (int j = no + lane; j < z.max_other; j += WV::kLanes) {
        double* q = out.other + ((size_t)w * z.max_other + j) * 5;
        q[0] = q[1] = q[2] = q[3] = q[4] = 0.0;
        out.other_lane[(size_t)w * z.max_other + j] = -1;
    }
    if (lane == 0) out.n_other[w] = no;
}

// An ego in no world sees nothing, and nobody sees it.
EMP_HD void exchange_no_world(const Sizes& z, const In& in, const Out& out, int b) {
    if (!in_no_world(in.ego_off, z.W, z.B, b)) return;
    for (int r = 0; r < z.max_act * 4; ++r) out.actors[(size_t)b * z.max_act * 4 + r] = 0.0;
    out.n_act[b] = 0;
    out.wx_status[b] = kNoWorld;
}

// ---- the launch and the argument rules, host side ---------------------------------------------------------------------------------
struct ExchangePlan {
    int grid = 0, block = 0;
    int world_blocks = 0, ego_blocks = 0;      // one block per world, then one per 64 egos for those in no world
    const char* error = nullptr;
};

constexpr const char* kBadExchangeSizes = "W < 0, B < 0, max_global < 1, or max_world outside [1, EMP_TRAFFIC_MAX_WORLD]";
constexpr const char* kBadExchangeRows = "max_act outside [1, 64] or max_other outside [0, 64]";
constexpr const char* kBadExchangeFlags = "lane_window must be at least 0 and see_egos 0 or 1";
constexpr const char* kBadEgoOff = "ego_off must be non-decreasing and lie within [0, B]";
constexpr const char* kBadEpoch = "other_tick0 must lie in [0, tick0]";
constexpr const char* kBadSpan = "the periods differ: |T * vp->dt - Ta * agent_params->dt| must not exceed 1e-9";
constexpr const char* kBadAgentClock = "Ta < 1, atick0 < 0 or atick0 + K * Ta > INT32_MAX";

// The sizes are refused before the empty batch is let through.
static inline ExchangePlan plan_exchange(int W, int B, int max_world, int max_global, int max_act, int max_other, int lane_window,
                                         int see_egos) {
    ExchangePlan p;
    if (W < 0 || B < 0 || max_global < 1 || max_world < 1 || max_world > kMaxRows) p.error = kBadExchangeSizes;
    else if (max_act < 1 || max_act > kMaxRows || max_other < 0 || max_other > kMaxRows) p.error = kBadExchangeRows;
    else if (lane_window < 0 || (see_egos != 0 && see_egos != 1)) p.error = kBadExchangeFlags;
    if (p.error || W == 0 || B == 0) return p;
    p.world_blocks = W;
    p.ego_blocks = (int)(((long long)B + kMaxRows - 1) / kMaxRows);
    p.grid = p.world_blocks + p.ego_blocks;
    p.block = kMaxRows;
    return p;
}

// ego_off [W + 1] as the host sees it (EMP_HOST): null when it is in order
static inline const char* ego_off_error(const int32_t* ego_off, int W, int B) {
    int prev = 0;
    for (int w = 0; w <= W; ++w) {
        if (ego_off[w] < prev || ego_off[w] > B) return kBadEgoOff;
        prev = ego_off[w];
    }
    return nullptr;
}

// emp_traffic_rollout_epoch: the others' rows were taken at a tick of the past or at this one
static inline const char* epoch_error(int64_t tick0, int64_t other_tick0) {
    return (other_tick0 < 0 || other_tick0 > tick0) ? kBadEpoch : nullptr;
}

// The agents' clock of emp_world_drive: period k starts at agent tick atick0 + k * Ta, and both fleets cover the same span of time.
struct WorldClockPlan {
    int64_t atick0 = 0;
    int Ta = 0;
    const char* error = nullptr;
    int64_t tick(int k) const { return atick0 + (int64_t)k * Ta; }
};
static inline WorldClockPlan plan_world_clock(int K, int T, double dt, int Ta, double agent_dt, int64_t atick0) {
    WorldClockPlan p;
    p.atick0 = atick0;
    p.Ta = Ta;
    if (Ta < 1 || K < 1 || atick0 < 0 || atick0 + (int64_t)K * Ta > 2147483647ll) {
        p.error = kBadAgentClock;
        return p;
    }
    const double diff = (double)T * dt - (double)Ta * agent_dt;
    if (!(diff <= 1e-9 && diff >= -1e-9)) p.error = kBadSpan;        // (a NaN is refused)
    return p;
}

}  // namespace wx
}  // namespace emp
