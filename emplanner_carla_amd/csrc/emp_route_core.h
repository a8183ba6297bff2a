// emp_route_core.h - global routing: the reference's A* over a road graph held as arrays, the expansion of a route into waypoints
// and their heading / curvature, as plain functions that hipcc (route_kernel, emp_route_kernels.h: one query per wavefront) and
// g++ (tests/host_check/route_check.cpp: one lane) both compile.  include/emplanner.h states the procedure and its arithmetic
// once (emp_route_graph's block); this file is that statement in C++.
// ref: planner/global_planning.py _A_star (:168-214), _route_search (:153-166), search_path_way (:234-272).
//
// Every function is written for the lanes of ONE wavefront working on ONE query.  `W` is how they talk to each other: the lane's
// number, the lane count, a barrier that makes the lanes' stores visible to each other, and three collectives.  HostWave below is
// the one-lane form; the device form is in emp_route_kernels.h.  Every value a branch depends on is either read by all lanes from
// the same address or comes out of a collective, so control flow is uniform across the wavefront and every lane meets every
// barrier.  No loop waits on data: each is bounded by N, by an out-degree or by a waypoint count.
//
// Arithmetic contract: as emp_control_core.h - written order, separately rounded binary64 operations, -ffp-contract=off.
#pragma once

#include <vector>

#include "emp_core.h"             // EMP_HD
#include "emp_frenet_core.h"      // centred_diff: the heading / curvature of emp_heading_kappa

namespace emp {
namespace route {

constexpr int kMaxNodes = 4096;           // EMP_ROUTE_MAX_NODES
constexpr int kMaxLength = 1 << 18;       // EMP_ROUTE_MAX_LENGTH: N * kMaxLength stays below 2^31
constexpr int kUnreachable = 1, kTruncated = 2, kBadQuery = 4;      // EMP_ROUTE_*
constexpr int kNew = 0, kOpen = 1, kClosed = 2;

struct Graph {
    const double* vertex;
    const int* succ_off;
    const int* succ;
    const int* length;
    const int* wp_off;
    const double* wp;
    int n_nodes, n_edges, n_wp;
};

// The per-node state of one query, N entries each (LDS on the device).  After backtrack() `stamp` holds the route's forward links.
struct State {
    double* h;
    int* g;
    int* parent;
    int* stamp;
    int* state;
};
// (P: the kernel's LDS pointer, or a byte count from 0 on the host, whose `end` is what the launch asks for)
template <class P>
struct StateLds {
    P h, g, parent, stamp, state, end;
};
template <class P>
EMP_HD StateLds<P> state_lds(P at, int n_nodes) {
    StateLds<P> L;
    L.h = at;      at += (size_t)n_nodes * 8;
    L.g = at;      at += (size_t)n_nodes * 4;
    L.parent = at; at += (size_t)n_nodes * 4;
    L.stamp = at;  at += (size_t)n_nodes * 4;
    L.state = at;  at += (size_t)n_nodes * 4;
    L.end = at;
    return L;
}

struct HostWave {
    static constexpr int kLanes = 1;
    int lane() const { return 0; }
    void sync() const {}
    // every lane leaves with the smallest (f, key) among the lanes whose idx >= 0, and that lane's idx; -1 when there is none
    void argmin(double&, int&, int&) const {}
    // the number of lower lanes whose flag is set; *total: of all lanes
    int prefix(bool flag, int* total) const {
        *total = flag ? 1 : 0;
        return 0;
    }
    bool any(bool flag) const { return flag; }
};

EMP_HD double dist3(const double* p, const double* q) {
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return sqrt(((dx * dx) + (dy * dy)) + (dz * dz));
}

// (a.f, a.key) before (b.f, b.key)?  Only among candidates that exist (idx >= 0).
EMP_HD bool before(double af, int akey, int aidx, double bf, int bkey, int bidx) {
    if (aidx < 0) return false;
    return bidx < 0 || af < bf || (af == bf && akey < bkey);
}

// The ends of edge id e: n_exit = succ[e], n_end = the node whose list holds e.  False for an id that no list holds.
EMP_HD bool edge_ends(const Graph& G, int e, int* n_end, int* n_exit) {
    if (e < 0 || e >= G.n_edges) return false;
    int lo = 0, hi = G.n_nodes;                   // the last node whose offset is <= e: at most 13 halvings, whatever the offsets hold
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (G.succ_off[mid] <= e) lo = mid; else hi = mid;
    }
    if (!(G.succ_off[lo] <= e && e < G.succ_off[lo + 1])) return false;
    const int x = G.succ[e];
    if (x < 0 || x >= G.n_nodes) return false;
    *n_end = lo;
    *n_exit = x;
    return true;
}

// _A_star.  Returns 0 (n_end closed: parent[] leads back to start), kUnreachable or kBadQuery.  start and n_end lie in [0, N).
template <class W>
EMP_HD int search(const Graph& G, const State& S, int start, int n_end, const W& w) {
    const int N = G.n_nodes, lane = w.lane();
    for (int n = lane; n < N; n += W::kLanes) {
        S.h[n] = dist3(G.vertex + 3 * (size_t)n, G.vertex + 3 * (size_t)n_end);
        S.state[n] = kNew;
    }
    w.sync();
    if (lane == 0) {
        S.state[start] = kOpen;
        S.g[start] = 0;
        S.parent[start] = -1;
        S.stamp[start] = 0;
    }
    w.sync();
    int next_stamp = 1;
    for (int pop = 0; pop < N; ++pop) {           // each pass closes one node
        double bf = 0.0;
        int bs = 0, c = -1;
        for (int n = lane; n < N; n += W::kLanes) {
            if (S.state[n] != kOpen) continue;
            double f = (double)S.g[n] + S.h[n];
            if (!(f == f)) f = INFINITY;
            if (before(f, S.stamp[n], n, bf, bs, c)) {
                bf = f;
                bs = S.stamp[n];
                c = n;
            }
        }
        w.argmin(bf, bs, c);
        if (c < 0) return kUnreachable;
        if (c == n_end) {
            if (lane == 0) S.state[c] = kClosed;
            w.sync();
            return 0;
        }
        const int e0 = G.succ_off[c], e1 = G.succ_off[c + 1];
        if (e0 < 0 || e1 > G.n_edges || e0 > e1) return kBadQuery;
        const int gc = S.g[c];
        for (int base = e0; base < e1; base += W::kLanes) {      // 64 successors at a time, stamps in CSR order
            const int e = base + lane;
            int suc = -1;
            bool bad = false;
            if (e < e1) {
                suc = G.succ[e];
                if (suc < 0 || suc >= N) {
                    bad = true;
                    suc = -1;
                }
            }
            if (w.any(bad)) return kBadQuery;
            bool is_new = false;
            int ng = 0;
            if (suc >= 0) {
                ng = (int)((unsigned)gc + (unsigned)G.length[e]);
                const int st = S.state[suc];
                if (st == kOpen) {
                    if (ng < S.g[suc]) {
                        S.g[suc] = ng;
                        S.parent[suc] = c;
                    }
                } else if (st == kNew) {
                    is_new = true;
                }
            }
            int total = 0;
            const int pos = w.prefix(is_new, &total);
            if (is_new) {
                S.state[suc] = kOpen;
                S.g[suc] = ng;
                S.parent[suc] = c;
                S.stamp[suc] = next_stamp + pos;
            }
            next_stamp += total;
            w.sync();
        }
        if (lane == 0) S.state[c] = kClosed;
        w.sync();
    }
    return kUnreachable;
}

// The route behind a successful search: the number of nodes from start to n_end, and in S.stamp the link from each of them to the
// next.  A chain of parents visits no node twice (every node is closed once), so N steps bound it.
template <class W>
EMP_HD int backtrack(const Graph& G, const State& S, int n_end, const W& w) {
    int count = 1;
    for (int n = n_end; S.parent[n] >= 0 && count < G.n_nodes; n = S.parent[n]) ++count;
    w.sync();                                      // (stamps were read by the search until here)
    if (w.lane() == 0) {
        int n = n_end;
        for (int i = 1; i < count; ++i) {
            const int p = S.parent[n];
            S.stamp[p] = n;
            n = p;
        }
    }
    w.sync();
    return count;
}

// The first edge of u that leads to v, -1 without one (or with offsets out of range)
EMP_HD int find_edge(const Graph& G, int u, int v) {
    const int e0 = G.succ_off[u], e1 = G.succ_off[u + 1];
    if (e0 < 0 || e1 > G.n_edges) return -1;
    for (int e = e0; e < e1; ++e)
        if (G.succ[e] == v) return e;
    return -1;
}

// _closest_index over the waypoints [a, b): relative to a, -1 where no distance is below +inf (the reference's initial index)
template <class W>
EMP_HD int closest(const Graph& G, const double* p, int a, int b, const W& w) {
    double bd = INFINITY;
    int bj = -1;
    for (int j = a + w.lane(); j < b; j += W::kLanes) {
        const double d = dist3(G.wp + 3 * (size_t)j, p);
        if (d < bd) {
            bd = d;
            bj = j;
        }
    }
    int key = bj;
    w.argmin(bd, key, bj);
    return bj < 0 ? -1 : bj - a;
}

struct PathOut {
    int* wp_index;            // [max_global]
    double* global_path;      // [max_global][4]
    int max_global;
};

// appends the waypoints [a, b) at position `at`; what lies beyond the capacity is counted only
template <class W>
EMP_HD long long emit(const Graph& G, const PathOut& o, long long at, int a, int b, const W& w) {
    for (int j = a + w.lane(); j < b; j += W::kLanes) {
        const long long pos = at + (j - a);
        if (pos >= o.max_global) break;
        o.wp_index[pos] = j;
        o.global_path[4 * pos] = G.wp[3 * (size_t)j];
        o.global_path[4 * pos + 1] = G.wp[3 * (size_t)j + 1];
    }
    return at + (b > a ? b - a : 0);
}

// the waypoint range of edge (u, v); false where the graph's own indices are out of range
EMP_HD bool edge_waypoints(const Graph& G, int u, int v, int* a, int* b) {
    const int e = find_edge(G, u, v);
    if (e < 0) return false;
    *a = G.wp_off[e];
    *b = G.wp_off[e + 1];
    return *a >= 0 && *b <= G.n_wp && *b - *a >= 2;
}

// search_path_way's expansion of the route start -> ... -> n_end (count nodes, linked through S.stamp) -> n_exit.  Returns the
// number of waypoints (all of them, written or not), -1 where the graph's indices are out of range.
template <class W>
EMP_HD long long expand(const Graph& G, const State& S, int start, int count, int n_exit, const double* origin_wp,
                        const double* dest_wp, const PathOut& o, const W& w) {
    long long at = 0;
    int u = start, a = 0, b = 0;
    for (int i = 0; i < count; ++i) {             // edge i of `count`: the last one leads to n_exit
        const bool last = i == count - 1;
        const int v = last ? n_exit : S.stamp[u];
        if (!edge_waypoints(G, u, v, &a, &b)) return -1;
        if (i == 0) {                             // path[k:], and path[-1:] is the exit alone
            const int k = closest(G, origin_wp, a, b, w);
            at = emit(G, o, at, k < 0 ? b - 1 : a + k, b, w);
        } else if (!last) {
            at = emit(G, o, at, a + 1, b, w);
        }
        if (last) {                               // path[:k + 1] when k != 0, and path[:0] is empty
            const int k = closest(G, dest_wp, a + 1, b, w);
            if (k > 0) at = emit(G, o, at, a + 1, a + 1 + k + 1, w);
        }
        u = v;
    }
    return at;
}

// cal_heading_kappa on the m written points of a global path [m][4]: emp_frenet_core.h's heading_kappa, a point per lane
template <class W>
EMP_HD void heading_kappa_rows(double* gp, int m, const W& w) {
    if (m < 2) return;
    w.sync();
    for (int i = w.lane(); i < m; i += W::kLanes) {
        const double dx = centred_diff(gp, 4, i, m), dy = centred_diff(gp + 1, 4, i, m);
        gp[4 * (size_t)i + 2] = atan2(dy, dx);
    }
    w.sync();
    for (int i = w.lane(); i < m; i += W::kLanes) {
        const double dx = centred_diff(gp, 4, i, m), dy = centred_diff(gp + 1, 4, i, m);
        gp[4 * (size_t)i + 3] = sin(centred_diff(gp + 2, 4, i, m)) / sqrt(dx * dx + dy * dy);
    }
}

struct Query {
    int start_node, end_edge;
    const double* origin_wp;      // [3]; null: A* only
    const double* dest_wp;
};
struct Result {
    int* route;                   // [max_route]
    int max_route;
    PathOut path;                 // unused for A* only
    int route_len, n_global, status;
};

// One query, from its numbers to its outputs.  The arrays of `r` are zero on entry and the lanes write only what is used.
template <class W>
EMP_HD void run_query(const Graph& G, const State& S, const Query& q, Result& r, const W& w) {
    r.route_len = r.n_global = 0;
    r.status = kBadQuery;
    int n_end = 0, n_exit = 0;
    if (q.start_node < 0 || q.start_node >= G.n_nodes || !edge_ends(G, q.end_edge, &n_end, &n_exit)) return;
    r.status = search(G, S, q.start_node, n_end, w);
    if (r.status) return;
    const int count = backtrack(G, S, n_end, w);
    long long n_global = 0;
    if (q.origin_wp) {
        n_global = expand(G, S, q.start_node, count, n_exit, q.origin_wp, q.dest_wp, r.path, w);
        if (n_global < 0) {           // nothing stays of what was written before the bad index
            r.status = kBadQuery;
            w.sync();
            for (int pos = w.lane(); pos < r.path.max_global; pos += W::kLanes) {
                r.path.wp_index[pos] = 0;
                r.path.global_path[4 * (size_t)pos] = r.path.global_path[4 * (size_t)pos + 1] = 0.0;
            }
            return;
        }
    }
    if (w.lane() == 0) {
        int n = q.start_node;
        for (int i = 0; i < count && i < r.max_route; ++i) {
            r.route[i] = n;
            if (i < count - 1) n = S.stamp[n];
        }
        if (count < r.max_route) r.route[count] = n_exit;
    }
    r.route_len = count + 1;
    r.n_global = n_global > 0x7fffffffLL ? 0x7fffffff : (int)n_global;
    if (r.route_len > r.max_route || n_global > r.path.max_global) r.status |= kTruncated;
    if (q.origin_wp) heading_kappa_rows(r.path.global_path, n_global < r.path.max_global ? (int)n_global : r.path.max_global, w);
}

// What RoadGraph and the EMP_HOST entry points refuse: null when the graph is sound.  Host only.
inline const char* graph_error(const Graph& G) {
    if (G.n_nodes < 1 || G.n_nodes > kMaxNodes) return "route graph: n_nodes outside [1, EMP_ROUTE_MAX_NODES]";
    if (G.n_edges < 0 || G.n_wp < 0) return "route graph: negative count";
    for (long long i = 0; i < 3LL * G.n_nodes; ++i)
        if (!(G.vertex[i] - G.vertex[i] == 0.0)) return "route graph: vertex is not finite";
    if (G.succ_off[0] != 0 || G.succ_off[G.n_nodes] != G.n_edges) return "route graph: succ_off does not span [0, n_edges]";
    for (int n = 0; n < G.n_nodes; ++n)
        if (G.succ_off[n] > G.succ_off[n + 1]) return "route graph: succ_off is not monotone";
    for (int e = 0; e < G.n_edges; ++e) {
        if (G.succ[e] < 0 || G.succ[e] >= G.n_nodes) return "route graph: successor index out of range";
        if (G.length[e] < 0 || G.length[e] > kMaxLength) return "route graph: length outside [0, 2^18]";
    }
    std::vector<int> listed_by(G.n_nodes, -1);         // the lanes relax one node's successors side by side: each at most once
    for (int n = 0; n < G.n_nodes; ++n)
        for (int e = G.succ_off[n]; e < G.succ_off[n + 1]; ++e) {
            if (listed_by[G.succ[e]] == n) return "route graph: a node lists the same successor twice";
            listed_by[G.succ[e]] = n;
        }
    if (G.wp_off[0] != 0 || G.wp_off[G.n_edges] != G.n_wp) return "route graph: wp_off does not span [0, n_wp]";
    for (int e = 0; e < G.n_edges; ++e)
        if (G.wp_off[e + 1] - (long long)G.wp_off[e] < 2) return "route graph: an edge with fewer than 2 waypoints";
    for (long long i = 0; i < 3LL * G.n_wp; ++i)
        if (!(G.wp[i] - G.wp[i] == 0.0)) return "route graph: waypoint is not finite";
    return nullptr;
}

}  // namespace route
}  // namespace emp
