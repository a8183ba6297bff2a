// route_wave64.cpp - csrc/emp_route_core.h in its lane-parallel form on the CPU: a ThreadWave of 64 threads in place of a
// wavefront.  sync() is a barrier, and argmin / prefix / any go through a shared array between two barriers, so the strided scans,
// the prefix ranks of the stamps and every w.sync() of the core are exercised without a GPU - and a missing barrier is a data race
// that ThreadSanitizer reports.  TEST TOOL ONLY: compiled with g++ -ffp-contract=off into a temporary directory by
// tests/test_route_hard_host.py, never by the package.
//   rw_route            rc_route's signature (route_check.cpp), the queries of a batch one after the other on the same 64 threads
//   -DROUTE_WAVE64_MAIN a program: reads a graph and queries from the file named on its command line, runs the 64-thread wave and
//                       the one-lane HostWave, exits non-zero unless every output byte agrees.  This is what sanitizer builds run.
#include <pthread.h>
#include <stddef.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../emplanner_carla_amd/csrc/emp_route_core.h"
#include "../../include/emplanner.h"

using namespace emp;

namespace {

struct Shared {
    pthread_barrier_t barrier;
    double f[64];
    int key[64], idx[64], flag[64];
};

struct ThreadWave {
    static constexpr int kLanes = 64;
    int id;
    Shared* s;
    int lane() const { return id; }
    void sync() const { pthread_barrier_wait(&s->barrier); }
    void argmin(double& f, int& key, int& idx) const {
        s->f[id] = f;
        s->key[id] = key;
        s->idx[id] = idx;
        sync();
        double bf = s->f[0];
        int bk = s->key[0], bi = s->idx[0];
        for (int l = 1; l < kLanes; ++l)
            if (route::before(s->f[l], s->key[l], s->idx[l], bf, bk, bi)) {
                bf = s->f[l];
                bk = s->key[l];
                bi = s->idx[l];
            }
        sync();
        f = bf;
        key = bk;
        idx = bi;
    }
    int prefix(bool flag, int* total) const {
        s->flag[id] = flag ? 1 : 0;
        sync();
        int below = 0, all = 0;
        for (int l = 0; l < kLanes; ++l) {
            if (l < id) below += s->flag[l];
            all += s->flag[l];
        }
        sync();
        *total = all;
        return below;
    }
    bool any(bool flag) const {
        int total = 0;
        prefix(flag, &total);
        return total != 0;
    }
};

struct Batch {
    route::Graph G;
    int B, max_route, max_global;
    const int *start_node, *end_edge;
    const double *origin_wp, *dest_wp;      // null: A* only
    int *route, *route_len, *wp_index;
    double* global_path;
    int *n_global, *status;
};

// one query on wave `w`; lane 0 stores the counts, as route_kernel does
template <class W>
void one_query(const Batch& t, const route::State& S, int b, const W& w) {
    route::Query q = {t.start_node[b], t.end_edge[b], nullptr, nullptr};
    route::Result r = {t.route + (size_t)b * t.max_route, t.max_route, {nullptr, nullptr, t.max_global}, 0, 0, 0};
    if (t.origin_wp) {
        q.origin_wp = t.origin_wp + 3 * (size_t)b;
        q.dest_wp = t.dest_wp + 3 * (size_t)b;
        r.path.wp_index = t.wp_index + (size_t)b * t.max_global;
        r.path.global_path = t.global_path + (size_t)b * t.max_global * 4;
    }
    route::run_query(t.G, S, q, r, w);
    if (w.lane() == 0) {
        t.route_len[b] = r.route_len;
        t.status[b] = r.status;
        if (t.origin_wp) t.n_global[b] = r.n_global;
    }
}

struct StateArrays {
    std::vector<double> h;
    std::vector<int> g, parent, stamp, state;
    explicit StateArrays(int n) : h(n), g(n), parent(n), stamp(n), state(n) {}
    route::State view() { return {h.data(), g.data(), parent.data(), stamp.data(), state.data()}; }
};

void run_wave64(const Batch& t) {
    StateArrays arrays(t.G.n_nodes);
    const route::State S = arrays.view();
    Shared shared;
    pthread_barrier_init(&shared.barrier, nullptr, ThreadWave::kLanes);
    std::vector<std::thread> lanes;
    for (int id = 0; id < ThreadWave::kLanes; ++id)
        lanes.emplace_back([&t, &S, &shared, id] {
            const ThreadWave w = {id, &shared};
            for (int b = 0; b < t.B; ++b) {
                one_query(t, S, b, w);
                w.sync();                     // the next query is another block's on the device: it starts on a state nobody reads
            }
        });
    for (auto& th : lanes) th.join();
    pthread_barrier_destroy(&shared.barrier);
}

[[maybe_unused]] void run_one_lane(const Batch& t) {      // (the program's other half)
    StateArrays arrays(t.G.n_nodes);
    const route::State S = arrays.view();
    for (int b = 0; b < t.B; ++b) one_query(t, S, b, route::HostWave{});
}

}  // namespace

extern "C" {

// emp_route_paths on 64 CPU threads (origin_wp == null: emp_route_search).  The outputs are zero on entry.
void rw_route(const emp_route_graph* g, int B, int max_route, int max_global, const int* start_node, const int* end_edge,
              const double* origin_wp, const double* dest_wp, int* route, int* route_len, int* wp_index, double* global_path,
              int* n_global, int* status) {
    const Batch t = {{g->vertex, g->succ_off, g->succ, g->length, g->wp_off, g->wp, g->n_nodes, g->n_edges, g->n_wp}, B, max_route, max_global,
                     start_node, end_edge, origin_wp, dest_wp, route, route_len, wp_index, global_path, n_global, status};
    run_wave64(t);
}

}  // extern "C"

#ifdef ROUTE_WAVE64_MAIN
#include <stdio.h>

// The file: int32 N, E, W, B, max_route, max_global, search_only; then vertex [N][3] f64, succ_off [N+1], succ [E], length [E],
// wp_off [E+1] i32, wp [W][3] f64, start_node [B], end_edge [B] i32, origin_wp [B][3], dest_wp [B][3] f64 - each array padded to
// a multiple of 8 bytes.
struct Reader {
    std::vector<char> bytes;
    size_t at = 0;
    bool ok = true;
    template <class T>
    std::vector<T> take(size_t n) {
        std::vector<T> v(n);
        const size_t size = n * sizeof(T);
        if (at + size > bytes.size()) {
            ok = false;
            return v;
        }
        if (size) memcpy(v.data(), bytes.data() + at, size);
        at += (size + 7) / 8 * 8;
        return v;
    }
};

struct Outputs {
    std::vector<int> route, route_len, wp_index, n_global, status;
    std::vector<double> global_path;
    Outputs(int B, int max_route, int max_global)
        : route((size_t)B * max_route), route_len(B), wp_index((size_t)B * max_global), n_global(B), status(B),
          global_path((size_t)B * max_global * 4) {}
};

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main(int argc, char** argv) {
    if (argc != 2) return printf("usage: route_wave64 <file>\n"), 2;
    Reader in;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return printf("route_wave64: cannot open %s\n", argv[1]), 2;
    char chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) in.bytes.insert(in.bytes.end(), chunk, chunk + n);
    fclose(f);
    const std::vector<int> head = in.take<int>(8);
    if (!in.ok) return printf("route_wave64: short file\n"), 2;
    const int N = head[0], E = head[1], W = head[2], B = head[3], max_route = head[4], max_global = head[5], search_only = head[6];
    if (N < 1 || N > route::kMaxNodes || E < 0 || W < 0 || B < 0 || max_route < 2 || max_global < 1) return printf("route_wave64: bad header\n"), 2;
    const std::vector<double> vertex = in.take<double>(3 * (size_t)N);
    const std::vector<int> succ_off = in.take<int>((size_t)N + 1), succ = in.take<int>(E), length = in.take<int>(E), wp_off = in.take<int>((size_t)E + 1);
    const std::vector<double> wp = in.take<double>(3 * (size_t)W);
    const std::vector<int> start_node = in.take<int>(B), end_edge = in.take<int>(B);
    const std::vector<double> origin_wp = in.take<double>(3 * (size_t)B), dest_wp = in.take<double>(3 * (size_t)B);
    if (!in.ok) return printf("route_wave64: short file\n"), 2;
    const route::Graph G = {vertex.data(), succ_off.data(), succ.data(), length.data(), wp_off.data(), wp.data(), N, E, W};
    if (const char* e = route::graph_error(G)) return printf("route_wave64: %s\n", e), 2;
    Outputs a(B, max_route, max_global), b(B, max_route, max_global);
    Batch t = {G, B, max_route, max_global, start_node.data(), end_edge.data(), search_only ? nullptr : origin_wp.data(),
               search_only ? nullptr : dest_wp.data(), a.route.data(), a.route_len.data(), a.wp_index.data(), a.global_path.data(),
               a.n_global.data(), a.status.data()};
    run_wave64(t);
    t.route = b.route.data(), t.route_len = b.route_len.data(), t.wp_index = b.wp_index.data(), t.global_path = b.global_path.data();
    t.n_global = b.n_global.data(), t.status = b.status.data();
    run_one_lane(t);
    const bool same = same_bytes(a.route, b.route) && same_bytes(a.route_len, b.route_len) && same_bytes(a.wp_index, b.wp_index) &&
                      same_bytes(a.global_path, b.global_path) && same_bytes(a.n_global, b.n_global) && same_bytes(a.status, b.status);
    int routed = 0;
    for (int q = 0; q < B; ++q) routed += b.status[q] == 0;
    printf("route_wave64: %d queries, %d routed, 64 threads and one lane %s\n", B, routed, same ? "agree" : "DIFFER");
    return same ? 0 : 1;
}
#endif
