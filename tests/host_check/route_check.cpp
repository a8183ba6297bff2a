// route_check.cpp - runs csrc/emp_route_core.h (the A* search, the expansion and the heading / curvature of global routing) and
// csrc/emp_route_launch.h (its launch plan) on the CPU for the `-m "not gpu"` suite: the very functions route_kernel compiles, with
// one lane in place of a wavefront.  TEST TOOL ONLY: compiled with g++ -ffp-contract=off into a temporary directory by
// tests/test_routing_host.py, never by the package.  With -DROUTE_CHECK_MAIN it is a program of its own (a ring graph, every pair)
// that a sanitizer build can run.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../emplanner_carla_amd/csrc/emp_route_launch.h"
#include "../../include/emplanner.h"

using namespace emp;

static route::Graph graph_of(const emp_route_graph* g) {
    return {g->vertex, g->succ_off, g->succ, g->length, g->wp_off, g->wp, g->n_nodes, g->n_edges, g->n_wp};
}

extern "C" {

// out4 = grid, block, lds bytes, waves per compute unit; returns the refusal's text or null
const char* rc_plan(int B, int n_nodes, int max_route, int max_global, long long* out4) {
    const RoutePlan p = plan_route(B, n_nodes, max_route, max_global);
    out4[0] = p.grid;
    out4[1] = p.block;
    out4[2] = (long long)p.lds;
    out4[3] = p.waves_per_cu;
    return p.error;
}

const char* rc_graph_error(const emp_route_graph* g) { return route::graph_error(graph_of(g)); }

// sizeof and the offsets of emp_route_graph's ten fields
void rc_layout(long long* out11) {
    const size_t v[11] = {sizeof(emp_route_graph), offsetof(emp_route_graph, vertex), offsetof(emp_route_graph, succ_off),
                          offsetof(emp_route_graph, succ), offsetof(emp_route_graph, length), offsetof(emp_route_graph, wp_off),
                          offsetof(emp_route_graph, wp), offsetof(emp_route_graph, n_nodes), offsetof(emp_route_graph, n_edges),
                          offsetof(emp_route_graph, n_wp), offsetof(emp_route_graph, reserved)};
    for (int i = 0; i < 11; ++i) out11[i] = (long long)v[i];
}

// emp_route_paths on the CPU (origin_wp == null: emp_route_search).  The outputs are zero on entry, as the library makes them.
void rc_route(const emp_route_graph* g, int B, int max_route, int max_global, const int* start_node, const int* end_edge,
              const double* origin_wp, const double* dest_wp, int* route, int* route_len, int* wp_index, double* global_path,
              int* n_global, int* status) {
    const route::Graph G = graph_of(g);
    std::vector<double> h(G.n_nodes);
    std::vector<int> gc(G.n_nodes), parent(G.n_nodes), stamp(G.n_nodes), state(G.n_nodes);
    const route::State S = {h.data(), gc.data(), parent.data(), stamp.data(), state.data()};
    for (int b = 0; b < B; ++b) {
        route::Query q = {start_node[b], end_edge[b], nullptr, nullptr};
        route::Result r = {route + (size_t)b * max_route, max_route, {nullptr, nullptr, max_global}, 0, 0, 0};
        if (origin_wp) {
            q.origin_wp = origin_wp + 3 * (size_t)b;
            q.dest_wp = dest_wp + 3 * (size_t)b;
            r.path.wp_index = wp_index + (size_t)b * max_global;
            r.path.global_path = global_path + (size_t)b * max_global * 4;
        }
        route::run_query(G, S, q, r, route::HostWave{});
        route_len[b] = r.route_len;
        status[b] = r.status;
        if (origin_wp) n_global[b] = r.n_global;
    }
}

}  // extern "C"

#ifdef ROUTE_CHECK_MAIN
#include <stdio.h>

// A ring of n nodes, both ways, two waypoints between neighbours: every (start, end edge) pair must give a route whose length is the
// shorter way round plus the exit node, with every capacity one short of need and exactly enough.
int main() {
    const int n = 17;
    std::vector<double> vertex, wp;
    std::vector<int> succ_off{0}, succ, length, wp_off{0};
    auto at = [&](int k, double* p) {
        p[0] = 10.0 * cos(6.283185307179586 * k / n);
        p[1] = 10.0 * sin(6.283185307179586 * k / n);
        p[2] = 0.25 * (k % 2);
    };
    for (int k = 0; k < n; ++k) {
        double p[3];
        at(k, p);
        vertex.insert(vertex.end(), p, p + 3);
        for (int v : {(k + 1) % n, (k + n - 1) % n}) {
            double q[3];
            at(v, q);
            succ.push_back(v);
            length.push_back(3);
            for (int i = 0; i <= 3; ++i)
                for (int c = 0; c < 3; ++c) wp.push_back(p[c] + (q[c] - p[c]) * i / 3.0);
            wp_off.push_back((int)wp.size() / 3);
        }
        succ_off.push_back((int)succ.size());
    }
    const emp_route_graph g = {vertex.data(), succ_off.data(), succ.data(), length.data(), wp_off.data(), wp.data(), n, (int)succ.size(),
                               (int)wp.size() / 3, 0};
    if (const char* e = rc_graph_error(&g)) return printf("graph refused: %s\n", e), 1;
    int bad = 0;
    for (int cap = 0; cap < 2; ++cap)
        for (int s = 0; s < n; ++s)
            for (int e = 0; e < g.n_edges; ++e) {
                const int n_end = e / 2, hops = (n_end - s + n) % n < (s - n_end + n) % n ? (n_end - s + n) % n : (s - n_end + n) % n;
                const int need = hops + 2, max_route = need - cap < 2 ? 2 : need - cap, max_global = 3 * need + 4 - 20 * cap < 1 ? 1 : 3 * need + 4 - 20 * cap;
                std::vector<int> route(max_route), wpi(max_global);
                std::vector<double> gp(4 * (size_t)max_global);
                int len = 0, ng = 0, st = 0;
                rc_route(&g, 1, max_route, max_global, &s, &e, &wp[3 * (size_t)wp_off[2 * s]], &wp[3 * (size_t)wp_off[e + 1] - 3], route.data(), &len,
                         wpi.data(), gp.data(), &ng, &st);
                if (len != need || (st & ~EMP_ROUTE_TRUNCATED) || ((st != 0) != (len > max_route || ng > max_global))) ++bad;
            }
    printf("route_check: %d bad of %d\n", bad, 2 * n * g.n_edges);
    return bad != 0;
}
#endif
