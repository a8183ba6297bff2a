// world_check.cpp - runs csrc/emp_world_core.h (who sees whom in emp_world_exchange; the launch plan and the argument rules of the
// world calls) on the CPU for the `-m "not gpu"` suite.  The actor rows are passed in as data, so libm plays no part.  TEST TOOL
// ONLY: compiled with g++ into a temporary directory by tests/test_world_host.py, never by the package.
#include "../../emplanner_carla_amd/csrc/emp_world_core.h"

namespace {

using namespace emp::wx;

// the one lane of a CPU run: the strided loops visit every index, the reduction has nothing to do
struct Wave1 {
    static constexpr int kLanes = 1;
    int lane() const { return 0; }
    void argmin(double&, int&) const {}
};

struct DataRows {
    const double* agent_rows;      // [max_world][4] of this world
    const double* ego_rows;        // [B][4]
    void agent(int slot, double* v) const {
        for (int i = 0; i < 4; ++i) v[i] = agent_rows[4 * slot + i];
    }
    void ego(int b, double* v) const {
        for (int i = 0; i < 4; ++i) v[i] = ego_rows[4 * (size_t)b + i];
    }
};

}  // namespace

extern "C" {

// The kernel's grid on the CPU: every world's block, then every ego for the no-world pass.
void wc_exchange(int W, int B, int max_world, int max_global, int max_act, int max_other, int lane_window, int see_egos, const int* n_world,
                 const int* ego_off, const double* ego_state, const double* ego_extent, const double* global_path, const int* n_global,
                 const int* ego_lane, const int* pre_match_index, const double* agent_rows, const double* ego_rows, double* actors,
                 int* n_act, double* other, int* other_lane, int* n_other, int* wx_status) {
    const Sizes z{W, B, max_world, max_global, max_act, max_other, lane_window, see_egos};
    const In in{n_world, ego_off, ego_state, ego_extent, global_path, n_global, ego_lane, pre_match_index};
    const Out out{actors, n_act, other, other_lane, n_other, wx_status};
    for (int w = 0; w < W; ++w) exchange_world(z, in, out, w, Wave1{}, DataRows{agent_rows + 4 * (size_t)w * max_world, ego_rows});
    for (int b = 0; b < B; ++b) exchange_no_world(z, in, out, b);
}

// The match of ego b as 64 lanes make it: each lane's strided scan, then the xor butterfly of the kernel on (d2, index).
// -> the winning index (-1 with n == 0), or -2 if the lanes do not end on the same pair.
int wc_match64(int max_global, int lane_window, int b, const double* ego_state, const double* global_path, const int* n_global,
               const int* pre_match_index) {
    const Sizes z{0, 0, 1, max_global, 1, 0, lane_window, 0};
    const In in{nullptr, nullptr, ego_state, nullptr, global_path, n_global, nullptr, pre_match_index};
    const Window w = window(n_global[b], max_global, pre_match_index[b], lane_window);
    if (w.n == 0) return -1;
    double d[64];
    int at[64];
    for (int l = 0; l < 64; ++l) scan_window(z, in, b, w, l, 64, &d[l], &at[l]);
    for (int off = 32; off; off >>= 1) {
        double nd[64];
        int na[64];
        for (int l = 0; l < 64; ++l) {
            const bool take = before(d[l ^ off], at[l ^ off], d[l], at[l]);
            nd[l] = take ? d[l ^ off] : d[l];
            na[l] = take ? at[l ^ off] : at[l];
        }
        for (int l = 0; l < 64; ++l) {
            d[l] = nd[l];
            at[l] = na[l];
        }
    }
    for (int l = 1; l < 64; ++l)
        if (at[l] != at[0]) return -2;
    return at[0];
}

// out5 = grid, block, world_blocks, ego_blocks, refused; -> the refusal's text or null
const char* wc_plan(int W, int B, int max_world, int max_global, int max_act, int max_other, int lane_window, int see_egos, int* out5) {
    const ExchangePlan p = plan_exchange(W, B, max_world, max_global, max_act, max_other, lane_window, see_egos);
    out5[0] = p.grid;
    out5[1] = p.block;
    out5[2] = p.world_blocks;
    out5[3] = p.ego_blocks;
    out5[4] = p.error ? 1 : 0;
    return p.error;
}

const char* wc_ego_off(const int* ego_off, int W, int B) { return ego_off_error(ego_off, W, B); }

const char* wc_epoch(long long tick0, long long other_tick0) { return epoch_error(tick0, other_tick0); }

// ticks[k] = the agents' tick of period k for k < min(K, n); -> the refusal's text or null
const char* wc_clock(int K, int T, double dt, int Ta, double agent_dt, long long atick0, long long* ticks, int n) {
    const WorldClockPlan p = plan_world_clock(K, T, dt, Ta, agent_dt, atick0);
    if (p.error) return p.error;
    for (int k = 0; k < K && k < n; ++k) ticks[k] = p.tick(k);
    return nullptr;
}

}  // extern "C"
