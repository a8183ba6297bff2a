// CPU check of the rows solver's LDS layout (csrc/emp_qp_core.h, PathQpRowsLayout): test tool only, built with g++ by
// tests/test_qp_rows_layout_host.py.  For one (GP, R) it returns the layout's offsets and sizes, and replays the windows the
// solver reads and the padding path_qp_group_rows writes on a model of one wavefront's LDS, so that the test can compare
// them with arithmetic of its own.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../emplanner_carla_amd/csrc/emp_core.h"
#include "../../emplanner_carla_amd/csrc/emp_qp_core.h"

using namespace emp;

namespace {

// out: C, cc, P, q, u, dua, rhs, c, lo, hi, tmp, wgt, words, result, path, obstacles(max_obs), stride(max_obs), max_stations
template <int GP, int R>
void offsets(int max_obs, long long* out) {
    using L = PathQpRowsLayout<GP, R>;
    const long long v[] = {L::C, L::cc, L::P, L::q, L::u, L::dua, L::rhs, L::c, L::lo, L::hi, L::tmp, L::wgt, L::words, L::result, L::path,
                           max_obs <= L::C ? L::obstacles : L::words, L::stride(max_obs), L::max_stations};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// Every double of one wavefront's LDS (64 / GP groups at the launcher's stride) gets an owner tag: group * 16 + array
// (1 cc .. 11 wgt, 0 = unused).  Then every address a lane of group `grp` reads through the solver's windows, and every
// address the padding of a problem with N unknowns and ns stations writes, is looked up.  returns 0, or a code that names
// what went wrong first: 1 out of the wavefront's bytes, 2 another group's double, 3 a padded double inside the problem,
// 4 a window double outside the problem that the padding does not write, 5 arrays overlap.
template <int GP, int R>
int replay(int max_obs, int N, int ns, long long wave_bytes) {
    using L = PathQpRowsLayout<GP, R>;
    constexpr int C = L::C, G = 64 / GP;
    const long long total = wave_bytes / 8;
    std::vector<int> owner((size_t)total, 0), padded((size_t)total, 0);
    const int off[11] = {L::cc, L::P, L::q, L::u, L::dua, L::rhs, L::c, L::lo, L::hi, L::tmp, L::wgt};
    const int len[11] = {C + 4, 4 * C, C, C, C, C, 2 * C, 2 * C, 2 * C, 2 * C, 2 * C};
    for (int g = 0; g < G; ++g)
        for (int a = 0; a < 11; ++a)
            for (int i = 0; i < len[a]; ++i) {
                const long long at = (long long)g * L::stride(max_obs) + off[a] + i;
                if (at < 0 || at >= total) return 1;
                if (owner[(size_t)at]) return 5;
                owner[(size_t)at] = g * 16 + a + 1;
            }
    for (int grp = 0; grp < G; ++grp) {
        const long long base = (long long)grp * L::stride(max_obs);
        int err = 0;
        // inside: this address belongs to the problem's own data (must not be padded); else it must be padded
        // the padding, through the list the kernel stores through (PathQpRowsLayout::pad_ranges)
        L::pad_ranges(N, ns, [&](int first, int last, double) {
            for (int i = first; i < last; ++i) {
                const long long at = base + i;
                if (at < base || at >= base + L::stride(max_obs) || at >= total) { if (!err) err = at < 0 || at >= total ? 1 : 2; continue; }
                padded[(size_t)at] = 1;
            }
        });
        if (err) return err;
        auto read = [&](int array_off, int i, bool in_problem) {
            const long long at = base + array_off + i;
            if (at < 0 || at >= total) { if (!err) err = 1; return; }
            if (at < base || at >= base + L::stride(max_obs)) { if (!err) err = 2; return; }
            if (in_problem && padded[(size_t)at]) { if (!err) err = 3; }
            if (!in_problem && !padded[(size_t)at]) { if (!err) err = 4; }
        };
        for (int gl = 0; gl < GP; ++gl) {
            const int b = gl * R;
            for (int i = 0; i < R + 2; ++i) {                                   // win: u, dua, rhs at b - 2 + i
                const int k = b - 2 + i;
                read(L::u, k, k >= 0 && k < N);
                read(L::dua, k, k >= 0 && k < N);
                read(L::rhs, k, k >= 0 && k < N);
                for (int f = 0; f < 2; ++f) {                                   // gather / ww: stations b .. b + R + 1
                    read(L::tmp, (b + i) * 2 + f, b + i < ns);
                    read(L::wgt, (b + i) * 2 + f, b + i < ns);
                }
            }
            for (int i = 0; i < R + 6; ++i) read(L::u, b - 3 + i, b - 3 + i >= 0 && b - 3 + i < N);      // ux
            for (int r = 0; r < R; ++r) {
                const int m = b + r;
                read(L::q, m, m < N);
                for (int d = 0; d < 4; ++d) read(L::P, m * 4 + d, m < N);
                for (int d = 1; d < 4; ++d) read(L::P, (m - d) * 4 + d, m - d >= 0 && m - d < N);
                for (int f = 0; f < 2; ++f) {
                    read(L::c, m * 2 + f, m < ns);
                    read(L::lo, m * 2 + f, m < ns);
                    read(L::hi, m * 2 + f, m < ns);
                }
            }
        }
        if (err) return err;
    }
    return 0;
}

}  // namespace

extern "C" {

int ql_offsets(int gp, int r, int max_obs, long long* out) {
    if (gp == 8 && r == 3) { offsets<8, 3>(max_obs, out); return 0; }
    if (gp == 8 && r == 4) { offsets<8, 4>(max_obs, out); return 0; }
    if (gp == 16 && r == 4) { offsets<16, 4>(max_obs, out); return 0; }
    return -1;
}

// bytes of dynamic LDS the launcher asks for (emp_api.hip, dev_cycle_qp: 64 / gp groups of cycle_qp_group_words doubles)
long long ql_wave_bytes(int gp, int r, int max_obs) {
    if (gp == 8 && r == 3) return (long long)PathQpRowsLayout<8, 3>::wave_bytes(max_obs);
    if (gp == 8 && r == 4) return (long long)PathQpRowsLayout<8, 4>::wave_bytes(max_obs);
    if (gp == 16 && r == 4) return (long long)PathQpRowsLayout<16, 4>::wave_bytes(max_obs);
    return -1;
}

int ql_replay(int gp, int r, int max_obs, int N, int ns, long long wave_bytes) {
    if (gp == 8 && r == 3) return replay<8, 3>(max_obs, N, ns, wave_bytes);
    if (gp == 8 && r == 4) return replay<8, 4>(max_obs, N, ns, wave_bytes);
    if (gp == 16 && r == 4) return replay<16, 4>(max_obs, N, ns, wave_bytes);
    return -1;
}

}  // extern "C"
