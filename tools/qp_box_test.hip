// Check of the interior-point fallbacks of the smoothing QP, box_qp_lanes<32> and smooth_pair_lanes (emp_qp_wave.h), called
// directly: the active-set solver in front of them settles on every test and benchmark scene, so nothing else runs this code.
// <32, 1>: box_qp_lanes<32>, two unrelated problems in the two halves of a wavefront (sizes 2, 3, 5, 31, 32, unlike sizes side by
// side, an empty half beside a live one); <64, 2>: smooth_pair_lanes, an x and a y problem with different data in the same lanes
// (sizes 2, 33, 63, 64).  Boxes of
// 0.2 (the slacks start shifted) and 1.5 (they do not); references that are nearly smooth, zig-zag at the box size, noise of
// three boxes, every point twice.  Checked: status 0, every coordinate inside its box to 1e-12, agreement with box_qp_setup +
// RangeQp::solve_scalar on the host to kHostTol, an x problem solved beside a y problem has the bits it has beside a copy of
// itself, and m < 2 or thr <= 0 return 2 with the reference untouched.  Run by tests/test_gpu_band_solvers.py; exits non-zero
// on a HIP error or a failed check.  `--dump` prints every result in hex (to compare two builds of the header bit for bit; the
// two QP_BOX_CALL macros can be set on the command line to the call names of another revision).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iemplanner_carla_amd/csrc tools/qp_box_test.hip -o tools/_build/qbt
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "emp_qp_wave.h"
using namespace emp;

#ifndef QP_BOX_CALL_32      // (double r, int m, SmoothQpParams prm, double (&out)[1], int* iters)
#define QP_BOX_CALL_32(r, m, prm, out, it) box_qp_lanes<32>(r, m, prm, &(out)[0], it)
#endif
#ifndef QP_BOX_CALL_64      // (double rx, double ry, int m, SmoothQpParams sx, sy, double (&out)[2], int* iters)
#define QP_BOX_CALL_64(rx, ry, m, sx, sy, out, it) smooth_pair_lanes(rx, ry, m, sx, sy, &(out)[0], &(out)[1], it)
#endif

// Largest deviation from the host's scalar solver that is accepted, in metres: ten times the largest one measured on these
// cases, 7.788e-9 m (profiles/ipm_step/README.md; the factor is headroom for another summation order).  That is more than two
// solvers that stop at a primal residual of 1e-10 should differ by, and the cause is known: the fallbacks still stop at
// mu <= 1e-13, box_qp_forms' rule of old, where the host's box_qp_forms now asks 1e-16 - at 1e-13 a point beside a weakly active
// bound stops 1e-8 m from the minimiser (emp_qp_core.h, box_qp_forms).  Inherited, like the rest of the stopping rules.
constexpr double kHostTol = 7.8e-8;

#define HIP_OK(call)                                                                                      \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                           \
            printf("HIP error %s at %s:%d: %s\nFAILED\n", hipGetErrorName(e_), __FILE__, __LINE__, #call); \
            exit(2);                                                                                      \
        }                                                                                                 \
    } while (0)

template <class T>
static T* to_device(const T* host, size_t count) {          // a device copy (zeros if host == nullptr)
    T* dev = nullptr;
    HIP_OK(hipMalloc(&dev, count * sizeof(T)));
    if (host) HIP_OK(hipMemcpy(dev, host, count * sizeof(T), hipMemcpyHostToDevice));
    else HIP_OK(hipMemset(dev, 0, count * sizeof(T)));
    return dev;
}
template <class T>
static void from_device(T* host, T* dev, size_t count) {    // copy back and free
    HIP_OK(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(dev));
}

// One problem: m points of one coordinate, its box.  A wavefront solves two: the halves of <32, 1>, or x and y of <64, 2>.
struct Problem {
    int m;
    SmoothQpParams prm;
    double ref[64];
};
struct Result {
    double out[64];
    int rc, iters;
};

// block b: problems 2b (lanes 0-31) and 2b + 1 (lanes 32-63)
__global__ void k_box32(const Problem* pr, Result* res) {
    const int lane = threadIdx.x & 63, grp = lane >> 5, gl = lane & 31;
    const Problem& P = pr[2 * blockIdx.x + grp];
    const double r = gl < P.m ? P.ref[gl] : 0.0;
    double out[1] = {r};
    int iters = 0;
    const int rc = QP_BOX_CALL_32(r, P.m, P.prm, out, &iters);
    Result& R = res[2 * blockIdx.x + grp];
    R.out[gl] = out[0];
    if (gl == 0) {
        R.rc = rc;
        R.iters = iters;
    }
}
// block b: problems 2b (x) and 2b + 1 (y), of the same size, in the same lanes; one status and iteration count for both
__global__ void k_box64(const Problem* pr, Result* res) {
    const int lane = threadIdx.x & 63;
    const Problem &X = pr[2 * blockIdx.x], &Y = pr[2 * blockIdx.x + 1];
    const int m = X.m;
    const double rx = lane < m ? X.ref[lane] : 0.0, ry = lane < m ? Y.ref[lane] : 0.0;
    double out[2] = {rx, ry};
    int iters = 0;
    const int rc = QP_BOX_CALL_64(rx, ry, m, X.prm, Y.prm, out, &iters);
    for (int p = 0; p < 2; ++p) {
        Result& R = res[2 * blockIdx.x + p];
        R.out[lane] = out[p];
        if (lane == 0) {
            R.rc = rc;
            R.iters = iters;
        }
    }
}

static unsigned long long g_seed = 77;
static double uniform() {                                   // in [-1, 1)
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_seed >> 11) / 4503599627370496.0 - 1.0;
}
// kind 0 nearly smooth (no bound active), 1 zig-zag at the box size, 2 noise of three boxes, 3 every point twice
static Problem problem(int m, int kind, double thr, bool is_y) {
    Problem P;
    memset(&P, 0, sizeof P);
    P.m = m;
    P.prm = SmoothQpParams{0.4, 0.3, 0.3, thr};             // emp_smooth_params_default
    const double box = fabs(thr) > 0.0 ? fabs(thr) : 0.2;
    for (int i = 0; i < m && i < 64; ++i) {
        const int j = (kind == 3) ? i / 2 : i;
        const double t = 2.0 * j, base = is_y ? 8.0 * sin(t / 25.0) : t;
        double dev = 0.0;
        if (kind == 0) dev = 0.1 * box * uniform();
        else if (kind == 1) dev = 1.0000001 * box * (((is_y ? i / 2 : i) & 1) ? -1.0 : 1.0);
        else if (kind == 2) dev = 3.0 * box * uniform();
        P.ref[i] = base + dev;
    }
    return P;
}

static double g_worst_host = 0.0;
// the checks of one live problem; returns the number of failures
static int check(const char* tag, int id, const Problem& P, const Result& R) {
    int bad = 0;
    if (P.m < 2 || !(P.prm.thr > 0.0)) {                    // nothing to solve: 2, reference untouched
        bad += R.rc != 2;
        for (int i = 0; i < P.m; ++i) bad += R.out[i] != P.ref[i];
        if (bad) printf("%s %d: m %d thr %g must return 2 and the reference, got rc %d\n", tag, id, P.m, P.prm.thr, R.rc);
        return bad;
    }
    if (R.rc != 0) {
        printf("%s %d: m %d thr %g status %d after %d iterations\n", tag, id, P.m, P.prm.thr, R.rc, R.iters);
        return 1;
    }
    BoxRangeQp Q;
    std::vector<double> mem(BoxRangeQp::words(P.m, P.m), 0.0);
    Q.bind(mem.data(), P.m, P.m);
    if (box_qp_setup(Q, P.ref, 1, P.m, P.prm) != 0 || Q.solve_scalar() != 0) {
        printf("%s %d: the host solver failed\n", tag, id);
        return 1;
    }
    double out_of_box = 0.0, dev = 0.0;
    for (int i = 0; i < P.m; ++i) {
        const double o = R.out[i];
        out_of_box = (o == o) ? fmax(out_of_box, fabs(o - P.ref[i]) - P.prm.thr) : 1e300;
        dev = (o == o) ? fmax(dev, fabs(o - Q.u[i])) : 1e300;
    }
    g_worst_host = fmax(g_worst_host, dev);
    if (out_of_box > 1e-12 || dev > kHostTol) {
        printf("%s %d: m %d thr %g: %.3e outside the box, %.3e from the host solver (%d / %d iterations)\n", tag, id, P.m, P.prm.thr,
               out_of_box, dev, R.iters, Q.iters);
        bad = 1;
    }
    return bad;
}

static void dump(const char* tag, const std::vector<Problem>& pr, const std::vector<Result>& res) {
    for (size_t k = 0; k < pr.size(); ++k) {
        printf("%s %zu m %d rc %d iters %d:", tag, k, pr[k].m, res[k].rc, res[k].iters);
        for (int i = 0; i < pr[k].m; ++i) {
            unsigned long long bits;
            memcpy(&bits, &res[k].out[i], 8);
            printf(" %016llx", bits);
        }
        printf("\n");
    }
}

template <class K>
static std::vector<Result> solve(K kernel, const std::vector<Problem>& pr) {
    std::vector<Result> res(pr.size());
    Problem* dp = to_device(pr.data(), pr.size());
    Result* dr = to_device<Result>(nullptr, pr.size());
    hipLaunchKernelGGL(kernel, dim3((unsigned)pr.size() / 2), dim3(64), 0, 0, dp, dr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    from_device(res.data(), dr, pr.size());
    HIP_OK(hipFree(dp));
    return res;
}

int main(int argc, char** argv) {
    const bool want_dump = argc > 1 && !strcmp(argv[1], "--dump");
    const double thrs[2] = {0.2, 1.5};
    int bad = 0;

    // ---- <32, 1>: every (size, kind, box) once; its neighbour in the wavefront is an unrelated problem of another size
    std::vector<Problem> spec;
    const int m32[5] = {2, 3, 5, 31, 32};
    for (int a = 0; a < 5; ++a)
        for (int kind = 0; kind < 4; ++kind)
            for (int b = 0; b < 2; ++b) spec.push_back(problem(m32[a], kind, thrs[b], (kind + b) & 1));
    std::vector<Problem> p32;
    for (size_t k = 0; k < spec.size(); ++k) {
        p32.push_back(spec[k]);
        p32.push_back(spec[(k * 7 + 11) % spec.size()]);
    }
    const Problem small = problem(2, 2, 0.2, false), full = problem(32, 2, 0.2, true);
    const Problem pairs[][2] = {{small, full},
                                {full, small},
                                {problem(0, 0, 0.2, false), full},          // an empty half beside a live one
                                {full, problem(0, 0, 0.2, false)},
                                {problem(1, 0, 0.2, false), full},
                                {full, problem(5, 1, 0.0, true)},           // no box: nothing to solve
                                {problem(31, 2, -1.0, false), full}};
    for (const auto& pp : pairs) {
        p32.push_back(pp[0]);
        p32.push_back(pp[1]);
    }
    const std::vector<Result> r32 = solve(k_box32, p32);
    for (size_t k = 0; k < p32.size(); ++k) bad += check("<32, 1>", (int)k, p32[k], r32[k]);

    // ---- <64, 2>: x and y with different data (and, in every other case, different boxes); then x beside x and y beside y
    std::vector<Problem> p64;
    const int m64[4] = {2, 33, 63, 64};
    for (int a = 0; a < 4; ++a)
        for (int kind = 0; kind < 4; ++kind)
            for (int b = 0; b < 2; ++b) {
                p64.push_back(problem(m64[a], kind, thrs[b], false));
                p64.push_back(problem(m64[a], (kind + 1 + b) & 3, thrs[(b + kind) & 1], true));
            }
    const size_t mixed = p64.size();
    for (size_t k = 0; k < mixed; ++k) {                    // problem k beside a copy of itself: blocks mixed / 2 + k
        p64.push_back(p64[k]);
        p64.push_back(p64[k]);
    }
    const Problem none[][2] = {{problem(1, 0, 0.2, false), problem(1, 0, 0.2, true)},
                               {problem(0, 0, 0.2, false), problem(0, 0, 0.2, true)},
                               {problem(33, 2, 0.0, false), problem(33, 2, 0.2, true)},
                               {problem(64, 1, 0.2, false), problem(64, 1, -1.0, true)}};
    const size_t none_at = p64.size();
    for (const auto& pp : none) {
        p64.push_back(pp[0]);
        p64.push_back(pp[1]);
    }
    const std::vector<Result> r64 = solve(k_box64, p64);
    for (size_t k = 0; k < none_at; ++k) bad += check("<64, 2>", (int)k, p64[k], r64[k]);
    for (size_t k = none_at; k < p64.size(); ++k) {         // one status for the pair: 2, both references untouched
        int b2 = r64[k].rc != 2;
        for (int i = 0; i < p64[k].m; ++i) b2 += r64[k].out[i] != p64[k].ref[i];
        if (b2) printf("<64, 2> %zu: a pair with nothing to solve must return 2 and the references, got rc %d\n", k, r64[k].rc);
        bad += b2;
    }
    int unlike = 0;
    for (size_t k = 0; k < mixed; ++k) {
        const Result& twin = r64[mixed + 2 * k + (k & 1)];  // the same slot (x or y) of the pair of copies
        unlike += memcmp(r64[k].out, twin.out, sizeof(double) * p64[k].m) != 0;
    }
    if (unlike) printf("<64, 2>: %d problems differ in bits from their solve beside a copy of themselves\n", unlike);
    bad += unlike;

    if (want_dump) {
        dump("<32, 1>", p32, r32);
        dump("<64, 2>", p64, r64);
    }
    printf("%zu + %zu problems, largest deviation from the host solver %.3e m (accepted %.1e)\n", p32.size(), p64.size(), g_worst_host,
           kHostTol);
    printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
