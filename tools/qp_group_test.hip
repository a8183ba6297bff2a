// Check of the one-row-per-lane sweeps of emp_qp_wave.h against the scalar band_chol / band_solve of emp_qp_core.h on
// random SPD band matrices: band_chol_group / band_solve_group on both groups of a wavefront, band_chol_group_n /
// band_solve_group_n with two different problems in the same lanes, and the group reductions.  Run by
// tests/test_gpu_band_solvers.py; exits non-zero on a HIP error or a relative error of 1e-11.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iemplanner_carla_amd/csrc tools/qp_group_test.hip -o tools/_build/qgt
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "emp_qp_wave.h"
using namespace emp;

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
static void launched() {
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
}

// a random SPD band matrix of N rows (like the path-QP Hessian: not far from losing diagonal dominance) and a right-hand
// side: the band at stride 4 for the device, and the scalar solver's solution
template <int KD>
static bool problem(int N, double* band4, double* rhs, double* ref) {
    double M[64 * (KD + 1)] = {0};
    for (int i = 0; i < N; ++i) {
        for (int d = 0; d <= KD; ++d) {
            double v = (d == 0) ? 1317.0 + (rand() % 100) : (d == 1) ? 510.0 : (d == 2) ? 82.0 : -0.48;
            if (i + d >= N) v = 0.0;
            band4[i * 4 + d] = v;
            M[i * (KD + 1) + d] = v;
        }
        rhs[i] = (rand() % 2000) / 100.0 - 10.0;
        ref[i] = rhs[i];
    }
    if (!band_chol<KD>(M, N)) { printf("scalar chol failed\n"); return false; }
    band_solve<KD>(M, ref, N);
    return true;
}
static double worst_err(const double* x, const double* ref, int N) {
    double worst = 0;
    for (int i = 0; i < N; ++i) {
        const double e = fabs(x[i] - ref[i]) / fmax(1.0, fabs(ref[i]));
        worst = (e == e) ? fmax(worst, e) : 1e300;
    }
    return worst;
}

template <int G, int KD>
__global__ void k_test(const double* band, const double* rhs, const int* Ns, double* x, double* shifts, int* okout) {
    const int lane = threadIdx.x & 63, grp = lane / G, gl = lane & (G - 1);
    const int N = Ns[grp];
    double a[KD + 1], low[KD + 1], rinv;
    for (int d = 0; d <= KD; ++d) a[d] = gl < N ? band[(grp * 64 + gl) * 4 + d] : 0.0;
    const bool ok = band_chol_group<G, KD>(a, rinv, low, N, gl, true);
    double b = gl < N ? rhs[grp * 64 + gl] : 0.0;
    band_solve_group<G, KD>(a, rinv, low, b, N, gl);
    x[lane] = b;
    okout[lane] = ok;
    shifts[lane] = lane_up1((double)lane);
    shifts[64 + lane] = lane_dn1((double)lane);
}

template <int G, int KD>
int run(int N0, int N1) {
    double hb[2 * 64 * 4] = {0}, hr[2 * 64] = {0}, ref[2 * 64] = {0};
    int hN[2] = {N0, N1};
    for (int g = 0; g < 64 / G; ++g)
        if (!problem<KD>(hN[g], hb + g * 64 * 4, hr + g * 64, ref + g * 64)) return 1;
    double *db = to_device(hb, 2 * 64 * 4), *dr = to_device(hr, 2 * 64), *dx = to_device<double>(nullptr, 64),
           *ds = to_device<double>(nullptr, 128);
    int *dN = to_device(hN, 2), *dok = to_device<int>(nullptr, 64);
    hipLaunchKernelGGL((k_test<G, KD>), dim3(1), dim3(64), 0, 0, db, dr, dN, dx, ds, dok);
    launched();
    double hx[64], hs[128]; int hok[64];
    from_device(hx, dx, 64); from_device(hs, ds, 128); from_device(hok, dok, 64);
    HIP_OK(hipFree(db)); HIP_OK(hipFree(dr)); HIP_OK(hipFree(dN));
    double worst = 0;
    for (int g = 0; g < 64 / G; ++g) worst = fmax(worst, worst_err(hx + g * G, ref + g * 64, hN[g]));
    printf("G %d KD %d N %d/%d: worst rel err %.3e, ok flags %d %d; up1[0..2] %.0f %.0f %.0f up1[32] %.0f dn1[0] %.0f dn1[63] %.0f\n",
           G, KD, N0, N1, worst, hok[0], hok[63], hs[0], hs[1], hs[2], hs[32], hs[64], hs[127]);
    return worst < 1e-11 ? 0 : 1;
}

// NP problems of the same size in the same lanes: band[(p * 64 + gl) * 4 + d], rhs[p * 64 + gl]
template <int G, int KD, int NP>
__global__ void k_test_n(const double* band, const double* rhs, int N, double* x, double* rinv_out, int* okout) {
    const int lane = threadIdx.x & 63, gl = lane & (G - 1);
    double a[NP][KD + 1], low[NP][KD + 1], rinv[NP], b[NP];
    bool active[NP];
    for (int p = 0; p < NP; ++p) {
        for (int d = 0; d <= KD; ++d) a[p][d] = gl < N ? band[(p * 64 + gl) * 4 + d] : 0.0;
        b[p] = gl < N ? rhs[p * 64 + gl] : 0.0;
        active[p] = true;
    }
    const bool ok = band_chol_group_n<G, KD, NP>(a, rinv, low, N, gl, active);
    band_solve_group_n<G, KD, NP>(a, rinv, low, b, N, gl);
    for (int p = 0; p < NP; ++p) {
        x[p * 64 + lane] = b[p];
        rinv_out[p * 64 + lane] = rinv[p];
    }
    okout[lane] = ok;
}

template <int G, int KD, int NP>
int run_n(int N) {
    static_assert(G == 64, "one group a wavefront");
    double hb[NP * 64 * 4] = {0}, hr[NP * 64] = {0}, ref[NP * 64] = {0};
    for (int p = 0; p < NP; ++p)                         // (rand() goes on: every problem gets another matrix)
        if (!problem<KD>(N, hb + p * 64 * 4, hr + p * 64, ref + p * 64)) return 1;
    double *db = to_device(hb, NP * 64 * 4), *dr = to_device(hr, NP * 64), *dx = to_device<double>(nullptr, NP * 64),
           *dri = to_device<double>(nullptr, NP * 64);
    int* dok = to_device<int>(nullptr, 64);
    hipLaunchKernelGGL((k_test_n<G, KD, NP>), dim3(1), dim3(64), 0, 0, db, dr, N, dx, dri, dok);
    launched();
    double hx[NP * 64], hri[NP * 64]; int hok[64];
    from_device(hx, dx, NP * 64); from_device(hri, dri, NP * 64); from_device(hok, dok, 64);
    HIP_OK(hipFree(db)); HIP_OK(hipFree(dr));
    int bad = hok[0] ? 0 : 1;
    printf("G %d KD %d NP %d N %d: ok flag %d;", G, KD, NP, N, hok[0]);
    for (int p = 0; p < NP; ++p) {
        const double worst = worst_err(hx + p * 64, ref + p * 64, N);
        int marked = 0;                                   // rinv <= 0 is the family's mark of a failed pivot
        for (int i = 0; i < N; ++i) marked += !(hri[p * 64 + i] > 0.0);
        printf(" problem %d worst rel err %.3e, marked pivots %d;", p, worst, marked);
        bad += (worst < 1e-11 && marked == 0) ? 0 : 1;
    }
    printf("\n");
    return bad ? 1 : 0;
}

__global__ void k_red(const double* v, double* out) {
    const double x = v[threadIdx.x];
    out[threadIdx.x] = group_max<32>(x);
    out[64 + threadIdx.x] = group_min<32>(x);
    out[128 + threadIdx.x] = group_sum<32>(x);
    out[192 + threadIdx.x] = group_max<64>(x);
    out[256 + threadIdx.x] = group_sum<64>(x);
}

static int test_reductions() {
    double h[64], o[320];
    for (int i = 0; i < 64; ++i) h[i] = (rand() % 2001) - 1000;            // integers: sums are exact in any order
    double *dv = to_device(h, 64), *dout = to_device<double>(nullptr, 320);
    hipLaunchKernelGGL(k_red, dim3(1), dim3(64), 0, 0, dv, dout);
    launched();
    from_device(o, dout, 320);
    HIP_OK(hipFree(dv));
    int bad = 0;
    for (int g = 0; g < 2; ++g) {
        double mx = -1e300, mn = 1e300, sm = 0;
        for (int i = 0; i < 32; ++i) { mx = fmax(mx, h[g * 32 + i]); mn = fmin(mn, h[g * 32 + i]); sm += h[g * 32 + i]; }
        for (int i = 0; i < 32; ++i) bad += (o[g * 32 + i] != mx) + (o[64 + g * 32 + i] != mn) + (o[128 + g * 32 + i] != sm);
    }
    double mx = -1e300, sm = 0;
    for (int i = 0; i < 64; ++i) { mx = fmax(mx, h[i]); sm += h[i]; }
    for (int i = 0; i < 64; ++i) bad += (o[192 + i] != mx) + (o[256 + i] != sm);
    printf("group reductions: %d mismatches\n", bad);
    return bad ? 1 : 0;
}

int main() {
    int bad = test_reductions();
    bad += run<32, 3>(17, 17);
    bad += run<32, 3>(32, 5);
    bad += run<32, 3>(1, 30);
    bad += run<32, 2>(32, 19);
    bad += run<64, 3>(17, 0);
    bad += run<64, 3>(64, 0);
    bad += run<64, 2>(41, 0);
    bad += run_n<64, 2, 2>(41);
    bad += run_n<64, 2, 2>(64);
    bad += run_n<64, 2, 2>(2);
    printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
