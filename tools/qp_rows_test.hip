// Check of band_chol_rows / band_solve_rows (R rows per lane on groups of 8 or 16 lanes, half bandwidth KD = 3 and 2,
// emp_qp_rows.h) and of the path QP's hand-unrolled pair band_chol_rows3 / band_solve_rows3 (HAND) against the scalar band_chol / band_solve of emp_qp_core.h on random SPD band matrices, with groups of
// different sizes - 0, 1, 2, KD and a full group among them - side by side in one wavefront.  Run by
// tests/test_gpu_band_solvers.py; exits non-zero on a HIP error, a relative error of 1e-11 or a NaN in a factor.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iemplanner_carla_amd/csrc tools/qp_rows_test.hip -o tools/_build/qrt
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "emp_qp_rows.h"
using namespace emp;

#define HIP_OK(call)                                                                                      \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                           \
            printf("HIP error %s at %s:%d: %s\nFAILED\n", hipGetErrorName(e_), __FILE__, __LINE__, #call); \
            exit(2);                                                                                      \
        }                                                                                                 \
    } while (0)

// band[(grp * 64 + j) * 4 + d] = A[j][j + d] of group grp; x and fac are indexed the same way
template <int GP, int R, int KD, bool HAND>
__global__ void k_rows(const double* band, const double* rhs, const int* Ns, double* x, int* okout, double* fac) {
    const int lane = threadIdx.x & 63, grp = lane / GP, gl = lane & (GP - 1);
    const int N = Ns[grp];
    double a[R][KD + 1], low[R][KD + 1], rinv[R], b[R];
    for (int r = 0; r < R; ++r) {
        const int j = gl * R + r;
        for (int d = 0; d <= KD; ++d) a[r][d] = (j < N && j + d < N) ? band[(grp * 64 + j) * 4 + d] : 0.0;
        b[r] = j < N ? rhs[grp * 64 + j] : 0.0;
    }
    const int steps = oct_wave_max<GP>((N + R - 1) / R);
    bool ok;
    if constexpr (HAND) {
        static_assert(KD == 3, "the hand-unrolled pair is the path QP's");
        ok = band_chol_rows3<GP, R>(a, rinv, low, N, gl, N > 0, steps);
        band_solve_rows3<R>(a, rinv, low, b, steps);
    } else {
        ok = band_chol_rows<GP, R, KD>(a, rinv, low, N, gl, N > 0, steps);
        band_solve_rows<R, KD>(a, rinv, low, b, steps);
    }
    for (int r = 0; r < R; ++r) {
        x[grp * 64 + gl * R + r] = b[r];
        for (int d = 0; d <= KD; ++d) fac[((grp * 64) + gl * R + r) * 4 + d] = a[r][d];
    }
    okout[lane] = ok;
}

template <int GP, int R, int KD, bool HAND>
int run(const int* hN) {
    static_assert(GP * R <= 64, "the arrays hold 64 rows a group");
    constexpr int NG = 64 / GP;
    static double hb[NG * 64 * 4], hr[NG * 64], ref[NG * 64], hx[NG * 64], hf[NG * 64 * 4];
    for (int i = 0; i < NG * 64 * 4; ++i) hb[i] = 0.0;
    for (int i = 0; i < NG * 64; ++i) hr[i] = ref[i] = 0.0;
    for (int g = 0; g < NG; ++g) {
        const int N = hN[g];
        double M[64 * (KD + 1)] = {0};
        for (int i = 0; i < N; ++i) {
            for (int d = 0; d <= KD; ++d) {
                double v = (d == 0) ? 1317.0 + (rand() % 100) : (d == 1) ? 510.0 : (d == 2) ? 82.0 : -0.48;
                if (i + d >= N) v = 0.0;
                hb[(g * 64 + i) * 4 + d] = v;
                M[i * (KD + 1) + d] = v;
            }
            hr[g * 64 + i] = (rand() % 2000) / 100.0 - 10.0;
            ref[g * 64 + i] = hr[g * 64 + i];
        }
        if (N && !band_chol<KD>(M, N)) { printf("scalar chol failed\n"); return 1; }
        if (N) band_solve<KD>(M, ref + g * 64, N);
    }
    double *db, *dr, *dx, *df;
    int *dN, *dok;
    HIP_OK(hipMalloc(&db, sizeof(hb)));
    HIP_OK(hipMalloc(&dr, sizeof(hr)));
    HIP_OK(hipMalloc(&dx, sizeof(hx)));
    HIP_OK(hipMalloc(&df, sizeof(hf)));
    HIP_OK(hipMalloc(&dN, NG * sizeof(int)));
    HIP_OK(hipMalloc(&dok, 64 * sizeof(int)));
    HIP_OK(hipMemcpy(db, hb, sizeof(hb), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dr, hr, sizeof(hr), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dN, hN, NG * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dx, 0, sizeof(hx)));
    HIP_OK(hipMemset(df, 0, sizeof(hf)));
    HIP_OK(hipMemset(dok, 0, 64 * sizeof(int)));
    hipLaunchKernelGGL((k_rows<GP, R, KD, HAND>), dim3(1), dim3(64), 0, 0, db, dr, dN, dx, dok, df);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    int hok[64];
    HIP_OK(hipMemcpy(hx, dx, sizeof(hx), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hf, df, sizeof(hf), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hok, dok, sizeof(hok), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(db)); HIP_OK(hipFree(dr)); HIP_OK(hipFree(dx)); HIP_OK(hipFree(df)); HIP_OK(hipFree(dN)); HIP_OK(hipFree(dok));
    double worst = 0;
    int nanfac = 0, oks = 0;
    for (int g = 0; g < NG; ++g) {
        oks += hok[g * GP];
        for (int i = 0; i < hN[g]; ++i) {
            const double e = fabs(hx[g * 64 + i] - ref[g * 64 + i]) / fmax(1.0, fabs(ref[g * 64 + i]));
            worst = (e == e) ? fmax(worst, e) : 1e300;
        }
        // every factor entry a lane of the group holds, the rows past the problem's end included
        for (int i = 0; i < GP * R * 4; ++i) nanfac += !(hf[g * 64 * 4 + i] == hf[g * 64 * 4 + i]);
    }
    printf("GP %d R %d KD %d%s N", GP, R, KD, HAND ? " by hand" : "");
    for (int g = 0; g < NG; ++g) printf(" %d", hN[g]);
    printf(": worst rel err %.3e, ok groups %d of %d, NaN factor entries %d\n", worst, oks, NG, nanfac);
    return (worst < 1e-11 && nanfac == 0 && oks == NG) ? 0 : 1;
}

template <int KD, bool HAND>
int run_all() {
    int bad = 0;
    { const int n[8] = {17, 17, 17, 17, 17, 17, 17, 17}; bad += run<8, 3, KD, HAND>(n); }
    { const int n[8] = {17, 1, 22, 0, 18, 3, 24, 9}; bad += run<8, 3, KD, HAND>(n); }
    { const int n[8] = {24, 24, 24, 24, 24, 24, 24, 24}; bad += run<8, 3, KD, HAND>(n); }
    { const int n[8] = {24, 1, 2, 0, 17, 3, 24, 9}; bad += run<8, 3, KD, HAND>(n); }
    { const int n[8] = {30, 17, 32, 1, 0, 29, 4, 31}; bad += run<8, 4, KD, HAND>(n); }
    { const int n[8] = {32, 2, 31, 1, 0, 29, 4, 32}; bad += run<8, 4, KD, HAND>(n); }
    { const int n[4] = {57, 64, 17, 0}; bad += run<16, 4, KD, HAND>(n); }
    { const int n[4] = {64, 2, 57, 0}; bad += run<16, 4, KD, HAND>(n); }
    return bad;
}

int main() {
    const int bad = run_all<3, false>() + run_all<2, false>() + run_all<3, true>();
    printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
