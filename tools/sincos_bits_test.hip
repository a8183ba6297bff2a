// The Frenet helpers form cos and sin of one angle with a single sincos (emp_frenet_core.h: sincos_pair) where they used to call
// cos(x) and sin(x) one after the other.  This program compares the device's sincos(x) with its sin(x) and cos(x) by bit pattern
// (NaN equal to NaN) on 2^30 operands and a few thousand special ones:
//   - an even sweep of [-4 pi, 4 pi], the headings the planner sees,
//   - a hashed sweep of bit patterns: the exponent field runs through all 2048 values in turn (denormals, the large-argument
//     reduction, inf / NaN among them), sign and mantissa come from splitmix64,
//   - denormals of either sign, +-0, +-inf, NaN, the largest and the smallest normal numbers, multiples of pi / 2 and their neighbours.
// Prints the number of operands on which either result differs in any bit; 0 expected.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math tools/sincos_bits_test.hip -o /tmp/scb && /tmp/scb
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

// The separate calls, each in a function of its own that is not inlined: whatever the compiler does with a sin and a cos of the
// same argument side by side, these two stay what a lone call is.
__device__ __attribute__((noinline)) double lone_sin(double x) { return sin(x); }
__device__ __attribute__((noinline)) double lone_cos(double x) { return cos(x); }

__device__ inline bool same_bits(double a, double b) {
    if (a != a && b != b) return true;
    return __double_as_longlong(a) == __double_as_longlong(b);
}

__device__ inline bool differs(double x) {
    double s, c;
    sincos(x, &s, &c);
    return !(same_bits(s, lone_sin(x)) && same_bits(c, lone_cos(x)));
}

__device__ inline unsigned long long splitmix64(unsigned long long i) {
    unsigned long long z = i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void check(unsigned long long per_thread, unsigned long long* bad, unsigned long long* done, unsigned long long* example) {
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long total = (unsigned long long)gridDim.x * blockDim.x * per_thread;
    const double four_pi = 12.566370614359172;
    unsigned long long mine = 0;
    for (unsigned long long k = 0; k < per_thread; ++k) {
        const unsigned long long i = tid * per_thread + k;
        const double even = -four_pi + ((double)i + 0.5) * (2.0 * four_pi / (double)total);
        const unsigned long long z = splitmix64(i);
        const unsigned long long bits = (z & 0x800FFFFFFFFFFFFFull) | ((i & 2047ull) << 52);
        const double hashed = __longlong_as_double((long long)bits);
        if (differs(even)) {
            ++mine;
            *example = (unsigned long long)__double_as_longlong(even);
        }
        if (differs(hashed)) {
            ++mine;
            *example = bits;
        }
    }
    if (mine) atomicAdd(bad, mine);
    if (threadIdx.x == 0) atomicAdd(done, 1ull);      // the host checks that every block ran to its end
}

// one operand per thread from a list the host wrote
__global__ void check_list(int n, const double* x, unsigned long long* bad, unsigned long long* done, unsigned long long* example) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && differs(x[t])) {
        atomicAdd(bad, 1ull);
        *example = (unsigned long long)__double_as_longlong(x[t]);
    }
    if (threadIdx.x == 0) atomicAdd(done, 1ull);
}

#define CHECK(call)                                                                        \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            printf("%s failed: %s\n", #call, hipGetErrorString(e_));                       \
            return 2;                                                                      \
        }                                                                                  \
    } while (0)

static double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}

int main() {
    // special operands
    constexpr int kMaxList = 16384;
    static double list[kMaxList];
    int n = 0;
    const uint64_t fixed[] = {0x0000000000000000ull, 0x8000000000000000ull, 0x7FF0000000000000ull, 0xFFF0000000000000ull,
                              0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, 0x7FFFFFFFFFFFFFFFull,
                              0x0000000000000001ull, 0x8000000000000001ull, 0x000FFFFFFFFFFFFFull, 0x800FFFFFFFFFFFFFull,
                              0x0010000000000000ull, 0x8010000000000000ull, 0x7FEFFFFFFFFFFFFFull, 0xFFEFFFFFFFFFFFFFull};
    for (uint64_t b : fixed) list[n++] = from_bits(b);
    uint64_t z = 1;
    for (int i = 0; i < 2048; ++i) {                 // denormals: every width of mantissa, hashed bits, either sign
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t m = (z >> 12) >> (i % 52);
        list[n++] = from_bits((m ? m : 1) | ((uint64_t)(i & 1) << 63));
    }
    for (int q = -1024; q <= 1024; ++q) {            // multiples of pi / 2 as binary64 and their two neighbours
        const double v = (double)q * 1.5707963267948966;
        uint64_t b;
        memcpy(&b, &v, 8);
        list[n++] = v;
        if (q != 0) {
            list[n++] = from_bits(b - 1);
            list[n++] = from_bits(b + 1);
        }
    }
    unsigned long long *bad, *done, *example;
    double* dlist;
    CHECK(hipMalloc(&bad, 8));
    CHECK(hipMalloc(&done, 8));
    CHECK(hipMalloc(&example, 8));
    CHECK(hipMalloc(&dlist, sizeof(double) * n));
    CHECK(hipMemset(bad, 0, 8));
    CHECK(hipMemset(done, 0, 8));         // a kernel that never ran cannot read as "0 differences": `done` counts its blocks
    CHECK(hipMemset(example, 0, 8));
    CHECK(hipMemcpy(dlist, list, sizeof(double) * n, hipMemcpyHostToDevice));
    const unsigned long long per_thread = 1ull << 9;
    const unsigned blocks = 1u << 12, list_blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(check, dim3(blocks), dim3(256), 0, 0, per_thread, bad, done, example);
    CHECK(hipGetLastError());
    hipLaunchKernelGGL(check_list, dim3(list_blocks), dim3(256), 0, 0, n, dlist, bad, done, example);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    unsigned long long h = ~0ull, d = 0, ex = 0;
    CHECK(hipMemcpy(&h, bad, 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&d, done, 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&ex, example, 8, hipMemcpyDeviceToHost));
    if (d != blocks + list_blocks) {
        printf("only %llu of %u blocks ran\n", d, blocks + list_blocks);
        return 2;
    }
    if (h) printf("one differing operand: 0x%016llx\n", ex);
    printf("operands checked: %llu, sincos differing from sin / cos: %llu\n", 2ull * blocks * 256 * per_thread + (unsigned long long)n, h);
    return h != 0;
}
