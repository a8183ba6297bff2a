// drive_clock_check.cpp - runs plan_drive_clock (csrc/emp_dp_launch.h: the clock of emp_drive_timed and its refusals) on the CPU
// for the `-m "not gpu"` suite.  TEST TOOL ONLY: compiled with g++ into a temporary directory by tests/test_drive_timed_host.py,
// never by the package.
#include "../../emplanner_carla_amd/csrc/emp_dp_launch.h"

extern "C" {

// -> 1 when the clock is refused; otherwise 0, *end = tick0 + K * T and ticks[k] = period k's first tick for k < min(K, n)
int dcc_clock(int tick0, int K, int T, long long* end, int* ticks, int n) {
    const emp::DriveClockPlan p = emp::plan_drive_clock(tick0, K, T);
    if (p.error) return 1;
    *end = p.end;
    for (int k = 0; k < K && k < n; ++k) ticks[k] = p.tick(k);
    return 0;
}

// the two clocks of period k's first tick as the kernels form them: t0 + (double)tick * dt, and that + plan_lead
void dcc_times(double t0, int tick, double dt, double plan_lead, double* out2) {
    const double clock = t0 + (double)tick * dt;
    out2[0] = clock;
    out2[1] = clock + plan_lead;
}

}  // extern "C"
