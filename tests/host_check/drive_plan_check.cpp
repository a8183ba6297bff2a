// drive_plan_check.cpp - runs plan_drive_request (csrc/emp_dp_launch.h: the launch geometry of the fleet loop's wave-per-vehicle
// kernels) on the CPU for the `-m "not gpu"` suite.  TEST TOOL ONLY: compiled with g++ into a temporary directory by
// tests/test_drive_host.py, never by the package.
#include "../../emplanner_carla_amd/csrc/emp_dp_launch.h"

extern "C" {

// out4 = wpb, grid, block, refused (0 / 1)
void dpc_plan(int B, int* out4) {
    const emp::DriveRequestPlan p = emp::plan_drive_request(B);
    out4[0] = p.wpb;
    out4[1] = p.grid;
    out4[2] = p.block;
    out4[3] = p.error ? 1 : 0;
}

}  // extern "C"
