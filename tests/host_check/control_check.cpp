// control_check.cpp - runs csrc/emp_control_core.h (the PID step and the actuation of the fused vehicle-control kernels) on the
// CPU for the `-m "not gpu"` suite.  TEST TOOL ONLY: compiled with g++ -ffp-contract=off into a temporary directory by
// tests/test_control_host.py, never by the package.
#include "../../emplanner_carla_amd/csrc/emp_control_core.h"

using namespace emp;

extern "C" {

// One PID_control call; buffer in / out as emp_pid_longitudinal (in may equal out).
double cc_pid_step(const double* prm5, double speed_kmh, double target, const double* in, int n_in, double* out, int* n_out) {
    const ctl::PidParams p{prm5[0], prm5[1], prm5[2], prm5[3], prm5[4]};
    return ctl::pid_step(p, speed_kmh, target, in, n_in, out, n_out);
}

void cc_actuate(double steer_cmd, double acc_cmd, double* out3) { ctl::actuate(steer_cmd, acc_cmd, &out3[0], &out3[1], &out3[2]); }

int cc_pid_buffer(void) { return ctl::kPidBuffer; }

}  // extern "C"
