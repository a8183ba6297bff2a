// vehicle_check.cpp - runs the vehicle model of csrc/emp_control_core.h (ctl::vehicle_step, the arithmetic of emp_vehicle_step
// and emp_rollout) on the CPU for the `-m "not gpu"` suite.  TEST TOOL ONLY: compiled with g++ -ffp-contract=off into a
// temporary directory by tests/test_rollout_host.py, never by the package.
#include "../../emplanner_carla_amd/csrc/emp_control_core.h"

using namespace emp;

extern "C" {

// n vehicles, one tick each: prm11 = a, b, Cf, Cr, m, Iz, dt, steer_gain, throttle_accel, brake_decel, drag; state [n][6],
// control [n][3] = throttle, steer, brake; out [n][6] (may be `state`), ctl_out [n][3] = clamped Vx+, speed_kmh, 0 (or NULL).
void vc_step(const double* prm11, int n, const double* state, const double* control, double* out, double* ctl_out) {
    const ctl::VehicleParams p{prm11[0], prm11[1], prm11[2], prm11[3], prm11[4], prm11[5], prm11[6], prm11[7], prm11[8], prm11[9],
                               prm11[10]};
    for (int i = 0; i < n; ++i) {
        const double* s = state + 6 * i;
        const ctl::VehicleState nx = ctl::vehicle_step(p, ctl::VehicleState{s[0], s[1], s[2], s[3], s[4], s[5]}, control[3 * i],
                                                       control[3 * i + 1], control[3 * i + 2]);
        double* o = out + 6 * i;
        o[0] = nx.x; o[1] = nx.y; o[2] = nx.fi; o[3] = nx.Vy; o[4] = nx.fi_dot; o[5] = nx.Vx;
        if (ctl_out) {
            ctl_out[3 * i] = ctl::clamp_vx(nx.Vx);
            ctl_out[3 * i + 1] = ctl::speed_kmh_of(nx.Vx, nx.Vy);
            ctl_out[3 * i + 2] = 0.0;
        }
    }
}

}  // extern "C"
