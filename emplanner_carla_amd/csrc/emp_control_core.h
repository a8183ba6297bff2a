// emp_control_core.h - the longitudinal PID step and the actuation mapping of the reference's Vehicle_control, as plain
// functions that hipcc (device code of the fused control kernels) and g++ (tests/host_check/control_check.cpp) both compile.
// ref: controller/controller.py class Longitudinal_PID_controller (:614-678) and Vehicle_control.run_step (:680-724).
//
// Arithmetic contract: bit-exact with the reference's Python floats.  Every expression is evaluated in the written order with
// separately rounded IEEE-754 binary64 operations: compile with -ffp-contract=off (build.py does) and include this header
// outside any `#pragma clang fp contract(fast)` region (emp_qp_wave.h opens one and closes it at its end).  `/` is IEEE
// division here (no v_rcp_f64 seed).
#pragma once

#include "emp_core.h"      // EMP_HD

namespace emp {
namespace ctl {

constexpr int kPidBuffer = 60;                 // deque(maxlen=60), ref :637
constexpr int kPidChunk = 12;                  // entries loaded at once by pid_step (a fifth of the buffer)

struct PidParams {
    double kp, ki, kd, dt, error_threshold;    // ref :622-638: 1.15, 0, 0, 0.01, 1
};

// One PID_fun call (ref :641-672) on one vehicle's error buffer `in` (oldest first, n_in entries; a count outside [0, 60]
// is clamped).  Writes the buffer after the call to `out` (may be the same array as `in`: entries are read before the slot
// they land in is written) and its length to *n_out; the entries of `out` at and past *n_out are 0.  Returns the command
// K_P e + K_I i + K_D d.
//   - the error is appended BEFORE the separation test; a full buffer drops its oldest entry (deque maxlen)
//   - fewer than 2 entries: integral and derivative 0; else integral = sum(oldest..newest) * dt (a left-to-right sum, as
//     Python's sum over the deque), derivative = (newest - previous) / dt
//   - |e| > error_threshold: the integral is 0 and the buffer is cleared; the derivative term stays
// dt = 0 gives IEEE inf / NaN where the reference raises ZeroDivisionError.
EMP_HD double pid_step(const PidParams& p, double speed_kmh, double target_speed, const double* in, int n_in, double* out,
                       int* n_out) {
    const double e = target_speed - speed_kmh;
    const int n = n_in < 0 ? 0 : (n_in > kPidBuffer ? kPidBuffer : n_in);
    const int drop = (n == kPidBuffer) ? 1 : 0;
    const int m = n - drop + 1;                // entries after the append
    // The kept entries move in chunks: a chunk's loads are issued together before its stores (one memory round trip per chunk
    // instead of one per entry; `in` and `out` may alias, so a store may not pass a later load).  Reads run ahead of writes
    // (index i + drop >= i), which is what makes the aliased form safe.
    double sum = 0.0, prev = 0.0;
    for (int c0 = 0; c0 + 1 < m; c0 += kPidChunk) {
        double v[kPidChunk];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < kPidChunk; ++j) v[j] = (c0 + j + 1 < m) ? in[c0 + j + drop] : 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < kPidChunk; ++j)
            if (c0 + j + 1 < m) {
                sum = sum + v[j];
                out[c0 + j] = v[j];
                prev = v[j];
            }
    }
    sum = sum + e;
    double integral = 0.0, differential = 0.0;
    if (m >= 2) {
        integral = sum * p.dt;
        differential = (e - prev) / p.dt;
    }
    int keep = m;
    out[m - 1] = e;
    if (fabs(e) > p.error_threshold) {
        integral = 0.0;
        keep = 0;
    }
    for (int i = keep; i < kPidBuffer; ++i) out[i] = 0.0;
    *n_out = keep;
    return (p.kp * e + p.ki * integral) + p.kd * differential;
}

// Actuation of Vehicle_control.run_step (ref :705-718) with the reference's limits (max steer 1, min steer -1, max throttle 1,
// max brake 1).  Python's min(a, b) / max(a, b) return `a` unless `b` is strictly smaller / larger, so a NaN steering command
// gives -1 and a NaN acceleration throttle 0, brake 1; -0.0 takes the >= 0 branches.  brake = max(1, acc) for acc < 0 is
// always 1: the reference's own expression, kept.
EMP_HD void actuate(double steer_cmd, double acc_cmd, double* throttle, double* steer, double* brake) {
    if (steer_cmd >= 0.0) *steer = (steer_cmd < 1.0) ? steer_cmd : 1.0;
    else *steer = (steer_cmd > -1.0) ? steer_cmd : -1.0;
    if (acc_cmd >= 0.0) {
        *throttle = (acc_cmd < 1.0) ? acc_cmd : 1.0;
        *brake = 0.0;
    } else {
        *throttle = 0.0;
        *brake = (acc_cmd > 1.0) ? acc_cmd : 1.0;
    }
}

}  // namespace ctl
}  // namespace emp
