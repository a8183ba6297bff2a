// emp_control_core.h - the longitudinal PID step and the actuation mapping of the reference's Vehicle_control, and the
// project's vehicle model (vehicle_step, below) and its rule for sampling a timed trajectory (speed_target), as plain functions
// that hipcc (device code of the fused control and rollout kernels) and g++ (tests/host_check/control_check.cpp,
// tests/host_check/vehicle_check.cpp, tests/host_check/speed_target_check.cpp) both compile.
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
// A NaN error enters the buffer as THE quiet NaN (0x7ff8000000000000): IEEE 754 leaves the sign of a NaN result open and the
// compiler may carry the negation of `target - speed` across an operation, so the stored NaN had either sign bit depending on the
// kernel this function was inlined into (emp_rollout's against emp_vehicle_control's, LQR) - and the two are bit-for-bit equal.
EMP_HD double pid_step(const PidParams& p, double speed_kmh, double target_speed, const double* in, int n_in, double* out,
                       int* n_out) {
    const double diff = target_speed - speed_kmh;
    const double e = (diff != diff) ? __builtin_nan("") : diff;
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

// ---------------------------------------------------------------------------------------------------------------------------
// The PID's target from a timed trajectory (emp_speed_target / emp_rollout_timed).  THE RULE IS THE PROJECT'S: the reference plans
// the 401-point profile (speed_planning_test.py:517, "control runs 10x as often as planning") and then drives with a constant
// ref_speed (test_10.py:554).  include/emplanner.h states the rule in full; tests/speed_target_port.py is its port.  Only + - * /
// and comparisons: g++ and the device give the same bits.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kTimedPoints = 401;              // EMP_TIMED_POINTS: increase_points' samples (ref speed_planning_test.py:517)
constexpr int kTgtBefore = 1, kTgtPast = 2, kTgtNoProfile = 4, kTgtCapped = 8;     // EMP_TGT_*

// n_v: the number of leading samples in which neither the time nor the speed is NaN
EMP_HD int profile_count(const double* speed, const double* time) {
    int n = 0;
    while (n < kTimedPoints && !(time[n] != time[n]) && !(speed[n] != speed[n])) ++n;
    return n;
}

// the clock of tick `tick`: the product is rounded, then the sum
EMP_HD double tick_clock(double t0, int tick, double dt) { return t0 + (double)tick * dt; }

// One tick's target in km/h from rows speed[0..n_v) (m/s) and time[0..n_v) (s).  *cursor is the bracket the last tick used (any
// int: it is clamped) and receives this tick's; *bits receives this tick's EMP_TGT_* bits.
EMP_HD double speed_target(const double* speed, const double* time, int n_v, double clock, double cap, int* cursor, int* bits) {
    if (n_v <= 0 || clock != clock) {
        if (n_v <= 0) *cursor = 0;
        *bits = kTgtNoProfile;
        return cap;
    }
    int b = 0;
    double v;
    if (clock < time[0]) {
        v = speed[0];
        b = kTgtBefore;
    } else if (clock >= time[n_v - 1]) {
        v = speed[n_v - 1];
        b = kTgtPast;
    } else {                                   // time[0] <= clock < time[n_v - 1]: n_v >= 2
        int j = *cursor;
        j = j < 0 ? 0 : (j > n_v - 2 ? n_v - 2 : j);
        while (j + 1 <= n_v - 2 && time[j + 1] <= clock) ++j;
        const double tj = time[j], sj = speed[j];
        const double d = time[j + 1] - tj;
        v = sj;
        if (d > 0.0) {
            const double w = (clock - tj) / d;
            v = sj + w * (speed[j + 1] - sj);
        }
        *cursor = j;
    }
    double target = 3.6 * v;
    if (target > cap) {
        target = cap;
        b |= kTgtCapped;
    }
    *bits = b;
    return target;
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

// ---------------------------------------------------------------------------------------------------------------------------
// The vehicle model of emp_vehicle_step / emp_rollout.  THIS IS THE PROJECT'S DEFINITION, NOT THE REFERENCE'S: the reference has
// no vehicle model (CARLA's physics is its plant).  It is the dynamic bicycle model that the controllers' own cal_A_B_C_fun
// (ref controller.py:115-148) linearises, stepped with the bilinear rule the controllers discretise it with (:159-165), so the
// plant and the controllers' prediction agree by construction.  Same arithmetic contract as above: written order, separately
// rounded operations, IEEE `/`; only the pose uses libm (sin, cos) and speed_kmh sqrt.
// ---------------------------------------------------------------------------------------------------------------------------
struct VehicleParams {
    double a, b, Cf, Cr, m, Iz;                // vehicle_para as the controllers unpack it (ref :132)
    double dt;                                 // tick (0.01: the PID's)
    double steer_gain;                         // wheel angle [rad] per unit steer (1: the MPC treats u as the wheel angle)
    double throttle_accel, brake_decel, drag;  // m/s^2 per unit throttle / brake; 1/s
};

struct VehicleState {
    double x, y, fi, Vy, fi_dot, Vx;           // pose, body-frame lateral velocity, yaw rate, body-frame longitudinal velocity
};

// cal_vehicle_info's sign-preserving clamp |Vx| >= 0.005 (ref :106-109), Python's max(a, b): `a` unless b is strictly larger
EMP_HD double clamp_vx(double Vx) {
    if (Vx < 0.0) {
        const double av = fabs(Vx);
        return -((0.005 > av) ? 0.005 : av);
    }
    return (0.005 > Vx) ? 0.005 : Vx;
}

// 3.6 * |velocity| as the PID reads it (ref :647-649), from the body-frame components
EMP_HD double speed_kmh_of(double Vx, double Vy) { return 3.6 * sqrt(Vx * Vx + Vy * Vy); }

// One tick.  delta = steer_gain * steer; ax = throttle_accel * throttle - brake_decel * brake - drag * Vx.  The lateral pair
// z = (Vy, fi_dot) solves (I - dt/2 A) z+ = (I + dt/2 A) z + dt * bv * delta by Cramer's rule, with
//   A = [[(Cf+Cr)/(m Vxc), (a Cf - b Cr)/(m Vxc) - Vxc], [(a Cf - b Cr)/(Iz Vxc), (a^2 Cf + b^2 Cr)/(Iz Vxc)]], Vxc = clamp_vx(Vx),
//   bv = (-Cf/m, -a Cf/Iz)
// (A-stable: no speed makes the step blow up where the continuous model decays).  The pose steps from the OLD values; Vx+ =
// max(Vx + dt * ax, 0): the model does not reverse (a NaN speed becomes 0).
EMP_HD VehicleState vehicle_step(const VehicleParams& p, const VehicleState& s, double throttle, double steer, double brake) {
    const double delta = p.steer_gain * steer;
    const double ax = (p.throttle_accel * throttle - p.brake_decel * brake) - p.drag * s.Vx;
    const double Vxc = clamp_vx(s.Vx);
    const double a11 = (p.Cf + p.Cr) / (p.m * Vxc);
    const double a12 = (p.a * p.Cf - p.b * p.Cr) / (p.m * Vxc) - Vxc;
    const double a21 = (p.a * p.Cf - p.b * p.Cr) / (p.Iz * Vxc);
    const double a22 = (p.a * p.a * p.Cf + p.b * p.b * p.Cr) / (p.Iz * Vxc);
    const double bv1 = -p.Cf / p.m, bv2 = -p.a * p.Cf / p.Iz;
    const double h = p.dt / 2.0;
    const double m11 = h * a11, m12 = h * a12, m21 = h * a21, m22 = h * a22;
    const double l11 = 1.0 - m11, l12 = -m12, l21 = -m21, l22 = 1.0 - m22;
    const double r1 = ((1.0 + m11) * s.Vy + m12 * s.fi_dot) + (p.dt * bv1) * delta;
    const double r2 = (m21 * s.Vy + (1.0 + m22) * s.fi_dot) + (p.dt * bv2) * delta;
    const double det = l11 * l22 - l12 * l21;
    VehicleState n;
    n.Vy = (r1 * l22 - l12 * r2) / det;
    n.fi_dot = (l11 * r2 - l21 * r1) / det;
    const double c = cos(s.fi), sn = sin(s.fi);
    n.x = s.x + p.dt * (s.Vx * c - s.Vy * sn);
    n.y = s.y + p.dt * (s.Vx * sn + s.Vy * c);
    n.fi = s.fi + p.dt * s.fi_dot;
    const double v = s.Vx + p.dt * ax;
    n.Vx = (v > 0.0) ? v : 0.0;
    return n;
}

}  // namespace ctl
}  // namespace emp
