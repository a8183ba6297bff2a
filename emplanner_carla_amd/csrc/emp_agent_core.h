// emp_agent_core.h - the law that drives the reference's dynamic obstacle along a route, as plain functions that hipcc (the agent
// kernels, emp_agent_kernels.h) and g++ (tests/host_check/agent_check.cpp) both compile.  With no hazard in sight the reference's
// BehaviorAgent.run_step is LocalPlanner.run_step (agents/navigation/local_planner.py:208-260: purge the waypoint queue, take its
// head as the target) and VehiclePIDController.run_step (agents/navigation/controller.py:54-92: a longitudinal and a lateral PID,
// each over a deque of 10, the steering rate limit and the actuation clamps).  include/emplanner.h states the rule in full and what
// of the reference is not reproduced; tests/agent_port.py is the same in Python floats.
//
// Arithmetic contract as in emp_control_core.h: written order, separately rounded binary64 operations (-ffp-contract=off), IEEE `/`
// and sqrt; libm enters through acos (the law) and through sin and cos (observe) only.
#pragma once

#include "emp_core.h"      // EMP_HD

namespace emp {
namespace agt {

constexpr int kBuffer = 10;                    // EMP_AGENT_BUFFER: deque(maxlen=10), ref controller.py:124, :193
constexpr int kDone = 1;                       // EMP_AGT_DONE

struct Params {
    double lat_kp, lat_ki, lat_kd;             // ref local_planner.py:73: 1.95, 0.05, 0.2
    double lon_kp, lon_ki, lon_kd;             // ref :74: 1.0, 0.05, 0
    double dt;                                 // ref :70: 1 / 20
    double max_throttle, max_brake, max_steer; // ref :75-77: 0.75, 0.3, 0.8
    double base_min_distance;                  // ref :79: 3.0
};

// np.clip(v, -1.0, 1.0) = minimum(maximum(v, -1), 1): a NaN passes through, -0.0 stays -0.0
EMP_HD double clip1(double v) {
    if (v != v) return v;
    return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);
}

// A NaN enters a deque as THE quiet NaN, for the reason ctl::pid_step gives: IEEE 754 leaves a NaN result's sign open, and the one
// kernel and the chain of three are bit-for-bit equal.
EMP_HD double quiet(double v) { return (v != v) ? __builtin_nan("") : v; }

// One _pid_control call (ref controller.py:141-160, :243-251) on the deque `buf` (kBuffer doubles, oldest first, *n entries; a
// count outside [0, 10] is clamped), in place: `e` is appended, a full deque drops its oldest entry, entries at and past the new
// count stay as they are.  With at least 2 entries de = (e[-1] - e[-2]) / dt and ie = (sum from +0, oldest first) * dt, else both
// are 0.  Returns clip((kp e + kd de) + ki ie).  Every index is a constant once the loop is unrolled: a deque held in registers
// stays there.
EMP_HD double pid10(double kp, double ki, double kd, double dt, double e_in, double* buf, int* n) {
    const double e = quiet(e_in);
    const int n0 = *n < 0 ? 0 : (*n > kBuffer ? kBuffer : *n);
    const bool drop = n0 == kBuffer;
    const int m = n0 - (drop ? 1 : 0) + 1;     // entries after the append
    double sum = 0.0, prev = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < kBuffer; ++i) {
        const double v = (drop && i + 1 < kBuffer) ? buf[i + 1] : buf[i];      // read ahead of the write below
        if (i < m - 1) {
            sum = sum + v;
            prev = v;
            buf[i] = v;
        } else if (i == m - 1) {
            sum = sum + e;
            buf[i] = e;
        }
    }
    double de = 0.0, ie = 0.0;
    if (m >= 2) {
        de = (e - prev) / dt;
        ie = sum * dt;
    }
    *n = m;
    return clip1((kp * e + kd * de) + ki * ie);
}

// What the CARLA getters return for a vehicle of the project's model (emp_agent_observe): the forward vector, the world-frame
// velocity and get_speed's km/h (ref agents/tools/misc.py:32-41).
struct Obs {
    double c, s, wx, wy, kmh;
};
EMP_HD Obs observe(double fi, double Vy, double Vx) {
    Obs o;
    o.c = cos(fi);
    o.s = sin(fi);
    o.wx = Vx * o.c - Vy * o.s;
    o.wy = Vx * o.s + Vy * o.c;
    o.kmh = 3.6 * sqrt((o.wx * o.wx + o.wy * o.wy) + 0.0);
    return o;
}

// An agent between two ticks.  lon / lat point at its two deques (kBuffer doubles each, any memory); (px, py) is path[at] while
// at >= 0: the head waypoint is loaded again only when `head` has moved.
struct Agent {
    int head, n_lon, n_lat;
    double past_steer;
    double* lon;
    double* lat;
    int at;
    double px, py;
};

struct Tick {
    double throttle, steer, brake;
    double lat_error, lon_command;             // the signed angle and the clipped longitudinal command; 0 in a DONE tick
    int status;
};

EMP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

EMP_HD void head_point(const double* path, Agent& a) {
    if (a.at != a.head) {
        a.px = path[4 * (size_t)a.head];
        a.py = path[4 * (size_t)a.head + 1];
        a.at = a.head;
    }
}

// One tick of one agent at (x, y) with forward vector (c, s): `path` is its [n_path][4] rows (n_path already clamped to the row),
// a.head in [0, n_path].
EMP_HD Tick tick(const Params& p, const double* path, int n_path, double x, double y, double c, double s, double speed_kmh,
                 double target_speed, Agent& a) {
    // 1. purge (ref local_planner.py:224-243)
    const double min_distance = p.base_min_distance + 0.5 * (speed_kmh / 3.6);
    while (a.head < n_path) {
        head_point(path, a);
        const double md = (n_path - a.head == 1) ? 1.0 : min_distance;
        const double dx = x - a.px, dy = y - a.py;
        if (sqrt(dx * dx + dy * dy) < md) ++a.head;        // a NaN distance compares false: the purge stops
        else break;
    }
    Tick k;
    // 2. empty queue (ref :246-252): the controller is not called
    if (a.head >= n_path) {
        k.throttle = 0.0;
        k.steer = 0.0;
        k.brake = 1.0;
        k.lat_error = 0.0;
        k.lon_command = 0.0;
        k.status = kDone;
        return k;
    }
    // 3. longitudinal PID (ref controller.py:141-160)
    const double acc = pid10(p.lon_kp, p.lon_ki, p.lon_kd, p.dt, target_speed - speed_kmh, a.lon, &a.n_lon);
    // 4. lateral PID (ref :207-251) and actuation (ref :68-90)
    const double wx = a.px - x, wy = a.py - y;
    const double nn = sqrt(wx * wx + wy * wy) * sqrt((c * c + s * s) + 0.0);
    double dot;
    if (nn == 0.0) dot = 1.0;                               // the reference's own value: one radian
    else dot = acos(clip1(((wx * c + wy * s) + 0.0) / nn));
    if (c * wy - s * wx < 0.0) dot = -dot;
    dot = quiet(dot);
    double cs = pid10(p.lat_kp, p.lat_ki, p.lat_kd, p.dt, dot, a.lat, &a.n_lat);
    if (cs > a.past_steer + 0.1) cs = a.past_steer + 0.1;
    else if (cs < a.past_steer - 0.1) cs = a.past_steer - 0.1;
    // Python's min(a, b) / max(a, b) keep `a` unless b is strictly smaller / larger: a NaN cs gives -max_steer, a NaN acc
    // throttle 0 and a NaN brake
    if (cs >= 0.0) k.steer = (cs < p.max_steer) ? cs : p.max_steer;
    else k.steer = (cs > -p.max_steer) ? cs : -p.max_steer;
    if (acc >= 0.0) {
        k.throttle = (p.max_throttle < acc) ? p.max_throttle : acc;
        k.brake = 0.0;
    } else {
        const double aa = fabs(acc);
        k.throttle = 0.0;
        k.brake = (p.max_brake < aa) ? p.max_brake : aa;
    }
    a.past_steer = k.steer;
    k.lat_error = dot;
    k.lon_command = acc;
    k.status = 0;
    return k;
}

}  // namespace agt
}  // namespace emp
