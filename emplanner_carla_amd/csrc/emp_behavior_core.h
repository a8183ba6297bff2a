// emp_behavior_core.h - the car-following law of the reference's BehaviorAgent.run_step (agents/navigation/behavior_agent.py), as
// plain functions that hipcc (emp_behavior_kernels.h) and g++ (tests/host_check/behavior_check.cpp) both compile: the speed-limit
// target, the vehicle-ahead detector (_vehicle_obstacle_detected: lane test, distance, the 30 degree cone), the time-to-collision
// rule (car_following_manager) and the emergency stop, on top of agt::tick (emp_agent_core.h), which it calls unchanged.
// include/emplanner.h states the rule in full and what of the reference is not reproduced; tests/behavior_port.py is the same in
// Python floats.
//
// Arithmetic contract as in emp_agent_core.h: written order, separately rounded binary64 operations, IEEE `/` and sqrt; libm enters
// through the detector's acos (and through agt::tick's).
#pragma once

#include "emp_agent_core.h"

namespace emp {
namespace bhv {

constexpr int kMaxWorld = 64;                  // EMP_TRAFFIC_MAX_WORLD: agents of a world, and others of a world
enum Mode { kNormal = 0, kSlow = 1, kFollow = 2, kClear = 3, kEmergency = 4, kDone = 5 };      // EMP_BHV_*
constexpr int kCountedModes = 5;               // mode_ticks: every mode but DONE

struct Params {
    double max_speed, speed_lim_dist, speed_decrease, safety_time, min_proximity_threshold, braking_distance;   // behavior_types.py
    double min_speed;                          // BehaviorAgent._min_speed: 5
    double emergency_brake;                    // BasicAgent._max_brake: 0.5
    double up_angle;                           // the detector's cone, degrees: 30
    int look_steps;                            // get_incoming_waypoint_and_direction(steps=5)
};

// Python's min(a, b) and max(a, b): `a` unless b is strictly smaller / larger (a NaN b never is)
EMP_HD double pymin(double a, double b) { return b < a ? b : a; }
EMP_HD double pymax(double a, double b) { return b > a ? b : a; }

constexpr double kEps = 2.220446049250313e-16;         // np.finfo(float).eps = 2^-52 (misc.py:161)
constexpr double kRadToDeg = 57.29577951308232;        // 180 / pi as math.degrees multiplies

// is_within_distance(target, ego, th, [0, up_angle]) (misc.py:66-103) for the vector (tvx, tvy) from the ego to the target
EMP_HD bool within(const Params& p, double th, double c, double s, double tvx, double tvy) {
    const double norm = sqrt(tvx * tvx + tvy * tvy);
    if (norm < 0.001) return true;
    if (norm > th) return false;
    const double angle = acos(agt::clip1((c * tvx + s * tvy) / norm)) * kRadToDeg;
    return 0.0 < angle && angle < p.up_angle;           // a NaN angle (a NaN norm passes both tests above) is no hit
}

// The same arithmetic with the cone as an argument (emp_hazard_core.h: 90 degrees for a traffic light, 60 for a walker)
EMP_HD bool within(double up_angle, double th, double c, double s, double tvx, double tvy) {
    const double norm = sqrt(tvx * tvx + tvy * tvy);
    if (norm < 0.001) return true;
    if (norm > th) return false;
    const double angle = acos(agt::clip1((c * tvx + s * tvy) / norm)) * kRadToDeg;
    return 0.0 < angle && angle < up_angle;
}

// The vehicles an agent may see, as the start of the tick left them.  Agents: n_agents slots of ax / ay / akmh / aext / akey (the
// agent's own slot `self` is passed over); others: n_others rows of other[5] = x, y, vx, vy, half extent with keys okey, moved to
// time tau.  Any memory: LDS in the kernels.
struct Scene {
    int self, n_agents, n_others;
    const double *ax, *ay, *akmh, *aext;
    const int* akey;
    const double* other;
    const int* okey;
    double tau;
};

struct Out {
    agt::Tick k;
    int mode, blocker;                         // blocker: position in the scan order, -1 if none
    double distance, ttc, target;              // +inf where the rule does not compute them
};

EMP_HD double infinity() { return __builtin_inf(); }

// One tick of one agent at (x, y) with forward vector (c, s): `path` / `lane` are its rows (n_path already clamped to the row),
// a.head in [0, n_path].
EMP_HD Out behave(const agt::Params& ap, const Params& p, const double* path, const int* lane, int n_path, double x, double y, double c,
                  double s, double kmh, double limit, double extent, const Scene& sc, agt::Agent& a) {
    Out o;
    o.blocker = -1;
    o.distance = o.ttc = infinity();
    if (a.head >= n_path) {                    // the reference raises here (_incoming_waypoint is None): defined as the DONE tick
        o.k.throttle = 0.0; o.k.steer = 0.0; o.k.brake = 1.0;
        o.k.lat_error = 0.0; o.k.lon_command = 0.0;
        o.k.status = agt::kDone;
        o.mode = kDone;
        o.target = limit;
        return o;
    }
    const double th = pymax(p.min_proximity_threshold, limit / 3.0);
    const int key_cur = lane[a.head - 1 < 0 ? 0 : a.head - 1];
    const int ahead = a.head + p.look_steps;
    const int key_next = lane[agt::clampi(ahead, 0, n_path - 1)];
    // the scan: the first hit wins, kept by predicate so that the lanes of a wavefront stay together; acos runs only for a candidate
    // that passed the key and distance tests
    int blocker = -1;
    for (int j = 0; j < sc.n_agents; ++j) {
        const int key = sc.akey[j];
        if (blocker < 0 && j != sc.self && key >= 0 && (key == key_cur || key == key_next) &&
            within(p, th, c, s, sc.ax[j] - x, sc.ay[j] - y))
            blocker = j;
    }
    bool is_other = false;
    for (int q = 0; q < sc.n_others; ++q) {
        const int key = sc.okey[q];
        const double* r = sc.other + 5 * q;
        if (blocker < 0 && key >= 0 && (key == key_cur || key == key_next) &&
            within(p, th, c, s, (r[0] + r[2] * sc.tau) - x, (r[1] + r[3] * sc.tau) - y)) {
            blocker = q;
            is_other = true;
        }
    }
    const double normal = pymin(p.max_speed, limit - p.speed_lim_dist);
    int ticks = 1;                             // agent ticks of this tick
    if (blocker < 0) {
        o.mode = kNormal;
        o.target = normal;
    } else {
        double xj, yj, vs, ext_j;
        if (is_other) {
            const double* r = sc.other + 5 * blocker;
            xj = r[0] + r[2] * sc.tau;
            yj = r[1] + r[3] * sc.tau;
            vs = 3.6 * sqrt((r[2] * r[2] + r[3] * r[3]) + 0.0);
            ext_j = r[4];
            o.blocker = sc.n_agents - (sc.self >= 0 && sc.self < sc.n_agents ? 1 : 0) + blocker;
        } else {
            xj = sc.ax[blocker];
            yj = sc.ay[blocker];
            vs = sc.akmh[blocker];
            ext_j = sc.aext[blocker];
            o.blocker = blocker - (sc.self >= 0 && blocker > sc.self ? 1 : 0);
        }
        const double dx = x - xj, dy = y - yj;
        const double d = ((sqrt((dx * dx + dy * dy) + 0.0) + kEps) - ext_j) - extent;      // compute_distance, less the two extents
        o.distance = d;
        if (d < p.braking_distance) {              // emergency_stop(): a fresh control; the local planner is not called
            o.k.throttle = 0.0; o.k.steer = 0.0; o.k.brake = p.emergency_brake;
            o.k.lat_error = 0.0; o.k.lon_command = 0.0;
            o.k.status = 0;
            o.mode = kEmergency;
            o.target = limit;                      // _update_information's set_speed(speed_limit) stands
            return o;
        }
        const double dv = pymax(1.0, (kmh - vs) / 3.6);
        const double ttc = d / dv;
        o.ttc = ttc;
        if (p.safety_time > ttc && ttc > 0.0) {
            const double v = vs - p.speed_decrease;
            o.mode = kSlow;
            o.target = pymin(pymin(v > 0.0 ? v : 0.0, p.max_speed), limit - p.speed_lim_dist);
        } else if (2.0 * p.safety_time > ttc && ttc >= p.safety_time) {
            o.mode = kFollow;
            o.target = pymin(pymin(pymax(p.min_speed, vs), p.max_speed), limit - p.speed_lim_dist);
        } else {
            o.mode = kClear;
            o.target = normal;
        }
        // The reference steps its local planner in car_following_manager and once more at the end of run_step (behavior_agent.py:275,
        // :284, :292, then :360): two ticks on one observation.  The second purge finds nothing to do, both deques take the error
        // twice, the rate limit applies twice; the second control is the one returned.
        ticks = 2;
    }
    // (one call site: agt::tick is inlined once, and the kernels need no stack)
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int r = 0; r < ticks; ++r) o.k = agt::tick(ap, path, n_path, x, y, c, s, kmh, o.target, a);
    return o;
}

// The lane key a vehicle shows to the others: the key of the waypoint behind its queue's head, -1 without a plan.
EMP_HD int shown_key(const int* lane, int n_path, int head) {
    if (n_path <= 0) return -1;
    return lane[head - 1 < 0 ? 0 : head - 1];
}

}  // namespace bhv
}  // namespace emp
