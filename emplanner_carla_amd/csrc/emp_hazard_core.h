// emp_hazard_core.h - the two checks the reference's BehaviorAgent.run_step (agents/navigation/behavior_agent.py:312-328) runs before
// car-following, as plain functions that hipcc (emp_hazard_kernels.h) and g++ (tests/host_check/hazard_check.cpp) both compile:
// red lights (traffic_light_manager -> BasicAgent._affected_by_traffic_light, basic_agent.py:201-249, with the sticky
// _last_traffic_light) and pedestrians (pedestrian_avoid_manager, :225-251: the 10 m filter, the lane test, the 60 degree cone),
// then bhv::behave (emp_behavior_core.h), called unchanged.  include/emplanner.h states the rule in full and what of the reference is
// not reproduced; tests/hazard_port.py is the same in Python floats.
//
// Arithmetic contract as in emp_behavior_core.h: written order, separately rounded binary64 operations, IEEE `/` and sqrt; libm
// enters through acos only.  The light's phase is int64 arithmetic on the tick index: nothing accumulates.
#pragma once

#include "emp_behavior_core.h"

namespace emp {
namespace hz {

constexpr int kMaxLight = 64;                  // EMP_HAZARD_MAX: lights of a world, and walkers of a world
constexpr int kMaxWalker = 64;
enum Cause { kNone = 0, kLight = 1, kWalker = 2, kVehicle = 3 };       // EMP_HZ_*
constexpr int kCountedCauses = 3;              // cause_ticks: light, walker, vehicle

struct Params {
    double tlight_threshold;                   // BasicAgent._base_tlight_threshold: 5
    double tlight_up_angle;                    // basic_agent.py:245: 90
    double walker_radius;                      // behavior_agent.py:239: 10
    double walker_up_angle;                    // :249: 60
};

// What of a world is not a vehicle, as the tick finds it.  light[4] = x, y, dx, dy of the trigger waypoint, light_cycle[3] = period,
// red_from, red_to; walker[5] = x, y, vx, vy, half extent, moved to time tau.  Any memory: LDS in the kernels.
struct Scene {
    int n_light, n_walker;
    const double* light;
    const int* light_key;
    const int* light_cycle;
    const double* walker;
    const int* walker_key;
    long long k;                               // the tick index tick0 + t
    double tau;                                // k * dt
};

struct Out {
    bhv::Out b;
    int cause, light_hit, walker_hit;          // indices into the world's rows, -1 if none
    double walker_distance;                    // +inf if none
};

// traffic_light.state == Red at tick k
EMP_HD bool is_red(const int* cycle, long long k) {
    const long long period = cycle[0];
    if (period < 1) return false;
    const long long ph = k % period;
    return (long long)cycle[1] <= ph && ph < (long long)cycle[2];
}

// emergency_stop(): a fresh control; the local planner is not called and the agent state stays
EMP_HD void emergency(const bhv::Params& p, double limit, bhv::Out& o) {
    o.k.throttle = 0.0; o.k.steer = 0.0; o.k.brake = p.emergency_brake;
    o.k.lat_error = 0.0; o.k.lon_command = 0.0;
    o.k.status = 0;
    o.mode = bhv::kEmergency;
    o.target = limit;
    o.blocker = -1;
    o.distance = o.ttc = bhv::infinity();
}

// _affected_by_traffic_light: the index of the light that holds the agent, -1 if none; last_light is updated.
EMP_HD int light_scan(const Params& hp, const double* path, const int* lane, int n_path, int head, double x, double y, double c, double s,
                      const Scene& sc, int& last_light) {
    if (last_light < 0 || last_light >= sc.n_light) last_light = -1;
    if (last_light >= 0) {
        if (is_red(sc.light_cycle + 3 * last_light, sc.k)) return last_light;      // no geometry is looked at
        last_light = -1;
    }
    const int at = head - 1 < 0 ? 0 : head - 1;
    const int key_cur = lane[at];
    double vex = 0.0, vey = 0.0;               // the ego lane waypoint's forward vector: only the sign of its dot product counts
    if (n_path >= 2) {
        const int i0 = at < n_path - 2 ? at : n_path - 2;
        vex = path[4 * (i0 + 1)] - path[4 * i0];
        vey = path[4 * (i0 + 1) + 1] - path[4 * i0 + 1];
    }
    int hit = -1;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int q = 0; q < sc.n_light; ++q) {
        const int key = sc.light_key[q];
        const double* r = sc.light + 4 * q;
        if (hit < 0 && key >= 0 && key == key_cur && !(vex * r[2] + vey * r[3] < 0.0) && is_red(sc.light_cycle + 3 * q, sc.k) &&
            bhv::within(hp.tlight_up_angle, hp.tlight_threshold, c, s, r[0] - x, r[1] - y))
            hit = q;
    }
    if (hit >= 0) last_light = hit;
    return hit;
}

// pedestrian_avoid_manager: the index of the first walker seen, -1 if none; d is its distance less the two extents.
EMP_HD int walker_scan(const Params& hp, const bhv::Params& p, const double* path, const int* lane, int n_path, int head, double x,
                       double y, double c, double s, double limit, double extent, const Scene& sc, double& d) {
    const int at = head - 1 < 0 ? 0 : head - 1;
    const double px = path[4 * at], py = path[4 * at + 1];         // the ego's lane waypoint
    const double th = bhv::pymax(p.min_proximity_threshold, limit / 3.0);
    const int key_cur = lane[at];
    const int key_next = lane[agt::clampi(head + p.look_steps, 0, n_path - 1)];
    int hit = -1;
    double hx = 0.0, hy = 0.0, hext = 0.0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int q = 0; q < sc.n_walker; ++q) {
        const int key = sc.walker_key[q];
        const double* r = sc.walker + 5 * q;
        const double wx = r[0] + r[2] * sc.tau, wy = r[1] + r[3] * sc.tau;
        const double ex = wx - px, ey = wy - py;
        if (hit < 0 && sqrt((ex * ex + ey * ey) + 0.0) < hp.walker_radius && key >= 0 && (key == key_cur || key == key_next) &&
            bhv::within(hp.walker_up_angle, th, c, s, wx - x, wy - y)) {
            hit = q;
            hx = wx; hy = wy; hext = r[4];
        }
    }
    d = bhv::infinity();
    if (hit >= 0) {
        const double dx = x - hx, dy = y - hy;
        d = ((sqrt((dx * dx + dy * dy) + 0.0) + bhv::kEps) - hext) - extent;
    }
    return hit;
}

// One tick of one agent: steps 0 to 2 of the rule, then bhv::behave.  Arguments as bhv::behave's, plus the lights and walkers and
// the agent's sticky light.
EMP_HD Out behave(const agt::Params& ap, const bhv::Params& p, const Params& hp, const double* path, const int* lane, int n_path, double x,
                  double y, double c, double s, double kmh, double limit, double extent, const bhv::Scene& vsc, const Scene& sc,
                  agt::Agent& a, int& last_light) {
    Out o;
    o.cause = kNone;
    o.light_hit = o.walker_hit = -1;
    o.walker_distance = bhv::infinity();
    bool stop = false;
    if (a.head < n_path) {                     // the DONE tick is bhv::behave's: the reference raises before it looks at a light
        o.light_hit = light_scan(hp, path, lane, n_path, a.head, x, y, c, s, sc, last_light);
        if (o.light_hit >= 0) {
            o.cause = kLight;
            stop = true;
        } else {
            o.walker_hit = walker_scan(hp, p, path, lane, n_path, a.head, x, y, c, s, limit, extent, sc, o.walker_distance);
            if (o.walker_hit >= 0 && o.walker_distance < p.braking_distance) {
                o.cause = kWalker;
                stop = true;
            }                                  // a walker seen farther off is ignored, as in the reference
        }
    }
    if (stop) {
        emergency(p, limit, o.b);
        return o;
    }
    o.b = bhv::behave(ap, p, path, lane, n_path, x, y, c, s, kmh, limit, extent, vsc, a);
    if (o.b.mode == bhv::kEmergency) o.cause = kVehicle;
    return o;
}

}  // namespace hz
}  // namespace emp
