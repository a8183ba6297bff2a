// agent_check.cpp - runs csrc/emp_agent_core.h (the agents' law: purge, two PIDs over deques of 10, rate limit, actuation, and the
// observation that stands in for the CARLA getters) on the CPU for the `-m "not gpu"` suite: the very functions the agent kernels
// compile, one agent at a time, with ctl::vehicle_step as the plant of the rollout.  TEST TOOL ONLY: compiled with g++
// -ffp-contract=off into a temporary directory by tests/test_agent_host.py, never by the package.  With -DAGENT_CHECK_MAIN it is a
// program of its own (a corner path driven to its end, the rollout against the chain of ticks) that a sanitizer build can run.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../emplanner_carla_amd/csrc/emp_agent_core.h"
#include "../../emplanner_carla_amd/csrc/emp_control_core.h"
#include "../../include/emplanner.h"

using namespace emp;

static agt::Params params_of(const emp_agent_params* p) {
    return agt::Params{p->lat_K_P, p->lat_K_I, p->lat_K_D, p->lon_K_P, p->lon_K_I, p->lon_K_D, p->dt, p->max_throttle, p->max_brake,
                       p->max_steer, p->base_min_distance};
}
static ctl::VehicleParams vehicle_of(const emp_vehicle_params* p) {
    return ctl::VehicleParams{p->a, p->b, p->Cf, p->Cr, p->m, p->Iz, p->dt, p->steer_gain, p->throttle_accel, p->brake_decel, p->drag};
}

// the agent of row a as the kernels load it: the two deques copied to lon / lat
static agt::Agent load(int a, int n_path, const int* head, const double* past, const double* lon_in, const int* n_lon, const double* lat_in,
                       const int* n_lat, double* lon, double* lat) {
    agt::Agent g;
    g.head = agt::clampi(head[a], 0, n_path);
    g.n_lon = agt::clampi(n_lon[a], 0, agt::kBuffer);
    g.n_lat = agt::clampi(n_lat[a], 0, agt::kBuffer);
    g.past_steer = past[a];
    g.lon = lon;
    g.lat = lat;
    g.at = -1;
    g.px = g.py = 0.0;
    memcpy(lon, lon_in + (size_t)a * agt::kBuffer, sizeof(double) * agt::kBuffer);
    memcpy(lat, lat_in + (size_t)a * agt::kBuffer, sizeof(double) * agt::kBuffer);
    return g;
}
static void store(int a, const agt::Agent& g, int* head, double* past, double* lon, int* n_lon, double* lat, int* n_lat) {
    head[a] = g.head;
    past[a] = g.past_steer;
    n_lon[a] = g.n_lon;
    n_lat[a] = g.n_lat;
    memcpy(lon + (size_t)a * agt::kBuffer, g.lon, sizeof(double) * agt::kBuffer);
    memcpy(lat + (size_t)a * agt::kBuffer, g.lat, sizeof(double) * agt::kBuffer);
}

extern "C" {

// sizeof and the field offsets of emp_agent_params (12 fields) and emp_agent_rollout_io (24 fields)
void ac_layout(long long* out13, long long* out25) {
#define P(f) offsetof(emp_agent_params, f)
    const size_t p[13] = {sizeof(emp_agent_params), P(lat_K_P), P(lat_K_I), P(lat_K_D), P(lon_K_P), P(lon_K_I), P(lon_K_D), P(dt),
                          P(max_throttle), P(max_brake), P(max_steer), P(base_min_distance), P(reserved)};
#undef P
#define R(f) offsetof(emp_agent_rollout_io, f)
    const size_t r[25] = {sizeof(emp_agent_rollout_io), R(path), R(n_path), R(state), R(target_speed), R(head), R(past_steer), R(lon_err),
                          R(n_lon), R(lat_err), R(n_lat), R(state_out), R(head_out), R(past_steer_out), R(lon_err_out), R(n_lon_out),
                          R(lat_err_out), R(n_lat_out), R(status), R(done_tick), R(actors_out), R(log_state), R(log_control), R(log_head),
                          R(reserved)};
#undef R
    for (int i = 0; i < 13; ++i) out13[i] = (long long)p[i];
    for (int i = 0; i < 25; ++i) out25[i] = (long long)r[i];
}

// the defaults as the library sets them are the header's comments; this is pid10 alone: returns the command, buf / n in place
double ac_pid(double kp, double ki, double kd, double dt, double e, double* buf, int* n) { return agt::pid10(kp, ki, kd, dt, e, buf, n); }

void ac_observe(int A, const double* state, double* forward, double* speed_kmh, double* actors) {
    for (int a = 0; a < A; ++a) {
        const double* st = state + 6 * (size_t)a;
        const agt::Obs o = agt::observe(st[2], st[3], st[5]);
        if (forward) {
            forward[2 * a] = o.c;
            forward[2 * a + 1] = o.s;
        }
        if (speed_kmh) speed_kmh[a] = o.kmh;
        if (actors) {
            double* q = actors + 4 * (size_t)a;
            q[0] = st[0]; q[1] = st[1]; q[2] = o.wx; q[3] = o.wy;
        }
    }
}

// emp_agent_control on the CPU; each agent-state output may be its input
void ac_control(const emp_agent_params* p, int A, int max_path, const double* path, const int* n_path, const double* state,
                const double* forward, const double* speed_kmh, const double* target_speed, const int* head, const double* past_steer,
                const double* lon_err, const int* n_lon, const double* lat_err, const int* n_lat, double* control, int* status,
                int* head_out, double* past_steer_out, double* lon_err_out, int* n_lon_out, double* lat_err_out, int* n_lat_out,
                double* lat_error, double* lon_command) {
    const agt::Params prm = params_of(p);
    for (int a = 0; a < A; ++a) {
        const int np_ = agt::clampi(n_path[a], 0, max_path);
        double lon[agt::kBuffer], lat[agt::kBuffer];
        agt::Agent g = load(a, np_, head, past_steer, lon_err, n_lon, lat_err, n_lat, lon, lat);
        const agt::Tick k = agt::tick(prm, path + (size_t)a * max_path * 4, np_, state[6 * (size_t)a], state[6 * (size_t)a + 1], forward[2 * a],
                                      forward[2 * a + 1], speed_kmh[a], target_speed[a], g);
        store(a, g, head_out, past_steer_out, lon_err_out, n_lon_out, lat_err_out, n_lat_out);
        control[3 * a] = k.throttle;
        control[3 * a + 1] = k.steer;
        control[3 * a + 2] = k.brake;
        status[a] = k.status;
        if (lat_error) lat_error[a] = k.lat_error;
        if (lon_command) lon_command[a] = k.lon_command;
    }
}

// emp_agent_rollout on the CPU, statement for statement agent_rollout_kernel
void ac_rollout(const emp_agent_params* p, const emp_vehicle_params* vpp, int A, int max_path, int T, int log_every,
                const emp_agent_rollout_io* io) {
    const agt::Params prm = params_of(p);
    const ctl::VehicleParams vp = vehicle_of(vpp);
    for (int a = 0; a < A; ++a) {
        const double* path = io->path + (size_t)a * max_path * 4;
        const int np_ = agt::clampi(io->n_path[a], 0, max_path);
        double lon[agt::kBuffer], lat[agt::kBuffer];
        agt::Agent g = load(a, np_, io->head, io->past_steer, io->lon_err, io->n_lon, io->lat_err, io->n_lat, lon, lat);
        const double* q = io->state + 6 * (size_t)a;
        ctl::VehicleState s{q[0], q[1], q[2], q[3], q[4], q[5]};
        const double target = io->target_speed[a];
        int status = 0, done_tick = -1;
        for (int t = 0; t < T; ++t) {
            const agt::Obs o = agt::observe(s.fi, s.Vy, s.Vx);
            const agt::Tick k = agt::tick(prm, path, np_, s.x, s.y, o.c, o.s, o.kmh, target, g);
            if (t % log_every == 0) {
                const size_t row = (size_t)(t / log_every) * A + a;
                if (io->log_state) {
                    double* w = io->log_state + 6 * row;
                    w[0] = s.x; w[1] = s.y; w[2] = s.fi; w[3] = s.Vy; w[4] = s.fi_dot; w[5] = s.Vx;
                }
                if (io->log_control) {
                    double* w = io->log_control + 3 * row;
                    w[0] = k.throttle; w[1] = k.steer; w[2] = k.brake;
                }
                if (io->log_head) io->log_head[row] = g.head;
            }
            if ((k.status & agt::kDone) && done_tick < 0) done_tick = t;
            status |= k.status;
            s = ctl::vehicle_step(vp, s, k.throttle, k.steer, k.brake);
        }
        double* w = io->state_out + 6 * (size_t)a;
        w[0] = s.x; w[1] = s.y; w[2] = s.fi; w[3] = s.Vy; w[4] = s.fi_dot; w[5] = s.Vx;
        store(a, g, io->head_out, io->past_steer_out, io->lon_err_out, io->n_lon_out, io->lat_err_out, io->n_lat_out);
        io->status[a] = status;
        io->done_tick[a] = done_tick;
        if (io->actors_out) {
            const agt::Obs o = agt::observe(s.fi, s.Vy, s.Vx);
            double* v = io->actors_out + 4 * (size_t)a;
            v[0] = s.x; v[1] = s.y; v[2] = o.wx; v[3] = o.wy;
        }
    }
}

}  // extern "C"

#ifdef AGENT_CHECK_MAIN
#include <stdio.h>

// Three agents on one corner path (12 points straight, a 12 m radius right angle, 8 points straight, 2 m apart): one from the
// start, one with counts and a head out of range (clamped), one with no plan.  The rollout of T ticks must equal the chain of T
// single ticks bit for bit, drive the two routed agents to DONE near the path's end, and leave the third DONE at tick 0.  Every
// array is exactly as long as the call may touch, so a sanitizer sees an overrun.
int main() {
    std::vector<double> xy;
    for (int i = 0; i < 12; ++i) { xy.push_back(2.0 * i); xy.push_back(0.0); }
    for (int i = 1; i <= 9; ++i) {
        const double th = 1.5707963267948966 * i / 9.0;
        xy.push_back(22.0 + 12.0 * sin(th));
        xy.push_back(12.0 - 12.0 * cos(th));
    }
    for (int i = 1; i <= 8; ++i) { xy.push_back(34.0); xy.push_back(12.0 + 2.0 * i); }
    const int M = (int)xy.size() / 2, A = 3, T = 1600, every = 7, n_log = (T + every - 1) / every;
    std::vector<double> path((size_t)A * M * 4, 0.0);
    for (int a = 0; a < A; ++a)
        for (int i = 0; i < M; ++i) {
            path[((size_t)a * M + i) * 4] = xy[2 * i];
            path[((size_t)a * M + i) * 4 + 1] = xy[2 * i + 1];
        }
    std::vector<int> n_path{M, M + 50, 0}, head{0, -3, 9}, n_lon{0, 99, 0}, n_lat{0, -4, 0};
    std::vector<double> state{0.0, 0.3, 0.0, 0.0, 0.0, 2.0, -1.0, -0.5, 0.1, 0.0, 0.0, 0.0, 5.0, 5.0, 1.0, 0.0, 0.0, 3.0};
    std::vector<double> target{20.0, 30.0, 20.0}, past{0.0, 0.2, 0.0}, lon((size_t)A * 10, 0.25), lat((size_t)A * 10, 0.01);
    emp_agent_params p;
    p.lat_K_P = 1.95; p.lat_K_I = 0.05; p.lat_K_D = 0.2; p.lon_K_P = 1.0; p.lon_K_I = 0.05; p.lon_K_D = 0.0; p.dt = 0.05;
    p.max_throttle = 0.75; p.max_brake = 0.3; p.max_steer = 0.8; p.base_min_distance = 3.0; p.reserved = 0;
    const emp_vehicle_params vp = {1.015, 1.895, -148970.0, -82204.0, 1412.0, 1537.0, 0.05, 1.0, 3.0, 6.0, 0.0, 0};

    // the rollout
    std::vector<double> r_state(A * 6), r_past(A), r_lon(A * 10), r_lat(A * 10), r_act(A * 4), l_state((size_t)n_log * A * 6), l_ctl((size_t)n_log * A * 3);
    std::vector<int> r_head(A), r_nlon(A), r_nlat(A), r_status(A), r_done(A), l_head((size_t)n_log * A);
    const emp_agent_rollout_io io = {path.data(), n_path.data(), state.data(), target.data(), head.data(), past.data(), lon.data(), n_lon.data(),
                                     lat.data(), n_lat.data(), r_state.data(), r_head.data(), r_past.data(), r_lon.data(), r_nlon.data(),
                                     r_lat.data(), r_nlat.data(), r_status.data(), r_done.data(), r_act.data(), l_state.data(), l_ctl.data(),
                                     l_head.data(), 0};
    ac_rollout(&p, &vp, A, M, T, every, &io);

    // the chain, in place
    std::vector<double> c_state = state, c_past = past, c_lon = lon, c_lat = lat, fw(A * 2), kmh(A), ctl3(A * 3);
    std::vector<int> c_head = head, c_nlon = n_lon, c_nlat = n_lat, st(A), c_status(A, 0), c_done(A, -1);
    int bad = 0;
    for (int t = 0; t < T; ++t) {
        ac_observe(A, c_state.data(), fw.data(), kmh.data(), nullptr);
        ac_control(&p, A, M, path.data(), n_path.data(), c_state.data(), fw.data(), kmh.data(), target.data(), c_head.data(), c_past.data(),
                   c_lon.data(), c_nlon.data(), c_lat.data(), c_nlat.data(), ctl3.data(), st.data(), c_head.data(), c_past.data(), c_lon.data(),
                   c_nlon.data(), c_lat.data(), c_nlat.data(), nullptr, nullptr);
        for (int a = 0; a < A; ++a) {
            if (t % every == 0) {
                const size_t row = (size_t)(t / every) * A + a;
                bad += memcmp(&l_state[6 * row], &c_state[6 * a], 48) != 0 || memcmp(&l_ctl[3 * row], &ctl3[3 * a], 24) != 0 || l_head[row] != c_head[a];
            }
            c_status[a] |= st[a];
            if ((st[a] & EMP_AGT_DONE) && c_done[a] < 0) c_done[a] = t;
            const double* q = &c_state[6 * a];
            const ctl::VehicleState n = ctl::vehicle_step(vehicle_of(&vp), ctl::VehicleState{q[0], q[1], q[2], q[3], q[4], q[5]}, ctl3[3 * a],
                                                          ctl3[3 * a + 1], ctl3[3 * a + 2]);
            const double v[6] = {n.x, n.y, n.fi, n.Vy, n.fi_dot, n.Vx};
            memcpy(&c_state[6 * a], v, 48);
        }
    }
    bad += memcmp(r_state.data(), c_state.data(), sizeof(double) * A * 6) != 0;
    bad += memcmp(r_lon.data(), c_lon.data(), sizeof(double) * A * 10) != 0 || memcmp(r_lat.data(), c_lat.data(), sizeof(double) * A * 10) != 0;
    bad += memcmp(r_past.data(), c_past.data(), sizeof(double) * A) != 0;
    bad += r_head != c_head || r_nlon != c_nlon || r_nlat != c_nlat || r_status != c_status || r_done != c_done;
    // the two routed agents end DONE within braking distance of the last waypoint (1 m + v^2 / 12 at 30 km/h), at rest; the third
    // was DONE at once
    int wrong = 0;
    for (int a = 0; a < 2; ++a) {
        const double dx = r_state[6 * a] - 34.0, dy = r_state[6 * a + 1] - 28.0;
        wrong += !(r_status[a] == EMP_AGT_DONE && r_done[a] > 100 && r_head[a] == M && dx * dx + dy * dy < 100.0 && r_state[6 * a + 5] == 0.0);
    }
    wrong += !(r_done[2] == 0 && r_head[2] == 0 && r_nlon[2] == 0 && r_past[2] == 0.0);
    printf("agent_check: %d bad, %d wrong (done ticks %d %d %d)\n", bad, wrong, r_done[0], r_done[1], r_done[2]);
    return bad != 0 || wrong != 0;
}
#endif
