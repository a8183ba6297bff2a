// behavior_check.cpp - runs csrc/emp_behavior_core.h (the car-following law of the reference's BehaviorAgent) and
// csrc/emp_behavior_launch.h (the launch plan of its kernels) on the CPU for the `-m "not gpu"` suite: the very functions the
// behaviour kernels compile, a world at a time, with the published rows of a tick in plain arrays where the kernels keep them in
// LDS.  TEST TOOL ONLY: compiled with g++ -ffp-contract=off into a temporary directory by tests/test_behavior_host.py, never by the
// package.  With -DBEHAVIOR_CHECK_MAIN it is a program of its own (a platoon on an arc, the rollout against the chain of ticks and
// against itself cut in two) that a sanitizer build can run.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../emplanner_carla_amd/csrc/emp_behavior_core.h"
#include "../../emplanner_carla_amd/csrc/emp_behavior_launch.h"
#include "../../emplanner_carla_amd/csrc/emp_control_core.h"
#include "../../include/emplanner.h"

using namespace emp;

static agt::Params params_of(const emp_agent_params* p) {
    return agt::Params{p->lat_K_P, p->lat_K_I, p->lat_K_D, p->lon_K_P, p->lon_K_I, p->lon_K_D, p->dt, p->max_throttle, p->max_brake,
                       p->max_steer, p->base_min_distance};
}
static bhv::Params behavior_of(const emp_behavior_params* p) {
    return bhv::Params{p->max_speed, p->speed_lim_dist, p->speed_decrease, p->safety_time, p->min_proximity_threshold, p->braking_distance,
                       p->min_speed, p->emergency_brake, p->up_angle, (int)p->look_steps};
}
static ctl::VehicleParams vehicle_of(const emp_vehicle_params* p) {
    return ctl::VehicleParams{p->a, p->b, p->Cf, p->Cr, p->m, p->Iz, p->dt, p->steer_gain, p->throttle_accel, p->brake_decel, p->drag};
}

namespace {

// a world's agents between two ticks, as the kernels hold them
struct Lane {
    agt::Agent g;
    double lon[agt::kBuffer], lat[agt::kBuffer];
    ctl::VehicleState s;
    int np_;
};

void load(const emp_behavior_io* io, int a, int max_path, Lane& l) {
    l.np_ = agt::clampi(io->n_path[a], 0, max_path);
    l.g.head = agt::clampi(io->head[a], 0, l.np_);
    l.g.n_lon = agt::clampi(io->n_lon[a], 0, agt::kBuffer);
    l.g.n_lat = agt::clampi(io->n_lat[a], 0, agt::kBuffer);
    l.g.past_steer = io->past_steer[a];
    l.g.lon = l.lon;
    l.g.lat = l.lat;
    l.g.at = -1;
    l.g.px = l.g.py = 0.0;
    memcpy(l.lon, io->lon_err + (size_t)a * agt::kBuffer, sizeof(l.lon));
    memcpy(l.lat, io->lat_err + (size_t)a * agt::kBuffer, sizeof(l.lat));
    const double* q = io->state + 6 * (size_t)a;
    l.s = ctl::VehicleState{q[0], q[1], q[2], q[3], q[4], q[5]};
}

void store(const emp_behavior_io* io, int a, const Lane& l) {
    io->head_out[a] = l.g.head;
    io->past_steer_out[a] = l.g.past_steer;
    io->n_lon_out[a] = l.g.n_lon;
    io->n_lat_out[a] = l.g.n_lat;
    memcpy(io->lon_err_out + (size_t)a * agt::kBuffer, l.lon, sizeof(l.lon));
    memcpy(io->lat_err_out + (size_t)a * agt::kBuffer, l.lat, sizeof(l.lat));
}

struct Pub {
    double x[bhv::kMaxWorld], y[bhv::kMaxWorld], kmh[bhv::kMaxWorld], ext[bhv::kMaxWorld];
    int key[bhv::kMaxWorld];
};

}  // namespace

extern "C" {

// sizeof and the field offsets of emp_behavior_params (11 fields) and emp_behavior_io (44 fields)
void bc_layout(long long* out12, long long* out45) {
#define P(f) offsetof(emp_behavior_params, f)
    const size_t p[12] = {sizeof(emp_behavior_params), P(max_speed), P(speed_lim_dist), P(speed_decrease), P(safety_time),
                          P(min_proximity_threshold), P(braking_distance), P(min_speed), P(emergency_brake), P(up_angle), P(look_steps),
                          P(reserved)};
#undef P
#define R(f) offsetof(emp_behavior_io, f)
    const size_t r[45] = {sizeof(emp_behavior_io), R(n_world), R(path), R(n_path), R(lane), R(state), R(forward), R(speed_kmh), R(speed_limit),
                          R(extent), R(head), R(past_steer), R(lon_err), R(n_lon), R(lat_err), R(n_lat), R(n_other), R(other), R(other_lane),
                          R(head_out), R(past_steer_out), R(lon_err_out), R(n_lon_out), R(lat_err_out), R(n_lat_out), R(status), R(control),
                          R(mode), R(blocker), R(distance), R(ttc), R(target_speed_out), R(lat_error), R(lon_command), R(state_out),
                          R(done_tick), R(mode_ticks), R(min_gap), R(actors_out), R(log_state), R(log_control), R(log_head), R(log_mode),
                          R(log_target), R(reserved)};
#undef R
    for (int i = 0; i < 12; ++i) out12[i] = (long long)p[i];
    for (int i = 0; i < 45; ++i) out45[i] = (long long)r[i];
}

// plan_behavior: out[6] = grid, block, lds, blocks_per_cu, n_log, refused; returns the refusal's text (or null)
const char* bc_plan(int W, int max_world, int max_other, int max_path, int T, int log_every, long long tick0, long long* out6) {
    const bhv::BehaviorPlan p = bhv::plan_behavior(W, max_world, max_other, max_path, T, log_every, tick0);
    out6[0] = p.grid; out6[1] = p.block; out6[2] = (long long)p.lds; out6[3] = p.blocks_per_cu; out6[4] = (long long)p.n_log;
    out6[5] = p.error != nullptr;
    return p.error;
}

// emp_agent_behave on the CPU, statement for statement agent_behave_kernel; each agent-state output may be its input
void bc_behave(const emp_agent_params* p, const emp_behavior_params* bpp, int W, int max_world, int max_path, int max_other, long long tick0,
               const emp_behavior_io* io) {
    const agt::Params ap = params_of(p);
    const bhv::Params bp = behavior_of(bpp);
    std::vector<Lane> lanes(bhv::kMaxWorld);
    for (int w = 0; w < W; ++w) {
        const int nw = agt::clampi(io->n_world[w], 0, max_world);
        const int no = (max_other > 0 && io->n_other) ? agt::clampi(io->n_other[w], 0, max_other) : 0;
        Pub pub;
        for (int i = 0; i < nw; ++i) {                     // every lane reads all of its inputs before any lane writes
            const int a = w * max_world + i;
            load(io, a, max_path, lanes[i]);
            pub.x[i] = lanes[i].s.x;
            pub.y[i] = lanes[i].s.y;
            pub.kmh[i] = io->speed_kmh[a];
            pub.ext[i] = io->extent[a];
            pub.key[i] = bhv::shown_key(io->lane + (size_t)a * max_path, lanes[i].np_, lanes[i].g.head);
        }
        for (int i = 0; i < nw; ++i) {
            const int a = w * max_world + i;
            const bhv::Scene sc{i, nw, no, pub.x, pub.y, pub.kmh, pub.ext, pub.key, no ? io->other + (size_t)w * max_other * 5 : nullptr,
                                no ? io->other_lane + (size_t)w * max_other : nullptr, (double)tick0 * ap.dt};
            const bhv::Out o = bhv::behave(ap, bp, io->path + (size_t)a * max_path * 4, io->lane + (size_t)a * max_path, lanes[i].np_, pub.x[i],
                                           pub.y[i], io->forward[2 * a], io->forward[2 * a + 1], pub.kmh[i], io->speed_limit[a], pub.ext[i], sc,
                                           lanes[i].g);
            store(io, a, lanes[i]);
            io->control[3 * a] = o.k.throttle; io->control[3 * a + 1] = o.k.steer; io->control[3 * a + 2] = o.k.brake;
            io->status[a] = o.k.status;
            io->mode[a] = o.mode;
            io->blocker[a] = o.blocker;
            io->distance[a] = o.distance;
            io->ttc[a] = o.ttc;
            io->target_speed_out[a] = o.target;
            if (io->lat_error) io->lat_error[a] = o.k.lat_error;
            if (io->lon_command) io->lon_command[a] = o.k.lon_command;
        }
    }
}

// emp_traffic_rollout on the CPU, statement for statement traffic_rollout_kernel
void bc_rollout(const emp_agent_params* p, const emp_behavior_params* bpp, const emp_vehicle_params* vpp, int W, int max_world, int max_path,
                int max_other, int T, int log_every, long long tick0, const emp_behavior_io* io) {
    const agt::Params ap = params_of(p);
    const bhv::Params bp = behavior_of(bpp);
    const ctl::VehicleParams vp = vehicle_of(vpp);
    const int A = W * max_world;
    std::vector<Lane> lanes(bhv::kMaxWorld);
    for (int w = 0; w < W; ++w) {
        const int nw = agt::clampi(io->n_world[w], 0, max_world);
        const int no = (max_other > 0 && io->n_other) ? agt::clampi(io->n_other[w], 0, max_other) : 0;
        Pub pub;
        std::vector<int> status(nw, 0), done(nw, -1), ticks((size_t)nw * bhv::kCountedModes, 0);
        std::vector<double> gap(nw, bhv::infinity());
        std::vector<agt::Obs> obs(nw);
        for (int i = 0; i < nw; ++i) {
            load(io, w * max_world + i, max_path, lanes[i]);
            pub.ext[i] = io->extent[w * max_world + i];
        }
        for (int t = 0; t < T; ++t) {
            for (int i = 0; i < nw; ++i) {
                const int a = w * max_world + i;
                obs[i] = agt::observe(lanes[i].s.fi, lanes[i].s.Vy, lanes[i].s.Vx);
                pub.x[i] = lanes[i].s.x;
                pub.y[i] = lanes[i].s.y;
                pub.kmh[i] = obs[i].kmh;
                pub.key[i] = bhv::shown_key(io->lane + (size_t)a * max_path, lanes[i].np_, lanes[i].g.head);
            }
            for (int i = 0; i < nw; ++i) {
                const int a = w * max_world + i;
                Lane& l = lanes[i];
                const bhv::Scene sc{i, nw, no, pub.x, pub.y, pub.kmh, pub.ext, pub.key, no ? io->other + (size_t)w * max_other * 5 : nullptr,
                                    no ? io->other_lane + (size_t)w * max_other : nullptr, (double)(tick0 + t) * ap.dt};
                const bhv::Out r = bhv::behave(ap, bp, io->path + (size_t)a * max_path * 4, io->lane + (size_t)a * max_path, l.np_, l.s.x, l.s.y,
                                               obs[i].c, obs[i].s, obs[i].kmh, io->speed_limit[a], pub.ext[i], sc, l.g);
                if (t % log_every == 0) {
                    const size_t row = (size_t)(t / log_every) * A + a;
                    if (io->log_state) {
                        double* q = io->log_state + 6 * row;
                        q[0] = l.s.x; q[1] = l.s.y; q[2] = l.s.fi; q[3] = l.s.Vy; q[4] = l.s.fi_dot; q[5] = l.s.Vx;
                    }
                    if (io->log_control) {
                        double* q = io->log_control + 3 * row;
                        q[0] = r.k.throttle; q[1] = r.k.steer; q[2] = r.k.brake;
                    }
                    if (io->log_head) io->log_head[row] = l.g.head;
                    if (io->log_mode) io->log_mode[row] = r.mode;
                    if (io->log_target) io->log_target[row] = r.target;
                }
                if ((r.k.status & agt::kDone) && done[i] < 0) done[i] = t;
                status[i] |= r.k.status;
                if (r.mode < bhv::kCountedModes) ++ticks[(size_t)i * bhv::kCountedModes + r.mode];
                if (r.blocker >= 0 && r.distance < gap[i]) gap[i] = r.distance;
                l.s = ctl::vehicle_step(vp, l.s, r.k.throttle, r.k.steer, r.k.brake);       // x, y of this tick stay published in pub
            }
        }
        for (int i = 0; i < nw; ++i) {
            const int a = w * max_world + i;
            const Lane& l = lanes[i];
            double* q = io->state_out + 6 * (size_t)a;
            q[0] = l.s.x; q[1] = l.s.y; q[2] = l.s.fi; q[3] = l.s.Vy; q[4] = l.s.fi_dot; q[5] = l.s.Vx;
            store(io, a, l);
            io->status[a] = status[i];
            io->done_tick[a] = done[i];
            for (int m = 0; m < bhv::kCountedModes; ++m) io->mode_ticks[(size_t)a * bhv::kCountedModes + m] = ticks[(size_t)i * bhv::kCountedModes + m];
            io->min_gap[a] = gap[i];
            if (io->actors_out) {
                const agt::Obs o = agt::observe(l.s.fi, l.s.Vy, l.s.Vx);
                double* v = io->actors_out + 4 * (size_t)a;
                v[0] = l.s.x; v[1] = l.s.y; v[2] = o.wx; v[3] = o.wy;
            }
        }
    }
}

}  // extern "C"

#ifdef BEHAVIOR_CHECK_MAIN
#include <math.h>
#include <stdio.h>

// Two worlds of max_world 4 on a 100 m-radius arc of 120 waypoints 2 m apart: world 0 holds a platoon of three (the leader limited
// to 23 km/h, the followers to 60, 30 m apart) and one other vehicle parked on the arc; world 1 holds one agent alone.  The padding
// slots hold counts and heads out of range.  The rollout of T ticks must equal the chain of T single ticks bit for bit, and equal
// itself cut in two; a follower must have reacted and kept a gap; the lone agent never reacts.  Every array is exactly as long as
// the call may touch, so a sanitizer sees an overrun.
int main() {
    const int W = 2, N = 4, M = 120, K = 1, A = W * N, T = 500, every = 7, cut = 170;
    std::vector<double> path((size_t)A * M * 4, 0.0);
    std::vector<int> lane((size_t)A * M, 3);
    for (int a = 0; a < A; ++a)
        for (int i = 0; i < M; ++i) {
            const double th = 2.0 * i / 100.0;
            path[((size_t)a * M + i) * 4] = 100.0 * sin(th);
            path[((size_t)a * M + i) * 4 + 1] = 100.0 - 100.0 * cos(th);
        }
    auto on_arc = [](double sdist, double v, double* q) {
        const double th = sdist / 100.0;
        q[0] = 100.0 * sin(th); q[1] = 100.0 - 100.0 * cos(th); q[2] = th; q[3] = 0.0; q[4] = 0.0; q[5] = v;
    };
    std::vector<double> state((size_t)A * 6, 0.0), limit(A, 60.0), extent(A, 2.4), past(A, 0.0), lon((size_t)A * 10, 0.0), lat((size_t)A * 10, 0.0);
    std::vector<int> n_world{3, 1}, n_path(A, M), head(A, 0), n_lon(A, 0), n_lat(A, 0), n_other{1, 0}, other_lane{3, -1};
    on_arc(0.0, 12.0, &state[0]);
    on_arc(30.0, 10.0, &state[6]);
    on_arc(60.0, 6.0, &state[12]);
    on_arc(10.0, 8.0, &state[24]);
    limit[2] = 23.0;
    head[1] = 14; head[2] = 29; head[4] = 4;
    n_path[3] = 9999; head[3] = -7; n_lon[3] = 99;                 // a padding slot: never read
    std::vector<double> other((size_t)W * K * 5, 0.0);
    { double q[6]; on_arc(200.0, 0.0, q); other[0] = q[0]; other[1] = q[1]; other[4] = 2.0; }
    emp_agent_params p;
    p.lat_K_P = 1.95; p.lat_K_I = 0.05; p.lat_K_D = 0.2; p.lon_K_P = 1.0; p.lon_K_I = 0.05; p.lon_K_D = 0.0; p.dt = 0.05;
    p.max_throttle = 0.75; p.max_brake = 0.3; p.max_steer = 0.8; p.base_min_distance = 3.0; p.reserved = 0;
    const emp_behavior_params bp = {50.0, 3.0, 10.0, 3.0, 10.0, 5.0, 5.0, 0.5, 30.0, 5, 0};
    const emp_vehicle_params vp = {1.015, 1.895, -148970.0, -82204.0, 1412.0, 1537.0, 0.05, 1.0, 3.0, 6.0, 0.0, 0};

    struct Run {
        std::vector<double> state, past, lon, lat, act, gap, l_state, l_ctl, l_tgt;
        std::vector<int> head, nlon, nlat, status, done, ticks, l_head, l_mode;
    };
    auto rollout = [&](const Run* from, int ticks, int every_, long long tick0, bool logs) {
        Run r;
        const size_t nl = logs ? (size_t)((ticks + every_ - 1) / every_) : 0;
        r.state.assign((size_t)A * 6, -1.0); r.past.assign(A, -1.0); r.lon.assign((size_t)A * 10, -1.0); r.lat.assign((size_t)A * 10, -1.0);
        r.act.assign((size_t)A * 4, -1.0); r.gap.assign(A, -1.0); r.head.assign(A, -1); r.nlon.assign(A, -1); r.nlat.assign(A, -1);
        r.status.assign(A, -1); r.done.assign(A, -9); r.ticks.assign((size_t)A * 5, -1);
        r.l_state.assign(nl * A * 6, -1.0); r.l_ctl.assign(nl * A * 3, -1.0); r.l_tgt.assign(nl * A, -1.0); r.l_head.assign(nl * A, -1);
        r.l_mode.assign(nl * A, -1);
        emp_behavior_io io;
        memset(&io, 0, sizeof(io));
        io.n_world = n_world.data(); io.path = path.data(); io.n_path = n_path.data(); io.lane = lane.data();
        io.state = from ? from->state.data() : state.data();
        io.speed_limit = limit.data(); io.extent = extent.data();
        io.head = from ? from->head.data() : head.data(); io.past_steer = from ? from->past.data() : past.data();
        io.lon_err = from ? from->lon.data() : lon.data(); io.n_lon = from ? from->nlon.data() : n_lon.data();
        io.lat_err = from ? from->lat.data() : lat.data(); io.n_lat = from ? from->nlat.data() : n_lat.data();
        io.n_other = n_other.data(); io.other = other.data(); io.other_lane = other_lane.data();
        io.head_out = r.head.data(); io.past_steer_out = r.past.data(); io.lon_err_out = r.lon.data(); io.n_lon_out = r.nlon.data();
        io.lat_err_out = r.lat.data(); io.n_lat_out = r.nlat.data(); io.status = r.status.data(); io.state_out = r.state.data();
        io.done_tick = r.done.data(); io.mode_ticks = r.ticks.data(); io.min_gap = r.gap.data(); io.actors_out = r.act.data();
        if (logs) {
            io.log_state = r.l_state.data(); io.log_control = r.l_ctl.data(); io.log_head = r.l_head.data(); io.log_mode = r.l_mode.data();
            io.log_target = r.l_tgt.data();
        }
        bc_rollout(&p, &bp, &vp, W, N, M, K, ticks, every_, tick0, &io);
        return r;
    };
    const Run whole = rollout(nullptr, T, every, 0, true);
    int bad = 0;
    // the padding slots of the outputs stay as they were
    const int pad[4] = {3, 5, 6, 7};
    for (int a : pad) bad += whole.head[a] != -1 || whole.status[a] != -1 || whole.state[6 * a] != -1.0 || whole.gap[a] != -1.0 || whole.l_mode[a] != -1;
    // cut in two
    Run first = rollout(nullptr, cut, 1, 0, false);
    for (int a : pad) {                                            // the second half reads the first's outputs: give its padding the inputs' poison
        first.head[a] = head[a]; first.nlon[a] = n_lon[a]; first.nlat[a] = n_lat[a];
    }
    const Run second = rollout(&first, T - cut, 1, cut, false);
    bad += second.state != whole.state || second.head != whole.head || second.lon != whole.lon || second.lat != whole.lat || second.past != whole.past;

    // the chain of single ticks, in place
    std::vector<double> c_state = state, c_past = past, c_lon = lon, c_lat = lat, fw((size_t)A * 2, 0.0), kmh(A, 0.0), ctl3((size_t)A * 3, 0.0), dist(A), ttc(A),
                        tgt(A), c_gap(A, bhv::infinity());
    std::vector<int> c_head = head, c_nlon = n_lon, c_nlat = n_lat, st(A, 0), mode(A, -1), blk(A), c_ticks((size_t)A * 5, 0);
    const int live[4] = {0, 1, 2, 4};
    for (int t = 0; t < T; ++t) {
        for (int a : live) {
            const agt::Obs o = agt::observe(c_state[6 * a + 2], c_state[6 * a + 3], c_state[6 * a + 5]);
            fw[2 * a] = o.c; fw[2 * a + 1] = o.s; kmh[a] = o.kmh;
        }
        emp_behavior_io io;
        memset(&io, 0, sizeof(io));
        io.n_world = n_world.data(); io.path = path.data(); io.n_path = n_path.data(); io.lane = lane.data(); io.state = c_state.data();
        io.forward = fw.data(); io.speed_kmh = kmh.data(); io.speed_limit = limit.data(); io.extent = extent.data();
        io.head = c_head.data(); io.past_steer = c_past.data(); io.lon_err = c_lon.data(); io.n_lon = c_nlon.data(); io.lat_err = c_lat.data();
        io.n_lat = c_nlat.data(); io.n_other = n_other.data(); io.other = other.data(); io.other_lane = other_lane.data();
        io.head_out = c_head.data(); io.past_steer_out = c_past.data(); io.lon_err_out = c_lon.data(); io.n_lon_out = c_nlon.data();
        io.lat_err_out = c_lat.data(); io.n_lat_out = c_nlat.data(); io.status = st.data(); io.control = ctl3.data(); io.mode = mode.data();
        io.blocker = blk.data(); io.distance = dist.data(); io.ttc = ttc.data(); io.target_speed_out = tgt.data();
        bc_behave(&p, &bp, W, N, M, K, t, &io);
        for (int a : live) {
            if (t % every == 0) {
                const size_t row = (size_t)(t / every) * A + a;
                bad += memcmp(&whole.l_state[6 * row], &c_state[6 * a], 48) != 0 || memcmp(&whole.l_ctl[3 * row], &ctl3[3 * a], 24) != 0 ||
                       whole.l_head[row] != c_head[a] || whole.l_mode[row] != mode[a] || memcmp(&whole.l_tgt[row], &tgt[a], 8) != 0;
            }
            if (mode[a] < 5) ++c_ticks[5 * a + mode[a]];
            if (blk[a] >= 0 && dist[a] < c_gap[a]) c_gap[a] = dist[a];
            const double* q = &c_state[6 * a];
            const ctl::VehicleState n = ctl::vehicle_step(vehicle_of(&vp), ctl::VehicleState{q[0], q[1], q[2], q[3], q[4], q[5]}, ctl3[3 * a],
                                                          ctl3[3 * a + 1], ctl3[3 * a + 2]);
            const double v[6] = {n.x, n.y, n.fi, n.Vy, n.fi_dot, n.Vx};
            memcpy(&c_state[6 * a], v, 48);
        }
    }
    for (int a : live) {
        bad += memcmp(&whole.state[6 * a], &c_state[6 * a], 48) != 0 || whole.head[a] != c_head[a] || whole.nlon[a] != c_nlon[a] ||
               memcmp(&whole.lon[10 * a], &c_lon[10 * a], 80) != 0 || memcmp(&whole.lat[10 * a], &c_lat[10 * a], 80) != 0 ||
               memcmp(&whole.gap[a], &c_gap[a], 8) != 0 || memcmp(&whole.ticks[5 * a], &c_ticks[5 * a], 20) != 0;
    }
    // what the scene is for: both followers reacted (the gap is bumper to bumper and may go below 0: the law brakes late), the leader and the lone agent never reacted
    int wrong = 0;
    for (int a = 0; a < 2; ++a) {
        const int* k = &whole.ticks[5 * a];
        wrong += !(k[1] + k[2] + k[3] + k[4] > 0 && whole.gap[a] < 30.0);
    }
    wrong += !(whole.ticks[5 * 4] > 0 && whole.ticks[5 * 4 + 1] + whole.ticks[5 * 4 + 2] + whole.ticks[5 * 4 + 3] + whole.ticks[5 * 4 + 4] == 0 &&
               whole.gap[4] == bhv::infinity());
    printf("behavior_check: %d bad, %d wrong (follower 0 ticks %d %d %d %d %d, min gap %.3f)\n", bad, wrong, whole.ticks[0], whole.ticks[1],
           whole.ticks[2], whole.ticks[3], whole.ticks[4], whole.gap[0]);
    return bad != 0 || wrong != 0;
}
#endif
