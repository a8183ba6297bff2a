// hazard_check.cpp - runs csrc/emp_hazard_core.h (red lights and pedestrians in front of the car-following law) and
// csrc/emp_hazard_launch.h (the launch plan of its kernels) on the CPU for the `-m "not gpu"` suite: the very functions the hazard
// kernels compile, a world at a time, with the rows the kernels keep in LDS in plain arrays.  It builds on behavior_check.cpp (the
// agents between two ticks, the published rows).  TEST TOOL ONLY: compiled with g++ -ffp-contract=off into a temporary directory by
// tests/test_hazard_host.py, never by the package.  With -DHAZARD_CHECK_MAIN it is a program of its own (two agents, a light that
// switches and a walker that crosses: the rollout against the chain of ticks and against itself cut in two) that a sanitizer build
// can run.
#include "behavior_check.cpp"

#include "../../emplanner_carla_amd/csrc/emp_hazard_core.h"
#include "../../emplanner_carla_amd/csrc/emp_hazard_launch.h"

static hz::Params hazard_of(const emp_hazard_params* p) {
    return hz::Params{p->tlight_threshold, p->tlight_up_angle, p->walker_radius, p->walker_up_angle};
}

namespace {

// stage_hazards: the rows of world w and their clamped counts
hz::Scene scene_of(const emp_hazard_io* h, int w, int max_light, int max_walker) {
    hz::Scene sc;
    sc.n_light = (max_light > 0 && h->n_light) ? agt::clampi(h->n_light[w], 0, max_light) : 0;
    sc.n_walker = (max_walker > 0 && h->n_walker) ? agt::clampi(h->n_walker[w], 0, max_walker) : 0;
    sc.light = sc.n_light ? h->light + (size_t)w * max_light * 4 : nullptr;
    sc.light_key = sc.n_light ? h->light_lane + (size_t)w * max_light : nullptr;
    sc.light_cycle = sc.n_light ? h->light_cycle + (size_t)w * max_light * 3 : nullptr;
    sc.walker = sc.n_walker ? h->walker + (size_t)w * max_walker * 5 : nullptr;
    sc.walker_key = sc.n_walker ? h->walker_lane + (size_t)w * max_walker : nullptr;
    sc.k = 0;
    sc.tau = 0.0;
    return sc;
}

}  // namespace

extern "C" {

// sizeof and the field offsets of emp_hazard_params (5 fields) and emp_hazard_io (17 fields)
void hc_layout(long long* out6, long long* out18) {
#define P(f) offsetof(emp_hazard_params, f)
    const size_t p[6] = {sizeof(emp_hazard_params), P(tlight_threshold), P(tlight_up_angle), P(walker_radius), P(walker_up_angle), P(reserved)};
#undef P
#define R(f) offsetof(emp_hazard_io, f)
    const size_t r[18] = {sizeof(emp_hazard_io), R(n_light), R(light), R(light_lane), R(light_cycle), R(n_walker), R(walker), R(walker_lane),
                          R(last_light), R(last_light_out), R(cause), R(light_hit), R(walker_hit), R(walker_distance), R(cause_ticks),
                          R(min_walker_gap), R(log_cause), R(reserved)};
#undef R
    for (int i = 0; i < 6; ++i) out6[i] = (long long)p[i];
    for (int i = 0; i < 18; ++i) out18[i] = (long long)r[i];
}

// plan_hazards: out[6] as bc_plan's; offs[6] = the LDS offsets in doubles and the layout's length
const char* hc_plan(int W, int max_world, int max_other, int max_light, int max_walker, int max_path, int T, int log_every, long long tick0,
                    long long* out6, long long* offs6) {
    const bhv::BehaviorPlan p = hz::plan_hazards(W, max_world, max_other, max_light, max_walker, max_path, T, log_every, tick0);
    out6[0] = p.grid; out6[1] = p.block; out6[2] = (long long)p.lds; out6[3] = p.blocks_per_cu; out6[4] = (long long)p.n_log;
    out6[5] = p.error != nullptr;
    offs6[0] = hz::kOffLight; offs6[1] = hz::kOffLightKey; offs6[2] = hz::kOffLightCycle; offs6[3] = hz::kOffWalker;
    offs6[4] = hz::kOffWalkerKey; offs6[5] = hz::kLdsDoubles;
    return p.error;
}

// emp_agent_behave_hazards on the CPU, statement for statement agent_behave_hazards_kernel
void hc_behave(const emp_agent_params* p, const emp_behavior_params* bpp, const emp_hazard_params* hpp, int W, int max_world, int max_path,
               int max_other, int max_light, int max_walker, long long tick0, const emp_behavior_io* io, const emp_hazard_io* h) {
    const agt::Params ap = params_of(p);
    const bhv::Params bp = behavior_of(bpp);
    const hz::Params hp = hazard_of(hpp);
    std::vector<Lane> lanes(bhv::kMaxWorld);
    for (int w = 0; w < W; ++w) {
        const int nw = agt::clampi(io->n_world[w], 0, max_world);
        const int no = (max_other > 0 && io->n_other) ? agt::clampi(io->n_other[w], 0, max_other) : 0;
        hz::Scene hs = scene_of(h, w, max_light, max_walker);
        Pub pub;
        int last[bhv::kMaxWorld];
        for (int i = 0; i < nw; ++i) {                     // every lane reads all of its inputs before any lane writes
            const int a = w * max_world + i;
            load(io, a, max_path, lanes[i]);
            pub.x[i] = lanes[i].s.x;
            pub.y[i] = lanes[i].s.y;
            pub.kmh[i] = io->speed_kmh[a];
            pub.ext[i] = io->extent[a];
            pub.key[i] = bhv::shown_key(io->lane + (size_t)a * max_path, lanes[i].np_, lanes[i].g.head);
            last[i] = h->last_light[a];
        }
        hs.k = tick0;
        hs.tau = (double)tick0 * ap.dt;
        for (int i = 0; i < nw; ++i) {
            const int a = w * max_world + i;
            const bhv::Scene sc{i, nw, no, pub.x, pub.y, pub.kmh, pub.ext, pub.key, no ? io->other + (size_t)w * max_other * 5 : nullptr,
                                no ? io->other_lane + (size_t)w * max_other : nullptr, hs.tau};
            const hz::Out o = hz::behave(ap, bp, hp, io->path + (size_t)a * max_path * 4, io->lane + (size_t)a * max_path, lanes[i].np_,
                                         pub.x[i], pub.y[i], io->forward[2 * a], io->forward[2 * a + 1], pub.kmh[i], io->speed_limit[a],
                                         pub.ext[i], sc, hs, lanes[i].g, last[i]);
            store(io, a, lanes[i]);
            io->control[3 * a] = o.b.k.throttle; io->control[3 * a + 1] = o.b.k.steer; io->control[3 * a + 2] = o.b.k.brake;
            io->status[a] = o.b.k.status;
            io->mode[a] = o.b.mode;
            io->blocker[a] = o.b.blocker;
            io->distance[a] = o.b.distance;
            io->ttc[a] = o.b.ttc;
            io->target_speed_out[a] = o.b.target;
            if (io->lat_error) io->lat_error[a] = o.b.k.lat_error;
            if (io->lon_command) io->lon_command[a] = o.b.k.lon_command;
            h->last_light_out[a] = last[i];
            h->cause[a] = o.cause;
            h->light_hit[a] = o.light_hit;
            h->walker_hit[a] = o.walker_hit;
            h->walker_distance[a] = o.walker_distance;
        }
    }
}

// emp_traffic_rollout_hazards on the CPU, statement for statement traffic_rollout_hazards_kernel
void hc_rollout(const emp_agent_params* p, const emp_behavior_params* bpp, const emp_hazard_params* hpp, const emp_vehicle_params* vpp, int W,
                int max_world, int max_path, int max_other, int max_light, int max_walker, int T, int log_every, long long tick0,
                const emp_behavior_io* io, const emp_hazard_io* h) {
    const agt::Params ap = params_of(p);
    const bhv::Params bp = behavior_of(bpp);
    const hz::Params hp = hazard_of(hpp);
    const ctl::VehicleParams vp = vehicle_of(vpp);
    const int A = W * max_world;
    std::vector<Lane> lanes(bhv::kMaxWorld);
    for (int w = 0; w < W; ++w) {
        const int nw = agt::clampi(io->n_world[w], 0, max_world);
        const int no = (max_other > 0 && io->n_other) ? agt::clampi(io->n_other[w], 0, max_other) : 0;
        hz::Scene hs = scene_of(h, w, max_light, max_walker);
        Pub pub;
        std::vector<int> status(nw, 0), done(nw, -1), ticks((size_t)nw * bhv::kCountedModes, 0), causes((size_t)nw * hz::kCountedCauses, 0),
            last(nw, -1);
        std::vector<double> gap(nw, bhv::infinity()), wgap(nw, bhv::infinity());
        std::vector<agt::Obs> obs(nw);
        for (int i = 0; i < nw; ++i) {
            load(io, w * max_world + i, max_path, lanes[i]);
            pub.ext[i] = io->extent[w * max_world + i];
            last[i] = h->last_light[w * max_world + i];
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
            hs.k = tick0 + t;
            hs.tau = (double)hs.k * ap.dt;
            for (int i = 0; i < nw; ++i) {
                const int a = w * max_world + i;
                Lane& l = lanes[i];
                const bhv::Scene sc{i, nw, no, pub.x, pub.y, pub.kmh, pub.ext, pub.key, no ? io->other + (size_t)w * max_other * 5 : nullptr,
                                    no ? io->other_lane + (size_t)w * max_other : nullptr, hs.tau};
                int ll = last[i];
                const hz::Out r = hz::behave(ap, bp, hp, io->path + (size_t)a * max_path * 4, io->lane + (size_t)a * max_path, l.np_, l.s.x,
                                             l.s.y, obs[i].c, obs[i].s, obs[i].kmh, io->speed_limit[a], pub.ext[i], sc, hs, l.g, ll);
                last[i] = ll;
                if (t % log_every == 0) {
                    const size_t row = (size_t)(t / log_every) * A + a;
                    if (io->log_state) {
                        double* q = io->log_state + 6 * row;
                        q[0] = l.s.x; q[1] = l.s.y; q[2] = l.s.fi; q[3] = l.s.Vy; q[4] = l.s.fi_dot; q[5] = l.s.Vx;
                    }
                    if (io->log_control) {
                        double* q = io->log_control + 3 * row;
                        q[0] = r.b.k.throttle; q[1] = r.b.k.steer; q[2] = r.b.k.brake;
                    }
                    if (io->log_head) io->log_head[row] = l.g.head;
                    if (io->log_mode) io->log_mode[row] = r.b.mode;
                    if (io->log_target) io->log_target[row] = r.b.target;
                    if (h->log_cause) h->log_cause[row] = r.cause;
                }
                if ((r.b.k.status & agt::kDone) && done[i] < 0) done[i] = t;
                status[i] |= r.b.k.status;
                if (r.b.mode < bhv::kCountedModes) ++ticks[(size_t)i * bhv::kCountedModes + r.b.mode];
                if (r.cause >= 1) ++causes[(size_t)i * hz::kCountedCauses + r.cause - 1];
                if (r.b.blocker >= 0 && r.b.distance < gap[i]) gap[i] = r.b.distance;
                if (r.walker_hit >= 0 && r.walker_distance < wgap[i]) wgap[i] = r.walker_distance;
                l.s = ctl::vehicle_step(vp, l.s, r.b.k.throttle, r.b.k.steer, r.b.k.brake);
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
            h->last_light_out[a] = last[i];
            for (int m = 0; m < hz::kCountedCauses; ++m) h->cause_ticks[(size_t)a * hz::kCountedCauses + m] = causes[(size_t)i * hz::kCountedCauses + m];
            h->min_walker_gap[a] = wgap[i];
        }
    }
}

}  // extern "C"

#ifdef HAZARD_CHECK_MAIN
#include <math.h>
#include <stdio.h>

// One world of max_world 3 on a straight road of 150 waypoints 2 m apart along +x: agent 0 starts at x = 0 with 8 m/s, agent 1 at
// x = 150 with 8 m/s; slot 2 is padding with counts out of range.  Light 0 stands at x = 60 and is red for ticks [0, 260) of a
// 400-tick period; light 1 is on another key.  A walker crosses the road at x = 230 while agent 1 comes up to it.  The rollout of T
// ticks must equal the chain of T single ticks bit for bit, and itself cut in two at a tick where agent 0 is held by the light.
// Every array is exactly as long as the call may touch, so a sanitizer sees an overrun.
int main() {
    const int W = 1, N = 3, M = 150, A = W * N, T = 500, every = 7, cut = 200, ML = 2, MW = 1;
    std::vector<double> path((size_t)A * M * 4, 0.0);
    std::vector<int> lane((size_t)A * M, 3);
    for (int a = 0; a < A; ++a)
        for (int i = 0; i < M; ++i) path[((size_t)a * M + i) * 4] = 2.0 * i + 0.25;
    std::vector<double> state((size_t)A * 6, 0.0), limit(A, 30.0), extent(A, 2.4), past(A, 0.0), lon((size_t)A * 10, 0.0), lat((size_t)A * 10, 0.0);
    std::vector<int> n_world{2}, n_path(A, M), head(A, 0), n_lon(A, 0), n_lat(A, 0), last0(A, -1);
    state[0] = 0.0; state[1] = 0.1; state[5] = 8.0;
    state[6] = 150.0; state[7] = -0.1; state[11] = 8.0;
    head[1] = 75;
    n_path[2] = 9999; head[2] = -7; n_lon[2] = 99; last0[2] = 12345;
    std::vector<int> n_light{ML}, light_lane{3, 4}, light_cycle{400, 0, 260, 1, 0, 1}, n_walker{MW}, walker_lane{3};
    std::vector<double> light{60.0, 0.0, 1.0, 0.0, 20.0, 0.0, 1.0, 0.0};
    std::vector<double> walker{230.0, 6.0, 0.0, -0.7, 0.4};
    emp_agent_params p;
    p.lat_K_P = 1.95; p.lat_K_I = 0.05; p.lat_K_D = 0.2; p.lon_K_P = 1.0; p.lon_K_I = 0.05; p.lon_K_D = 0.0; p.dt = 0.05;
    p.max_throttle = 0.75; p.max_brake = 0.3; p.max_steer = 0.8; p.base_min_distance = 3.0; p.reserved = 0;
    const emp_behavior_params bp = {50.0, 3.0, 10.0, 3.0, 10.0, 5.0, 5.0, 0.5, 30.0, 5, 0};
    const emp_hazard_params hp = {5.0, 90.0, 10.0, 60.0, 0};
    const emp_vehicle_params vp = {1.015, 1.895, -148970.0, -82204.0, 1412.0, 1537.0, 0.05, 1.0, 3.0, 6.0, 0.0, 0};

    struct Run {
        std::vector<double> state, past, lon, lat, gap, wgap, l_state, l_ctl;
        std::vector<int> head, nlon, nlat, status, done, ticks, last, causes, l_mode, l_cause;
    };
    auto hazards = [&](emp_hazard_io& h) {
        memset(&h, 0, sizeof(h));
        h.n_light = n_light.data(); h.light = light.data(); h.light_lane = light_lane.data(); h.light_cycle = light_cycle.data();
        h.n_walker = n_walker.data(); h.walker = walker.data(); h.walker_lane = walker_lane.data();
    };
    auto rollout = [&](const Run* from, int ticks, int every_, long long tick0, bool logs) {
        Run r;
        const size_t nl = logs ? (size_t)((ticks + every_ - 1) / every_) : 0;
        r.state.assign((size_t)A * 6, -1.0); r.past.assign(A, -1.0); r.lon.assign((size_t)A * 10, -1.0); r.lat.assign((size_t)A * 10, -1.0);
        r.gap.assign(A, -1.0); r.wgap.assign(A, -1.0); r.head.assign(A, -1); r.nlon.assign(A, -1); r.nlat.assign(A, -1);
        r.status.assign(A, -1); r.done.assign(A, -9); r.ticks.assign((size_t)A * 5, -1); r.last.assign(A, -5); r.causes.assign((size_t)A * 3, -1);
        r.l_state.assign(nl * A * 6, -1.0); r.l_ctl.assign(nl * A * 3, -1.0); r.l_mode.assign(nl * A, -1); r.l_cause.assign(nl * A, -1);
        emp_behavior_io io;
        memset(&io, 0, sizeof(io));
        io.n_world = n_world.data(); io.path = path.data(); io.n_path = n_path.data(); io.lane = lane.data();
        io.state = from ? from->state.data() : state.data();
        io.speed_limit = limit.data(); io.extent = extent.data();
        io.head = from ? from->head.data() : head.data(); io.past_steer = from ? from->past.data() : past.data();
        io.lon_err = from ? from->lon.data() : lon.data(); io.n_lon = from ? from->nlon.data() : n_lon.data();
        io.lat_err = from ? from->lat.data() : lat.data(); io.n_lat = from ? from->nlat.data() : n_lat.data();
        io.head_out = r.head.data(); io.past_steer_out = r.past.data(); io.lon_err_out = r.lon.data(); io.n_lon_out = r.nlon.data();
        io.lat_err_out = r.lat.data(); io.n_lat_out = r.nlat.data(); io.status = r.status.data(); io.state_out = r.state.data();
        io.done_tick = r.done.data(); io.mode_ticks = r.ticks.data(); io.min_gap = r.gap.data();
        emp_hazard_io h;
        hazards(h);
        h.last_light = from ? from->last.data() : last0.data(); h.last_light_out = r.last.data();
        h.cause_ticks = r.causes.data(); h.min_walker_gap = r.wgap.data();
        if (logs) {
            io.log_state = r.l_state.data(); io.log_control = r.l_ctl.data(); io.log_mode = r.l_mode.data(); h.log_cause = r.l_cause.data();
        }
        hc_rollout(&p, &bp, &hp, &vp, W, N, M, 0, ML, MW, ticks, every_, tick0, &io, &h);
        return r;
    };
    const Run whole = rollout(nullptr, T, every, 0, true);
    int bad = 0;
    bad += whole.head[2] != -1 || whole.status[2] != -1 || whole.state[12] != -1.0 || whole.last[2] != -5 || whole.wgap[2] != -1.0 ||
           whole.l_cause[2] != -1;                                   // the padding slot of the outputs stays as it was
    Run first = rollout(nullptr, cut, 1, 0, false);
    const int held = first.last[0];
    first.head[2] = head[2]; first.nlon[2] = n_lon[2]; first.nlat[2] = n_lat[2];
    const Run second = rollout(&first, T - cut, 1, cut, false);
    bad += second.state != whole.state || second.head != whole.head || second.lon != whole.lon || second.lat != whole.lat ||
           second.past != whole.past || second.last != whole.last;

    // the chain of single ticks, in place
    std::vector<double> c_state = state, c_past = past, c_lon = lon, c_lat = lat, fw((size_t)A * 2, 0.0), kmh(A, 0.0), ctl3((size_t)A * 3, 0.0), dist(A),
                        ttc(A), tgt(A), wd(A), c_wgap(A, bhv::infinity());
    std::vector<int> c_head = head, c_nlon = n_lon, c_nlat = n_lat, c_last = last0, st(A, 0), mode(A, -1), blk(A), cause(A, -1), lhit(A), whit(A),
                     c_causes((size_t)A * 3, 0);
    for (int t = 0; t < T; ++t) {
        for (int a = 0; a < 2; ++a) {
            const agt::Obs o = agt::observe(c_state[6 * a + 2], c_state[6 * a + 3], c_state[6 * a + 5]);
            fw[2 * a] = o.c; fw[2 * a + 1] = o.s; kmh[a] = o.kmh;
        }
        emp_behavior_io io;
        memset(&io, 0, sizeof(io));
        io.n_world = n_world.data(); io.path = path.data(); io.n_path = n_path.data(); io.lane = lane.data(); io.state = c_state.data();
        io.forward = fw.data(); io.speed_kmh = kmh.data(); io.speed_limit = limit.data(); io.extent = extent.data();
        io.head = c_head.data(); io.past_steer = c_past.data(); io.lon_err = c_lon.data(); io.n_lon = c_nlon.data(); io.lat_err = c_lat.data();
        io.n_lat = c_nlat.data();
        io.head_out = c_head.data(); io.past_steer_out = c_past.data(); io.lon_err_out = c_lon.data(); io.n_lon_out = c_nlon.data();
        io.lat_err_out = c_lat.data(); io.n_lat_out = c_nlat.data(); io.status = st.data(); io.control = ctl3.data(); io.mode = mode.data();
        io.blocker = blk.data(); io.distance = dist.data(); io.ttc = ttc.data(); io.target_speed_out = tgt.data();
        emp_hazard_io h;
        hazards(h);
        h.last_light = c_last.data(); h.last_light_out = c_last.data(); h.cause = cause.data(); h.light_hit = lhit.data();
        h.walker_hit = whit.data(); h.walker_distance = wd.data();
        hc_behave(&p, &bp, &hp, W, N, M, 0, ML, MW, t, &io, &h);
        for (int a = 0; a < 2; ++a) {
            if (t % every == 0) {
                const size_t row = (size_t)(t / every) * A + a;
                bad += memcmp(&whole.l_state[6 * row], &c_state[6 * a], 48) != 0 || memcmp(&whole.l_ctl[3 * row], &ctl3[3 * a], 24) != 0 ||
                       whole.l_mode[row] != mode[a] || whole.l_cause[row] != cause[a];
            }
            if (cause[a] >= 1) ++c_causes[3 * a + cause[a] - 1];
            if (whit[a] >= 0 && wd[a] < c_wgap[a]) c_wgap[a] = wd[a];
            const double* q = &c_state[6 * a];
            const ctl::VehicleState n = ctl::vehicle_step(vehicle_of(&vp), ctl::VehicleState{q[0], q[1], q[2], q[3], q[4], q[5]}, ctl3[3 * a],
                                                          ctl3[3 * a + 1], ctl3[3 * a + 2]);
            const double v[6] = {n.x, n.y, n.fi, n.Vy, n.fi_dot, n.Vx};
            memcpy(&c_state[6 * a], v, 48);
        }
    }
    for (int a = 0; a < 2; ++a)
        bad += memcmp(&whole.state[6 * a], &c_state[6 * a], 48) != 0 || whole.head[a] != c_head[a] || whole.last[a] != c_last[a] ||
               memcmp(&whole.lon[10 * a], &c_lon[10 * a], 80) != 0 || memcmp(&whole.wgap[a], &c_wgap[a], 8) != 0 ||
               memcmp(&whole.causes[3 * a], &c_causes[3 * a], 12) != 0;
    // what the scene is for: agent 0 was stopped by the light, held by it at the cut, and went on; agent 1 saw the walker
    int wrong = 0;
    wrong += !(whole.causes[0] > 0 && held == 0 && whole.last[0] == -1 && whole.state[0] > 62.0);
    wrong += !(whole.wgap[1] < bhv::infinity() && whole.causes[3] == 0);
    printf("hazard_check: %d bad, %d wrong (agent 0: %d light ticks, ends at x %.2f; agent 1: %d walker ticks, min walker gap %.3f)\n", bad, wrong,
           whole.causes[0], whole.state[0], whole.causes[4], whole.wgap[1]);
    return bad != 0 || wrong != 0;
}
#endif
