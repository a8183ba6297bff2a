"""Python-float port of the timed rollout's sampling rule (csrc/emp_control_core.h: ctl::speed_target, the arithmetic of
emp_speed_target and emp_rollout_timed), operation by operation as include/emplanner.h states it, the case generator the CPU and
GPU suites share, and the CPU closed loop that tracks a profile.  The rule is the project's own definition (the reference drives
with a constant ref_speed).  Test tool only: the package never imports it."""
from __future__ import annotations

import math

import numpy as np

N = 401                                     # EMP_TIMED_POINTS
BEFORE, PAST, NO_PROFILE, CAPPED = 1, 2, 4, 8
NAN = float("nan")


def profile_count(speed, time):
    """n_v: the leading samples in which neither the time nor the speed is NaN."""
    n = 0
    while n < N and not (time[n] != time[n]) and not (speed[n] != speed[n]):
        n += 1
    return n


def clock_of(t0, tick, dt):
    return float(t0) + float(tick) * float(dt)


def speed_target(speed, time, n_v, clock, cap, cursor):
    """One tick: (target km/h, outgoing cursor, bits)."""
    cursor = int(cursor)
    if n_v <= 0 or clock != clock:
        return cap, (0 if n_v <= 0 else cursor), NO_PROFILE
    bits = 0
    if clock < time[0]:
        v, bits = speed[0], BEFORE
    elif clock >= time[n_v - 1]:
        v, bits = speed[n_v - 1], PAST
    else:
        j = min(max(cursor, 0), n_v - 2)
        while j + 1 <= n_v - 2 and time[j + 1] <= clock:
            j += 1
        d = time[j + 1] - time[j]
        v = speed[j]
        if d > 0.0:
            w = (clock - time[j]) / d
            v = speed[j] + w * (speed[j + 1] - speed[j])
        cursor = j
    target = 3.6 * v
    if target > cap:
        target, bits = cap, bits | CAPPED
    return target, cursor, bits


def sample(traj, t0, tick, dt, cap, cursor):
    """emp_speed_target on one vehicle's (7, 401) trajectory, all Python floats."""
    speed, time = [float(v) for v in traj[4]], [float(v) for v in traj[6]]
    return speed_target(speed, time, profile_count(speed, time), clock_of(t0, tick, dt), float(cap), int(cursor))


# -----------------------------------------------------------------------------------------------------------------------------
# the case generator: every vehicle / case gets its own (trajectory, t0, cap, cursor); `tick` and `dt` are the caller's
# -----------------------------------------------------------------------------------------------------------------------------
KINDS = ("full", "n0", "n1", "n2", "n3", "n400", "nan_speed", "nan_time", "equal_times", "backwards", "short_row")
CLOCKS = ("before", "on_sample", "between", "on_last", "past", "nan")


def make_case(rng, kind=None, where=None, tick=0, dt=0.01):
    """One case: dict(traj (7, 401), t0, cap, cursor, kind, where).  `where` places the clock of tick `tick` and t0 is solved
    from it: with tick = 0 the clock IS t0 and 'on a sample' is exact; with another tick it holds up to the rounding of
    t0 + tick * dt (the expected result always comes from the port, never from the label)."""
    kind = kind or KINDS[int(rng.integers(len(KINDS)))]
    where = where or CLOCKS[int(rng.integers(len(CLOCKS)))]
    traj = rng.normal(0.0, 30.0, (7, N))
    T = float(rng.uniform(2.0, 9.0))
    base = float(rng.choice([0.0, 0.1, 12.5, 1234.0]))
    time = np.array([(i - 1) * T / 400 for i in range(1, N + 1)]) + base          # increase_points: (i - 1) * T / 400
    v0, v1 = rng.uniform(0.0, 20.0, 2)
    speed = v0 + (v1 - v0) * np.linspace(0.0, 1.0, N) + rng.normal(0.0, 0.05, N)
    n_v = N
    if kind in ("n0", "n1", "n2", "n3", "n400"):
        n_v = {"n0": 0, "n1": 1, "n2": 2, "n3": 3, "n400": 400}[kind]
        (speed if rng.random() < 0.5 else time)[n_v] = NAN
        if n_v < 399 and rng.random() < 0.5:
            speed[n_v + 1:], time[n_v + 1:] = rng.normal(0, 5, N - n_v - 1), rng.normal(0, 5, N - n_v - 1)    # junk behind the NaN
    elif kind == "nan_speed":
        n_v = int(rng.integers(4, 400))
        speed[n_v] = NAN
    elif kind == "nan_time":
        n_v = int(rng.integers(4, 400))
        time[n_v] = NAN
    elif kind == "equal_times":
        k = int(rng.integers(1, 399))
        time[k + 1] = time[k]
    elif kind == "backwards":
        k = int(rng.integers(2, 398))
        time[k + 1] = time[k - 1] - 0.003
    elif kind == "short_row":
        n_v = int(rng.integers(4, 60))
        time[n_v:] = NAN
    traj[4], traj[6] = speed, time
    if n_v == 0 or where == "nan":
        clock = NAN if where == "nan" else base + 1.0
    elif where == "before":
        clock = time[0] - float(rng.uniform(1e-9, 3.0))
    elif where == "on_sample":
        clock = time[int(rng.integers(0, n_v))]
    elif where == "between":
        k = int(rng.integers(0, max(1, n_v - 1)))
        clock = time[k] + float(rng.uniform(0.0, 1.0)) * (time[min(k + 1, n_v - 1)] - time[k])
    elif where == "on_last":
        clock = time[n_v - 1]
    else:
        clock = time[n_v - 1] + float(rng.uniform(0.0, 3.0))
    t0 = clock - float(tick) * dt                                                # exact for tick 0: the clock IS the sample then
    vmax = 3.6 * max(float(np.nanmax(np.abs(speed[:max(n_v, 1)]))) if n_v else 10.0, 1.0)
    cap = float(rng.choice([vmax + 5.0, 0.5 * vmax, NAN, 50.0, 3.6 * float(speed[0]) if speed[0] == speed[0] else 20.0]))
    cursor = int(rng.choice([0, 0, int(rng.integers(0, N)), -5, 2 ** 31 - 1, -2 ** 31, n_v - 2, n_v - 1, 1000]))
    return dict(traj=traj, t0=t0, cap=cap, cursor=cursor, kind=kind, where=where)


def make_cases(n, seed, tick=0, dt=0.01):
    """n cases covering every (kind, clock) pair in turn, then random ones: arrays traj (n, 7, 401), t0, cap, cursor + labels."""
    rng = np.random.default_rng(seed)
    pairs = [(k, w) for k in KINDS for w in CLOCKS]
    cases = [make_case(rng, *(pairs[i % len(pairs)] if i < 2 * len(pairs) else (None, None)), tick=tick, dt=dt) for i in range(n)]
    return dict(traj=np.array([c["traj"] for c in cases]), t0=np.array([c["t0"] for c in cases]),
                cap=np.array([c["cap"] for c in cases]), cursor=np.array([c["cursor"] for c in cases], np.int32),
                kind=[c["kind"] for c in cases], where=[c["where"] for c in cases])


def port_batch(c, tick, dt, cursor=None):
    """The port on every case of make_cases' arrays: (target (n,), cursor (n,) int32, bits (n,) int32)."""
    cur = c["cursor"] if cursor is None else cursor
    out = [sample(c["traj"][i], c["t0"][i], tick, dt, c["cap"][i], cur[i]) for i in range(len(c["t0"]))]
    return (np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.int32))


# -----------------------------------------------------------------------------------------------------------------------------
# the CPU closed loop that tracks a profile: vehicle_port.closed_loop_mpc with the rule in front of the PID
# -----------------------------------------------------------------------------------------------------------------------------
def closed_loop_mpc_timed(prm, path, state, min_index, cap, traj, t0, T, tick0=0, cursor=0, gains=(1.15, 0.0, 0.0, 0.01, 1.0)):
    """T ticks of one vehicle.  Returns states (T, 6), controls (T, 3), targets (T,), the final state, the final cursor and the OR
    of the ticks' bits.  traj = None: the constant target `cap` (vehicle_port.closed_loop_mpc's loop)."""
    import vehicle_port as vp
    from oracle import mpc_lateral as mpc
    para = tuple(float(v) for v in prm[:6])
    dt = float(prm[6])
    state = tuple(float(v) for v in state)
    if traj is not None:
        speed, time = [float(v) for v in traj[4]], [float(v) for v in traj[6]]
        n_v = profile_count(speed, time)
    buf, bits_or = [], 0
    S, U, G = [], [], []
    for t in range(T):
        r = mpc.lateral_mpc(path, state[:5], vp.clamp_vx(state[5]), int(min_index), para)
        min_index = r["min_index"]
        target = float(cap)
        if traj is not None:
            target, cursor, bits = speed_target(speed, time, n_v, clock_of(t0, tick0 + t, dt), float(cap), cursor)
            bits_or |= bits
        acc, buf = vp.pid_step(gains, vp.speed_kmh(state[5], state[3]), target, buf)
        u = vp.actuate(r["steering"], acc)
        S.append(state)
        U.append(u)
        G.append(target)
        state = vp.step(prm, state, u)
    return np.array(S), np.array(U), np.array(G), np.array(state), cursor, bits_or


def braking_profile():
    """The tracking test's profile: times (i - 1) * 0.02 + 0.1, 10 m/s falling linearly to 6 m/s over the first 2 s, then constant;
    the rows that are not read hold NaN."""
    traj = np.full((7, N), NAN)
    time = np.array([(i - 1) * 0.02 + 0.1 for i in range(1, N + 1)])
    rel = np.array([(i - 1) * 0.02 for i in range(1, N + 1)])
    traj[6] = time
    traj[4] = np.where(rel < 2.0, 10.0 - 4.0 * (rel / 2.0), 6.0)
    return traj
