"""Shared machinery of the ragged-batch GPU tests (test_gpu_frenet_batch.py, test_gpu_control_batch.py,
test_gpu_speed_backend_batch.py, test_gpu_cycle_batch.py, test_gpu_speed_front_batch.py): bit comparison, the batch-invariance runs and raw guarded
C-ABI calls.  A plain helper module (no fixtures, no hooks)."""
import numpy as np

from emplanner_carla_amd import _lib as L

F_GUARD = -7.25e77          # output guard sentinels
I_GUARD = -777


def bits(a):
    a = np.ascontiguousarray(a)
    return a.shape, a.dtype, a.tobytes()


def to_np(x):
    if x is None:
        return None
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def to_device(args):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x for x in args]


def invariant(call, args, what):
    """call(args, device) -> {name: array or None} for the batch ``args`` (arrays batch-major; anything else passed
    through).  Checks, bit for bit, that every scene's outputs are the same in the batch, on the device path (torch
    tensors), in the reversed batch, in the batch shifted by one (a copy of the middle scene in front, so every scene gets
    another wavefront / block partner) and alone (its B = 1 slice of the same padded arrays).  Returns the batch outputs."""
    full = call(args, False)
    B = next(x.shape[0] for x in args if isinstance(x, np.ndarray))
    sub = lambda f: [f(x) if isinstance(x, np.ndarray) else x for x in args]
    dev = call(to_device(args), True)
    for n, o in full.items():
        assert (o is None) == (dev[n] is None)
        assert o is None or bits(o) == bits(dev[n]), f"{what}: {n} differs between the host and the device call"
    rev = call(sub(lambda x: x[::-1].copy()), False)
    extra = B // 2
    sh = call(sub(lambda x: np.concatenate([x[extra:extra + 1], x])), False)
    for n, o in full.items():
        if o is None:
            continue
        bad = [b for b in range(B) if bits(o[b]) != bits(rev[n][B - 1 - b])]
        assert not bad, f"{what}: {n} of scenes {bad[:8]} changes when the batch is reversed"
        bad = [b for b in range(B) if bits(o[b]) != bits(sh[n][b + 1])]
        assert not bad, f"{what}: {n} of scenes {bad[:8]} changes when the batch is shifted by one"
        assert bits(sh[n][0]) == bits(o[extra]), f"{what}: {n} of the extra scene differs from its own"
    for b in range(B):
        one = call(sub(lambda x: x[b:b + 1]), False)
        for n, o in full.items():
            if o is not None:
                assert bits(o[b]) == bits(one[n][0]), f"{what}: {n} of scene {b} differs alone and in the batch"
    return full


class Guarded:
    """Raw EMP_DEVICE call on views into torch tensors with one guard row before and one after the batch.
    spec: dict(fn=<emp_* name>, sig=[argument names and scalars in call order], ins={name: (array, guard fill)},
    outs={name: (row shape, dtype)}, counts={name: capacity}).  A guard fill is a scalar or one row (an array of the row's
    shape)."""

    def __init__(self, pl, spec, B=None):
        import torch
        self.torch, self.pl, self.spec = torch, pl, spec
        self.B = B if B is not None else next(iter(spec["ins"].values()))[0].shape[0]
        self.t = {}
        for name, (arr, fill) in spec["ins"].items():
            arr = np.ascontiguousarray(arr[:self.B])
            t = torch.empty((self.B + 2,) + arr.shape[1:], dtype=torch.from_numpy(arr).dtype, device="cuda")
            if isinstance(fill, np.ndarray):
                fill = torch.from_numpy(np.ascontiguousarray(fill, dtype=arr.dtype)).cuda()
            t[0] = fill
            t[-1] = fill
            t[1:-1] = torch.from_numpy(arr).cuda()
            self.t[name] = t
        for name, (row, dt) in spec["outs"].items():
            tdt = torch.float64 if dt == np.float64 else torch.int32
            self.t[name] = torch.full((self.B + 2,) + tuple(row), F_GUARD if dt == np.float64 else I_GUARD, dtype=tdt,
                                      device="cuda")
        self.guard = {n: (self.t[n][0].clone(), self.t[n][-1].clone()) for n in spec["outs"]}

    def set_count(self, name, values):
        self.t[name][1:-1] = self.torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).cuda()

    def call(self):
        args = []
        for a in self.spec["sig"]:
            if a == "B":
                args.append(self.B)
            elif isinstance(a, str):
                args.append(self.t[a][1:].data_ptr())       # row 1 = scene 0 (B = 0: a pointer at the trailing guard)
            else:
                args.append(a)
        self.torch.cuda.synchronize()
        rc = getattr(self.pl._lib, self.spec["fn"])(self.pl._h, *args, L.EMP_DEVICE)
        assert rc == 0, f"{self.spec['fn']}: rc {rc}"
        self.pl.synchronize()
        return {n: self.t[n][1:-1].cpu().numpy().copy() for n in self.spec["outs"]}

    def check_guards(self, what):
        for n, (g0, g1) in self.guard.items():
            assert self.torch.equal(self.t[n][0], g0) and self.torch.equal(self.t[n][-1], g1), \
                f"{what}: a guard row of {n} was written"
        if self.B == 0:
            for n in self.spec["outs"]:
                assert self.torch.equal(self.t[n][1], self.guard[n][0]), f"{what}: B = 0 wrote {n}"


def check_count_contract(pl, spec, wild_rows, what):
    """One middle scene and the last scene at capacity + 3, one scene at -1 (wild_rows = (mid, neg)), for each count of
    spec["counts"]: both guard rows unchanged, every other scene bit-equal to the clean call, the wild scenes bit-equal to
    the call with their counts clamped to [0, capacity]."""
    assert all(cap >= 3 for cap in spec["counts"].values())
    g = Guarded(pl, spec)
    B = g.B
    clean = g.call()
    g.check_guards(f"{what} clean")
    mid, neg = wild_rows
    wild_ix = [mid, neg, B - 1]
    others = np.setdiff1d(np.arange(B), wild_ix)
    for cname, cap in spec["counts"].items():
        base = np.array(spec["ins"][cname][0], dtype=np.int32)
        wild = base.copy()
        wild[[mid, B - 1]] = cap + 3
        wild[neg] = -1
        g.set_count(cname, wild)
        got = g.call()
        g.check_guards(f"{what} with {cname} wild")
        g.set_count(cname, np.clip(wild, 0, cap))
        clamped = g.call()
        g.set_count(cname, base)
        for n in spec["outs"]:
            assert bits(got[n][others]) == bits(clean[n][others]), \
                f"{what}: {cname} beyond the capacity changed another scene's {n}"
            for b in wild_ix:
                assert bits(got[n][b]) == bits(clamped[n][b]), \
                    f"{what}: scene {b} with {cname} = {wild[b]} differs from the clamped count ({n})"


CYCLE_OUTS = ("dp_rows", "dp_s", "dp_l", "dp_len", "path_s", "path_l", "path_len", "traj", "traj_len", "status")


class GuardedCycle:
    """Guarded's sibling for calls that take an emp_cycle_io: a raw EMP_DEVICE emp_plan_cycle on views into torch tensors with
    one guard row before and one after the batch.  ins: plan_cycle's array inputs by name (ref_line, n_ref, origin_xy, start_xy,
    start_v, start_a, obs_xy, n_obs); fills: name -> guard fill (a scalar or one row), 0 where absent; p, q, sp: the parameter
    structs; max_pts: the output capacity."""

    def __init__(self, pl, p, q, sp, ins, fills, max_pts, mode=L.EMP_DP_TWO_KERNEL, B=None):
        import torch
        self.torch, self.pl, self.p, self.q, self.sp, self.mode = torch, pl, p, q, sp, mode
        self.B = B if B is not None else len(ins["n_ref"])
        self.P, self.mo, self.M = ins["ref_line"].shape[1], ins["obs_xy"].shape[1], int(max_pts)
        self.t = {}
        for name, arr in ins.items():
            arr = np.ascontiguousarray(arr[:self.B])
            t = torch.empty((self.B + 2,) + arr.shape[1:], dtype=torch.from_numpy(arr).dtype, device="cuda")
            fill = fills.get(name, 0)
            if isinstance(fill, np.ndarray):
                fill = torch.from_numpy(np.ascontiguousarray(fill, dtype=arr.dtype)).cuda()
            t[0] = fill
            t[-1] = fill
            t[1:-1] = torch.from_numpy(arr).cuda()
            self.t[name] = t
        M = self.M
        rows = dict(dp_rows=(int(p.col),), dp_s=(M,), dp_l=(M,), dp_len=(), path_s=(M,), path_l=(M,), path_len=(), traj=(M + 1, 4),
                    traj_len=(), status=())
        self.outs = CYCLE_OUTS
        self.spec = {"outs": CYCLE_OUTS}                  # what Guarded.check_guards walks
        for name in self.outs:
            integer = name in ("dp_len", "path_len", "traj_len", "status")
            self.t[name] = torch.full((self.B + 2,) + rows[name], I_GUARD if integer else F_GUARD,
                                      dtype=torch.int32 if integer else torch.float64, device="cuda")
        self.guard = {n: (self.t[n][0].clone(), self.t[n][-1].clone()) for n in self.outs}

    def set_count(self, name, values):
        self.t[name][1:-1] = self.torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).cuda()

    def call(self):
        import ctypes as C
        io = L.CycleIO()
        for name, t in self.t.items():
            setattr(io, name, C.c_void_p(t[1:].data_ptr()))           # row 1 = scene 0 (B = 0: a pointer at the trailing guard)
        self.torch.cuda.synchronize()
        rc = self.pl._lib.emp_plan_cycle(self.pl._h, C.byref(self.p), C.byref(self.q), C.byref(self.sp), self.B, self.P, self.mo,
                                         self.M, int(self.mode), C.byref(io), L.EMP_DEVICE)
        assert rc == 0, f"emp_plan_cycle: rc {rc}"
        self.pl.synchronize()
        return {n: self.t[n][1:-1].cpu().numpy().copy() for n in self.outs}

    check_guards = Guarded.check_guards
