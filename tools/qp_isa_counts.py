"""Static instruction counts of the path-QP rows kernels from the device assembly (no GPU needed):

    hipcc <FLAGS of emplanner_carla_amd/build.py without -shared> --cuda-device-only -S csrc/emp_api.hip -o emp_api.s
    python tools/qp_isa_counts.py emp_api.s [more.s ...]

Per kernel: register allocation, scratch, and for the interior-point loop - the widest backward branch of the kernel, which
contains the lane-step loops of the factorisation and the substitutions once each - the vector, select, scalar, exec-save,
LDS and barrier instructions as written (static: a lane-step loop's body counts once)."""
import re
import sys

KERNELS = ("cycle_qp_rows_kernelILi8ELi3E", "cycle_qp_rows_kernelILi8ELi4E", "cycle_qp_rows_kernelILi16ELi4E")


def body(lines, key):
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN3emp") and key in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def meta(lines, key):
    at = next(i for i, l in enumerate(lines) if ".name:" in l and key in l and not l.rstrip().endswith(".kd"))
    lo = max(i for i in range(at) if lines[i].lstrip().startswith("- .a"))      # start of this kernel's metadata entry
    hi = next((i for i in range(at + 1, len(lines)) if lines[i].lstrip().startswith("- .a")), len(lines))
    out = {}
    for l in lines[lo:hi]:
        m = re.match(r"\s+\.(sgpr_count|vgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def loop_counts(b):
    label_at = {}
    for i, l in enumerate(b):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i
    best = (0, 0, 0)
    for i, l in enumerate(b):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)|\s+s_branch\s+(\.LBB\d+_\d+)", l)
        if m:
            t = label_at.get(m.group(1) or m.group(2), i)
            if t < i and i - t > best[0]:
                best = (i - t, t, i)
    ins = [l.split()[0] for l in b[best[1]:best[2] + 1] if re.match(r"\s+[a-z]", l) and not l.lstrip().startswith((".", ";"))]
    n = lambda pred: sum(1 for x in ins if pred(x))
    return dict(all=len(ins), vector=n(lambda x: x.startswith("v_")), v_cndmask=n(lambda x: x.startswith("v_cndmask")),
                v_cmp=n(lambda x: x.startswith("v_cmp")), scalar=n(lambda x: x.startswith("s_")),
                exec_save=n(lambda x: "saveexec" in x), lds=n(lambda x: x.startswith("ds_")),
                waitcnt=n(lambda x: x.startswith("s_waitcnt")), barrier=n(lambda x: x.startswith("s_barrier")),
                dpp_or_mov=n(lambda x: x.startswith("v_mov")))


if __name__ == "__main__":
    for path in sys.argv[1:]:
        lines = open(path).read().splitlines()
        for k in KERNELS:
            print(path, k, meta(lines, k), "loop:", loop_counts(body(lines, k)), flush=True)
