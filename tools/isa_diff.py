#!/usr/bin/env python3
"""Device assembly of two builds, function by function.

    hipcc <the library's flags> -S --cuda-device-only csrc/emp_api.hip -o a.s      (once per build)
    python tools/isa_diff.py a.s b.s [--all]

For a refactor that must leave the kernels alone: the same set of functions, the same resource figures (registers, LDS,
scratch, spills, occupancy, kernel descriptor) for each, and - with block labels and comments stripped - which functions'
instructions differ, by how many lines.  Prints a summary and a markdown table of the functions that differ (--all: of
every function); exits 1 if the function sets or any resource figure differ, 0 otherwise (differing instructions alone
are reported, not judged).
"""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

FIGURES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
SPILLS = (".sgpr_spill_count", ".vgpr_spill_count")


def functions(path):
    """name -> {"code": [normalised lines], "desc": [.amdhsa_ lines], "fig": {figure: value}}"""
    out, cur, part = {}, None, None
    meta_name = None
    for raw in open(path, errors="replace"):
        line = raw.rstrip("\n")
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur, part = {"code": [], "desc": [], "fig": {}}, "code"
            out[m.group(1)] = cur
            continue
        m = re.match(r"\s*\.name:\s+(\S+)", line)                  # the code object's metadata, behind all functions
        if m:
            meta_name = m.group(1)
            continue
        m = re.match(r"\s*(\.\w+_spill_count):\s+(\d+)", line)
        if m and meta_name in out:
            out[meta_name]["fig"][m.group(1)] = m.group(2)
            continue
        if cur is None:
            continue
        if part == "code":
            if re.match(r"\s*\.section\s", line) or re.match(r"\.Lfunc_end\d+:", line):
                part = "tail"
            else:
                text = re.sub(r"\.LBB\d+_\d+", ".LBB", line.split(";")[0]).strip()
                if text:
                    cur["code"].append(text)
                continue
        if re.match(r"\s*\.amdhsa_", line):
            cur["desc"].append(line.strip())
        m = re.match(r";\s*(\w+)\s*[:=]\s*(\d+)", line)
        if m and m.group(1) in FIGURES:
            cur["fig"][m.group(1)] = m.group(2)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    short = lambda s: re.sub(r"\(.*", "", s)                         # the arguments say nothing the name does not
    return {n: short(r) for n, r in zip(names, res)} if len(res) == len(names) else {n: n for n in names}


def instructions(code):
    return sum(1 for t in code if not t.endswith(":") and not t.startswith("."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--all", action="store_true", help="list every function, not only those that differ")
    args = ap.parse_args()
    A, B = functions(args.a), functions(args.b)
    both = [n for n in A if n in B]
    print(f"functions: {len(A)} / {len(B)}; only in {args.a}: {sorted(set(A) - set(B))}; only in {args.b}: {sorted(set(B) - set(A))}")
    fig_diff = [n for n in both if A[n]["fig"] != B[n]["fig"]]
    desc_diff = [n for n in both if A[n]["desc"] != B[n]["desc"]]
    code_diff = [n for n in both if A[n]["code"] != B[n]["code"]]
    print(f"of {len(both)} common functions: resource figures differ for {len(fig_diff)}, kernel descriptors for {len(desc_diff)}, "
          f"instructions for {len(code_diff)}")
    listed = both if args.all else [n for n in both if n in fig_diff or n in desc_diff or n in code_diff]
    names = demangle(listed)
    keys = FIGURES + SPILLS
    print("\n| function | lines a / b | lines - / + | instructions a / b | " + " | ".join(k.lstrip(".") for k in keys) + " |")
    print("|---|---|---|---|" + "---|" * len(keys))
    for n in listed:
        a, b = A[n], B[n]
        d = list(difflib.unified_diff(a["code"], b["code"], n=0, lineterm="")) if n in code_diff else []
        minus = sum(1 for t in d if t.startswith("-") and not t.startswith("---"))
        plus = sum(1 for t in d if t.startswith("+") and not t.startswith("+++"))
        figs = []
        for k in keys:
            x, y = a["fig"].get(k, "-"), b["fig"].get(k, "-")
            figs.append(x if x == y else f"**{x} -> {y}**")
        print(f"| `{names[n]}` | {len(a['code'])} / {len(b['code'])} | {minus} / {plus} | {instructions(a['code'])} / {instructions(b['code'])} | "
              + " | ".join(figs) + " |")
    return 1 if (set(A) != set(B) or fig_diff or desc_diff) else 0


if __name__ == "__main__":
    sys.exit(main())
