#!/usr/bin/env python3
"""What stands in front of a kernel's first operand load, read from a gfx950 listing of csrc/fmt_api.hip:

    hipcc <the Makefile's CXXFLAGS without -fPIC> <FLAGS_fmt_api> --cuda-device-only -S fmt_api.hip -o fmt_api.s
    tools/launch_head_listing.py fmt_api.s [regex of demangled kernel names]

Per kernel: the kernarg preload length of its descriptor, the instructions executed from its entry to the first operand or row
load (a 16-byte global load; for a preloading kernel the entry is the one behind the compatibility prologue's s_branch, which
only firmware without preload executes) along the shortest path, and how many `s_waitcnt lgkmcnt(0)` - scalar-memory round
trips - that path holds.  Default: the step chain's seven kernels."""
import re
import subprocess
import sys

CHAIN = (r"fmt_gemm_kernel<FP16, 3, 4, 8, [137]>|fmt_gemm_kernel<FP16, 3, 1, 8, 4>|fmt_lnmod_kernel<FP16, 4, [04], true, true>|"
         r"fmt_attn_kernel<FP16, 16, true, true>")


def demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def kernels(path):
    """{symbol: (body lines, preload length)} of every .amdhsa_kernel of the listing."""
    lines = open(path).read().split("\n")
    starts = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            starts[m.group(1)] = i
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", l)
        if m and m.group(1) in starts:
            pre = 0
            for k in lines[i:i + 80]:
                p = re.match(r"^\s*\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", k)
                if p:
                    pre = int(p.group(1))
            out[m.group(1)] = (lines[starts[m.group(1)] + 1:i], pre)
    return out


def head(body, preload):
    """(instructions executed up to and including the first 16-byte global load, lgkmcnt(0) waits among them) along the
    shortest path from the kernel's entry: operand and row loads are dwordx4, the touches of later weights single dwords."""
    insns, labels = [], {}
    for l in body:
        l = l.split(";")[0].strip()
        if not l or l.startswith("."):
            m = re.match(r"^(\.L\w+):", l)
            if m:
                labels[m.group(1)] = len(insns)
            continue
        insns.append(l)
    start = 0
    if preload:  # the prologue (s_load ... s_waitcnt, s_branch to the entry) is only run by firmware that does not preload
        for i, l in enumerate(insns[:16]):
            if l.startswith("s_branch"):
                start = labels[l.split()[1]]
                break
    dist, todo = {start: (1, None)}, [start]
    while todo:  # breadth first over single instructions = fewest instructions first
        nxt = []
        for i in todo:
            l = insns[i]
            if l.startswith("global_load_dwordx4"):
                n, waits, j = dist[i][0], 0, i
                while j is not None:
                    waits += bool(re.match(r"s_waitcnt.*lgkmcnt\(0\)", insns[j]))
                    j = dist[j][1]
                return n, waits
            succ = []
            if l.startswith("s_branch") or l.startswith("s_cbranch"):
                succ.append(labels[l.split()[1]])
            if not l.startswith("s_branch") and not l.startswith("s_endpgm") and i + 1 < len(insns):
                succ.append(i + 1)
            for j in succ:
                if j not in dist:
                    dist[j] = (dist[i][0] + 1, i)
                    nxt.append(j)
        todo = nxt
    return None, 0


def main():
    path = sys.argv[1]
    pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else CHAIN)
    ks = kernels(path)
    names = demangle(list(ks))
    print("%-58s %8s %12s %14s" % ("kernel", "preload", "first load", "lgkmcnt(0) before"))
    for sym in sorted(ks, key=lambda s: names[s]):
        if not pat.search(names[sym]):
            continue
        body, pre = ks[sym]
        n, w = head(body, pre)
        short = re.sub(r"^void |\(.*$", "", names[sym])
        print("%-58s %8d %12s %14d" % (short, pre, n, w))


if __name__ == "__main__":
    main()
