#!/usr/bin/env python3
"""What stands behind a kernel's last matrix instruction, read from a gfx950 listing of csrc/fmt_api.hip (the sibling of
tools/launch_head_listing.py, same listing):

    hipcc <the Makefile's CXXFLAGS without -fPIC> <FLAGS_fmt_api> --cuda-device-only -S fmt_api.hip -o fmt_api.s
    tools/launch_tail_listing.py fmt_api.s [regex of demangled kernel names] [-v]

In a launch-bound chain the code between the last MFMA and s_endpgm is as serial as the code in front of the first load.  Per
kernel, along the LONGEST path (in instructions, loop back edges not taken) from the start point to an s_endpgm:
  * start point: the last v_mfma of the listing (a kernel that carries two forms of its body lists the straight-line form, the
    one the step chain runs, last); for kernels without MFMA (LayerNorm, attention) the last 16-byte global load - the last
    operand the output depends on (the touches of later weights are single dwords);
  * `insns`: instructions on the path;
  * `vmcnt` / `lgkmcnt`: the s_waitcnt values on the path in order - a vmcnt(0) that is not the last one is a full wait for
    global memory in front of dependent work;
  * `loads behind barrier`: global loads issued on the path behind its last s_barrier (operands fetched late; for the kernels
    without a barrier: behind the start point);
  * `lds st/ld`: the LDS store and load instructions on the path by mnemonic (the K-split exchange);
and from the kernel descriptor the unified VGPR count, the waves per SIMD that count allows (512 registers per lane and SIMD,
granule 8, at most 8 waves) and the scratch bytes (spills).  -v prints the path's waits, barriers, loads and LDS instructions
in order.  Default: the step chain's seven kernels."""
import re
import sys

from launch_head_listing import CHAIN, demangle, kernels


def descriptor(path):
    """{symbol: (next_free_vgpr, scratch bytes)} from the .amdhsa_kernel blocks."""
    out, cur = {}, None
    for l in open(path):
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", l)
        if m:
            cur = m.group(1)
            out[cur] = [0, 0]
        elif cur:
            m = re.match(r"^\s*\.amdhsa_next_free_vgpr (\d+)", l)
            if m:
                out[cur][0] = int(m.group(1))
            m = re.match(r"^\s*\.amdhsa_private_segment_fixed_size (\d+)", l)
            if m:
                out[cur][1] = int(m.group(1))
            if ".end_amdhsa_kernel" in l:
                cur = None
    return out


def parse(body):
    insns, labels = [], {}
    for l in body:
        l = l.split(";")[0].strip()
        if not l or l.startswith("."):
            m = re.match(r"^(\.L\w+):", l)
            if m:
                labels[m.group(1)] = len(insns)
            continue
        insns.append(l)
    return insns, labels


def tail(body):
    """(start kind, path) - the longest forward path, as a list of instructions, from the start point to an s_endpgm."""
    insns, labels = parse(body)
    mf = [i for i, l in enumerate(insns) if l.startswith("v_mfma")]
    if mf:
        kind, start = "mfma", mf[-1]
    else:
        ld = [i for i, l in enumerate(insns) if l.startswith("global_load_dwordx4")]
        if not ld:
            return None, []
        kind, start = "load", ld[-1]
    # successors per instruction; the edges that close a loop (to an instruction on the depth-first stack) are dropped, so a
    # loop counts one trip and the longest path is well defined
    n = len(insns)

    def succ(i):
        l, out = insns[i], []
        if l.startswith("s_endpgm"):
            return out
        if l.startswith("s_branch") or l.startswith("s_cbranch"):
            t = labels.get(l.split()[1])
            if t is not None:
                out.append(t)
        if not l.startswith("s_branch") and i + 1 < n:
            out.append(i + 1)
        return out

    edges, state, stack = {}, {start: 1}, [(start, iter(succ(start)))]
    while stack:
        i, it = stack[-1]
        j = next(it, None)
        if j is None:
            state[i] = 2
            stack.pop()
        elif state.get(j) == 1:
            continue  # back edge
        else:
            edges.setdefault(i, []).append(j)
            if j not in state:
                state[j] = 1
                stack.append((j, iter(succ(j))))
    order, best, nxt = [], {}, {}
    seen, stack = {start}, [(start, iter(edges.get(start, [])))]
    while stack:  # post order of the loop-free graph
        i, it = stack[-1]
        j = next(it, None)
        if j is None:
            order.append(i)
            stack.pop()
        elif j not in seen:
            seen.add(j)
            stack.append((j, iter(edges.get(j, []))))
    for i in order:
        if insns[i].startswith("s_endpgm"):
            best[i] = 1
        for j in edges.get(i, []):
            if j in best and best[j] + 1 > best.get(i, 0):
                best[i], nxt[i] = best[j] + 1, j
    path, i = [], start
    while i is not None and i in best:
        path.append(insns[i])
        i = nxt.get(i)
    return kind, path[1:]  # behind the start point


def summary(path):
    vm, lg, loads, st, ld = [], [], 0, {}, {}
    for l in path:
        op = l.split()[0]
        if op == "s_waitcnt":
            vm += re.findall(r"vmcnt\((\d+)\)", l)
            lg += re.findall(r"lgkmcnt\((\d+)\)", l)
        elif op == "s_barrier":
            loads = 0
        elif op.startswith("global_load") or op.startswith("buffer_load"):
            loads += 1
        elif op.startswith("ds_write"):
            st[op] = st.get(op, 0) + 1
        elif op.startswith("ds_read"):
            ld[op] = ld.get(op, 0) + 1
    fmt = lambda d: " ".join("%dx%s" % (v, k) for k, v in sorted(d.items())) or "-"  # noqa: E731
    return vm, lg, loads, fmt(st), fmt(ld)


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    path = args[0]
    pat = re.compile(args[1] if len(args) > 1 else CHAIN)
    ks, desc = kernels(path), descriptor(path)
    names = demangle(list(ks))
    for sym in sorted(ks, key=lambda s: names[s]):
        if not pat.search(names[sym]):
            continue
        kind, p = tail(ks[sym][0])
        vgpr, scratch = desc.get(sym, (0, 0))
        waves = min(8, 512 // max(8, (vgpr + 7) // 8 * 8))
        print(re.sub(r"^void |\(.*$", "", names[sym]))
        print("    vgprs %d (%d waves/SIMD), scratch %d B" % (vgpr, waves, scratch))
        if kind is None:
            print("    no MFMA and no 16-byte load")
            continue
        vm, lg, loads, st, ld = summary(p)
        print("    from the last %s: %d insns; vmcnt [%s]; lgkmcnt [%s]" % (kind, len(p), " ".join(vm), " ".join(lg)))
        print("    loads behind barrier: %d; lds st: %s; lds ld: %s" % (loads, st, ld))
        if verbose:
            for l in p:
                if re.match(r"s_waitcnt|s_barrier|global_|buffer_|ds_|s_endpgm", l):
                    print("        " + l)


if __name__ == "__main__":
    main()
