#!/usr/bin/env python3
"""How a kernel's cross-lane reductions were compiled, read from a gfx950 listing (the listing of tools/launch_head_listing.py
and tools/launch_tail_listing.py, or the same command on csrc/dec_api.hip):

    tools/xlane_listing.py fmt_api.s [regex of demangled kernel names]

Per kernel, in listing order: the ds_bpermute_b32 (what __shfl_xor compiles to: an LDS-pipe round trip each), the
v_permlane{16,32}_swap and the VALU instructions with a DPP operand; the s_waitcnt lgkmcnt(..) between the first and the last
of these cross-lane instructions (each one a stop of the wave's only instruction stream); and from the kernel descriptor the
VGPRs, the waves per SIMD they allow and the scratch bytes.  Default: LayerNorm and attention of the step chain."""
import re
import sys

from launch_head_listing import demangle, kernels
from launch_tail_listing import descriptor

DEFAULT = r"fmt_lnmod_kernel<FP16, 4, [04], true, true>|fmt_attn_kernel<FP16, 16, true, true>"
DPP = re.compile(r"\b(quad_perm|row_shl|row_shr|row_ror|row_mirror|row_half_mirror|row_bcast|row_newbcast)\b")


def main():
    path = sys.argv[1]
    pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else DEFAULT)
    ks, desc = kernels(path), descriptor(path)
    names = demangle(list(ks))
    for sym in sorted(ks, key=lambda s: names[s]):
        if not pat.search(names[sym]):
            continue
        insns = [l.split(";")[0].strip() for l in ks[sym][0]]
        insns = [l for l in insns if l and not l.startswith(".") and not l.endswith(":")]
        kind = ["bpermute" if l.startswith("ds_bpermute_b32") else "swap" if l.startswith("v_permlane") else
                "dpp" if DPP.search(l) else None for l in insns]
        at = [i for i, k in enumerate(kind) if k]
        waits = [l for l in insns[at[0]:at[-1]] if l.startswith("s_waitcnt") and "lgkmcnt" in l] if at else []
        vgpr, scratch = desc.get(sym, (0, 0))
        print(re.sub(r"^void |\(.*$", "", names[sym]))
        print("    ds_bpermute_b32 %d, v_permlane*_swap %d, DPP %d; lgkmcnt waits between the first and the last of them: %d" %
              (kind.count("bpermute"), kind.count("swap"), kind.count("dpp"), len(waits)))
        print("    vgprs %d (%d waves/SIMD), scratch %d B" % (vgpr, min(8, 512 // max(8, (vgpr + 7) // 8 * 8)), scratch))


if __name__ == "__main__":
    main()
