#!/usr/bin/env python3
"""Build guard: the register budget of large_syrk_bf16x3<false> (ekf_large.h).  The kernel runs three workgroups of four waves per CU, which takes
168 VGPRs per lane at most (512 / 3, in steps of 8) -- __launch_bounds__(256, 3) makes the compiler keep that and SPILL what does not fit.  The
tail path (large_syrk_tail) keeps its slab-to-slab state in accumulators that are dead on its wave, and its wave-uniform condition is left to the
compiler as a divergent one, because the other forms made hipcc spill accumulators inside the K loop.  That is a dependency on the compiler's
behaviour; this guard is what notices when a toolchain stops honouring it: the kernel's scratch must not exceed the few bytes of loop-invariant
values spilled around the K loop (12 bytes before the tail path, 8 with it).

usage: check_syrk_budget.py file.s     exit 1 and a report when the budget is exceeded"""
import re
import sys

KERNEL = "_ZN5aslam17large_syrk_bf16x3ILb0EEEvNS_7DevViewENS_9LargeViewIfEEiPKi"
MAX_VGPR = 168     # three workgroups of 256 threads per CU
MAX_SCRATCH = 16   # bytes per lane


def figures(path):
    out = {}
    pat = re.compile(r"\.set\s+" + re.escape(KERNEL) + r"\.(num_vgpr|num_agpr|private_seg_size),\s*(\d+)")
    for line in open(path):
        m = pat.search(line)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def main(path):
    f = figures(path)
    if set(f) != {"num_vgpr", "num_agpr", "private_seg_size"}:
        print(f"check_syrk_budget: {path}: the resource symbols of large_syrk_bf16x3<false> were not found ({sorted(f)})")
        return 1
    bad = []
    if f["num_vgpr"] + f["num_agpr"] > MAX_VGPR:
        bad.append(f"{f['num_vgpr']} VGPR + {f['num_agpr']} AGPR > {MAX_VGPR}: fewer than three workgroups per CU")
    if f["private_seg_size"] > MAX_SCRATCH:
        bad.append(f"{f['private_seg_size']} bytes of scratch > {MAX_SCRATCH}: the compiler spills more than the loop-invariant values around the K loop")
    for b in bad:
        print(f"check_syrk_budget: large_syrk_bf16x3<false>: {b}")
    if not bad:
        print(f"check_syrk_budget: clean (large_syrk_bf16x3<false>: {f['num_vgpr']} VGPR, {f['num_agpr']} AGPR, {f['private_seg_size']} bytes of scratch)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
