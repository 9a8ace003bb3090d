#!/usr/bin/env python3
"""Compare two compilations of aslam_core.hip kernel by kernel: the set of kernel names, every kernel's row of
-Rpass-analysis=kernel-resource-usage, and the per-kernel device assembly of -save-temps.

    hipcc $(HIPFLAGS) -DASLAM_HAVE_UKF=1 -save-temps -Rpass-analysis=kernel-resource-usage -c -o aslam_core.o aslam_core.hip 2> remarks.txt

in a directory per tree, then

    tools/compare_kernel_builds.py PARENT_DIR THIS_DIR [--family REGEX] [--table]

Exit status 0 when names, resources and bodies are all equal.  Assembly bodies are compared without comments and with the function
index taken out of local labels (.LBB12_3 -> .LBB_3), which changes when the order of the kernels in the module does.
"""
import argparse
import glob
import os
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
SHORT = ["SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "SGPR spill", "VGPR spill", "static LDS"]


def resources(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(?:\S+:\s+)?([A-Za-z][^:]*): (\S.*) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return out


def bodies(path):
    out, name, buf = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):\s", line)
        if name is None and m:
            name, buf = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = "".join(buf)
                name = None
                continue
            line = line.split(";")[0].rstrip()
            if line:
                buf.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", line)) + "\n")
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except Exception:
        return {n: n for n in names}


def short(dem):
    return re.sub(r"\(.*", "", dem).replace("aslam::", "").replace("void ", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--family", default="ekf_small_kernel|ukf_small_kernel|frontend_kernel", help="the kernels the table lists")
    ap.add_argument("--table", action="store_true", help="print the markdown table of the family")
    a = ap.parse_args()
    res, asm = [], []
    for d in (a.parent, a.this):
        res.append(resources(os.path.join(d, "remarks.txt")))
        asm.append(bodies(glob.glob(os.path.join(d, "aslam_core-hip-amdgcn-*.s"))[0]))
    names = [sorted(r) for r in res]
    fam = re.compile(a.family)
    dem = demangle(sorted(set(names[0]) | set(names[1])))
    ok = names[0] == names[1]
    print(f"kernels: parent {len(names[0])}, this {len(names[1])}, names {'identical' if ok else 'DIFFER'}; "
          f"family /{a.family}/: {sum(bool(fam.search(n)) for n in names[0])} / {sum(bool(fam.search(n)) for n in names[1])}")
    for n in sorted(set(names[0]) ^ set(names[1])):
        print("  only in", "parent" if n in res[0] else "this", dem[n])
    common = [n for n in names[0] if n in res[1]]
    rdiff = [n for n in common if any(res[0][n].get(f) != res[1][n].get(f) for f in FIELDS)]
    bdiff = [n for n in common if asm[0].get(n) != asm[1].get(n)]
    print(f"resource rows that differ: {len(rdiff)}")
    for n in rdiff:
        print("  ", short(dem[n]), [(s, res[0][n].get(f), res[1][n].get(f)) for f, s in zip(FIELDS, SHORT) if res[0][n].get(f) != res[1][n].get(f)])
    print(f"assembly bodies that differ: {len(bdiff)} (of {len(common)}; {sum(n not in asm[0] for n in common)} not found)")
    for n in bdiff:
        print("  ", short(dem[n]))
    if a.table:
        print("\n| kernel | " + " | ".join(SHORT) + " | row | body |\n|---|" + "---|" * (len(SHORT) + 2))
        for n in sorted((n for n in common if fam.search(n)), key=lambda n: short(dem[n])):
            print(f"| `{short(dem[n])}` | " + " | ".join(res[1][n].get(f, "?") for f in FIELDS) +
                  f" | {'changed' if n in rdiff else 'equal'} | {'differs' if n in bdiff else 'equal'} |")
    return 0 if ok and not rdiff and not bdiff else 1


if __name__ == "__main__":
    sys.exit(main())
