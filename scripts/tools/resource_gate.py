#!/usr/bin/env python3
"""usage: scripts/tools/resource_gate.py [--out FILE]      (compile only: needs hipcc, no GPU)

Compiles blutils_amd/csrc/consensus_kernel.hip for gfx950 with -Rpass-analysis=kernel-resource-usage (the flags of the
Makefile) and holds every blu_consensus_stream_kernel instantiation to what its launch bounds promise:

  * LDS per block <= 163 840 B (160 KiB per CU: one persistent block per CU),
  * occupancy [waves per SIMD] equal to the second __launch_bounds__ argument of that build (3 with the ring and in the
    f64 layouts, 4 in the milli-percent builds without the ring),
  * no scratch in the builds with the ring.

A list capacity (LIST_CAP*) raised by hand cannot cost a wave per SIMD or spill without this failing.  Prints one line per
kernel; exit status 1 if a build misses.  --out writes the same lines to a file (profiles/*_resource_usage.txt)."""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "blutils_amd", "csrc")
LDS_PER_CU = 160 * 1024
ARCH = "gfx950"
# the Makefile's CXXFLAGS (warnings aside)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
         "--offload-arch=" + ARCH, "-x", "hip", "-c", "consensus_kernel.hip", "-o", os.devnull,
         "-Rpass-analysis=kernel-resource-usage"]
STREAM = re.compile(r"blu_consensus_stream_kernelILi(\d)ELi(\d)ELb(\d)E")
LAYOUT_NAMES = {0: "f64 columns", 1: "milli columns", 2: "packed", 3: "packed64"}


def find_hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def expected_occupancy(layout: int, ring: bool) -> int:
    """The second __launch_bounds__ argument of blu_consensus_stream_kernel<STRAT, LAYOUT, RING>."""
    return 3 if (ring or layout in (0, 3)) else 4


def resource_usage(hipcc: str):
    """[{name, VGPRs, ScratchSize [bytes/lane], LDS Size [bytes/block], Occupancy [waves/SIMD], ...}] per kernel."""
    p = subprocess.run([hipcc] + FLAGS, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + p.stdout[-4000:])
    rows, cur = [], None
    for line in p.stdout.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = {"name": text.split(":", 1)[1].strip()}
            rows.append(cur)
        elif ":" in text and cur is not None:
            k, v = text.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


def check(rows):
    """(lines, failures) for the stream kernel's instantiations."""
    lines, failures = [], []
    for r in rows:
        m = STREAM.search(r["name"])
        if not m:
            continue
        strat, layout, ring = int(m.group(1)), int(m.group(2)), m.group(3) == "1"
        lds, occ = int(r["LDS Size [bytes/block]"]), int(r["Occupancy [waves/SIMD]"])
        scratch, vgpr = int(r["ScratchSize [bytes/lane]"]), int(r["VGPRs"])
        label = "stream<%s, %s, %s>" % ("relaxed" if strat == 1 else "cautious", LAYOUT_NAMES[layout], "ring" if ring else "no ring")
        lines.append("%-44s LDS %6d B  VGPRs %3d  scratch %3d B/lane  waves/SIMD %d" % (label, lds, vgpr, scratch, occ))
        if lds > LDS_PER_CU:
            failures.append("%s: %d B of LDS per block > %d" % (label, lds, LDS_PER_CU))
        if occ != expected_occupancy(layout, ring):
            failures.append("%s: %d waves per SIMD, its launch bounds say %d" % (label, occ, expected_occupancy(layout, ring)))
        if ring and scratch != 0:
            failures.append("%s: %d B/lane of scratch in a ring build" % (label, scratch))
    return lines, failures


def main(argv):
    hipcc = find_hipcc()
    if hipcc is None:
        print("resource_gate: no hipcc", file=sys.stderr)
        return 2
    lines, failures = check(resource_usage(hipcc))
    if len(lines) != 16:
        failures.append("expected 16 instantiations of blu_consensus_stream_kernel, found %d" % len(lines))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write(text)
    for f in failures:
        print("FAIL " + f, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
