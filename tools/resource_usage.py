#!/usr/bin/env python3
"""Register / scratch / occupancy table of every kernel in a HIP translation unit (gfx950):
    python tools/resource_usage.py em_scan_16_1 [name-filter]
    python tools/resource_usage.py ldsr_amd/csrc/kernels_serial.hip [name-filter]
Parses hipcc -Rpass-analysis=kernel-resource-usage (no GPU needed)."""
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldsr_amd", "csrc")


def unit_source(unit):
    """compiler arguments that name a translation unit: a source file, or a member of the EM kernel families
    by the name of its object -- em_scan_<L>_<W>, em_pair_<L>_<LPC> (ldsr_amd/csrc/em_members.h, Makefile)"""
    m = re.fullmatch(r"em_(scan|pair)_(\d+)_(\d+)", unit)
    if not m:
        return [unit]
    first, second = ("SCAN_L", "SCAN_W") if m.group(1) == "scan" else ("PAIR_L", "PAIR_LPC")
    return ["-D%s=%s" % (first, m.group(2)), "-D%s=%s" % (second, m.group(3)), "-x", "hip",
            os.path.join(CSRC, "em_%s_launch.inc" % m.group(1))]


def table(unit, flt=""):
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
           "-Rpass-analysis=kernel-resource-usage", "-c"] + unit_source(unit) + ["-o", "/dev/null"]
    txt = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows = []
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        mangled = b.split()[0]
        name = subprocess.run(["c++filt", mangled], capture_output=True,
                              text=True).stdout.strip()
        if flt and flt not in name:
            continue

        def g(k):
            m = re.search(re.escape(k) + r": (\d+)", b)
            return int(m.group(1)) if m else -1
        rows.append((name, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("ScratchSize [bytes/lane]"),
                     g("Occupancy [waves/SIMD]"), g("TotalSGPRs"), g("SGPRs Spill")))
    return rows


if __name__ == "__main__":
    rows = table(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
    print("%-64s %5s %5s %6s %8s %4s %5s %6s" % ("kernel", "VGPR", "AGPR", "vspill", "scratchB", "occ", "SGPR", "sspill"))
    for r in rows:
        print("%-64s %5d %5d %6d %8d %4d %5d %6d" % r)
