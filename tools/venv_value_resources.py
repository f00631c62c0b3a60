#!/usr/bin/env python3
"""Registers, LDS and scratch of every instantiation of the record-reading
value kernels (net_value_kernels.hip), from a cross-compile with
-Rpass-analysis=kernel-resource-usage: one JSON line per kernel to
profiles/venv_value_resources.jsonl.  Needs hipcc, no GPU.

  python tools/venv_value_resources.py [--out profiles/venv_value_resources.jsonl]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dependence_free_rl_amd", "csrc")
FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "SGPRs": "sgprs",
          "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
          "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
          "LDS Size [bytes/block]": "lds_bytes"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "venv_value_resources.jsonl"))
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [args.hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
               "-I" + os.path.join(ROOT, "include"), "-I" + SRC,
               "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(SRC, "net_value_kernels.hip"),
               "-o", os.path.join(tmp, "net_value_kernels.o")]
        res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode:
        sys.exit(res.stderr)
    rows, cur = [], None
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            k = re.search(r"net_value_(fwd|bwd)_kernelILi(\d+)ELi(\d+)E", val)
            cur = None
            if k:
                B, D = int(k.group(2)), int(k.group(3))
                cur = {"kernel": "net_value_%s_kernel" % k.group(1), "bins": B,
                       "dims": D, "fin": 2 * B * D}
                rows.append(cur)
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    rows.sort(key=lambda r: (r["kernel"], r["dims"], r["bins"]))
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    for r in rows:
        print("%-21s %3d bins %d-D: vgpr %3d agpr %3d lds %5d scratch %d occ %d"
              % (r["kernel"], r["bins"], r["dims"], r["vgprs"], r["agprs"],
                 r["lds_bytes"], r["scratch_bytes_per_lane"],
                 r["occupancy_waves_per_simd"]))
    print("%d kernels -> %s" % (len(rows), args.out))


if __name__ == "__main__":
    main()
