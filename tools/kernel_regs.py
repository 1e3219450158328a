#!/usr/bin/env python3
"""VGPRs / scratch / LDS per kernel of tm_kernels.hip (hipcc resource-usage
remarks): the main walks, k_walk_fast and k_walk_pairs (one wave per block),
must stay within 64 VGPRs, no scratch and 5,120 B of LDS per block (8 waves
per SIMD).
usage: kernel_regs.py [-Dextra ...]"""
import re
import subprocess
import sys
from pathlib import Path

MAIN_WALKS = ("k_walk_fast", "k_walk_pairs")
VGPR_MAX, LDS_MAX = 64, 5120

src = Path(sys.argv.pop(1)) if len(sys.argv) > 1 and sys.argv[1].endswith(".hip") else Path(__file__).resolve().parent.parent / "emqx_amd" / "csrc" / "tm_kernels.hip"
r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", "-o", "/dev/null", str(src),
                    "-Rpass-analysis=kernel-resource-usage"] + sys.argv[1:], capture_output=True, text=True)
name, rows = None, {}
for line in r.stderr.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        name = re.sub(r"^_ZN3tmx\d+", "", m.group(1)).split("EEEv")[0].split("ENS_")[0]
    m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
    if m and name:
        rows.setdefault(name, {})[m.group(1).split()[0]] = int(m.group(2))
for k, v in rows.items():
    print(f"{k:32s} VGPRs {v.get('VGPRs')}  scratch {v.get('ScratchSize')}  LDS {v.get('LDS')}  "
          f"occupancy {v.get('Occupancy')}")
ok = r.returncode == 0
for walk in MAIN_WALKS:
    w = [v for k, v in rows.items() if k.startswith(walk)]
    good = bool(w) and all(v.get("VGPRs", 99) <= VGPR_MAX and v.get("ScratchSize", 1) == 0 and
                           v.get("LDS", LDS_MAX + 1) <= LDS_MAX for v in w)
    if not good:
        print(f"FAIL {walk}: over {VGPR_MAX} VGPRs, scratch, over {LDS_MAX} B LDS, or not found", file=sys.stderr)
    ok = ok and good
sys.exit(0 if ok else 1)
