#!/usr/bin/env python
"""Registers, spills, scratch, occupancy and LDS of every kernel of the library as the compiler reports them
(-Rpass-analysis=kernel-resource-usage), and the memory instructions of its code by address space -- flat_* (generic pointers: the
address space is decided per lane at run time, the access counts against both memory counters), ds_read* / ds_write* (LDS), other ds_*
(LDS atomics and the like), global_* --: python scripts/resource_usage.py > profiles/rNN_resource_usage.txt"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc", "k4lz4_capi.hip")
with tempfile.TemporaryDirectory() as d:
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        *sys.argv[1:], "-S", SRC, "-o", os.path.join(d, "o.s")], capture_output=True, text=True)
    asm = open(os.path.join(d, "o.s")).read() if r.returncode == 0 else ""
if r.returncode != 0:
    sys.exit(r.stderr)

def short(name):
    n = re.sub(r"^_ZN2k4\d+", "", name)
    return re.sub(r"E(NS_|P|j|i|x).*$", "", n)

# the code of one function: from its label to its .Lfunc_end
mix = {}
for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
    c = {"flat": 0, "ds_rw": 0, "ds_other": 0, "global": 0}
    for line in m.group(2).splitlines():
        op = line.split(None, 1)[0] if line.strip() else ""
        if op.startswith("flat_"): c["flat"] += 1
        elif op.startswith("ds_read") or op.startswith("ds_write"): c["ds_rw"] += 1
        elif op.startswith("ds_") and not op.startswith(("ds_bpermute", "ds_permute", "ds_swizzle")): c["ds_other"] += 1
        elif op.startswith("global_"): c["global"] += 1
    mix[m.group(1)] = c

t = r.stderr
for m in re.finditer(r"Function Name: (\S+).*?SGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", t, re.S):
    c = mix.get(m.group(1), None)
    ops = f" | flat {c['flat']:>3} ds_read/write {c['ds_rw']:>3} ds_other {c['ds_other']:>3} global {c['global']:>3}" if c else ""
    print(f"{short(m.group(1)):36s} VGPR {m.group(3):>3} AGPR {m.group(4):>3} SGPR {m.group(2):>3} sspill {m.group(7):>3} vspill {m.group(8):>2} scratch {m.group(5):>3} occ {m.group(6)} lds {m.group(9)}{ops}")
