#!/usr/bin/env python3
"""Barriers, lane spills and scratch instructions of rdf_cell_pair_kernel instantiations, in the whole kernel and
inside the basic blocks that hold a hot step (a ds_add_u32), from the ISA of one build (no GPU needed):

    scripts/isa_hot_blocks.py [label]

compiles mdhelper_amd/csrc/mdx_rdf.hip with the Makefile's flags and --save-temps in a scratch directory and prints
one line per instantiation.  For another tree (the parent's), run its own copy of this script or pass its csrc
directory as the second argument."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
label = sys.argv[1] if len(sys.argv) > 1 else "this tree"
csrc = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "mdhelper_amd", "csrc")
include = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
KERNELS = ("ILb1ELb0ELi0ELb0ELb1E", "ILb0ELb0ELi0ELb0ELb1E", "ILb1ELb1ELi0ELb0ELb1E", "ILb1ELb0ELi0ELb0ELb0E")
SCRATCH = ("scratch_", "buffer_load_dword", "buffer_store_dword")

with tempfile.TemporaryDirectory() as tmp:
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-fno-slp-vectorize", "--save-temps", "-I" + include, "-c", os.path.join(csrc, "mdx_rdf.hip"),
                    "-o", "out.o"], cwd=tmp, check=True, capture_output=True)
    text = open(os.path.join(tmp, "mdx_rdf-hip-amdgcn-amd-amdhsa-gfx950.s")).read()

for k in KERNELS:
    name = "_Z20rdf_cell_pair_kernel" + k + "Ev8CellArgs"
    i = text.index(name + ":")
    body = text[i:text.index(".Lfunc_end", i)].split("\n")
    blocks, cur = [], []
    for line in body:
        if re.match(r"^\.LBB\d+_\d+:", line):
            blocks.append(cur)
            cur = []
        elif line.startswith("\t") and not line.strip().startswith((".", ";")):
            cur.append(line.strip())
    blocks.append(cur)
    ins = [x for b in blocks for x in b]
    hot = [b for b in blocks if any(x.startswith("ds_add_u32") for x in b)]
    hi = [x for b in hot for x in b]

    def count(seq, prefix):
        return sum(1 for x in seq if x.startswith(prefix))

    print(f"{label} {k}: {len(ins)} instr, s_barrier {count(ins, 's_barrier')}, v_readlane {count(ins, 'v_readlane')}, "
          f"v_writelane {count(ins, 'v_writelane')}, scratch {count(ins, SCRATCH)}, ds_add_rtn {count(ins, 'ds_add_rtn')}, "
          f"ds_wrxchg_rtn {count(ins, 'ds_wrxchg')} | hot blocks {len(hot)}: {len(hi)} instr, "
          f"v_readlane {count(hi, 'v_readlane')}, v_writelane {count(hi, 'v_writelane')}, scratch {count(hi, SCRATCH)}")
