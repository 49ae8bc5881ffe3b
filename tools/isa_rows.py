#!/usr/bin/env python
"""Static comparison aid for the HBM-bound row kernels (gfx950, no GPU needed): compiles .hip files device-only to ISA and prints,
per kernel, VGPRs / SGPRs / LDS / scratch / occupancy, the instruction count, a hash of the opcode sequence with operands stripped
(two builds of a kernel with the same hash differ at most in register numbering and kernel-argument offsets), and per loop the
vector-memory instructions, branches and floating-point mix (instruction classes of tools/isa_count.py).

    python tools/isa_rows.py wav2lip_amd/csrc/train_rows.hip wav2lip_amd/csrc/api.hip [-k name-substring ...]
"""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_count import HIPCC, classify  # noqa: E402

MIX = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_mul_f32", "v_pk_mul_f32", "v_add_f32", "v_pk_add_f32", "v_sub_f32", "v_fma_f64",
       "v_fmac_f64", "v_add_f64", "v_mul_f64", "v_cndmask", "v_cmp")
META = (("vgpr", "NumVgprs"), ("sgpr", "TotalNumSgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"), ("occ", "Occupancy"))


def kernels(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, src], check=True,
                       stderr=subprocess.DEVNULL)
        text = open(out).read()
    for m in re.finditer(r"\n(_Z\w+):\s*; @\1\n", text):
        end = text.find(".Lfunc_end", m.end())
        meta = {k: int(re.search(r"; %s: (\d+)" % pat, text[end:end + 6000]).group(1)) for k, pat in META}
        # binutils' c++filt does not know DF16b (__bf16) yet: hand it the same type as a vendor-extended name
        name = subprocess.run(["c++filt", m.group(1).replace("DF16b", "u6__bf16")], capture_output=True, text=True).stdout.strip()
        yield name.split("(")[0].replace("void ", "").replace("w2l::", ""), text[m.end():end], meta


def walk(body):
    """(opcodes of the kernel, [(loop header label, class counts, floating-point mix)])"""
    ops, loops, cur = [], [], None
    for line in body.split("\n"):
        s = line.strip()
        lm = re.match(r"(\.LBB\d+_\d+):\s*(;.*)?", s)
        if lm:
            c = lm.group(2) or ""
            if "Loop Header" in c:
                cur = (lm.group(1), collections.Counter(), collections.Counter())
                loops.append(cur)
            elif "in Loop" not in c and "Parent Loop" not in c:
                cur = None
            continue
        s = s.split(";")[0].strip()
        if not s or s.startswith((".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        ops.append(op)
        if cur is None:
            continue
        cur[1][classify(op)] += 1
        if op.startswith("s_cbranch") or op == "s_branch":
            cur[1]["branch"] += 1
        for p in MIX:
            if op.startswith(p):
                cur[2][p[2:]] += 1
    return ops, loops


def main():
    args = sys.argv[1:]
    want = []
    while "-k" in args:
        i = args.index("-k")
        want.append(args[i + 1])
        del args[i:i + 2]
    for src in args:
        print("#### %s" % os.path.relpath(src))
        for name, body, meta in kernels(src):
            if "kernel" not in name or (want and not any(w in name for w in want)):
                continue
            ops, loops = walk(body)
            print("%-44s vgpr %3d sgpr %3d lds %5d scratch %d occ %d  %4d instructions, opcode sequence %s" % (
                name, meta["vgpr"], meta["sgpr"], meta["lds"], meta["scratch"], meta["occ"], len(ops),
                hashlib.sha256(" ".join(ops).encode()).hexdigest()[:10]))
            for lab, c, mix in loops:
                print("      loop %-10s vmem %2d branch %2d valu %3d salu %3d lds rd/wr %d/%d | %s" % (
                    lab, c["vmem"], c["branch"], c["valu"], c["salu"], c["lds_rd"], c["lds_wr"],
                    " ".join("%s %d" % kv for kv in sorted(mix.items()))))


if __name__ == "__main__":
    main()
