#!/usr/bin/env python3
"""Static instruction mix of every kernel of one csrc/*.hip file, without a GPU.

usage: tools/isa_counts.py [csrc/fast_kernels.hip] [--top N] [--kernel SUBSTR] [--keep-asm FILE]
(the extractor's stages: pyramid_, fast_, blur_, desc_kernels.hip and orb_kernels.hip for the octree; default fast_kernels.hip)

The file is cross-compiled to gfx950 assembly with the flags orb-slam3-mac_amd/Makefile gives it (HIPFLAGS plus the file's own
FILEFLAGS), device code only.  Per kernel: static counts of vector (VALU, MFMA apart), scalar, LDS and memory instructions, the
resource lines of its descriptor, and the most frequent mnemonics.  Static counts say what a straight-line kernel issues per lane
and trip; loops count once.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")


def makefile_flags(src):
    """HIPFLAGS and the per-object FILEFLAGS of `src`, read from the Makefile (no $(EXTRA))."""
    text = open(os.path.join(PKG, "Makefile")).read().replace("\\\n", " ")
    var = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M))
    flags = var["HIPFLAGS"].replace("$(ARCH)", var.get("ARCH", "gfx950")).replace("$(EXTRA)", "").split()
    obj = "build/%s.o" % os.path.splitext(os.path.basename(src))[0]
    m = re.search(r"^%s:\s*FILEFLAGS\s*=\s*(.*)$" % re.escape(obj), text, re.M)
    return var.get("HIPCC", "/opt/rocm/bin/hipcc"), flags + (m.group(1).split() if m else [])


def classify(mn):
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith("v_"):
        return "vector"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_", "tbuffer_")):
        return "memory"
    if mn.startswith("s_"):
        return "scalar"
    return "other"


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def parse(asm):
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res = {}
    for name, body in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        res[name] = dict(re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size)\s+(\S+)", body))
    out, cur = collections.OrderedDict(), None
    for line in asm.split("\n"):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m:
            if m.group(1) in kernels:
                cur = out.setdefault(m.group(1), [])
            elif m.group(1).startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)(\s|$)", line)
        if m and not m.group(1).startswith("."):
            cur.append(m.group(1))
    return out, res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", nargs="?", default=os.path.join(PKG, "csrc", "fast_kernels.hip"))
    ap.add_argument("--top", type=int, default=20)
    ap.add_argument("--kernel", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--keep-asm", default="", help="also write the assembly here")
    a = ap.parse_args()
    hipcc, flags = makefile_flags(a.src)
    with tempfile.TemporaryDirectory() as td:
        s = a.keep_asm or os.path.join(td, "out.s")
        cmd = [hipcc] + [f for f in flags if f != "-fPIC"] + ["--cuda-device-only", "-S", "-o", s, a.src]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit("compile failed: %s\n%s" % (" ".join(cmd), r.stdout))
        asm = open(s).read()
    print("# %s" % os.path.relpath(a.src, ROOT))
    print("# flags: %s" % " ".join(flags))
    kern, res = parse(asm)
    names = demangle(list(kern))
    for k, ins in kern.items():
        nm = names[k]
        if a.kernel not in nm:
            continue
        cls = collections.Counter(classify(m) for m in ins)
        r = res.get(k, {})
        print("\n%s" % nm)
        print("  total %d  vector %d  mfma %d  scalar %d  lds %d  memory %d  other %d" % (
            len(ins), cls["vector"], cls["mfma"], cls["scalar"], cls["lds"], cls["memory"], cls["other"]))
        print("  vgpr %s  accum_offset %s  sgpr %s  lds %s B  scratch %s B" % (
            r.get("next_free_vgpr", "?"), r.get("accum_offset", "-"), r.get("next_free_sgpr", "?"),
            r.get("group_segment_fixed_size", "?"), r.get("private_segment_fixed_size", "?")))
        top = collections.Counter(ins).most_common(a.top)
        print("  top: " + "  ".join("%s %d" % t for t in top))


if __name__ == "__main__":
    main()
