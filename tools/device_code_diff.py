#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libgfship's objects, byte for byte.

    tools/device_code_diff.py [--rename OLD=NEW]... OBJDIR_A OBJDIR_B

For every *.o of OBJDIR_A: the .hip_fatbin section is taken out of both objects, the gfx950 code
object unbundled, and its .text and .rodata compared.  Where a section differs (a changed order of
template instantiations permutes .text) the kernels and functions are compared one by one instead:
names, sizes and bytes of every defined symbol of the section; of a kernel descriptor (NAME.kd in
.rodata) all but bytes 16-23, the offset from the descriptor to the kernel's code, which moves with
the kernel.  --rename OLD=NEW (mangled names, repeatable) compares the kernel OLD of OBJDIR_A with the kernel
NEW of OBJDIR_B, for a kernel whose name changed with the type of an argument.  Prints one line per file; exit
status 1 if any file differs."""
import glob
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    try:
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj)
    except subprocess.CalledProcessError:       # a file without kernels
        return None
    run(os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--unbundle",
        "--input=" + fat, "--output=" + co)
    return co


def section(co, name, tmp, tag):
    out = os.path.join(tmp, tag + name)
    open(out, "wb").close()
    try:
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", "%s=%s" % (name, out), co)
    except subprocess.CalledProcessError:       # a code object without kernels has no such section
        return b""
    with open(out, "rb") as f:
        return f.read()


RENAME = {}


def symbols(co, sec, data):
    """{name: bytes} of the defined symbols of section `sec' (llvm-readobj --symbols)"""
    out, cur = {}, {}
    base = None
    for line in run(os.path.join(LLVM, "llvm-readobj"), "--sections", "--symbols", co).splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] in ("Section", "Symbol") and w[-1] == "{":
            cur = {"kind": w[0]}
        elif w[0].rstrip(":") in ("Name", "Address", "Value", "Size", "Section"):
            cur[w[0].rstrip(":")] = w[1]
        elif w[0] == "}":
            if cur.get("kind") == "Section" and cur.get("Name") == sec:
                base = int(cur["Address"], 16)
            elif cur.get("kind") == "Symbol" and cur.get("Section") == sec and int(cur["Size"]):
                out[cur["Name"]] = (int(cur["Value"], 16), int(cur["Size"]))
            cur = {}
    code = {n: data[a - base:a - base + s] for n, (a, s) in out.items()}
    code = {n: c[:16] + c[24:] if n.endswith(".kd") else c for n, c in code.items()}
    return {RENAME.get(n[:-3], n[:-3]) + ".kd" if n.endswith(".kd") else RENAME.get(n, n): c for n, c in code.items()}


def main(a, b):
    bad = 0
    for oa in sorted(glob.glob(os.path.join(a, "*.o"))):
        name = os.path.basename(oa)
        with tempfile.TemporaryDirectory() as tmp:
            ca, cb = code_object(oa, tmp, "a"), code_object(os.path.join(b, name), tmp, "b")
            verdict = []
            if ca is None or cb is None:
                print("%-24s %s" % (name, "no device code" if ca is cb else "DIFFERS: device code in one build only"))
                bad |= ca is not cb
                continue
            for sec in (".text", ".rodata"):
                da, db = section(ca, sec, tmp, "a"), section(cb, sec, tmp, "b")
                if da == db:
                    verdict.append("%s identical (%d bytes)" % (sec, len(da)))
                elif len(da) == len(db) and symbols(ca, sec, da) == symbols(cb, sec, db):
                    verdict.append("%s permuted, every symbol identical (%d symbols)" % (sec, len(symbols(ca, sec, da))))
                else:
                    sa, sb = symbols(ca, sec, da), symbols(cb, sec, db)
                    diff = sorted(n for n in set(sa) | set(sb) if sa.get(n) != sb.get(n))
                    verdict.append("%s DIFFERS (%d symbols: %s)" % (sec, len(diff), ", ".join(diff[:4])))
                    bad = 1
            print("%-24s %s" % (name, "; ".join(verdict)))
    return bad


if __name__ == "__main__":
    args = sys.argv[1:]
    while len(args) > 1 and args[0] == "--rename":
        old, new = args[1].split("=")
        RENAME[old] = new
        args = args[2:]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1]))
