#!/usr/bin/env python3
"""Body-by-body comparison of the gfx950 kernels of two built objects, for refactors that must not change what is emitted:
tools/compare_code_objects.py PARENT.o HEAD.o [substring]. Prints the number of kernels on each side, whether the name sets
are equal, and the demangled names whose disassembled bodies differ (tools/kernel_meta.py then shows their resources).
Exit status 1 if the name sets differ. Touches no GPU."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def bodies(obj):
    """mangled kernel name -> hash of its disassembled body (no addresses, no encodings)"""
    tmp = tempfile.mkdtemp(prefix="kcmp_")
    try:
        local = os.path.join(tmp, "unit.o")
        shutil.copy(obj, local)
        run(os.path.join(LLVM, "llvm-objdump"), "--offloading", local)
        co = os.path.join(tmp, [f for f in os.listdir(tmp) if "gfx950" in f][0])
        asm = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
        kernels = set(re.findall(r"\.name:\s+(\S+)", run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    asm = re.sub(r"//\s*[0-9A-Fa-f]+:(\s[0-9A-Fa-f]{8})+", "//", asm)  # branch lines keep address + encoding in a comment
    parts = re.split(r"^<([^>]+)>:\n", asm, flags=re.M)
    return {name: hashlib.sha256(body.encode()).hexdigest() for name, body in zip(parts[1::2], parts[2::2]) if name in kernels}


def main():
    needle = sys.argv[3] if len(sys.argv) > 3 else ""
    a, b = ({k: h for k, h in bodies(p).items() if needle in k} for p in sys.argv[1:3])
    differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
    print(f"kernels: {len(a)} / {len(b)}; names {'equal' if a.keys() == b.keys() else 'DIFFER'}; "
          f"bodies identical {len(a.keys() & b.keys()) - len(differ)}, differ {len(differ)}")
    for k in sorted(a.keys() ^ b.keys()):
        print(("only in first:  " if k in a else "only in second: ") + k)
    if differ:
        for d in run("c++filt", *differ).splitlines():
            print("differs: " + re.sub(r"\(.*$", "", re.sub(r"^void ", "", d)))
    return 0 if a.keys() == b.keys() else 1


if __name__ == "__main__":
    sys.exit(main())
