#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 disassembly of two builds of libirlosc.so (a refactor's evidence: text only).

    python tools/kernel_diff.py <parent libirlosc.so> <branch libirlosc.so> [--dump DIR]

Cuts the code objects out of both libraries (kernel_regs.code_objects), disassembles them with llvm-objdump and compares the
instruction text AND encodings of every function symbol; the addresses in the listing's comments are dropped (a kernel
may move inside its code object).  Prints the kernel counts, the names on one side only and the names whose text differs;
--dump writes the listings of the differing ones as DIR/<side>/<mangled name>.s.  Exit status 1 if anything differs."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_regs import code_objects  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(lib):
    """mangled name -> [instruction lines] over every code object of the library (.kd descriptors are data, not listed)"""
    out = {}
    with open(lib, "rb") as f:
        blob = f.read()
    for off, size in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as t:
            t.write(blob[off:off + size])
            t.flush()
            txt = subprocess.run([OBJDUMP, "-d", t.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for ln in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
            if m:
                cur = out.setdefault(m.group(1), [])
            elif cur is not None and ln.strip():
                cur.append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", ln).strip())
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--dump"]
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
    if dump:
        args.remove(dump)
    a, b = kernels(args[0]), kernels(args[1])
    print(f"functions: {len(a)} / {len(b)}")
    only = sorted(set(a) ^ set(b))
    for n in only:
        print(("only in parent: " if n in a else "only in branch: ") + n)
    differ = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    for n in differ:
        print(f"differs ({len(a[n])} / {len(b[n])} instructions): {n}")
        if dump:
            for side, k in (("parent", a), ("branch", b)):
                os.makedirs(os.path.join(dump, side), exist_ok=True)
                with open(os.path.join(dump, side, n[:200] + ".s"), "w") as f:
                    f.write("\n".join(k[n]) + "\n")
    print(f"identical: {len(set(a) & set(b)) - len(differ)}, differing: {len(differ)}, on one side only: {len(only)}")
    return 1 if (only or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
