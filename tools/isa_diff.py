#!/usr/bin/env python3
"""Compare every gfx950 kernel of two builds of libmi355fa.so: instructions (llvm-objdump, addresses and encodings
stripped) and register / LDS / scratch counts from the code-object metadata.

usage: isa_diff.py OLD.so [NEW.so]      (NEW defaults to the in-tree library)
Prints one line per kernel that changed, then the kernels only one side has; exits 1 if a kernel present in both differs.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def disasm(lib):
    """{kernel symbol: [instruction text]} over every gfx950 code object of the library."""
    out = {}
    for co in codeobj.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", "--mcpu=gfx950", f.name],
                                  capture_output=True, text=True, check=True).stdout
        for part in re.split(r"\n(?=<)", text):
            m = re.match(r"<([^>]+)>:", part)
            if not m:
                continue
            # trailing comments (branch target addresses) are dropped
            lines = [re.sub(r"//.*", "", l).strip() for l in part.splitlines()[1:]]
            out[m.group(1)] = [l for l in lines if l and l != "..."]  # "...": padding to the next symbol
    return out


def counts(lib):
    return {k["name"]: {x: k[x] for x in ("vgpr", "agpr", "sgpr", "spill", "scratch", "lds")} for k in codeobj.kernels(lib)}


def main():
    old = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else codeobj.DEFAULT_LIB
    d_old, d_new = disasm(old), disasm(new)
    c_old, c_new = counts(old), counts(new)
    common = sorted(set(c_old) & set(c_new))
    changed = 0
    for name in common:
        same_isa = d_old.get(name) == d_new.get(name)
        same_regs = c_old[name] == c_new[name]
        if not (same_isa and same_regs):
            changed += 1
            print("CHANGED %s isa=%s regs=%s->%s" % (codeobj.demangle_short(name), "same" if same_isa else "differs",
                                                      c_old[name], c_new[name]))
    print("%d kernels in both builds, %d changed" % (len(common), changed))
    for name in sorted(set(c_new) - set(c_old)):
        print("new     %-44s %s" % (codeobj.demangle_short(name), c_new[name]))
    for name in sorted(set(c_old) - set(c_new)):
        print("removed %s" % codeobj.demangle_short(name))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
