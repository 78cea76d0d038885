#!/usr/bin/env python3
"""Compare every gfx950 kernel of two builds of libmi355fa.so: instructions (llvm-objdump, addresses and encodings
stripped) and register / LDS / scratch counts from the code-object metadata.

usage: isa_diff.py [--scalar-ok] [--renames MAP.json] OLD.so [NEW.so]      (NEW defaults to the in-tree library)
Prints one line per kernel that changed, then the kernels only one side has; exits 1 if a kernel present in both differs.

--scalar-ok: a kernel present in both builds that differs is held to the bar of a renamed pair (below) instead of to
identity, and printed as SCALAR with the pair's summary if it meets it; it then does not count as changed.

--renames: for a change that renames kernels.  MAP.json is {old stem: [new stem, [flag, ...]]}: the old kernel
stem<args...> is compared with the new kernel stem<args..., flags...> (flags are booleans).  Kernel arguments may move with
such a change, so a renamed pair is held to this instead of to identity: the same VGPR, AGPR, LDS, scratch and spill
counts; the same sequence of non-scalar instructions (every line that does not start with "s_", with operands; a pair
that matches only once SGPR numbers are blanked is marked "sgpr-renumbered"); at most MAX_SCALAR_DELTA instructions more
or fewer.  One line per pair, with the scalar lines that differ counted by mnemonic; exits 1 if a pair misses the bar or
an old stem of the map has no partner.
"""
import collections
import difflib
import json
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


MAX_SCALAR_DELTA = 8


def renamed(name, renames):
    """The mangled name of the kernel that replaces `name` under the rename map, or None."""
    m = re.match(r"_ZN2fa\d+(\w+?_kernel)I(.+?E)EEv", name)
    if not m or m.group(1) not in renames:
        return None
    stem, flags = renames[m.group(1)]
    return "_ZN2fa%d%sI%s%sEEv" % (len(stem), stem, m.group(2), "".join("Lb%dE" % bool(f) for f in flags))


def compare_renamed(a, b, ca, cb):
    """(ok, text) for an old kernel (instructions a, counts ca) and the kernel that replaces it."""
    regs = all(ca[x] == cb[x] for x in ("vgpr", "agpr", "lds", "scratch", "spill"))
    va, vb = ([l for l in x if not l.startswith("s_")] for x in (a, b))
    blank = lambda ls: [re.sub(r"\bs(\d+|\[\d+:\d+\])", "s#", l) for l in ls]  # noqa: E731
    vector = "same" if va == vb else "sgpr-renumbered" if blank(va) == blank(vb) else "DIFFERS"
    sa, sb = ([l for l in x if l.startswith("s_")] for x in (a, b))
    diff = collections.Counter()
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, sa, sb, autojunk=False).get_opcodes():
        if tag != "equal":
            diff.update(l.split()[0] for l in sa[i1:i2] + sb[j1:j2])
    ok = regs and vector != "DIFFERS" and abs(len(a) - len(b)) <= MAX_SCALAR_DELTA
    return ok, "insns %d->%d vector=%s regs=%s sgpr %d->%d scalar lines differing: %s" % (
        len(a), len(b), vector, "same" if regs else "%s->%s" % (ca, cb), ca["sgpr"], cb["sgpr"],
        " ".join("%s:%d" % kv for kv in sorted(diff.items())) or "none")


def main():
    argv = sys.argv[1:]
    scalar_ok = bool(argv) and argv[0] == "--scalar-ok"
    argv = argv[scalar_ok:]
    renames = {}
    if argv and argv[0] == "--renames":
        renames = json.load(open(argv[1]))
        argv = argv[2:]
    old = argv[0]
    new = argv[1] if len(argv) > 1 else codeobj.DEFAULT_LIB
    d_old, d_new = disasm(old), disasm(new)
    c_old, c_new = counts(old), counts(new)
    common = sorted(set(c_old) & set(c_new))
    changed = scalar = 0
    pairs = {}
    for name in sorted(set(c_old) - set(c_new)):
        to = renamed(name, renames)
        if to:
            to = [n for n in c_new if n.startswith(to)]
            pairs[name] = to[0] if len(to) == 1 else None
    for name, to in pairs.items():
        ok, text = compare_renamed(d_old[name], d_new[to], c_old[name], c_new[to]) if to else (False, "no such kernel")
        changed += not ok
        print("%s %s -> %s\n    %s" % ("RENAMED" if ok else "MISMATCH", name, codeobj.demangle_short(to) if to else "?", text))
    if renames:
        print("%d renamed kernels" % len(pairs))
        c_old = {k: v for k, v in c_old.items() if k not in pairs}
        c_new = {k: v for k, v in c_new.items() if k not in pairs.values()}
    for name in common:
        same_isa = d_old.get(name) == d_new.get(name)
        same_regs = c_old[name] == c_new[name]
        if not (same_isa and same_regs):
            if scalar_ok:
                ok, text = compare_renamed(d_old[name], d_new[name], c_old[name], c_new[name])
                if ok:
                    scalar += 1
                    print("SCALAR  %s\n    %s" % (codeobj.demangle_short(name), text))
                    continue
            changed += 1
            print("CHANGED %s isa=%s regs=%s->%s" % (codeobj.demangle_short(name), "same" if same_isa else "differs",
                                                      c_old[name], c_new[name]))
    print("%d kernels in both builds, %d changed%s" % (len(common), changed, ", %d scalar-only" % scalar if scalar_ok else ""))
    for name in sorted(set(c_new) - set(c_old)):
        print("new     %-44s %s" % (codeobj.demangle_short(name), c_new[name]))
    for name in sorted(set(c_old) - set(c_new)):
        print("removed %s" % codeobj.demangle_short(name))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
