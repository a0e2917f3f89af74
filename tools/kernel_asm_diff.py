#!/usr/bin/env python3
"""Which kernels differ between two device assembly files of libg2n (host-only).

  hipcc <the Makefile's CXXFLAGS> --offload-device-only -S -o X.s g2n_pipeline.hip    (once per tree)
  tools/kernel_asm_diff.py OLD.s NEW.s [--allow NAME ...] [--rename OLD=NEW ...]

Each file is split into functions (`<mangled>:` .. `.Lfunc_endN:`), a kernel's `.amdhsa_kernel`
descriptor kept apart from its body; comments are stripped and the local labels' function numbers
dropped (`.LBB12_3` -> `.LBB_3`), so that adding or removing a kernel leaves the others' text alone.
Prints the kernels that are gone, new or changed (for those, the descriptor fields that differ and the
instruction counts).  Exit status 1 for a new or changed kernel that no --allow NAME (a substring of the
mangled name) covers.  --rename OLD=NEW replaces the text OLD by NEW in OLD.s first (a renamed kernel:
part of its mangled name, which its LDS symbols carry too), so that it is compared, not gone and new.
Code-object bytes do not serve for this: entry offsets and PC-relative literals
move when a kernel is removed.
"""
import argparse
import re
import sys

LABEL = re.compile(r"\.L([A-Za-z_]*[A-Za-z])\d+")


def functions(path, renames=()):
    """{mangled name: (body lines, {descriptor field: value})}"""
    out, name, body, desc, in_desc = {}, None, [], {}, False
    for raw in open(path, errors="replace"):
        for a, b in renames:
            raw = raw.replace(a, b)
        line = LABEL.sub(r".L\1", raw.split(";", 1)[0].rstrip())
        if not line.strip():
            continue
        if name is None:
            m = re.match(r"([A-Za-z_$][\w$.]*):$", line)
            if m and not line.startswith(".L"):
                name, body, desc = m.group(1), [], {}
        elif line.startswith(".Lfunc_end"):
            out[name] = (body, desc)
            name = None
        elif line.strip().startswith(".amdhsa_kernel"):
            in_desc = True
        elif line.strip() == ".end_amdhsa_kernel":
            in_desc = False
        elif in_desc:
            k, _, v = line.strip().partition(" ")
            desc[k] = v.strip()
        elif not desc:  # (after the descriptor: only the switch back to the function's text section)
            body.append(line)
    return out


def n_instr(body):
    return sum(1 for l in body if l[:1] in "\t " and not l.strip().startswith("."))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", nargs="*", default=[], metavar="NAME")
    ap.add_argument("--rename", nargs="*", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    old, new = functions(a.old, [r.split("=", 1) for r in a.rename]), functions(a.new)
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k in old and k in new and old[k] == new[k]:
            continue
        what = "gone" if k not in new else "new" if k not in old else "changed"
        ok = what == "gone" or any(n in k for n in a.allow)
        bad += not ok
        print(f"{what}{'' if ok else ' (not allowed)'}: {k}")
        if what == "changed":
            print(f"  instructions {n_instr(old[k][0])} -> {n_instr(new[k][0])}"
                  f"{'' if old[k][0] != new[k][0] else ' (body identical)'}")
            for f in sorted(set(old[k][1]) | set(new[k][1])):
                if old[k][1].get(f) != new[k][1].get(f):
                    print(f"  {f} {old[k][1].get(f)} -> {new[k][1].get(f)}")
    same = sum(1 for k in old if k in new and old[k] == new[k])
    print(f"{same} functions identical, {len(old)} before, {len(new)} after")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
