"""Compare the gfx950 function bodies of two builds of one translation unit.

    python tools/asm_compare.py OLD.s NEW.s [--list]

The inputs are `hipcc ... --cuda-device-only -S` outputs of the same unit from two trees (the Makefile's
flags).  A function body runs from its label to its .Lfunc_end; block labels are renumbered in order of
appearance and comments dropped, so that only the instructions and their operands are compared.  Prints
how many of OLD's functions are identical, differ, or are missing in NEW, and what only NEW has.
"""
import re
import sys


def bodies(path):
    out, name, cur = {}, None, []
    for ln in open(path, errors="replace"):
        ln = ln.split(";")[0].rstrip()
        if not ln.strip():
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*$", ln)
        if name is None:
            if m and not m.group(1).startswith(".L"):
                name, cur = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            out[name] = cur
            name = None
            continue
        if ln.lstrip().startswith((".p2align", ".loc", ".file", ".cfi", ".type", ".size", ".globl", ".section")):
            continue
        cur.append(ln.strip())
    return out


def normal(body):
    names = {}

    def sub(m):
        return names.setdefault(m.group(0), f".L{len(names)}")

    return [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", sub, ln) for ln in body]


def main():
    old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
    same = [n for n in old if n in new and normal(old[n]) == normal(new[n])]
    differ = sorted(n for n in old if n in new and n not in set(same))
    gone = sorted(n for n in old if n not in new)
    added = sorted(n for n in new if n not in old)
    print(f"{len(old)} of the parent's functions, {len(same)} identical, {len(differ)} differ, "
          f"{len(gone)} only in the parent's build; {len(added)} only in this build")
    if "--list" in sys.argv:
        for tag, names in (("differ", differ), ("only parent", gone), ("only this", added)):
            for n in names:
                print(f"   {tag}: {n}")


if __name__ == "__main__":
    main()
