"""Are the kernels of two builds the same machine code?

    python tools/isa_same.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...]

Each side is one or more device-only listings (hipcc ... --cuda-device-only -S,
the product flags otherwise); kernels may have moved between files. Per kernel
symbol the text from its label to its end label is compared: comments dropped,
the compiler's local labels (.LBB.., .Ltmp.., .Lfunc_end..) renumbered by first
appearance, which leaves the instruction sequence and the .amdhsa_ resource
block. Prints a count per file, every symbol that differs, is gone or is new,
and a one-line verdict; exits 1 unless both sides hold the same symbols and
every kernel is identical.
"""
import argparse
import re
import sys

LOCAL = re.compile(r"\.L(?:BB|tmp|func_end|JTI)[0-9_]+")


def kernels(path):
    """{kernel symbol: normalised text} of one listing."""
    lines = open(path).read().split("\n")
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, name, body, seen = {}, None, [], {}
    for l in lines:
        if name is None:
            m = re.match(r"(\S+):", l)
            if m and m.group(1) in names:
                name, body, seen = m.group(1), [], {}
            continue
        l = l.split(";", 1)[0].strip()
        if not l:
            continue
        end = l.startswith(".Lfunc_end")
        body.append(LOCAL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), l))
        if end:
            out[name] = "\n".join(body)
            name = None
    return out


def side(paths):
    all_k = {}
    for p in paths:
        k = kernels(p)
        print(f"  {p}: {len(k)} kernels")
        for s in k:
            if s in all_k:
                sys.exit(f"{s} is in two listings of one side")
        all_k.update(k)
    return all_k


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    print("old:")
    old = side(a.old)
    print("new:")
    new = side(a.new)
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(s for s in set(old) & set(new) if old[s] != new[s])
    for tag, syms in (("DIFFERENT", differ), ("GONE", gone), ("NEW", added)):
        for s in syms:
            print(tag, s)
    same = len(set(old) & set(new)) - len(differ)
    print(f"{len(old)} old, {len(new)} new: {same} same, {len(differ)} different, {len(gone)} gone, {len(added)} new")
    return 1 if differ or gone or added else 0


if __name__ == "__main__":
    sys.exit(main())
