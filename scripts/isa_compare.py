"""Per-kernel comparison of the device assembly of two trees (diagnostic, CPU only).

usage: python scripts/isa_compare.py [--added-default ARG] PARENT_DIR TREE_DIR name [name ...]
  (DIR/name.s from: hipcc <CXXFLAGS> --cuda-device-only -S csrc/name.hip -o DIR/name.s, as scripts/isa_stats.py)
Kernels are matched by name and template arguments, not by the mangled parameter types (a renamed struct changes
those and nothing else). Per kernel: the instruction counts, scratch bytes / SGPRs / VGPRs of both builds, and a
verdict: identical text, the same instruction multiset in another order, the same opcode multiset with other
registers or operands, or the opcodes whose counts differ.
--added-default ARG (a mangled template argument, e.g. Li3): the tree gave kernels one more trailing template
parameter whose default is ARG; a parent kernel K<args> is then compared with the tree's K<args, ARG>, and the
tree's instantiations with another value of it are listed as new.
"""
import collections
import re
import sys


def kernels(path):
    s = open(path).read()
    code, meta = {}, {}
    for m in re.finditer(r"^(\S+):\s*; @\S+\n(.*?)^\.Lfunc_end", s, re.S | re.M):
        lines = (line.split(";")[0].strip() for line in m.group(2).splitlines())
        code[key(m.group(1))] = [re.sub(r"\s+", " ", ln) for ln in lines if ln and not ln.endswith(":")
                                 and not ln.startswith(".")]
    for blk in re.split(r"\n  - \.agpr_count", s)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[key(name.group(1))] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in
                                             ("private_segment_fixed_size", "sgpr_count", "vgpr_count"))
    return code, meta


def key(symbol):
    m = re.match(r"_ZN3avr\d+([a-z0-9_]+?_kernel)(I[A-Za-z0-9_]+?E)?E", symbol)
    return symbol if not m else m.group(1) + (f"<{m.group(2)[1:-1]}>" if m.group(2) else "")


def opcodes(ins):
    return collections.Counter(i.split(" ")[0] for i in ins)


def with_default(code, meta, parent, arg):
    """The tree's K<args, arg> under the parent's key K<args> where the parent has that kernel."""
    tail = f"E{arg}>"
    for k in [k for k in code if k.endswith(tail) and k[:-len(tail)] + ">" in parent]:
        code[k[:-len(tail)] + ">"] = code.pop(k)
        if k in meta:
            meta[k[:-len(tail)] + ">"] = meta.pop(k)


def main():
    argv = sys.argv[1:]
    added = None
    if argv and argv[0] == "--added-default":
        added, argv = argv[1], argv[2:]
    for f in argv[2:]:
        (a, ma), (b, mb) = kernels(f"{argv[0]}/{f}.s"), kernels(f"{argv[1]}/{f}.s")
        if added:
            with_default(b, mb, a, added)
        print(f"== {f}.hip")
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                print(f"{k}: only in the {'parent' if k in a else 'tree'}")
                continue
            A, B = a[k], b[k]
            if A == B:
                verdict = "identical"
            elif collections.Counter(A) == collections.Counter(B):
                verdict = "same instruction multiset, other order"
            elif opcodes(A) == opcodes(B):
                verdict = "same opcode multiset, other registers / operands"
            else:
                d = opcodes(B)
                d.subtract(opcodes(A))
                verdict = "DIFFERS: " + " ".join(f"{o}{n:+d}" for o, n in sorted(d.items()) if n)
            print(f"{k:34s} insns {len(A):4d} -> {len(B):4d}  scratch/sgpr/vgpr {ma.get(k)} -> {mb.get(k)}  {verdict}")


if __name__ == "__main__":
    main()
