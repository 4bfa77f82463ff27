"""Are the gfx950 kernels of two builds the same instructions?  Disassembles the code object of every object file in two
build directories (normalizingflows.jl_amd/build of two checkouts), strips addresses, comments and the numbering of local
labels, and compares the text per demangled kernel name.  Prints the kernels only in A, the kernels only in B and the common
kernels whose instruction text differs, each with its class: "reordered" when the instruction count, the histogram of
mnemonics (the first token of a line) and the kernel's row of tools/kernel_resources.py are all equal -- the same instructions in
another order or under other register names, as far as counting can tell -- and "changed" otherwise.  Exits non-zero if any common
kernel changed, and if any was reordered unless --allow-reordered is given.  A comparison of text and counts.
usage: python tools/isa_identity.py <build-dir-A> <build-dir-B> [--rename 'old=new' ...] [--allow-reordered]
  --rename: `old` is replaced by `new` in A's kernel names before the comparison (a template parameter that went away)"""
import argparse
import collections
import difflib
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_objects, kernel_table


def kernels(bdir):
    """{demangled name: [normalised instruction lines]} of every function in the code objects under `bdir`"""
    blocks = {}
    with tempfile.TemporaryDirectory(prefix="nfhip_isa_") as tmp:
        for obj, co in code_objects(bdir, tmp):
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "--symbolize-operands", co],
                                 capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.split("\n"):
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
                if m and not re.fullmatch(r"L\d+", m.group(1)):
                    cur = blocks.setdefault((obj, m.group(1)), [])
                elif cur is not None:
                    text = line.split("//")[0].strip()  # the comments carry the addresses
                    if text and text != "...":  # "...": objdump's elision of the zero fill between two functions, not an instruction
                        cur.append(text)
    for lines in blocks.values():  # local labels are numbered per file: renumber them per kernel, in the order they are defined
        order = {m.group(1): f"L{i}" for i, m in enumerate(filter(None, (re.fullmatch(r"<(L\d+)>:", t) for t in lines)))}
        lines[:] = [re.sub(r"\bL\d+\b", lambda m: order.get(m.group(0), m.group(0)), t) for t in lines]
    mangled = sorted(blocks)
    names = subprocess.run(["c++filt"], input="\n".join(m for _, m in mangled), capture_output=True, text=True).stdout.split("\n")
    return {n: blocks[k] for n, k in zip(names, mangled)}


def histogram(lines):
    """{mnemonic: count} of a kernel's instruction lines (labels left out)"""
    return collections.Counter(t.split()[0] for t in lines if not t.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--allow-reordered", action="store_true")
    args = ap.parse_args()
    ka, kb = kernels(args.a), kernels(args.b)
    ra, rb = ({r[0]: r[1:] for r in kernel_table(d)} for d in (args.a, args.b))  # (agpr, vgpr, sgpr, scratch, lds) by name
    for r in args.rename:
        old, new = r.split("=", 1)
        ka = {n.replace(old, new): t for n, t in ka.items()}
        ra = {n.replace(old, new): t for n, t in ra.items()}
    common = sorted(set(ka) & set(kb))
    differ = [n for n in common if ka[n] != kb[n]]
    print(f"A: {args.a}: {len(ka)} kernels, {sum(map(len, ka.values()))} instructions")
    print(f"B: {args.b}: {len(kb)} kernels, {sum(map(len, kb.values()))} instructions")
    reordered = [n for n in differ if len(ka[n]) == len(kb[n]) and histogram(ka[n]) == histogram(kb[n]) and ra.get(n) == rb.get(n)]
    changed = [n for n in differ if n not in reordered]
    for title, names in (("only in A", sorted(set(ka) - set(kb))), ("only in B", sorted(set(kb) - set(ka))),
                         ("differ, reordered (count, histogram and resources equal)", reordered), ("differ, changed", changed)):
        print(f"{title}: {len(names)}")
        for n in names:
            print(f"  {n}")
            if n in differ:  # instructions, then agpr vgpr sgpr scratch lds, of A -> of B
                print(f"    {len(ka[n])} {ra.get(n)} -> {len(kb[n])} {rb.get(n)}")
    for n in differ[:5]:  # the first lines of the first few differences, to see what kind they are
        print("\n".join(list(difflib.unified_diff(ka[n], kb[n], "A: " + n[:100], "B", lineterm="", n=1))[:20]))
    print(f"common: {len(common)}, identical: {len(common) - len(differ)}, reordered: {len(reordered)}, changed: {len(changed)}")
    return 1 if changed or (reordered and not args.allow_reordered) else 0


if __name__ == "__main__":
    sys.exit(main())
