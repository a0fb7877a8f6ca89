"""Per-kernel comparison of two gfx950 device assembly files (hipcc <build.py FLAGS>
--cuda-device-only -S): every .amdhsa_* directive of the kernel descriptor and the instruction
stream, with local label numbers (.LBB<function>_<block>, .Ltmp, .Lfunc_end) normalised and
assembler comments dropped. One line per kernel of the first file whose demangled name matches
--only (a regular expression); kernels only the second file has are listed as new.

  python tools/isa_compare.py parent.s new.s --only 'search_cand|search_resolve' > profiles/x.txt
"""
import argparse
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (descriptor directives, instruction lines)}"""
    text = open(path).read().split("\n")
    desc, cur = {}, None
    for ln in text:
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):
            cur = s.split()[1]
            desc[cur] = []
        elif s == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and s.startswith(".amdhsa_"):
            desc[cur].append(s)
    out = {}
    for name in desc:
        start = next(i for i, ln in enumerate(text) if ln.split(";")[0].strip() == name + ":")
        body = []
        for ln in text[start + 1:]:
            s = ln.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or s.startswith(".") and not s.endswith(":"):
                continue          # directives (.p2align, .loc, ...); labels are kept
            s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
            s = re.sub(r"\.Ltmp\d+", ".Ltmp", s)
            body.append(s)
        out[name] = (desc[name], body)
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.split("\n")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--only", default=".")
    a = ap.parse_args()
    A, B = kernels(a.parent), kernels(a.new)
    dm = demangle(sorted(set(A) | set(B)))
    short = lambda n: re.sub(r"\(.*", "", dm[n]).replace("void ", "")  # noqa: E731
    differ = 0
    # a kernel whose declared signature changed spelling (a dependent parameter type) has another
    # mangled name: matched by its demangled name without the parameter list, and said so
    by_short = {short(n): n for n in B}
    renamed = {}
    for n in list(A):
        if n not in B and short(n) in by_short and by_short[short(n)] not in A:
            renamed[n] = by_short[short(n)]
    for n in A:
        if not re.search(a.only, dm[n]):
            continue
        if n in renamed:
            B[n] = B.pop(renamed[n])
            print(f"# {short(n)}: symbol {n} -> {renamed[n]}")
        if n not in B:
            print(f"{short(n)}: missing in the new file")
            differ += 1
            continue
        (da, ia), (db, ib) = A[n], B[n]
        ninst = sum(1 for s in ia if not s.endswith(":"))
        lds = next(s.split()[1] for s in da if s.startswith(".amdhsa_group_segment_fixed_size"))
        scr = next(s.split()[1] for s in da if s.startswith(".amdhsa_private_segment_fixed_size"))
        if da == db and ia == ib:
            print(f"{short(n)}: equal ({len(da)} .amdhsa directives, static LDS {lds}, scratch {scr}; "
                  f"{ninst} instructions)")
        else:
            differ += 1
            what = []
            if da != db:
                what.append("descriptor: " + ", ".join(
                    f"{x} -> {y}" for x, y in zip(da, db) if x != y))
            if ia != ib:
                first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
                what.append(f"instruction stream: {len(ia)} -> {len(ib)} lines, first difference at "
                            f"line {first}")
            print(f"{short(n)}: DIFFERS ({'; '.join(what)})")
    for n in B:
        if n not in A and re.search(a.only, dm[n]):
            db, ib = B[n]
            ninst = sum(1 for s in ib if not s.endswith(":"))
            lds = next(s.split()[1] for s in db if s.startswith(".amdhsa_group_segment_fixed_size"))
            scr = next(s.split()[1] for s in db if s.startswith(".amdhsa_private_segment_fixed_size"))
            print(f"{short(n)}: new (static LDS {lds}, scratch {scr}; {ninst} instructions)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
