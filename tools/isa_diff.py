"""Per-kernel comparison of two directories of device assembly (`make asm` output).
    python tools/isa_diff.py [--detail] OLD_ASM_DIR NEW_ASM_DIR
A kernel is its text from the symbol's label to .Lfunc_end plus its .amdhsa_kernel descriptor,
looked up by symbol over all files of a directory (kernels may move between translation units),
with comments dropped and the function-number part of local labels normalised.  Prints the number of kernels
compared and identical and the names that differ or exist on one side only; exit status 1 if any.

--detail adds, for each kernel that differs: VGPRs, AGPRs, SGPRs, scratch and LDS of both sides, the
number of lines of both sides and of differing lines, whether the text from the first v_mfma line
to the end (descriptor included) is identical, and whether every differing line precedes the first
s_barrier: what a change confined to a kernel's once-per-block prologue looks like."""
import difflib
import glob
import os
import re
import sys

from isa_mix import kernels

FIELDS = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"),
          ("lds", "LDSByteSize"))


def load(asm_dir):
    """({symbol: normalised text}, {symbol: the five resource fields of the compiler's summary})."""
    out, res = {}, {}
    for path in sorted(glob.glob(os.path.join(asm_dir, "*.s"))):
        whole = open(path).read()
        descs = dict(re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?\.end_amdhsa_kernel)", whole, re.M | re.S))
        for name, body in kernels(path):
            if name in descs:
                text = re.sub(r"[ \t]*;.*$", "", body + descs[name], flags=re.M)     # comments: label columns shift
                out[name] = re.sub(r"\.(LBB|LJTI|LCPI|Lfunc_begin|Lfunc_end)\d+", r".\1", text)
                summary = whole[whole.index(body) + len(body):][:4096]
                res[name] = tuple(int(m.group(1)) if m else None
                                  for m in (re.search(rf"^; {key}: (\d+)", summary, re.M) for _, key in FIELDS))
    return out, res


def first(lines, word):
    return next((i for i, line in enumerate(lines) if word in line), len(lines))


def detail(name, old, new, res_old, res_new):
    a, b = ([line for line in t.splitlines() if line.strip()] for t in (old, new))
    ops = [op for op in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if op[0] != "equal"]
    changed = sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops)
    tail_same = a[first(a, "v_mfma"):] == b[first(b, "v_mfma"):]
    bar_a, bar_b = first(a, "s_barrier"), first(b, "s_barrier")
    before = all(i2 <= bar_a and j2 <= bar_b for _, _, i2, _, j2 in ops)
    fmt = lambda r: " ".join(f"{k}={v}" for (k, _), v in zip(FIELDS, r))
    print(f"    old: {fmt(res_old)}  lines={len(a)}")
    print(f"    new: {fmt(res_new)}  lines={len(b)}")
    print(f"    resources {'equal' if res_old == res_new else 'DIFFER'}; {changed} lines differ; "
          f"from the first v_mfma to the end: {'identical' if tail_same else 'DIFFERENT'}; "
          f"every difference before the first s_barrier: {'yes' if before else 'NO'}")


def main():
    args = [a for a in sys.argv[1:] if a != "--detail"]
    (old, res_old), (new, res_new) = load(args[0]), load(args[1])
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k] != new[k]]
    print(f"kernels compared: {len(both)}  identical: {len(both) - len(differ)}  different: {len(differ)}")
    for title, names in (("different", differ), ("only in old", sorted(set(old) - set(new))),
                         ("only in new", sorted(set(new) - set(old)))):
        for k in names:
            print(f"  {title}: {k}")
            if title == "different" and "--detail" in sys.argv[1:]:
                detail(k, old[k], new[k], res_old[k], res_new[k])
    return 1 if differ or set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
