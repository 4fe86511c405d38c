"""Per-kernel comparison of two directories of device assembly (`make asm` output).
    python tools/isa_diff.py OLD_ASM_DIR NEW_ASM_DIR
A kernel is its text from the symbol's label to .Lfunc_end plus its .amdhsa_kernel descriptor,
looked up by symbol over all files of a directory (kernels may move between translation units),
with comments dropped and the function-number part of local labels normalised.  Prints the number of kernels
compared and identical and the names that differ or exist on one side only; exit status 1 if any."""
import glob
import os
import re
import sys

from isa_mix import kernels


def load(asm_dir):
    out = {}
    for path in sorted(glob.glob(os.path.join(asm_dir, "*.s"))):
        descs = dict(re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?\.end_amdhsa_kernel)", open(path).read(), re.M | re.S))
        for name, body in kernels(path):
            if name in descs:
                text = re.sub(r"[ \t]*;.*$", "", body + descs[name], flags=re.M)     # comments: label columns shift
                out[name] = re.sub(r"\.(LBB|LJTI|LCPI|Lfunc_begin|Lfunc_end)\d+", r".\1", text)
    return out


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k] != new[k]]
    print(f"kernels compared: {len(both)}  identical: {len(both) - len(differ)}  different: {len(differ)}")
    for title, names in (("different", differ), ("only in old", sorted(set(old) - set(new))),
                         ("only in new", sorted(set(new) - set(old)))):
        for k in names:
            print(f"  {title}: {k}")
    return 1 if differ or set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
