"""Are the device kernels of two builds the same code?  No GPU needed.

    for f in $SRCS; do hipcc $CXXFLAGS --cuda-device-only -S $f -o DIR/${f%.hip}.s; done     # once per tree
    python tools/kernel_asm_diff.py DIR_A DIR_B

For every `.amdhsa_kernel <name>` in the *.s files of a directory the text from the kernel's label to its function-end
label (instructions and the .amdhsa_kernel block: registers, scratch, LDS) is taken; local labels (.LBB<k>_<n>,
.Lfunc_end<k>, ...) carry the function's ordinal within its file, so they are renumbered by first appearance.  The two
directories must hold the same kernel names with the same texts, whichever file a kernel lives in (a static kernel that
two files define counts twice).  Exit status 1 and the names that differ otherwise."""
import collections
import glob
import os
import re
import sys


def kernels(directory):
    out = collections.defaultdict(list)
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        for name in [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]:
            beg = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
            seen = {}

            def renumber(m):
                return seen.setdefault(m.group(0), "%s#%d" % (m.group(1), len(seen)))

            text = "\n".join(re.sub(r"\s*;.*", "", l) for l in lines[beg:end + 1])      # comments name basic blocks too
            out[name].append(re.sub(r"(\.L[A-Za-z_]+)[0-9_]+", renumber, text))
    return {k: sorted(v) for k, v in out.items()}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("%d kernel names in %s, %d in %s, %d differ" % (len(a), sys.argv[1], len(b), sys.argv[2], len(bad)))
    for k in bad:
        print("  " + ("only in one: " if (k in a) != (k in b) else "code differs: ") + k)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
