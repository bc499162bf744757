r"""Compare the gfx950 code of every kernel between two builds' saved assembly (the Makefile's -save-temps=obj output,
build/obj/*-hip-amdgcn-amd-amdhsa-gfx950.s).  Used to show that a change leaves the existing kernel instantiations' ISA
untouched: e.g. build the parent commit, copy build/obj/*.s aside, build this tree, then

    python3 tools/isa_diff.py [--rename REGEX=REPL ...] OLD_DIR build/obj

Each kernel is compared from its entry label to its .Lfunc_end marker, with label names, the kernel's own symbol, section
directives and comments normalised away; kernels
are matched by demangled name, an empty template parameter pack ignored (a kernel that gained a trailing `class... Rng` pack, e.g.
k_stratified -> k_stratified<>, is the same kernel when its plain instance's code is).  --rename REGEX=REPL (repeatable) rewrites the
OLD build's demangled names with re.sub before matching, for a kernel whose template parameter list changed: e.g. after a
constant third parameter was dropped, --rename 'k_mlp_fused<(\d+), (\d+), 1, =k_mlp_fused<\1, \2, ' pairs the old
k_mlp_fused<1, 256, 1, 8, 2, true> with the new k_mlp_fused<1, 256, 8, 2, true>.
Prints one line per kernel of the OLD build (same / DIFFERENT / missing) and the kernels only the new build has; exit status
1 if any old kernel differs or is missing."""
import glob
import os
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"^void ", "", d.replace("<>", "")) for n, d in zip(names, out)}


def kernels(path):
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        text = open(f).read()
        for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
            body = []
            for line in m.group(2).splitlines():
                line = line.split(";")[0].rstrip().replace(m.group(1), "<self>")
                if not line.strip() or line.strip().startswith((".text", ".section")):
                    continue                # a template kernel lives in a comdat section of its own
                line = re.sub(r"\.L\w+", ".L", line)          # local labels are numbered per file
                body.append(line)
            out[m.group(1)] = (os.path.basename(f), body)
    names = demangle(sorted(out))
    return {names[k]: v for k, v in out.items()}


def renamed(name, renames):
    for pat, repl in renames:
        name = re.sub(pat, repl, name)
    return name


def main(old_dir, new_dir, renames=()):
    old, new = kernels(old_dir), kernels(new_dir)
    old = {renamed(k, renames): v for k, v in old.items()}
    bad = 0
    for name in sorted(old):
        if name not in new:
            print("missing   %s" % name)
            bad += 1
        elif old[name][1] != new[name][1]:
            print("DIFFERENT %s (%d -> %d lines)" % (name, len(old[name][1]), len(new[name][1])))
            bad += 1
        else:
            print("same      %s (%d lines)" % (name, len(old[name][1])))
    for name in sorted(set(new) - set(old)):
        print("new       %s (%d lines)" % (name, len(new[name][1])))
    print("%d kernel(s) of the old build: %d identical, %d different or missing" % (len(old), len(old) - bad, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="re.sub applied to the OLD build's demangled kernel names before matching (repeatable)")
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    args = ap.parse_args()
    sys.exit(main(args.old_dir, args.new_dir, [tuple(r.split("=", 1)) for r in args.rename]))
