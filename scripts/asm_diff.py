#!/usr/bin/env python3
"""Developer aid: compare the device code of two builds kernel by kernel, whichever file a kernel lives in.
usage: scripts/asm_diff.py dir_a dir_b      (two directories of hipcc -save-temps output: every *gfx950*.s in them is read)

One line per kernel: the lines that differ, of how many, and the file(s) it was found in; then the differing lines of every kernel that
has any, kernels that exist on one side only or more than once, and a total. Kernels are matched by demangled name with the
anonymous-namespace tag dropped. Of a kernel's text -- its code and its .amdhsa_kernel descriptor (registers, LDS, scratch) -- comments
and .loc / .file / .cfi lines are dropped and the function number in local labels is blanked, nothing else. It compares text and looks
for nothing in particular. Exit status 1 when anything differs."""
import difflib, glob, os, re, subprocess, sys

DROP = re.compile(r"\s*\.(loc|file|cfi_\w+)\b")
LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::", "", d) for n, d in zip(names, out)}


def normalise(lines):
    out = []
    for l in lines:
        l = l.split(";", 1)[0].rstrip()
        if l.strip() and not DROP.match(l):
            out.append(LABEL.sub(lambda m: ".L" + m.group(1), l))
    return out


def kernels(directory):
    """{demangled name: [(file, normalised lines), ...]} of every kernel of every device assembly file of the directory"""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*gfx950*.s"))):
        lines = open(path).read().split("\n")
        desc = {}                                              # mangled name -> descriptor lines
        for i, l in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
            if m:
                end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
                desc[m.group(1)] = lines[i:end + 1]
        names = demangle(list(desc))
        short = re.sub(r"-hip-amdgcn.*$", "", os.path.basename(path))
        for mangled, d in desc.items():
            start = next(j for j, l in enumerate(lines) if l.startswith(mangled + ":"))
            end = next(j for j in range(start, len(lines)) if lines[j].startswith(".Lfunc_end"))
            found.setdefault(names[mangled], []).append((short, normalise(lines[start:end]) + normalise(d)))
    return found


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    total = total_lines = bad = 0
    details = []
    for name in sorted(set(a) | set(b)):
        ka, kb = a.get(name, []), b.get(name, [])
        where = ",".join(f for f, _ in ka) + " -> " + ",".join(f for f, _ in kb)
        if len(ka) != 1 or len(kb) != 1:
            print(f"{'':>7s} present {len(ka)} x in a, {len(kb)} x in b: {name}   [{where}]")
            bad += 1
            continue
        ta, tb = ka[0][1], kb[0][1]
        diff = [] if ta == tb else [l for l in difflib.unified_diff(ta, tb, "a/" + ka[0][0], "b/" + kb[0][0], lineterm="", n=0)]
        n = sum(1 for l in diff[2:] if l[0] in "+-")
        total += n
        total_lines += len(ta)
        print(f"{n:7d} differing lines of {len(ta)}: {name}   [{where}]")
        if n:
            details += ["", name] + diff
    print("\n".join(details))
    print(f"\ntotal: {total} differing lines of {total_lines} in {len(set(a) | set(b)) - bad} kernels; {bad} kernels not present exactly once on each side")
    sys.exit(1 if total or bad else 0)


if __name__ == "__main__":
    main()
