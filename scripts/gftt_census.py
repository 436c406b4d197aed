"""Static census of the gfx950 assembly of a gftt kernel: registers and the instruction mix of its loops.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S -o gftt.s hybvio_amd/csrc/gftt.hip
    python scripts/gftt_census.py gftt.s [kernel-name-substring]

Prints the mix of the whole kernel and of every labelled block of more than 8 lines.
"""
import collections
import re
import sys


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "gftt_march_kernelILi32E"
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % want, l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    body = lines[start:end]
    meta = {}
    for key in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
        for i, l in enumerate(lines):
            if l.strip().startswith(".name:") and want in l:
                for m in lines[max(0, i - 12):i + 25]:
                    if m.strip().startswith("." + key + ":"):
                        meta[key] = int(m.split(":")[1])
    print(want, meta)

    def mix(seg, title):
        ops = collections.Counter()
        for l in seg:
            t = l.strip()
            if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
                continue
            ops[t.split()[0]] += 1
        valu = sum(n for o, n in ops.items() if o.startswith("v_"))
        vmem = sum(n for o, n in ops.items() if o.startswith(("global_", "flat_", "buffer_", "scratch_")))
        salu = sum(n for o, n in ops.items() if o.startswith("s_"))
        print(f"{title}: {sum(ops.values())} instructions, VALU {valu}, SALU {salu}, VMEM {vmem}")
        print("   " + ", ".join(f"{o} {n}" for o, n in ops.most_common() if o.startswith("v_") or o.startswith(("global_", "flat_"))))

    mix(body, "whole kernel")
    # per labelled block: the loops of this kernel branch around the rare square-root path, so the steady state is read
    # off as the sum of the blocks on the common path
    cuts = [0] + [i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l.strip())] + [len(body)]
    for a, b in zip(cuts, cuts[1:]):
        if b - a > 8:
            mix(body[a:b], f"block {body[a].strip().split(':')[0]} (lines {a}..{b})")


if __name__ == "__main__":
    main()
