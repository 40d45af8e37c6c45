"""Static instruction census of a kernel per source region (diagnostic).

The kernel's source carries GSM_REGION("name") marks (gsm_device.h); an
assembly listing built with -DGSM_REGION_MARKS shows each as a comment line.
Every instruction is counted under the last mark above it in the listing, by
the issue classes of tools/isa_cost.py. The listing's order is the compiler's
block layout, not the control flow: a block the compiler moved out of line
(cold paths, usually placed behind the loop) counts under the mark that
happens to precede it there, and instructions scheduled across a mark count on
the other side of it. Read the figures as shares, not as exact counts.

Usage: python tools/isa_regions.py FILE.s KERNEL_SUBSTRING
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DGSM_REGION_MARKS
 --cuda-device-only -S -Iinclude -Igs-marl_amd/csrc gs-marl_amd/csrc/gsm_seg_kernels.hip -o seg.s)
"""
import re
import sys
from collections import Counter

sys.path.insert(0, __file__.rsplit("/", 1)[0])
from isa_cost import classify  # noqa: E402

CATS = ("scalar", "valu", "lds", "vmem", "smem", "branch", "other")


def main(path, kname):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^[\w.$]+:", l) and kname in l and not l.startswith("."))
    regions, order = {}, []
    cur = "entry"
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        t = l.strip()
        m = re.match(r"^; gsm-region (.*)$", t)
        if m:
            cur = m.group(1).strip()
            continue
        if not t or t.startswith((";", ".", "//")) or re.match(r"^[\w.$]+:", t):
            continue
        parts = t.split(None, 1)
        ops = parts[1].split(";")[0] if len(parts) > 1 else ""
        if cur not in regions:
            regions[cur] = Counter()
            order.append(cur)
        regions[cur][classify(parts[0], ops)] += 1
    print(f"{'region':<20}" + "".join(f"{c:>8}" for c in CATS))
    for r in order:
        print(f"{r:<20}" + "".join(f"{regions[r][c]:>8}" for c in CATS))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
