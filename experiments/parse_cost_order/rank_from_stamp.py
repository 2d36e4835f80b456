#!/usr/bin/env python
"""Two class rankings for the throw-away oracle order, from a stamp_probe.py output of the parent (ENCODE part).
A: by the stamped duration of the class's blocks that had an LDS table all the time (kernel 4); a class without at least 8 such
   blocks: its memory-start duration (kernels 5 / 6) minus the median difference of the classes that have both.
B: by the duration with a start in memory (kernels 5 / 6, weighted); a class without: LDS duration plus that median difference.
Prints  A=<12 ranks, class order of corpus.SILESIA_NAMES, 11 = most expensive>  and B=... on two lines, explanation on stderr."""
import re, sys
NAMES = ("dickens", "mozilla", "mr", "nci", "ooffice", "osdb", "reymont", "samba", "sao", "webster", "xml", "x-ray")
lds, mem = {}, {}
kern, on = None, False
for line in open(sys.argv[1]):
    if line.startswith("ENCODE"): on = True; continue
    if line.startswith("DECODE"): on = False
    if not on: continue
    m = re.match(r"\s*kernel (\d+) blocks", line)
    if m: kern = int(m.group(1)); continue
    m = re.match(r"\s*(\S+)\s+n\s+(\d+)\s+start.*duration mean ([\d.]+)", line)
    if m and kern is not None:
        name, cnt, d = m.group(1), int(m.group(2)), float(m.group(3))
        if kern == 4: lds[name] = (cnt, d)
        elif kern in (5, 6):
            c0, d0 = mem.get(name, (0, 0.0))
            mem[name] = (c0 + cnt, (c0 * d0 + cnt * d) / (c0 + cnt))
both = sorted(mem[k][1] - lds[k][1] for k in NAMES if k in lds and k in mem and lds[k][0] >= 8 and mem[k][0] >= 8)
pen = both[len(both) // 2] if both else 0.4
estA, estB = {}, {}
for k in NAMES:
    estA[k] = lds[k][1] if k in lds and lds[k][0] >= 8 else max(0.0, mem[k][1] - pen)
    estB[k] = mem[k][1] if k in mem and mem[k][0] >= 8 else lds[k][1] + pen
for tag, est in (("A", estA), ("B", estB)):
    ranked = sorted(NAMES, key=lambda k: est[k])           # cheapest first -> rank 0
    rank = {k: i for i, k in enumerate(ranked)}
    print("%s=%s" % (tag, ",".join(str(rank[k]) for k in NAMES)))
    print("# %s penalty %.3f most expensive first: %s" % (tag, pen, "  ".join("%s %.3f" % (k, est[k]) for k in reversed(ranked))), file=sys.stderr)
