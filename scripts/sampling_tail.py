"""Sampling tail of the LLM decode steps in a kernel trace: the sampling
kernels between the 8B lm_head GEMM and the step's step_publish (the other
decoder's kernels can interleave, so the most common sequence is reported)."""
import csv, sys, statistics as st
from collections import Counter
KEEP = ("masked_argmax", "argmax_finalize", "fillBuffer", "step_publish")
rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
tails, cur = [], None
for s, e, n in rows:
    if "skinny_gemm_kernel<2, 1, 4>" in n:
        cur = [(s, e, n)]
    elif cur is not None and any(k in n for k in KEEP):
        cur.append((s, e, n))
        if "step_publish" in n:
            tails.append(cur); cur = None
        elif len(cur) > 10:
            cur = None
if tails:
    seqs = Counter(tuple(x[2].split("(")[0][:60] for x in t[1:]) for t in tails)
    (names, cnt), = seqs.most_common(1)
    print(f"sampling tail: {len(tails)} steps; after the lm_head, most common node sequence "
          f"({cnt} steps): {len(names)} nodes")
    for n in names:
        print("     ", n)
    head = st.median([(t[0][1] - t[0][0]) / 1e3 for t in tails])
    span = st.median([(t[-1][1] - t[0][0]) / 1e3 for t in tails])
    print(f"   lm_head median {head:.1f} us; lm_head start -> step_publish end median {span:.1f} us")
else:
    print("sampling tail: no steps found")
