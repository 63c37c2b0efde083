#!/usr/bin/env python3
"""Is a kernel refactor codegen-neutral? Compares, kernel symbol by kernel
symbol, two device-only compiles of the same unit (before / after):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -Icsrc/kernels \\
      --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \\
      csrc/kernels/gemm_skinny.hip -o before.s 2> before.res

    python scripts/kernel_asm_diff.py before.s before.res after.s after.res

Per symbol: whether the instruction text between its label and ``.Lfunc_end``
is identical (comments and directives dropped, basic-block labels renumbered
per function); the compiler's resource remarks (VGPRs, AGPRs, accum_offset,
SGPRs, LDS, scratch, occupancy, spills); the counts of MFMAs, vector-memory
loads / stores / atomics, LDS reads / writes, barriers, and the multiset of
``s_waitcnt vmcnt(n)`` values.

Exit status 1 when a kernel of the "after" set is not in the "before" set, or
a surviving kernel differs in resources, in an operation count, or has more
``vmcnt(0)`` waits (a drained prefetch: see stream_k in gemm_skinny.h).
Removed kernels are listed, not failed: whether they were meant to go is the
caller's to say (``--removed-ok PATTERN`` fails every other removal).
"""
import argparse
import collections
import re
import subprocess
import sys

RES = {"sgpr": r"TotalSGPRs: (\d+)", "vgpr": r" VGPRs: (\d+)", "agpr": r"AGPRs: (\d+)",
       "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "occ": r"Occupancy \[waves/SIMD\]: (\d+)",
       "sspill": r"SGPRs Spill: (\d+)", "vspill": r"VGPRs Spill: (\d+)",
       "lds": r"LDS Size \[bytes/block\]: (\d+)"}
# operation classes by mnemonic prefix (vector memory and LDS only)
OPS = {"mfma": ("v_mfma",), "vload": ("global_load", "buffer_load", "flat_load"),
       "vstore": ("global_store", "buffer_store", "flat_store"),
       "vatomic": ("global_atomic", "buffer_atomic", "flat_atomic"),
       "ds_read": ("ds_read", "ds_load"), "ds_write": ("ds_write", "ds_store"),
       "barrier": ("s_barrier",)}


def parse_remarks(text):
    """{symbol: {resource: int}} from the -Rpass-analysis=kernel-resource-usage remarks."""
    out = {}
    for block in re.split(r"remark: Function Name: ", text)[1:]:
        out[block.split()[0]] = {k: int(m.group(1)) for k, p in RES.items() if (m := re.search(p, block))}
    return out


def parse_asm(text):
    """{symbol: {"text": [instruction lines], "accum_offset": int}} of every kernel."""
    out, name, cur, pending = {}, None, None, None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if name is None:
            if m := re.match(r"\.type\s+(\S+),@function", line):
                pending = m.group(1)
            elif pending and line == pending + ":":
                name, cur = pending, {"text": [], "accum_offset": None, "kernel": False}
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            if cur["kernel"]:
                out[name] = cur
            name = pending = None
            continue
        if line.startswith(".") and not line.endswith(":"):
            if line.startswith(".amdhsa_kernel"):
                cur["kernel"] = True
            elif m := re.match(r"\.amdhsa_accum_offset\s+(\d+)", line):
                cur["accum_offset"] = int(m.group(1))
            continue
        cur["text"].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", line)))
    return out


def op_counts(lines):
    c = collections.Counter()
    waits = collections.Counter()
    for ln in lines:
        mnem = ln.split(" ", 1)[0]
        for k, prefixes in OPS.items():
            if mnem.startswith(prefixes):
                c[k] += 1
        if mnem == "s_waitcnt" and (m := re.search(r"vmcnt\((\d+)\)", ln)):
            waits[int(m.group(1))] += 1
    return {k: c[k] for k in OPS}, dict(sorted(waits.items()))


def load(asm_path, res_path):
    with open(asm_path) as f:
        asm = parse_asm(f.read())
    with open(res_path) as f:
        res = parse_remarks(f.read())
    for sym, k in asm.items():
        k["res"] = dict(res.get(sym, {}), accum_offset=k["accum_offset"])
        k["ops"], k["vmcnt"] = op_counts(k["text"])
    return asm


def compare(before, after, removed_ok=None):
    """-> (report dict, [failure strings])"""
    fails = []
    added = sorted(set(after) - set(before))
    removed = sorted(set(before) - set(after))
    fails += [f"added: {s}" for s in added]
    if removed_ok is not None:
        fails += [f"removed, not expected: {s}" for s in removed if not re.search(removed_ok, s)]
    same, diff = [], []
    for sym in sorted(set(after) & set(before)):
        b, a = before[sym], after[sym]
        if a["text"] == b["text"]:
            same.append(sym)
        else:
            diff.append((sym, len(a["text"]) - len(b["text"])))
        for k in sorted(set(a["res"]) | set(b["res"])):
            if a["res"].get(k) != b["res"].get(k):
                fails.append(f"{k} {b['res'].get(k)} -> {a['res'].get(k)}: {sym}")
        for k in OPS:
            if a["ops"][k] != b["ops"][k]:
                fails.append(f"{k} count {b['ops'][k]} -> {a['ops'][k]}: {sym}")
        if a["vmcnt"].get(0, 0) > b["vmcnt"].get(0, 0):
            fails.append(f"vmcnt(0) waits {b['vmcnt'].get(0, 0)} -> {a['vmcnt'].get(0, 0)}: {sym}")
    return {"before": len(before), "after": len(after), "added": added, "removed": removed,
            "identical": same, "different": diff}, fails


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        out = r.stdout.split("\n")
        return dict(zip(names, out)) if r.returncode == 0 and len(out) >= len(names) else {}
    except OSError:
        return {}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before_s"), ap.add_argument("before_res")
    ap.add_argument("after_s"), ap.add_argument("after_res")
    ap.add_argument("--removed-ok", metavar="PATTERN", help="regex every removed symbol must match")
    ap.add_argument("--list", action="store_true", help="also list the removed and the non-identical kernels")
    args = ap.parse_args()
    rep, fails = compare(load(args.before_s, args.before_res), load(args.after_s, args.after_res),
                         args.removed_ok)
    deltas = [d for _, d in rep["different"]]
    print(f"kernels: {rep['before']} -> {rep['after']} ({len(rep['removed'])} removed, {len(rep['added'])} added)")
    print(f"surviving: {len(rep['identical'])} identical instruction text, {len(rep['different'])} not"
          + (f" (instruction count {min(deltas):+d} .. {max(deltas):+d})" if deltas else ""))
    if args.list:
        dem = demangle(rep["removed"] + [s for s, _ in rep["different"]])
        for s in rep["removed"]:
            print("removed  ", dem.get(s, s))
        for s, d in rep["different"]:
            print(f"differs {d:+4d}", dem.get(s, s))
    for f in fails:
        print("FAIL", f)
    print("resources, operation counts and vmcnt(0) waits of every surviving kernel: "
          + ("unchanged" if not fails else f"{len(fails)} differences"))
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
