"""Bit-for-bit check of the three argmax ops across two builds (one-off, for
the collapse of the three masked-argmax kernels into one template).

``run --out DIR [--root TREE]``: on a GPU, call ``ops.masked_argmax``,
``masked_argmax_logprob`` and ``masked_argmax_logprob_probe`` of the package
under TREE (default: this checkout) on seeded inputs over the grid of the
existing tests - V 7 / 8192 / 8193 / 51866, row stride equal / odd / padded to
64, no mask / one shared mask row / per-row masks, f32 / bf16, continuous and
integer-valued (tied) logits, with and without ``token_ids``, probe columns 0,
8191, 8192, V - 1 and non-probing rows, a row with nothing allowed and a row
of -inf only - and save every output to DIR/<case>.npz: indices as int32,
floats as their int32 bit patterns. One plain process per build, no profiler.

``compare DIR_A DIR_B``: on the host; every array of every case must be
identical. Prints the number of cases, arrays and differing elements; exit
status 1 if anything differs.
"""
import argparse
import itertools
import os
import sys

import numpy as np


def cases():
    for V, ldk, mk, dt, tied in itertools.product(
            (7, 8192, 8193, 51866), ("eq", "odd", "pad64"), ("none", "shared", "rows"),
            ("f32", "bf16"), (False, True)):
        yield f"V{V}_{ldk}_{mk}_{dt}_{'tied' if tied else 'cont'}", V, ldk, mk, dt, tied


def run(root: str, out_dir: str) -> int:
    sys.path.insert(0, root)
    import torch
    from loqa_hub_amd import ops
    from loqa_hub_amd.ops.reference import pack_mask
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    os.makedirs(out_dir, exist_ok=True)
    B = 6
    n = 0
    for seed, (name, V, ldk, mk, dt, tied) in enumerate(cases()):
        g = torch.Generator().manual_seed(seed)
        ld = {"eq": V, "odd": V + 1 + V % 2, "pad64": -(-V // 64) * 64 + 64}[ldk]
        x = torch.randn(B, ld, generator=g) * 4
        if tied:
            x = x.round()
        x[3, : V // 2] = float("-inf")
        x[4] = float("-inf")                       # a row of -inf only
        x = x.to(torch.bfloat16 if dt == "bf16" else torch.float32).to(dev)
        logits = x[:, :V]
        mask = rows = None
        if mk != "none":
            allowed = torch.rand(1 if mk == "shared" else B, V, generator=g) < 0.7
            if mk == "rows":
                allowed[2] = False                 # nothing allowed
                allowed[5] = False
                allowed[5, V - 1] = True           # only one token allowed
            mask = pack_mask(allowed).to(dev)
            if mk == "shared":
                rows = torch.zeros(B, dtype=torch.int32, device=dev)
        probe = torch.tensor([0, -1, V - 1, min(8191, V - 1), min(8192, V - 1), -1],
                             dtype=torch.int32, device=dev)
        ids = (torch.arange(V, dtype=torch.int32) * 3 + 5).to(dev)
        arrays = {}
        for tag, tok in (("", None), ("_ids", ids)):
            arrays["idx" + tag] = ops.masked_argmax(logits, mask, rows, tok)
            i1, lp1 = ops.masked_argmax_logprob(logits, mask, rows, tok)
            i2, lp2, pr = ops.masked_argmax_logprob_probe(logits, mask, rows, probe, tok)
            arrays.update({"lse_idx" + tag: i1, "lse_lp" + tag: lp1, "probe_idx" + tag: i2,
                           "probe_lp" + tag: lp2, "probe_p" + tag: pr})
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, name + ".npz"),
                 **{k: v.cpu().numpy().view(np.int32) for k, v in arrays.items()})
        n += 1
    print(f"{n} cases written to {out_dir}")
    return 0


def compare(a: str, b: str) -> int:
    names = sorted(f for f in os.listdir(a) if f.endswith(".npz"))
    assert names and names == sorted(f for f in os.listdir(b) if f.endswith(".npz")), \
        "the two directories hold different cases"
    arrays = elems = diff = 0
    for f in names:
        za, zb = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert sorted(za.files) == sorted(zb.files), f
        for k in za.files:
            assert za[k].dtype == np.int32 and za[k].shape == zb[k].shape, (f, k)
            d = int((za[k] != zb[k]).sum())
            if d:
                print(f"DIFF {f} {k}: {d} elements")
            arrays, elems, diff = arrays + 1, elems + za[k].size, diff + d
    print(f"{len(names)} cases, {arrays} arrays, {elems} elements compared: "
          f"{diff} differing elements")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    r = sub.add_parser("run")
    r.add_argument("--out", required=True)
    r.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                  "..", ".."))
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    a = ap.parse_args()
    sys.exit(run(os.path.abspath(a.root), a.out) if a.what == "run" else compare(a.a, a.b))
