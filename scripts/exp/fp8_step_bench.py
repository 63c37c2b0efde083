"""One whole Llama decode step (fused decode GEMMs, graph replay) and the
resident weight bytes, bf16 against the fp8 (e4m3) and MXFP4 weight streams.

    python scripts/exp/fp8_step_bench.py --weights bf16 [--model llama3-8b]
    python scripts/exp/fp8_step_bench.py --weights fp8
    python scripts/exp/fp8_step_bench.py --weights mxfp4

``--seqs`` sequences each feed one token per step (8 -> Mpad 16) on a context
of ``--ctx`` tokens. ``--weights bf16`` uses nothing that the fp8 path added, so
it also runs on a tree without it (the baseline figure). Weights are the
compact single-copy layout in both cases, which is what fp8 implies; the
decode step of the default two-copy bf16 layout runs the same kernels.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from loqa_hub_amd import ops  # noqa: E402
from loqa_hub_amd.engine.llm_engine import GenRequest, LLMEngine  # noqa: E402
from loqa_hub_amd.models.configs import llama_config  # noqa: E402


def resident_bytes(w) -> int:
    seen, total = set(), 0

    def add(t):
        nonlocal total
        if isinstance(t, torch.Tensor):
            key = t.untyped_storage().data_ptr()
            if key not in seen:
                seen.add(key)
                total += t.untyped_storage().nbytes()
        elif hasattr(t, "wp") and hasattr(t, "scale"):
            add(t.wp); add(t.scale)
        elif hasattr(t, "wp") and hasattr(t, "scales"):
            add(t.wp); add(t.scales)
    for t in (w.embed, getattr(w, "lm_head", None), getattr(w, "lm_head_p", None), w.final_norm):
        add(t)
    for L in list(w.layers) + list(getattr(w, "decode_layers", [])):
        for t in L.values():
            add(t)
    return total


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--weights", choices=["bf16", "fp8", "mxfp4"], default="bf16")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    kw = dict(weight_dtype=args.weights) if args.weights != "bf16" else {}
    eng = LLMEngine(llama_config(args.model), "cuda", max_seqs=args.seqs, max_seq_len=1024,
                    use_graphs=False, compact=True, **kw)
    Mpad = ops.mpad_for(args.seqs)
    seqs = []
    for i in range(args.seqs):
        r = GenRequest([], [])
        r.seq_id = 1000 + i
        eng.kv.pool.add_seq(r.seq_id, [])
        seqs.append(r)
    g = torch.Generator().manual_seed(1)
    V = eng.cfg.vocab_size

    def meta_for(n):
        feeds = [torch.randint(10, V - 10, (n,), generator=g).tolist() for _ in seqs]
        max_q, max_ctx, host = eng._meta(seqs, feeds, True, len(seqs), ops.mpad_for(n * len(seqs)))
        return eng._build_meta(eng._to_device(host), max_q, max_ctx, True)

    def step(meta):
        return eng.model.forward_decode_fused(meta, eng.kv.k, eng.kv.v, eng.attn_ws, eng.scratch)
    fed = 0
    while fed < args.ctx:      # grow the context, 4 tokens per sequence and step
        step(meta_for(4))
        fed += 4
    meta = meta_for(1)
    assert meta.tokens.numel() == Mpad
    reps = 6
    ms = ops.graph_time(lambda: step(meta), reps, trials=5) / reps
    w = eng.weights
    row = dict(weights=args.weights, model=args.model, seqs=args.seqs, Mpad=Mpad, ctx=fed + 1,
               step_ms=round(ms, 4), resident_weight_bytes=resident_bytes(w),
               layouts={":".join(str(t) for t in k): list(v) for k, v in ops._FSPLITS.items()})
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
