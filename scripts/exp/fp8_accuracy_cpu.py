"""Informational: what fp8 (e4m3, per-row scale) weights do to the logits of a
random-init model, on the CPU reference path. The same prompts (the intent
prompt over the synthetic transcripts) are teacher-forced, one token per
step, through a bf16 and an fp8 engine; per position: relative logit error
and whether the greedy token agrees.

    python scripts/exp/fp8_accuracy_cpu.py [--model test-tiny] [--prompts 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from loqa_hub_amd.engine.llm_engine import GenRequest, LLMEngine  # noqa: E402
from loqa_hub_amd.engine.synthetic import make_batch  # noqa: E402
from loqa_hub_amd.models.configs import llama_config  # noqa: E402


def logits_of(eng, prompts):
    out = []
    for i, toks in enumerate(prompts):
        r = GenRequest([], [])
        r.seq_id = 5000 + i
        eng.kv.pool.add_seq(r.seq_id, [])
        rows = []
        for t in toks:
            max_q, max_ctx, host = eng._meta([r], [[t]], True, 1, 16)
            meta = eng._build_meta(eng._to_device(host), max_q, max_ctx, True)
            lg = eng.model.forward_decode_fused(meta, eng.kv.k, eng.kv.v, eng.attn_ws, eng.scratch)
            rows.append(lg[0].float())
        out.append(torch.stack(rows))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--model", default="test-tiny")
    ap.add_argument("--prompts", type=int, default=16)
    ap.add_argument("--max-tokens", type=int, default=48)
    args = ap.parse_args()
    cfg = llama_config(args.model)
    kw = dict(max_seqs=4, use_graphs=False)
    bf = LLMEngine(cfg, "cpu", compact=True, **kw)
    f8 = LLMEngine(cfg, "cpu", weight_dtype="fp8", **kw)
    utts = make_batch(0, args.prompts, [1, 2, 3, 4])
    prompts = [bf.tok.encode(f"Voice command: {u.text}", bos=True)[: args.max_tokens] for u in utts]
    a, b = logits_of(bf, prompts), logits_of(f8, prompts)
    rel = [float((y - x).norm() / x.norm()) for x, y in zip(a, b)]
    agree = torch.cat([(x.argmax(-1) == y.argmax(-1)).float() for x, y in zip(a, b)])
    print(json.dumps(dict(model=args.model, prompts=len(prompts), positions=int(agree.numel()),
                          rel_logit_error_mean=round(sum(rel) / len(rel), 4),
                          rel_logit_error_max=round(max(rel), 4),
                          greedy_token_agreement=round(float(agree.mean()), 4),
                          note="random-init weights: logits are near-flat, so agreement is a "
                               "pessimistic figure for a trained checkpoint")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
