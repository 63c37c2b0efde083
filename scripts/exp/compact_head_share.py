"""What the compact sampling head is worth at a given share of the vocabulary.

One whole Llama decode step with its sampling tail (fused decode GEMMs, lm_head,
masked argmax), graph-replayed as in ``fp8_step_bench.py``: the full head
against compact heads over random token-id sets of 1 / 25 / 50 / 75 / 100 % of
the vocabulary. Every variant is timed ``--rounds`` times, the variants
interleaved, so the spread of repeated runs stands beside the differences.
Prints one JSON line per variant (step ms of every round, resident weight
bytes) and one summary line.

    python scripts/exp/compact_head_share.py [--model llama3-8b] [--out FILE]
    python scripts/exp/compact_head_share.py --tokenizer tokenizer.json   # + its real share
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
from loqa_hub_amd.models.llama import CompactHead  # noqa: E402
from loqa_hub_amd.ops.reference import pack_mask  # noqa: E402


def tokenizer_share(path: str) -> dict:
    """Share of a checkpoint tokenizer's vocabulary that the engine's grammar
    rows allow (CPU only)."""
    from loqa_hub_amd.engine.grammar import INTENTS, GrammarTables
    from loqa_hub_amd.engine.tokenizer import HFTokenizer
    from tokenizers import Tokenizer
    tok = HFTokenizer(path, Tokenizer.from_file(path).get_vocab_size(with_added_tokens=True))
    g = GrammarTables(tok)
    g.trie(INTENTS)
    g.trie(["true", "false"])
    ids, allowed = LLMEngine.compact_ids(g._rows)
    return dict(tokenizer=path, vocab=tok.vocab_size, allowed=int(allowed.sum()),
                share=round(int(allowed.sum()) / tok.vocab_size, 4))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=64)
    ap.add_argument("--shares", default="0.01,0.25,0.5,0.75,1.0")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokenizer", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.tokenizer:
        lines.append(tokenizer_share(args.tokenizer))
        print(json.dumps(lines[-1]), flush=True)
    eng = LLMEngine(llama_config(args.model), "cuda", max_seqs=args.seqs, max_seq_len=1024,
                    use_graphs=False, compact=True, compact_head="0")
    w, dev = eng.weights, eng.device
    V = eng.cfg.vocab_size
    seqs = []
    for i in range(args.seqs):
        r = GenRequest([], [])
        r.seq_id = 1000 + i
        eng.kv.pool.add_seq(r.seq_id, [])
        seqs.append(r)
    g = torch.Generator().manual_seed(1)

    def meta_for(n):
        feeds = [torch.randint(10, V - 10, (n,), generator=g).tolist() for _ in seqs]
        max_q, max_ctx, host = eng._meta(seqs, feeds, True, len(seqs), ops.mpad_for(n * len(seqs)))
        return eng._build_meta(eng._to_device(host), max_q, max_ctx, True)

    rows = torch.zeros(args.seqs, dtype=torch.int32, device=dev)

    def step_fn(meta, head, mask):
        def step():
            lg = eng.model.forward_decode_fused(meta, eng.kv.k, eng.kv.v, eng.attn_ws, eng.scratch,
                                                head=head)[:args.seqs]
            return ops.masked_argmax(lg, mask, rows, token_ids=None if head is None else head.ids)
        return step

    fed = 0
    while fed < args.ctx:      # grow the context, 4 tokens per sequence and step
        step_fn(meta_for(4), None, None)()
        fed += 4
    meta = meta_for(1)
    base_bytes = w.resident_bytes()
    variants = [("full", None, pack_mask(torch.ones(1, V, dtype=torch.bool)).to(dev), V, 0)]
    for sh in [float(x) for x in args.shares.split(",")]:
        n = max(1, min(V, round(sh * V)))
        allowed = torch.zeros(V, dtype=torch.bool)
        allowed[torch.randperm(V, generator=g)[:n]] = True
        ids, _ = LLMEngine.compact_ids([allowed])
        head = CompactHead(w.lm_head_p, ids.to(dev))
        cm = LLMEngine.compact_mask([allowed], ids, n).to(dev)
        variants.append((f"compact {sh:g}", head, cm, n, head.wp.numel() * head.wp.element_size()))
    # the variants must agree before their times are compared
    want = step_fn(meta, None, variants[0][2])()
    for _, head, cm, n, _ in variants[1:]:
        if n == V:
            assert torch.equal(step_fn(meta, head, cm)(), want), "100 % compact head != full head"
    reps = 6
    times = {name: [] for name, *_ in variants}
    for _ in range(args.rounds):
        for name, head, mask, _, _ in variants:
            times[name].append(round(ops.graph_time(step_fn(meta, head, mask), reps, trials=5) / reps, 4))
    for name, head, _, n, extra in variants:
        lines.append(dict(variant=name, model=args.model, seqs=args.seqs, Mpad=meta.tokens.numel(),
                          ctx=fed + 1, tokens=n, share=round(n / V, 4), step_ms=times[name],
                          step_ms_median=sorted(times[name])[len(times[name]) // 2],
                          resident_weight_bytes=base_bytes + extra, head_bytes=extra))
        print(json.dumps(lines[-1]), flush=True)
    full = times["full"]
    spread = max(full) - min(full)
    summary = dict(full_ms=full, full_spread_ms=round(spread, 4),
                   gain_ms={name: round(sorted(full)[len(full) // 2] - sorted(t)[len(t) // 2], 4)
                            for name, t in times.items() if name != "full"},
                   beats_full_every_round={name: max(t) < min(full)
                                           for name, t in times.items() if name != "full"})
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
