"""A/B of the Whisper sampling tail with and without token log-probabilities
(``STTEngine(token_logprobs=True)``, ``HUB_STT_CONFIDENCE=acoustic``), on a GPU.

``op``: ``ops.masked_argmax`` against ``ops.masked_argmax_logprob`` and
``ops.masked_argmax_logprob_probe`` (a probe column on every row), one shared
mask row, at ``--shape``: ``whisper`` (the Whisper step: f32, 16 rows x 51866
columns of a [16, 51904] lm_head output), ``llama`` (bf16, 16 x 128256, the
Llama vocabulary) or ``compact`` (bf16, 16 x 4096 with ``token_ids``: the
compact head's single-workgroup path) - between them both dtypes, and the
chunked and the single-workgroup form of the argmax kernel. Each side is a
captured graph of ``--ops`` back-to-back calls (launch overhead off the
host), replayed alternately ``--rounds`` times between device events; per
call: median, min, max over the rounds. The indices of all sides, and the
log-probabilities of the last two, must be equal.

``step``: whole decode steps of a Whisper engine (free decoding, ``--batch``
utterances, captured step graphs, synchronous steps), feature on against off on
one GPU, alternating; per step: wall time of ``transcribe()`` minus the encoder,
over the decode steps. The tokens of both sides must be equal.
"""
import argparse
import json
import os
import statistics as st
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loqa_hub_amd import ops  # noqa: E402
from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest  # noqa: E402
from loqa_hub_amd.models.configs import whisper_config  # noqa: E402
from loqa_hub_amd.ops.reference import pack_mask  # noqa: E402


# --shape: (dtype, rows, columns, row stride, token_ids)
SHAPES = {
    "whisper": (torch.float32, 16, 51866, 51904, False),    # multi-chunk, f32
    "llama": (torch.bfloat16, 16, 128256, 128256, False),   # multi-chunk, bf16
    "compact": (torch.bfloat16, 16, 4096, 4096, True),      # one workgroup per row, token_ids
}


def bench_op(n_ops: int, rounds: int, shape: str = "whisper") -> dict:
    dev = torch.device("cuda", 0)
    dtype, B, V, ld, with_ids = SHAPES[shape]
    g = torch.Generator().manual_seed(0)
    buf = (torch.randn(B, ld, generator=g) * 4).to(dtype).to(dev)
    logits = buf[:, :V]
    allowed = torch.rand(1, V, generator=g) < 0.9
    mask = pack_mask(allowed).to(dev)
    rows = torch.zeros(B, dtype=torch.int32, device=dev)
    ids = (torch.arange(V, dtype=torch.int32) * 3).to(dev) if with_ids else None
    probe = torch.full((B,), V // 2, dtype=torch.int32, device=dev)   # every row probes
    sides = {"masked_argmax": lambda: ops.masked_argmax(logits, mask, rows, ids),
             "masked_argmax_logprob": lambda: ops.masked_argmax_logprob(logits, mask, rows, ids),
             "masked_argmax_logprob_probe":
                 lambda: ops.masked_argmax_logprob_probe(logits, mask, rows, probe, ids)}
    graphs, outs = {}, {}
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        for name, fn in sides.items():
            for _ in range(3):
                outs[name] = fn()
            s.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                for _ in range(n_ops):
                    fn()
            graphs[name] = gr
        assert torch.equal(outs["masked_argmax"], outs["masked_argmax_logprob"][0])
        for x, y in zip(outs["masked_argmax_logprob"], outs["masked_argmax_logprob_probe"]):
            assert torch.equal(x, y)
        times = {k: [] for k in sides}
        for name in sides:                       # warm both graphs
            graphs[name].replay()
        s.synchronize()
        for _ in range(rounds):
            for name in sides:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                graphs[name].replay()
                b.record(s)
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / n_ops)
    return {k: {"median_us": round(st.median(v), 3), "min_us": round(min(v), 3),
                "max_us": round(max(v), 3)} for k, v in times.items()}


def bench_step(model: str, batch: int, new_tokens: int, rounds: int) -> dict:
    cfg = whisper_config(model)
    rng = np.random.default_rng(1)
    pcms = [(rng.standard_normal(16000 + 4000 * i) * 3000).astype(np.int16) for i in range(batch)]
    off = STTEngine(cfg, "cuda", seed=2, max_batch=batch)
    engines = {"off": off, "on": STTEngine(cfg, "cuda", seed=2, max_batch=batch, weights=off.weights,
                                           token_logprobs=True)}
    times, tokens = {k: [] for k in engines}, {}
    for r in range(rounds + 1):                  # round 0 captures the graphs
        for name, eng in engines.items():
            reqs = [STTRequest(p, max_new_tokens=new_tokens) for p in pcms]
            enc0, n0 = eng.stats["encode_s"], eng.stats["decode_steps"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.transcribe(reqs)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0 - (eng.stats["encode_s"] - enc0)
            tokens[name] = [q.tokens for q in reqs]
            if r:
                times[name].append(dt * 1e6 / (eng.stats["decode_steps"] - n0))
    assert tokens["on"] == tokens["off"]
    out = {k: {"median_us": round(st.median(v), 1), "min_us": round(min(v), 1),
               "max_us": round(max(v), 1)} for k, v in times.items()}
    out["steps_per_round"] = engines["on"].stats["decode_steps"] // (rounds + 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["op", "step", "both"], nargs="?", default="both")
    ap.add_argument("--ops", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="whisper")
    ap.add_argument("--model", default="whisper-large-v3")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--new-tokens", type=int, default=48)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {}
    if a.what in ("op", "both"):
        res["op"] = {"shape": a.shape, **bench_op(a.ops, a.rounds, a.shape)}
    if a.what in ("step", "both"):
        res["step"] = bench_step(a.model, a.batch, a.new_tokens, a.rounds)
    print(json.dumps(res))
