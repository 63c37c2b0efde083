"""A/B of the Whisper sampling tail with and without token log-probabilities
(``STTEngine(token_logprobs=True)``, ``HUB_STT_CONFIDENCE=acoustic``), on a GPU.

``op``: ``ops.masked_argmax`` against ``ops.masked_argmax_logprob`` at the
Whisper step shape: f32 logits, 16 rows x 51866 columns of a [16, 51904]
lm_head output, one shared suppress-mask row. Each side is a captured graph of
``--ops`` back-to-back calls (launch overhead off the host), replayed
alternately ``--rounds`` times between device events; per call: median, min,
max over the rounds. The indices of both sides must be equal.

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


def bench_op(n_ops: int, rounds: int) -> dict:
    dev = torch.device("cuda", 0)
    B, V, ld = 16, 51866, 51904
    g = torch.Generator().manual_seed(0)
    buf = (torch.randn(B, ld, generator=g) * 4).to(dev)
    logits = buf[:, :V]
    allowed = torch.rand(1, V, generator=g) < 0.9
    mask = pack_mask(allowed).to(dev)
    rows = torch.zeros(B, dtype=torch.int32, device=dev)
    sides = {"masked_argmax": lambda: ops.masked_argmax(logits, mask, rows),
             "masked_argmax_logprob": lambda: ops.masked_argmax_logprob(logits, mask, rows)}
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
        idx_new = outs["masked_argmax_logprob"][0]
        assert torch.equal(outs["masked_argmax"], idx_new)
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
    ap.add_argument("--model", default="whisper-large-v3")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--new-tokens", type=int, default=48)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {}
    if a.what in ("op", "both"):
        res["op"] = bench_op(a.ops, a.rounds)
    if a.what in ("step", "both"):
        res["step"] = bench_step(a.model, a.batch, a.new_tokens, a.rounds)
    print(json.dumps(res))
