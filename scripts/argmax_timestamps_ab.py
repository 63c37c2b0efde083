"""A/B of the Whisper sampling tail with and without the timestamp rules
(``STTEngine(timestamps=True)``, ``HUB_STT_TIMESTAMPS=segment``), on a GPU.

``op``: ``ops.masked_argmax_logprob_probe`` (MODE 2) against
``ops.masked_argmax_timestamps`` (MODE 3, every row ruled, ``ts_ctl = 2``) on
the same logits: bf16, 16 rows x 51866 columns of a [16, 51904] lm_head output,
Whisper's token layout, one shared mask row. Each side is a captured graph of
``--ops`` back-to-back calls, replayed alternately ``--rounds`` times between
device events. MODE 2 is measured ``--repeats`` times (whole blocks of rounds,
MODE 3 in between): the spread of its medians is the margin a difference has
to exceed. In a tree without MODE 3 only MODE 2 is measured.

``step``: whole decode steps of a Whisper engine (free decoding, ``--batch``
utterances, captured step graphs, synchronous steps), ``timestamps=True``
against ``False`` on one GPU, alternating; per step: wall time of
``transcribe()`` minus the encoder, over the decode steps.
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

B, V, LD = 16, 51866, 51904
EOT, TS_BEGIN, TS_COUNT = 50257, 50365, 1501


def bench_op(n_ops: int, rounds: int, repeats: int, mode2_only: bool = False) -> dict:
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    buf = (torch.randn(B, LD, generator=g) * 4).to(torch.bfloat16).to(dev)
    logits = buf[:, :V]
    allowed = torch.rand(1, V, generator=g) < 0.9
    allowed[0, EOT + 1:] = False
    mask = pack_mask(allowed).to(dev)
    rows = torch.zeros(B, dtype=torch.int32, device=dev)
    probe = torch.full((B,), EOT + 100, dtype=torch.int32, device=dev)   # every row probes
    sides = {"mode2": lambda: ops.masked_argmax_logprob_probe(logits, mask, rows, probe)}
    if hasattr(ops, "masked_argmax_timestamps") and not mode2_only:
        ctl = torch.full((B,), 2, dtype=torch.int32, device=dev)
        state = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        slot = torch.arange(B, dtype=torch.int32, device=dev)
        sides["mode3"] = lambda: ops.masked_argmax_timestamps(
            logits, mask, rows, probe, ctl, state, slot, TS_BEGIN, TS_COUNT, EOT, 50)
    graphs = {}
    s = torch.cuda.Stream(dev)
    blocks = {k: [] for k in sides}
    with torch.cuda.stream(s):
        for name, fn in sides.items():
            for _ in range(3):
                fn()
            s.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                for _ in range(n_ops):
                    fn()
            graphs[name] = gr
        for name in sides:
            graphs[name].replay()
        s.synchronize()
        for _ in range(repeats):
            times = {k: [] for k in sides}
            for _ in range(rounds):
                for name in sides:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s)
                    graphs[name].replay()
                    b.record(s)
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) * 1e3 / n_ops)
            for k, v in times.items():
                blocks[k].append(round(st.median(v), 3))
    out = {k: {"block_medians_us": v, "median_us": round(st.median(v), 3),
               "spread_us": round(max(v) - min(v), 3)} for k, v in blocks.items()}
    return out


def bench_step(model: str, batch: int, new_tokens: int, rounds: int) -> dict:
    cfg = whisper_config(model)
    rng = np.random.default_rng(1)
    pcms = [(rng.standard_normal(16000 + 4000 * i) * 3000).astype(np.int16) for i in range(batch)]
    off = STTEngine(cfg, "cuda", seed=2, max_batch=batch)
    engines = {"off": off}
    if hasattr(ops, "masked_argmax_timestamps"):
        engines["on"] = STTEngine(cfg, "cuda", seed=2, max_batch=batch, weights=off.weights,
                                  timestamps=True)
    times = {k: [] for k in engines}
    for r in range(rounds + 1):                  # round 0 captures the graphs
        for name, eng in engines.items():
            reqs = [STTRequest(p, max_new_tokens=new_tokens) for p in pcms]
            enc0, n0 = eng.stats["encode_s"], eng.stats["decode_steps"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.transcribe(reqs)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0 - (eng.stats["encode_s"] - enc0)
            if r:
                times[name].append(dt * 1e6 / (eng.stats["decode_steps"] - n0))
    out = {k: {"median_us": round(st.median(v), 1), "min_us": round(min(v), 1),
               "max_us": round(max(v), 1)} for k, v in times.items()}
    out["steps_per_round"] = {k: e.stats["decode_steps"] // (rounds + 1) for k, e in engines.items()}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["op", "step", "both"], nargs="?", default="both")
    ap.add_argument("--ops", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode2-only", action="store_true",
                    help="op: MODE 2 alone, as a tree without MODE 3 measures it")
    ap.add_argument("--model", default="whisper-large-v3")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--new-tokens", type=int, default=48)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {}
    if a.what in ("op", "both"):
        res["op"] = bench_op(a.ops, a.rounds, a.repeats, a.mode2_only)
    if a.what in ("step", "both"):
        res["step"] = bench_step(a.model, a.batch, a.new_tokens, a.rounds)
    print(json.dumps(res))
