"""What word timestamps cost (``STTEngine(word_timestamps=True)``,
``HUB_STT_WORD_TIMESTAMPS``), on a GPU; the figures of docs/PERF.md.

* The three alignment launches (``ops.align_scores``, ``ops.align_cost``,
  ``ops.dtw``) each and back to back, between device events, 5 warm-up and 40
  timed calls, with Whisper-large-v3's 10 alignment heads: a typical command
  (N = 20 tokens, F = 150 frames) and the worst case (448 rows x 1500 frames).
* The captured synchronous Whisper decode step (``whisper-large-v3``, 8
  teacher-forced sequences, 49 steps per run) of an engine with the record
  launch against the same engine without it: host clock around steps that each
  end in a stream synchronise, the two engines alternating, one warm-up round
  (which captures the graphs) and 6 timed ones; per step.

``--rehearse``: tiny sizes on the CPU with a host clock; it checks the script
and measures nothing. ``--out FILE``: the results as JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loqa_hub_amd import ops  # noqa: E402
from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest  # noqa: E402
from loqa_hub_amd.models.configs import whisper_config  # noqa: E402
from loqa_hub_amd.models.whisper import WhisperWeights  # noqa: E402

REHEARSE = "--rehearse" in sys.argv
DEV = torch.device("cpu" if REHEARSE else "cuda:0")
OUT = {}
LARGE_V3_HEADS = [(7, 0), (10, 17), (12, 18), (13, 12), (16, 1), (17, 14), (19, 11), (21, 4),
                  (24, 1), (25, 6)]


def timed(fn, warm=5, reps=40):
    """median / min / max milliseconds of fn() (device events; CPU: host clock)."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        if DEV.type == "cuda":
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        else:
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def kernels(name, A, N, F, n_lead=3, H=20, D=64, n_ctx=448, T=1500):
    g = torch.Generator().manual_seed(1)
    heads = LARGE_V3_HEADS[:A]
    R = N + n_lead
    aq = torch.randn(A, n_ctx, D, generator=g).to(torch.bfloat16).to(DEV)
    xkv = {l: torch.randn(T, 2 * H * D, generator=g).to(torch.bfloat16).to(DEV)
           for l in {l for l, _ in heads}}
    rows = torch.arange(R, dtype=torch.int32, device=DEV)
    P = torch.empty(A * R * F, dtype=torch.float32, device=DEV)
    cost = torch.empty(N * F, dtype=torch.float32, device=DEV)
    trace = torch.empty(ops.dtw_workspace(N, F), dtype=torch.uint8, device=DEV)
    tf = torch.empty(N, dtype=torch.int32, device=DEV)
    tot = torch.empty(1, dtype=torch.float32, device=DEV)
    Pv = ops.align_scores(aq, rows, xkv, heads, 0, F, out=P)
    cv = ops.align_cost(Pv, n_lead, out=cost)
    res = {"A": A, "N": N, "F": F,
           "scores": timed(lambda: ops.align_scores(aq, rows, xkv, heads, 0, F, out=P)),
           "cost": timed(lambda: ops.align_cost(Pv, n_lead, out=cost)),
           "dtw": timed(lambda: ops.dtw(cv, trace, tf, tot)),
           "all_three": timed(lambda: (ops.align_scores(aq, rows, xkv, heads, 0, F, out=P),
                                       ops.align_cost(Pv, n_lead, out=cost),
                                       ops.dtw(cv, trace, tf, tot)))}
    OUT[name] = res
    print(name, json.dumps(res), flush=True)


def step_times():
    cfg = whisper_config("test-whisper" if REHEARSE else "whisper-large-v3")
    heads = "1:0,1:1" if REHEARSE else ",".join(f"{l}:{h}" for l, h in LARGE_V3_HEADS)
    w = WhisperWeights(cfg, DEV, seed=0)
    mk = lambda **kw: STTEngine(cfg, DEV, seed=0, max_batch=8, weights=w,  # noqa: E731
                                token_logprobs=True, **kw)
    engines = {"parent": mk(), "record": mk(word_timestamps=True, alignment_heads=heads)}
    text = " ".join(["turn on the kitchen lights and play some music in the bedroom"] * 4)
    rng = np.random.default_rng(0)
    pcms = [(rng.standard_normal(16000) * 3000).astype(np.int16) for _ in range(8)]
    per_step = {k: [] for k in engines}
    for rnd in range(2 if REHEARSE else 7):          # alternating; round 0 warms up (captures)
        for name, eng in engines.items():
            reqs = [STTRequest(p, transcript=text) for p in pcms]
            eng._admit(reqs, list(range(8)))
            if name == "record":
                eng.align.align = lambda *a, **k: [0] * 448      # time the steps, not the alignment
            live, steps = list(reqs), 0
            if DEV.type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            while live:
                eng._decode_once(live)               # synchronous captured step
                steps += 1
                live = [r for r in live if r.t_done == 0.0]
            dt = time.perf_counter() - t0
            if rnd:
                per_step[name].append(dt / steps * 1e3)
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": v}
           for k, v in per_step.items()}
    res["steps_per_run"] = steps
    OUT["captured_step"] = res
    print("captured_step", json.dumps(res), flush=True)


if __name__ == "__main__":
    if REHEARSE:
        kernels("typical", 2, 5, 20)
    else:
        kernels("typical", 10, 20, 150)
        kernels("worst", 10, 445, 1500)
    step_times()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(OUT, f, indent=1)
