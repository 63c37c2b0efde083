"""What a beam search step costs (``STTEngine(beam_size=5)``,
``HUB_STT_BEAM_SIZE``), on a GPU; the figures of docs/PERF.md.

One freely decoded utterance (one group) on ``whisper-large-v3`` shapes,
random-init weights, ``max_new_tokens`` 24: the host clock around
``_decode_once`` calls that each end in a device read-back, the prompt steps
left out, per search step. In the same run, alternating with it, the greedy
engine (``beam_size=1``) decodes the same utterance one synchronous step at a
time: the captured step, and the eager-launch step the beam engine builds on
(``use_graphs=False``). Round 0 warms up (tunes, captures); 6 timed rounds.
Also, between device events, the three beam launches alone on 5 rows of 51866
bf16 logits.

``--rehearse``: tiny sizes on the CPU; it checks the script and measures
nothing. ``--out FILE``: the results as JSON."""
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
B, NEW = 5, 24


def sync():
    if DEV.type == "cuda":
        torch.cuda.synchronize()


def step_times():
    cfg = whisper_config("test-whisper" if REHEARSE else "whisper-large-v3")
    w = WhisperWeights(cfg, DEV, seed=0)
    mk = lambda **kw: STTEngine(cfg, DEV, seed=0, max_batch=8, weights=w,  # noqa: E731
                                token_logprobs=True, **kw)
    engines = {"greedy_captured": mk(), "greedy_eager": mk(use_graphs=False),
               "beam5": mk(beam_size=B)}
    pcm = (np.random.default_rng(0).standard_normal(16000) * 3000).astype(np.int16)
    per_step = {k: [] for k in engines}
    steps = {}
    for rnd in range(2 if REHEARSE else 7):
        for name, eng in engines.items():
            r = STTRequest(pcm, max_new_tokens=NEW)
            eng._admit([r], [0])
            while not r.tokens and r.beam is None and r.t_done == 0.0:
                eng._decode_once([r])               # the prompt (and the first sampled token)
            n = 0
            sync()
            t0 = time.perf_counter()
            while r.t_done == 0.0:
                eng._decode_once([r])
                n += 1
            sync()
            dt = time.perf_counter() - t0
            steps[name] = n
            if rnd and n:
                per_step[name].append(dt / n * 1e3)
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": v,
               "steps_per_run": steps[k]} for k, v in per_step.items() if v}
    res["beam_kv_copies"] = engines["beam5"].stats["beam_kv_copies"]
    OUT["step"] = res
    print("step", json.dumps(res), flush=True)


def launches():
    V, ld = (100, 104) if REHEARSE else (51866, 51904)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, ld, generator=g).to(torch.bfloat16).to(DEV)[:, :V]
    cum = torch.zeros(1, B, device=DEV)
    cid, clp, elp = ops.beam_topk(x, None, None, 3, B)
    k = torch.zeros(32, 64, 20, 16, 64, dtype=torch.bfloat16, device=DEV) if not REHEARSE else \
        torch.zeros(2, 8, 2, 16, 64, dtype=torch.bfloat16, device=DEV)
    v = torch.zeros_like(k)
    pairs = [(0, 4), (1, 5), (0, 6), (1, 7)]        # two forks of a two-block history

    def timed(fn, warm=5, reps=40):
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

    res = {"beam_topk": timed(lambda: ops.beam_topk(x, None, None, 3, B)),
           "masked_argmax_logprob": timed(lambda: ops.masked_argmax_logprob(x)),
           "beam_merge": timed(lambda: ops.beam_merge(cid, clp, elp, cum, B)),
           "kv_copy_blocks": timed(lambda: ops.kv_copy_blocks(k, v, pairs))}
    OUT["launches"] = res
    print("launches", json.dumps(res), flush=True)


if __name__ == "__main__":
    launches()
    step_times()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(OUT, f, indent=1)
