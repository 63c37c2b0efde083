"""What hotword biasing costs per Whisper decoder step (``STTEngine(hotwords=
[...])``, ``HUB_STT_HOTWORDS``), on a GPU: the figures under "Hotword biasing" in
docs/PERF.md (raw: profiles/hotword_step_timing.json).

Eight freely decoded 1 s utterances (8 rows) on ``whisper-large-v3`` shapes,
random-init weights, ``max_new_tokens`` 24: the host clock around every
captured synchronous ``_decode_once`` call after the prompt (each ends in a
stream synchronisation), with hotwords off and with 50 phrases on, the two
engines alternating over the same weights. Round 0 warms up (tunes, captures);
6 timed rounds; the median over all their steps. Also, between device events,
``ops.hotword_step`` alone on 8 rows of 51866 bf16 logits.

It drives the engine's own step loop (``_admit`` / ``_decode_once``, as
scripts/beam_step_timing.py does) and decodes every request to its end.

On a tree without the feature (``STTEngine`` has no ``hotwords`` argument) only
the "off" engine is measured: that is the parent's figure.

``--rehearse``: tiny sizes on the CPU; it checks the script and measures
nothing. ``--out FILE``: the results as JSON."""
import inspect
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
from loqa_hub_amd.engine.tokenizer import _COMMON  # noqa: E402
from loqa_hub_amd.models.configs import whisper_config  # noqa: E402
from loqa_hub_amd.models.whisper import WhisperWeights  # noqa: E402

REHEARSE = "--rehearse" in sys.argv
DEV = torch.device("cpu" if REHEARSE else "cuda:0")
HAS = "hotwords" in inspect.signature(STTEngine.__init__).parameters
OUT = {"feature": HAS}
ROWS, NEW = 8, 24
_W = [w for w in dict.fromkeys(_COMMON) if len(w) > 3]
HOT = _W[:30] + [f"{a} {b}" for a, b in zip(_W[30:50], _W[50:70])]      # 50 phrases


def sync():
    if DEV.type == "cuda":
        torch.cuda.synchronize()


def med(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def step_times():
    cfg = whisper_config("test-whisper" if REHEARSE else "whisper-large-v3")
    w = WhisperWeights(cfg, DEV, seed=0)
    mk = lambda **kw: STTEngine(cfg, DEV, seed=0, max_batch=ROWS, weights=w, **kw)  # noqa: E731
    engines = {"off": mk()}
    if HAS:
        engines["on_50_phrases"] = mk(hotwords=HOT, hotword_boost=2.0)
    rng = np.random.default_rng(0)
    pcms = [(rng.standard_normal(16000) * 3000).astype(np.int16) for _ in range(ROWS)]
    per_step = {k: [] for k in engines}
    for rnd in range(2 if REHEARSE else 7):
        for name, eng in engines.items():
            reqs = [STTRequest(p, max_new_tokens=NEW) for p in pcms]
            eng._admit(reqs, list(range(ROWS)))
            while not all(r.tokens for r in reqs):
                eng._decode_once(reqs)              # the prompt (and the first sampled token)
            while True:
                live = [r for r in reqs if r.t_done == 0.0]
                if not live:
                    break
                sync()
                t0 = time.perf_counter()
                eng._decode_once(live)
                sync()
                if rnd and len(live) == ROWS:
                    per_step[name].append((time.perf_counter() - t0) * 1e3)
    res = {k: med(v) for k, v in per_step.items() if v}
    OUT["step"] = res
    print("step", json.dumps(res), flush=True)


def launch():
    from loqa_hub_amd.engine.hotwords import compile_hotwords
    from loqa_hub_amd.engine.tokenizer import get_tokenizer
    V, ld = (2048, 2052) if REHEARSE else (51866, 51904)
    auto = compile_hotwords(HOT, 2.0, get_tokenizer(V).encode, V)
    table = ops.HotwordTable(DEV)
    table.load(auto)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(ROWS, ld, generator=g).to(torch.bfloat16).to(DEV)[:, :V]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    ctl, slot = i32([2] * ROWS), i32(list(range(ROWS)))
    state, last = i32([0] * (ROWS + 1)), i32([int(auto.tok[0])] * (ROWS + 1))
    fn = lambda: ops.hotword_step(x, V, ctl, slot, state, last, table)  # noqa: E731
    for _ in range(5):
        fn()
    ts = []
    for _ in range(40):
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
    OUT["launch"] = {"hotword_step": med(ts), "nodes": auto.N, "table_entries": auto.T}
    print("launch", json.dumps(OUT["launch"]), flush=True)


if __name__ == "__main__":
    if HAS:
        launch()
    step_times()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(OUT, f, indent=1)
