#!/usr/bin/env python3
"""The Whisper decode alone with the start-of-transcript probe off / on / auto:
one set of weights, three engines, batches of 8 teacher-forced synthetic
utterances through the scheduler (two-deep pipeline, captured graphs),
interleaved rounds. Prints one JSON line per engine and round: the mean decode
span (decoder start to transcript), the batch's wall time and its decoder steps.

  python scripts/exp/sot_probe_stt_ab.py --stt whisper-large-v3 --rounds 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest  # noqa: E402
from loqa_hub_amd.engine.synthetic import make_batch  # noqa: E402
from loqa_hub_amd.models.configs import whisper_config  # noqa: E402
from loqa_hub_amd.models.whisper import WhisperWeights  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--stt", default="whisper-large-v3")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=6, help="timed batches per engine and round")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = whisper_config(args.stt)
    weights = WhisperWeights(cfg, dev, seed=0)
    kinds = {"off": {}, "on": {"sot_probe": True}, "auto": {"language": "auto"}}
    engines = {}
    for k, kw in kinds.items():
        e = STTEngine(cfg, dev, seed=0, max_batch=args.batch, weights=weights, **kw)
        e.warmup_graphs()
        engines[k] = e
    utts = make_batch(0, args.batch, [1, 2, 3, 4])

    def batch(eng):
        reqs = [STTRequest(u.pcm, transcript=u.text) for u in utts]
        t0 = time.perf_counter()
        eng.submit_batch(reqs).result(timeout=300)
        wall = time.perf_counter() - t0
        return wall, [r.t_done - r.t_dec0 for r in reqs]
    for eng in engines.values():
        batch(eng)                                # warm-up
    for rnd in range(args.rounds):
        for k, eng in engines.items():
            s0 = eng.stats["decode_steps"]
            walls, spans = [], []
            for _ in range(args.batches):
                w, sp = batch(eng)
                walls.append(w)
                spans += sp
            print(json.dumps({"stt": args.stt, "probe": k, "round": rnd, "batch": args.batch,
                              "decode_span_ms_mean": round(float(np.mean(spans)) * 1e3, 3),
                              "batch_wall_ms_mean": round(float(np.mean(walls)) * 1e3, 3),
                              "decode_steps_per_batch": (eng.stats["decode_steps"] - s0) / args.batches}),
                  flush=True)
    for eng in engines.values():
        eng.stop()
    return 0


if __name__ == "__main__":
    sys.exit(main())
