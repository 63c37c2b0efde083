#!/usr/bin/env python3
"""Cost of FLAC reply audio on the GPU (docs/PERF.md "FLAC replies").

* Encoder time: the three launches of ``loqa_flac_encode`` between two HIP
  events, for 4 rows of 3 s at 22.05 kHz (a noisy decaying tone), with 1024 and
  with 4096 samples a frame, alternating the two in one process; the median,
  minimum and maximum of ``--reps`` repetitions after a warm-up, and the size
  of the streams against the same rows as WAV.
* Reply cost: ``VitsTTSEngine.stats["gpu_s"]`` (launch to result on the host)
  and the bytes copied to the host per batch for the same phrases as ``wav``
  and as ``flac`` with either frame size, alternating the three engines.

One JSON line per measurement (``--out FILE`` appends them to a file as well).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loqa_hub_amd.ops import _lib  # noqa: E402
from loqa_hub_amd.ops import reference as ref  # noqa: E402

RATE = 22050
BLOCKS = (1024, 4096)


def emit(fout, **kw):
    print(json.dumps(kw), flush=True)
    if fout is not None:
        fout.write(json.dumps(kw) + "\n")


def stats_ms(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


def kernel_bench(fout, rows: int, seconds: float, reps: int) -> None:
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    n = int(seconds * RATE)
    t = np.arange(n)
    x = np.stack([9000 * np.sin(t * (0.03 + 0.01 * r)) * np.exp(-2.0 * t / n)
                  + rng.normal(0, 200, n) for r in range(rows)])
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    pcm = torch.from_numpy(x).to(dev)
    lens = torch.full((rows,), n, dtype=torch.int32, device=dev)
    k = _lib.kernels()
    calls, bufs = {}, {}
    for block in BLOCKS:
        frames = ref.flac_check(n, RATE, block)
        cap = ref.flac_capacity(n, block)
        out = torch.empty(rows, cap, dtype=torch.uint8, device=dev)
        out_len = torch.empty(rows, dtype=torch.int32, device=dev)
        staging = torch.empty(rows * frames * (2 * block + 16), dtype=torch.uint8, device=dev)
        sizes = torch.empty(2, rows * frames, dtype=torch.int32, device=dev)
        bufs[block] = (out, out_len, staging, sizes)

        def call(block=block, cap=cap, out=out, out_len=out_len, staging=staging, sizes=sizes):
            _lib.check(k.loqa_flac_encode(_lib.ptr(pcm), n, n, _lib.ptr(lens), 0, rows, RATE, block,
                                          _lib.ptr(out), cap, _lib.ptr(out_len), _lib.ptr(staging),
                                          _lib.ptr(sizes[0]), _lib.ptr(sizes[1]),
                                          _lib.stream_ptr(pcm)), "flac_encode")
        calls[block] = call
    for _ in range(5):
        for block in BLOCKS:
            calls[block]()
    torch.cuda.synchronize()
    ms = {block: [] for block in BLOCKS}
    for _ in range(reps):                      # alternate: both see the same machine state
        for block in BLOCKS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            calls[block]()
            b.record()
            torch.cuda.synchronize()
            ms[block].append(a.elapsed_time(b))
    wav = rows * (44 + 2 * n)
    for block in BLOCKS:
        out, out_len = bufs[block][0].cpu().numpy(), bufs[block][1].cpu().numpy()
        want = ref.flac_encode(x, [n] * rows, RATE, block)
        same = all(out[r, :out_len[r]].tobytes() == want[r] for r in range(rows))
        emit(fout, kernel="flac_encode", rows=rows, samples=n, block=block, reps=reps,
             ms=stats_ms(ms[block]), flac_bytes=int(out_len.sum()), wav_bytes=wav,
             ratio=round(float(out_len.sum()) / wav, 4), equals_host_model=same)


def reply_bench(fout, voice: str, batches: int) -> None:
    from loqa_hub_amd.engine.tts_engine import VitsTTSEngine
    from loqa_hub_amd.models.configs import vits_config
    texts = ["Turning on the kitchen lights.", "Okay, playing some jazz in the living room.",
             "The front door is locked.", "Setting the thermostat to twenty one degrees."]
    kinds = {"wav": ("wav", 4096), "flac-1024": ("flac", 1024), "flac-4096": ("flac", 4096)}
    engines = {name: VitsTTSEngine(vits_config(voice), "cuda", flac_block=block)
               for name, (_, block) in kinds.items()}
    for name, e in engines.items():
        for _ in range(3):
            e.synthesize_batch(texts, formats=[kinds[name][0]] * len(texts))
    per = {name: [] for name in engines}
    copied = {}
    for _ in range(batches):                   # alternate: all see the same machine state
        for name, e in engines.items():
            g0, c0 = e.stats["gpu_s"], e.stats["d2h_bytes"]
            e.synthesize_batch(texts, formats=[kinds[name][0]] * len(texts))
            per[name].append((e.stats["gpu_s"] - g0) * 1e3)
            copied[name] = e.stats["d2h_bytes"] - c0
    for name, ts in per.items():
        emit(fout, reply="vits", voice=voice, phrases=len(texts), format=name, batches=batches,
             gpu_ms=stats_ms(ts), d2h_bytes_last_batch=int(copied[name]))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--voice", default="vits-ljs", help="VITS config, or 'none'")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("flac_bench needs a GPU", file=sys.stderr)
        return 2
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "a")
    try:
        kernel_bench(fout, a.rows, a.seconds, a.reps)
        if a.voice != "none":
            reply_bench(fout, a.voice, a.batches)
    finally:
        if fout is not None:
            fout.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
