#!/usr/bin/env python3
"""Cost of sample-rate conversion on the GPU (docs/PERF.md "Sample-rate
conversion").

* Kernel time, graph-timed (a captured graph of back-to-back launches, HIP
  events around its replay): ``loqa_pcm16_resample_pad`` for 8 rows of 30 s at
  48 kHz and at 44.1 kHz, beside ``loqa_pcm16_f32_pad`` for the same 8 rows at
  16 kHz, and the Whisper encoder on those rows for scale.
* Reply cost: ``VitsTTSEngine.stats["gpu_s"]`` per phrase batch with
  ``sample_rate=16000`` against the voice's own rate, alternating the two.

One JSON line per measurement (``--out FILE`` appends them to a file as well).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loqa_hub_amd import ops  # noqa: E402
from loqa_hub_amd.ops import _lib  # noqa: E402
from loqa_hub_amd.ops import reference as ref  # noqa: E402

N_SAMPLES = 480000


def gtime(fn, inner=10, reps=15):
    """Per-call time (us) of ``fn`` replayed from a captured graph of ``inner`` calls."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def emit(fout, **kw):
    print(json.dumps(kw), flush=True)
    if fout is not None:
        fout.write(json.dumps(kw) + "\n")


def kernel_bench(fout, rows_n: int, encoder: str) -> None:
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    k = _lib.kernels()
    out = torch.empty(rows_n, N_SAMPLES, dtype=torch.float32, device=dev)
    sumsq = torch.empty(rows_n, dtype=torch.float32, device=dev)
    for rate in (16000, 44100, 48000):
        n_src = 30 * rate
        pcm = torch.from_numpy(rng.integers(-32768, 32768, rows_n * n_src, dtype=np.int16)).to(dev)
        tab, L, M, T = ops.resample_filter(rate, 16000, dev)
        desc = np.array([(i * n_src, n_src, 0, N_SAMPLES, L, M, T, tab.data_ptr())
                         for i in range(rows_n)], np.int64)
        ddev = torch.from_numpy(desc).to(dev)

        def resample():
            _lib.check(k.loqa_pcm16_resample_pad(_lib.ptr(pcm), _lib.ptr(out), _lib.ptr(ddev),
                                                 desc.ctypes.data, _lib.ptr(sumsq), rows_n,
                                                 N_SAMPLES, _lib.stream_ptr(pcm)), "resample_pad")
        # bytes: PCM16 in + f32 out; flops: 2 per tap
        mb = (pcm.numel() * 2 + out.numel() * 4) / 1e6
        gflop = 2.0 * T * out.numel() / 1e9
        med, lo, hi = gtime(resample)
        emit(fout, kernel="pcm16_resample_pad", rate=rate, rows=rows_n, taps=T, us=round(med, 1),
             us_min=round(lo, 1), us_max=round(hi, 1), MB=round(mb, 1), GFLOP=round(gflop, 3),
             GBps=round(mb / med * 1e3, 1), GFLOPps=round(gflop / med * 1e6, 1))
        if rate == 16000:
            offs = torch.arange(rows_n + 1, dtype=torch.int64, device=dev) * n_src

            def plain():
                _lib.check(k.loqa_pcm16_f32_pad(_lib.ptr(pcm), _lib.ptr(out), _lib.ptr(offs),
                                                _lib.ptr(sumsq), rows_n, N_SAMPLES,
                                                _lib.stream_ptr(pcm)), "f32_pad")
            med, lo, hi = gtime(plain)
            emit(fout, kernel="pcm16_f32_pad", rate=rate, rows=rows_n, us=round(med, 1),
                 us_min=round(lo, 1), us_max=round(hi, 1), MB=round(mb, 1),
                 GBps=round(mb / med * 1e3, 1))
    if encoder != "none":
        from loqa_hub_amd.models.configs import whisper_config
        from loqa_hub_amd.models.whisper import WhisperModel, WhisperWeights
        model = WhisperModel(WhisperWeights(whisper_config(encoder), dev, seed=0))
        audio = out * 0.1
        with torch.inference_mode():
            med, lo, hi = gtime(lambda: model.encode(audio), inner=2, reps=7)
        emit(fout, kernel="whisper_encoder", model=encoder, rows=rows_n, us=round(med, 1),
             us_min=round(lo, 1), us_max=round(hi, 1))


def reply_bench(fout, voice: str, batches: int) -> None:
    from loqa_hub_amd.engine.tts_engine import VitsTTSEngine
    from loqa_hub_amd.models.configs import vits_config
    texts = ["Turning on the kitchen lights.", "Okay, playing some jazz in the living room.",
             "The front door is locked.", "Setting the thermostat to twenty one degrees."]
    engines = {rate: VitsTTSEngine(vits_config(voice), "cuda", sample_rate=rate) for rate in (0, 16000)}
    for e in engines.values():
        for _ in range(3):
            e.synthesize_batch(texts)
    per = {rate: [] for rate in engines}
    for _ in range(batches):                  # alternate: both see the same machine state
        for rate, e in engines.items():
            g0 = e.stats["gpu_s"]
            e.synthesize_batch(texts)
            per[rate].append(e.stats["gpu_s"] - g0)
    for rate, ts in per.items():
        ts.sort()
        emit(fout, reply="vits", voice=voice, phrases=len(texts), out_rate=engines[rate].sample_rate,
             gpu_ms_median=round(ts[len(ts) // 2] * 1e3, 3), gpu_ms_min=round(ts[0] * 1e3, 3),
             gpu_ms_max=round(ts[-1] * 1e3, 3), batches=batches)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--encoder", default="whisper-base", help="Whisper config, or 'none'")
    ap.add_argument("--voice", default="vits-ljs", help="VITS config, or 'none'")
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("resample_bench needs a GPU", file=sys.stderr)
        return 2
    assert ref.resample_len(30 * 48000, 48000, 16000) == N_SAMPLES
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "a")
    try:
        kernel_bench(fout, a.rows, a.encoder)
        if a.voice != "none":
            reply_bench(fout, a.voice, a.batches)
    finally:
        if fout is not None:
            fout.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
