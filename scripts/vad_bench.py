#!/usr/bin/env python3
"""Cost of voice activity detection on the GPU (docs/PERF.md "VAD").

For a batch of eight 5 s utterances and for one 600 s utterance, at 16 kHz:

* ``vad``: what ``STTEngine.upload`` adds per batch with a VAD utterance - the
  two launches of ``ops.vad`` (``loqa_vad_energy``, ``loqa_vad_spans``) and the
  one read-back of the spans through pinned memory, host-timed from the first
  launch to the end of the stream synchronisation;
* ``convert``: the convert launch the upload does anyway
  (``ops.pcm16_to_f32_padded`` into 30 s rows) on the same batch, timed the same
  way (launch + synchronisation);
* ``vad_kernels``: the two launches alone, from HIP events.

One JSON line per measurement (``--out FILE`` appends them to a file as well).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loqa_hub_amd import ops  # noqa: E402
from loqa_hub_amd.ops import reference as ref  # noqa: E402

N_SAMPLES = 480000


def _speech_like(rng, n):
    """Alternating 0.6 s loud and 0.4 s quiet stretches: spans to find."""
    x = rng.integers(-20, 21, n).astype(np.int16)
    for s in range(0, n, 16000):
        e = min(n, s + 9600)
        x[s:e] = rng.integers(-6000, 6001, e - s)
    return x


def wall(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def case(name, lens, reps, emit):
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    pcm = torch.from_numpy(np.concatenate([_speech_like(rng, n) for n in lens])).to(dev)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    params = ref.vad_params()
    descs, f0 = [], 0
    for o, n in zip(offs[:-1], lens):
        descs.append((int(o), n, 16000, f0))
        f0 += ref.vad_frames(n, 16000)
    U, cap = len(lens), max(ref.vad_frames(n, 16000) for n in lens) // 2 + 1
    n_sp = U * cap * 2
    buf = torch.empty(n_sp + 2 * U, dtype=torch.int32, device=dev)
    E = torch.zeros(f0, dtype=torch.int32, device=dev)
    out = (E, buf[:n_sp].view(U, cap, 2), buf[n_sp:n_sp + U], buf[n_sp + U:])
    host = torch.empty(buf.numel(), dtype=torch.int32).pin_memory()

    def vad():
        ops.vad(pcm, descs, params, out=out)
        host.copy_(buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()

    # the parent's rows: fixed 30 s windows of every utterance
    row_lens = [min(N_SAMPLES, n - w * N_SAMPLES) for n in lens for w in range(-(-n // N_SAMPLES))]
    row_offs = np.concatenate([[0], np.cumsum(row_lens)]).astype(np.int64)
    off_t = torch.from_numpy(row_offs).to(dev)

    def convert():
        ops.pcm16_to_f32_padded(pcm, off_t, N_SAMPLES, row_offs)
        torch.cuda.current_stream().synchronize()

    v = wall(vad, reps)
    c = wall(convert, reps)
    k = events(lambda: ops.vad(pcm, descs, params, out=out), reps)
    n_spans = int(host[n_sp:n_sp + U].sum())
    for what, (med, lo, hi) in (("vad", v), ("convert", c), ("vad_kernels", k)):
        emit(case=name, what=what, utterances=U, seconds=sum(lens) / 16000, rows=len(row_lens),
             us=round(med, 1), us_min=round(lo, 1), us_max=round(hi, 1), spans=n_spans)
    emit(case=name, what="ratio", vad_over_convert=round(v[0] / c[0], 3))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("vad_bench needs a GPU", file=sys.stderr)
        return 2
    fout = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fout = open(a.out, "a")

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        if fout is not None:
            fout.write(json.dumps(kw) + "\n")
    try:
        case("8x5s", [5 * 16000] * 8, a.reps, emit)
        case("1x600s", [600 * 16000], a.reps, emit)
    finally:
        if fout is not None:
            fout.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
