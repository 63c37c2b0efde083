"""Decode GEMMs on cold weights, bf16 against the fp8 (e4m3) and the MXFP4
(e2m1 + a scale byte per 32 weights) weight streams.

For each Llama-3-8B / 70B decode shape and Mpad 16 / 64 the tuner of the
engine (``ops.tune_fused`` / ``ops.tune_skinny_splits``) times every layout
with ``ops.graph_time`` on cold weight copies; the fastest layout's time per
launch is reported with the effective bandwidth over the weight bytes.

    python scripts/exp/fp8_gemm_bench.py --weights bf16 --out bf16.jsonl
    python scripts/exp/fp8_gemm_bench.py --weights fp8 --out fp8.jsonl
    python scripts/exp/fp8_gemm_bench.py --weights mxfp4 --out mxfp4.jsonl

``--weights mxfp4`` has no lm_head row: the head stays on the fp8 stream.

``--weights bf16`` uses nothing that the fp8 path added, so it also runs on a
tree without it (the baseline figures).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from loqa_hub_amd import ops  # noqa: E402
from loqa_hub_amd.ops import reference as ref  # noqa: E402

# (model, name, mode, N, K, norm, heads)
SHAPES = [
    ("8b", "qkv", "rope", 6144, 4096, "rms", (32, 8, 128)),
    ("8b", "o", "resid", 4096, 4096, None, None),
    ("8b", "gate_up", "silu", 28672, 4096, "rms", None),
    ("8b", "down", "resid", 4096, 14336, None, None),
    ("8b", "lm_head", "head", 128256, 4096, None, None),
    ("70b", "qkv", "rope", 10240, 8192, "rms", (64, 8, 128)),
    ("70b", "o", "resid", 8192, 8192, None, None),
    ("70b", "gate_up", "silu", 57344, 8192, "rms", None),
    ("70b", "down", "resid", 8192, 28672, None, None),
    ("70b", "lm_head", "head", 128256, 8192, None, None),
]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--weights", choices=["bf16", "fp8", "mxfp4"], default="bf16")
    ap.add_argument("--mpads", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--models", nargs="+", default=["8b", "70b"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    fp8, mx4 = args.weights == "fp8", args.weights == "mxfp4"
    tag = (args.weights,) if fp8 or mx4 else ()
    timed: list = []
    real = ops.graph_time

    def recording(fn, reps=8, trials=3):
        t = real(fn, reps, trials)
        timed.append(t / reps * 1e3)   # us per launch
        return t
    ops.graph_time = recording
    rows = []
    for model, name, mode, N, K, norm, heads in SHAPES:
        if model not in args.models or (mx4 and mode == "head"):
            continue
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02
        wp = ops.quantize_weight_mxfp4(w) if mx4 else ops.quantize_weight_fp8(w) if fp8 \
            else ops.shuffle_weight(w)
        del w
        wbytes = N * K * 17 // 32 if mx4 else N * K * (1 if fp8 else 2)
        cs = ref.rope_cos_sin(heads[2], 4096, 500000.0, device=dev) if heads else None
        for Mpad in args.mpads:
            timed.clear()
            if mode == "head":
                got = ops.tune_skinny_splits(wp, mpads=(Mpad,))
                layout = list(got.values())
            else:
                ops.tune_fused(wp, mode, mpads=(Mpad,), norm=norm, heads=heads, cos_sin=cs)
                layout = [v for k, v in ops._FSPLITS.items()
                          if k[:4] == (mode, N, K, Mpad) and tuple(k[4:]) == tag]
            us = min(timed)
            row = dict(weights=args.weights, model=model, gemm=name, N=N, K=K, Mpad=Mpad,
                       layout=layout, us=round(us, 2), weight_bytes=wbytes,
                       tb_s=round(wbytes / us / 1e6, 3), candidates=len(timed))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del wp
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
