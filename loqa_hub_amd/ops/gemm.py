"""The LDS-tiled MFMA GEMMs of the prompt passes and their dispatch.

``gemm_tile`` (csrc/kernels/gemm_tile.hip), ``gemm_sk`` (gemm_sk.hip) and
``gemm_ws`` (gemm_ws.hip) share their device pieces (csrc/kernels/gemm_mfma.h)
and, here, one epilogue map, one fp32 reference and one argument check.
``proj`` picks the measured-fastest of them per shape. Everything public is
re-exported from ``loqa_hub_amd.ops``.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from ._lib import check, kernels, ptr, stream_ptr

# epilogue numbering of csrc/kernels/gemm_mfma.h
_EPI = {"bf16": 0, "swiglu": 1, "resid": 2, "slabs": 3}


def _tiled_ref(x: torch.Tensor, w: torch.Tensor, epi: str, *, bias=None, act: str | None = None,
               residual=None, pos=None, splits: int = 1) -> torch.Tensor:
    """fp32 reference of the tiled GEMMs' epilogues (the CPU path of all three)."""
    xf, wf = x.float(), w.float()
    if epi == "slabs":
        ks = xf.shape[1] // splits
        return torch.stack([xf[:, s * ks:(s + 1) * ks] @ wf[:, s * ks:(s + 1) * ks].t()
                            for s in range(splits)])
    y = xf @ wf.t()
    if epi == "swiglu":
        F = w.shape[0] // 2
        g = y[:, :F].to(torch.bfloat16).float()
        u = y[:, F:].to(torch.bfloat16).float()
        return (g * torch.sigmoid(g) * u).to(torch.bfloat16)
    if bias is not None:
        y = y + bias.float()
    if epi == "resid":
        return (residual.float() + y).to(torch.bfloat16)
    if act == "gelu":
        y = y.to(torch.bfloat16).float()
        y = 0.5 * y * (1.0 + torch.erf(y * 0.70710678118654752))
    if pos is not None:
        rows = torch.arange(y.shape[0], device=y.device) % pos.shape[0]
        y = y.to(torch.bfloat16).float() + pos.float()[rows]
    return y.to(torch.bfloat16)


def _gt_ref(x2: torch.Tensor, w: torch.Tensor, bias, act: str | None, pos, epi: str, splits: int):
    return _tiled_ref(x2, w, epi, bias=bias, act=act, pos=pos, splits=splits)


def _sk_ref(x: torch.Tensor, w: torch.Tensor, epi: str, bias, residual, act: str | None = None):
    return _tiled_ref(x, w, epi, bias=bias, act=act, residual=residual)


def _check_operands(name: str, x: torch.Tensor, w: torch.Tensor, bias, N: int) -> None:
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise TypeError(f"{name} needs bf16 operands")
    if x.stride(1) != 1 or not w.is_contiguous():
        raise ValueError(f"{name} needs K-contiguous operands")
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N


# ------------------------------------------------------- LDS-tiled MFMA GEMM
# csrc/kernels/gemm_tile.hip: (waves along N, waves along M, LDS stages); the
# workgroup tile is (64 * WN features) x (64 * WM rows).
GEMM_TILE_LAYOUTS = {0: (2, 2, 2), 1: (2, 2, 3), 2: (4, 2, 2), 3: (2, 4, 2), 4: (4, 2, 3),
                     5: (2, 4, 3), 6: (2, 4, 2), 7: (4, 2, 2), 8: (2, 2, 2), 9: (2, 2, 2)}
# (FN, FM) 16-wide MFMA fragments per wave along features / rows
GEMM_TILE_FRAGS = {6: (8, 4), 7: (4, 8), 8: (8, 4), 9: (4, 8)}
# the measured best on every served shape (scripts/exp/gemm_tile_bench.py,
# docs/PERF.md); callers pass ``layout=`` to force another
GEMM_TILE_DEFAULT_LAYOUT = 1
_GT_ZEROS: dict = {}


def gemm_tile_dims(layout: int) -> tuple[int, int]:
    """(features, rows) of a layout's workgroup tile."""
    wn, wm, _ = GEMM_TILE_LAYOUTS[layout]
    fn, fm = GEMM_TILE_FRAGS.get(layout, (4, 4))
    return 16 * fn * wn, 16 * fm * wm


def conv_k3_weight(w: torch.Tensor, cin: int) -> torch.Tensor:
    """torch conv1d weight flattened [Cout, Cin * 3] (k = c * 3 + tap) -> the
    tiled GEMM's implicit-im2col order [Cout, 3 * Cin] (k = tap * Cin + c)."""
    cout = w.shape[0]
    return w.reshape(cout, cin, 3).permute(0, 2, 1).reshape(cout, 3 * cin).contiguous()


def conv_k3_im2col_ref(x: torch.Tensor, B: int, tin: int, stride: int) -> torch.Tensor:
    """Reference implicit im2col: x [B * tin, cin] time-major -> [B * tout, 3 * cin]
    (k = tap * cin + c, zero padding 1)."""
    cin = x.shape[1]
    xb = x.reshape(B, tin, cin)
    xp = torch.nn.functional.pad(xb, (0, 0, 1, 1))
    tout = (tin + 2 - 3) // stride + 1
    cols = [xp[:, tap: tap + stride * (tout - 1) + 1: stride] for tap in range(3)]
    return torch.cat(cols, dim=2).reshape(B * tout, 3 * cin)


def gemm_tile(x: torch.Tensor, w: torch.Tensor, *, bias: torch.Tensor | None = None,
              act: str | None = None, pos: torch.Tensor | None = None, epi: str = "bf16",
              splits: int = 1, layout: int | None = None, out: torch.Tensor | None = None,
              conv: tuple[int, int] | None = None) -> torch.Tensor:
    """Y = X W^T on the LDS-tiled MFMA GEMM (``csrc/kernels/gemm_tile.hip``).

    x [M, K] bf16 (row stride may exceed K), w [N, K] bf16 row-major.
    ``epi``: "bf16" -> [M, N] (+ f32 ``bias``, ``act`` "gelu", + bf16 ``pos``
    rows m % len(pos)); "slabs" -> f32 split-K partials [S, M, N]; "swiglu" ->
    silu(gate) * up [M, N / 2] with gate rows [0, N/2) and up rows [N/2, N).
    ``layout``: a ``GEMM_TILE_LAYOUTS`` key (default ``GEMM_TILE_DEFAULT_LAYOUT``).
    ``conv`` = (B, stride): x is a time-major conv input [B * T_in, Cin] and w a
    ``conv_k3_weight`` [N, 3 * Cin]; the output rows are (b, t_out) of the
    k = 3, padding 1 conv1d (implicit im2col: the input rows are gathered by the
    tile loader, no column matrix is built)."""
    N, K = w.shape
    if conv is not None:
        B, stride = conv
        cin = x.shape[1]
        assert K == 3 * cin
        tin = x.shape[0] // B
        tout = (tin + 2 - 3) // stride + 1
        M = B * tout
    else:
        M = x.shape[0]
        assert x.shape[1] == K, (x.shape, w.shape)
    if not x.is_cuda:
        x2 = conv_k3_im2col_ref(x, B, tin, stride) if conv is not None else x
        y = _gt_ref(x2, w, bias, act, pos, epi, splits)
        if out is not None:
            out.copy_(y)
            return out
        return y
    _check_operands("gemm_tile", x, w, bias, N)
    p = _lib.GemmTileParams()
    p.x, p.ldx, p.w = ptr(x), x.stride(0), ptr(w)
    p.M, p.N, p.K, p.S, p.epi = M, N, K, splits, _EPI[epi]
    p.act = 1 if act == "gelu" else 0
    p.bias = ptr(bias)
    if pos is not None:
        assert pos.dtype == torch.bfloat16 and pos.is_contiguous() and pos.shape[1] == N
        p.pos, p.pos_rows = ptr(pos), pos.shape[0]
    if epi == "slabs":
        y = out if out is not None else torch.empty(splits, M, N, dtype=torch.float32,
                                                    device=x.device)
        p.part = ptr(y)
    else:
        cols = N // 2 if epi == "swiglu" else N
        y = out if out is not None else torch.empty(M, cols, dtype=torch.bfloat16, device=x.device)
        assert y.shape == (M, cols) and y.stride(1) == 1
        p.y, p.ldy = ptr(y), y.stride(0)
    if conv is not None:
        z = _GT_ZEROS.get((x.device, cin))
        if z is None:
            z = _GT_ZEROS[(x.device, cin)] = torch.zeros(max(cin, 64), dtype=torch.bfloat16,
                                                         device=x.device)
        p.conv_cin, p.conv_tin, p.conv_tout, p.conv_stride, p.zeros = cin, tin, tout, stride, ptr(z)
    p.layout = GEMM_TILE_DEFAULT_LAYOUT if layout is None else layout
    check(kernels().loqa_gemm_tile(ctypes.byref(p), stream_ptr(x)), "gemm_tile")
    return y


# ---------------------------------------------------------------------------
# Split-K tiled GEMM with an in-launch reduction (csrc/kernels/gemm_sk.hip)
# layout -> (features, rows, resident workgroups per CU (LDS), per-CU efficiency)
# efficiency: relative MFMA rate of the wave tile (LDS bytes per MFMA: 64 x 64
# = 1.0; 64 x 32 tiles read 1.5x the LDS per MFMA; 128 x 64 0.75x).
# (features, rows) restate gemm_sk.hip's layout list: tests/test_gemm_shared.py
# holds them to loqa_gemm_sk_dims.
SK_LAYOUTS = {0: (128, 128, 2, 1.0), 1: (128, 64, 3, 0.85), 2: (256, 64, 2, 1.0),
              3: (256, 128, 1, 1.0), 4: (128, 64, 2, 0.9), 5: (128, 128, 1, 1.05),
              6: (256, 256, 1, 1.15), 7: (64, 64, 4, 0.6), 8: (256, 64, 1, 1.05),
              9: (256, 128, 1, 1.1), 10: (128, 128, 1, 1.1), 11: (128, 64, 1, 0.95)}
SK_CUS = 256
_SK_WS: dict = {}


# measured picks (scripts/exp/gemm_sk_bench.py --grid, cold weights, one
# MI355X; profiles/r4_gemm_sk_grid.txt): (N, K) -> [(max M, layout, chunks)]
SK_TABLE = {
    (6144, 4096): [(400, 4, 1), (900, 5, 1), (1 << 30, 0, 1)],        # Llama-3-8B qkv
    (4096, 4096): [(900, 4, 1), (1 << 30, 1, 1)],                     # o
    (28672, 4096): [(400, 4, 1), (1 << 30, 0, 1)],                    # gate|up
    (4096, 14336): [(400, 8, 3), (900, 0, 3), (1 << 30, 0, 1)],       # down
    (3840, 1280): [(1 << 30, 0, 1)],                                  # Whisper-large-v3 enc qkv
    (1280, 1280): [(2000, 4, 1), (4000, 5, 1), (1 << 30, 3, 1)],      # enc o
    (5120, 1280): [(1 << 30, 0, 1)],                                  # enc fc1
    (1280, 5120): [(2000, 4, 1), (4000, 5, 1), (1 << 30, 0, 1)],      # enc fc2
}


def gemm_sk_plan(M: int, N: int, K: int, epi: str = "bf16",
                 layouts=(0, 1, 2, 3, 4, 5)) -> tuple[int, int]:
    """(layout, K chunks) for a shape: the measured table for the served
    shapes, else an analytic plan - the fewest
    MFMA-cycle rounds over the resident workgroup slots, counting padded rows
    and wave-tile efficiency, with at most 3 K chunks (each chunk's partial
    costs a write and a serial read in the reduction: 16 chunks measured up
    to 7x slower than 1)."""
    for m_max, lay, s in SK_TABLE.get((N, K), ()):
        if M <= m_max and N % SK_LAYOUTS[lay][0] == 0:
            return lay, s
    KT = K // 64
    best, best_t = (7, 1), float("inf")
    for lay in layouts:
        bn, bm, occ, eff = SK_LAYOUTS[lay]
        if N % bn:
            continue
        tiles = -(-M // bm) * (N // bn)
        for s in (1, 2, 3):
            if s > KT or (s > 1 and KT // s < 8) or (epi == "swiglu" and s > 1):
                continue
            grid = tiles * s
            rounds = -(-grid // (SK_CUS * occ))
            t = rounds * occ * bm * bn * (KT / s) / eff + (s - 1) * bm * bn * 64.0
            if t < best_t:
                best, best_t = (lay, s), t
    return best


_SK_WS_GRAPHS: list = []   # workspaces owned by captured graphs (never reused)


def _sk_workspace(dev: torch.device, stream: int, floats: int, tiles: int):
    """Split-K partials + arrival counters (zero on entry; each tile's reducer
    re-zeroes its own). Eager launches share one growing workspace per stream
    (stream order serialises them). A launch being CAPTURED gets a workspace of
    its own that lives as long as the process: a shared one could be regrown
    by a later capture, freeing memory an earlier graph still replays into,
    and two graphs replayed on different streams would race on it."""
    if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        ws = (torch.empty(floats, dtype=torch.float32, device=dev),
              torch.zeros(tiles, dtype=torch.int32, device=dev))
        _SK_WS_GRAPHS.append(ws)
        return ws
    key = (dev, stream)
    ws = _SK_WS.get(key)
    if ws is None or ws[0].numel() < floats or ws[1].numel() < tiles:
        f = max(floats, 0 if ws is None else ws[0].numel())
        t = max(tiles, 0 if ws is None else ws[1].numel())
        ws = (torch.empty(f, dtype=torch.float32, device=dev),
              torch.zeros(t, dtype=torch.int32, device=dev))
        _SK_WS[key] = ws
    return ws


def _fused_epi_args(name: str, p, x: torch.Tensor, w: torch.Tensor, epi: str, bias, act, residual, out):
    """What gemm_sk and gemm_ws share. Returns ``(y, on_gpu)``: for CPU inputs
    ``y`` is the finished fp32-reference result (written to ``residual`` /
    ``out`` where given); for GPU inputs the operands are checked, ``y`` is the
    output tensor and the operand / epilogue fields of the params struct ``p``
    are filled (the caller adds its plan and launches)."""
    N, K = w.shape
    M = x.shape[0]
    assert x.shape[1] == K, (x.shape, w.shape)
    if epi == "resid":
        assert residual is not None and residual.shape == (M, N)
    if not x.is_cuda:
        y = _sk_ref(x, w, epi, bias, residual, act)
        dst = residual if epi == "resid" else out
        if dst is not None:
            dst.copy_(y)
            return dst, False
        return y, False
    _check_operands(name, x, w, bias, N)
    assert not act or epi == "bf16"
    assert bias is None or epi != "swiglu"
    if epi == "resid":
        y = residual
        assert y.dtype == torch.bfloat16 and y.stride(1) == 1
    else:
        cols = N // 2 if epi == "swiglu" else N
        y = out if out is not None else torch.empty(M, cols, dtype=torch.bfloat16, device=x.device)
        assert y.shape == (M, cols) and y.stride(1) == 1
    p.x, p.ldx, p.w = ptr(x), x.stride(0), ptr(w)
    p.M, p.N, p.K, p.epi = M, N, K, _EPI[epi]
    p.act = 1 if act == "gelu" else 0
    p.bias = ptr(bias)
    p.y, p.ldy = ptr(y), y.stride(0)
    return y, True


def gemm_sk(x: torch.Tensor, w: torch.Tensor, *, epi: str = "bf16", bias: torch.Tensor | None = None,
            act: str | None = None, residual: torch.Tensor | None = None,
            out: torch.Tensor | None = None, layout: int | None = None,
            splits: int | None = None) -> torch.Tensor:
    """Y = X W^T on the split-K tiled GEMM (``csrc/kernels/gemm_sk.hip``); the
    S K-chunks of a tile are summed in-launch by the tile's last workgroup.

    x [M, K] bf16 (row stride may exceed K), w [N, K] bf16 row-major.
    ``epi``: "bf16" -> [M, N] (+ f32 ``bias``, ``act`` "gelu"); "swiglu" -> silu(gate) * up
    [M, N / 2] (gate rows [0, N/2), up rows [N/2, N)); "resid" -> ``residual``
    [M, N] += X W^T (+ ``bias``) in place (one bf16 rounding), returned."""
    p = _lib.GemmSkParams()
    y, on_gpu = _fused_epi_args("gemm_sk", p, x, w, epi, bias, act, residual, out)
    if not on_gpu:
        return y
    M, (N, K) = x.shape[0], w.shape
    if layout is None or splits is None:
        pl, ps = gemm_sk_plan(M, N, K, epi)
        layout = pl if layout is None else layout
        splits = ps if splits is None else splits
    bn, bm = SK_LAYOUTS[layout][:2]
    if N % bn or K % 64:
        raise ValueError(f"gemm_sk layout {layout}: N {N} / K {K} not tileable")
    p.S, p.layout = splits, layout
    st = stream_ptr(x)
    if splits > 1:
        tiles = -(-M // bm) * (N // bn)
        ws, cnt = _sk_workspace(x.device, st, tiles * splits * bm * bn, tiles)
        p.ws, p.counters = ptr(ws), ptr(cnt)
    check(kernels().loqa_gemm_sk(ctypes.byref(p), st), "gemm_sk")
    return y


# ---------------------------------------------------------------------------
# Row-resident weight-streaming GEMM (csrc/kernels/gemm_ws.hip)
WS_MAX_BM = 384


def gemm_ws_rows(M: int, depth: int = 0) -> int:
    """Rows per workgroup: M split into the fewest blocks of <= 384 rows
    (<= 256 at depth 1), each rounded up to 64."""
    cap = WS_MAX_BM if depth == 0 else 256
    nb = -(-M // cap)
    return -(-(-(-M // nb)) // 64) * 64


def gemm_ws(x: torch.Tensor, w: torch.Tensor, *, epi: str = "bf16", bias: torch.Tensor | None = None,
            act: str | None = None, residual: torch.Tensor | None = None,
            out: torch.Tensor | None = None, depth: int | None = None,
            bm: int | None = None, splits: int = 1) -> torch.Tensor:
    """Y = X W^T on the row-resident weight-streaming GEMM: a workgroup owns
    128 output features x all the rows of its row block (up to 384), so every
    weight byte is read once; ``splits`` K chunks per tile, summed in-launch.
    Epilogues as :func:`gemm_sk`."""
    p = _lib.GemmWsParams()
    y, on_gpu = _fused_epi_args("gemm_ws", p, x, w, epi, bias, act, residual, out)
    if not on_gpu:
        return y
    M, (N, K) = x.shape[0], w.shape
    if N % 128 or K % 64:
        raise ValueError("gemm_ws needs N % 128 == 0, K % 64 == 0")
    depth = 0 if depth is None else depth
    p.bm = gemm_ws_rows(M, depth) if bm is None else bm
    p.S = splits
    st = stream_ptr(x)
    if splits > 1:
        tiles = -(-M // p.bm) * (N // 128)
        ws, cnt = _sk_workspace(x.device, st, tiles * splits * p.bm * 128, tiles)
        p.ws, p.counters = ptr(ws), ptr(cnt)
    check(kernels().loqa_gemm_ws(ctypes.byref(p), depth, st), "gemm_ws")
    return y


# ---------------------------------------------------------------------------
# Projection dispatch for prompt passes (prefill, Whisper encoder): the
# hand-written GEMM measured fastest per (N, K) and row count
# (scripts/exp/gemm_sk_bench.py --grid, cold weights; profiles/r4_gemm_proj_grid.txt):
# ("sk", layout, K chunks) = gemm_sk, ("ws", depth[, K chunks]) = gemm_ws.
PROJ_TABLE = {
    # the chunked prompt passes (LOQA_CHUNK_PREFILL) also run 64-256 rows:
    # more K chunks fill the CUs there (profiles/r4_gemm_small_m.txt; a 32 /
    # 128-row pass 4.81 / 6.33 vs 6.70 / 7.21 ms, headline neutral:
    # profiles/r4_ab_proj_small_m.txt)
    (6144, 4096): [(64, ("sk", 4, 4)), (128, ("sk", 4, 2)), (400, ("sk", 4, 1)),
                   (900, ("sk", 5, 1)), (1 << 30, ("sk", 0, 1))],                         # Llama qkv
    (4096, 4096): [(128, ("sk", 4, 4)), (256, ("sk", 4, 2)), (900, ("sk", 4, 1)),
                   (1 << 30, ("sk", 0, 1))],                                               # o
    (28672, 4096): [(256, ("ws", 1)), (384, ("ws", 0)), (900, ("ws", 0)),
                    (1 << 30, ("sk", 6, 1))],                                              # gate|up
    # 400-1000 rows (whole-prompt passes of two or three prompts, nothing
    # decoding): down on the weight-streaming GEMM with K chunks, gate|up on it
    # unsplit (600 rows: 94 vs 118 us, 160 vs 196 us; profiles/r4_ws_splitk.txt).
    # At 300-400 rows, the chunked passes beside the Whisper decoder, the split-K
    # weight-streaming down too: round 4's 3 pairs read neutral (19.03 vs 19.07),
    # round 5's 5 interleaved pairs all favour it - mixed pass 13.0 -> 12.4 ms,
    # +1.2% utt/s (profiles/r5_ab_down_ws.txt)
    (4096, 14336): [(64, ("sk", 4, 8)), (128, ("sk", 5, 8)), (256, ("sk", 5, 4)),
                    (400, ("ws", 0, 4)), (700, ("ws", 0, 4)), (1000, ("ws", 0, 2)),
                    (1 << 30, ("sk", 6, 3))],                                              # down
    # encoder qkv / fc1: gemm_ws is ~8% faster alone (24.2 / 25.8 vs 26.2 / 28.2
    # us) but its long-lived 512-thread workgroups cost the concurrent decoders
    # more than that (encoder on ws: 18.82 / 19.02 vs 19.15 / 18.99 utt/s)
    (3840, 1280): [(2000, ("sk", 1, 1)), (1 << 30, ("sk", 6, 1))],                        # enc qkv
    (1280, 1280): [(2000, ("sk", 4, 1)), (1 << 30, ("sk", 5, 1))],                        # enc o
    (5120, 1280): [(2000, ("sk", 0, 1)), (1 << 30, ("sk", 6, 1))],                        # enc fc1
    (1280, 5120): [(2000, ("sk", 4, 1)), (1 << 30, ("sk", 5, 1))],                        # enc fc2
    # Llama-3-70B TP=8 shards, prompt passes of ~320 rows (grid search,
    # profiles/r5_tp70_shard_grid.jsonl): the planner's (4, 2) / (5, 1) picks
    # were 38.1 / 85.3 us, these 27.2 / 69.7 us (hipBLASLt 28.1 / 69.8); o and
    # down shards keep the planner's (5, 1) (15.2 / 37.6 us)
    # deeper LDS rings (layouts 9 / 11, profiles/r5_sk_grid_deep.jsonl): 25.6 /
    # 62.9 us vs 26.9 / 68.9 (a TP rank runs no decoder beside its prompt pass)
    (1280, 8192): [(512, ("sk", 11, 4))],                                                  # qkv/8
    (7168, 8192): [(512, ("sk", 9, 3))],                                                   # gate|up/8
}
# the 8B prompt-pass projections at ~300 rows on the 4-stage rings (qkv 32.7 ->
# 30.3, o 32.0 -> 30.2, down 76.3 -> 73.4 us alone; one workgroup per CU
# instead of two beside the decoders): LOQA_SK_DEEP
SK_DEEP = os.environ.get("LOQA_SK_DEEP", "0") == "1"
# experiment override of the <= 400-row (chunked prompt pass) pick of a shape:
# "NxK:sk,layout,chunks;NxK:ws,depth,chunks"
for _ov in filter(None, os.environ.get("LOQA_PROJ_OVERRIDE", "").split(";")):
    try:
        _shape, _pick = _ov.split(":")
        _n, _k = map(int, _shape.split("x"))
        _kind, *_args = _pick.split(",")
        if _kind not in ("sk", "ws"):
            raise ValueError(_kind)
        PROJ_TABLE[(_n, _k)] = [(400, (_kind, *map(int, _args)))] + [
            e for e in PROJ_TABLE.get((_n, _k), []) if e[0] > 400]
    except ValueError:
        import warnings
        warnings.warn(f"LOQA_PROJ_OVERRIDE: ignoring malformed entry {_ov!r}")
if SK_DEEP:
    PROJ_TABLE[(6144, 4096)].insert(2, (400, ("sk", 11, 1)))
    PROJ_TABLE[(4096, 4096)].insert(2, (400, ("sk", 11, 1)))
    PROJ_TABLE[(4096, 14336)][3] = (400, ("sk", 9, 4))


def proj(x: torch.Tensor, w: torch.Tensor, *, epi: str = "bf16", bias: torch.Tensor | None = None,
         act: str | None = None, residual: torch.Tensor | None = None) -> torch.Tensor:
    """A prompt-pass projection on the fastest hand-written GEMM for its shape
    (``PROJ_TABLE``; shapes outside it: the gemm_sk planner). Epilogues as
    :func:`gemm_sk`."""
    M = x.shape[0]
    N, K = w.shape
    choice = None
    for m_max, c in PROJ_TABLE.get((N, K), ()):
        if M <= m_max:
            choice = c
            break
    if choice is not None and choice[0] == "ws" and N % 128 == 0:
        return gemm_ws(x, w, epi=epi, bias=bias, act=act, residual=residual, depth=choice[1],
                       splits=choice[2] if len(choice) > 2 else 1)
    if choice is not None and choice[0] == "sk" and N % SK_LAYOUTS[choice[1]][0] == 0:
        return gemm_sk(x, w, epi=epi, bias=bias, act=act, residual=residual, layout=choice[1],
                       splits=choice[2])
    return gemm_sk(x, w, epi=epi, bias=bias, act=act, residual=residual)
