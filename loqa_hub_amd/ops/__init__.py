"""Hot ops of the voice hub.

Every op has two implementations:

* the **HIP kernel** (``csrc/kernels``, gfx950 MFMA/LDS) used whenever the inputs
  live on the GPU - a missing native library is a hard error there, never a
  silent fallback;
* a plain-PyTorch fp32 **reference** (``loqa_hub_amd.ops.reference``) used for
  CPU inputs (the CPU test tier, the config-1 plumbing path) and as the
  numerics oracle in ``tests/test_kernels_gpu.py``.

Plain GEMMs go to hipBLASLt through ``torch.nn.functional.linear``; every fused
elementwise/normalisation/attention/audio op around them is ours.
"""
from __future__ import annotations

import copy
import ctypes
import math
import os

import torch

from . import reference as ref
from . import _lib
from ._lib import FusedParams, check, kernels, ptr, stream_ptr


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _bf16_contig(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be bfloat16, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


# --------------------------------------------------------------------- norms
def _norm_rows(x: torch.Tensor, residual, row_idx) -> tuple[int, int]:
    d = x.shape[-1]
    if row_idx is not None:
        # gathered rows: y[i] = norm(x[row_idx[i]]); no residual update then
        assert residual is None and x.dim() == 2
        assert row_idx.dtype == torch.int64 and row_idx.is_contiguous()
        return row_idx.numel(), d
    return x.numel() // d, d


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float,
            residual: torch.Tensor | None = None,
            row_idx: torch.Tensor | None = None) -> torch.Tensor:
    """y = rmsnorm(x [+ residual]) * w; if residual is given it is updated in place
    to x + residual (the fused pre-norm residual stream). ``row_idx`` (int64)
    normalises only rows x[row_idx] (the decode step's logit rows) in the same
    launch."""
    if not _gpu(x):
        if row_idx is not None:
            x = x.index_select(0, row_idx.long())
        return ref.rmsnorm(x, w, eps, residual)
    rows, d = _norm_rows(x, residual, row_idx)
    _bf16_contig(x, "x"); _bf16_contig(w, "w")
    if residual is not None:
        _bf16_contig(residual, "residual")
        assert residual.shape == x.shape
    assert w.numel() == d
    y = torch.empty((rows, d) if row_idx is not None else x.shape, dtype=x.dtype, device=x.device)
    check(kernels().loqa_rmsnorm(ptr(x), ptr(residual), ptr(w), ptr(y), rows, d, eps,
                                 ptr(row_idx), stream_ptr(x)), "rmsnorm")
    return y


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float,
              residual: torch.Tensor | None = None,
              row_idx: torch.Tensor | None = None) -> torch.Tensor:
    """y = layernorm(x [+ residual]) * w + b; ``residual`` / ``row_idx`` as in
    :func:`rmsnorm`."""
    if not _gpu(x):
        if row_idx is not None:
            x = x.index_select(0, row_idx.long())
        return ref.layernorm(x, w, b, eps, residual)
    rows, d = _norm_rows(x, residual, row_idx)
    _bf16_contig(x, "x"); _bf16_contig(w, "w"); _bf16_contig(b, "b")
    if residual is not None:
        _bf16_contig(residual, "residual")
        assert residual.shape == x.shape
    y = torch.empty((rows, d) if row_idx is not None else x.shape, dtype=x.dtype, device=x.device)
    check(kernels().loqa_layernorm(ptr(x), ptr(residual), ptr(w), ptr(b), ptr(y), rows, d, eps,
                                   ptr(row_idx), stream_ptr(x)), "layernorm")
    return y


# --------------------------------------------------------------- elementwise
def silu_mul(x: torch.Tensor) -> torch.Tensor:
    """x: [..., 2F] = [gate | up] -> silu(gate) * up: [..., F]"""
    if not _gpu(x):
        return ref.silu_mul(x)
    _bf16_contig(x, "x")
    F = x.shape[-1] // 2
    rows = x.numel() // (2 * F)
    out = torch.empty(*x.shape[:-1], F, dtype=x.dtype, device=x.device)
    check(kernels().loqa_silu_mul(ptr(x), ptr(out), rows, F, stream_ptr(x)), "silu_mul")
    return out


def gelu_bias_(x: torch.Tensor, bias: torch.Tensor | None = None,
               pos: torch.Tensor | None = None) -> torch.Tensor:
    """In place: x = gelu(x + bias) [+ pos[row % pos.shape[0]]]."""
    if not _gpu(x):
        return ref.gelu_bias_(x, bias, pos)
    _bf16_contig(x, "x")
    F = x.shape[-1]
    rows = x.numel() // F
    if bias is not None:
        _bf16_contig(bias, "bias"); assert bias.numel() == F
    period = 0
    if pos is not None:
        _bf16_contig(pos, "pos"); assert pos.shape[-1] == F
        period = pos.shape[0]
    check(kernels().loqa_gelu_bias(ptr(x), ptr(bias), ptr(pos), rows, F, period, stream_ptr(x)),
          "gelu_bias")
    return x


def rope_kv_append(qkv: torch.Tensor, positions: torch.Tensor | None, cos_sin: torch.Tensor | None,
                   k_cache: torch.Tensor, v_cache: torch.Tensor, slots: torch.Tensor,
                   n_heads: int, n_kv: int, head_dim: int) -> None:
    """Rotate q (in place in ``qkv``) and k, and append k/v to the paged cache.

    qkv: [T, >= (H + 2 Hkv) * D] bf16; positions/slots: [T] int32;
    cos_sin: [max_pos, D/2, 2] f32 or None (no rotation);
    caches: [n_blocks, Hkv, BLK, D] bf16.
    """
    if not _gpu(qkv):
        return ref.rope_kv_append(qkv, positions, cos_sin, k_cache, v_cache, slots, n_heads, n_kv,
                                  head_dim)
    T = qkv.shape[0]
    if T == 0:
        return None
    assert qkv.dtype == torch.bfloat16 and qkv.stride(-1) == 1
    assert qkv.shape[1] >= (n_heads + 2 * n_kv) * head_dim
    assert slots.dtype == torch.int32 and slots.numel() == T and slots.is_contiguous()
    if cos_sin is not None:
        assert positions is not None and positions.dtype == torch.int32 and positions.numel() == T
        assert cos_sin.dtype == torch.float32 and cos_sin.shape[-2] == head_dim // 2
    assert k_cache.shape[1] == n_kv and k_cache.shape[3] == head_dim and k_cache.is_contiguous()
    blk = k_cache.shape[2]
    check(kernels().loqa_rope_kv_append(ptr(qkv), qkv.stride(0), ptr(positions), ptr(cos_sin),
                                        ptr(k_cache), ptr(v_cache), ptr(slots), T, n_heads, n_kv,
                                        head_dim, blk, stream_ptr(qkv)), "rope_kv_append")
    return None


# ----------------------------------------------------------------- attention
class AttnWorkspace:
    """Split-K partial buffers for grouped decode attention (allocated once per
    engine so the decode step stays graph-capturable)."""

    def __init__(self, device, max_tokens: int, n_heads: int, head_dim: int, max_splits: int):
        self.max_tokens, self.max_splits = max_tokens, max_splits
        self.part_o = torch.empty(max_splits * max_tokens * n_heads * head_dim, dtype=torch.float32,
                                  device=device)
        self.part_ml = torch.empty(max_splits * max_tokens * n_heads * 2, dtype=torch.float32,
                                   device=device)
        # split-arrival tickets of the decode kernel's in-launch combine, one per
        # (sequence, kv head); the last arriving split resets its counter
        self.counters = torch.zeros(max_tokens * n_heads, dtype=torch.int32, device=device)


# decode attention (attn_decode.hip): splits of at least this many keys run on
# 8-wave workgroups (0: always 4 waves)
ATTN8_MIN_KEYS = int(os.environ.get("LOQA_ATTN8_MIN_KEYS", "0"))
# splits of at least this many keys (and more than one tile per wave) prefetch
# a wave's next K / V tile (4 waves: one per SIMD; 0: never)
ATTN_PF_MIN_KEYS = int(os.environ.get("LOQA_ATTN_PF_MIN_KEYS", "0"))


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_q: torch.Tensor, *,
              n_heads: int, n_kv: int, head_dim: int, causal: bool, max_q: int,
              cu_k: torch.Tensor | None = None, ctx_lens: torch.Tensor | None = None,
              block_tables: torch.Tensor | None = None, scale: float | None = None,
              grouped: bool = False, split_keys: int = 256, num_splits: int = 1,
              workspace: AttnWorkspace | None = None, out: torch.Tensor | None = None,
              max_k: int | None = None) -> torch.Tensor:
    """Varlen flash attention.

    q: [Tq, >=H*D] (row stride may exceed H*D, e.g. a view into the fused QKV
    output). K/V: contiguous [Tk, >=Hkv*D] with ``cu_k``, or paged caches
    [n_blocks, Hkv, BLK, D] with ``ctx_lens`` + ``block_tables``.
    Query i of sequence b sits at absolute position ctx_len_b - q_len_b + i.
    Returns [Tq, H*D] bf16.
    """
    scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    if not _gpu(q):
        return ref.attention(q, k, v, cu_q, n_heads=n_heads, n_kv=n_kv, head_dim=head_dim,
                             causal=causal, cu_k=cu_k, ctx_lens=ctx_lens,
                             block_tables=block_tables, scale=scale, out=out)
    Tq = q.shape[0]
    B = cu_q.numel() - 1
    if out is None:
        out = torch.empty(Tq, n_heads * head_dim, dtype=torch.bfloat16, device=q.device)
    if Tq == 0 or B == 0:
        return out
    assert q.dtype == torch.bfloat16 and q.stride(-1) == 1 and q.shape[1] >= n_heads * head_dim
    assert cu_q.dtype == torch.int32 and cu_q.is_contiguous()
    assert out.stride(-1) == 1 and out.shape[0] == Tq
    paged = block_tables is not None
    if paged:
        assert k.dim() == 4 and k.shape[1] == n_kv and k.shape[3] == head_dim and k.is_contiguous()
        assert v.shape == k.shape and v.is_contiguous()
        assert ctx_lens is not None and ctx_lens.dtype == torch.int32 and ctx_lens.numel() == B
        assert block_tables.dtype == torch.int32 and block_tables.is_contiguous()
        assert block_tables.shape[0] == B
        blk, max_blocks, kv_stride = k.shape[2], block_tables.shape[1], 0
        if max_k is not None:
            assert max_k <= max_blocks * blk, "context exceeds block table"
    else:
        assert cu_k is not None and cu_k.dtype == torch.int32
        if ctx_lens is None:
            assert cu_k.numel() == B + 1
        else:  # explicit per-sequence starts (cu_k) and lengths (ctx_lens)
            assert cu_k.numel() >= B and ctx_lens.dtype == torch.int32 and ctx_lens.numel() == B
        assert k.stride(-1) == 1 and v.stride(-1) == 1 and k.stride(0) == v.stride(0)
        blk, max_blocks, kv_stride = 0, 0, k.stride(0)
    part_o = part_ml = None
    if grouped and (n_heads // n_kv) * max_q <= 32 and split_keys % 32 == 0 and \
            (paged or ctx_lens is not None):
        # split-key decode kernel (attn_decode.hip): paged cache, or contiguous
        # rows at per-sequence starts cu_k[b] with lengths ctx_lens[b]
        assert workspace is not None and workspace.max_splits >= num_splits
        assert workspace.max_tokens >= Tq and B * n_kv <= workspace.counters.numel()
        assert not paged or (blk >= 16 and blk & (blk - 1) == 0)
        kv_stride = 0 if paged else k.stride(0)
        # a split of >= ATTN8_MIN_KEYS keys runs on 8 waves (256 keys per
        # pass); with more than 256 keys a wave also prefetches its next tile
        waves = 8 if (ATTN8_MIN_KEYS and split_keys >= ATTN8_MIN_KEYS) else 4
        pf = int(split_keys > 32 * waves and ATTN_PF_MIN_KEYS and split_keys >= ATTN_PF_MIN_KEYS)
        check(kernels().loqa_attn_decode(
            ptr(q), q.stride(0), ptr(k), ptr(v), kv_stride, None if paged else ptr(cu_k),
            ptr(out), out.stride(0), ptr(cu_q), ptr(ctx_lens),
            ptr(block_tables) if paged else None, max_blocks, blk, B, max_q, n_heads, n_kv,
            head_dim, scale, int(causal), split_keys, num_splits, ptr(workspace.part_o),
            ptr(workspace.part_ml), Tq, ptr(workspace.counters), waves, pf, stream_ptr(q)),
            "attn_decode")
        return out
    if grouped:
        G = n_heads // n_kv
        assert max_q * G <= 128, "grouped attention handles at most 128/G query tokens"
        if num_splits > 1:
            assert workspace is not None and workspace.max_splits >= num_splits
            assert workspace.max_tokens >= Tq
            part_o, part_ml = workspace.part_o, workspace.part_ml
    check(kernels().loqa_attention(
        ptr(q), q.stride(0), ptr(k), ptr(v), kv_stride, ptr(out), out.stride(0), ptr(cu_q),
        ptr(cu_k), ptr(ctx_lens), ptr(block_tables), max_blocks, blk, B, max_q, n_heads, n_kv,
        head_dim, scale, int(causal), int(grouped), split_keys, num_splits, ptr(part_o),
        ptr(part_ml), Tq, stream_ptr(q)), "attention")
    return out


# ----------------------------------------------------------------- sampling
ARG_CHUNK = 8192    # tokens per workgroup of the argmax kernel (elementwise.hip)


def _check_token_ids(logits: torch.Tensor, token_ids: torch.Tensor | None) -> None:
    if token_ids is not None:
        assert token_ids.dtype == torch.int32 and token_ids.is_contiguous()
        assert token_ids.numel() >= logits.shape[-1] and token_ids.device == logits.device


def _argmax_args(logits: torch.Tensor, mask, mask_rows, n_float: int, ws_words: int):
    """GPU-side checks and buffers shared by the three argmax ops: the leading
    arguments of their entry points, the int32 [B] result, ``n_float`` float32
    [B] results, and the workspace of a row wider than one chunk (``ws_words``
    int64 per row and chunk; 0: one per row), written before it is read."""
    assert logits.dim() == 2 and logits.stride(-1) == 1
    B, V = logits.shape
    W = 0
    if mask is not None:
        assert mask.dtype == torch.int32 and mask.is_contiguous()
        W = mask.shape[-1]
        assert W * 32 >= V
        if mask_rows is not None:
            assert mask_rows.dtype == torch.int32 and mask_rows.numel() == B
        else:
            assert mask.shape[0] >= B
    is_bf16 = logits.dtype == torch.bfloat16
    assert is_bf16 or logits.dtype == torch.float32
    out = torch.empty(B, dtype=torch.int32, device=logits.device)
    floats = [torch.empty(B, dtype=torch.float32, device=logits.device) for _ in range(n_float)]
    chunks = (V + ARG_CHUNK - 1) // ARG_CHUNK
    ws = torch.empty(B * chunks * ws_words if ws_words else B, dtype=torch.int64,
                     device=logits.device) if chunks > 1 else None
    head = (ptr(logits), int(is_bf16), logits.stride(0), B, V, ptr(mask), ptr(mask_rows), W)
    return head, out, floats, ws


def masked_argmax(logits: torch.Tensor, mask: torch.Tensor | None = None,
                  mask_rows: torch.Tensor | None = None,
                  token_ids: torch.Tensor | None = None) -> torch.Tensor:
    """argmax over tokens allowed by a packed uint32 bitmask (bit v%32 of word
    v//32). ``mask_rows`` optionally maps each logits row to a mask-table row.
    ``token_ids`` (int32 [V], ascending): the columns are a gathered subset of
    the vocabulary (the compact sampling head; ``mask`` is in column order) and
    the result is ``token_ids[column]``. Returns int32 [B] (-1 if nothing is
    allowed)."""
    _check_token_ids(logits, token_ids)
    if not _gpu(logits):
        return ref.masked_argmax(logits, mask, mask_rows, token_ids)
    head, out, _, ws = _argmax_args(logits, mask, mask_rows, 0, 0)
    check(kernels().loqa_masked_argmax(*head, ptr(out), ptr(ws), ptr(token_ids),
                                       stream_ptr(logits)), "masked_argmax")
    return out


def masked_argmax_logprob(logits: torch.Tensor, mask: torch.Tensor | None = None,
                          mask_rows: torch.Tensor | None = None,
                          token_ids: torch.Tensor | None = None
                          ) -> tuple[torch.Tensor, torch.Tensor]:
    """``masked_argmax`` and the log-probability of the token it selects:
    ``x[winner] - logsumexp(x over the allowed tokens)``, the log-softmax after
    the mask, in fp32. Returns (int32 [B], float32 [B]); a row with nothing
    allowed gives (-1, -inf), a row whose only allowed token wins gives 0.0.
    One launch for V <= 8192, else per-chunk partials and a fixed-order merge
    (no memset, no atomics: bitwise repeatable)."""
    _check_token_ids(logits, token_ids)
    if not _gpu(logits):
        return ref.masked_argmax_logprob(logits, mask, mask_rows, token_ids)
    head, out, (lp,), ws = _argmax_args(logits, mask, mask_rows, 1, 2)   # 16-byte records
    check(kernels().loqa_masked_argmax_lse(*head, ptr(out), ptr(lp), ptr(ws), ptr(token_ids),
                                           stream_ptr(logits)), "masked_argmax_lse")
    return out, lp


def masked_argmax_logprob_probe(logits: torch.Tensor, mask: torch.Tensor | None,
                                mask_rows: torch.Tensor | None, probe: torch.Tensor,
                                token_ids: torch.Tensor | None = None
                                ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``masked_argmax_logprob`` (the same two results, bit for bit) plus, per
    row, the log-softmax of one fixed column BEFORE the mask:
    ``x[b, probe[b]] - logsumexp(x[b, :])`` over all columns, in fp32 (Whisper's
    log ``no_speech_prob`` at the start-of-transcript row). ``probe``: int32 [B];
    a row with ``probe[b] < 0`` gives exactly +0.0 and does not pay for the
    second sum, a row of -inf only gives -inf. A column >= V is a ValueError
    when ``probe`` is a host tensor; on the device such a row counts as < 0.
    Returns (int32 [B], float32 [B], float32 [B])."""
    _check_token_ids(logits, token_ids)
    assert logits.dim() == 2 and logits.stride(-1) == 1
    B, V = logits.shape
    assert probe.dtype == torch.int32 and probe.is_contiguous() and probe.numel() == B
    assert probe.device == logits.device
    if probe.device.type == "cpu" and B and int(probe.max()) >= V:
        raise ValueError(f"probe column {int(probe.max())} is outside the {V} logits")
    if not _gpu(logits):
        return ref.masked_argmax_logprob_probe(logits, mask, mask_rows, probe, token_ids)
    head, out, (lp, plp), ws = _argmax_args(logits, mask, mask_rows, 2, 4)   # 32-byte records
    check(kernels().loqa_masked_argmax_lse_probe(
        *head, ptr(probe), ptr(out), ptr(lp), ptr(plp), ptr(ws), ptr(token_ids),
        stream_ptr(logits)), "masked_argmax_lse_probe")
    return out, lp, plp


def masked_argmax_timestamps(logits: torch.Tensor, mask: torch.Tensor | None,
                             mask_rows: torch.Tensor | None, probe: torch.Tensor,
                             ts_ctl: torch.Tensor, ts_state: torch.Tensor, row_slot: torch.Tensor,
                             ts_begin: int, ts_count: int, eot: int, max_initial: int
                             ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``masked_argmax_logprob_probe`` under Whisper's timestamp rules, decided
    on the device (``ops.reference.masked_argmax_timestamps`` has the rules).
    ``ts_ctl`` int32 [B]: 0 = rules off, the row is
    ``masked_argmax_logprob_probe``'s bit for bit; 1 = the window's first
    sampled token; 2 = continue from ``ts_state[row_slot[b]]``. ``ts_state``
    int32 [slots] is read and updated in place by the ruled rows (their slots
    must differ). Timestamp token k is column ``ts_begin + k``, k < ``ts_count``;
    columns below ``eot`` are text; ``max_initial`` (clamped to ``ts_count -
    1``) bounds a window's first timestamp. Returns (int32 [B], float32 [B],
    float32 [B])."""
    assert logits.dim() == 2 and logits.stride(-1) == 1
    B, V = logits.shape
    for t in (probe, ts_ctl, row_slot):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B
        assert t.device == logits.device
    assert ts_state.dtype == torch.int32 and ts_state.is_contiguous() and ts_state.dim() == 1
    assert ts_state.device == logits.device
    if not (0 <= eot <= ts_begin and ts_count >= 1 and ts_begin + ts_count <= V
            and max_initial >= 0):
        raise ValueError(f"timestamp layout eot={eot} ts_begin={ts_begin} ts_count={ts_count} "
                         f"max_initial={max_initial} does not fit {V} logits")
    max_initial = min(int(max_initial), ts_count - 1)
    if probe.device.type == "cpu" and B:
        if int(probe.max()) >= V:
            raise ValueError(f"probe column {int(probe.max())} is outside the {V} logits")
        ruled = row_slot[(ts_ctl == 1) | (ts_ctl == 2)]
        assert ruled.numel() == ruled.unique().numel(), "two ruled rows share a state slot"
        assert not ruled.numel() or (0 <= int(ruled.min()) and int(ruled.max()) < ts_state.numel())
    if not _gpu(logits):
        return ref.masked_argmax_timestamps(logits, mask, mask_rows, probe, ts_ctl, ts_state,
                                            row_slot, ts_begin, ts_count, eot, max_initial)
    head, out, (lp, plp), ws = _argmax_args(logits, mask, mask_rows, 2, 6)   # 48-byte records
    check(kernels().loqa_masked_argmax_ts(
        *head, ptr(probe), ptr(ts_ctl), ptr(ts_state), ptr(row_slot), ts_state.numel(), ts_begin,
        ts_count, eot, max_initial, ptr(out), ptr(lp), ptr(plp), ptr(ws), stream_ptr(logits)),
        "masked_argmax_ts")
    return out, lp, plp


def masked_argmax_sample(logits: torch.Tensor, mask: torch.Tensor | None,
                         mask_rows: torch.Tensor | None, probe: torch.Tensor,
                         ts_ctl: torch.Tensor | None, ts_state: torch.Tensor | None,
                         row_slot: torch.Tensor | None, ts_begin: int, ts_count: int, eot: int,
                         max_initial: int, temp: torch.Tensor, rng: torch.Tensor
                         ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``masked_argmax_timestamps`` with temperature sampling per row, drawn on
    the device. ``temp`` float32 [B], finite and >= 0; ``rng`` int32 [B], the bits
    of each row's uint32 key (``ops.reference.sample_key``). A row with ``temp[b]
    == 0`` is ``masked_argmax_timestamps``'s bit for bit. A row with ``temp[b] >
    0`` draws its token by Gumbel-max over ``logits / temp`` among what the mask
    and the rules leave (the mass rule is applied at temperature 1 first, as
    Whisper filters its logits before sampling) with the counter-based noise
    ``gumbel_noise(rng[b], column)``; its log-probability is at temperature 1.
    ``ts_ctl`` None: every row is rule-off (``ts_state``, ``row_slot`` and the
    layout arguments are ignored) - ``masked_argmax_logprob_probe`` with the
    draw. A bad ``temp`` is a ValueError when it is a host tensor; on the device
    a row whose ``temp`` is not > 0 (NaN included) is greedy. Returns (int32 [B],
    float32 [B], float32 [B])."""
    assert logits.dim() == 2 and logits.stride(-1) == 1
    B, V = logits.shape
    rows = (probe, temp, rng) if ts_ctl is None else (probe, temp, rng, ts_ctl, row_slot)
    for t in rows:
        assert t.is_contiguous() and t.numel() == B and t.device == logits.device
        assert t.dtype == (torch.float32 if t is temp else torch.int32)
    if temp.device.type == "cpu" and B:
        if not bool(torch.isfinite(temp).all()) or float(temp.min()) < 0:
            raise ValueError("temp must be finite and >= 0")
    if probe.device.type == "cpu" and B and int(probe.max()) >= V:
        raise ValueError(f"probe column {int(probe.max())} is outside the {V} logits")
    if ts_ctl is None:
        if not _gpu(logits):
            return ref.masked_argmax_sample(logits, mask, mask_rows, probe, None, None, None, 0, 0,
                                            0, 0, temp, rng)
        slots = 0
    else:
        assert ts_state.dtype == torch.int32 and ts_state.is_contiguous() and ts_state.dim() == 1
        assert ts_state.device == logits.device
        if not (0 <= eot <= ts_begin and ts_count >= 1 and ts_begin + ts_count <= V
                and max_initial >= 0):
            raise ValueError(f"timestamp layout eot={eot} ts_begin={ts_begin} ts_count={ts_count} "
                             f"max_initial={max_initial} does not fit {V} logits")
        max_initial = min(int(max_initial), ts_count - 1)
        if probe.device.type == "cpu" and B:
            ruled = row_slot[(ts_ctl == 1) | (ts_ctl == 2)]
            assert ruled.numel() == ruled.unique().numel(), "two ruled rows share a state slot"
            assert not ruled.numel() or (0 <= int(ruled.min())
                                         and int(ruled.max()) < ts_state.numel())
        if not _gpu(logits):
            return ref.masked_argmax_sample(logits, mask, mask_rows, probe, ts_ctl, ts_state,
                                            row_slot, ts_begin, ts_count, eot, max_initial, temp,
                                            rng)
        slots = ts_state.numel()
    head, out, (lp, plp), ws = _argmax_args(logits, mask, mask_rows, 2, 8)   # 64-byte records
    check(kernels().loqa_masked_argmax_sample(
        *head, ptr(probe), ptr(ts_ctl), ptr(ts_state), ptr(row_slot), slots, ts_begin, ts_count,
        eot, max_initial, ptr(temp), ptr(rng), ptr(out), ptr(lp), ptr(plp), ptr(ws),
        stream_ptr(logits)), "masked_argmax_sample")
    return out, lp, plp


def gumbel_noise(rng: torch.Tensor, V: int) -> torch.Tensor:
    """float32 [B, V]: ``-log(-log(u))`` of ``masked_argmax_sample``'s counter-based
    uniforms for the row keys ``rng`` (int32 [B]) - on the GPU written by the
    device function the sampling kernel draws with."""
    assert rng.dtype == torch.int32 and rng.is_contiguous() and rng.dim() == 1 and V >= 1
    if not _gpu(rng):
        return ref.gumbel_noise(rng, V)
    out = torch.empty(rng.numel(), V, dtype=torch.float32, device=rng.device)
    check(kernels().loqa_gumbel_noise(ptr(rng), rng.numel(), V, ptr(out), stream_ptr(rng)),
          "gumbel_noise")
    return out


# --------------------------------------------------------------- beam search
BEAM_MAX = 8        # widest beam of the kernels (csrc/kernels/beam.hip)


def beam_topk(logits: torch.Tensor, mask: torch.Tensor | None, mask_rows: torch.Tensor | None,
              eot: int, KB: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per logits row the ``KB`` (<= 8) best allowed columns other than ``eot``
    and their log-softmax after the mask, plus EOT's: (``cand_id`` int32
    [R, KB], descending, ties to the lower column, -1 past the allowed count;
    ``cand_lp`` float32 [R, KB]; ``eot_lp`` float32 [R], -inf when masked).
    The sums run over every allowed column, EOT included, in
    ``masked_argmax_logprob``'s order: ``cand_lp[r, 0]`` has that op's bits
    whenever its winner is not EOT. Chunked like it (no memset, no atomics)."""
    if logits.dim() != 2 or logits.stride(-1) != 1:
        raise ValueError("beam_topk: logits must be [R, V] with unit column stride")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"beam_topk: logits must be bfloat16 or float32, got {logits.dtype}")
    R, V = logits.shape
    if not 1 <= int(KB) <= BEAM_MAX:
        raise ValueError(f"beam_topk: KB {KB} is outside 1..{BEAM_MAX}")
    if mask is not None:
        _i32(mask, "beam_topk mask", logits.device)
        if mask.dim() != 2 or mask.shape[-1] * 32 < V:
            raise ValueError("beam_topk: mask must be [rows, >= ceil(V / 32)] packed words")
        if mask_rows is not None:
            _i32(mask_rows, "beam_topk mask_rows", logits.device)
            if mask_rows.numel() != R:
                raise ValueError("beam_topk: one mask row index per logits row")
        elif mask.shape[0] < R:
            raise ValueError("beam_topk: fewer mask rows than logits rows")
    if not _gpu(logits):
        return ref.beam_topk(logits, mask, mask_rows, int(eot), int(KB))
    dev = logits.device
    cand_id = torch.empty(R, KB, dtype=torch.int32, device=dev)
    cand_lp = torch.empty(R, KB, dtype=torch.float32, device=dev)
    eot_lp = torch.empty(R, dtype=torch.float32, device=dev)
    chunks = (V + ARG_CHUNK - 1) // ARG_CHUNK
    ws = None
    if chunks > 1:
        words = kernels().loqa_beam_topk_record_size() // 8
        ws = torch.empty(R * chunks * words, dtype=torch.int64, device=dev)
    check(kernels().loqa_beam_topk(
        ptr(logits), int(logits.dtype == torch.bfloat16), logits.stride(0), R, V, ptr(mask),
        ptr(mask_rows) if mask is not None else None, mask.shape[-1] if mask is not None else 0,
        int(eot), int(KB), ptr(cand_id), ptr(cand_lp), ptr(eot_lp), ptr(ws), stream_ptr(logits)),
        "beam_topk")
    return cand_id, cand_lp, eot_lp


def beam_merge(cand_id: torch.Tensor, cand_lp: torch.Tensor, eot_lp: torch.Tensor,
               cum_in: torch.Tensor, n_src: int):
    """The cross-beam selection of one step, per group g of ``cum_in`` [G, B]
    (2 <= B <= 8): the B best of the ``n_src * B`` candidates of ``beam_topk``
    rows ``g * n_src ..`` (``n_src`` 1 or B) by ``cum_in[g, src] + cand_lp``
    (one f32 add), ranked score first, then the lower source beam, then the
    lower column. Returns (tok, parent, lp, cum_out, eot_score, eot_fin), each
    [G, B] (int32, int32, f32, f32, f32, int32); see ``ref.beam_merge``."""
    if cum_in.dim() != 2 or cum_in.dtype != torch.float32 or not cum_in.is_contiguous():
        raise ValueError("beam_merge: cum_in must be contiguous float32 [G, B]")
    G, B = cum_in.shape
    dev = cum_in.device
    if not 2 <= B <= BEAM_MAX:
        raise ValueError(f"beam_merge: B {B} is outside 2..{BEAM_MAX}")
    if n_src not in (1, B):
        raise ValueError(f"beam_merge: n_src {n_src} must be 1 or B = {B}")
    _i32(cand_id, "beam_merge cand_id", dev)
    for t, name, shape in ((cand_id, "cand_id", (G * n_src, B)), (cand_lp, "cand_lp", (G * n_src, B)),
                           (eot_lp, "eot_lp", (G * n_src,))):
        if tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"beam_merge: {name} must be contiguous {shape} on {dev}")
    if cand_lp.dtype != torch.float32 or eot_lp.dtype != torch.float32:
        raise TypeError("beam_merge: cand_lp and eot_lp must be float32")
    if not _gpu(cum_in):
        return ref.beam_merge(cand_id, cand_lp, eot_lp, cum_in, n_src)
    i = lambda: torch.empty(G, B, dtype=torch.int32, device=dev)
    f = lambda: torch.empty(G, B, dtype=torch.float32, device=dev)
    tok, parent, lp, cum_out, eot_score, eot_fin = i(), i(), f(), f(), f(), i()
    check(kernels().loqa_beam_merge(ptr(cand_id), ptr(cand_lp), ptr(eot_lp), ptr(cum_in), G, n_src,
                                    B, ptr(tok), ptr(parent), ptr(lp), ptr(cum_out),
                                    ptr(eot_score), ptr(eot_fin), stream_ptr(cum_in)), "beam_merge")
    return tok, parent, lp, cum_out, eot_score, eot_fin


def kv_copy_blocks(k: torch.Tensor, v: torch.Tensor, pairs) -> None:
    """Copy paged KV blocks in place: for every (source block, destination
    block) of ``pairs`` (a host list or array [P, 2]) and every layer,
    ``k[:, dst] = k[:, src]`` and the same for ``v`` ([L, blocks, n_kv,
    block_size, D], as ``PagedKVCache``), one launch. No block may be both a
    source and a destination and no destination may repeat: a bad list raises
    ValueError before anything is launched."""
    if k.dim() != 5 or k.shape != v.shape or k.dtype != v.dtype or k.device != v.device:
        raise ValueError("kv_copy_blocks: k and v must be equal [L, blocks, n_kv, block, D] caches")
    if not (k.is_contiguous() and v.is_contiguous()):
        raise ValueError("kv_copy_blocks: k and v must be contiguous")
    if isinstance(pairs, torch.Tensor):
        pairs = pairs.cpu().numpy()
    p = ref.check_copy_pairs(pairs, k.shape[1])
    if not len(p):
        return
    if not _gpu(k):
        return ref.kv_copy_blocks(k, v, p)
    block_bytes = k[0, 0].numel() * k.element_size()
    if block_bytes % 16:
        raise ValueError(f"kv_copy_blocks: a block of {block_bytes} bytes is not 16-byte vectors")
    pd = torch.from_numpy(p).to(k.device)
    check(kernels().loqa_kv_copy_blocks(ptr(k), ptr(v), k.shape[0], k.shape[1], block_bytes,
                                        ptr(pd), len(p), stream_ptr(k)), "kv_copy_blocks")


# ------------------------------------------------------------ hotword biasing
HOTWORD_WG = 64     # workgroup size of hotword_step_kernel (csrc/kernels/hotword.hip)


class HotwordTable:
    """A hotword automaton (``engine.hotwords.HotwordAutomaton``) where
    ``hotword_step`` reads it: on a GPU four int32 buffers (header, ``off``,
    ``tok``, ``dst``) allocated once at the worst case of the limits, so that
    captured graphs hold pointers that ``load`` rewrites in place; on the CPU
    the automaton itself. ``auto`` None or without edges: the step is a no-op."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.auto = None
        self.hdr = self.off = self.tok = self.dst = None
        if self.device.type == "cuda":
            z = lambda n: torch.zeros(n, dtype=torch.int32, device=self.device)
            self.hdr, self.off = z(4), z(ref.HOTWORD_N_CAP + 1)
            self.tok, self.dst = z(ref.HOTWORD_T_CAP), z(ref.HOTWORD_T_CAP)

    def load(self, auto) -> None:
        """Make ``auto`` (None: no phrases) the table's automaton. The device
        buffers are rewritten in place after the device has finished what was
        launched; the caller keeps decoder steps from running meanwhile."""
        if auto is not None and (auto.N > ref.HOTWORD_N_CAP or auto.T > ref.HOTWORD_T_CAP):
            raise ValueError(f"hotword automaton of {auto.N} nodes / {auto.T} table entries exceeds "
                             f"the buffers ({ref.HOTWORD_N_CAP} / {ref.HOTWORD_T_CAP})")
        self.auto = auto
        if self.hdr is None:
            return
        torch.cuda.synchronize(self.device)
        self.hdr.zero_()            # an empty header first: N = T = 0 is the no-op
        if auto is not None and auto.T > 0:
            self.off[: auto.N + 1].copy_(torch.from_numpy(auto.off))
            self.tok[: auto.T].copy_(torch.from_numpy(auto.tok))
            self.dst[: auto.T].copy_(torch.from_numpy(auto.dst))
            self.hdr.copy_(torch.from_numpy(auto.header()))
        torch.cuda.synchronize(self.device)


def hotword_step(logits: torch.Tensor, V: int, hw_ctl: torch.Tensor, row_slot: torch.Tensor,
                 hw_state: torch.Tensor, last_tok: torch.Tensor, table: HotwordTable) -> None:
    """One decoder step of hotword biasing, in place, before the sampler
    (``ops.reference.hotword_step`` has the semantics and is the CPU path).
    ``logits`` [B, >= V] f32 or bf16 with a row stride >= V; per row b with s =
    ``row_slot[b]``: ``hw_ctl[b]`` 0 = untouched bit for bit, state included; 1
    = the window's first freely sampled token, node 0; 2 = node
    ``advance(hw_state[s], last_tok[s])``. The node is stored in ``hw_state[s]``
    and the automaton's boost is added once to every column below ``V`` that
    the node expects. The slots of ruled rows must differ and lie within
    ``hw_state`` / ``last_tok`` (a ValueError when the fields are host tensors;
    on the device a row whose slot is out of range is left alone)."""
    if logits.dim() != 2 or logits.stride(-1) != 1 or not 0 < V <= logits.shape[1] or \
            (logits.shape[0] > 1 and logits.stride(0) < V):
        raise ValueError(f"hotword_step: logits {tuple(logits.shape)} (strides {logits.stride()}) "
                         f"do not hold rows of {V} columns")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"hotword_step: logits must be float32 or bfloat16, got {logits.dtype}")
    B, dev = logits.shape[0], logits.device
    for t, name in ((hw_ctl, "hw_ctl"), (row_slot, "row_slot")):
        _i32(t, name, dev)
        if t.numel() != B:
            raise ValueError(f"hotword_step: {name} has {t.numel()} entries for {B} rows")
    _i32(hw_state, "hw_state", dev)
    _i32(last_tok, "last_tok", dev)
    if table.device.type != dev.type:
        raise ValueError(f"hotword_step: the table is on {table.device}, the logits on {dev}")
    slots = min(hw_state.numel(), last_tok.numel())
    if dev.type == "cpu" and B:
        ruled = row_slot[(hw_ctl == 1) | (hw_ctl == 2)]
        if ruled.numel() != ruled.unique().numel():
            raise ValueError("hotword_step: two ruled rows share a state slot")
        if ruled.numel() and not (0 <= int(ruled.min()) and int(ruled.max()) < slots):
            raise ValueError(f"hotword_step: a ruled row's slot is outside the {slots} slots")
    if not _gpu(logits):
        return ref.hotword_step(logits, V, hw_ctl, row_slot, hw_state, last_tok, table.auto)
    if B == 0:
        return
    check(kernels().loqa_hotword_step(
        ptr(logits), int(logits.dtype == torch.bfloat16), logits.stride(0) if B > 1 else
        max(logits.stride(0), V), B, V, ptr(hw_ctl), ptr(row_slot), ptr(hw_state), ptr(last_tok),
        slots, ptr(table.hdr), ptr(table.off), ptr(table.tok), ptr(table.dst), ref.HOTWORD_N_CAP,
        ref.HOTWORD_T_CAP, stream_ptr(logits)), "hotword_step")


# -------------------------------------------- word timestamps (alignment)
def _i32(t: torch.Tensor, name: str, device) -> None:
    if t.dtype != torch.int32 or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name}: a contiguous int32 tensor on {device}")


def _align_heads(heads, n_layers_given, H: int) -> list:
    heads = [(int(l), int(h)) for l, h in heads]
    if not 1 <= len(heads) <= ref.MAX_ALIGN_HEADS:
        raise ValueError(f"{len(heads)} alignment heads: 1 .. {ref.MAX_ALIGN_HEADS}")
    for l, h in heads:
        if l not in n_layers_given or not 0 <= h < H:
            raise ValueError(f"alignment head {l}:{h}: no such layer buffer / head")
    return heads


def align_record(qs: dict, heads, positions: torch.Tensor, slots: torch.Tensor,
                 cu_q: torch.Tensor, row_slot: torch.Tensor, align_q: torch.Tensor) -> None:
    """Keep a decoder step's cross-attention queries of the alignment heads:
    row r with ``slots[r] >= 0`` copies head (l, h)'s D values of ``qs[l]``
    ([rows, H * D] bf16, the layer's xq output) to ``align_q[row_slot[b], a,
    positions[r]]`` (``align_q`` [slots, A, n_text_ctx, D] bf16), b the sequence
    with ``cu_q[b] <= r < cu_q[b + 1]``. One launch, 16-byte copies, padding rows
    write nothing; a slot or position outside ``align_q`` writes nothing."""
    if align_q.dim() != 4 or align_q.dtype != torch.bfloat16 or not align_q.is_contiguous():
        raise ValueError("align_q: contiguous bf16 [slots, A, n_text_ctx, D]")
    S, A, n_ctx, D = align_q.shape
    dev = align_q.device
    T = slots.numel()
    for name, t in (("positions", positions), ("slots", slots), ("cu_q", cu_q),
                    ("row_slot", row_slot)):
        _i32(t, name, dev)
    B = cu_q.numel() - 1
    if positions.numel() < T or B < 1 or row_slot.numel() < B:
        raise ValueError("align_record: positions / cu_q / row_slot do not cover the step")
    ld = {int(q.stride(0)) for q in qs.values()}
    if len(ld) != 1:
        raise ValueError("align_record: the layers' query buffers differ in row stride")
    ldq = ld.pop()
    H = min(q.shape[1] for q in qs.values()) // D
    heads = _align_heads(heads, qs, H)
    if len(heads) != A:
        raise ValueError(f"align_record: {len(heads)} heads, align_q holds {A}")
    for q in qs.values():
        if q.dtype != torch.bfloat16 or q.stride(1) != 1 or q.shape[0] < T or q.device != dev:
            raise ValueError("align_record: query buffers are bf16 [>= rows, H * D] on the device")
    if D % 8 or ldq % 8:
        raise ValueError("align_record: D and the row stride must be multiples of 8")
    if not _gpu(align_q):
        return ref.align_record(qs, heads, positions, slots, cu_q, row_slot, align_q)
    ptrs = (ctypes.c_void_p * A)(*[qs[l].data_ptr() + h * D * 2 for l, h in heads])
    check(kernels().loqa_align_record(ptrs, A, D, ldq, ptr(positions), ptr(slots), ptr(cu_q),
                                      ptr(row_slot), T, B, ptr(align_q), S, n_ctx,
                                      stream_ptr(align_q)), "align_record")


def align_scores(aq: torch.Tensor, rows: torch.Tensor, xkv, heads, k_row0: int, F: int,
                 scale: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Whisper's alignment weights of one window: ``aq`` [A, n_text_ctx, D] bf16
    (one slot of the query store), ``rows`` int32 [R] (positions in it), ``xkv``
    the layers' cross-attention K|V buffers (K of head h of layer l = columns
    h * D .. of ``xkv[l]``, the window's encoder rows start at ``k_row0``) ->
    P [A, R, F] f32, P[a, r, :] = softmax_f(scale * q . k) over the first ``F``
    frames (``scale`` default 1 / sqrt(D)). bf16 MFMA, f32 softmax; K rows >= F
    and positions outside ``rows`` are not read."""
    if aq.dim() != 3 or aq.dtype != torch.bfloat16 or not aq.is_contiguous():
        raise ValueError("aq: contiguous bf16 [A, n_text_ctx, D]")
    A, n_ctx, D = aq.shape
    dev = aq.device
    _i32(rows, "rows", dev)
    R = rows.numel()
    xkv = dict(enumerate(xkv)) if not isinstance(xkv, dict) else xkv
    heads = _align_heads(heads, xkv, min(k.shape[1] for k in xkv.values()) // D)
    if len(heads) != A:
        raise ValueError(f"align_scores: {len(heads)} heads, aq holds {A}")
    ld = {int(xkv[l].stride(0)) for l, _ in heads}
    if len(ld) != 1:
        raise ValueError("align_scores: the layers' K|V buffers differ in row stride")
    ldk = ld.pop()
    for l, _ in heads:
        k = xkv[l]
        if k.dtype != torch.bfloat16 or k.stride(1) != 1 or k.device != dev or \
                k_row0 < 0 or k_row0 + F > k.shape[0]:
            raise ValueError("align_scores: K|V buffers are bf16 rows on the device holding "
                             "rows k_row0 .. k_row0 + F")
    if R < 1 or F < 1:
        raise ValueError("align_scores: R and F must be >= 1")
    if rows.device.type == "cpu" and (int(rows.min()) < 0 or int(rows.max()) >= n_ctx):
        raise ValueError("align_scores: a row lies outside the query store")
    if D not in (32, 64, 128) or ldk % 8:
        raise ValueError("align_scores: head_dim 32, 64 or 128 and a row stride that is a "
                         "multiple of 8")
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    if not _gpu(aq):
        q = aq[:, rows.long()]
        k = torch.stack([xkv[l][k_row0:k_row0 + F, h * D:(h + 1) * D] for l, h in heads])
        P = ref.align_scores(q, k, scale)
        if out is not None:
            out[: P.numel()].view(P.shape).copy_(P)
        return P
    if out is None:
        out = torch.empty(A * R * F, dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < A * R * F:
        raise ValueError("align_scores: out holds fewer than A * R * F floats")
    ptrs = (ctypes.c_void_p * A)(*[xkv[l].data_ptr() + (k_row0 * ldk + h * D) * 2
                                   for l, h in heads])
    check(kernels().loqa_align_scores(ptr(aq), ptr(rows), R, ptrs, A, D, n_ctx, ldk, F, scale,
                                      ptr(out), stream_ptr(aq)), "align_scores")
    return out.view(-1)[: A * R * F].view(A, R, F)


def align_cost(P: torch.Tensor, n_lead: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """``ref.align_cost``: P [A, R, F] f32 -> the DTW cost [R - n_lead, F] f32
    (rows normalised per head and frame, median filter of width 7 over the
    frames, mean over the heads, negated). Every sum runs in a fixed order:
    repeated launches agree bitwise."""
    if P.dim() != 3 or P.dtype != torch.float32 or not P.is_contiguous():
        raise ValueError("P: contiguous f32 [A, R, F]")
    A, R, F = P.shape
    if not (1 <= A <= ref.MAX_ALIGN_HEADS and 0 <= n_lead < R and F >= 1):
        raise ValueError(f"align_cost: A={A} R={R} F={F} n_lead={n_lead}")
    N = R - n_lead
    if not _gpu(P):
        c = ref.align_cost(P, n_lead)
        if out is not None:
            out.view(-1)[: c.numel()].view(c.shape).copy_(c)
        return c
    if out is None:
        out = torch.empty(N * F, dtype=torch.float32, device=P.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < N * F:
        raise ValueError("align_cost: out holds fewer than N * F floats")
    check(kernels().loqa_align_cost(ptr(P), A, R, F, n_lead, ptr(out), stream_ptr(P)),
          "align_cost")
    return out.view(-1)[: N * F].view(N, F)


DTW_MAX_ROWS = 448


def dtw_workspace(N: int, M: int) -> int:
    """Bytes of trace workspace ``dtw`` needs for an N x M cost."""
    return (N + M - 1) * N


def dtw(x: torch.Tensor, trace: torch.Tensor | None = None,
        tok_frame: torch.Tensor | None = None, total: torch.Tensor | None = None
        ) -> tuple[torch.Tensor, torch.Tensor]:
    """``ref.dtw`` of the cost x [N, M] f32, N <= 448: (tok_frame int32 [N], the
    frame of the first path cell of every row; the total cost f32 [1]), both on
    x's device and bit for bit the reference's. One workgroup walks the
    anti-diagonal wavefront and the path back; ``trace`` (uint8,
    ``dtw_workspace(N, M)`` bytes) holds the trace codes of a large cost."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("dtw: x is a contiguous f32 [N, M]")
    N, M = x.shape
    if not (1 <= N <= DTW_MAX_ROWS and M >= 1):
        raise ValueError(f"dtw: N={N} (1 .. {DTW_MAX_ROWS}), M={M} (>= 1)")
    if not _gpu(x):
        tf, c = ref.dtw(x, return_cost=True)
        return torch.from_numpy(tf), torch.tensor([c], dtype=torch.float32)
    need = dtw_workspace(N, M)
    if trace is None:
        trace = torch.empty(need, dtype=torch.uint8, device=x.device)
    if trace.dtype != torch.uint8 or not trace.is_contiguous() or trace.numel() < need or \
            trace.device != x.device:
        raise ValueError(f"dtw: trace holds fewer than {need} bytes")
    if tok_frame is None:
        tok_frame = torch.empty(N, dtype=torch.int32, device=x.device)
    if total is None:
        total = torch.empty(1, dtype=torch.float32, device=x.device)
    _i32(tok_frame, "tok_frame", x.device)
    if tok_frame.numel() < N or total.dtype != torch.float32 or total.device != x.device:
        raise ValueError("dtw: tok_frame holds fewer than N entries / total is not f32")
    check(kernels().loqa_dtw(ptr(x), N, M, ptr(trace), ptr(tok_frame), ptr(total), stream_ptr(x)),
          "dtw")
    return tok_frame[:N], total


class AlignStore:
    """What an engine keeps for word timestamps: the alignment heads, the
    per-slot query store ``align_q`` [slots, A, n_text_ctx, D] bf16 the decoder
    steps record into, the alignment layers' query buffers of the fused step
    (``qbuf[layer]`` [rows, H * D]) and one window's P / cost / trace workspaces.
    Everything that writes or reads them runs on the engine's one stream."""

    def __init__(self, cfg, heads, n_slots: int, device, max_rows: int = 128):
        self.heads = [(int(l), int(h)) for l, h in heads]
        self.layers = sorted({l for l, _ in self.heads})
        A, D, H = len(self.heads), cfg.head_dim, cfg.n_heads
        self.n_text_ctx, self.n_audio_ctx = cfg.n_text_ctx, cfg.n_audio_ctx
        z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        self.align_q = z(n_slots, A, cfg.n_text_ctx, D)
        self.qbuf = {l: z(max_rows, H * D) for l in self.layers}
        self.P = z(A * cfg.n_text_ctx * cfg.n_audio_ctx, dt=torch.float32)
        self.cost = z(cfg.n_text_ctx * cfg.n_audio_ctx, dt=torch.float32)
        self.trace = z(dtw_workspace(min(cfg.n_text_ctx, DTW_MAX_ROWS), cfg.n_audio_ctx),
                       dt=torch.uint8)
        self.tok_frame = z(cfg.n_text_ctx, dt=torch.int32)
        self.total = z(1, dt=torch.float32)
        self.host = torch.zeros(cfg.n_text_ctx, dtype=torch.int32)
        if torch.device(device).type == "cuda":
            self.host = self.host.pin_memory()

    def record(self, qs: dict, positions, slots, cu_q, row_slot) -> None:
        align_record({l: qs[l] for l in self.layers}, self.heads, positions, slots, cu_q, row_slot,
                     self.align_q)

    def align(self, slot: int, rows: list, xkv, F: int, n_lead: int) -> list:
        """``tok_frame`` (a list of ints) of one window: the three alignment
        launches on the current stream, the result copied to pinned memory and
        waited for."""
        dev = self.align_q.device
        r = torch.tensor(rows, dtype=torch.int32)
        if dev.type == "cuda":
            r = r.pin_memory().to(dev, non_blocking=True)
        P = align_scores(self.align_q[slot], r, xkv, self.heads, slot * self.n_audio_ctx, F,
                         out=self.P)
        cost = align_cost(P, n_lead, out=self.cost)
        tf, _ = dtw(cost, self.trace, self.tok_frame, self.total)
        n = len(rows) - n_lead
        if dev.type != "cuda":
            return [int(v) for v in tf[:n]]
        self.host[:n].copy_(tf[:n], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        return [int(v) for v in self.host[:n]]


# -------------------------------------------------------------------- audio
def pcm16_to_f32_sumsq(pcm: torch.Tensor, offsets: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """pcm: int16 [N] (concatenated segments), offsets: int64 [S+1].
    Returns (f32 samples [N] = x/32767, per-segment sum of squares [S])."""
    if not _gpu(pcm):
        return ref.pcm16_to_f32_sumsq(pcm, offsets)
    assert pcm.dtype == torch.int16 and pcm.is_contiguous()
    assert offsets.dtype == torch.int64 and offsets.is_contiguous()
    S = offsets.numel() - 1
    out = torch.empty(pcm.numel(), dtype=torch.float32, device=pcm.device)
    sumsq = torch.empty(max(S, 1), dtype=torch.float32, device=pcm.device)
    seg = offsets.cpu()
    max_len = int((seg[1:] - seg[:-1]).max()) if S > 0 else 0
    assert int(seg[-1]) <= pcm.numel()
    check(kernels().loqa_pcm16_f32_sumsq(ptr(pcm), ptr(out), ptr(offsets), ptr(sumsq), S, max_len,
                                         stream_ptr(pcm)), "pcm16_f32_sumsq")
    return out, sumsq[:S]


def pcm16_to_f32_padded(pcm: torch.Tensor, offsets: torch.Tensor, ld: int,
                        offsets_host: "np.ndarray | None" = None) -> tuple[torch.Tensor, torch.Tensor]:
    """pcm int16 [N] (S concatenated segments, offsets int64 [S+1]) -> f32
    [S, ld] (x / 32767, zero-padded / truncated to ``ld`` samples) and the
    per-segment sum of squares [S] of the kept samples."""
    S = offsets.numel() - 1
    if not _gpu(pcm):
        return ref.pcm16_to_f32_padded(pcm, offsets, ld)
    assert pcm.dtype == torch.int16 and pcm.is_contiguous()
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.is_cuda
    out = torch.empty(S, ld, dtype=torch.float32, device=pcm.device)
    sumsq = torch.empty(max(S, 1), dtype=torch.float32, device=pcm.device)
    if offsets_host is not None:
        assert int(offsets_host[-1]) <= pcm.numel()
    check(kernels().loqa_pcm16_f32_pad(ptr(pcm), ptr(out), ptr(offsets), ptr(sumsq), S, ld,
                                       stream_ptr(pcm)), "pcm16_f32_pad")
    return out, sumsq[:S]


# sample-rate conversion (csrc/kernels/resample.hip): the rates a relay may
# record at / a reply may be played at
RESAMPLE_RATES = ref.RESAMPLE_RATES
_resample_tables: dict = {}


def resample_filter(rate_in: int, rate_out: int, device="cpu") -> tuple[torch.Tensor, int, int, int]:
    """(f32 table [L, T] on ``device``, L, M, T) of the polyphase filter of
    ``rate_in`` -> ``rate_out``: ``ref.resample_filter``'s fp64 table rounded
    once to f32, kept per (pair, device). An unsupported rate: ValueError."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (rate_in, rate_out, device)
    hit = _resample_tables.get(key)
    if hit is None:
        tab, L, M, T = ref.resample_filter(rate_in, rate_out)
        import numpy as np
        hit = _resample_tables[key] = (torch.from_numpy(tab.astype(np.float32)).to(device), L, M, T)
    return hit


def pcm16_resample_padded(pcm: torch.Tensor, rows, ld: int, rate_out: int = 16000
                          ) -> tuple[torch.Tensor, torch.Tensor]:
    """The resampling sibling of :func:`pcm16_to_f32_padded`, one launch for
    rows of any supported rates. pcm: int16 [N] (concatenated utterances);
    ``rows``: one host tuple (src_first, src_len, out_first, out_len, rate_in)
    per output row - the utterance pcm[src_first : src_first + src_len] at
    ``rate_in`` and the row's slice [out_first, out_first + out_len) of its
    signal resampled to ``rate_out`` (a 30 s window: the filter reads across
    the window boundary, so cutting an utterance into rows equals resampling it
    whole). Returns (f32 [R, ld] = samples / 32767, +0.0 beyond out_len; sum of
    squares [R]). A row already at ``rate_out`` is ``pcm16_to_f32_padded``'s bits."""
    rows = [tuple(int(v) for v in r) for r in rows]
    for r in rows:          # before any launch
        ref.check_rate(r[4])
        n_all = ref.resample_len(r[1], r[4], rate_out)
        if min(r[:4]) < 0 or r[0] + r[1] > pcm.numel() or (r[3] and r[2] + r[3] > n_all):
            raise ValueError(f"resample row {r} outside its utterance ({pcm.numel()} samples, "
                             f"{n_all} outputs)")
    if not _gpu(pcm):
        return ref.pcm16_resample_padded(pcm, rows, ld, rate_out)
    import numpy as np
    assert pcm.dtype == torch.int16 and pcm.is_contiguous()
    R = len(rows)
    out = torch.empty(R, ld, dtype=torch.float32, device=pcm.device)
    sumsq = torch.empty(max(R, 1), dtype=torch.float32, device=pcm.device)
    if R == 0:
        return out, sumsq[:0]
    desc = np.zeros((R, 8), np.int64)
    for i, r in enumerate(rows):
        tab, L, M, T = resample_filter(r[4], rate_out, pcm.device)
        desc[i] = (*r[:4], L, M, T, tab.data_ptr())
    dev = torch.from_numpy(desc).pin_memory().to(pcm.device, non_blocking=True)
    check(kernels().loqa_pcm16_resample_pad(ptr(pcm), ptr(out), ptr(dev), desc.ctypes.data,
                                            ptr(sumsq), R, ld, stream_ptr(pcm)),
          "pcm16_resample_pad")
    return out, sumsq[:R]


def pcm16_resample(pcm: torch.Tensor, lens: torch.Tensor, rate_in: int, rate_out: int
                   ) -> tuple[torch.Tensor, torch.Tensor]:
    """PCM16 rows [B, N] holding ``lens`` [B] samples (int32 / int64, on the
    device: the host never reads them) at ``rate_in`` -> (int16 [B, ceil(N L /
    M)] at ``rate_out``, zero beyond each row's length; int32 lengths [B],
    ceil(len L / M), written by the kernel). Values: the f32 filter sum rounded
    to nearest even, saturated to int16."""
    ref.check_rate(rate_in), ref.check_rate(rate_out)
    assert pcm.dim() == 2 and lens.numel() == pcm.shape[0]
    if not _gpu(pcm):
        return ref.pcm16_resample(pcm, lens, rate_in, rate_out)
    B, N = pcm.shape
    ld_in = pcm.stride(0) if B > 1 else N       # a single row's stride means nothing
    assert pcm.dtype == torch.int16 and (N <= 1 or pcm.stride(1) == 1) and ld_in >= N
    assert lens.dtype in (torch.int32, torch.int64) and lens.is_contiguous() and lens.is_cuda
    tab, L, M, T = resample_filter(rate_in, rate_out, pcm.device)
    ld_out = max(1, -(-N * L // M))
    out = torch.empty(B, ld_out, dtype=torch.int16, device=pcm.device)
    n_out = torch.empty(B, dtype=torch.int32, device=pcm.device)
    check(kernels().loqa_pcm16_resample(ptr(pcm), ld_in, N, ptr(lens),
                                        int(lens.dtype == torch.int64), ptr(out), ld_out,
                                        ptr(n_out), B, L, M, T, ptr(tab), stream_ptr(pcm)),
          "pcm16_resample")
    return out, n_out


# voice activity detection (csrc/kernels/vad.hip)
VadParams = ref.VadParams
vad_params = ref.vad_params


def vad_tile() -> int:
    """Frames per tile of the spans kernel (its workgroup walks longer
    utterances tile by tile)."""
    return int(kernels().loqa_vad_tile())


def vad(pcm: torch.Tensor, descs, params: "ref.VadParams", out=None
        ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Voice activity of the utterances in ``pcm`` (int16 [N], concatenated).
    ``descs``: one host tuple (src_first, src_len, rate, frame_first) per
    utterance - pcm[src_first : src_first + src_len] at ``rate`` (one of
    RESAMPLE_RATES), its 20 ms frames at ``frame_first`` of the frame array.
    ``params``: ``vad_params(...)``. Returns (E int32 [frames]: the frames'
    mean squares, at most 2^30; spans int32 [U, cap, 2]: the speech runs as
    [start, end) frames, cap = F_max // 2 + 1; n_spans int32 [U];
    speech_frames int32 [U]) - the values of ``ref.vad``, bit for bit. Rows of
    ``spans`` beyond ``n_spans`` are not written (-1 on the CPU).

    On the GPU: two launches on the current stream, no host synchronisation;
    the results stay on the device. ``out`` = (E, spans, n_spans,
    speech_frames) to write into. A wrong dtype, a non-contiguous tensor, a
    descriptor outside ``pcm`` or the frame array, an unsupported rate or a
    parameter out of range: ValueError before anything is launched."""
    import numpy as np
    if not isinstance(pcm, torch.Tensor) or pcm.dtype != torch.int16 or pcm.dim() != 1 or \
            not pcm.is_contiguous():
        raise ValueError("vad: pcm must be a contiguous 1-D int16 tensor")
    if not isinstance(params, ref.VadParams):
        raise ValueError("vad: params must be VadParams (ops.vad_params)")
    ref.check_vad_params(params)
    if out is not None:
        if len(out) != 4 or any(not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or
                                not t.is_contiguous() or t.device != pcm.device for t in out):
            raise ValueError("vad: out must be four contiguous int32 tensors on pcm's device")
    descs = ref.vad_check_descs(descs, pcm.numel(), None if out is None else out[0].numel())
    U = len(descs)
    Fs = [ref.vad_frames(n, r) for _, n, r, _ in descs]
    F_max = max(Fs + [0])
    cap = F_max // 2 + 1
    if out is not None:
        sp, ns, sf = out[1], out[2], out[3]
        if sp.dim() != 3 or sp.shape[0] < U or sp.shape[1] < cap or sp.shape[2] != 2 or \
                ns.numel() < U or sf.numel() < U:
            raise ValueError(f"vad: out holds fewer than {U} utterances of {cap} spans")
    if not _gpu(pcm):
        return ref.vad(pcm, descs, params, out)
    dev = pcm.device
    if out is None:
        total = max([d[3] + F for d, F in zip(descs, Fs)] + [0])
        out = (torch.zeros(max(total, 1), dtype=torch.int32, device=dev)[:total],
               torch.empty(max(U, 1), cap, 2, dtype=torch.int32, device=dev)[:U],
               torch.empty(max(U, 1), dtype=torch.int32, device=dev)[:U],
               torch.empty(max(U, 1), dtype=torch.int32, device=dev)[:U])
    if U == 0:
        return out
    E, spans, n_spans, speech = out
    desc = np.asarray(descs, np.int64).reshape(U, 4)
    d_dev = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)
    prm = np.asarray(params.ints(), np.int32)
    ws_words = ref.VAD_WS_WORDS * U * max(F_max, 1)
    ws = torch.empty(ws_words, dtype=torch.int32, device=dev)
    k, st = kernels(), stream_ptr(pcm)
    check(k.loqa_vad_energy(ptr(pcm), pcm.numel(), ptr(d_dev), desc.ctypes.data, U, ptr(E),
                            E.numel(), st), "vad_energy")
    check(k.loqa_vad_spans(ptr(d_dev), desc.ctypes.data, U, ptr(E), E.numel(), prm.ctypes.data,
                           ptr(ws), ws_words, ptr(spans), spans.shape[1], ptr(n_spans),
                           ptr(speech), st), "vad_spans")
    return out


FLAC_BLOCKS = ref.FLAC_BLOCKS


def flac_encode(pcm: torch.Tensor, lens: torch.Tensor, rate: int, block: int = 4096,
                out: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """PCM16 rows [R, N] (inner stride 1, any row stride >= N) holding ``lens``
    [R] samples (int32 / int64, on the device: the host never reads them;
    clamped to [0, N]) at ``rate`` -> (uint8 [R, cap], int32 out_len [R]): row
    b's FLAC stream is out[b, :out_len[b]], nothing is written beyond it. The
    bytes are ``ref.flac_encode``'s (mono, 16 bits, ``block`` samples a frame,
    CONSTANT / VERBATIM / FIXED subframes); cap = 42 + ceil(N / block) (2 block
    + 15). ``out``: a contiguous uint8 [R, cap] to write into (GPU only). Three
    launches (csrc/kernels/flac.hip), no host synchronisation."""
    if pcm.dim() != 2 or pcm.dtype != torch.int16 or lens.numel() != pcm.shape[0]:
        raise ValueError(f"flac_encode wants int16 [R, N] and R lengths, got "
                         f"{tuple(pcm.shape)} {pcm.dtype}, {lens.numel()} lengths")
    R, N = pcm.shape
    frames = ref.flac_check(N, rate, block)          # before any work
    if N > 1 and pcm.stride(1) != 1:
        raise ValueError("flac_encode rows must be contiguous in their samples")
    cap = ref.flac_capacity(N, block)
    if not _gpu(pcm):
        streams = ref.flac_encode(pcm, lens, rate, block)
        out = torch.zeros(R, cap, dtype=torch.uint8)
        for b, st in enumerate(streams):
            out[b, :len(st)] = torch.frombuffer(bytearray(st), dtype=torch.uint8)
        return out, torch.tensor([len(st) for st in streams], dtype=torch.int32)
    ld = pcm.stride(0) if R > 1 else N           # a single row's stride means nothing
    if ld < N:
        raise ValueError(f"flac_encode row stride {ld} < {N} samples")
    assert lens.dtype in (torch.int32, torch.int64) and lens.is_contiguous() and lens.is_cuda
    dev = pcm.device
    if out is None:
        out = torch.empty(R, cap, dtype=torch.uint8, device=dev)
    elif out.shape != (R, cap) or out.dtype != torch.uint8 or not out.is_contiguous() \
            or out.device != dev:
        raise ValueError(f"flac_encode out must be a contiguous uint8 [{R}, {cap}] on {dev}")
    out_len = torch.empty(R, dtype=torch.int32, device=dev)
    staging = torch.empty(R * frames * (2 * block + 16), dtype=torch.uint8, device=dev)
    sizes = torch.empty(2, max(R * frames, 1), dtype=torch.int32, device=dev)   # sizes, offsets
    check(kernels().loqa_flac_encode(ptr(pcm), ld, N, ptr(lens), int(lens.dtype == torch.int64),
                                     R, rate, block, ptr(out), cap, ptr(out_len), ptr(staging),
                                     ptr(sizes[0]), ptr(sizes[1]), stream_ptr(pcm)),
          "flac_encode")
    return out, out_len


def log_mel(audio: torch.Tensor, consts: "ref.MelConstants") -> torch.Tensor:
    """audio [B, n_samples] f32 (padded to 30 s) -> whisper log-mel [B, n_mels, frames] bf16."""
    if not _gpu(audio):
        return ref.log_mel(audio, consts).to(torch.bfloat16)
    assert audio.dtype == torch.float32 and audio.is_contiguous() and audio.dim() == 2
    B, n = audio.shape
    frames = n // 160
    c = consts.to(audio.device)
    work = torch.empty(B, c.n_mels, frames, dtype=torch.float32, device=audio.device)
    gmax = torch.empty(B, dtype=torch.float32, device=audio.device)
    out = torch.empty(B, c.n_mels, frames, dtype=torch.bfloat16, device=audio.device)
    check(kernels().loqa_log_mel(ptr(audio), B, n, ptr(c.window), ptr(c.cos_basis),
                                 ptr(c.sin_basis), ptr(c.filters), c.n_mels, ptr(work), ptr(gmax),
                                 ptr(out), frames, stream_ptr(audio)), "log_mel")
    return out


def im2col_k3(x: torch.Tensor, strides: tuple[int, int, int], B: int, C: int, L: int,
              stride: int) -> torch.Tensor:
    """Unfold a k=3/pad=1 conv1d input. x element (b,c,t) at
    b*strides[0] + c*strides[1] + t*strides[2]. Returns [B*Lout, 3C] bf16."""
    Lout = (L - 1) // stride + 1
    if not _gpu(x):
        return ref.im2col_k3(x, strides, B, C, L, stride)
    assert x.dtype == torch.bfloat16
    cols = torch.empty(B * Lout, 3 * C, dtype=torch.bfloat16, device=x.device)
    check(kernels().loqa_im2col_k3(ptr(x), strides[0], strides[1], strides[2], B, C, L, stride,
                                   ptr(cols), stream_ptr(x)), "im2col_k3")
    return cols


def tensor_seed(seed: int, *key) -> int:
    """uint32 stream id of one weight tensor of a seeded random init (stable
    across processes and Python versions: no ``hash()``)."""
    h = (seed * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    for k in key:
        for ch in str(k).encode():
            h = ((h ^ ch) * 0x01000193) & 0xFFFFFFFF
        h = ((h ^ 0xFF) * 0x01000193) & 0xFFFFFFFF
    return h


def init_normal(rows: int, cols: int, *, seed: int, key: tuple, std: float = 0.02,
                ld: int | None = None, row0: int = 0, col0: int = 0, device="cpu") -> torch.Tensor:
    """Seeded random-init block [rows, cols] bf16 of a conceptual [*, ld] tensor
    at (row0, col0): zero mean, standard deviation ``std`` (Irwin-Hall(4), a
    near-normal with bounded tails). A shard generated on its own holds
    exactly the values of the unsharded tensor, on the GPU and the CPU alike."""
    ld = cols if ld is None else ld
    s = tensor_seed(seed, *key)
    scale = float(torch.tensor(std * math.sqrt(3.0), dtype=torch.float32))
    dev = torch.device(device)
    if dev.type != "cuda":
        return ref.init_uniform4(rows, cols, ld, row0, col0, s, scale).to(dev)
    out = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev)
    check(kernels().loqa_init_uniform4(ptr(out), rows, cols, ld, row0, col0, s, scale,
                                       stream_ptr(out)), "init_uniform4")
    return out


def linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None = None) -> torch.Tensor:
    """Plain GEMM: hipBLASLt via torch on the GPU."""
    return torch.nn.functional.linear(x, w, b)


# ------------------------------------------------- decode GEMM + slab consumers
MPADS = (16, 32, 64, 128)


def mpad_for(m: int) -> int:
    for p in MPADS:
        if m <= p:
            return p
    raise ValueError(f"skinny GEMM supports at most {MPADS[-1]} rows, got {m}")


_SPLITS: dict[tuple[int, int, int], int] = {}
# K must be a multiple of S * 128 (4 waves x 32-wide k-steps); 5 and 10 cover
# Whisper's K = 1280 (= 10 * 128)
SPLIT_CANDIDATES = (1, 2, 4, 5, 8, 10)


def tune_skinny_splits(wp: torch.Tensor, mpads=MPADS, reps: int = 8) -> dict:
    """Time the skinny GEMM for every split-K option on the real weight and
    cache the fastest per (N, K, Mpad). Per-CU bandwidth (~24 GB/s per CU) makes
    grid balance across the 256 CUs the dominant effect, and it depends on the
    shape, so it is measured rather than modelled. Run before graph capture."""
    N, K = wp.shape[0] * 16, wp.shape[1] * 32
    if not _gpu(wp) or NO_TUNE:
        return {}
    out = {}
    tag = _wtag(wp)
    for Mpad in mpads:
        key = (N, K, Mpad) + tag
        if key in _SPLITS:
            out[key] = _SPLITS[key]
            continue
        x = torch.randn(Mpad, K, device=wp.device, dtype=torch.bfloat16)
        best, best_t = 1, float("inf")
        for s in SPLIT_CANDIDATES:
            if K % (s * (256 if tag else 128)):
                continue
            t = graph_time(lambda: skinny_gemm(x, wp, s), reps)
            if t < best_t * 0.98:
                best, best_t = s, t
        _SPLITS[key] = best
        out[key] = best
    return out


_FSPLITS: dict = {}
MAX_DECODE_WGS = int(os.environ.get("LOQA_MAX_DECODE_WGS", "256"))
# LOQA_NO_TUNE=1: skip every split-K / layout measurement and use the
# heuristic defaults (processes sharing one GPU - e.g. a TP rehearsal on a
# 1-GPU box - cannot time anything meaningful, and the timing dominates start-up)
NO_TUNE = os.environ.get("LOQA_NO_TUNE", "0") == "1"
# fused-GEMM decode steps: embedding + layer-0 row statistics in one launch and
# the final norm gathering its logit rows itself (False: the unfused torch ops)
FUSED_EMBED = True
_CAP = [MAX_DECODE_WGS]   # active co-scheduling cap while tuning (see decode_cap)


class decode_cap:
    """Context: tune decode GEMMs for a grid of at most ``n`` workgroups (an
    engine confined to n CUs by a CU mask gets n; default MAX_DECODE_WGS)."""

    def __init__(self, n: int | None):
        self.n = n or MAX_DECODE_WGS

    def __enter__(self):
        self.prev = _CAP[0]
        _CAP[0] = self.n
        return self

    def __exit__(self, *exc):
        _CAP[0] = self.prev


def _fsplit_override(key: tuple) -> tuple[int, int, int] | None:
    """``LOQA_FSPLIT_OVERRIDE="silu:28672x4096:M16=2,2,1;..."`` pins the
    (split-K, rt, wr) of a fused GEMM shape (experiments / deployment pins)."""
    spec = os.environ.get("LOQA_FSPLIT_OVERRIDE", "")
    name = f"{key[0]}:{key[1]}x{key[2]}:M{key[3]}" + "".join(f":{t}" for t in key[4:])
    for item in spec.split(";"):
        if "=" in item:
            k, v = item.split("=", 1)
            if k.strip() == name:
                return tuple(int(t) for t in v.split(","))
    return None


class contended_tuning:
    """Context: while tuning, keep a Llama-3-8B-like gate|up weight stream
    (rows-per-wave fused GEMM over ~700 MB of cold weights) running on a
    background stream. The Whisper decoder always runs beside the LLM decode;
    its kernels' best split-K / tile shape under that load differs from the
    isolated optimum (split-K hand-offs cost extra memory round trips that
    queue behind the co-resident weight stream)."""

    def __init__(self, device, enabled: bool = True):
        self.device, self.enabled = torch.device(device), enabled

    def __enter__(self):
        if not (self.enabled and self.device.type == "cuda"):
            return self
        import threading
        dev = self.device
        bf = dict(dtype=torch.bfloat16, device=dev)
        self._ws = [shuffle_weight(torch.randn(28672, 4096, **bf) * 0.02) for _ in range(3)]
        self._x = torch.randn(16, 4096, **bf)
        self._scr = FusedScratch(dev)
        self._scr.rowsq[: 128 * 16].fill_(32.0)
        self._stop = threading.Event()
        self._stream = torch.cuda.Stream(dev)
        ready = threading.Event()

        # the background work is one captured graph, replayed and paced by
        # event polling: no synchronising HIP call while the tuner captures
        with torch.cuda.stream(self._stream):
            for i in range(3):
                skinny_fused(self._x, self._ws[i], "silu", self._scr, splits=1, rt=2, wr=4, norm=True,
                             rowsq_tiles=128)
        self._stream.synchronize()
        self._g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g, stream=self._stream):
            for i in range(12):
                skinny_fused(self._x, self._ws[i % 3], "silu", self._scr, splits=1, rt=2, wr=4,
                             norm=True, rowsq_tiles=128)

        def loop():
            import time as _time
            torch.cuda.set_device(dev)
            with torch.cuda.stream(self._stream):
                while not self._stop.is_set():
                    self._g.replay()
                    ev = torch.cuda.Event()
                    ev.record(self._stream)
                    while not ev.query():
                        _time.sleep(0.0002)
                    ready.set()
        self._th = threading.Thread(target=loop, daemon=True)
        self._th.start()
        ready.wait(30)
        return self

    def __exit__(self, *exc):
        if getattr(self, "_th", None) is not None:
            self._stop.set()
            self._th.join()
            torch.cuda.synchronize(self.device)
            del self._g, self._ws, self._x, self._scr
            self._th = None


def tune_fused_splits(key: tuple, run, K: int, reps: int = 8, rts=(2,), ncopies: int = 1,
                      wr4: bool = False, fewest: bool = True, xl: str = "no") -> tuple:
    """(split-K, tile rows / 16, waves along rows) for a fused-epilogue GEMM,
    measured: ``run(s, rt, wr, i)`` launches it on weight copy ``i`` (the graph
    cycles through ``ncopies`` copies so every call streams COLD weights, as a
    decode step that reads the whole model does; a warm replay of one copy is
    partly served by the 256 MB Infinity Cache and ranks the options wrongly).
    The in-launch reduce adds a store-drain + ticket round trip to every
    workgroup's tail, so the best split is lower than the plain GEMM's; 16-row
    tiles (rt=1, residual / act epilogues only) double the workgroups without
    any reduction; ``wr4`` adds the 4-waves-along-rows layout (S = 1 only). ``xl``: "no",
    "also" (add the x-through-LDS layouts, any split) or "only" (Mpad 128).
    Returns (split-K, rt, wr) or (split-K, rt, 4, 1) for an XL layout.
    ``key`` = (mode, N, K, Mpad), with "fp8" appended for an fp8 weight stream
    (a wave's k range is then a whole number of 64-wide k-step pairs) or
    "mxfp4" for an MXFP4 one (of 128-wide loads: K % (S * waves-along-K * 128) == 0)."""
    if key in _FSPLITS:
        return _FSPLITS[key]
    ov = _fsplit_override(key)
    if ov is not None:
        _FSPLITS[key] = ov
        return ov
    N = key[1]
    kq = _KGRANULE[tuple(key[4:])]       # k granule of one weight load
    cands = [] if xl == "only" else \
        [(s, rt, 1) for rt in rts for s in SPLIT_CANDIDATES if K % (s * 4 * kq) == 0]
    # (MXFP4 at K < 512, where no split of the 4-waves-along-K form holds whole
    # loads, has the rows-per-wave layouts only)
    if (wr4 or (kq == 128 and not cands)) and xl != "only":
        cands += [(1, rt, 4) for rt in rts if N % (64 * rt) == 0 and K % kq == 0]
    if xl != "no":
        cands += [(s, rt, 4, 1) for rt in (1, 2) for s in SPLIT_CANDIDATES
                  if K % (s * 128) == 0 and N % (64 * rt) == 0]   # >= every format's granule
    # co-scheduling cap: the STT and LLM decoders run concurrently on their own
    # streams; a grid that fills every CU slot makes the other stream's small
    # latency-bound kernels wait for it to drain (measured: a 768-workgroup
    # qkv GEMM, fastest in isolation, slowed the concurrent Whisper decoder 5x
    # and the whole pipeline 1.8x). Keep at most one workgroup per CU.
    units = {c: (N // (16 * c[1] * c[2])) * c[0] for c in cands}
    capped = [c for c in cands if units[c] <= _CAP[0]]
    if not capped and fewest:
        # a GEMM too large for any layout under the cap (Llama-3-70B gate|up:
        # >= 448 workgroups) takes the fewest-workgroup layouts (measured cold,
        # 70B gate|up: 448 WGs 154 us vs 3584 WGs 169 us)
        least = min(units.values())
        capped = [c for c in cands if units[c] <= max(_CAP[0], 2 * least)]
    elif not capped:
        # Llama-3-8B gate|up at Mpad 64 (jump-forward decode steps beside the
        # Whisper decoder): the short-lived 16-row tiles. Measured in the
        # pipeline: 18.9 utt/s, vs 17.2 for 896 longer 32-row workgroups
        # (fastest alone) and 11.0 for 224 4-wave 32-row workgroups.
        capped = cands[:1]
    cands = capped
    best, best_t = cands[0] if xl == "only" else (1, rts[-1], 1), float("inf")
    n = max(1, ncopies)
    for c in cands:
        it = iter(range(1 << 30))
        t = graph_time(lambda: run(*c[:3], next(it) % n, *c[3:]), max(reps, 2 * n))
        if t < best_t * 0.98:
            best, best_t = c, t
    _FSPLITS[key] = best
    return best


_TUNE_STREAM: dict = {}


def _tune_stream() -> "torch.cuda.Stream":
    """One side stream per device for every tuning capture. ``torch.cuda.Stream()``
    and ``torch.cuda.graph()`` without a stream take the NEXT stream of
    PyTorch's round-robin pool, and pool streams land on the process's few HIP
    hardware queues in creation order: a tuner that drew one pool stream per
    candidate left the decoder streams created after it on queues that
    depended on how many layouts were timed (see docs/PERF.md, the cliff)."""
    d = torch.cuda.current_device()
    if d not in _TUNE_STREAM:
        _TUNE_STREAM[d] = torch.cuda.Stream()
    return _TUNE_STREAM[d]


def graph_time(fn, reps: int = 8, trials: int = 3) -> float:
    """Device time (ms) of ``reps`` back-to-back calls of ``fn`` replayed from
    a captured HIP graph (no host launch overhead in the measurement: a few-µs
    kernel is otherwise hidden behind its own launch cost); min over trials."""
    # A new pool stream per call, on purpose: the stream-pool cursor this
    # leaves behind decides which hardware queues the decoder streams created
    # later land on, and the measured-best placement (18.7-19.2 utt/s) is the
    # one this produces. A fixed tuning stream (``_tune_stream``) measured
    # 17.3 (docs/PERF.md, "the 1.8x cliff").
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    del g
    return best


def choose_splits(N: int, K: int, Mpad: int, target_wgs: int = 512, tag: tuple = ()) -> int:
    """Split-K factor: the tuned value if available, else enough splits for
    >= ~2 workgroups per CU (256 CUs). ``tag`` = ("fp8",) for an fp8 weight,
    ("mxfp4",) for an MXFP4 one (the 4 waves along K each take whole loads)."""
    tuned = _SPLITS.get((N, K, Mpad) + tag)
    if tuned is not None:
        return tuned
    rt = 2 if Mpad <= 32 else 4
    tiles = max(1, N // (16 * rt))
    best = 1
    for s in SPLIT_CANDIDATES:
        if K % (s * 4 * _KGRANULE[tag]) != 0:
            continue
        best = s
        if tiles * s >= target_wgs:
            break
    return best


def decode_attn_splits(max_ctx: int, units: int, split_keys: int = 128,
                       max_wgs: int | None = None) -> tuple[int, int]:
    """(num_splits, split_keys) of the split-key decode attention for a
    context bound and ``units`` = sequences x kv heads workgroup rows: splits of
    ``split_keys`` keys, but at most ``max_wgs`` workgroups in all (the
    co-scheduling cap of ``tune_fused_splits``) - longer splits then loop."""
    max_wgs = MAX_DECODE_WGS if max_wgs is None else max_wgs
    ns = max(1, -(-max_ctx // split_keys))
    cap = max(1, max_wgs // max(1, units))
    if ns > cap:
        ns = cap
        split_keys = -(-(-(-max_ctx // ns)) // 32) * 32
    return ns, split_keys


def shuffle_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] bf16 -> MFMA-fragment-ordered [N/16, K/32, 64, 8] (skinny GEMM layout)."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0
    if not _gpu(w):
        return ref.shuffle_weight(w)
    _bf16_contig(w, "w")
    out = torch.empty(N // 16, K // 32, 64, 8, dtype=torch.bfloat16, device=w.device)
    check(kernels().loqa_shuffle_weight(ptr(w), ptr(out), N, K, stream_ptr(w)), "shuffle_weight")
    return out


class Fp8Weight:
    """A decode GEMM weight as an fp8 (OCP e4m3fn) stream: ``wp`` uint8
    [N/16, K/64, 64, 16] in the kernels' fp8 fragment order (``ref.shuffle_fp8``)
    and ``scale`` f32 [N], one per row (in the row order of ``wp``). Stands in
    for a shuffled bf16 weight wherever the decode GEMMs take one: ``shape`` is
    the shape of that bf16 tensor, so ``shape[0] * 16`` / ``shape[1] * 32``
    give N and K as they do for it."""

    def __init__(self, wp: torch.Tensor, scale: torch.Tensor, N: int, K: int):
        assert wp.dtype == torch.uint8 and wp.shape == (N // 16, K // 64, 64, 16)
        assert scale.dtype == torch.float32 and scale.shape == (N,)
        self.wp, self.scale, self.N, self.K = wp, scale, N, K

    shape = property(lambda self: (self.N // 16, self.K // 32, 64, 8))
    device = property(lambda self: self.wp.device)
    is_cuda = property(lambda self: self.wp.is_cuda)
    nbytes = property(lambda self: self.wp.numel() + 4 * self.scale.numel())

    def numel(self) -> int:
        return self.wp.numel()

    def element_size(self) -> int:
        return 1

    def clone(self) -> "Fp8Weight":
        return Fp8Weight(self.wp.clone(), self.scale.clone(), self.N, self.K)

    def to(self, device) -> "Fp8Weight":
        return Fp8Weight(self.wp.to(device), self.scale.to(device), self.N, self.K)


class Mxfp4Weight:
    """A fused decode GEMM weight as an OCP MXFP4 stream: ``wp`` uint8
    [N/16, K/128, 64, 16], e2m1 nibbles in the kernels' fragment order, and
    ``scales`` uint8 [N/16, K/128, 16, 4], one e8m0 byte per row and block of
    32 k values (``ref.shuffle_mxfp4``). 4.25 bits per weight. Stands in for a
    shuffled bf16 weight wherever the fused decode GEMMs take one (``shape`` as
    for ``Fp8Weight``); the plain ``skinny_gemm`` has no MXFP4 form."""

    def __init__(self, wp: torch.Tensor, scales: torch.Tensor, N: int, K: int):
        assert wp.dtype == torch.uint8 and wp.shape == (N // 16, K // 128, 64, 16)
        assert scales.dtype == torch.uint8 and scales.shape == (N // 16, K // 128, 16, 4)
        self.wp, self.scales, self.N, self.K = wp, scales, N, K

    shape = property(lambda self: (self.N // 16, self.K // 32, 64, 8))
    device = property(lambda self: self.wp.device)
    is_cuda = property(lambda self: self.wp.is_cuda)
    nbytes = property(lambda self: self.wp.numel() + self.scales.numel())

    def numel(self) -> int:
        return self.wp.numel() + self.scales.numel()

    def element_size(self) -> int:
        return 1

    def clone(self) -> "Mxfp4Weight":
        return Mxfp4Weight(self.wp.clone(), self.scales.clone(), self.N, self.K)

    def to(self, device) -> "Mxfp4Weight":
        return Mxfp4Weight(self.wp.to(device), self.scales.to(device), self.N, self.K)


# k values per 16-byte lane load of a weight stream: a wave's k range is a
# whole number of them
_KGRANULE = {(): 32, ("fp8",): 64, ("mxfp4",): 128}


def _wtag(wp) -> tuple:
    """Suffix of the tuning-cache keys of a weight: () for bf16 (the keys are
    what they always were), ("fp8",) for an fp8 stream, ("mxfp4",) for MXFP4."""
    if isinstance(wp, Mxfp4Weight):
        return ("mxfp4",)
    return ("fp8",) if isinstance(wp, Fp8Weight) else ()


def quantize_weight_mxfp4(w: torch.Tensor) -> Mxfp4Weight:
    """[N, K] bf16 (rows already norm-folded and permuted) -> ``Mxfp4Weight``:
    per block of 32 k values the smallest power-of-two scale that clips
    nothing, e2m1 codes rounded to nearest even (``ref.quantize_mxfp4_rows``),
    in fragment order. Load time only."""
    N, K = w.shape
    assert N % 16 == 0 and K % 128 == 0, "MXFP4 weights need N % 16 == 0 and K % 128 == 0"
    code, scales = ref.quantize_mxfp4_rows(w)
    return Mxfp4Weight(*ref.shuffle_mxfp4(code, scales), N, K)


def quantize_weight_fp8(w: torch.Tensor) -> Fp8Weight:
    """[N, K] bf16 (rows already norm-folded and permuted) -> ``Fp8Weight``:
    per-row scale amax / 448 (1 for an all-zero row, whose outputs are then
    exactly 0), e4m3fn bytes in fragment order. Load time only."""
    N, K = w.shape
    assert N % 16 == 0 and K % 64 == 0, "fp8 weights need N % 16 == 0 and K % 64 == 0"
    q, scale = ref.quantize_fp8_rows(w)
    return Fp8Weight(ref.shuffle_fp8(q.view(torch.uint8)), scale.contiguous(), N, K)


def skinny_gemm(x: torch.Tensor, wp, splits: int | None = None,
                max_wgs: int = 0) -> torch.Tensor:
    """x [Mpad, K] bf16 (Mpad in 16/32/64/128, padded rows finite) @ W^T with W
    given pre-shuffled (``shuffle_weight``, or an ``Fp8Weight``) -> split-K
    partial slabs [S, Mpad, N] f32 (sum over S = x @ W^T)."""
    Mpad, K = x.shape
    N = wp.shape[0] * 16
    assert wp.shape[1] * 32 == K, "weight/activation K mismatch"
    S = splits or choose_splits(N, K, Mpad, tag=_wtag(wp))
    if not _gpu(x):
        return ref.skinny_gemm(x, wp, S)
    assert Mpad in MPADS and x.dtype == torch.bfloat16 and x.stride(1) == 1
    if isinstance(wp, Mxfp4Weight):
        raise TypeError("skinny_gemm has no MXFP4 kernel (fused decode GEMMs only)")
    part = torch.empty(S, Mpad, N, dtype=torch.float32, device=x.device)
    if isinstance(wp, Fp8Weight):
        assert wp.is_cuda and wp.wp.is_contiguous() and wp.scale.is_contiguous()
        check(kernels().loqa_skinny_gemm_fp8(ptr(x), x.stride(0), ptr(wp.wp), ptr(wp.scale),
                                             ptr(part), Mpad, N, K, S, max_wgs, stream_ptr(x)),
              "skinny_gemm_fp8")
        return part
    _bf16_contig(wp, "wp")
    check(kernels().loqa_skinny_gemm(ptr(x), x.stride(0), ptr(wp), ptr(part), Mpad, N, K, S,
                                     max_wgs, stream_ptr(x)), "skinny_gemm")
    return part


def slab_rmsnorm(part: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                 row_idx: torch.Tensor | None = None, write_residual: bool = True) -> torch.Tensor:
    """residual[src] += sum_s part[s, src]; y[i] = rmsnorm(residual[src]) * w with
    src = row_idx[i] (or i). Returns y [rows, d] bf16."""
    S, Mpad, d = part.shape
    rows = row_idx.numel() if row_idx is not None else Mpad
    if not _gpu(part):
        return ref.slab_rmsnorm(part, residual, w, eps, row_idx, write_residual)
    assert part.dtype == torch.float32 and part.is_contiguous()
    _bf16_contig(residual, "residual")
    assert residual.shape[-1] == d and residual.shape[0] >= Mpad
    if row_idx is not None:
        assert row_idx.dtype == torch.int64 and row_idx.is_contiguous()
    y = torch.empty(rows, d, dtype=torch.bfloat16, device=part.device)
    check(kernels().loqa_slab_rmsnorm(ptr(part), S, Mpad, ptr(row_idx), rows, ptr(residual),
                                      int(write_residual), ptr(w), ptr(y), d, eps,
                                      stream_ptr(part)), "slab_rmsnorm")
    return y


def slab_rope_append(part: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor | None,
                     k_cache: torch.Tensor, v_cache: torch.Tensor, slots: torch.Tensor,
                     n_heads: int, n_kv: int, head_dim: int,
                     bias: torch.Tensor | None = None) -> torch.Tensor:
    """qkv slabs [S, Mpad, (H+2Hkv)D] (+ optional projection bias) -> rotated q
    [Mpad, H*D] bf16; k/v to cache (``cos_sin`` None = no rotary embedding)."""
    S, Mpad, N = part.shape
    assert N == (n_heads + 2 * n_kv) * head_dim
    if not _gpu(part):
        return ref.slab_rope_append(part, positions, cos_sin, k_cache, v_cache, slots, n_heads,
                                    n_kv, head_dim, bias)
    assert slots.dtype == torch.int32 and slots.numel() == Mpad
    assert positions.dtype == torch.int32 and positions.numel() == Mpad
    assert k_cache.is_contiguous() and k_cache.shape[1] == n_kv and k_cache.shape[3] == head_dim
    q = torch.empty(Mpad, n_heads * head_dim, dtype=torch.bfloat16, device=part.device)
    check(kernels().loqa_slab_rope_append(ptr(part), S, Mpad, Mpad, ptr(positions), ptr(cos_sin),
                                          ptr(q), ptr(k_cache), ptr(v_cache), ptr(slots), n_heads,
                                          n_kv, head_dim, k_cache.shape[2], ptr(bias),
                                          stream_ptr(part)),
          "slab_rope_append")
    return q


def slab_layernorm(part: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
                   eps: float, bias: torch.Tensor | None = None,
                   row_idx: torch.Tensor | None = None, write_residual: bool = True,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """residual[src] += bf16(sum_s part[s, src] + bias); y[i] = layernorm(residual[src])."""
    S, Mpad, d = part.shape
    rows = row_idx.numel() if row_idx is not None else Mpad
    if not _gpu(part):
        return ref.slab_layernorm(part, residual, w, b, eps, bias, row_idx, write_residual)
    assert part.dtype == torch.float32 and part.is_contiguous()
    _bf16_contig(residual, "residual")
    assert residual.shape[-1] == d and residual.shape[0] >= Mpad
    if row_idx is not None:
        assert row_idx.dtype == torch.int64 and row_idx.is_contiguous()
    if bias is not None:
        _bf16_contig(bias, "bias")
        assert bias.numel() == d
    y = out if out is not None else torch.empty(rows, d, dtype=torch.bfloat16, device=part.device)
    check(kernels().loqa_slab_layernorm(ptr(part), S, Mpad, ptr(row_idx), rows, ptr(bias),
                                        ptr(residual), int(write_residual), ptr(w), ptr(b), ptr(y),
                                        d, eps, stream_ptr(part)), "slab_layernorm")
    return y


def slab_bias_act(part: torch.Tensor, bias: torch.Tensor | None, act: str = "none") -> torch.Tensor:
    """bf16(act(sum_s part + bias)) [Mpad, N]; act in {"none", "gelu"}."""
    S, Mpad, N = part.shape
    a = {"none": 0, "gelu": 1}[act]
    if not _gpu(part):
        return ref.slab_bias_act(part, bias, act)
    if bias is not None:
        _bf16_contig(bias, "bias")
        assert bias.numel() == N
    out = torch.empty(Mpad, N, dtype=torch.bfloat16, device=part.device)
    check(kernels().loqa_slab_bias_act(ptr(part), S, Mpad, Mpad, N, ptr(bias), a, ptr(out),
                                       stream_ptr(part)), "slab_bias_act")
    return out


def embed_pos(tokens: torch.Tensor, positions: torch.Tensor, tok_embed: torch.Tensor,
              pos_embed: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16(tok_embed[tokens] + pos_embed[positions]) [rows, d]."""
    rows, d = tokens.numel(), tok_embed.shape[1]
    if not _gpu(tok_embed):
        # a negative id (a padding row) reads row 0, as the kernel does
        return (tok_embed[tokens.long().clamp(min=0)].float()
                + pos_embed[positions.long()].float()).to(torch.bfloat16)
    assert tokens.dtype == torch.int32 and positions.dtype == torch.int32
    out = out if out is not None else torch.empty(rows, d, dtype=torch.bfloat16,
                                                  device=tok_embed.device)
    check(kernels().loqa_embed_pos(ptr(tokens), ptr(positions), ptr(tok_embed), ptr(pos_embed),
                                   ptr(out), rows, d, stream_ptr(tok_embed)), "embed_pos")
    return out


def embed_stats(tokens: torch.Tensor, tok_embed: torch.Tensor, scratch: "FusedScratch",
                positions: torch.Tensor | None = None, pos_embed: torch.Tensor | None = None,
                sums: bool = False) -> torch.Tensor:
    """Decode-step input of the fused-GEMM path in one launch: the embedded rows
    tok_embed[tokens] (+ pos_embed[positions]) [rows, d] bf16, with their row
    sums of squares (and sums) written to ``scratch`` as ONE partial tile for
    layer 0's norm prologue (what ``scratch.seed_stats`` computes)."""
    rows, d = tokens.numel(), tok_embed.shape[1]
    if not _gpu(tok_embed):
        x = tok_embed[tokens.long().clamp(min=0)]
        if pos_embed is not None:
            x = (x.float() + pos_embed[positions.long()].float()).to(torch.bfloat16)
        scratch.seed_stats(x, sums=sums)
        return x
    assert tokens.dtype == torch.int32 and tokens.is_contiguous()
    _bf16_contig(tok_embed, "tok_embed")
    if pos_embed is not None:
        assert positions is not None and positions.dtype == torch.int32
        assert positions.numel() == rows and positions.is_contiguous()
        _bf16_contig(pos_embed, "pos_embed")
        assert pos_embed.shape[1] == d
    assert rows <= scratch.rowsq.numel()
    out = torch.empty(rows, d, dtype=torch.bfloat16, device=tok_embed.device)
    check(kernels().loqa_embed_stats(ptr(tokens), ptr(positions if pos_embed is not None else None),
                                     ptr(tok_embed), ptr(pos_embed), ptr(out), ptr(scratch.rowsq),
                                     ptr(scratch.rowsum) if sums else None, rows, d,
                                     stream_ptr(tok_embed)), "embed_stats")
    scratch.stat_tiles = 1
    return out


def slab_silu_mul(part: torch.Tensor) -> torch.Tensor:
    S, Mpad, F2 = part.shape
    F = F2 // 2
    if not _gpu(part):
        return ref.slab_silu_mul(part)
    out = torch.empty(Mpad, F, dtype=torch.bfloat16, device=part.device)
    check(kernels().loqa_slab_silu_mul(ptr(part), S, Mpad, Mpad, F, ptr(out), stream_ptr(part)),
          "slab_silu_mul")
    return out


def slab_reduce(part: torch.Tensor) -> torch.Tensor:
    S, Mpad, N = part.shape
    if S == 1:
        return part[0]
    if not _gpu(part):
        return part.sum(0)
    out = torch.empty(Mpad, N, dtype=torch.float32, device=part.device)
    check(kernels().loqa_slab_reduce(ptr(part), S, Mpad, Mpad, N, ptr(out), stream_ptr(part)),
          "slab_reduce")
    return out


# ------------------------------------------------------------- VITS / HiFi-GAN
class ConvWeight:
    """A conv1d weight prepared for the MFMA implicit-GEMM kernel: [Cout_pad, K,
    Cin] bf16 (Cout padded to 32; gated convs interleave the tanh / sigmoid
    halves in 16-channel blocks). Keeps the torch-layout copy for the CPU path."""

    def __init__(self, w: torch.Tensor, bias: torch.Tensor | None = None, gated: bool = False):
        self.w, self.bias, self.gated = w, bias, gated      # w [Cout, Cin, K]
        Cout, Cin, K = w.shape
        self.Cout, self.Cin, self.K = Cout, Cin, K
        assert Cin % 16 == 0, "input channels must be a multiple of 16"
        perm = torch.arange(Cout, device=w.device)
        if gated:
            Hh = Cout // 2
            assert Hh % 16 == 0
            blocks = []
            for q in range(Hh // 16):
                blocks += [torch.arange(16 * q, 16 * q + 16), torch.arange(Hh + 16 * q, Hh + 16 * q + 16)]
            perm = torch.cat(blocks).to(w.device)
        cpad = (Cout + 31) // 32 * 32
        wp = torch.zeros(cpad, K, Cin, dtype=torch.bfloat16, device=w.device)
        wp[:Cout] = w[perm].permute(0, 2, 1).to(torch.bfloat16)
        self.wp = wp.contiguous()
        self.bp = None
        if bias is not None:
            bp = torch.zeros(cpad, dtype=torch.bfloat16, device=w.device)
            bp[:Cout] = bias[perm].to(torch.bfloat16)
            self.bp = bp
        self.cpad = cpad

    @property
    def out_channels(self) -> int:
        return self.Cout // 2 if self.gated else self.Cout


def conv1d(x: torch.Tensor, cw: ConvWeight, *, dil: int = 1, pad: int | None = None,
           stride: int = 1, pre_slope: float | None = None, act: str | None = None,
           res: torch.Tensor | None = None, alpha: float = 1.0, acc: torch.Tensor | None = None,
           lens: torch.Tensor | None = None, out: torch.Tensor | None = None,
           pcm16: bool = False, Tout: int | None = None, ostride: int = 1, ophase: int = 0,
           Tq: int | None = None) -> torch.Tensor:
    """Channels-last conv1d [B, Tin, Cin] -> [B, Tout, Cout'] with fused
    pre-activation (leaky ReLU), bias, act (relu / tanh / gated), residual add,
    scale, accumulate and length mask (see conv1d.hip). ``pad`` defaults to
    'same'. ``res``/``acc``/``out`` may be strided views; ``acc`` may alias ``out``."""
    B, Tin, Cin = x.shape
    assert Cin == cw.Cin
    if pad is None:
        pad = dil * (cw.K - 1) // 2
    if Tq is None:
        Tq = (Tin + 2 * pad - dil * (cw.K - 1) - 1) // stride + 1
    T_out = Tout if Tout is not None else Tq * ostride + ophase
    Co = cw.out_channels
    act_id = {None: 0, "relu": 1, "tanh": 2, "gated": 3}[act]
    assert (act == "gated") == cw.gated
    if not _gpu(x):
        y = ref.conv1d(x, cw.w, cw.bias, dil=dil, pad=pad, stride=stride, pre_slope=pre_slope,
                       act=act, res=res, alpha=alpha, acc=acc, lens=lens, Tout=T_out,
                       ostride=ostride, ophase=ophase, Tq=Tq)
        if pcm16:
            y = (y.clamp(-1, 1) * 32767).round().to(torch.int16)
        else:
            y = y.to(torch.bfloat16)
        if out is not None:
            if ostride == 1 and ophase == 0 and Tq == T_out:
                out.copy_(y)
            else:  # polyphase: only this phase's rows
                q = torch.arange(Tq, device=x.device) * ostride + ophase
                q = q[(q >= 0) & (q < T_out)]
                out[:, q] = y[:, q]
            return out
        return y
    assert x.dtype == torch.bfloat16 and x.stride(-1) == 1
    dt = torch.int16 if pcm16 else torch.bfloat16
    if out is None:
        out = torch.empty(B, T_out, Co, dtype=dt, device=x.device)
    assert out.dtype == dt and out.stride(-1) == 1 and out.shape[1] == T_out

    def bs(t):
        return (0, 0) if t is None else (t.stride(0), t.stride(1))
    for t in (res, acc):
        if t is not None:
            assert t.dtype == torch.bfloat16 and t.stride(-1) == 1 and t.shape[1] >= T_out
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.numel() == B
    check(kernels().loqa_conv1d(
        ptr(x), x.stride(0), x.stride(1), ptr(cw.wp), ptr(cw.bp), ptr(out), out.stride(0),
        out.stride(1), ptr(res), *bs(res), ptr(acc), *bs(acc), ptr(lens), B, Tin, Cin, Tq,
        cw.cpad, cw.K, dil, pad, stride, ostride, ophase, T_out,
        0 if pre_slope is None else 1, float(pre_slope or 0.0), act_id, float(alpha), int(pcm16),
        Co, stream_ptr(x)), "conv1d")
    return out


class ConvTransposeWeight:
    """ConvTranspose1d(kernel Kt = 2s-style, stride s) as s polyphase convs:
    y[q*s + r - p] = sum_j x[q - j] w[:, :, r + j*s]."""

    def __init__(self, w: torch.Tensor, bias: torch.Tensor | None, stride: int, padding: int):
        Cin, Cout, Kt = w.shape
        assert Kt % stride == 0
        self.w, self.bias, self.stride, self.padding = w, bias, stride, padding
        self.taps = Kt // stride
        self.phases = []
        for r in range(stride):
            # tap kk of the regular conv reads x[q - (taps-1) + kk] with weight w[r + (taps-1-kk)*s]
            ks = [r + (self.taps - 1 - kk) * stride for kk in range(self.taps)]
            wr = w[:, :, ks].permute(1, 0, 2).contiguous()  # [Cout, Cin, taps]
            self.phases.append(ConvWeight(wr, bias))
        self.Cout = Cout

    def out_len(self, Tin: int) -> int:
        return (Tin - 1) * self.stride - 2 * self.padding + self.taps * self.stride


def conv_transpose1d(x: torch.Tensor, ct: ConvTransposeWeight, *,
                     pre_slope: float | None = None, polyphase: bool | None = None) -> torch.Tensor:
    """ConvTranspose1d on channels-last rows; on the GPU always as polyphase
    MFMA convolutions (``polyphase=True`` forces that decomposition on the CPU
    too, for testing)."""
    B, Tin, _ = x.shape
    T_out = ct.out_len(Tin)
    s, p = ct.stride, ct.padding
    if not _gpu(x) and not polyphase:
        return ref.conv_transpose1d(x, ct.w, ct.bias, stride=s, padding=p,
                                    pre_slope=pre_slope).to(torch.bfloat16)
    out = torch.zeros(B, T_out, ct.Cout, dtype=torch.bfloat16, device=x.device)
    for r, cw in enumerate(ct.phases):
        Tq = (T_out - r + p + s - 1) // s
        conv1d(x, cw, dil=1, pad=ct.taps - 1, stride=1, pre_slope=pre_slope, out=out, Tout=T_out,
               ostride=s, ophase=r - p, Tq=Tq)
    return out


def relpos_attention(qkv: torch.Tensor, emb_k: torch.Tensor, emb_v: torch.Tensor,
                     lens: torch.Tensor | None, n_heads: int, head_dim: int, window: int,
                     scale: float | None = None) -> torch.Tensor:
    """VITS windowed relative-position self-attention over q|k|v rows [B, T, 3C]."""
    B, T, _ = qkv.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    if not _gpu(qkv):
        return ref.relpos_attention(qkv, emb_k, emb_v, lens, n_heads, head_dim, window,
                                    scale).to(torch.bfloat16)
    assert qkv.dtype == torch.bfloat16 and qkv.stride(-1) == 1
    # the kernel addresses row (b, i) at (b * T + i) * ld: no batch stride of its own
    assert B == 1 or qkv.stride(0) == T * qkv.stride(1), "qkv: batch stride must be T * row stride"
    assert lens is None or (lens.dtype == torch.int32 and lens.device == qkv.device
                            and lens.is_contiguous() and lens.numel() == B), \
        "lens: int32 [B] on the device of qkv"
    out = torch.empty(B, T, n_heads * head_dim, dtype=torch.bfloat16, device=qkv.device)
    check(kernels().loqa_relpos_attention(ptr(qkv), qkv.stride(1), ptr(emb_k), ptr(emb_v),
                                          ptr(lens), ptr(out), out.stride(1), B, T, n_heads,
                                          head_dim, window, scale, stream_ptr(qkv)),
          "relpos_attention")
    return out


def expand_sample(stats: torch.Tensor, cum: torch.Tensor, flen: torch.Tensor, F: int,
                  noise_scale: float, seed: int = 0,
                  seed_dev: torch.Tensor | None = None) -> torch.Tensor:
    """Length regulation + prior sampling: [B, T, 2C] stats -> z_p [B, F, C] bf16.
    ``seed_dev`` (GPU, int32 [1]): the seed read on the device (graph replay)."""
    B, T, C2 = stats.shape
    if not _gpu(stats):
        g = torch.Generator().manual_seed(seed)
        noise = torch.randn(B, F, C2 // 2, generator=g)
        return ref.expand_sample(stats, cum, flen, F, noise_scale, noise).to(torch.bfloat16)
    assert cum.dtype == torch.int32 and flen.dtype == torch.int32
    # the kernel addresses row (b, i) at (b * T + i) * ld: no batch stride of its own
    assert stats.dtype == torch.bfloat16 and stats.stride(2) == 1
    assert B == 1 or stats.stride(0) == T * stats.stride(1), "stats: batch stride must be T * row stride"
    assert cum.is_contiguous() and cum.shape == (B, T) and flen.is_contiguous()
    z = torch.empty(B, F, C2 // 2, dtype=torch.bfloat16, device=stats.device)
    check(kernels().loqa_expand_sample(ptr(stats), stats.stride(1), ptr(cum), B, T, ptr(flen),
                                       ptr(z), F, C2 // 2, float(noise_scale), seed & 0xFFFFFFFF,
                                       ptr(seed_dev), stream_ptr(stats)), "expand_sample")
    return z


# ------------------------------------------------------------ fused decode GEMMs
class FusedScratch:
    """Device state shared by the fused decode GEMMs of one engine: split-K
    ticket counters (zeroed once; each reducer resets its own) and the per-tile
    row statistics (sums of squares, sums) handed from the residual epilogues to
    the next GEMM's norm prologue."""

    def __init__(self, device, max_tiles: int = 8192, max_rows: int = 128):
        # max_rows = the largest Mpad (128): the 70B gate|up at Mpad 128 has
        # 3584 row tiles x 128 rows of statistics
        self.counters = torch.zeros(max_tiles, dtype=torch.int32, device=device)
        self.rowsq = torch.zeros(max_tiles * max_rows, dtype=torch.float32, device=device)
        self.rowsum = torch.zeros(max_tiles * max_rows, dtype=torch.float32, device=device)
        self.stat_tiles = 0   # partial tiles written by the last residual epilogue

    def seed_stats(self, x: torch.Tensor, sums: bool = True) -> None:
        """Row statistics of ``x`` as ONE partial tile (layer 0's norm input)."""
        M = x.shape[0]
        xf = x.float()
        torch.sum(xf.square(), 1, out=self.rowsq[:M])
        if sums:
            torch.sum(xf, 1, out=self.rowsum[:M])
        self.stat_tiles = 1


_FUSED_MODES = {"silu": 1, "resid": 2, "rope": 3, "act": 4}
_NORMS = {None: 0, False: 0, True: 1, "rms": 1, "ln": 2}
_ACTS = {"none": 0, "gelu": 1, "f32": 2}   # "f32": no activation, f32 output


class FusedLinear:
    """A decode projection prepared for the fused GEMM: the pre-shuffled weight
    (rows optionally permuted), with the input norm's weight folded into it and
    the norm's shift / the linear bias folded into one f32 output bias.

    norm "rms": rmsnorm(x; g) W^T            -> s * (W g) x
    norm "ln" : layernorm(x; g, b) W^T + c   -> s * ((W g) x - mean * colsum) + (W b + c)
    """

    def __init__(self, w: torch.Tensor, *, norm: str | None = None, norm_w=None, norm_b=None,
                 bias=None, perm: torch.Tensor | None = None):
        wf = w.float()
        self.norm = norm
        if norm is not None:
            wf = wf * norm_w.float()[None, :]
        wb = wf.to(torch.bfloat16)
        b = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
        if bias is not None:
            b = b + bias.float()
        if norm == "ln" and norm_b is not None:
            # W @ beta as a multiply + row sum (load time; keeps rocBLAS's GEMV
            # out of the process, so a kernel trace holds no vendor BLAS at all)
            b = b + (w.float() * norm_b.float()[None, :]).sum(1)
        self.colsum = wb.float().sum(1) if norm == "ln" else None
        self.has_bias = bias is not None or (norm == "ln" and norm_b is not None)
        if perm is not None:
            wb = wb[perm]
            b = b[perm]
            if self.colsum is not None:
                self.colsum = self.colsum[perm].contiguous()
        self.bias = b.contiguous() if self.has_bias else None
        self.wp = shuffle_weight(wb.contiguous())
        self.N, self.K = w.shape


def tune_fused(wp, mode: str, *, mpads=(16, 32, 64, 128), norm=None, act: str = "none",
               heads: tuple | None = None, cos_sin=None, prefill: bool = False,
               xl: bool = True) -> None:
    """Measure the split-K of one fused decode GEMM shape on dummy operands
    (``heads`` = (H, Hkv, D) for "rope"); before any graph capture.
    ``prefill``: Mpad 64 is the chunked prefill of compact weights (a whole
    weight pass per 64 tokens, on its own stream): 64-row tiles and 4 waves
    along rows are then candidates too (70B gate|up 64 tokens: 204 us vs 483 us
    for 16-row tiles). Otherwise Mpad 64 is a decode step beside the Whisper
    decoder, where those long-lived workgroups slow the pipeline."""
    lin = wp if isinstance(wp, FusedLinear) else None
    w = lin.wp if lin is not None else wp
    if not _gpu(w) or NO_TUNE:
        return
    dev = w.device
    N, K = w.shape[0] * 16, w.shape[1] * 32
    scr = FusedScratch(dev)
    bf = dict(dtype=torch.bfloat16, device=dev)
    nrm = norm if norm is not None else (lin.norm if lin is not None else None)
    # cold-weight timing: enough copies that the set outgrows the Infinity Cache
    nbytes = w.numel() * w.element_size()
    copies = [wp]
    for _ in range(min(15, -(-(768 << 20) // nbytes) - 1)):
        if lin is not None:
            c = copy.copy(lin)
            c.wp = lin.wp.clone()
        else:
            c = wp.clone()
        copies.append(c)
    xl_on = xl and os.environ.get("LOQA_TUNE_XL", "1") != "0"
    for Mpad in mpads:
        if Mpad == 128 and not xl_on:
            continue
        key = (mode, N, K, Mpad) + _wtag(w)
        if key in _FSPLITS:
            continue
        x = torch.randn(Mpad, K, **bf)
        kw: dict = {}
        if nrm:
            tiles = max(1, K // 32)
            scr.rowsq[: tiles * Mpad].fill_(float(K) / tiles)
            kw.update(rowsq_tiles=tiles)
        if mode == "resid":
            kw.update(residual=torch.zeros(Mpad, N, **bf))
        elif mode == "act":
            kw.update(act=act)
        elif mode == "rope":
            H, Hkv, D = heads
            kc = torch.zeros(max(4, Mpad // 16), Hkv, 16, D, **bf)   # one slot per row
            pos = torch.arange(Mpad, dtype=torch.int32, device=dev)
            kw.update(positions=pos, cos_sin=cos_sin, q_out=torch.empty(Mpad, H * D, **bf),
                      k_cache=kc, v_cache=torch.zeros_like(kc), slots=pos, n_heads=H, n_kv=Hkv,
                      head_dim=D)
        wide = Mpad <= 32 or prefill
        rts = (1, 2, 4) if (prefill and Mpad == 64) else (1, 2)
        # XL layouts only at Mpad 128: at Mpad 64 / 32 they win in isolation but,
        # as decode steps beside the Whisper decoder, took the pipeline from 17.6
        # to 10.3 utt/s (long-lived 4-wave workgroups: the co-scheduling cliff,
        # docs/PERF.md)
        xl = "only" if Mpad == 128 else "no"
        tune_fused_splits(key, lambda sp, rt, wr, i, xl_=0: skinny_fused(
            x, copies[i], mode, scr, splits=sp, rt=rt, wr=wr, norm=nrm, xl=xl_, **kw), K, rts=rts,
            ncopies=len(copies), wr4=wide, fewest=wide, xl=xl)
    del copies


def fold_norm(w: torch.Tensor, norm_w: torch.Tensor) -> torch.Tensor:
    """Weight rows with an RMSNorm weight folded in (W * diag(g)), the operand
    of a ``norm=True`` fused GEMM: rmsnorm(x) W^T = s(x) * (x (W diag(g))^T)."""
    return (w.float() * norm_w.float()[None, :]).to(w.dtype)


def skinny_fused(x: torch.Tensor, wp, mode: str, scratch: FusedScratch, *,
                 splits: int | None = None, norm=None, eps: float = 1e-5,
                 rowsq_tiles: int | None = None, rt: int | None = None,
                 residual: torch.Tensor | None = None, positions=None, cos_sin=None, q_out=None,
                 k_cache=None, v_cache=None, slots=None, n_heads: int = 0, n_kv: int = 0,
                 head_dim: int = 0, out=None, act: str = "none", bias=None, colsum=None,
                 row_sums: bool = False, wr: int | None = None, xl: int | None = None,
                 attn: dict | None = None) -> torch.Tensor:
    """Skinny GEMM with a fused epilogue and optional input norm; Mpad 16, 32,
    64 or 128 (``xl``: activations staged through LDS, 4 waves along rows,
    required at Mpad 128; chosen by the tuner at 64).

    ``wp`` is a shuffled weight or a ``FusedLinear`` (which supplies the norm
    kind unless ``norm`` is given, the folded bias and the LayerNorm column
    sums). ``norm`` True/"rms":
    RMSNorm, "ln": LayerNorm; the row statistics come from ``rowsq_tiles``
    partial tiles in ``scratch`` (default: what the last residual epilogue wrote); the norm
    weight is folded into the weight.
    mode "silu": returns bf16 [Mpad, N/2] (weights in ``perm_gate_up`` order);
    "resid": residual += x W^T (+ bias) in place, writes per-tile row sums of
    squares (and row sums with ``row_sums``);
    "rope": q -> q_out, k (RoPE'd when ``cos_sin``) and v -> paged caches
    (``perm_rope_qkv`` order); "act": returns act(x W^T + bias) bf16 [Mpad, N].

    ``attn`` (mode "rope"): the step's causal decode attention over the paged
    caches (keys of :func:`attention`: cu_q, ctx_lens, block_tables, max_q,
    split_keys, num_splits, workspace, max_k, scale, out) follows the GEMM and
    its output is returned (mode "act": attention over contiguous K / V rows,
    keys k, v, kv_start). Two launches: the one-launch hand-off was measured
    slower in every configuration and removed (docs/PERF.md, round 5)."""
    if attn is not None:
        assert mode in ("rope", "act")
        rope = mode == "rope"
        if not rope and out is None:
            out = torch.empty(x.shape[0], wp.shape[0] * 16 if not isinstance(wp, FusedLinear)
                              else wp.N, dtype=torch.bfloat16, device=x.device)
        qq = skinny_fused(x, wp, mode, scratch, splits=splits, norm=norm, eps=eps,
                          rowsq_tiles=rowsq_tiles, rt=rt, positions=positions, cos_sin=cos_sin,
                          q_out=q_out, k_cache=k_cache, v_cache=v_cache, slots=slots,
                          n_heads=n_heads, n_kv=n_kv, head_dim=head_dim, bias=bias,
                          colsum=colsum, wr=wr, xl=xl, out=out, act=act)
        if rope:
            return attention(q_out, k_cache, v_cache, attn["cu_q"], n_heads=n_heads,
                             n_kv=n_kv, head_dim=head_dim, causal=True, max_q=attn["max_q"],
                             ctx_lens=attn["ctx_lens"], block_tables=attn["block_tables"],
                             scale=attn.get("scale"), grouped=True,
                             split_keys=attn["split_keys"], num_splits=attn["num_splits"],
                             workspace=attn["workspace"], out=attn.get("out"),
                             max_k=attn.get("max_k"))
        return attention(qq, attn["k"], attn["v"], attn["cu_q"], n_heads=n_heads, n_kv=n_kv,
                         head_dim=head_dim, causal=False, max_q=attn["max_q"],
                         cu_k=attn["kv_start"], ctx_lens=attn["ctx_lens"],
                         scale=attn.get("scale"), grouped=True,
                         split_keys=attn["split_keys"], num_splits=attn["num_splits"],
                         workspace=attn["workspace"], out=attn.get("out"))
    if isinstance(wp, FusedLinear):
        lin = wp
        wp = lin.wp
        norm = lin.norm if norm is None else norm
        bias = lin.bias if bias is None else bias
        colsum = lin.colsum if colsum is None else colsum
    Mpad, K = x.shape
    N = wp.shape[0] * 16
    nrm = _NORMS[norm]
    fp8, mx4 = isinstance(wp, Fp8Weight), isinstance(wp, Mxfp4Weight)
    tuned = _FSPLITS.get((mode, N, K, Mpad) + _wtag(wp))
    S = splits or (tuned[0] if tuned else choose_splits(N, K, Mpad, tag=_wtag(wp)))
    rt = rt or (tuned[1] if tuned else (1 if Mpad == 128 else 2))
    if xl is None:
        xl = tuned[3] if (tuned and not splits and len(tuned) > 3) else int(Mpad == 128)
    if wr is None:
        wr = tuned[2] if (tuned and not splits and len(tuned) > 2) else 1
        if mx4 and wr == 1 and not xl and K % (S * 512):
            # untuned MXFP4, K not a whole number of loads for 4 waves along K:
            # the rows-per-wave layout takes any K % 128 == 0
            S, wr = 1, 4
            rt = rt if N % (64 * rt) == 0 else 1
    if xl:
        wr = 4
        rt = rt if rt in (1, 2) and N % (64 * rt) == 0 else 1
    elif wr != 1 and (S != 1 or N % (64 * rt)):
        wr = 1
    if rowsq_tiles is None:
        rowsq_tiles = scratch.stat_tiles
    m = _FUSED_MODES[mode]
    ntiles = N // (16 * rt)
    if mode == "resid":
        scratch.stat_tiles = ntiles
    if mode == "silu" and out is None:
        out = torch.empty(Mpad, N // 2, dtype=torch.bfloat16, device=x.device)
    elif mode == "act" and out is None:
        out = torch.empty(Mpad, N, dtype=torch.float32 if act == "f32" else torch.bfloat16,
                          device=x.device)
    if not _gpu(x):
        return _skinny_fused_ref(x, wp, mode, scratch, nrm, eps, rowsq_tiles, residual,
                                 positions, cos_sin, q_out, k_cache, v_cache, slots, n_heads,
                                 n_kv, head_dim, out, act, bias, colsum, row_sums, rt)
    assert Mpad in (16, 32, 64, 128) and x.dtype == torch.bfloat16 and x.stride(1) == 1
    assert Mpad != 128 or xl, "Mpad 128 needs the XL layout"
    assert ntiles <= scratch.counters.numel() and ntiles * Mpad <= scratch.rowsq.numel()
    if nrm == 2:
        assert colsum is not None and colsum.numel() == N
    if fp8:
        assert nrm != 2, "fp8 weights: no LayerNorm prologue"
        assert wp.is_cuda and wp.wp.is_contiguous() and wp.scale.is_contiguous()
    elif mx4:
        assert nrm != 2, "MXFP4 weights: no LayerNorm prologue"
        assert wp.is_cuda and wp.wp.is_contiguous() and wp.scales.is_contiguous()
        assert wp.wp.data_ptr() % 16 == 0 and wp.scales.data_ptr() % 4 == 0
    else:
        _bf16_contig(wp, "wp")
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
    if mode == "act":
        assert out.dtype == (torch.float32 if act == "f32" else torch.bfloat16)
        assert out.stride(0) % 4 == 0 and out.shape[0] >= Mpad and out.shape[1] >= N
    if mode == "rope":   # the epilogue reads slots / positions for every padded row
        assert slots.numel() >= Mpad and q_out.shape[0] >= Mpad and k_cache.is_contiguous()
        assert cos_sin is None or positions.numel() >= Mpad
    elif mode == "resid":
        assert residual.shape[0] >= Mpad and residual.shape[1] == N
    part = torch.empty(S, Mpad, N, dtype=torch.float32, device=x.device) if S > 1 else None
    blk = k_cache.shape[2] if k_cache is not None else 0
    p = FusedParams()
    p.x, p.ldx, p.Wp, p.part, p.counters = ptr(x), x.stride(0), ptr(wp.wp if fp8 or mx4 else wp), \
        ptr(part), ptr(scratch.counters)
    if fp8:
        p.wdtype, p.wscale = 1, ptr(wp.scale)
    elif mx4:
        p.wdtype, p.wscale = 2, ptr(wp.scales)
    p.Mpad, p.N, p.K, p.S, p.mode, p.norm = Mpad, N, K, S, m, nrm
    if nrm:
        p.rowsq_in, p.rowsum_in = ptr(scratch.rowsq), ptr(scratch.rowsum)
    p.rowstat_tiles, p.eps = rowsq_tiles, eps
    p.colsum, p.bias = ptr(colsum), ptr(bias)
    p.out, p.ldo, p.act = ptr(out), (out.stride(0) if out is not None else 0), _ACTS[act]
    if mode == "resid":
        p.residual, p.rowsq_out = ptr(residual), ptr(scratch.rowsq)
        p.rowsum_out = ptr(scratch.rowsum) if row_sums else None
    p.positions, p.cs, p.q_out = ptr(positions), ptr(cos_sin), ptr(q_out)
    p.kc, p.vc, p.slots = ptr(k_cache), ptr(v_cache), ptr(slots)
    p.H, p.Hkv, p.D, p.blk = n_heads, n_kv, head_dim, blk
    p.rt, p.wr, p.xl = rt, wr, int(bool(xl))
    check(kernels().loqa_skinny_fused(ctypes.byref(p), stream_ptr(x)), "skinny_fused")
    if mode in ("silu", "act"):
        return out
    return q_out if mode == "rope" else residual


def set_launch_priority(prio: int) -> None:
    """Wave issue priority (s_setprio 3) of the decode attention and fused
    GEMM kernels this host THREAD launches or captures from now on (0 =
    default); the STT decoder thread sets it under ``LOQA_STT_WAVE_PRIO``."""
    if torch.cuda.is_available():
        kernels().loqa_set_launch_prio(int(prio))


def _skinny_fused_ref(x, wp, mode, scratch, nrm, eps, rowsq_tiles, residual, positions,
                      cos_sin, q_out, k_cache, v_cache, slots, H, Hkv, D, out, act, bias, colsum,
                      row_sums, rt=2):
    Mpad, K = x.shape
    N = wp.shape[0] * 16
    y = x.float() @ ref.unshuffle_weight(wp).float().t()  # [Mpad, N] in permuted row order
    if nrm:
        rs = scratch.rowsq[: rowsq_tiles * Mpad].view(rowsq_tiles, Mpad)
        if nrm == 1:
            y = y * ref.fused_row_scale(rs, eps, K)[:, None]
        else:
            sm = scratch.rowsum[: rowsq_tiles * Mpad].view(rowsq_tiles, Mpad)
            mean, rstd = ref.fused_ln_stats(rs, sm, eps, K)
            y = rstd[:, None] * (y - mean[:, None] * colsum.float()[None, :])
    if bias is not None:
        y = y + bias.float()[None, :]
    if mode == "silu":
        F = N // 2
        inv = torch.argsort(ref.perm_gate_up(F))
        y = y[:, inv]
        out.copy_(ref.silu_mul(y.to(torch.bfloat16)))
        return out
    if mode == "act":
        if act == "f32":
            out.copy_(y)
            return out
        yb = y.to(torch.bfloat16)
        if act == "gelu":
            yb = torch.nn.functional.gelu(yb.float()).to(torch.bfloat16)
        out.copy_(yb)
        return out
    if mode == "resid":
        h = (y + residual.float()).to(torch.bfloat16)
        residual.copy_(h)
        R = 16 * rt
        sq = h.float().pow(2).view(Mpad, N // R, R).sum(-1).t().contiguous()  # [tiles, Mpad]
        scratch.rowsq[: sq.numel()] = sq.flatten()
        if row_sums:
            sm = h.float().view(Mpad, N // R, R).sum(-1).t().contiguous()
            scratch.rowsum[: sm.numel()] = sm.flatten()
        return residual
    inv = torch.argsort(ref.perm_rope_qkv(H, Hkv, D))
    qkv = y[:, inv].to(torch.bfloat16)
    ref.rope_kv_append(qkv, positions, cos_sin, k_cache, v_cache, slots, H, Hkv, D)
    q_out.copy_(qkv[:, : H * D])
    return q_out


# ------------------------------------------------------------- prefill GEMM
PREFILL_GEMM_NT = 128     # features per workgroup of the default layout (3)


# v2 layouts: (row tiles, feature tiles) per wave and waves along M (the other
# 4 / WM waves go along N) -> workgroup tile (16 WM rbw) x (16 (4 / WM) ft)
PREFILL2_LAYOUTS = {0: (5, 4, 2), 1: (10, 4, 2), 2: (5, 2, 2), 3: (10, 2, 1), 4: (10, 4, 1)}
# layout 3 (v1's 1 x 4 waves with the one-barrier pipeline) measured fastest on
# every prefill / encoder shape (profiles/r3_prefill_gemm2_layouts.txt)
PREFILL2_LAYOUT = 3


def prefill_gemm2(x: torch.Tensor, wp: torch.Tensor, splits: int = 1, epi: str = "bf16",
                  layout: int | None = None) -> torch.Tensor:
    """x [M, K] bf16 @ W^T for prefill-sized M (64 - a few thousand rows), W
    pre-shuffled (``shuffle_weight``; ``csrc/kernels/gemm_prefill.hip`` v2).
    ``epi``: "bf16" -> [M, N]; "slabs" -> f32 split-K partials [S, M, N] (a
    slab consumer sums them); "swiglu" -> silu(gate) * up [M, N / 2] bf16 from
    a ``perm_gate_up`` weight (16-row gate|up pair tiles)."""
    M, K = x.shape
    N = wp.shape[0] * 16
    assert wp.shape[1] * 32 == K
    lay = PREFILL2_LAYOUT if layout is None else layout
    rbw, ft, wm = PREFILL2_LAYOUTS[lay]
    e = {"bf16": 0, "slabs": 1, "swiglu": 2}[epi]
    assert e == 1 or splits == 1
    if not _gpu(x):
        part = ref.skinny_gemm(x, wp, splits)
        if e == 1:
            return part
        y = part.sum(0)
        if e == 2:
            y = ref.swiglu_pairs(y)
        return y.to(torch.bfloat16)
    _bf16_contig(x, "x")
    assert N % (16 * ft * (4 // wm)) == 0 and K % (splits * 64) == 0, (N, K, splits, lay)
    if e == 1:
        out = torch.empty(splits, M, N, dtype=torch.float32, device=x.device)
        rc = kernels().loqa_gemm_prefill2(ptr(x), M, K, ptr(wp), N, splits, None, ptr(out), 1, lay,
                                          stream_ptr(x))
    else:
        out = torch.empty(M, N // 2 if e == 2 else N, dtype=torch.bfloat16, device=x.device)
        rc = kernels().loqa_gemm_prefill2(ptr(x), M, K, ptr(wp), N, 1, ptr(out), None, e, lay,
                                          stream_ptr(x))
    check(rc, "gemm_prefill2")
    return out



# ----------------------------------------- tiled MFMA GEMMs (ops/gemm.py)
from .gemm import (  # noqa: E402,F401
    GEMM_TILE_DEFAULT_LAYOUT, GEMM_TILE_FRAGS, GEMM_TILE_LAYOUTS, PROJ_TABLE, SK_DEEP, SK_LAYOUTS,
    SK_TABLE, _SK_WS, _gt_ref, _sk_ref, conv_k3_im2col_ref, conv_k3_weight, gemm_sk, gemm_sk_plan,
    gemm_tile, gemm_tile_dims, gemm_ws, gemm_ws_rows, proj,
)
