"""Plain-PyTorch fp32 reference implementations of every hot op.

These are the numerics oracle for the HIP kernels (tests compare kernel output
against them) and the CPU execution path (no GPU in the CI tier).
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from ..config import AUDIO_SAMPLE_RATES as RESAMPLE_RATES
from ..config import FLAC_BLOCK_SIZES as FLAC_BLOCKS
from ..config import HOTWORD_MAX_PHRASES, HOTWORD_MAX_TOKENS  # noqa: F401


def rmsnorm(x, w, eps, residual=None):
    if residual is not None:
        s = (x.float() + residual.float()).to(residual.dtype)
        residual.copy_(s)
        x = s
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return y.to(x.dtype)


def layernorm(x, w, b, eps, residual=None):
    if residual is not None:
        s = (x.float() + residual.float()).to(residual.dtype)
        residual.copy_(s)
        x = s
    y = torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps)
    return y.to(x.dtype)


def silu_mul(x):
    F = x.shape[-1] // 2
    g, u = x[..., :F].float(), x[..., F:].float()
    return (torch.nn.functional.silu(g) * u).to(x.dtype)


def gelu_bias_(x, bias=None, pos=None):
    y = x.float()
    if bias is not None:
        y = y + bias.float()
    y = torch.nn.functional.gelu(y)
    if pos is not None:
        rows = y.reshape(-1, y.shape[-1]).shape[0]
        idx = torch.arange(rows, device=x.device) % pos.shape[0]
        y = (y.reshape(-1, y.shape[-1]) + pos.float()[idx]).reshape(y.shape)
    x.copy_(y.to(x.dtype))
    return x


def rope_cos_sin(head_dim: int, max_pos: int, theta: float, device=None,
                 scaling: tuple | None = None) -> torch.Tensor:
    """[max_pos, D/2, 2] f32 table of (cos, sin) for NeoX rotate-half RoPE.
    ``scaling`` = (factor, low_freq_factor, high_freq_factor, original max
    positions): Llama-3.1 frequency scaling - wavelengths longer than
    original / low are divided by ``factor``, shorter than original / high
    kept, and the band between interpolated."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling is not None:
        factor, low, high, orig = scaling
        wavelen = 2 * math.pi / inv
        smooth = ((orig / wavelen - low) / (high - low)).clamp(0.0, 1.0)
        inv = torch.where(wavelen > orig / low, inv / factor,
                          torch.where(wavelen < orig / high, inv,
                                      (1 - smooth) * inv / factor + smooth * inv))
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).float().to(device)


def apply_rope(x: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    """x [T, H, D] (any float), cs [T, D/2, 2] -> rotated x (fp32)."""
    half = x.shape[-1] // 2
    a, b = x[..., :half].float(), x[..., half:].float()
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


def rope_kv_append(qkv, positions, cos_sin, k_cache, v_cache, slots, H, Hkv, D):
    T = qkv.shape[0]
    if T == 0:
        return None
    q = qkv[:, : H * D].view(T, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(T, Hkv, D)
    v = qkv[:, (H + Hkv) * D:(H + 2 * Hkv) * D].view(T, Hkv, D)
    if cos_sin is not None:
        cs = cos_sin[positions.long()]
        q.copy_(apply_rope(q, cs).to(q.dtype))
        k = apply_rope(k, cs).to(qkv.dtype)
    blk = k_cache.shape[2]
    sl = slots.long()
    valid = sl >= 0
    b, o = (sl // blk)[valid], (sl % blk)[valid]
    k_cache[b, :, o, :] = k[valid].to(k_cache.dtype)
    v_cache[b, :, o, :] = v[valid].to(v_cache.dtype)
    return None


def attention(q, k, v, cu_q, *, n_heads, n_kv, head_dim, causal, cu_k=None, ctx_lens=None,
              block_tables=None, scale=None, out=None):
    H, Hkv, D = n_heads, n_kv, head_dim
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    Tq = q.shape[0]
    res = torch.zeros(Tq, H * D, dtype=torch.float32, device=q.device)
    cuq = cu_q.tolist()
    G = H // Hkv
    for b in range(len(cuq) - 1):
        q0, q1 = cuq[b], cuq[b + 1]
        ql = q1 - q0
        if ql == 0:
            continue
        if block_tables is not None:
            L = int(ctx_lens[b])
            blk = k.shape[2]
            idx = torch.arange(L, device=k.device)
            bt = block_tables[b].long()[idx // blk]
            kb = k[bt, :, idx % blk, :].float()  # [L, Hkv, D]
            vb = v[bt, :, idx % blk, :].float()
        else:
            k0 = int(cu_k[b])
            k1 = k0 + int(ctx_lens[b]) if ctx_lens is not None else int(cu_k[b + 1])
            L = k1 - k0
            kb = k[k0:k1, : Hkv * D].reshape(L, Hkv, D).float()
            vb = v[k0:k1, : Hkv * D].reshape(L, Hkv, D).float()
        qb = q[q0:q1, : H * D].reshape(ql, H, D).float()
        kb = kb.repeat_interleave(G, dim=1)
        vb = vb.repeat_interleave(G, dim=1)
        s = torch.einsum("qhd,khd->hqk", qb, kb) * scale
        if causal:
            qpos = torch.arange(ql, device=q.device) + (L - ql)
            kpos = torch.arange(L, device=q.device)
            s = s.masked_fill(kpos[None, None, :] > qpos[None, :, None], float("-inf"))
        p = torch.softmax(s, dim=-1)
        p = torch.nan_to_num(p, nan=0.0)
        res[q0:q1] = torch.einsum("hqk,khd->qhd", p, vb).reshape(ql, H * D)
    r = res.to(q.dtype)
    if out is not None:
        out.copy_(r)
        return out
    return r


def masked_argmax(logits, mask=None, mask_rows=None, token_ids=None):
    """``token_ids``: the columns are a gathered vocabulary subset; the result
    is the token id of the winning column (lowest column on a tie)."""
    x = logits.float()
    B, V = x.shape
    if mask is not None:
        m = mask if mask_rows is None else mask[mask_rows.long()]
        bits = unpack_mask(m, V)
        x = x.masked_fill(~bits, float("-inf"))
        none = ~bits.any(dim=-1)
    else:
        none = torch.zeros(B, dtype=torch.bool, device=x.device)
    r = x.argmax(dim=-1).to(torch.int32)
    if token_ids is not None:
        r = token_ids.to(torch.int32)[r.long()]
    r[none] = -1
    return r


def masked_argmax_logprob(logits, mask=None, mask_rows=None, token_ids=None):
    """``masked_argmax`` plus the selected token's log-softmax over the allowed
    tokens (masked fill, then ``log_softmax`` in fp32). Nothing allowed, or a
    winner of -inf: -inf (never NaN)."""
    idx = masked_argmax(logits, mask, mask_rows, token_ids)
    x = logits.float()
    B, V = x.shape
    if mask is not None:
        m = mask if mask_rows is None else mask[mask_rows.long()]
        x = x.masked_fill(~unpack_mask(m, V), float("-inf"))
    col = x.argmax(dim=-1, keepdim=True)
    lp = torch.log_softmax(x, dim=-1).gather(1, col)[:, 0]
    top = x.gather(1, col)[:, 0]
    lp = torch.where(torch.isinf(top) & (top < 0), torch.full_like(lp, float("-inf")), lp)
    return idx, lp


def masked_argmax_logprob_probe(logits, mask, mask_rows, probe, token_ids=None):
    """``masked_argmax_logprob`` plus ``x[b, probe[b]] - logsumexp(x[b, :])`` over
    ALL columns (the mask ignored), in fp32. ``probe[b] < 0`` (or >= V): +0.0;
    a probed logit of -inf or a row of -inf only: -inf (never NaN)."""
    idx, lp = masked_argmax_logprob(logits, mask, mask_rows, token_ids)
    x = logits.float()
    B, V = x.shape
    p = probe.long()
    on = (p >= 0) & (p < V)
    px = x.gather(1, p.clamp(0, V - 1)[:, None])[:, 0]
    plp = px - torch.logsumexp(x, dim=-1)
    plp = torch.where(torch.isinf(px) & (px < 0), torch.full_like(plp, float("-inf")), plp)
    plp = torch.where(on, plp, torch.zeros_like(plp))
    return idx, lp, plp


def ts_state_pack(last: int, f_last: bool, f_pen: bool) -> int:
    """The timestamp-rule state word of one decoder sequence: ``last`` = the
    last timestamp index sampled in the window (-1: none), ``f_last`` = the last
    sampled token was a timestamp, ``f_pen`` = the one before it was (or fewer
    than two tokens have been sampled)."""
    return ((int(last) + 1) << 2) | (int(bool(f_last)) << 1) | int(bool(f_pen))


def ts_state_unpack(word: int) -> tuple[int, bool, bool]:
    """``ts_state_pack`` reversed: (last, f_last, f_pen)."""
    word = int(word)
    return (word >> 2) - 1, bool((word >> 1) & 1), bool(word & 1)


def ts_state_next(word: int, ctl: int, winner: int, ts_begin: int) -> int:
    """The state word after a ruled row (``ctl`` 1 or 2) sampled ``winner``."""
    last, f_last, _ = (-1, False, True) if ctl == 1 else ts_state_unpack(word)
    is_ts = winner >= ts_begin
    return ts_state_pack(winner - ts_begin if is_ts else last, is_ts, True if ctl == 1 else f_last)


def ts_allowed(word: int, ctl: int, ts_count: int, max_initial: int) -> tuple[int, int, int]:
    """Whisper's timestamp rules for a ruled row as ``(text_ok, lo, hi)``:
    ``text_ok`` 2 = every column below ``ts_begin`` that the mask allows, 1 =
    only those at or above ``eot`` (a lone timestamp is followed by a timestamp
    or EOT), 0 = none (a window opens with a timestamp); ``lo .. hi`` = the
    timestamp indices allowed (``lo > hi``: none, the token after a closed pair
    is text). ``ctl`` 1 ignores ``word``."""
    if ctl == 1:
        return 0, 0, min(int(max_initial), ts_count - 1)
    last, f_last, f_pen = ts_state_unpack(word)
    hi = ts_count - 1
    if f_last and f_pen:
        return 2, hi + 1, hi
    lo = 0 if last < 0 else (last if f_last and not f_pen else last + 1)
    return (1 if f_last and not f_pen else 2), min(lo, hi + 1), hi


def ts_mass_rule(lse_t, lse_a, xt):
    """The f32 comparison of Whisper's mass rule, as the kernel spells it: the
    timestamps' log-probability mass against the best text token's."""
    return (lse_t - lse_a) > (xt - lse_a)


def masked_argmax_timestamps(logits, mask, mask_rows, probe, ts_ctl, ts_state, row_slot,
                             ts_begin, ts_count, eot, max_initial):
    """``masked_argmax_logprob_probe`` under Whisper's timestamp rules
    (``ApplyTimestampRules`` as a state machine, see ``ts_allowed``), in fp32.
    A row with ``ts_ctl[b] == 0`` is ``masked_argmax_logprob_probe``'s. A ruled
    row selects among A = the mask's columns below ``ts_begin`` that the rules
    leave plus the timestamp columns ``ts_begin + lo .. ts_begin + hi`` (their
    mask bits ignored): the best timestamp, with its log-softmax over the
    allowed timestamps, when logsumexp(timestamps) - logsumexp(A) exceeds the
    best other logit - logsumexp(A) (or nothing else is allowed), else the best
    other column with its log-softmax over A. It then updates
    ``ts_state[row_slot[b]]`` in place; nothing allowed: (-1, -inf), the state
    unchanged. Returns (int32 [B], float32 [B], float32 [B])."""
    idx, lp, plp = masked_argmax_logprob_probe(logits, mask, mask_rows, probe)
    x = logits.float()
    B, V = x.shape
    ninf = float("-inf")
    max_initial = min(int(max_initial), ts_count - 1)
    for b in range(B):
        ctl = int(ts_ctl[b])
        if ctl not in (1, 2):
            continue
        slot = int(row_slot[b])
        word = int(ts_state[slot])
        okx, okt, fire, lse_a, lse_t = _ts_classes(x[b], mask, mask_rows, b, word, ctl, ts_begin,
                                                   ts_count, eot, max_initial)
        if not (bool(okx.any()) or bool(okt.any())):
            idx[b], lp[b] = -1, ninf
            continue
        row, lse = (x[b].masked_fill(~okt, ninf), lse_t) if fire else \
            (x[b].masked_fill(~okx, ninf), lse_a)
        w = int(row.argmax())
        idx[b] = w
        lp[b] = row[w] - lse if row[w] != ninf else ninf
        ts_state[slot] = ts_state_next(word, ctl, w, ts_begin)
    return idx, lp, plp


def _ts_classes(xb, mask, mask_rows, b, word, ctl, ts_begin, ts_count, eot, max_initial):
    """A ruled row's two classes and the mass rule: (``okx`` = the mask's
    columns below ``ts_begin`` that the rules leave, ``okt`` = the allowed
    timestamp columns, the rule fires, logsumexp over both, over ``okt``)."""
    V = xb.shape[0]
    ninf = float("-inf")
    text_ok, lo, hi = ts_allowed(word, ctl, ts_count, max_initial)
    if mask is not None:
        okx = unpack_mask(mask[int(mask_rows[b]) if mask_rows is not None else b], V).clone()
    else:
        okx = torch.ones(V, dtype=torch.bool)
    okx[ts_begin:] = False
    okx[: (ts_begin, eot, 0)[text_ok]] = False
    okt = torch.zeros(V, dtype=torch.bool)
    okt[ts_begin + lo: ts_begin + hi + 1] = True
    xx = xb.masked_fill(~okx, ninf)
    any_x, any_t = bool(okx.any()), bool(okt.any())
    lse_a = torch.logsumexp(xb.masked_fill(~(okx | okt), ninf), dim=-1)
    lse_t = torch.logsumexp(xb.masked_fill(~okt, ninf), dim=-1)
    fire = any_t and (not any_x or bool(ts_mass_rule(lse_t, lse_a, xx.max())))
    return okx, okt, fire, lse_a, lse_t


# Temperature sampling (MODE 4 of the row scan): counter-based Gumbel noise in
# integer arithmetic that the device reproduces exactly, and the draw.
_M32 = 0xFFFFFFFF


def fmix32(h: int) -> int:
    """murmur3's 32-bit finalizer on a Python int (``_fmix32`` on tensors)."""
    h &= _M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def sample_key(seed: int, window: int, attempt: int, token_index: int) -> int:
    """The uint32 row key of one sampled token: an ``fmix32`` chain over (request
    seed, 30 s window, fallback attempt, index of the token in the window). It
    names the draw, so it is the same in any batch, bucket or pipeline depth."""
    h = fmix32((int(seed) + 0x9E3779B9) & _M32)
    for x in (window, attempt, token_index):
        h = fmix32(((h ^ (int(x) & _M32)) + 0x9E3779B9) & _M32)
    return h


def key_i32(key: int) -> int:
    """A uint32 key as the int32 with the same bits (the step field's type)."""
    key &= _M32
    return key - (1 << 32) if key >= (1 << 31) else key


def gumbel_hash(rng: torch.Tensor, V: int) -> torch.Tensor:
    """h[b, v] = fmix32(rng[b] ^ fmix32(v + 0x9E3779B9)) as int64 in [0, 2^32);
    ``rng``: int32 [B] (the bits of a uint32 key)."""
    key = (rng.to(torch.int64).cpu() & _M32)[:, None]
    col = _fmix32((torch.arange(V, dtype=torch.int64)[None, :] + 0x9E3779B9) & _M32)
    return _fmix32(key ^ col)


def gumbel_uniform(h: torch.Tensor) -> torch.Tensor:
    """u = (2 (h >> 9) + 1) / 2^24 of a 32-bit hash: an exact float32 in
    [2^-24, 1 - 2^-24], so ``-log(-log(u))`` is finite."""
    return (2 * (h.to(torch.int64) >> 9) + 1).to(torch.float32) * (1.0 / 16777216.0)


def gumbel_noise(rng: torch.Tensor, V: int) -> torch.Tensor:
    """g[b, v] = -log(-log(u)) in float32 for ``u = gumbel_uniform(gumbel_hash(rng,
    V))``: the CPU engine's noise. The device takes the same ``u`` through its own
    ``logf``, so its ``g`` agrees to a few ulp, not bit for bit."""
    u = gumbel_uniform(gumbel_hash(rng, V))
    return -torch.log(-torch.log(u))


def masked_argmax_sample(logits, mask, mask_rows, probe, ts_ctl, ts_state, row_slot, ts_begin,
                         ts_count, eot, max_initial, temp, rng, noise=None):
    """``masked_argmax_timestamps`` with a per-row temperature ``temp`` (float32
    [B]) and random key ``rng`` (int32 [B]). ``temp[b] == 0``: that op's row
    (``ts_ctl`` None: ``masked_argmax_logprob_probe``'s, every row rule-off).
    ``temp[b] > 0``: the row draws by Gumbel-max, the winner maximises
    ``x + T * g`` (fp64, rounded once to float32: the device's fmaf) over the
    allowed timestamps when the mass rule - evaluated at temperature 1, as
    Whisper filters the logits before it samples - fires, else over every
    allowed column; its log-probability is at temperature 1 over the same set.
    ``noise`` (float32 [B, V]): ``g``, default ``gumbel_noise(rng, V)``."""
    x = logits.float()
    B, V = x.shape
    ninf = float("-inf")
    T = temp.float().cpu()
    sampling = T > 0
    if ts_ctl is None:
        idx, lp, plp = masked_argmax_logprob_probe(logits, mask, mask_rows, probe)
        ctl_all = torch.zeros(B, dtype=torch.int32)
    else:
        ctl_all = ts_ctl.clone()
        ctl_all[~((ctl_all == 1) | (ctl_all == 2))] = 0
        greedy_ctl = ctl_all.clone()
        greedy_ctl[sampling] = 0          # the greedy pass leaves their state alone
        idx, lp, plp = masked_argmax_timestamps(logits, mask, mask_rows, probe, greedy_ctl,
                                                ts_state, row_slot, ts_begin, ts_count, eot,
                                                max_initial)
        max_initial = min(int(max_initial), ts_count - 1)
    if not bool(sampling.any()):
        return idx, lp, plp
    g = gumbel_noise(rng, V) if noise is None else noise.float().cpu()
    key = (x.double() + T.double()[:, None] * g.double()).float()
    for b in range(B):
        if not bool(sampling[b]):
            continue
        ctl = int(ctl_all[b])
        if ctl:
            slot = int(row_slot[b])
            word = int(ts_state[slot])
            okx, okt, fire, _, _ = _ts_classes(x[b], mask, mask_rows, b, word, ctl, ts_begin,
                                               ts_count, eot, max_initial)
            allowed = okt if fire else (okx | okt)
        elif mask is not None:
            allowed = unpack_mask(mask[int(mask_rows[b]) if mask_rows is not None else b], V)
        else:
            allowed = torch.ones(V, dtype=torch.bool)
        cols = allowed.nonzero()[:, 0]
        if not cols.numel():
            idx[b], lp[b] = -1, ninf
            continue
        w = int(cols[key[b, cols].argmax()])      # the first maximum: the lowest column
        idx[b] = w
        lse = torch.logsumexp(x[b].masked_fill(~allowed, ninf), dim=-1)
        lp[b] = x[b, w] - lse if x[b, w] != ninf else ninf
        if ctl:
            ts_state[slot] = ts_state_next(word, ctl, w, ts_begin)
    return idx, lp, plp


def unpack_mask(m: torch.Tensor, V: int) -> torch.Tensor:
    """int32 words [..., W] -> bool [..., V]"""
    shifts = torch.arange(32, device=m.device, dtype=torch.int32)
    bits = (m.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(*m.shape[:-1], -1)[..., :V].bool()


def pack_mask(bits: torch.Tensor) -> torch.Tensor:
    """bool [..., V] -> int32 words [..., ceil(V/32)]"""
    V = bits.shape[-1]
    W = (V + 31) // 32
    pad = torch.zeros(*bits.shape[:-1], W * 32, dtype=torch.int64, device=bits.device)
    pad[..., :V] = bits.long()
    w = (pad.reshape(*bits.shape[:-1], W, 32) << torch.arange(32, device=bits.device)).sum(-1)
    w = torch.where(w >= 2**31, w - 2**32, w)
    return w.to(torch.int32)


# ----------------------------------------------------------------- beam search
# Whisper's BeamSearchDecoder + MaximumLikelihoodRanker (patience 1, no length
# penalty). One order ranks candidates: higher score first, then the lower
# source beam, then the lower column.
def beam_topk(logits, mask=None, mask_rows=None, eot: int = -1, KB: int = 1):
    """Per row of ``logits`` [R, V]: ``cand_id`` int32 [R, KB], the KB allowed
    non-EOT columns of largest logit, descending, ties to the lower column, -1
    past the allowed count; ``cand_lp`` f32 [R, KB], their log-softmax over all
    allowed columns (EOT included; -inf past the count); ``eot_lp`` f32 [R],
    EOT's (-inf when the mask forbids it or ``eot`` is no column)."""
    x = logits.float().cpu()
    R, V = x.shape
    allowed = torch.ones(R, V, dtype=torch.bool)
    if mask is not None:
        m = mask if mask_rows is None else mask[mask_rows.long()]
        allowed = unpack_mask(m.cpu(), V)[:R]
    xm = x.masked_fill(~allowed, float("-inf"))
    lsm = torch.log_softmax(xm, dim=-1)
    lsm = torch.where(torch.isinf(xm) & (xm < 0), torch.full_like(lsm, float("-inf")), lsm)
    cand_id = np.full((R, KB), -1, np.int32)
    cand_lp = np.full((R, KB), -np.inf, np.float32)
    eot_lp = np.full(R, -np.inf, np.float32)
    xn, ln, an = xm.numpy(), lsm.numpy(), allowed.numpy()
    for r in range(R):
        cols = np.nonzero(an[r])[0]
        if 0 <= eot < V and an[r, eot]:
            eot_lp[r] = ln[r, eot]
            cols = cols[cols != eot]
        order = cols[np.lexsort((cols, -xn[r, cols]))][:KB]
        cand_id[r, :len(order)] = order
        cand_lp[r, :len(order)] = ln[r, order]
    dev = logits.device
    return (torch.from_numpy(cand_id).to(dev), torch.from_numpy(cand_lp).to(dev),
            torch.from_numpy(eot_lp).to(dev))


def beam_merge(cand_id, cand_lp, eot_lp, cum_in, n_src: int):
    """Per group g of ``cum_in`` [G, B]: the B best of the ``n_src * B``
    candidates of rows ``g * n_src ..`` by the f32 sum ``cum_in[g, src] +
    cand_lp``. Returns (tok, parent, lp, cum_out, eot_score, eot_fin), each
    [G, B]: missing candidates give tok = parent = -1 and lp = cum_out = -inf;
    ``eot_score = cum_in + eot_lp`` (-inf past ``n_src``); ``eot_fin`` = 1 for
    a source beam whose eot_score is strictly above ``cum_out[g, B - 1]``, or
    when fewer than B candidates exist."""
    dev = cum_in.device
    cid = cand_id.cpu().numpy()
    clp = cand_lp.cpu().numpy().astype(np.float32)
    elp = eot_lp.cpu().numpy().astype(np.float32)
    cum = cum_in.cpu().numpy().astype(np.float32)
    G, B = cum.shape
    assert n_src in (1, B) and cid.shape == (G * n_src, B)
    tok = np.full((G, B), -1, np.int32)
    parent = np.full((G, B), -1, np.int32)
    lp = np.full((G, B), -np.inf, np.float32)
    cum_out = np.full((G, B), -np.inf, np.float32)
    eot_score = np.full((G, B), -np.inf, np.float32)
    eot_fin = np.zeros((G, B), np.int32)
    with np.errstate(invalid="ignore"):
        for g in range(G):
            cands = []
            for s in range(n_src):
                for j in range(B):
                    c = int(cid[g * n_src + s, j])
                    if c >= 0:
                        l = clp[g * n_src + s, j]
                        cands.append((np.float32(cum[g, s] + l), s, c, l))
            cands.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
            for i, (sc, s, c, l) in enumerate(cands[:B]):
                tok[g, i], parent[g, i], lp[g, i], cum_out[g, i] = c, s, l, sc
            for s in range(n_src):
                eot_score[g, s] = np.float32(cum[g, s] + elp[g * n_src + s])
                eot_fin[g, s] = int(len(cands) < B or eot_score[g, s] > cum_out[g, B - 1])
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(tok), t(parent), t(lp), t(cum_out), t(eot_score), t(eot_fin)


class BeamState:
    """Host side of one beam search (one 30 s window): the live beams' tokens
    and log-probabilities, their cumulative scores (the next ``cum_in`` row) and
    the finished hypotheses, advanced by one ``beam_merge`` result per step.
    The first step has one source row (``n_src == 1``), later ones B."""

    def __init__(self, B: int, eot: int, max_new: int):
        self.B, self.eot, self.max_new = int(B), int(eot), int(max_new)
        self.beams = [([], [])]
        self.cum = np.full(self.B, -np.inf, np.float32)
        self.cum[0] = 0.0
        self.finished: list = []        # (tokens, sum_logprob, logprobs), EOT included
        # per beam / finished hypothesis, the source row that produced each token
        self.trace: list = [[]]
        self.finished_trace: list = []
        self.steps = 0
        self.done = self.max_new <= 0

    @property
    def n_src(self) -> int:
        return len(self.beams)

    def advance(self, tok, parent, lp, cum_out, eot_score, eot_fin, eot_lp) -> list:
        """One step's merge outputs (rows of length B; ``eot_lp``: n_src):
        EOT extensions that finish join ``finished`` best first until B are
        held, the selected extensions become the beams. Returns the new beams'
        parents. ``done``: B finished, ``max_new`` steps, or fewer than B
        extensions exist."""
        new = []
        for j, (t, l) in enumerate(self.beams):
            if int(eot_fin[j]) and float(eot_score[j]) > -np.inf:
                new.append((t + [self.eot], float(eot_score[j]), l + [float(eot_lp[j])]))
                new[-1] += (self.trace[j] + [j],)
        new.sort(key=lambda h: -h[1])       # stable: equal scores keep beam order
        for h in new:
            if len(self.finished) >= self.B:
                break
            self.finished.append(h[:3])
            self.finished_trace.append(h[3])
        live = [i for i in range(self.B) if int(tok[i]) >= 0]
        old = self.beams
        self.beams = [(old[int(parent[i])][0] + [int(tok[i])],
                       old[int(parent[i])][1] + [float(lp[i])]) for i in live]
        self.trace = [self.trace[int(parent[i])] + [int(parent[i])] for i in live]
        self.cum = np.asarray(cum_out, np.float32).copy()
        self.steps += 1
        self.done = len(self.finished) >= self.B or self.steps >= self.max_new or \
            len(live) < self.B
        return [int(parent[i]) for i in live]

    def result(self) -> tuple[list, int]:
        """(hypotheses, winner index): the finished hypotheses, filled up to B
        with the live beams in score order at their current sum; the winner
        maximises sum_logprob / max(1, tokens without EOT) (the first maximum)."""
        hyps = list(self.finished)
        self.result_trace = list(self.finished_trace)
        for i, (t, l) in enumerate(self.beams):
            if len(hyps) >= self.B:
                break
            hyps.append((list(t), float(self.cum[i]), list(l)))
            self.result_trace.append(list(self.trace[i]))
        score = [s / max(1, sum(1 for x in t if x != self.eot)) for t, s, _ in hyps]
        return hyps, (int(np.argmax(score)) if hyps else -1)


def beam_search(step_fn, B: int, eot: int, max_new: int, mask=None):
    """The whole search over ``step_fn(prefix) -> logits row [V]`` (``prefix``:
    the list of tokens sampled so far). Returns (hypotheses, winner index), a
    hypothesis = (tokens, sum_logprob, logprobs)."""
    st = BeamState(B, eot, max_new)
    while not st.done:
        rows = torch.stack([torch.as_tensor(step_fn(list(t))).float() for t, _ in st.beams])
        rm = None if mask is None else torch.zeros(len(rows), dtype=torch.int32)
        cid, clp, elp = beam_topk(rows, mask, rm, eot, B)
        out = beam_merge(cid, clp, elp, torch.from_numpy(st.cum)[None], st.n_src)
        st.advance(*(o[0].numpy() for o in out), elp.numpy())
    return st.result()


def kv_copy_blocks(k, v, pairs) -> None:
    """``k[:, dst] = k[:, src]`` (and ``v``) for every (src, dst) of ``pairs``;
    sources and destinations are disjoint (``check_copy_pairs``)."""
    if not len(pairs):
        return
    p = torch.as_tensor(pairs, dtype=torch.long, device=k.device).reshape(-1, 2)
    k[:, p[:, 1]] = k[:, p[:, 0]]
    v[:, p[:, 1]] = v[:, p[:, 0]]


def check_copy_pairs(pairs, num_blocks: int) -> np.ndarray:
    """``pairs`` as int32 [P, 2] (source block, destination block): every index
    inside the cache, no destination twice, no block both read and written."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    if p.size and (p.min() < 0 or p.max() >= num_blocks):
        raise ValueError(f"kv_copy_blocks: block index outside [0, {num_blocks})")
    if len(set(p[:, 1].tolist())) != len(p):
        raise ValueError("kv_copy_blocks: a destination block appears twice")
    if set(p[:, 0].tolist()) & set(p[:, 1].tolist()):
        raise ValueError("kv_copy_blocks: source and destination blocks overlap")
    return p.astype(np.int32)


def _pcm16_to_f32(pcm):
    """x / 32767 as the kernels compute it: one f32 multiply by the f32 nearest
    to 1 / 32767 (within one f32 ulp of the quotient; ``pcm.float() / 32767``
    differs from it in the last bit for 1536 of the 65536 values)."""
    return pcm.float() * torch.tensor(1.0 / 32767.0, dtype=torch.float32)


def pcm16_to_f32_sumsq(pcm, offsets):
    f = _pcm16_to_f32(pcm)
    off = offsets.tolist()
    ss = torch.tensor([float((f[off[i]:off[i + 1]].double() ** 2).sum()) for i in range(len(off) - 1)],
                      dtype=torch.float32)
    return f, ss


def pcm16_to_f32_padded(pcm, offsets, ld):
    """Segment s in row s of out [S, ld] (truncated to ``ld`` samples, +0.0
    beyond it) and the sum of squares of the kept samples."""
    off = offsets.tolist()
    S = len(off) - 1
    out = torch.zeros(S, ld, dtype=torch.float32)
    for i in range(S):
        n = min(off[i + 1] - off[i], ld)
        out[i, :n] = _pcm16_to_f32(pcm[off[i]:off[i] + n])
    return out, out.double().square().sum(1).float()


# ------------------------------------------------------ sample-rate conversion
# One filter definition for the kernel (csrc/kernels/resample.hip) and this
# reference: a Kaiser-windowed sinc, evaluated per output phase.
RESAMPLE_CUTOFF = 0.945     # of the lower Nyquist
RESAMPLE_ZEROS = 32         # sinc zero crossings per side
RESAMPLE_BETA = 12.0


def check_rate(rate) -> int:
    if rate not in RESAMPLE_RATES:
        raise ValueError(f"unsupported sample rate {rate}")
    return int(rate)


@functools.lru_cache(maxsize=None)
def resample_filter(rate_in: int, rate_out: int):
    """(table fp64 [L, T], L, M, T) of ``rate_in`` -> ``rate_out``: output n
    sits at source time n * M / L, base = n * M // L, phase = n * M % L and
    y[n] = sum_j x[base - H + j] * table[phase, j], H = (T - 1) // 2, where
    table[p, j] = h(p / L - (j - H)), h(tau) = c sinc(c tau) kaiser(tau / W; 12)
    for |tau| < W, c = 0.945 min(1, rate_out / rate_in), W = 32 / c. No
    per-phase renormalisation. The table is read-only (cached per pair)."""
    rate_in, rate_out = check_rate(rate_in), check_rate(rate_out)
    if rate_in == rate_out:                 # nothing to convert: the identity, one tap
        tab = np.ones((1, 1), np.float64)
        tab.setflags(write=False)
        return tab, 1, 1, 1
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    c = RESAMPLE_CUTOFF * min(1.0, rate_out / rate_in)
    W = RESAMPLE_ZEROS / c
    H = int(math.ceil(W))
    T = 2 * H + 1
    tau = np.arange(L, dtype=np.float64)[:, None] / L - (np.arange(T, dtype=np.float64)[None] - H)
    a2 = np.clip(1.0 - (tau / W) ** 2, 0.0, None)
    tab = c * np.sinc(c * tau) * np.i0(RESAMPLE_BETA * np.sqrt(a2)) / np.i0(RESAMPLE_BETA)
    tab[np.abs(tau) >= W] = 0.0
    tab.setflags(write=False)
    return tab, L, M, T


def resample_len(src_len: int, rate_in: int, rate_out: int) -> int:
    """Output samples of ``src_len`` source samples: ceil(src_len * L / M)."""
    _, L, M, _ = resample_filter(rate_in, rate_out)
    return -(-int(src_len) * L // M)


def resample(x, rate_in: int, rate_out: int, first: int = 0, count: int | None = None,
             table=None) -> np.ndarray:
    """fp64 resample of the 1-D signal ``x`` (zeros outside it): outputs
    [first, first + count) of its resample_len(len(x)) samples (default: all).
    ``table``: another [L, T] table of the pair (the kernel's f32-rounded one)."""
    tab, L, M, T = resample_filter(rate_in, rate_out)
    if table is not None:
        tab = np.asarray(table, np.float64)
    x = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
    n_all = -(-x.shape[0] * L // M)
    count = n_all - first if count is None else count
    assert first >= 0 and count >= 0 and first + count <= n_all
    out = np.zeros(count, np.float64)
    H = (T - 1) // 2
    step = max(1, (1 << 22) // T)                # bounds the gathered [step, T] block
    for o in range(0, count, step):
        t = (first + o + np.arange(min(step, count - o), dtype=np.int64)) * M
        base, phase = t // L, t % L
        lo, hi = int(base[0]) - H, int(base[-1]) + H + 1
        seg = np.zeros(hi - lo, np.float64)
        a, b = max(lo, 0), min(hi, x.shape[0])
        if b > a:
            seg[a - lo:b - lo] = x[a:b]
        idx = (base - base[0])[:, None] + np.arange(T)[None]
        out[o:o + t.shape[0]] = np.einsum("nt,nt->n", seg[idx], tab[phase])
    return out


def pcm16_resample_padded(pcm, rows, ld, rate_out: int = 16000):
    """The resampling sibling of ``pcm16_to_f32_padded``. ``rows``: one
    (src_first, src_len, out_first, out_len, rate_in) per output row - the
    utterance's samples pcm[src_first : src_first + src_len] at ``rate_in``,
    and the row's slice [out_first, out_first + out_len) of the utterance's
    resampled signal (a 30 s window of it). Returns (f32 [R, ld]: the slice
    * f32(1 / 32767), +0.0 beyond it; the rows' sums of squares [R])."""
    rows = [tuple(int(v) for v in r) for r in rows]
    scale = float(np.float32(1.0 / 32767.0))
    x = pcm.numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
    out = torch.zeros(len(rows), ld, dtype=torch.float32)
    for i, (s0, sn, o0, on, rate) in enumerate(rows):
        check_rate(rate)
        on = max(0, min(on, ld))
        if on:
            y = resample(x[s0:s0 + sn].astype(np.float64), rate, rate_out, o0, on)
            out[i, :on] = torch.from_numpy((y * scale).astype(np.float32))
    return out, out.double().square().sum(1).float()


def pcm16_resample(pcm, lens, rate_in: int, rate_out: int):
    """int16 [B, N] with lengths [B] -> (int16 [B, resample_len(N)], int32
    lengths [B]): the fp64 resample rounded to nearest even and saturated."""
    _, L, M, _ = resample_filter(rate_in, rate_out)
    x = pcm.numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
    n = np.clip(np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens, np.int64),
                0, x.shape[1])
    n_out = -(-n * L // M)
    out = np.zeros((x.shape[0], max(1, -(-x.shape[1] * L // M))), np.int16)
    for b in range(x.shape[0]):
        y = resample(x[b, :n[b]].astype(np.float64), rate_in, rate_out)
        out[b, :n_out[b]] = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    return torch.from_numpy(out), torch.from_numpy(n_out.astype(np.int32))


# ------------------------------------------------------------------------ FLAC
# Mono 16-bit FLAC with a fixed block size and the FIXED predictors only: the
# model of csrc/kernels/flac.hip, which must give these bytes. Every decision is
# integer arithmetic (docs/ARCHITECTURE.md "FLAC replies" states the rule).
FLAC_MAX_FRAMES = 65536          # frame numbers of at most 3 coded bytes
FLAC_HEADER_BYTES = 42           # "fLaC" + block header + STREAMINFO
_FLAC_RATE_CODE = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}


def flac_check(n_max: int, rate: int, block: int) -> int:
    """The checks made before any work; returns the frames of an ``n_max``-sample row."""
    check_rate(rate)
    if block not in FLAC_BLOCKS:
        raise ValueError(f"FLAC block size must be one of {FLAC_BLOCKS}, not {block}")
    if n_max < 0:
        raise ValueError(f"negative sample count {n_max}")
    frames = -(-int(n_max) // block)
    if frames > FLAC_MAX_FRAMES:
        raise ValueError(f"{frames} FLAC frames of {block} samples: more than {FLAC_MAX_FRAMES}")
    return frames


def flac_capacity(n_max: int, block: int) -> int:
    """Bytes that hold any stream of ``n_max`` samples: a VERBATIM frame is at
    most 2 n + 15 bytes (header <= 12, subframe byte, footer 2)."""
    return FLAC_HEADER_BYTES + -(-int(n_max) // block) * (2 * block + 15)


def _crc_table(poly: int, width: int) -> list:
    top, mask = 1 << (width - 1), (1 << width) - 1
    tab = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_CRC8_TAB = _crc_table(0x07, 8)
_CRC16_TAB = _crc_table(0x8005, 16)


def _flac_crc8(data) -> int:
    c = 0
    for b in data:
        c = _CRC8_TAB[c ^ b]
    return c


def _flac_crc16(data) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16_TAB[(c >> 8) ^ b]
    return c


def _flac_bits(values, width: int) -> np.ndarray:
    """The low ``width`` bits of each value, MSB first, as a flat 0/1 array."""
    v = np.atleast_1d(np.asarray(values, np.int64))
    return ((v[:, None] >> np.arange(width - 1, -1, -1)) & 1).astype(np.uint8).ravel()


def flac_frame_plan(x) -> tuple:
    """The selection rule for one block of samples: ("constant",), ("verbatim",)
    or ("fixed", order, partition order, [k per partition])."""
    x = np.asarray(x, np.int64)
    n = x.shape[0]
    if (x == x[0]).all():
        return ("constant",)
    omax = min(4, n - 1)
    res = [x]
    for _ in range(omax):
        res.append(np.diff(res[-1]))
    # E_o over the samples every order predicts, i = omax .. n-1
    err = [int(np.abs(res[o][omax - o:]).sum()) for o in range(omax + 1)]
    o = int(np.argmin(err))
    r = res[o]
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    pad = np.concatenate([np.zeros(o, np.int64), u])        # zeros add nothing to a sum
    best = None
    for p in range(9):
        if n % (1 << p) or (n >> p) <= o:
            continue
        parts = pad.reshape(1 << p, n >> p)
        cnt = np.full(1 << p, n >> p, np.int64)
        cnt[0] -= o
        ks = np.arange(15, dtype=np.int64)
        cost = cnt[:, None] * (ks + 1)[None] + (parts[:, :, None] >> ks).sum(1)
        k = cost.argmin(1)                                   # the lowest k on ties
        bits = int((4 + cost[np.arange(1 << p), k]).sum())
        if best is None or bits < best[0]:
            best = (bits, p, k)
    bits, p, k = best
    if 16 * o + 6 + bits >= 16 * n:
        return ("verbatim",)
    return ("fixed", o, p, [int(v) for v in k])


def _flac_frame(x: np.ndarray, number: int, rate: int, block: int) -> bytes:
    n = x.shape[0]
    hdr = bytearray(b"\xff\xf8")
    if n == block:
        size_code, size_extra = 8 + FLAC_BLOCKS.index(block), b""
    elif n <= 256:
        size_code, size_extra = 6, bytes([n - 1])
    else:
        size_code, size_extra = 7, (n - 1).to_bytes(2, "big")
    rate_code = _FLAC_RATE_CODE.get(rate, 13)
    hdr.append(size_code << 4 | rate_code)
    hdr.append(0x08)                                         # mono, 16 bits
    if number < 0x80:
        hdr.append(number)
    elif number < 0x800:
        hdr += bytes([0xC0 | number >> 6, 0x80 | number & 0x3F])
    else:
        hdr += bytes([0xE0 | number >> 12, 0x80 | (number >> 6) & 0x3F, 0x80 | number & 0x3F])
    hdr += size_extra
    if rate_code == 13:
        hdr += rate.to_bytes(2, "big")
    hdr.append(_flac_crc8(hdr))

    plan = flac_frame_plan(x)
    if plan[0] == "constant":
        bits = [_flac_bits(0, 8), _flac_bits(x[0], 16)]
    elif plan[0] == "verbatim":
        bits = [_flac_bits(1 << 1, 8), _flac_bits(x, 16)]
    else:
        _, o, p, ks = plan
        r = np.diff(x, o) if o else x
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        bits = [_flac_bits((8 | o) << 1, 8), _flac_bits(x[:o], 16), _flac_bits(p, 6)]
        first = 0
        for j, k in enumerate(ks):
            cnt = (n >> p) - (o if j == 0 else 0)
            v = u[first:first + cnt]
            first += cnt
            q = v >> k
            end = np.cumsum(q + 1 + k)
            code = np.zeros(int(end[-1]) if cnt else 0, np.uint8)
            one = end - k - 1
            code[one] = 1
            for b in range(k):
                code[one + 1 + b] = (v >> (k - 1 - b)) & 1
            bits += [_flac_bits(k, 4), code]
    body = np.concatenate(bits)
    body = np.packbits(np.concatenate([body, np.zeros(-body.shape[0] % 8, np.uint8)])).tobytes()
    frame = bytes(hdr) + body
    return frame + _flac_crc16(frame).to_bytes(2, "big")


def flac_encode(pcm_rows, lens, rate: int, block: int = 4096) -> list:
    """int16 rows [R, N] holding ``lens`` [R] samples (clamped to [0, N]) at
    ``rate`` -> one FLAC stream (bytes) per row: mono, 16 bits, ``block``
    samples per frame, CONSTANT / VERBATIM / FIXED subframes by the rule of
    ``flac_frame_plan``. The CPU path of ``ops.flac_encode`` and the arbiter of
    its kernel."""
    x = pcm_rows.cpu().numpy() if isinstance(pcm_rows, torch.Tensor) else np.asarray(pcm_rows)
    assert x.ndim == 2 and x.dtype == np.int16
    flac_check(x.shape[1], rate, block)
    n_all = np.clip(np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens, np.int64),
                    0, x.shape[1])
    out = []
    for row, n in zip(x, n_all):
        n = int(n)
        frames = [_flac_frame(row[f:min(f + block, n)].astype(np.int64), f // block, rate, block)
                  for f in range(0, n, block)]
        sizes = [len(f) for f in frames]
        info = (block.to_bytes(2, "big") * 2 + (min(sizes) if sizes else 0).to_bytes(3, "big")
                + (max(sizes) if sizes else 0).to_bytes(3, "big")
                + (rate << 44 | 0 << 41 | 15 << 36 | n).to_bytes(8, "big") + bytes(16))
        out.append(b"fLaC\x80\x00\x00\x22" + info + b"".join(frames))
    return out


def flac_info(data: bytes) -> tuple:
    """(sample_rate, n_samples) of a FLAC stream, read from STREAMINFO."""
    if data[:4] != b"fLaC" or data[4] & 0x7F != 0:
        raise ValueError("not a FLAC stream that starts with STREAMINFO")
    v = int.from_bytes(data[18:26], "big")
    return v >> 44, v & ((1 << 36) - 1)


class _FlacReader:
    """MSB-first bit reader of the decoder."""

    def __init__(self, data: bytes, pos: int):
        self.data, self.pos = data, pos * 8

    def read(self, width: int) -> int:
        if self.pos + width > len(self.data) * 8:
            raise ValueError("FLAC stream ends inside a frame")
        a, b = self.pos >> 3, (self.pos + width + 7) >> 3
        v = int.from_bytes(self.data[a:b], "big") >> (b * 8 - self.pos - width)
        self.pos += width
        return v & ((1 << width) - 1)

    def signed(self, width: int) -> int:
        v = self.read(width)
        return v - (1 << width) if v >> (width - 1) else v

    def unary(self) -> int:
        q = 0
        while True:                       # whole zero bytes first, then bit by bit
            if self.pos & 7 == 0 and self.pos >> 3 < len(self.data) and not self.data[self.pos >> 3]:
                q, self.pos = q + 8, self.pos + 8
            elif self.read(1):
                return q
            else:
                q += 1


def flac_decode(data: bytes) -> tuple:
    """FLAC stream -> (int16 [channels, n], sample_rate). Its own code, none of
    the encoder's: it checks each frame's CRC-8 and CRC-16, that the frame
    numbers count 0, 1, 2, ... and that the stream ends with its last frame.
    It reads what ``flac_encode`` writes (fixed block size, CONSTANT / VERBATIM /
    FIXED subframes, 4-bit Rice parameters) and also wasted bits and two
    independent channels."""
    rate_info, total = flac_info(data)
    if data[4] != 0x80 or int.from_bytes(data[5:8], "big") != 34:
        raise ValueError("FLAC metadata other than one STREAMINFO block")
    info_bits = (int.from_bytes(data[18:26], "big") >> 36) & 0xFF
    channels_info, bps_info = (info_bits >> 5) + 1, (info_bits & 31) + 1
    rates = {4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000}
    sizes = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}
    chans: list = [[] for _ in range(channels_info)]
    pos, expect = FLAC_HEADER_BYTES, 0
    while pos < len(data):
        rd = _FlacReader(data, pos)
        if rd.read(15) != 0x7FFC:
            raise ValueError(f"no frame sync at byte {pos}")
        if rd.read(1):
            raise ValueError("variable block size streams are not supported")
        size_code, rate_code = rd.read(4), rd.read(4)
        assign, bps_code, reserved = rd.read(4), rd.read(3), rd.read(1)
        if reserved or assign not in (0, 1) or assign + 1 != channels_info:
            raise ValueError(f"channel assignment {assign} not supported")
        lead = rd.read(8)                                  # the coded frame number
        extra = 0 if lead < 0x80 else 1 if lead >> 5 == 6 else 2 if lead >> 4 == 14 else None
        if extra is None:
            raise ValueError("frame number longer than 3 bytes")
        number = lead if not extra else lead & (0x1F >> (extra - 1))
        for _ in range(extra):
            cont = rd.read(8)
            if cont >> 6 != 2:
                raise ValueError("bad frame number continuation byte")
            number = number << 6 | cont & 0x3F
        if number != expect:
            raise ValueError(f"frame number {number}, expected {expect}")
        expect += 1
        if size_code == 6:
            n = rd.read(8) + 1
        elif size_code == 7:
            n = rd.read(16) + 1
        elif size_code >= 8:
            n = 256 << (size_code - 8)
        else:
            raise ValueError(f"block size code {size_code} not supported")
        rate = rd.read(16) if rate_code == 13 else rate_info if rate_code == 0 else rates[rate_code]
        if rate != rate_info:
            raise ValueError("frame sample rate differs from STREAMINFO")
        bps = bps_info if bps_code == 0 else sizes[bps_code]
        head_end = rd.pos >> 3
        crc = 0
        for byte in data[pos:head_end]:                    # bitwise, unlike the encoder's table
            crc ^= byte
            for _ in range(8):
                crc = (crc << 1 ^ 0x07) & 0xFF if crc & 0x80 else crc << 1
        if crc != rd.read(8):
            raise ValueError(f"CRC-8 mismatch in frame {number}")
        for ch in range(channels_info):
            if rd.read(1):
                raise ValueError("subframe padding bit set")
            kind, wasted = rd.read(6), rd.read(1)
            if wasted:
                wasted = rd.unary() + 1
            width = bps - wasted
            if kind == 0:
                s = np.full(n, rd.signed(width), np.int64)
            elif kind == 1:
                s = np.array([rd.signed(width) for _ in range(n)], np.int64)
            elif 8 <= kind <= 12:
                o = kind - 8
                warm = np.array([rd.signed(width) for _ in range(o)], np.int64)
                if rd.read(2) != 0:
                    raise ValueError("only 4-bit Rice parameters are supported")
                p = rd.read(4)
                if n % (1 << p) or (n >> p) < o:
                    raise ValueError("partition order does not fit the block")
                r = []
                for j in range(1 << p):
                    k = rd.read(4)
                    if k == 15:
                        raise ValueError("escaped partitions are not supported")
                    for _ in range((n >> p) - (o if j == 0 else 0)):
                        v = rd.unary() << k | (rd.read(k) if k else 0)
                        r.append(-(v >> 1) - 1 if v & 1 else v >> 1)
                s = np.asarray(r, np.int64)
                for j in range(o - 1, -1, -1):              # undo one difference per pass
                    start = np.diff(warm, j)[-1] if j else warm[-1]
                    s = start + np.cumsum(s)
                s = np.concatenate([warm, s])
            else:
                raise ValueError(f"subframe type {kind} not supported")
            chans[ch].append(s << wasted)
        rd.pos = (rd.pos + 7) & ~7
        end = rd.pos >> 3
        crc = 0
        for byte in data[pos:end]:
            crc ^= byte << 8
            for _ in range(8):
                crc = (crc << 1 ^ 0x8005) & 0xFFFF if crc & 0x8000 else crc << 1
        if crc != rd.read(16):
            raise ValueError(f"CRC-16 mismatch in frame {number}")
        pos = end + 2
    out = np.stack([np.concatenate(c) if c else np.zeros(0, np.int64) for c in chans])
    if out.shape[1] != total:
        raise ValueError(f"{out.shape[1]} samples decoded, STREAMINFO says {total}")
    if out.size and (out.min() < -32768 or out.max() > 32767):
        raise ValueError("decoded sample outside 16 bits")
    return out.astype(np.int16), rate_info


# ------------------------------------------------------------- log-mel consts
def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    freqs = f_sp * m
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), freqs)


def mel_filterbank(sr: int = 16000, n_fft: int = 400, n_mels: int = 80) -> np.ndarray:
    """Slaney-style mel filterbank (librosa defaults, as whisper uses)."""
    n_freqs = 1 + n_fft // 2
    fftfreqs = np.linspace(0, sr / 2, n_freqs)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels])
    return (w * enorm[:, None]).astype(np.float32)


@dataclass
class MelConstants:
    n_mels: int
    window: torch.Tensor      # [400]
    cos_basis: torch.Tensor   # [400, 224]
    sin_basis: torch.Tensor   # [400, 224]
    filters: torch.Tensor     # [n_mels, 201]

    @staticmethod
    def create(n_mels: int = 80) -> "MelConstants":
        n = np.arange(400)
        window = (0.5 - 0.5 * np.cos(2 * np.pi * n / 400)).astype(np.float32)  # periodic Hann
        k = np.arange(224)
        ang = 2 * np.pi * np.outer(n, k) / 400
        cosb = np.cos(ang)
        sinb = -np.sin(ang)
        cosb[:, 201:] = 0
        sinb[:, 201:] = 0
        return MelConstants(n_mels, torch.from_numpy(window), torch.from_numpy(cosb.astype(np.float32)),
                            torch.from_numpy(sinb.astype(np.float32)),
                            torch.from_numpy(mel_filterbank(n_mels=n_mels)))

    def to(self, device) -> "MelConstants":
        device = torch.device(device)
        if self.window.device == device:
            return self
        cache = self.__dict__.setdefault("_dev_cache", {})
        key = str(device)
        if key not in cache:
            cache[key] = MelConstants(self.n_mels, self.window.to(device), self.cos_basis.to(device),
                                      self.sin_basis.to(device), self.filters.to(device))
        return cache[key]


def log_mel_db(audio: torch.Tensor, c: MelConstants) -> torch.Tensor:
    """log10 of the clamped mel power spectrum in fp32, before Whisper's
    max - 8 floor and scaling: [B, n_mels, n//160]."""
    win = c.window.to(audio.device)
    st = torch.stft(audio.float(), 400, 160, window=win, return_complex=True, center=True,
                    pad_mode="reflect")
    mag = st[..., :-1].abs() ** 2
    mel = c.filters.to(audio.device) @ mag
    return torch.clamp(mel, min=1e-10).log10()


def log_mel(audio: torch.Tensor, c: MelConstants) -> torch.Tensor:
    """Whisper log-mel (whisper/audio.py semantics) in fp32: [B, n_mels, n//160]."""
    lg = log_mel_db(audio, c)
    mx = lg.amax(dim=(-2, -1), keepdim=True)
    lg = torch.maximum(lg, mx - 8.0)
    return (lg + 4.0) / 4.0


def im2col_k3(x, strides, B, C, L, stride):
    Lout = (L - 1) // stride + 1
    flat = x.reshape(-1)
    b = torch.arange(B, device=x.device)[:, None, None, None]
    to = torch.arange(Lout, device=x.device)[None, :, None, None]
    c = torch.arange(C, device=x.device)[None, None, :, None]
    k = torch.arange(3, device=x.device)[None, None, None, :]
    t = to * stride + k - 1
    valid = (t >= 0) & (t < L)
    idx = b * strides[0] + c * strides[1] + t.clamp(0, L - 1) * strides[2]
    vals = flat[idx.reshape(-1)].reshape(B, Lout, C, 3)
    vals = torch.where(valid.expand(B, Lout, C, 3), vals, torch.zeros((), dtype=x.dtype))
    return vals.reshape(B * Lout, 3 * C)


# ----------------------------------------------------------- decode slabs
def shuffle_weight(w):
    N, K = w.shape
    return w.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(
        N // 16, K // 32, 64, 8)


FP8_MAX = 448.0   # largest finite e4m3fn value


def quantize_fp8_rows(w):
    """Per-row e4m3fn quantisation of w [N, K]: (q float8_e4m3fn [N, K], scale
    f32 [N]) with scale = amax(|row|) / 448 (1 for an all-zero row) and
    w ~ q * scale. Clamped before the cast: torch's cast does not saturate."""
    wf = w.float()
    amax = wf.abs().amax(1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q, scale


def shuffle_fp8(q):
    """e4m3 bytes [N, K] (uint8) -> fragment order [N/16, K/64, 64, 16]: lane l
    holds row (l & 15); bytes 0-7 the 8 k values at offset 8 * (l >> 4) of
    k-step 2j, bytes 8-15 the same of k-step 2j + 1."""
    N, K = q.shape
    return q.reshape(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous().reshape(
        N // 16, K // 64, 64, 16)


def unshuffle_fp8(wp):
    T, KP = wp.shape[:2]
    return wp.reshape(T, KP, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(T * 16, KP * 64)


def dequant_fp8(weight):
    """f32 [N, K] = e4m3 * scale of an fp8 weight container (``ops.Fp8Weight``:
    ``wp`` uint8 in fragment order, ``scale`` f32 [N])."""
    q = unshuffle_fp8(weight.wp).contiguous().view(torch.float8_e4m3fn)
    return q.float() * weight.scale.float()[:, None]


E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # code & 7 -> magnitude; bit 3 is the sign
MXFP4_BLOCK = 32                   # k values per e8m0 scale: one MFMA k-step
# e8m0 scale bytes the quantiser emits: 2^(b - 127) for b in [2, 252], so the
# smallest non-zero product 0.5 * 2^-125 and the largest 6 * 2^125 are normal
# bf16 values. (0 shifted into an f32 exponent is 0.0, not 2^-127; 255 is NaN.)
MXFP4_SCALE_MIN, MXFP4_SCALE_MAX = 2, 252


def quantize_mxfp4_rows(w):
    """OCP MXFP4 quantisation of w [N, K] (K % 32 == 0): (codes uint8 [N, K],
    one e2m1 code 0..15 per element; scales uint8 [N, K/32], e8m0). Per block
    of 32 the scale is the smallest power of two with amax / scale <= 6 (nothing
    clips; 1 for an all-zero block, whose codes are +0), its exponent clamped to
    [-125, 125]; elements round to the nearest grid point, ties to the even
    code."""
    N, K = w.shape
    wf = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(2)
    # amax = m * 2^e with m in [0.5, 1): amax / 2^(e - 2) = 4m in [2, 4) <= 6, and
    # one power less (8m) fits only while m <= 0.75
    m, e = torch.frexp(amax)
    e = torch.where(m <= 0.75, e - 3, e - 2)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(MXFP4_SCALE_MIN - 127, MXFP4_SCALE_MAX - 127)
    v = (wf * torch.exp2(-e.float())[..., None]).abs().clamp(max=6.0)   # exact: a power of two
    # round to nearest on {0, .5, 1, 1.5 | 2, 3 | 4, 6}: the spacing doubles at 2
    # and at 4; torch.round is half-to-even, and an even multiple of the
    # spacing is an even code in each segment
    step = torch.where(v < 2, torch.full_like(v, 0.5), torch.where(v < 4, torch.ones_like(v),
                                                                    torch.full_like(v, 2.0)))
    r = torch.round(v / step) * step
    grid = torch.tensor(E2M1_GRID, device=w.device)
    code = torch.bucketize(r, grid).to(torch.uint8)         # r is a grid point: its index
    code = code | ((wf < 0) & (r > 0)).to(torch.uint8) << 3
    return code.reshape(N, K), (e + 127).to(torch.uint8)


def shuffle_mxfp4(code, scales):
    """codes [N, K] and e8m0 bytes [N, K/32] -> (wp uint8 [N/16, K/128, 64, 16],
    ws uint8 [N/16, K/128, 16, 4]) in the kernels' order: lane l holds row
    (l & 15); its bytes 4j..4j+3 are the 8 k values at offset 8 * (l >> 4) of
    k-step 4g + j, ascending, two per byte with the even k in the low nibble.
    ws[t, g, r, j] is the scale of row 16 t + r, k-step 4g + j."""
    N, K = code.shape
    b = code.reshape(N, K // 2, 2)
    b = b[..., 0] | (b[..., 1] << 4)                                   # [N, K/2]
    wp = b.reshape(N // 16, 16, K // 128, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).contiguous().reshape(
        N // 16, K // 128, 64, 16)
    ws = scales.reshape(N // 16, 16, K // 128, 4).permute(0, 2, 1, 3).contiguous()
    return wp, ws


def unshuffle_mxfp4(wp, ws):
    """Inverse of ``shuffle_mxfp4``: (codes uint8 [N, K], scales uint8 [N, K/32])."""
    T, G = wp.shape[:2]
    b = wp.reshape(T, G, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(T * 16, G * 64)
    code = torch.stack([b & 15, b >> 4], -1).reshape(T * 16, G * 128)
    return code, ws.permute(0, 2, 1, 3).reshape(T * 16, G * 4)


def dequant_mxfp4(weight):
    """f32 [N, K] = e2m1 * 2^(e8m0 - 127) of an MXFP4 weight container
    (``ops.Mxfp4Weight``), by table: what the kernels' in-register convert
    must reproduce bit for bit."""
    code, sc = unshuffle_mxfp4(weight.wp, weight.scales)
    grid = torch.tensor(E2M1_GRID + tuple(-g for g in E2M1_GRID), device=code.device)
    v = grid[code.long()]
    return v * torch.exp2(sc.float() - 127.0).repeat_interleave(MXFP4_BLOCK, 1)


def unshuffle_weight(wp):
    if hasattr(wp, "scales"):     # MXFP4 container: the dequantised rows (f32)
        return dequant_mxfp4(wp)
    if hasattr(wp, "scale"):      # fp8 container: the dequantised rows (f32)
        return dequant_fp8(wp)
    T, KS = wp.shape[:2]
    return wp.reshape(T, KS, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(T * 16, KS * 32)


def skinny_gemm(x, wp, S):
    w = unshuffle_weight(wp)
    Mpad, K = x.shape
    kc = K // S
    parts = [x[:, s * kc:(s + 1) * kc].float() @ w[:, s * kc:(s + 1) * kc].float().t() for s in range(S)]
    return torch.stack(parts, 0)


def slab_rmsnorm(part, residual, w, eps, row_idx=None, write_residual=True):
    tot = part.sum(0)
    idx = row_idx.long() if row_idx is not None else torch.arange(part.shape[1], device=part.device)
    s = (tot[idx] + residual[idx].float()).to(residual.dtype)
    if write_residual:
        residual[idx] = s
    xf = s.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return y.to(residual.dtype)


def slab_rope_append(part, positions, cos_sin, k_cache, v_cache, slots, H, Hkv, D, bias=None):
    tot = part.sum(0)
    if bias is not None:
        tot = tot + bias.float()
    qkv = tot.to(torch.bfloat16)
    rope_kv_append(qkv, positions, cos_sin, k_cache, v_cache, slots, H, Hkv, D)
    return qkv[:, : H * D].contiguous()


def slab_layernorm(part, residual, w, b, eps, bias=None, row_idx=None, write_residual=True):
    tot = part.sum(0)
    if bias is not None:
        tot = tot + bias.float()
    tot = tot.to(torch.bfloat16).float()
    idx = row_idx.long() if row_idx is not None else torch.arange(part.shape[1], device=part.device)
    s = (tot[idx] + residual[idx].float()).to(residual.dtype)
    if write_residual:
        residual[idx] = s
    return torch.nn.functional.layer_norm(s.float(), (s.shape[-1],), w.float(), b.float(),
                                          eps).to(residual.dtype)


def slab_bias_act(part, bias=None, act="none"):
    tot = part.sum(0)
    if bias is not None:
        tot = tot + bias.float()
    if act == "gelu":
        tot = torch.nn.functional.gelu(tot.to(torch.bfloat16).float())
    return tot.to(torch.bfloat16)


def slab_silu_mul(part):
    return silu_mul(part.sum(0).to(torch.bfloat16))


# ------------------------------------------------------------------ VITS / HiFi-GAN
def conv1d(x, w, bias=None, *, dil=1, pad=0, stride=1, pre_slope=None, act=None, res=None,
           alpha=1.0, acc=None, lens=None, Tout=None, ostride=1, ophase=0, Tq=None):
    """Reference of loqa_conv1d: x [B, Tin, Cin] (channels-last), w [Cout, Cin, K]
    (torch layout) -> y [B, Tout, Cout'] following the kernel's epilogue order.
    Returns float32 (callers round)."""
    B, Tin, Cin = x.shape
    xf = x.float()
    if pre_slope is not None:
        xf = torch.nn.functional.leaky_relu(xf, pre_slope)
    xf = xf.to(torch.bfloat16).float()  # the kernel feeds bf16 operands to the MFMA
    y = torch.nn.functional.conv1d(xf.transpose(1, 2), w.float(), None, stride=stride, padding=pad,
                                   dilation=dil).transpose(1, 2)
    if Tq is not None:
        y = y[:, :Tq]
    if bias is not None:
        y = y + bias.float()
    if act == "relu":
        y = torch.relu(y)
    elif act == "tanh":
        y = torch.tanh(y)
    elif act == "gated":
        Hh = y.shape[-1] // 2
        a, g = y[..., :Hh].to(torch.bfloat16).float(), y[..., Hh:].to(torch.bfloat16).float()
        y = torch.tanh(a) * torch.sigmoid(g)
    T_out = Tout if Tout is not None else y.shape[1] * ostride + ophase
    full = torch.zeros(B, T_out, y.shape[-1], dtype=torch.float32, device=x.device)
    q = torch.arange(y.shape[1], device=x.device)
    oi = q * ostride + ophase
    ok = (oi >= 0) & (oi < T_out)
    full[:, oi[ok]] = y[:, q[ok]]
    idx = oi[ok]
    if res is not None:
        full[:, idx] += res[:, idx].float()
    full[:, idx] *= alpha
    if acc is not None:
        full[:, idx] += acc[:, idx].float()
    if lens is not None:
        t = torch.arange(T_out, device=x.device)
        # a select, not a multiply: rows past lens are 0 whatever res / acc hold there
        full = full.masked_fill((t[None, :] >= lens[:, None].to(x.device))[..., None], 0.0)
    return full


def conv_transpose1d(x, w, bias=None, *, stride, padding, pre_slope=None):
    """torch ConvTranspose1d on channels-last x; w [Cin, Cout, K] torch layout."""
    xf = x.float()
    if pre_slope is not None:
        xf = torch.nn.functional.leaky_relu(xf, pre_slope)
    xf = xf.to(torch.bfloat16).float()
    y = torch.nn.functional.conv_transpose1d(xf.transpose(1, 2), w.float(),
                                             None if bias is None else bias.float(),
                                             stride=stride, padding=padding)
    return y.transpose(1, 2)


def relpos_attention(qkv, emb_k, emb_v, lens, H, D, window, scale):
    B, T, _ = qkv.shape
    C = H * D
    idx = torch.arange(T, device=qkv.device)
    L = lens.to(qkv.device) if lens is not None else torch.full((B,), T, device=qkv.device)
    valid = idx[None, :] < L[:, None]
    # rows at or past lens[b] are never read: whatever they hold (NaN too) stays out
    qkv = torch.where(valid[..., None], qkv, torch.zeros((), dtype=qkv.dtype, device=qkv.device))
    q = qkv[..., :C].float().view(B, T, H, D).transpose(1, 2) * scale
    k = qkv[..., C:2 * C].float().view(B, T, H, D).transpose(1, 2)
    v = qkv[..., 2 * C:3 * C].float().view(B, T, H, D).transpose(1, 2)
    s = q @ k.transpose(-1, -2)
    rel = idx[None, :] - idx[:, None]
    inwin = rel.abs() <= window
    ek = emb_k.float()
    rl = torch.einsum("bhid,rd->bhir", q, ek)  # [B,H,T,2w+1]
    ridx = (rel + window).clamp(0, 2 * window)
    s = s + torch.where(inwin, rl.gather(-1, ridx[None, None].expand(B, H, T, T)),
                        torch.zeros((), device=qkv.device))
    m = valid[:, None, :, None] & valid[:, None, None, :]
    s = s.masked_fill(~m, -1e4)
    p = torch.softmax(s, -1)
    o = p @ v
    pw = torch.where(inwin, p, torch.zeros((), device=qkv.device))
    pr = torch.zeros(B, H, T, 2 * window + 1, device=qkv.device)
    pr.scatter_add_(-1, ridx[None, None].expand(B, H, T, T), pw)
    o = o + pr @ emb_v.float()
    o = torch.where(valid[:, None, :, None], o, torch.zeros((), device=qkv.device))     # +0.0, never -0.0
    return o.transpose(1, 2).reshape(B, T, C)


def expand_sample(stats, cum, flen, F, noise_scale, noise=None):
    """z[b, f] = m[i(f)] + noise * exp(logs[i(f)]) * noise_scale."""
    B, T, C2 = stats.shape
    C = C2 // 2
    z = torch.zeros(B, F, C, device=stats.device)
    for b in range(B):
        n = int(flen[b])
        f = torch.arange(n, device=stats.device)
        i = torch.searchsorted(cum[b].to(stats.device), f, right=True)
        m, lg = stats[b, i, :C].float(), stats[b, i, C:].float()
        e = noise[b, :n].float() if noise is not None else torch.zeros_like(m)
        z[b, :n] = m + e * torch.exp(lg) * noise_scale
    return z


def hash32(x: np.ndarray) -> np.ndarray:
    """The integer mixer of ``expand_sample`` (tts.hip ``hash32``), uint32."""
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def gauss_uniforms(seed: int, B: int, F: int, C: int):
    """The integer part of the device noise of ``expand_sample``, exactly:
    ``(a, u1, u2)`` [B, F, C] - the first hash (uint32) and the two f32
    uniforms, ``u1`` in (0, 1], ``u2`` in [0, 1). The noise of (row, frame,
    channel) does not depend on B or F."""
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    f = np.arange(F, dtype=np.uint64)[None, :, None]
    c = np.arange(C, dtype=np.uint64)[None, None, :]
    idx = ((b << np.uint64(24)) + f) * np.uint64(C) + c
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    a = hash32(np.uint32(seed & 0xFFFFFFFF) ^ hash32(lo ^ np.uint32(0x9E3779B9)) ^ hi)
    c2 = hash32(a ^ np.uint32(0x85EBCA6B))
    # 1.0f / 16777217.0f: the divisor is no f32 and rounds to 2**24
    u1 = ((a >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = (c2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return a, u1, u2


def gauss_noise(seed: int, B: int, F: int, C: int) -> np.ndarray:
    """Host model of the device noise of ``expand_sample`` [B, F, C], fp64:
    the hashes and both uniforms bit for bit, Box-Muller in fp64 from them."""
    _, u1, u2 = gauss_uniforms(seed, B, F, C)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


# ------------------------------------------------------------ fused decode GEMMs
def perm_rope_qkv(H, Hkv, D):
    """Row order of the fused qkv weight: per q / k head, 16-row pair tiles
    holding 8 first-half rows c0.. and their RoPE partners c0 + D/2 (the
    epilogue pairs lane l with lane l ^ 32); v rows unchanged."""
    half = D // 2
    rows = []
    for base, n in ((0, H), (H * D, Hkv)):
        for h in range(n):
            for s in range(D // 16):
                c0 = 8 * s
                rows += list(range(base + h * D + c0, base + h * D + c0 + 8))
                rows += list(range(base + h * D + half + c0, base + h * D + half + c0 + 8))
    rows += list(range((H + Hkv) * D, (H + 2 * Hkv) * D))
    return torch.tensor(rows, dtype=torch.long)


def perm_gate_up(F):
    """Row order of the fused gate|up weight: 16-row pair tiles of (8 gate, 8 up)."""
    rows = []
    for t in range(F // 8):
        rows += list(range(8 * t, 8 * t + 8)) + list(range(F + 8 * t, F + 8 * t + 8))
    return torch.tensor(rows, dtype=torch.long)


def swiglu_pairs(y):
    """silu(gate) * up of a ``perm_gate_up``-ordered product [M, 2F] (16-column
    pair tiles: 8 gate, 8 up) -> [M, F] (f32)."""
    M, F2 = y.shape
    t = y.float().view(M, F2 // 16, 2, 8)
    g, u = t[:, :, 0], t[:, :, 1]
    g = g.to(torch.bfloat16).float()
    u = u.to(torch.bfloat16).float()
    return (torch.nn.functional.silu(g) * u).reshape(M, F2 // 2)


def fused_ln_stats(rowsq_in, rowsum_in, eps, K):
    """LayerNorm (mean, 1/std) per row from per-tile partial sums [tiles, Mpad]."""
    mean = rowsum_in.float().sum(0) / K
    var = (rowsq_in.float().sum(0) / K - mean * mean).clamp_min(0.0)
    return mean, torch.rsqrt(var + eps)


def fused_row_scale(rowsq_in, eps, K):
    """RMSNorm row scale 1/rms from per-tile partial sums of squares [tiles, Mpad]."""
    tot = rowsq_in.float().sum(0)  # [Mpad]
    return torch.rsqrt(tot / K + eps)


def _fmix32(h: torch.Tensor) -> torch.Tensor:
    m = 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & m
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def init_uniform4(rows: int, cols: int, ld: int, row0: int, col0: int, s: int,
                  scale: float) -> torch.Tensor:
    """CPU twin of elementwise.hip ``init_uniform4_kernel``: bf16 [rows, cols],
    element (r, c) = scale * (sum_k fmix32(4 idx + k + s) / 2^32 - 2) with
    idx = (row0 + r) * ld + col0 + c (uint32 arithmetic, exact f32 sums)."""
    r = torch.arange(rows, dtype=torch.int64)[:, None] + row0
    c = torch.arange(cols, dtype=torch.int64)[None, :] + col0
    idx = (r * ld + c) & 0xFFFFFFFF
    acc = torch.zeros(rows, cols, dtype=torch.float32)
    for k in range(4):
        h = _fmix32((idx * 4 + k + s) & 0xFFFFFFFF)
        acc += (h >> 8).to(torch.float32) * (1.0 / 16777216.0)
    return ((acc - 2.0) * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16)


# ------------------------------------------------------------ whole models
def _causal_attn(q, k, v, G: int, scale: float, q0: int = 0):
    """q [T, H, D], k / v [L, Hkv, D] (fp32); query i sits at position q0 + i."""
    k = k.repeat_interleave(G, dim=1)
    v = v.repeat_interleave(G, dim=1)
    s = torch.einsum("qhd,khd->hqk", q, k) * scale
    qpos = torch.arange(q.shape[0], device=q.device) + q0
    kpos = torch.arange(k.shape[0], device=q.device)
    s = s.masked_fill(kpos[None, None, :] > qpos[None, :, None], float("-inf"))
    return torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v)


@torch.no_grad()
def llama_forward_ref(w, tokens: list[int]) -> torch.Tensor:
    """fp32 forward of a whole Llama model (``LlamaWeights``, unsharded, with
    its row-major layer copies) over one sequence at positions 0..T-1; returns
    fp32 logits [T, V]. Every weight is the model's own bf16 tensor upcast:
    the oracle of the fused bf16 decode path (tests/test_engine_gpu.py)."""
    cfg = w.cfg
    H, Hkv, D, F = w.h, w.hkv, cfg.head_dim, w.f
    dev = w.embed.device
    t = torch.tensor(tokens, dtype=torch.long, device=dev)
    T = t.numel()
    cs = w.cos_sin[:T].float()

    def rms(x, g):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.norm_eps) * g.float()
    x = w.embed[t].float()
    for L in w.layers:
        h = rms(x, L["attn_norm"])
        qkv = h @ L["wqkv"].float().t()
        q = apply_rope(qkv[:, : H * D].view(T, H, D), cs)
        k = apply_rope(qkv[:, H * D:(H + Hkv) * D].view(T, Hkv, D), cs)
        v = qkv[:, (H + Hkv) * D:].view(T, Hkv, D)
        a = _causal_attn(q, k, v, H // Hkv, 1.0 / math.sqrt(D)).reshape(T, H * D)
        x = x + a @ L["wo"].float().t()
        gu = rms(x, L["mlp_norm"]) @ L["w_gate_up"].float().t()
        x = x + (torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]) @ L["w_down"].float().t()
    return rms(x, w.final_norm) @ w.lm_head.float().t()


@torch.no_grad()
def whisper_decoder_ref(w, tokens: list[int], enc: torch.Tensor) -> torch.Tensor:
    """fp32 Whisper decoder (``WhisperWeights``) over one sequence at positions
    0..T-1 with cross-attention over the encoder states ``enc`` [T_enc, d];
    returns fp32 logits [T, vocab] (tied embedding)."""
    cfg = w.cfg
    d, H, D = cfg.d_model, cfg.n_heads, cfg.head_dim
    dev = w.tok_embed.device
    t = torch.tensor(tokens, dtype=torch.long, device=dev)
    T = t.numel()
    e = enc.float()

    def ln(x, g, b):
        return torch.nn.functional.layer_norm(x, (d,), g.float(), b.float(), 1e-5)

    def lin(x, W, b):
        return x @ W.float().t() + b.float()

    def gelu(x):
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))
    x = w.tok_embed[t].float() + w.dec_pos[:T].float()
    sc = 1.0 / math.sqrt(D)
    for L in w.dec:
        qkv = lin(ln(x, L["ln1_w"], L["ln1_b"]), L["wqkv"], L["bqkv"])
        q, k, v = (qkv[:, i * d:(i + 1) * d].view(T, H, D) for i in range(3))
        x = x + lin(_causal_attn(q, k, v, 1, sc).reshape(T, d), L["wo"], L["bo"])
        q = lin(ln(x, L["lnx_w"], L["lnx_b"]), L["xq"], L["xq_b"]).view(T, H, D)
        kv = lin(e, L["xkv"], L["xkv_b"])
        Te = e.shape[0]
        k, v = kv[:, :d].view(Te, H, D), kv[:, d:].view(Te, H, D)
        p = torch.softmax(torch.einsum("qhd,khd->hqk", q, k) * sc, dim=-1)
        x = x + lin(torch.einsum("hqk,khd->qhd", p, v).reshape(T, d), L["xo"], L["xo_b"])
        x = x + lin(gelu(lin(ln(x, L["ln2_w"], L["ln2_b"]), L["fc1"], L["fc1_b"])), L["fc2"],
                    L["fc2_b"])
    return ln(x, w.dec_ln_w, w.dec_ln_b) @ w.tok_embed.float().t()


# ------------------------------------------------- word timestamps (alignment)
# Whisper's find_alignment, in this engine's terms: the cross-attention queries
# of the alignment heads are kept while a window is decoded (align_record), the
# window's rows are scored against the encoder K rows (align_scores), normalised
# over the rows, median-filtered over the frames and averaged over the heads
# (align_cost), and dynamic time warping over that cost gives every token the
# 20 ms frame at which it starts (dtw).
MAX_ALIGN_HEADS = 32
ALIGN_MEDIAN_WIDTH = 7


def alignment_heads(dec_layers: int, n_heads: int, spec: str | None = None,
                    generation_config: dict | None = None) -> list:
    """The alignment heads as a list of (layer, head). In order: ``spec``
    (``HUB_STT_ALIGNMENT_HEADS``, "l:h,l:h,..."), the checkpoint's
    ``generation_config["alignment_heads"]``, else every head of the upper half
    of the decoder layers (Whisper's default). At most ``MAX_ALIGN_HEADS``: the
    per-slot query store is A * n_text_ctx * D * 2 bytes."""
    if spec is not None and str(spec).strip():
        heads = []
        for item in str(spec).split(","):
            try:
                l, h = item.strip().split(":")
                heads.append((int(l), int(h)))
            except ValueError:
                raise ValueError(f"HUB_STT_ALIGNMENT_HEADS {spec!r}: expected 'layer:head,...'") \
                    from None
    elif generation_config and generation_config.get("alignment_heads"):
        heads = [(int(l), int(h)) for l, h in generation_config["alignment_heads"]]
    else:
        heads = [(l, h) for l in range(dec_layers // 2, dec_layers) for h in range(n_heads)]
    if not heads:
        raise ValueError("HUB_STT_ALIGNMENT_HEADS: no alignment heads")
    if len(heads) > MAX_ALIGN_HEADS:
        raise ValueError(f"HUB_STT_ALIGNMENT_HEADS: {len(heads)} alignment heads, at most "
                         f"{MAX_ALIGN_HEADS} (name them with HUB_STT_ALIGNMENT_HEADS)")
    if len(set(heads)) != len(heads):
        raise ValueError(f"HUB_STT_ALIGNMENT_HEADS: duplicate heads in {heads}")
    for l, h in heads:
        if not (0 <= l < dec_layers and 0 <= h < n_heads):
            raise ValueError(f"HUB_STT_ALIGNMENT_HEADS: head {l}:{h} outside {dec_layers} layers "
                             f"x {n_heads} heads")
    return heads


def align_frames(window_samples: int, n_audio_ctx: int) -> int:
    """Frames (20 ms each) of a window's audio: min(n_audio_ctx, max(1, ceil(samples / 320)))."""
    return min(n_audio_ctx, max(1, -(-int(window_samples) // 320)))


def align_record(qs: dict, heads, positions, slots, cu_q, row_slot, align_q) -> None:
    """Row r of a step (``slots[r] >= 0``) copies the D values of every
    alignment head from its layer's query buffer ``qs[layer]`` [Mpad, H * D] to
    ``align_q[row_slot[b], a, positions[r]]``, b the sequence with
    ``cu_q[b] <= r < cu_q[b + 1]``. Padding rows write nothing."""
    D = align_q.shape[-1]
    cu = [int(c) for c in cu_q]
    for r in range(len(slots)):
        if int(slots[r]) < 0:
            continue
        b = next((b for b in range(len(cu) - 1) if cu[b] <= r < cu[b + 1]), None)
        if b is None:
            continue
        s, p = int(row_slot[b]), int(positions[r])
        if not (0 <= s < align_q.shape[0] and 0 <= p < align_q.shape[2]):
            continue
        for a, (l, h) in enumerate(heads):
            align_q[s, a, p] = qs[l][r, h * D:(h + 1) * D]


def align_scores(q, k, scale: float):
    """q [A, R, D], k [A, F, D] -> P[a, r, :] = softmax_f(scale * q[a, r] . k[a, f]),
    f32 (fp64 inputs: fp64)."""
    dt = torch.float64 if q.dtype == torch.float64 else torch.float32
    s = torch.einsum("ard,afd->arf", q.to(dt), k.to(dt)) * scale
    return torch.softmax(s, dim=-1)


def align_cost(P, n_lead: int):
    """Whisper's alignment matrix from P [A, R, F]: per (a, f) normalise over
    the R rows (population std; 0 where it is 0: a frame whose rows all hold
    the same value, whatever the rounding of their mean), median filter of
    width 7 along f with reflect padding (F <= 3: unchanged), mean over the
    heads, negated, without the first ``n_lead`` rows -> [R - n_lead, F]."""
    mean = P.mean(dim=1, keepdim=True)
    std = (P - mean).pow(2).mean(dim=1, keepdim=True).sqrt()
    std = torch.where((P == P[:, :1]).all(dim=1, keepdim=True), torch.zeros_like(std), std)
    Z = torch.where(std == 0, torch.zeros_like(P), (P - mean) / torch.where(std == 0, 1, std))
    pad = ALIGN_MEDIAN_WIDTH // 2
    if Z.shape[-1] > pad:
        Zp = torch.nn.functional.pad(Z, (pad, pad), mode="reflect")
        Z = Zp.unfold(-1, ALIGN_MEDIAN_WIDTH, 1).sort(dim=-1)[0][..., pad]
    return -(Z.sum(dim=0) / Z.shape[0])[n_lead:].contiguous()


def _dtw_cells(x: np.ndarray):
    """Whisper's recurrence, literally: column-major j, i in f32."""
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    trace = np.full((N + 1, M + 1), -1, np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = x[i - 1, j - 1] + c
            trace[i, j] = t
    return cost, trace


def _dtw_wavefront(x: np.ndarray):
    """The same cells, a whole anti-diagonal i + j = t at a time (the order the
    device kernel takes): a cell reads only cells of the two diagonals before."""
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    trace = np.full((N + 1, M + 1), -1, np.int8)
    cost[0, 0] = 0
    for t in range(2, N + M + 1):
        i = np.arange(max(1, t - M), min(N, t - 1) + 1)
        j = t - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        d = (c0 < c1) & (c0 < c2)
        u = ~d & (c1 < c0) & (c1 < c2)
        c = np.where(d, c0, np.where(u, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = np.where(d, 0, np.where(u, 1, 2))
    return cost, trace


def dtw(x, return_cost: bool = False, literal: bool = False):
    """Dynamic time warping over the cost x [N, M] (f32), Whisper's recurrence
    and backtrace: ``tok_frame[N]`` (int32), the frame of the first path cell
    of every row (Whisper's ``jumps``); with ``return_cost`` also the total cost
    c[N, M] (f32). ``literal``: the cell loop in Whisper's order (the wavefront
    order computes the same f32 add of the same operands in every cell)."""
    x = np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float32)
    N, M = x.shape
    with np.errstate(invalid="ignore"):
        cost, trace = (_dtw_cells if literal else _dtw_wavefront)(x)
    trace[0, :] = 2
    trace[:, 0] = 1
    tok_frame = np.zeros(N, np.int32)
    i, j = N, M
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            tok_frame[i - 1] = j - 1     # the last visit going back is the row's first cell
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return (tok_frame, cost[N, M]) if return_cost else tok_frame


# ------------------------------------------------------------ hotword biasing
# Limits of a hotword automaton (engine/hotwords.py) and the sizes its device
# buffers are allocated at: every phrase has two token variants of at most
# HOTWORD_MAX_TOKENS tokens, so the trie has at most HOTWORD_N_CAP nodes; the
# flattened table (a span per node: the edges of its whole failure chain) is
# bounded by HOTWORD_T_CAP entries, beyond which compiling raises.
HOTWORD_N_CAP = 1 + 2 * HOTWORD_MAX_PHRASES * HOTWORD_MAX_TOKENS
HOTWORD_T_CAP = 1 << 18


def hotword_advance(auto, n: int, t: int) -> int:
    """The node after ``t`` is sampled in node ``n``: the first ``m`` of
    ``chain(n)`` = n, fail[n], ..., 0 with an edge on ``t`` gives its target;
    none: the root."""
    for m in auto.chain(n):
        c = auto.edges[m].get(int(t))
        if c is not None:
            return c
    return 0


def hotword_boosted(auto, n: int) -> set:
    """The columns that get the boost in node ``n``: the edge tokens of every
    node of ``chain(n)``, each once however many chain nodes carry it."""
    out = set()
    for m in auto.chain(n):
        out.update(auto.edges[m])
    return out


def hotword_step(logits, V: int, hw_ctl, row_slot, hw_state, last_tok, auto) -> None:
    """One decoder step of hotword biasing, in place, by walking the failure
    chains. Row b with ``hw_ctl[b]`` 1 starts at the root, with 2 at
    ``advance(hw_state[s], last_tok[s])`` (s = ``row_slot[b]``; a state outside
    the automaton counts as the root); the node is stored in ``hw_state[s]`` and
    ``boost`` is added, in f32 and rounded to the logits' type (a NaN keeps its
    bits), to every column of ``boosted(node)`` below ``V``. Any other ``hw_ctl``, or a slot out of
    range, leaves row and state alone; so does an automaton without edges."""
    if auto is None or auto.T == 0:
        return
    boost = torch.tensor(auto.boost, dtype=torch.float32)
    slots = min(hw_state.numel(), last_tok.numel())
    for b in range(logits.shape[0]):
        ctl = int(hw_ctl[b])
        s = int(row_slot[b])
        if ctl not in (1, 2) or not 0 <= s < slots:
            continue
        n = 0
        if ctl == 2:
            n = int(hw_state[s])
            n = hotword_advance(auto, n if 0 <= n < auto.N else 0, int(last_tok[s]))
        hw_state[s] = n
        cols = sorted(c for c in hotword_boosted(auto, n) if c < V)
        if cols:
            idx = torch.tensor(cols, dtype=torch.long)
            x = logits[b, idx]
            logits[b, idx] = torch.where(torch.isnan(x), x, (x.float() + boost).to(logits.dtype))


# ------------------------------------------------- voice activity detection
# The model of csrc/kernels/vad.hip, which must give these values exactly:
# everything is integer arithmetic (docs/ARCHITECTURE.md "Voice activity
# detection" states the rules).
VAD_FRAME_HZ = 50                # 20 ms frames: one encoder position each
VAD_WS_WORDS = 6                 # kernel workspace, int32 words per frame
VAD_MAX_FLOOR_FRAMES = 3000      # W: 60 s a side
VAD_MAX_RUN_FRAMES = 500         # min_speech, min_silence, pad: 10 s


@dataclass(frozen=True)
class VadParams:
    """The detector's integer parameters, as the kernel gets them."""
    level_min: int       # E below it is never speech: round(2^30 10^(dBFS / 10))
    floor_max: int       # cap on the noise floor, the same scale
    ratio_q: int         # speech needs E * 256 > floor * ratio_q: round(256 10^(dB / 10))
    W: int               # noise-floor window, frames a side
    min_speech: int      # shortest speech run kept, frames
    min_silence: int     # gaps shorter than this are filled, frames
    pad: int             # padding around speech, frames

    def ints(self) -> tuple:
        return (self.level_min, self.floor_max, self.ratio_q, self.W, self.min_speech,
                self.min_silence, self.pad)


def check_vad_params(p: VadParams) -> VadParams:
    """Range check of the integer parameters (ValueError), as the launcher's."""
    lim = (("level_min", 0, 1 << 30), ("floor_max", 0, 1 << 30), ("ratio_q", 256, 2560000),
           ("W", 0, VAD_MAX_FLOOR_FRAMES), ("min_speech", 1, VAD_MAX_RUN_FRAMES),
           ("min_silence", 0, VAD_MAX_RUN_FRAMES), ("pad", 0, VAD_MAX_RUN_FRAMES))
    for name, lo, hi in lim:
        v = getattr(p, name)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"VAD parameter {name} = {v!r} is outside {lo}..{hi}")
    return p


def _vad_frames_of_ms(name: str, ms, lo: int) -> int:
    if isinstance(ms, bool) or not isinstance(ms, (int, float)) or ms != int(ms) or int(ms) % 20:
        raise ValueError(f"VAD {name} = {ms!r} ms must be a multiple of 20")
    n = int(ms) // 20
    if not lo <= n <= VAD_MAX_RUN_FRAMES:
        raise ValueError(f"VAD {name} = {ms} ms is outside {20 * lo}..{20 * VAD_MAX_RUN_FRAMES}")
    return n


def vad_params(threshold_db: float = 9.0, min_level_dbfs: float = -55.0,
               floor_max_dbfs: float = -30.0, floor_s: float = 3.0, min_speech_ms: int = 100,
               min_silence_ms: int = 500, pad_ms: int = 200) -> VadParams:
    """dB, seconds and milliseconds -> ``VadParams``. threshold_db in [0, 40]
    (above the noise floor); the two levels in [-100, 0] dBFS, where 0 dBFS is a
    mean square of 2^30; floor_s in [0, 60]; the millisecond values multiples of
    20, min_speech_ms at least 20, each at most 10 s. ValueError otherwise."""
    def num(name, v, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or \
                not lo <= v <= hi:
            raise ValueError(f"VAD {name} = {v!r} is outside [{lo}, {hi}]")
        return float(v)
    thr = num("threshold_db", threshold_db, 0.0, 40.0)
    lvl = num("min_level_dbfs", min_level_dbfs, -100.0, 0.0)
    cap = num("floor_max_dbfs", floor_max_dbfs, -100.0, 0.0)
    fs = num("floor_s", floor_s, 0.0, VAD_MAX_FLOOR_FRAMES / VAD_FRAME_HZ)
    return check_vad_params(VadParams(
        level_min=int(round((1 << 30) * 10.0 ** (lvl / 10.0))),
        floor_max=int(round((1 << 30) * 10.0 ** (cap / 10.0))),
        ratio_q=int(round(256 * 10.0 ** (thr / 10.0))),
        W=int(round(fs * VAD_FRAME_HZ)),
        min_speech=_vad_frames_of_ms("min_speech_ms", min_speech_ms, 1),
        min_silence=_vad_frames_of_ms("min_silence_ms", min_silence_ms, 0),
        pad=_vad_frames_of_ms("pad_ms", pad_ms, 0)))


def vad_frames(n: int, rate: int) -> int:
    """20 ms frames of ``n`` samples at ``rate``: ceil(n * 50 / rate)."""
    return -(-int(n) * VAD_FRAME_HZ // int(rate))


def vad_check_descs(descs, pcm_len: int, frames_cap: int | None = None) -> list:
    """``descs`` as tuples of ints (src_first, src_len, rate, frame_first),
    checked: a supported rate, the utterance inside the ``pcm_len`` samples,
    its frames inside ``frames_cap`` (when given) and apart from every other
    utterance's. ValueError otherwise."""
    out = [tuple(int(v) for v in d) for d in descs]
    spans = []
    for d in out:
        if len(d) != 4:
            raise ValueError(f"VAD descriptor {d}: (src_first, src_len, rate, frame_first)")
        s0, n, rate, f0 = d
        check_rate(rate)
        if s0 < 0 or n < 0 or f0 < 0 or s0 + n > pcm_len:
            raise ValueError(f"VAD descriptor {d} is outside the PCM ({pcm_len} samples)")
        F = vad_frames(n, rate)
        if frames_cap is not None and f0 + F > frames_cap:
            raise ValueError(f"VAD descriptor {d}: frames [{f0}, {f0 + F}) exceed the frame "
                             f"array ({frames_cap})")
        if F:
            spans.append((f0, f0 + F))
    spans.sort()
    for (_, e0), (s1, _) in zip(spans, spans[1:]):
        if s1 < e0:
            raise ValueError("VAD descriptors: the utterances' frame ranges overlap")
    return out


def vad_energy(pcm, descs, out=None) -> np.ndarray:
    """Frame energies, uint32: E[frame_first + f] = floor(sum x^2 / count) over
    the source samples [f * rate // 50, min(n, (f + 1) * rate // 50)) of each
    utterance, f < ceil(n * 50 / rate). ``out``: the frame array to write into
    (only the utterances' frames change); default: zeros up to the last frame."""
    x = pcm.numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
    descs = vad_check_descs(descs, x.shape[0], None if out is None else out.shape[0])
    if out is None:
        out = np.zeros(max([f0 + vad_frames(n, r) for _, n, r, f0 in descs] + [0]), np.uint32)
    for s0, n, rate, f0 in descs:
        F = vad_frames(n, rate)
        if F == 0:
            continue
        edges = np.minimum(np.arange(F + 1, dtype=np.int64) * rate // VAD_FRAME_HZ, n)
        sq = x[s0:s0 + n].astype(np.int64) ** 2
        csum = np.zeros(n + 1, np.int64)
        np.cumsum(sq, out=csum[1:])              # < 2^30 * 2^33: exact in int64
        out[f0:f0 + F] = ((csum[edges[1:]] - csum[edges[:-1]]) // np.diff(edges)).astype(np.uint32)
    return out


def _runs(s: np.ndarray) -> list:
    """Maximal runs of True in the bool vector ``s`` as [start, end) pairs."""
    d = np.diff(np.concatenate(([0], s.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def vad_raw(E, p: VadParams) -> np.ndarray:
    """The raw per-frame decision of one utterance's energies (bool [F]):
    N[f] = min(floor_max, min E[g] for |g - f| <= W inside the utterance),
    raw[f] = E[f] >= level_min and E[f] * 256 > N[f] * ratio_q."""
    E = np.asarray(E, np.uint32).astype(np.uint64)
    F = E.shape[0]
    N = np.empty(F, np.uint64)
    for f in range(F):
        N[f] = E[max(0, f - p.W):f + p.W + 1].min()
    N = np.minimum(N, np.uint64(p.floor_max))
    return (E >= np.uint64(p.level_min)) & (E * np.uint64(256) > N * np.uint64(p.ratio_q))


def vad_smooth(raw, p: VadParams) -> np.ndarray:
    """Close, open, pad - each on the result of the one before (bool [F])."""
    s = np.array(raw, bool)
    F = s.shape[0]
    for a, b in _runs(~s):                       # close: inner gaps shorter than min_silence
        if a > 0 and b < F and b - a < p.min_silence:
            s[a:b] = True
    for a, b in _runs(s):                        # open: speech runs shorter than min_speech
        if b - a < p.min_speech:
            s[a:b] = False
    out = s.copy()
    for a, b in _runs(s):                        # pad, clipped to the utterance
        out[max(0, a - p.pad):min(F, b + p.pad)] = True
    return out


def vad_spans(E, F: int, p: VadParams) -> tuple[np.ndarray, int]:
    """(int32 [n, 2] spans as [start, end) frames, ascending; speech frames) of
    one utterance: ``E[:F]`` are its frame energies."""
    check_vad_params(p)
    s = vad_smooth(vad_raw(np.asarray(E)[:F], p), p)
    return np.asarray(_runs(s), np.int32).reshape(-1, 2), int(s.sum())


def vad(pcm, descs, p: VadParams, out=None):
    """Energies and spans of every utterance (the CPU path of ``ops.vad``):
    (E uint32 [frames] as int32 bits, spans int32 [U, cap, 2], n_spans int32
    [U], speech_frames int32 [U]) as tensors, cap = F_max // 2 + 1. Entries of
    ``spans`` beyond ``n_spans`` are -1, or stay as they are in ``out`` = (E,
    spans, n_spans, speech_frames), which is then written in place."""
    check_vad_params(p)
    x = pcm.numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
    descs = vad_check_descs(descs, x.shape[0], None if out is None else out[0].numel())
    Fs = [vad_frames(n, r) for _, n, r, _ in descs]
    U, cap = len(descs), max(Fs + [0]) // 2 + 1
    if out is None:
        total = max([d[3] + F for d, F in zip(descs, Fs)] + [0])
        out = (torch.zeros(total, dtype=torch.int32),
               torch.full((U, cap, 2), -1, dtype=torch.int32),
               torch.zeros(U, dtype=torch.int32), torch.zeros(U, dtype=torch.int32))
    E_t, spans_t, n_t, sf_t = out
    E = E_t.numpy().view(np.uint32)
    vad_energy(x, descs, E)
    for u, (d, F) in enumerate(zip(descs, Fs)):
        sp, n_speech = vad_spans(E[d[3]:d[3] + F], F, p)
        spans_t[u, :len(sp)] = torch.from_numpy(sp)
        n_t[u] = len(sp)
        sf_t[u] = n_speech
    return E_t, spans_t, n_t, sf_t
