"""Key masks and addressing of every attention kernel, one key at a time.

Every attention kernel decides per key whether it counts (causal bound,
context end, split / tile ends, block-table lookup, start / length addressing,
the ``lens`` mask of the VITS attention). The inputs here make a one-key
error change a whole output row, and the memory a kernel must not use is
hostile instead of benign:

* **ramp-up**: key ``j`` scores exactly ``32 * j * scale`` (2.8 nats per key
  at D = 128, 4 at D = 64), so the softmax sits on the last permitted key;
* **ramp-down**: the same keys with ``Q = -32``: key 0 dominates;
* **spike**: one key ``j*`` per sequence scores ``2048 * scale``; the output
  is ``V[j*]`` unless a block-table entry, tile or split loses it.

"Outside" memory (slots past ``ctx_len`` in a last block, blocks in no table,
the block unused table entries point at, block 0 of the zero tables of padding
sequences, contiguous rows outside ``[start, start + len)``) is filled three
ways: *continuation* (the K ramp goes on in both directions, the spike is
doubled, ``V = 1000`` - an included key dominates the row), zeros, and NaN.

Assertions, per case:

* per (query row, head), continuation fill:
  ``max|o - ref| <= 2e-2 * max|ref_row|`` against the unrounded fp32
  ``ops.reference.attention`` of the ``.float()`` inputs (the bound of
  ``test_mixed_attention.py``, here per row instead of per tensor);
* the outputs of the three fills are bitwise equal (a load nullified by
  ``P = 0`` rather than never made turns the NaN fill into NaN);
* decode kernel: a replay is bitwise equal, the split tickets are left zero,
  nothing is written past the ``Tq`` rows of a sentinel-filled output buffer,
  and the split workspace starts NaN-filled (it is ``torch.empty`` in the
  engines).

The CPU tests at the bottom prove the checker without a GPU: the reference
rounded to bf16 passes; ``ctx_lens +- 1``, a dropped first key and swapped
block-table entries miss the bound in every row of every affected sequence; a
candidate with the kernels' rounding (bf16 P, bf16 output) passes.

Deviation from a literal cross product: the older grouped kernel
(``attn_fwd_kernel<GROUPED>``) covers ``num_splits * split_keys`` keys by
contract (every caller sizes the splits from the longest context), so
``num_splits = 1`` with ``split_keys = 128`` cannot serve a 300-key context.
The single-split launch is run twice instead: contexts ``[300, 65, 16]`` with
one 320-key split, and ``split_keys = 128`` with contexts ``[128, 65, 16]``.

Worst per-row ratio observed on an MI355X (bound 2e-2), per kernel path:

    attn_prefill2_kernel, contiguous        0.0042
    attn_prefill2_kernel, paged + prefix    0.0043
    attn_decode, paged (all four forms)     0.0048
    attn_decode, contiguous start / len     0.0036
    attn_fwd_kernel<GROUPED> + combine      0.0038
    relpos_attention_kernel                 0.0038

(the CPU candidate with bf16 P and bf16 output: 0.0041; ``ctx_lens +- 1``
leaves no row under 0.7). Every kernel passed as it is: none needed a fix.
"""
import functools
import math

import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as R

BOUND = 2e-2
HKV = 2
FILLS = ("cont", "zeros", "nan")
FAR = 2048          # ramp position of slots that belong to no sequence
SPIKE_CTX = 300
SPIKES = (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, SPIKE_CTX - 1)
SENTINEL = -7.0

# decode-attention kernel forms: (8-wave min keys, prefetch min keys) -> the
# 4-wave kernel, the 8-wave single-pass one, and the prefetching variants
ATTN_FORMS = {"w4": (0, 0), "w8": (256, 0), "w4pf": (0, 64), "w8pf": (256, 64)}


@pytest.fixture(params=sorted(ATTN_FORMS))
def attn_form(request, monkeypatch):
    w8, pf = ATTN_FORMS[request.param]
    monkeypatch.setattr(ops, "ATTN8_MIN_KEYS", w8)
    monkeypatch.setattr(ops, "ATTN_PF_MIN_KEYS", pf)
    return request.param


# ------------------------------------------------------------------- inputs
def _ramp(pos: torch.Tensor) -> torch.Tensor:
    """Signed positions [n] -> [n, 3] floats that sum to the position, each
    exact in bf16 (0..15, multiples of 16 below 256, multiples of 256)."""
    lo = torch.remainder(pos, 16)
    mid = 16 * torch.remainder(torch.div(pos, 16, rounding_mode="floor"), 16)
    hi = 256 * torch.div(pos, 256, rounding_mode="floor")
    return torch.stack([lo, mid, hi], -1).float()


def _cu(lens) -> torch.Tensor:
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)


class Case:
    """One batch: queries, K/V slots in token-major order with the
    continuation fill, the mask of the slots the op may use, and the metadata
    of the launch. ``meta`` holds ``ctx`` and ``bt`` (paged) or ``starts``."""

    def __init__(self, fam, qlens, slot_pos, inside, spike, *, H, D, causal, g, hkv=HKV, blk=0,
                 **meta):
        self.fam, self.qlens, self.H, self.D, self.hkv = fam, list(qlens), H, D, hkv
        self.causal, self.blk, self.inside, self.meta = causal, blk, inside, meta
        self.Tq = sum(qlens)
        self.cu_q = _cu(qlens)
        self.seq_of_row = torch.repeat_interleave(torch.arange(len(qlens)), torch.tensor(qlens))
        S = slot_pos.numel()
        sign = -1.0 if fam == "down" else 1.0
        q = 0.5 * torch.randn(self.Tq, H, D, generator=g)
        K = 0.5 * torch.randn(S, hkv, D, generator=g)
        V = torch.randn(S, hkv, D, generator=g)
        q[..., :4] = 0
        K[..., :4] = 0
        if fam == "spike":
            q[..., 3] = 32
            K[spike, :, 3] = 64
            K[~inside, :, 3] = 128
        else:
            q[..., :3] = 32 * sign
            K[..., :3] = _ramp(slot_pos)[:, None, :]
        V[~inside] = 1000
        # q is a view into a wider row, as in the fused qkv output
        self.qbuf = torch.full((self.Tq, H * D + 64), float("nan")).bfloat16()
        self.qbuf[:, : H * D] = q.view(self.Tq, H * D).bfloat16()
        self.K, self.V = K, V

    def kv(self, fill: str):
        """K, V in the op's layout (CPU bf16) with the outside memory filled."""
        K, V = self.K.clone(), self.V.clone()
        if fill != "cont":
            x = 0.0 if fill == "zeros" else float("nan")
            K[~self.inside] = x
            V[~self.inside] = x
        K, V = K.bfloat16(), V.bfloat16()
        S = K.shape[0]
        if self.blk:
            nb = S // self.blk
            return tuple(t.view(nb, self.blk, self.hkv, self.D).permute(0, 2, 1, 3).contiguous()
                         for t in (K, V))
        return (torch.cat([K.view(S, -1), V.view(S, -1)], 1),)     # one k|v row buffer

    def args(self, dev="cpu", fill="cont", **over):
        """Positional and keyword arguments of ``ops.attention`` on ``dev``;
        ``over`` replaces ``ctx`` / ``bt`` / ``starts`` (the mutation checks)."""
        m = dict(self.meta)
        m.update(over)
        n = self.hkv * self.D
        kv = [t.to(dev) for t in self.kv(fill)]
        k, v = kv if self.blk else (kv[0][:, :n], kv[0][:, n:])
        kw = dict(n_heads=self.H, n_kv=self.hkv, head_dim=self.D, causal=self.causal)
        if m.get("ctx") is not None:
            kw["ctx_lens"] = m["ctx"].to(dev)
        if self.blk:
            kw["block_tables"] = m["bt"].to(dev)
        else:
            kw["cu_k"] = m["starts"].to(dev)
        return (self.qbuf.to(dev)[:, : self.H * self.D], k, v, self.cu_q.to(dev)), kw

    def run(self, dev="cpu", fill="cont", over=None, **launch):
        a, kw = self.args(dev, fill, **(over or {}))
        return ops.attention(*a, max_q=max(self.qlens), **kw, **launch)

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        """Unrounded fp32 reference of the continuation-filled inputs."""
        (q, k, v, cu), kw = self.args()
        return R.attention(q.float(), k.float(), v.float(), cu, **kw)


def _paged_slots(ctx, blk, width, g, down=False, n_pad=0):
    """A random paged layout: block table [B + n_pad, width], the logical
    position of every cache slot and the mask of the slots inside a context.
    Unused entries of a sequence's row point at one poison block; padding
    sequences have an all-zero row and block 0 belongs to nobody; four more
    blocks are in no table."""
    need = [-(-c // blk) for c in ctx]
    used = sum(need)
    nb = used + 6
    ids = torch.randperm(nb - 1, generator=g) + 1
    bt = torch.full((len(ctx) + n_pad, width), int(ids[used]), dtype=torch.int32)
    bt[len(ctx):] = 0
    pos = ((-FAR if down else FAR) + torch.arange(blk)).repeat(nb, 1)
    inside = torch.zeros(nb, blk, dtype=torch.bool)
    at = 0
    for b, (c, n) in enumerate(zip(ctx, need)):
        mine = ids[at:at + n]
        at += n
        bt[b, :n] = mine.int()
        p = torch.arange(n * blk).view(n, blk)
        pos[mine] = p               # the ramp runs on past ctx in the last block
        inside[mine] = p < c
    return bt, pos.view(-1), inside.view(-1)


def _paged_spikes(bt, blk, n_slots):
    js = torch.tensor(SPIKES)
    spike = torch.zeros(n_slots, dtype=torch.bool)
    spike[bt[torch.arange(len(SPIKES)), js // blk].long() * blk + js % blk] = True
    return spike


def _row_slots(lens, gap, skip_after=None, lead=64):
    """Contiguous K/V rows: sequences of ``lens`` rows with ``gap`` poison rows
    between them (``lead`` before the first, 64 after the last) and, after
    sequence ``skip_after``, a whole utterance nobody wrote. Poison rows carry
    the ramp on from the sequence before them, and the 32 rows before a
    sequence count down to it (negative positions)."""
    starts, at = [], lead
    for i, n in enumerate(lens):
        starts.append(at)
        at += n + gap
        if i == skip_after:
            at += max(lens) + gap
    rows = torch.arange(at - gap + 64)
    st, ln = torch.tensor(starts), torch.tensor(lens)
    i = torch.searchsorted(st, rows, right=True) - 1
    prev, nxt = st[i.clamp(min=0)], st[(i + 1).clamp(max=len(lens) - 1)]
    inside = (i >= 0) & (rows - prev < ln[i.clamp(min=0)])
    before = ((i < 0) | ((i + 1 < len(lens)) & (rows >= nxt - 32))) & ~inside
    pos = torch.where(before, rows - nxt, rows - prev)
    return torch.tensor(starts, dtype=torch.int32), pos, inside


def _row_spikes(starts, n_rows):
    spike = torch.zeros(n_rows, dtype=torch.bool)
    spike[starts.long() + torch.tensor(SPIKES)] = True
    return spike


PREFILL_LENS = [1, 63, 64, 65, 127, 128, 129, 191, 193, 257]
PREFIX_PAIRS = [(1, 33), (90, 90), (129, 149), (64, 128), (130, 131)]
DECODE_CTX = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 640]
DECODE_Q = [1, 3, 1, 7]
CROSS_LENS = [1500, 33, 64]
GROUPED_CTX = [300, 65, 16]


@functools.lru_cache(maxsize=None)
def prefill_contig_case(fam, D, G, causal, layout):
    """Self-attention over contiguous rows: "gapped" addresses each sequence by
    start / length with poison rows between; "packed" is the cu_k form (the
    sequences back to back, poison before the first and after the last)."""
    g = torch.Generator().manual_seed(1)
    lens = PREFILL_LENS
    if layout == "gapped":
        starts, pos, inside = _row_slots(lens, 64, skip_after=4)
        meta = dict(starts=starts, ctx=torch.tensor(lens, dtype=torch.int32))
    else:
        starts, pos, inside = _row_slots(lens, 0)
        meta = dict(starts=torch.cat([starts, starts[-1:] + lens[-1]]), ctx=None)
    return Case(fam, lens, pos, inside, None, H=HKV * G, D=D, causal=causal, g=g, **meta)


@functools.lru_cache(maxsize=None)
def prefill_paged_case(fam, D, G, blk):
    g = torch.Generator().manual_seed(2)
    if fam == "spike":
        qlens, ctx = [3] * len(SPIKES), [SPIKE_CTX] * len(SPIKES)
    else:
        qlens, ctx = [p[0] for p in PREFIX_PAIRS], [p[1] for p in PREFIX_PAIRS]
    bt, pos, inside = _paged_slots(ctx, blk, -(-max(ctx) // blk) + 1, g, fam == "down")
    spike = _paged_spikes(bt, blk, pos.numel()) if fam == "spike" else None
    return Case(fam, qlens, pos, inside, spike, H=HKV * G, D=D, causal=True, g=g, blk=blk, bt=bt,
                ctx=torch.tensor(ctx, dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def decode_paged_case(fam, D, blk, spare):
    """The decode batch: every context length around a tile, a split and the
    table end, then two graph-bucket padding sequences (q_len 0, ctx 0, zero
    table). ``spare`` = 0: the table is exactly as wide as the longest context
    needs (the look-ahead clamp is hit); 3: three spare entries."""
    g = torch.Generator().manual_seed(3)
    ctx = [SPIKE_CTX] * len(SPIKES) if fam == "spike" else DECODE_CTX
    qlens = [DECODE_Q[i % 4] for i in range(len(ctx))]
    bt, pos, inside = _paged_slots(ctx, blk, -(-max(ctx) // blk) + spare, g, fam == "down", n_pad=2)
    spike = _paged_spikes(bt, blk, pos.numel()) if fam == "spike" else None
    return Case(fam, qlens + [0, 0], pos, inside, spike, H=HKV * 4, D=D, causal=True, g=g, blk=blk,
                bt=bt, ctx=torch.tensor(ctx + [0, 0], dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def decode_contig_case(fam, qlen, hkv):
    """Whisper cross-attention: live utterances addressed by start / length in
    one k|v row buffer, one utterance in between never written."""
    g = torch.Generator().manual_seed(4)
    lens = [SPIKE_CTX] * len(SPIKES) if fam == "spike" else CROSS_LENS
    starts, pos, inside = _row_slots(lens, 64, skip_after=0)
    spike = _row_spikes(starts, pos.numel()) if fam == "spike" else None
    return Case(fam, [qlen] * len(lens), pos, inside, spike, H=6, D=64, causal=False, g=g, hkv=hkv,
                starts=starts, ctx=torch.tensor(lens, dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def grouped_case(fam, D, G, max_q, ctx0):
    g = torch.Generator().manual_seed(5)
    ctx = [ctx0] + GROUPED_CTX[1:]
    bt, pos, inside = _paged_slots(ctx, 16, -(-ctx0 // 16) + 1, g, fam == "down")
    return Case(fam, [max_q, 1, max_q], pos, inside, None, H=HKV * G, D=D, causal=True, g=g, blk=16,
                bt=bt, ctx=torch.tensor(ctx, dtype=torch.int32))


# ------------------------------------------------------------------ checker
def row_ratio(o: torch.Tensor, ref: torch.Tensor, D: int) -> torch.Tensor:
    """max|o - ref| / max|ref| of every (query row, head): [Tq, H]."""
    o, ref = o.float().cpu().reshape(ref.shape[0], -1, D), ref.reshape(ref.shape[0], -1, D)
    return (o - ref).abs().amax(-1) / ref.abs().amax(-1)


def assert_rows(o, c: Case, path: str) -> None:
    ratio = row_ratio(o, c.ref, c.D)
    bad = ~(ratio <= BOUND)             # NaN is bad
    print(f"attention-masks {path} {c.fam}: worst row ratio {float(ratio.max()):.5f} (bound {BOUND})")
    assert not bad.any(), (path, c.fam, "rows over the bound:", bad.nonzero()[:8].tolist(),
                           "worst", float(ratio[bad].nan_to_num(float("inf")).max()))


def assert_every_row_fails(o, c: Case, seqs) -> float:
    """A broken candidate must miss the bound in EVERY (row, head) of ``seqs``."""
    ratio = row_ratio(o, c.ref, c.D)[torch.isin(c.seq_of_row, torch.tensor(seqs))]
    assert ratio.numel() > 0
    missed = ratio <= BOUND
    assert not missed.any(), f"{int(missed.sum())} of {missed.numel()} rows passed a broken candidate"
    return float(ratio.nan_to_num(float("inf")).min())


def check_fills(c: Case, dev, path: str, **launch) -> None:
    outs = {f: c.run(dev, f, **launch) for f in FILLS}
    assert_rows(outs["cont"], c, path)
    for f in FILLS[1:]:
        assert torch.equal(outs[f], outs["cont"]), (path, c.fam, f"{f} fill changes the output")


def check_decode(c: Case, dev, path: str, split_keys: int, **launch) -> None:
    """``check_fills`` for the decode kernel, with its extras."""
    ns = -(-int(c.meta["ctx"].max()) // split_keys) + 1    # the grid is sized past the longest context
    ws = ops.AttnWorkspace(dev, 64, c.H, c.D, ns)
    outs = {}
    for f in FILLS:
        a, kw = c.args(dev, f)
        kw.update(max_q=max(c.qlens), grouped=True, split_keys=split_keys, num_splits=ns,
                  workspace=ws, **launch)
        ws.part_o.fill_(float("nan"))
        ws.part_ml.fill_(float("nan"))
        big = torch.full((c.Tq + 8, c.H * c.D), SENTINEL, dtype=torch.bfloat16, device=dev)
        outs[f] = ops.attention(*a, out=big[: c.Tq], **kw)
        assert outs[f].data_ptr() == big.data_ptr()
        again = ops.attention(*a, **kw)
        assert torch.equal(again, outs[f]), (path, f, "replay differs")
        assert int(ws.counters.abs().sum()) == 0, (path, f, "split tickets not reset")
        assert bool((big[c.Tq:] == SENTINEL).all()), (path, f, "wrote past the query rows")
    assert_rows(outs["cont"], c, path)
    for f in FILLS[1:]:
        assert torch.equal(outs[f], outs["cont"]), (path, c.fam, f"{f} fill changes the output")


# ---------------------------------------------------------------- GPU tests
DEV = "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["gapped", "packed"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("fam", ["up", "down"])
def test_prefill_contiguous(fam, D, G, causal, layout):
    """attn_prefill2_kernel: 128-row query tiles, 64-key tiles split over two
    wave halves - one, odd and even tile counts, tails on both sides of 64."""
    check_fills(prefill_contig_case(fam, D, G, causal, layout), DEV, "prefill2-contiguous")


@pytest.mark.gpu
@pytest.mark.parametrize("blk", [16, 64])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("fam", ["up", "down", "spike"])
def test_prefill_paged_prefix(fam, D, G, blk):
    """attn_prefill2_kernel through the block table, queries behind a prefix."""
    check_fills(prefill_paged_case(fam, D, G, blk), DEV, "prefill2-paged")


@pytest.mark.gpu
@pytest.mark.parametrize("spare", [0, 3])
@pytest.mark.parametrize("blk", [16, 32, 64])
@pytest.mark.parametrize("D,split_keys", [(128, 128), (128, 256), (128, 512), (64, 128), (64, 512)])
@pytest.mark.parametrize("fam", ["up", "down"])
def test_decode_paged(fam, D, split_keys, blk, spare, attn_form):
    """attn_decode.hip over the paged cache: 4 / 8 waves, with and without the
    prefetch; cache blocks below, at and above the 32-key tile."""
    check_decode(decode_paged_case(fam, D, blk, spare), DEV, "decode-paged", split_keys)


@pytest.mark.gpu
@pytest.mark.parametrize("blk", [16, 32, 64])
@pytest.mark.parametrize("split_keys", [128, 512])
def test_decode_paged_spike(split_keys, blk, attn_form):
    check_decode(decode_paged_case("spike", 128, blk, 0), DEV, "decode-paged", split_keys)


@pytest.mark.gpu
@pytest.mark.parametrize("hkv", [2, 6])
@pytest.mark.parametrize("split_keys", [128, 1536])
@pytest.mark.parametrize("qlen", [1, 4])
@pytest.mark.parametrize("fam", ["up", "down", "spike"])
def test_decode_contiguous(fam, qlen, split_keys, hkv, attn_form):
    """attn_decode.hip on contiguous rows at start / length (cross-attention):
    1500 % 32 != 0, so the tail tile of an utterance overlaps rows nobody wrote."""
    check_decode(decode_contig_case(fam, qlen, hkv), DEV, "decode-contiguous", split_keys)


@pytest.mark.gpu
@pytest.mark.parametrize("ctx0,split_keys,num_splits", [(300, 128, 3), (300, 320, 1), (128, 128, 1)])
@pytest.mark.parametrize("G,max_q", [(8, 5), (8, 16), (4, 9)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("fam", ["up", "down"])
def test_grouped_fwd_combine(fam, D, G, max_q, ctx0, split_keys, num_splits):
    """attn_fwd_kernel<GROUPED> (+ attn_combine_kernel): G * max_q in (32, 128]."""
    c = grouped_case(fam, D, G, max_q, ctx0)
    ws = ops.AttnWorkspace(DEV, 64, c.H, D, 4)
    ws.part_o.fill_(float("nan"))
    ws.part_ml.fill_(float("nan"))
    check_fills(c, DEV, "grouped-fwd", grouped=True, split_keys=split_keys, num_splits=num_splits,
                workspace=ws)


# ---------------------------------------------------- VITS relative attention
RP = dict(B=5, T=130, H=2, D=96, W=4, lens=[130, 1, 63, 64, 65])


@functools.lru_cache(maxsize=None)
def relpos_case(fam):
    g = torch.Generator().manual_seed(6)
    B, T, H, D, W = (RP[k] for k in "BTHDW")
    q = 0.5 * torch.randn(B, T, H, D, generator=g)
    k = 0.5 * torch.randn(B, T, H, D, generator=g)
    v = torch.randn(B, T, H, D, generator=g)
    q[..., :4] = 0
    k[..., :4] = 0
    q[..., :3] = -32 if fam == "down" else 32
    k[..., :3] = _ramp(torch.arange(T))[None, :, None, :]
    qkv = torch.cat([t.reshape(B, T, H * D) for t in (q, k, v)], -1).bfloat16()
    ek = (0.1 * torch.randn(2 * W + 1, D, generator=g)).bfloat16()
    ev = (0.1 * torch.randn(2 * W + 1, D, generator=g)).bfloat16()
    lens = torch.tensor(RP["lens"], dtype=torch.int32)
    valid = torch.arange(T)[None, :] < lens[:, None]
    fills = {"zeros": qkv.clone(), "big": qkv.clone()}
    fills["zeros"][~valid] = 0
    fills["big"][~valid] = (1000.0 * (1 - 2 * (torch.arange(3 * H * D) % 2))).bfloat16()
    ref = R.relpos_attention(fills["big"].float(), ek.float(), ev.float(), lens, H, D, W,
                             1 / math.sqrt(D))
    return fills, ek, ev, lens, valid, ref


def check_relpos(fam, dev):
    fills, ek, ev, lens, valid, ref = relpos_case(fam)
    H, D, W = RP["H"], RP["D"], RP["W"]
    outs = {f: ops.relpos_attention(x.to(dev), ek.to(dev), ev.to(dev), lens.to(dev), H, D, W).cpu()
            for f, x in fills.items()}
    ratio = row_ratio(outs["big"][valid], ref[valid], D)
    print(f"attention-masks relpos {fam}: worst row ratio {float(ratio.max()):.5f} (bound {BOUND})")
    assert not (~(ratio <= BOUND)).any(), float(ratio.max())
    assert torch.equal(outs["big"][valid], outs["zeros"][valid]), "padding rows leak into valid rows"
    for f, o in outs.items():
        assert not o[~valid].any(), f"{f}: padded rows are not exactly zero"
    return outs["big"], ref, valid


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["up", "down"])
def test_relpos_attention_lens(fam):
    """relpos_attention_kernel: the ``lens`` mask on keys and on query rows;
    rows at or past ``lens[b]`` hold zeros, then +-1000 (no NaN fill: the
    -1e4 mask of VITS multiplies 0 * V in the reference too)."""
    check_relpos(fam, DEV)


# ------------------------------------------------- CPU self-checks of the checker
def _sim_attention(q, k, v, cu_q, *, n_heads, n_kv, head_dim, causal, cu_k=None, ctx_lens=None,
                   block_tables=None):
    """The kernels' rounding scheme on the CPU: fp32 scores and row sum, P
    rounded to bf16 before P.V, bf16 output."""
    H, D, G = n_heads, head_dim, n_heads // n_kv
    out = torch.zeros(q.shape[0], H * D)
    cuq = cu_q.tolist()
    for b in range(len(cuq) - 1):
        q0, q1 = cuq[b], cuq[b + 1]
        if q1 == q0:
            continue
        if block_tables is not None:
            idx = torch.arange(int(ctx_lens[b]))
            blocks = block_tables[b].long()[idx // k.shape[2]]
            kb, vb = k[blocks, :, idx % k.shape[2]], v[blocks, :, idx % k.shape[2]]
        else:
            k0 = int(cu_k[b])
            k1 = k0 + int(ctx_lens[b]) if ctx_lens is not None else int(cu_k[b + 1])
            kb, vb = k[k0:k1].reshape(k1 - k0, n_kv, D), v[k0:k1].reshape(k1 - k0, n_kv, D)
        L = kb.shape[0]
        kb, vb = kb.float().repeat_interleave(G, 1), vb.float().repeat_interleave(G, 1)
        qb = q[q0:q1].reshape(q1 - q0, H, D).float()
        s = torch.einsum("qhd,khd->hqk", qb, kb) / math.sqrt(D)
        if causal:
            qpos = torch.arange(q1 - q0) + L - (q1 - q0)
            s = s.masked_fill(torch.arange(L)[None, None, :] > qpos[None, :, None], float("-inf"))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.einsum("hqk,khd->qhd", e.bfloat16().float(), vb) / e.sum(-1).t()[..., None]
        out[q0:q1] = o.reshape(q1 - q0, H * D)
    return out.bfloat16()


CPU_CASES = {
    "prefill-gapped": lambda fam: prefill_contig_case(fam, 64, 4, True, "gapped"),
    "prefill-packed": lambda fam: prefill_contig_case(fam, 128, 1, False, "packed"),
    "prefill-paged": lambda fam: prefill_paged_case(fam, 128, 4, 16),
    "decode-paged": lambda fam: decode_paged_case(fam, 128, 16, 3),
    "decode-paged-full-table": lambda fam: decode_paged_case(fam, 64, 64, 0),
    "decode-contiguous": lambda fam: decode_contig_case(fam, 4, 2),
    "grouped": lambda fam: grouped_case(fam, 64, 8, 16, 300),
}


# the spike sweep runs on the paged paths and on start / length rows
SPIKE_PATHS = ("prefill-paged", "decode-paged", "decode-paged-full-table", "decode-contiguous")
CPU_PARAMS = [(p, f) for p in sorted(CPU_CASES) for f in ("up", "down", "spike")
              if f != "spike" or p in SPIKE_PATHS]


@pytest.mark.parametrize("path,fam", CPU_PARAMS)
def test_checker_passes_the_reference(path, fam):
    """Unmutated: the reference rounded to bf16 passes every assertion, and
    it never reads the outside memory."""
    check_fills(CPU_CASES[path](fam), "cpu", "cpu-" + path)


@pytest.mark.parametrize("path,fam", CPU_PARAMS)
def test_checker_accepts_bf16_scheme(path, fam):
    """bf16 P and bf16 output - the rounding the kernels do - stay inside the
    per-row bound on these inputs."""
    c = CPU_CASES[path](fam)
    a, kw = c.args()
    assert_rows(_sim_attention(*a, **kw), c, "cpu-bf16-scheme-" + path)


@pytest.mark.parametrize("delta", [1, -1])
@pytest.mark.parametrize("path,D,causal", [("paged", 128, True), ("paged", 64, True),
                                           ("rows", 64, False), ("rows", 128, False),
                                           ("rows", 64, True), ("rows", 128, True)])
def test_checker_catches_ctx_off_by_one(path, D, causal, delta):
    """One key too many (it lands on the continuation fill) or too few on a
    ramp-up case: every row of every sequence misses the bound."""
    if path == "paged":
        c = decode_paged_case("up", D, 16, 3)
    else:
        c = prefill_contig_case("up", D, 4, causal, "gapped")
    live = [b for b, n in enumerate(c.qlens) if n]
    ctx = c.meta["ctx"].clone()
    ctx[live] += delta
    least = assert_every_row_fails(c.run(over=dict(ctx=ctx)), c, live)
    print(f"attention-masks ctx{delta:+d} {path} D={D} causal={causal}: least row error {least:.3f} x scale")


@pytest.mark.parametrize("qlen", [1, 4])
def test_checker_catches_dropped_first_key(qlen):
    c = decode_contig_case("down", qlen, 2)
    over = dict(starts=c.meta["starts"] + 1, ctx=c.meta["ctx"] - 1)
    assert_every_row_fails(c.run(over=over), c, list(range(len(c.qlens))))


@pytest.mark.parametrize("blk", [16, 64])
def test_checker_catches_swapped_table_entries(blk):
    """Two used entries swapped between sequences a and b (the block that
    holds a's spike): a loses its spike and b gains a second one."""
    c = decode_paged_case("spike", 128, blk, 0)
    for a, b in ((0, 7), (4, 9), (6, 5)):      # a's spike lies before every query of b
        col = SPIKES[a] // blk
        assert SPIKES[b] // blk != col
        bt = c.meta["bt"].clone()
        bt[a, col], bt[b, col] = c.meta["bt"][b, col], c.meta["bt"][a, col]
        o = c.run(over=dict(bt=bt))
        assert_every_row_fails(o, c, [a, b])
        others = ~torch.isin(c.seq_of_row, torch.tensor([a, b]))
        assert bool((row_ratio(o, c.ref, c.D)[others] <= BOUND).all())


@pytest.mark.parametrize("fam", ["up", "down"])
def test_checker_relpos_cpu(fam):
    """The relpos checks on the CPU reference; on the ramp-up case a ``lens``
    off by one fails every valid row of the sequences it changes."""
    o, ref, valid = check_relpos(fam, "cpu")
    if fam != "up":
        return
    fills, ek, ev, lens, _, _ = relpos_case(fam)
    H, D, W = RP["H"], RP["D"], RP["W"]
    for delta in (1, -1):
        ch = [b for b, n in enumerate(RP["lens"]) if 1 < n + delta <= RP["T"]]
        l2 = lens.clone()
        l2[ch] += delta
        bad = ops.relpos_attention(fills["big"], ek, ev, l2, H, D, W)
        both = valid[ch] & (torch.arange(RP["T"])[None, :] < l2[ch][:, None])
        assert not (row_ratio(bad[ch][both], ref[ch][both], D) <= BOUND).any()
