"""The beam-search kernels (``csrc/kernels/beam.hip``) against their host
definitions (``ops.reference``).

``beam_topk``: logits are small integers, so the selection (with its many ties)
is exact and ``cand_id`` must equal the reference's, -1 padding included. The
log-probabilities are held to fp64 computed from the stored values within the
bound that ``tests/test_argmax_logprob.py`` derives for the row scan's
log-softmax (same chunks, same reduction order; with integer logits ``x - m``
is exact, so the one extra subtraction rounds once, inside that bound's
``4 R u`` exponent term that integers do not spend). ``cand_lp[:, 0]`` must be
``ops.masked_argmax_logprob``'s bits on every row whose winner is not EOT.

The logits are a view into a NaN-filled buffer (a row above and below, the
padding columns), the mask table lies between rows that allow everything and
its own padding bits are set: anything read outside the operands shows.
"""
import math

import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref
from loqa_hub_amd.ops.reference import pack_mask
from test_argmax_logprob import bound

pytestmark = pytest.mark.gpu

EOT = 50
SHAPES = [(51866, 51904), (8192, 8192), (100, 104)]     # (V, row stride)
RS = [1, 5, 16]
KBS = [1, 2, 5, 8]

_CASES: dict = {}


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def make_case(V: int, ld: int, R: int, dtype):
    """CPU operands, built once: (buffer [R + 2, ld] of NaN holding the logits
    at [1 : R + 1, :V], allowed [3, V], mask table [5, W] whose rows 1..3 are
    the table, mask_rows [R]). Mask row 0: half the columns and EOT; row 1:
    three columns, EOT masked; row 2: nothing."""
    key = (V, ld, R, dtype)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(V + 31 * R)
    x = torch.randint(-8, 9, (R, V), generator=g).float()
    x[::4, EOT] = 9.0                                      # EOT the row maximum on every 4th row
    buf = torch.full((R + 2, ld), float("nan"), dtype=dtype)
    buf[1:R + 1, :V] = x.to(dtype)
    allowed = torch.zeros(3, V, dtype=torch.bool)
    allowed[0] = torch.rand(V, generator=g) < 0.5
    allowed[0, EOT] = True
    allowed[1, [3, V // 2 + 1, V - 1]] = True
    table = torch.full((5, (V + 31) // 32), -1, dtype=torch.int32)
    table[1:4] = pack_mask(allowed)
    if V % 32:                                             # the table's own padding bits
        table[1:4, -1] |= torch.tensor(-(1 << (V % 32)), dtype=torch.int32)
    rows = (torch.arange(R) % 2).to(torch.int32)
    if R >= 5:
        rows[R - 1] = 2                                    # a row with nothing allowed
    out = (buf, allowed, table, rows)
    _CASES[key] = out
    return out


def oracle64(view: torch.Tensor, allow: torch.Tensor, cid: torch.Tensor):
    """fp64 log-softmax over the allowed columns at ``cid`` and at EOT."""
    x = view.double().masked_fill(~allow, float("-inf"))
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    lp = x.gather(1, cid.long().clamp(min=0)) - lse
    lp = torch.where(cid >= 0, lp, torch.full_like(lp, float("-inf")))
    elp = x[:, EOT] - lse[:, 0]
    nothing = ~allow.any(dim=1)
    lp[nothing] = float("-inf")
    elp[nothing | ~allow[:, EOT]] = float("-inf")
    return lp, elp


def max_err(got: torch.Tensor, want: torch.Tensor) -> float:
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got.cpu()), fin), "-inf in different places"
    if not fin.any():
        return 0.0
    return (got.cpu().double()[fin] - want[fin]).abs().max().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_beam_topk(V, ld, dtype):
    dev = torch.device("cuda")
    for R in RS:
        buf, allowed, table, rows = make_case(V, ld, R, dtype)
        view_c = buf[1:R + 1, :V]
        allow = allowed[rows.long()]
        dbuf, dtab = buf.to(dev), table.to(dev)
        view, mask, drows = dbuf[1:R + 1, :V], dtab[1:4], rows.to(dev)
        assert view.stride(0) == ld
        want_id, _, _ = ref.beam_topk(view_c, table[1:4], rows, EOT, 8)
        am_idx, am_lp = ops.masked_argmax_logprob(view, mask, drows)
        for KB in KBS:
            cid, clp, elp = ops.beam_topk(view, mask, drows, EOT, KB)
            assert cid.dtype == torch.int32 and clp.dtype == elp.dtype == torch.float32
            assert cid.shape == clp.shape == (R, KB) and elp.shape == (R,)
            assert torch.equal(cid.cpu(), want_id[:, :KB]), (V, R, KB)
            lp64, elp64 = oracle64(view_c, allow, cid.cpu())
            err = max(max_err(clp, lp64), max_err(elp, elp64))
            print(f"V={V} R={R} KB={KB} {dtype}: err {err:.3e} bound {bound(V, dtype):.3e}")
            assert err <= bound(V, dtype), (err, bound(V, dtype))
            # the argmax row scan's bits, wherever its winner is not EOT
            sel = ((am_idx != EOT) & (am_idx >= 0)).cpu()
            assert torch.equal(cid.cpu()[sel, 0], am_idx.cpu()[sel])
            assert bits_equal(clp[:, 0].cpu()[sel], am_lp.cpu()[sel])
            if R >= 5:                                     # rows 2, 6, ..: half the columns
                assert sel[2].item() and not sel[0].item()
            again = ops.beam_topk(view, mask, drows, EOT, KB)
            assert torch.equal(cid, again[0]) and bits_equal(clp, again[1]) and \
                bits_equal(elp, again[2])
        if R >= 5:                                         # the row with nothing allowed
            assert cid[R - 1].tolist() == [-1] * 8
            assert clp[R - 1].tolist() == [float("-inf")] * 8 and elp[R - 1].item() == -math.inf
        if R > 1:                                          # three columns allowed, EOT masked
            assert cid[1].tolist()[3:] == [-1] * 5 and (cid[1, :3] >= 0).all()


def test_beam_topk_without_a_mask():
    dev = torch.device("cuda")
    V, ld, R = 51866, 51904, 5
    buf, _, _, _ = make_case(V, ld, R, torch.bfloat16)
    view = buf.to(dev)[1:R + 1, :V]
    cid, clp, elp = ops.beam_topk(view, None, None, EOT, 5)
    want_id, _, _ = ref.beam_topk(buf[1:R + 1, :V], None, None, EOT, 5)
    assert torch.equal(cid.cpu(), want_id)
    lp64, elp64 = oracle64(buf[1:R + 1, :V], torch.ones(R, V, dtype=torch.bool), cid.cpu())
    assert max(max_err(clp, lp64), max_err(elp, elp64)) <= bound(V, torch.bfloat16)
    am_idx, am_lp = ops.masked_argmax_logprob(view)
    sel = (am_idx != EOT).cpu()
    assert bits_equal(clp[:, 0].cpu()[sel], am_lp.cpu()[sel])


def test_beam_topk_checks_its_arguments():
    x = torch.zeros(2, 100, device="cuda")
    with pytest.raises(ValueError):
        ops.beam_topk(x, None, None, EOT, 9)
    with pytest.raises(TypeError):
        ops.beam_topk(x.half(), None, None, EOT, 2)
    with pytest.raises(ValueError):
        ops.beam_topk(x, torch.zeros(2, 3, dtype=torch.int32, device="cuda"), None, EOT, 2)


@pytest.mark.parametrize("n_src_is_b", [False, True], ids=["first_step", "later_step"])
@pytest.mark.parametrize("B", [2, 5, 8])
@pytest.mark.parametrize("G", [1, 3])
def test_beam_merge(G, B, n_src_is_b):
    dev = torch.device("cuda")
    n_src = B if n_src_is_b else 1
    V, R = 100, G * n_src
    g = torch.Generator().manual_seed(100 * G + 10 * B + n_src)
    x = torch.randint(-4, 5, (R, V), generator=g).float()
    allowed = torch.ones(2, V, dtype=torch.bool)
    allowed[1] = False
    allowed[1, [7, 9, EOT]] = True                          # missing candidates for B > 2
    rows = (torch.arange(R) % 3 == 2).to(torch.int32)
    if G == 3:
        rows[-n_src:] = 1                                   # a whole group short of candidates
    cid, clp, elp = ops.beam_topk(x.to(dev), pack_mask(allowed).to(dev), rows.to(dev), EOT, B)
    cum = -torch.rand(G, B, generator=g) * 3
    cum[:, -1] = float("-inf")                              # a dead source beam
    if not n_src_is_b:
        cum[:, 1:] = float("-inf")
    got = ops.beam_merge(cid, clp, elp, cum.to(dev), n_src)
    want = ref.beam_merge(cid.cpu(), clp.cpu(), elp.cpu(), cum, n_src)
    names = ("tok", "parent", "lp", "cum_out", "eot_score", "eot_fin")
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape == (G, B), name
        assert bits_equal(a, b), (name, a.cpu(), b)
    again = ops.beam_merge(cid, clp, elp, cum.to(dev), n_src)
    assert all(bits_equal(a, b) for a, b in zip(got, again))
    if G == 3 and B > 2 and not n_src_is_b:
        assert got[0][-1].tolist()[2:] == [-1] * (B - 2)    # two candidates, the rest missing
        assert got[3][-1].tolist()[2:] == [-math.inf] * (B - 2)
        assert got[5][-1, 0].item() == 1


def test_beam_merge_checks_its_arguments():
    dev = torch.device("cuda")
    cid = torch.zeros(3, 3, dtype=torch.int32, device=dev)
    clp = torch.zeros(3, 3, device=dev)
    with pytest.raises(ValueError):
        ops.beam_merge(cid, clp, torch.zeros(3, device=dev), torch.zeros(1, 3, device=dev), 2)
    with pytest.raises(ValueError):
        ops.beam_merge(cid, clp, torch.zeros(2, device=dev), torch.zeros(1, 3, device=dev), 3)
    with pytest.raises(ValueError):
        ops.beam_merge(cid, clp, torch.zeros(3, device=dev), torch.zeros(1, 9, device=dev), 1)


def test_kv_copy_blocks():
    dev = torch.device("cuda")
    L, blocks, n_kv, bs, D = 2, 9, 3, 16, 64
    g = torch.Generator().manual_seed(5)
    k = torch.randn(L, blocks, n_kv, bs, D, generator=g).to(torch.bfloat16)
    v = torch.randn(L, blocks, n_kv, bs, D, generator=g).to(torch.bfloat16)
    pairs = [(0, 3), (0, 8), (5, 1), (6, 2)]
    want_k, want_v = k.clone(), v.clone()
    ref.kv_copy_blocks(want_k, want_v, pairs)
    for s, d in pairs:
        assert torch.equal(want_k[:, d], k[:, s]) and not torch.equal(k[:, d], k[:, s])
    dk, dv = k.to(dev), v.to(dev)
    ops.kv_copy_blocks(dk, dv, pairs)
    assert torch.equal(dk.cpu().view(torch.int16), want_k.view(torch.int16))
    assert torch.equal(dv.cpu().view(torch.int16), want_v.view(torch.int16))
    for s, _ in pairs:                                      # the sources are unchanged
        assert torch.equal(dk[:, s].cpu().view(torch.int16), k[:, s].view(torch.int16))
    before = dk.clone()
    for bad in ([(0, 3), (3, 4)], [(0, 3), (1, 3)], [(0, 9)]):
        with pytest.raises(ValueError):
            ops.kv_copy_blocks(dk, dv, bad)
    assert torch.equal(dk, before)                          # rejected before any launch
    ops.kv_copy_blocks(dk, dv, [])
    assert torch.equal(dk, before)
