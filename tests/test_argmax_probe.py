"""``ops.masked_argmax_logprob_probe``: ``ops.masked_argmax_logprob`` plus the
log-softmax of one fixed column per row BEFORE the mask
(``csrc/kernels/elementwise.hip``, ``masked_argmax_kernel<.., 2>`` +
``argmax_finalize_kernel<2>``; on the CPU
``ops.reference.masked_argmax_logprob_probe``).

**Bitwise against the sibling.** ``idx`` and ``lp`` equal
``ops.masked_argmax_logprob`` on the same inputs bit for bit on every row,
probing or not, and two runs agree bitwise on all three outputs.

**Probe value**, against fp64 computed from the stored logit values:
``x[p] - logsumexp(x over ALL columns 0..V-1)``. The kernel returns
``(x[p] - m) - logf(s)`` with ``m`` the row maximum and
``s = sum exp(x - m) >= 1`` over all columns, accumulated exactly as the
sibling accumulates its masked sum. With ``u = 2**-24`` and every logit of
columns ``0..V-1`` in ``[-R, R]``, ``R = 22`` (the masked-out columns too: they
enter this sum, so here they hold ordinary logits, not the hostile fill):

* the relative error of ``s`` and the ``logf`` are those of
  ``tests/test_argmax_logprob.py`` applied to the all-column sum:
  ``6u * depth + 4R u + 4u ln V`` with
  ``depth = n_t + n_t / vec + 6 + 3 + chunks - 1``,
  ``n_t = vec * ceil(min(V, 8192) / (256 * vec))`` (vec = 4 for f32, 8 for bf16);
* two roundings more: ``d = x[p] - m`` with ``|d| <= 2R`` is off by at most
  ``2R u``, and ``d - log s`` with ``|result| <= 2R + ln V`` by at most
  ``(2R + ln V) u``: together ``(4R + ln V) u``.

``probe_bound = 6u * depth + 4R u + 4u ln V + (4R + ln V) u``: 3.4e-5 at
V = 51866, f32. The fp64 oracle's own error is far below ``u``.

**Hostile memory.** The logits are the view ``[:B, :V]`` of a ``[B + 2, ld]``
buffer; columns ``>= V`` and rows ``>= B`` hold a value 20 above the row
maximum, so one of them leaking into either sum moves a result by ~20. A
masked-out logit planted 10 above the allowed maximum must leave ``lp`` bitwise
unchanged and move the probe value by ~10.

**Positions.** The probe column at 0, V - 1, 8191, 8192, at the last element of
a partial vector group, on a masked-out column and on the row maximum, its logit
10 away from every other: dropping it, or taking a neighbour's, moves the
result by ~10.
"""
import math

import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops.reference import pack_mask

R = 22.0          # logits of columns < V: |x| <= 12, a planted one at most 10 above
U = 2.0 ** -24
CHUNK, THREADS = 8192, 256

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
VS = [1, 7, 8191, 8192, 8193, 51866]
BS = [1, 3, 16]


def sibling_bound(V: int, dtype) -> float:
    """The bound of tests/test_argmax_logprob.py (-log s of one accumulated sum)."""
    vec = 8 if dtype == torch.bfloat16 else 4
    n_t = vec * math.ceil(min(V, CHUNK) / (THREADS * vec))
    chunks = math.ceil(V / CHUNK)
    depth = n_t + n_t // vec + 6 + 3 + chunks - 1
    return 6 * U * depth + 4 * R * U + 4 * U * math.log(max(V, 2))


def probe_bound(V: int, dtype) -> float:
    return sibling_bound(V, dtype) + (4 * R + math.log(max(V, 2))) * U


def test_bound_is_the_derived_figure():
    assert sibling_bound(51866, torch.float32) == pytest.approx(2.75e-5, rel=0.02)
    assert probe_bound(51866, torch.float32) == pytest.approx(3.34e-5, rel=0.02)
    assert probe_bound(7, torch.float32) < probe_bound(8193, torch.float32) \
        < probe_bound(51866, torch.float32)


def _ld(V: int, kind: str) -> int:
    if kind == "eq":
        return V
    if kind == "odd":              # ld % 8 != 0 and ld % 4 != 0: the scalar path
        return (V + 3) | 1
    ld = -(-V // 64) * 64          # the lm_head GEMM's padded row
    return ld if ld > V else ld + 64


_CACHE: dict = {}


def make_case(B, V, dtype, ld_kind, mask_kind, seed=0):
    """CPU tensors: (buffer [B + 2, ld], allowed bool [B, V], mask, mask_rows,
    probe int32 [B]). Every column < V holds an ordinary logit, allowed or not.
    Rows with b % 3 == 1 do not probe. Built once per shape and shared between
    the CPU and the GPU run."""
    key = (B, V, dtype, ld_kind, mask_kind, seed)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + B)
    ld = _ld(V, ld_kind)
    x = (torch.randn(B, V, generator=g) * 6).clamp_(-12, 12).to(dtype)
    if mask_kind == "none":
        allowed = torch.ones(B, V, dtype=torch.bool)
        mask = rows = None
    elif mask_kind == "shared":
        a = torch.rand(1, V, generator=g) < 0.5
        a[0, torch.randint(V, (1,), generator=g)] = True
        allowed = a.expand(B, V).clone()
        # a table of two rows; every logits row points at row 1
        mask = torch.cat([torch.zeros_like(pack_mask(a)), pack_mask(a)])
        rows = torch.ones(B, dtype=torch.int32)
    else:
        allowed = torch.rand(B, V, generator=g) < 0.5
        allowed[torch.arange(B), torch.randint(V, (B,), generator=g)] = True
        mask, rows = pack_mask(allowed), None
    hostile = x.float().max(dim=1, keepdim=True).values + 20      # <= 32
    buf = (hostile.max() * torch.ones(B + 2, ld)).to(dtype)
    buf[:B] = hostile.expand(B, ld).to(dtype)
    buf[:B, :V] = x
    probe = torch.randint(V, (B,), generator=g).to(torch.int32)
    probe[torch.arange(B) % 3 == 1] = -1
    out = (buf, allowed, mask, rows, probe)
    _CACHE[key] = out
    return out


def oracle(view: torch.Tensor, allowed: torch.Tensor, probe: torch.Tensor):
    """fp64 from the stored values: (winner column, its log-softmax over the
    allowed columns, the probed column's log-softmax over all columns; 0 where
    the row does not probe)."""
    x = view.double().cpu()
    xm = x.masked_fill(~allowed, float("-inf"))
    col = xm.argmax(dim=1)
    lp = xm.gather(1, col[:, None])[:, 0] - torch.logsumexp(xm, dim=1)
    p = probe.long()
    plp = x.gather(1, p.clamp(min=0)[:, None])[:, 0] - torch.logsumexp(x, dim=1)
    return col, lp, torch.where(p >= 0, plp, torch.zeros_like(plp))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32)


def run(buf, B, V, mask, rows, probe, dev, token_ids=None):
    d = torch.device(dev)
    view = buf.to(d)[:B, :V]
    assert view.stride(0) == buf.shape[1]
    m = None if mask is None else mask.to(d)
    r = None if rows is None else rows.to(d)
    t = None if token_ids is None else token_ids.to(d)
    p = probe.to(d)
    idx, lp, plp = ops.masked_argmax_logprob_probe(view, m, r, p, token_ids=t)
    assert idx.dtype == torch.int32 and lp.dtype == plp.dtype == torch.float32
    assert idx.shape == lp.shape == plp.shape == (B,)
    # the sibling's two results, bit for bit, on every row
    want_idx, want_lp = ops.masked_argmax_logprob(view, m, r, token_ids=t)
    assert torch.equal(idx, want_idx), (idx, want_idx)
    assert torch.equal(bits(lp), bits(want_lp)), (lp, want_lp)
    # determinism: bitwise, run to run
    idx2, lp2, plp2 = ops.masked_argmax_logprob_probe(view, m, r, p, token_ids=t)
    assert torch.equal(idx, idx2) and torch.equal(bits(lp), bits(lp2))
    assert torch.equal(bits(plp), bits(plp2))
    # a row that does not probe: exactly +0.0
    off = (probe < 0) | (probe >= V)
    assert (bits(plp.cpu())[off] == 0).all(), plp
    return idx.cpu(), lp.cpu(), plp.cpu()


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mask_kind", ["none", "shared", "per_row"])
@pytest.mark.parametrize("ld_kind", ["eq", "odd", "pad64"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_argmax_probe(V, dtype, ld_kind, mask_kind, dev):
    """Mixed batches: rows 1, 4, 7, ... do not probe (B = 1: the row probes)."""
    for B in BS:
        buf, allowed, mask, rows, probe = make_case(B, V, dtype, ld_kind, mask_kind)
        idx, lp, plp = run(buf, B, V, mask, rows, probe, dev)
        col, want_lp, want = oracle(buf[:B, :V], allowed, probe)
        err_lp = (lp.double() - want_lp).abs().max().item()
        err = (plp.double() - want).abs().max().item()
        print(f"V={V} B={B} {dtype} {ld_kind} {mask_kind} {dev}: probe err {err:.3e} "
              f"bound {probe_bound(V, dtype):.3e}, lp err {err_lp:.3e}")
        assert torch.equal(idx.long(), col)
        assert torch.isfinite(plp).all() and (plp <= 0).all()
        assert err_lp <= sibling_bound(V, dtype), (err_lp, sibling_bound(V, dtype))
        assert err <= probe_bound(V, dtype), (err, probe_bound(V, dtype))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("where", ["allowed", "masked_out", "row_max"])
@pytest.mark.parametrize("V,col", [(51866, 0), (51866, 51865), (51866, 8191), (51866, 8192),
                                   (8193, 8192), (8197, 8196), (7, 6)])
def test_probe_positions(V, col, where, dtype, dev):
    """The probed logit is 10 away from every other logit of the row.
    (8193, 8192) is a second chunk of one element, (8197, 8196) and
    (51866, 51865) the last element of a partial vector group, (7, 6) a row
    without a full group. ``allowed``: 10 below the row minimum, on an allowed
    column; ``masked_out``: 10 above the row maximum, on a masked-out column
    (``lp`` must not see it: the bitwise check in ``run``); ``row_max``: 10
    above, allowed, so it is the winner as well."""
    B = 3
    for ld_kind in ("eq", "pad64"):
        buf, allowed, _, _, _ = make_case(B, V, dtype, ld_kind, "per_row", seed=3)
        buf, allowed = buf.clone(), allowed.clone()
        x = buf[:B, :V].float()
        if where == "allowed":
            buf[:B, col] = (x.min(dim=1).values - 10).to(dtype)       # >= -22
        else:
            buf[:B, col] = (x.max(dim=1).values + 10).to(dtype)       # <= 22
        allowed[:, col] = where != "masked_out"
        if where == "masked_out" and not allowed.any(dim=1).all():    # V = 7: keep one allowed
            allowed[:, 0] = True
        probe = torch.full((B,), col, dtype=torch.int32)
        idx, lp, plp = run(buf, B, V, pack_mask(allowed), None, probe, dev)
        wcol, want_lp, want = oracle(buf[:B, :V], allowed, probe)
        assert torch.equal(idx.long(), wcol)
        if where == "row_max":
            assert idx.tolist() == [col] * B
        assert (lp.double() - want_lp).abs().max().item() <= sibling_bound(V, dtype)
        assert (plp.double() - want).abs().max().item() <= probe_bound(V, dtype)
        if where == "allowed":
            assert (plp < -9.5).all()          # a neighbour's logit: about 10 higher
        else:
            assert (plp > -2.0).all()          # without it: -10 or lower


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,col", [(7, 2), (8193, 8192), (51866, 30001)])
def test_masked_out_logit_enters_the_probe_sum_only(V, col, dtype, dev):
    B = 3
    for ld_kind in ("odd", "pad64"):
        buf, allowed, _, _, probe = make_case(B, V, dtype, ld_kind, "per_row", seed=6)
        buf, allowed = buf.clone(), allowed.clone()
        allowed[:, col] = False
        allowed[:, (col + 1) % V] = True          # the allowed maximum is the row's
        buf[:B, (col + 1) % V] = buf[:B, :V].float().max(dim=1).values.to(dtype)
        probe = torch.full((B,), (col + 3) % V, dtype=torch.int32)
        mask = pack_mask(allowed)
        _, lp0, plp0 = run(buf, B, V, mask, None, probe, dev)
        top = buf[:B, :V].float().masked_fill(~allowed, -12.0).max(dim=1).values
        buf[:B, col] = (top + 10).to(dtype)       # masked out, 10 above the allowed maximum
        idx, lp, plp = run(buf, B, V, mask, None, probe, dev)
        _, want_lp, want = oracle(buf[:B, :V], allowed, probe)
        assert torch.equal(bits(lp), bits(lp0))   # lp never sees it
        assert (lp.double() - want_lp).abs().max().item() <= sibling_bound(V, dtype)
        assert (plp.double() - want).abs().max().item() <= probe_bound(V, dtype)
        assert (plp0 - plp > 1.0).all(), (plp0, plp)     # the probe sum does


@pytest.mark.parametrize("dev", DEVICES)
def test_token_ids(dev):
    B, V = 3, 8193
    buf, allowed, mask, rows, probe = make_case(B, V, torch.float32, "pad64", "per_row", seed=1)
    ids = (torch.arange(V + 5) * 3 + 5).to(torch.int32)
    idx, lp, plp = run(buf, B, V, mask, rows, probe, dev, token_ids=ids)
    col, want_lp, want = oracle(buf[:B, :V], allowed, probe)
    assert torch.equal(idx.long(), col * 3 + 5)       # the probe stays a column
    assert (lp.double() - want_lp).abs().max().item() <= sibling_bound(V, torch.float32)
    assert (plp.double() - want).abs().max().item() <= probe_bound(V, torch.float32)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("V", [7, 8192, 51866])
def test_edge_rows(V, dev):
    B = 3
    buf, allowed, _, _, _ = make_case(B, V, torch.float32, "pad64", "none", seed=5)
    probe = torch.tensor([V - 1, 0, -1], dtype=torch.int32)
    allowed = allowed.clone()
    allowed[1] = False                            # row 1: nothing allowed, still probed
    idx, lp, plp = run(buf, B, V, pack_mask(allowed), None, probe, dev)
    _, _, want = oracle(buf[:B, :V], allowed, probe)
    assert idx[1].item() == -1 and lp[1].item() == float("-inf")
    assert (plp.double() - want).abs().max().item() <= probe_bound(V, torch.float32)
    assert math.isfinite(plp[1].item()) and plp[1].item() < 0
    buf = buf.clone()
    buf[1, :V] = float("-inf")                    # row 1: every logit -inf
    buf[0, V - 1] = float("-inf")                 # row 0: the probed logit alone
    idx, lp, plp = run(buf, B, V, None, None, probe, dev)
    assert not torch.isnan(lp).any() and not torch.isnan(plp).any()
    assert lp[1].item() == float("-inf") and plp[1].item() == float("-inf")
    assert plp[0].item() == float("-inf") and math.isfinite(lp[0].item())


def test_probe_column_outside_the_row():
    B, V = 3, 8193
    buf, _, _, _, _ = make_case(B, V, torch.float32, "pad64", "none", seed=5)
    probe = torch.tensor([0, V, -1], dtype=torch.int32)
    with pytest.raises(ValueError, match="probe"):     # the host knows: rejected
        ops.masked_argmax_logprob_probe(buf[:B, :V], None, None, probe)


@pytest.mark.gpu
@pytest.mark.parametrize("V", [7, 8193])
def test_probe_column_outside_the_row_on_the_device(V):
    """The host does not read a device ``probe``: the kernel treats a column
    >= V as < 0 (+0.0, and no read past the row; columns >= V are hostile)."""
    B = 3
    buf, allowed, _, _, _ = make_case(B, V, torch.float32, "pad64", "none", seed=5)
    probe = torch.tensor([V, V + 1, 2 ** 31 - 1], dtype=torch.int32)
    _, _, plp = run(buf, B, V, None, None, probe, "cuda")
    assert (bits(plp) == 0).all()
