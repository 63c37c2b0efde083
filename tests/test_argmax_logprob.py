"""``ops.masked_argmax_logprob``: the masked argmax and the log-probability of
the token it selects (``csrc/kernels/elementwise.hip``,
``masked_argmax_kernel<.., 1>`` + ``argmax_finalize_kernel<1>``; on the CPU
``ops.reference.masked_argmax_logprob``).

**Index.** ``torch.equal`` to ``ops.masked_argmax`` on the same inputs: winner,
lowest-index tie rule (one exact tie inside a chunk, one across two chunks),
``token_ids`` mapping, -1 when nothing is allowed.

**Log-probability**, against fp64 computed from the stored logit values:
``x[sel] - logsumexp(x over the allowed columns)``. The winner is the maximum
``m``, so the kernel returns ``-log(s)`` with ``s = sum exp(x - m) >= 1`` and an
absolute error of the result is a relative error of ``s``. With ``u = 2**-24``
and allowed logits in ``[-R, R]``:

* a thread accumulates ``n_t = vec * ceil(min(V, 8192) / (256 * vec))`` terms
  (vec = 4 for f32, 8 for bf16; 32 for a full chunk) with an online softmax:
  ``s += expf(x - m)``, ONE ``expf`` per element, and ``s *= expf(m - m')``
  when a vector group raises the thread's maximum, at most once per group
  (the scalar path rescales inside the same step instead: fewer steps).
  ``expf`` and ``logf`` are budgeted at 2 ulp = 4u relative (HIP's math API
  lists both at 1 ulp), plus one rounding for the multiply and one for the
  add: ``6u`` per step, and every term takes part in at most
  ``n_t + n_t / vec`` steps;
* the reduction is 6 shuffle merges (64 lanes), 3 merges of the 4 waves and
  ``chunks - 1`` merges of the chunk records; a merge is
  ``s1 * expf(m1 - m) + s2 * expf(m2 - m)``: again ``6u`` on each summand. So
  ``depth = n_t + n_t / vec + 6 + 3 + chunks - 1`` steps of ``6u``;
* the exponents: a term's own ``d = x - m`` is rounded once, ``|d| <= 2R``, an
  absolute ``2R u`` on the exponent = relative on the term; the rescale
  exponents along a term's chain of maxima are each rounded once and their
  magnitudes sum to at most ``2R`` (the maxima only rise): another ``2R u``;
* one ``logf`` of ``s <= V``: ``4u * ln V``; the final ``0 - log`` is exact.

``bound = 6u * depth + 4R u + 4u ln V``: 2.8e-5 at R = 22, V = 51866, f32.
The fp64 oracle's own error (1e-16 relative) is far below ``u``.

**Hostile memory.** The logits are the view ``[:B, :V]`` of a ``[B + 2, ld]``
buffer; columns ``>= V``, rows ``>= B`` and every masked-out token hold a value
20 above the row maximum, so any of them leaking in moves the result by ~20.

**Presence.** A dominant allowed logit (10 above the rest) at column 0, V - 1,
8191, 8192 and at the last element of a partial vector group: dropping it
changes the index and moves the log-probability by ~10.
"""
import math

import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops.reference import pack_mask

R = 22.0          # allowed logits: |x| <= 12, a planted maximum at most 10 above
U = 2.0 ** -24
CHUNK, THREADS = 8192, 256

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
VS = [1, 7, 8191, 8192, 8193, 51866]
BS = [1, 3, 16]


def bound(V: int, dtype) -> float:
    vec = 8 if dtype == torch.bfloat16 else 4
    n_t = vec * math.ceil(min(V, CHUNK) / (THREADS * vec))
    chunks = math.ceil(V / CHUNK)
    depth = n_t + n_t // vec + 6 + 3 + chunks - 1
    return 6 * U * depth + 4 * R * U + 4 * U * math.log(max(V, 2))


def test_bound_is_the_derived_figure():
    assert bound(51866, torch.float32) == pytest.approx(2.75e-5, rel=0.02)
    assert bound(7, torch.float32) < bound(8193, torch.float32) < bound(51866, torch.float32)


def _ld(V: int, kind: str) -> int:
    if kind == "eq":
        return V
    if kind == "odd":              # ld % 8 != 0 and ld % 4 != 0: the scalar path
        return (V + 3) | 1
    ld = -(-V // 64) * 64          # the lm_head GEMM's padded row
    return ld if ld > V else ld + 64


_CACHE: dict = {}


def make_case(B, V, dtype, ld_kind, mask_kind, seed=0):
    """CPU tensors: (buffer [B + 2, ld], allowed bool [B, V], mask, mask_rows).
    Built once per shape and shared between the CPU and the GPU run."""
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
    buf[:B, :V] = torch.where(allowed, x, hostile.expand(B, V).to(dtype))
    out = (buf, allowed, mask, rows)
    _CACHE[key] = out
    return out


def oracle(view: torch.Tensor, allowed: torch.Tensor):
    """fp64 from the stored values: (column of the winner, its log-softmax)."""
    x = view.double().cpu().masked_fill(~allowed, float("-inf"))
    col = x.argmax(dim=1)
    lp = x.gather(1, col[:, None])[:, 0] - torch.logsumexp(x, dim=1)
    return col, lp


def run(buf, B, V, mask, rows, dev, token_ids=None):
    d = torch.device(dev)
    view = buf.to(d)[:B, :V]
    assert view.stride(0) == buf.shape[1]
    m = None if mask is None else mask.to(d)
    r = None if rows is None else rows.to(d)
    t = None if token_ids is None else token_ids.to(d)
    idx, lp = ops.masked_argmax_logprob(view, m, r, token_ids=t)
    want_idx = ops.masked_argmax(view, m, r, token_ids=t)
    assert idx.dtype == torch.int32 and lp.dtype == torch.float32
    assert idx.shape == lp.shape == (B,)
    assert torch.equal(idx, want_idx), (idx, want_idx)
    idx2, lp2 = ops.masked_argmax_logprob(view, m, r, token_ids=t)
    # determinism: bitwise, run to run
    assert torch.equal(idx, idx2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))
    return idx.cpu(), lp.cpu()


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mask_kind", ["none", "shared", "per_row"])
@pytest.mark.parametrize("ld_kind", ["eq", "odd", "pad64"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_argmax_logprob(V, dtype, ld_kind, mask_kind, dev):
    for B in BS:
        buf, allowed, mask, rows = make_case(B, V, dtype, ld_kind, mask_kind)
        idx, lp = run(buf, B, V, mask, rows, dev)
        col, want = oracle(buf[:B, :V], allowed)
        err = (lp.double() - want).abs().max().item()
        print(f"V={V} B={B} {dtype} {ld_kind} {mask_kind} {dev}: err {err:.3e} "
              f"bound {bound(V, dtype):.3e}")
        assert torch.equal(idx.long(), col)
        assert torch.isfinite(lp).all() and (lp <= 0).all()
        assert err <= bound(V, dtype), (err, bound(V, dtype))


@pytest.mark.parametrize("dev", DEVICES)
def test_token_ids(dev):
    B, V = 3, 8193
    buf, allowed, mask, rows = make_case(B, V, torch.float32, "pad64", "per_row", seed=1)
    ids = (torch.arange(V + 5) * 3 + 5).to(torch.int32)
    idx, lp = run(buf, B, V, mask, rows, dev, token_ids=ids)
    col, want = oracle(buf[:B, :V], allowed)
    assert torch.equal(idx.long(), col * 3 + 5)
    assert (lp.double() - want).abs().max().item() <= bound(V, torch.float32)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("a,b", [(100, 5000), (8000, 9000)], ids=["in_chunk", "across_chunks"])
def test_exact_tie_goes_to_the_lowest_index(a, b, dtype, dev):
    B, V = 3, 51866
    buf, allowed, mask, rows = make_case(B, V, dtype, "pad64", "shared", seed=2)
    buf = buf.clone()
    top = buf[:B, :V].float().masked_fill(~allowed, -12.0).max().item()
    for c in (a, b):
        allowed = allowed.clone()
        allowed[:, c] = True
        buf[:B, c] = top + 1.0          # exact in bf16 too (|top| <= 12)
    mask = torch.cat([torch.zeros_like(pack_mask(allowed[:1])), pack_mask(allowed[:1])])
    idx, lp = run(buf, B, V, mask, rows, dev)
    _, want = oracle(buf[:B, :V], allowed)
    assert idx.tolist() == [a] * B
    assert (lp.double() - want).abs().max().item() <= bound(V, dtype)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,col", [(51866, 0), (51866, 51865), (51866, 8191), (51866, 8192),
                                   (8193, 8192), (8197, 8196), (7, 6)])
def test_presence(V, col, dtype, dev):
    """A dominant allowed logit (10 above the rest). (8193, 8192) is a second
    chunk of one element, (8197, 8196) and (51866, 51865) the last element of a
    partial vector group, (7, 6) a row without a full group."""
    B = 3
    for ld_kind in ("eq", "pad64"):
        buf, allowed, mask, rows = make_case(B, V, dtype, ld_kind, "per_row", seed=3)
        buf, allowed = buf.clone(), allowed.clone()
        top = buf[:B, :V].float().masked_fill(~allowed, -12.0).max(dim=1).values
        allowed[:, col] = True
        buf[:B, col] = (top + 10).to(dtype)       # still 10 under the hostile fill
        idx, lp = run(buf, B, V, pack_mask(allowed), None, dev)
        _, want = oracle(buf[:B, :V], allowed)
        assert idx.tolist() == [col] * B
        assert (lp.double() - want).abs().max().item() <= bound(V, dtype)
        assert (lp > -1.0).all()                  # without it: about -10


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,col", [(7, 3), (8193, 8192), (51866, 49999)])
def test_single_allowed_token_is_exactly_zero(V, col, dtype, dev):
    B = 3
    buf, _, _, _ = make_case(B, V, dtype, "pad64", "none", seed=4)
    buf = torch.full_like(buf, 20.0)              # everything else is hostile
    buf[:B, col] = torch.tensor([-3.25, 0.0, 7.5]).to(dtype)
    allowed = torch.zeros(B, V, dtype=torch.bool)
    allowed[:, col] = True
    idx, lp = run(buf, B, V, pack_mask(allowed), None, dev)
    assert idx.tolist() == [col] * B
    assert lp.tolist() == [0.0] * B


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("V", [7, 8192, 51866])
def test_nothing_allowed_and_all_minus_inf(V, dev):
    B = 3
    buf, allowed, _, _ = make_case(B, V, torch.float32, "pad64", "none", seed=5)
    allowed = allowed.clone()
    allowed[1] = False                            # row 1: nothing allowed
    idx, lp = run(buf, B, V, pack_mask(allowed), None, dev)
    assert idx[1].item() == -1 and lp[1].item() == float("-inf")
    assert idx[0].item() >= 0 and math.isfinite(lp[0].item()) and math.isfinite(lp[2].item())
    buf = buf.clone()
    buf[1, :V] = float("-inf")                    # row 1: every logit -inf
    idx, lp = run(buf, B, V, None, None, dev)     # (the index check is in run)
    assert not torch.isnan(lp).any()
    assert lp[1].item() == float("-inf") and math.isfinite(lp[0].item())
