"""The VITS text-side kernels (``csrc/kernels/tts.hip``), one element at a
time: ``loqa_relpos_attention`` and the noise half of ``loqa_expand_sample``
(its mean gather is exact in ``test_conv_exact.py``). The older test ran one
attention shape under ``||o - ref|| / ||ref|| < 1e-2`` with ``emb_*`` scaled by
0.1 and judged the noise by the mean and standard deviation of one row.

**Operands and guards.** Every operand and every output is a slice of a larger
flat buffer with 64 guard elements before and after it. ``qkv`` rows are
``ld >= 3C`` wide. What the kernel must not read is filled three ways: *cont*
(1000), zeros, NaN: the guards, the ``qkv`` columns beyond ``3C`` and the
``qkv`` rows at ``j >= lens[b]`` (the contract below). Guards of index arrays
hold 0. Outputs start as the sentinel -7. After a launch EVERY buffer is
compared whole: inputs and guards bit for bit with what they held, the output
bitwise or within its bound, and the three fills must give equal bits.

**Contract for padded rows** (decided here): valid output rows do not depend on
what ``qkv`` rows ``j >= lens[b]`` hold, NaN included; output rows
``i >= lens[b]`` are ``+0.0``. VITS runs the kernel at bucketed ``T`` and
nothing else initialises those rows. The kernel did not keep it: its V stage
multiplied ``p[j] = 0`` by the V rows of all ``T`` keys, and ``0 * NaN``
turns every valid row of a sequence with ``len < T`` into NaN (all ``len * C``
elements of such a sequence under the NaN fill; cont and zeros are right).
The CPU reference did the same and failed ``test_checker_passes_*`` that way.
Fixed in ``tts.hip``: the V and ``emb_v`` loops run over ``j < len`` (``len``
clamped to ``T``), which is also less work; on finite rows the bits are
unchanged since the skipped terms were ``+-0``. ``ops.reference`` had the same
``0 * NaN`` and now zeroes the padded rows first. ``ops.relpos_attention``
addressed batch ``b`` at ``b * T * stride(1)`` without checking ``stride(0)``:
a bucket-padded view ``qkv[:, :T]`` was read wrongly in silence; it is refused
now, and ``lens`` must be int32 on the device.

**Selector family, bitwise.** Every softmax is exactly one-hot in f32: the
winner's score exceeds every other (the -1e4 of masked keys included) by more
than 104 (asserted; here >= 128), so ``__expf`` of the rest underflows to 0,
the sum is 1 and the output is ``v[j*] + emb_v[j* - i + window]`` (the
``emb_v`` term only inside the window) in small integers: exact. ``scale = 1``.
Keys and offsets are coded as +-1 bit patterns on dims spread up to ``D - 1``,
queries are 64 times the pattern wanted. The winner is chosen

* ``qk``: through ``q . k`` alone (``emb_k = 0``), ``j* = (5 i + 3 h + b + 1) % len``;
* ``emb``: through ``q . emb_k[r]`` alone (``k = 0``) for each of the
  ``2 window + 1`` offsets in turn (every offset is used, asserted): the output
  names the offset, so a mirrored sign or an edge off by one changes bits;
* ``last``: ``j* = len - 1`` with a score twice as large planted in row
  ``j = len``: the mask must beat it.

Shapes ``(B, T, H, D, window)``: (3, 77, 2, 96, 4) lens (77, 40, 0);
(2, 130, 2, 96, 4) lens (130, 65); (2, 9, 1, 256, 10) lens (9, 5).

**Random family, per-element bound.** ``q, k, v, emb_k, emb_v`` standard
normal, rounded to bf16 (``emb_*`` NOT scaled down, so the relative terms
weigh as much as the keys). Reference: fp64 on the identical bf16 operands,
the ``-1e4`` fill as the kernel has it, ``scale`` the f32 the kernel gets.
With ``u = 2**-24``, ``x_j = s_j - max``, ``p`` the fp64 softmax, ``w_j`` the
value row of key ``j`` (``v_j``, and ``emb_v[j - i + window]`` as a term of
its own inside the window):

* score: ``|ds_j| <= (D + 3) u S_j``, ``S_j = sum_d |q_d scale k_jd| + sum_d
  |q_d scale emb_k[r]_d|``: two dot products of length ``D`` (any order loses
  at most ``D u`` of the absolute sum), the rounding of ``q * scale``, the add
  of the two and the subtraction of the maximum. An error of the maximum
  itself scales numerator and denominator alike and cancels.
* ``__expf``: relative ``eps_j = ds_j + 2 u |x_j| + 4 u``: the argument is
  rounded once as ``s - max`` and once in ``x * log2(e)``, each ``|x_j| u``
  absolute, which is relative in ``e**x``; 4 u for the exp2 itself (2 ulp).
* sums: the denominator has ``T`` terms, the numerator ``len + 2 window + 1``,
  all of the first non-negative: ``T u`` relative there, ``(T + 2 window + 1)
  u`` of ``sum_j p_j |w_j|`` here; 4 u for ``1 / sum``, the product and slack.
* store: ``2**-8 |ref|`` (half a bf16 ulp at worst).

      bound = 2**-8 |ref| + sum_j p_j |w_j| eps_j + (T + 2 window + 5) u sum_j p_j |w_j|
              + |ref| (sum_j p_j eps_j + (T + 4) u)

The second and third terms are proportional to ``sum_j p_j |w_j|``, not to
``|ref|``: the output is a signed sum and may cancel. The dot-product length
enters as ``D`` per product (``D + 2 window + 1`` would mix it with the band
width, which belongs to the value sum). Rows ``i >= len`` are bitwise ``+0.0``.
Every valid row's maximum is above -1e3 (asserted), so masked keys weigh 0 in
fp64 and in f32 alike.

Shapes, with ``lens``: (3, 1, 2, 96, 4) (1, 1, 0); (3, 77, 2, 96, 4)
(77, 50, 1); (2, 130, 2, 96, 4) (130, 129); (2, 512, 1, 64, 4) (512, 300);
(2, 9, 1, 256, 10) (9, 0), window wider than T; (2, 40, 3, 32, 4) (40, 17)
with row stride ``3C + 24``. ``scale`` is the wrapper's default ``1 /
sqrt(D)``. T = 513 and D = 264 are refused and the output keeps its sentinel.
Where the shape allows it the wrapper ``ops.relpos_attention`` must return the
bits of the launcher.

**Noise of ``expand_sample``.** ``ops.reference.gauss_noise(seed, B, F, C)``
reproduces the integer part exactly (``hash32``, the ``idx`` packing with
``idx >> 32``, ``u1``, ``u2``; ``1.0f / 16777217.0f`` is ``2**-24`` since the
divisor is no f32) and runs Box-Muller in fp64 from the f32 uniforms. With
``stats = 0`` and ``noise_scale = 1`` the kernel stores ``bf16(g_device)``.
Every element must equal ``bf16(g64 + t)`` for some ``|t| <= a R``, ``R =
sqrt(-2 ln u1)``: it is ``bf16(g64)`` or, only where ``g64`` lies within ``a
R`` of the rounding boundary, the neighbour. ``a`` is the absolute error of the
fast ``__logf`` / ``__cosf`` pair relative to ``R``, measured on the GPU as the
largest boundary distance of a mismatching element over its ``R``:

    measured 3.101e-07 = 2**-21.62 (``A_MEASURED``);  a = 4 * that = 1.24e-06 = 2**-19.6

(rounding flips are sparse samples of the true error, hence the factor 4).
Whatever is measured, ``a <= 2**-16`` and at most 1 % of the elements may
mismatch ``bf16(g64)`` (the fp64 model against itself: none; a wrong hash:
nearly all). With non-zero ``stats`` at ``noise_scale = 0.667`` the centre is
``m + g64 exp(logs) 0.667`` and the tolerance ``a R s + 8 u |g64| s + u
|centre|``, ``s = exp(logs) 0.667``: the f32 roundings of ``__expf``, the two
products and the add. Frames ``f >= flen[b]`` are ``+0.0`` bits.

Cases ``(B, F, C)``: (2, 37, 192); (24, 3, 192), where ``idx >> 32`` is
non-zero for b = 23 (asserted; it is from b = 2 on, since ``2 * 2**24 * 192 >=
2**32``, and the older test's B = 2 never reached it); seed ``0x80000001`` as
the argument and as the negative int32 ``seed_dev``, the same bits both ways
and at ``F`` and ``F + 96``; a seed solved from the inverse hash so that
element (0, 0, 0) has ``a >> 8 = 0``, the smallest ``u1 = 2**-24`` (``R =
5.77``); non-zero ``stats`` over T = 5 phonemes with one row shorter than F.

**CPU tests that prove the checkers.** A pure-torch / numpy f32 candidate
takes each kernel's place. ``ops.relpos_attention`` on CPU tensors and a clean
f32 candidate that sums every dot product and the value sum sequentially in
REVERSE order pass everything; the fp64 noise model and its f32 twin pass
(the CPU branch of ``ops.expand_sample`` draws ``torch.randn`` and is left as
it is, so it is no candidate).
Each mutant fails, in the elements it touches:

    (a) ``rel`` mirrored in the ``emb_k`` lookup
    (b) ``|rel| < window``
    (c) ``emb_v`` of offset ``r + 1``
    (d) the scale left off the ``emb_k`` term
    (e) keys ``>= len`` unmasked
    (f) a padded query row left as the sentinel
    (g) V of head ``h + 1``
    (h) one element 2 bf16 ulps off
    (i) noise: the channel left out of ``idx``
    (j) noise: ``idx >> 32`` dropped (rows b >= 2 only)
    (k) noise: ``u1`` without its ``+ 1``

(k) moves ``R`` by ``2**-24 / (u1 R)``, far inside ``a R`` unless ``u1`` is
tiny: it fails in the planted element with ``a >> 8 = 0``, where it yields
``inf``, and in no other.

**The old criteria**, measured on the old shape (``test_old_criteria``):

    attention ``_rel`` (accepts below 1e-2), T = 77, D = 96, emb * 0.1
        clean f32 candidate 0.0017   (a) 0.0500   (b) 0.0173   (c) 0.0477
        (d) 0.4858   (e) 0.4234   (f) 16.29   (g) 1.4407   (h) 0.0017
    noise: |mean| and |std - 1| of row 0 (accept below 0.05), 101 x 64 draws
        clean 0.0169 / 0.0108   (i) 0.2367 / 0.1384   (j) the bits of clean
        (k) 0.0169 / 0.0108

(h), (j) and (k) pass the old criteria. (a) to (c) were expected to pass them
too, as a reason for this file; that premise is wrong: on random operands a
wrong relative term moves 2-5 % of the norm even with ``emb_*`` scaled by 0.1,
above the 1 % the old test allowed. The test asserts the measured side of
each. What the old test could not see at all is the NaN
poisoning, the batch stride, ``idx >> 32`` and T past two lane strides.

Measured on an MI355X, worst ``err / bound`` of the random family (the store's
rounding is nearly all of it, as for any accurate candidate; ``MEASURED``):

    (3, 1, 2, 96, 4)   0.9315   (3, 77, 2, 96, 4)  0.9316   (2, 130, 2, 96, 4) 0.9401
    (2, 512, 1, 64, 4) 0.9101   (2, 9, 1, 256, 10) 0.8213   (2, 40, 3, 32, 4)  0.9801

The selector family is bitwise equal in all nine cases, the three fills give
equal buffers (NaN in the padded rows included, after the fix) and no guard or
sentinel is disturbed.
"""
import functools
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import _lib
from loqa_hub_amd.ops import reference as R

# worst err / bound of the random family on an MI355X, by shape (B, T, H, D, window)
MEASURED = {
    (3, 1, 2, 96, 4): 0.9315, (3, 77, 2, 96, 4): 0.9316, (2, 130, 2, 96, 4): 0.9401,
    (2, 512, 1, 64, 4): 0.9101, (2, 9, 1, 256, 10): 0.8213, (2, 40, 3, 32, 4): 0.9801,
}
# largest boundary distance / R of a mismatching noise element on an MI355X
# (2**-21.62; 2 of 44,160 elements mismatch bf16(g64) over the four stats = 0 cases)
A_MEASURED = 3.101e-07
A = 4 * A_MEASURED
A_CAP = 2.0 ** -16

FILLS = ("cont", "zeros", "nan")
_FILLV = {"cont": 1000.0, "zeros": 0.0, "nan": float("nan")}
BF, F32, F64, I16, I32, I64 = (torch.bfloat16, torch.float32, torch.float64, torch.int16, torch.int32,
                               torch.int64)
U = 2.0 ** -24
SENT = -7.0
GUARD = 64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.view({2: I16, 4: I32, 8: I64}[t.element_size()]) if t.is_floating_point() else t


class Buf:
    """``core`` as a view into a flat buffer with guards of ``fv`` around it."""

    def __init__(self, core, fv, dev, view=None):
        n = core.numel()
        flat = torch.full((GUARD + n + GUARD,), fv if core.dtype.is_floating_point else 0, dtype=core.dtype)
        flat[GUARD:GUARD + n] = core.reshape(-1)
        self.before, self.flat = flat.clone(), flat.to(dev)
        shape, stride = view or (tuple(core.shape), core.contiguous().stride())
        self.spec = (shape, stride, GUARD)
        self.v = self.flat.as_strided(*self.spec)

    def of(self, flat):
        return flat.as_strided(*self.spec)

    def unchanged(self):
        return torch.equal(_bits(self.flat.cpu()), _bits(self.before))


def bf16_of(x):
    """fp64 -> bf16, rounded once (through f32 it could round twice)."""
    x32 = x.float()
    tie = (x32.view(I32) & 0xFFFF) == 0x8000
    d = x - x32.double()
    toward = torch.where(d > 0, torch.full_like(x32, math.inf), torch.full_like(x32, -math.inf))
    x32 = torch.where(tie & (d != 0), torch.nextafter(x32, toward), x32)
    return x32.to(BF)


def bf16_step(t, n):
    """The bf16 value ``n`` steps up (down for negative ``n``) from ``t``."""
    i = t.view(I16).to(I32)
    mag = i & 0x7FFF
    o = torch.where(i < 0, -mag, mag) + n
    back = torch.where(o < 0, (-o) | 0x8000, o)
    return torch.where(back >= 0x8000, back - 0x10000, back).to(I16).view(BF)


# ====================================================== relpos_attention
def band(p, W):
    """[..., T, T] -> [..., T, 2W + 1]: ``out[i, r] = p[i, i + r - W]`` (0 outside)."""
    T = p.shape[-1]
    out = torch.zeros(p.shape[:-1] + (2 * W + 1,), dtype=p.dtype)
    for r in range(2 * W + 1):
        off = r - W
        if abs(off) >= T:
            continue
        d = p.diagonal(off, -2, -1)
        if off >= 0:
            out[..., :T - off, r] = d
        else:
            out[..., -off:, r] = d
    return out


def attn_ref64(qkv, ek, ev, lens, H, D, W, scale):
    """fp64 reference on bf16 operands -> (ref, bound, margin): [B, T, C] each,
    ``bound = -1`` in the rows ``i >= len``; margin = the smallest gap between
    the best and the second best score of a valid row."""
    B, T, _ = qkv.shape
    C = H * D
    scale = float(np.float32(scale))
    idx = torch.arange(T)
    valid = idx[None, :] < lens.long()[:, None]
    x = torch.where(valid[..., None], qkv.double(), torch.zeros((), dtype=F64))
    q, k, v = (x[..., n * C:(n + 1) * C].view(B, T, H, D).transpose(1, 2) for n in range(3))
    q = q * scale
    rel = idx[None, :] - idx[:, None]
    inwin = rel.abs() <= W
    ridx = (rel + W).clamp(0, 2 * W)[None, None].expand(B, H, T, T)
    zero = torch.zeros((), dtype=F64)
    s = q @ k.transpose(-1, -2) + torch.where(inwin, (q @ ek.double().t()).gather(-1, ridx), zero)
    Se = (q.abs() @ ek.double().abs().t()).gather(-1, ridx)
    S = q.abs() @ k.abs().transpose(-1, -2) + torch.where(inwin, Se, zero)
    vj = valid[:, None, None, :]
    s = torch.where(vj, s, torch.full((), -1e4, dtype=F64))
    mx = s.amax(-1, keepdim=True)
    vi = valid[:, None, :, None]
    assert bool((mx[vi.expand_as(mx)] > -1e3).all())
    top2 = s.topk(min(2, T), -1).values
    gap = (top2[..., :1] - top2[..., 1:2]) if T > 1 else torch.full_like(mx, math.inf)
    margin = float(gap[vi.expand_as(gap)].min()) if bool(vi.any()) else math.inf
    xj = s - mx
    p = torch.exp(xj)
    p = p / p.sum(-1, keepdim=True)
    eps = torch.where(vj, (D + 3) * U * S + 2 * U * xj.abs() + 4 * U, zero)
    evd = ev.double()
    ref = p @ v + band(p, W) @ evd
    Aw = p @ v.abs() + band(p, W) @ evd.abs()
    AwE = (p * eps) @ v.abs() + band(p * eps, W) @ evd.abs()
    Eavg = (p * eps).sum(-1, keepdim=True)
    bound = 2.0 ** -8 * ref.abs() + AwE + (T + 2 * W + 5) * U * Aw + ref.abs() * (Eavg + (T + 4) * U)
    ref = torch.where(vi, ref, zero)
    bound = torch.where(vi, bound, torch.full((), -1.0, dtype=F64))
    flat = lambda t: t.transpose(1, 2).reshape(B, T, C)
    return flat(ref), flat(bound), margin


def _code(n, nb):
    return torch.tensor([1.0 if (n >> b) & 1 else -1.0 for b in range(nb)])


class AttnCase:
    """One launch of relpos_attention. ``family``: "random" or a selector way."""

    def __init__(self, B, T, H, D, W, lens, pad=0, family="random"):
        self.B, self.T, self.H, self.D, self.W, self.pad, self.family = B, T, H, D, W, pad, family
        self.name = f"relpos-{family}-B{B}-T{T}-H{H}-D{D}-W{W}-pad{pad}"
        self.lens = torch.tensor(lens, dtype=I32)
        self.plant = {}
        C, Rn = H * D, 2 * W + 1
        g = _gen(B + T + H + D + W)
        if family == "random":
            self.scale = 1.0 / math.sqrt(D)
            self.qkv = torch.randn(B, T, 3 * C, generator=g).to(BF)
            self.ek = torch.randn(Rn, D, generator=g).to(BF)
            self.ev = torch.randn(Rn, D, generator=g).to(BF)
        else:
            self.scale = 1.0
            self._selector(g)
        self.ref, self.bound, self.margin = attn_ref64(self._finite(), self.ek, self.ev, self.lens, H, D, W,
                                                       self.scale)
        if family != "random":
            assert self.margin > 104, (self.name, self.margin)
            # in fp64 the losers weigh e**-128, not 0: equal up to that
            assert float((self.ref - self.want.double()).abs().max()) < 1e-40, self.name
            self.ref = self.want.double()
            self.bound = torch.full_like(self.bound, -1.0)

    def _selector(self, g):
        B, T, H, D, W = self.B, self.T, self.H, self.D, self.W
        Rn, nbk = 2 * W + 1, 8
        nbr = max(1, math.ceil(math.log2(Rn)))
        assert T <= 2 ** nbk and D >= nbk
        pk = [(b + 1) * (D // nbk) - 1 for b in range(nbk)]
        pr = [(b + 1) * (D // nbr) - 1 for b in range(nbr)]
        q, k = torch.zeros(B, T, H, D), torch.zeros(B, T, H, D)
        v = torch.randint(-8, 9, (B, T, H, D), generator=g).float()
        self.ev = torch.randint(-4, 5, (Rn, D), generator=g).float().to(BF)
        assert torch.unique(self.ev.float(), dim=0).shape[0] == Rn
        ek = torch.zeros(Rn, D)
        want = torch.zeros(B, T, H, D)
        self.used = set()
        for b in range(B):
            n = int(self.lens[b])
            for h in range(H):
                for i in range(n):
                    if self.family == "emb":
                        r = (i + b + 2 * h) % Rn - W
                        r = r if 0 <= i + r < n else -r if 0 <= i - r < n else 0
                        js = i + r
                        q[b, i, h, pr] = 64 * _code(r + W, nbr)
                        if n == T:
                            self.used.add(r)
                    else:
                        js = n - 1 if self.family == "last" else (5 * i + 3 * h + b + 1) % n
                        q[b, i, h, pk] = 64 * _code(js, nbk)
                    want[b, i, h] = v[b, js, h] + (self.ev[js - i + W].float() if abs(js - i) <= W else 0)
        if self.family == "emb":
            for r in range(Rn):
                ek[r, pr] = _code(r, nbr)
        else:
            for j in range(T):
                k[:, j, :, pk] = _code(j, nbk)
        self.ek = ek.to(BF)
        self.qkv = torch.cat([t.reshape(B, T, H * D) for t in (q, k, v)], -1).to(BF)
        self.want = want.reshape(B, T, H * D).to(BF)
        if self.family == "last":
            for b in range(B):
                n = int(self.lens[b])
                if 0 < n < T:
                    kp = torch.zeros(H, D)
                    kp[:, pk] = 2 * _code(n - 1, nbk)
                    self.plant[(b, n)] = torch.cat([torch.zeros(H * D), kp.reshape(-1),
                                                    torch.full((H * D,), 9.0)])
            assert self.plant

    def _finite(self):
        return self.qkv

    def ground(self, fill, dev):
        B, T, C3 = self.qkv.shape
        fv = _FILLV[fill]
        ld = C3 + self.pad
        rows = torch.full((B, T, ld), fv, dtype=BF)
        rows[..., :C3] = self.qkv
        for b in range(B):
            rows[b, int(self.lens[b]):] = fv
        for (b, j), row in self.plant.items():
            rows[b, j, :C3] = row.to(BF)
        return {"qkv": Buf(rows, fv, dev, ((B, T, C3), (T * ld, ld, 1))),
                "ek": Buf(self.ek, fv, dev), "ev": Buf(self.ev, fv, dev), "lens": Buf(self.lens, 0, dev),
                "out": Buf(torch.full((B, T, C3 // 3), SENT, dtype=BF), SENT, dev)}

    def launch(self, be, g):
        return be.relpos(g["qkv"].v, g["ek"].v, g["ev"].v, g["lens"].v, g["out"].v, self.H, self.D, self.W,
                         self.scale)

    def judge(self, g):
        """-> (bad over the output view, bad over the whole flat output outside the view)."""
        out = g["out"]
        flat = out.flat.cpu()
        got = out.of(flat)
        exact = bf16_of(self.ref)
        bad = _bits(got) != _bits(exact)
        err = (got.double() - self.ref).abs()
        bad = torch.where(self.bound >= 0, ~(err <= self.bound), bad)
        outside = _bits(flat) != _bits(out.before)
        out.of(outside)[...] = False
        pos = self.bound > 0
        worst = float((err[pos] / self.bound[pos]).max()) if bool(pos.any()) else 0.0
        return bad, outside, worst


class Report:
    pass


def run(case, be, dev="cpu", fills=FILLS):
    rep = Report()
    rep.bad, rep.outside, rep.out, rep.inputs_ok, rep.worst, rep.rc = {}, {}, {}, {}, {}, {}
    for f in fills:
        g = case.ground(f, dev)
        rep.rc[f] = case.launch(be, g)
        rep.bad[f], rep.outside[f], rep.worst[f] = case.judge(g)
        rep.out[f] = g["out"].flat.cpu()
        rep.inputs_ok[f] = all(b.unchanged() for n, b in g.items() if n != "out")
    rep.fills_equal = all(torch.equal(_bits(rep.out[f]), _bits(rep.out[fills[0]])) for f in fills[1:])
    return rep


def check(case, be, dev="cpu"):
    rep = run(case, be, dev)
    print(f"tts-exact {be.name} {case.name}: worst err/bound {max(rep.worst.values()):.4f}")
    for f in FILLS:
        assert rep.rc[f] == 0, (case.name, f, rep.rc[f])
        assert rep.inputs_ok[f], (case.name, f, "an input or its guard changed")
        assert not rep.outside[f].any(), (case.name, f, "store outside the output")
        assert not rep.bad[f].any(), (case.name, f, int(rep.bad[f].sum()), "elements differ, first at",
                                      rep.bad[f].nonzero()[:8].tolist())
    assert rep.fills_equal, (case.name, "the fill of unread memory changes the output")
    return rep


class Native:
    """The HIP kernels through their C entry points; where the wrapper can
    take the same operands it must return the same bits."""
    name = "hip"

    def relpos(self, qkv, ek, ev, lens, out, H, D, W, scale):
        B, T, _ = qkv.shape
        rc = _lib.kernels().loqa_relpos_attention(_lib.ptr(qkv), qkv.stride(1), _lib.ptr(ek), _lib.ptr(ev),
                                                  _lib.ptr(lens), _lib.ptr(out), out.stride(1), B, T, H, D, W,
                                                  scale, _lib.stream_ptr(qkv))
        torch.cuda.synchronize()
        if rc == 0:
            got = ops.relpos_attention(qkv, ek, ev, lens, H, D, W, scale)
            assert torch.equal(_bits(got), _bits(out)), "wrapper and launcher differ"
        return rc

    def expand(self, stats, cum, flen, z, noise_scale, seed, seed_dev):
        B, T, C2 = stats.shape
        F = z.shape[1]
        rc = _lib.kernels().loqa_expand_sample(_lib.ptr(stats), stats.stride(1), _lib.ptr(cum), B, T,
                                               _lib.ptr(flen), _lib.ptr(z), F, C2 // 2, noise_scale,
                                               seed & 0xFFFFFFFF, _lib.ptr(seed_dev), _lib.stream_ptr(stats))
        torch.cuda.synchronize()
        got = ops.expand_sample(stats, cum, flen, F, noise_scale, seed=seed, seed_dev=seed_dev)
        assert torch.equal(_bits(got), _bits(z)), "wrapper and launcher differ"
        return rc


class CpuOps:
    name = "ops-cpu"

    def relpos(self, qkv, ek, ev, lens, out, H, D, W, scale):
        out.copy_(ops.relpos_attention(qkv, ek, ev, lens, H, D, W, scale))
        return 0


class Sim:
    """The kernels in plain f32 torch / numpy, every sum sequential in REVERSE
    order, and through ``mut`` their possible faults."""
    name = "sim-fp32"

    def __init__(self, **mut):
        self.mut = mut

    def relpos(self, qkv, ek, ev, lens, out, H, D, W, scale):
        m = self.mut
        B, T, _ = qkv.shape
        C, Rn = H * D, 2 * W + 1
        if T > 512 or D > 256:
            return 1
        idx = torch.arange(T)
        valid = idx[None, :] < lens.long().clamp(max=T)[:, None]
        x = qkv.float()
        if not m.get("unmasked"):
            x = torch.where(valid[..., None], x, torch.zeros(()))
        q, k, v = (x[..., n * C:(n + 1) * C].reshape(B, T, H, D).transpose(1, 2) for n in range(3))
        if m.get("v_head_next"):
            v = v.roll(-1, 1)
        qs = q * torch.tensor(scale, dtype=F32)
        qe = q if m.get("emb_unscaled") else qs
        ekf, evf = ek.float(), ev.float()
        if m.get("emb_v_next"):
            evf = evf.roll(-1, 0)
        s, rl = torch.zeros(B, H, T, T), torch.zeros(B, H, T, Rn)
        for d in reversed(range(D)):
            s = s + qs[..., :, None, d] * k[..., None, :, d]
            rl = rl + qe[..., :, None, d] * ekf[None, None, None, :, d]
        rel = idx[None, :] - idx[:, None]
        inwin = (rel.abs() < W) if m.get("edge") else (rel.abs() <= W)
        if m.get("mirrored"):
            rel = -rel
        ridx = (rel + W).clamp(0, 2 * W)[None, None].expand(B, H, T, T)
        s = s + torch.where(inwin, rl.gather(-1, ridx), torch.zeros(()))
        vj = valid[:, None, None, :]
        if not m.get("unmasked"):
            s = torch.where(vj, s, torch.full((), -1e4))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        tot = torch.zeros(B, H, T)
        acc = torch.zeros(B, H, T, D)
        eb = band(e if m.get("unmasked") else torch.where(vj, e, torch.zeros(())), W)
        for r in reversed(range(Rn)):
            acc = acc + eb[..., r, None] * evf[r]
        for j in reversed(range(T)):
            tot = tot + e[..., j]
            acc = acc + e[..., j, None] * v[..., None, j, :]
        o = (acc * (1.0 / tot)[..., None]).transpose(1, 2).reshape(B, T, C).to(BF)
        if m.get("pad_row_sentinel"):
            o = torch.where(valid[..., None], o, out)
        else:
            o = torch.where(valid[..., None], o, torch.zeros((), dtype=BF))
        if "bump" in m:
            at, n = m["bump"]
            o[at] = bf16_step(o[at].reshape(1), n)[0]
        out.copy_(o)
        return 0

    def expand(self, stats, cum, flen, z, noise_scale, seed, seed_dev):
        m = self.mut
        B, T, C2 = stats.shape
        F, C = z.shape[1], C2 // 2
        if seed_dev is not None:
            seed = int(seed_dev[0])
        f32 = np.float32
        b = np.arange(B, dtype=np.uint64)[:, None, None]
        f = np.arange(F, dtype=np.uint64)[None, :, None]
        c = np.arange(C, dtype=np.uint64)[None, None, :]
        idx = ((b << np.uint64(24)) + f) * np.uint64(C) + (c * np.uint64(0) if m.get("no_channel") else c)
        lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hi = (idx >> np.uint64(32)).astype(np.uint32)
        if m.get("no_hi"):
            hi = hi * np.uint32(0)
        a = R.hash32(np.uint32(seed & 0xFFFFFFFF) ^ R.hash32(lo ^ np.uint32(0x9E3779B9)) ^ hi)
        c2 = R.hash32(a ^ np.uint32(0x85EBCA6B))
        u1 = ((a >> np.uint32(8)) + np.uint32(0 if m.get("u1_no_plus1") else 1)).astype(f32) * f32(2.0 ** -24)
        u2 = (c2 >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)
        with np.errstate(divide="ignore"):
            g = np.sqrt(f32(-2) * np.log(u1)) * np.cos(f32(6.283185307179586) * u2)
        assert g.dtype == f32
        g = torch.from_numpy(g)
        o = torch.zeros(B, F, C)
        for bi in range(B):
            n = int(flen[bi])
            i = torch.searchsorted(cum[bi].long(), torch.arange(n), right=True)
            mm, lg = stats[bi, i, :C].float(), stats[bi, i, C:].float()
            o[bi, :n] = mm + g[bi, :n] * torch.exp(lg) * torch.tensor(noise_scale, dtype=F32)
        z.copy_(o.to(BF))
        return 0


@functools.lru_cache(maxsize=None)
def attn_case(*args):
    return AttnCase(*args)


RANDOM = [((3, 1, 2, 96, 4), (1, 1, 0), 0), ((3, 77, 2, 96, 4), (77, 50, 1), 0),
          ((2, 130, 2, 96, 4), (130, 129), 0), ((2, 512, 1, 64, 4), (512, 300), 0),
          ((2, 9, 1, 256, 10), (9, 0), 0), ((2, 40, 3, 32, 4), (40, 17), 24)]
SELECT = [((3, 77, 2, 96, 4), (77, 40, 0)), ((2, 130, 2, 96, 4), (130, 65)), ((2, 9, 1, 256, 10), (9, 5))]
WAYS = ("qk", "emb", "last")
_sid = lambda s: "-".join(map(str, s[0]))


# ------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("spec", RANDOM, ids=_sid)
def test_relpos_random_gpu(spec):
    shape, lens, pad = spec
    rep = check(attn_case(*shape, lens, pad, "random"), Native(), "cuda")
    print(f"tts-exact MEASURED {shape}: {max(rep.worst.values()):.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("spec", SELECT, ids=_sid)
def test_relpos_selector_gpu(spec, way):
    shape, lens = spec
    check(attn_case(*shape, lens, 0, way), Native(), "cuda")


def _refused(be, dev):
    for shape, lens in (((1, 513, 1, 32, 4), (513,)), ((1, 4, 1, 264, 4), (4,))):
        B, T, H, D, W = shape
        g = _gen(T)
        c = AttnCase.__new__(AttnCase)
        c.B, c.T, c.H, c.D, c.W, c.pad, c.plant, c.scale = B, T, H, D, W, 0, {}, 1.0
        c.qkv = torch.randn(B, T, 3 * H * D, generator=g).to(BF)
        c.ek = torch.randn(2 * W + 1, D, generator=g).to(BF)
        c.ev = torch.randn(2 * W + 1, D, generator=g).to(BF)
        c.lens = torch.tensor(lens, dtype=I32)
        gr = c.ground("cont", dev)
        rc = be.relpos(gr["qkv"].v, gr["ek"].v, gr["ev"].v, gr["lens"].v, gr["out"].v, H, D, W, 1.0)
        assert rc != 0, shape
        assert all(b.unchanged() for b in gr.values()), (shape, "a refused launch wrote something")


@pytest.mark.gpu
def test_relpos_refused_gpu():
    """T = 513 and D = 264 return an error; the output keeps its sentinel."""
    _refused(Native(), "cuda")
    K = _lib.kernels()
    out = torch.full((8,), SENT, dtype=BF, device="cuda")
    assert K.loqa_relpos_attention(None, 0, None, None, None, _lib.ptr(out), 0, 0, 4, 1, 32, 4, 1.0,
                                   _lib.stream_ptr(out)) == 0          # B = 0: nothing to do
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


@pytest.mark.gpu
def test_relpos_batch_stride_gpu():
    """A bucket-padded view ``qkv[:, :T]`` has a batch stride the kernel cannot
    address: refused, as ``expand_sample`` refuses its ``stats``. ``lens``
    must be int32 on the device."""
    c = attn_case(2, 40, 3, 32, 4, (40, 17), 24, "random")
    big = torch.zeros(2, 48, 3 * 96, dtype=BF, device="cuda")
    big[:, :40] = c.qkv.cuda()
    ek, ev, lens = c.ek.cuda(), c.ev.cuda(), c.lens.cuda()
    with pytest.raises(AssertionError, match="batch stride"):
        ops.relpos_attention(big[:, :40], ek, ev, lens, 3, 32, 4)
    with pytest.raises(AssertionError, match="lens"):
        ops.relpos_attention(big[:, :40].contiguous(), ek, ev, lens.long(), 3, 32, 4)
    with pytest.raises(AssertionError, match="lens"):
        ops.relpos_attention(big[:, :40].contiguous(), ek, ev, c.lens, 3, 32, 4)
    # the same rows, made contiguous or as one sequence of a padded batch, are served
    want = ops.relpos_attention(big[:, :40].contiguous(), ek, ev, lens, 3, 32, 4)
    one = ops.relpos_attention(big[1:, :40], ek, ev, lens[1:].contiguous(), 3, 32, 4)
    assert torch.equal(_bits(one[0]), _bits(want[1]))
    ref, bound, _ = attn_ref64(c.qkv, c.ek, c.ev, c.lens, 3, 32, 4, 1 / math.sqrt(32))
    err = (want.cpu().double() - ref).abs()
    assert bool((err <= bound.clamp(min=0)).all())


# ================================================================= noise
def solve_seed(a, idx_lo=0):
    """The seed for which the element with ``idx = idx_lo`` (< 2**32) has the
    first hash ``a``: ``hash32`` is a bijection and inverted step by step."""
    M = 1 << 32
    x = a
    x ^= x >> 16
    x = x * pow(0x846CA68B, -1, M) % M
    x ^= (x >> 15) ^ (x >> 30)
    x = x * pow(0x7FEB352D, -1, M) % M
    x ^= x >> 16
    inner = int(R.hash32(np.array([idx_lo ^ 0x9E3779B9], dtype=np.uint32))[0])
    return x ^ inner


class NoiseCase:
    def __init__(self, B, F, C, seed, dev_seed=False, stats=False, F_launch=None):
        self.B, self.F, self.C, self.seed, self.dev_seed = B, F_launch or F, C, seed, dev_seed
        self.name = f"noise-B{B}-F{self.F}-C{C}-seed{seed:#x}-dev{int(dev_seed)}-stats{int(stats)}"
        g = _gen(B + F + C)
        if stats:
            self.T, self.ns = 5, 0.667
            self.stats = (0.5 * torch.randn(B, self.T, 2 * C, generator=g)).to(BF)
            dur = torch.randint(1, F // self.T + 1, (B, self.T), generator=g)
            dur[0, -1] += F - int(dur[0].sum())          # row 0 fills F, the others stay shorter
            self.cum = dur.cumsum(1).to(I32)
        else:
            self.T, self.ns = 1, 1.0
            self.stats = torch.zeros(B, 1, 2 * C, dtype=BF)
            self.cum = torch.full((B, 1), F, dtype=I32)
        self.flen = self.cum[:, -1].contiguous()
        assert int(self.flen.max()) == F and (not stats or int(self.flen.min()) < F)
        F = self.F
        a, u1, u2 = R.gauss_uniforms(seed, B, F, C)
        self.a_hash = a
        g64 = torch.from_numpy(R.gauss_noise(seed, B, F, C))
        self.Rr = torch.from_numpy(np.sqrt(-2.0 * np.log(u1.astype(np.float64))))
        ns = float(np.float32(self.ns))
        fr = torch.arange(F)
        i = torch.stack([torch.searchsorted(self.cum[b].long(), fr, right=True).clamp(max=self.T - 1)
                         for b in range(B)])
        st = self.stats.double()[torch.arange(B)[:, None], i]
        m, lg = st[..., :C], st[..., C:]
        s = torch.exp(lg) * ns
        self.live = (fr[None, :] < self.flen[:, None].long())[..., None].expand(B, F, C)
        self.center = torch.where(self.live, m + g64 * s, torch.zeros((), dtype=F64))
        self.unit = torch.where(self.live, self.Rr * s, torch.zeros((), dtype=F64))
        self.extra = 8 * U * g64.abs() * s + U * self.center.abs()
        if not stats:
            self.extra = torch.zeros_like(self.center)
        self.extra = torch.where(self.live, self.extra, torch.zeros((), dtype=F64))

    def ground(self, fill, dev):
        fv = _FILLV[fill]
        g = {"stats": Buf(self.stats, fv, dev), "cum": Buf(self.cum, 0, dev), "flen": Buf(self.flen, 0, dev),
             "out": Buf(torch.full((self.B, self.F, self.C), SENT, dtype=BF), SENT, dev)}
        if self.dev_seed:
            s = self.seed - (1 << 32) if self.seed >= 1 << 31 else self.seed
            g["seed"] = Buf(torch.tensor([s], dtype=I32), 0, dev)
        return g

    def launch(self, be, g):
        return be.expand(g["stats"].v, g["cum"].v, g["flen"].v, g["out"].v, self.ns,
                         0 if self.dev_seed else self.seed, g["seed"].v if self.dev_seed else None)

    def judge(self, g, a=None):
        """-> (bad, outside, stats): an element is right iff it is
        ``bf16(centre + t)`` for some ``|t| <= a * unit + extra``."""
        a = A if a is None else a
        out = g["out"]
        flat = out.flat.cpu()
        got = out.of(flat)
        tol = a * self.unit + self.extra
        lo, hi, mid = bf16_of(self.center - tol), bf16_of(self.center + tol), bf16_of(self.center)
        gf = got.float()
        bad = ~((lo.float() <= gf) & (gf <= hi.float()))
        bad |= ~self.live & (_bits(got) != 0)
        mism = (_bits(got) != _bits(mid)) & self.live
        # the smallest |t| that rounds to what was stored, over the element's unit
        up = gf > mid.float()
        edge = torch.where(up, (bf16_step(got, -1).double() + got.double()) / 2,
                           (bf16_step(got, 1).double() + got.double()) / 2)
        need = ((edge - self.center).abs() - self.extra).clamp(min=0) / self.unit.clamp(min=1e-300)
        seen = mism & torch.isfinite(gf)
        a_seen = float(need[seen].max()) if bool(seen.any()) else 0.0
        outside = _bits(flat) != _bits(out.before)
        out.of(outside)[...] = False
        return bad, outside, dict(a_seen=a_seen, mismatch=float(mism.float().sum() / self.live.float().sum()))


def check_noise(case, be, dev="cpu"):
    outs = {}
    for f in FILLS:
        g = case.ground(f, dev)
        assert case.launch(be, g) == 0
        bad, outside, st = case.judge(g)
        print(f"tts-exact {be.name} {case.name} {f}: a_seen 2**{math.log2(max(st['a_seen'], 1e-300)):.2f}, "
              f"mismatching {st['mismatch']:.5f}")
        assert all(b.unchanged() for n, b in g.items() if n != "out"), (case.name, f)
        assert not outside.any(), (case.name, f, "store outside the output")
        assert not bad.any(), (case.name, f, int(bad.sum()), bad.nonzero()[:8].tolist())
        assert st["mismatch"] <= 0.01 and A <= A_CAP
        outs[f] = g["out"].flat.cpu()
    assert all(torch.equal(_bits(outs[f]), _bits(outs["cont"])) for f in FILLS)
    return g["out"].of(outs["cont"]), st


SEED_NEG = 0x80000001
SEED_TAIL = solve_seed(5)          # element (0, 0, 0): a = 5, a >> 8 = 0, u1 = 2**-24


@functools.lru_cache(maxsize=None)
def noise_case(*args):
    return NoiseCase(*args)


NOISE = [(2, 37, 192, 7), (24, 3, 192, 7), (2, 37, 192, SEED_NEG), (2, 5, 192, SEED_TAIL)]


def _noise_all(be, dev):
    for spec in NOISE:
        check_noise(noise_case(*spec), be, dev)
    c = noise_case(24, 3, 192, 7)
    idx23 = (23 << 24) * 192
    assert idx23 >> 32 != 0 and (1 << 24) * 192 + 3 * 192 < 1 << 32 <= (2 << 24) * 192
    # the seed as the argument and read on the device, at F and at F + 96
    z0, _ = check_noise(noise_case(2, 37, 192, SEED_NEG), be, dev)
    z1, _ = check_noise(noise_case(2, 37, 192, SEED_NEG, True), be, dev)
    z2, _ = check_noise(noise_case(2, 37, 192, SEED_NEG, True, False, 37 + 96), be, dev)
    assert torch.equal(_bits(z0), _bits(z1)) and torch.equal(_bits(z0), _bits(z2[:, :37]))
    assert not _bits(z2[:, 37:]).any()
    # gather and noise together
    z3, _ = check_noise(noise_case(3, 37, 192, 11, False, True), be, dev)
    z4, _ = check_noise(noise_case(3, 37, 192, 11, True, True, 37 + 96), be, dev)
    assert torch.equal(_bits(z3), _bits(z4[:, :37]))
    return c


@pytest.mark.gpu
def test_noise_gpu():
    _noise_all(Native(), "cuda")
    # the measurement behind A_MEASURED: the bound wide open, the largest need
    worst = 0.0
    for spec in NOISE:
        c = noise_case(*spec)
        g = c.ground("cont", "cuda")
        c.launch(Native(), g)
        worst = max(worst, c.judge(g, A_CAP)[2]["a_seen"])
    print(f"tts-exact noise A_MEASURED candidate: {worst:.3e} = 2**{math.log2(max(worst, 1e-300)):.2f}")
    assert worst <= A


# ------------------------------------------------------------- CPU tests
BACKENDS = [CpuOps(), Sim()]


@pytest.mark.parametrize("be", BACKENDS, ids=lambda b: b.name)
@pytest.mark.parametrize("spec", RANDOM, ids=_sid)
def test_checker_passes_random(spec, be):
    shape, lens, pad = spec
    check(attn_case(*shape, lens, pad, "random"), be)


@pytest.mark.parametrize("be", BACKENDS, ids=lambda b: b.name)
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("spec", SELECT, ids=_sid)
def test_checker_passes_selector(spec, way, be):
    shape, lens = spec
    c = attn_case(*shape, lens, 0, way)
    check(c, be)
    if way == "emb" and shape[1] > 2 * shape[4] + 1:
        assert c.used == set(range(-shape[4], shape[4] + 1))


def test_checker_refused():
    _refused(Sim(), "cpu")


def _rows(bad):
    """(b, i) of the output rows with a wrong element."""
    return {tuple(r) for r in bad.any(-1).nonzero().tolist()}


def _valid_rows(c):
    return {(b, i) for b in range(c.B) for i in range(min(int(c.lens[b]), c.T))}


SEL = ((3, 77, 2, 96, 4), (77, 40, 0))


def test_mutant_mirrored_and_edge():
    """(a) mirrored ``rel``: in the ``emb`` selector every row whose offset is
    not 0 picks another key or none; (b) ``|rel| < window``: exactly the rows
    whose offset is +-window; neither shows where ``emb_k = 0``."""
    c = attn_case(*SEL[0], SEL[1], 0, "emb")
    B, T, H, D, W = SEL[0]
    off = {}
    for b in range(B):
        n = int(c.lens[b])
        for i in range(n):
            for h in range(H):
                r = (i + b + 2 * h) % (2 * W + 1) - W
                r = r if 0 <= i + r < n else -r if 0 <= i - r < n else 0
                off.setdefault((b, i), set()).add(r)
    rep = run(c, Sim(mirrored=True))
    want = {k for k, rs in off.items() if rs != {0}}
    # the mirrored key may be masked and the right one the nearest code left: a few rows survive
    for f in FILLS:
        rows = _rows(rep.bad[f])
        assert rows <= want and len(rows) >= 0.9 * len(want) and not rep.outside[f].any()
    rep = run(c, Sim(edge=True))
    for f in FILLS:
        assert _rows(rep.bad[f]) == {k for k, rs in off.items() if rs & {W, -W}}
    for mut in ("mirrored", "edge"):
        rep = run(attn_case(*SEL[0], SEL[1], 0, "qk"), Sim(**{mut: True}), fills=("cont",))
        assert not rep.bad["cont"].any()
        cr = attn_case(3, 77, 2, 96, 4, (77, 50, 1), 0, "random")
        rows = _rows(run(cr, Sim(**{mut: True}), fills=("cont",)).bad["cont"])
        assert rows and rows <= _valid_rows(cr)


def test_mutant_emb_v_next_and_head():
    """(c) ``emb_v`` of offset ``r + 1``: every row whose winner lies inside
    the window; (g) V of head ``h + 1``: every valid row."""
    for way in ("qk", "emb"):
        c = attn_case(*SEL[0], SEL[1], 0, way)
        rep = run(c, Sim(emb_v_next=True), fills=("cont",))
        rows = _rows(rep.bad["cont"])
        assert rows and rows <= _valid_rows(c)
        if way == "emb":
            assert rows == _valid_rows(c)
        rep = run(c, Sim(v_head_next=True), fills=("cont",))
        assert _rows(rep.bad["cont"]) == _valid_rows(c)
    c = attn_case(2, 130, 2, 96, 4, (130, 129), 0, "random")
    for mut in ("emb_v_next", "v_head_next"):
        assert _rows(run(c, Sim(**{mut: True}), fills=("cont",)).bad["cont"]) == _valid_rows(c)


def test_mutant_emb_unscaled():
    """(d) the scale left off the ``emb_k`` term (random family; the selector
    runs at scale 1)."""
    c = attn_case(3, 77, 2, 96, 4, (77, 50, 1), 0, "random")
    rep = run(c, Sim(emb_unscaled=True), fills=("cont",))
    rows = _rows(rep.bad["cont"])
    assert rows <= _valid_rows(c) and len(rows) >= 0.9 * len(_valid_rows(c))


def test_mutant_unmasked_and_pad_row():
    """(e) keys ``>= len`` unmasked: the planted key wins every row of the
    ``last`` selector, and under the NaN fill every valid row of a short
    sequence is NaN; (f) a padded query row left as the sentinel."""
    c = attn_case(*SEL[0], SEL[1], 0, "last")
    short = {(b, i) for (b, i) in _valid_rows(c) if int(c.lens[b]) < c.T}
    rep = run(c, Sim(unmasked=True))
    for f in FILLS:
        assert _rows(rep.bad[f]) == short, f
    assert not rep.fills_equal
    c = attn_case(3, 77, 2, 96, 4, (77, 50, 1), 0, "random")
    short = {(b, i) for (b, i) in _valid_rows(c) if int(c.lens[b]) < c.T}
    rep = run(c, Sim(unmasked=True))
    # cont: the padded keys all score 1000 * scale * sum(q), which half the queries have below 0
    assert _rows(rep.bad["nan"]) == short and len(short) / 4 < len(_rows(rep.bad["cont"])) and \
        _rows(rep.bad["cont"]) <= short
    for cc in (c, attn_case(*SEL[0], SEL[1], 0, "qk")):
        rep = run(cc, Sim(pad_row_sentinel=True), fills=("cont",))
        every = {(b, i) for b in range(cc.B) for i in range(cc.T)}
        assert _rows(rep.bad["cont"]) == every - _valid_rows(cc) and not rep.outside["cont"].any()


@pytest.mark.parametrize("spec", RANDOM[1:], ids=_sid)
def test_mutant_one_element(spec):
    """(h) one element off by 2 bf16 ulps, where the store term dominates:
    exactly that element fails."""
    shape, lens, pad = spec
    c = attn_case(*shape, lens, pad, "random")
    at = tuple(int(i) for i in (c.ref.abs() == c.ref.abs().max()).nonzero()[0])
    for n in (2, -2):
        rep = run(c, Sim(bump=(at, n)), fills=("cont",))
        assert rep.bad["cont"].nonzero().tolist() == [list(at)]


# ---- noise: the host model and the checker
class Model64:
    """The fp64 host model in the kernel's place."""
    name = "model-fp64"

    def expand(self, stats, cum, flen, z, noise_scale, seed, seed_dev):
        B, T, C2 = stats.shape
        F, C = z.shape[1], C2 // 2
        if seed_dev is not None:
            seed = int(seed_dev[0])
        g = torch.from_numpy(R.gauss_noise(seed & 0xFFFFFFFF, B, F, C))
        o = torch.zeros(B, F, C, dtype=F64)
        for b in range(B):
            n = int(flen[b])
            i = torch.searchsorted(cum[b].long(), torch.arange(n), right=True)
            o[b, :n] = (stats[b, i, :C].double() + g[b, :n] * torch.exp(stats[b, i, C:].double())
                        * float(np.float32(noise_scale)))
        z.copy_(bf16_of(o))
        return 0


def test_noise_checker_passes():
    _noise_all(Sim(), "cpu")
    _noise_all(Model64(), "cpu")
    for spec in NOISE:
        c = noise_case(*spec)
        g = c.ground("cont", "cpu")
        c.launch(Model64(), g)
        assert c.judge(g)[2]["mismatch"] == 0.0


def test_noise_mutants():
    """(i) the channel left out of ``idx``: nearly everything; (j) ``idx >>
    32`` dropped: nearly everything in the rows b >= 2 and nothing below;
    (k) ``u1`` without ``+ 1``: the planted element (0, 0, 0), inf, alone."""
    c = noise_case(2, 37, 192, 7)
    g = c.ground("cont", "cpu")
    c.launch(Sim(no_channel=True), g)
    bad, _, st = c.judge(g)
    assert float(bad.float().mean()) > 0.9 and st["mismatch"] > 0.9
    c = noise_case(24, 3, 192, 7)
    g = c.ground("cont", "cpu")
    c.launch(Sim(no_hi=True), g)
    bad, _, _ = c.judge(g)
    assert not bad[:2].any() and float(bad[2:].float().mean()) > 0.9
    assert bool(bad[2:].reshape(22, -1).any(1).all())
    c = noise_case(2, 37, 192, 7)           # B = 2 never reaches the term
    g = c.ground("cont", "cpu")
    c.launch(Sim(no_hi=True), g)
    assert not c.judge(g)[0].any()
    c = noise_case(2, 5, 192, SEED_TAIL)
    assert int(c.a_hash[0, 0, 0]) >> 8 == 0
    g = c.ground("cont", "cpu")
    c.launch(Sim(u1_no_plus1=True), g)
    assert c.judge(g)[0].nonzero().tolist() == [[0, 0, 0]]
    assert math.isinf(float(g["out"].v[0, 0, 0]))


def test_noise_host_model_statistics():
    """2 x 64 x 192 draws of the host model: mean and variance within 4
    standard errors, no first hash shared by two triples, lag-1 correlation
    along c and along f below 4 standard errors."""
    for seed in (7, SEED_NEG):
        a, u1, u2 = R.gauss_uniforms(seed, 2, 64, 192)
        g = R.gauss_noise(seed, 2, 64, 192)
        n = g.size
        assert float(u1.min()) > 0 and float(u1.max()) <= 1 and float(u2.min()) >= 0 and float(u2.max()) < 1
        assert abs(g.mean()) < 4 / math.sqrt(n)
        assert abs(g.var() - 1) < 4 * math.sqrt(2 / n)
        assert np.unique(a).size == n
        for x, y in ((g[:, :, :-1], g[:, :, 1:]), (g[:, :-1], g[:, 1:])):
            assert abs(float((x * y).mean())) < 4 / math.sqrt(x.size)
    assert np.array_equal(R.gauss_noise(7, 3, 8, 16)[:2, :5], R.gauss_noise(7, 2, 5, 16))


# ---- what the old criteria saw (tests/test_kernels_gpu.py::test_relpos_attention_and_expand)
def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def old_criteria():
    g = _gen(0)
    B, T, H, D, W = 2, 77, 2, 96, 4
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(BF)
    ek = (torch.randn(2 * W + 1, D, generator=g).to(BF).float() * 0.1).to(BF)
    ev = (torch.randn(2 * W + 1, D, generator=g).to(BF).float() * 0.1).to(BF)
    lens = torch.tensor([T, 50], dtype=I32)
    sc = 1 / math.sqrt(D)
    want = R.relpos_attention(qkv, ek, ev, lens, H, D, W, sc)
    out = {}
    at = tuple(int(i) for i in (want.abs() == want.abs().max()).nonzero()[0])
    muts = {"clean": {}, "a": dict(mirrored=True), "b": dict(edge=True), "c": dict(emb_v_next=True),
            "d": dict(emb_unscaled=True), "e": dict(unmasked=True), "f": dict(pad_row_sentinel=True),
            "g": dict(v_head_next=True), "h": dict(bump=(at, 2))}
    for name, m in muts.items():
        o = torch.full((B, T, H * D), SENT, dtype=BF)
        Sim(**m).relpos(qkv, ek, ev, lens, o, H, D, W, sc)
        out[name] = _rel(o, want)
    F, C = 101, 64
    cum, flen = torch.full((B, 1), F, dtype=I32), torch.full((B,), F, dtype=I32)
    for name, m in {"clean": {}, "i": dict(no_channel=True), "j": dict(no_hi=True),
                    "k": dict(u1_no_plus1=True)}.items():
        z = torch.zeros(B, F, C, dtype=BF)
        Sim(**m).expand(torch.zeros(B, 1, 2 * C, dtype=BF), cum, flen, z, 1.0, 7, None)
        out["noise-" + name] = (abs(float(z[0].float().mean())), abs(float(z[0].float().std()) - 1))
    return out


def test_old_criteria():
    """The measured side of each (module docstring): the old ratio accepts the
    clean candidate and (h); it rejects (a), (c)-(g) on random operands even
    with ``emb_*`` scaled by 0.1, and (b) too. The old noise criterion accepts
    (j) and (k), which leave B = 2 rows untouched, and rejects (i)."""
    r = old_criteria()
    for k, v in r.items():
        print(f"tts-exact old criterion {k}: {v}")
    assert r["clean"] < 1e-2 and r["h"] < 1e-2
    for k in "abcdefg":
        assert r[k] > 1e-2, k
    assert max(r["noise-clean"]) < 0.05
    assert r["noise-j"] == r["noise-clean"] and max(r["noise-k"]) < 0.05
    assert max(r["noise-i"]) > 0.05
