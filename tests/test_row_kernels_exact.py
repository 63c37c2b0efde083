"""The kernels between the GEMMs, one element at a time: the norms and embeds
(``csrc/kernels/norm.hip``), the split-K slab consumers (``slab_ops.hip``) and
the stream kernels of ``elementwise.hip`` (SwiGLU, bias+GELU(+pos), both
RoPE/KV-append forms, both PCM16 forms). A whole-tensor norm ratio cannot see a
statistic that leaves out one 16-byte vector, one wrong RoPE group, one head not
appended, a row gathered from the neighbouring index or a store next to the
output. Two input families and one checker, as in ``test_conv_exact.py``.

**Every operand is a slice of a larger flat buffer** with a guard band of at
least one row (rounded up to 8 elements, so the 16-byte alignment the kernels
need is kept) before and after it; ``qkv`` is the column view at offset 8 of a
buffer 24 columns wider than needed, with a guard row above and below. The
guards and the rows a kernel must not read (``x`` / ``part`` / ``residual``
rows not named by ``row_idx``, embedding and cos/sin table rows no token names,
cache slots no token writes) are filled three ways: *cont* (1000: finite and
dominating), zeros, NaN. Guards of index arrays hold 0, a valid index whose
use shows in the values. Everything a kernel writes (``y``, ``residual``,
``q_out``, ``qkv``, both caches, ``out``, ``rowsq`` / ``rowsum``, ``sumsq``)
lies in a buffer of this kind; output buffers and the cache slots that are
written start as a sentinel (-7; NaN for the padded PCM rows), not zeros. The
checker builds the buffer it expects from the buffer before the launch and
compares EVERY buffer of the launch whole, inputs included: bitwise outside the
bounded elements. The three fills must give bitwise equal buffers wherever the
buffers were equal before the launch. Rows with ``slots[t] = -1`` leave every
cache byte as it was while their ``q`` is still rotated.

**Integer family, bitwise** (``rope_kv_append`` both forms,
``slab_rope_append``, ``slab_reduce``, ``slab_bias_act("none")``,
``embed_pos``, the row copy of ``embed_stats``). The cos/sin table is an
argument, so it is synthetic: ``cs[p, c] = ((2p + c) % 5 - 2, (p + 3c + p // 5)
% 5 - 2)``, integers in [-2, 2] that differ between any two of the nine
positions and between neighbouring columns, row 0 = (1, 0). ``q``, ``k``, ``v`` are integers in
[-8, 8], slab entries integers whose S-way sum stays in [-8, 8], bias integers
in [-4, 4]: every product and sum is an integer below 256, exact in fp32 and in
bf16, so kernel and ``ops.reference`` agree bitwise. T = 7 (slabs: T = Mpad =
16), ``blk = 4``, slots shuffled and slot 0 unused, ``-1`` rows at position 0
and at another position, one repeated position. The launcher takes the batched form iff
``(Hq + Hkv) * D/8 <= 1024 and Hkv * D/8 <= 128``:

    (5, 1, 64)     48 groups,   8 V pieces   batched, q/k boundary inside a pass
    (8, 2, 128)   160,         32            batched
    (56, 8, 128) 1024,        128            batched, exactly full
    (57, 8, 128) 1040                        loop (one group over)
    (20, 20, 64)  320,        160            loop (V pieces), cos_sin=None: Whisper
    (4, 16, 128)  320,        256            loop through the V limit alone

PCM16: the input is a permutation of all 65536 int16 values; segment lengths
{1, 0, 8191, 8192, 8193, ld, ld + 5} with ``ld = 8292`` (two chunks, no
multiple of ``PCM_CHUNK``), the third segment starting at sample 1; the
unpadded form adds two segments for the rest of the values, the padded form
runs on the array and on its reverse, which together convert every value.
Samples equal ``float32(x) * float32(1 / 32767)`` bitwise, which is within one
fp32 ulp (measured: 0.52) of ``x / 32767`` in fp64; padding is ``+0.0`` bits
over a NaN-filled ``out``; ``sumsq`` is within ``n * 2**-24 * sum`` of the fp64
sum of the stored samples' squares (``n`` the kept length; all terms are
non-negative, so any order stays within it), 0 for the empty segment. No
segment spans more than two chunks, so the atomic sums are order independent.

**Random family, per-element bound.** bf16 random operands (fp32 slabs);
reference fp64 on the identically rounded operands. What a kernel rounds to
bf16 on the way is bitwise first: the updated ``residual``, the slab sum in
kernel order ``s = 0..S-1`` in fp32, the bf16 projection output of
``slab_layernorm`` / ``slab_silu_mul`` / ``slab_bias_act("gelu")`` - the fp64
reference starts from those bits. With ``u = 2**-24`` and the store term
``st = 2**-8 * |ref|`` (half a bf16 ulp at worst):

* rmsnorm, slab_rmsnorm: ``st + (d + 16) u |ref|`` - a sum of ``d``
  non-negative squares loses at most ``d u`` relative in any order; ``16 u``
  for ``rsqrtf``, ``/ d``, ``+ eps`` and two multiplies.
* layernorm, slab_layernorm: ``st + |w| dmu / sigma + (d + 16) u |ref - b| +
  4 u |ref|`` with ``dmu = d u mean|s|``, ``sigma = sqrt(var + eps)``, ``mu``
  and ``var`` in fp64. Odd rows have mean 3 and std 1, so the mean's error
  matters; every row has ``sigma >= |mu| / 8`` (asserted).
* embed_stats: ``rowsq`` within ``d u sum x**2``, ``rowsum`` within ``d u
  sum |x|`` of the fp64 sums of the stored bf16 row.
* silu_mul, slab_silu_mul: ``st + (|g| + 16) u |ref|``, ``|g| <= 16``
  (``__expf`` rounds its argument: ``|g| u`` relative).
* gelu_bias_, slab_bias_act("gelu"): ``st + 8 u |ref| + |v| 2**-21 + u |pos|``,
  ``v`` the pre-activation, ``|v| <= 8``; the absolute term is the error of
  ``erff`` through ``0.5 v (1 + erf)``, which cancels for negative ``v``.

Shapes: norm widths ``d/8`` in {1, 255, 256, 257, 1024} (1280 too for
layernorm), 5 rows, ``row_idx = [4, 0, 2, 2, 1]`` over 6 rows; slab consumers S
in {1, 3}, ``Mpad = 16``, widths {8, 2056}, ``row_idx`` with
``write_residual=False`` (a duplicate index with a residual write would race);
``silu_mul`` / ``gelu_bias_`` F = 8 with 65539 rows (two launches, ``pos`` of
period 7) and F = 2056 with 3 rows, ``bias`` and ``pos`` on and off. ``d = 12``,
``d = 8200`` and ``row_idx`` with ``residual`` are refused and write nothing.

**CPU tests that prove the checker**: a pure-torch candidate takes the kernel's
place. ``ops.*`` on CPU tensors and an fp32 candidate whose statistics are
summed sequentially in REVERSE order pass everything. Each of these mutants
fails, in the elements it touches:

    (a) the norm statistic leaves out the row's last 8 columns
    (b) ``row_idx[i]`` replaced by ``i``
    (c) the weight shifted by 8 columns
    (d) the RoPE partner taken 4 columns off
    (e) the position of token ``t + 1``
    (f) K of head ``h`` appended at head ``h + 1``
    (g) a ``-1`` row appended at slot 0
    (h) V of the last head not appended
    (i) slab ``S - 1`` left out
    (j) ``pos[row]`` instead of ``pos[row % period]``
    (k) the second 65535-row launch starting at row 0
    (l) one element off by 2 bf16 ulps
    (m) q of a ``-1`` row left unrotated

(a) moves a row by 0.2% at d = 2056, inside ``st`` for most elements: it is
caught in the elements it pushes over a rounding boundary: some in every row,
more than 2% of all. (m) needs a ``-1`` row at a position other than 0, whose
table row (1, 0) is the identity: every case has ``-1`` rows at position 0 and
at another one (asserted in ``test_tables``).

**The old criterion** (``|y - ref| / |ref| < 1e-2`` on dense operands, zero
caches), ``test_old_criterion_accepts``, measured:

    clean fp32 candidate, d = 4096, 37 rows                       0.00011
    (a) statistic without the last 8 columns, d = 4096, 37 rows   0.00234
    (l) one element off by 2 bf16 ulps                            0.00019
    (h) V of the last head not appended, zero cache, Hkv = 2      0.69881

(a) and (l) pass the old criterion. (h) was expected to pass it with a
zero-initialised cache, as a reason for writing this file; that premise is
wrong, and the test asserts the opposite: (h) is rejected, zero cache or not,
because leaving out one of Hkv heads costs ``sqrt(1 / Hkv)`` of the norm whatever the cache
held before (and ``test_rope_kv_append`` compares V with ``torch.equal``).
What a zero cache hides is a missed append of zeros and a store to a slot
nobody reads back; here the written slots start as a sentinel and the others
are compared too. The test asserts the measured side of each.

Worst ``err / bound`` on an MI355X (random family; the store's rounding is
nearly all of it, as for any accurate candidate):

    rmsnorm       0.9647   layernorm      0.9681   silu_mul      0.9956
    slab_rmsnorm  0.9629   slab_layernorm 0.9647   gelu_bias_    0.9959
    slab_silu_mul 0.9917   slab_bias_act("gelu")   0.9748
    embed_stats   rowsq 0.0008, rowsum 0.0000      pcm16 sumsq   0.3771

(``sumsq``: the one-sample segment, whose bound is one rounding of ``f * f``.)

The integer family is bitwise equal in both RoPE forms and every slab consumer,
the three fills give equal buffers and no sentinel is disturbed: no kernel
needed a fix. Two CPU branches did: ``ops.embed_pos`` / ``ops.embed_stats``
indexed ``tok_embed[-1]`` for a negative id where the kernels clamp to row 0,
and the PCM16 references divided by 32767 where the kernels multiply by
``float32(1 / 32767)`` (1536 of 65536 values differ in the last bit).
"""
import functools
import math

import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import _lib
from loqa_hub_amd.ops import reference as R

FILLS = ("cont", "zeros", "nan")
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
I16, I32, I64 = torch.int16, torch.int32, torch.int64
U = 2.0 ** -24
SENT = -7.0
EPS = 1e-5
IDX = (4, 0, 2, 2, 1)
_FILLV = {"cont": 1000.0, "zeros": 0.0, "nan": float("nan")}
_FILL16 = {"cont": 1000, "zeros": 0, "nan": -32768}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _bits(t):
    return t.view({2: I16, 4: I32, 8: I64}[t.element_size()]) if t.is_floating_point() else t


# ------------------------------------------------------------------- buffers
class Ground:
    """The buffers of one launch: every operand a view into a flat buffer of
    its own with guard bands, on ``dev``."""

    def __init__(self, fill, dev):
        self.fill, self.dev, self.flat, self.spec, self.v = fill, dev, {}, {}, {}

    def fillv(self, dtype):
        if dtype.is_floating_point:
            return _FILLV[self.fill]
        return _FILL16[self.fill] if dtype == I16 else 0

    def hide(self, core, rows):
        """``core`` with the given rows (first dim) replaced by the fill."""
        core = core.clone()
        if rows:
            core[list(rows)] = self.fillv(core.dtype)
        return core

    def put(self, name, core, sent=None, col=None):
        """``core`` (CPU) -> a view of its shape inside a flat buffer filled
        with the fill (``sent``: with a sentinel). ``col``: a column view of a
        buffer 24 columns wider, one guard row above and below."""
        if core is None:
            self.v[name] = None
            return None
        fv = self.fillv(core.dtype) if sent is None else sent
        n = core.numel()
        if col is None:
            gd = max(8, -(-core.shape[-1] // 8) * 8)
            flat = torch.full((gd + n + gd,), fv, dtype=core.dtype)
            flat[gd:gd + n] = core.reshape(-1)
            flat = flat.to(self.dev)
            v = flat[gd:gd + n].view(core.shape)
        else:
            T, W = core.shape
            buf = torch.full((T + 2, W + 24), fv, dtype=core.dtype)
            buf[1:T + 1, col:col + W] = core
            flat = buf.to(self.dev).view(-1)
            v = flat.view(T + 2, W + 24)[1:T + 1, col:col + W]
        self.flat[name], self.v[name] = flat, v
        self.spec[name] = (tuple(v.shape), v.stride(), v.storage_offset())
        return v

    def out(self, name, shape, dtype=BF, sent=SENT):
        return self.put(name, torch.full(shape, sent, dtype=dtype), sent=sent)

    def snapshot(self):
        return {n: f.cpu().clone() for n, f in self.flat.items()}

    def view(self, name, flats):
        """The operand's view into another set of flat buffers (CPU clones)."""
        return flats[name].as_strided(*self.spec[name]) if name in self.spec else None

    def bounded(self, name, ref, bound, ex):
        """Elements of ``name`` compared with ``ref`` (fp64) within ``bound``."""
        if name not in ex.ref64:
            n = ex.exp[name].numel()
            ex.ref64[name] = torch.zeros(n, dtype=F64)
            ex.bnd[name] = torch.full((n,), -1.0, dtype=F64)
        self.view(name, ex.ref64)[...] = ref
        self.view(name, ex.bnd)[...] = bound


class Expect:
    """What the buffers of one launch must hold afterwards: ``exp`` bitwise,
    except where ``bnd >= 0``: there within ``bnd`` of ``ref64``."""

    def __init__(self, before):
        self.exp = {n: b.clone() for n, b in before.items()}
        self.ref64, self.bnd = {}, {}


class Report:
    def __init__(self, case):
        self.case, self.g, self.before, self.after, self.ex = case, {}, {}, {}, {}

    def bad(self, fill="cont"):
        """name -> bool over the whole flat buffer: elements that are not what
        was expected (NaN misses every bound)."""
        ex, out = self.ex[fill], {}
        for name, a in self.after[fill].items():
            b = _bits(a) != _bits(ex.exp[name])
            if name in ex.bnd:
                err = (a.double() - ex.ref64[name]).abs()
                b = torch.where(ex.bnd[name] >= 0, ~(err <= ex.bnd[name]), b)
            out[name] = b
        return out

    def bad_view(self, name, fill="cont"):
        return self.g[fill].view(name, self.bad(fill))

    def bad_outside(self, name, fill="cont"):
        b = {name: self.bad(fill)[name].clone()}
        self.g[fill].view(name, b)[...] = False
        return b[name]

    def bad_names(self, fill="cont"):
        return {n for n, b in self.bad(fill).items() if b.any()}

    def fills_equal(self):
        fs = list(self.after)
        for name in self.after[fs[0]]:
            b0, a0 = _bits(self.before[fs[0]][name]), _bits(self.after[fs[0]][name])
            same = torch.ones_like(b0, dtype=torch.bool)
            for f in fs[1:]:
                same &= _bits(self.before[f][name]) == b0
            for f in fs[1:]:
                if not torch.equal(_bits(self.after[f][name])[same], a0[same]):
                    return False
        return True

    def worst(self, fill="cont"):
        """name -> worst err / bound over the bounded elements."""
        ex, out = self.ex[fill], {}
        for name, bn in ex.bnd.items():
            pos = bn > 0
            err = (self.after[fill][name].double() - ex.ref64[name]).abs()
            out[name] = float((err[pos] / bn[pos]).max()) if pos.any() else 0.0
        return out

    def assert_clean(self):
        what = self.case.name
        for f in self.after:
            for name, b in self.bad(f).items():
                out = self.bad_outside(name, f)
                assert not out.any(), (what, f, name, "differs outside the operand at",
                                       out.nonzero()[:8].tolist())
                assert not b.any(), (what, f, name, int(b.sum()), "elements differ, first at",
                                     self.bad_view(name, f).nonzero()[:8].tolist())
        if len(self.after) > 1:
            assert self.fills_equal(), (what, "the fill of outside memory changes a buffer")


def run(case, be, dev="cpu", fills=FILLS):
    """Launch ``case`` on backend ``be`` under every fill of the outside memory."""
    rep = Report(case)
    for f in fills:
        g = case.ground(f, dev)
        rep.g[f], rep.before[f] = g, g.snapshot()
        case.launch(be, g.v)
        rep.after[f] = g.snapshot()
        ex = Expect(rep.before[f])
        case.expect(g, ex)
        rep.ex[f] = ex
    return rep


def check(case, be, dev="cpu"):
    rep = run(case, be, dev)
    for name, w in rep.worst().items():
        print(f"row-exact {be.name} {case.name} {name}: worst err/bound {w:.4f}")
    rep.assert_clean()
    return rep


# ------------------------------------------------------- fp64 references
def rms_ref(s, w):
    d = s.shape[-1]
    ref = s / torch.sqrt((s * s).mean(-1, keepdim=True) + EPS) * w
    return ref, 2.0 ** -8 * ref.abs() + (d + 16) * U * ref.abs()


def ln_ref(s, w, b):
    d = s.shape[-1]
    mu = s.mean(-1, keepdim=True)
    sigma = torch.sqrt(((s - mu) ** 2).mean(-1, keepdim=True) + EPS)
    assert bool((sigma >= mu.abs() / 8).all())
    ref = (s - mu) / sigma * w + b
    dmu = d * U * s.abs().mean(-1, keepdim=True)
    return ref, (2.0 ** -8 * ref.abs() + w.abs() * dmu / sigma + (d + 16) * U * (ref - b).abs()
                 + 4 * U * ref.abs())


def gelu_ref(v, pos=None):
    ref = 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))
    p = 0.0
    if pos is not None:
        ref, p = ref + pos, U * pos.abs()
    return ref, 2.0 ** -8 * ref.abs() + 8 * U * ref.abs() + v.abs() * 2.0 ** -21 + p


def silu_ref(g, u):
    ref = g * torch.sigmoid(g) * u
    return ref, 2.0 ** -8 * ref.abs() + (g.abs() + 16) * U * ref.abs()


def slab_sum(part, S=None):
    """The slabs summed in the kernels' order, fp32."""
    tot = part[0].clone()
    for s in range(1, part.shape[0] if S is None else S):
        tot = tot + part[s]
    return tot


# ---------------------------------------------------------------------- cases
class NormCase:
    """rmsnorm / layernorm: plain, with ``residual``, with ``row_idx``."""

    def __init__(self, kind, d, mode):
        g = _gen(d + len(mode))
        self.kind, self.d, self.mode, self.name = kind, d, mode, f"{kind}norm-d{d}-{mode}"
        nx = 6 if mode == "row_idx" else 5
        x = torch.randn(nx, d, generator=g)
        x[1::2] += 3
        self.x = x.to(BF)
        self.res = torch.randn(5, d, generator=g).to(BF) if mode == "residual" else None
        self.w = (1 + 0.1 * torch.randn(d, generator=g)).to(BF)
        self.b = torch.randn(d, generator=g).to(BF) if kind == "ln" else None
        self.idx = torch.tensor(IDX, dtype=I64) if mode == "row_idx" else None
        self.unread = sorted(set(range(nx)) - set(IDX)) if mode == "row_idx" else []

    def ground(self, fill, dev):
        g = Ground(fill, dev)
        g.put("x", g.hide(self.x, self.unread))
        g.put("residual", self.res)
        g.put("w", self.w)
        g.put("b", self.b)
        g.put("row_idx", self.idx)
        g.out("y", (5, self.d))
        return g

    def launch(self, be, v):
        if self.kind == "rms":
            be.rmsnorm(v["x"], v["w"], EPS, v["residual"], v["row_idx"], v["y"])
        else:
            be.layernorm(v["x"], v["w"], v["b"], EPS, v["residual"], v["row_idx"], v["y"])

    @functools.cached_property
    def ref(self):
        s = self.x[list(IDX)] if self.idx is not None else self.x
        if self.res is not None:
            s = (s.float() + self.res.float()).to(BF)
        r = rms_ref(s.double(), self.w.double()) if self.kind == "rms" else \
            ln_ref(s.double(), self.w.double(), self.b.double())
        return (s,) + r

    def expect(self, g, ex):
        s, ref, bound = self.ref
        if self.res is not None:
            g.view("residual", ex.exp)[...] = s
        g.bounded("y", ref, bound, ex)


class EmbedCase:
    """embed_pos / embed_stats (with and without positions and row sums);
    token -1 reads row 0."""
    TOK, POS, V, P = (3, -1, 0, 5, 3), (2, 0, 4, 1, 2), 6, 5

    def __init__(self, op, d, family, with_pos=True, sums=True):
        g = _gen(d + len(family))
        self.op, self.d, self.with_pos, self.sums = op, d, with_pos, sums
        self.name = f"embed_{op}-d{d}-{family}-pos{int(with_pos)}-sums{int(sums)}"
        if family == "int":
            self.te, self.pe = _ints(g, -8, 8, self.V, d).to(BF), _ints(g, -4, 4, self.P, d).to(BF)
        else:
            self.te = torch.randn(self.V, d, generator=g).to(BF)
            self.pe = torch.randn(self.P, d, generator=g).to(BF)
        self.tok, self.pos = torch.tensor(self.TOK, dtype=I32), torch.tensor(self.POS, dtype=I32)

    def ground(self, fill, dev):
        g = Ground(fill, dev)
        g.put("tok", self.tok)
        g.put("pos", self.pos)
        g.put("te", g.hide(self.te, set(range(self.V)) - {max(t, 0) for t in self.TOK}))
        g.put("pe", g.hide(self.pe, set(range(self.P)) - set(self.POS)) if self.with_pos else None)
        g.out("out", (5, self.d))
        if self.op == "stats":
            g.out("rowsq", (5,), F32)
            g.out("rowsum", (5,), F32)
        return g

    def launch(self, be, v):
        if self.op == "pos":
            be.embed_pos(v["tok"], v["pos"], v["te"], v["pe"], v["out"])
        else:
            be.embed_stats(v["tok"], v["pos"] if self.with_pos else None, v["te"], v["pe"], v["out"],
                           v["rowsq"], v["rowsum"] if self.sums else None)

    def expect(self, g, ex):
        x = self.te[self.tok.long().clamp(min=0)]
        if self.with_pos:
            x = (x.float() + self.pe[self.pos.long()].float()).to(BF)
        g.view("out", ex.exp)[...] = x
        if self.op == "stats":
            xd = x.double()
            g.bounded("rowsq", (xd * xd).sum(1), self.d * U * (xd * xd).sum(1), ex)
            if self.sums:
                g.bounded("rowsum", xd.sum(1), self.d * U * xd.abs().sum(1), ex)


MPAD = 16


class SlabNormCase:
    """slab_rmsnorm / slab_layernorm; ``row_idx`` comes with write_residual=False."""

    def __init__(self, kind, S, d, mode):
        g = _gen(S + d + len(mode))
        self.kind, self.S, self.d, self.mode = kind, S, d, mode
        self.name = f"slab_{kind}norm-S{S}-d{d}-{mode}"
        self.part = torch.randn(S, MPAD, d, generator=g)
        res = torch.randn(MPAD, d, generator=g)
        res[1::2] += 3
        self.res = res.to(BF)
        self.w = (1 + 0.1 * torch.randn(d, generator=g)).to(BF)
        self.b = torch.randn(d, generator=g).to(BF) if kind == "ln" else None
        self.bias = torch.randn(d, generator=g).to(BF) if kind == "ln" and S == 3 else None
        self.idx = torch.tensor(IDX, dtype=I64) if mode == "row_idx" else None
        self.write = mode != "row_idx"
        self.rows = 5 if mode == "row_idx" else MPAD
        self.unread = sorted(set(range(MPAD)) - set(IDX)) if mode == "row_idx" else []

    def ground(self, fill, dev):
        g = Ground(fill, dev)
        g.put("part", g.hide(self.part.transpose(0, 1), self.unread).transpose(0, 1).contiguous())
        g.put("residual", g.hide(self.res, self.unread))
        g.put("w", self.w)
        g.put("b", self.b)
        g.put("bias", self.bias)
        g.put("row_idx", self.idx)
        g.out("y", (self.rows, self.d))
        return g

    def launch(self, be, v):
        if self.kind == "rms":
            be.slab_rmsnorm(v["part"], v["residual"], v["w"], EPS, v["row_idx"], self.write, v["y"])
        else:
            be.slab_layernorm(v["part"], v["residual"], v["w"], v["b"], EPS, v["bias"], v["row_idx"],
                              self.write, v["y"])

    @functools.cached_property
    def ref(self):
        tot = slab_sum(self.part)
        if self.kind == "ln":
            if self.bias is not None:
                tot = tot + self.bias.float()
            tot = tot.to(BF).float()
        idx = list(IDX) if self.idx is not None else list(range(MPAD))
        s = (tot[idx] + self.res[idx].float()).to(BF)
        r = rms_ref(s.double(), self.w.double()) if self.kind == "rms" else \
            ln_ref(s.double(), self.w.double(), self.b.double())
        return (s,) + r

    def expect(self, g, ex):
        s, ref, bound = self.ref
        if self.write:
            g.view("residual", ex.exp)[...] = s
        g.bounded("y", ref, bound, ex)


class SlabActCase:
    """slab_reduce / slab_bias_act("none") on integers, slab_bias_act("gelu") /
    slab_silu_mul on random slabs."""

    def __init__(self, op, S, N):
        g = _gen(S + N + len(op))
        self.op, self.S, self.N, self.name = op, S, N, f"slab_{op}-S{S}-N{N}"
        W = 2 * N if op == "silu" else N
        if op in ("reduce", "none"):
            part = _ints(g, -3, 3, S, MPAD, W)
            part[0] = _ints(g, -8, 8, MPAD, W) - part[1:].sum(0)
            self.bias = _ints(g, -4, 4, N).to(BF) if op == "none" and S == 3 else None
        else:
            part = torch.randn(S, MPAD, W, generator=g) * (0.8 if op == "gelu" else 1.0)
            self.bias = torch.randn(N, generator=g).clamp(-2, 2).to(BF) if op == "gelu" and S == 3 else None
        self.part = part

    def ground(self, fill, dev):
        g = Ground(fill, dev)
        g.put("part", self.part)
        g.put("bias", self.bias)
        g.out("out", (MPAD, self.N), F32 if self.op == "reduce" else BF)
        return g

    def launch(self, be, v):
        if self.op == "reduce":
            be.slab_reduce(v["part"], v["out"])
        elif self.op == "silu":
            be.slab_silu_mul(v["part"], v["out"])
        else:
            be.slab_bias_act(v["part"], v["bias"], self.op, v["out"])

    @functools.cached_property
    def ref(self):
        tot = slab_sum(self.part)
        if self.bias is not None:
            tot = tot + self.bias.float()
        if self.op == "reduce":
            return tot, None
        if self.op == "none":
            assert torch.equal(R.slab_bias_act(self.part, self.bias), tot.to(BF))
            return tot.to(BF), None
        t = tot.to(BF).double()
        if self.op == "gelu":
            assert float(t.abs().max()) <= 8
            return gelu_ref(t)
        gt, up = t[:, :self.N], t[:, self.N:]
        assert float(gt.abs().max()) <= 16
        return silu_ref(gt, up)

    def expect(self, g, ex):
        ref, bound = self.ref
        if bound is None:
            g.view("out", ex.exp)[...] = ref
        else:
            g.bounded("out", ref, bound, ex)


PERIOD = 7


class StreamCase:
    """silu_mul ([rows, 2F] -> [rows, F]) and gelu_bias_ (in place); 65539 rows
    take two launches."""

    def __init__(self, op, F, rows, bias=False, pos=False):
        g = _gen(F + rows)
        self.op, self.F, self.rows = op, F, rows
        self.name = f"{op}-F{F}-rows{rows}-bias{int(bias)}-pos{int(pos)}"
        self.bias = self.pos = None
        if op == "silu":
            gate = (torch.randn(rows, F, generator=g) * 3).clamp(-16, 16)
            self.x = torch.cat([gate, torch.randn(rows, F, generator=g)], 1).to(BF)
        else:
            self.x = (torch.randn(rows, F, generator=g) * 2).clamp(-6, 6).to(BF)
            if bias:
                self.bias = torch.randn(F, generator=g).clamp(-2, 2).to(BF)
            if pos:
                self.pos = torch.randn(PERIOD, F, generator=g).to(BF)

    def ground(self, fill, dev):
        g = Ground(fill, dev)
        g.put("x", self.x)
        g.put("bias", self.bias)
        g.put("pos", self.pos)
        if self.op == "silu":
            g.out("out", (self.rows, self.F))
        return g

    def launch(self, be, v):
        if self.op == "silu":
            be.silu_mul(v["x"], v["out"])
        else:
            be.gelu_bias_(v["x"], v["bias"], v["pos"])

    @functools.cached_property
    def ref(self):
        x = self.x.double()
        if self.op == "silu":
            return silu_ref(x[:, :self.F], x[:, self.F:])
        v = x if self.bias is None else x + self.bias.double()
        assert float(v.abs().max()) <= 8
        pos = None if self.pos is None else self.pos.double()[torch.arange(self.rows) % PERIOD]
        return gelu_ref(v, pos)

    def expect(self, g, ex):
        g.bounded("out" if self.op == "silu" else "x", *self.ref, ex)


BLK = 4
ROPE_SHAPES = {(5, 1, 64): "batched", (8, 2, 128): "batched", (56, 8, 128): "batched", (57, 8, 128): "loop",
               (20, 20, 64): "loop", (4, 16, 128): "loop"}


def rope_form(Hq, Hkv, D):
    """The launcher's condition (``loqa_rope_kv_append``)."""
    return "batched" if (Hq + Hkv) * (D // 8) <= 8 * 128 and Hkv * (D // 8) <= 128 else "loop"


def cos_sin_table(P, half):
    p, c = torch.arange(P)[:, None], torch.arange(half)[None, :]
    cs = torch.stack([(2 * p + c) % 5 - 2, (p + 3 * c + p // 5) % 5 - 2], -1).float()
    cs[0, :, 0], cs[0, :, 1] = 1.0, 0.0
    return cs


class RopeCase:
    """rope_kv_append (``S`` None: bf16 qkv, rotated in place) and
    slab_rope_append (fp32 slabs -> q_out), integer family."""
    P = 9

    def __init__(self, Hq, Hkv, D, use_cs=True, S=None, bias=False):
        self.H, self.Hkv, self.D, self.S, self.use_cs = Hq, Hkv, D, S, use_cs
        self.T = T = 7 if S is None else MPAD
        self.name = f"rope-{Hq}-{Hkv}-{D}-cs{int(use_cs)}" + ("" if S is None else f"-S{S}-bias{int(bias)}")
        g = _gen(Hq + Hkv + D + T)
        self.W = W = (Hq + 2 * Hkv) * D
        self.nb = nb = (T + 1 + BLK - 1) // BLK + 1
        pos = torch.randint(1, self.P, (T,), generator=g)
        pos[1], pos[3] = 0, pos[0]
        self.pos = pos.to(I32)
        slots = torch.randperm(nb * BLK - 1, generator=g)[:T] + 1       # slot 0 stays free
        slots[1] = slots[2] = -1                # token 1 is at position 0, token 2 is not
        if T > 8:
            slots[T - 2] = slots[9] = -1
        self.slots = slots.to(I32)
        self.cs = cos_sin_table(self.P, D // 2) if use_cs else None
        self.bias = None
        if S is None:
            self.qkv = _ints(g, -8, 8, T, W).to(BF)
        else:
            part = _ints(g, -3, 3, S, T, W)
            part[0] = _ints(g, -8, 8, T, W) - part[1:].sum(0)
            self.part = part
            if bias:
                self.bias = _ints(g, -4, 4, W).to(BF)
        written = torch.zeros(nb * BLK, dtype=torch.bool)
        written[self.slots[self.slots >= 0].long()] = True
        self.written = written.view(nb, 1, BLK, 1)

    def ground(self, fill, dev):
        g = Ground(fill, dev)
        if self.S is None:
            g.put("qkv", self.qkv, col=8)
        else:
            g.put("part", self.part)
            g.put("bias", self.bias)
            g.out("q_out", (self.T, self.H * self.D))
        g.put("pos", self.pos)
        g.put("slots", self.slots)
        if self.cs is not None:
            g.put("cs", g.hide(self.cs, set(range(self.P)) - set(self.pos.tolist())))
        else:
            g.put("cs", None)
        cache = torch.full((self.nb, self.Hkv, BLK, self.D), g.fillv(BF))
        cache = torch.where(self.written, torch.full((), SENT), cache).to(BF)
        g.put("kc", cache)
        g.put("vc", cache)
        return g

    def launch(self, be, v):
        if self.S is None:
            be.rope_kv_append(v["qkv"], v["pos"] if self.use_cs else None, v["cs"], v["kc"], v["vc"],
                              v["slots"], self.H, self.Hkv, self.D)
        else:
            be.slab_rope_append(v["part"], v["pos"], v["cs"], v["q_out"], v["kc"], v["vc"], v["slots"],
                                self.H, self.Hkv, self.D, v["bias"])

    def expect(self, g, ex):
        e = lambda n: g.view(n, ex.exp)
        dims = (self.H, self.Hkv, self.D)
        if self.S is None:
            R.rope_kv_append(e("qkv"), e("pos"), e("cs"), e("kc"), e("vc"), e("slots"), *dims)
        else:
            e("q_out")[...] = R.slab_rope_append(e("part"), e("pos"), e("cs"), e("kc"), e("vc"), e("slots"),
                                                 *dims, e("bias"))


LD = 8292
PCM_LENS = (1, 0, 8191, 8192, 8193, LD, LD + 5)
PCM_SCALE = torch.tensor(1.0 / 32767.0, dtype=F32)


class PcmCase:
    """pcm16_to_f32_sumsq / pcm16_to_f32_padded over every int16 value."""

    def __init__(self, form, flip):
        self.form, self.flip, self.name = form, flip, f"pcm16-{form}-flip{int(flip)}"
        pcm = (torch.randperm(65536, generator=_gen(1)) - 32768).to(I16)
        self.pcm = pcm.flip(0) if flip else pcm
        lens = list(PCM_LENS)
        if form == "sumsq":
            rest = 65536 - sum(lens)
            lens += [16384, rest - 16384]
        self.off = torch.tensor([0] + lens, dtype=I64).cumsum(0)
        assert int(self.off[2]) % 2 == 1 and int(self.off[-1]) <= 65536 and max(lens) <= 16384
        self.nseg = len(lens)

    def ground(self, fill, dev):
        g = Ground(fill, dev)
        g.put("pcm", self.pcm)
        g.put("off", self.off)
        if self.form == "sumsq":
            g.out("out", (65536,), F32)
        else:
            g.out("out", (self.nseg, LD), F32, float("nan"))
        g.out("sumsq", (self.nseg,), F32)
        return g

    def launch(self, be, v):
        be.pcm16(self.form, v["pcm"], v["off"], v["out"], v["sumsq"])

    @functools.cached_property
    def ref(self):
        f = self.pcm.float() * PCM_SCALE
        q = self.pcm.double() / 32767
        ulp = torch.exp2(torch.floor(torch.log2(q.abs().clamp_min(2.0 ** -126))) - 23)
        assert bool(((f.double() - q).abs() <= ulp).all())       # the documented meaning: x / 32767
        off = self.off.tolist()
        if self.form == "sumsq":
            out, kept = f, [off[i + 1] - off[i] for i in range(self.nseg)]
        else:
            out, kept = torch.zeros(self.nseg, LD), [min(off[i + 1] - off[i], LD) for i in range(self.nseg)]
            for i, n in enumerate(kept):
                out[i, :n] = f[off[i]:off[i] + n]
        ss = torch.stack([(f[off[i]:off[i] + n].double() ** 2).sum() for i, n in enumerate(kept)])
        return out, ss, torch.tensor(kept, dtype=F64) * U * ss

    def expect(self, g, ex):
        out, ss, bound = self.ref
        g.view("out", ex.exp)[...] = out
        g.bounded("sumsq", ss, bound, ex)


@functools.lru_cache(maxsize=None)
def case(cls, *args):
    return cls(*args)


# ------------------------------------------------------------------- backends
class Native:
    """The HIP kernels: through the public wrapper where it takes the output
    buffer, else through the launcher (and then the wrapper, where it has no
    side effect, must return the same bits)."""
    name = "hip"

    @staticmethod
    def _same(got, view):
        assert got.shape == view.shape and torch.equal(_bits(got), _bits(view)), "wrapper and launcher differ"

    def rmsnorm(self, x, w, eps, residual, row_idx, y):
        p, K = _lib.ptr, _lib.kernels()
        _lib.check(K.loqa_rmsnorm(p(x), p(residual), p(w), p(y), y.shape[0], x.shape[-1], eps, p(row_idx),
                                  _lib.stream_ptr(x)), "rmsnorm")
        if residual is None:
            self._same(ops.rmsnorm(x, w, eps, row_idx=row_idx), y)

    def layernorm(self, x, w, b, eps, residual, row_idx, y):
        p, K = _lib.ptr, _lib.kernels()
        _lib.check(K.loqa_layernorm(p(x), p(residual), p(w), p(b), p(y), y.shape[0], x.shape[-1], eps,
                                    p(row_idx), _lib.stream_ptr(x)), "layernorm")
        if residual is None:
            self._same(ops.layernorm(x, w, b, eps, row_idx=row_idx), y)

    def embed_pos(self, tok, pos, te, pe, out):
        assert ops.embed_pos(tok, pos, te, pe, out=out) is out

    def embed_stats(self, tok, pos, te, pe, out, rowsq, rowsum):
        p, K = _lib.ptr, _lib.kernels()
        _lib.check(K.loqa_embed_stats(p(tok), p(pos), p(te), p(pe), p(out), p(rowsq), p(rowsum), tok.numel(),
                                      te.shape[1], _lib.stream_ptr(te)), "embed_stats")
        sc = ops.FusedScratch(te.device, max_tiles=1, max_rows=8)
        self._same(ops.embed_stats(tok, te, sc, positions=pos, pos_embed=pe, sums=rowsum is not None), out)
        self._same(sc.rowsq[:tok.numel()], rowsq)
        if rowsum is not None:
            self._same(sc.rowsum[:tok.numel()], rowsum)

    def slab_rmsnorm(self, part, residual, w, eps, row_idx, write, y):
        p, K = _lib.ptr, _lib.kernels()
        S, Mpad, d = part.shape
        _lib.check(K.loqa_slab_rmsnorm(p(part), S, Mpad, p(row_idx), y.shape[0], p(residual), int(write),
                                       p(w), p(y), d, eps, _lib.stream_ptr(part)), "slab_rmsnorm")
        if not write:
            self._same(ops.slab_rmsnorm(part, residual, w, eps, row_idx=row_idx, write_residual=False), y)

    def slab_layernorm(self, part, residual, w, b, eps, bias, row_idx, write, y):
        assert ops.slab_layernorm(part, residual, w, b, eps, bias=bias, row_idx=row_idx, write_residual=write,
                                  out=y) is y

    def slab_rope_append(self, part, pos, cs, q_out, kc, vc, slots, H, Hkv, D, bias):
        p, K = _lib.ptr, _lib.kernels()
        S, Mpad, _ = part.shape
        _lib.check(K.loqa_slab_rope_append(p(part), S, Mpad, Mpad, p(pos), p(cs), p(q_out), p(kc), p(vc),
                                           p(slots), H, Hkv, D, kc.shape[2], p(bias), _lib.stream_ptr(part)),
                   "slab_rope_append")
        # the wrapper appends the same values once more
        self._same(ops.slab_rope_append(part, pos, cs, kc, vc, slots, H, Hkv, D, bias=bias), q_out)

    def slab_bias_act(self, part, bias, act, out):
        p, K = _lib.ptr, _lib.kernels()
        S, Mpad, N = part.shape
        _lib.check(K.loqa_slab_bias_act(p(part), S, Mpad, Mpad, N, p(bias), {"none": 0, "gelu": 1}[act],
                                        p(out), _lib.stream_ptr(part)), "slab_bias_act")
        self._same(ops.slab_bias_act(part, bias, act), out)

    def slab_silu_mul(self, part, out):
        S, Mpad, F2 = part.shape
        _lib.check(_lib.kernels().loqa_slab_silu_mul(_lib.ptr(part), S, Mpad, Mpad, F2 // 2, _lib.ptr(out),
                                                     _lib.stream_ptr(part)), "slab_silu_mul")
        self._same(ops.slab_silu_mul(part), out)

    def slab_reduce(self, part, out):
        S, Mpad, N = part.shape
        _lib.check(_lib.kernels().loqa_slab_reduce(_lib.ptr(part), S, Mpad, Mpad, N, _lib.ptr(out),
                                                   _lib.stream_ptr(part)), "slab_reduce")
        self._same(ops.slab_reduce(part), out)

    def silu_mul(self, x, out):
        _lib.check(_lib.kernels().loqa_silu_mul(_lib.ptr(x), _lib.ptr(out), x.shape[0], out.shape[1],
                                                _lib.stream_ptr(x)), "silu_mul")
        self._same(ops.silu_mul(x), out)

    def gelu_bias_(self, x, bias, pos):
        assert ops.gelu_bias_(x, bias, pos) is x

    def rope_kv_append(self, qkv, pos, cs, kc, vc, slots, H, Hkv, D):
        ops.rope_kv_append(qkv, pos, cs, kc, vc, slots, H, Hkv, D)

    def pcm16(self, form, pcm, off, out, sumsq):
        p, K = _lib.ptr, _lib.kernels()
        S = off.numel() - 1
        if form == "sumsq":
            seg = off.cpu()
            longest = int((seg[1:] - seg[:-1]).max())
            _lib.check(K.loqa_pcm16_f32_sumsq(p(pcm), p(out), p(off), p(sumsq), S, longest,
                                              _lib.stream_ptr(pcm)), "pcm16_f32_sumsq")
            got = ops.pcm16_to_f32_sumsq(pcm, off)
            self._same(got[0], out)
            self._same(got[1], sumsq)       # no segment spans more than two chunks: order independent
        else:
            _lib.check(K.loqa_pcm16_f32_pad(p(pcm), p(out), p(off), p(sumsq), S, out.shape[1],
                                            _lib.stream_ptr(pcm)), "pcm16_f32_pad")
            got = ops.pcm16_to_f32_padded(pcm, off, out.shape[1])
            self._same(got[0], out)
            self._same(got[1], sumsq)


class CpuOps:
    """``ops.*`` on CPU tensors, the result copied where the kernel stores it."""
    name = "ops-cpu"

    def rmsnorm(self, x, w, eps, residual, row_idx, y):
        y.copy_(ops.rmsnorm(x, w, eps, residual=residual, row_idx=row_idx))

    def layernorm(self, x, w, b, eps, residual, row_idx, y):
        y.copy_(ops.layernorm(x, w, b, eps, residual=residual, row_idx=row_idx))

    def embed_pos(self, tok, pos, te, pe, out):
        out.copy_(ops.embed_pos(tok, pos, te, pe))

    def embed_stats(self, tok, pos, te, pe, out, rowsq, rowsum):
        sc = ops.FusedScratch("cpu", max_tiles=1, max_rows=8)
        out.copy_(ops.embed_stats(tok, te, sc, positions=pos, pos_embed=pe, sums=rowsum is not None))
        rowsq.copy_(sc.rowsq[:tok.numel()])
        if rowsum is not None:
            rowsum.copy_(sc.rowsum[:tok.numel()])

    def slab_rmsnorm(self, part, residual, w, eps, row_idx, write, y):
        y.copy_(ops.slab_rmsnorm(part, residual, w, eps, row_idx=row_idx, write_residual=write))

    def slab_layernorm(self, part, residual, w, b, eps, bias, row_idx, write, y):
        y.copy_(ops.slab_layernorm(part, residual, w, b, eps, bias=bias, row_idx=row_idx,
                                   write_residual=write))

    def slab_rope_append(self, part, pos, cs, q_out, kc, vc, slots, H, Hkv, D, bias):
        q_out.copy_(ops.slab_rope_append(part, pos, cs, kc, vc, slots, H, Hkv, D, bias=bias))

    def slab_bias_act(self, part, bias, act, out):
        out.copy_(ops.slab_bias_act(part, bias, act))

    def slab_silu_mul(self, part, out):
        out.copy_(ops.slab_silu_mul(part))

    def slab_reduce(self, part, out):
        out.copy_(ops.slab_reduce(part))

    def silu_mul(self, x, out):
        out.copy_(ops.silu_mul(x))

    def gelu_bias_(self, x, bias, pos):
        ops.gelu_bias_(x, bias, pos)

    def rope_kv_append(self, qkv, pos, cs, kc, vc, slots, H, Hkv, D):
        ops.rope_kv_append(qkv, pos, cs, kc, vc, slots, H, Hkv, D)

    def pcm16(self, form, pcm, off, out, sumsq):
        o, s = ops.pcm16_to_f32_sumsq(pcm, off) if form == "sumsq" else ops.pcm16_to_f32_padded(pcm, off,
                                                                                                 out.shape[1])
        out.copy_(o)
        sumsq.copy_(s)


def _seq_sum(t, skip_last=0):
    """[rows, d] fp32 -> [rows, 1]: one fp32 add per column, LAST column first."""
    acc = torch.zeros(t.shape[0], dtype=F32)
    for j in reversed(range(t.shape[1] - skip_last)):
        acc = acc + t[:, j]
    return acc[:, None]


LAUNCH_ROWS = 65535


class Sim:
    """The kernels in plain fp32 torch - statistics summed sequentially in
    reverse order, slabs in the kernels' order, one rounding where the kernels
    round - and, through ``mut``, their possible faults."""
    name = "sim-fp32"

    def __init__(self, **mut):
        self.mut = mut

    def _bump(self, name, t):
        if self.mut.get("bump", (None,))[0] == name:
            _, at, n = self.mut["bump"]
            t.view(I16)[at] += n

    def _norm(self, kind, s, w, b, eps, y):
        d = s.shape[-1]
        skip = 8 if self.mut.get("stat_short") else 0
        wf = w.float().roll(8) if self.mut.get("w_shift") else w.float()
        if kind == "rms":
            o = s * torch.rsqrt(_seq_sum(s * s, skip) / d + eps) * wf
        else:
            mean = _seq_sum(s, skip) / d
            t = s - mean
            o = t * torch.rsqrt(_seq_sum(t * t, skip) / d + eps) * wf + b.float()
        y.copy_(o.to(BF))
        self._bump("y", y)

    def _gather(self, x, residual, row_idx, rows):
        idx = torch.arange(rows) if row_idx is None or self.mut.get("idx_is_row") else row_idx
        s = x[idx].float()
        if residual is not None:
            sb = (s + residual.float()).to(BF)
            residual.copy_(sb)
            s = sb.float()
        return s

    def rmsnorm(self, x, w, eps, residual, row_idx, y):
        self._norm("rms", self._gather(x, residual, row_idx, y.shape[0]), w, None, eps, y)

    def layernorm(self, x, w, b, eps, residual, row_idx, y):
        self._norm("ln", self._gather(x, residual, row_idx, y.shape[0]), w, b, eps, y)

    def _embed(self, tok, pos, te, pe):
        x = te[tok.long().clamp(min=0)]
        return x if pe is None else (x.float() + pe[pos.long()].float()).to(BF)

    def embed_pos(self, tok, pos, te, pe, out):
        out.copy_(self._embed(tok, pos, te, pe))

    def embed_stats(self, tok, pos, te, pe, out, rowsq, rowsum):
        x = self._embed(tok, pos, te, pe)
        out.copy_(x)
        rowsq.copy_(_seq_sum(x.float() ** 2)[:, 0])
        if rowsum is not None:
            rowsum.copy_(_seq_sum(x.float())[:, 0])

    def _tot(self, part, bias=None):
        tot = slab_sum(part, part.shape[0] - 1 if self.mut.get("drop_slab") else None)
        return tot if bias is None else tot + bias.float()

    def _slab_rows(self, tot, residual, row_idx, write, rows):
        idx = torch.arange(rows) if row_idx is None or self.mut.get("idx_is_row") else row_idx
        sb = (tot[idx] + residual[idx].float()).to(BF)
        if write:
            residual[idx] = sb
        return sb.float()

    def slab_rmsnorm(self, part, residual, w, eps, row_idx, write, y):
        s = self._slab_rows(self._tot(part), residual, row_idx, write, y.shape[0])
        self._norm("rms", s, w, None, eps, y)

    def slab_layernorm(self, part, residual, w, b, eps, bias, row_idx, write, y):
        tot = self._tot(part, bias).to(BF).float()
        self._norm("ln", self._slab_rows(tot, residual, row_idx, write, y.shape[0]), w, b, eps, y)

    @staticmethod
    def _gelu(v):
        return 0.5 * v * (1 + torch.erf(v * 0.70710678118654752))

    def slab_bias_act(self, part, bias, act, out):
        tot = self._tot(part, bias)
        out.copy_((self._gelu(tot.to(BF).float()) if act == "gelu" else tot).to(BF))

    def slab_silu_mul(self, part, out):
        t = self._tot(part).to(BF).float()
        F = t.shape[1] // 2
        out.copy_((t[:, :F] / (1 + torch.exp(-t[:, :F])) * t[:, F:]).to(BF))

    def slab_reduce(self, part, out):
        out.copy_(self._tot(part))

    def _second_launch(self, rows):
        """Row ranges of the launches: the second starts at row 0 in mutant (k)."""
        out = []
        for r0 in range(0, rows, LAUNCH_ROWS):
            n = min(LAUNCH_ROWS, rows - r0)
            out.append((0 if self.mut.get("launch_row0") else r0, n))
        return out

    def silu_mul(self, x, out):
        F = out.shape[1]
        for r0, n in self._second_launch(x.shape[0]):
            g, u = x[r0:r0 + n, :F].float(), x[r0:r0 + n, F:].float()
            out[r0:r0 + n] = (g / (1 + torch.exp(-g)) * u).to(BF)

    def gelu_bias_(self, x, bias, pos):
        for r0, n in self._second_launch(x.shape[0]):
            v = x[r0:r0 + n].float()
            if bias is not None:
                v = v + bias.float()
            v = self._gelu(v)
            if pos is not None:
                row = torch.arange(r0, r0 + n)
                if self.mut.get("pos_no_period"):       # rows past the table: the row after it
                    P, F = pos.shape
                    ext = pos.as_strided((P + 1, F), pos.stride(), pos.storage_offset())
                    v = v + ext[row.clamp(max=P)].float()
                else:
                    v = v + pos[row % pos.shape[0]].float()
            x[r0:r0 + n] = v.to(BF)
        self._bump("x", x)

    def _rope(self, qkv, pos, cs, kc, vc, slots, H, Hkv, D):
        """qkv [T, >= W] (values exact in bf16) -> rotated q [T, H * D] bf16."""
        T, half, m = qkv.shape[0], D // 2, self.mut
        q = qkv[:, :H * D].reshape(T, H, D).float()
        k = qkv[:, H * D:(H + Hkv) * D].reshape(T, Hkv, D).float()
        v = qkv[:, (H + Hkv) * D:(H + 2 * Hkv) * D].reshape(T, Hkv, D).to(BF)
        if cs is not None:
            p = pos.long().roll(-1) if m.get("pos_next") else pos.long()
            ex, ey = cs[p][:, None, :, 0], cs[p][:, None, :, 1]

            def rot(x):
                a, b = x[..., :half], x[..., half:]
                pa, pb = (a.roll(-4, -1), b.roll(-4, -1)) if m.get("partner_off") else (a, b)
                return torch.cat([a * ex - pb * ey, b * ex + pa * ey], -1)
            qr, k = rot(q), rot(k)
            q = torch.where((slots < 0)[:, None, None], q, qr) if m.get("padding_q_unrotated") else qr
        if m.get("k_head_next"):
            k = k.roll(1, 1)
        blk = kc.shape[2]
        for t in range(T):
            s = int(slots[t])
            if s < 0:
                if not m.get("append_padding"):
                    continue
                s = 0
            b, o = s // blk, s % blk
            kc[b, :, o] = k[t].to(BF)
            nv = Hkv - 1 if m.get("v_last_head") else Hkv
            vc[b, :nv, o] = v[t, :nv]
        return q.reshape(T, H * D).to(BF)

    def rope_kv_append(self, qkv, pos, cs, kc, vc, slots, H, Hkv, D):
        qkv[:, :H * D] = self._rope(qkv, pos, cs, kc, vc, slots, H, Hkv, D)

    def slab_rope_append(self, part, pos, cs, q_out, kc, vc, slots, H, Hkv, D, bias):
        q_out.copy_(self._rope(self._tot(part, bias).to(BF), pos, cs, kc, vc, slots, H, Hkv, D))

    def pcm16(self, form, pcm, off, out, sumsq):
        f, o = pcm.float() * PCM_SCALE, off.tolist()
        for i in range(len(o) - 1):
            n = o[i + 1] - o[i]
            if form == "sumsq":
                out[o[i]:o[i + 1]] = f[o[i]:o[i + 1]]
            else:
                n = min(n, out.shape[1])
                out[i, :n], out[i, n:] = f[o[i]:o[i] + n], 0.0
            seg = f[o[i]:o[i] + n].flip(0)
            sumsq[i] = (seg * seg).sum()


# --------------------------------------------------------------------- tables
NORM_D = (8, 2040, 2048, 2056, 8192)
NORM_CASES = [("rms", d) for d in NORM_D] + [("ln", d) for d in NORM_D + (1280,)]
NORM_MODES = ("plain", "residual", "row_idx")
EMBED_CASES = [("pos", 8, "int", True, True), ("pos", 2056, "int", True, True),
               ("stats", 8, "int", True, True), ("stats", 2056, "int", False, False),
               ("stats", 2056, "rand", True, True), ("stats", 8192, "rand", True, False),
               ("stats", 8, "rand", False, True)]
SLAB_NORM_CASES = [(k, S, d) for k in ("rms", "ln") for S in (1, 3) for d in (8, 2056)]
SLAB_ACT_CASES = [(op, S, N) for op in ("reduce", "none", "gelu", "silu") for S in (1, 3) for N in (8, 2056)]
STREAM_CASES = ([("silu", 8, 65539, False, False), ("silu", 2056, 3, False, False)]
                + [("gelu", F, rows, b, p) for F, rows in ((8, 65539), (2056, 3))
                   for b, p in ((False, False), (True, True), (True, False), (False, True))])
ROPE_CASES = [s + (s != (20, 20, 64),) for s in ROPE_SHAPES]
SLAB_ROPE_CASES = [(H, Hkv, D, cs, S, bias) for H, Hkv, D in ((5, 1, 64), (8, 2, 128)) for S in (1, 3)
                   for bias in (False, True) for cs in (True, False)]
PCM_CASES = [(form, flip) for form in ("sumsq", "padded") for flip in (False, True)]


def check_norm(kind, d, be, dev):
    for mode in NORM_MODES:
        check(case(NormCase, kind, d, mode), be, dev)


def check_slab_norm(kind, S, d, be, dev):
    for mode in ("all", "row_idx"):
        check(case(SlabNormCase, kind, S, d, mode), be, dev)


# ------------------------------------------------------------------ GPU tests
DEV = "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,d", NORM_CASES)
def test_norm(kind, d):
    check_norm(kind, d, Native(), DEV)


@pytest.mark.gpu
def test_norm_rejections():
    """d = 12, d = 8200 and row_idx together with residual: an error, and
    neither ``y`` nor ``residual`` is written."""
    p, K = _lib.ptr, _lib.kernels()
    for d, with_idx in ((12, False), (8200, False), (2048, True)):
        g = Ground("cont", DEV)
        x = g.put("x", torch.ones(6, d, dtype=BF))
        res = g.put("residual", torch.ones(5, d, dtype=BF))
        w = g.put("w", torch.ones(d, dtype=BF))
        idx = g.put("row_idx", torch.tensor(IDX, dtype=I64)) if with_idx else None
        y = g.out("y", (5, d))
        before = g.snapshot()
        sp = _lib.stream_ptr(x)
        assert K.loqa_rmsnorm(p(x), p(res), p(w), p(y), 5, d, EPS, p(idx), sp) != 0
        assert K.loqa_layernorm(p(x), p(res), p(w), p(w), p(y), 5, d, EPS, p(idx), sp) != 0
        if not with_idx:
            with pytest.raises(RuntimeError):
                ops.rmsnorm(x[:5], w, EPS)
            with pytest.raises(RuntimeError):
                ops.layernorm(x[:5], w, w, EPS, residual=res)
        else:
            with pytest.raises(AssertionError):
                ops.rmsnorm(x, w, EPS, residual=res, row_idx=idx)
        after = g.snapshot()
        for n in before:
            assert torch.equal(_bits(before[n]), _bits(after[n])), (d, n)


@pytest.mark.gpu
@pytest.mark.parametrize("op,d,family,with_pos,sums", EMBED_CASES)
def test_embed(op, d, family, with_pos, sums):
    check(case(EmbedCase, op, d, family, with_pos, sums), Native(), DEV)


@pytest.mark.gpu
def test_embed_negative_token_reads_row_zero():
    """The kernels clamp a negative id to row 0 (the engines pass -1 for
    padding rows); the CPU branch of the wrappers does the same."""
    g = _gen(3)
    te, pe = _ints(g, -8, 8, 4, 16).to(BF), _ints(g, -4, 4, 3, 16).to(BF)
    tok, pos = torch.tensor([-1, 3, -5], dtype=I32), torch.tensor([2, 1, 0], dtype=I32)
    want = (te[[0, 3, 0]].float() + pe[[2, 1, 0]].float()).to(BF)
    for dev in ("cpu", DEV):
        a = [t.to(dev) for t in (tok, pos, te, pe)]
        assert torch.equal(ops.embed_pos(*a).cpu(), want), dev
        sc = ops.FusedScratch(dev, max_tiles=1, max_rows=8)
        assert torch.equal(ops.embed_stats(a[0], a[2], sc, positions=a[1], pos_embed=a[3]).cpu(), want), dev
        assert torch.equal(sc.rowsq[:3].cpu(), want.float().square().sum(1)), dev


@pytest.mark.gpu
@pytest.mark.parametrize("kind,S,d", SLAB_NORM_CASES)
def test_slab_norm(kind, S, d):
    check_slab_norm(kind, S, d, Native(), DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("op,S,N", SLAB_ACT_CASES)
def test_slab_act(op, S, N):
    check(case(SlabActCase, op, S, N), Native(), DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("op,F,rows,bias,pos", STREAM_CASES)
def test_stream(op, F, rows, bias, pos):
    check(case(StreamCase, op, F, rows, bias, pos), Native(), DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,D,use_cs", ROPE_CASES)
def test_rope_kv_append(Hq, Hkv, D, use_cs):
    check(case(RopeCase, Hq, Hkv, D, use_cs), Native(), DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,D,use_cs,S,bias", SLAB_ROPE_CASES)
def test_slab_rope_append(Hq, Hkv, D, use_cs, S, bias):
    check(case(RopeCase, Hq, Hkv, D, use_cs, S, bias), Native(), DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("form,flip", PCM_CASES)
def test_pcm16(form, flip):
    check(case(PcmCase, form, flip), Native(), DEV)


# ------------------------------------- CPU: the candidates pass, the mutants fail
BACKENDS = [Sim(), CpuOps()]
_ids = lambda be: be.name if hasattr(be, "name") else None


def test_tables():
    for s, form in ROPE_SHAPES.items():
        assert rope_form(*s) == form, s
    assert (56 + 8) * 16 == 1024 and 8 * 16 == 128
    cs = cos_sin_table(9, 64)
    assert cs[0].tolist() == [[1.0, 0.0]] * 64 and float(cs.abs().max()) <= 2
    assert all(bool((cs[i] != cs[j]).any(-1).all()) for i in range(9) for j in range(i))
    assert bool((cs[1:] != cs[:-1]).any(-1).all()) and bool((cs[1:, 1:] != cs[1:, :-1]).any(-1).all())
    c = case(RopeCase, 8, 2, 128, True)
    for spec in ROPE_CASES + SLAB_ROPE_CASES:
        c = case(RopeCase, *spec)
        pad = c.pos[c.slots < 0].tolist()
        assert 0 in pad and any(pad), spec          # a -1 row whose rotation is not the identity
        assert 0 not in c.slots.tolist() and int(c.pos[0]) == int(c.pos[3]) and int(c.pos[1]) == 0
    both = torch.cat([case(PcmCase, "padded", f).ref[0].flatten() for f in (False, True)])
    assert torch.unique(both).numel() >= 65535          # every int16 value is converted (0: the padding too)
    assert torch.unique(case(PcmCase, "sumsq", False).pcm).numel() == 65536


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("kind,d", [("rms", 8), ("rms", 2056), ("ln", 8), ("ln", 2040), ("ln", 1280)])
def test_checker_passes_norm(kind, d, be):
    check_norm(kind, d, be, "cpu")


@pytest.mark.parametrize("kind", ["rms", "ln"])
def test_checker_passes_norm_widest(kind):
    check(case(NormCase, kind, 8192, "residual"), Sim())
    check(case(NormCase, kind, 8192, "row_idx"), CpuOps())


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("op,d,family,with_pos,sums", EMBED_CASES)
def test_checker_passes_embed(op, d, family, with_pos, sums, be):
    check(case(EmbedCase, op, d, family, with_pos, sums), be)


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("kind,S,d", SLAB_NORM_CASES)
def test_checker_passes_slab_norm(kind, S, d, be):
    check_slab_norm(kind, S, d, be, "cpu")


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("op,S,N", SLAB_ACT_CASES)
def test_checker_passes_slab_act(op, S, N, be):
    check(case(SlabActCase, op, S, N), be)


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("op,F,rows,bias,pos", STREAM_CASES[:4] + STREAM_CASES[6:8])
def test_checker_passes_stream(op, F, rows, bias, pos, be):
    check(case(StreamCase, op, F, rows, bias, pos), be)


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("Hq,Hkv,D,use_cs", ROPE_CASES)
def test_checker_passes_rope(Hq, Hkv, D, use_cs, be):
    check(case(RopeCase, Hq, Hkv, D, use_cs), be)


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("Hq,Hkv,D,use_cs,S,bias", SLAB_ROPE_CASES[::3])
def test_checker_passes_slab_rope(Hq, Hkv, D, use_cs, S, bias, be):
    check(case(RopeCase, Hq, Hkv, D, use_cs, S, bias), be)


@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
@pytest.mark.parametrize("form,flip", PCM_CASES)
def test_checker_passes_pcm(form, flip, be):
    check(case(PcmCase, form, flip), be)


def _rows(bad):
    """Rows of a view with a wrong element -> set."""
    return set(bad.reshape(bad.shape[0], -1).any(1).nonzero().flatten().tolist())


NORMS = [(NormCase, "rms", 2056, "plain"), (NormCase, "ln", 2056, "residual"),
         (SlabNormCase, "rms", 3, 2056, "all"), (SlabNormCase, "ln", 3, 2056, "all")]


@pytest.mark.parametrize("spec", NORMS, ids=lambda s: s[0].__name__ + "-" + s[1])
def test_mutant_statistic_short(spec):
    """(a) the statistic leaves out the row's last 8 columns: about 0.2% on
    every element (less where those columns are small), over the bound in a
    part of every row - and nowhere else."""
    c = case(*spec)
    rep = run(c, Sim(stat_short=True), fills=("cont",))
    assert rep.bad_names() == {"y"} and not rep.bad_outside("y").any()
    bad = rep.bad_view("y")
    assert _rows(bad) == set(range(bad.shape[0]))
    assert float(bad.float().mean()) > 0.02


@pytest.mark.parametrize("cls,kind", [(NormCase, "rms"), (NormCase, "ln")])
def test_mutant_row_idx(cls, kind):
    """(b) row_idx[i] replaced by i: wrong where row_idx[i] != i."""
    c = case(cls, kind, 2056, "row_idx")
    rep = run(c, Sim(idx_is_row=True))
    for f in FILLS:
        assert rep.bad_names(f) == {"y"}
        assert _rows(rep.bad_view("y", f)) == {i for i, r in enumerate(IDX) if i != r}
    assert not rep.fills_equal()            # row 3 is not named: it holds the fill


@pytest.mark.parametrize("spec", NORMS, ids=lambda s: s[0].__name__ + "-" + s[1])
def test_mutant_weight_shift(spec):
    """(c) the weight shifted by 8 columns."""
    rep = run(case(*spec), Sim(w_shift=True), fills=("cont",))
    bad = rep.bad_view("y")
    assert rep.bad_names() == {"y"} and _rows(bad) == set(range(bad.shape[0]))
    assert float(bad.float().mean()) > 0.5


ROPE_M = [(8, 2, 128, True), (57, 8, 128, True), (8, 2, 128, True, 3, True)]


@pytest.mark.parametrize("spec", ROPE_M, ids=str)
def test_mutant_rope_partner_and_position(spec):
    """(d) the rotate-half partner 4 columns off, (e) the position of token
    t + 1: q of every token and K of every appended one; V and qkv's k | v stay."""
    c = case(RopeCase, *spec)
    qn = "qkv" if c.S is None else "q_out"
    for mut in ("partner_off", "pos_next"):
        rep = run(c, Sim(**{mut: True}), fills=("cont",))
        assert rep.bad_names() == {qn, "kc"}, mut
        assert not rep.bad_outside(qn).any() and not rep.bad_outside("kc").any()
        bad = rep.bad_view(qn)
        assert not bad[:, c.H * c.D:].any()
        rows = _rows(bad)
        if mut == "partner_off":
            assert rows == {t for t in range(c.T) if c.pos[t] != 0}      # position 0 is (1, 0): no partner
        else:       # a token at the position of the next one stays right
            assert rows == {t for t in range(c.T) if c.pos[t] != c.pos[(t + 1) % c.T]}
        kbad = rep.bad_view("kc")
        assert bool((kbad.any(-1).any(1).flatten() <= c.written.flatten()).all())


@pytest.mark.parametrize("spec", ROPE_M + [(5, 1, 64, True), (56, 8, 128, True)], ids=str)
def test_mutant_padding_q_unrotated(spec):
    """(m) q of the rows with slots[t] = -1 left unrotated: exactly the -1 rows
    at a position other than 0 are wrong, in q only."""
    c = case(RopeCase, *spec)
    qn = "qkv" if c.S is None else "q_out"
    rep = run(c, Sim(padding_q_unrotated=True))
    want = {t for t in range(c.T) if c.slots[t] < 0 and c.pos[t] != 0}
    assert want
    for f in FILLS:
        assert rep.bad_names(f) == {qn} and _rows(rep.bad_view(qn, f)) == want
        assert not rep.bad_outside(qn, f).any()


@pytest.mark.parametrize("spec", ROPE_M, ids=str)
def test_mutant_cache_rows(spec):
    """(f) K of head h at head h + 1; (g) a -1 row appended at slot 0; (h) V of
    the last head not appended: each shows in that cache, in those rows, only."""
    c = case(RopeCase, *spec)
    rep = run(c, Sim(k_head_next=True), fills=("cont",))
    assert rep.bad_names() == {"kc"}
    assert torch.equal(rep.bad_view("kc").any(-1), c.written.expand(c.nb, c.Hkv, BLK, 1)[..., 0])
    rep = run(c, Sim(append_padding=True))
    for f in FILLS:
        assert rep.bad_names(f) == {"kc", "vc"}
        for n in ("kc", "vc"):
            bad = rep.bad_view(n, f).any(-1)
            assert bool(bad[0, :, 0].all()) and int(bad.sum()) == c.Hkv     # slot 0, every head, nothing else
    rep = run(c, Sim(v_last_head=True))
    for f in FILLS:
        assert rep.bad_names(f) == {"vc"}
        want = c.written.expand(c.nb, c.Hkv, BLK, 1)[..., 0].clone()
        want[:, :-1] = False
        assert torch.equal(rep.bad_view("vc", f).any(-1), want)


@pytest.mark.parametrize("spec", [(SlabNormCase, "rms", 3, 8, "all"),
                                  (SlabNormCase, "ln", 3, 2056, "row_idx"),
                                  (SlabActCase, "reduce", 3, 8), (SlabActCase, "none", 3, 2056),
                                  (SlabActCase, "gelu", 3, 8), (SlabActCase, "silu", 3, 2056),
                                  (RopeCase, 5, 1, 64, True, 3, False)], ids=str)
def test_mutant_slab_left_out(spec):
    """(i) slab S - 1 left out of the sum."""
    c = case(*spec)
    rep = run(c, Sim(drop_slab=True), fills=("cont",))
    names = rep.bad_names()
    assert names and names <= {"y", "residual", "out", "q_out", "kc", "vc"}
    for n in names:
        assert not rep.bad_outside(n).any()
    main = "y" if "y" in rep.g["cont"].v else "q_out" if "q_out" in rep.g["cont"].v else "out"
    bad = rep.bad_view(main)
    assert _rows(bad) == set(range(bad.shape[0]))


def test_mutant_pos_period_and_second_launch():
    """(j) pos[row] instead of pos[row % period]: right in the first period
    only; (k) the second 65535-row launch starting at row 0: the rows past
    65535 are not written (gelu: not transformed, and the first rows twice)."""
    c = case(StreamCase, "gelu", 8, 65539, True, True)
    rep = run(c, Sim(pos_no_period=True))
    for f in FILLS:
        rows = _rows(rep.bad_view("x", f))
        assert rep.bad_names(f) == {"x"} and min(rows) >= PERIOD and len(rows) > 0.99 * (65539 - PERIOD)
    rep = run(c, Sim(launch_row0=True), fills=("cont",))
    rows = _rows(rep.bad_view("x"))
    assert set(range(65535, 65539)) <= rows <= set(range(4)) | set(range(65535, 65539)) and len(rows) > 4
    c = case(StreamCase, "silu", 8, 65539, False, False)
    rep = run(c, Sim(launch_row0=True), fills=("cont",))
    assert rep.bad_names() == {"out"} and _rows(rep.bad_view("out")) == set(range(65535, 65539))
    c = case(StreamCase, "gelu", 2056, 3, True, True)          # one launch, one period: neither mutant shows
    assert not run(c, Sim(pos_no_period=True, launch_row0=True), fills=("cont",)).bad_names()


@pytest.mark.parametrize("spec", [(NormCase, "rms", 2056, "plain"), (NormCase, "ln", 1280, "row_idx"),
                                  (SlabNormCase, "ln", 3, 2056, "all"),
                                  (StreamCase, "gelu", 2056, 3, True, True)], ids=str)
def test_mutant_one_element(spec):
    """(l) one element off by 2 bf16 ulps, where the store term dominates
    (|ref| >= 2**-4): exactly that element fails."""
    c = case(*spec)
    name = "x" if isinstance(c, StreamCase) else "y"
    ref = c.ref[-2]
    at = tuple(int(i) for i in (ref.abs() == ref.abs().max()).nonzero()[0])
    assert float(ref[at].abs()) >= 2.0 ** -4
    for n in (2, -2):
        rep = run(c, Sim(bump=(name, at, n)), fills=("cont",))
        assert rep.bad_names() == {name}
        assert rep.bad_view(name).nonzero().tolist() == [list(at)]


# ---- what the old criterion saw: ||y - ref|| / ||ref|| < 1e-2, dense operands,
# zero caches (tests/test_kernels_gpu.py)
def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def old_ratios():
    torch.manual_seed(0)
    out = {}
    # test_rmsnorm[4096-37], with and without the mutant (a) / (l)
    x, w = torch.randn(37, 4096).to(BF), (1 + 0.1 * torch.randn(4096)).to(BF)
    yr = R.rmsnorm(x, w, EPS)
    y = torch.empty_like(yr)
    Sim().rmsnorm(x, w, EPS, None, None, y)
    out["clean"] = _rel(y, yr)
    Sim(stat_short=True).rmsnorm(x, w, EPS, None, None, y)
    out["a-statistic-short"] = _rel(y, yr)
    at = tuple(int(i) for i in (yr.float().abs() == yr.float().abs().max()).nonzero()[0])
    Sim(bump=("y", at, 2)).rmsnorm(x, w, EPS, None, None, y)
    out["l-one-element-2ulp"] = _rel(y, yr)
    # test_slab_consumers: slab_rope_append into zero caches, (h) and (g)
    Mpad, H, Hkv, D = 32, 4, 2, 128
    qkv = torch.randn(2, Mpad, (H + 2 * Hkv) * D)
    pos = torch.arange(Mpad, dtype=I32)
    cs = R.rope_cos_sin(D, 256, 10000.0)
    slots = torch.arange(Mpad, dtype=I32)
    slots[-5:] = -1
    caches = [torch.zeros(4, Hkv, 16, D, dtype=BF) for _ in range(4)]
    R.slab_rope_append(qkv, pos, cs, caches[0], caches[1], slots, H, Hkv, D)
    q = torch.empty(Mpad, H * D, dtype=BF)
    Sim(v_last_head=True).slab_rope_append(qkv, pos, cs, q, caches[2], caches[3], slots, H, Hkv, D, None)
    out["h-v-last-head"] = _rel(caches[3], caches[1])
    return out


def test_old_criterion_accepts():
    """The reason for this file: (a) and (l) pass the norm ratio of the older
    tests on their shapes. (h) with a zero-initialised cache was expected to
    pass it too. That expectation is wrong and this test asserts the opposite
    of it: one of Hkv heads is sqrt(1 / Hkv) of the norm whatever the cache
    held, so the old criterion rejects (h) at about 0.7 (module docstring).
    The new checker rejects each of them (tests above)."""
    r = old_ratios()
    for name, v in r.items():
        print(f"row-exact old criterion {name}: {v:.5f} (accepts below 1e-2)")
    assert r["clean"] < 1e-2
    assert r["a-statistic-short"] < 1e-2
    assert r["l-one-element-2ulp"] < 1e-2
    assert abs(r["h-v-last-head"] - math.sqrt(0.5)) < 0.02
