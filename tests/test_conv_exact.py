"""The VITS conv kernels (``csrc/kernels/conv1d.hip``), one element at a time.

``loqa_conv1d`` has three code paths (the register form and the LDS form with
64- or 32-channel chunks) and an epilogue that fuses bias, activation, residual
add, scale, accumulate, length mask, the gate's cross-lane exchange and a bf16
or PCM16 store at ``to * ostride + ophase``. A whole-tensor norm ratio cannot
see one wrong tap in a padded row, a ``lens`` mask off by one row, one wrong
element or a store next to the output. Two input families and one checker:

**Integer family, compared bitwise.** ``x`` holds integers in [-4, 4], ``w``
in [-2, 2] (dense), ``bias`` / ``res`` / ``acc`` small integers, ``alpha`` in
{1, 0.5, -1}, ``pre_slope`` in {None, 0.5}, ``K * Cin <= 1408``. Every partial
sum is a multiple of 0.5 below 2^24, so fp32 accumulation is exact in any
order, ``(y + bias + res) * alpha + acc`` is exact, and kernel and reference
(``ops.reference.conv1d`` of the ``.float()`` inputs, rounded once) differ by
nothing. PCM16 (``alpha = 2**-10``) is the same three fp32 operations (clamp,
``* 32767``, round to nearest even) on both sides.

**Operands are views, everything around them is hostile.** ``x`` is a view at
column 8 of ``[B, lead + Tin + trail, Cin + 16]`` (``lead = trail =
(K - 1) * dil`` rows); ``res`` and ``acc`` are views into wider buffers too.
Everything outside the views, and the ``res`` / ``acc`` rows at or past
``lens[b]``, is filled three ways: *cont* (1000: finite and dominating), zeros,
NaN. ``out`` is a view into a sentinel-filled ``[B, Tout + 4, Co + 8]``. The
checker builds the buffer it expects (the buffer before the launch with the
reference in the view's rows) and compares the whole buffer: a store at a
padded channel, at a row of another polyphase phase or past ``Tout`` shows as a
disturbed sentinel. The three fills must give bitwise equal buffers, and rows
at or past ``lens[b]`` must hold ``+0.0`` bits. The flow pattern of
``models/vits.py`` (``x1 = z[..., half:]``, ``out = x1, acc = x1, alpha = -1``)
is part of every case: the ``x0`` half is outside the view.

**Random family, per-element bound.** For tanh, the gate and the tanh PCM16
output, inputs scaled by fan-in. Reference: fp64 on the bf16 operands. Per
output element, with ``n = K * Cin`` and ``S = sum |x| |w|`` (a conv of the
absolute values in fp64):

* pre-activation: ``e = n * 2**-24 * S`` - the worst case of fp32 summation,
  in any order;
* through the activation: tanh has Lipschitz constant 1, the sigmoid 1/4:
  ``d = e`` (tanh), ``d = e_a + e_g / 4 + ulp(a) + ulp(g) / 4`` (gate: both
  pre-activations are rounded to bf16, and a value near a rounding boundary
  may round to the neighbour - one bf16 ulp of ``a``, a quarter ulp of ``g``);
* the residual is added exactly in the reference and the scale multiplies the
  error: ``d <- |alpha| * d``;
* bf16 store: ``bound = d + 2**-8 * |ref|``;
* PCM16 store: ``bound = 0.5 + 32767 * d`` LSB against the unrounded
  ``32767 * clamp(ref)``.

Nothing is added for the bias add, the epilogue's fp32 roundings or the error
of ``tanhf`` / ``__expf`` themselves: ``n * 2**-24 * S`` is far above what a
sum of ``n`` terms really loses, and that slack has to cover them.

Rows at or past ``lens[b]`` have bound 0. The bound is pinned from both sides
on the CPU: an fp32 conv that sums the taps in reverse passes; a candidate with
one element off by 2 bf16 ulps (PCM16: by the bound at that element + 1 LSB)
fails.

**CPU tests that prove the checker** (bottom of the file): a pure-torch
candidate takes the kernel's place. The reverse-order fp32 candidate and
``ops.conv1d`` on CPU tensors pass the whole harness; ten mutants (pad +- 1,
padding read from the buffer, ``lens +- 1``, a tap dropped in the last partial
128-step tile, the gate partner from the neighbouring 16-channel block, a store
at ``oc = cout_real``, ``ophase + 1``, ``Tq`` one short, ``acc`` before
``alpha``, one element off by 2 ulps) each fail in the elements they touch.

**The old criterion** (``|y - ref| / |ref| < 1e-2`` over ``[2, 300, C]``, dense
operands, so what lies around a row is more rows of the same kind; 400 LSB for
PCM16) on the same mutants, ``test_old_criterion_accepts``:

    (b) padding read from the buffer          0.049     in one row only  0.0124
    (c) lens + 1 / lens - 1                   0.038 / 0.061
    (d) tap dropped in the last partial tile  0.043     in one row only  0.0075
    (j) one element off by 2 bf16 ulps        0.0013    PCM16: 12 LSB of 400

At B = 2, T = 300 a fault in every row of a padded edge, a tile edge or at
``lens`` is 4 to 6 times over the old bound - where the old tests ran the code
at all (never the register form, never a view, never ``T`` = 128 / 129 or a
``lens`` on a tile edge); a fault within one row or one element is under it.
The test asserts that for (d) in one row and for (j).

T = 257 alone cannot show (d): the single row of its last tile has its last
taps in the padding. Three 300-row cases (one per kernel form) are added to
the table of the integer family for that.

Worst ``err / bound`` observed on an MI355X (random family). The store's
rounding is most of it and is the same for any accurate candidate, so the
second figure leaves it out: the worst ``(err - store term) / d`` (store term
``2**-8 * |ref|`` or 0.5 LSB; negative: the error never left the store term):

                        gated            tanh             tanh -> PCM16
    register form       0.8205 -0.0000   0.9869 -0.0027   0.4847 +0.0006
    LDS form, 32 ch.    0.7848 -0.0000   0.9498 -0.0013   0.3102 -0.0002
    LDS form, 64 ch.    0.7825 -0.0000   0.8708 -0.0119   0.1007 +0.0002

(the reverse-order fp32 candidate on the CPU: the same first figures, second
figures up to +0.11 on the gate.) Beyond the store term the kernels' error is at most
0.0006 of ``d``: a later tightening can divide ``e`` by a large factor.

The integer family is bitwise equal on all three forms, the three fills give
bitwise equal buffers and no sentinel is disturbed: no kernel needed a fix.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from loqa_hub_amd import ops
from loqa_hub_amd.ops import _lib
from loqa_hub_amd.ops import reference as R

FILLS = ("cont", "zeros", "nan")
SENT = -7.0            # bf16 sentinel around ``out``
SENT_PCM = -7777       # int16 sentinel
B = 3
BF, I16 = torch.bfloat16, torch.int16


# -------------------------------------------------------------------- cases
class Shape:
    """One conv: the kernel form it must take and its sizes."""

    def __init__(self, name, form, Cin, K, dil=1, stride=1):
        self.name, self.form, self.Cin, self.K, self.dil, self.stride = name, form, Cin, K, dil, stride
        self.span = (K - 1) * dil
        self.pad = self.span // 2

    def tout(self, Tin):
        return (Tin + 2 * self.pad - self.span - 1) // self.stride + 1


SHAPES = {s.name: s for s in [
    Shape("reg-c16", 0, 16, 7), Shape("reg-c48", 0, 48, 7), Shape("reg-s2", 0, 64, 3, stride=2),
    Shape("reg-k17", 0, 32, 17),
    Shape("lds64-c64", 64, 64, 5), Shape("lds64-c192", 64, 192, 5),
    Shape("lds32-c32", 32, 32, 5), Shape("lds32-c96", 32, 96, 5), Shape("lds32-c128", 32, 128, 11, dil=5),
    # K 7, dil 3 for Tin 1 and 2: every tap but the centre is padding
    Shape("reg-c16-d3", 0, 16, 7, dil=3), Shape("lds32-c32-d3", 32, 32, 7, dil=3),
    Shape("lds64-c64-d3", 64, 64, 7, dil=3),
]}
MAIN = [n for n in SHAPES if not n.endswith("-d3")]
TINY = [n for n in SHAPES if n.endswith("-d3")]
TIMES = {"257": (257, None), "257-edge": (257, (257, 129, 1)), "257-tile": (257, (128, 127, 0)),
         "128": (128, None), "1": (1, None), "2": (2, None),
         # a last tile of 44 rows: at 257 the one row of the last tile has its last taps in the padding
         "300": (300, (300, 211, 130))}
COUTS = (32, 16, 1)
INT_CASES = ([(s, co, t) for s in MAIN for co in COUTS for t in ("257", "257-edge", "257-tile", "128")]
             + [(s, co, t) for s in TINY for co in COUTS for t in ("1", "2")]
             + [(s, 32, "300") for s in ("reg-c48", "lds64-c64", "lds32-c128")])

# epilogues of the integer family: act, pre_slope, alpha, res, acc ("own": a
# buffer of its own, "out": aliased to out, "flow": out = acc = x1 of a z
# buffer whose x0 half must stay), pcm16
EPIS = {
    "plain": dict(act=None, pre=None, alpha=1.0, res=False, acc=None, pcm=False),
    "res-alpha": dict(act="relu", pre=0.5, alpha=0.5, res=True, acc=None, pcm=False),
    "inplace": dict(act=None, pre=0.5, alpha=1.0, res=False, acc="out", pcm=False),
    "all": dict(act="relu", pre=None, alpha=0.5, res=True, acc="own", pcm=False),
    "flow": dict(act=None, pre=None, alpha=-1.0, res=False, acc="flow", pcm=False),
    "pcm16": dict(act=None, pre=0.5, alpha=2.0 ** -10, res=True, acc=None, pcm=True),
}

# random family: shape, Cout (of the weight), act, pre_slope, pcm16
RAND_SHAPES = {s.name: s for s in [
    Shape("reg-c48", 0, 48, 5), Shape("lds32-c96", 32, 96, 5), Shape("lds64-c192", 64, 192, 5),
    Shape("reg-c16", 0, 16, 7), Shape("lds32-c32", 32, 32, 7), Shape("lds64-c64", 64, 64, 7),
]}
RAND_CASES = [
    ("reg-c48", 64, "gated", None, False), ("lds32-c96", 64, "gated", None, False),
    ("lds64-c192", 384, "gated", None, False),
    ("reg-c16", 16, "tanh", 0.1, False), ("lds32-c32", 32, "tanh", None, False),
    ("lds64-c64", 1, "tanh", 0.1, False),
    ("reg-c16", 1, "tanh", 0.01, True), ("lds32-c32", 1, "tanh", 0.01, True),
    ("lds64-c64", 1, "tanh", 0.01, True),
]
RAND_T, RAND_LENS = 257, (257, 129, 128)

TRANS = [(64, 32, 16, 8, 64), (32, 16, 4, 2, 32), (16, 16, 4, 2, 0)]     # Cin, Cout, Kt, s, form
TRANS_T = (1, 2, 17, 129)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _fillv(fill):
    return {"cont": 1000.0, "zeros": 0.0, "nan": float("nan")}[fill]


def _embed(core, lead, trail, col, extra, fill, g=None):
    """``core`` [B, T, C] as rows [lead, lead + T), columns [col, col + C) of a
    buffer [B, lead + T + trail, C + extra] filled with ``fill`` ("benign":
    values like the operand's own, what a dense tensor has around a row)."""
    Bn, T, C = core.shape
    if fill == "benign":
        buf = core.flatten()[torch.randint(0, core.numel(), (Bn, lead + T + trail, C + extra), generator=g)]
    else:
        buf = torch.full((Bn, lead + T + trail, C + extra), _fillv(fill))
    buf[:, lead:lead + T, col:col + C] = core
    return buf.to(BF)


class Case:
    """Weights and operand values of one conv launch (CPU, float, all values
    exact in bf16) and the keyword arguments of ``ops.conv1d``."""

    def __init__(self, shape, Cout, Tin, lens, *, act=None, pre=None, alpha=1.0, res=False, acc=None,
                 pcm=False, family="int", seed=0, Bn=B, ostride=1, ophase=0, Tq=None, Tout=None,
                 pad=None, w=None, bias=None, x=None):
        g = torch.Generator().manual_seed(seed)
        self.shape, self.Cout, self.Tin, self.B = shape, Cout, Tin, Bn
        self.act, self.pre, self.alpha, self.pcm, self.accmode = act, pre, alpha, pcm, acc
        self.family = family
        Cin, K = shape.Cin, shape.K
        self.Co = Cout // 2 if act == "gated" else Cout
        self.pad = shape.pad if pad is None else pad
        self.Tq = shape.tout(Tin) if Tq is None else Tq
        self.ostride, self.ophase = ostride, ophase
        self.Tout = Tout if Tout is not None else self.Tq * ostride + ophase
        self.lens = None if lens is None else torch.tensor(lens[:Bn], dtype=torch.int32)
        n = K * Cin
        if family == "int":
            self.w = _ints(g, -2, 2, Cout, Cin, K) if w is None else w
            self.bias = _ints(g, -3, 3, Cout) if bias is None else bias
            self.x = _ints(g, -4, 4, Bn, Tin, Cin) if x is None else x
            self.res = _ints(g, -8, 8, Bn, self.Tout, self.Co) if res else None
            accv = _ints(g, -8, 8, Bn, self.Tout, self.Co)
            self.x0 = _ints(g, -8, 8, Bn, self.Tout, self.Co)
        else:
            r = lambda *s: torch.randn(*s, generator=g)
            self.w = (r(Cout, Cin, K) * n ** -0.5).to(BF).float()
            self.bias = (r(Cout) * 0.1).to(BF).float()
            self.x = r(Bn, Tin, Cin).to(BF).float()
            self.res = r(Bn, self.Tout, self.Co).to(BF).float() if res else None
            accv = r(Bn, self.Tout, self.Co).to(BF).float()
            self.x0 = accv.flip(0)
        self.acc = accv if acc else None
        self._cw = {}

    def cw(self, dev):
        if dev not in self._cw:
            self._cw[dev] = ops.ConvWeight(self.w.to(dev), self.bias.to(dev), gated=self.act == "gated")
        return self._cw[dev]

    def past_lens(self):
        """[B, Tout] bool: output rows at or past ``lens[b]``."""
        if self.lens is None:
            return torch.zeros(self.B, self.Tout, dtype=torch.bool)
        return torch.arange(self.Tout)[None, :] >= self.lens[:, None]

    def operands(self, fill, dev="cpu", g=None):
        """-> (x, kwargs, outbuf, view): hostile buffers on ``dev``; ``view`` is
        the (rows, columns) slice of ``out`` within ``outbuf``."""
        sh, Co, T = self.shape, self.Co, self.Tout
        x = _embed(self.x, sh.span, sh.span, 8, 16, fill, g).to(dev)[:, sh.span:sh.span + self.Tin, 8:8 + sh.Cin]
        past = self.past_lens()[..., None]

        def side(v):
            if fill != "benign":
                v = torch.where(past, torch.full((), _fillv(fill)), v)
            return _embed(v, 2, 2, 8, 16, fill, g).to(dev)[:, 2:2 + T, 8:8 + Co]
        kw = dict(dil=sh.dil, pad=self.pad, stride=sh.stride, pre_slope=self.pre, act=self.act,
                  alpha=self.alpha, pcm16=self.pcm, lens=None if self.lens is None else self.lens.to(dev))
        if self.ostride != 1 or self.ophase or self.Tq != self.Tout:
            kw.update(ostride=self.ostride, ophase=self.ophase, Tq=self.Tq, Tout=self.Tout)
        if self.res is not None:
            kw["res"] = side(self.res)
        c0 = 4
        if self.pcm:
            outbuf = torch.full((self.B, T + 4, Co + 8), SENT_PCM, dtype=I16)
        elif self.accmode == "flow":
            c0 = 4 + Co
            outbuf = torch.full((self.B, T + 4, 2 * Co + 8), SENT).to(BF)
            outbuf[:, 2:2 + T, 4:4 + Co] = self.x0.to(BF)
        else:
            outbuf = torch.full((self.B, T + 4, Co + 8), SENT).to(BF)
        view = (slice(2, 2 + T), slice(c0, c0 + Co))
        if self.accmode in ("out", "flow"):
            a = self.acc if fill == "benign" else torch.where(past, torch.full((), _fillv(fill)), self.acc)
            outbuf[:, view[0], view[1]] = a.to(BF)
        outbuf = outbuf.to(dev)
        out = outbuf[:, view[0], view[1]]
        if self.accmode == "own":
            kw["acc"] = side(self.acc)
        elif self.accmode:
            kw["acc"] = out
        kw["out"] = out
        return x, kw, outbuf, view

    def rows(self):
        """Output rows this launch stores (all of them unless polyphase)."""
        oi = torch.arange(self.Tq) * self.ostride + self.ophase
        return oi[(oi >= 0) & (oi < self.Tout)]

    @functools.cached_property
    def ref(self):
        """Integer family: ``ops.reference.conv1d`` of the float operands,
        rounded once -> [B, Tout, Co] bf16 or int16."""
        y = R.conv1d(self.x, self.w, self.bias, dil=self.shape.dil, pad=self.pad, stride=self.shape.stride,
                     pre_slope=self.pre, act=self.act, res=self.res, alpha=self.alpha, acc=self.acc,
                     lens=self.lens, Tout=self.Tout, ostride=self.ostride, ophase=self.ophase, Tq=self.Tq)
        if self.pcm:
            return (y.clamp(-1, 1) * 32767).round().to(I16)
        return y.to(BF)

    @functools.cached_property
    def ref64(self):
        """Random family: fp64 reference and the per-element bound (module
        docstring) -> (ref, bound, d), PCM16 in LSB; ``bound - d`` is the store term."""
        sh = self.shape
        xf = self.x if self.pre is None else F.leaky_relu(self.x, self.pre)
        xd, wd = xf.to(BF).double().transpose(1, 2), self.w.double()
        conv = lambda a, b: F.conv1d(a, b, None, stride=sh.stride, padding=self.pad,
                                     dilation=sh.dil).transpose(1, 2)[:, :self.Tq]
        pre = conv(xd, wd) + self.bias.double()
        e = sh.K * sh.Cin * 2.0 ** -24 * conv(xd.abs(), wd.abs())
        ulp = lambda v: torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)
        if self.act == "gated":
            Hh = self.Co
            a, gt = pre[..., :Hh].to(BF).double(), pre[..., Hh:].to(BF).double()
            v = torch.tanh(a) * torch.sigmoid(gt)
            d = e[..., :Hh] + e[..., Hh:] / 4 + ulp(a) + ulp(gt) / 4
        elif self.act == "tanh":
            v, d = torch.tanh(pre), e
        else:
            v, d = (torch.relu(pre) if self.act == "relu" else pre), e
        if self.res is not None:
            v = v + self.res.double()
        t = v * self.alpha
        ref = t + self.acc.double() if self.acc is not None else t
        past = self.past_lens()[..., None]
        ref, d = ref.masked_fill(past, 0.0), (abs(self.alpha) * d).masked_fill(past, 0.0)
        if self.pcm:
            ref, d, store = 32767 * ref.clamp(-1, 1), 32767 * d, torch.full_like(d, 0.5).masked_fill(past, 0.0)
        else:
            store = 2.0 ** -8 * ref.abs()
        return ref, d + store, d


@functools.lru_cache(maxsize=None)
def int_case(sname, Cout, tname, epi):
    Tin, lens = TIMES[tname]
    e = EPIS[epi]
    return Case(SHAPES[sname], Cout, Tin, lens, act=e["act"], pre=e["pre"], alpha=e["alpha"], res=e["res"],
                acc=e["acc"], pcm=e["pcm"], seed=len(sname) + Cout + Tin)


@functools.lru_cache(maxsize=None)
def rand_case(sname, Cout, act, pre, pcm):
    return Case(RAND_SHAPES[sname], Cout, RAND_T, RAND_LENS, act=act, pre=pre, alpha=1.0 if pcm else 0.5,
                res=not pcm, pcm=pcm, family="rand", seed=7)


# ------------------------------------------------------------------ checker
class Report:
    """What one candidate did on one case: per fill the whole ``out`` buffer
    after the launch, and the buffer that was expected."""

    def __init__(self, case, view, before, after, expected=None, err=None, bound=None):
        self.case, self.view, self.before, self.after = case, view, before, after
        self.expected, self.err, self.bound = expected, err, bound

    def bad(self, fill="cont"):
        """[B, rows, cols] bool over the whole buffer: elements that differ from
        the expected buffer (NaN differs from everything)."""
        a = self.after[fill].double()
        if self.expected is not None:
            return a != self.expected.double()
        bad = a != self.before[fill].double()             # outside the view: untouched
        r, c = self.view
        bad[:, r, c] = ~(self.err[fill] <= self.bound)      # NaN misses every bound
        return bad

    def in_view(self, bad):
        r, c = self.view
        return bad[:, r, c]

    def outside(self, bad):
        bad = bad.clone()
        r, c = self.view
        bad[:, r, c] = False
        return bad

    def fills_equal(self):
        bits = [self.after[f].view(I16) for f in FILLS]
        return all(torch.equal(bits[0], b) for b in bits[1:])

    def masked_bits(self, fill="cont"):
        """Bits of the rows at or past ``lens[b]`` (must all be 0: +0.0)."""
        r, c = self.view
        return self.after[fill][:, r, c].view(I16)[self.case.past_lens()]

    def worst(self):
        pos = self.bound > 0
        return float((self.err["cont"][pos] / self.bound[pos]).max())

    def worst_sum(self):
        """Worst (err - store term) / d: what the sums and the activation lost."""
        pos = self.d > 0
        return float(((self.err["cont"] - (self.bound - self.d))[pos] / self.d[pos]).max())

    def assert_clean(self, what):
        for f in self.after:
            bad = self.bad(f)
            assert not self.outside(bad).any(), (what, f, "stored outside the output view at",
                                                 self.outside(bad).nonzero()[:8].tolist())
            assert not bad.any(), (what, f, int(bad.sum()), "elements differ from the reference, first at",
                                   self.in_view(bad).nonzero()[:8].tolist())
            assert not self.masked_bits(f).any(), (what, f, "rows at or past lens are not +0.0")
        if len(self.after) > 1:
            assert self.fills_equal(), (what, "the fill of outside memory changes the output")


def run_case(case, fn, dev="cpu", fills=FILLS):
    """Launch ``fn`` (a stand-in for ``ops.conv1d``) on ``case`` under every
    fill of the outside memory."""
    before, after = {}, {}
    for f in fills:
        x, kw, outbuf, view = case.operands(f, dev)
        before[f] = outbuf.cpu().clone()
        y = fn(x, case.cw(dev), **kw)
        assert y.data_ptr() == kw["out"].data_ptr()
        after[f] = outbuf.cpu()
    rep = Report(case, view, before, after)
    rows = case.rows()
    if case.family == "int":
        exp = before["cont"].clone()
        full = exp[:, view[0], view[1]]
        full[:, rows] = case.ref[:, rows]     # the same under every fill: an aliased acc is overwritten
        rep.expected = exp
    else:
        assert rows.numel() == case.Tout
        ref, rep.bound, rep.d = case.ref64
        rep.err = {f: (after[f][:, view[0], view[1]].double() - ref).abs() for f in fills}
    return rep


def assert_form(shape):
    got = _lib.kernels().loqa_conv1d_form(shape.Cin, shape.K, shape.dil, shape.stride)
    assert got == shape.form, (shape.name, "runs kernel form", got, "not", shape.form)


def check_int(sname, Cout, tname, fn, dev):
    for epi in EPIS:
        run_case(int_case(sname, Cout, tname, epi), fn, dev).assert_clean((sname, Cout, tname, epi))


def check_rand(sname, Cout, act, pre, pcm, fn, dev):
    rep = run_case(rand_case(sname, Cout, act, pre, pcm), fn, dev)
    path = "pcm16" if pcm else act
    print(f"conv-exact random {path} form {RAND_SHAPES[sname].form}: worst err/bound {rep.worst():.4f}, "
          f"without the store term {rep.worst_sum():+.4f}")
    rep.assert_clean((sname, Cout, act, pcm))
    return rep


# ---- transposed convolution: all phases through ops.conv_transpose1d, and one
# phase at a time into a sentinel-filled buffer
class TCase:
    def __init__(self, Cin, Cout, Kt, s, Tin):
        g = torch.Generator().manual_seed(Cin + Kt + Tin)
        self.Cin, self.Cout, self.Kt, self.s, self.Tin, self.p = Cin, Cout, Kt, s, Tin, (Kt - s) // 2
        self.w = _ints(g, -2, 2, Cin, Cout, Kt)
        self.bias = _ints(g, -3, 3, Cout)
        self.x = _ints(g, -4, 4, 2, Tin, Cin)
        self.taps = Kt // s
        self.shape = Shape("phase", None, Cin, self.taps)
        self.Tout = (Tin - 1) * s - 2 * self.p + Kt
        self._ct = {}

    def ct(self, dev):
        if dev not in self._ct:
            self._ct[dev] = ops.ConvTransposeWeight(self.w.to(dev), self.bias.to(dev), self.s, self.p)
        return self._ct[dev]

    def xview(self, fill, dev):
        sp = self.taps - 1
        return _embed(self.x, sp, sp, 8, 16, fill).to(dev)[:, sp:sp + self.Tin, 8:8 + self.Cin]

    @functools.cached_property
    def ref(self):
        """torch's conv_transpose1d of the float operands, rounded once."""
        y = F.conv_transpose1d(F.leaky_relu(self.x, 0.5).transpose(1, 2), self.w, self.bias, stride=self.s,
                               padding=self.p)
        return y.transpose(1, 2).to(BF)

    def phase(self, r, dev):
        """Phase ``r`` as a ``Case`` (same x, the phase's taps as its weight)."""
        cwr = self.ct(dev).phases[r]
        Tq = (self.Tout - r + self.p + self.s - 1) // self.s
        c = Case(self.shape, self.Cout, self.Tin, None, pre=0.5, Bn=2, ostride=self.s, ophase=r - self.p, Tq=Tq,
                 Tout=self.Tout, pad=self.taps - 1, w=cwr.w.cpu().float(), bias=self.bias, x=self.x)
        c._cw[dev] = cwr
        c.ref = self.ref
        return c


@functools.lru_cache(maxsize=None)
def trans_case(Cin, Cout, Kt, s, Tin):
    return TCase(Cin, Cout, Kt, s, Tin)


def check_transpose(tc, dev, conv_fn, full_fn):
    outs = [full_fn(tc.xview(f, dev), tc.ct(dev), pre_slope=0.5).cpu() for f in FILLS]
    assert outs[0].shape == tc.ref.shape and torch.equal(outs[0], tc.ref), "all phases"
    for o in outs[1:]:
        assert torch.equal(o.view(I16), outs[0].view(I16)), "the fill of outside memory changes the output"
    for r in range(tc.s):
        run_case(tc.phase(r, dev), conv_fn, dev).assert_clean(("phase", r))


# ---- expand_sample with noise_scale = 0: a gather of the mean rows
def expand_case(dev):
    g = torch.Generator().manual_seed(5)
    Bn, T, C = 4, 37, 64
    dur = torch.randint(1, 5, (Bn, T), generator=g, dtype=torch.int32)
    dur[0, 0] = 0                       # cum[b, 0] == 0
    dur[1, :3] = 0
    dur[1, 10:17] = 0                   # a run of zeros in the middle
    dur[2] = 0                          # flen == 0
    dur[3, 20:] = 0                     # zeros to the end
    cum = torch.cumsum(dur, 1, dtype=torch.int32)
    flen = cum[:, -1].contiguous()
    Fr = -(-int(flen.max()) // 32) * 32 + 32              # frame-padded
    core = torch.randn(Bn, T, 2 * C, generator=g)
    stats = _embed(core, 0, 0, 8, 16, "nan").to(dev)[..., 8:8 + 2 * C]      # ld != 2C, NaN beside the rows
    want = torch.zeros(Bn, Fr, C, dtype=BF)
    for b in range(Bn):
        f = torch.arange(int(flen[b]))
        want[b, :int(flen[b])] = core.to(BF)[b, torch.searchsorted(cum[b], f.int(), right=True), :C]
    return stats, cum.to(dev), flen.to(dev), Fr, want


def check_expand(dev):
    stats, cum, flen, Fr, want = expand_case(dev)
    assert stats.stride(1) != stats.shape[2] and int(flen.min()) == 0
    z = ops.expand_sample(stats, cum, flen, Fr, 0.0)
    assert z.shape == want.shape and torch.equal(z.cpu(), want)


# ---------------------------------------------------------------- GPU tests
DEV = "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("sname,Cout,tname", INT_CASES)
def test_conv_integer_exact(sname, Cout, tname):
    """Every epilogue of the integer family, bitwise, under the three fills."""
    assert_form(SHAPES[sname])
    check_int(sname, Cout, tname, ops.conv1d, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("sname,Cout,act,pre,pcm", RAND_CASES)
def test_conv_random_bound(sname, Cout, act, pre, pcm):
    assert_form(RAND_SHAPES[sname])
    check_rand(sname, Cout, act, pre, pcm, ops.conv1d, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("Tin", TRANS_T)
@pytest.mark.parametrize("Cin,Cout,Kt,s,form", TRANS)
def test_conv_transpose_exact(Cin, Cout, Kt, s, form, Tin):
    assert _lib.kernels().loqa_conv1d_form(Cin, Kt // s, 1, 1) == form
    check_transpose(trans_case(Cin, Cout, Kt, s, Tin), DEV, ops.conv1d, ops.conv_transpose1d)


@pytest.mark.gpu
def test_expand_sample_gathers_means_exactly():
    check_expand(DEV)


@pytest.mark.gpu
def test_expand_sample_refuses_other_batch_stride():
    """The kernel addresses row (b, i) at (b * T + i) * ld: a view whose batch
    stride is not T rows must not reach it."""
    stats, cum, flen, Fr, _ = expand_case(DEV)
    wide = torch.zeros(stats.shape[0], stats.shape[1] + 3, stats.shape[2], dtype=BF, device=DEV)
    with pytest.raises(AssertionError):
        ops.expand_sample(wide[:, :stats.shape[1]], cum, flen, Fr, 0.0)


# -------------------------------------------- CPU: a candidate in torch, mutants
def sim_conv1d(x, cw, *, dil=1, pad=None, stride=1, pre_slope=None, act=None, res=None, alpha=1.0,
               acc=None, lens=None, out=None, pcm16=False, Tout=None, ostride=1, ophase=0, Tq=None,
               mut=None):
    """``ops.conv1d`` in plain torch with the kernel's arithmetic - fp32 sums
    (taps in REVERSE order, one matmul per tap), the kernel's epilogue order,
    one rounding - and, through ``mut``, its possible faults."""
    mut = mut or {}
    Bn, Tin, Cin = x.shape
    K, span = cw.K, dil * (cw.K - 1)
    pad = span // 2 if pad is None else pad
    Tq = (Tin + 2 * pad - span - 1) // stride + 1 if Tq is None else Tq
    T_out = Tout if Tout is not None else Tq * ostride + ophase
    Co = cw.out_channels
    padl = pad + mut.get("pad", 0)
    padr = max(0, (Tq - 1) * stride - padl + span - (Tin - 1))
    w = cw.w.to(BF).float()

    def sums(from_buffer, drop):
        if from_buffer:                 # the rows around the view instead of zeros
            xp = x.as_strided((Bn, padl + Tin + padr, Cin), x.stride(),
                              x.storage_offset() - padl * x.stride(1)).float()
        else:
            xp = F.pad(x.float(), (0, 0, padl, padr))
        if pre_slope is not None:
            xp = F.leaky_relu(xp, pre_slope)
        xp = xp.to(BF).float()
        y = torch.zeros(Bn, Tq, w.shape[0])
        for tap in reversed(range(K)):
            t = xp[:, tap * dil: tap * dil + (Tq - 1) * stride + 1: stride] @ w[:, :, tap].t()
            if drop and tap == K - 1 and Tq % 128:
                t[:, Tq // 128 * 128:] = 0
            y = y + t
        return y
    y = sums(mut.get("pad_from_buffer"), mut.get("drop_tail_tap"))
    if "only_row" in mut:               # the fault in the sums confined to one output row
        clean = sums(False, False)
        clean[mut["only_row"]] = y[mut["only_row"]]
        y = clean
    if cw.bias is not None:
        y = y + cw.bias.to(BF).float()
    if act == "relu":
        y = torch.relu(y)
    elif act == "tanh":
        y = torch.tanh(y)
    elif act == "gated":
        a, gt = y[..., :Co].to(BF).float(), y[..., Co:].to(BF).float()
        if mut.get("gate_neighbour"):
            gt = gt.roll(16, -1)
        y = torch.tanh(a) * torch.sigmoid(gt)
    q = torch.arange(Tq)
    oi = q * ostride + ophase
    ok = (oi >= 0) & (oi < T_out) & (q < Tq - mut.get("tq_short", 0))
    idx, v = oi[ok], y[:, ok]
    r = res[:, idx].float() if res is not None else 0.0
    c = acc[:, idx].float() if acc is not None else 0.0
    v = (v + r + c) * alpha if mut.get("acc_before_alpha") else (v + r) * alpha + c
    if lens is not None:
        v = v.masked_fill((idx[None, :] >= (lens.long() + mut.get("lens", 0))[:, None])[..., None], 0.0)
    s = (v.clamp(-1, 1) * 32767).round().to(I16) if pcm16 else v.to(BF)
    if out is None:
        out = torch.zeros(Bn, T_out, Co, dtype=s.dtype)
    idx = idx + mut.get("ophase", 0)
    keep = idx < T_out
    out[:, idx[keep]] = s[:, keep]
    if mut.get("store_pad_channel"):    # oc = cout_real is stored too
        wide = out.as_strided((Bn, T_out, Co + 1), out.stride(), out.storage_offset())
        wide[:, idx[keep], Co] = s[:, keep, 0]
    if "bump" in mut:                   # one element off: (b, t, c, steps)
        b_, t_, c_, n = mut["bump"]
        if pcm16:
            out[b_, t_, c_] += n
        else:
            bits = out.view(I16)
            bits[b_, t_, c_] += n
    return out


def mutant(**mut):
    return functools.partial(sim_conv1d, mut=mut)


CPU_INT = [("reg-c16", 1, "257-edge"), ("lds64-c64", 32, "257-tile"), ("lds32-c128", 16, "257"),
           ("reg-s2", 32, "257-edge"), ("reg-k17", 16, "128"), ("lds64-c64-d3", 32, "1"),
           ("reg-c16-d3", 1, "2")]
CPU_TRANS = [(64, 32, 16, 8, 2), (32, 16, 4, 2, 17), (16, 16, 4, 2, 1)]


def test_cases_cover_every_form():
    for table in (SHAPES, RAND_SHAPES):
        assert {s.form for s in table.values()} == {0, 32, 64}
    assert {SHAPES[s].form for s, _, _ in INT_CASES} == {0, 32, 64}
    assert {RAND_SHAPES[c[0]].form for c in RAND_CASES if c[2] == "gated"} == {0, 32, 64}
    assert {f for *_, f in TRANS} == {0, 32, 64}
    assert len(INT_CASES) + len(RAND_CASES) + len(TRANS) * len(TRANS_T) + 2 == 152
    for s in SHAPES.values():
        assert s.K * s.Cin <= 1408
    for s in list(SHAPES.values()) + list(RAND_SHAPES.values()):     # the dispatch rule needs no GPU
        assert_form(s)


@pytest.mark.parametrize("fn", [sim_conv1d, ops.conv1d], ids=["reverse-taps-fp32", "ops-cpu"])
@pytest.mark.parametrize("sname,Cout,tname", CPU_INT)
def test_checker_passes_integer(sname, Cout, tname, fn):
    """Another summation order and the CPU path of ``ops.conv1d`` are bitwise
    equal to the reference through the whole harness."""
    check_int(sname, Cout, tname, fn, "cpu")


@pytest.mark.parametrize("fn", [sim_conv1d, ops.conv1d], ids=["reverse-taps-fp32", "ops-cpu"])
@pytest.mark.parametrize("sname,Cout,act,pre,pcm", RAND_CASES[::2] + RAND_CASES[1:2])
def test_checker_passes_random(sname, Cout, act, pre, pcm, fn):
    check_rand(sname, Cout, act, pre, pcm, fn, "cpu")


@pytest.mark.parametrize("Cin,Cout,Kt,s,Tin", CPU_TRANS)
def test_checker_passes_transpose(Cin, Cout, Kt, s, Tin):
    for conv_fn in (sim_conv1d, ops.conv1d):
        check_transpose(trans_case(Cin, Cout, Kt, s, Tin), "cpu", conv_fn,
                        functools.partial(ops.conv_transpose1d, polyphase=True))


def test_checker_passes_expand_cpu():
    check_expand("cpu")


def _rows_of(bad):
    """Rows (b, t) of the view with a wrong element -> set."""
    return {(int(b), int(t)) for b, t in bad.any(-1).nonzero().tolist()}


M_CASE = ("lds64-c64", 32, "257-edge")      # K 5, pad 2, Tout 257, lens [257, 129, 1]


@pytest.mark.parametrize("epi", ["plain", "all", "pcm16"])
@pytest.mark.parametrize("delta", [1, -1])
def test_mutant_pad(delta, epi):
    """(a) pad +- 1: every unmasked row is wrong."""
    c = int_case(*M_CASE, epi)
    rep = run_case(c, mutant(pad=delta))
    bad = rep.in_view(rep.bad())
    live = (~c.past_lens()).sum()
    assert not rep.outside(rep.bad()).any()
    assert len(_rows_of(bad)) >= 0.9 * int(live)


@pytest.mark.parametrize("sname", ["lds64-c64", "reg-c16", "lds32-c128"])
def test_mutant_padding_from_buffer(sname):
    """(b) padding rows read from the buffer: invisible with zeros around x,
    wrong in the first and last ``pad`` rows with the cont fill, NaN there with
    the NaN fill - and only there."""
    c = int_case(sname, 32, "257", "plain")
    rep = run_case(c, mutant(pad_from_buffer=True))
    assert not rep.bad("zeros").any()
    assert not rep.fills_equal()
    pad, T = c.pad, c.Tout
    edge = {(b, t) for b in range(B) for t in list(range(pad)) + list(range(T - pad, T))}
    for f in ("cont", "nan"):
        assert _rows_of(rep.in_view(rep.bad(f))) == edge
        assert not rep.outside(rep.bad(f)).any()


@pytest.mark.parametrize("epi", ["plain", "all", "flow", "pcm16"])
@pytest.mark.parametrize("delta", [1, -1])
def test_mutant_lens(delta, epi):
    """(c) the mask at lens +- 1: exactly one row per batch row is wrong (none
    where the shifted bound leaves [0, Tout])."""
    c = int_case(*M_CASE, epi)
    rep = run_case(c, mutant(lens=delta))
    want = {(b, int(n) + min(delta, 0)) for b, n in enumerate(c.lens) if 0 <= int(n) + min(delta, 0) < c.Tout}
    for f in FILLS:
        if c.pcm and f == "nan" and delta > 0:
            continue        # an int16 cannot hold the NaN of res[lens]; the other fills show the row
        got = _rows_of(rep.in_view(rep.bad(f)))
        # lens - 1 zeroes a row whose reference may be 0 in some channels, never in all
        assert got == want, (f, got, want)
    if delta > 0 and EPIS[epi]["res"]:
        assert not rep.fills_equal()          # the unmasked row adds res[lens] = the fill


@pytest.mark.parametrize("sname", ["reg-c48", "lds64-c64", "lds32-c128"])
def test_mutant_tail_tile_tap(sname):
    """(d) the last tap dropped in the last partial 128-step tile: rows 256 to
    299 less the last ``pad``, whose last tap lies in the padding (which is why
    T = 257 alone cannot show it: the 300-row cases are there for this)."""
    c = int_case(sname, 32, "300", "plain")
    rep = run_case(c, mutant(drop_tail_tap=True))
    got = _rows_of(rep.in_view(rep.bad()))
    assert got == {(b, t) for b in range(B) for t in range(256, min(int(c.lens[b]), 300 - c.pad))}
    assert rep.fills_equal()
    assert not _rows_of(run_case(int_case(sname, 32, "257", "plain"), mutant(drop_tail_tap=True)).bad())


def test_mutant_gate_partner():
    """(e) the gate partner from the neighbouring 16-channel block: every
    unmasked row misses the bound."""
    c = rand_case("lds32-c96", 64, "gated", None, False)
    rep = run_case(c, mutant(gate_neighbour=True))
    bad = rep.in_view(rep.bad())
    assert _rows_of(bad) == {(b, t) for b in range(B) for t in range(int(c.lens[b]))}
    assert float(bad.float().mean()) > 0.3


@pytest.mark.parametrize("Cout,epi", [(16, "plain"), (1, "pcm16"), (16, "flow")])
def test_mutant_store_at_cout_real(Cout, epi):
    """(f) a store at oc = cout_real: the view is right, the sentinel column
    next to it is not."""
    rep = run_case(int_case("lds32-c32", Cout, "257-edge", epi), mutant(store_pad_channel=True))
    bad = rep.bad()
    assert not rep.in_view(bad).any()
    cols = rep.outside(bad).any(0).any(0).nonzero().flatten().tolist()
    assert cols == [rep.view[1].stop]


@pytest.mark.parametrize("Cin,Cout,Kt,s,Tin", CPU_TRANS)
def test_mutant_polyphase(Cin, Cout, Kt, s, Tin):
    """(g) ophase + 1 writes rows of the next phase; (h) Tq one short leaves
    the sentinel in a phase's last row."""
    tc = trans_case(Cin, Cout, Kt, s, Tin)
    for r in range(tc.s):
        c = tc.phase(r, "cpu")
        rows = c.rows()
        rep = run_case(c, mutant(ophase=1))
        got = {t for _, t in _rows_of(rep.in_view(rep.bad()))}
        assert got and got <= set(rows.tolist()) | set((rows + 1).tolist())
        assert set(rows.tolist()) <= got        # own rows keep the sentinel
        rep = run_case(c, mutant(tq_short=1))
        assert {t for _, t in _rows_of(rep.in_view(rep.bad()))} == {int(rows[-1])}
    with pytest.raises(AssertionError):
        check_transpose(tc, "cpu", mutant(tq_short=1), functools.partial(ops.conv_transpose1d, polyphase=True))


@pytest.mark.parametrize("epi", ["all", "flow"])
def test_mutant_acc_before_alpha(epi):
    """(i) (v + res + acc) * alpha instead of (v + res) * alpha + acc."""
    c = int_case(*M_CASE, epi)
    rep = run_case(c, mutant(acc_before_alpha=True))
    bad = rep.in_view(rep.bad())
    assert not c.past_lens()[bad.any(-1)].any() and float(bad[~c.past_lens()].float().mean()) > 0.5


def _bump_at(score, past):
    """The element of largest ``score`` among the unmasked rows -> (b, t, c)."""
    a = score.double().masked_fill(past[..., None], float("-inf"))
    b_, t_, c_ = [int(i) for i in (a == a.max()).nonzero()[0]]
    return b_, t_, c_


@pytest.mark.parametrize("kind", ["int", "tanh", "pcm16-int", "pcm16-tanh"])
def test_mutant_one_element(kind):
    """(j) one element off by 2 bf16 ulps (PCM16: by more than the bound at
    that element): exactly that element fails."""
    if kind == "int":
        c = int_case(*M_CASE, "all")
        at, n = _bump_at(c.ref.float().abs(), c.past_lens()), 2
    elif kind == "pcm16-int":
        c = int_case(*M_CASE, "pcm16")
        at, n = _bump_at(-(c.ref.float().abs()), c.past_lens()), 1       # away from the clamp
    else:
        c = rand_case("lds64-c64", 1, "tanh", 0.1 if kind == "tanh" else 0.01, kind != "tanh")
        ref, bound, _ = c.ref64
        at = _bump_at(ref.abs() if kind == "tanh" else -ref.abs(), c.past_lens())
        n = 2 if kind == "tanh" else int(math.ceil(2 * float(bound[at]))) + 1
    rep = run_case(c, mutant(bump=(*at, n)))
    bad = rep.bad()
    assert not rep.outside(bad).any()
    assert rep.in_view(bad).nonzero().tolist() == [list(at)]


# ---- what the old criterion saw: ||y - ref|| / ||ref|| < 1e-2 on [2, 300, C]
OLD_MUTANTS = {
    "b-padding-from-buffer": dict(pad_from_buffer=True),
    "b-in-one-row": dict(pad_from_buffer=True, only_row=(1, 0)),
    "c-lens+1": dict(lens=1),
    "c-lens-1": dict(lens=-1),
    "d-tail-tile-tap": dict(drop_tail_tap=True),
    "d-in-one-row": dict(drop_tail_tap=True, only_row=(0, 256)),
    "j-one-element-2ulp": "bump",
}
# measured here (the ratios are printed): a fault in every row of a tile edge,
# a padded edge or at lens is 4 to 6 times over the old bound at this size -
# where the old tests ran the code at all; three padded taps of seven in one row
# are just over it, one tap in one row and one element are under it
OLD_ACCEPTS = ("d-in-one-row", "j-one-element-2ulp")


@functools.lru_cache(maxsize=None)
def old_case():
    """``test_kernels_gpu.py::test_conv1d_mfma`` (64, 32, 7, 3, relu, 0.1):
    B = 2, T = 300, res of the output's magnitude, alpha 0.5, lens [300, 211]."""
    return Case(Shape("old", 64, 64, 7, dil=3), 32, 300, (300, 211), act="relu", pre=0.1, alpha=0.5, res=True,
                family="rand", seed=0, Bn=2)


def old_ratio(mut):
    c = old_case()
    if mut == "bump":
        mut = dict(bump=(*_bump_at(c.ref64[0].abs(), c.past_lens()), 2))
    x, kw, outbuf, view = c.operands("benign", g=torch.Generator().manual_seed(1))
    y = sim_conv1d(x, c.cw("cpu"), **kw, mut=mut).float()
    yr = R.conv1d(x, c.w, c.bias, dil=3, pad=c.pad, pre_slope=c.pre, act=c.act, res=kw["res"], alpha=0.5,
                  lens=c.lens)
    return float((y - yr).norm() / yr.norm())


def test_old_criterion_accepts():
    """The reason for this file: faults the per-element checks reject pass the
    norm ratio of the older test (dense operands: what lies around a row is
    more rows of the same kind), and its 400 LSB for PCM16."""
    assert old_ratio({}) < 1e-2
    ratios = {name: old_ratio(mut) for name, mut in OLD_MUTANTS.items()}
    for name, r in ratios.items():
        print(f"conv-exact old criterion {name}: {r:.5f} (accepts below 1e-2)")
    for name in OLD_ACCEPTS:
        assert ratios[name] < 1e-2, (name, ratios[name])
    # (j) for PCM16: a sample off by more than its bound is far inside 400 LSB
    c = rand_case("lds64-c64", 1, "tanh", 0.01, True)
    ref, bound, _ = c.ref64
    at = _bump_at(-ref.abs(), c.past_lens())
    n = int(math.ceil(2 * float(bound[at]))) + 1
    rep = run_case(c, mutant(bump=(*at, n)), fills=("cont",))
    assert rep.in_view(rep.bad()).nonzero().tolist() == [list(at)]
    off = float((rep.in_view(rep.after["cont"]).double() - ref.round()).abs().max())
    print(f"conv-exact old criterion j-pcm16: {off:.0f} LSB off, bound {float(bound[at]):.2f} (accepts up to 400)")
    assert off <= 400
