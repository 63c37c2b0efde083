"""The Whisper audio front end (``csrc/kernels/audio.hip``), one element at a
time: both launches of ``loqa_log_mel`` (f32 MFMA STFT + mel + log10 + row
maximum; floor, scale and bf16 store) and ``loqa_im2col_k3``. The older tests
ran one shape each: 2 x 480000 samples under ``max|m - ref| < 0.05`` (more than
ten bf16 ulps of an output in [-1.5, 1.5]), where both grid-stride loops take a
single trip, no row is silent, both rows peak within a fraction of a decade and
only four of 3000 frames touch the reflect pad.

**Operands and guards.** ``audio``, ``window``, both DFT bases, the filterbank,
``work``, ``gmax`` and the bf16 output are each a slice of a larger flat buffer
with 64 guard elements before and after. The guards - for ``audio`` that is
what lies beyond ``n_samples`` of the last row and before the first - are
filled three ways: *cont* (1000), zeros, NaN. ``work`` / ``gmax`` / ``out``
start as the sentinel -7. The C entry point is called through ``ops._lib``
since the wrapper hides ``work`` and ``gmax``; with Whisper's own constants the
wrapper ``ops.log_mel`` must return the launcher's bits. After a launch every
buffer is compared whole (inputs and guards bit for bit) and the three fills
must give equal bits.

**First launch: ``work`` inside a derived interval.** Reference: fp64 numpy on
the identical f32 audio and the identical f32 constants of ``MelConstants``:
reflect pad 200, 400-tap frames at hop 160, DFT bins 0..200, power,
filterbank, ``log10(max(., 1e-10f))``. It agrees with ``ref.log_mel_db`` to
1.1e-5 on these inputs (3e-7 but for the mels 60 dB under the DC peak of the
one-frame sine row; asserted below 1e-4 in ``test_reference_agrees``). With
``u = 2**-24`` and ``A = sum_n |x_n w_n|`` of the frame:

* re and im are each within ``e = c * 400 u A`` of fp64 with **c = 1**: the
  kernel guide states that ``v_mfma_f32_32x32x2_f32`` is bit for bit a
  k-ordered f32 ``fmaf`` chain with one rounding per step and no wider
  accumulator. The kernel runs two chains of at most 208 and 192 steps and
  adds them: ``(208 + 1) u`` of ``sum |x w| |basis| <= A`` in the worst case,
  plus ``u A`` for the f32 rounding of ``x * w``: 210 u A < 400 u A.
* power: ``max(|re| - e, 0)**2 + max(|im| - e, 0)**2 <= pow <= (|re| + e)**2 +
  (|im| + e)**2``; the filterbank is non-negative, so ``mel_lo = (1 - 202 u)
  filt . pow_lo`` and ``mel_hi = (1 + 202 u) filt . pow_hi``. The 202-term sum
  runs as two chains of 101 steps, so 202 u also holds the three roundings of
  ``re * re + im * im``.
* ``work`` must lie in ``[log10(max(mel_lo, 1e-10f)), log10(max(mel_hi,
  1e-10f))]``, widened by the 2 ulp = 4 u relative that
  ``test_argmax_logprob.py`` budgets for the device log.
* ``gmax[b]`` equals the maximum of the stored ``work`` row bit for bit (a
  maximum of stored values does not depend on the order).

The figure reported is the worst ``(work - ref) / (hi - ref)`` or ``(ref -
work) / (ref - lo)``.

Inputs, B = 4 rows: white noise of amplitude 0.1; all zeros (``atomic_max``
only takes its negative branch: ``gmax = log10f(1e-10f)``); a unit impulse at sample 1,
in a second case at sample ``n - 2`` (each lands in the reflect pad a second
time, under another window tap); a 0.3 sine at 440 Hz on a 0.25 DC offset, cut
to zero after a third of the row. ``n_samples`` in {201, 399, 5000, 5123} (1
frame; 2; 31; 32 frames = one tile with a ragged last hop) and 480000 with B =
2 (noise, sine); ``n_mels`` in {80, 128}.

Whisper's filterbank is exactly 0 in column 200 (the last triangle ends at the
Nyquist frequency), so with it a dropped Nyquist bin changes nothing and cannot
be seen. ``filt`` is an argument: the cases ``synth`` run n = 5123 with
``filt[m, k] = (1 + k % 3) / 4`` where ``k % n_mels == m``, which gives every
bin, 200 included, a mel of its own.

``n_samples = 200`` and ``n_mels = 129`` return an error and leave the
sentinel; B = 0 returns 0 and writes nothing.

**Second launch, bitwise.** From the ``work`` and ``gmax`` bits the first
launch stored, the output equals ``bf16((max(work, gmax[b] - 8) + 4) * 0.25)``
computed in f32 on the host, bit for bit. The case ``b6`` (B = 6, 128 mels,
3000 frames, 2,304,000 elements; noise at ``0.5 * 10**(-0.9 b)``) takes the
second trip of the grid-stride loop (8192 x 256 = 2,097,152 per trip) and is
held to the first launch's interval too; rows 0 and 5 differ in ``gmax`` by
more than 1 (asserted: about 9), so a batch-wide maximum shows.

**``ref.log_mel`` against an outside implementation** (CPU,
``test_reference_matches_transformers``): ``WhisperFeatureExtractor`` of
``transformers`` on 30 s of seeded noise, n in {80, 128}: ``mel_filterbank``
equals ``mel_filters.T`` to 9e-10 / 2e-9 and ``log_mel`` equals
``input_features`` to 2e-6 / 1.1e-5 (measured); asserted at four times these.

**im2col, ``torch.equal``.** Both layouts of the model at B = 4, C = 384, L =
3000: channel-major with stride 1 (13,824,000 elements) and channels-last with
stride 2 (6,912,000) pass the grid cap of 16384 x 256 = 4,194,304 and take 4
and 2 trips; L in {1, 2, 7} with stride 2 (B = 2, C = 5) in both layouts.
``cols`` is sentinel filled with guards, ``x`` guarded by the three fills.

**CPU tests that prove the checker.** ``ops.log_mel`` / ``ref.log_mel_db`` on
CPU tensors (``torch.stft``) and a clean f32 numpy candidate that sums the taps
and the bins in REVERSE order pass every case. Each mutant fails, in the
elements it touches:

    (a) the reflect index ``-idx - 1``           frames 0, 1 of the non-silent rows
    (b) the window shifted one tap                every frame with signal
    (c) the Nyquist bin dropped                   ``synth``: mel 200 % n_mels, alone
    (d) taps 384..399 dropped                     every frame with signal
    (e) one maximum for the whole batch           ``gmax`` of all rows but the loudest
    (f) the second trip of launch 2 skipped       ``b6``: elements >= 2,097,152
    (g) a store to frame ``n_frames``             the next row's frame 0 / the guard
    (h) im2col: the trips after the first skipped

**The old criterion** (``max|m - ref.log_mel| < 0.05`` on the bf16 output, a
sine row and a noise row; here 16000 samples), ``test_old_criterion``:

    clean 0.0037   (a) 0.4793   (b) 0.0199   (c) 0.0037   (d) 0.4589
    (e) 0.0037 (both rows peak alike)   (g) 0.0037

It accepts (b), (c), (e) and (g). (a) and (d) were expected to pass it too, as
a reason for this file; that premise is wrong: a maximum over all elements
sees the two frames of (a) as long as the row is not silent there, and (d)
moves every frame. The test asserts the measured side of each. What the old
test could not see at all: the silent row, the second trips, a ragged or
single tile, and (c) with any filterbank whose column 200 is not 0.

Measured on an MI355X (``MEASURED``), worst position over both ``n_mels`` and
both impulse places. Elements held by the 1e-10 floor stand at 0.4024 in every
case: ``log10f(1e-10f)`` comes out one f32 ulp under -10, inside the 2 ulp
budget, and nothing else is in their interval. Above the floor:

    n = 201  0.0520   n = 399  0.0149   n = 5000  0.0309   n = 5123  0.0149
    n = 480000  0.0107   synth  0.0150   b6  0.0097

so the MFMA chains lose a few percent of the worst case ``400 u A`` allows, as
a sum of 400 roundings of mixed sign does. ``gmax``, the second launch and
im2col are bitwise in every case, the three fills give equal buffers and no
guard or sentinel is disturbed. No kernel of ``audio.hip``
needed a fix; its header comment spoke of 256 threads and four waves where the
kernel runs 512 threads and 8 waves, and is corrected.
"""
import functools

import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import _lib
from loqa_hub_amd.ops import reference as R

# worst position of ``work`` inside its interval on an MI355X (1 = at the edge), elements above the
# 1e-10 floor; the elements held by the floor stand at 0.4024 in every case
MEASURED = {"n201": 0.0520, "n399": 0.0149, "n5000": 0.0309, "n5123": 0.0149, "n480000": 0.0107,
            "synth": 0.0150, "b6": 0.0097}

FILLS = ("cont", "zeros", "nan")
_FILLV = {"cont": 1000.0, "zeros": 0.0, "nan": float("nan")}
BF, F32, F64, I16, I32, I64 = (torch.bfloat16, torch.float32, torch.float64, torch.int16, torch.int32,
                               torch.int64)
U = 2.0 ** -24
C_MFMA = 1.0
SENT = -7.0
GUARD = 64
NFFT, HOP, NBINS = 400, 160, 201
FLOOR = np.float64(np.float32(1e-10))
TRIP2 = 8192 * 256
TRIP_IM2COL = 16384 * 256


def _bits(t):
    return t.view({2: I16, 4: I32, 8: I64}[t.element_size()]) if t.is_floating_point() else t


class Buf:
    """``core`` as a view into a flat buffer with guards of ``fv`` around it."""

    def __init__(self, core, fv, dev):
        n = core.numel()
        flat = torch.full((GUARD + n + GUARD,), fv, dtype=core.dtype)
        flat[GUARD:GUARD + n] = core.reshape(-1)
        self.before, self.flat = flat.clone(), flat.to(dev)
        self.spec = (tuple(core.shape), core.contiguous().stride(), GUARD)
        self.v = self.flat.as_strided(*self.spec)

    def of(self, flat):
        return flat.as_strided(*self.spec)

    def unchanged(self):
        return torch.equal(_bits(self.flat.cpu()), _bits(self.before))

    def outside(self, flat):
        """bool over the flat buffer: a guard element that changed."""
        o = _bits(flat) != _bits(self.before)
        self.of(o)[...] = False
        return o


# ------------------------------------------------------------------ inputs
def consts(n_mels, synth=False):
    c = R.MelConstants.create(n_mels)
    if synth:
        k = np.arange(NBINS)
        f = np.zeros((n_mels, NBINS), dtype=np.float32)
        f[k % n_mels, k] = (1 + k % 3) / 4
        c = R.MelConstants(n_mels, c.window, c.cos_basis, c.sin_basis, torch.from_numpy(f))
    return c


def signals(n, imp):
    """The four rows: noise, silence, impulse at ``imp``, sine on DC cut after a third."""
    rs = np.random.RandomState(n % 9973)
    t = np.arange(n) / 16000.0
    x = np.zeros((4, n), dtype=np.float32)
    x[0] = 0.1 * rs.randn(n)
    x[2, imp] = 1.0
    x[3] = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.25) * (np.arange(n) < n // 3)
    return x


def ref64(audio, c, n_frames):
    """fp64 reference and the interval of ``work``: (ref, lo, hi) [B, n_mels, n_frames]."""
    x = audio.astype(np.float64)
    w = c.window.numpy().astype(np.float64)
    cb = c.cos_basis.numpy().astype(np.float64)[:, :NBINS]
    sb = c.sin_basis.numpy().astype(np.float64)[:, :NBINS]
    filt = c.filters.numpy().astype(np.float64)
    assert (filt >= 0).all()
    xp = np.pad(x, ((0, 0), (NFFT // 2, NFFT // 2)), mode="reflect")
    idx = np.arange(n_frames)[:, None] * HOP + np.arange(NFFT)[None, :]
    xw = xp[:, idx] * w
    A = np.abs(xw).sum(-1, keepdims=True)
    re, im = xw @ cb, xw @ sb
    e = C_MFMA * NFFT * U * A
    pw = re ** 2 + im ** 2
    plo = np.maximum(np.abs(re) - e, 0) ** 2 + np.maximum(np.abs(im) - e, 0) ** 2
    phi = (np.abs(re) + e) ** 2 + (np.abs(im) + e) ** 2
    lg = lambda p, s: np.log10(np.maximum((p @ filt.T) * (1 + s * 202 * U), FLOOR)).transpose(0, 2, 1)
    ref, lo, hi = lg(pw, 0), lg(plo, -1), lg(phi, 1)
    return ref, lo - 4 * U * np.abs(lo), hi + 4 * U * np.abs(hi)


class MelCase:
    def __init__(self, kind, n, n_mels, imp=1):
        self.kind, self.n, self.n_mels = kind, n, n_mels
        self.name = f"logmel-{kind}-n{n}-m{n_mels}-imp{imp}"
        self.c = consts(n_mels, kind == "synth")
        if kind == "b6":
            rs = np.random.RandomState(6)
            self.audio = (rs.randn(6, n) * (0.5 * 10.0 ** (-0.9 * np.arange(6)))[:, None]).astype(np.float32)
        elif n == 480000:
            self.audio = signals(n, 1)[[0, 3]]
        else:
            self.audio = signals(n, imp if imp >= 0 else n + imp)
        self.B, self.nf = self.audio.shape[0], n // HOP
        self.ref, self.lo, self.hi = (torch.from_numpy(a) for a in ref64(self.audio, self.c, self.nf))

    def ground(self, fill, dev):
        fv, c = _FILLV[fill], self.c
        shape = (self.B, self.n_mels, self.nf)
        return {"audio": Buf(torch.from_numpy(self.audio), fv, dev), "window": Buf(c.window, fv, dev),
                "cos": Buf(c.cos_basis, fv, dev), "sin": Buf(c.sin_basis, fv, dev),
                "filt": Buf(c.filters, fv, dev), "work": Buf(torch.full(shape, SENT), SENT, dev),
                "gmax": Buf(torch.full((self.B,), SENT), SENT, dev),
                "out": Buf(torch.full(shape, SENT, dtype=BF), SENT, dev)}

    def launch(self, be, g):
        v = {n: b.v for n, b in g.items()}
        return be.log_mel(v["audio"], v["window"], v["cos"], v["sin"], v["filt"], self.n_mels, v["work"],
                          v["gmax"], v["out"], self.nf, self.c if self.kind != "synth" else None)

    def judge(self, g):
        """-> dict of bool masks over the views (``work``, ``gmax``, ``out``),
        ``outside`` (any guard changed) and the worst position in the interval."""
        flat = {n: g[n].flat.cpu() for n in ("work", "gmax", "out")}
        work, gmax, out = (g[n].of(flat[n]) for n in ("work", "gmax", "out"))
        wd = work.double()
        bad_work = ~((self.lo <= wd) & (wd <= self.hi))
        span = torch.where(wd >= self.ref, self.hi - self.ref, self.ref - self.lo)
        pos = ((wd - self.ref).abs() / span.clamp(min=1e-300))
        worst = float(pos[~torch.isnan(wd)].max())
        sig = ~torch.isnan(wd) & (self.lo > float(np.log10(FLOOR)))      # not held by the 1e-10 floor
        worst_sig = float(pos[sig].max()) if bool(sig.any()) else 0.0
        bad_gmax = _bits(gmax) != _bits(work.reshape(self.B, -1).amax(1))
        want = ((torch.maximum(work, gmax[:, None, None] - 8.0) + 4.0) * 0.25).to(BF)
        bad_out = _bits(out) != _bits(want)
        outside = {n: g[n].outside(flat[n]) for n in flat}
        return dict(work=bad_work, gmax=bad_gmax, out=bad_out, outside=outside, worst=worst,
                    worst_sig=worst_sig, flat=flat)


def run(case, be, dev="cpu", fills=FILLS):
    res = {}
    for f in fills:
        g = case.ground(f, dev)
        rc = case.launch(be, g)
        res[f] = case.judge(g)
        res[f]["rc"] = rc
        res[f]["inputs_ok"] = all(g[n].unchanged() for n in ("audio", "window", "cos", "sin", "filt"))
    return res


def check(case, be, dev="cpu", fills=FILLS):
    res = run(case, be, dev, fills)
    print(f"logmel-exact {be.name} {case.name}: worst position in the interval "
          f"{max(r['worst'] for r in res.values()):.4f}, above the floor "
          f"{max(r['worst_sig'] for r in res.values()):.4f}")
    for f, r in res.items():
        assert r["rc"] == 0 and r["inputs_ok"], (case.name, f)
        for n in ("work", "gmax", "out"):
            assert not r["outside"][n].any(), (case.name, f, n, "a guard changed")
            assert not r[n].any(), (case.name, f, n, int(r[n].sum()), "elements wrong, first at",
                                    r[n].nonzero()[:8].tolist())
        for n, fl in r["flat"].items():
            assert torch.equal(_bits(fl), _bits(res["cont"]["flat"][n])), (case.name, f, n, "fills differ")
    return res


# ---------------------------------------------------------------- backends
class Native:
    name = "hip"

    def log_mel(self, audio, window, cosb, sinb, filt, n_mels, work, gmax, out, n_frames, c):
        p = _lib.ptr
        B, n = audio.shape
        rc = _lib.kernels().loqa_log_mel(p(audio), B, n, p(window), p(cosb), p(sinb), p(filt), n_mels,
                                         p(work), p(gmax), p(out), n_frames, _lib.stream_ptr(audio))
        torch.cuda.synchronize()
        if rc == 0 and c is not None:
            assert torch.equal(_bits(ops.log_mel(audio, c)), _bits(out)), "wrapper and launcher differ"
        return rc

    def im2col(self, x, strides, B, C, L, stride, cols):
        rc = _lib.kernels().loqa_im2col_k3(_lib.ptr(x), *strides, B, C, L, stride, _lib.ptr(cols),
                                           _lib.stream_ptr(x))
        torch.cuda.synchronize()
        return rc


class CpuOps:
    """``torch.stft`` in f32: ``ref.log_mel_db`` for ``work``, ``ops.log_mel`` for the output."""
    name = "ops-cpu"

    def log_mel(self, audio, window, cosb, sinb, filt, n_mels, work, gmax, out, n_frames, c):
        c = R.MelConstants(n_mels, window, cosb, sinb, filt)
        work.copy_(R.log_mel_db(audio, c))
        gmax.copy_(work.reshape(work.shape[0], -1).amax(1))
        out.copy_(ops.log_mel(audio, c))
        return 0

    def im2col(self, x, strides, B, C, L, stride, cols):
        cols.copy_(ops.im2col_k3(x, strides, B, C, L, stride))
        return 0


class Sim:
    """Both launches in plain f32 numpy, taps and bins summed in REVERSE order
    (sequentially up to 64 frames), and through ``mut`` their possible faults."""
    name = "sim-fp32"

    def __init__(self, **mut):
        self.mut = mut

    def log_mel(self, audio, window, cosb, sinb, filt, n_mels, work, gmax, out, n_frames, c):
        m, f32 = self.mut, np.float32
        B, n = audio.shape
        if B <= 0:
            return 0
        if n_frames <= 0 or n_mels <= 0 or n_mels > 128 or n <= NFFT // 2:
            return 1
        x, w = audio.numpy(), window.numpy()
        if m.get("window_shift"):
            w = np.roll(w, 1)
        idx = np.arange(n_frames)[:, None] * HOP + np.arange(NFFT)[None, :] - NFFT // 2
        idx = np.where(idx < 0, -idx - (1 if m.get("reflect_m1") else 0), idx)
        idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
        xw = x[:, idx] * w
        taps = 384 if m.get("tail_dropped") else NFFT
        cb, sb = cosb.numpy()[:, :NBINS], sinb.numpy()[:, :NBINS]
        if n_frames <= 64:
            re, im = np.zeros((B, n_frames, NBINS), f32), np.zeros((B, n_frames, NBINS), f32)
            for k in reversed(range(taps)):
                re += xw[..., k, None] * cb[k]
                im += xw[..., k, None] * sb[k]
        else:
            re, im = xw[..., taps - 1::-1] @ cb[taps - 1::-1], xw[..., taps - 1::-1] @ sb[taps - 1::-1]
        pw = re * re + im * im
        if m.get("nyquist_dropped"):
            pw[..., 200] = 0
        fl = filt.numpy()
        if n_frames <= 64:
            mel = np.zeros((B, n_frames, n_mels), f32)
            for k in reversed(range(NBINS)):
                mel += pw[..., k, None] * fl[:, k]
        else:
            mel = pw[..., ::-1] @ fl[:, ::-1].T
        assert mel.dtype == f32
        lg = torch.from_numpy(np.log10(np.maximum(mel, f32(1e-10))).transpose(0, 2, 1).copy())
        work.copy_(lg)
        if m.get("store_past"):       # frame n_frames of the last (b, mel) row
            torch.as_strided(work, (1,), (1,), work.storage_offset() + work.numel())[0] = lg[-1, -1, -1]
        gm = lg.reshape(B, -1).amax(1)
        if m.get("batch_max"):
            gm = gm.max().expand(B).clone()
        gmax.copy_(gm)
        o = ((torch.maximum(lg, gm[:, None, None] - 8.0) + 4.0) * 0.25).to(BF)
        if m.get("trip2_skipped"):
            flat = out.reshape(-1).clone()
            flat[:TRIP2] = o.reshape(-1)[:TRIP2]
            o = flat.view_as(o)
        out.copy_(o)
        return 0

    def im2col(self, x, strides, B, C, L, stride, cols):
        want = R.im2col_k3(x, strides, B, C, L, stride).reshape(-1)
        if self.mut.get("one_trip"):
            want = torch.cat([want[:TRIP_IM2COL], cols.reshape(-1)[TRIP_IM2COL:]])
        cols.copy_(want.view_as(cols))
        return 0


@functools.lru_cache(maxsize=None)
def mel_case(*args):
    return MelCase(*args)


SMALL = [("plain", n, m, imp) for n in (201, 399, 5000, 5123) for m in (80, 128) for imp in (1, -2)]
SYNTH = [("synth", 5123, 80, 1), ("synth", 5123, 128, -2)]
LONG = [("plain", 480000, 80, 1), ("plain", 480000, 128, 1)]
B6 = ("b6", 480000, 128, 1)
_cid = lambda s: "-".join(map(str, s))


# --------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("spec", SMALL + SYNTH + LONG + [B6], ids=_cid)
def test_log_mel_gpu(spec):
    c = mel_case(*spec)
    res = check(c, Native(), "cuda")
    if spec == B6:
        gm = res["cont"]["flat"]["gmax"][GUARD:GUARD + 6]
        assert float(gm[0] - gm[5]) > 1 and c.B * c.n_mels * c.nf > TRIP2
    else:
        # the silent row: log10f(1e-10f), taken by the negative branch of the atomic maximum
        assert abs(float(res["cont"]["flat"]["gmax"][GUARD + 1]) + 10.0) < 2e-6 or c.n == 480000


def _return_codes(be, dev):
    c = consts(80)
    for n, n_mels, B in ((200, 80, 2), (5000, 129, 2), (5000, 80, 0)):
        audio = Buf(torch.zeros(max(B, 1), n) + 0.5, 1000.0, dev)
        filt = Buf(torch.zeros(n_mels, NBINS), 1000.0, dev)
        bufs = [Buf(t, 1000.0, dev) for t in (c.window, c.cos_basis, c.sin_basis)]
        shape = (max(B, 1), n_mels, n // HOP)
        work, gmax, out = Buf(torch.full(shape, SENT), SENT, dev), Buf(torch.full((2,), SENT), SENT, dev), \
            Buf(torch.full(shape, SENT, dtype=BF), SENT, dev)
        a = audio.v[:B] if B else audio.v[:0]
        rc = be.log_mel(a, bufs[0].v, bufs[1].v, bufs[2].v, filt.v, n_mels, work.v, gmax.v, out.v, n // HOP,
                        None)
        assert (rc == 0) == (B == 0), (n, n_mels, B, rc)
        assert work.unchanged() and gmax.unchanged() and out.unchanged(), (n, n_mels, B)


@pytest.mark.gpu
def test_log_mel_return_codes_gpu():
    """``n_samples = 200`` and ``n_mels = 129``: an error, the sentinel stays; B = 0: 0, nothing written."""
    _return_codes(Native(), "cuda")


IM2COL = [("cm", 4, 384, 3000, 1), ("cl", 4, 384, 3000, 2)] + \
         [(lay, 2, 5, L, 2) for lay in ("cm", "cl") for L in (1, 2, 7)]


def check_im2col(spec, be, dev, fills=FILLS):
    lay, B, C, L, stride = spec
    g = torch.Generator().manual_seed(L + C)
    x = torch.randn((B, C, L) if lay == "cm" else (B, L, C), generator=g).to(BF)
    strides = (C * L, L, 1) if lay == "cm" else (L * C, 1, C)
    Lout = (L - 1) // stride + 1
    want = R.im2col_k3(x, strides, B, C, L, stride)
    assert want.shape == (B * Lout, 3 * C)
    bad = {}
    for f in fills:
        xb = Buf(x, _FILLV[f], dev)
        cols = Buf(torch.full((B * Lout, 3 * C), SENT, dtype=BF), SENT, dev)
        assert be.im2col(xb.v, strides, B, C, L, stride, cols.v) == 0
        flat = cols.flat.cpu()
        assert xb.unchanged()
        assert not cols.outside(flat).any(), (spec, f, "a guard of cols changed")
        bad[f] = _bits(cols.of(flat)) != _bits(want)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("spec", IM2COL, ids=_cid)
def test_im2col_gpu(spec):
    for f, bad in check_im2col(spec, Native(), "cuda").items():
        assert not bad.any(), (spec, f, int(bad.sum()), bad.nonzero()[:8].tolist())


# --------------------------------------------------------------- CPU tests
BACKENDS = [CpuOps(), Sim()]


@pytest.mark.parametrize("be", BACKENDS, ids=lambda b: b.name)
@pytest.mark.parametrize("spec", SMALL + SYNTH + LONG[:1], ids=_cid)
def test_checker_passes(spec, be):
    check(mel_case(*spec), be)


def test_checker_passes_b6():
    c = mel_case(*B6)
    res = check(c, Sim(), fills=("cont",))
    gm = res["cont"]["flat"]["gmax"][GUARD:GUARD + 6]
    assert float(gm[0] - gm[5]) > 1


def test_checker_return_codes():
    _return_codes(Sim(), "cpu")


def test_reference_agrees():
    """The fp64 reference and ``ref.log_mel_db`` (torch.stft, f32) agree."""
    for spec in SMALL[::3] + LONG[:1]:
        c = mel_case(*spec)
        got = R.log_mel_db(torch.from_numpy(c.audio), c.c).double()
        assert float((got - c.ref).abs().max()) < 1e-4, spec
    for n in (80, 128):
        assert float(consts(n).filters[:, 200].abs().max()) == 0
    f = consts(80, True).filters
    assert int((f > 0).sum()) == NBINS and float(f[200 % 80, 200]) > 0


def test_reference_matches_transformers():
    """``ref.mel_filterbank`` / ``ref.log_mel`` against WhisperFeatureExtractor
    on 30 s of seeded noise; tolerances four times the measured 9e-10 / 2e-9
    and 2e-6 / 1.1e-5."""
    tf = pytest.importorskip("transformers")
    audio = (0.1 * np.random.RandomState(0).randn(480000)).astype(np.float32)
    for n, tol_f, tol_m in ((80, 4 * 9e-10, 4 * 2e-6), (128, 4 * 2e-9, 4 * 1.1e-5)):
        fe = tf.WhisperFeatureExtractor(feature_size=n)
        theirs = np.asarray(fe.mel_filters, np.float64).T
        df = float(np.abs(R.mel_filterbank(n_mels=n).astype(np.float64) - theirs).max())
        feats = fe(audio, sampling_rate=16000, return_tensors="np").input_features[0]
        mine = R.log_mel(torch.from_numpy(audio)[None], R.MelConstants.create(n))[0].numpy()
        dm = float(np.abs(mine.astype(np.float64) - feats.astype(np.float64)).max())
        print(f"logmel-exact transformers n_mels {n}: filterbank {df:.2e}, log-mel {dm:.2e}")
        assert mine.shape == feats.shape == (n, 3000)
        assert df <= tol_f and dm <= tol_m


def _frames(bad):
    """(b, frame) with a wrong element in a [B, n_mels, n_frames] mask."""
    return {tuple(r) for r in bad.any(1).nonzero().tolist()}


M5123 = ("plain", 5123, 80, 1)


def test_mutant_reflect_window_tail():
    c = mel_case(*M5123)
    loud = {(b, f) for b in (0, 2, 3) for f in range(c.nf)}
    # (a): the left pad is read by frames 0 and 1; the silent row cannot tell
    r = run(c, Sim(reflect_m1=True), fills=("cont",))["cont"]
    assert _frames(r["work"]) == {(b, f) for b in (0, 2, 3) for f in (0, 1)}
    c2 = mel_case("plain", 201, 128, -2)
    assert _frames(run(c2, Sim(reflect_m1=True), fills=("cont",))["cont"]["work"]) == {(0, 0), (2, 0), (3, 0)}
    # (b), (d): every frame that holds signal (the impulse row: the frames that see it)
    for mut in ("window_shift", "tail_dropped"):
        r = run(c, Sim(**{mut: True}), fills=("cont",))["cont"]
        got = _frames(r["work"])
        sig = {(b, f) for (b, f) in loud
               if float(np.abs(c.audio[b, max(0, f * 160 - 200):f * 160 + 200]).max()) > 0}
        assert got <= sig and {(0, f) for f in range(c.nf)} <= got, mut
        assert ((2, 0) in got) == (mut == "window_shift")       # the impulse lies under taps 199 and 201
        assert len(got) >= 0.75 * len(sig), (mut, len(got), len(sig))


def test_mutant_nyquist():
    """(c): seen with the synthetic filterbank, in the mel that holds bin 200
    alone; with Whisper's filterbank column 200 is 0 and nothing changes."""
    for spec in SYNTH:
        c = mel_case(*spec)
        r = run(c, Sim(nyquist_dropped=True), fills=("cont",))["cont"]
        mels = set(r["work"].any(2).any(0).nonzero().flatten().tolist())
        assert mels == {200 % c.n_mels} and not r["outside"]["work"].any()
        assert {b for b, _ in _frames(r["work"])} == {0, 2, 3}
    r = run(mel_case(*M5123), Sim(nyquist_dropped=True), fills=("cont",))["cont"]
    assert not r["work"].any() and not r["out"].any()


def test_mutant_batch_max_trip_and_store():
    c = mel_case(*M5123)
    r = run(c, Sim(batch_max=True), fills=("cont",))["cont"]          # (e)
    loudest = int(c.ref.reshape(4, -1).amax(1).argmax())
    assert set(r["gmax"].nonzero().flatten().tolist()) == {0, 1, 2, 3} - {loudest} and not r["work"].any()
    r = run(c, Sim(store_past=True), fills=("cont",))["cont"]         # (g): the guard after the last row
    assert r["outside"]["work"].nonzero().flatten().tolist() == [GUARD + 4 * 80 * 32]
    c6 = mel_case(*B6)
    r = run(c6, Sim(trip2_skipped=True, batch_max=True), fills=("cont",))["cont"]      # (f) and (e) at once
    bad = r["out"].reshape(-1)
    assert not bad[:TRIP2].any() and bool(bad[TRIP2:].all()) and not r["work"].any()
    # the output is held to the gmax that was stored, so (e) shows in gmax alone
    assert set(r["gmax"].nonzero().flatten().tolist()) == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("be", BACKENDS, ids=lambda b: b.name)
@pytest.mark.parametrize("spec", IM2COL[1:], ids=_cid)
def test_checker_passes_im2col(spec, be):
    for f, bad in check_im2col(spec, be, "cpu").items():
        assert not bad.any(), (spec, f)


def test_mutant_im2col_one_trip():
    """(h): the elements past the first trip keep the sentinel."""
    bad = check_im2col(IM2COL[1], Sim(one_trip=True), "cpu", fills=("cont",))["cont"].reshape(-1)
    assert not bad[:TRIP_IM2COL].any() and bool(bad[TRIP_IM2COL:].all())


def old_criterion():
    n = 16000
    t = np.arange(n) / 16000
    rs = np.random.RandomState(1)
    a = np.stack([0.3 * np.sin(2 * np.pi * 440 * t) * (t < 0.3), 0.1 * rs.randn(n)]).astype(np.float32)
    audio, c = torch.from_numpy(a), consts(80)
    want = R.log_mel(audio, c)
    out = {}
    for name, m in {"clean": {}, "a": dict(reflect_m1=True), "b": dict(window_shift=True),
                    "c": dict(nyquist_dropped=True), "d": dict(tail_dropped=True), "e": dict(batch_max=True),
                    "g": dict(store_past=True)}.items():
        work, gmax = torch.full((2 * 80 * 100 + 1,), SENT), torch.full((2,), SENT)
        o = torch.full((2, 80, 100), SENT, dtype=BF)
        Sim(**m).log_mel(audio, c.window, c.cos_basis, c.sin_basis, c.filters, 80, work[:-1].view(2, 80, 100),
                         gmax, o, 100, None)
        out[name] = float((o.float() - want).abs().max())
    return out


def test_old_criterion():
    """The measured side of each (module docstring): the old bound accepts the
    clean candidate and (b), (c), (e), (g); it rejects (a) and (d)."""
    r = old_criterion()
    for k, v in r.items():
        print(f"logmel-exact old criterion {k}: {v:.4f} (accepts below 0.05)")
    for k in ("clean", "b", "c", "e", "g"):
        assert r[k] < 0.05, k
    assert r["a"] > 0.05 and r["d"] > 0.05
