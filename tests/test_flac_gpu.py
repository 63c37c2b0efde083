"""The FLAC encoder kernels (``csrc/kernels/flac.hip``) on the GPU: their bytes
are the host model's (``ref.flac_encode``) byte for byte - every decision of
the encoder is integer arithmetic, so there is no tolerance - and nothing
outside a row's samples is read, nothing beyond a stream's length written."""
import asyncio

import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

RATE = 22050
LONG = 129 * 256 + 3            # a two-byte frame number at 256 samples a frame


def _tone(rng, n):
    t = np.arange(n)
    x = 9000 * np.sin(t * 0.05) * np.exp(-2.0 * t / max(n, 1)) + rng.normal(0, 200, n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _rows_256():
    """(samples, ...) of the rows of the 256-sample launch: every length at
    which the kernel takes another path, every kind of content."""
    rng = np.random.default_rng(11)
    rows = [_tone(rng, n) for n in (0, 1, 15, 255, 256, 257, 1124, LONG)]
    rows.append(np.full(1124, -1234, np.int16))                       # CONSTANT frames
    rows.append(np.full(257, 7, np.int16))
    z = _tone(rng, 1124)
    z[200:700] = 0                                                    # a zero stretch
    rows.append(z)
    rows.append(np.tile(np.array([-32768, 32767], np.int16), 562))    # VERBATIM frames
    rows.append(np.tile(np.array([-32768, 32767], np.int16), 128))
    spike = np.zeros(255, np.int16)                                   # one unary run of 468 zeros
    spike[100] = 30000
    rows.append(spike)
    quiet = rng.integers(-40, 41, 1124).astype(np.int16)
    quiet[[5, 300, 301, 777]] = (-32768, 32767, -32768, 32767)
    rows.append(quiet)
    rows.append(rng.integers(-32768, 32768, 600).astype(np.int16))    # full-scale noise
    return rows


def _hostile(rows, N, ld, shift, seed=1):
    """The rows as views into a buffer of random int16: row stride ``ld`` > N,
    the first row ``shift`` samples into the buffer, garbage beyond each row's
    length. Returns (int16 [R, N] view on the GPU, lengths)."""
    rng = np.random.default_rng(seed)
    buf = rng.integers(-32768, 32768, shift + len(rows) * ld + 64).astype(np.int16)
    for b, x in enumerate(rows):
        buf[shift + b * ld: shift + b * ld + len(x)] = x
    dev = torch.from_numpy(buf).cuda()
    view = dev[shift: shift + len(rows) * ld].view(len(rows), ld)[:, :N]
    return view, [len(x) for x in rows]


@pytest.fixture(scope="module")
def case_256():
    rows = _rows_256()
    return rows, ref.flac_encode(*_dense(rows, LONG), RATE, 256)


def _dense(rows, N):
    x = np.zeros((len(rows), N), np.int16)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, [len(r) for r in rows]


def _check(out, out_len, want, cap):
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    assert out.shape == (len(want), cap) and out_len.dtype == np.int32
    for b, w in enumerate(want):
        got = out[b, :out_len[b]].tobytes()
        assert out_len[b] == len(w), (b, int(out_len[b]), len(w))
        if got != w:
            first = next(i for i in range(len(w)) if got[i] != w[i])
            raise AssertionError(f"row {b}: first differing byte {first} of {len(w)}: "
                                 f"{got[first:first + 8].hex()} != {w[first:first + 8].hex()}")
        assert (out[b, out_len[b]:] == 0xFF).all(), f"row {b}: bytes written beyond its stream"


@pytest.mark.parametrize("lens_dtype", [torch.int32, torch.int64])
def test_bytes_equal_the_host_model_256(case_256, lens_dtype):
    rows, want = case_256
    assert ref.flac_frame_plan(rows[13].astype(np.int64)) == ("fixed", 0, 0, [7])
    pcm, lens = _hostile(rows, LONG, LONG + 37, shift=5)
    lens = torch.tensor(lens, dtype=lens_dtype, device="cuda")
    cap = ref.flac_capacity(LONG, 256)
    out = torch.full((len(rows), cap), 0xFF, dtype=torch.uint8, device="cuda")
    got, out_len = ops.flac_encode(pcm, lens, RATE, 256, out=out)
    assert got is out
    _check(out, out_len, want, cap)
    first = out.clone()
    again, again_len = ops.flac_encode(pcm, lens, RATE, 256, out=out)   # a second launch
    assert torch.equal(again, first) and torch.equal(again_len, out_len)
    # the streams decode to the rows (the long one: 130 frames, checked numbers)
    x, rate = ref.flac_decode(out[7, :out_len[7]].cpu().numpy().tobytes())
    assert rate == RATE and np.array_equal(x[0], rows[7])


def test_shifted_rows_same_bytes(case_256):
    """The same samples at another place of another hostile buffer: the bytes
    do not change, so nothing outside a row's samples is read."""
    rows, want = case_256
    cap = ref.flac_capacity(LONG, 256)
    for shift, ld, seed in ((0, LONG + 1, 2), (33, LONG + 200, 3)):
        pcm, lens = _hostile(rows, LONG, ld, shift, seed)
        out = torch.full((len(rows), cap), 0xFF, dtype=torch.uint8, device="cuda")
        _, out_len = ops.flac_encode(pcm, torch.tensor(lens, dtype=torch.int32, device="cuda"),
                                     RATE, 256, out=out)
        _check(out, out_len, want, cap)


@pytest.mark.parametrize("rate", [16000, 11025])
def test_bytes_equal_the_host_model_4096(rate):
    """Full and one-sample-short-of-two frames of 4096, a length clamped to N,
    and a rate that is written out in the frame header (11025)."""
    rng = np.random.default_rng(4)
    loud = _tone(rng, 8192)
    loud[5000:5600] = rng.integers(-32768, 32768, 600)
    rows = [_tone(rng, 4097), loud, np.full(8192, 3, np.int16)]
    want = ref.flac_encode(*_dense(rows, 8192), rate, 4096)
    pcm, lens = _hostile(rows, 8192, 8192 + 8, shift=1)
    lens[2] = 9000                                    # clamped to N = 8192
    cap = ref.flac_capacity(8192, 4096)
    out = torch.full((3, cap), 0xFF, dtype=torch.uint8, device="cuda")
    _, out_len = ops.flac_encode(pcm, torch.tensor(lens, dtype=torch.int32, device="cuda"),
                                 rate, 4096, out=out)
    _check(out, out_len, want, cap)
    for block in (512, 1024, 2048):                   # the other frame sizes, no sentinel
        got, got_len = ops.flac_encode(pcm, torch.tensor(lens, dtype=torch.int32, device="cuda"),
                                       rate, block)
        want_b = ref.flac_encode(*_dense(rows, 8192), rate, block)
        got, got_len = got.cpu().numpy(), got_len.cpu().numpy()
        assert [got[b, :got_len[b]].tobytes() for b in range(3)] == want_b


def test_rejections():
    pcm = torch.zeros(2, 512, dtype=torch.int16, device="cuda")
    lens = torch.tensor([512, 100], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.flac_encode(pcm[:, ::2], lens, RATE, 256)
    with pytest.raises(ValueError, match="block size"):
        ops.flac_encode(pcm, lens, RATE, 300)
    with pytest.raises(ValueError, match="unsupported sample rate"):
        ops.flac_encode(pcm, lens, 44000, 256)
    with pytest.raises(ValueError, match="FLAC frames"):
        ops.flac_encode(pcm[:1, :1].expand(1, 65537 * 256), lens[:1], RATE, 256)
    # the entry point itself refuses what the wrapper cannot even express
    from loqa_hub_amd.ops._lib import kernels, ptr, stream_ptr
    cap = ref.flac_capacity(512, 256)
    out = torch.full((2, cap), 0xFF, dtype=torch.uint8, device="cuda")
    n_out = torch.zeros(2, dtype=torch.int32, device="cuda")
    work = torch.zeros(2 * 2 * 528 + 64, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(2, 4, dtype=torch.int32, device="cuda")

    def call(N=512, ld=512, rate=RATE, block=256, cap=cap):
        return kernels().loqa_flac_encode(ptr(pcm), ld, N, ptr(lens), 0, 2, rate, block, ptr(out),
                                          cap, ptr(n_out), ptr(work), ptr(sizes[0]), ptr(sizes[1]),
                                          stream_ptr(pcm))
    assert call(N=-1) != 0 and call(ld=511) != 0 and call(rate=44000) != 0
    assert call(block=300) != 0 and call(cap=cap - 1) != 0
    torch.cuda.synchronize()
    assert (out == 0xFF).all() and not n_out.any()     # refused before any launch
    assert call() == 0


@pytest.mark.parametrize("sample_rate", [0, 16000])
def test_engine_flac_reply_gpu(sample_rate):
    """With graphs on: the FLAC reply decodes to the PCM reply of an engine with
    the same seed, at the voice's rate and resampled; a batch of one ``wav`` and
    one ``flac`` request answers each in its own container."""
    from loqa_hub_amd.engine.tts_engine import VitsTTSEngine, wav_info
    from loqa_hub_amd.llm.tts import TTSOptions
    from loqa_hub_amd.models.configs import VITS_CONFIGS
    cfg = VITS_CONFIGS["test-vits"]
    rate = sample_rate or cfg.sample_rate
    a = VitsTTSEngine(cfg, "cuda", seed=3, sample_rate=sample_rate)
    b = VitsTTSEngine(cfg, "cuda", seed=3, sample_rate=sample_rate, flac_block=1024)
    assert a.use_graphs and b.use_graphs
    text = "Turning on the kitchen lights."
    p = asyncio.run(a.synthesize(text, TTSOptions(response_format="pcm")))
    f = asyncio.run(b.synthesize(text, TTSOptions(response_format="flac")))
    assert (f.format, f.content_type, f.sample_rate) == ("flac", "audio/flac", rate)
    assert f.length == len(f.audio)
    x, r = ref.flac_decode(f.audio)
    assert r == rate and len(p.audio) > 2000
    assert x[0].astype("<i2").tobytes() == p.audio
    print(f"rate {rate}: flac {len(f.audio)} bytes, pcm {len(p.audio)} bytes, "
          f"ratio {len(f.audio) / (len(p.audio) + 44):.3f}")

    async def batch(e, formats):
        return await asyncio.gather(*[e.synthesize("hello there", TTSOptions(response_format=k))
                                      for k in formats])
    want = asyncio.run(batch(a, ("pcm", "pcm")))
    w, f2 = asyncio.run(batch(b, ("wav", "flac")))
    assert (w.format, f2.format) == ("wav", "flac") and wav_info(w.audio)[0] == rate
    assert w.audio[44:] == want[0].audio
    assert ref.flac_decode(f2.audio)[0][0].astype("<i2").tobytes() == want[1].audio
    assert b.stats["flac_phrases"] == 2 and b.stats["format_downgrades"] == 0
    assert b._runner is not None and b._runner.stats["replays"] > 0
