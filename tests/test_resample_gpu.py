"""The resampling kernels (``csrc/kernels/resample.hip``) on the GPU against the
fp64 reference, per element, and through the STT / TTS engines.

The f32 limit is derived from the filter, not measured: an output is a chain of
T fmas over terms bounded by ``S = max over phases of sum|h|`` (full-scale
input, in units of 32768 / 32767 after the 1 / 32767 scale), each rounding
within 2^-24 of that bound, plus the table's own rounding to f32, the scale
multiply and its constant: ``(T + 4) * 2^-24 * S * 32768 / 32767``."""
import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

LD = 2048
INGEST = [(r, 16000) for r in ref.RESAMPLE_RATES if r != 16000]
REPLY = [(22050, 16000), (22050, 48000), (16000, 8000), (16000, 22050)]
SCALE = float(np.float32(1.0 / 32767.0))


def _limit(rate_in, rate_out):
    tab, _, _, T = ref.resample_filter(rate_in, rate_out)
    return (T + 4) * 2.0 ** -24 * float(np.abs(tab).sum(1).max()) * 32768 / 32767


def _pcm(rng, n):
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    x[rng.integers(0, max(n, 1), n // 8)] = 32767          # full scale, both signs
    x[rng.integers(0, max(n, 1), n // 8)] = -32768
    if n >= 3:
        x[:3] = (32767, -32767, -32768)
    return x


def _rows(lens, rate_in, rate_out, ld=LD):
    """Every ``ld``-output window of utterances of ``lens`` samples laid end
    to end, as descriptor rows."""
    rows, o = [], 0
    for n in lens:
        n_out = ref.resample_len(n, rate_in, rate_out)
        for w in range(max(1, -(-n_out // ld))):
            rows.append((o, n, w * ld, max(0, min(ld, n_out - w * ld)), rate_in))
        o += n
    return rows


@pytest.mark.parametrize("rate_in,rate_out", INGEST + REPLY)
def test_padded_kernel_against_fp64(rate_in, rate_out):
    T = ref.resample_filter(rate_in, rate_out)[3]
    lens = [0, 1, 5, T - 1, 300, 5000]
    rng = np.random.default_rng(rate_in + rate_out)
    xs = [_pcm(rng, n) for n in lens]
    rows = _rows(lens, rate_in, rate_out)
    pcm = torch.from_numpy(np.concatenate(xs)).cuda()
    got, ss = ops.pcm16_resample_padded(pcm, rows, LD, rate_out)
    assert got.shape == (len(rows), LD) and got.dtype == torch.float32 and ss.shape == (len(rows),)
    g, s = got.cpu().numpy(), ss.cpu().numpy()
    lim = _limit(rate_in, rate_out)
    i = 0
    for u, n in enumerate(lens):
        n_out = ref.resample_len(n, rate_in, rate_out)
        y = ref.resample(xs[u].astype(np.float64), rate_in, rate_out) * SCALE
        for w in range(max(1, -(-n_out // LD))):
            cnt = max(0, min(LD, n_out - w * LD))
            want = y[w * LD:w * LD + cnt]
            err = float(np.abs(g[i, :cnt] - want).max()) if cnt else 0.0
            print(f"{rate_in}->{rate_out} n={n} window={w} err={err:.3e} limit={lim:.3e}")
            assert err <= lim
            assert not g[i, cnt:].any() and not np.signbit(g[i, cnt:]).any()
            s64 = float((want ** 2).sum())
            assert abs(float(s[i]) - s64) <= 1e-5 * s64
            i += 1
    assert i == len(rows)
    # repeatability: no atomics on the output path
    again, _ = ops.pcm16_resample_padded(pcm, rows, LD, rate_out)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_16k_rows_are_the_plain_convert_bitwise():
    """A mixed batch: the 16 kHz rows are ``pcm16_to_f32_padded``'s bits (every
    int16 value among them), the 44.1 kHz row is within its limit."""
    rng = np.random.default_rng(5)
    every = np.arange(-32768, 32768).astype(np.int16)
    a, b, c = every[:3000], _pcm(rng, 4410), every[3000:]
    cs = [c[i:i + LD] for i in range(0, c.size, LD)]
    segs = [a[:LD], a[LD:], b] + cs
    rates = [16000, 16000, 44100] + [16000] * len(cs)
    pcm = torch.from_numpy(np.concatenate(segs)).cuda()
    offs = np.concatenate([[0], np.cumsum([s.size for s in segs])])
    rows = [(int(o), s.size, 0, ref.resample_len(s.size, r, 16000), r)
            for o, s, r in zip(offs, segs, rates)]
    got, ss = ops.pcm16_resample_padded(pcm, rows, LD)
    k = [i for i, r in enumerate(rates) if r == 16000]
    p16 = torch.from_numpy(np.concatenate([segs[i] for i in k])).cuda()
    o16 = torch.from_numpy(np.concatenate([[0], np.cumsum([segs[i].size for i in k])])).cuda()
    want, wss = ops.pcm16_to_f32_padded(p16, o16, LD)
    assert torch.equal(got[k].view(torch.int32), want.view(torch.int32))
    assert torch.allclose(ss[k], wss, rtol=1e-5, atol=0)
    y = ref.resample(b.astype(np.float64), 44100, 16000) * SCALE
    assert np.abs(got[2, :y.size].cpu().numpy() - y).max() <= _limit(44100, 16000)


def test_window_boundary_bitwise():
    """Three rows cut from one 48 kHz utterance are the single-row resample."""
    rng = np.random.default_rng(6)
    n = 3 * LD * 3 - 100                       # 3 windows, the last one short
    pcm = torch.from_numpy(_pcm(rng, n)).cuda()
    n_out = ref.resample_len(n, 48000, 16000)
    assert 2 * LD < n_out < 3 * LD
    whole, wss = ops.pcm16_resample_padded(pcm, [(0, n, 0, n_out, 48000)], 8192)
    rows = _rows([n], 48000, 16000)
    cut, ss = ops.pcm16_resample_padded(pcm, rows, LD)
    assert len(rows) == 3
    assert torch.equal(cut.reshape(-1)[:n_out].view(torch.int32), whole[0, :n_out].view(torch.int32))
    assert not cut.reshape(-1)[n_out:].any() and not whole[0, n_out:].any()
    assert ss.sum().item() == pytest.approx(wss.item(), rel=1e-5)


def test_64bit_output_index():
    """One row far into a long 44.1 kHz utterance: n * M = 4.19e9 does not fit
    a signed 32-bit integer (nor, a little further, an unsigned one)."""
    first, rate = 9_500_000, 44100
    _, L, M, T = ref.resample_filter(rate, 16000)
    assert first * M > 2 ** 31
    n = 26_200_000
    assert ref.resample_len(n, rate, 16000) >= first + LD
    rng = np.random.default_rng(7)
    x = rng.integers(-32768, 32768, n, dtype=np.int16)
    got, ss = ops.pcm16_resample_padded(torch.from_numpy(x).cuda(), [(0, n, first, LD, rate)], LD)
    want = ref.resample(x, rate, 16000, first, LD) * SCALE      # this row only
    err = np.abs(got[0].cpu().numpy() - want).max()
    print(f"row at output {first}: err={err:.3e} limit={_limit(rate, 16000):.3e}")
    assert err <= _limit(rate, 16000)
    s64 = float((want ** 2).sum())
    assert abs(float(ss[0]) - s64) <= 1e-5 * s64


@pytest.mark.parametrize("rate_in,rate_out", REPLY)
def test_int16_entry_point(rate_in, rate_out):
    tab, L, M, T = ref.resample_filter(rate_in, rate_out)
    lens = [0, 1, 5, T - 1, 300, 5000]
    rng = np.random.default_rng(rate_in * 3 + rate_out)
    N = 5000
    x = np.zeros((len(lens), N), np.int16)
    for b, n in enumerate(lens):
        x[b, :n] = _pcm(rng, n)
        x[b, n:] = 12345                                   # past the length: never read
    for dt in (torch.int32, torch.int64):
        n_dev = torch.tensor(lens, dtype=dt, device="cuda")
        out, n_out = ops.pcm16_resample(torch.from_numpy(x).cuda(), n_dev, rate_in, rate_out)
        assert out.dtype == torch.int16 and n_out.dtype == torch.int32 and n_out.is_cuda
        assert out.shape == (len(lens), -(-N * L // M))
        assert n_out.tolist() == [-(-n * L // M) for n in lens]
        g = out.cpu().numpy().astype(np.int64)
        tol = _limit(rate_in, rate_out) * 32767
        for b, n in enumerate(lens):
            y = ref.resample(x[b, :n].astype(np.float64), rate_in, rate_out)
            r = np.clip(np.rint(y), -32768, 32767).astype(np.int64)
            d = np.abs(g[b, :y.size] - r)
            assert d.max(initial=0) <= 1
            clear = np.abs(np.abs(y - np.floor(y)) - 0.5) > tol      # away from a rounding tie
            assert not d[clear].any(), (n, int(d[clear].max()))
            print(f"{rate_in}->{rate_out} n={n}: {int((d != 0).sum())} of {y.size} differ by 1, "
                  f"{int(clear.sum())} clear of a tie")
            assert not g[b, y.size:].any()
    again, _ = ops.pcm16_resample(torch.from_numpy(x).cuda(), n_dev, rate_in, rate_out)
    assert torch.equal(again, out)


def test_int16_saturates():
    sq = np.where(np.arange(4000) % 40 < 20, 32767, -32768).astype(np.int16)[None]
    out, n = ops.pcm16_resample(torch.from_numpy(sq).cuda(), torch.tensor([4000], device="cuda"),
                                16000, 48000)
    y = ref.resample(sq[0].astype(np.float64), 16000, 48000)
    assert y.max() > 32767 + 100 and y.min() < -32768 - 100        # it would wrap
    g = out[0].cpu().numpy().astype(np.int64)
    assert n.tolist() == [12000] and g.max() == 32767 and g.min() == -32768
    assert np.abs(g - np.clip(np.rint(y), -32768, 32767)).max() <= 1


# -------------------------------------------------------------------- engines
def test_stt_upload_resamples_staged_slots(monkeypatch):
    """A 44.1 kHz relay's pinned slot (one slot, and a chain of two), with and
    without stream-in, beside a 16 kHz request: the GPU engine's rows are the
    CPU engine's within the limit."""
    from loqa_hub_amd.engine import stt_engine
    from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
    from loqa_hub_amd.models.configs import whisper_config
    cfg = whisper_config("whisper-tiny")
    rng = np.random.default_rng(8)
    short, chained = _pcm(rng, 44100 + 123), _pcm(rng, 480000 + 4411)
    other = _pcm(rng, 5000)
    cpu = STTEngine(cfg, "cpu", max_batch=4)
    reqs = [STTRequest(short, sample_rate=44100), STTRequest(chained, sample_rate=44100),
            STTRequest(other)]
    want, wss = cpu.upload(reqs)
    want = want.numpy()
    lim = _limit(44100, 16000)
    eng = STTEngine(cfg, "cuda", max_batch=4, use_graphs=False)
    for stream_in in (True, False):
        monkeypatch.setattr(stt_engine, "PCM_STREAM_IN", stream_in)
        if getattr(eng, "stager", None) is not None:
            eng.stager.close()
        eng.stager = None                       # the next slot builds a stager in this mode
        staged = []
        for x in (short, chained):
            slot = eng.new_pcm_slot()
            slot.rate = 44100
            b = x.tobytes()
            for i in range(0, len(b), 8820):                 # 100 ms chunks
                slot.append(b[i:i + 8820])
            staged.append(slot)
        assert eng.stager.stream_in == stream_in
        assert len(staged[0].slots) == 1 and len(staged[1].slots) == 2
        rg = [STTRequest(np.zeros(0, np.int16), staged=staged[0], sample_rate=44100),
              STTRequest(np.zeros(0, np.int16), staged=staged[1], sample_rate=44100),
              STTRequest(other)]
        assert eng.rows_needed(rg) == 3
        got, ss = eng.upload(rg)
        torch.cuda.synchronize()
        assert [r.n_samples for r in rg] == [r.n_samples for r in reqs]
        assert [r.windows for r in rg] == [1, 1, 1] and got.shape == (3, N_SAMPLES)
        g = got.cpu().numpy()
        for i, r in enumerate(rg):
            err = np.abs(g[i] - want[i]).max()
            print(f"stream_in={stream_in} row {i}: err={err:.3e} limit={lim:.3e}")
            assert err <= (lim if i < 2 else 0.0)
            assert not g[i, r.n_samples:].any()
        assert torch.allclose(ss.cpu(), wss, rtol=1e-5, atol=0)
        assert all(s.released for s in staged)


def test_tts_engine_resamples_on_device(monkeypatch):
    """``VitsTTSEngine(sample_rate=16000)`` with graphs: what it returns is the
    CPU resample of the native PCM it synthesized, within 1 LSB."""
    from loqa_hub_amd.engine import tts_engine
    from loqa_hub_amd.models.configs import VITS_CONFIGS
    e = tts_engine.VitsTTSEngine(VITS_CONFIGS["test-vits"], "cuda", sample_rate=16000)
    assert e.use_graphs and e.sample_rate == 16000 and e.cfg.sample_rate == 22050
    seen = []
    real = ops.pcm16_resample

    def spy(pcm, n, rate_in, rate_out):
        assert pcm.is_cuda and n.is_cuda and (rate_in, rate_out) == (22050, 16000)
        seen.append((pcm.cpu().numpy().copy(), n.cpu().numpy().copy()))
        return real(pcm, n, rate_in, rate_out)
    monkeypatch.setattr(tts_engine.ops, "pcm16_resample", spy)
    for texts in (["Turning on the lights."], ["Turning on the lights.", "Hi!"]):
        outs = e.synthesize_batch(texts)
        native, n = seen[-1]
        assert e._runner is not None and e._runner.stats["replays"] > 0
        for b, o in enumerate(outs):
            x = native[b, :int(n[b])]
            want = np.clip(np.rint(ref.resample(x.astype(np.float64), 22050, 16000)), -32768, 32767)
            assert o.dtype == np.int16 and o.size == -(-x.size * 320 // 441) > 0
            assert np.abs(o.astype(np.int64) - want.astype(np.int64)).max() <= 1
            assert np.abs(o.astype(np.float64)).mean() > 10
