"""Sample-rate conversion without a GPU: the shared filter design and its fp64
reference (``ops/reference.py``), the CPU entry points, the rate's way through
the STT engine, the audio service (``HUB_AUDIO_INPUT_RATE``) and the reply voice
(``HUB_TTS_SAMPLE_RATE``), and the two configuration keys."""
import asyncio
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref

RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
INGEST = tuple(r for r in RATES if r != 16000)


def _tone(freq, rate, seconds=0.25):
    return np.sin(2 * np.pi * freq * np.arange(int(seconds * rate)) / rate)


# ------------------------------------------------------------- filter design
def test_rates_and_table_shapes():
    assert ref.RESAMPLE_RATES == RATES == ops.RESAMPLE_RATES
    for r in INGEST:
        tab, L, M, T = ref.resample_filter(r, 16000)
        g = math.gcd(r, 16000)
        c = 0.945 * min(1.0, 16000 / r)
        assert (L, M) == (16000 // g, r // g) and T == 2 * math.ceil(32 / c) + 1
        assert tab.shape == (L, T) and tab.dtype == np.float64
        s = np.abs(tab).sum(1).max()
        assert 2.0 < s < 2.4, (r, s)          # no per-phase renormalisation
    assert ref.resample_filter(48000, 16000)[3] == 205
    assert ref.resample_filter(8000, 16000)[3] == 69
    assert ref.resample_filter(11025, 16000)[0].shape == (640, 69)
    tab, L, M, T = ref.resample_filter(16000, 16000)
    assert (L, M, T) == (1, 1, 1) and tab.tolist() == [[1.0]]
    for bad in (7000, 0, 96000):
        with pytest.raises(ValueError, match="unsupported sample rate"):
            ref.resample_filter(bad, 16000)
        with pytest.raises(ValueError, match="unsupported sample rate"):
            ops.resample_filter(16000, bad)
    t32, L, M, T = ops.resample_filter(44100, 16000)
    assert t32.dtype == torch.float32 and t32.shape == (L, T) == (160, 189)
    assert np.array_equal(t32.numpy(), ref.resample_filter(44100, 16000)[0].astype(np.float32))
    assert ops.resample_filter(44100, 16000)[0] is t32          # cached


@pytest.mark.parametrize("rate", INGEST)
def test_passband(rate):
    """Tones of amplitude 1 come out as the analytic 16 kHz tone (limit 1e-5,
    measured <= 9.8e-7), first and last 200 outputs aside."""
    for f in (1000, 2500, 3300):
        y = ref.resample(_tone(f, rate), rate, 16000)
        want = np.sin(2 * np.pi * f * np.arange(y.size) / 16000)
        err = np.abs(y - want)[200:-200].max()
        print(rate, f, err)
        assert err <= 1e-5


@pytest.mark.parametrize("rate", [r for r in RATES if r >= 22050])
def test_alias_rejection(rate):
    """Tones above the 16 kHz Nyquist leave at most -100 dB (measured <= -121)."""
    for f in (9000, min(9500, 0.45 * rate)):
        y = ref.resample(_tone(f, rate), rate, 16000)[200:-200]
        db = 20 * np.log10(np.abs(y).max())
        print(rate, f, db)
        assert db <= -100.0


def test_output_lengths():
    for rate_in, rate_out in [(44100, 16000), (48000, 16000), (8000, 16000), (11025, 16000),
                              (22050, 48000), (16000, 22050), (16000, 16000)]:
        g = math.gcd(rate_in, rate_out)
        L, M = rate_out // g, rate_in // g
        for n in (0, 1, 7, 441, 5000):
            want = -(-n * L // M)
            assert ref.resample_len(n, rate_in, rate_out) == want
            assert ref.resample(np.ones(n), rate_in, rate_out).shape == (want,)
    assert [ref.resample_len(n, 44100, 16000) for n in (0, 1, 7, 441, 5000)] == [0, 1, 3, 160, 1815]


def test_resample_slices_and_definition():
    """``first`` / ``count`` cut the whole signal's outputs; one output against
    the written-out sum."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal(900)
    full = ref.resample(x, 44100, 16000)
    assert np.array_equal(ref.resample(x, 44100, 16000, 100, 57), full[100:157])
    tab, L, M, T = ref.resample_filter(44100, 16000)
    H = (T - 1) // 2
    n = 123
    base, phase = n * M // L, n * M % L
    acc = sum(x[base + k] * tab[phase, k + H] for k in range(-H, H + 1) if 0 <= base + k < x.size)
    assert full[n] == pytest.approx(acc, rel=1e-12, abs=1e-15)


# -------------------------------------------------------- CPU entry points
def _pcm(rng, n):
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    if n >= 3:
        x[:3] = (32767, -32767, -32768)
    return x


def test_padded_16k_row_is_the_plain_convert():
    rng = np.random.default_rng(1)
    a, b = _pcm(rng, 700), _pcm(rng, 300)
    pcm = torch.from_numpy(np.concatenate([a, b]))
    want, wss = ref.pcm16_to_f32_padded(pcm, torch.tensor([0, 700, 1000]), 512)
    for fn in (ref.pcm16_resample_padded, ops.pcm16_resample_padded):
        got, ss = fn(pcm, [(0, 700, 0, 512, 16000), (700, 300, 0, 300, 16000)], 512)
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert torch.equal(ss, wss)
        assert not torch.signbit(got[1, 300:]).any()


def test_padded_rows_cut_equals_whole():
    rng = np.random.default_rng(2)
    x = _pcm(rng, 6000)
    pcm = torch.from_numpy(np.concatenate([np.zeros(10, np.int16), x]))
    n_out = ref.resample_len(6000, 48000, 16000)
    assert n_out == 2000
    whole, _ = ops.pcm16_resample_padded(pcm, [(10, 6000, 0, n_out, 48000)], 2048)
    y = ref.resample(x.astype(np.float64), 48000, 16000) * float(np.float32(1 / 32767))
    assert np.array_equal(whole[0, :n_out].numpy(), y.astype(np.float32))
    assert not whole[0, n_out:].any()
    rows = [(10, 6000, w * 768, min(768, n_out - w * 768), 48000) for w in range(3)]
    cut, ss = ops.pcm16_resample_padded(pcm, rows, 768)
    assert torch.equal(cut.reshape(-1)[:n_out], whole[0, :n_out])
    assert not cut[2, n_out - 2 * 768:].any()
    assert ss.sum().item() == pytest.approx(float((y ** 2).sum()), rel=1e-6)


def test_padded_rejects_bad_rows():
    pcm = torch.zeros(100, dtype=torch.int16)
    with pytest.raises(ValueError, match="unsupported sample rate 7000"):
        ops.pcm16_resample_padded(pcm, [(0, 100, 0, 10, 7000)], 64)
    with pytest.raises(ValueError, match="outside its utterance"):
        ops.pcm16_resample_padded(pcm, [(50, 100, 0, 10, 48000)], 64)
    with pytest.raises(ValueError, match="outside its utterance"):
        ops.pcm16_resample_padded(pcm, [(0, 90, 20, 20, 48000)], 64)


def test_int16_entry_point_cpu():
    rng = np.random.default_rng(3)
    x = np.stack([_pcm(rng, 882), _pcm(rng, 882)]) // 2
    lens = torch.tensor([882, 441], dtype=torch.int32)
    out, n = ops.pcm16_resample(torch.from_numpy(x), lens, 22050, 16000)
    assert out.dtype == torch.int16 and out.shape == (2, 640) and n.tolist() == [640, 320]
    y = np.rint(ref.resample(x[1, :441].astype(np.float64), 22050, 16000))
    assert np.array_equal(out[1, :320].numpy(), y.astype(np.int16)) and not out[1, 320:].any()
    sq = np.where(np.arange(2000) % 40 < 20, 32767, -32768).astype(np.int16)[None]
    out, n = ops.pcm16_resample(torch.from_numpy(sq), torch.tensor([2000]), 16000, 48000)
    y = ref.resample(sq[0].astype(np.float64), 16000, 48000)
    assert y.max() > 32767 and y.min() < -32768           # the filter overshoots the edges
    assert n.tolist() == [6000] and out.max() == 32767 and out.min() == -32768
    with pytest.raises(ValueError, match="unsupported sample rate"):
        ops.pcm16_resample(torch.from_numpy(sq), torch.tensor([2000]), 16000, 44000)


# --------------------------------------------------------------- STT engine
def test_stt_upload_mixed_rates_cpu():
    """A 44.1 kHz and a 16 kHz request in one batch: the rows are the
    reference's, windows and ``n_samples`` count 16 kHz samples."""
    from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
    from loqa_hub_amd.models.configs import whisper_config
    eng = STTEngine(whisper_config("test-whisper"), torch.device("cpu"), seed=0, max_batch=4)
    rng = np.random.default_rng(4)
    a, b = _pcm(rng, 44100 + 17), _pcm(rng, 5000)
    ra, rb = STTRequest(a, sample_rate=44100), STTRequest(b)
    assert rb.sample_rate == 16000 and eng.rows_needed([ra, rb]) == 2
    audio, ss = eng.upload([ra, rb])
    n_a = ref.resample_len(a.size, 44100, 16000)
    assert n_a == -(-a.size * 160 // 441)
    assert (ra.n_samples, ra.windows, rb.n_samples, rb.windows) == (n_a, 1, 5000, 1)
    assert audio.shape == (2, N_SAMPLES) and audio.dtype == torch.float32
    want, wss = ref.pcm16_resample_padded(torch.from_numpy(np.concatenate([a, b])),
                                          [(0, a.size, 0, n_a, 44100), (a.size, 5000, 0, 5000, 16000)],
                                          N_SAMPLES)
    assert torch.equal(audio, want) and torch.equal(ss, wss)
    plain, _ = ref.pcm16_to_f32_padded(torch.from_numpy(b), torch.tensor([0, 5000]), N_SAMPLES)
    assert torch.equal(audio[1], plain[0])
    # a 48 kHz utterance of 31 s is two 30 s windows of 16 kHz samples
    c = np.zeros(31 * 48000, np.int16)
    rc = STTRequest(c, sample_rate=48000)
    assert eng.rows_needed([rc]) == 2
    audio, _ = eng.upload([rc])
    assert (rc.n_samples, rc.windows, audio.shape[0]) == (31 * 16000, 2, 2)
    with pytest.raises(ValueError, match="unsupported sample rate 7000"):
        eng.upload([STTRequest(b, sample_rate=7000)])
    # all 16 kHz: the plain convert, as before
    audio, _ = eng.upload([STTRequest(b)])
    assert torch.equal(audio, plain)


def test_pipeline_job_carries_rate():
    from loqa_hub_amd.engine.pipeline import PipelineJob, _stt_request
    assert _stt_request(PipelineJob("r", "q", np.zeros(4, np.int16))).sample_rate == 16000
    j = PipelineJob("r", "q", np.zeros(4, np.int16), ["a", "b"], sample_rate=48000)
    assert _stt_request(j).sample_rate == 48000


def test_pcm_slot_bound_follows_rate():
    from loqa_hub_amd.engine import pcm_staging
    slot = pcm_staging.PCMSlot.__new__(pcm_staging.PCMSlot)
    slot.rate = 16000
    assert slot.max_samples == pcm_staging.MAX_SAMPLES
    slot.rate = 48000
    assert slot.max_samples == int(pcm_staging.MAX_UTTERANCE_S * 48000)


# ------------------------------------------------------------ audio service
class _Slot:
    def __init__(self):
        self.data, self.released, self.rate = bytearray(), False, 16000

    def append(self, data):
        self.data += data

    def release(self):
        self.released = True


class _Processor:
    takes_pcm16 = True

    def __init__(self):
        self.calls, self.slots = [], []

    def new_pcm_slot(self):
        self.slots.append(_Slot())
        return self.slots[-1]

    async def process(self, relay_id, request_id, audio, sample_rate, pcm16=None, pcm_slot=None):
        from loqa_hub_amd.transport.audio_service import UtteranceResult
        self.calls.append((relay_id, sample_rate, len(pcm_slot.data) // 2))
        pcm_slot.release()
        return UtteranceResult(transcription="ok", response_text="ok", intents=["turn_on"],
                               confidence=0.9)


class _Store:
    def __init__(self):
        self.events = []

    def insert(self, ev):
        self.events.append(ev)


class _Ctx:
    def __init__(self):
        self.sent = []

    async def write(self, msg):
        self.sent.append(msg)


async def _stream(relay_id, rates, n=960):
    from loqa_hub_amd.transport.audio_proto import AudioChunk
    data = (np.arange(n) % 2000).astype("<i2").tobytes()
    for i, r in enumerate(rates):
        yield AudioChunk(relay_id=relay_id, audio_data=data, sample_rate=r, is_wake_word=i == 0,
                         is_end_of_speech=i == len(rates) - 1)


def _serve(mode, rates):
    from loqa_hub_amd.transport.audio_service import AudioService
    proc, store, ctx = _Processor(), _Store(), _Ctx()
    kw = {} if mode is None else {"input_rate": mode}
    svc = AudioService(proc, window_duration=0.02, events_store=store, **kw)
    asyncio.run(svc.StreamAudio(_stream("den", rates), ctx))
    return svc, proc, store, ctx


def test_audio_service_relay_rate():
    svc, proc, store, ctx = _serve("relay", [48000, 48000, 48000])
    assert proc.calls == [("den", 48000, 3 * 960)]
    ev = store.events[0]
    assert ev.sample_rate == 48000 and ev.audio_duration == pytest.approx(3 * 960 / 48000)
    assert proc.slots[0].rate == 48000 and ctx.sent[-1].success
    assert svc.stats["rate_changes"] == 0 and svc.stats["unsupported_rate"] == 0
    # 0 means 16 kHz; the first non-zero rate is the stream's
    svc, proc, store, _ = _serve("relay", [0, 0])
    assert proc.calls[0][1] == 16000 and store.events[0].sample_rate == 16000
    svc, proc, store, _ = _serve("relay", [0, 44100, 44100])
    assert proc.calls[0][1] == 44100 and svc.stats["rate_changes"] == 0


def test_audio_service_unsupported_rate_fails_and_frees_the_slot():
    from loqa_hub_amd.transport.audio_service import MSG_STT_FAILED
    svc, proc, store, ctx = _serve("relay", [7000, 7000])
    assert proc.calls == [] and svc.stats["unsupported_rate"] == 1
    assert len(proc.slots) == 1 and proc.slots[0].released
    r = ctx.sent[-1]
    assert not r.success and r.response_text == MSG_STT_FAILED
    ev = store.events[0]
    assert ev.error_message == "unsupported sample rate 7000" and ev.sample_rate == 7000


def test_audio_service_rate_change_is_counted():
    svc, proc, store, _ = _serve("relay", [48000, 16000, 16000, 48000, 44100])
    assert svc.stats["rate_changes"] == 3
    assert proc.calls[0][1] == 48000 and store.events[0].sample_rate == 48000


@pytest.mark.parametrize("mode", [None, "fixed"])
def test_audio_service_fixed_ignores_the_chunk_rate(mode):
    svc, proc, store, _ = _serve(mode, [48000, 7000, 48000])
    assert proc.calls == [("den", 16000, 3 * 960)]
    ev = store.events[0]
    assert ev.sample_rate == 16000 and ev.audio_duration == pytest.approx(3 * 960 / 16000)
    assert svc.stats["rate_changes"] == 0 and svc.stats["unsupported_rate"] == 0
    assert proc.slots[0].rate == 16000
    from loqa_hub_amd.transport.audio_service import AudioService
    with pytest.raises(ValueError):
        AudioService(None, input_rate="auto")


def test_gpu_voice_processor_passes_the_rate_on():
    from loqa_hub_amd.transport.voice_processor import GPUVoiceProcessor

    class Pipe:
        batch_window, max_batch, jobs = 0.0, 1, []

        async def submit(self, j):
            self.jobs.append(j)
            j.stt_failed, j.error = True, "stop here"

    p = GPUVoiceProcessor(Pipe())
    asyncio.run(p.process("den", "q", np.zeros(0, np.float32), 44100, pcm16=np.zeros(8, np.int16)))
    assert Pipe.jobs[-1].sample_rate == 44100


# ---------------------------------------------------------------- reply voice
def test_tts_engine_output_rate_cpu():
    from loqa_hub_amd.engine.tts_engine import VitsTTSEngine, wav_info
    from loqa_hub_amd.llm.tts import TTSOptions
    from loqa_hub_amd.models.configs import VITS_CONFIGS
    cfg = VITS_CONFIGS["test-vits"]
    assert cfg.sample_rate == 22050
    texts = ["Turning on the lights.", "Hi!"]
    native = VitsTTSEngine(cfg, "cpu")
    assert native.sample_rate == 22050
    base = native.synthesize_batch(texts)
    for same in (0, 22050):
        e = VitsTTSEngine(cfg, "cpu", sample_rate=same)
        assert e.sample_rate == 22050
        assert all(np.array_equal(a, b) for a, b in zip(e.synthesize_batch(texts), base))
    e = VitsTTSEngine(cfg, "cpu", sample_rate=16000)
    assert e.sample_rate == 16000
    outs = e.synthesize_batch(texts)
    for o, b in zip(outs, base):
        assert o.dtype == np.int16 and o.size == -(-b.size * 320 // 441)
        want = np.clip(np.rint(ref.resample(b.astype(np.float64), 22050, 16000)), -32768, 32767)
        assert np.abs(o.astype(np.int64) - want.astype(np.int64)).max() <= 1

    async def go():
        w, p = await asyncio.gather(e.synthesize("hello"),
                                    e.synthesize("hello", TTSOptions(response_format="pcm")))
        sr, n = wav_info(w.audio)
        assert sr == 16000 and w.sample_rate == 16000 and p.sample_rate == 16000
        assert n == len(p.audio) // 2
    asyncio.run(go())
    with pytest.raises(ValueError, match="unsupported sample rate 44000"):
        VitsTTSEngine(cfg, "cpu", sample_rate=44000)


# --------------------------------------------------------------------- config
def test_config_keys():
    from loqa_hub_amd import config
    c = config.load({})
    assert c.gpu.audio_input_rate == "fixed" and c.gpu.tts_sample_rate == 0
    assert config.AUDIO_SAMPLE_RATES == RATES
    c = config.load({"HUB_AUDIO_INPUT_RATE": "Relay", "HUB_TTS_SAMPLE_RATE": "48000"})
    assert c.gpu.audio_input_rate == "relay" and c.gpu.tts_sample_rate == 48000
    # relay rates with an external STT are allowed: only its WAV header changes
    c = config.load({"HUB_AUDIO_INPUT_RATE": "relay", "HUB_STT_BACKEND": "http"})
    assert c.gpu.audio_input_rate == "relay"
    for env, msg in (({"HUB_AUDIO_INPUT_RATE": "auto"}, "HUB_AUDIO_INPUT_RATE"),
                     ({"HUB_TTS_SAMPLE_RATE": "44000"}, "HUB_TTS_SAMPLE_RATE"),
                     ({"HUB_TTS_SAMPLE_RATE": "-1"}, "HUB_TTS_SAMPLE_RATE"),
                     ({"HUB_TTS_SAMPLE_RATE": "fast"}, "HUB_TTS_SAMPLE_RATE")):
        with pytest.raises(config.ConfigError, match=msg):
            config.load(env)
