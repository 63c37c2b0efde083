"""FLAC reply audio on the CPU: the host model of the encoder
(``ops/reference.py`` ``flac_encode``, the arbiter of csrc/kernels/flac.hip), its
independent decoder, the engine's ``flac`` response format and the served hub
with ``TTS_FORMAT=flac``. The kernel itself is held to the model's bytes in
``tests/test_flac_gpu.py``."""
import asyncio
import base64
import hashlib
import os

import numpy as np
import pytest

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd.config import AUDIO_SAMPLE_RATES
from loqa_hub_amd.ops import reference as ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "flac_rfc9639_example1.hex")


def signal(n, seed=0):
    """A decaying tone in Gaussian noise with a stretch of zeros and a stretch
    of full-scale noise (where the row is long enough to hold them)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 9000 * np.sin(t * 0.05) * np.exp(-2.0 * t / max(n, 1)) + rng.normal(0, 200, n)
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    if n >= 300:
        x[n // 3: n // 3 + n // 10] = 0
        x[n // 2: n // 2 + n // 10] = rng.integers(-32768, 32768, n // 10)
    return x


def plans(x, block):
    return [ref.flac_frame_plan(x[f:f + block].astype(np.int64))[0] for f in range(0, len(x), block)]


# ------------------------------------------------------------------- decoder
def test_decoder_known_answer():
    """RFC 9639's first example: two channels, one sample each, both VERBATIM
    with wasted bits; the decoder's CRC checks pass and the samples' MD5 is the
    one STREAMINFO records."""
    data = bytes.fromhex("".join(open(GOLDEN).read().split()))
    assert len(data) == 57
    x, rate = ref.flac_decode(data)
    assert x.dtype == np.int16 and x.tolist() == [[25588], [10416]] and rate == 44100
    assert hashlib.md5(x.T.astype("<i2").tobytes()).digest() == data[26:42]
    assert ref.flac_info(data) == (44100, 1)


def test_decoder_rejects_damage():
    x = signal(700)
    st = ref.flac_encode(x[None], [700], 16000, 256)[0]
    body = bytearray(st)
    body[60] ^= 0x10                               # inside the first frame's residual
    with pytest.raises(ValueError, match="CRC-16"):
        ref.flac_decode(bytes(body))
    head = bytearray(st)
    head[44] ^= 0x01                               # the first frame's header
    with pytest.raises(ValueError, match="CRC-8|not supported|sample rate"):
        ref.flac_decode(bytes(head))
    with pytest.raises(ValueError):
        ref.flac_decode(st + b"\x00")               # the stream must end with its last frame
    with pytest.raises(ValueError):
        ref.flac_decode(st[:-1])


# ---------------------------------------------------------------- round trip
SHAPES = [(22050, 22050, 4096), (16000, 5000, 256), (11025, 777, 1024), (48000, 1, 256),
          (24000, 4097, 4096), (8000, 300, 256), (16000, 0, 256), (12000, 2049, 2048),
          (32000, 1030, 512)]


@pytest.mark.parametrize("rate,n,block", SHAPES)
def test_round_trip(rate, n, block):
    x = signal(n, seed=n)
    st = ref.flac_encode(x[None], [n], rate, block)[0]
    y, r = ref.flac_decode(st)
    assert r == rate and y.shape == (1, n) and np.array_equal(y[0], x)
    assert ref.flac_info(st) == (rate, n)
    assert len(st) <= ref.flac_capacity(n, block)
    if n == 0:
        assert len(st) == 42 and st[12:18] == bytes(6)
    else:
        assert int.from_bytes(st[8:10], "big") == int.from_bytes(st[10:12], "big") == block


@pytest.mark.parametrize("rate", AUDIO_SAMPLE_RATES)
def test_round_trip_every_rate(rate):
    x = signal(333, seed=rate)
    st = ref.flac_encode(x[None], [333], rate, 256)[0]
    y, r = ref.flac_decode(st)
    assert r == rate and np.array_equal(y[0], x) and ref.flac_info(st) == (rate, 333)


def test_rows_and_lengths():
    """Rows of one call are independent streams; lengths are clamped to [0, N]
    and nothing beyond a row's length reaches its stream."""
    x = np.stack([signal(900, 1), signal(900, 2), signal(900, 3)])
    out = ref.flac_encode(x, [900, 5000, -3], 22050, 256)
    assert out[0] == out[1][:0] + ref.flac_encode(x[:1], [900], 22050, 256)[0]
    assert np.array_equal(ref.flac_decode(out[1])[0][0], x[1])
    assert len(out[2]) == 42
    short = ref.flac_encode(x, [500, 500, 500], 22050, 256)
    x[:, 500:] = 77
    assert ref.flac_encode(x, [500, 500, 500], 22050, 256) == short


# -------------------------------------------------------------- derived sizes
def test_constant_frames_size():
    x = np.full(600, -5, np.int16)
    st = ref.flac_encode(x[None], [600], 16000, 256)[0]
    assert plans(x, 256) == ["constant"] * 3
    # header 4 + number 1 + CRC 1, subframe 1 + 2, footer 2 = 11; the short
    # last frame has one more byte for its size
    assert len(st) == 42 + 11 + 11 + 12 == 76
    assert np.array_equal(ref.flac_decode(st)[0][0], x)


def test_verbatim_frames_size():
    x = np.tile(np.array([-32768, 32767], np.int16), 256)
    st = ref.flac_encode(x[None], [512], 16000, 256)[0]
    assert plans(x, 256) == ["verbatim"] * 2
    assert len(st) == 42 + 2 * (6 + 1 + 512 + 2) == 1084
    assert np.array_equal(ref.flac_decode(st)[0][0], x)
    u = np.random.default_rng(5).integers(-32768, 32768, 600).astype(np.int16)
    assert plans(u, 256) == ["verbatim"] * 3
    assert np.array_equal(ref.flac_decode(ref.flac_encode(u[None], [600], 16000, 256)[0])[0][0], u)


def test_plan_of_a_lone_spike():
    x = np.zeros(255, np.int64)
    x[100] = 30000
    assert ref.flac_frame_plan(x) == ("fixed", 0, 0, [7])


# -------------------------------------------------------------- frame numbers
def test_three_byte_frame_numbers():
    n = 2049 * 256 - 100
    x = np.full(n, 1234, np.int16)
    rng = np.random.default_rng(9)
    for f in (0, 127, 128, 2047, 2048):
        x[f * 256: f * 256 + 156] = rng.normal(0, 300, 156).astype(np.int16)
    st = ref.flac_encode(x[None], [n], 16000, 256)[0]
    y, _ = ref.flac_decode(st)                      # it checks the number sequence
    assert np.array_equal(y[0], x)
    # the short last frame: size code 0110, 16 kHz, number 2048 as e0 a0 80, 156 - 1
    assert st.rfind(b"\xff\xf8\x65\x08\xe0\xa0\x80\x9b") > len(st) - 400


def test_too_many_frames_refused():
    with pytest.raises(ValueError, match="65537 FLAC frames"):
        ref.flac_check(65537 * 256, 16000, 256)
    assert ref.flac_check(65536 * 256, 16000, 256) == 65536
    import torch
    from loqa_hub_amd import ops
    big = torch.zeros(1, 1, dtype=torch.int16).expand(1, 65537 * 256)
    with pytest.raises(ValueError, match="65537 FLAC frames"):
        ops.flac_encode(big, torch.tensor([10]), 16000, 256)
    with pytest.raises(ValueError, match="block size"):
        ref.flac_encode(np.zeros((1, 10), np.int16), [10], 16000, 300)
    with pytest.raises(ValueError, match="unsupported sample rate"):
        ref.flac_encode(np.zeros((1, 10), np.int16), [10], 44000, 256)


# --------------------------------------------------------------------- engine
@pytest.mark.parametrize("sample_rate", [0, 16000])
def test_engine_flac_reply_cpu(sample_rate):
    """The FLAC reply decodes to exactly the PCM reply of an engine with the
    same seed, at the voice's rate and resampled."""
    from loqa_hub_amd.engine.tts_engine import VitsTTSEngine
    from loqa_hub_amd.llm.tts import TTSOptions
    from loqa_hub_amd.models.configs import VITS_CONFIGS
    cfg = VITS_CONFIGS["test-vits"]
    rate = sample_rate or cfg.sample_rate
    a = VitsTTSEngine(cfg, "cpu", seed=3, sample_rate=sample_rate)
    b = VitsTTSEngine(cfg, "cpu", seed=3, sample_rate=sample_rate, flac_block=1024)
    text = "Turning on the kitchen lights."
    p = asyncio.run(a.synthesize(text, TTSOptions(response_format="pcm")))
    f = asyncio.run(b.synthesize(text, TTSOptions(response_format="flac")))
    assert (f.format, f.content_type, f.sample_rate) == ("flac", "audio/flac", rate)
    assert f.length == len(f.audio) and f.audio[:4] == b"fLaC"
    x, r = ref.flac_decode(f.audio)
    assert r == rate and x.shape[0] == 1
    assert x[0].astype("<i2").tobytes() == p.audio and len(p.audio) > 2000
    assert int.from_bytes(f.audio[8:10], "big") == 1024
    assert b.stats["format_downgrades"] == 0 and b.stats["flac_phrases"] == 1
    assert a.stats["flac_phrases"] == 0

    async def batch(e, formats):       # one batch of three requests
        return await asyncio.gather(*[e.synthesize("hello there", TTSOptions(response_format=f))
                                      for f in formats])
    want = asyncio.run(batch(a, ("pcm", "pcm", "pcm")))
    w, f2, p2 = asyncio.run(batch(b, ("wav", "flac", "pcm")))
    assert (w.format, f2.format, p2.format) == ("wav", "flac", "pcm")
    assert w.audio[:4] == b"RIFF" and w.audio[44:] == want[0].audio
    assert ref.flac_decode(f2.audio)[0][0].astype("<i2").tobytes() == want[1].audio
    assert p2.audio == want[2].audio and b.stats["flac_phrases"] == 2
    with pytest.raises(ValueError, match="flac_block"):
        VitsTTSEngine(cfg, "cpu", flac_block=300)


# ----------------------------------------------------------------- served hub
def test_config_flac_block():
    assert cfgmod.load({}).gpu.tts_flac_block == 4096
    assert cfgmod.load({"HUB_TTS_FLAC_BLOCK": "1024"}).gpu.tts_flac_block == 1024
    for bad in ("300", "abc", "0"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_TTS_FLAC_BLOCK"):
            cfgmod.load({"HUB_TTS_FLAC_BLOCK": bad})


HINT = "hey loqa turn on the kitchen lights and then play some jazz"


def _serve(tmp_path, streaming: bool):
    """One utterance through a hub with ``TTS_FORMAT=flac`` on the CPU engines,
    in the pattern of ``tests/test_hub_served.py``: (last gRPC message, NATS
    ``audio.<relay>`` messages, the TTS engine's stats)."""
    grpc = pytest.importorskip("grpc")
    import json
    from loqa_hub_amd.messaging.nats_client import NATSClient
    from loqa_hub_amd.server import HubServer, build_gpu_processor, build_tts
    from loqa_hub_amd.transport.audio_proto import AudioChunk, stream_audio_stub
    relay = "kitchen-relay"
    t = np.arange(16000) / 16000.0
    pcm = (6000 * np.sin(2 * np.pi * 220 * t)).astype("<i2").tobytes()

    async def chunks():
        yield AudioChunk(relay_id=relay, audio_data=pcm, sample_rate=16000, is_wake_word=True)
        for i in range(2):
            await asyncio.sleep(0.01)
            yield AudioChunk(relay_id=relay, audio_data=pcm, sample_rate=16000,
                             is_end_of_speech=i == 1)

    async def go():
        env = {"LOQA_DB_PATH": str(tmp_path / "hub.db"), "NATS_URL": "embedded",
               "ARBITRATION_WINDOW_DURATION": "50ms", "HUB_STT_MODEL": "test-whisper",
               "HUB_LLM_MODEL": "test-tiny", "HUB_MAX_BATCH": "4", "HUB_TTS_MODEL": "test-vits",
               "STREAMING_ENABLED": "true" if streaming else "false", "TTS_FORMAT": "flac",
               "HUB_TTS_FLAC_BLOCK": "1024"}
        cfg = cfgmod.load(env)
        srv = HubServer(cfg, skills_dir=str(tmp_path / "skills"),
                        skills_config_store=str(tmp_path / "skillcfg"),
                        transcript_hints=lambda r: HINT)
        await srv._connect_nats()
        tts = build_tts(cfg, "cpu")
        srv.processor = await asyncio.to_thread(build_gpu_processor, cfg, srv.nats, "cpu", tts,
                                                skills=srv.skills)
        await srv.start(host="127.0.0.1", http_port=0, grpc_port=0)
        msgs = []
        sub = NATSClient(name="test-relay")
        await sub.connect(srv.nats.url)
        await sub.subscribe(f"audio.{relay}", lambda m: msgs.append(json.loads(m.data)))
        await sub.flush()
        try:
            async with grpc.aio.insecure_channel(f"127.0.0.1:{srv.grpc_port}") as ch:
                got = [x async for x in stream_audio_stub(ch)(chunks())]
            await asyncio.sleep(0.3)
            await sub.flush()
            return got[-1], msgs, dict(tts.stats)
        finally:
            await sub.close()
            await srv.stop()
    return asyncio.run(go())


def test_hub_served_flac_cpu(tmp_path):
    last, msgs, stats = _serve(tmp_path, streaming=False)
    assert last.success and last.audio_format == "flac"
    x, rate = ref.flac_decode(last.response_audio)
    assert rate == 22050 and x.shape[1] > 1000
    assert last.audio_duration == pytest.approx(x.shape[1] / 22050)
    assert len(msgs) == 1 and msgs[0]["audio_format"] == "flac" and msgs[0]["sample_rate"] == 22050
    assert base64.b64decode(msgs[0]["audio_data"]) == last.response_audio
    assert stats["format_downgrades"] == 0 and stats["flac_phrases"] >= 1


def test_hub_served_flac_streaming_cpu(tmp_path):
    last, msgs, stats = _serve(tmp_path, streaming=True)
    assert last.success and last.audio_format == "flac"
    assert last.response_audio == b""               # FLAC phrases are not joined into one file
    assert msgs and all(m["audio_format"] == "flac" and m["sample_rate"] == 22050 for m in msgs)
    total = 0
    for m in msgs:
        x, rate = ref.flac_decode(base64.b64decode(m["audio_data"]))
        assert rate == 22050 and x.shape[1] > 0
        total += x.shape[1]
    assert last.audio_duration == pytest.approx(total / 22050)
    assert stats["format_downgrades"] == 0 and stats["flac_phrases"] == len(msgs)
