"""Temperature fallback of the STT engine on the CPU
(``STTEngine(temperatures=..., compression_ratio_threshold=...)``): the fallback
decision, what a retry keeps and discards, the host-known staging of ``temp``
and ``rng``, the prompt reset, the configuration and the result fields. The
random-init ``test-whisper`` weights with the synthetic tokenizer decode
arbitrary tokens, so the thresholds force the paths: a compression-ratio
threshold of 0 retries every window up to the last temperature, ``inf`` with a
log-probability threshold of ``-inf`` never retries.
"""
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd import ops
from loqa_hub_amd.engine.stt_engine import (STTEngine, STTRequest, check_temperatures,
                                            compression_ratio, needs_fallback)
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref

CFG = whisper_config("test-whisper")
CPU = torch.device("cpu")
TEMPS = (0.0, 0.4, 1.0)
INF = math.inf


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, CPU, seed=0)


def _pcms():
    rng = np.random.default_rng(1)
    return [(rng.standard_normal(n) * 3000).astype(np.int16)
            for n in (16000, 48000, 31 * 16000)]


def _engine(weights, **kw):
    return STTEngine(CFG, CPU, seed=0, max_batch=4, weights=weights, **kw)


def _reqs(seed=5, n=10, **kw):
    return [STTRequest(p, max_new_tokens=n, sample_seed=seed + i, **kw)
            for i, p in enumerate(_pcms())]


# ------------------------------------------------------------ the decision
def test_needs_fallback_around_the_threshold():
    loop = "turn on the " * 12
    sentence = "turn on the kitchen lights and play some music in the bedroom please"
    assert compression_ratio(loop) > 2.4 > compression_ratio(sentence) > 1.0 > 0.0
    assert compression_ratio("") == 1.0
    assert compression_ratio("é" * 40) == 80 / len(__import__("zlib").compress(("é" * 40).encode()))
    assert needs_fallback(loop, -0.2, 2.4, -1.0)
    assert not needs_fallback(sentence, -0.2, 2.4, -1.0)
    assert needs_fallback(sentence, -1.5, 2.4, -1.0)          # improbable
    assert not needs_fallback(sentence, -1.0, 2.4, -1.0)      # strictly below
    assert not needs_fallback(sentence, None, 2.4, -1.0)
    r = compression_ratio(loop)
    assert not needs_fallback(loop, -0.2, r, -1.0) and needs_fallback(loop, -0.2, r - 1e-9, -1.0)
    assert needs_fallback(sentence, -INF, INF, -1.0) and not needs_fallback(loop, -50.0, INF, -INF)


def test_temperature_schedule_checks(weights):
    assert check_temperatures([0, 0.2, 1]) == (0.0, 0.2, 1.0)
    for bad in ((), (0.2, 0.4), (0.0, 0.4, 0.4), (0.0, 0.6, 0.4), (0.0, 1.2), (0.0, math.nan),
                ("a",), 0.5):
        with pytest.raises(ValueError, match="temperatures"):
            check_temperatures(bad)
    with pytest.raises(ValueError, match="temperatures"):
        _engine(weights, temperatures=(0.2,))
    with pytest.raises(ValueError, match="compression_ratio_threshold"):
        _engine(weights, temperatures=TEMPS, compression_ratio_threshold=-1.0)


# ------------------------------------------------------ feature off: the parent
def test_feature_off_stages_the_parents_fields(weights, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("masked_argmax_sample with the feature off")
    monkeypatch.setattr(ops, "masked_argmax_sample", boom)
    calls = []
    for name in ("masked_argmax", "masked_argmax_logprob", "masked_argmax_logprob_probe",
                 "masked_argmax_timestamps"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=fn, _n=name, **k: (calls.append(_n),
                                                                        _f(*a, **k))[1])
    S = STTEngine.STEP_FIELDS
    want = {(): (S, "masked_argmax"),
            (("token_logprobs", True),): (S, "masked_argmax_logprob"),
            (("sot_probe", True),): (S[:8] + ("mask_row", "probe") + S[8:],
                                     "masked_argmax_logprob_probe"),
            (("timestamps", True),): (S[:8] + ("mask_row", "probe", "ts_ctl") + S[8:],
                                      "masked_argmax_timestamps")}
    for kw, (fields, op) in want.items():
        for extra in ({}, {"temperatures": (0.0,)}, {"temperatures": [0],
                                                     "compression_ratio_threshold": 0.0}):
            eng = _engine(weights, **dict(kw), **extra)
            assert not eng.fallback and eng.step_fields == fields
            assert list(eng._layout(4, 16).shapes) == list(fields)
            assert "fallback_windows" not in eng.stats and "fallback_attempts" not in eng.stats
        del calls[:]
        r = STTRequest(_pcms()[0], max_new_tokens=4)
        eng.transcribe([r])
        assert set(calls) == {op}, (kw, calls)
        assert r.temperatures == [] and r.compression_ratios == [] and r.fallback_attempts == 0
        assert r.sample_seed is None
    off = _engine(weights)
    assert off.row_fields is False and off.token_logprobs is False
    lay = off._layout(4, 16)
    assert lay.n32 == STTEngine.step_layout(4, 16, off.max_blocks).n32


def test_feature_on_layout(weights):
    S = STTEngine.STEP_FIELDS
    eng = _engine(weights, temperatures=TEMPS)
    assert eng.fallback and eng.row_fields and eng.token_logprobs and not eng.sot_probe
    assert eng.step_fields == S[:8] + ("mask_row", "probe", "temp", "rng") + S[8:]
    ts = _engine(weights, temperatures=TEMPS, timestamps=True)
    assert ts.step_fields == S[:8] + ("mask_row", "probe", "ts_ctl", "temp", "rng") + S[8:]
    assert ts._layout(4, 16).shapes["temp"] == (4,) and ts._layout(4, 16).shapes["rng"] == (4,)
    assert eng.stats["fallback_windows"] == 0 and eng.stats["fallback_attempts"] == 0


# ----------------------------------------------------------- forced fallback
KWS = [{}, {"timestamps": True}, {"timestamps": True, "language": "auto", "no_speech": True}]
KW_IDS = ["plain", "timestamps", "timestamps-probing"]


@pytest.mark.parametrize("kw", KWS, ids=KW_IDS)
def test_forced_fallback_runs_every_temperature(weights, kw, monkeypatch):
    eng = _engine(weights, temperatures=TEMPS, compression_ratio_threshold=0.0, **kw)
    staged = []
    sample = ops.masked_argmax_sample

    def tap(logits, mask, mask_rows, probe, ts_ctl, *a):
        staged.append((a[-2].clone(), a[-1].clone(), None if ts_ctl is None else ts_ctl.clone(),
                       probe.clone()))
        return sample(logits, mask, mask_rows, probe, ts_ctl, *a)
    monkeypatch.setattr(ops, "masked_argmax_sample", tap)
    reqs = _reqs()
    eng.transcribe(reqs)
    assert [r.windows for r in reqs] == [1, 1, 2]
    for r in reqs:
        assert r.fallback_attempts == (len(TEMPS) - 1) * r.windows
        assert r.temperatures == [TEMPS[-1]] * r.windows
        assert len(r.compression_ratios) == r.windows and all(c > 0 for c in r.compression_ratios)
        assert len(r.tokens) > 0 and len(r.logprobs) == len(r.tokens)
        assert math.isfinite(r.avg_logprob) and r.avg_logprob < 0
        if eng.sot_probe:
            assert len(r.no_speech_probs) == r.windows      # a retry's SOT step records nothing
            assert r.language is not None
        if eng.timestamps:
            assert eng.ts_begin <= r.tokens[0] <= eng.ts_begin + eng.max_initial
            assert r.segments is not None
    if eng.sot_probe:
        assert sum(eng.stats["languages"].values()) == len(reqs)
    assert eng.stats["fallback_windows"] == 4 and eng.stats["fallback_attempts"] == 8
    # staging: the temperatures are the schedule's, a greedy row has key 0, a
    # probing row (the SOT step) and a rule-off row (prompt chunks) are greedy
    seen = set()
    for temp, rng, ctl, probe in staged:
        assert temp.dtype == torch.float32 and rng.dtype == torch.int32
        for b in range(temp.numel()):
            t = float(temp[b])
            seen.add(t)
            assert t in (0.0, float(np.float32(0.4)), 1.0)
            if t == 0.0:
                assert int(rng[b]) == 0
            if int(probe[b]) >= 0:
                assert t == 0.0
            if ctl is not None and t > 0:
                assert int(ctl[b]) in (1, 2)
    assert seen == {0.0, float(np.float32(0.4)), 1.0}
    # the keys name the draw: (seed, window, attempt, token index)
    keys = {int(k) for _, rng, _, _ in staged for k in rng.tolist() if k}
    r = reqs[2]
    for w in range(2):
        for a in (1, 2):
            for i in range(len(r.tokens)):
                assert ref.key_i32(ref.sample_key(r.sample_seed, w, a, i)) in keys
    assert ref.key_i32(ref.sample_key(r.sample_seed, 0, 0, 0)) not in keys    # attempt 0 is greedy


def test_no_trigger_is_one_greedy_attempt(weights):
    on = _engine(weights, temperatures=TEMPS, compression_ratio_threshold=INF,
                 logprob_threshold=-INF)
    plain = _engine(weights, token_logprobs=True)
    a, b = _reqs(), [STTRequest(p, max_new_tokens=10) for p in _pcms()]
    on.transcribe(a)
    plain.transcribe(b)
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and x.text == y.text and len(x.tokens) > 0
        assert np.asarray(x.logprobs, np.float32).tobytes() == \
            np.asarray(y.logprobs, np.float32).tobytes()
        assert x.avg_logprob == y.avg_logprob
        assert x.fallback_attempts == 0 and x.temperatures == [0.0] * x.windows
        assert x.compression_ratios == [compression_ratio(t) for t in x.win_texts]
    assert on.stats["fallback_windows"] == 0 and on.stats["fallback_attempts"] == 0


def test_logprob_condition_alone_triggers(weights):
    # random-init tokens: a mean log-probability far below -1 -> retried; the
    # last temperature's result is kept whatever its quality
    eng = _engine(weights, temperatures=(0.0, 0.5), compression_ratio_threshold=INF)
    reqs = _reqs()[:1]
    eng.transcribe(reqs)
    assert reqs[0].fallback_attempts == 1 and reqs[0].temperatures == [0.5]
    assert reqs[0].avg_logprob < -1.0


def test_seeds(weights):
    eng = _engine(weights, temperatures=TEMPS, compression_ratio_threshold=0.0)
    a, b, c = _reqs(5), _reqs(5), _reqs(900)
    eng.transcribe(a)
    eng.transcribe(b[::-1])                 # another batch order: the keys do not depend on it
    eng.transcribe(c)
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and x.logprobs == y.logprobs and x.text == y.text
    assert any(x.tokens != z.tokens for x, z in zip(a, c))
    # an unset seed is assigned by the engine, a different one per request
    d = [STTRequest(p, max_new_tokens=6) for p in _pcms()[:2]]
    eng.transcribe(d)
    assert d[0].sample_seed is not None and d[0].sample_seed != d[1].sample_seed
    # one request at a time takes the same draws as the batch
    solo = _reqs(5)
    for r in solo:
        eng.transcribe([r])
    for x, y in zip(a, solo):
        assert x.tokens == y.tokens


def test_prompt_reset_above_half(weights, monkeypatch):
    begun = []
    begin = STTEngine._begin_window

    def tap(self, r, w):
        begin(self, r, w)
        begun.append((w, r.attempt, list(r.chunks[0])))
    monkeypatch.setattr(STTEngine, "_begin_window", tap)
    for temps, prompted in (((0.0, 0.4), True), ((0.0, 1.0), False), ((0.0, 0.5), True)):
        del begun[:]
        eng = _engine(weights, temperatures=temps, compression_ratio_threshold=0.0)
        r = _reqs()[2]
        eng.transcribe([r])
        assert r.windows == 2 and r.temperatures == [temps[1]] * 2
        assert [(w, a) for w, a, _ in begun] == [(0, 0), (0, 1), (1, 0), (1, 1)]
        for w, a, first in begun[2:]:
            assert (first[0] == eng.sop) == prompted, (temps, w, a, first)
        assert begun[0][2][0] != eng.sop


def test_teacher_forced_windows_never_retry(weights):
    eng = _engine(weights, temperatures=TEMPS, compression_ratio_threshold=0.0, timestamps=True)
    texts = ["turn on the kitchen lights", "play music in the bedroom"]
    reqs = [STTRequest(p, transcript=t, sample_seed=3) for p, t in zip(_pcms(), texts)]
    eng.transcribe(reqs)
    plain = _engine(weights, timestamps=True)
    want = [STTRequest(p, transcript=t) for p, t in zip(_pcms(), texts)]
    plain.transcribe(want)
    for r, w in zip(reqs, want):
        assert r.fallback_attempts == 0 and r.temperatures == [0.0]
        assert r.tokens == w.tokens and r.text == w.text and r.text and r.logprobs == []
    assert eng.stats["fallback_attempts"] == 0
    assert eng.ts_state.tolist() == [0] * 5           # every row ran rule-off and greedy


def test_gated_windows_never_retry(weights):
    kw = dict(no_speech=True, no_speech_threshold=1e-9, logprob_threshold=0.0)
    eng = _engine(weights, temperatures=TEMPS, compression_ratio_threshold=0.0, **kw)
    reqs = _reqs()
    eng.transcribe(reqs)
    for r in reqs:
        assert r.gated_windows == r.windows and r.text == "" and r.fallback_attempts == 0
        assert r.temperatures == [0.0] * r.windows and len(r.no_speech_probs) == r.windows
    assert eng.stats["fallback_attempts"] == 0 and eng.stats["no_speech_windows"] == 4


def test_scheduler_thread_takes_the_same_steps(weights):
    kw = dict(temperatures=TEMPS, compression_ratio_threshold=0.0, timestamps=True)
    a = _reqs()
    _engine(weights, **kw).transcribe(a)
    sched = _engine(weights, **kw)
    b = _reqs()
    try:
        sched.submit_batch(b).result(timeout=300)
    finally:
        sched.stop()
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and x.logprobs == y.logprobs and x.text == y.text
        assert x.temperatures == y.temperatures and x.fallback_attempts == y.fallback_attempts


# ------------------------------------------------------- configuration, surface
def test_config():
    g = cfgmod.load({})
    assert g.gpu.stt_temperature == [0.0] and g.gpu.stt_compression_ratio_threshold == 2.4
    c = cfgmod.load({"HUB_STT_TEMPERATURE": "0, 0.2,0.4,0.6,0.8,1.0",
                     "HUB_STT_COMPRESSION_RATIO_THRESHOLD": "2.0"})
    assert c.gpu.stt_temperature == [0.0, 0.2, 0.4, 0.6, 0.8, 1.0]
    assert c.gpu.stt_compression_ratio_threshold == 2.0
    assert cfgmod.load({"HUB_STT_TEMPERATURE": "0"}).gpu.stt_temperature == [0.0]
    for bad in ("0.2", "0,0.4,0.4", "0,0.6,0.4", "0,1.5", "0,nan", "0,hot", "0,,1", "-0,-0.1"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_TEMPERATURE"):
            cfgmod.load({"HUB_STT_TEMPERATURE": bad})
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BACKEND=gpu"):
        cfgmod.load({"HUB_STT_TEMPERATURE": "0,0.5", "HUB_STT_BACKEND": "http"})
    cfgmod.load({"HUB_STT_TEMPERATURE": "0", "HUB_STT_BACKEND": "http"})
    for bad in ("0", "-1", "nan", "high"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_COMPRESSION_RATIO_THRESHOLD"):
            cfgmod.load({"HUB_STT_COMPRESSION_RATIO_THRESHOLD": bad})


def test_transcriber_and_pipeline_carry_the_fields(weights):
    from types import SimpleNamespace as NS

    from loqa_hub_amd.engine.pipeline import PipelineJob, VoicePipeline
    from loqa_hub_amd.llm.transcriber import TranscriptionResult, to_transcription_result
    t = TranscriptionResult()
    assert t.temperature is None and t.compression_ratio is None
    t = to_transcription_result("hey loqa lights on", temperature=0.4, compression_ratio=1.2)
    assert (t.temperature, t.compression_ratio, t.text) == (0.4, 1.2, "lights on")
    t = to_transcription_result("lights on", -0.3, temperature=1.0, compression_ratio=3.0)
    assert (t.temperature, t.compression_ratio, t.avg_logprob) == (1.0, 3.0, -0.3)
    eng = _engine(weights, temperatures=(0.0, 0.4), compression_ratio_threshold=0.0)
    r = _reqs()[2]
    eng.transcribe([r])
    j = PipelineJob("relay", "req", r.pcm)
    VoicePipeline._stt_post(NS(stt_acoustic=False, stt_confirm_below=0.6), j, r)
    assert j.transcription.temperature == float(0.4) and j.stt_fallback
    assert j.transcription.compression_ratio == max(r.compression_ratios)
    off = _engine(weights)
    r = STTRequest(_pcms()[0], max_new_tokens=4)
    off.transcribe([r])
    j = PipelineJob("relay", "req", r.pcm)
    VoicePipeline._stt_post(NS(stt_acoustic=False, stt_confirm_below=0.6), j, r)
    assert j.transcription.temperature is None and j.transcription.compression_ratio is None
    assert not j.stt_fallback


def test_served_utterance_carries_the_fallback(tmp_path):
    """Through ``server.build_gpu_processor`` (CPU engines): the knobs reach the
    engine, the result's ``metrics["stt"]`` and the processor's counter."""
    from test_stt_sot_probe import _serve
    base, bjob, bstats, bpipe, _ = _serve(tmp_path)
    assert not bpipe.stt.fallback and bstats["stt_fallback"] == 0 and not bjob.stt_fallback
    assert set(base.metrics["stt"]) == {"confidence", "avg_logprob"}
    # random-init tokens: the mean log-probability is far below -1, so every
    # window falls through to the last temperature
    res, job, stats, pipe, _ = _serve(tmp_path, HUB_STT_TEMPERATURE="0,0.5,1",
                                      HUB_STT_COMPRESSION_RATIO_THRESHOLD="3.5")
    stt = pipe.stt
    assert stt.temperatures == (0.0, 0.5, 1.0) and stt.compression_ratio_threshold == 3.5
    assert stt.fallback and stt.logprob_threshold == -1.0
    assert stats["stt_fallback"] == 1 and job.stt_fallback
    assert stt.stats["fallback_windows"] == 1 and stt.stats["fallback_attempts"] == 2
    m, tr = res.metrics["stt"], job.transcription
    assert m["temperature"] == tr.temperature == 1.0
    assert m["compression_ratio"] == tr.compression_ratio > 0.0
    # a threshold no window misses: enabled, never triggered, the default's transcript
    res, job, stats, pipe, _ = _serve(tmp_path, HUB_STT_TEMPERATURE="0,0.5,1",
                                      HUB_STT_LOGPROB_THRESHOLD="-1000",
                                      HUB_STT_COMPRESSION_RATIO_THRESHOLD="1000")
    assert stats["stt_fallback"] == 0 and pipe.stt.stats["fallback_attempts"] == 0
    assert job.raw_text == bjob.raw_text != "" and res.metrics["stt"]["temperature"] == 0.0
    assert (res.command, res.intents, res.transcription) == \
        (base.command, base.intents, base.transcription)
