"""Acoustic STT confidence on the CPU engines: ``STTEngine(token_logprobs=True)``
records the log-probability of every sampled Whisper token, the hub turns the
mean (Whisper's ``avg_logprob``) into the transcript's confidence
(``HUB_STT_CONFIDENCE=acoustic``) and asks for a confirmation below
``HUB_STT_CONFIRM_BELOW``. With the feature off nothing changes.

Tolerance of the recomputed mean (``test_avg_logprob_matches_recomputation``):
the engine under test and the recomputation run ``WhisperModel.decode_step``
on the same token batches, so both see the same logits; what differs is the
engine's fp32 ``log_softmax`` against fp64. That error is the bound of
``tests/test_argmax_logprob.py`` for one workgroup over ``V`` = 4096 f32 logits
(``n_t`` = 16 terms per thread, depth 16 + 4 + 6 + 3, ``6u`` per step, ``4Ru`` for
the exponents with ``R`` = the largest |logit| seen, ``4u ln V`` for the log),
which the CPU reference is held to there as well; a mean of values within the
bound is within the bound.
"""
import asyncio
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd import ops
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
from loqa_hub_amd.llm.transcriber import (CONFIRMATION_THRESHOLD, post_process_transcription,
                                          to_transcription_result)
from loqa_hub_amd.models.configs import whisper_config

CPU = torch.device("cpu")
U = 2.0 ** -24


def _pcms(seed=1, lens=(16000, 48000, 30000)):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 3000).astype(np.int16) for n in lens]


def _engine(**kw):
    return STTEngine(whisper_config("test-whisper"), CPU, seed=2, max_batch=4, **kw)


@pytest.fixture(scope="module")
def free_run():
    """Three free-decoded requests through ``transcribe()`` (shared, read-only)."""
    eng = _engine(token_logprobs=True)
    reqs = [STTRequest(p, max_new_tokens=10) for p in _pcms()]
    eng.transcribe(reqs)
    return eng, reqs


def test_one_logprob_per_token(free_run):
    eng, reqs = free_run
    n = 0
    for r in reqs:
        assert len(r.tokens) > 0 and len(r.logprobs) == len(r.tokens)
        assert all(math.isfinite(x) and x <= 0.0 for x in r.logprobs)
        assert r.avg_logprob == pytest.approx(float(np.mean(np.asarray(r.logprobs, np.float64))),
                                              abs=1e-12)
        n += len(r.tokens)
    assert eng.stats["logprob_tokens"] == n
    assert eng.stats["logprob_sum"] == pytest.approx(
        sum(float(np.sum(np.asarray(r.logprobs, np.float64))) for r in reqs), abs=1e-9)


def test_avg_logprob_matches_recomputation():
    """Teacher-force the emitted tokens through ``WhisperModel.decode_step``
    (the eager decoder, one request at a time, on both sides) and take the fp64
    ``log_softmax`` at the emitted ids."""
    V = whisper_config("test-whisper").vocab_size
    for pcm in _pcms()[:2]:
        eng = _engine(token_logprobs=True, fast_decode=False)
        r = STTRequest(pcm, max_new_tokens=8)
        eng.transcribe([r])
        assert len(r.logprobs) == len(r.tokens) > 0

        ref = _engine(fast_decode=False)
        seen = []
        argmax = ref._argmax
        ref._argmax = lambda logits: (seen.append(logits.detach().double().clone()),
                                      argmax(logits))[1]
        q = STTRequest(pcm, max_new_tokens=8)
        ref._admit([q], [0])
        for t in r.tokens:
            ref._eager_step([q])          # WhisperModel.decode_step over q.feed
            q.feed = [t]
        assert len(seen) == len(r.tokens) and all(x.shape == (1, V) for x in seen)
        want = [float(torch.log_softmax(x[0], dim=-1)[t]) for x, t in zip(seen, r.tokens)]
        # free decoding: every emitted token is the argmax of its step
        assert [int(x[0].argmax()) for x in seen] == r.tokens
        R = max(float(x.abs().max()) for x in seen)
        tol = 6 * U * (16 + 4 + 6 + 3) + 4 * R * U + 4 * U * math.log(V)
        err = max(abs(a - b) for a, b in zip(r.logprobs, want))
        print(f"max |logit| {R:.2f}  per-token err {err:.3e}  tol {tol:.3e}")
        assert err <= tol
        assert abs(r.avg_logprob - float(np.mean(want))) <= tol


def test_scheduler_matches_transcribe(free_run):
    _, reqs = free_run
    eng = _engine(token_logprobs=True)
    again = [STTRequest(p, max_new_tokens=10) for p in _pcms()]
    try:
        eng.submit_batch(again).result(timeout=120)
    finally:
        eng.stop()
    for a, b in zip(again, reqs):
        assert a.tokens == b.tokens
        assert a.logprobs == b.logprobs and a.avg_logprob == b.avg_logprob


def test_teacher_forced_request_has_no_logprob():
    eng = _engine(token_logprobs=True)
    r = STTRequest(_pcms()[0], transcript="turn on the kitchen lights")
    f = STTRequest(_pcms()[1], max_new_tokens=4)
    eng.transcribe([r, f])
    assert r.text and r.avg_logprob is None and r.logprobs == []
    assert f.avg_logprob is not None and len(f.logprobs) == len(f.tokens)
    assert eng.stats["logprob_tokens"] == len(f.tokens)


def test_long_form_is_the_token_weighted_mean(monkeypatch):
    eng = _engine(token_logprobs=True)
    rng = np.random.default_rng(3)
    r = STTRequest((rng.standard_normal(45 * 16000) * 3000).astype(np.int16), max_new_tokens=5)
    assert len(r.pcm) > N_SAMPLES
    windows = []
    finish = eng._finish
    monkeypatch.setattr(eng, "_finish", lambda q: (windows.append((list(q.tokens), list(q.logprobs))),
                                                   finish(q))[1])
    eng.transcribe([r])
    assert r.windows == 2 and len(windows) == 2
    assert all(len(t) == len(lp) > 0 for t, lp in windows)
    assert r.logprobs == windows[1][1]            # the last window's
    every = np.asarray(windows[0][1] + windows[1][1], np.float64)
    assert r.avg_logprob == pytest.approx(float(every.sum() / every.size), abs=1e-12)
    assert eng.stats["logprob_tokens"] == every.size


def test_off_never_calls_the_new_op(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("masked_argmax_logprob called with token_logprobs=False")
    monkeypatch.setattr(ops, "masked_argmax_logprob", boom)
    eng = _engine()
    reqs = [STTRequest(p, max_new_tokens=4) for p in _pcms()]
    eng.transcribe(reqs)
    assert all(r.tokens and r.logprobs == [] and r.avg_logprob is None for r in reqs)
    assert "logprob_tokens" not in eng.stats
    on = _engine(token_logprobs=True)
    with pytest.raises(AssertionError, match="masked_argmax_logprob called"):
        on.transcribe([STTRequest(_pcms()[0], max_new_tokens=2)])


# ------------------------------------------------------------ above the engine
TEXTS = ["", "a", "hey loqa", "hey loqa turn on the lights", "turn on the kitchen lights",
         "hmm...", "what???", "aaaaaa bbb", "Loqa, play some jazz", "ok"]


def _heuristic(raw):
    p = post_process_transcription(raw)
    return (p.cleaned_text, p.confidence_estimate, p.wake_word_detected, p.wake_word_variant,
            p.needs_confirmation)


def test_transcription_result_without_logprob_is_unchanged():
    for raw in TEXTS:
        t = to_transcription_result(raw)
        assert (t.text, t.confidence_estimate, t.wake_word_detected, t.wake_word_variant,
                t.needs_confirmation) == _heuristic(raw)
        assert t.avg_logprob is None
        assert to_transcription_result(raw, None, 0.99) == t     # the threshold is the reference's


def test_transcription_result_with_logprob():
    c = math.exp(-0.1)
    t = to_transcription_result("turn on the kitchen lights", avg_logprob=-0.1)
    assert t.confidence_estimate == c and t.avg_logprob == -0.1
    assert not t.needs_confirmation and c > CONFIRMATION_THRESHOLD
    assert to_transcription_result("turn on the lights", -0.1, c + 1e-6).needs_confirmation
    assert not to_transcription_result("turn on the lights", -0.1, c).needs_confirmation
    assert not to_transcription_result("turn on the lights", -0.1, c - 1e-6).needs_confirmation
    # a fluent hallucination: the text heuristic is content, the decoder is not
    assert not to_transcription_result("thank you for watching").needs_confirmation
    assert to_transcription_result("thank you for watching", -1.5).needs_confirmation
    assert to_transcription_result("x", 0.5).confidence_estimate == 1.0
    assert to_transcription_result("x", float("-inf")).confidence_estimate == 0.0
    # the wake word alone asks for a confirmation whatever the confidence
    w = to_transcription_result("hey loqa", -0.01, 0.0)
    assert w.wake_word_detected and w.text == "" and w.needs_confirmation


def test_config_validation():
    g = cfgmod.load({}).gpu
    assert (g.stt_confidence, g.stt_confirm_below) == ("heuristic", CONFIRMATION_THRESHOLD)
    g = cfgmod.load({"HUB_STT_CONFIDENCE": "Acoustic", "HUB_STT_CONFIRM_BELOW": "0.45"}).gpu
    assert (g.stt_confidence, g.stt_confirm_below) == ("acoustic", 0.45)
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_CONFIDENCE"):
        cfgmod.load({"HUB_STT_CONFIDENCE": "loud"})
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BACKEND=gpu"):
        cfgmod.load({"HUB_STT_CONFIDENCE": "acoustic", "HUB_STT_BACKEND": "http"})
    for bad in ("-0.1", "1.5"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_CONFIRM_BELOW"):
            cfgmod.load({"HUB_STT_CONFIRM_BELOW": bad})


def _serve(tmp_path, **env):
    """One utterance without a transcript hint through the hub's voice
    processor (``server.build_gpu_processor`` on the CPU engines, command queue
    on an embedded broker); returns (result, job, processor stats, engine)."""
    from loqa_hub_amd.messaging.nats_server import NATSServer
    from loqa_hub_amd.messaging.nats_service import NATSService
    from loqa_hub_amd.server import build_gpu_processor

    async def go():
        cfg = cfgmod.load({"LOQA_DB_PATH": str(tmp_path / "hub.db"), "HUB_STT_MODEL": "test-whisper",
                           "HUB_LLM_MODEL": "test-tiny", "HUB_MAX_BATCH": "4", **env})
        broker = await NATSServer("127.0.0.1", 0).start()
        nats = NATSService(broker.url)
        await nats.connect()
        proc = None
        try:
            proc = await asyncio.to_thread(build_gpu_processor, cfg, nats, "cpu", None, bridge=False)
            proc.job_sink = []
            res = await proc.process("kitchen-relay", "req-1", np.zeros(0, np.float32), 16000,
                                     pcm16=_pcms(7, (24000,))[0])
            return res, proc.job_sink[0], dict(proc.stats), proc.pipeline.stt
        finally:
            if proc is not None:
                await proc.close()
            await nats.close()
            await broker.stop()
    return asyncio.run(go())


@pytest.mark.parametrize("below,confirm", [("1.0", True), ("0.0", False)])
def test_served_acoustic_confidence(tmp_path, below, confirm):
    res, job, stats, stt = _serve(tmp_path, HUB_STT_CONFIDENCE="acoustic",
                                  HUB_STT_CONFIRM_BELOW=below)
    assert stt.token_logprobs
    tr = job.transcription
    assert tr.avg_logprob is not None and tr.avg_logprob < 0.0
    m = res.metrics["stt"]
    assert m["avg_logprob"] == tr.avg_logprob and m["confidence"] == math.exp(tr.avg_logprob)
    # exp(avg) is in (0, 1): under 1.0 and not under 0.0, whatever the model's
    # probabilities are (the wake-word-only rule aside)
    assert tr.needs_confirmation == (confirm or (tr.wake_word_detected and tr.text == ""))
    assert stats["stt_low_confidence"] == int(confirm)
    assert res.intents and tr.needs_confirmation == confirm
    assert res.command == ("confirmation_needed" if confirm else "voice_command_success")


def test_served_default_is_the_heuristic(tmp_path):
    res, job, stats, stt = _serve(tmp_path)
    assert not stt.token_logprobs and "logprob_tokens" not in stt.stats
    tr = job.transcription
    want = post_process_transcription(job.raw_text)
    assert res.metrics["stt"] == {"confidence": want.confidence_estimate, "avg_logprob": None}
    assert (tr.text, tr.needs_confirmation) == (want.cleaned_text, want.needs_confirmation)
    # the command of the parent commit: decided by the text heuristic alone
    assert res.intents
    assert res.command == ("confirmation_needed" if want.needs_confirmation
                           else "voice_command_success")
    assert stats["stt_low_confidence"] == int(want.confidence_estimate < CONFIRMATION_THRESHOLD)
