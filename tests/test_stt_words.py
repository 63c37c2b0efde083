"""Word timestamps on the host and on the CPU engine: the word assembly of
``engine/stt_words.py`` (splitting, punctuation, durations, offsets, segment
index), ``STTEngine(word_timestamps=True)`` on ``test-whisper`` (teacher-forced
and free, long-form with a previous-text prompt, a fallback retry), the feature
switched off, the configuration and ``TranscriptionResult.command_start_s``.
"""
import math
import weakref

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd.engine import stt_words as sw
from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest
from loqa_hub_amd.engine.tokenizer import get_tokenizer
from loqa_hub_amd.llm.transcriber import command_start, to_transcription_result
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref

CFG = whisper_config("test-whisper")
CPU = torch.device("cpu")
TOK = get_tokenizer(CFG.vocab_size)


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, CPU, seed=0)


def _pcm(seconds: float, seed: int = 1) -> np.ndarray:
    return (np.random.default_rng(seed).standard_normal(int(seconds * 16000)) * 3000).astype(np.int16)


def _engine(weights, **kw):
    return STTEngine(CFG, CPU, seed=0, max_batch=4, weights=weights, **kw)


# ------------------------------------------------------------ word assembly
def test_split_and_punctuation_on_the_synthetic_tokenizer():
    text = " hey loqa, turn on the kitchen lights."
    toks = TOK.encode(text)
    words, groups = sw.split_tokens_on_spaces(toks, TOK.decode)
    assert "".join(words) == text and [t for g in groups for t in g] == toks
    assert words[0] == " hey" and "," in words and words[-1] == " lights."
    frames = [10 * i for i in range(len(toks))]
    lps = [math.log(0.5)] * len(toks)
    out = sw.window_words(TOK.decode, toks, frames, 10 * len(toks), lps)
    assert [w.word for w in out] == [" hey", " loqa,", " turn", " on", " the", " kitchen",
                                     " lights."]
    assert [t for w in out for t in w.tokens] == toks
    # a word starts at its first token's frame; the last one ends at ``end_frame``
    b = 0
    for w in out:
        assert w.start_s == pytest.approx(frames[b] * 0.02)
        assert w.probability == pytest.approx(0.5)
        b += len(w.tokens)
    assert out[-1].end_s == pytest.approx(10 * len(toks) * 0.02)
    # merged punctuation does not move its host's times: " loqa" ends where "," started
    comma = toks.index(TOK.encode(",")[0])
    assert out[1].end_s == pytest.approx(frames[comma] * 0.02)
    assert out[2].start_s == pytest.approx(frames[comma + 1] * 0.02)
    # teacher forcing: no probabilities; prepended punctuation joins what follows
    out = sw.window_words(TOK.decode, toks, frames, 10 * len(toks))
    assert all(w.probability is None for w in out)
    W = sw.Word
    out = sw.merge_punctuations([W(0.0, 1.0, " say", None, [1]), W(1.0, 2.0, ' "', None, [2]),
                                 W(2.0, 3.0, " hello", None, [3]), W(3.0, 4.0, "!", None, [4])])
    assert [(w.word, w.start_s, w.end_s, w.tokens) for w in out] == \
        [(" say", 0.0, 1.0, [1]), (' " hello!', 2.0, 3.0, [2, 3, 4])]
    assert sw.window_words(TOK.decode, [], [], 5) == []
    with pytest.raises(ValueError):
        sw.window_words(TOK.decode, toks, frames[:-1], 5)


def test_unicode_units_and_languages_without_spaces():
    toks = TOK.encode("é on")            # é = two byte tokens: one unit
    words, groups = sw.split_tokens_on_unicode(toks, TOK.decode)
    assert words[0] == "é" and len(groups[0]) == 2 and "".join(words) == "é on"
    w_sp, _ = sw.split_words(toks, TOK.decode, "en")
    w_zh, _ = sw.split_words(toks, TOK.decode, "zh")
    assert w_sp == ["é", " on"] and w_zh == words
    assert set(sw.NO_SPACE_LANGUAGES) == {"zh", "ja", "th", "lo", "my", "yue"}


def test_duration_constraint_at_sentence_ends():
    W = sw.Word
    words = [W(0.0, 0.2, " a", None), W(0.2, 0.4, " b", None), W(0.4, 3.0, ".", None),
             W(3.0, 6.0, " c", None), W(6.0, 6.2, " d", None)]
    sw.constrain_durations(words)
    # median of (0.2, 0.2, 2.6, 3.0, 0.2) = 0.2 -> at most 0.4 s at sentence boundaries
    assert (words[2].start_s, words[2].end_s) == (0.4, pytest.approx(0.8))
    assert (words[3].start_s, words[3].end_s) == (pytest.approx(5.6), 6.0)
    assert (words[1].start_s, words[1].end_s) == (0.2, 0.4)
    long = [W(0.0, 2.0, " a", None), W(2.0, 4.0, ".", None), W(4.0, 9.0, " b", None)]
    sw.constrain_durations(long)         # the median is capped at 0.7 s -> 1.4 s
    assert long[1].end_s == pytest.approx(3.4) and long[2].start_s == pytest.approx(7.6)
    same = [W(1.0, 1.0, " a", None)]
    sw.constrain_durations(same)         # no non-zero duration: nothing to do
    assert (same[0].start_s, same[0].end_s) == (1.0, 1.0)


def test_offsets_clamping_and_segment_index():
    toks = TOK.encode(" turn on the lights")
    n = len(toks)
    out = sw.window_words(TOK.decode, toks, list(range(0, 100 * n, 100)), 1500, None, "en",
                          [0] * 2 + [None] * (n - 2))
    assert out[0].segment == 0 and out[-1].segment is None
    words = sw.utterance_words(out, 1, 33.0)
    assert words[0][:2] == (30.0, 32.0) and words[0][2] == " turn" and words[0][3] is None
    assert all(30.0 <= a <= b <= 33.0 for a, b, _, _ in words)
    assert words[-1][:2] == (33.0, 33.0)                  # past the utterance's end: clamped
    assert sw.utterance_words(out, 0, 100.0)[1][:2] == (2.0, 4.0)


# ------------------------------------------------------------------ engine
def _spy(eng):
    calls, orig, store = [], eng.align.align, weakref.proxy(eng.align)   # no reference cycle

    def align(slot, rows, xkv, F, n_lead):
        out = orig.__func__(store, slot, rows, xkv, F, n_lead)
        calls.append((slot, list(rows), F, n_lead, list(out)))
        return out
    eng.align.align = align
    return calls


def _recompute(eng, slot, rows, F, n_lead):
    """``tok_frame`` from the engine's query store and K rows, by the reference."""
    D, T = CFG.head_dim, CFG.n_audio_ctx
    q = eng.align.align_q[slot][:, torch.tensor(rows)]
    k = torch.stack([eng.xkv[l][slot * T:slot * T + F, h * D:(h + 1) * D]
                     for l, h in eng.align.heads])
    return ref.dtw(ref.align_cost(ref.align_scores(q, k, 1.0 / math.sqrt(D)), n_lead)).tolist()


def _check_words(r: STTRequest):
    dur = r.n_samples / 16000.0
    # (the windows' texts are stripped and joined by a space: compare without spaces)
    assert "".join("".join(w for _, _, w, _ in r.words).split()) == "".join(r.text.split())
    last = 0.0
    for a, b, w, p in r.words:
        assert 0.0 <= a <= b <= dur and a >= last and w
        last = a
    assert len(r.word_segments) == len(r.words)


@pytest.mark.parametrize("kw", [{}, {"timestamps": True}, {"sot_probe": True}, {"fast_decode": False}],
                         ids=["plain", "timestamps", "probe", "eager"])
def test_cpu_engine_teacher_forced_and_free(weights, kw):
    eng = _engine(weights, word_timestamps=True, **kw)
    assert eng.align.heads == [(1, 0), (1, 1)]            # the upper half of 2 layers
    calls = _spy(eng)
    forced = STTRequest(_pcm(2.0), transcript="hey loqa, turn on the kitchen lights.")
    free = STTRequest(_pcm(3.0, 2), max_new_tokens=12)
    eng.transcribe([forced, free])
    assert eng.stats["aligned_windows"] == len(calls) == 2
    assert eng.stats["aligned_words"] == len(forced.words) + len(free.words)
    n_sot = len(eng.sot)
    for r, (slot, rows, F, n_lead, out) in zip((forced, free), calls):
        _check_words(r)
        assert r.token_frames == [out] and slot == r.slot
        assert F == r.n_samples // 320 and n_lead == n_sot - 1
        assert rows[:n_lead] == list(range(n_lead))        # the SOT inputs but the last
        assert out == _recompute(eng, slot, rows, F, n_lead)
        assert all(0 <= f < F for f in out) and out == sorted(out)
    # teacher-forced: every target token (text + EOT) has a row, in order
    assert calls[0][1][n_lead:] == list(range(n_sot - 1, n_sot - 1 + len(forced.tokens)))
    assert [w for _, _, w, _ in forced.words] == [" hey", " loqa,", " turn", " on", " the",
                                                  " kitchen", " lights."]
    assert all(p is None for _, _, _, p in forced.words)
    assert forced.words[-1][1] == pytest.approx(forced.token_frames[0][-1] * 0.02)  # the EOT row
    assert all(p is not None and 0.0 <= p <= 1.0 for _, _, _, p in free.words)
    # free: the rows skip what produced timestamp tokens; no EOT row when cut by the limit
    ts0 = eng.ts_begin if eng.timestamps else 10 ** 9
    keep = [k for k, t in enumerate(free.tokens) if t < ts0 or t == eng.eot]
    assert calls[1][1][n_lead:] == [n_sot - 1 + k for k in keep]
    if eng.eot not in free.tokens and free.words:
        assert free.words[-1][1] == pytest.approx(min(F * 0.02, 3.0))


def test_long_form_prompt_offsets_the_rows(weights):
    eng = _engine(weights, word_timestamps=True)
    calls = _spy(eng)
    r = STTRequest(_pcm(31.0), transcript_windows=["turn on the kitchen lights.", "play music"])
    eng.transcribe([r])
    assert r.windows == 2 and len(calls) == 2 and len(r.token_frames) == 2
    _check_words(r)
    n_prev = 1 + len(TOK.encode(" turn on the kitchen lights."))   # <|startofprev|> + window 0
    (s0, rows0, F0, nl, out0), (s1, rows1, F1, _, out1) = calls
    assert (s0, s1) == tuple(r.slots) and (F0, F1) == (1500, 50)
    assert rows0[0] == 0 and rows1[0] == n_prev and rows1[nl] == n_prev + len(eng.sot) - 1
    assert out0 == _recompute(eng, s0, rows0, F0, nl) and out1 == _recompute(eng, s1, rows1, F1, nl)
    assert r.token_frames == [out0, out1]
    second = [w for w, s in zip(r.words, r.word_segments) if s == 1]
    assert [w[2] for w in second] == [" play", " music"]
    assert all(30.0 <= a <= b <= 31.0 for a, b, _, _ in second)
    assert r.word_segments[0] == 0


def test_fallback_aligns_only_the_kept_attempt(weights):
    eng = _engine(weights, word_timestamps=True, temperatures=(0.0, 0.4, 1.0),
                  compression_ratio_threshold=0.0)         # every attempt but the last fails
    calls = _spy(eng)
    r = STTRequest(_pcm(2.0), max_new_tokens=8, sample_seed=5)
    eng.transcribe([r])
    assert r.fallback_attempts == 2 and r.temperatures == [1.0]
    assert len(calls) == 1 and eng.stats["aligned_windows"] == 1
    slot, rows, F, nl, out = calls[0]
    assert r.token_frames == [out] == [_recompute(eng, slot, rows, F, nl)]
    _check_words(r)
    # a window gated by the no-speech rule is not aligned
    eng = _engine(weights, word_timestamps=True, no_speech=True, no_speech_threshold=1e-9,
                  logprob_threshold=0.0)
    calls = _spy(eng)
    r = STTRequest(_pcm(1.0), max_new_tokens=6)
    eng.transcribe([r])
    assert r.gated_windows == 1 and calls == [] and r.words == [] and r.token_frames == []


def test_feature_off_is_the_parent(weights, monkeypatch):
    from loqa_hub_amd import ops

    def boom(*a, **k):
        raise AssertionError("alignment op with the feature off")
    for name in ("align_record", "align_scores", "align_cost", "dtw"):
        monkeypatch.setattr(ops, name, boom)
    # (word timestamps record token log-probabilities for the words' probabilities)
    KW = ({"token_logprobs": True}, {"timestamps": True}, {"temperatures": (0.0, 1.0)})
    offs = []
    for kw in KW:
        off = _engine(weights, **kw)
        assert off.align is None and "aligned_windows" not in off.stats
        r = STTRequest(_pcm(1.0), max_new_tokens=4, sample_seed=3)
        off.transcribe([r])
        assert r.words is None and r.word_segments is None and r.token_frames == []
        offs.append((off, r))
    monkeypatch.undo()
    # switched on: the same step fields and layout, the same tokens and log-probabilities
    for kw, (off, r) in zip(KW, offs):
        on = _engine(weights, word_timestamps=True, **kw)
        assert on.step_fields == off.step_fields and on.row_fields == off.row_fields
        assert list(on._layout(4, 16).shapes) == list(off._layout(4, 16).shapes)
        r2 = STTRequest(_pcm(1.0), max_new_tokens=4, sample_seed=3)
        on.transcribe([r2])
        assert r2.tokens == r.tokens and r2.logprobs == r.logprobs and r2.text == r.text
        assert r2.words is not None and len(r2.token_frames) == 1
    assert _engine(weights, word_timestamps=True).token_logprobs


def test_alignment_heads_of_the_engine(weights):
    eng = _engine(weights, word_timestamps=True, alignment_heads="0:1,1:0")
    assert eng.align.heads == [(0, 1), (1, 0)] and eng.align.layers == [0, 1]
    assert eng.align.align_q.shape == (5, 2, CFG.n_text_ctx, CFG.head_dim)
    assert _engine(weights, word_timestamps=True, alignment_heads=[(0, 0)]).align.heads == [(0, 0)]
    with pytest.raises(ValueError, match="HUB_STT_ALIGNMENT_HEADS"):
        _engine(weights, word_timestamps=True, alignment_heads="2:0")


# ------------------------------------------------------------------ config
def test_config_knobs():
    base = {"HUB_STT_BACKEND": "gpu"}
    c = cfgmod.load(base)
    assert c.gpu.stt_word_timestamps == "off" and c.gpu.stt_alignment_heads == ""
    c = cfgmod.load({**base, "HUB_STT_WORD_TIMESTAMPS": " ON ",
                     "HUB_STT_ALIGNMENT_HEADS": "1:0, 1:1"})
    c.validate()
    assert c.gpu.stt_word_timestamps == "on" and c.gpu.stt_alignment_heads == "1:0,1:1"
    for env in ({**base, "HUB_STT_WORD_TIMESTAMPS": "word"},
                {**base, "HUB_STT_ALIGNMENT_HEADS": "1-0"},
                {**base, "HUB_STT_ALIGNMENT_HEADS": ",".join(["0:0"] * 33)},
                {"HUB_STT_BACKEND": "external", "HUB_STT_WORD_TIMESTAMPS": "on"}):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_(WORD_TIMESTAMPS|ALIGNMENT_HEADS)"):
            cfgmod.load(env).validate()
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_TIMESTAMPS"):
        cfgmod.load({**base, "HUB_STT_TIMESTAMPS": "word"}).validate()


# --------------------------------------------------------- command_start_s
def test_command_start():
    words = [(0.1, 0.4, " hey", 0.9), (0.4, 0.9, " loqa,", 0.8), (1.2, 1.5, " turn", 0.7),
             (1.5, 1.7, " on", 0.9)]
    res = to_transcription_result("hey loqa, turn on", words=words)
    assert res.wake_word_detected and res.wake_word_variant == "hey loqa"
    assert res.words == words and res.command_start_s == 1.2
    res = to_transcription_result("loqa turn on", -0.1, words=words[1:])
    assert res.wake_word_variant == "loqa" and res.command_start_s == 1.2
    res = to_transcription_result("turn on the lights", words=words[2:])
    assert not res.wake_word_detected and res.command_start_s is None and res.words == words[2:]
    res = to_transcription_result("hey loqa", words=words[:2])              # the wake word only
    assert res.wake_word_detected and res.command_start_s is None
    res = to_transcription_result("hey loqa, turn on")                      # feature off
    assert res.words is None and res.command_start_s is None
    assert command_start([], "loqa") is None and command_start(words, "") is None


def test_words_reach_the_job_and_the_result(weights):
    from types import SimpleNamespace

    from loqa_hub_amd.engine.pipeline import PipelineJob, VoicePipeline
    eng = _engine(weights, word_timestamps=True)
    r = STTRequest(_pcm(2.0), transcript="hey loqa, turn on the kitchen lights.")
    eng.transcribe([r])
    j = PipelineJob("relay", "req", r.pcm)
    VoicePipeline._stt_post(SimpleNamespace(stt_acoustic=None, stt_confirm_below=0.6), j, r)
    assert j.words == r.words and j.transcription.words == r.words
    assert j.transcription.wake_word_variant == "hey loqa"
    assert j.transcription.command_start_s == r.words[2][0] and r.words[2][2] == " turn"
    off = STTRequest(_pcm(1.0), transcript="turn on the lights")
    _engine(weights).transcribe([off])
    VoicePipeline._stt_post(SimpleNamespace(stt_acoustic=None, stt_confirm_below=0.6), j, off)
    assert j.words is None and j.transcription.words is None
    assert j.transcription.command_start_s is None
