"""Transcriber interface + transcript post-processing (wake-word stripping and
heuristic confidence).

Behavioural spec: ``internal/llm/transcriber.go:11-29`` (interface/result),
``internal/llm/stt_client.go:401-458`` (postProcessTranscription: 10 wake-word
variants most-specific first, separator stripping, NeedsConfirmation when
confidence < 0.6 or only the wake word was spoken) and ``:461-513``
(estimateConfidence: base 0.8, -0.3 if < 3 chars, -0.2 for ``...``/``???``,
-0.3 per word with a character > 60 %, +0.1 for hey/loqa, clamp [0, 1]).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Protocol

import numpy as np

WAKE_WORD_PATTERNS = ["hey loqa", "hey loca", "hey luka", "hey luca", "hey logic", "hey local",
                      "loqa", "loca", "luka", "luca"]
CONFIRMATION_THRESHOLD = 0.6


@dataclass
class TranscriptionResult:
    text: str = ""
    confidence_estimate: float = 0.0
    wake_word_detected: bool = False
    wake_word_variant: str = ""
    needs_confirmation: bool = False
    avg_logprob: float | None = None   # mean Whisper token log-probability (acoustic confidence)
    # read from the Whisper start-of-transcript logits (gpu backend with
    # language detection or the no-speech rule; else None)
    language: str | None = None
    language_prob: float | None = None
    no_speech_prob: float | None = None
    # HUB_STT_TIMESTAMPS=segment (gpu backend; else None): (start_s, end_s, text)
    # segments in utterance time, the first one's start and the last one's end
    segments: list | None = None
    speech_start_s: float | None = None
    speech_end_s: float | None = None
    # HUB_STT_TEMPERATURE with a fallback (gpu backend; else None): the highest
    # temperature any 30 s window was kept at and the largest compression ratio
    # of the windows' texts
    temperature: float | None = None
    compression_ratio: float | None = None
    # HUB_STT_WORD_TIMESTAMPS=on (gpu backend; else None): (start_s, end_s, word,
    # probability) in utterance time, the decoder's words before the wake-word
    # cut, and the start of the first word after the wake word's words (None
    # without a wake word or without a word after it)
    words: list | None = None
    command_start_s: float | None = None
    # HUB_STT_HOTWORDS (gpu backend; else None): the configured phrases that the
    # decoder's text contains, in order of first occurrence
    hotwords: list | None = None
    # HUB_STT_VAD=on (gpu backend; else None): the detector's speech spans as
    # (start_s, end_s) in utterance time, the speech they hold in seconds, and
    # whether the utterance had none at all (it was not transcribed)
    vad_spans: list | None = None
    vad_speech_s: float | None = None
    vad_silent: bool = False


@dataclass
class PostProcessingResult:
    original_text: str
    cleaned_text: str
    wake_word_detected: bool
    wake_word_variant: str
    confidence_estimate: float
    needs_confirmation: bool


class Transcriber(Protocol):
    async def transcribe(self, audio: np.ndarray, sample_rate: int) -> str: ...

    async def transcribe_with_confidence(self, audio: np.ndarray,
                                         sample_rate: int) -> TranscriptionResult: ...

    async def close(self) -> None: ...


def estimate_confidence(text: str) -> float:
    if text == "":
        return 0.0
    c = 0.8
    # Go len() counts bytes
    if len(text.encode("utf-8")) < 3:
        c -= 0.3
    if "..." in text or "???" in text:
        c -= 0.2
    for word in text.split():
        wl = len(word.encode("utf-8"))
        if wl > 2:
            counts: dict[str, int] = {}
            for ch in word:
                counts[ch] = counts.get(ch, 0) + 1
            if any(n / wl > 0.6 for n in counts.values()):
                c -= 0.3
    low = text.lower()
    if "hey" in low or "loqa" in low:
        c += 0.1
    return min(1.0, max(0.0, c))


def post_process_transcription(raw: str) -> PostProcessingResult:
    res = PostProcessingResult(raw, raw, False, "", estimate_confidence(raw), False)
    low = raw.strip().lower()
    for pat in WAKE_WORD_PATTERNS:
        if low.startswith(pat):
            res.wake_word_detected = True
            res.wake_word_variant = pat
            # the reference slices the *untrimmed* text by the pattern length
            remaining = raw[len(pat):].strip()
            res.cleaned_text = remaining.lstrip(" ,.!?")
            break
    res.needs_confirmation = res.confidence_estimate < CONFIRMATION_THRESHOLD
    if res.wake_word_detected and res.cleaned_text.strip() == "":
        res.cleaned_text = ""
        res.needs_confirmation = True
    return res


def command_start(words, wake_word_variant: str) -> float | None:
    """``post_process_transcription``'s wake-word cut in seconds: the start of
    the first word after the wake word's words (``len(variant.split())`` of
    ``words``, (start_s, end_s, word, probability) tuples); None without a wake
    word or without a word after it."""
    if not words or not wake_word_variant:
        return None
    n = len(wake_word_variant.split())
    return float(words[n][0]) if n < len(words) else None


def to_transcription_result(raw: str, avg_logprob: float | None = None,
                            confirm_below: float = CONFIRMATION_THRESHOLD, *,
                            language: str | None = None, language_prob: float | None = None,
                            no_speech_prob: float | None = None, segments: list | None = None,
                            speech_start_s: float | None = None,
                            speech_end_s: float | None = None,
                            temperature: float | None = None,
                            compression_ratio: float | None = None,
                            words: list | None = None,
                            hotwords: list | None = None, vad_spans: list | None = None,
                            vad_speech_s: float | None = None,
                            vad_silent: bool = False) -> TranscriptionResult:
    """``avg_logprob`` (the on-device Whisper decode's mean token
    log-probability): the confidence is the geometric-mean token probability
    ``min(1, exp(avg_logprob))`` instead of the text heuristic, and a
    confirmation is needed below ``confirm_below``. None: the reference's
    heuristic and threshold. The wake-word-only rule holds either way.
    ``language`` / ``language_prob`` / ``no_speech_prob``: what the decoder read
    at the start-of-transcript position, carried as they are; so are
    ``segments`` / ``speech_start_s`` / ``speech_end_s`` of a decode with
    timestamps (their texts are the decoder's, before the wake-word cut), and
    ``temperature`` / ``compression_ratio`` of a decode with temperature fallback,
    and ``words`` of a decode with word timestamps, from which ``command_start_s``
    (the wake-word cut in seconds) is read, and ``hotwords`` of a decode with
    hotword biasing, and ``vad_spans`` / ``vad_speech_s`` / ``vad_silent`` of an
    engine with voice activity detection."""
    p = post_process_transcription(raw)
    probe = dict(language=language, language_prob=language_prob, no_speech_prob=no_speech_prob,
                 segments=segments, speech_start_s=speech_start_s, speech_end_s=speech_end_s,
                 temperature=temperature, compression_ratio=compression_ratio, words=words,
                 hotwords=hotwords, vad_spans=vad_spans, vad_speech_s=vad_speech_s,
                 vad_silent=vad_silent,
                 command_start_s=command_start(words, p.wake_word_variant)
                 if p.wake_word_detected else None)
    if avg_logprob is None:
        return TranscriptionResult(p.cleaned_text, p.confidence_estimate, p.wake_word_detected,
                                   p.wake_word_variant, p.needs_confirmation, **probe)
    conf = min(1.0, math.exp(avg_logprob))
    confirm = conf < confirm_below or (p.wake_word_detected and p.cleaned_text == "")
    return TranscriptionResult(p.cleaned_text, conf, p.wake_word_detected, p.wake_word_variant,
                               confirm, avg_logprob, **probe)
