"""Words of a Whisper window from its token alignment (host only, pure).

The device gives every text token of a window the 20 ms frame at which it
starts (``ops.dtw`` over the cross-attention alignment, ``tok_frame``). This
module turns tokens + frames into words the way Whisper's
``add_word_timestamps`` does:

1. the text tokens are split into words: at spaces and punctuation
   (``split_tokens_on_spaces``), or per decodable unit for languages written
   without spaces (``split_tokens_on_unicode``);
2. a word starts at its first token's frame and ends where the next word
   starts; the last word ends at the frame of the sampled ``<|endoftext|>``,
   or at the window's last frame when none was sampled;
3. its probability is the mean of its tokens' probabilities;
4. words at sentence boundaries are held to twice the median word duration
   (the median capped at 0.7 s);
5. punctuation is merged into the neighbouring word (``merge_punctuations``;
   the merged word keeps its own times and probability, as in Whisper).

Whisper's pause heuristics at segment boundaries are not applied.
"""
from __future__ import annotations

import math
import string
from dataclasses import dataclass, field

from .stt_segments import WINDOW_S

FRAME_S = 0.02
NO_SPACE_LANGUAGES = ("zh", "ja", "th", "lo", "my", "yue")
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
SENTENCE_END_MARKS = ".。!！?？"
MAX_MEDIAN_S = 0.7
_REPLACEMENT = "�"


@dataclass
class Word:
    start_s: float
    end_s: float
    word: str
    probability: float | None
    tokens: list = field(default_factory=list)
    segment: int | None = None       # index of the segment the first token belongs to


def split_tokens_on_unicode(tokens, decode) -> tuple[list, list]:
    """Tokens grouped into the shortest runs that decode to whole characters."""
    full = decode(tokens)
    words, word_tokens, cur, off = [], [], [], 0
    for t in tokens:
        cur.append(int(t))
        s = decode(cur)
        if _REPLACEMENT not in s or \
                full[off + s.index(_REPLACEMENT): off + s.index(_REPLACEMENT) + 1] == _REPLACEMENT:
            words.append(s)
            word_tokens.append(cur)
            cur = []
            off += len(s)
    if cur:                      # an incomplete character at the end stays a word of its own
        words.append(decode(cur))
        word_tokens.append(cur)
    return words, word_tokens


def split_tokens_on_spaces(tokens, decode) -> tuple[list, list]:
    """Unicode units joined into words: a unit that starts with a space or is
    punctuation starts a new word."""
    subs, sub_tokens = split_tokens_on_unicode(tokens, decode)
    words, word_tokens = [], []
    for s, st in zip(subs, sub_tokens):
        with_space = s.startswith(" ")
        punct = s.strip() != "" and s.strip() in string.punctuation
        if with_space or punct or not words:
            words.append(s)
            word_tokens.append(list(st))
        else:
            words[-1] += s
            word_tokens[-1] += st
    return words, word_tokens


def split_words(tokens, decode, language: str | None = None) -> tuple[list, list]:
    if language in NO_SPACE_LANGUAGES:
        return split_tokens_on_unicode(tokens, decode)
    return split_tokens_on_spaces(tokens, decode)


def merge_punctuations(words: list, prepended: str = PREPEND_PUNCTUATIONS,
                       appended: str = APPEND_PUNCTUATIONS) -> list:
    """Whisper's ``merge_punctuations`` on a list of ``Word``: text and tokens
    of a punctuation word move into its neighbour; emptied words are dropped."""
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        prev, nxt = words[i], words[j]
        if prev.word.startswith(" ") and prev.word.strip() in prepended and prev.word.strip():
            nxt.word = prev.word + nxt.word
            nxt.tokens = prev.tokens + nxt.tokens
            prev.word, prev.tokens = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        prev, nxt = words[i], words[j]
        if prev.word and not prev.word.endswith(" ") and nxt.word in appended and nxt.word:
            prev.word += nxt.word
            prev.tokens = prev.tokens + nxt.tokens
            nxt.word, nxt.tokens = "", []
        else:
            i = j
        j += 1
    return [w for w in words if w.word]


def constrain_durations(words: list) -> None:
    """Whisper's duration hack, in place: a word longer than twice the median
    duration (median of the non-zero durations, capped at 0.7 s) is cut at its
    end when it is a sentence-end mark, at its start when it follows one."""
    durs = sorted(w.end_s - w.start_s for w in words if w.end_s - w.start_s != 0)
    if not durs:
        return
    n = len(durs)
    median = durs[n // 2] if n % 2 else 0.5 * (durs[n // 2 - 1] + durs[n // 2])
    max_d = 2.0 * min(MAX_MEDIAN_S, float(median))
    for i in range(1, len(words)):
        w = words[i]
        if w.end_s - w.start_s > max_d:
            if w.word.strip() and w.word in SENTENCE_END_MARKS:
                w.end_s = w.start_s + max_d
            elif words[i - 1].word.strip() and words[i - 1].word in SENTENCE_END_MARKS:
                w.start_s = w.end_s - max_d


def window_words(decode, tokens, frames, end_frame: int, logprobs=None,
                 language: str | None = None, segments=None) -> list:
    """The words of one window, times relative to the window.

    ``tokens``: its text tokens (no timestamps, no EOT); ``frames``: their
    ``tok_frame``; ``end_frame``: where the last word ends (the EOT row's frame,
    or the window's frame count); ``logprobs``: the tokens' log-probabilities or
    None (teacher forcing: probability None); ``segments``: per token the index
    of its segment, or None."""
    tokens = [int(t) for t in tokens]
    if len(frames) != len(tokens):
        raise ValueError(f"{len(tokens)} text tokens but {len(frames)} frames")
    if logprobs is not None and len(logprobs) != len(tokens):
        raise ValueError(f"{len(tokens)} text tokens but {len(logprobs)} log-probabilities")
    if not tokens:
        return []
    texts, groups = split_words(tokens, decode, language)
    out, b = [], 0
    for text, g in zip(texts, groups):
        e = b + len(g)
        start = frames[b] * FRAME_S
        end = (frames[e] if e < len(tokens) else end_frame) * FRAME_S
        prob = None
        if logprobs is not None:
            prob = sum(math.exp(float(x)) for x in logprobs[b:e]) / len(g)
        out.append(Word(start, max(end, start), text, prob, list(g),
                        None if segments is None else segments[b]))
        b = e
    constrain_durations(out)
    return merge_punctuations(out)


def utterance_words(words: list, window: int, duration_s: float,
                    offset_s: float | None = None, end_s: float | None = None) -> list:
    """``(start_s, end_s, word, probability)`` in utterance time: + 30 s per
    window, clamped to the utterance's duration. ``offset_s`` / ``end_s``: the
    window's own start and end in the utterance (``STTRequest.win_starts``, a
    VAD window plan) instead of 30 s per window; times are clamped to its end."""
    off = window * WINDOW_S if offset_s is None else offset_s
    if end_s is not None:
        duration_s = min(duration_s, end_s)
    out = []
    for w in words:
        a = min(off + w.start_s, duration_s)
        b = min(max(off + w.end_s, a), duration_s)
        out.append((a, b, w.word, w.probability))
    return out
