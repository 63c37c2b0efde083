"""Segments of a Whisper window decoded with timestamps (host only, pure).

A window's sampled tokens are text tokens and timestamp tokens (ids at or above
``ts_begin``; index k stands for 0.02 k seconds from the window's start). They
are cut the way Whisper's transcribe loop cuts them:

1. each pair of consecutive timestamps closes a segment and opens the next;
2. a single trailing timestamp closes the last segment;
3. text after the last timestamp runs to the window's end and is marked open
   (its closing timestamp was never sampled: the window edge, EOT or the token
   limit came first).

Segments without text tokens are dropped.
"""
from __future__ import annotations

from dataclasses import dataclass, field

TS_STEP_S = 0.02
WINDOW_S = 30.0


@dataclass
class Segment:
    start_s: float
    end_s: float
    tokens: list = field(default_factory=list)
    open: bool = False            # no closing timestamp was sampled


def cut_window(tokens, ts_begin: int, eot: int | None = None,
               window_s: float = WINDOW_S) -> list[Segment]:
    """The segments of one window's token list, times relative to the window."""
    toks = [int(t) for t in tokens if eot is None or int(t) != eot]
    segs: list[Segment] = []
    start, cur = 0.0, []
    for t in toks:
        if t < ts_begin:
            cur.append(t)
            continue
        sec = (t - ts_begin) * TS_STEP_S
        if cur:
            # a timestamp after text closes the segment: the first of a pair,
            # or the single trailing one
            segs.append(Segment(start, max(sec, start), cur))
            cur = []
        # the next segment opens at the latest timestamp: the second of a pair,
        # or the window's opening one
        start = sec
    if cur:
        segs.append(Segment(start, max(window_s, start), cur, open=True))
    return segs


def text_tokens(tokens, ts_begin: int, eot: int | None = None) -> list[int]:
    """The window's text tokens (no timestamps, no EOT)."""
    return [int(t) for t in tokens if int(t) < ts_begin and (eot is None or int(t) != eot)]


def utterance_segments(segs: list[Segment], window: int, duration_s: float, decode,
                       offset_s: float | None = None, end_s: float | None = None
                       ) -> list[tuple[float, float, str]]:
    """``(start_s, end_s, text)`` in utterance time for window ``window``'s
    segments: offset by 30 s per window, clamped to the utterance's duration;
    segments whose text is empty are dropped. ``offset_s`` / ``end_s``: where
    the window starts and ends in the utterance when it is not a fixed 30 s one
    (``STTRequest.win_starts``, a VAD window plan); times are clamped to its end."""
    out = []
    off = window * WINDOW_S if offset_s is None else offset_s
    if end_s is not None:
        duration_s = min(duration_s, end_s)
    for s in segs:
        text = decode(s.tokens).strip()
        if not text:
            continue
        a = min(off + s.start_s, duration_s)
        b = min(max(off + s.end_s, a), duration_s)
        out.append((a, b, text))
    return out
