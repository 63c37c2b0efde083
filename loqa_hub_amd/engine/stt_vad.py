"""Voice activity detection for ``STTEngine``: its configuration and the
window plan (host side; the detector is ``ops.vad``, csrc/kernels/vad.hip).

The detector reports an utterance's speech as ``[start, end)`` spans of 20 ms
frames - one encoder position and one Whisper timestamp step each.
``plan_windows`` turns them into the encoder rows of the utterance: windows of
at most 30 s (1500 frames) that start and end at speech and are cut at pauses.
An utterance without a span is silent and gets no window at all.
"""
from __future__ import annotations

from dataclasses import dataclass

from ..ops import reference as ref

WINDOW_FRAMES = 1500        # 30 s: the encoder's positions
FRAME_S = 0.02
FRAME_HZ = 50               # frame f starts at f / 50 s (the double nearest to 0.02 f)
FRAME_SAMPLES = 320         # 16 kHz samples per frame


@dataclass(frozen=True)
class VadConfig:
    """The detector's knobs in their configuration units (``HUB_VAD_*``);
    ``params`` are the integers the kernel gets. The defaults are not tuned on
    speech data: they lean towards keeping audio."""
    threshold_db: float = 9.0        # above the noise floor
    min_level_dbfs: float = -55.0    # below it a frame is never speech
    floor_max_dbfs: float = -30.0    # cap on the noise floor
    floor_s: float = 3.0             # noise-floor window, each side
    min_speech_ms: int = 100         # shortest speech run kept
    min_silence_ms: int = 500        # gaps shorter than this are filled
    pad_ms: int = 200                # padding around speech

    def __post_init__(self):
        self.params                  # ValueError for a value out of range

    @property
    def params(self) -> ref.VadParams:
        return ref.vad_params(self.threshold_db, self.min_level_dbfs, self.floor_max_dbfs,
                              self.floor_s, self.min_speech_ms, self.min_silence_ms, self.pad_ms)


def greedy_windows(spans) -> list:
    """Windows ``(a, b)`` in frames, every ``b - a <= 1500``: a window starts
    at the first unused span's start ``a``, takes the following spans while
    ``span.end - a <= 1500`` and ends at the end of the last one taken. A span
    longer than 1500 frames gives ``(a, a + 1500)``; its rest is planned as a
    new span."""
    todo = [(int(a), int(b)) for a, b in spans if int(b) > int(a)]
    out, i = [], 0
    while i < len(todo):
        a, end = todo[i]
        if end - a > WINDOW_FRAMES:
            out.append((a, a + WINDOW_FRAMES))
            todo[i] = (a + WINDOW_FRAMES, end)
            continue
        i += 1
        while i < len(todo) and todo[i][1] - a <= WINDOW_FRAMES:
            end = todo[i][1]
            i += 1
        out.append((a, end))
    return out


def fixed_windows(a: int, b: int) -> list:
    """Consecutive 1500-frame windows over ``[a, b)`` (the last one shorter)."""
    return [(s, min(s + WINDOW_FRAMES, b)) for s in range(a, b, WINDOW_FRAMES)]


def plan_windows_counted(spans, reserved: int) -> tuple:
    """``(plan, fell_back)``: the encoder windows of an utterance whose speech
    is ``spans`` (ascending ``[start, end)`` frames) - ``greedy_windows``,
    unless that needs more than the ``reserved`` cross-attention slots the
    admission counted (one per 30 s of the utterance); then (``fell_back``)
    fixed 1500-frame windows over ``[first span's start, last span's end)``,
    which always fit. No spans: ``([], False)``, the utterance is silent."""
    spans = [(int(a), int(b)) for a, b in spans if int(b) > int(a)]
    if not spans:
        return [], False
    plan = greedy_windows(spans)
    fell_back = len(plan) > reserved
    if fell_back:
        plan = fixed_windows(spans[0][0], spans[-1][1])
    assert len(plan) <= max(reserved, 1), "VAD plan exceeds the reserved windows"
    return plan, fell_back


def plan_windows(spans, reserved: int) -> list:
    """The plan of ``plan_windows_counted`` alone."""
    return plan_windows_counted(spans, reserved)[0]


def clip_spans(spans, frames: int) -> list:
    """``spans`` clipped to ``[0, frames)``; empty ones dropped."""
    out = []
    for a, b in spans:
        a, b = max(0, int(a)), min(int(b), frames)
        if b > a:
            out.append((a, b))
    return out


def spans_seconds(spans, duration_s: float) -> list:
    """``(start_s, end_s)`` of frame spans, clamped to the utterance's duration."""
    return [(min(a / FRAME_HZ, duration_s), min(b / FRAME_HZ, duration_s)) for a, b in spans]
