"""Voice activity detection on the CPU: known answers of the integer host
model (``ops.reference.vad*``, the arbiter of csrc/kernels/vad.hip), the window
plan, the configuration, the STT engine with ``vad=`` and a served utterance."""
import asyncio
import dataclasses

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd import ops
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
from loqa_hub_amd.engine.stt_vad import (VadConfig, fixed_windows, greedy_windows, plan_windows,
                                         plan_windows_counted)
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref

P = ref.VadParams(level_min=10, floor_max=1000, ratio_q=512, W=2, min_speech=3, min_silence=3,
                  pad=2)


def _bits(s):
    return np.array([c == "1" for c in s], bool)


def _spans(s, **kw):
    """Spans of a raw pattern ('1' speech, '.' not) after close, open, pad."""
    out = ref.vad_smooth(_bits(s), dataclasses.replace(P, **kw))
    return [list(map(int, r)) for r in ref._runs(out)]


# ------------------------------------------------------------------ host model
def test_params_from_decibels():
    p = ref.vad_params()
    # 2^30 10^-5.5 = 3395.4, 2^30 10^-3 = 1073741.8, 256 10^0.9 = 2033.5 - 0.02
    assert p == ref.VadParams(level_min=3395, floor_max=1073742, ratio_q=2033, W=150,
                              min_speech=5, min_silence=25, pad=10)
    q = ref.vad_params(0, 0, -100, 0, 20, 0, 0)
    assert q == ref.VadParams(1 << 30, 0, 256, 0, 1, 0, 0)
    assert ref.vad_params(40, -100, 0, 60, 10000, 10000, 10000).ints() == \
        (0, 1 << 30, 2560000, 3000, 500, 500, 500)
    for kw in (dict(threshold_db=-0.1), dict(threshold_db=40.1), dict(min_level_dbfs=0.1),
               dict(min_level_dbfs=-101), dict(floor_max_dbfs=1), dict(floor_s=-1),
               dict(floor_s=60.1), dict(min_speech_ms=0), dict(min_speech_ms=30),
               dict(min_silence_ms=-20), dict(min_silence_ms=510), dict(pad_ms=10020),
               dict(pad_ms=7), dict(threshold_db=float("nan")), dict(floor_s="3")):
        with pytest.raises(ValueError):
            ref.vad_params(**kw)
    for kw in (dict(level_min=-1), dict(floor_max=(1 << 30) + 1), dict(ratio_q=255),
               dict(ratio_q=2560001), dict(W=3001), dict(min_speech=0), dict(min_silence=501),
               dict(pad=-1), dict(pad=2.0)):
        with pytest.raises(ValueError):
            ref.check_vad_params(dataclasses.replace(P, **kw))


def test_energies_by_hand():
    # a constant: its square; all -32768: 2^30 (the sum of 320 of them needs 39 bits)
    x = np.concatenate([np.full(640, -5, np.int16), np.full(700, -32768, np.int16)])
    E = ref.vad_energy(x, [(0, 640, 16000, 0), (640, 700, 16000, 2)])
    assert E.dtype == np.uint32 and E.tolist() == [25, 25, 1 << 30, 1 << 30, 1 << 30]
    # 11025 Hz: frame 0 is [0, 220), frame 1 [220, 441), frame 2 the 10 left over
    y = np.zeros(451, np.int16)
    y[:220] = 3
    y[440] = 221            # the last sample of frame 1: 221^2 / 221
    y[441:] = 7
    assert ref.vad_frames(451, 11025) == 3 and ref.vad_frames(441, 11025) == 2
    assert ref.vad_energy(y, [(0, 451, 11025, 0)]).tolist() == [9, 221, 49]
    # floor, not rounding: (220 * 9 + 16) / 221 = 9.03 (a frame 0 of 221 samples would give it too,
    # so move the odd sample: frame 0 alone stays 9 only if it has 220 samples)
    y[220] = 4
    assert ref.vad_energy(y, [(0, 451, 11025, 0)]).tolist() == [9, (16 + 221 * 221) // 221, 49]
    # only the utterance is read, only its frames are written
    z = np.concatenate([np.full(7, -32768, np.int16), np.full(320, 2, np.int16),
                        np.full(9, -32768, np.int16)])
    out = np.full(6, 77, np.uint32)
    assert ref.vad_energy(z, [(7, 320, 16000, 3)], out).tolist() == [77, 77, 77, 4, 77, 77]
    assert ref.vad_energy(z, [(7, 0, 16000, 0)]).size == 0
    for bad in ([(7, 330, 16000, 0)], [(-1, 3, 16000, 0)], [(0, 3, 16001, 0)], [(0, 3, 16000, -1)],
                [(0, 320, 16000, 0), (0, 320, 16000, 0)]):
        with pytest.raises(ValueError):
            ref.vad_energy(z, bad)


def test_raw_decision_by_hand():
    # W = 0: the floor is the frame itself, capped: only a frame above the cap can pass
    assert ref.vad_raw([100, 5000, 100], dataclasses.replace(P, W=0)).tolist() == [False, True, False]
    assert ref.vad_raw([100, 300, 100], dataclasses.replace(P, W=0)).tolist() == [False] * 3
    # W larger than F: the floor is the utterance's minimum, 300 * 256 > 100 * 512
    assert ref.vad_raw([100, 300, 100], dataclasses.replace(P, W=50)).tolist() == [False, True, False]
    # W = 1 reaches one frame: 300 sees the 100 beside it, 250 (two away) does not
    assert ref.vad_raw([100, 300, 300, 250, 240], dataclasses.replace(P, W=1)).tolist() == \
        [False, True, False, False, False]
    # equality is not speech: 200 * 256 == 100 * 512; level_min is inclusive
    assert ref.vad_raw([100, 200, 201], dataclasses.replace(P, W=9)).tolist() == [False, False, True]
    assert ref.vad_raw([0, 9, 10], dataclasses.replace(P, W=9, level_min=10)).tolist() == \
        [False, False, True]
    # uint64: 2^30 * 256 and 2^30 * 2560000 both pass 2^32
    big = ref.VadParams(0, 1 << 30, 2560000, 1, 1, 0, 0)
    assert ref.vad_raw([1 << 30, 100], big).tolist() == [True, False]


def test_smoothing_by_hand():
    # close fills the gaps of 2 and 1 (not the 3), open then drops the runs of 2
    # at both ends (the lone frames merged by close stay), pad joins across the 3
    raw = "11" "....." "111" ".." "1" "..." "1111" "......." "1" "." "1" "......" "11"
    assert len(raw) == 38
    assert _spans(raw) == [[5, 22], [25, 32]]
    assert _spans(raw, pad=0) == [[7, 13], [16, 20], [27, 30]]
    assert _spans(raw, pad=0, min_silence=0) == [[7, 10], [16, 20]]
    assert _spans(raw, pad=0, min_speech=1) == [[0, 2], [7, 13], [16, 20], [27, 30], [36, 38]]
    # runs of min - 1, min, min + 1 at both ends of the utterance
    for n, kept in ((2, False), (3, True), (4, True)):
        s = "1" * n + "." * 6 + "1" * n
        assert _spans(s, pad=0) == ([[0, n], [n + 6, 2 * n + 6]] if kept else [])
    for g, filled in ((2, True), (3, False), (4, False)):
        s = "111" + "." * g + "111"
        assert _spans(s, pad=0) == ([[0, 6 + g]] if filled else [[0, 3], [3 + g, 6 + g]])
    # leading and trailing silence is never filled, however short
    assert _spans(".111.", pad=0) == [[1, 4]]
    assert _spans("..1.", pad=0, min_speech=1) == [[2, 3]]
    # pad reaches past frame 0 and past F - 1
    assert _spans(".111........111.", pad=3) == [[0, 7], [9, 16]]
    assert _spans(".111.", pad=3) == [[0, 5]]
    assert _spans("", pad=3) == [] and _spans("....") == []


def test_whole_detector_by_hand():
    p = ref.vad_params()
    # digital silence: no spans
    E, sp, n, sf = ref.vad(np.zeros(16000, np.int16), [(0, 16000, 16000, 0)], p)
    assert n.tolist() == [0] and sf.tolist() == [0] and not E.any() and (sp == -1).all()
    # a loud utterance without a pause: its own minimum is no floor, floor_max decides
    loud = np.full(16000, 8000, np.int16)
    E, sp, n, sf = ref.vad(loud, [(0, 16000, 16000, 0)], p)
    assert E.tolist() == [64000000] * 50 and sp[0, :1].tolist() == [[0, 50]] and sf.tolist() == [50]
    assert sp.shape == (1, 26, 2)
    uncapped = ref.vad_params(floor_max_dbfs=0.0)
    assert ref.vad(loud, [(0, 16000, 16000, 0)], uncapped)[2].tolist() == [0]
    # two utterances, the second empty; spans() on one utterance's energies
    x = np.concatenate([np.zeros(3200, np.int16), np.full(3200, 1000, np.int16),
                        np.zeros(9600, np.int16)])
    E, sp, n, sf = ref.vad(x, [(0, 16000, 16000, 4), (16000, 0, 16000, 0)], p)
    assert n.tolist() == [1, 0] and sp[0, 0].tolist() == [0, 30] and sf.tolist() == [30, 0]
    got, speech = ref.vad_spans(E.numpy().view(np.uint32)[4:54], 50, dataclasses.replace(p, pad=0))
    assert got.tolist() == [[10, 20]] and speech == 10


# ------------------------------------------------------------------ window plan
def test_plan_windows():
    assert plan_windows([], 1) == [] and plan_windows([], 0) == []          # silent
    assert plan_windows([(12, 80)], 1) == [(12, 80)]                         # one short span
    assert plan_windows([(12, 80), (100, 900), (950, 1512)], 2) == [(12, 1512)]     # packed
    assert plan_windows([(12, 80), (100, 900), (950, 1513)], 2) == [(12, 900), (950, 1513)]
    # a cut at the last pause before 30 s
    spans = [(0, 400), (450, 1400), (1450, 1600), (1700, 2900)]
    assert plan_windows(spans, 2) == [(0, 1400), (1450, 2900)]
    # a span longer than 30 s: full windows, the rest planned as a new span
    assert plan_windows([(10, 4000)], 3) == [(10, 1510), (1510, 3010), (3010, 4000)]
    assert plan_windows([(10, 3200), (3300, 3500)], 3) == [(10, 1510), (1510, 3010), (3010, 3500)]
    # three 20 s spans in 60 s: three windows against two reserved -> fixed windows
    three = [(0, 990), (1010, 1990), (2010, 3000)]
    assert greedy_windows(three) == three
    assert plan_windows_counted(three, 2) == ([(0, 1500), (1500, 3000)], True)
    assert plan_windows(three, 2) == [(0, 1500), (1500, 3000)] == fixed_windows(0, 3000)
    assert plan_windows_counted(three, 3) == (three, False) and plan_windows(three, 3) == three
    assert plan_windows_counted([], 2) == ([], False)
    assert all(b - a <= 1500 for a, b in plan_windows([(5, 9000)], 6))


# ---------------------------------------------------------------- configuration
def test_config():
    g = cfgmod.load({}).gpu
    assert g.stt_vad == "off" and g.vad_config() is None
    assert (g.vad_threshold_db, g.vad_min_level_dbfs, g.vad_floor_max_dbfs, g.vad_floor_s,
            g.vad_min_speech_ms, g.vad_min_silence_ms, g.vad_pad_ms) == \
        (9.0, -55.0, -30.0, 3.0, 100, 500, 200)
    g = cfgmod.load({"HUB_STT_VAD": "on", "HUB_VAD_THRESHOLD_DB": "12", "HUB_VAD_PAD_MS": "0",
                     "HUB_VAD_FLOOR_S": "0.5"}).gpu
    vc = g.vad_config()
    assert vc == VadConfig(threshold_db=12.0, pad_ms=0, floor_s=0.5)
    assert vc.params == ref.vad_params(12.0, pad_ms=0, floor_s=0.5) and vc.params.W == 25
    bad = [{"HUB_STT_VAD": "maybe"}, {"HUB_STT_VAD": "on", "HUB_STT_BACKEND": "http"},
           {"HUB_VAD_THRESHOLD_DB": "-1"}, {"HUB_VAD_THRESHOLD_DB": "41"},
           {"HUB_VAD_THRESHOLD_DB": "loud"}, {"HUB_VAD_THRESHOLD_DB": "nan"},
           {"HUB_VAD_MIN_LEVEL_DBFS": "1"}, {"HUB_VAD_FLOOR_MAX_DBFS": "0.5"},
           {"HUB_VAD_FLOOR_S": "-1"}, {"HUB_VAD_FLOOR_S": "61"},
           {"HUB_VAD_MIN_SPEECH_MS": "0"}, {"HUB_VAD_MIN_SPEECH_MS": "110"},
           {"HUB_VAD_MIN_SILENCE_MS": "505"}, {"HUB_VAD_MIN_SILENCE_MS": "-20"},
           {"HUB_VAD_PAD_MS": "30"}, {"HUB_VAD_PAD_MS": "10020"}, {"HUB_VAD_PAD_MS": "1.5"}]
    for env in bad:
        with pytest.raises(cfgmod.ConfigError, match="HUB_(STT_)?VAD"):
            cfgmod.load(env)
    cfgmod.load({"HUB_STT_BACKEND": "http", "HUB_VAD_PAD_MS": "40"})         # knobs alone are fine
    with pytest.raises(ValueError):
        VadConfig(pad_ms=30)
    with pytest.raises(ValueError, match="VadConfig"):
        STTEngine(whisper_config("test-whisper"), "cpu", vad=True)


# ----------------------------------------------------------------------- engine
CFG = whisper_config("test-whisper")
CPU = torch.device("cpu")
VC = VadConfig()


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, CPU, seed=0)


def _engine(weights, **kw):
    return STTEngine(CFG, CPU, seed=0, max_batch=4, weights=weights, **kw)


def _utterance(parts, seed=3, rate=16000):
    """PCM of (seconds, amplitude) parts: uniform noise of that amplitude."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(-a, a + 1, int(round(s * rate))).astype(np.int16)
                           for s, a in parts])


def _want_row(pcm, a, b):
    row = torch.zeros(N_SAMPLES)
    x = torch.from_numpy(pcm[a * 320:b * 320])
    row[: x.numel()] = ref._pcm16_to_f32(x)
    return row


def test_upload_rows_follow_the_plan(weights):
    eng = _engine(weights, vad=VC)
    one = _utterance([(0.7, 3), (1.0, 6000), (0.613, 3)])
    two = _utterance([(0.5, 3), (1.2, 6000), (29.0, 3), (1.0, 6000), (0.3, 3)], seed=4)
    forced = _utterance([(0.5, 3), (0.5, 6000)], seed=5)
    reqs = [STTRequest(one), STTRequest(np.zeros(8000, np.int16)), STTRequest(two),
            STTRequest(forced, transcript="turn on the lights")]
    assert eng.rows_needed(reqs) == 5
    rows, ss = eng.upload(reqs)
    # 200 ms of padding around the loud part, in whole frames
    assert reqs[0].win_frames == [(25, 95)] and reqs[0].win_starts == [0.5]
    assert reqs[0].vad_spans == [(0.5, 1.9)] and reqs[0].vad_speech_s == pytest.approx(1.4)
    assert reqs[1].win_frames == [] and reqs[1].vad_silent and reqs[1].windows == 0
    assert reqs[1].vad_spans == [] and reqs[1].vad_speech_s == 0.0
    assert reqs[2].win_frames == [(15, 95), (1525, 1595)] and reqs[2].windows == 2
    assert reqs[2].win_starts == [0.3, 30.5]
    # teacher-forced: today's fixed window, never gated, no VAD result
    assert reqs[3].win_frames is None and reqs[3].windows == 1 and reqs[3].win_starts == [0.0]
    assert reqs[3].vad_spans is None and not reqs[3].vad_silent
    assert rows.shape == (4, N_SAMPLES) and ss.shape == (4,)
    want = [_want_row(one, 25, 95), _want_row(two, 15, 95), _want_row(two, 1525, 1595),
            _want_row(forced, 0, 1500)]
    for i, w in enumerate(want):
        assert torch.equal(rows[i].view(torch.int32), w.view(torch.int32)), i    # +0.0 after them
        assert float(ss[i]) == pytest.approx(float(w.double().square().sum()), rel=1e-6)
    assert eng.stats["vad_utterances"] == 3 and eng.stats["vad_windows_saved"] == 1
    assert eng.stats["vad_plan_fallbacks"] == 0
    # another rate: the spans are the same frames, the rows the resampled signal's
    src = _utterance([(0.7, 3), (1.0, 6000), (0.613, 3)], rate=48000)
    r48 = STTRequest(src, sample_rate=48000)
    rows48, _ = eng.upload([r48])
    assert r48.win_frames == [(25, 95)]
    whole, _ = ops.pcm16_resample_padded(torch.from_numpy(src), [(0, src.size, 0, r48.n_samples,
                                                                  48000)], N_SAMPLES)
    assert torch.equal(rows48[0, :70 * 320], whole[0, 25 * 320:95 * 320])
    assert not rows48[0, 70 * 320:].any()


def test_plan_fallback_is_counted(weights):
    eng = _engine(weights, vad=VadConfig(min_silence_ms=100))
    x = _utterance([(19.7, 6000), (0.5, 3)] * 3)[: 60 * 16000 - 1600]
    r = STTRequest(x)
    assert eng.rows_needed([r]) == 2
    rows, _ = eng.upload([r])
    assert len(r.vad_spans) == 3 and eng.stats["vad_plan_fallbacks"] == 1
    assert r.win_frames == [(0, 1500), (1500, 2995)] and rows.shape[0] == 2
    assert torch.equal(rows[1].view(torch.int32), _want_row(x, 1500, 2995).view(torch.int32))


def test_silent_utterance_skips_the_encoder(weights, monkeypatch):
    eng = _engine(weights, vad=VC)
    calls = []
    encode = eng.encode
    monkeypatch.setattr(eng, "encode", lambda a: (calls.append(a.shape[0]), encode(a))[1])
    r = STTRequest(np.zeros(24000, np.int16), max_new_tokens=8)
    eng.transcribe([r])
    assert calls == [] and r.text == "" and r.tokens == [] and r.vad_silent and r.windows == 0
    assert r.t_done > 0 and r.slots == [] and eng.stats["decode_steps"] == 0
    assert eng.stats["vad_silent_utterances"] == 1 and eng.stats["utterances"] == 1
    # beside a spoken one: one encoder row, and the spoken one decodes as alone
    quiet = STTRequest(_utterance([(1.0, 3)]), max_new_tokens=8)
    spoken = STTRequest(_utterance([(0.5, 3), (1.0, 6000)]), max_new_tokens=8)
    eng.transcribe([quiet, spoken])
    assert calls == [1] and quiet.vad_silent and not spoken.vad_silent and spoken.tokens
    alone = STTRequest(spoken.pcm, max_new_tokens=8)
    eng.transcribe([alone])
    assert alone.tokens == spoken.tokens and eng.stats["vad_silent_utterances"] == 2
    # the continuous scheduler: a silent request completes and frees nothing it never held
    eng.start()
    try:
        q2 = STTRequest(np.zeros(16000, np.int16), max_new_tokens=8)
        s2 = STTRequest(spoken.pcm, max_new_tokens=8)
        done = eng.submit_batch([q2, s2]).result(timeout=120)
        assert done == [q2, s2] and q2.vad_silent and q2.text == "" and s2.tokens == spoken.tokens
        assert sorted(eng._free_slots) == list(range(eng.max_slots))
    finally:
        eng.stop()


def test_single_window_equals_the_trimmed_slice(weights):
    on, off = _engine(weights, vad=VC), _engine(weights)
    x = _utterance([(0.7, 3), (1.0, 6000), (0.613, 3)])
    r = STTRequest(x, max_new_tokens=12)
    on.transcribe([r])
    (a, b), = r.win_frames
    assert (a, b) == (25, 95)
    t = STTRequest(x[a * 320:b * 320], max_new_tokens=12)
    off.transcribe([t])
    assert r.tokens == t.tokens and r.text == t.text and len(r.tokens) > 0
    assert r.sumsq == pytest.approx(t.sumsq, rel=1e-6)      # the rows written, not the utterance


def test_vad_off_never_calls_the_detector(weights, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("ops.vad called with VAD off")
    monkeypatch.setattr(ops, "vad", boom)
    eng = _engine(weights)
    assert eng.vad is None and not any(k.startswith("vad") for k in eng.stats)
    r = STTRequest(_utterance([(0.5, 3), (0.5, 6000)]), max_new_tokens=8)
    eng.transcribe([r])
    assert r.win_starts == [0.0] and r.vad_spans is None and r.vad_speech_s is None
    assert r.win_frames is None and not r.vad_silent and r.windows == 1
    long = STTRequest(np.zeros(N_SAMPLES + 5, np.int16), transcript="a b")
    eng.upload([long])
    assert long.win_starts == [0.0, 30.0]
    # an engine with VAD and a batch of teacher-forced requests alone: nothing either
    on = _engine(weights, vad=VC)
    on.transcribe([STTRequest(np.zeros(16000, np.int16), transcript="turn on")])
    assert on.stats["vad_utterances"] == 0


def _record_window_times(monkeypatch):
    """Spy on the engine's ``utterance_segments`` / ``utterance_words`` calls:
    per call (kind, window, offset_s, end_s, the times it returned)."""
    from loqa_hub_amd.engine import stt_engine
    calls = []
    for kind in ("segments", "words"):
        real = getattr(stt_engine, "utterance_" + kind)

        def spy(items, window, duration_s, *a, _real=real, _kind=kind):
            out = _real(items, window, duration_s, *a)
            off, end = a[-2:]
            calls.append((_kind, window, off, end, [(o[0], o[1]) for o in out]))
            return out
        monkeypatch.setattr(stt_engine, "utterance_" + kind, spy)
    return calls


def _check_window_times(r, calls):
    """Every recorded call of window w got that window's start and end, and
    every time it returned lies in [a_w / 50, b_w / 50]; together the calls
    account for all of ``r.segments`` and ``r.words``."""
    n = {"segments": 0, "words": 0}
    for kind, w, off, end, times in calls:
        a, b = r.win_frames[w]
        assert off == r.win_starts[w] == a / 50 and end == b / 50, (kind, w, off, end)
        for t0, t1 in times:
            assert a / 50 <= t0 <= t1 <= b / 50, (kind, w, t0, t1)
        n[kind] += len(times)
    return n


def test_segment_and_word_times_lie_in_their_window(weights, monkeypatch):
    calls = _record_window_times(monkeypatch)
    eng = _engine(weights, vad=VC, timestamps=True, word_timestamps=True)
    x = _utterance([(0.5, 3), (1.2, 6000), (29.0, 3), (1.0, 6000), (0.3, 3)], seed=4)
    r = STTRequest(x, max_new_tokens=24)
    eng.transcribe([r])
    assert r.win_frames == [(15, 95), (1525, 1595)] and len(r.token_frames) == 2
    assert r.segments and r.words
    assert sorted({(k, w) for k, w, *_ in calls}) == [("segments", 0), ("segments", 1),
                                                      ("words", 0), ("words", 1)]
    n = _check_window_times(r, calls)
    assert n == {"segments": len(r.segments), "words": len(r.words)}
    # each window has times of its own that the clamp did not move: they start
    # at the window's offset plus the decoder's time, not at 30 s per window
    for w, (a, b) in enumerate(r.win_frames):
        inside = [t0 for k, cw, _, _, ts in calls if cw == w for t0, _ in ts if t0 < b / 50]
        assert inside and all(a / 50 <= t < b / 50 for t in inside), (w, inside)
    assert eng.window_frames(r) == 70
    # the unit functions: offset and clamp to the window's end
    from loqa_hub_amd.engine.stt_segments import Segment, utterance_segments
    seg = [Segment(0.5, 9.0, [1], False)]
    assert utterance_segments(seg, 1, 40.0, lambda t: "x") == [(30.5, 39.0, "x")]
    assert utterance_segments(seg, 1, 40.0, lambda t: "x", 30.5, 31.9) == [(31.0, 31.9, "x")]
    from loqa_hub_amd.engine.stt_words import Word, utterance_words
    ws = [Word(0.5, 0.75, "a", 0.5), Word(1.0, 9.0, "b", None), Word(9.5, 9.75, "c", 0.25)]
    assert utterance_words(ws, 1, 40.0) == [(30.5, 30.75, "a", 0.5), (31.0, 39.0, "b", None),
                                            (39.5, 39.75, "c", 0.25)]
    assert utterance_words(ws, 1, 40.0, 30.5, 31.75) == \
        [(31.0, 31.25, "a", 0.5), (31.5, 31.75, "b", None), (31.75, 31.75, "c", 0.25)]


# ------------------------------------------------------------------- served hub
def _serve(tmp_path, pcm, **env):
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
            proc.job_sink, built = [], []
            build = proc.pipeline.build_request
            proc.pipeline.build_request = lambda j: (lambda r: (built.append(r), r)[1])(build(j))
            res = await proc.process("kitchen-relay", "req-1", np.zeros(0, np.float32), 16000,
                                     pcm16=pcm)
            return res, proc.job_sink[0], dict(proc.stats), proc.pipeline, built
        finally:
            if proc is not None:
                await proc.close()
            await nats.close()
            await broker.stop()
    return asyncio.run(go())


def test_served_silent_utterance_is_no_speech(tmp_path):
    from loqa_hub_amd.transport.audio_service import MSG_NO_SPEECH
    hum = _utterance([(1.5, 4)])
    res, job, stats, pipe, built = _serve(tmp_path, hum, HUB_STT_VAD="on")
    assert pipe.stt.vad == VadConfig()
    assert res.command == "no_speech" and res.response_text == MSG_NO_SPEECH and not res.success
    assert job.raw_text == "" and job.no_speech and job.vad_silent and job.transcription.vad_silent
    assert built == [None]                                   # no LLM request
    assert pipe.llm.stats["decode_steps"] == 0 and pipe.llm.stats["prefill_tokens"] == 0
    assert stats["stt_vad_silent"] == 1 and stats["stt_no_speech"] == 1 and stats["utterances"] == 1
    assert pipe.stt.stats["vad_silent_utterances"] == 1 and pipe.stt.stats["decode_steps"] == 0
    assert res.metrics["stt"]["vad_silent"] is True and res.metrics["stt"]["vad_spans"] == []
    assert res.metrics["stt"]["vad_speech_s"] == 0.0
    # speech: spans in the result, not silent; the feature off: none of it exists
    talk = _utterance([(0.5, 4), (1.0, 6000)])
    res, job, stats, pipe, built = _serve(tmp_path, talk, HUB_STT_VAD="on")
    assert res.metrics["stt"]["vad_spans"] == [[0.3, 1.5]] and not job.vad_silent
    assert res.metrics["stt"]["vad_speech_s"] == pytest.approx(1.2) and stats["stt_vad_silent"] == 0
    assert job.transcription.vad_spans == [(0.3, 1.5)]
    res, job, stats, pipe, built = _serve(tmp_path, hum)
    assert pipe.stt.vad is None and "stt_vad_silent" not in stats
    assert "vad_spans" not in res.metrics["stt"] and job.transcription.vad_spans is None
    assert not job.vad_silent
