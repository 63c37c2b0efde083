"""The voice activity kernels (``csrc/kernels/vad.hip``) on the GPU against the
integer host model (``ops.reference.vad*``) - equality, never closeness - and
through the STT engine with graphs."""
import dataclasses

import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SENT = -7777            # pre-fill of every output: what the kernels must not touch
GUARD = 37              # samples of -32768 between utterances (odd: odd src_first)
PARAMS = ref.VadParams(level_min=3000, floor_max=1 << 20, ratio_q=2033, W=8, min_speech=3,
                       min_silence=4, pad=2)


def _layout(xs, rates):
    """Utterances laid end to end between guards of -32768, at odd offsets:
    (pcm int16, descs with consecutive frame ranges after 5 spare frames)."""
    parts, descs, o, f0 = [np.full(GUARD, -32768, np.int16)], [], GUARD, 5
    for x, r in zip(xs, rates):
        if o % 2 == 0:
            parts.append(np.full(1, -32768, np.int16))
            o += 1
        descs.append((o, x.size, r, f0))
        parts += [x, np.full(GUARD, -32768, np.int16)]
        o += x.size + GUARD
        f0 += ref.vad_frames(x.size, r)
    return np.concatenate(parts), descs


def _outs(descs, device="cuda", extra=7):
    Fs = [ref.vad_frames(n, r) for _, n, r, _ in descs]
    total = max([d[3] + F for d, F in zip(descs, Fs)] + [0]) + extra
    cap = max(Fs + [0]) // 2 + 1
    U = len(descs)
    return tuple(torch.full(s, SENT, dtype=torch.int32, device=device)
                 for s in ((total,), (U, cap, 2), (U,), (U,)))


def _check(pcm_np, descs, params):
    """Run the kernels and the host model into sentinel-filled outputs; every
    word of all four must be equal (so nothing outside an utterance's frames or
    beyond its n_spans was written). Returns the device outputs."""
    got = ops.vad(torch.from_numpy(pcm_np).cuda(), descs, params, out=_outs(descs))
    want = ref.vad(torch.from_numpy(pcm_np), descs, params, out=_outs(descs, "cpu"))
    torch.cuda.synchronize()
    for name, g, w in zip(("E", "spans", "n_spans", "speech_frames"), got, want):
        assert torch.equal(g.cpu(), w), name
    return got


def test_energies_every_rate_and_length():
    rng = np.random.default_rng(1)
    xs, rates = [], []
    for rate in (8000, 11025, 16000, 44100, 48000):
        q = rate // 50
        for n in (0, 1, q - 1, q, q + 1, 3 * rate + 7):
            xs.append(rng.integers(-32768, 32768, n).astype(np.int16))
            rates.append(rate)
    xs.append(np.full(48000 // 50 * 3 + 5, -32768, np.int16))      # a 32-bit sum overflows
    rates.append(48000)
    pcm, descs = _layout(xs, rates)
    assert all(d[0] % 2 == 1 for d in descs)
    E = _check(pcm, descs, PARAMS)[0].cpu().numpy()
    f0 = descs[-1][3]
    assert (E[f0:f0 + 4] == 1 << 30).all() and (E[:5] == SENT).all() and (E[-7:] == SENT).all()
    # a frame that read one sample across its utterance's edge would differ:
    # the guards are full scale, the utterance beside them is not
    quiet = np.full(16000 // 50 * 2, 3, np.int16)
    pcm, descs = _layout([quiet], [16000])
    E = _check(pcm, descs, PARAMS)[0].cpu().numpy()
    assert (E[5:7] == 9).all()


def _runs_pcm(rng, F, rate=16000, lens=(1, 2, 3, 4, 5, 6, 9)):
    """``F`` frames of alternating loud and quiet runs whose lengths straddle
    min_speech, min_silence and pad of PARAMS; the last frame is short."""
    q = rate // 50
    x = np.empty(F * q, np.int16)
    f, loud = 0, bool(rng.integers(2))
    while f < F:
        n = int(rng.choice(lens))
        amp = 4000 if loud else 20
        seg = x[f * q:(f + n) * q]
        seg[:] = rng.integers(-amp, amp + 1, seg.size)
        f += n
        loud = not loud
    return x[: F * q - (q // 3 if F > 1 else 0)]


def test_spans_at_the_tile_sizes():
    T = ops.vad_tile()
    rng = np.random.default_rng(2)
    Fs = [1, T - 1, 0, T, T + 1, 2 * T + 1]               # different F in one launch, one empty
    xs = [_runs_pcm(rng, F) if F else np.zeros(0, np.int16) for F in Fs]
    pcm, descs = _layout(xs, [16000] * len(xs))
    assert [ref.vad_frames(d[1], d[2]) for d in descs] == Fs
    got = _check(pcm, descs, PARAMS)
    n = got[2].cpu().numpy()
    assert n[2] == 0 and n[1] > 20 and n[5] > 40          # the patterns do give many spans
    again = ops.vad(torch.from_numpy(pcm).cuda(), descs, PARAMS, out=_outs(descs))
    for a, b in zip(again, got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("corner", [
    dict(W=0), dict(pad=0), dict(min_speech=1), dict(min_silence=0),
    dict(W=0, pad=0, min_speech=1, min_silence=0), dict(W=3000), dict(floor_max=100),
])
def test_spans_parameter_corners(corner):
    T = ops.vad_tile()
    rng = np.random.default_rng(3)
    xs = [_runs_pcm(rng, T + 37, 8000), _runs_pcm(rng, 50, 11025), _runs_pcm(rng, 3, 16000)]
    pcm, descs = _layout(xs, [8000, 11025, 16000])
    _check(pcm, descs, dataclasses.replace(PARAMS, **corner))


def test_spans_of_30000_frames():
    rng = np.random.default_rng(4)
    x = _runs_pcm(rng, 30000, 8000, lens=(1, 2, 3, 4, 5, 6, 9, 40, 400))
    pcm, descs = _layout([x], [8000])
    got = _check(pcm, descs, dataclasses.replace(PARAMS, W=150))
    assert int(got[2][0]) > 100


def test_rejections_before_any_launch():
    x = np.full(5000, 1000, np.int16)
    pcm = torch.from_numpy(x).cuda()
    good = [(1, 4001, 16000, 0)]
    bad_calls = [
        (pcm.to(torch.int32), good, PARAMS),                       # dtype
        (torch.from_numpy(np.full(10000, 1000, np.int16)).cuda()[::2], good, PARAMS),   # strided
        (pcm, [(1000, 4001, 16000, 0)], PARAMS),                   # past the end of pcm
        (pcm, [(-1, 100, 16000, 0)], PARAMS),
        (pcm, [(0, 100, 16001, 0)], PARAMS),                       # unsupported rate
        (pcm, [(0, 640, 16000, 0), (640, 640, 16000, 1)], PARAMS),  # overlapping frames
        (pcm, good, dataclasses.replace(PARAMS, ratio_q=255)),
        (pcm, good, dataclasses.replace(PARAMS, min_speech=0)),
        (pcm, good, dataclasses.replace(PARAMS, W=3001)),
        (pcm, good, dataclasses.replace(PARAMS, level_min=(1 << 30) + 1)),
        (pcm, good, PARAMS.ints()),                                # not VadParams
    ]
    for p, d, prm in bad_calls:
        out = _outs(good)
        with pytest.raises(ValueError):
            ops.vad(p, d, prm, out=out)
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in out)
    out = _outs(good)
    with pytest.raises(ValueError):                               # frames past the frame array
        ops.vad(pcm, [(1, 4001, 16000, out[0].numel() - 3)], PARAMS, out=out)
    small = tuple(t[:0] if i == 1 else t for i, t in enumerate(_outs(good)))
    with pytest.raises(ValueError):                               # spans too small
        ops.vad(pcm, good, PARAMS, out=small)
    # the launchers check the same things themselves (a caller that skips ops.vad)
    from loqa_hub_amd.ops._lib import kernels, ptr
    out = _outs(good)
    desc = np.asarray([(1, 5000, 16000, 0)], np.int64)
    d_dev = torch.from_numpy(desc).cuda()
    rc = kernels().loqa_vad_energy(ptr(pcm), pcm.numel(), ptr(d_dev), desc.ctypes.data, 1,
                                   ptr(out[0]), out[0].numel(), None)
    assert rc != 0
    torch.cuda.synchronize()
    assert bool((out[0] == SENT).all())


# ----------------------------------------------------------------------- engine
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest  # noqa: E402
from loqa_hub_amd.engine.stt_vad import VadConfig  # noqa: E402
from loqa_hub_amd.models.configs import whisper_config  # noqa: E402

CFG = whisper_config("test-whisper")


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, torch.device("cuda", 0), seed=2)


def _mk(weights, **kw):
    return STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, **kw)


def _utterance(parts, seed=3, rate=16000):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(-a, a + 1, int(round(s * rate))).astype(np.int16)
                           for s, a in parts])


def _want_row(pcm, a, b):
    row = torch.zeros(N_SAMPLES)
    x = torch.from_numpy(pcm[a * 320:b * 320])
    row[: x.numel()] = ref._pcm16_to_f32(x)
    return row


def test_engine_rows_silence_and_trimmed_slice(weights, monkeypatch):
    eng = _mk(weights, vad=VadConfig())
    assert eng.use_graphs
    one = _utterance([(0.7, 3), (1.0, 6000), (0.613, 3)])
    two = _utterance([(0.5, 3), (1.2, 6000), (29.0, 3), (1.0, 6000), (0.3, 3)], seed=4)
    src = _utterance([(0.7, 3), (1.0, 6000), (0.613, 3)], rate=48000)
    reqs = [STTRequest(one), STTRequest(np.zeros(8000, np.int16)), STTRequest(two),
            STTRequest(src, sample_rate=48000)]
    rows, ss = eng.upload(reqs)
    torch.cuda.synchronize()
    assert [r.win_frames for r in reqs] == [[(25, 95)], [], [(15, 95), (1525, 1595)], [(25, 95)]]
    assert reqs[1].vad_silent and reqs[0].vad_spans == [(0.5, 1.9)] and rows.shape[0] == 4
    for i, w in enumerate([_want_row(one, 25, 95), _want_row(two, 15, 95),
                           _want_row(two, 1525, 1595)]):
        assert torch.equal(rows[i].cpu().view(torch.int32), w.view(torch.int32)), i
    assert not rows[3, 70 * 320:].any() and rows[3, :70 * 320].abs().max() > 0.1
    # a silent utterance: no encoder call, no decoder step
    calls = []
    encode = eng.encode
    monkeypatch.setattr(eng, "encode", lambda a: (calls.append(a.shape[0]), encode(a))[1])
    quiet = STTRequest(np.zeros(24000, np.int16), max_new_tokens=8)
    eng.transcribe([quiet])
    assert calls == [] and quiet.vad_silent and quiet.text == "" and quiet.windows == 0
    assert eng.stats["decode_steps"] == 0 and eng.stats["vad_silent_utterances"] == 1
    # one window with VAD on = the same engine kind with VAD off on the trimmed slice
    r = STTRequest(one, max_new_tokens=12)
    eng.transcribe([r])
    off = _mk(weights)
    t = STTRequest(one[25 * 320:95 * 320], max_new_tokens=12)
    off.transcribe([t])
    assert calls == [1] and r.tokens == t.tokens and len(r.tokens) > 0 and r.text == t.text
    assert eng._graphs and off._graphs          # the captured step ran in both


def test_engine_70_s_in_three_windows_at_speech(weights, monkeypatch):
    """Pauses at 28 s and 55 s: three windows that start at speech, decoded by
    the continuous scheduler (encoder thread, two-deep pipeline, graphs), beside
    a silent utterance whose reserved slot comes back."""
    from test_vad import _check_window_times, _record_window_times
    calls = _record_window_times(monkeypatch)
    eng = _mk(weights, vad=VadConfig(), timestamps=True)
    x = _utterance([(0.5, 3), (27.0, 6000), (1.0, 3), (26.0, 6000), (1.0, 3), (14.0, 6000),
                    (0.5, 3)], seed=6)
    assert x.size == 70 * 16000
    r = STTRequest(x, max_new_tokens=10)
    q = STTRequest(np.zeros(16000, np.int16), max_new_tokens=10)
    try:
        done = eng.submit_batch([q, r]).result(timeout=240)
    finally:
        eng.stop()
    assert done == [q, r] and q.vad_silent and q.text == "" and q.slots == []
    assert r.win_frames == [(15, 1385), (1415, 2735), (2765, 3485)] and r.windows == 3
    assert r.win_starts == [0.3, 28.3, 55.3] and len(r.slots) == 3
    assert r.vad_spans == [(0.3, 27.7), (28.3, 54.7), (55.3, 69.7)]
    assert r.vad_speech_s == pytest.approx(27.4 + 26.4 + 14.4)
    assert len(r.win_texts) == 3 and eng.stats["long_form_windows"] == 2
    # every window's segments got that window's start and end, and lie inside it
    assert [(k, w) for k, w, *_ in calls] == [("segments", 0), ("segments", 1), ("segments", 2)]
    assert _check_window_times(r, calls)["segments"] == len(r.segments)
    assert sorted(eng._free_slots) == list(range(eng.max_slots))
    assert eng.stats["vad_plan_fallbacks"] == 0 and eng.stats["vad_silent_utterances"] == 1
