"""``STTEngine(word_timestamps=True)`` on the GPU (``test-whisper``, utterances
of 1 - 3 s and one of 31 s = two windows): the captured synchronous step and the
two-deep pipeline record the same query bits and give the same ``token_frames``
and ``words``; ``token_frames`` is ``ref.dtw`` of the cost recomputed with
``ops`` from the engine's buffers; tokens and log-probabilities are those of the
engine with the feature off, bit for bit; a forced fallback aligns only the
attempt that is kept.

The pipeline's discarded speculative step writes one position past a window's
last row and the two schedules may hand out other slots, so the query store is
compared at the rows each alignment reads, taken when it runs.
"""
import weakref

import numpy as np
import pytest
import torch
from test_argmax_timestamps_gpu import CFG
from test_stt_fallback_gpu import _bits, _run

from loqa_hub_amd import ops
from loqa_hub_amd.engine.stt_engine import STTEngine
from loqa_hub_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
TEMPS = (0.0, 0.4, 1.0)


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, torch.device("cuda", 0), seed=2)


def _spy(eng):
    """Every alignment the engine runs: (rows, F, n_lead, the query rows' bits,
    ``tok_frame``, ``ref.dtw`` of the cost recomputed with ``ops``)."""
    # (the wrapper holds the store weakly: a reference cycle would keep the
    # engine and its captured graphs alive until a garbage collection, which
    # may then run inside a later engine's stream capture)
    calls, orig, store = [], eng.align.align, weakref.proxy(eng.align)

    def align(slot, rows, xkv, F, n_lead):
        out = orig.__func__(store, slot, rows, xkv, F, n_lead)
        r = torch.tensor(rows, dtype=torch.int32, device="cuda")
        P = ops.align_scores(store.align_q[slot], r, xkv, store.heads,
                             slot * CFG.n_audio_ctx, F)
        again = ref.dtw(ops.align_cost(P, n_lead).cpu()).tolist()
        q = store.align_q[slot][:, r.long()].cpu().view(torch.int16).numpy().tobytes()
        calls.append((list(rows), F, n_lead, q, list(out), again))
        return out
    eng.align.align = align
    return calls


def _mk(weights, **kw):
    return STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, **kw)


def _check(reqs, calls):
    assert sum(len(r.token_frames) for r in reqs) == len(calls) > 0
    for rows, F, n_lead, _, out, again in calls:
        assert out == again and len(out) == len(rows) - n_lead
        assert all(0 <= f < F for f in out) and out == sorted(out)
    for r in reqs:
        dur = r.n_samples / 16000.0
        # (the windows' texts are stripped and joined by a space: compare without spaces)
        assert "".join("".join(w for _, _, w, _ in r.words).split()) == "".join(r.text.split())
        assert all(0.0 <= a <= b <= dur for a, b, _, _ in r.words)
        assert len(r.token_frames) == r.windows - r.gated_windows


@pytest.mark.parametrize("kw", [{}, {"timestamps": True},
                                {"temperatures": TEMPS, "compression_ratio_threshold": 0.0}],
                         ids=["plain", "timestamps", "fallback"])
def test_sync_and_pipelined_steps_agree(weights, kw):
    sync = _mk(weights, word_timestamps=True, **kw)
    c_sync = _spy(sync)
    a = _run(sync)
    piped = _mk(weights, word_timestamps=True, **kw)
    assert piped.warmup_graphs() > 0
    c_piped = _spy(piped)
    b = _run(piped, pipelined=True)
    assert piped.stats["pl_steps"] > 0 and piped.stats["pl_spec"] > 0
    _check(a, c_sync)
    _check(b, c_piped)
    assert [r.windows for r in a] == [1, 1, 1, 2]           # the 31 s request: two windows
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and _bits(x.logprobs) == _bits(y.logprobs)
        assert x.token_frames == y.token_frames and x.words == y.words and len(x.tokens) > 0
        assert x.word_segments == y.word_segments
    # the same windows were aligned from the same query bits (the schedules
    # finish them in another order: match them by their rows and frames)
    key = lambda c: (c[0], c[1], c[4])  # noqa: E731
    assert sorted(map(key, c_sync)) == sorted(map(key, c_piped))
    assert sorted(c[3] for c in c_sync) == sorted(c[3] for c in c_piped)
    if "temperatures" in kw:
        # every window was retried twice; only the kept attempt was aligned
        assert all(r.fallback_attempts == 2 * r.windows for r in a)
        assert len(c_sync) == len(c_piped) == 5 == sync.stats["aligned_windows"]
    # the feature off: the same tokens and log-probability bits
    off = _mk(weights, **({"token_logprobs": True} if not kw else kw))
    for x, y in zip(a, _run(off, pipelined=True)):
        assert x.tokens == y.tokens and _bits(x.logprobs) == _bits(y.logprobs)
        assert x.text == y.text and y.words is None and y.token_frames == []


@pytest.mark.parametrize("kw", [{"use_graphs": False}, {"fused": False}, {"fast_decode": False}],
                         ids=["eager-fused", "captured-fast", "eager-reference"])
def test_every_step_function_records(weights, kw):
    eng = _mk(weights, word_timestamps=True, **kw)
    calls = _spy(eng)
    reqs = _run(eng)
    _check(reqs, calls)
    assert eng.stats["aligned_windows"] == 5
    assert eng.stats["aligned_words"] == sum(len(r.words) for r in reqs)


def test_teacher_forced_words_on_the_gpu(weights):
    from loqa_hub_amd.engine.stt_engine import STTRequest
    eng = _mk(weights, word_timestamps=True)
    calls = _spy(eng)
    pcm = (np.random.default_rng(3).standard_normal(40000) * 3000).astype(np.int16)
    r = STTRequest(pcm, transcript="hey loqa, turn on the kitchen lights.")
    eng.transcribe([r])
    _check([r], calls)
    assert [w for _, _, w, _ in r.words] == [" hey", " loqa,", " turn", " on", " the", " kitchen",
                                             " lights."]
    assert all(p is None for _, _, _, p in r.words) and calls[0][1] == 125
    assert len(r.token_frames[0]) == len(r.tokens)          # text tokens + EOT
