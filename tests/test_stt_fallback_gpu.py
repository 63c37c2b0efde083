"""``STTEngine(temperatures=...)`` on the GPU: the eager-launch step, the captured
synchronous step and the two-deep pipeline (captured, and through
``_launch_sync`` with no graph) stage the same ``temp`` / ``rng`` per sampled
token and run the same kernel, so with every fallback forced
(``compression_ratio_threshold=0``) they give the same tokens and
log-probability bits, ``temperatures`` and ``fallback_attempts``.

The GPU and the CPU engine are *not* required to draw the same tokens: the
device's ``logf`` differs from the host's in the last ulp, and the decoders
differ (bf16 against fp32 logits), so a near-tie between two Gumbel keys may go
either way. The CPU engine is held to the same invariants in
``tests/test_stt_fallback.py``.
"""
import numpy as np
import pytest
import torch
from test_argmax_timestamps_gpu import CFG, _pcms

from loqa_hub_amd import ops
from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest

pytestmark = pytest.mark.gpu
TEMPS = (0.0, 0.4, 1.0)


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, torch.device("cuda", 0), seed=2)


def _run(eng, pipelined=False, seed=40):
    """``test_argmax_timestamps_gpu._run`` with seeded requests: three arrive
    one step apart, then the 31 s one (two windows) once two slots are free."""
    from loqa_hub_amd.engine.stt_pipeline import STTPipeline
    reqs = [STTRequest(p, max_new_tokens=12, sample_seed=seed + i) for i, p in enumerate(_pcms())]
    pl = STTPipeline(eng) if pipelined else None
    pending, live, free = list(reqs), [], list(range(eng.max_batch))
    while pending or live:
        if pending and eng.rows_needed(pending[:1]) <= len(free):
            r = pending.pop(0)
            eng._admit([r], [free.pop(0) for _ in range(eng.rows_needed([r]))])
            if pl is not None:
                pl.admit(r)
            live.append(r)
        for r in (pl.pump(live) if pl is not None else eng._decode_once(live)) if live else []:
            free = sorted(free + r.slots)
        live = [r for r in live if r.t_done == 0.0]
    if pl is not None:
        pl.drain()
    torch.cuda.synchronize()
    return reqs


def _bits(xs):
    return np.asarray(xs, np.float32).tobytes()


@pytest.mark.parametrize("kw", [{}, {"timestamps": True},
                                {"timestamps": True, "language": "auto", "no_speech": True}],
                         ids=["plain", "timestamps", "timestamps-probing"])
def test_engine_paths_agree_under_forced_fallback(weights, kw):
    mk = lambda **k: STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights,
                               temperatures=TEMPS, compression_ratio_threshold=0.0, **kw, **k)
    eager = _run(mk(use_graphs=False))
    graph = _run(mk())
    warm = mk()
    assert warm.warmup_graphs() > 0 and warm._graphs_frozen
    keys = set(warm._graphs)
    piped = _run(warm, pipelined=True)
    assert set(warm._graphs) == keys and warm.stats["pl_steps"] > 0 and warm.stats["pl_spec"] > 0
    frozen = mk()
    frozen._graphs_frozen = True
    synced = _run(frozen, pipelined=True)
    assert frozen._graphs == {} and frozen.stats["pl_steps"] == 0
    for e, g, p, s in zip(eager, graph, piped, synced):
        assert e.tokens == g.tokens == p.tokens == s.tokens and len(e.tokens) > 0
        assert _bits(e.logprobs) == _bits(g.logprobs) == _bits(p.logprobs) == _bits(s.logprobs)
        assert len(e.logprobs) == len(e.tokens)
        assert e.text == g.text == p.text == s.text
        assert e.temperatures == g.temperatures == p.temperatures == s.temperatures \
            == [TEMPS[-1]] * e.windows
        assert e.fallback_attempts == g.fallback_attempts == p.fallback_attempts \
            == s.fallback_attempts == (len(TEMPS) - 1) * e.windows
        assert e.compression_ratios == g.compression_ratios == p.compression_ratios \
            == s.compression_ratios
        assert e.avg_logprob == g.avg_logprob == p.avg_logprob == s.avg_logprob
        assert e.segments == g.segments == p.segments == s.segments
        assert e.no_speech_probs == g.no_speech_probs == p.no_speech_probs == s.no_speech_probs
        if "no_speech" in kw:
            assert len(e.no_speech_probs) == e.windows
        if "timestamps" in kw:
            b = warm.ts_begin
            assert b <= e.tokens[0] <= b + warm.max_initial
            stamps = [t for t in e.tokens if t >= b]
            assert stamps == sorted(stamps)
    assert [r.windows for r in eager] == [1, 1, 1, 2]
    for eng in (warm, frozen):
        assert eng.stats["fallback_windows"] == 5 and eng.stats["fallback_attempts"] == 10
    if kw:
        return
    # another seed draws other tokens; the same seed, the same
    other = _run(mk(), seed=900)
    assert any(a.tokens != b.tokens for a, b in zip(graph, other))
    again = _run(mk(), pipelined=True)
    assert [r.tokens for r in again] == [r.tokens for r in graph]


@pytest.mark.parametrize("kw", [{"token_logprobs": True}, {"timestamps": True}],
                         ids=["plain", "timestamps"])
def test_untriggered_fallback_is_the_greedy_engine_bitwise(weights, kw):
    """Enabled but never triggered: every row runs at temperature 0 through
    ``masked_argmax_kernel<.., 4>`` and gives the feature-off engine's tokens and
    log-probability bits (MODE 1 / MODE 3 there)."""
    on = STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, temperatures=TEMPS,
                   compression_ratio_threshold=float("inf"), logprob_threshold=float("-inf"),
                   **{k: v for k, v in kw.items() if k != "token_logprobs"})
    off = STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, **kw)
    a, b = _run(on, pipelined=True), _run(off, pipelined=True)
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and len(x.tokens) > 0 and x.text == y.text
        assert _bits(x.logprobs) == _bits(y.logprobs) and x.segments == y.segments
        assert x.fallback_attempts == 0 and x.temperatures == [0.0] * x.windows
        assert y.temperatures == []


def test_feature_off_engine_is_the_parent_path(weights, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("masked_argmax_sample with the feature off")
    monkeypatch.setattr(ops, "masked_argmax_sample", boom)
    off = STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights)
    one = STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, temperatures=(0.0,))
    assert off.step_fields == one.step_fields == STTEngine.STEP_FIELDS
    assert not off.fallback and not one.fallback and not one.row_fields
    a, b = _run(off, pipelined=True), _run(one, pipelined=True)
    assert [r.tokens for r in a] == [r.tokens for r in b] and all(r.tokens for r in a)
    assert set(off._graphs) == set(one._graphs)
