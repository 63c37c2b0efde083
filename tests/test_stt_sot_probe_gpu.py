"""``STTEngine(sot_probe=True)`` on the GPU (``whisper-tiny``, ``max_batch=4``):
the captured synchronous steps, the scheduler's two-deep pipeline (with
captured graphs, and through ``_launch_sync`` when no graph may be captured)
and the eager-launch fast path run ``loqa_masked_argmax_lse_probe`` on the same
inputs - graph nodes publish through ``loqa_step_publish_lp2`` - and its chunk
records merge in a fixed order, so tokens are equal and log-probabilities,
language, its probability and every window's no_speech_prob are compared
bitwise, as in ``test_whisper_logprobs_graphs_match_eager_fast``. With the
probe off the engine launches what the parent launched."""
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
from loqa_hub_amd.engine.stt_pipeline import STTPipeline
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.models.whisper import WhisperWeights

pytestmark = pytest.mark.gpu

CFG = whisper_config("whisper-tiny")


@pytest.fixture(scope="module")
def weights():
    return WhisperWeights(CFG, torch.device("cuda", 0), seed=2)


@pytest.fixture(scope="module")
def pcms():
    """Three utterances of 1 to 3 s and one of 31 s (two windows)."""
    rng = np.random.default_rng(1)
    out = [(rng.standard_normal(n) * 3000).astype(np.int16)
           for n in (16000, 48000, 30000, 31 * 16000)]
    assert len(out[3]) > N_SAMPLES
    return out


def _engine(weights, **kw):
    return STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, **kw)


def _run(eng, pcms, scheduler=False):
    reqs = [STTRequest(p, max_new_tokens=12) for p in pcms]
    if scheduler:                 # the scheduler thread runs the two-deep STTPipeline
        try:
            eng.submit_batch(reqs).result(timeout=120)
        finally:
            eng.stop()
    else:                         # 5 encoder rows > max_batch: two synchronous batches
        eng.transcribe(reqs[:3])
        eng.transcribe(reqs[3:])
    return reqs


@pytest.fixture
def launches(monkeypatch):
    """Every pipelined launch as (step index, speculative, the steps of that
    request still in flight at the launch, its window's SOT step and prompt
    steps), from the pipeline's entries."""
    seen = []
    launch = STTPipeline._launch

    def wrapped(self, live):
        before = [(r, k) for st in self.inflight for r, (k, _) in zip(st.rows, st.entries)]
        n = len(self.inflight)
        ok = launch(self, live)
        if ok and len(self.inflight) > n:
            st = self.inflight[-1]
            for r, (k, sp) in zip(st.rows, st.entries):
                seen.append((k, sp, [k0 for r0, k0 in before if r0 is r], r.sot_step,
                             r.prompt_steps))
        return ok
    monkeypatch.setattr(STTPipeline, "_launch", wrapped)
    return seen


def test_sot_probe_paths_agree(weights, pcms, launches):
    graph = _run(_engine(weights, language="auto"), pcms)
    warm = _engine(weights, language="auto")
    n_graphs = warm.warmup_graphs()
    assert n_graphs > 0 and warm._graphs_frozen
    keys = set(warm._graphs)
    piped = _run(warm, pcms, scheduler=True)
    # after warmup_graphs() the serving run captures nothing
    assert warm._graphs_frozen and set(warm._graphs) == keys
    assert warm.stats["pl_steps"] > 0 and warm.stats["pl_spec"] > 0
    n_piped = len(launches)
    # no graph may be captured: every pipelined step goes through _launch_sync
    frozen = _engine(weights, language="auto")
    frozen._graphs_frozen = True
    synced = _run(frozen, pcms, scheduler=True)
    assert frozen._graphs == {} and frozen.stats["pl_steps"] == 0
    assert frozen.stats["decode_steps"] > 0 and len(launches) > n_piped
    eager = _run(_engine(weights, language="auto", use_graphs=False), pcms)
    for g, p, s, e in zip(graph, piped, synced, eager):
        assert g.tokens == e.tokens == p.tokens == s.tokens
        assert len(e.logprobs) == len(e.tokens) > 0
        assert all(math.isfinite(x) and x <= 0.0 for x in e.logprobs)
        # bitwise: the floats came from the same f32 values
        assert g.logprobs == e.logprobs, (g.logprobs, e.logprobs)
        assert p.logprobs == e.logprobs, (p.logprobs, e.logprobs)
        assert s.logprobs == e.logprobs, (s.logprobs, e.logprobs)
        assert g.avg_logprob == e.avg_logprob == p.avg_logprob == s.avg_logprob
        assert e.language in ("en", "es", "fr", "de")
        assert g.language == p.language == s.language == e.language
        assert g.language_prob == p.language_prob == s.language_prob == e.language_prob
        assert 0.25 <= e.language_prob < 1.0
        assert len(e.no_speech_probs) == e.windows
        assert g.no_speech_probs == p.no_speech_probs == s.no_speech_probs == e.no_speech_probs
        assert all(0.0 < x < 1.0 for x in e.no_speech_probs)
        assert e.no_speech_prob == min(e.no_speech_probs)
        assert g.text == p.text == s.text == e.text
    assert [r.windows for r in eager] == [1, 1, 1, 2]
    # the SOT step is never speculated past: a launch never includes a request
    # whose SOT step is in flight, and only decoded tokens are device-fed
    assert any(sp for _, sp, _, _, _ in launches[:n_piped])
    sot_steps = 0
    for k, sp, inflight, sot_step, prompt_steps in launches:
        assert sot_step >= 0 and sot_step not in inflight, (k, sp, inflight, sot_step)
        assert not (sp and k < prompt_steps)
        assert len(inflight) < STTPipeline.DEPTH
        sot_steps += k == sot_step
    assert sot_steps == 2 * 5              # one per window, in both scheduler runs


class _Counter:
    """Counts the calls of every entry point of the kernel library."""

    def __init__(self, monkeypatch):
        lib = ops._lib.kernels()
        self.n = {}
        for name in ops._lib._KERNEL_SIGS:
            fn = getattr(lib, name)
            self.n[name] = 0
            monkeypatch.setattr(lib, name, self._wrap(name, fn), raising=False)

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            return fn(*a)
        return call


def test_probe_off_launches_what_the_parent_launched(weights, pcms, monkeypatch):
    c = _Counter(monkeypatch)
    off = _engine(weights)
    assert not off.sot_probe and off.io.lp_cols == 0 and off.io.res_lp is None
    reqs = _run(off, pcms)
    # the parent's keys: B = 3 -> 4 rows (fewer once a request has ended), at
    # most 12 tokens -> 16 token rows, context <= 128; the long utterance alone: 1 row
    possible = {(b, 16, 128) for b in (1, 2, 4)}
    assert {(4, 16, 128), (1, 16, 128)} <= set(off._graphs) <= possible
    for k in off._graphs.values():
        assert list(k["layout"].shapes) == list(STTEngine.STEP_FIELDS)
    n = len(off._graphs)
    assert c.n["loqa_masked_argmax_lse_probe"] == 0 and c.n["loqa_step_publish_lp2"] == 0
    assert c.n["loqa_masked_argmax_lse"] == 0 and c.n["loqa_step_publish_lp"] == 0
    # per graph: the warm-up's and the capture's argmax, one fetch and one publish node
    assert c.n["loqa_masked_argmax"] == 2 * n and c.n["loqa_step_publish"] == n
    assert c.n["loqa_step_fetch"] == n
    assert all(r.tokens and r.language is None and r.no_speech_probs == [] for r in reqs)
    lp = _engine(weights, token_logprobs=True)
    _run(lp, pcms[:1])
    assert set(lp._graphs) == {(1, 16, 128)}
    assert c.n["loqa_masked_argmax_lse"] == 2 and c.n["loqa_step_publish_lp"] == 1
    assert c.n["loqa_masked_argmax_lse_probe"] == 0 and c.n["loqa_step_publish_lp2"] == 0
    # the probing engine: the same graph buckets, the new entry points
    before = dict(c.n)
    on = _engine(weights, sot_probe=True)
    got = _run(on, pcms)
    m = len(on._graphs)
    assert {(4, 16, 128), (1, 16, 128)} <= set(on._graphs) <= possible
    assert c.n["loqa_masked_argmax_lse_probe"] == 2 * m and c.n["loqa_step_publish_lp2"] == m
    for name in ("loqa_masked_argmax", "loqa_masked_argmax_lse", "loqa_step_publish",
                 "loqa_step_publish_lp"):
        assert c.n[name] == before[name], name
    for a, b in zip(reqs, got):
        assert b.language == "en" and b.language_prob == 1.0
        assert len(b.no_speech_probs) == b.windows and len(b.logprobs) == len(b.tokens)
