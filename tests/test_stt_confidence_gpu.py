"""``STTEngine(token_logprobs=True)`` on the GPU: the captured, pipelined step
(``loqa_masked_argmax_lse`` + ``loqa_step_publish_lp`` as graph nodes) against
the eager-launch fast path. Both run the same kernels on the same inputs and
the chunk records merge in a fixed order, so tokens AND log-probabilities are
compared bitwise; and the feature does not change what is transcribed."""
import math

import numpy as np
import pytest

from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest
from loqa_hub_amd.models.configs import whisper_config

pytestmark = pytest.mark.gpu


def _run(eng, pcms, scheduler=False):
    reqs = [STTRequest(p, max_new_tokens=12) for p in pcms]
    if scheduler:                 # the scheduler thread runs the two-deep STTPipeline
        try:
            eng.submit_batch(reqs).result(timeout=120)
        finally:
            eng.stop()
    else:
        eng.transcribe(reqs)
    return reqs


def test_whisper_logprobs_graphs_match_eager_fast():
    cfg = whisper_config("whisper-tiny")
    rng = np.random.default_rng(1)
    pcms = [(rng.standard_normal(n) * 3000).astype(np.int16) for n in (16000, 48000, 30000)]
    graph = _run(STTEngine(cfg, "cuda", seed=2, max_batch=4, token_logprobs=True), pcms)
    piped = _run(STTEngine(cfg, "cuda", seed=2, max_batch=4, token_logprobs=True), pcms,
                 scheduler=True)
    eager = _run(STTEngine(cfg, "cuda", seed=2, max_batch=4, token_logprobs=True,
                           use_graphs=False), pcms)
    off = _run(STTEngine(cfg, "cuda", seed=2, max_batch=4), pcms)
    for g, p, e, o in zip(graph, piped, eager, off):
        assert g.tokens == e.tokens == p.tokens == o.tokens
        assert len(e.logprobs) == len(e.tokens) > 0
        assert all(math.isfinite(x) and x <= 0.0 for x in e.logprobs)
        # bitwise: the floats came from the same f32 values
        assert g.logprobs == e.logprobs, (g.logprobs, e.logprobs)
        assert p.logprobs == e.logprobs, (p.logprobs, e.logprobs)
        assert g.avg_logprob == e.avg_logprob == p.avg_logprob
        assert o.logprobs == [] and o.avg_logprob is None
