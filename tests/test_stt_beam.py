"""Beam search in the STT engine (``STTEngine(beam_size=B)``,
``engine/stt_beam.py``) on the CPU engines, the configuration key
``HUB_STT_BEAM_SIZE`` and the hub's confidence from the winner.

The random-init ``test-whisper`` weights with the synthetic tokenizer decode
arbitrary tokens: the beams diverge, so every step re-parents sequences and
copies KV blocks.
"""
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref
from test_stt_confidence import _serve

CFG = whisper_config("test-whisper")
CPU = torch.device("cpu")
N = 8


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, CPU, seed=2)


def _pcms():
    rng = np.random.default_rng(1)
    return [(rng.standard_normal(n) * 3000).astype(np.int16) for n in (16000, 48000, 31 * 16000)]


def _engine(weights, **kw):
    return STTEngine(CFG, CPU, seed=2, max_batch=12, weights=weights, **kw)


@pytest.fixture(scope="module")
def beam_run(weights):
    eng = _engine(weights, beam_size=3)
    reqs = [STTRequest(p, max_new_tokens=N) for p in _pcms()]
    eng.transcribe(reqs)
    return eng, reqs


def _score(tokens, s, eot):
    return s / max(1, sum(1 for t in tokens if t != eot))


def test_hypotheses_are_sorted_and_complete(beam_run):
    eng, reqs = beam_run
    assert eng.stats["beam_windows"] == sum(r.windows for r in reqs) == 4
    assert eng.stats["beam_kv_copies"] > 0
    for r in reqs:
        assert r.beam_size == 3 and len(r.window_hypotheses) == r.windows
        assert r.hypotheses is r.window_hypotheses[-1]
        for hyps in r.window_hypotheses:
            assert len(hyps) == 3 and len({tuple(t) for t, _ in hyps}) == 3
            scores = [_score(t, s, eng.eot) for t, s in hyps]
            assert scores == sorted(scores, reverse=True)
            for t, s in hyps:
                assert 0 < len(t) <= N and math.isfinite(s) and s < 0
                assert eng.eot not in t[:-1]
                assert t[-1] == eng.eot or len(t) == N      # finished, or cut at max_new_tokens
        # the winner is the request's result
        tokens, s = r.hypotheses[0]
        assert r.tokens == tokens and len(r.logprobs) == len(tokens)
        assert sum(r.logprobs) == pytest.approx(s, abs=1e-4)
        assert r.text == " ".join(filter(None, r.win_texts))
    assert eng.kv.pool.free_blocks() == eng.kv.num_blocks     # every beam's blocks came back


def test_avg_logprob_is_the_winners(beam_run):
    eng, reqs = beam_run
    for r in reqs:
        total = sum(hyps[0][1] for hyps in r.window_hypotheses)
        n = sum(len(hyps[0][0]) for hyps in r.window_hypotheses)
        assert r.avg_logprob == pytest.approx(total / n, abs=1e-5)
    assert eng.stats["logprob_tokens"] == sum(
        len(h[0][0]) for r in reqs for h in r.window_hypotheses)


def test_beam_finds_no_worse_a_sum_than_greedy(weights, beam_run):
    """Greedy's path is one of the candidates: unless the search pruned it,
    the best hypothesis by sum scores at least greedy's sum. On these windows
    it does (a regression guard for the selection, not a theorem)."""
    _, reqs = beam_run
    greedy = [STTRequest(p, max_new_tokens=N) for p in _pcms()[:2]]
    _engine(weights, token_logprobs=True).transcribe(greedy)
    for r, q in zip(reqs, greedy):
        assert max(s for _, s in r.hypotheses) >= sum(q.logprobs) - 1e-4


def test_beam_one_is_the_greedy_engine(weights):
    a = [STTRequest(p, max_new_tokens=N) for p in _pcms()]
    b = [STTRequest(p, max_new_tokens=N) for p in _pcms()]
    ea, eb = _engine(weights, token_logprobs=True), _engine(weights, token_logprobs=True, beam_size=1)
    ea.transcribe(a)
    eb.transcribe(b)
    assert eb._beam is None and "beam_windows" not in eb.stats
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and x.logprobs == y.logprobs and x.text == y.text
        assert y.hypotheses == [] and y.beam_size == 1


def test_engine_follows_the_reference_search(weights):
    """The engine's search over the real decoder equals ``ref.beam_search``
    over a step function that runs the reference decoder on the same prefix."""
    eng = _engine(weights, beam_size=3)
    eng.beam_debug = []
    r = STTRequest(_pcms()[0], max_new_tokens=5)
    eng.transcribe([r])
    steps = [d for d in eng.beam_debug if d["request"] is r]
    assert [d["step"] for d in steps] == list(range(len(steps))) and 1 <= len(steps) <= 5
    assert steps[0]["cand_id"].shape == (1, 3) and all(d["cand_id"].shape == (3, 3) for d in steps[1:])
    # replay the recorded rows through the host model of the search
    st = ref.BeamState(3, eng.eot, 5)
    for d in steps:
        out = ref.beam_merge(torch.from_numpy(d["cand_id"]), torch.from_numpy(d["cand_lp"]),
                             torch.from_numpy(d["eot_lp"]), torch.from_numpy(st.cum)[None], st.n_src)
        st.advance(*(o[0].numpy() for o in out), d["eot_lp"])
    hyps, w = st.result()
    assert st.done and r.tokens == hyps[w][0]
    assert sorted(map(tuple, (t for t, _ in r.hypotheses))) == sorted(tuple(t) for t, _, _ in hyps)


def test_teacher_forced_requests_use_one_row(weights):
    eng = _engine(weights, beam_size=3)
    forced = STTRequest(_pcms()[0], transcript="turn on the lights", max_new_tokens=N)
    free = STTRequest(_pcms()[1], max_new_tokens=N)
    eng.transcribe([forced, free])
    assert forced.text == "turn on the lights" and forced.hypotheses == [] and forced.beam_size == 1
    assert forced.logprobs == [] and forced.avg_logprob is None
    assert len(free.hypotheses) == 3 and eng.stats["beam_windows"] == 1


def test_scheduler_matches_transcribe(weights, beam_run):
    _, want = beam_run
    eng = _engine(weights, beam_size=3)
    reqs = [STTRequest(p, max_new_tokens=N) for p in _pcms()]
    try:
        eng.submit_batch(reqs).result(timeout=120)
    finally:
        eng.stop()
    for r, q in zip(reqs, want):
        assert r.tokens == q.tokens and r.window_hypotheses == q.window_hypotheses


def test_probing_engine_with_beams(weights):
    eng = _engine(weights, beam_size=2, language="auto", no_speech=True)
    reqs = [STTRequest(p, max_new_tokens=6) for p in _pcms()[:2]]
    eng.transcribe(reqs)
    for r in reqs:
        assert r.language is not None and len(r.no_speech_probs) == 1
        assert len(r.hypotheses) == 2 and r.tokens == r.hypotheses[0][0]


def test_constructor_rejects_what_beams_do_not_carry(weights):
    for kw in ({"timestamps": True}, {"word_timestamps": True}, {"temperatures": (0.0, 0.5)}):
        with pytest.raises(ValueError, match="beam_size"):
            _engine(weights, beam_size=2, **kw)
    for b in (0, 9):
        with pytest.raises(ValueError, match="beam_size"):
            _engine(weights, beam_size=b)
    assert _engine(weights, beam_size=4).max_slots == 3


def test_config_parsing_and_rejected_combinations():
    assert cfgmod.load({}).gpu.stt_beam_size == 1
    assert cfgmod.load({"HUB_STT_BEAM_SIZE": " 5 "}).gpu.stt_beam_size == 5
    assert cfgmod.load({"HUB_STT_BEAM_SIZE": "1", "HUB_STT_BACKEND": "http"}).gpu.stt_beam_size == 1
    assert cfgmod.load({"HUB_STT_BEAM_SIZE": "1", "HUB_STT_TIMESTAMPS": "segment"}).gpu.stt_beam_size == 1
    for bad in ("0", "9", "-2", "five", "2.5"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BEAM_SIZE"):
            cfgmod.load({"HUB_STT_BEAM_SIZE": bad})
    for env, what in (({"HUB_STT_BACKEND": "http"}, "HUB_STT_BACKEND=gpu"),
                      ({"HUB_STT_TIMESTAMPS": "segment"}, "HUB_STT_TIMESTAMPS"),
                      ({"HUB_STT_WORD_TIMESTAMPS": "on"}, "HUB_STT_WORD_TIMESTAMPS"),
                      ({"HUB_STT_TEMPERATURE": "0,0.5"}, "HUB_STT_TEMPERATURE"),
                      ({"HUB_MAX_BATCH": "2"}, "HUB_MAX_BATCH")):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BEAM_SIZE") as ei:
            cfgmod.load({"HUB_STT_BEAM_SIZE": "3", **env})
        assert what in str(ei.value)
    cfgmod.load({"HUB_STT_BEAM_SIZE": "3", "HUB_STT_TEMPERATURE": "0"})


def test_served_confidence_comes_from_the_winner(tmp_path):
    res, job, stats, stt = _serve(tmp_path, HUB_STT_CONFIDENCE="acoustic", HUB_STT_BEAM_SIZE="3",
                                  HUB_STT_CONFIRM_BELOW="0.0")
    assert stt.beam_size == 3 and stt.stats["beam_windows"] == 1 and stt.stats["beam_kv_copies"] > 0
    tr = job.transcription
    assert tr.avg_logprob is not None and tr.avg_logprob < 0.0
    m = res.metrics["stt"]
    assert m["avg_logprob"] == tr.avg_logprob and m["confidence"] == math.exp(tr.avg_logprob)
    # the same utterance through a second engine of the same seed: the hub's
    # figure is the winner's sum over its tokens
    r = STTRequest(__import__("test_stt_confidence")._pcms(7, (24000,))[0])
    STTEngine(CFG, CPU, seed=0, max_batch=4, beam_size=3).transcribe([r])
    tokens, s = r.hypotheses[0]
    assert tr.avg_logprob == pytest.approx(s / len(tokens), abs=1e-5)
    assert r.avg_logprob == pytest.approx(tr.avg_logprob, abs=1e-6)
