"""``STTEngine(beam_size=B)`` on the GPU (``engine/stt_beam.py`` over
``csrc/kernels/beam.hip``), random-init ``test-whisper`` weights: the beams
diverge, so sequences are re-parented and KV blocks copied at every step.

What a copied history must not change is checked by replay: every search step's
``beam_topk`` outputs are recorded (``engine.beam_debug``); then each final
hypothesis is decoded again in a fresh group whose row i is made to follow
hypothesis i with the identity as parents (``STTRequest.beam_force``: no
re-parenting, no copies after the prompt's fork). Row i of the replay and the
recorded ancestor row of hypothesis i saw the same prefix - once through
copied blocks at changing row positions, once in place - so their candidate
lists must agree: ``cand_id`` equal, ``cand_lp`` bit for bit.
"""
import numpy as np
import pytest
import torch
from test_argmax_timestamps_gpu import CFG, _pcms

from loqa_hub_amd.engine.stt_engine import PREV_TOKENS, STTEngine, STTRequest

pytestmark = pytest.mark.gpu
N = 10


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, torch.device("cuda", 0), seed=2)


def _engine(weights, **kw):
    return STTEngine(CFG, "cuda", seed=2, max_batch=12, weights=weights, **kw)


def _bits(xs):
    return np.asarray(xs, np.float32).tobytes()


@pytest.fixture(scope="module")
def recorded(weights):
    """One request decoded alone with three beams, every step recorded."""
    eng = _engine(weights, beam_size=3)
    eng.beam_debug = []
    r = STTRequest(_pcms()[1], max_new_tokens=N)
    eng.transcribe([r])
    torch.cuda.synchronize()
    return eng, r


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_beam_one_is_the_greedy_engine(weights, use_graphs):
    a = [STTRequest(p, max_new_tokens=N) for p in _pcms()]
    b = [STTRequest(p, max_new_tokens=N) for p in _pcms()]
    _engine(weights, token_logprobs=True, use_graphs=use_graphs).transcribe(a)
    eb = _engine(weights, token_logprobs=True, use_graphs=use_graphs, beam_size=1)
    eb.transcribe(b)
    assert eb._beam is None and "beam_windows" not in eb.stats
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and len(x.tokens) > 0
        assert _bits(x.logprobs) == _bits(y.logprobs) and x.text == y.text
        assert x.avg_logprob == y.avg_logprob and y.hypotheses == []


def test_search_moves_kv_and_a_replay_in_place_sees_the_same_rows(weights, recorded):
    eng, r = recorded
    assert eng.stats["beam_kv_copies"] > 2          # more than the prompt's fork
    assert len(r.hypotheses) == 3 and r.tokens == r.hypotheses[0][0]
    assert len({tuple(t) for t, _ in r.hypotheses}) == 3
    steps = [d for d in eng.beam_debug if d["request"] is r]
    assert [d["step"] for d in steps] == list(range(len(steps)))
    rep = _engine(weights, beam_size=3)
    rep.beam_debug = []
    q = STTRequest(_pcms()[1], max_new_tokens=max(len(t) for t, _ in r.hypotheses))
    q.beam_force = [list(t) for t, _ in r.hypotheses]
    rep.transcribe([q])
    torch.cuda.synchronize()
    assert rep.stats["beam_kv_copies"] == 2         # the prompt's fork alone
    replay = rep.beam_debug
    worst, checked = 0.0, 0
    for i, ((tokens, _), trace) in enumerate(zip(r.hypotheses, r.hypothesis_traces)):
        assert len(trace) == len(tokens)
        for t, src in enumerate(trace):
            want_id, want_lp = steps[t]["cand_id"][src], steps[t]["cand_lp"][src]
            row = 0 if t == 0 else i
            got_id, got_lp = replay[t]["cand_id"][row], replay[t]["cand_lp"][row]
            fin = np.isfinite(want_lp) & np.isfinite(got_lp)
            worst = max(worst, float(np.abs(want_lp[fin] - got_lp[fin]).max()))
            assert got_id.tolist() == want_id.tolist(), (i, t)
            assert got_lp.tobytes() == want_lp.tobytes(), (i, t, worst)
            want_e, got_e = steps[t]["eot_lp"][src], replay[t]["eot_lp"][row]
            assert np.float32(want_e).tobytes() == np.float32(got_e).tobytes(), (i, t)
            checked += 1
    print(f"replayed {checked} rows, largest |cand_lp| difference {worst:.3e}")
    assert checked >= 3 * 2


def test_a_group_alone_and_beside_two_others(weights, recorded):
    _, alone = recorded
    eng = _engine(weights, beam_size=3)
    pcms = _pcms()
    reqs = [STTRequest(pcms[0], max_new_tokens=N), STTRequest(pcms[1], max_new_tokens=N),
            STTRequest(pcms[2], max_new_tokens=N)]
    eng.transcribe(reqs)
    torch.cuda.synchronize()
    assert eng.stats["beam_windows"] == 3
    got, want = reqs[1].hypotheses, alone.hypotheses
    print("alone :", want, "\nbeside:", got)
    assert [t for t, _ in got] == [t for t, _ in want]
    assert _bits([s for _, s in got]) == _bits([s for _, s in want])
    assert reqs[1].tokens == alone.tokens and _bits(reqs[1].logprobs) == _bits(alone.logprobs)
    assert eng.kv.pool.free_blocks() == eng.kv.num_blocks


def test_long_form_prompts_the_second_window_with_the_winner(weights):
    eng = _engine(weights, beam_size=3)
    r = STTRequest(_pcms()[3], max_new_tokens=N)
    eng.transcribe([r])
    torch.cuda.synchronize()
    assert r.windows == 2 and len(r.window_hypotheses) == 2 and eng.stats["beam_windows"] == 2
    w0 = [t for t in r.window_hypotheses[0][0][0] if t != eng.eot]
    w1 = [t for t in r.window_hypotheses[1][0][0] if t != eng.eot]
    assert eng.sop is not None and 0 < len(w0) <= PREV_TOKENS
    # the second window's prompt: <|startofprev|>, the first winner's text, the SOT sequence
    assert r.prompt_len == 1 + len(w0) + len(eng.sot)
    assert r.prev_tokens == (w0 + w1)[-PREV_TOKENS:]
    assert r.text == " ".join(filter(None, r.win_texts)) and len(r.win_texts) == 2
    assert r.tokens == r.window_hypotheses[1][0][0]
