"""The Whisper start-of-transcript probe on the CPU engine
(``STTEngine(sot_probe=True)``, ``whisper-tiny``, random-init weights, the
synthetic tokenizer with its Whisper-only extension): prompt chunking, the
detected language, Whisper's ``no_speech_prob``, the no-speech rule and its way
up to the hub's answer.

The values are compared with fp64 computed from the logits of the
start-of-transcript row, taken from ``WhisperModel.decode_step`` (the eager
decoder, which the engine under test runs as well, ``fast_decode=False``):

* ``language`` is the fp64 argmax over the candidate language logits,
  ``language_prob`` is within 1e-5 of the fp64 softmax over them;
* ``log(no_speech_prob)`` is within the bound of ``tests/test_argmax_probe.py``
  (one workgroup row of f32 logits wider than 8192: ``6u * depth + 4R u +
  4u ln V + (4R + ln V) u`` with ``R`` the largest |logit| of the row), which
  the CPU reference is held to there as well.

The random-init model gives every window a ``no_speech_prob`` near 1 / V and a
mean token log-probability near -ln V, so the gating cases take their
thresholds from the values the test's own fixed-seed requests measure.
"""
import asyncio
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd import ops
from loqa_hub_amd.engine import stt_engine as stt_mod
from loqa_hub_amd.engine.step_io import DEV
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
from loqa_hub_amd.engine.stt_pipeline import STTPipeline
from loqa_hub_amd.engine.tokenizer import WHISPER_PROBE_TOKENS, get_tokenizer
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.models.whisper import WhisperWeights
from loqa_hub_amd.transport.voice_processor import MSG_NO_SPEECH

CPU = torch.device("cpu")
CFG = whisper_config("whisper-tiny")
U = 2.0 ** -24
CHUNK, THREADS = 8192, 256
FIELDS = ("tokens", "positions", "slots", "cu_q", "ctx_lens", "block_tables",
          "enc_starts", "enc_lens", "src", "row_slot")


def probe_bound(V: int, R: float) -> float:
    """tests/test_argmax_probe.py's bound for f32 logits, |x| <= R."""
    n_t = 4 * math.ceil(min(V, CHUNK) / (THREADS * 4))
    depth = n_t + n_t // 4 + 6 + 3 + math.ceil(V / CHUNK) - 1
    return 6 * U * depth + 4 * R * U + 4 * U * math.log(V) + (4 * R + math.log(V)) * U


def _pcms(seed=1, lens=(16000, 48000, 30000)):
    """The utterances of tests/test_stt_confidence_gpu.py."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 3000).astype(np.int16) for n in lens]


@pytest.fixture(scope="module")
def weights():
    return WhisperWeights(CFG, CPU, seed=2)


def _engine(weights, **kw):
    return STTEngine(CFG, CPU, seed=2, max_batch=4, weights=weights, **kw)


def _tap(eng):
    """Every ``WhisperModel.decode_step`` result of ``eng`` (fp64 copies)."""
    seen = []
    step = eng.model.decode_step
    eng.model.decode_step = lambda *a, **k: (lambda x: (seen.append(x.detach().double().clone()), x)[1])(
        step(*a, **k))
    return seen


# ------------------------------------------------------------------ tokenizer
def test_synthetic_extension_leaves_the_base_tokenizer_alone(weights):
    base = get_tokenizer(CFG.vocab_size)
    n_real, strings = base.n_real, list(base.strings)
    eng = _engine(weights, language="auto")
    assert get_tokenizer(CFG.vocab_size) is base and base.n_real == n_real
    assert base.strings == strings
    ids = [eng.tok.token_id(s) for s in WHISPER_PROBE_TOKENS]
    assert ids == list(range(n_real, n_real + 4))            # the first reserved filler ids
    assert all(base.strings[i].startswith("<|reserved_") for i in ids)
    with pytest.raises(KeyError):
        base.token_id("<|nospeech|>")
    assert eng.nospeech == n_real
    assert eng.lang_codes == ["en", "es", "fr", "de"]
    assert eng.lang_ids == [base.token_id("<|en|>")] + ids[1:]
    assert eng.tok.encode(" turn on the lights") == base.encode(" turn on the lights")
    assert eng.tok.decode(ids + base.encode("hey loqa")) == "hey loqa"
    off = _engine(weights)
    assert off.tok is base and not off.sot_probe


def test_constructor_flags(weights):
    assert not _engine(weights).token_logprobs
    for kw in ({"sot_probe": True}, {"language": "auto"}, {"language": ""}, {"no_speech": True}):
        eng = _engine(weights, **kw)
        assert eng.sot_probe and eng.token_logprobs, kw
    assert _engine(weights, language="").auto_language
    assert _engine(weights, language="AUTO").auto_language
    assert not _engine(weights, no_speech=True).auto_language
    assert _engine(weights, language="auto", languages=["fr", "en"]).lang_codes == ["en", "fr"]
    assert _engine(weights, language="fr", sot_probe=True).lang_codes == ["fr"]
    for kw in ({"language": "xx"}, {"language": "xx", "sot_probe": True},
               {"language": "auto", "languages": ["en", "xx"]},
               {"language": "fr"}):                   # no <|fr|> without the extension
        with pytest.raises(ValueError, match="language"):
            _engine(weights, **kw)


# ------------------------------------------------------------ prompt chunking
def test_prompt_chunking(weights):
    on, off = _engine(weights, language="auto"), _engine(weights)
    c = len(on.sot)
    assert c == 4 and on.n_prompt_tokens_per_step == 4
    sot_tok = on.sot[0]
    for eng in (on, off):
        for n_prev in range(0, 41):
            r = STTRequest(np.zeros(16, np.int16), max_new_tokens=4)
            r.slots, r.windows = [0, 1], 2
            r.prev_tokens = list(range(100, 100 + n_prev))
            eng._begin_window(r, 1 if n_prev else 0)
            eng.kv.pool.free_seq(r.seq_id)
            prev = r.prev_tokens[-stt_mod.PREV_TOKENS:]
            prefix = ([eng.sop] + prev) if n_prev else []
            flat = [t for ch in r.chunks for t in ch]
            assert all(1 <= len(ch) <= c for ch in r.chunks)
            if eng is off:          # the parent's stride-4 slices of prefix + the 4 SOT tokens
                assert flat == prefix + eng.sot == r.feed
                assert r.chunks == [r.feed[i:i + c] for i in range(0, len(r.feed), c)]
                assert r.prompt_steps == len(r.chunks) == -(-len(r.feed) // c)
                assert r.sot_step == -1 and not r.sot_pending
                continue
            assert flat == prefix + [sot_tok] == r.feed
            assert r.chunks[-1][-1] == sot_tok                 # SOT ends a chunk ...
            assert sot_tok not in flat[:-1]                    # ... and no chunk crosses it
            assert r.sot_step == len(r.chunks) - 1 and r.sot_pending
            assert r.prompt_steps == len(r.chunks) + 1
            # what follows SOT is a host-known chunk, fed once the SOT step retired
            post = eng._sot_result(r, eng.lang_ids[1], -0.5, -3.0)
            assert post == [eng.lang_ids[1]] + eng.sot[2:] and DEV not in post
            assert r.chunks[-1] == post and len(r.chunks) == r.prompt_steps
            assert not r.sot_pending and r.language == "es"
            assert r.language_prob == pytest.approx(math.exp(-0.5))
            assert r.no_speech_probs == [pytest.approx(math.exp(-3.0))]


def test_pipeline_feed_waits_for_the_sot_step(weights):
    """``STTPipeline._feed`` (host logic only): the prompt chunks in order, no
    feed while the SOT step is in flight, then the host-known chunk, then the
    decoded tokens."""
    eng = _engine(weights, sot_probe=True)
    pl = STTPipeline(eng)
    r = STTRequest(np.zeros(16, np.int16), max_new_tokens=4)
    r.slots, r.windows, r.prev_tokens = [0, 1], 2, list(range(100, 109))
    eng._begin_window(r, 1)
    pl.admit(r)
    n_pre = len(r.chunks)
    assert n_pre == 3                                  # sop + 9 previous + SOT = 11 tokens
    for k in range(n_pre):
        assert pl._feed(r) == (r.chunks[k], False)
        r.pl_launched += 1
        r.pl_fl += 1
    assert r.pl_launched - 1 == r.sot_step
    assert pl._feed(r) is None                         # the SOT step is in flight
    r.pl_fl = 0
    assert pl._feed(r) is None                         # ... or retired but not read yet
    post = eng._sot_result(r, eng.lang_ids[0], 0.0, -1.0)
    assert pl._feed(r) == (post, False)
    r.pl_launched += 1
    r.pl_fl += 1
    assert r.pl_launched == r.prompt_steps
    assert pl._feed(r) == ([DEV], True)                # greedy: fed from the device
    eng.kv.pool.free_seq(r.seq_id)


# ------------------------------------------------------------------- language
def _sot_row_oracle(eng, logits):
    """fp64 from the SOT row: (candidate index, softmax over the candidates,
    log softmax of <|nospeech|> over the whole vocabulary, largest |logit|)."""
    row = logits[0]
    cand = row[eng.lang_ids]
    return (int(cand.argmax()), torch.softmax(cand, dim=0),
            float(torch.log_softmax(row, dim=0)[eng.nospeech]), float(row.abs().max()))


@pytest.mark.parametrize("i", [0, 1, 2])
def test_language_and_no_speech_value_against_fp64(weights, i):
    pcm = _pcms()[i]
    eng = _engine(weights, language="auto", fast_decode=False)
    seen = _tap(eng)
    r = STTRequest(pcm, max_new_tokens=3)
    eng.transcribe([r])
    assert seen[0].shape == (1, CFG.vocab_size)       # the step that fed [SOT] alone
    k, p, want_lns, R = _sot_row_oracle(eng, seen[0])
    assert r.language == eng.lang_codes[k] and r.lang_id == eng.lang_ids[k]
    assert abs(r.language_prob - float(p[k])) <= 1e-5
    assert 0.25 <= r.language_prob < 1.0
    assert eng.stats["languages"] == {r.language: 1}
    # the token fed after SOT is the detected language's
    assert r.chunks == [[eng.sot[0]], [r.lang_id] + eng.sot[2:]]
    assert len(r.no_speech_probs) == 1 and r.no_speech_prob == r.no_speech_probs[0]
    err = abs(math.log(r.no_speech_prob) - want_lns)
    print(f"lang {r.language} p {r.language_prob:.6f}  no_speech {r.no_speech_prob:.4e}  "
          f"log err {err:.3e}  bound {probe_bound(CFG.vocab_size, R):.3e}  R {R:.2f}")
    assert err <= probe_bound(CFG.vocab_size, R)
    # a single candidate: probability exactly 1, and <|es|> follows SOT
    one = _engine(weights, language="auto", languages=["es"], fast_decode=False)
    q = STTRequest(pcm, max_new_tokens=3)
    one.transcribe([q])
    assert q.language == "es" and q.language_prob == 1.0
    assert q.chunks[-1][0] == one.tok.token_id("<|es|>") == q.lang_id
    assert q.no_speech_probs == r.no_speech_probs     # the same SOT row, the same probe


def test_paths_agree_on_the_cpu(weights):
    """transcribe() and the scheduler thread take the same steps on the same
    decoder: the same values, bit for bit (the eager decoder is held to fp64
    above)."""
    runs = []
    for sched in (False, True):
        eng = _engine(weights, language="auto")
        reqs = [STTRequest(p, max_new_tokens=6) for p in _pcms()]
        if sched:
            try:
                eng.submit_batch(reqs).result(timeout=300)
            finally:
                eng.stop()
        else:
            eng.transcribe(reqs)
        runs.append(reqs)
    for a, c in zip(*runs):
        assert a.language == c.language and a.language in ("en", "es", "fr", "de")
        assert a.tokens == c.tokens and a.logprobs == c.logprobs and len(a.tokens) > 0
        assert a.no_speech_probs == c.no_speech_probs and a.language_prob == c.language_prob
        assert a.avg_logprob == c.avg_logprob


# --------------------------------------------------------------------- gating
@pytest.fixture(scope="module")
def measured(weights):
    """The test's requests decoded freely without gating: (no_speech_prob,
    mean token log-probability, tokens, text) of each."""
    eng = _engine(weights, sot_probe=True)
    reqs = [STTRequest(p, max_new_tokens=8) for p in _pcms()]
    eng.transcribe(reqs)
    assert all(r.tokens and len(r.logprobs) == len(r.tokens) for r in reqs)
    return [(r.no_speech_prob, r.avg_logprob, list(r.tokens), r.text) for r in reqs]


def test_gated_window(weights, measured):
    nsp = min(m[0] for m in measured)
    lo, hi = min(m[1] for m in measured), max(m[1] for m in measured)
    assert nsp > 0 and hi < 0
    # both conditions hold for every request
    eng = _engine(weights, no_speech=True, no_speech_threshold=nsp / 2, logprob_threshold=hi / 2)
    reqs = [STTRequest(p, max_new_tokens=8) for p in _pcms()]
    eng.transcribe(reqs)
    for r, m in zip(reqs, measured):
        assert r.tokens == m[2] and r.no_speech_prob == m[0]       # decoded as ever ...
        assert r.text == "" and r.gated_windows == 1               # ... and dropped
        assert r.avg_logprob is None and r.lp_n == 0               # the window is excluded
    assert eng.stats["no_speech_windows"] == 3 and eng.stats["no_speech_utterances"] == 3
    assert eng.stats["logprob_tokens"] == 0 and eng.stats["utterances"] == 3


def test_probability_condition_alone_keeps_the_text(weights, measured):
    nsp = min(m[0] for m in measured)
    lo = min(m[1] for m in measured)
    eng = _engine(weights, no_speech=True, no_speech_threshold=nsp / 2, logprob_threshold=2 * lo)
    reqs = [STTRequest(p, max_new_tokens=8) for p in _pcms()]
    eng.transcribe(reqs)
    for r, m in zip(reqs, measured):
        assert r.no_speech_prob > eng.no_speech_threshold and r.avg_logprob > eng.logprob_threshold
        assert (r.tokens, r.text, r.avg_logprob) == (m[2], m[3], m[1]) and r.gated_windows == 0
    assert eng.stats["no_speech_windows"] == eng.stats["no_speech_utterances"] == 0
    # the log-probability condition alone: kept as well
    nsp_hi = max(m[0] for m in measured)
    eng = _engine(weights, no_speech=True, no_speech_threshold=min(1.0, 2 * nsp_hi),
                  logprob_threshold=max(m[1] for m in measured) / 2)
    reqs = [STTRequest(p, max_new_tokens=8) for p in _pcms()]
    eng.transcribe(reqs)
    assert [r.text for r in reqs] == [m[3] for m in measured]
    assert eng.stats["no_speech_windows"] == 0


def test_teacher_forced_requests_are_never_gated(weights):
    eng = _engine(weights, no_speech=True, no_speech_threshold=1e-9, logprob_threshold=0.0)
    text = "turn on the kitchen lights"
    forced = STTRequest(_pcms()[0], transcript=text)
    free = STTRequest(_pcms()[1], max_new_tokens=4)
    eng.transcribe([forced, free])
    assert forced.text == text and forced.gated_windows == 0 and forced.avg_logprob is None
    assert forced.language == "en" and forced.language_prob == 1.0
    assert len(forced.no_speech_probs) == 1 and 0 < forced.no_speech_prob < 1     # recorded
    assert free.text == "" and free.gated_windows == 1
    assert eng.stats["no_speech_windows"] == 1 and eng.stats["no_speech_utterances"] == 1
    # the same steps as a request without the probe: the same forced tokens
    off = _engine(weights)
    plain = STTRequest(_pcms()[0], transcript=text)
    off.transcribe([plain])
    assert plain.tokens == forced.tokens and plain.text == forced.text


# ------------------------------------------------------------------ long-form
def _windows_of(eng, monkeypatch):
    """Record (tokens, logprobs, prev_tokens at the window's start, lang fed)
    of every finished window of ``eng``."""
    out, starts = [], []
    finish, begin = eng._finish, eng._begin_window
    monkeypatch.setattr(eng, "_begin_window",
                        lambda r, w: (starts.append(list(r.prev_tokens)), begin(r, w))[1])
    monkeypatch.setattr(eng, "_finish", lambda r: (
        out.append((list(r.tokens), list(r.logprobs), starts[-1], r.chunks[-1][0])), finish(r))[1])
    return out


def test_long_form_first_window_gated(weights, monkeypatch):
    rng = np.random.default_rng(8)      # window 1's mean log-probability is the lower by 0.18
    pcm = (rng.standard_normal(31 * 16000) * 3000).astype(np.int16)
    assert len(pcm) > N_SAMPLES
    # measure both windows as the gated run decodes them: window 2 without a
    # previous-text prompt (a gated window leaves none)
    monkeypatch.setattr(stt_mod, "PREV_TOKENS", 0)
    eng = _engine(weights, language="auto")
    wins = _windows_of(eng, monkeypatch)
    r = STTRequest(pcm, max_new_tokens=5)
    eng.transcribe([r])
    assert r.windows == 2 and len(wins) == 2 and len(r.no_speech_probs) == 2
    means = [float(np.mean(np.asarray(w[1], np.float64))) for w in wins]
    nsps = list(r.no_speech_probs)
    monkeypatch.undo()
    # thresholds that gate window 1 alone: by the log-probability if it is the
    # lower one, else by the no-speech probability
    if means[0] < means[1]:
        kw = dict(no_speech_threshold=min(nsps) / 2, logprob_threshold=(means[0] + means[1]) / 2)
    else:
        assert nsps[0] > nsps[1], "pick another seed: window 1 cannot be gated alone"
        kw = dict(no_speech_threshold=(nsps[0] + nsps[1]) / 2, logprob_threshold=max(means) / 2)
    eng = _engine(weights, language="auto", no_speech=True, **kw)
    assert stt_mod.PREV_TOKENS > 0
    got = _windows_of(eng, monkeypatch)
    q = STTRequest(pcm, max_new_tokens=5)
    eng.transcribe([q])
    assert q.windows == 2 and q.gated_windows == 1
    assert eng.stats["no_speech_windows"] == 1 and eng.stats["no_speech_utterances"] == 0
    assert eng.stats["long_form_windows"] == 1
    assert got[0][0] == wins[0][0] and got[1][0] == wins[1][0]         # decoded as measured
    assert q.win_texts[0] == "" and q.win_texts[1] == eng.tok.decode(
        [t for t in got[1][0] if t != eng.eot]).strip()
    assert q.text == q.win_texts[1]                                     # window 2 is kept
    assert got[1][2] == []                                              # no previous text
    assert q.no_speech_probs == nsps and q.no_speech_prob == min(nsps)
    assert got[0][3] == got[1][3] == q.lang_id                          # window 0's language
    assert eng.stats["languages"] == {q.language: 1}
    # the utterance's avg_logprob: window 2 alone
    assert q.avg_logprob == pytest.approx(means[1], abs=1e-12) and q.lp_n == len(got[1][1])


# ------------------------------------------------------------------ probe off
def test_probe_off_layout_is_the_parents():
    assert STTEngine.STEP_FIELDS == FIELDS
    for B_pad, T_pad, mb in ((1, 16, 28), (4, 16, 3), (8, 32, 28), (128, 128, 2)):
        lay = STTEngine.step_layout(B_pad, T_pad, mb)
        sizes = [T_pad, T_pad, T_pad, B_pad + 1, B_pad, B_pad * mb, B_pad, B_pad, T_pad, B_pad]
        assert list(lay.shapes) == list(FIELDS)
        assert [lay.offsets[f] for f in FIELDS] == [sum(sizes[:i]) for i in range(len(sizes))]
        assert lay.n32 == sum(sizes) and lay.n64 == max(16, ops.mpad_for(B_pad))
        assert lay.src_off == lay.offsets["src"]


def test_probing_layout_is_the_instances(weights):
    on, off = _engine(weights, sot_probe=True), _engine(weights)
    assert off.step_fields == FIELDS and on.STEP_FIELDS == FIELDS
    assert on.step_fields == FIELDS[:8] + ("mask_row", "probe") + FIELDS[8:]
    lay, base = on._layout(4, 16), off._layout(4, 16)
    assert list(base.shapes) == list(FIELDS) and base.n32 == STTEngine.step_layout(4, 16, off.max_blocks).n32
    assert lay.shapes["mask_row"] == lay.shapes["probe"] == (4,)
    assert lay.n32 == base.n32 + 8 and lay.n64 == base.n64
    # staged per step: the SOT row gets (1, nospeech), every other row (0, -1)
    a, b = STTRequest(np.zeros(16, np.int16)), STTRequest(np.zeros(16, np.int16))
    for r in (a, b):
        r.slots = [0]
        on._begin_window(r, 0)
    on._sot_result(b, on.lang_ids[0], 0.0, -1.0)
    b.feed = b.chunks[-1]
    _, host = on._host_meta([a, b], 4, 16)
    assert host["mask_row"].tolist() == [1, 0, 0, 0]
    assert host["probe"].tolist() == [on.nospeech, -1, -1, -1]
    for r in (a, b):
        on.kv.pool.free_seq(r.seq_id)


def _parent_greedy(eng, pcm, n):
    """The parent's decode of one request, written out: the 4-token SOT prompt
    in one step, then one sampled token per step (argmax of decode_step)."""
    r = STTRequest(pcm, max_new_tokens=n)
    eng._admit([r], [0])
    r.feed = list(eng.sot)
    toks = []
    while len(toks) < n:
        t = int(eng._eager_step([r])[0])
        toks.append(t)
        if t == eng.eot:
            break
        r.feed = [t]
    eng.kv.pool.free_seq(r.seq_id)
    return toks


def test_probe_off_tokens_and_calls_are_the_parents(weights, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("masked_argmax_logprob_probe called without the probe")
    monkeypatch.setattr(ops, "masked_argmax_logprob_probe", boom)
    off = _engine(weights, fast_decode=False)
    reqs = [STTRequest(p, max_new_tokens=12) for p in _pcms()]
    off.transcribe(reqs)
    ref = _engine(weights, fast_decode=False)
    for r, p in zip(reqs, _pcms()):
        assert r.chunks == [off.sot] and r.prompt_steps == 1
        assert r.tokens == _parent_greedy(ref, p, 12)
        assert r.language is None and r.no_speech_prob is None and r.no_speech_probs == []
    assert "no_speech_windows" not in off.stats and "languages" not in off.stats
    on = _engine(weights, sot_probe=True)
    with pytest.raises(AssertionError, match="masked_argmax_logprob_probe called"):
        on.transcribe([STTRequest(_pcms()[0], max_new_tokens=2)])


def test_probe_on_decodes_the_same_tokens(weights):
    """Fixed ``en``: SOT in a step of its own, then [en, transcribe,
    notimestamps] - the same prompt as the parent's single 4-token step, so
    the same greedy tokens. The steps' logits differ in rounding only; every
    step's top-two margin is far above that, so the equality is not luck."""
    for pcm in _pcms():
        off, on = _engine(weights, fast_decode=False), _engine(weights, sot_probe=True,
                                                               fast_decode=False)
        seen_off, seen_on = _tap(off), _tap(on)
        a, b = STTRequest(pcm, max_new_tokens=12), STTRequest(pcm, max_new_tokens=12)
        off.transcribe([a])
        on.transcribe([b])
        assert len(seen_on) == len(seen_off) + 1          # the SOT step
        assert b.language == "en" and b.language_prob == 1.0
        for x, y in zip(seen_off, seen_on[1:]):
            top = x[0].topk(2).values
            margin = float(top[0] - top[1])
            assert margin > 1e-3, margin
            assert float((x - y).abs().max()) < margin / 10
        assert a.tokens == b.tokens and len(b.logprobs) == len(b.tokens)


# ------------------------------------------------------------------ hub level
def _serve(tmp_path, **env):
    """One utterance without a transcript hint through the hub's voice
    processor (``server.build_gpu_processor`` on the CPU engines)."""
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
                                     pcm16=_pcms(7, (24000,))[0])
            return res, proc.job_sink[0], dict(proc.stats), proc.pipeline, built
        finally:
            if proc is not None:
                await proc.close()
            await nats.close()
            await broker.stop()
    return asyncio.run(go())


def test_served_gated_utterance_is_no_speech(tmp_path):
    # the random-init model: no_speech_prob ~ 1 / V > 1e-9, mean log-probability < -0.5
    res, job, stats, pipe, built = _serve(
        tmp_path, HUB_STT_NO_SPEECH="on", HUB_STT_NO_SPEECH_THRESHOLD="1e-9",
        HUB_STT_LOGPROB_THRESHOLD="-0.5", STT_LANGUAGE="auto", HUB_STT_LANGUAGES="fr,de")
    stt = pipe.stt
    assert stt.sot_probe and stt.no_speech and stt.auto_language and stt.lang_codes == ["fr", "de"]
    assert (stt.no_speech_threshold, stt.logprob_threshold) == (1e-9, -0.5)
    assert res.command == "no_speech" and res.response_text == MSG_NO_SPEECH and not res.success
    assert job.raw_text == "" and job.no_speech and job.transcription.text == ""
    assert built == [None]                                   # no LLM request ...
    assert pipe.llm.stats["decode_steps"] == 0 and pipe.llm.stats["prefill_tokens"] == 0
    assert stats["stt_no_speech"] == 1 and stats["utterances"] == 1
    assert stt.stats["no_speech_windows"] == stt.stats["no_speech_utterances"] == 1
    m, tr = res.metrics["stt"], job.transcription
    assert m["language"] == tr.language and tr.language in ("fr", "de")
    assert m["language_prob"] == tr.language_prob and 0.5 <= tr.language_prob < 1.0
    assert m["no_speech_prob"] == tr.no_speech_prob and 1e-9 < tr.no_speech_prob < 1.0
    assert stt.stats["languages"] == {tr.language: 1}


def test_served_kept_utterance_is_unchanged(tmp_path):
    base, bjob, bstats, bpipe, _ = _serve(tmp_path)
    assert not bpipe.stt.sot_probe and bstats["stt_no_speech"] == 0
    assert set(base.metrics["stt"]) == {"confidence", "avg_logprob"}
    res, job, stats, pipe, built = _serve(
        tmp_path, HUB_STT_NO_SPEECH="on", HUB_STT_NO_SPEECH_THRESHOLD="1e-9",
        HUB_STT_LOGPROB_THRESHOLD="-1000")
    assert pipe.stt.sot_probe and pipe.stt.lang_codes == ["en"]
    assert stats["stt_no_speech"] == 0 and pipe.stt.stats["no_speech_windows"] == 0
    assert job.raw_text == bjob.raw_text != "" and not job.no_speech
    assert (res.command, res.intents, res.transcription) == \
        (base.command, base.intents, base.transcription)
    assert len(built) == 1 and built[0] is not None
    assert res.metrics["stt"]["language"] == "en" and res.metrics["stt"]["language_prob"] == 1.0


# --------------------------------------------------------------------- config
def test_config():
    g = cfgmod.load({})
    assert g.stt.language == "en" and g.gpu.stt_languages == []
    assert (g.gpu.stt_no_speech, g.gpu.stt_no_speech_threshold, g.gpu.stt_logprob_threshold) == \
        ("off", 0.6, -1.0)
    for v in ("auto", "AUTO", "", "  "):
        assert cfgmod.load({"STT_LANGUAGE": v}).stt.language == "auto", v
    assert cfgmod.load({"STT_LANGUAGE": "es"}).stt.language == "es"
    c = cfgmod.load({"STT_LANGUAGE": "auto", "HUB_STT_LANGUAGES": " en, ES ,fr,",
                     "HUB_STT_NO_SPEECH": "On", "HUB_STT_NO_SPEECH_THRESHOLD": "1",
                     "HUB_STT_LOGPROB_THRESHOLD": "0"})
    assert c.gpu.stt_languages == ["en", "es", "fr"] and c.gpu.stt_no_speech == "on"
    assert (c.gpu.stt_no_speech_threshold, c.gpu.stt_logprob_threshold) == (1.0, 0.0)
    for bad in ("0", "-0.1", "1.01", "nan", "loud"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_NO_SPEECH_THRESHOLD"):
            cfgmod.load({"HUB_STT_NO_SPEECH_THRESHOLD": bad})
    for bad in ("0.1", "nan", "low"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_LOGPROB_THRESHOLD"):
            cfgmod.load({"HUB_STT_LOGPROB_THRESHOLD": bad})
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_NO_SPEECH"):
        cfgmod.load({"HUB_STT_NO_SPEECH": "maybe"})
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_LANGUAGES"):
        cfgmod.load({"HUB_STT_LANGUAGES": "en,english"})
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BACKEND=gpu"):
        cfgmod.load({"HUB_STT_NO_SPEECH": "on", "HUB_STT_BACKEND": "http"})
    # detection with an external STT service: the reference's pass-through
    c = cfgmod.load({"STT_LANGUAGE": "", "HUB_STT_BACKEND": "http"})
    assert c.stt.language == "auto"
    from loqa_hub_amd.llm.stt_client import STTClient
    assert STTClient("http://stt:8000", c.stt.language, client=object()).language == ""
    assert STTClient("http://stt:8000", "es", client=object()).language == "es"
    assert STTClient("http://stt:8000", "", client=object()).language == "en"


def test_metrics_export_the_new_counters():
    from types import SimpleNamespace as NS

    from loqa_hub_amd.api.metrics import MetricsHandler
    stt = NS(stats={"utterances": 3, "no_speech_windows": 2, "no_speech_utterances": 1,
                    "languages": {"en": 2, "de": 1}})
    proc = NS(stats={"utterances": 3, "stt_no_speech": 1},
              pipeline=NS(llm=NS(stats={"decode_steps": 7}), stt=stt))
    srv = NS(audio_service=None, skills=None, processor=proc, nats=None)
    text = "\n".join(MetricsHandler(srv).collect())
    for want in ("loqa_processor_stt_no_speech_total 1", "loqa_stt_no_speech_windows 2",
                 "loqa_stt_no_speech_utterances 1", 'loqa_stt_languages{language="de"} 1',
                 'loqa_stt_languages{language="en"} 2', "loqa_llm_decode_steps 7"):
        assert want in text, (want, text)
