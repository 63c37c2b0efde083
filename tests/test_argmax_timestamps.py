"""Whisper's timestamp rules as a state machine (``ops.masked_argmax_timestamps``;
on the CPU ``ops.reference.masked_argmax_timestamps``), the segment cutter, the
tokenizers' timestamp tokens, the CPU engine with ``timestamps=True`` and the
configuration. The kernel itself is held to this reference in
``tests/test_argmax_timestamps_gpu.py``.

**Rule equivalence.** ``whisper_rules`` below is ``ApplyTimestampRules`` in its
own formulation: it looks at the sampled tokens of the window, not at a state
word. 200 random walks of 24 steps are decoded with it and with the state
machine; the allowed sets and the tokens agree at every step. Both compare in
f32; a walk would only part where the two roundings of one comparison differ,
and the seeded logits hold no such step.

**Decision edges** use logits that are 0, equal small integers or -inf and
allowed sets of 1, 2 or 4 columns, so every ``exp`` is 1 or 0 and every sum a
power of two: the decisions and log-probabilities are exact.
"""
import math
import os

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd import ops
from loqa_hub_amd.engine import stt_segments as seg
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
from loqa_hub_amd.engine.tokenizer import (SyntheticTimestampTokenizer, SyntheticTokenizer,
                                           SyntheticWhisperTokenizer, get_tokenizer)
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref
from loqa_hub_amd.ops.reference import pack_mask

NINF = float("-inf")
V, EOT, TSB, TSC, MAXI = 160, 100, 120, 40, 5


# ------------------------------------------------------------ rule equivalence
def whisper_rules(seq, mask_bits):
    """bool [V]: what ``ApplyTimestampRules`` leaves of ``mask_bits`` after the
    window's sampled tokens ``seq`` (suppression by scanning the history)."""
    ok = mask_bits.clone()
    ok[TSB:TSB + TSC] = True             # the suppress mask does not govern timestamps
    ok[TSB + TSC:] = False
    last_ts = len(seq) >= 1 and seq[-1] >= TSB
    pen_ts = len(seq) < 2 or seq[-2] >= TSB
    if last_ts:
        if pen_ts:
            ok[TSB:] = False             # has to be non-timestamp
        else:
            ok[:EOT] = False             # cannot be normal text tokens
    stamps = [t for t in seq if t >= TSB]
    if stamps:
        # timestamps do not decrease; a closing one may repeat, an opening one may not
        first = stamps[-1] if last_ts and not pen_ts else stamps[-1] + 1
        ok[TSB:first] = False
    if not seq:
        ok[:TSB] = False                 # a window opens with a timestamp ...
        ok[TSB + MAXI + 1:] = False      # ... of at most max_initial
    return ok


def whisper_pick(x, ok):
    """Whisper's sampling of one row after the rules: log-softmax over the
    allowed columns, then the mass rule, then the argmax."""
    lp = torch.log_softmax(x.float().masked_fill(~ok, NINF), dim=-1)
    if ok[TSB:].any() and (not ok[:TSB].any()
                           or torch.logsumexp(lp[TSB:], dim=-1) > lp[:TSB].max()):
        lp[:TSB] = NINF
    return int(lp.argmax())


def machine_allowed(word, ctl, mask_bits):
    text_ok, lo, hi = ref.ts_allowed(word, ctl, TSC, MAXI)
    ok = mask_bits.clone()
    ok[TSB:] = False
    ok[: (TSB, EOT, 0)[text_ok]] = False
    ok[TSB + lo:TSB + hi + 1] = True
    return ok


def well_formed(seq):
    """The first token is a timestamp <= max_initial; timestamps do not
    decrease; never three in a row; a lone timestamp (after text) is followed
    by a timestamp or EOT, a pair by a non-timestamp."""
    assert TSB <= seq[0] <= TSB + MAXI, seq
    stamps = [t for t in seq if t >= TSB]
    assert stamps == sorted(stamps), seq
    for i in range(len(seq)):
        a = seq[i] >= TSB
        b = i >= 1 and seq[i - 1] >= TSB
        c = i >= 2 and seq[i - 2] >= TSB
        assert not (a and b and c), seq
        if i >= 2 and b and not c:           # a lone timestamp closed a segment
            assert seq[i] >= EOT, seq
        if i >= 1 and b and (c or i == 1):   # a pair (or the opening one): text next
            assert not a, seq


def test_state_machine_equals_the_history_rules():
    g = torch.Generator().manual_seed(11)
    W, STEPS = 200, 24
    mask_bits = torch.rand(V, generator=g) < 0.8
    mask_bits[EOT] = True
    mask_bits[EOT + 1:TSB] = False               # the other specials are suppressed
    mask_bits[TSB:] = False                      # the suppress row clears the timestamps
    mask = pack_mask(mask_bits[None])
    rows = torch.zeros(W, dtype=torch.int32)
    probe = torch.full((W,), -1, dtype=torch.int32)
    slot = torch.arange(W, dtype=torch.int32)
    state = torch.full((W + 1,), 12345, dtype=torch.int32)   # garbage: ctl 1 ignores it
    seqs = [[] for _ in range(W)]
    for step in range(STEPS):
        x = torch.randn(W, V, generator=g) * 3
        x[:, TSB:] += 2.0                     # so that text and timestamps both win often
        ctl = torch.full((W,), 1 if step == 0 else 2, dtype=torch.int32)
        before = state.clone()
        idx, lp, _ = ref.masked_argmax_timestamps(x, mask, rows, probe, ctl, state, slot, TSB, TSC,
                                                  EOT, MAXI)
        for w in range(W):
            ok = whisper_rules(seqs[w], mask_bits)
            assert torch.equal(ok, machine_allowed(int(before[w]), int(ctl[w]), mask_bits)), \
                (step, w, seqs[w])
            assert ok.any()
            t = whisper_pick(x[w], ok)
            assert t == int(idx[w]), (step, w, seqs[w], t, int(idx[w]))
            seqs[w].append(t)
            assert int(state[w]) == ref.ts_state_next(int(before[w]), int(ctl[w]), t, TSB)
            assert math.isfinite(float(lp[w])) and float(lp[w]) <= 0.0
    for s in seqs:
        well_formed(s)
    n_ts = sum(t >= TSB for s in seqs for t in s)
    assert 0.2 < n_ts / (W * STEPS) < 0.8        # both kinds are sampled
    assert any(t == EOT for s in seqs for t in s)
    assert int(state[W]) == 12345                # no row pointed at the last slot


def test_state_word_round_trip():
    for last in (-1, 0, 7, 1500):
        for f_last in (False, True):
            for f_pen in (False, True):
                w = ref.ts_state_pack(last, f_last, f_pen)
                assert ref.ts_state_unpack(w) == (last, f_last, f_pen)
    assert ref.ts_allowed(999, 1, 40, 50) == (0, 0, 39)          # max_initial is clamped
    assert ref.ts_allowed(ref.ts_state_pack(7, True, True), 2, 40, 5) == (2, 40, 39)
    assert ref.ts_allowed(ref.ts_state_pack(7, True, False), 2, 40, 5) == (1, 7, 39)
    assert ref.ts_allowed(ref.ts_state_pack(7, False, True), 2, 40, 5) == (2, 8, 39)
    assert ref.ts_allowed(ref.ts_state_pack(-1, False, False), 2, 40, 5) == (2, 0, 39)
    assert ref.ts_allowed(ref.ts_state_pack(39, False, False), 2, 40, 5) == (2, 40, 39)


# -------------------------------------------------------------- decision edges
def edge_cases():
    """(name, logits row [V], mask bits [V], state word, ctl, want idx, want lp,
    want next word or None = unchanged). Logits 0 / 3 / -inf, all exact."""
    text = ref.ts_state_pack(2, False, False)        # text allowed, timestamps from 3
    out = []
    mb = torch.zeros(V, dtype=torch.bool)
    mb[[10, 20, EOT]] = True
    hot = torch.full((V,), NINF)
    # one allowed timestamp equal to the best text logit: an exact tie, text wins
    x = hot.clone()
    x[[10, TSB + 3]] = 0.0
    out.append(("tie", x, mb, text, 2, 10, -math.log(2.0), ref.ts_state_pack(2, False, False)))
    # two such timestamps: their mass is twice the text token's
    x = hot.clone()
    x[[10, TSB + 3, TSB + 9]] = 0.0
    out.append(("two", x, mb, text, 2, TSB + 3, -math.log(2.0), ref.ts_state_pack(3, True, False)))
    # timestamps below ``lo`` do not count: the tie again
    x = hot.clone()
    x[[10, TSB + 2, TSB + 3]] = 0.0
    out.append(("below_lo", x, mb, text, 2, 10, -math.log(2.0), ref.ts_state_pack(2, False, False)))
    # nothing allowed below ts_begin (the window's first token): the rule fires
    x = torch.zeros(V)
    x[10] = 3.0
    x[TSB + MAXI + 1:] = 3.0                         # past max_initial: not allowed
    x[TSB:TSB + 2] = NINF                            # 4 of the 6 initial ones stay
    out.append(("first", x, mb, 777, 1, TSB + 2, -math.log(4.0), ref.ts_state_pack(2, True, True)))
    # no timestamp allowed (a closed pair): text, even under a huge timestamp
    x = hot.clone()
    x[[10, 20]] = 0.0
    x[TSB:] = 3.0
    pair = ref.ts_state_pack(4, True, True)
    out.append(("no_ts", x, mb, pair, 2, 10, -math.log(2.0), ref.ts_state_pack(4, False, True)))
    # a lone timestamp: EOT or a timestamp, text is out
    x = hot.clone()
    x[[10, 20]] = 3.0
    x[EOT] = 0.0
    lone = ref.ts_state_pack(4, True, False)
    out.append(("eot", x, mb, lone, 2, EOT, 0.0, ref.ts_state_pack(4, False, True)))
    # nothing allowed at all: (-1, -inf), the state stays
    none = torch.zeros(V, dtype=torch.bool)
    none[TSB:] = True                                # timestamps ignore their mask bits
    out.append(("none", torch.zeros(V), none, pair, 2, -1, NINF, None))
    return out


def run_edges(dev, dtype=torch.float32):
    cases = edge_cases()
    B = len(cases)
    x = torch.stack([c[1] for c in cases]).to(dtype).to(dev)
    mask = pack_mask(torch.stack([c[2] for c in cases])).to(dev)
    state = torch.tensor([c[3] for c in cases] + [4242], dtype=torch.int32, device=dev)
    ctl = torch.tensor([c[4] for c in cases], dtype=torch.int32, device=dev)
    slot = torch.arange(B, dtype=torch.int32, device=dev)
    probe = torch.full((B,), -1, dtype=torch.int32, device=dev)
    idx, lp, plp = ops.masked_argmax_timestamps(x, mask, None, probe, ctl, state, slot, TSB, TSC,
                                                EOT, MAXI)
    for i, (name, _, _, word, _, want, want_lp, nxt) in enumerate(cases):
        assert int(idx[i]) == want, (name, int(idx[i]), want)
        got = float(lp[i])
        # bitwise: the f32 nearest to the exact value (log 2 and log 4 = 2 log 2)
        assert got == float(np.float32(want_lp)), (name, got, want_lp)
        assert int(state[i]) == (word if nxt is None else nxt), (name, int(state[i]), nxt)
    assert int(state[B]) == 4242 and plp.tolist() == [0.0] * B


def test_decision_edges():
    run_edges("cpu")


# --------------------------------------------------------------- rule-off rows
def test_rule_off_rows_are_the_probe_op_bitwise():
    g = torch.Generator().manual_seed(3)
    B = 5
    x = torch.randn(B, V, generator=g) * 4
    bits = torch.rand(B, V, generator=g) < 0.5
    mask = pack_mask(bits)
    probe = torch.tensor([-1, 3, 150, -1, 0], dtype=torch.int32)
    ctl = torch.tensor([0, 0, 0, 1, 0], dtype=torch.int32)
    state = torch.full((B + 1,), 99, dtype=torch.int32)
    slot = torch.arange(B, dtype=torch.int32)
    a = ops.masked_argmax_timestamps(x, mask, None, probe, ctl, state, slot, TSB, TSC, EOT, MAXI)
    b = ops.masked_argmax_logprob_probe(x, mask, None, probe)
    keep = ctl == 0
    assert torch.equal(a[0][keep], b[0][keep])
    for u, w in zip(a[1:], b[1:]):
        assert torch.equal(u[keep].view(torch.int32), w[keep].view(torch.int32))
    assert TSB <= int(a[0][3]) <= TSB + MAXI
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))   # the probe ignores rules
    assert state.tolist() == [99, 99, 99, ref.ts_state_pack(int(a[0][3]) - TSB, True, True), 99, 99]


def test_wrapper_checks():
    x = torch.zeros(2, V)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    state = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(AssertionError, match="share a state slot"):
        ops.masked_argmax_timestamps(x, None, None, i32(-1, -1), i32(2, 2), state, i32(1, 1),
                                     TSB, TSC, EOT, MAXI)
    ops.masked_argmax_timestamps(x, None, None, i32(-1, -1), i32(2, 0), state, i32(1, 1),
                                 TSB, TSC, EOT, MAXI)
    for bad in ((TSB, TSC + 1, EOT), (TSB, TSC, TSB + 1), (TSB, 0, EOT)):
        with pytest.raises(ValueError, match="timestamp layout"):
            ops.masked_argmax_timestamps(x, None, None, i32(-1, -1), i32(0, 0), state, i32(0, 1),
                                         bad[0], bad[1], bad[2], MAXI)


# ----------------------------------------------------------------- stt_segments
def test_segments():
    B = 1000
    ts = lambda s: B + round(s / 0.02)
    E = 999
    # pairs: <0.00> a b <1.00><1.00> c <2.50><2.50> (an empty last segment is dropped)
    s = seg.cut_window([ts(0), 1, 2, ts(1), ts(1), 3, ts(2.5), ts(2.5), E], B, E)
    assert [(x.start_s, x.end_s, x.tokens, x.open) for x in s] == \
        [(0.0, 1.0, [1, 2], False), (1.0, 2.5, [3], False)]
    # a trailing single timestamp closes the last segment
    s = seg.cut_window([ts(0.2), 1, ts(1), ts(1.5), 2, ts(3)], B, E)
    assert [(x.start_s, x.end_s, x.tokens, x.open) for x in s] == \
        [(0.2, 1.0, [1], False), (1.5, 3.0, [2], False)]
    # an open tail runs to the window's end
    s = seg.cut_window([ts(0), 1, ts(1), ts(1), 2, 3], B, E)
    assert [(x.start_s, x.end_s, x.tokens, x.open) for x in s] == \
        [(0.0, 1.0, [1], False), (1.0, 30.0, [2, 3], True)]
    # empty segments: <0.00><0.00>? never sampled, but <0.50> EOT and a pair without text are
    assert seg.cut_window([ts(0.5), E], B, E) == []
    assert seg.cut_window([ts(0), 1, ts(1), ts(2), ts(2), 2, ts(4)], B, E)[1].start_s == 2.0
    assert seg.cut_window([], B, E) == []
    assert seg.text_tokens([ts(0), 1, ts(1), E, 2], B, E) == [1, 2]
    # utterance time: window offset, the clamp to the duration, blank text dropped
    dec = lambda t: "".join(" w%d" % i if i != 9 else " " for i in t)
    s = seg.cut_window([ts(0), 1, ts(1), ts(1), 9, ts(2), ts(2), 2], B, E)
    assert seg.utterance_segments(s, 0, 40.0, dec) == [(0.0, 1.0, "w1"), (2.0, 30.0, "w2")]
    assert seg.utterance_segments(s, 1, 31.5, dec) == [(30.0, 31.0, "w1"), (31.5, 31.5, "w2")]
    for a, b, _ in seg.utterance_segments(s, 1, 30.5, dec):
        assert 30.0 <= a <= b <= 30.5


# -------------------------------------------------------------------- tokenizers
def test_synthetic_timestamp_tokens():
    base = get_tokenizer(4096)
    assert isinstance(base, SyntheticTokenizer)
    tok = SyntheticTimestampTokenizer(SyntheticWhisperTokenizer(base))
    b, n = tok.timestamp_tokens()
    assert (b, n) == (4096 - 1501, 1501)
    assert tok.token_id("<|0.00|>") == b and tok.token_id("<|30.00|>") == 4095
    assert tok.token_id("<|0.02|>") == b + 1 and tok.token_id("<|endoftext|>") == b - 1
    assert tok.token_id("<|nospeech|>") == base.n_real and tok.token_id("<|en|>") == 4
    with pytest.raises(KeyError):
        tok.token_id("<|30.02|>")
    with pytest.raises(KeyError):
        tok.token_id("<|0.01|>")
    ids = base.encode(" turn on the lights")
    assert tok.decode([b] + ids + [b + 50, b - 1]) == " turn on the lights"
    assert tok.decode(ids + [b + 3], skip_from=b) == " turn on the lights"
    # a small vocabulary: as many as fit, at least 11
    small = SyntheticTimestampTokenizer(SyntheticTokenizer(base.n_real + 31))
    assert small.timestamp_tokens() == (base.n_real + 1, 30)
    with pytest.raises(ValueError, match="timestamp"):
        SyntheticTimestampTokenizer(SyntheticTokenizer(base.n_real + 11))
    # the base tokenizer is untouched
    assert base.token_id("<|endoftext|>") == 7 and base.decode([b, b - 1]) == ""


HF_SPECIALS = ["<|endoftext|>", "<|startoftranscript|>", "<|en|>", "<|translate|>",
               "<|transcribe|>", "<|startofprev|>", "<|nospeech|>", "<|notimestamps|>"]
STAMPS = [f"<|{k * 0.02:.2f}|>" for k in range(11)]      # <|0.00|> .. <|0.20|>


def _hf_tokenizer(path, added):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers
    corpus = ["turn on the kitchen lights and play music in the bedroom",
              "turn off the tv then dim the living room lamp", "hello what time is it"] * 20
    t = Tokenizer(models.BPE())
    t.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    t.decoder = decoders.ByteLevel()
    t.train_from_iterator(corpus, trainers.BpeTrainer(
        vocab_size=500, special_tokens=[], initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    t.add_special_tokens(list(added))        # Whisper's layout: the specials come last
    os.makedirs(path, exist_ok=True)
    t.save(os.path.join(path, "tokenizer.json"))
    return os.path.join(path, "tokenizer.json")


def test_hf_timestamp_tokens(tmp_path):
    pytest.importorskip("tokenizers")
    from loqa_hub_amd.engine.tokenizer import load_tokenizer
    tok = load_tokenizer(_hf_tokenizer(str(tmp_path / "a"), HF_SPECIALS + STAMPS), 4096)
    b, n = tok.timestamp_tokens()
    assert n == 11 and b == tok.token_id("<|0.00|>") and b + n == tok.n_real
    assert tok.token_id("<|0.20|>") == b + 10 and tok.token_id("<|endoftext|>") < b
    ids = tok.encode(" turn on the lights")
    assert tok.decode([b] + ids + [b + 4], skip_from=b) == " turn on the lights"
    gap = HF_SPECIALS + STAMPS[:5] + STAMPS[6:]
    with pytest.raises(ValueError, match="contiguous"):
        load_tokenizer(_hf_tokenizer(str(tmp_path / "b"), gap), 4096).timestamp_tokens()
    with pytest.raises(ValueError, match="last tokens"):
        load_tokenizer(_hf_tokenizer(str(tmp_path / "c"), HF_SPECIALS[:-1] + STAMPS
                                     + HF_SPECIALS[-1:]), 4096).timestamp_tokens()
    with pytest.raises(ValueError, match="0.00"):
        load_tokenizer(_hf_tokenizer(str(tmp_path / "d"), HF_SPECIALS), 4096).timestamp_tokens()
    # an engine on the file's tokens: the rules' layout comes from the tokenizer
    eng = STTEngine(whisper_config("test-whisper"), torch.device("cpu"), seed=0, max_batch=2,
                    tokenizer=tok, timestamps=True)
    assert (eng.ts_begin, eng.ts_count, eng.max_initial) == (b, 11, 10)
    assert eng.sot == [tok.token_id(s) for s in
                       ("<|startoftranscript|>", "<|en|>", "<|transcribe|>")]
    rng = np.random.default_rng(1)
    r = STTRequest((rng.standard_normal(16000) * 3000).astype(np.int16), max_new_tokens=8)
    eng.transcribe([r])
    assert b <= r.tokens[0] < b + 11
    assert all(t <= eng.eot or t >= b for t in r.tokens)     # <|endoftext|> is the first special


# ---------------------------------------------------------------- engine, CPU
CFG = whisper_config("test-whisper")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, CPU, seed=0)


def _pcms():
    rng = np.random.default_rng(1)
    return [(rng.standard_normal(n) * 3000).astype(np.int16)
            for n in (16000, 48000, 31 * 16000)]


def _engine(weights, **kw):
    return STTEngine(CFG, CPU, seed=0, max_batch=4, weights=weights, **kw)


def _well_formed_window(toks, eng):
    b, eot = eng.ts_begin, eng.eot
    body = toks[:-1] if toks[-1] == eot else toks
    assert eot not in body
    assert b <= toks[0] <= b + eng.max_initial
    stamps = [t for t in body if t >= b]
    assert stamps == sorted(stamps) and all(t < b + eng.ts_count for t in stamps)
    for i in range(len(toks)):
        a = toks[i] >= b
        p = i >= 1 and toks[i - 1] >= b
        q = i >= 2 and toks[i - 2] >= b
        assert not (a and p and q)
        if i >= 2 and p and not q:
            assert toks[i] >= eot
        if i >= 1 and p and (q or i == 1):
            assert not a


@pytest.mark.parametrize("kw", [{}, {"language": "auto", "no_speech": True}],
                         ids=["plain", "probing"])
def test_engine_free_decoding(weights, kw, monkeypatch):
    eng = _engine(weights, timestamps=True, **kw)
    assert eng.timestamps and eng.token_logprobs and eng.sot_probe == bool(kw)
    assert len(eng.sot) == 3 and eng.tok.token_id("<|notimestamps|>") not in eng.sot
    assert eng.step_fields == STTEngine.STEP_FIELDS[:8] + ("mask_row", "probe", "ts_ctl") + \
        STTEngine.STEP_FIELDS[8:]
    assert eng.ts_state.shape == (5,) and eng.max_initial == 50
    windows = []
    finish = STTEngine._finish

    def tap(self, r):
        windows.append((r, r.win, list(r.tokens)))
        return finish(self, r)
    monkeypatch.setattr(STTEngine, "_finish", tap)
    reqs = [STTRequest(p, max_new_tokens=14) for p in _pcms()]
    eng.transcribe(reqs)
    assert [r.windows for r in reqs] == [1, 1, 2] and len(windows) == 4
    for r, w, toks in windows:
        _well_formed_window(toks, eng)
    for r, n in zip(reqs, (16000, 48000, 31 * 16000)):
        dur = n / 16000
        assert r.segments and len(r.logprobs) == len(r.tokens)
        for a, b, text in r.segments:
            assert 0.0 <= a <= b <= dur and text and "<|" not in text
        assert r.text == " ".join(t for _, _, t in r.segments) and "<|" not in r.text
        assert r.speech_start_s == r.segments[0][0] and r.speech_end_s == r.segments[-1][1]
        assert all(t < eng.eot for t in r.prev_tokens)
        assert set(r.open_segments) <= set(range(r.windows))
        assert math.isfinite(r.avg_logprob)
    if kw:
        # the post-SOT chunk drops <|notimestamps|> too
        assert reqs[0].chunks[-1] == [reqs[0].lang_id, eng.tok.token_id("<|transcribe|>")]
    # the 31 s request: two windows, the second's times offset by 30 s
    long = reqs[2]
    second = [s for s in long.segments if s[0] >= 30.0]
    assert second and all(30.0 <= a <= b <= 31.0 for a, b, _ in second)
    dec = lambda t: eng.tok.decode(t)
    want = []
    for w in (0, 1):
        toks = [toks for r, w_, toks in windows if r is long and w_ == w][0]
        want.append(seg.utterance_segments(seg.cut_window(toks, eng.ts_begin, eng.eot), w, 31.0,
                                           dec))
    assert long.segments == want[0] + want[1] and second == want[1]
    # the same tokens in window 0 would lie 30 s earlier (before the clamp to 31 s)
    toks = [toks for r, w_, toks in windows if r is long and w_ == 1][0]
    early = seg.utterance_segments(seg.cut_window(toks, eng.ts_begin, eng.eot), 0, 31.0, dec)
    assert [(min(a + 30.0, 31.0), min(b + 30.0, 31.0), t) for a, b, t in early] == second
    assert eng.stats["timestamp_segments"] == sum(len(r.segments) for r in reqs)
    assert eng.stats["open_segments"] == sum(len(r.open_segments) for r in reqs)
    # the scheduler thread takes the same steps
    monkeypatch.setattr(STTEngine, "_finish", finish)
    sched = _engine(weights, timestamps=True, **kw)
    again = [STTRequest(p, max_new_tokens=14) for p in _pcms()]
    try:
        sched.submit_batch(again).result(timeout=300)
    finally:
        sched.stop()
    for a, b in zip(reqs, again):
        assert a.tokens == b.tokens and a.logprobs == b.logprobs and a.segments == b.segments
        assert a.text == b.text and a.avg_logprob == b.avg_logprob


def test_teacher_forced_is_unchanged(weights):
    texts = ["turn on the kitchen lights", "play music in the bedroom"]
    outs = []
    for ts in (False, True):
        eng = _engine(weights, timestamps=ts)
        reqs = [STTRequest(p, transcript=t) for p, t in zip(_pcms(), texts)]
        eng.transcribe(reqs)
        outs.append((eng, reqs))
    (off, a), (on, b) = outs
    for x, y in zip(a, b):
        assert x.text == y.text and x.text
        # the targets are the same text tokens, closed by each engine's own EOT
        assert x.tokens[:-1] == y.tokens[:-1] and x.tokens[-1] == off.eot and y.tokens[-1] == on.eot
        assert y.segments == [] and y.logprobs == [] and x.segments is None
    assert on.ts_state.tolist() == [0] * 5       # teacher-forced rows run with the rules off


def test_timestamps_off_is_the_parent(weights, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("masked_argmax_timestamps with the feature off")
    monkeypatch.setattr(ops, "masked_argmax_timestamps", boom)
    off = _engine(weights)
    assert not off.timestamps and not off.row_fields and not hasattr(off, "ts_state")
    assert off.step_fields == STTEngine.STEP_FIELDS and len(off.sot) == 4
    assert off.sot[-1] == off.tok.token_id("<|notimestamps|>") and off.eot == 7
    assert "timestamp_segments" not in off.stats
    lay = off._layout(4, 16)
    assert list(lay.shapes) == list(STTEngine.STEP_FIELDS)
    assert lay.n32 == STTEngine.step_layout(4, 16, off.max_blocks).n32
    probing = _engine(weights, sot_probe=True)
    assert probing.step_fields == STTEngine.STEP_FIELDS[:8] + ("mask_row", "probe") + \
        STTEngine.STEP_FIELDS[8:]
    # the parent's greedy decode of the same seed: argmax of the eager decoder's logits
    pcm = _pcms()[0]
    r = STTRequest(pcm, max_new_tokens=6)
    off.transcribe([r])
    assert r.segments is None and r.speech_start_s is None and r.open_segments is None
    want = _parent_greedy(_engine(weights, fast_decode=False), pcm, 6)
    assert r.tokens == want and len(want) > 0


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


def test_constructor_errors(weights):
    with pytest.raises(ValueError, match="max_initial_timestamp"):
        _engine(weights, timestamps=True, max_initial_timestamp=31.0)
    eng = _engine(weights, timestamps=True, max_initial_timestamp=0.0)
    assert eng.max_initial == 0
    r = STTRequest(_pcms()[0], max_new_tokens=3)
    eng.transcribe([r])
    assert r.tokens[0] == eng.ts_begin


# ---------------------------------------------------------------------- config
def test_config_and_result():
    g = cfgmod.load({})
    assert (g.gpu.stt_timestamps, g.gpu.stt_max_initial_timestamp) == ("off", 1.0)
    c = cfgmod.load({"HUB_STT_TIMESTAMPS": " Segment ", "HUB_STT_MAX_INITIAL_TIMESTAMP": "0.5"})
    assert (c.gpu.stt_timestamps, c.gpu.stt_max_initial_timestamp) == ("segment", 0.5)
    for bad in ("on", "word", "1"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_TIMESTAMPS"):
            cfgmod.load({"HUB_STT_TIMESTAMPS": bad})
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BACKEND=gpu"):
        cfgmod.load({"HUB_STT_TIMESTAMPS": "segment", "HUB_STT_BACKEND": "http"})
    for bad in ("-0.1", "30.5", "nan", "late"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_MAX_INITIAL_TIMESTAMP"):
            cfgmod.load({"HUB_STT_MAX_INITIAL_TIMESTAMP": bad})
    from loqa_hub_amd.llm.transcriber import TranscriptionResult, to_transcription_result
    t = TranscriptionResult()
    assert t.segments is None and t.speech_start_s is None and t.speech_end_s is None
    segs = [(0.2, 1.0, "hey loqa"), (1.0, 2.5, "lights on")]
    t = to_transcription_result("hey loqa lights on", segments=segs, speech_start_s=0.2,
                                speech_end_s=2.5)
    assert (t.segments, t.speech_start_s, t.speech_end_s) == (segs, 0.2, 2.5)
    assert t.wake_word_detected and t.text == "lights on"


def test_pipeline_and_metrics_carry_the_segments(weights):
    from types import SimpleNamespace as NS

    from loqa_hub_amd.api.metrics import MetricsHandler
    from loqa_hub_amd.engine.pipeline import PipelineJob, VoicePipeline
    eng = _engine(weights, timestamps=True)
    r = STTRequest(_pcms()[0], max_new_tokens=8)
    eng.transcribe([r])
    j = PipelineJob("relay", "req", r.pcm)
    VoicePipeline._stt_post(NS(stt_acoustic=False, stt_confirm_below=0.6), j, r)
    assert j.segments == r.segments and j.open_segments == r.open_segments
    assert j.transcription.segments == r.segments
    assert j.transcription.speech_start_s == r.speech_start_s
    assert j.transcription.avg_logprob is None
    proc = NS(stats={}, pipeline=NS(llm=NS(stats={}), stt=eng))
    text = "\n".join(MetricsHandler(NS(audio_service=None, skills=None, processor=proc,
                                       nats=None)).collect())
    assert f"loqa_stt_timestamp_segments {len(r.segments)}" in text
    assert f"loqa_stt_open_segments {len(r.open_segments)}" in text
