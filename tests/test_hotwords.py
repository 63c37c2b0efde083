"""Hotword biasing of the STT engine on the CPU: the Aho-Corasick compile
(``engine/hotwords.py``), its flattened device form against the chain-walking
reference (``ops.reference.hotword_advance`` / ``hotword_boosted``), the step
(``ops.hotword_step``, whose CPU path is the reference), the engine with a
scripted decoder, and the configuration.

Toy tokenizers: ``_words`` gives word w the id 2 * index (at the start of the
text) or 2 * index + 1 (after a space), so the two variants of a phrase differ
in their first token only; ``_ints`` reads a phrase of numbers as its token ids.
"""
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import config as cfgmod
from loqa_hub_amd import ops
from loqa_hub_amd.engine.hotwords import compile_hotwords
from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref

WORDS = ["living", "room", "lamp", "fan", "hue", "iris", "pantry", "sonos"]


def _words(text):
    out, first = [], not text.startswith(" ")
    for w in text.split():
        out.append(2 * WORDS.index(w) + (0 if first else 1))
        first = False
    return out


def _ints(text):
    return [int(x) for x in text.split()]


def sp(w):      # the id of " w"
    return 2 * WORDS.index(w) + 1


def st(w):      # the id of "w" at the start
    return 2 * WORDS.index(w)


# ---------------------------------------------------------------------- compile
def test_compile_variants_duplicates_and_bfs():
    a = compile_hotwords(["living room lamp", "  room   fan ", "room fan", ""], 2.0, _words, 16)
    assert a.phrases == ["living room lamp", "room fan"]
    assert a.sequences == [(sp("living"), sp("room"), sp("lamp")), (st("living"), sp("room"), sp("lamp")),
                           (sp("room"), sp("fan")), (st("room"), sp("fan"))]
    # breadth-first, children in ascending token order, root 0
    assert list(a.edges[0]) == sorted(a.edges[0]) == [st("living"), sp("living"), st("room"), sp("room")]
    assert [a.edges[0][t] for t in sorted(a.edges[0])] == [1, 2, 3, 4]
    depth = {0: 0}
    for n in range(a.N):
        for c in a.edges[n].values():
            depth[c] = depth[n] + 1
    assert [depth[n] for n in range(a.N)] == sorted(depth[n] for n in range(a.N))
    assert a.N == 1 + 4 + 4 + 2 and a.fail[0] == 0
    # a tokenizer that ignores the leading space: the two variants collapse
    b = compile_hotwords(["3 4", "3 4", "5"], 1.0, _ints, 16)
    assert b.sequences == [(3, 4), (5,)] and b.N == 4
    assert b.header().tolist()[:2] == [b.N, b.T]
    assert np.int32(b.header()[2]).view(np.float32) == np.float32(1.0)


def test_failure_links_of_a_nested_suffix():
    a = compile_hotwords(["living room lamp", "room fan"], 2.0, _words, 16)
    n = 0
    for w in ("living", "room"):
        n = ref.hotword_advance(a, n, sp(w))
    assert n and a.fail[n] == a.edges[0][sp("room")] and a.chain(n) == [n, a.fail[n], 0]
    boosted = ref.hotword_boosted(a, n)
    assert sp("lamp") in boosted and sp("fan") in boosted and set(a.edges[0]) <= boosted
    assert a.boosted_flat(n) == boosted
    # the suffix takes over when the longer phrase breaks off
    m = ref.hotword_advance(a, n, sp("fan"))
    assert a.terminal[m] == (1,) and a.advance_flat(n, sp("fan")) == m
    assert a.matches([sp("living"), sp("room"), sp("fan")]) == [1]
    assert a.matches([st("living"), sp("room"), sp("lamp"), sp("room"), sp("fan")]) == [0, 1]
    assert a.matches([sp("room"), sp("lamp")]) == []
    for k in range(a.N):
        tk, _ = a.span(k)
        assert list(tk) == sorted(set(tk.tolist()))


def test_limits_raise_naming_the_phrase():
    ok = [f"{i} {i + 1}" for i in range(ref.HOTWORD_MAX_PHRASES)]
    compile_hotwords(ok, 1.0, _ints, 5000)
    with pytest.raises(ValueError, match="1024"):
        compile_hotwords(ok + ["4000 4001"], 1.0, _ints, 5000)
    long = " ".join(str(i) for i in range(ref.HOTWORD_MAX_TOKENS + 1))
    compile_hotwords([long[: long.rindex(" ")]], 1.0, _ints, 64)
    with pytest.raises(ValueError, match="0 1 2 3.*16"):
        compile_hotwords(["7", long], 1.0, _ints, 64)
    with pytest.raises(ValueError, match="'7 99'.*99"):
        compile_hotwords(["7 99"], 1.0, _ints, 99)
    with pytest.raises(ValueError, match="'-3'"):
        compile_hotwords(["-3"], 1.0, _ints, 99)
    for bad in (math.inf, -math.inf, math.nan, 1e39, "loud", None):
        with pytest.raises(ValueError, match="boost"):
            compile_hotwords(["7"], bad, _ints, 99)
    with pytest.raises(ValueError, match="list"):
        compile_hotwords("7 8", 1.0, _ints, 99)
    assert compile_hotwords([], 1.0, _ints, 99).T == 0


def test_table_capacity_raises(monkeypatch):
    import loqa_hub_amd.engine.hotwords as hw
    monkeypatch.setattr(hw, "HOTWORD_T_CAP", 10)
    compile_hotwords(["1 2 3", "4 5"], 1.0, _ints, 99)          # 2 + 2 + 1 entries
    with pytest.raises(ValueError, match="table"):
        compile_hotwords([f"{i} {i + 1} {i + 2}" for i in range(1, 9)], 1.0, _ints, 99)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_flattened_spans_against_the_chain_walk(seed):
    """Exhaustive over (node, token) of a 40-token vocabulary; the tokens are
    drawn from a skewed distribution so that phrases share prefixes and
    suffixes (failure links at every depth)."""
    rng = np.random.default_rng(seed)
    V = 40
    p = np.r_[np.full(4, 0.15), np.full(V - 4, 0.4 / (V - 4))]
    phrases = [" ".join(str(t) for t in rng.choice(V, size=int(rng.integers(1, 9)), p=p))
               for _ in range(60)]
    a = compile_hotwords(phrases, -1.5, _ints, V)
    assert a.N > 60 and any(a.fail[n] and a.fail[a.fail[n]] for n in range(a.N))
    assert a.off[0] == 0 and a.T == len(a.tok) == len(a.dst)
    for n in range(a.N):
        tk, _ = a.span(n)
        assert list(tk) == sorted(set(tk.tolist()))
        assert a.boosted_flat(n) == ref.hotword_boosted(a, n)
        for t in range(-1, V + 1):
            assert a.advance_flat(n, t) == ref.hotword_advance(a, n, t), (n, t)


# ------------------------------------------------------------------------- step
def _step(auto, logits, ctl, slot, state, last, V=None):
    t = ops.HotwordTable("cpu")
    t.load(auto)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    ops.hotword_step(logits, logits.shape[1] if V is None else V, i32(ctl), i32(slot), state, last, t)


def _plus(x, cols, boost):
    y = x.clone()
    idx = torch.tensor(sorted(cols), dtype=torch.long)
    y[idx] = (x[idx].float() + torch.tensor(boost, dtype=torch.float32)).to(x.dtype)
    return y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_reference_step(dtype):
    # nodes: A = (1), B = (2), AB = (1 2), BD = (2 4), ABC = (1 2 3)
    a = compile_hotwords(["1 2 3", "2 4"], 0.7, _ints, 16)
    A, B = a.edges[0][1], a.edges[0][2]
    AB, BD = a.edges[A][2], a.edges[B][4]
    ABC = a.edges[AB][3]
    assert a.fail[AB] == B and a.fail[ABC] == 0 and a.fail[BD] == 0
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(6, 12, generator=g) * 3).to(dtype)
    x[0, 1] = float("-inf")
    SENT = 77
    state = torch.tensor([AB, SENT, SENT, A, AB, AB, SENT], dtype=torch.int32)
    last = torch.tensor([4, 9, 9, 2, 1, 9, 9], dtype=torch.int32)
    want, y = x.clone(), x.clone()
    # row 0: slot 0, AB + 4 falls to the failure node's child BD (a leaf): the root's columns
    # row 1: ctl 0; row 2: slot 2 starts at the root; row 3: slot 3, A + 2 advances to AB:
    # 3 (AB), 4 (B) and the root's 1, 2; row 4: slot 4, AB + 1 falls to the root child A;
    # row 5: slot 5, AB + 9 falls to the root
    _step(a, y, [2, 0, 1, 2, 2, 2], [0, 1, 2, 3, 4, 5], state, last)
    want[0] = _plus(x[0], {1, 2}, 0.7)
    want[2] = _plus(x[2], {1, 2}, 0.7)
    want[3] = _plus(x[3], {1, 2, 3, 4}, 0.7)
    want[4] = _plus(x[4], {1, 2}, 0.7)
    want[5] = _plus(x[5], {1, 2}, 0.7)
    assert torch.equal(y.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    assert state.tolist() == [BD, SENT, 0, AB, A, 0, SENT]     # ctl 0 and the trash: untouched
    assert y[0, 1] == float("-inf") and not torch.equal(y[3], x[3])
    assert last.tolist() == [4, 9, 9, 2, 1, 9, 9]


def test_a_column_on_node_failure_node_and_root_is_boosted_once():
    a = compile_hotwords(["1 2 1", "2 1", "1"], 1.0, _ints, 8)
    AB = a.edges[a.edges[0][1]][2]
    B = a.edges[0][2]
    assert a.chain(AB) == [AB, B, 0] and all(1 in a.edges[m] for m in a.chain(AB))
    x = torch.zeros(1, 8)
    state = torch.tensor([a.edges[0][1], 0], dtype=torch.int32)
    _step(a, x, [2], [0], state, torch.tensor([2, 0], dtype=torch.int32))
    assert int(state[0]) == AB and x[0].tolist() == [0, 1.0, 1.0, 0, 0, 0, 0, 0]
    # the deepest node's target wins on the device form too
    assert a.advance_flat(AB, 1) == ref.hotword_advance(a, AB, 1) == a.edges[AB][1]


def test_step_boost_values_and_validation():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 9, generator=g)
    x[1, 2] = float("-inf")
    x[1, 5] = float("nan")
    for boost in (0.0, -3.25):
        a = compile_hotwords(["2 3", "5"], boost, _ints, 16)
        y = x.clone()
        state = torch.full((3,), 9, dtype=torch.int32)
        _step(a, y, [1, 1], [0, 1], state, torch.zeros(3, dtype=torch.int32))
        if boost == 0.0:
            assert torch.equal(y.view(torch.int32), x.view(torch.int32))
        else:
            assert y[0, 2] == x[0, 2] - 3.25 and y[0, 5] == x[0, 5] - 3.25
            assert y[1, 2] == float("-inf") and math.isnan(float(y[1, 5]))
            assert int(y.view(torch.int32)[1, 5]) == int(x.view(torch.int32)[1, 5])   # its bits kept
            assert torch.equal(y[:, [0, 1, 3, 4, 6, 7, 8]], x[:, [0, 1, 3, 4, 6, 7, 8]])
        assert state.tolist() == [0, 0, 9]
    a = compile_hotwords(["2 3", "5"], 1.0, _ints, 16)
    # V below the row's width: column 5 is past it
    y = x.clone()
    _step(a, y, [1, 0], [0, 1], torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), V=4)
    assert y[0, 2] == x[0, 2] + 1.0 and y[0, 5] == x[0, 5]
    # a garbage state and a negative / huge last token land on the root
    for s0, t0 in ((-5, 2), (10 ** 6, 2), (1, -1), (1, 2 ** 31 - 1)):
        state = torch.tensor([s0, 0], dtype=torch.int32)
        _step(a, x.clone(), [2, 0], [0, 1], state, torch.tensor([t0, 0], dtype=torch.int32))
        assert int(state[0]) == (a.edges[0][2] if (s0 != 1 and t0 == 2) else 0)
    # the trash slot (the last) is a slot like any other for a ruled row ...
    state = torch.tensor([7, 7, 7], dtype=torch.int32)
    _step(a, x.clone(), [1, 0], [2, 2], state, torch.zeros(3, dtype=torch.int32))
    assert state.tolist() == [7, 7, 0]
    # ... padding rows point at it with ctl 0, and two ruled rows may not share one
    with pytest.raises((ValueError, AssertionError), match="share"):
        _step(a, x.clone(), [1, 2], [1, 1], state, torch.zeros(3, dtype=torch.int32))
    with pytest.raises((ValueError, AssertionError), match="slot"):
        _step(a, x.clone(), [1, 0], [3, 0], state, torch.zeros(3, dtype=torch.int32))
    with pytest.raises((ValueError, AssertionError), match="slot"):
        _step(a, x.clone(), [0, 2], [0, -1], state, torch.zeros(3, dtype=torch.int32))
    # an automaton without phrases: nothing moves, the state included
    y, state = x.clone(), torch.tensor([7, 7, 7], dtype=torch.int32)
    _step(compile_hotwords([], 1.0, _ints, 16), y, [1, 2], [0, 1], state, torch.zeros(3, dtype=torch.int32))
    assert torch.equal(y.view(torch.int32), x.view(torch.int32)) and state.tolist() == [7, 7, 7]


# ----------------------------------------------------------------------- engine
CFG = whisper_config("test-whisper")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, CPU, seed=0)


def _pcm(n=16000):
    return (np.random.default_rng(1).standard_normal(n) * 3000).astype(np.int16)


def _engine(weights, **kw):
    return STTEngine(CFG, CPU, seed=0, max_batch=4, weights=weights, **kw)


def _script(eng, hook=None):
    """Replace the decoder's logits by a script keyed on the last fed token:
    "turn on the" is followed by " kitchen" at 5.0 with " pantry"'s first token
    just below at 4.0; inside " pantry" the next of its tokens leads by the same
    1.0; both end in " lights" and EOT."""
    tok = eng.tok
    pantry = tok.encode(" pantry")
    assert len(pantry) == len(set(pantry)) > 1
    one = lambda s: (lambda ids: ids[0] if len(ids) == 1 else pytest.fail(s))(tok.encode(s))
    turn, on, the, kitchen, lights = (one(s) for s in (" turn", " on", " the", " kitchen", " lights"))
    nxt = {eng.sot[-1]: {turn: 5.0}, turn: {on: 5.0}, on: {the: 5.0},
           the: {kitchen: 5.0, pantry[0]: 4.0}, kitchen: {lights: 5.0}, lights: {eng.eot: 5.0},
           pantry[-1]: {lights: 5.0}}
    for a, b in zip(pantry, pantry[1:]):
        nxt[a] = {b: 5.0, kitchen: 4.0}
    sample = eng._sample

    def scripted(logits, dev):
        cu = dev["cu_q"].tolist()
        for b in range(logits.shape[0]):
            logits[b].fill_(-10.0)
            fed = int(dev["tokens"][cu[b + 1] - 1]) if cu[b + 1] > cu[b] else -1
            for t, v in nxt.get(fed, {eng.eot: 5.0}).items():
                logits[b, t] = v
        if hook is not None:
            hook()
        return sample(logits, dev)
    eng._sample = scripted
    return pantry


def test_engine_writes_the_hotword(weights, monkeypatch):
    off = _engine(weights)
    _script(off)
    calls = []
    step = ops.hotword_step
    monkeypatch.setattr(ops, "hotword_step", lambda *a, **k: (calls.append(1), step(*a, **k))[1])
    r0 = STTRequest(_pcm(), max_new_tokens=16)
    off.transcribe([r0])
    assert r0.text == "turn on the kitchen lights" and r0.hotwords is None
    assert calls == [] and not off.hotwords_on
    plain = _engine(weights, hotwords=None)
    assert off.step_fields == plain.step_fields == STTEngine.STEP_FIELDS == \
        _engine(weights, hotwords=["", "  "]).step_fields
    assert "hotword_windows" not in off.stats and not hasattr(off, "hw_state")
    assert off._layout(4, 16).n32 == STTEngine.step_layout(4, 16, off.max_blocks).n32

    live_errors = []

    def poke():
        try:
            on.set_hotwords(["sonos"])
        except RuntimeError as e:
            live_errors.append(str(e))
    on = _engine(weights, hotwords=["pantry", "hue iris"], hotword_boost=2.0)
    pantry = _script(on, poke)
    S = STTEngine.STEP_FIELDS
    assert on.step_fields == S[:8] + ("hw_ctl",) + S[8:] and on.hw_state.numel() == 5
    r1 = STTRequest(_pcm(), max_new_tokens=16)
    on.transcribe([r1])
    assert r1.text == "turn on the pantry lights" and r1.hotwords == ["pantry"]
    assert all(t in r1.tokens for t in pantry)
    assert on.stats["hotword_windows"] == 1 and on.stats["hotword_matches"] == 1
    assert len(calls) == on.stats["decode_steps"] > 0
    assert live_errors and all("live" in e for e in live_errors)
    # a boost too small to close the gap, then none at all
    on.set_hotwords(["pantry"], boost=0.5)
    r2 = STTRequest(_pcm(), max_new_tokens=16)
    on.transcribe([r2])
    assert r2.text == r0.text and r2.hotwords == [] and on.hotword_boost == 0.5
    on.set_hotwords([])
    r3 = STTRequest(_pcm(), max_new_tokens=16)
    on.transcribe([r3])
    assert r3.tokens == r0.tokens and r3.hotwords == []
    # a negative boost discourages: " kitchen" pushed below " pantry"
    on.set_hotwords(["kitchen"], boost=-2.0)
    r4 = STTRequest(_pcm(), max_new_tokens=16)
    on.transcribe([r4])
    assert r4.text == "turn on the pantry lights" and r4.hotwords == []
    with pytest.raises(ValueError, match="without hotwords"):
        off.set_hotwords(["pantry"])
    with pytest.raises(ValueError, match="beam"):
        _engine(weights, hotwords=["pantry"], beam_size=2)
    with pytest.raises(ValueError, match="boost"):
        _engine(weights, hotwords=["pantry"], hotword_boost=math.inf)


@pytest.mark.parametrize("kw", [{"timestamps": True}, {"language": "auto", "no_speech": True},
                                {"temperatures": (0.0, 0.5), "compression_ratio_threshold": 0.0},
                                {"word_timestamps": True}],
                         ids=["timestamps", "probing", "fallback", "words"])
def test_engine_modes_stage_the_control_word(weights, kw, monkeypatch):
    """With the other STT modes the control word is 1 on a window's first freely
    sampled token (every fallback attempt anew), 2 after it, 0 on prompt chunks,
    the probe step and teacher-forced requests; long-form windows use their own
    slots."""
    eng = _engine(weights, hotwords=["the kitchen", "lights"], hotword_boost=1.0, **kw)
    seen = []
    step = ops.hotword_step

    def tap(logits, V, ctl, slot, state, last, table):
        seen.append((ctl.tolist(), slot.tolist()))
        return step(logits, V, ctl, slot, state, last, table)
    monkeypatch.setattr(ops, "hotword_step", tap)
    free = STTRequest(_pcm(31 * 16000), max_new_tokens=5)
    forced = STTRequest(_pcm(), transcript="turn on the kitchen lights")
    eng.transcribe([free, forced])
    assert free.windows == 2 and forced.hotwords == ["the kitchen", "lights"]
    per_slot = {}
    for ctl, slot in seen:
        for c, s in zip(ctl, slot):
            per_slot.setdefault(s, []).append(c)
    assert set(per_slot[2]) == {0}                         # the teacher-forced request
    attempts = 2 if "temperatures" in kw else 1
    for s in (0, 1):                                       # the free request's two windows
        ruled = [c for c in per_slot[s] if c]
        assert ruled.count(1) == attempts and ruled[0] == 1 and set(ruled) == {1, 2}
        assert len(ruled) == 5 * attempts
    assert eng.stats["hotword_windows"] == 2
    assert int(eng.hw_state[3]) == 0 and int(eng.hw_state[4]) == 0


# ---------------------------------------------------------------------- config
def test_config(tmp_path):
    g = cfgmod.load({}).gpu
    assert (g.stt_hotwords, g.stt_hotwords_file, g.stt_hotword_boost, g.stt_hotwords_skills) == \
        ([], "", 2.0, "off") and not g.hotwords_on and g.resolve_hotwords() == []
    f = tmp_path / "hot.txt"
    f.write_text("# rooms\npantry\n\n  hue   iris \n#sonos\nwine cellar\n", encoding="utf-8")
    g = cfgmod.load({"HUB_STT_HOTWORDS": "hue iris, Sonos,,pantry ", "HUB_STT_HOTWORDS_FILE": str(f),
                     "HUB_STT_HOTWORD_BOOST": "-1.5"}).gpu
    assert g.stt_hotwords == ["hue iris", "Sonos", "pantry", "wine cellar"] and g.hotwords_on
    assert g.stt_hotword_boost == -1.5 and g.stt_hotwords_file == str(f)
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_HOTWORDS_FILE"):
        cfgmod.load({"HUB_STT_HOTWORDS_FILE": str(tmp_path / "missing.txt")})
    for bad in ("inf", "-inf", "nan", "1e39", "loud"):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_HOTWORD_BOOST"):
            cfgmod.load({"HUB_STT_HOTWORD_BOOST": bad})
    with pytest.raises(cfgmod.ConfigError, match="HUB_STT_HOTWORDS_SKILLS"):
        cfgmod.load({"HUB_STT_HOTWORDS_SKILLS": "maybe"})
    many = ",".join(f"w{i}" for i in range(cfgmod.HOTWORD_MAX_PHRASES + 1))
    with pytest.raises(cfgmod.ConfigError, match="1024.*w1024"):
        cfgmod.load({"HUB_STT_HOTWORDS": many})
    cfgmod.load({"HUB_STT_HOTWORDS": many[: many.rindex(",")]})
    for env in ({"HUB_STT_HOTWORDS": "pantry"}, {"HUB_STT_HOTWORDS_SKILLS": "on"}):
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BACKEND=gpu"):
            cfgmod.load({**env, "HUB_STT_BACKEND": "http"})
        with pytest.raises(cfgmod.ConfigError, match="HUB_STT_BEAM_SIZE"):
            cfgmod.load({**env, "HUB_STT_BEAM_SIZE": "2"})
    cfgmod.load({"HUB_STT_BACKEND": "http", "HUB_STT_HOTWORD_BOOST": "3"})
    # the limits that need the tokenizer
    from loqa_hub_amd.engine.tokenizer import get_tokenizer
    tok = get_tokenizer(CFG.vocab_size)
    g.check_hotwords(g.stt_hotwords, tok.encode, CFG.vocab_size)
    with pytest.raises(cfgmod.ConfigError, match="zqzq.*16"):
        g.check_hotwords(["pantry", "zq" * 20], tok.encode, CFG.vocab_size)
    with pytest.raises(cfgmod.ConfigError, match="vocabulary"):
        g.check_hotwords(["pantry"], tok.encode, 100)


def _skills_dir(tmp_path):
    import json

    from test_skills import MODULE_SKILL, manifest
    root = tmp_path / "skills"
    (root / "coffee").mkdir(parents=True)
    (root / "coffee" / "skill.json").write_text(json.dumps(
        dict(manifest("coffee"), keywords=["espresso", "flat  white", "lights"])))
    (root / "coffee" / "skill.py").write_text(MODULE_SKILL)
    (root / "broken").mkdir()
    (root / "broken" / "skill.json").write_text("{")
    return root


def test_skills_source(tmp_path):
    import asyncio
    from types import SimpleNamespace as NS

    from loqa_hub_amd.server import HubServer, resolve_hotwords
    root = _skills_dir(tmp_path)
    on = cfgmod.load({"HUB_STT_HOTWORDS": "pantry,lights", "HUB_STT_HOTWORDS_SKILLS": "on",
                      "LOQA_DB_PATH": str(tmp_path / "hub.db")})
    server = HubServer(on, skills_dir=str(root), skills_config_store=str(tmp_path / "cfg"))
    assert resolve_hotwords(on, server.skills) == ["pantry", "lights"]     # nothing loaded yet
    asyncio.run(server.load_skills())
    asyncio.run(server.load_skills())                                      # once
    assert sorted(server.skills.skills) == ["builtin.lights", "coffee"]            # the broken one skipped
    words = resolve_hotwords(on, server.skills)
    assert words[:2] == ["pantry", "lights"] and words.count("lights") == 1
    assert {"espresso", "flat white", "smart home"} <= set(words)
    off = cfgmod.load({"HUB_STT_HOTWORDS": "pantry,lights"})
    assert resolve_hotwords(off, server.skills) == ["pantry", "lights"]
    assert resolve_hotwords(cfgmod.load({}), server.skills) == []
    assert resolve_hotwords(on, None) == ["pantry", "lights"]
    big = NS(keywords=[f"k{i}" for i in range(cfgmod.HOTWORD_MAX_PHRASES)])
    with pytest.raises(cfgmod.ConfigError, match="1024"):
        on.gpu.resolve_hotwords([big])
    # the limits that need the tokenizer are checked when the list is resolved
    long = cfgmod.load({"HUB_STT_HOTWORDS": "pantry," + "zq" * 20, "HUB_STT_MODEL": "test-whisper"})
    with pytest.raises(cfgmod.ConfigError, match="zqzq.*16"):
        resolve_hotwords(long)
    asyncio.run(server.skills.stop())
    server.database.close()


def test_the_root_resolves_one_list_for_every_engine(tmp_path, monkeypatch):
    """``cli.main.run`` loads the skills, resolves the list once and hands it
    to the one-GPU processor or, through the worker spec, to every DP worker,
    whose composition passes it on to its engine."""
    import asyncio
    from types import SimpleNamespace as NS

    import loqa_hub_amd.parallel.dp_serving as dps
    import loqa_hub_amd.server as srv
    from loqa_hub_amd.cli import main as cli
    _skills_dir(tmp_path)
    monkeypatch.chdir(tmp_path)
    cfg = cfgmod.load({"HUB_STT_HOTWORDS": "pantry", "HUB_STT_HOTWORDS_SKILLS": "on",
                       "LOQA_DB_PATH": str(tmp_path / "hub.db"), "HUB_STT_MODEL": "test-whisper",
                       "HUB_DP": "2"})
    got = {}

    async def nothing(self):
        return None
    monkeypatch.setattr(srv.HubServer, "_connect_nats", nothing)
    monkeypatch.setattr(srv.HubServer, "serve_forever", nothing)
    monkeypatch.setattr(srv, "build_gpu_processor",
                        lambda cfg, nats, *a, **k: got.update(one=k) or NS(pipeline=NS()))

    class DP:
        def __init__(self, spec, n):
            got["spec"] = spec

        async def start(self):
            pass
    monkeypatch.setattr(dps, "DPVoiceProcessor", DP)
    import torch
    want = ["pantry", "lights", "lighting", "smart home", "automation", "espresso", "flat white"]
    for n_gpus in (1, 2):
        monkeypatch.setattr(torch.cuda, "device_count", lambda n=n_gpus: n)
        asyncio.run(cli.run(cfg))
    assert got["one"]["hotwords"] == want and got["spec"]["hotwords"] == want
    # the worker's composition hands the spec's list to build_gpu_processor
    monkeypatch.setattr(srv, "build_tts", lambda cfg, device: None)
    spec = {"cfg": cfg, "skills_dir": str(tmp_path / "none"), "skills_config_store": str(tmp_path / "c"),
            "hotwords": ["only", "these"]}
    proc = asyncio.run(dps._build_worker_processor(spec, "cpu"))
    assert got["one"]["hotwords"] == ["only", "these"]
    asyncio.run(proc.dp_resources[1].stop())
    # build_dp_processor without a list: the configured phrases alone
    asyncio.run(srv.build_dp_processor(cfg, 2))
    assert got["spec"]["hotwords"] == ["pantry"]


def test_served_utterance_reports_hotwords(tmp_path):
    """Through ``server.build_gpu_processor`` (CPU engines): the list reaches
    the engine, ``metrics["stt"]`` and the processor's counter, which
    ``/api/metrics`` exposes; with the keys unset none of it exists."""
    from types import SimpleNamespace as NS

    from loqa_hub_amd.api.metrics import MetricsHandler
    from test_stt_sot_probe import _serve
    base, bjob, bstats, bpipe, _ = _serve(tmp_path)
    assert not bpipe.stt.hotwords_on and "stt_hotword" not in bstats
    assert "hotwords" not in base.metrics["stt"] and bjob.transcription.hotwords is None
    res, job, stats, pipe, _ = _serve(tmp_path, HUB_STT_HOTWORDS="hue iris,pantry",
                                      HUB_STT_HOTWORD_BOOST="3.5")
    stt = pipe.stt
    assert stt.hotwords_on and stt.hw_auto.phrases == ["hue iris", "pantry"]
    assert stt.hotword_boost == 3.5 and stt.stats["hotword_windows"] == 1
    assert res.metrics["stt"]["hotwords"] == job.transcription.hotwords
    assert isinstance(res.metrics["stt"]["hotwords"], list)
    assert stats["stt_hotword"] == int(bool(job.transcription.hotwords)) == int(job.stt_hotword)
    lines = MetricsHandler(NS(audio_service=None, skills=None, nats=None,
                              processor=NS(stats=stats))).collect()
    assert any(ln.startswith("loqa_processor_stt_hotword_total ") for ln in lines)
    # a boost above every logit gap of the random-init model and a phrase of one
    # token: every sampled token is " lights" or "lights", so the phrase is found
    res, job, stats, pipe, _ = _serve(tmp_path, HUB_STT_HOTWORDS="lights",
                                      HUB_STT_HOTWORD_BOOST="1000")
    assert "lights" in job.raw_text and job.transcription.hotwords == ["lights"]
    assert res.metrics["stt"]["hotwords"] == ["lights"] and job.stt_hotword
    assert stats["stt_hotword"] == 1 and pipe.stt.stats["hotword_matches"] == 1
    lines = MetricsHandler(NS(audio_service=None, skills=None, nats=None,
                              processor=NS(stats=stats))).collect()
    assert "loqa_processor_stt_hotword_total 1.0" in lines
