"""Hotword biasing on the GPU: ``hotword_step_kernel`` (csrc/kernels/hotword.hip)
bit for bit against the chain-walking host reference (the CPU path of
``ops.hotword_step``), logits and the whole ``hw_state`` array, and the STT
engine with hotwords through its eager, captured, pipelined and frozen-graph
paths on the random-init ``test-whisper`` model.
"""
import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.engine.hotwords import compile_hotwords
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
from loqa_hub_amd.engine.tokenizer import _COMMON
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref

W = ops.HOTWORD_WG
NAN = float("nan")
SENT = 0x5A5A5A     # state of slots no ruled row points at
SLOTS = 7           # the last one is the trash slot


def _ints(text):
    return [int(x) for x in text.split()]


def _auto(phrases, boost=1.375):
    return compile_hotwords(phrases, boost, _ints, 1 << 16)


def _singles(k):
    # k root edges, 3 columns apart: most lie past a 33-column row
    return [str(1 + 3 * i) for i in range(k)]


AUTOMATA = {
    "empty": [],
    "root-1": ["5"],
    "root-W-1": _singles(W - 1),
    "root-W": _singles(W),
    "root-W+1": _singles(W + 1),
    "root-2W+22": _singles(2 * W + 22),
    # node (5) carries 6 and 7, and so does the root
    "overlap": ["5 6", "5 7", "6", "7 5", "9", "4 31 4", "31 4 8"],
    # node (5 6) is a leaf and 6 is no root edge: its span is empty
    "leaf": ["5 6", "12"],
}
SHAPES = {"V33-ld40": (33, 40), "V8199": (8199, 8199)}
BATCHES = {"B1": ([2], [3]), "B5": ([2, 0, 1, 0, 2], [3, 1, 0, 2, 5])}


@pytest.mark.gpu
def test_workgroup_size_is_the_kernels():
    # the W - 1, W, W + 1 root spans below are cut at the kernel's own constant
    assert ops._lib.kernels().loqa_hotword_wg() == W == 64


@pytest.fixture(scope="module")
def table():
    return ops.HotwordTable("cuda")


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _logits(dtype, V, ld, B, auto, seed):
    """B rows of random logits and two rows beyond them; NaN past column V and
    in the rows at or beyond B; a -inf and a NaN on columns the root boosts."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B + 2, ld, generator=g) * 4).to(dtype)
    cols = [int(c) for c in auto.span(0)[0] if c < V] if auto.T else []
    if len(cols) > 3:
        x[0, cols[0]] = float("-inf")
        x[B - 1, cols[1]] = NAN
    x[:, V:] = NAN
    x[B:] = NAN
    return x


def _both(table, auto, x, V, B, ctl, slot, state, last, host_checks=True):
    """One step on the host reference and twice on the device from the same
    inputs; everything compared bit for bit. Returns the new state."""
    i32 = lambda v: torch.as_tensor(v, dtype=torch.int32)
    ctl, slot = i32(ctl), i32(slot)
    xc, sc = x.clone(), state.clone()
    if host_checks:
        tc = ops.HotwordTable("cpu")
        tc.load(auto)
        ops.hotword_step(xc[:B], V, ctl, slot, sc, last, tc)
    else:       # a slot out of range: ops refuses host fields, the reference skips the row
        ref.hotword_step(xc[:B], V, ctl, slot, sc, last, auto if auto.T else None)
    outs = []
    for _ in range(2):
        xg, sg, lg = x.cuda(), state.cuda(), last.cuda()
        ops.hotword_step(xg[:B], V, ctl.cuda(), slot.cuda(), sg, lg, table)
        torch.cuda.synchronize()
        outs.append((xg.cpu(), sg.cpu()))
        assert torch.equal(lg.cpu(), last)
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(_bits(outs[0][0]), _bits(xc)), "logits differ from the reference"
    assert torch.equal(outs[0][1], sc), (outs[0][1].tolist(), sc.tolist())
    # hostile fill: columns past V and the rows beyond B came back as they went in
    assert torch.equal(_bits(outs[0][0][:, V:]), _bits(x[:, V:]))
    assert torch.equal(_bits(outs[0][0][B:]), _bits(x[B:]))
    return sc, xc


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES, ids=list(BATCHES))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", AUTOMATA, ids=list(AUTOMATA))
def test_kernel_bitwise(table, kind, dtype, shape, batch):
    auto = _auto(AUTOMATA[kind])
    table.load(auto)
    V, ld = SHAPES[shape]
    ctl, slot = BATCHES[batch]
    B = len(ctl)
    rng = np.random.default_rng(len(kind) + V + B)
    edge_toks = auto.tok.tolist() or [5]
    touched = 0
    # (state, last token) of the ruled slots: random nodes fed tokens that mostly
    # are edges somewhere; then a last token of -1, and one at or beyond V
    draws = [None] * 4 + [-1, V, V + 5]
    for d, forced in enumerate(draws):
        state = torch.full((SLOTS,), SENT, dtype=torch.int32)
        last = torch.full((SLOTS,), 3, dtype=torch.int32)
        for c, s in zip(ctl, slot):
            state[s] = int(rng.integers(0, auto.N))
            last[s] = int(rng.choice(edge_toks)) if rng.random() < 0.8 else int(rng.integers(0, V))
            if forced is not None and c == 2:
                last[s] = forced
        if kind == "leaf" and d == 0:
            state[3] = auto.N - 1                   # the leaf itself, fed a non-edge
            last[3] = 7
        x = _logits(dtype, V, ld, B, auto, d)
        sc, xc = _both(table, auto, x, V, B, ctl, slot, state, last)
        for c, s in zip(ctl, slot):                 # ctl 0 rows and their slots: untouched
            if c == 0:
                assert int(sc[s]) == int(state[s])
        assert int(sc[SLOTS - 1]) == SENT and int(sc[4]) == SENT and int(sc[6]) == SENT
        touched += int((_bits(xc) != _bits(x)).sum())
    assert (touched > 0) == (auto.T > 0)
    if kind == "overlap":
        # node (5): its span {6, 7} lies inside the root's; each column moved once
        state = torch.full((SLOTS,), SENT, dtype=torch.int32)
        state[3] = 0
        last = torch.full((SLOTS,), 5, dtype=torch.int32)
        x = torch.zeros(3, ld, dtype=dtype)
        sc, xc = _both(table, auto, x, V, 1, [2], [3], state, last)
        assert int(sc[3]) == auto.edges[0][5]
        assert sorted(xc[0].nonzero()[:, 0].tolist()) == [4, 5, 6, 7, 9, 31]
        assert set(xc[0][[4, 5, 6, 7, 9, 31]].tolist()) == {1.375}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_depth_16_phrase_walked_from_last_tok(table, dtype):
    """A 16-token phrase token by token over 17 sequential calls, each fed the
    token its sequence 'sampled' through ``last_tok``, then a mismatch."""
    phrase = list(range(10, 26))
    auto = _auto([" ".join(map(str, phrase)), "12 13 30"], boost=-0.5)
    table.load(auto)
    V, ld, s = 33, 40, 2
    state = torch.full((SLOTS,), SENT, dtype=torch.int32)
    last = torch.full((SLOTS,), -7, dtype=torch.int32)
    nodes = []
    for k in range(18):
        if k > 0:
            last[s] = phrase[k - 1] if k <= 16 else 31          # call 17: a mismatch
        x = _logits(dtype, V, ld, 2, auto, k)
        state, _ = _both(table, auto, x, V, 2, [0, 1 if k == 0 else 2], [SLOTS - 1, s], state, last)
        nodes.append(int(state[s]))
    assert nodes[0] == 0 and nodes[17] == 0 and len(set(nodes[1:17])) == 16 and 0 not in nodes[1:17]
    assert not auto.edges[nodes[16]] and ref.hotword_boosted(auto, nodes[4]) >= {14, 30, 10, 12}


@pytest.mark.gpu
def test_device_row_slot_out_of_range_is_untouched(table):
    auto = _auto(AUTOMATA["overlap"])
    table.load(auto)
    V = ld = 33
    for bad in (SLOTS, -1, 1 << 20):
        state = torch.full((SLOTS,), SENT, dtype=torch.int32)
        state[1] = 1
        last = torch.full((SLOTS,), 5, dtype=torch.int32)
        x = _logits(torch.float32, V, ld, 3, auto, 9)
        sc, xc = _both(table, auto, x, V, 3, [1, 2, 2], [bad, 1, bad], state, last,
                       host_checks=False)
        assert torch.equal(_bits(xc[0]), _bits(x[0])) and torch.equal(_bits(xc[2]), _bits(x[2]))
        assert not torch.equal(_bits(xc[1]), _bits(x[1]))
        assert sc.tolist() == [SENT, int(sc[1])] + [SENT] * (SLOTS - 2) and int(sc[1]) != 1


@pytest.mark.gpu
def test_table_is_rewritten_in_place(table):
    ptrs = [t.data_ptr() for t in (table.hdr, table.off, table.tok, table.dst)]
    big, small = _auto(_singles(200)), _auto(["5"])
    for auto in (big, small, _auto([]), big):
        table.load(auto)
        assert [t.data_ptr() for t in (table.hdr, table.off, table.tok, table.dst)] == ptrs
        x = torch.zeros(3, 640, dtype=torch.float32)
        state = torch.zeros(SLOTS, dtype=torch.int32)
        _, xc = _both(table, auto, x, 640, 1, [1], [0], state, state.clone())
        assert int((xc != 0).sum()) == (len(auto.edges[0]) if auto.T else 0)
    assert table.hdr.cpu().tolist()[:2] == [big.N, big.T]


# ---------------------------------------------------------------------- engine
CFG = whisper_config("test-whisper")
HOT = [w for w in dict.fromkeys(_COMMON) if len(w) > 3][:40] + \
    ["living room", "kitchen lights", "turn on the", "the bedroom lamp", "room temperature",
     "good morning", "play music", "set timer", "volume up", "dining room"]


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, torch.device("cuda", 0), seed=2)


def _pcms():
    rng = np.random.default_rng(1)
    out = [(rng.standard_normal(n) * 3000).astype(np.int16)
           for n in (16000, 48000, 30000, 31 * 16000)]
    assert len(out[3]) > N_SAMPLES
    return out


def _run(eng, pipelined=False, n=4):
    """Three requests arrive one step apart, then the 31 s one (two windows)
    once two slots are free: the scheduler's loop without its thread, so the
    arrivals fall on the same steps in every run."""
    from loqa_hub_amd.engine.stt_pipeline import STTPipeline
    reqs = [STTRequest(p, max_new_tokens=12, sample_seed=5 + i) for i, p in enumerate(_pcms()[:n])]
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


def _mk(weights, **kw):
    return STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, **kw)


@pytest.fixture(scope="module")
def peak(weights):
    """The largest logit magnitude the sampler sees in a hotwords-off run of
    ``_run``: what the tests scale their boosts by."""
    off = _mk(weights, use_graphs=False)
    seen = []
    sample = off._sample
    off._sample = lambda logits, dev: (seen.append(float(logits.float().abs().max())),
                                       sample(logits, dev))[1]
    _run(off)
    assert np.isfinite(max(seen)) and max(seen) > 0.0
    return max(seen)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"timestamps": True},
                                {"temperatures": (0.0, 0.4), "compression_ratio_threshold": 0.0}],
                         ids=["plain", "timestamps", "fallback"])
def test_engine_paths_agree(weights, peak, kw):
    """Eager launches, the captured synchronous step, the two-deep pipeline and
    the frozen-graph ``_launch_sync`` path run the same kernels on the same
    state: tokens, log-probabilities, text and ``hotwords`` are equal. The
    boost is this model's largest logit magnitude: the bias decides tokens
    without drowning the logits."""
    mk = lambda **k: _mk(weights, hotwords=HOT, hotword_boost=peak, token_logprobs=True, **kw, **k)
    eager = _run(mk(use_graphs=False))
    graph = _run(mk())
    warm = mk()
    assert warm.warmup_graphs() > 0 and warm._graphs_frozen
    piped = _run(warm, pipelined=True)
    assert warm.stats["pl_steps"] > 0 and warm.stats["pl_spec"] > 0
    frozen = mk()
    frozen._graphs_frozen = True
    synced = _run(frozen, pipelined=True)
    assert frozen._graphs == {} and frozen.stats["pl_steps"] == 0
    for e, g, p, s in zip(eager, graph, piped, synced):
        assert e.tokens == g.tokens == p.tokens == s.tokens and len(e.tokens) > 0
        assert e.logprobs == g.logprobs == p.logprobs == s.logprobs
        assert len(e.logprobs) == len(e.tokens)
        assert e.text == g.text == p.text == s.text
        assert e.hotwords == g.hotwords == p.hotwords == s.hotwords and e.hotwords is not None
        assert e.avg_logprob == g.avg_logprob == p.avg_logprob == s.avg_logprob
    assert [r.windows for r in eager] == [1, 1, 1, 2]
    assert any(r.hotwords for r in eager)
    off = _run(_mk(weights, token_logprobs=True, use_graphs=False, **kw))
    assert [r.tokens for r in off] != [r.tokens for r in eager]     # the bias decided something
    for st in (warm.stats, frozen.stats):
        assert st["hotword_windows"] >= 5 and st["hotword_matches"] == sum(len(r.hotwords) for r in eager)


@pytest.mark.gpu
def test_dominating_boost_keeps_every_token_inside_the_automaton(weights, peak):
    """With a boost above any logit gap of the model, every freely sampled
    token is one its sequence's node expects. The boost is read off a
    hotwords-off run's logits; the nodes are replayed on the host from the
    sampler's inputs and outputs alone."""
    base = _run(_mk(weights, use_graphs=False))
    # a boosted column is at least boost - peak, any other at most peak
    boost = 4.0 * peak + 8.0
    eng = _mk(weights, use_graphs=False, hotwords=HOT, hotword_boost=boost)
    taps = []
    sample = eng._sample

    def tap(logits, dev):
        out = sample(logits, dev)
        B = logits.shape[0]
        taps.append((dev["hw_ctl"][:B].cpu().tolist(), dev["row_slot"][:B].cpu().tolist(),
                     (out[0] if isinstance(out, tuple) else out)[:B].cpu().tolist()))
        return out
    eng._sample = tap
    reqs = _run(eng)
    auto, node, last, checked = eng.hw_auto, {}, {}, 0
    for ctl, slot, toks in taps:
        for c, s, t in zip(ctl, slot, toks):
            if c == 1:
                node[s] = 0
            elif c == 2:
                node[s] = ref.hotword_advance(auto, node[s], last[s])
            last[s] = t
            if c:
                assert t in ref.hotword_boosted(auto, node[s]), (c, s, t, node[s])
                checked += 1
    assert checked == 12 * sum(r.windows for r in reqs) == 60
    assert all(len(r.tokens) == 12 for r in reqs)            # EOT is no hotword token
    assert [r.tokens for r in reqs] != [r.tokens for r in base]
    dev_state = eng.hw_state.cpu().tolist()
    assert all(dev_state[s] == n for s, n in node.items())   # the device holds the same nodes
    # the pipelined, captured engine samples the same tokens
    warm = _mk(weights, hotwords=HOT, hotword_boost=boost)
    warm.warmup_graphs()
    assert [r.tokens for r in _run(warm, pipelined=True)] == [r.tokens for r in reqs]


@pytest.mark.gpu
def test_set_hotwords_without_a_new_capture(weights, peak):
    other = [w for w in dict.fromkeys(_COMMON) if len(w) > 3][60:90]
    warm = _mk(weights, hotwords=HOT, hotword_boost=peak)
    warm.warmup_graphs()
    graphs = {k: id(g["graph"]) for k, g in warm._graphs.items()}
    first = _run(warm, pipelined=True, n=3)
    warm.set_hotwords(other, boost=1.5 * peak)
    second = _run(warm, pipelined=True, n=3)
    assert {k: id(g["graph"]) for k, g in warm._graphs.items()} == graphs
    assert [r.tokens for r in second] != [r.tokens for r in first]
    fresh = _run(_mk(weights, hotwords=other, hotword_boost=1.5 * peak, use_graphs=False), n=3)
    assert [r.tokens for r in second] == [r.tokens for r in fresh]
    assert [r.hotwords for r in second] == [r.hotwords for r in fresh]
    warm.set_hotwords(HOT, boost=peak)
    assert [r.tokens for r in _run(warm, pipelined=True, n=3)] == [r.tokens for r in first]
    warm.set_hotwords([])
    plain = _run(_mk(weights, use_graphs=False), n=3)
    assert [r.tokens for r in _run(warm, pipelined=True, n=3)] == [r.tokens for r in plain]


@pytest.mark.gpu
def test_hotwords_off_is_the_plain_engine(weights):
    plain = _mk(weights)
    plain.warmup_graphs()
    for hot in (None, [], ["  "]):
        off = _mk(weights, hotwords=hot)
        off.warmup_graphs()
        assert set(off._graphs) == set(plain._graphs) and off.step_fields == plain.step_fields
        assert not off.hotwords_on and off.hw_table is None and not hasattr(off, "hw_state")
    want = _run(plain, pipelined=True, n=3)
    got = _run(off, pipelined=True, n=3)
    assert [r.tokens for r in got] == [r.tokens for r in want]
    assert [r.text for r in got] == [r.text for r in want] and all(r.hotwords is None for r in got)
