"""Compact sampling head: the lm_head rows of the tokens the grammar's mask
table can select. Sampling from it must be indistinguishable from sampling
from the whole vocabulary: the same logits bit for bit, the same argmax (ties,
empty rows and maxima on disallowed tokens included), the same token sequences
from the engine - and a mask row added after start-up that reaches outside it
must send the engine back to the full head."""
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.engine.grammar import INTENTS, Choice, GrammarTables, Lit, multi_command_schema
from loqa_hub_amd.engine.llm_engine import GenRequest, LLMEngine
from loqa_hub_amd.engine.tokenizer import get_tokenizer
from loqa_hub_amd.models.configs import llama_config
from loqa_hub_amd.models.llama import CompactHead
from loqa_hub_amd.ops import reference as ref


# ------------------------------------------------------------------ CPU: sets
@pytest.fixture(scope="module")
def tables():
    g = GrammarTables(get_tokenizer(4096))
    g.trie(INTENTS)
    g.trie(["true", "false"])
    return g


def test_ids_cover_exactly_the_allowed_tokens(tables):
    rows = tables._rows
    ids, allowed = LLMEngine.compact_ids(rows)
    n = int(allowed.sum())
    assert ids.dtype == torch.int32 and ids.numel() % 16 == 0 and 0 < n <= ids.numel() < n + 16
    want = sorted({int(t) for r in rows for t in r.nonzero()[:, 0]})
    assert ids[:n].tolist() == want                       # every allowed token, no other
    assert torch.all(ids[1:n] > ids[:n - 1])              # ascending
    assert torch.all(ids[n:] == ids[n - 1])               # padding repeats the last id


def test_compact_mask_round_trip(tables):
    rows = tables._rows
    ids, allowed = LLMEngine.compact_ids(rows)
    n = int(allowed.sum())
    cm = LLMEngine.compact_mask(rows, ids, n)
    assert cm.dtype == torch.int32 and cm.shape == (len(rows), (ids.numel() + 31) // 32)
    bits = ref.unpack_mask(cm, cm.shape[1] * 32)
    full = ref.unpack_mask(tables.mask_table("cpu"), 4096)
    for r in range(len(rows)):
        assert torch.equal(bits[r, :n], full[r, ids[:n].long()])      # bit j = full bit ids[j]
        assert not bits[r, n:].any()                                  # padding stays off
        assert int(bits[r].sum()) == int(rows[r].sum())


# ---------------------------------------------------------------- CPU: argmax
def _allowed_set(V, n_allowed, g, seed):
    """``n_allowed`` random tokens that include id 0 and id V-1 (a set of one:
    id 0 or id V-1 by the seed's parity)."""
    allowed = torch.zeros(V, dtype=torch.bool)
    if n_allowed == 1:
        allowed[V - 1 if seed % 2 else 0] = True
    else:
        allowed[0] = allowed[V - 1] = True
        allowed[1 + torch.randperm(V - 2, generator=g)[:n_allowed - 2]] = True
    assert int(allowed.sum()) == n_allowed
    return allowed


def _argmax_case(V, n_allowed, seed, dtype=torch.float32, device="cpu"):
    """Logits [8, V] with the mask table, compact ids / mask and mask rows of
    the cases the sampler has to get right. Rows: 0-2 random, 3 one allowed
    token, 4 none allowed, 5 a tie between two allowed tokens, 6 the maximum on
    a disallowed token, 7 a tie with the padding's repeated last id."""
    g = torch.Generator().manual_seed(seed)
    allowed = _allowed_set(V, n_allowed, g, seed)
    idx = allowed.nonzero()[:, 0]
    sub = allowed & (torch.rand(V, generator=g) < 0.5)
    sub[idx[0]] = True
    one = torch.zeros(V, dtype=torch.bool)
    one[idx[len(idx) // 2]] = True
    table = [allowed, sub, one, torch.zeros(V, dtype=torch.bool)]
    mask_rows = torch.tensor([0, 1, 0, 2, 3, 0, 1, 0], dtype=torch.int32)
    logits = torch.randn(8, V, generator=g)
    lo, hi = idx[len(idx) // 3], idx[-1]
    logits[5, lo] = logits[5, hi] = 9.0                    # tie: the lower id wins
    logits[6, (~sub).nonzero()[0, 0]] = 11.0               # maximum outside the row's mask
    logits[7, hi] = 9.5                                    # the id the padding repeats
    ids, _ = LLMEngine.compact_ids(table)
    cmask = LLMEngine.compact_mask(table, ids, n_allowed)
    logits = logits.to(dtype)
    return dict(logits=logits.to(device), mask=ref.pack_mask(torch.stack(table)).to(device),
                rows=mask_rows.to(device), ids=ids.to(device), cmask=cmask.to(device),
                compact=logits[:, ids.long()].contiguous().to(device), lo=int(lo), hi=int(hi))


@pytest.mark.parametrize("n_allowed", [1, 17, 300, 4000])
def test_reference_argmax_with_token_ids(n_allowed):
    c = _argmax_case(4096, n_allowed, 12 + n_allowed)
    full = ref.masked_argmax(c["logits"], c["mask"], c["rows"])
    comp = ref.masked_argmax(c["compact"], c["cmask"], c["rows"], c["ids"])
    assert torch.equal(full, comp) and comp.dtype == torch.int32
    assert int(full[4]) == -1
    assert n_allowed == 1 or (int(full[5]) == c["lo"] and int(full[7]) == c["hi"])
    assert torch.equal(ops.masked_argmax(c["compact"], c["cmask"], c["rows"], token_ids=c["ids"]), full)


# ---------------------------------------------------------------- CPU: engine
PROMPTS = [("turn on the kitchen lights", 1), ("turn off the fan and then say hello", 2),
           ("what time is it and lights on and lights off", 3)]


def _drive(eng, late=("dim the hall lights and lock the door", 2)):
    """A fixed schedule with no scheduler thread, so two engines take the same
    steps: prompt pass, decode steps, then a late prompt in chunks through
    mixed passes beside the live decoders, then decode steps to the end."""
    tok = eng.tok
    reqs = [GenRequest(tok.encode(f"Voice command: {p}", bos=True),
                       multi_command_schema(n, min_response_tokens=3)) for p, n in PROMPTS]
    for r in reqs:
        eng.submit(r)
    eng.prefill(reqs)
    live = [r for r in reqs if not r.done]
    for _ in range(4):
        eng.decode_step(live)
        live = [r for r in live if not r.done]
    assert live
    b = GenRequest(tok.encode(f"Voice command: {late[0]}", bos=True),
                   multi_command_schema(late[1], min_response_tokens=3))
    eng.submit(b)
    b.chunk_total = len(b.feed)
    eng.chunk_prefill = 8
    prefilling, n_mixed = [b], 0
    while prefilling:
        live += eng._mixed_step(live, prefilling)
        prefilling = [r for r in prefilling if not getattr(r, "chunk_done", False)]
        live = [r for r in live if not r.done]
        n_mixed += 1
    assert n_mixed > 1
    while live:
        eng.decode_step(live)
        live = [r for r in live if not r.done]
    for r in reqs + [b]:
        eng.kv.pool.free_seq(r.seq_id)
    return [r.grammar.emitted for r in reqs + [b]]


def test_engine_same_tokens_cpu():
    cfg = llama_config("test-tiny")
    off = LLMEngine(cfg, "cpu", max_seqs=8, use_graphs=False, compact_head="0")
    on = LLMEngine(cfg, "cpu", max_seqs=8, use_graphs=False, compact_head="1")
    assert off.head is None and on.head is not None
    assert on.head.n < cfg.vocab_size and on.head.n % 16 == 0
    a, b = _drive(off), _drive(on)
    assert a == b and all(len(t) > 10 for t in a)
    assert on.weights.resident_bytes() > off.weights.resident_bytes()


def test_engine_knob(monkeypatch):
    cfg = llama_config("test-tiny")
    monkeypatch.setenv("HUB_LLM_COMPACT_HEAD", "0")
    assert LLMEngine(cfg, "cpu", max_seqs=2, use_graphs=False).head is None
    monkeypatch.setenv("HUB_LLM_COMPACT_HEAD", "auto")
    assert LLMEngine(cfg, "cpu", max_seqs=2, use_graphs=False).head is not None
    monkeypatch.setenv("HUB_LLM_COMPACT_HEAD", "sometimes")
    with pytest.raises(ValueError, match="HUB_LLM_COMPACT_HEAD"):
        LLMEngine(cfg, "cpu", max_seqs=2, use_graphs=False)


def _choice_run(eng, options):
    r = GenRequest(eng.tok.encode("Voice command: pick one", bos=True),
                   [Lit('{"k": "'), Choice("k", options), Lit('"}')])
    eng.generate([r])
    return r.grammar.emitted


def test_late_trie(caplog):
    cfg = llama_config("test-tiny")
    off = LLMEngine(cfg, "cpu", max_seqs=4, use_graphs=False, compact_head="0")
    on = LLMEngine(cfg, "cpu", max_seqs=4, use_graphs=False, compact_head="1")
    n_rows = on._n_mask_rows
    # a trie whose tokens all lie inside the head: rows appended, head kept
    inside = ["on", "off", "onward"]
    assert _choice_run(on, inside) == _choice_run(off, inside)
    assert on.head is not None and on._n_mask_rows > n_rows
    full = ref.unpack_mask(on.grammar.mask_table("cpu"), cfg.vocab_size)
    comp = ref.unpack_mask(on.cmasks[:on._n_mask_rows], on.cmasks.shape[1] * 32)
    assert torch.equal(comp[:, :on._head_n], full[:, on._head_ids[:on._head_n].long()])
    # a trie with a token no start-up row allows (the backslash): full head from here on
    outside = ["a\\b", "c\\d", "plain"]
    with caplog.at_level("WARNING", logger="loqa.llm"):
        got = _choice_run(on, outside)
    assert on.head is None and on.cmasks is None
    assert sum("compact sampling head: off" in m for m in caplog.messages) == 1
    assert got == _choice_run(off, outside)
    assert _drive(on) == _drive(off)                      # and the next requests still decode


# ------------------------------------------------------------------------ GPU
def _head_case(V, n_allowed, seed, d=256):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(V, d, generator=g) * 0.05).bfloat16().cuda()
    x = torch.randn(16, d, generator=g).bfloat16().cuda()
    allowed = _allowed_set(V, n_allowed, g, seed)
    ids, _ = LLMEngine.compact_ids([allowed])
    return w, x, ids


@pytest.mark.gpu
@pytest.mark.parametrize("V,n_allowed,seed", [(4096, 1, 0), (4096, 1, 1), (4096, 17, 2), (4096, 300, 3),
                                              (4096, 4000, 4), (16384, 8200, 5)])
def test_compact_logits_bitwise_gpu(V, n_allowed, seed):
    """Compact logits == full logits[:, ids], bit for bit, at equal split
    count (the heads run split 1; split 2, all d = 256 allows, slab by slab as well)."""
    w, x, ids = _head_case(V, n_allowed, seed)
    wp = ops.shuffle_weight(w)
    head = CompactHead(wp, ids.cuda())
    assert head.n == ids.numel() == -(-n_allowed // 16) * 16 and head.wp.shape[0] * 16 % 64 == 0
    for S in (1, 2):
        full = ops.skinny_gemm(x, wp, S)
        comp = ops.skinny_gemm(x, head.wp, S)[:, :, :head.n]
        assert torch.equal(comp, full[:, :, ids.long().cuda()])
    # the row-major view is the gathered weight itself
    assert torch.equal(head.rows(), w[ids.long().cuda()])


@pytest.mark.gpu
def test_compact_logits_bitwise_fp8_gpu():
    w, x, ids = _head_case(4096, 300, 6)
    wp = ops.quantize_weight_fp8(w)
    head = CompactHead(wp, ids.cuda())
    assert isinstance(head.wp, ops.Fp8Weight)
    full = ops.skinny_gemm(x, wp, 1)
    comp = ops.skinny_gemm(x, head.wp, 1)[:, :, :head.n]
    assert torch.equal(comp, full[:, :, ids.long().cuda()])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,n_allowed", [(4096, 1), (4096, 17), (4096, 300), (4096, 4000), (16384, 8200)])
def test_compact_argmax_gpu(V, n_allowed, dtype):
    """masked_argmax over the compact columns with token_ids == masked_argmax
    over the vocabulary: one workgroup per row up to 8192 columns, the
    multi-chunk atomic path past it (8200 columns, and the 16384-wide full
    row), f32 and bf16 logits, with the empty row and the ties."""
    c = _argmax_case(V, n_allowed, 21 + n_allowed, dtype, "cuda")
    want = ref.masked_argmax(c["logits"].cpu(), c["mask"].cpu(), c["rows"].cpu())
    full = ops.masked_argmax(c["logits"], c["mask"], c["rows"])
    comp = ops.masked_argmax(c["compact"], c["cmask"], c["rows"], token_ids=c["ids"])
    assert torch.equal(full.cpu(), want) and torch.equal(comp.cpu(), want)
    assert int(want[4]) == -1
    assert n_allowed == 1 or (int(want[5]) == c["lo"] and int(want[7]) == c["hi"])
    # without a mask: every column, padding included, mapped through token_ids
    nomask = ops.masked_argmax(c["compact"], token_ids=c["ids"]).cpu()
    assert torch.equal(nomask, c["ids"].cpu()[c["compact"].float().argmax(-1).cpu()])


@pytest.mark.gpu
def test_engine_same_tokens_gpu(monkeypatch):
    """Graph-replayed decode steps, prompt passes and mixed passes: identical
    tokens with the compact head on and off (default split-K, no tuning)."""
    monkeypatch.setattr(ops, "NO_TUNE", True)
    cfg = llama_config("test-tiny")
    outs = []
    for mode in ("0", "1"):
        eng = LLMEngine(cfg, "cuda", max_seqs=4, max_seq_len=512, use_graphs=True, compact_head=mode)
        assert (eng.head is not None) == (mode == "1")
        eng.warmup_graphs()
        outs.append(_drive(eng))
        assert eng.stats["decode_steps"] > 8 and eng.stats["mixed_steps"] > 1
    assert outs[0] == outs[1]
