"""The host side of the captured decode steps' I/O protocol
(``engine/step_io.py``): the flat metadata layout of both engines, the
device-fed token staging and the graph bucket enumeration. CPU only."""
import numpy as np
import pytest

from loqa_hub_amd import ops
from loqa_hub_amd.engine.llm_engine import LLMEngine
from loqa_hub_amd.engine.step_io import (DEV, StepIO, StepLayout, decode_buckets, stage_feeds,
                                         step_shapes)
from loqa_hub_amd.engine.stt_engine import STTEngine

MAX_BLOCKS = 3
ENGINES = [LLMEngine, STTEngine]
GRID = [(b, t) for b in LLMEngine.SEQ_BUCKETS for t in ops.MPADS]


def test_field_lists():
    common = ("tokens", "positions", "slots", "cu_q", "ctx_lens", "block_tables")
    assert LLMEngine.STEP_FIELDS == common + ("mask_rows", "src", "row_slot")
    assert STTEngine.STEP_FIELDS == common + ("enc_starts", "enc_lens", "src", "row_slot")
    assert STTEngine.SEQ_BUCKETS == LLMEngine.SEQ_BUCKETS


@pytest.mark.parametrize("eng", ENGINES, ids=["llm", "stt"])
def test_layout_every_bucket(eng):
    largest = eng.step_layout(eng.SEQ_BUCKETS[-1], ops.MPADS[-1], MAX_BLOCKS)
    for B_pad, T_pad in GRID:
        lay = eng.step_layout(B_pad, T_pad, MAX_BLOCKS)
        assert list(lay.shapes) == list(eng.STEP_FIELDS)
        assert lay.n32 <= largest.n32 and lay.n64 <= largest.n64
        assert lay.offsets["tokens"] == 0 and lay.src_off == lay.offsets["src"]
        assert lay.shapes["tokens"] == (T_pad,) and lay.shapes["src"] == (T_pad,)
        assert lay.shapes["row_slot"] == (B_pad,) and lay.shapes["cu_q"] == (B_pad + 1,)
        assert lay.shapes["block_tables"] == (B_pad, MAX_BLOCKS)
        # a staging row wider than the layout, as the rings' rows are
        flat32 = np.full(largest.n32, -7, np.int32)
        flat64 = np.full(largest.n64, -7, np.int64)
        v = lay.views(flat32, flat64)
        assert list(v) == list(eng.STEP_FIELDS) + ["logit_idx"]
        # disjoint, in declaration order, covering exactly [0, n32): field i
        # written with i + 1 gives the run-length pattern of the sizes
        end = 0
        for i, f in enumerate(eng.STEP_FIELDS):
            assert v[f].shape == lay.shapes[f] and lay.offsets[f] == end
            assert np.shares_memory(v[f], flat32)
            v[f][...] = i + 1
            end += v[f].size
        assert end == lay.n32
        want = np.repeat(np.arange(1, len(eng.STEP_FIELDS) + 1), [v[f].size for f in eng.STEP_FIELDS])
        assert np.array_equal(flat32[: lay.n32], want) and (flat32[lay.n32:] == -7).all()
        assert v["logit_idx"].shape == (lay.n64,) and np.shares_memory(v["logit_idx"], flat64)
        # a value written through one set of views is read at the same flat
        # index through a second views() of the layout (device buffers use
        # the same call)
        flat32[:] = np.arange(largest.n32)
        flat64[:] = np.arange(largest.n64)
        w = lay.views(flat32, flat64)
        for f in eng.STEP_FIELDS:
            o = lay.offsets[f]
            assert np.array_equal(w[f].ravel(), np.arange(o, o + w[f].size))
        assert np.array_equal(w["logit_idx"], np.arange(lay.n64))
        v["block_tables"][B_pad - 1, MAX_BLOCKS - 1] = -99
        assert flat32[lay.offsets["block_tables"] + B_pad * MAX_BLOCKS - 1] == -99
        assert w["block_tables"][B_pad - 1, MAX_BLOCKS - 1] == -99


def test_layout_n64():
    for B_pad, T_pad in GRID:
        assert LLMEngine.step_layout(B_pad, T_pad, MAX_BLOCKS).n64 == max(16, B_pad)
        assert STTEngine.step_layout(B_pad, T_pad, MAX_BLOCKS).n64 == max(16, ops.mpad_for(B_pad))


def test_layout_rejections():
    ok = step_shapes(LLMEngine.STEP_FIELDS, 4, 16, MAX_BLOCKS)
    StepLayout(ok, 16)
    swapped = {"positions": ok["positions"], **{k: v for k, v in ok.items() if k != "positions"}}
    assert list(swapped)[1] == "tokens"
    with pytest.raises(ValueError, match="tokens"):
        StepLayout(swapped, 16)
    for f in ("src", "row_slot"):
        with pytest.raises(ValueError, match=f):
            StepLayout({k: v for k, v in ok.items() if k != f}, 16)
    with pytest.raises(ValueError):
        StepLayout({}, 16)


def test_stage_feeds():
    lay = LLMEngine.step_layout(4, 16, MAX_BLOCKS)
    flat32 = np.full(lay.n32, 77, np.int32)       # stale values of an earlier step
    host = lay.views(flat32, np.zeros(lay.n64, np.int64))
    before = {f: host[f].copy() for f in lay.shapes if f not in ("tokens", "src", "row_slot")}
    trash = 9
    feeds = [[11, 12, 13], [DEV, 21], [DEV]]
    stage_feeds(host, feeds, [5, 0, 7], trash)
    assert host["tokens"].tolist() == [11, 12, 13, 0, 21, 0] + [0] * 10
    assert host["src"].tolist() == [-1, -1, -1, 0, -1, 7] + [-1] * 10
    assert host["row_slot"].tolist() == [5, 0, 7, trash]
    for f, a in before.items():                   # nothing else is touched
        assert np.array_equal(host[f], a), f
    # no sequences: an all-padding step
    stage_feeds(host, [], [], trash)
    assert (host["tokens"] == 0).all() and (host["src"] == -1).all()
    assert (host["row_slot"] == trash).all()


def _parent_llm_buckets(max_seqs, step_tokens, max_decode_q, ctx_bucket, max_seq_len):
    """``LLMEngine.warmup_graphs``' loops before they moved to decode_buckets."""
    def bucket(n, buckets):
        for b in buckets:
            if n <= b:
                return b
        return n
    out = []
    b_max = bucket(max(1, max_seqs), LLMEngine.SEQ_BUCKETS)
    for b in LLMEngine.SEQ_BUCKETS:
        if b > b_max:
            break
        t_min = ops.mpad_for(min(step_tokens, b // 2 + 1))
        t_max = ops.mpad_for(min(step_tokens, b * max_decode_q))
        for t in ops.MPADS:
            if t > t_max:
                break
            if t < t_min:
                continue
            for c in range(ctx_bucket, max_seq_len + ctx_bucket, ctx_bucket):
                out.append((b, t, min(c, max_seq_len)))
    return out


def _parent_stt_buckets(max_batch, step_tokens, n_sot, split_keys, n_text_ctx):
    """``STTEngine.warmup_graphs``' loops before they moved to decode_buckets."""
    out = []
    b_max = next((b for b in STTEngine.SEQ_BUCKETS if b >= max_batch), STTEngine.SEQ_BUCKETS[-1])
    for b in STTEngine.SEQ_BUCKETS:
        if b > b_max:
            break
        t_min = ops.mpad_for(min(step_tokens, b // 2 + 1))
        t_max = ops.mpad_for(min(step_tokens, b * n_sot))
        for t in ops.MPADS:
            if t > t_max:
                break
            if t < t_min:
                continue
            for c in range(split_keys, n_text_ctx + split_keys, split_keys):
                out.append((b, t, min(c, n_text_ctx)))
    return out


@pytest.mark.parametrize("n", [1, 8, 64, 200])
def test_decode_buckets(n):
    for step_tokens, max_q, max_seq_len in ((64, 8, 1024), (64, 2, 1000), (16, 32, 256)):
        got = decode_buckets(LLMEngine.SEQ_BUCKETS, n, step_tokens, max_q, LLMEngine.CTX_BUCKET,
                             max_seq_len)
        assert got == _parent_llm_buckets(n, step_tokens, max_q, LLMEngine.CTX_BUCKET, max_seq_len)
        assert got and len(set(got)) == len(got)
    for step_tokens, n_text_ctx in ((64, 448), (4, 448), (32, 100)):
        got = decode_buckets(STTEngine.SEQ_BUCKETS, n, step_tokens, 4, STTEngine.SPLIT_KEYS,
                             n_text_ctx)
        assert got == _parent_stt_buckets(n, step_tokens, 4, STTEngine.SPLIT_KEYS, n_text_ctx)
        assert got and len(set(got)) == len(got)


def test_ring_constants():
    # step_fetch_kernel picks the staging row with (counter & 1), and
    # step_publish_kernel<NLP> wraps the counter at 2 * nres
    assert StepIO.STAGE_SLOTS == 2 and StepIO.WRAP == 2 * StepIO.RES_SLOTS
    assert StepIO.WRAP % StepIO.STAGE_SLOTS == 0 and StepIO.WRAP % StepIO.RES_SLOTS == 0
    StepIO.check_depth(StepIO.RES_SLOTS - 1)
    with pytest.raises(AssertionError):
        StepIO.check_depth(StepIO.RES_SLOTS)
