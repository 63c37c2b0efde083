"""MXFP4 (OCP e2m1 elements, one e8m0 scale per 32 k values) weight streaming
for the fused Llama decode GEMMs: the quantiser and the fragment order (CPU),
the in-register convert probed through the real kernel, the MXFP4 kernels
bitwise against the bf16 kernels on the dequantised weights, against the fp32
CPU reference, beside hostile memory, and the ``weight_dtype="mxfp4"`` engine
/ hub."""
import ctypes

import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref
from tests.test_fp8_weights import D, H, HKV, LAYOUTS, N_OF, _run_fused, _spread_rows

GRID = torch.tensor(ref.E2M1_GRID)


def _k_rule(K, layout):
    """A wave's k range is a whole number of 4-k-step loads."""
    Mpad, rt, wr, S, xl = layout
    return K % (S * (4 // wr) * 128) == 0


# ----------------------------------------------------------------------- CPU
def test_quantiser_error_bound():
    """With no clipping (amax / scale <= 6) an element w / scale lies in [0, 6],
    where the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6} has spacing 0.5 below 2, 1
    on [2, 4] and 2 on [4, 6]; round-to-nearest errs by at most half the
    spacing at that magnitude: |w - dq(w)| <= scale * (0.25 | 0.5 | 1). The
    scale is the SMALLEST power of two that fits, so amax / scale > 3 and the
    worst case, scale * 1, is below amax_block / 3."""
    w = _spread_rows(64, 256)
    mw = ops.quantize_weight_mxfp4(w)
    code, sb = ref.unshuffle_mxfp4(mw.wp, mw.scales)
    assert sb.dtype == torch.uint8 and sb.shape == (64, 8)
    assert int(sb.min()) >= 2 and int(sb.max()) <= 252          # never 0 (-> 0.0) or 255 (NaN)
    dq = ref.dequant_mxfp4(mw)
    wf = w.float()
    scale = torch.exp2(sb.float() - 127).repeat_interleave(32, 1)
    amax = wf.reshape(64, 8, 32).abs().amax(2)
    # the smallest power of two with amax / scale <= 6; 1 for a zero block
    nz = amax > 0
    s8 = torch.exp2(sb.float() - 127)
    assert (amax[nz] / s8[nz] <= 6).all() and (amax[nz] / (s8[nz] / 2) > 6).all()
    assert (s8[~nz] == 1).all() and (~nz).any()
    v = wf.abs() / scale
    half = torch.where(v < 2, 0.25, torch.where(v < 4, 0.5, 1.0)) * scale
    err = (wf - dq).abs()
    assert (err <= half).all(), float((err / half).max())
    assert (err.reshape(64, 8, 32)[nz] < (amax[nz] / 3)[:, None]).all()
    # ties go to the even code
    tie = torch.tensor([[0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0] + [0.0] * 24] * 16).bfloat16()
    tc = ref.quantize_mxfp4_rows(torch.cat([tie, -tie], 1))[0]
    assert tc[0, :8].tolist() == [0, 2, 2, 4, 4, 6, 6, 7]
    assert tc[0, 32:40].tolist() == [0, 10, 10, 12, 12, 14, 14, 15]   # -0.25 -> +0, sign bit 3
    # the zero row gives exact zeros with code +0; the outlier is kept (it sets
    # its block's scale) and its block's small values flush to zero
    assert not dq[5].any() and not code[5].any()
    assert abs(float(dq[9, 17]) - 3000.0) <= 3000.0 / 3 and float(dq[9, 17]) == 3072.0
    assert not dq[9, :17].any() and dq[9, 32:].any()


def test_quantiser_scale_clamp_keeps_products_normal_bf16():
    """Blocks far outside any weight's range: the scale byte stays in [2, 252],
    so every non-zero product is a normal bf16 value (exact in registers)."""
    w = torch.zeros(16, 128)
    w[0, :32] = 2.0 ** -140            # below 0.5 * 2^-125: flushes to zero
    w[1, :32] = 2.0 ** -126
    w[2, :32] = 3.0e38
    code, sb = ref.quantize_mxfp4_rows(w)
    assert int(sb.min()) >= 2 and int(sb.max()) <= 252 and int(sb[0, 0]) == 2
    dq = ref.dequant_mxfp4(ops.Mxfp4Weight(*ref.shuffle_mxfp4(code, sb), 16, 128))
    nzv = dq[dq != 0]
    assert torch.equal(nzv.bfloat16().float(), nzv) and (nzv.abs() >= 2.0 ** -126).all()
    assert torch.isfinite(dq).all() and not dq[0].any() and float(dq[1, 0]) == 2.0 ** -126


def test_shuffle_round_trip_pins_fragment_order_and_format():
    w = _spread_rows(48, 384, seed=1)
    mw = ops.quantize_weight_mxfp4(w)
    assert mw.wp.dtype == torch.uint8 and mw.wp.shape == (3, 3, 64, 16)
    assert mw.scales.dtype == torch.uint8 and mw.scales.shape == (3, 3, 16, 4)
    assert (mw.N, mw.K) == (48, 384) and (mw.shape[0] * 16, mw.shape[1] * 32) == (48, 384)
    assert mw.nbytes == 48 * 384 // 2 + 48 * 384 // 32           # 4.25 bits per weight
    code, sb = ref.quantize_mxfp4_rows(w)
    c2, s2 = ref.unshuffle_mxfp4(mw.wp, mw.scales)
    assert torch.equal(c2, code) and torch.equal(s2, sb)
    sign = torch.where(code >= 8, -1.0, 1.0)
    want = sign * GRID[(code & 7).long()] * torch.exp2(sb.float() - 127).repeat_interleave(32, 1)
    assert torch.equal(ref.dequant_mxfp4(mw), want) and torch.equal(ref.unshuffle_weight(mw), want)
    # the documented order, element by element: lane l = row l & 15; byte 4j + c
    # holds k = 32 (4g + j) + 8 (l >> 4) + 2c in its low nibble and k + 1 in its
    # high nibble; scale byte j of (tile, g, row) is that of k-step 4g + j
    for t, g, lane, b in [(0, 0, 0, 0), (1, 2, 37, 11), (2, 1, 63, 15), (0, 2, 16, 7), (2, 0, 5, 8)]:
        row = t * 16 + (lane & 15)
        k = (4 * g + b // 4) * 32 + 8 * (lane >> 4) + 2 * (b % 4)
        assert int(mw.wp[t, g, lane, b]) == int(code[row, k]) | (int(code[row, k + 1]) << 4)
        assert int(mw.scales[t, g, lane & 15, b // 4]) == int(sb[row, 4 * g + b // 4])
    # every e2m1 * 2^e the quantiser can emit is a bf16 value (what makes the
    # in-register dequantisation exact)
    allv = torch.cat([GRID, -GRID])[:, None] * torch.exp2(torch.arange(2, 253).float() - 127)[None]
    assert torch.isfinite(allv).all() and torch.equal(allv.bfloat16().float(), allv)
    # stand-in surface
    c = mw.clone().to("cpu")
    assert torch.equal(c.wp, mw.wp) and torch.equal(c.scales, mw.scales) and c.wp.data_ptr() != mw.wp.data_ptr()


def test_mxfp4_engine_decodes_on_cpu():
    from loqa_hub_amd.engine.llm_engine import LLMEngine
    from loqa_hub_amd.models.configs import llama_config
    from tests.test_fused_decode import _decode_logits
    eng = LLMEngine(llama_config("test-tiny"), "cpu", max_seqs=8, use_graphs=False, weight_dtype="mxfp4")
    w = eng.weights
    assert w.weight_dtype == "mxfp4" and w.compact and eng.fused_decode
    for L, P in zip(w.layers, w.decode_layers):
        assert set(L) == {"attn_norm", "mlp_norm"}          # no row-major projection copy
        assert set(P) == {"wqkv_f", "w_gate_up_f", "wo", "w_down"}
        assert all(isinstance(v, ops.Mxfp4Weight) for v in P.values())
    assert isinstance(w.lm_head_p, ops.Fp8Weight)            # the head stays fp8
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(10, 4000, (3, 12), generator=g).tolist()
    for lg in _decode_logits(eng, True, 100, tok, 16):
        assert lg.shape[1] == eng.cfg.vocab_size and torch.isfinite(lg).all()
    f8 = LLMEngine(llama_config("test-tiny"), "cpu", max_seqs=8, use_graphs=False, weight_dtype="fp8")
    proj = lambda ww: sum(v.nbytes for P in ww.decode_layers for v in P.values())
    assert w.resident_bytes() < f8.weights.resident_bytes()
    # 4 bits + 1/32 byte per weight, against fp8's byte per weight + 4 per row
    assert proj(w) == sum(v.N * v.K * 17 // 32 for P in w.decode_layers for v in P.values())
    assert proj(f8.weights) == sum(v.N * (v.K + 4) for P in w.decode_layers for v in P.values())


def test_mxfp4_engine_rejections():
    from loqa_hub_amd.engine.llm_engine import LLMEngine
    from loqa_hub_amd.models.configs import llama_config
    from loqa_hub_amd.models.llama import LlamaWeights, TPGroup
    cfg = llama_config("test-tiny")
    with pytest.raises(ValueError, match="single-GPU"):
        LLMEngine(cfg, "cpu", weight_dtype="mxfp4", tp=TPGroup(0, 2))
    with pytest.raises(ValueError, match="single-GPU"):
        LlamaWeights(cfg, "cpu", weight_dtype="mxfp4", tp=TPGroup(0, 2))
    with pytest.raises(ValueError, match="fused_decode"):
        LLMEngine(cfg, "cpu", weight_dtype="mxfp4", fused_decode=False)
    with pytest.raises(ValueError, match="given weights are bf16"):
        LLMEngine(cfg, "cpu", weight_dtype="mxfp4", weights=LlamaWeights(cfg, "cpu", compact=True))
    with pytest.raises(ValueError, match="given weights are fp8"):
        LLMEngine(cfg, "cpu", weight_dtype="mxfp4", weights=LlamaWeights(cfg, "cpu", weight_dtype="fp8"))


def test_mxfp4_checkpoint_load_and_dp_worker_config(tmp_path):
    """A bf16 checkpoint served in MXFP4: the loader quantises layer by layer to
    the same bytes as the seeded MXFP4 weights and keeps no row-major copy; the
    DP worker spec carries the setting (it is the hub's Config)."""
    import pickle
    from loqa_hub_amd import config as cfgmod
    from loqa_hub_amd.models import loader
    from loqa_hub_amd.models.configs import llama_config
    from loqa_hub_amd.models.llama import LlamaWeights
    cfg = llama_config("test-tiny")
    path = str(tmp_path / "tiny.safetensors")
    loader.save_llama(LlamaWeights(cfg, "cpu", seed=1), path)
    w4 = loader.load_llama(cfg, path, "cpu", weight_dtype="mxfp4")
    want = LlamaWeights(cfg, "cpu", seed=1, weight_dtype="mxfp4")
    assert w4.weight_dtype == "mxfp4" and w4.compact and len(w4.decode_layers) == cfg.n_layers
    for L, P, Q in zip(w4.layers, w4.decode_layers, want.decode_layers):
        assert set(L) == {"attn_norm", "mlp_norm"}
        for k in Q:
            assert isinstance(P[k], ops.Mxfp4Weight)
            assert torch.equal(P[k].wp, Q[k].wp) and torch.equal(P[k].scales, Q[k].scales)
    assert isinstance(w4.lm_head_p, ops.Fp8Weight) and torch.equal(w4.lm_head_p.wp, want.lm_head_p.wp)
    hub = cfgmod.load({"HUB_LLM_WEIGHTS": "mxfp4"})
    assert pickle.loads(pickle.dumps({"cfg": hub}))["cfg"].gpu.llm_weights == "mxfp4"


def test_mxfp4_config():
    from loqa_hub_amd import config as cfgmod
    assert cfgmod.load({}).gpu.llm_weights == "bf16"
    assert cfgmod.load({"HUB_LLM_WEIGHTS": "MXFP4"}).gpu.llm_weights == "mxfp4"
    with pytest.raises(cfgmod.ConfigError, match=r"bf16 \| fp8 \| mxfp4"):
        cfgmod.load({"HUB_LLM_WEIGHTS": "int4"})
    with pytest.raises(cfgmod.ConfigError, match="HUB_LLM_WEIGHTS=mxfp4 needs HUB_TP=1"):
        cfgmod.load({"HUB_LLM_WEIGHTS": "mxfp4", "HUB_TP": "2"})
    with pytest.raises(cfgmod.ConfigError, match="HUB_LLM_WEIGHTS=mxfp4 needs HUB_LLM_BACKEND"):
        cfgmod.load({"HUB_LLM_WEIGHTS": "mxfp4", "HUB_LLM_BACKEND": "ollama"})


def test_mxfp4_tuning_keys_and_splits():
    import os
    w = _spread_rows(64, 256)
    tags = [ops._wtag(ops.shuffle_weight(w)), ops._wtag(ops.quantize_weight_fp8(w)),
            ops._wtag(ops.quantize_weight_mxfp4(w))]
    assert tags == [(), ("fp8",), ("mxfp4",)]
    os.environ["LOQA_FSPLIT_OVERRIDE"] = "silu:64x256:M16=2,2,1;silu:64x256:M16:fp8=1,1,1;silu:64x256:M16:mxfp4=1,2,4"
    try:
        assert ops._fsplit_override(("silu", 64, 256, 16)) == (2, 2, 1)
        assert ops._fsplit_override(("silu", 64, 256, 16, "fp8")) == (1, 1, 1)
        assert ops._fsplit_override(("silu", 64, 256, 16, "mxfp4")) == (1, 2, 4)
    finally:
        del os.environ["LOQA_FSPLIT_OVERRIDE"]
    # choose_splits offers only splits whose 4 waves along K take whole loads:
    # Llama-3-8B down, K = 14336 = 512 * 28, and TinyLlama, K = 5632 = 512 * 11
    for K in (14336, 5632, 4096, 256):
        for tiles_n in (32, 4096):
            s = ops.choose_splits(tiles_n, K, 16, tag=("mxfp4",))
            assert s == 1 or K % (s * 512) == 0, (K, s)
    assert ops.choose_splits(32, 4096, 16, tag=("mxfp4",)) == 8
    assert ops.choose_splits(32, 14336, 16, tag=("mxfp4",)) == 4
    assert ops.choose_splits(32, 5632, 16, tag=("mxfp4",)) == 1
    assert ops.choose_splits(32, 14336, 16) == 8                 # bf16: as it was


# ----------------------------------------------------------------------- GPU
def _mx_from(code, sb, dev):
    N, K = code.shape
    return ops.Mxfp4Weight(*(t.to(dev) for t in ref.shuffle_mxfp4(code, sb)), N, K)


def _random_mx(N, K, seed, lo=-10, hi=-2):
    """Random codes and random per-block scales 2^lo .. 2^hi (quantiser range)."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    sb = (torch.randint(lo, hi + 1, (N, K // 32), generator=g) + 127).to(torch.uint8)
    return code, sb


def _bf16_of(mw, dev):
    """The exactly dequantised weight in the bf16 kernels' layout."""
    dq = ref.dequant_mxfp4(mw.to("cpu"))
    assert torch.equal(dq.bfloat16().float(), dq)
    return ops.shuffle_weight(dq.bfloat16().to(dev))


@pytest.mark.gpu
def test_mxfp4_convert_probe_gpu():
    """What v_cvt_scalef32_pk_bf16_fp4 does, seen through the real fused kernel
    (act f32 output, Mpad 16, K = 512: one 16-byte load per wave): one-hot
    activation rows pick out weight columns, 16 per launch, all 512 columns.
    Code (n + 3k + k // 32) % 16 puts each of the 16 codes at each of the 32
    nibble positions of a lane load; scale bytes 2 + (16 n + block) % 251 cover
    the quantiser's whole range 2..252. The output is the table dequantisation
    bit for bit (-0 weights arrive as +0: they pass through the accumulator)."""
    dev, N, K = "cuda", 512, 512
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    code = ((n + 3 * k + k // 32) % 16).to(torch.uint8)
    sb = (2 + (16 * n + torch.arange(K // 32)[None, :]) % 251).to(torch.uint8)
    assert set(sb.flatten().tolist()) == set(range(2, 253))
    pos = (k % 128).expand(N, K)
    for p_ in range(128):                 # byte j, nibble, lane quarter: every code at every position
        assert len(set(code[pos == p_].tolist())) == 16
    mw = _mx_from(code, sb, dev)
    want = ref.dequant_mxfp4(mw.to("cpu")) + 0.0                 # [N, K] f32, -0 -> +0
    assert torch.isfinite(want).all() and 2.0 ** 124 < float(want.abs().max()) <= 6 * 2.0 ** 125
    scr = ops.FusedScratch(dev)
    for layout in [(2, 1), (1, 4)]:       # 4 waves along K (LDS reduce), rows per wave
        got = torch.empty(K, N)
        for c0 in range(0, K, 16):
            x = torch.zeros(16, K)
            x[torch.arange(16), c0 + torch.arange(16)] = 1.0
            o = ops.skinny_fused(x.bfloat16().to(dev), mw, "act", scr, splits=1, rt=layout[0], wr=layout[1],
                                 xl=0, act="f32")
            got[c0: c0 + 16] = o.cpu()
        bad = (got.t().contiguous().view(torch.int32) != want.view(torch.int32))
        assert not bad.any(), (layout, int(bad.sum()), bad.nonzero()[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [512, 1536, 2048])
# no residual GEMM takes a norm prologue (it would rewrite the statistics it reads)
@pytest.mark.parametrize("mode,norm", [("resid", None), ("silu", None), ("silu", "rms"), ("act", None),
                                       ("act", "rms"), ("rope", None), ("rope", "rms")])
def test_mxfp4_fused_bitwise_vs_bf16_kernel_gpu(mode, norm, K):
    """The MXFP4 kernel on random codes and random per-block scales against the
    bf16 kernel on the (exactly) dequantised weights, same layout: bitwise
    equal, every output. K = 2048: all eight layouts; K = 512 (one load per
    wave) and 1536 (three loads: the ping-pong tail): the six layouts with
    K % (S * waves-along-K * 128) == 0. None may be rejected."""
    dev = "cuda"
    N = N_OF[mode]
    mw = _mx_from(*_random_mx(N, K, seed=11), dev)
    wb = _bf16_of(mw, dev)
    g = torch.Generator().manual_seed(5)
    cs = ref.rope_cos_sin(D, 512, 10000.0)
    layouts = [l for l in LAYOUTS if _k_rule(K, l)]
    assert len(layouts) == (8 if K == 2048 else 6)
    if K != 2048:
        assert set(LAYOUTS) - set(layouts) == {(16, 2, 1, 4, 0), (32, 2, 1, 2, 0)}
    for Mpad, rt, wr, S, xl in layouts:
        x = torch.randn(Mpad, K, generator=g).bfloat16()
        res0 = torch.randn(Mpad, N, generator=g).bfloat16()
        rowsq = torch.rand(4 * Mpad, generator=g) * 300 + 50
        args = (mode, x, Mpad, rt, wr, S, xl, norm, res0, cs, rowsq)
        got = _run_fused(dev, mw, *args)
        want = _run_fused(dev, wb, *args)
        for a, b in zip(got, want):
            assert torch.isfinite(a.float()).all() and a.float().abs().max() > 0
            assert torch.equal(a, b), ((Mpad, rt, wr, S, xl), float((a.float() - b.float()).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [512, 1536, 2048])
def test_mxfp4_fused_act_f32_bitwise_gpu(K):
    """act="f32" (f32 output, no rounding): the same bitwise check."""
    dev, N = "cuda", 512
    mw = _mx_from(*_random_mx(N, K, seed=12), dev)
    wb = _bf16_of(mw, dev)
    layouts = [l for l in LAYOUTS if _k_rule(K, l)]
    assert len(layouts) == (8 if K == 2048 else 6)
    for Mpad, rt, wr, S, xl in layouts:
        x = torch.randn(Mpad, K).bfloat16().to(dev)
        scr = ops.FusedScratch(dev)
        a = ops.skinny_fused(x, mw, "act", scr, splits=S, rt=rt, wr=wr, xl=xl, act="f32")
        b = ops.skinny_fused(x, wb, "act", scr, splits=S, rt=rt, wr=wr, xl=xl, act="f32")
        assert a.dtype == torch.float32 and torch.equal(a, b), (Mpad, rt, wr, S, xl)


@pytest.mark.gpu
def test_mxfp4_every_dispatch_layout_bitwise_gpu():
    """Every (Mpad, rt, wr, xl) the host dispatch knows (all that fp8 accepts)
    is accepted for MXFP4 where the K rule holds, and is bitwise the bf16
    kernel: among them the layouts whose prefetch group is 2 k-steps (8-byte
    weight loads): Mpad 64 in the register form and XL with rt * Mpad / 16 >= 16.
    K = 1024: two loads per wave with 4 waves along K, split 2 in the XL form."""
    dev, N, K = "cuda", 512, 1024
    mw = _mx_from(*_random_mx(N, K, seed=21), dev)
    wb = _bf16_of(mw, dev)
    layouts = [(mp, rt, wr, 1, 0) for mp in (16, 32, 64) for rt in (1, 2) for wr in (1, 4)]
    layouts += [(64, 4, 1, 1, 0), (64, 4, 4, 1, 0)]
    layouts += [(mp, rt, 4, 2, 1) for mp in (32, 64, 128) for rt in (1, 2)]
    assert len(layouts) == 20 and all(_k_rule(K, l) for l in layouts)
    scr = ops.FusedScratch(dev)
    for Mpad, rt, wr, S, xl in layouts:
        x = torch.randn(Mpad, K).bfloat16().to(dev)
        a = ops.skinny_fused(x, mw, "act", scr, splits=S, rt=rt, wr=wr, xl=xl)
        b = ops.skinny_fused(x, wb, "act", scr, splits=S, rt=rt, wr=wr, xl=xl)
        assert a.float().abs().max() > 0 and torch.equal(a, b), (Mpad, rt, wr, S, xl)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [(16, 2, 1, 1, 0), (64, 2, 4, 1, 1), (128, 1, 4, 2, 1)])
@pytest.mark.parametrize("mode", ["resid", "silu", "act", "rope"])
def test_mxfp4_fused_vs_fp32_reference_gpu(mode, layout):
    """Arbitrary bf16 weights (row magnitudes 2^-3 .. 2^3, so a wrong or
    unpermuted scale index is a gross error) through ``quantize_weight_mxfp4``
    against the fp32 CPU reference of the same call on the same codes and
    scales; the bf16 kernels' metric and bound (tests/test_fused_decode.py):
    relative Frobenius error < 1e-2."""
    Mpad, rt, wr, S, xl = layout
    K, N = 1024, N_OF[mode]
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(N, K, generator=g) * 0.03 * torch.exp2(torch.rand(N, 1, generator=g) * 6 - 3)).bfloat16()
    if mode == "silu":
        w = w[ref.perm_gate_up(N // 2)].contiguous()
    elif mode == "rope":
        w = w[ref.perm_rope_qkv(H, HKV, D)].contiguous()
    mw = ops.quantize_weight_mxfp4(w)
    mg = mw.to("cuda")
    x = torch.randn(Mpad, K, generator=g).bfloat16()
    res0 = torch.randn(Mpad, N, generator=g).bfloat16()
    cs = ref.rope_cos_sin(D, 512, 10000.0)
    rowsq = torch.rand(4 * Mpad, generator=g) * 300 + 50
    norm = None if mode == "resid" else "rms"
    args = (mode, x, Mpad, rt, wr, S, xl, norm, res0, cs, rowsq)
    want = _run_fused("cpu", mw, *args)
    got = _run_fused("cuda", mg, *args)
    for a, b in zip(got, want):
        rel = float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-6))
        print(mode, layout, "rel", rel)
        assert rel < 1e-2, rel


@pytest.mark.gpu
def test_mxfp4_hostile_memory_gpu():
    """The nibbles and the scale bytes as views inside larger allocations
    filled with 0xff (-6 | -6; NaN in e8m0), the output inside a sentinel
    buffer: results unchanged and the sentinels intact, so nothing is read or
    written past them."""
    dev, K, N = "cuda", 1024, 512
    clean = _mx_from(*_random_mx(N, K, seed=14), dev)
    pad = 1 << 16
    big = torch.full((pad + N * K // 2 + pad,), 0xFF, dtype=torch.uint8, device=dev)
    big[pad: pad + N * K // 2] = clean.wp.flatten()
    sbig = torch.full((1024 + N * K // 32 + 1024,), 0xFF, dtype=torch.uint8, device=dev)
    sbig[1024: 1024 + N * K // 32] = clean.scales.flatten()
    hostile = ops.Mxfp4Weight(big[pad: pad + N * K // 2].view(N // 16, K // 128, 64, 16),
                              sbig[1024: 1024 + N * K // 32].view(N // 16, K // 128, 16, 4), N, K)
    assert hostile.wp.data_ptr() == big.data_ptr() + pad
    for Mpad, rt, wr, S, xl in [(16, 2, 1, 1, 0), (16, 1, 1, 2, 0), (16, 2, 4, 1, 0), (64, 4, 4, 1, 0),
                                (128, 2, 4, 4, 1)]:
        assert _k_rule(K, (Mpad, rt, wr, S, xl))
        x = torch.randn(Mpad, K).bfloat16().to(dev)
        scr = ops.FusedScratch(dev)
        obig = torch.full((Mpad + 8, N), 777.0, device=dev).bfloat16()
        a = ops.skinny_fused(x, hostile, "act", scr, splits=S, rt=rt, wr=wr, xl=xl, out=obig[4: 4 + Mpad])
        b = ops.skinny_fused(x, clean, "act", scr, splits=S, rt=rt, wr=wr, xl=xl)
        assert a.data_ptr() == obig.data_ptr() + 4 * N * 2
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
        assert (obig[:4] == 777.0).all() and (obig[4 + Mpad:] == 777.0).all()
        fbig = torch.full((Mpad + 8, N), 777.0, device=dev)
        a = ops.skinny_fused(x, hostile, "act", scr, splits=S, rt=rt, wr=wr, xl=xl, act="f32",
                             out=fbig[4: 4 + Mpad])
        assert torch.equal(a, ops.skinny_fused(x, clean, "act", scr, splits=S, rt=rt, wr=wr, xl=xl, act="f32"))
        assert (fbig[:4] == 777.0).all() and (fbig[4 + Mpad:] == 777.0).all()


@pytest.mark.gpu
def test_mxfp4_fused_rejects_unsupported_gpu():
    """K ranges that are not whole 4-k-step loads per wave, the LayerNorm
    prologue and a missing scale pointer are refused by the host dispatch
    (hipErrorInvalidValue); nothing is launched, the output keeps its sentinel."""
    dev, N = "cuda", 512
    scr = ops.FusedScratch(dev)
    for K, S, wr in [(256, 1, 1), (768, 1, 1), (1536, 2, 1), (2048, 8, 1)]:
        mw = _mx_from(*_random_mx(N, K, seed=15), dev)
        x = torch.randn(16, K).bfloat16().to(dev)
        out = torch.full((16, N), 777.0, device=dev).bfloat16()
        with pytest.raises(RuntimeError, match="hipError 1"):
            ops.skinny_fused(x, mw, "act", scr, splits=S, rt=2, wr=wr, xl=0, out=out)
        torch.cuda.synchronize()
        assert (out == 777.0).all()
    # K = 256 and 768 do run where every wave takes whole loads (rows per wave)
    for K in (256, 768):
        mw = _mx_from(*_random_mx(N, K, seed=16), dev)
        x = torch.randn(16, K).bfloat16().to(dev)
        a = ops.skinny_fused(x, mw, "act", scr, splits=1, rt=2, wr=4, xl=0)
        assert torch.equal(a, ops.skinny_fused(x, _bf16_of(mw, dev), "act", scr, splits=1, rt=2, wr=4, xl=0))
    K = 1536
    mw = _mx_from(*_random_mx(N, K, seed=15), dev)
    x = torch.randn(16, K).bfloat16().to(dev)
    p = ops.FusedParams()
    p.x, p.ldx, p.Wp, p.wscale, p.wdtype = x.data_ptr(), K, mw.wp.data_ptr(), mw.scales.data_ptr(), 2
    out = torch.full((16, N), 777.0, device=dev).bfloat16()
    p.Mpad, p.N, p.K, p.S, p.mode, p.norm = 16, N, K, 1, 4, 2                # LayerNorm
    p.rowsq_in = p.rowsum_in = p.colsum = scr.rowsq.data_ptr()
    p.rowstat_tiles, p.out, p.ldo, p.rt, p.wr = 1, out.data_ptr(), N, 2, 1
    st = torch.cuda.current_stream().cuda_stream
    assert ops.kernels().loqa_skinny_fused(ctypes.byref(p), st) == 1
    p.norm, p.wscale = 0, None                                              # no scale pointer
    assert ops.kernels().loqa_skinny_fused(ctypes.byref(p), st) == 1
    p.wscale, p.wdtype = mw.scales.data_ptr(), 3                            # no such format
    assert ops.kernels().loqa_skinny_fused(ctypes.byref(p), st) == 1
    torch.cuda.synchronize()
    assert (out == 777.0).all()
    with pytest.raises(TypeError, match="MXFP4"):                           # no plain skinny GEMM instance
        ops.skinny_gemm(x, mw, 1)


def _mx_engine_logits(device, Mpad, tok):
    from loqa_hub_amd.engine.llm_engine import LLMEngine
    from loqa_hub_amd.models.configs import llama_config
    from tests.test_fused_decode import _decode_logits
    eng = LLMEngine(llama_config("test-tiny"), device, max_seqs=8, use_graphs=False, weight_dtype="mxfp4")
    return eng, (lambda: _decode_logits(eng, True, 100, tok, Mpad))


_CPU_LOGITS: dict = {}


@pytest.mark.gpu
@pytest.mark.parametrize("splits,Mpad", [(None, 16), (None, 64), (2, 64)])
def test_mxfp4_engine_gpu_matches_cpu(splits, Mpad):
    """The MXFP4 ``test-tiny`` engine on the GPU against the same engine (the
    same codes, scales and fp8 head) on the CPU: logits within the bound the
    bf16 fused / unfused comparison uses (2e-2). The forced split: K = 256 and
    512 hold whole loads for a split only in the x-through-LDS layout (waves
    along rows), so it is pinned at Mpad 64 as (S 2, rt 1, wr 4, xl)."""
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(10, 4000, (3, 12), generator=g).tolist()
    if Mpad not in _CPU_LOGITS:
        _CPU_LOGITS[Mpad] = _mx_engine_logits("cpu", Mpad, tok)[1]()
    eng, run = _mx_engine_logits("cuda", Mpad, tok)
    assert all(isinstance(v, ops.Mxfp4Weight) and v.is_cuda for P in eng.weights.decode_layers for v in P.values())
    saved_f = dict(ops._FSPLITS)
    try:
        if splits is not None:
            ops._FSPLITS.clear()
            d, w = eng.cfg.d_model, eng.weights
            for mode, N, K in (("rope", w.h * 64 + 2 * w.hkv * 64, d), ("resid", d, w.h * 64),
                               ("silu", 2 * w.f, d), ("resid", d, w.f)):
                assert K % (splits * 128) == 0 and N % 64 == 0
                ops._FSPLITS[(mode, N, K, Mpad, "mxfp4")] = (splits, 1, 4, 1)
        got = run()
    finally:
        ops._FSPLITS.clear(); ops._FSPLITS.update(saved_f)
    for a, b in zip(got, _CPU_LOGITS[Mpad]):
        assert torch.isfinite(a).all()
        rel = float((a - b).norm() / (b.norm() + 1e-12))
        print("mxfp4 engine gpu vs cpu rel", rel)
        assert rel < 2e-2, rel


@pytest.mark.gpu
def test_mxfp4_engine_graphs_match_eager_gpu():
    import json
    from loqa_hub_amd.engine.grammar import multi_command_schema
    from loqa_hub_amd.engine.llm_engine import GenRequest, LLMEngine
    from loqa_hub_amd.models.configs import llama_config
    cfg = llama_config("test-tiny")

    def gen(eng):
        toks = [[] for _ in range(3)]
        reqs = [GenRequest(eng.tok.encode(f"Voice command: turn on the lights {i}", bos=True),
                           multi_command_schema(n, min_response_tokens=3), on_tokens=toks[i].extend)
                for i, n in enumerate([1, 2, 3])]
        return eng.generate(reqs), toks
    (a, ta), (b, tb) = (gen(LLMEngine(cfg, "cuda", max_seqs=8, use_graphs=g, weight_dtype="mxfp4"))
                        for g in (True, False))
    for x, y, tx, ty, n in zip(a, b, ta, tb, [1, 2, 3]):
        assert tx and tx == ty and x.output == y.output
        assert len(json.loads(x.output)["commands"]) == n


@pytest.mark.gpu
def test_mxfp4_hub_served_gpu(tmp_path, monkeypatch):
    """``HUB_LLM_WEIGHTS=mxfp4`` serves the hub end to end on one GPU: the
    served-hub checks (both commands of the utterance on the bus, the voice
    event, the spoken reply), with the MXFP4 projections and the fp8 lm_head in
    the engine and the dtype and resident bytes on /api/metrics."""
    import tests.test_hub_served as hs
    from loqa_hub_amd.models import llama
    load = hs.cfgmod.load
    monkeypatch.setattr(hs.cfgmod, "load", lambda env=None: load({**env, "HUB_LLM_WEIGHTS": "mxfp4"}))
    seen = []
    fin = llama.LlamaWeights._finalize
    monkeypatch.setattr(llama.LlamaWeights, "_finalize", lambda self: (fin(self), seen.append(self))[0])
    res = hs._served(tmp_path, "cuda:0", streaming=True, llm="test-tiny", stt="whisper-tiny",
                     tts_model="test-vits")
    hs._check_served(*res, streaming=True, relays=("kitchen-relay",))
    assert 'loqa_llm_weight_dtype{dtype="mxfp4"} 1.0' in res[5]
    assert "loqa_llm_weight_bytes " in res[5]
    w = [s for s in seen if getattr(s, "weight_dtype", "") == "mxfp4"]
    assert w and isinstance(w[0].lm_head_p, ops.Fp8Weight)
    assert all(isinstance(v, ops.Mxfp4Weight) for P in w[0].decode_layers for v in P.values())
