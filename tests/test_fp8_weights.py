"""FP8 (OCP e4m3fn) weight streaming for the Llama decode GEMMs: the quantiser
and the fragment order (CPU), the fp8 kernels bitwise against the bf16 kernels
on exactly representable weights, against the fp32 CPU reference, beside
hostile memory, and the ``weight_dtype="fp8"`` engine / hub."""
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn
H, HKV, D = 8, 2, 64
N_OF = {"resid": 512, "silu": 1024, "act": 512, "rope": (H + 2 * HKV) * D}
# Mpad, rt, wr, S, xl
LAYOUTS = [(16, 1, 1, 1, 0), (16, 2, 1, 4, 0), (16, 2, 4, 1, 0), (32, 2, 1, 2, 0), (64, 4, 4, 1, 0),
           (64, 2, 4, 2, 1), (128, 1, 4, 1, 1), (128, 2, 4, 4, 1)]


# ----------------------------------------------------------------------- CPU
def _spread_rows(N, K, seed=0):
    """bf16 rows with magnitudes spread over 2^-3 .. 2^3, row 5 all zero, row 9
    one large outlier."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.rand(N, 1, generator=g) * 6 - 3)
    w[5] = 0
    w[9] = torch.randn(K, generator=g) * 1e-3
    w[9, 17] = 3000.0
    return w.bfloat16()


def test_quantiser_error_bound():
    """|w - dq(w)| <= max(2^-4 |w|, 2^-10 scale_row): e4m3's half ulp for
    normals (3 mantissa bits) and half its subnormal step 2^-9 (in units of the
    row scale)."""
    w = _spread_rows(64, 256)
    fw = ops.quantize_weight_fp8(w)
    dq = ref.dequant_fp8(fw)
    assert fw.scale.dtype == torch.float32 and fw.scale.shape == (64,)
    assert torch.isfinite(dq).all() and torch.isfinite(fw.scale).all()
    wf = w.float()
    assert torch.equal(fw.scale, torch.where(wf.abs().amax(1) > 0, wf.abs().amax(1) / 448, torch.ones(64)))
    assert float(fw.scale[5]) == 1.0 and not dq[5].any()
    bound = torch.maximum(wf.abs() * 2.0 ** -4, fw.scale[:, None] * 2.0 ** -10)
    err = (wf - dq).abs()
    assert (err <= bound).all(), float((err / bound.clamp_min(1e-30)).max())
    # the outlier is kept (it sets the scale) and nothing saturates to NaN
    assert abs(float(dq[9, 17]) - 3000.0) <= 3000.0 * 2.0 ** -4


def test_shuffle_round_trip_pins_fragment_order_and_format():
    w = _spread_rows(48, 192, seed=1)
    fw = ops.quantize_weight_fp8(w)
    assert fw.wp.dtype == torch.uint8 and fw.wp.shape == (3, 3, 64, 16)
    assert (fw.N, fw.K) == (48, 192) and (fw.shape[0] * 16, fw.shape[1] * 32) == (48, 192)
    scale = fw.scale
    q = (w.float() / scale[:, None]).clamp(-448, 448).to(FP8)
    assert torch.equal(ref.dequant_fp8(fw), q.float() * scale[:, None])
    # the documented order, element by element: lane l = row l & 15; bytes 0-7
    # the k values at 8 * (l >> 4) of k-step 2j, bytes 8-15 those of k-step 2j + 1
    qb = q.view(torch.uint8)
    for t, j, lane, b in [(0, 0, 0, 0), (1, 2, 37, 11), (2, 1, 63, 15), (0, 2, 16, 7), (2, 0, 5, 8)]:
        row = t * 16 + (lane & 15)
        k = (2 * j + b // 8) * 32 + 8 * (lane >> 4) + b % 8
        assert int(fw.wp[t, j, lane, b]) == int(qb[row, k])
    # every e4m3 value is a bf16 value (what makes the in-register dequantisation exact)
    allv = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    fin = ~allv.isnan()
    assert torch.equal(allv[fin].bfloat16().float(), allv[fin])


def test_fp8_engine_decodes_on_cpu():
    from loqa_hub_amd.engine.llm_engine import LLMEngine
    from loqa_hub_amd.models.configs import llama_config
    from tests.test_fused_decode import _decode_logits
    eng = LLMEngine(llama_config("test-tiny"), "cpu", max_seqs=8, use_graphs=False, weight_dtype="fp8")
    w = eng.weights
    assert w.weight_dtype == "fp8" and w.compact and eng.fused_decode
    for L, P in zip(w.layers, w.decode_layers):
        assert set(L) == {"attn_norm", "mlp_norm"}          # no row-major projection copy
        assert set(P) == {"wqkv_f", "w_gate_up_f", "wo", "w_down"}
        assert all(isinstance(v, ops.Fp8Weight) for v in P.values())
    assert isinstance(w.lm_head_p, ops.Fp8Weight)
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(10, 4000, (3, 12), generator=g).tolist()
    for lg in _decode_logits(eng, True, 100, tok, 16):
        assert lg.shape[1] == eng.cfg.vocab_size and torch.isfinite(lg).all()
    bf = LLMEngine(llama_config("test-tiny"), "cpu", max_seqs=8, use_graphs=False, compact=True)
    assert w.resident_bytes() < bf.weights.resident_bytes()


def test_fp8_engine_rejections():
    from loqa_hub_amd.engine.llm_engine import LLMEngine
    from loqa_hub_amd.models.configs import llama_config
    from loqa_hub_amd.models.llama import TPGroup
    cfg = llama_config("test-tiny")
    with pytest.raises(ValueError, match="single-GPU"):
        LLMEngine(cfg, "cpu", weight_dtype="fp8", tp=TPGroup(0, 2))
    with pytest.raises(ValueError, match="fused_decode"):
        LLMEngine(cfg, "cpu", weight_dtype="fp8", fused_decode=False)
    with pytest.raises(ValueError, match="weight_dtype"):
        LLMEngine(cfg, "cpu", weight_dtype="int4")


def test_fp8_checkpoint_load_and_dp_worker_config(tmp_path):
    """A bf16 checkpoint served in fp8: the loader quantises layer by layer to
    the same bytes as the seeded fp8 weights, and keeps no row-major copy; the
    DP worker spec carries the setting (it is the hub's Config)."""
    import pickle
    from loqa_hub_amd import config as cfgmod
    from loqa_hub_amd.models import loader
    from loqa_hub_amd.models.configs import llama_config
    from loqa_hub_amd.models.llama import LlamaWeights
    cfg = llama_config("test-tiny")
    path = str(tmp_path / "tiny.safetensors")
    loader.save_llama(LlamaWeights(cfg, "cpu", seed=1), path)
    w8 = loader.load_llama(cfg, path, "cpu", weight_dtype="fp8")
    want = LlamaWeights(cfg, "cpu", seed=1, weight_dtype="fp8")
    assert w8.weight_dtype == "fp8" and w8.compact and len(w8.decode_layers) == cfg.n_layers
    for L, P, Q in zip(w8.layers, w8.decode_layers, want.decode_layers):
        assert set(L) == {"attn_norm", "mlp_norm"}
        for k in Q:
            assert torch.equal(P[k].wp, Q[k].wp) and torch.equal(P[k].scale, Q[k].scale)
    assert torch.equal(w8.lm_head_p.wp, want.lm_head_p.wp)
    hub = cfgmod.load({"HUB_LLM_WEIGHTS": "fp8"})
    assert pickle.loads(pickle.dumps({"cfg": hub}))["cfg"].gpu.llm_weights == "fp8"


def test_fp8_config():
    from loqa_hub_amd import config as cfgmod
    assert cfgmod.load({}).gpu.llm_weights == "bf16"
    assert cfgmod.load({"HUB_LLM_WEIGHTS": "fp8"}).gpu.llm_weights == "fp8"
    with pytest.raises(cfgmod.ConfigError, match="HUB_LLM_WEIGHTS"):
        cfgmod.load({"HUB_LLM_WEIGHTS": "int4"})
    with pytest.raises(cfgmod.ConfigError, match="HUB_TP"):
        cfgmod.load({"HUB_LLM_WEIGHTS": "fp8", "HUB_TP": "2"})
    with pytest.raises(cfgmod.ConfigError, match="HUB_LLM_BACKEND"):
        cfgmod.load({"HUB_LLM_WEIGHTS": "fp8", "HUB_LLM_BACKEND": "ollama"})


def test_fp8_tuning_keys_do_not_collide():
    w = _spread_rows(64, 256)
    assert ops._wtag(ops.shuffle_weight(w)) == () and ops._wtag(ops.quantize_weight_fp8(w)) == ("fp8",)
    assert ops._fsplit_override(("silu", 64, 256, 16)) is None
    import os
    os.environ["LOQA_FSPLIT_OVERRIDE"] = "silu:64x256:M16=2,2,1;silu:64x256:M16:fp8=1,1,1"
    try:
        assert ops._fsplit_override(("silu", 64, 256, 16)) == (2, 2, 1)
        assert ops._fsplit_override(("silu", 64, 256, 16, "fp8")) == (1, 1, 1)
    finally:
        del os.environ["LOQA_FSPLIT_OVERRIDE"]


# ----------------------------------------------------------------------- GPU
def _exact_weights(N, K, seed, zero_from=None):
    """(q e4m3 [N, K], scale [N] = 2^((n % 7) - 3)): q * scale is exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(N, K, generator=g) * 0.05).to(FP8)
    if zero_from is not None:
        q = q.view(torch.uint8).clone()
        q[zero_from:] = 0
        q = q.view(FP8)
    scale = torch.exp2((torch.arange(N) % 7 - 3).float())
    return q, scale


def _fp8_from(q, scale, dev):
    N, K = q.shape
    return ops.Fp8Weight(ref.shuffle_fp8(q.view(torch.uint8)).to(dev), scale.to(dev), N, K)


def _run_fused(dev, wp, mode, x, Mpad, rt, wr, S, xl, norm, res0, cs, rowsq, tiles=4):
    N = N_OF[mode]
    scr = ops.FusedScratch(dev)
    kw = dict(splits=S, wr=wr, rt=rt, xl=xl)
    if norm:
        scr.rowsq[: tiles * Mpad].copy_(rowsq.to(dev))
        kw.update(norm=norm, rowsq_tiles=tiles)
    xd = x.to(dev)
    if mode == "resid":
        res = res0.clone().to(dev)
        ops.skinny_fused(xd, wp, "resid", scr, residual=res, **kw)
        return [res.cpu(), scr.rowsq[: (N // (16 * rt)) * Mpad].cpu()]
    if mode == "rope":
        kc = torch.zeros(max(4, Mpad // 16), HKV, 16, D, device=dev).bfloat16()
        vc = torch.zeros_like(kc)
        pos = (torch.arange(Mpad, dtype=torch.int32) * 3 + 5).to(dev)
        slots = torch.arange(Mpad, dtype=torch.int32, device=dev)
        qo = torch.empty(Mpad, H * D, device=dev).bfloat16()
        ops.skinny_fused(xd, wp, "rope", scr, positions=pos, cos_sin=cs.to(dev), q_out=qo, k_cache=kc,
                         v_cache=vc, slots=slots, n_heads=H, n_kv=HKV, head_dim=D, **kw)
        return [qo.cpu(), kc.cpu(), vc.cpu()]
    return [ops.skinny_fused(xd, wp, mode, scr, **kw).cpu()]


def _rejected(e: RuntimeError) -> bool:
    return "failed with hipError 1" in str(e)       # hipErrorInvalidValue: nothing was launched


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 768, 1024, 1536])
@pytest.mark.parametrize("norm", [None, "rms"])
@pytest.mark.parametrize("mode", ["resid", "silu", "act", "rope"])
def test_fp8_fused_bitwise_vs_bf16_kernel_gpu(mode, norm, K):
    """The fp8 kernel on (q, power-of-two row scales) against the bf16 kernel
    on the (exactly) dequantised weights, same layout: bitwise equal, every
    output. K = 1536: an odd number of prefetch groups per wave (the ping-pong
    tail). A layout is skipped only when the host dispatch rejects it for fp8
    at this K; at most two of the eight.
    K = 256 and 768: with 4 waves along K the fp8 stream's two-k-step group, in
    one and in three groups. These K do not divide by every layout's split, so
    they run the layouts the entry checks take (K % (S * 128) == 0 and, fp8,
    K % (S * waves-along-K * 64) == 0) and none of those may be rejected."""
    if norm and mode == "resid":
        pytest.skip("no residual GEMM takes a norm prologue (it would rewrite the statistics it reads)")
    dev = "cuda"
    N = N_OF[mode]
    q, scale = _exact_weights(N, K, seed=11)
    w8 = _fp8_from(q, scale, dev)
    wb = ops.shuffle_weight((q.float() * scale[:, None]).bfloat16().to(dev))
    assert torch.equal(ref.unshuffle_weight(wb.cpu()).float(), ref.dequant_fp8(w8.to("cpu")))
    g = torch.Generator().manual_seed(5)
    cs = ref.rope_cos_sin(D, 512, 10000.0)
    skipped = []
    layouts = LAYOUTS
    if K < 1024:
        layouts = [l for l in LAYOUTS if K % (l[3] * 128) == 0 and K % (l[3] * (1 if l[2] == 4 else 4) * 64) == 0]
        assert (16, 1, 1, 1, 0) in layouts and len(layouts) >= 5
    for Mpad, rt, wr, S, xl in layouts:
        x = torch.randn(Mpad, K, generator=g).bfloat16()
        res0 = torch.randn(Mpad, N, generator=g).bfloat16()
        rowsq = torch.rand(4 * Mpad, generator=g) * 300 + 50
        args = (mode, x, Mpad, rt, wr, S, xl, norm, res0, cs, rowsq)
        try:
            got = _run_fused(dev, w8, *args)
        except RuntimeError as e:
            if not _rejected(e) or K < 1024:
                raise
            skipped.append((Mpad, rt, wr, S, xl))
            continue
        want = _run_fused(dev, wb, *args)
        for a, b in zip(got, want):
            assert torch.isfinite(a.float()).all()
            assert torch.equal(a, b), ((Mpad, rt, wr, S, xl), float((a.float() - b.float()).abs().max()))
    print("rejected for fp8:", skipped)
    assert len(skipped) <= 2, skipped


@pytest.mark.gpu
def test_fp8_fused_act_f32_bitwise_gpu():
    """act="f32" (f32 output, no rounding): the same bitwise check."""
    dev, K, N = "cuda", 1024, 512
    q, scale = _exact_weights(N, K, seed=12)
    w8 = _fp8_from(q, scale, dev)
    wb = ops.shuffle_weight((q.float() * scale[:, None]).bfloat16().to(dev))
    for Mpad, rt, wr, S, xl in [(16, 2, 1, 2, 0), (16, 1, 4, 1, 0), (128, 2, 4, 2, 1)]:
        x = torch.randn(Mpad, K).bfloat16().to(dev)
        scr = ops.FusedScratch(dev)
        a = ops.skinny_fused(x, w8, "act", scr, splits=S, rt=rt, wr=wr, xl=xl, act="f32")
        b = ops.skinny_fused(x, wb, "act", scr, splits=S, rt=rt, wr=wr, xl=xl, act="f32")
        assert a.dtype == torch.float32 and torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 768, 1024, 1536])
@pytest.mark.parametrize("Mpad", [16, 64])
def test_fp8_skinny_gemm_bitwise_vs_bf16_kernel_gpu(Mpad, K):
    """The lm_head form: slabs bitwise equal to the bf16 kernel's; N = 576
    padded to 640 with zero rows (scale 1), whose outputs are exactly 0.
    K = 256, 768: a wave's two-k-step group in one and in three groups (S = 1;
    S = 2 only where K % (S * 4 * 64) == 0, the fp8 entry check)."""
    dev, N, Np = "cuda", 576, 640
    q, scale = _exact_weights(Np, K, seed=13, zero_from=N)
    scale[N:] = 1.0
    w8 = _fp8_from(q, scale, dev)
    wb = ops.shuffle_weight((q.float() * scale[:, None]).bfloat16().to(dev))
    x = torch.randn(Mpad, K).bfloat16().to(dev)
    splits = [S for S in (1, 2) if K % (S * 4 * 64) == 0]
    assert 1 in splits and (K < 1024 or splits == [1, 2])
    for S in splits:
        a, b = ops.skinny_gemm(x, w8, S), ops.skinny_gemm(x, wb, S)
        assert a.shape == (S, Mpad, Np) and torch.equal(a, b)
        assert not a[:, :, N:].any()
        assert torch.equal(ops.skinny_gemm(x, w8, S, max_wgs=4), a)     # capped grid: tile-group loop
    with pytest.raises(RuntimeError, match="hipError 1"):               # a wave's k range must be even
        ops.skinny_gemm(x, w8, K // 128)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [(16, 2, 1, 1, 0), (64, 2, 4, 1, 1), (128, 1, 4, 2, 1)])
@pytest.mark.parametrize("mode", ["resid", "silu", "act", "rope"])
def test_fp8_fused_vs_fp32_reference_gpu(mode, layout):
    """Arbitrary bf16 weights (row magnitudes 2^-3 .. 2^3, so a wrong or
    unpermuted scale index is a gross error) through ``quantize_weight_fp8``
    against the fp32 CPU reference of the same call; the bf16 kernels' metric
    and bound (tests/test_fused_decode.py): relative Frobenius error < 1e-2."""
    Mpad, rt, wr, S, xl = layout
    K, N = 1024, N_OF[mode]
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(N, K, generator=g) * 0.03 * torch.exp2(torch.rand(N, 1, generator=g) * 6 - 3)).bfloat16()
    if mode == "silu":
        w = w[ref.perm_gate_up(N // 2)].contiguous()
    elif mode == "rope":
        w = w[ref.perm_rope_qkv(H, HKV, D)].contiguous()
    fw = ops.quantize_weight_fp8(w)
    fg = fw.to("cuda")                               # the same bytes and scales on both sides
    x = torch.randn(Mpad, K, generator=g).bfloat16()
    res0 = torch.randn(Mpad, N, generator=g).bfloat16()
    cs = ref.rope_cos_sin(D, 512, 10000.0)
    rowsq = torch.rand(4 * Mpad, generator=g) * 300 + 50
    norm = None if mode == "resid" else "rms"
    args = (mode, x, Mpad, rt, wr, S, xl, norm, res0, cs, rowsq)
    want = _run_fused("cpu", fw, *args)
    got = _run_fused("cuda", fg, *args)
    for a, b in zip(got, want):
        rel = float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-6))
        print(mode, layout, "rel", rel)
        assert rel < 1e-2, rel


@pytest.mark.gpu
def test_fp8_hostile_memory_gpu():
    """The fp8 bytes and the scales inside larger allocations filled with NaN
    (0x7f is NaN in e4m3fn): results unchanged, so nothing is read past them."""
    dev, K, N = "cuda", 1024, 512
    q, scale = _exact_weights(N, K, seed=14)
    clean = _fp8_from(q, scale, dev)
    pad = 1 << 16
    big = torch.full((pad + N * K + pad,), 0x7F, dtype=torch.uint8, device=dev)
    big[pad: pad + N * K] = clean.wp.flatten()
    sbig = torch.full((1024 + N + 1024,), float("nan"), device=dev)
    sbig[1024: 1024 + N] = clean.scale
    hostile = ops.Fp8Weight(big[pad: pad + N * K].view(N // 16, K // 64, 64, 16), sbig[1024: 1024 + N], N, K)
    assert hostile.wp.data_ptr() == big.data_ptr() + pad
    for Mpad, rt, wr, S, xl in [(16, 2, 1, 1, 0), (16, 1, 1, 4, 0), (16, 2, 4, 1, 0), (64, 4, 4, 1, 0),
                                (128, 2, 4, 4, 1)]:
        x = torch.randn(Mpad, K).bfloat16().to(dev)
        scr = ops.FusedScratch(dev)
        a = ops.skinny_fused(x, hostile, "act", scr, splits=S, rt=rt, wr=wr, xl=xl)
        b = ops.skinny_fused(x, clean, "act", scr, splits=S, rt=rt, wr=wr, xl=xl)
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    for Mpad in (16, 64):
        x = torch.randn(Mpad, K).bfloat16().to(dev)
        for S in (1, 4):
            a = ops.skinny_gemm(x, hostile, S)
            assert torch.isfinite(a).all() and torch.equal(a, ops.skinny_gemm(x, clean, S))


@pytest.mark.gpu
def test_fp8_fused_rejects_unsupported_gpu():
    """LayerNorm and k ranges that are not whole k-step pairs are refused by the
    host dispatch (hipErrorInvalidValue), never launched."""
    dev, K, N = "cuda", 1536, 512
    q, scale = _exact_weights(N, K, seed=15)
    w8 = _fp8_from(q, scale, dev)
    x = torch.randn(16, K).bfloat16().to(dev)
    scr = ops.FusedScratch(dev)
    with pytest.raises(RuntimeError, match="hipError 1"):
        ops.skinny_fused(x, w8, "act", scr, splits=4, rt=2, wr=1, xl=0)    # 1536 % (4 * 4 * 64) != 0
    p = ops.FusedParams()
    p.x, p.ldx, p.Wp, p.wscale, p.wdtype = x.data_ptr(), K, w8.wp.data_ptr(), w8.scale.data_ptr(), 1
    out = torch.empty(16, N, device=dev).bfloat16()
    p.Mpad, p.N, p.K, p.S, p.mode, p.norm = 16, N, K, 1, 4, 2                # LayerNorm
    p.rowsq_in = p.rowsum_in = p.colsum = scr.rowsq.data_ptr()
    p.rowstat_tiles, p.out, p.ldo, p.rt, p.wr = 1, out.data_ptr(), N, 2, 1
    import ctypes
    assert ops.kernels().loqa_skinny_fused(ctypes.byref(p), torch.cuda.current_stream().cuda_stream) == 1
    p.norm, p.wscale = 0, None                                              # no scale pointer
    assert ops.kernels().loqa_skinny_fused(ctypes.byref(p), torch.cuda.current_stream().cuda_stream) == 1
    torch.cuda.synchronize()


def _fp8_engine_logits(device, Mpad, tok):
    from loqa_hub_amd.engine.llm_engine import LLMEngine
    from loqa_hub_amd.models.configs import llama_config
    from tests.test_fused_decode import _decode_logits
    eng = LLMEngine(llama_config("test-tiny"), device, max_seqs=8, use_graphs=False, weight_dtype="fp8")
    return eng, (lambda: _decode_logits(eng, True, 100, tok, Mpad))


_CPU_LOGITS: dict = {}


@pytest.mark.gpu
@pytest.mark.parametrize("splits,Mpad", [(None, 16), (2, 16), (None, 64)])
def test_fp8_engine_gpu_matches_cpu(splits, Mpad):
    """The fp8 ``test-tiny`` engine on the GPU against the same engine (the
    same e4m3 bytes and scales) on the CPU: logits within the bound the bf16
    fused / unfused comparison uses (2e-2)."""
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(10, 4000, (3, 12), generator=g).tolist()
    if Mpad not in _CPU_LOGITS:
        _CPU_LOGITS[Mpad] = _fp8_engine_logits("cpu", Mpad, tok)[1]()
    eng, run = _fp8_engine_logits("cuda", Mpad, tok)
    saved_s, saved_f = dict(ops._SPLITS), dict(ops._FSPLITS)
    try:
        if splits is not None:   # force split-K where the fp8 k granule allows it
            ops._FSPLITS.clear()
            d, w = eng.cfg.d_model, eng.weights
            for N, K in ((w.h * 64 + 2 * w.hkv * 64, d), (d, w.h * 64), (2 * w.f, d), (d, w.f)):
                for mp in (16, 32, 64):
                    ops._SPLITS[(N, K, mp, "fp8")] = max(
                        s for s in ops.SPLIT_CANDIDATES if s <= splits and K % (s * 256) == 0)
            assert 2 in ops._SPLITS.values()
        got = run()
    finally:
        ops._SPLITS.clear(); ops._SPLITS.update(saved_s)
        ops._FSPLITS.clear(); ops._FSPLITS.update(saved_f)
    for a, b in zip(got, _CPU_LOGITS[Mpad]):
        assert torch.isfinite(a).all()
        rel = float((a - b).norm() / (b.norm() + 1e-12))
        print("fp8 engine gpu vs cpu rel", rel)
        assert rel < 2e-2, rel


@pytest.mark.gpu
def test_fp8_engine_graphs_match_eager_gpu():
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
    (a, ta), (b, tb) = (gen(LLMEngine(cfg, "cuda", max_seqs=8, use_graphs=g, weight_dtype="fp8"))
                        for g in (True, False))
    for x, y, tx, ty, n in zip(a, b, ta, tb, [1, 2, 3]):
        assert tx and tx == ty and x.output == y.output
        assert len(json.loads(x.output)["commands"]) == n


@pytest.mark.gpu
def test_fp8_hub_served_gpu(tmp_path, monkeypatch):
    """``HUB_LLM_WEIGHTS=fp8`` serves the hub end to end on one GPU: the served-
    hub checks (both commands of the utterance on the bus, the voice event, the
    spoken reply), with the fp8 weights visible on /api/metrics."""
    import tests.test_hub_served as hs
    load = hs.cfgmod.load
    monkeypatch.setattr(hs.cfgmod, "load", lambda env=None: load({**env, "HUB_LLM_WEIGHTS": "fp8"}))
    res = hs._served(tmp_path, "cuda:0", streaming=True, llm="test-tiny", stt="whisper-tiny",
                     tts_model="test-vits")
    hs._check_served(*res, streaming=True, relays=("kitchen-relay",))
    assert 'loqa_llm_weight_dtype{dtype="fp8"} 1.0' in res[5]
    assert "loqa_llm_weight_bytes " in res[5]
