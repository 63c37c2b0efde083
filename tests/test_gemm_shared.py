"""The contract the three tiled MFMA GEMMs share through csrc/kernels/gemm_mfma.h.

With no K split, gemm_tile, gemm_sk and gemm_ws accumulate every output
element over K in ascending 32-wide MFMA steps with the same operand roles (W
as A, X as B) and run the same epilogue arithmetic, so on the same inputs
their outputs are bitwise equal whatever the tile layout. With S K chunks
gemm_sk and gemm_ws both cut K at s * KT / S and sum the chunks in order
0..S-1. An edit to the shared header that changes one consumer only shows up
here.

Shapes: M = 70 (one full 64-row block + a ragged one; ragged for every larger
layout), N = 256 (a multiple of every layout's feature width), K = 384 (six
64-deep stages: even the 4-stage rings wrap)."""
import ctypes

import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import _lib

M, N, K = 70, 256, 384
SK = sorted(ops.SK_LAYOUTS)
TILE = sorted(ops.GEMM_TILE_LAYOUTS)


def test_layout_tables_match_the_kernels():
    """SK_LAYOUTS / gemm_tile_dims restate the kernels' layout lists: hold them
    to the exported loqa_gemm_*_dims (host-only calls, no GPU work)."""
    if not _lib.available():
        pytest.skip("native kernels library not built")
    lib = _lib.kernels()
    bn, bm = ctypes.c_int(), ctypes.c_int()
    for lay in SK:
        assert lib.loqa_gemm_sk_dims(lay, ctypes.byref(bn), ctypes.byref(bm)) == 0, lay
        assert (bn.value, bm.value) == ops.SK_LAYOUTS[lay][:2], lay
    assert lib.loqa_gemm_sk_dims(len(ops.SK_LAYOUTS), ctypes.byref(bn), ctypes.byref(bm)) != 0
    for lay in TILE:
        assert lib.loqa_gemm_tile_dims(lay, ctypes.byref(bn), ctypes.byref(bm)) == 0, lay
        assert (bn.value, bm.value) == ops.gemm_tile_dims(lay), lay
    assert lib.loqa_gemm_tile_dims(len(ops.GEMM_TILE_LAYOUTS), ctypes.byref(bn), ctypes.byref(bm)) != 0


def test_fused_params_mirror_has_the_kernels_size():
    """_lib.FusedParams is gemm_skinny.hip's FusedParams restated by hand: hold
    its size to the exported sizeof and the offset of every field, in
    declaration order, to the exported offsetof list - two same-sized fields
    swapped keep the size (host-only calls, no GPU work)."""
    if not _lib.available():
        pytest.skip("native kernels library not built")
    lib = _lib.kernels()
    assert ctypes.sizeof(_lib.FusedParams) == lib.loqa_skinny_fused_params_size()
    fields = [name for name, _ in _lib.FusedParams._fields_]
    off = (ctypes.c_int * (len(fields) + 8))()
    assert lib.loqa_skinny_fused_params_offsets(off, len(off)) == len(fields)
    assert [getattr(_lib.FusedParams, f).offset for f in fields] == list(off[: len(fields)])


@pytest.fixture(scope="module")
def inputs():
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(M, K, device=dev, generator=g).bfloat16()
    w = (torch.randn(N, K, device=dev, generator=g) * 0.05).bfloat16()
    b = torch.randn(N, device=dev, generator=g) * 0.1
    res = torch.randn(M, N, device=dev, generator=g).bfloat16()
    return x, w, b, res


def _all_equal(outs):
    """outs: [(label, tensor)]; every tensor bitwise equal to the first."""
    (l0, y0) = outs[0]
    assert torch.isfinite(y0.float()).all() and y0.float().abs().max() > 0
    for label, y in outs[1:]:
        assert torch.equal(y, y0), (label, "differs from", l0)


@pytest.mark.gpu
def test_bias_gelu_bitwise_equal_across_kernels(inputs):
    x, w, b, _ = inputs
    outs = [(("sk", l), ops.gemm_sk(x, w, bias=b, act="gelu", layout=l, splits=1)) for l in SK]
    outs += [(("tile", l), ops.gemm_tile(x, w, bias=b, act="gelu", layout=l)) for l in TILE]
    outs += [(("ws", d), ops.gemm_ws(x, w, bias=b, act="gelu", depth=d)) for d in (0, 1)]
    _all_equal(outs)


@pytest.mark.gpu
def test_swiglu_bitwise_equal_across_kernels(inputs):
    # every layout of the three kernels has an even fragment count along the
    # features, so all of them take the SwiGLU epilogue
    x, w, _, _ = inputs
    outs = [(("sk", l), ops.gemm_sk(x, w, epi="swiglu", layout=l, splits=1)) for l in SK]
    outs += [(("tile", l), ops.gemm_tile(x, w, epi="swiglu", layout=l)) for l in TILE]
    outs += [(("ws", d), ops.gemm_ws(x, w, epi="swiglu", depth=d)) for d in (0, 1)]
    assert outs[0][1].shape == (M, N // 2)
    _all_equal(outs)


@pytest.mark.gpu
def test_residual_add_bitwise_equal_sk_ws(inputs):
    x, w, b, res = inputs
    outs = [(("sk", l), ops.gemm_sk(x, w, epi="resid", bias=b, residual=res.clone(), layout=l, splits=1))
            for l in SK]
    outs += [(("ws", d), ops.gemm_ws(x, w, epi="resid", bias=b, residual=res.clone(), depth=d))
             for d in (0, 1)]
    assert not torch.equal(outs[0][1], res)
    _all_equal(outs)


@pytest.mark.gpu
def test_split_k_bitwise_equal_sk_ws_and_counters_left_zero(inputs):
    x, w, b, res = inputs
    S = 3
    outs = [(("sk", l), ops.gemm_sk(x, w, bias=b, act="gelu", layout=l, splits=S)) for l in SK]
    outs += [(("ws", d), ops.gemm_ws(x, w, bias=b, act="gelu", depth=d, splits=S)) for d in (0, 1)]
    _all_equal(outs)
    outs = [(("sk", l), ops.gemm_sk(x, w, epi="resid", bias=b, residual=res.clone(), layout=l, splits=S))
            for l in SK]
    outs += [(("ws", d), ops.gemm_ws(x, w, epi="resid", bias=b, residual=res.clone(), depth=d, splits=S))
             for d in (0, 1)]
    _all_equal(outs)
    torch.cuda.synchronize()
    assert ops._SK_WS
    for _, cnt in ops._SK_WS.values():
        assert int(cnt.abs().sum()) == 0
