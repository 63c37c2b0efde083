"""ctypes bindings for the in-tree native libraries (``loqa_hub_amd/_native``).

The libraries are loaded lazily, always *after* ``import torch`` so they bind
to the HIP runtime torch already mapped (same soname ``libamdhip64.so.7``).
On a GPU box a missing library is a hard error: GPU ops never silently fall
back to PyTorch.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must be imported before the HIP libraries)

_HERE = os.path.dirname(os.path.abspath(__file__))
_NATIVE = os.path.join(os.path.dirname(_HERE), "_native")
_lock = threading.Lock()
_kernels = None
_runtime = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_ll = ctypes.c_longlong
c_float = ctypes.c_float

class FusedParams(ctypes.Structure):
    """Mirror of ``FusedParams`` in csrc/kernels/gemm_skinny.h."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_ll), ("Wp", c_void_p), ("part", c_void_p),
        ("counters", c_void_p),
        ("Mpad", c_int), ("N", c_int), ("K", c_int), ("S", c_int), ("mode", c_int),
        ("norm", c_int),
        ("rowsq_in", c_void_p), ("rowsum_in", c_void_p), ("rowstat_tiles", c_int),
        ("eps", c_float),
        ("colsum", c_void_p), ("bias", c_void_p),
        ("out", c_void_p), ("ldo", c_ll), ("act", c_int),
        ("residual", c_void_p), ("rowsq_out", c_void_p), ("rowsum_out", c_void_p),
        ("positions", c_void_p), ("cs", c_void_p), ("q_out", c_void_p), ("kc", c_void_p),
        ("vc", c_void_p), ("slots", c_void_p),
        ("H", c_int), ("Hkv", c_int), ("D", c_int), ("blk", c_int),
        ("rt", c_int), ("wr", c_int), ("xl", c_int),
        ("wdtype", c_int), ("wscale", c_void_p),
    ]


class GemmTileParams(ctypes.Structure):
    """Mirror of ``GemmTileParams`` in csrc/kernels/gemm_tile.hip (``epi``: the
    numbering of csrc/kernels/gemm_mfma.h, as ``ops.gemm._EPI``)."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_ll), ("w", c_void_p),
        ("M", c_int), ("N", c_int), ("K", c_int), ("S", c_int),
        ("epi", c_int), ("act", c_int), ("bias", c_void_p),
        ("pos", c_void_p), ("pos_rows", c_int),
        ("y", c_void_p), ("ldy", c_ll), ("part", c_void_p),
        ("conv_cin", c_int), ("conv_tin", c_int), ("conv_tout", c_int), ("conv_stride", c_int),
        ("zeros", c_void_p), ("layout", c_int),
    ]


class GemmSkParams(ctypes.Structure):
    """Mirror of ``GemmSkParams`` in csrc/kernels/gemm_sk.hip."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_ll), ("w", c_void_p),
        ("M", c_int), ("N", c_int), ("K", c_int), ("S", c_int),
        ("epi", c_int), ("act", c_int), ("bias", c_void_p),
        ("y", c_void_p), ("ldy", c_ll),
        ("ws", c_void_p), ("counters", c_void_p), ("layout", c_int),
    ]


class GemmWsParams(ctypes.Structure):
    """Mirror of ``GemmWsParams`` in csrc/kernels/gemm_ws.hip."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_ll), ("w", c_void_p),
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("epi", c_int), ("act", c_int), ("bias", c_void_p),
        ("y", c_void_p), ("ldy", c_ll), ("bm", c_int),
        ("S", c_int), ("ws", c_void_p), ("counters", c_void_p),
    ]


_KERNEL_SIGS = {
    "loqa_rmsnorm": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p,
                     c_void_p],
    "loqa_layernorm": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float,
                       c_void_p, c_void_p],
    "loqa_silu_mul": [c_void_p, c_void_p, c_ll, c_int, c_void_p],
    "loqa_gelu_bias": [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, c_void_p],
    "loqa_rope_kv_append": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_int, c_int, c_int, c_int, c_int, c_void_p],
    "loqa_pcm16_f32_sumsq": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_ll, c_void_p],
    "loqa_pcm16_f32_pad": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_ll, c_void_p],
    # (pcm, out, rows, rows_host, sumsq, nrows, ld, stream)
    "loqa_pcm16_resample_pad": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_ll,
                                c_void_p],
    # (in, ld_in, max_in, n, n_is64, out, ld_out, n_out, B, L, M, T, table, stream)
    "loqa_pcm16_resample": [c_void_p, c_ll, c_ll, c_void_p, c_int, c_void_p, c_ll, c_void_p, c_int, c_int,
                            c_int, c_int, c_void_p, c_void_p],
    # (pcm, ld, N, lens, lens_is64, R, rate, block, out, cap, out_len, staging, sizes, offsets,
    #  stream)
    "loqa_flac_encode": [c_void_p, c_ll, c_ll, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                         c_ll, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "loqa_masked_argmax": [c_void_p, c_int, c_ll, c_int, c_int, c_void_p, c_void_p, c_int,
                           # (..., out_idx, workspace, token_ids, stream)
                           c_void_p, c_void_p, c_void_p, c_void_p],
    "loqa_attention": [c_void_p, c_ll, c_void_p, c_void_p, c_ll, c_void_p, c_ll, c_void_p,
                       c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                       c_int, c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                       c_void_p],
    "loqa_log_mel": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                     c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "loqa_im2col_k3": [c_void_p, c_ll, c_ll, c_ll, c_int, c_int, c_int, c_int, c_void_p,
                       c_void_p],
    "loqa_skinny_gemm": [c_void_p, c_ll, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                         c_void_p],
    "loqa_skinny_gemm_fp8": [c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                             c_int, c_int, c_void_p],
    "loqa_shuffle_weight": [c_void_p, c_void_p, c_int, c_int, c_void_p],
    "loqa_skinny_fused": [c_void_p, c_void_p],
    "loqa_skinny_fused_params_size": [],
    "loqa_skinny_fused_params_offsets": [c_void_p, c_int],
    "loqa_gemm_tile":[c_void_p, c_void_p],
    "loqa_gemm_tile_dims": [c_int, c_void_p, c_void_p],
    "loqa_gemm_sk": [c_void_p, c_void_p],
    "loqa_gemm_sk_dims": [c_int, c_void_p, c_void_p],
    "loqa_gemm_ws": [c_void_p, c_int, c_void_p],
    "loqa_attn_decode": [c_void_p, c_ll, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_ll,
                         c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                         c_int, c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                         c_int, c_int, c_void_p],
    "loqa_slab_rmsnorm": [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                          c_void_p, c_int, c_float, c_void_p],
    "loqa_slab_rope_append": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "loqa_slab_layernorm": [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                            c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p],
    "loqa_slab_bias_act": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                           c_void_p],
    "loqa_embed_pos": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "loqa_embed_stats": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_int, c_int, c_void_p],
    "loqa_conv1d": [c_void_p, c_ll, c_int, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_void_p,
                    c_ll, c_int, c_void_p, c_ll, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int,
                    c_float, c_int, c_int, c_void_p],
    "loqa_conv1d_form": [c_int, c_int, c_int, c_int],
    "loqa_relpos_attention": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                              c_int, c_int, c_int, c_int, c_int, c_float, c_void_p],
    "loqa_expand_sample": [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int,
                           c_int, c_float, ctypes.c_uint, c_void_p, c_void_p],
    "loqa_slab_silu_mul": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "loqa_slab_reduce": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "loqa_step_fetch": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                        c_int, c_int, c_void_p, c_void_p],
    "loqa_gemm_prefill2": [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int,
                           c_int, c_void_p],
    "loqa_init_uniform4": [c_void_p, c_ll, c_int, c_ll, c_ll, c_ll, ctypes.c_uint, c_float, c_void_p],
    "loqa_step_publish": [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                          c_void_p],
    "loqa_masked_argmax_lse": [c_void_p, c_int, c_ll, c_int, c_int, c_void_p, c_void_p, c_int,
                               # (..., out_idx, out_logprob, workspace, token_ids, stream)
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    # (out, logprobs, n, res, stride, res_lp, lp_stride, nres, ctr, row_slot, last_tok, stream)
    "loqa_step_publish_lp": [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                             c_void_p, c_void_p, c_void_p, c_void_p],
    "loqa_masked_argmax_lse_probe": [c_void_p, c_int, c_ll, c_int, c_int, c_void_p, c_void_p, c_int,
                                     # (..., probe, out_idx, out_logprob, out_probe, workspace,
                                     #  token_ids, stream)
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p],
    # (out, lp, lp2, n, res, stride, res_lp, lp_stride, plane, nres, ctr, row_slot, last_tok, stream)
    "loqa_step_publish_lp2": [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                              c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "loqa_masked_argmax_ts": [c_void_p, c_int, c_ll, c_int, c_int, c_void_p, c_void_p, c_int,
                              # (..., probe, ts_ctl, ts_state, row_slot, slots, ts_begin, ts_count,
                              #  eot, max_initial, out_idx, out_logprob, out_probe, workspace, stream)
                              c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                              c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "loqa_masked_argmax_sample": [c_void_p, c_int, c_ll, c_int, c_int, c_void_p, c_void_p, c_int,
                                  # (..., probe, ts_ctl, ts_state, row_slot, slots, ts_begin,
                                  #  ts_count, eot, max_initial, temp, rng, out_idx, out_logprob,
                                  #  out_probe, workspace, stream)
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p],
    # (rng, B, V, out, stream)
    "loqa_gumbel_noise": [c_void_p, c_int, c_int, c_void_p, c_void_p],
    # (q_ptrs[A], A, D, ldq, positions, slots, cu_q, row_slot, T, B, align_q, n_slots, n_ctx, stream)
    "loqa_align_record": [c_void_p, c_int, c_int, c_ll, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_int, c_int, c_void_p, c_int, c_int, c_void_p],
    # (align_q slot, rows, R, k_ptrs[A], A, D, n_ctx, ldk, F, scale, P, stream)
    "loqa_align_scores": [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_ll, c_int,
                          c_float, c_void_p, c_void_p],
    # (P, A, R, F, n_lead, out, stream)
    "loqa_align_cost": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    # (x, N, M, trace workspace, tok_frame, total, stream)
    "loqa_dtw": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    # (logits, is_bf16, ld, R, V, mask, mask_rows, W, eot, KB, cand_id, cand_lp, eot_lp,
    #  workspace, stream)
    "loqa_beam_topk": [c_void_p, c_int, c_ll, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                       c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "loqa_beam_topk_record_size": [],
    # (cand_id, cand_lp, eot_lp, cum_in, G, n_src, B, tok, parent, lp, cum_out, eot_score,
    #  eot_fin, stream)
    "loqa_beam_merge": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    # (k, v, L, blocks, block_bytes, pairs, P, stream)
    "loqa_kv_copy_blocks": [c_void_p, c_void_p, c_int, c_ll, c_ll, c_void_p, c_int, c_void_p],
    # (logits, is_bf16, ld, B, V, ctl, row_slot, hw_state, last_tok, slots, hdr, off, tok, dst,
    #  n_cap, t_cap, stream)
    "loqa_hotword_step": [c_void_p, c_int, c_ll, c_int, c_int, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                          c_void_p],
    "loqa_hotword_wg": [],
    # (pcm, pcm_len, descs, descs_host, U, E, E_cap, stream)
    "loqa_vad_energy": [c_void_p, c_ll, c_void_p, c_void_p, c_int, c_void_p, c_ll, c_void_p],
    # (descs, descs_host, U, E, E_cap, params_host, ws, ws_words, spans, cap, n_spans,
    #  speech_frames, stream)
    "loqa_vad_spans": [c_void_p, c_void_p, c_int, c_void_p, c_ll, c_void_p, c_void_p, c_ll,
                       c_void_p, c_int, c_void_p, c_void_p, c_void_p],
    "loqa_vad_tile": [],
}

# (argtypes, restype) of the custom all-reduce entry points (in the kernels library)
_CAR_SIGS = {
    "loqa_car_create": ([c_int, c_int, c_ll, c_ll], c_void_p),
    "loqa_car_inbuf": ([c_void_p, c_int], c_void_p),
    "loqa_set_launch_prio": ([c_int], None),
    "loqa_car_resid": ([c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p], c_int),
    "loqa_car_argmax": ([c_void_p, c_void_p, c_ll, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
                        c_int),
    "loqa_car_handle": ([c_void_p, c_void_p], c_int),
    "loqa_car_handle_size": ([], c_int),
    "loqa_car_open": ([c_void_p, c_void_p], c_int),
    "loqa_car_allreduce": ([c_void_p, c_void_p, c_void_p, c_ll, c_int, c_void_p], c_int),
    "loqa_car_error": ([c_void_p], c_int),
    "loqa_car_clear_error": ([c_void_p], c_int),
    "loqa_car_fill_inbuf": ([c_void_p, c_int, c_void_p, c_ll, c_void_p], c_int),
    "loqa_tp_emul_resid": ([c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p], c_int),
    "loqa_car_destroy": ([c_void_p], None),
}

_RUNTIME_SIGS = {
    "loqa_stager_create": ([c_int, c_ll, c_int], c_void_p),
    "loqa_stager_destroy": ([c_void_p], None),
    "loqa_stager_acquire": ([c_void_p], c_int),
    "loqa_stager_append": ([c_void_p, c_int, c_void_p, c_ll], c_ll),
    "loqa_stager_len": ([c_void_p, c_int], c_ll),
    "loqa_stager_host_ptr": ([c_void_p, c_int], c_void_p),
    "loqa_stager_upload": ([c_void_p, c_int, c_void_p, c_ll, c_void_p], c_int),
    "loqa_stager_release": ([c_void_p, c_int], None),
    "loqa_stager_set_stream": ([c_void_p, c_void_p, c_int], c_int),
    "loqa_stager_flush": ([c_void_p, c_int, c_ll], c_ll),
    "loqa_stager_flushed": ([c_void_p, c_int], c_ll),
    "loqa_memcpy_h2d_async": ([c_void_p, c_void_p, c_ll, c_void_p], c_int),
    "loqa_pool_create": ([c_int, c_int], c_void_p),
    "loqa_pool_destroy": ([c_void_p], None),
    "loqa_pool_debug_hash_mask": ([c_void_p, ctypes.c_ulonglong], None),
    "loqa_pool_free_blocks": ([c_void_p], c_int),
    "loqa_pool_add_seq": ([c_void_p, c_ll, c_void_p, c_int], c_ll),
    "loqa_pool_append": ([c_void_p, c_ll, c_int, c_void_p], c_int),
    "loqa_pool_cache_prefix": ([c_void_p, c_ll, c_void_p, c_int], c_int),
    "loqa_pool_block_table": ([c_void_p, c_ll, c_void_p, c_int], c_int),
    "loqa_pool_step_meta": ([c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int], c_int),
    "loqa_pool_seq_len": ([c_void_p, c_ll], c_ll),
    "loqa_pool_free_seq": ([c_void_p, c_ll], c_int),
    "loqa_pool_truncate": ([c_void_p, c_ll, c_ll], c_int),
    "loqa_tpctl_open": ([ctypes.c_char_p, c_int, c_int, c_int, c_ll], c_void_p),
    "loqa_tpctl_unlink": ([c_void_p], None),
    "loqa_tpctl_publish": ([c_void_p, c_void_p, c_ll, c_int, c_ll], c_int),
    "loqa_tpctl_recv": ([c_void_p, c_void_p, c_ll, ctypes.POINTER(c_int), c_ll], c_ll),
    "loqa_tpctl_close": ([c_void_p], None),
    "loqa_tpctl_beat": ([c_void_p], None),
    "loqa_tpctl_beat_age": ([c_void_p, c_int], c_ll),
}


class NativeLibraryMissing(RuntimeError):
    pass


def _load(name: str) -> ctypes.CDLL:
    path = os.path.join(_NATIVE, name)
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            f"{path} is missing: run `python -m loqa_hub_amd._native.build` (gfx950)")
    return ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def kernels() -> ctypes.CDLL:
    global _kernels
    if _kernels is None:
        with _lock:
            if _kernels is None:
                lib = _load("libloqa_kernels.so")
                for fn, sig in _KERNEL_SIGS.items():
                    f = getattr(lib, fn)
                    f.argtypes = sig
                    f.restype = c_int
                for fn, (args, res) in _CAR_SIGS.items():
                    f = getattr(lib, fn)
                    f.argtypes = args
                    f.restype = res
                _kernels = lib
    return _kernels


def runtime() -> ctypes.CDLL:
    global _runtime
    if _runtime is None:
        with _lock:
            if _runtime is None:
                lib = _load("libloqa_runtime.so")
                for fn, (args, res) in _RUNTIME_SIGS.items():
                    f = getattr(lib, fn)
                    f.argtypes = args
                    f.restype = res
                _runtime = lib
    return _runtime


def available() -> bool:
    try:
        kernels()
        return True
    except (NativeLibraryMissing, OSError):
        return False


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError {rc}")


def stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()
