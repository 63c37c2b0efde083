// The MXFP4 (OCP microscaling: e2m1 elements, one e8m0 power-of-two scale per
// 32 consecutive k values of a row) weight stream of the fused decode GEMMs:
// weight-only W4A16, 4.25 bits per weight. The kernels are the ones of
// gemm_skinny.h with the weight fragments loaded as raw nibbles (a quarter of
// the bf16 HBM traffic and prefetch registers) plus one scale byte per
// (row, k-step), converted to bf16 in registers - v_cvt_scalef32_pk_bf16_fp4,
// exactly: a scale block is one k-step of v_mfma_f32_16x16x32_bf16 and every
// e2m1 * 2^e the quantiser emits is a normal bf16 - in front of the same MFMA
// pipeline in the same k order. Nothing is applied to the accumulator, so the
// results are bitwise those of the bf16 kernel on the dequantised weights for
// every scale (tests/test_mxfp4_weights.py).
// Instantiated: modes silu / resid / rope / act x NORM_NONE / NORM_RMS. There
// is no MXFP4 instance of the plain skinny GEMM: the lm_head and the compact
// sampling heads stay on the fp8 stream.
#include "gemm_skinny.h"

// x: [Mpad, >=K] bf16; a.Wp: nibble bytes [N/16][K/128][64][16]; a.wscale: e8m0
// bytes [N/16][K/128][16][4]. K % (S * waves-along-K * 128) == 0: a wave's k
// range is a whole number of 4-k-step loads (checked here, before any launch).
int loqa_skinny_fused_mxfp4_launch(const FusedArgs& a, int mode, int norm, int rt, int wr, int xl,
                                   hipStream_t st) {
  if (!a.wscale || a.K % (a.S * (wr == 4 ? 1 : 4) * 128)) return (int)hipErrorInvalidValue;
  return dispatch_mode<WF_MXFP4>(a, mode, norm, rt, wr, xl, st);
}
