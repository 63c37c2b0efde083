// The fp8 (OCP e4m3fn) weight stream of the decode GEMMs: weight-only W8A16.
// The kernels are the ones of gemm_skinny.h with the weight fragments loaded
// as raw fp8 bytes (half the HBM traffic, half the prefetch registers),
// converted exactly to bf16 in registers in front of the same
// v_mfma_f32_16x16x32_bf16 pipeline, and a per-row f32 scale applied to the
// finished accumulator. With power-of-two scales the results are bitwise those
// of the bf16 kernel on the dequantised weights (tests/test_fp8_weights.py).
// Instantiated: modes silu / resid / rope / act x NORM_NONE / NORM_RMS.
#include "gemm_skinny.h"

int loqa_skinny_fused_fp8_launch(const FusedArgs& a, int mode, int norm, int rt, int wr, int xl,
                                 hipStream_t st) {
  return dispatch_mode<1>(a, mode, norm, rt, wr, xl, st);
}

// x: [Mpad, >=K] bf16; Wp8: e4m3fn bytes [N/16][K/64][64][16]; wscale: f32 [N];
// part: [S, Mpad, N] f32, already scaled (sum over S = x @ (q * scale)^T).
// K % (S * 4 * 64) == 0: a wave's k range is a whole number of k-step pairs.
extern "C" int loqa_skinny_gemm_fp8(const void* x, long long ldx_, const void* Wp8, const float* wscale,
                                    float* part, int Mpad, int N, int K, int S, int max_wgs,
                                    hipStream_t st) {
  if (S < 1 || K % (S * 4 * 64) != 0 || ldx_ % 8 != 0 || N % 16 != 0 || !wscale)
    return (int)hipErrorInvalidValue;
  return dispatch_skinny<fp8_t>(SkinnyArgs{x, ldx_, Wp8, wscale, part, N, K, S, Mpad, max_wgs}, st);
}
