// LDS-tiled MFMA GEMM for large-M projections: Y[M, N] = X[M, K] W[N, K]^T.
//
// Where it runs: the Whisper encoder projections (M =
// 1500 per utterance), the conv stem (k = 3 conv1d as an implicit im2col over
// the time-major input rows), the cross-attention K/V of all decoder layers in
// one launch, and the Llama prompt qkv / gate|up (SwiGLU epilogue). Both
// operands are K-contiguous row-major tensors (nn.Linear weights as loaded, no
// shuffled copy).
//
// Structure: see gemm_mfma.h (wave tiles, swizzled global_load_lds stages,
// counted vmcnt, MFMA step, epilogues). Here:
//   * workgroup = WN x WM waves, one ring of NBUF stages of (BN + BM) rows;
//   * XCD-aware workgroup order (xcd_remap), m fastest: consecutive workgroups
//     of an XCD share the weight tile in its L2;
//   * split-K S writes f32 slabs [S, M, N] that a slab consumer sums (EPI_SLABS);
//   * CONV: the activation rows are gathered by the loader (implicit im2col).
#include "gemm_mfma.h"

struct GemmTileParams {
  const void* x; long long ldx;   // [M, K] rows (conv: input rows [B * conv_tin, cin], row stride ldx)
  const void* w;                  // [N, K] row-major; SwiGLU: gate rows [0, N/2), up rows [N/2, N)
  int M, N, K, S;
  int epi, act;                   // EPI_BF16 / EPI_SWIGLU / EPI_SLABS; act: 0 none, 1 GELU (erf)
  const float* bias;              // [N] f32 or null (bf16 / slabs with S == 1)
  const void* pos; int pos_rows;  // bf16 [pos_rows, N] added after act, row m % pos_rows; or null
  void* y; long long ldy;         // bf16 out (SwiGLU: [M, N/2])
  float* part;                    // f32 slabs [S, M, N]
  int conv_cin, conv_tin, conv_tout, conv_stride;  // conv_cin > 0: implicit im2col, k = tap * cin + c
  const void* zeros;              // >= conv_cin zero bf16 (conv taps outside the input)
  int layout;
};

template <int WN, int WM, int FN, int FM, int NBUF, int EPI, bool CONV>
__global__ __launch_bounds__(64 * WN * WM) void gemm_tile_kernel(GemmTileParams p) {
  constexpr int NW = WN * WM;
  constexpr int TN = 16 * FN, TM = 16 * FM;      // wave tile: TN features x TM rows
  constexpr int BN = TN * WN, BM = TM * WM;
  constexpr int ROWS = BN + BM;
  constexpr int STAGE = ROWS * 128;             // bytes per stage
  constexpr int IPW = ROWS / 8 / NW;            // glds instructions per wave per stage
  static_assert(IPW * 8 * NW == ROWS, "stage rows must split evenly over the waves");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[NBUF * STAGE];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wn = wave % WN, wm = wave / WN;
  const int M = p.M, N = p.N;
  const int mblocks = (M + BM - 1) / BM, nblocks = N / BN;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int mb = id % mblocks, rest = id / mblocks;
  const int nb = rest % nblocks, s = rest / nblocks;
  if (s >= p.S) return;
  const int Ks = p.K / p.S, kbeg = s * Ks, nt = Ks / GEMM_BK;
  const int m0 = mb * BM, n0 = nb * BN;
  const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(p.x);
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(p.w);

  // per-lane source of each of this wave's stage instructions (k offset added per stage)
  const bf16_t* src[IPW];
  int cb[IPW], ct[IPW];          // conv: input row of (b, t, tap 0) and t * stride - 1
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int r = stage_row(wave * IPW + i, lane), c = stage_chunk(r, lane);
    cb[i] = r < BN ? -1 : 0;
    ct[i] = 0;
    if (r < BN) {
      src[i] = W + (size_t)weight_row<EPI == EPI_SWIGLU, TN>(r, n0, N) * p.K + c * 8;
    } else {
      const int m = min(m0 + r - BN, M - 1);
      if constexpr (CONV) {
        const int b = m / p.conv_tout, t = m - b * p.conv_tout;
        cb[i] = b * p.conv_tin;
        ct[i] = t * p.conv_stride - 1;
        src[i] = X + c * 8;
      } else {
        src[i] = X + (size_t)m * p.ldx + c * 8;
      }
    }
  }

  auto stage = [&](int buf, int kt) {
    const int kc = kbeg + kt * GEMM_BK;
    int tap = 0, c0 = kc;
    if constexpr (CONV) {
      tap = kc / p.conv_cin;
      c0 = kc - tap * p.conv_cin;
    }
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const bf16_t* g;
      if (CONV && cb[i] >= 0) {
        // conv input rows keep only their 16-byte chunk offset (c * 8) in src;
        // a tap outside [0, T_in) reads the same chunk of the zero row
        const int tt = ct[i] + tap;
        const int c8 = (int)(src[i] - X);
        g = (tt >= 0 && tt < p.conv_tin) ? X + (size_t)(cb[i] + tt) * p.ldx + c0 + c8
                                         : reinterpret_cast<const bf16_t*>(p.zeros) + c8;
      } else {
        g = src[i] + kc;
      }
      glds16(g, lds + buf * STAGE + (wave * IPW + i) * 1024);
    }
  };

  float4v acc[FN][FM];
  acc_zero(acc);
  const int fr = lane & 15, fq = lane >> 4;
  // prologue: NBUF - 1 stages in flight
  static_assert(NBUF == 2 || NBUF == 3, "the counted wait below covers rings of 2 and 3 stages");
  int issued = 0;
#pragma unroll
  for (int q = 0; q < NBUF - 1; ++q)
    if (q < nt) {
      stage(q, q);
      ++issued;
    }
  for (int t = 0; t < nt; ++t) {
    // stage t has landed once at most (issued - t - 1) newer stages are pending
    if (NBUF == 3 && issued - t - 1 >= 1) wait_vm<IPW>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    // the buffer refilled here was last read in iteration t - 1, which every
    // wave finished before the barrier above
    if (issued < nt) {
      stage(issued % NBUF, issued);
      ++issued;
    }
    // gemm_tile keeps the older "both halves up front" MFMA step
    const unsigned char* sb = lds + (t % NBUF) * STAGE;
    mfma_step_upfront(sb, wn * TN, sb, BN + wm * TM, fr, fq, acc);
  }

  epi_store<EPI>(acc, EpiOut{EPI == EPI_SLABS ? (void*)p.part : p.y, p.ldy, p.bias, p.act, p.pos, p.pos_rows},
                 m0 + wm * TM, M, n0 + wn * TN, N, (size_t)s * M, fr, fq);
}

template <int WN, int WM, int FN, int FM, int NBUF>
static int gt_launch(const GemmTileParams& p, hipStream_t st) {
  constexpr int BN = 16 * FN * WN, BM = 16 * FM * WM;
  if (p.N % BN || p.K % (p.S * GEMM_BK)) return (int)hipErrorInvalidValue;
  const int grid = ((p.M + BM - 1) / BM) * (p.N / BN) * p.S;
  dim3 block(64 * WN * WM);
  if (p.conv_cin > 0) {
    // the implicit-im2col loader's per-lane row state spills beside the
    // larger wave tiles: conv runs on the 64 x 64 wave tiles only
    if constexpr (FN * FM > 16) return (int)hipErrorInvalidValue;
    else {
      if (p.epi != EPI_BF16) return (int)hipErrorInvalidValue;
      hipLaunchKernelGGL((gemm_tile_kernel<WN, WM, FN, FM, NBUF, EPI_BF16, true>), dim3(grid), block, 0, st, p);
    }
  } else if (p.epi == EPI_SLABS) {
    hipLaunchKernelGGL((gemm_tile_kernel<WN, WM, FN, FM, NBUF, EPI_SLABS, false>), dim3(grid), block, 0, st, p);
  } else if (p.epi == EPI_SWIGLU) {
    hipLaunchKernelGGL((gemm_tile_kernel<WN, WM, FN, FM, NBUF, EPI_SWIGLU, false>), dim3(grid), block, 0, st, p);
  } else {
    hipLaunchKernelGGL((gemm_tile_kernel<WN, WM, FN, FM, NBUF, EPI_BF16, false>), dim3(grid), block, 0, st, p);
  }
  return (int)hipGetLastError();
}

// The layouts, once: X(layout, WN, WM, FN, FM, NBUF) = WN x WM waves of
// (16 FN features) x (16 FM rows), NBUF stages.
#define GT_LAYOUTS(X)                                              \
  X(0, 2, 2, 4, 4, 2) /* 128 x 128 */                              \
  X(1, 2, 2, 4, 4, 3) /* 128 x 128 */                              \
  X(2, 4, 2, 4, 4, 2) /* 256 x 128, 8 waves */                     \
  X(3, 2, 4, 4, 4, 2) /* 128 x 256, 8 waves */                     \
  X(4, 4, 2, 4, 4, 3) /* 256 x 128 */                              \
  X(5, 2, 4, 4, 4, 3) /* 128 x 256 */                              \
  X(6, 2, 4, 8, 4, 2) /* 256 x 256, wave tile 128 x 64 */          \
  X(7, 4, 2, 4, 8, 2) /* 256 x 256, wave tile 64 x 128 */          \
  X(8, 2, 2, 8, 4, 2) /* 256 x 128, 4 waves of 128 x 64 */         \
  X(9, 2, 2, 4, 8, 2) /* 128 x 256, 4 waves of 64 x 128 */

extern "C" int loqa_gemm_tile(const GemmTileParams* p, hipStream_t st) {
  if (!p || p->M <= 0 || p->S < 1 || !p->x || !p->w) return (int)hipErrorInvalidValue;
  if (p->epi != EPI_BF16 && p->epi != EPI_SWIGLU && p->epi != EPI_SLABS) return (int)hipErrorInvalidValue;
  if (p->epi == EPI_SLABS ? !p->part : !p->y) return (int)hipErrorInvalidValue;
  if (p->epi != EPI_SLABS && p->S != 1) return (int)hipErrorInvalidValue;
  if (p->ldx % 8 || (p->epi != EPI_SLABS && p->ldy % 4)) return (int)hipErrorInvalidValue;
  if (p->epi == EPI_SWIGLU && (p->bias || p->pos || p->act)) return (int)hipErrorInvalidValue;
  if (p->pos && p->pos_rows < 1) return (int)hipErrorInvalidValue;
  if (p->conv_cin > 0 && (p->conv_cin % GEMM_BK || p->K != 3 * p->conv_cin || !p->zeros ||
                          p->conv_tout < 1 || p->conv_stride < 1 || p->M % p->conv_tout))
    return (int)hipErrorInvalidValue;
  switch (p->layout) {
#define X(L, WN, WM, FN, FM, NBUF) \
  case L: return gt_launch<WN, WM, FN, FM, NBUF>(*p, st);
    GT_LAYOUTS(X)
#undef X
    default: return (int)hipErrorInvalidValue;
  }
}

// tile geometry of a layout (features, rows)
extern "C" int loqa_gemm_tile_dims(int layout, int* bn, int* bm) {
  switch (layout) {
#define X(L, WN, WM, FN, FM, NBUF) \
  case L: *bn = 16 * FN * WN, *bm = 16 * FM * WM; return 0;
    GT_LAYOUTS(X)
#undef X
    default: return (int)hipErrorInvalidValue;
  }
}
