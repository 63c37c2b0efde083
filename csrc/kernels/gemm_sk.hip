// Split-K LDS-tiled MFMA GEMM with an in-launch reduction and fused epilogues:
// Y[M, N] = X[M, K] W[N, K]^T for the projections of a prompt pass (Llama
// prefill: M = a few hundred to a few thousand rows) and the Whisper encoder.
//
// Why split-K inside the launch: at M ~ 300 a projection has few output tiles
// (qkv 6144 x 4096: 240 tiles of 128 x 64; o / down 4096 wide: 160), far fewer
// than the 256 CUs x 2-3 resident workgroups, and a whole tile's K loop is one
// workgroup's serial latency. Splitting each tile's K range over S workgroups
// fills the machine; the S partial accumulators are summed by the LAST
// workgroup of the tile to finish (splitk_reduce, see gemm_mfma.h), which then
// runs the epilogue - no f32 slabs for a later kernel to re-read and no extra
// launch. The sum is in fixed chunk order, so the result is bitwise identical
// whoever arrives last.
//
// Staging, fragments, the MFMA step and the epilogues (EPI_BF16, EPI_SWIGLU,
// EPI_RESID): see gemm_mfma.h. One ring of NBUF (BN + BM)-row stages, NBUF - 1
// in flight; XCD-aware workgroup order with a tile's K chunks adjacent on one
// XCD.
#include "gemm_mfma.h"

struct GemmSkParams {
  const void* x; long long ldx;   // [M, K] bf16 rows
  const void* w;                  // [N, K] bf16 row-major (SwiGLU: gate rows [0, N/2), up [N/2, N))
  int M, N, K, S;                 // S: K chunks per output tile
  int epi, act;                   // act (EPI_BF16): 0 none, 1 GELU (erf) after the bias
  const float* bias;              // [N] f32 or null (EPI_BF16, EPI_RESID)
  void* y; long long ldy;         // bf16 output (EPI_RESID: the residual, updated in place)
  float* ws;                      // S > 1: [tiles][S][BM * BN] f32 partials
  int* counters;                  // S > 1: [tiles] ints, zero on entry (left zero)
  int layout;
};

template <int WN, int WM, int FN, int FM, int NBUF, int EPI>
__global__ __launch_bounds__(64 * WN * WM) void gemm_sk_kernel(GemmSkParams p) {
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
  const int M = p.M, N = p.N, S = p.S;
  const int mblocks = (M + BM - 1) / BM;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int s = id % S, tile = id / S;
  const int mb = tile % mblocks, nb = tile / mblocks;
  const int KT = p.K / GEMM_BK;
  const int kt0 = (int)(((long long)s * KT) / S), kt1 = (int)(((long long)(s + 1) * KT) / S);
  const int m0 = mb * BM, n0 = nb * BN;
  const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(p.x);
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(p.w);

  // per-lane source of each of this wave's stage instructions (k offset added per stage)
  const bf16_t* src[IPW];
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int r = stage_row(wave * IPW + i, lane), c = stage_chunk(r, lane);
    if (r < BN) src[i] = W + (size_t)weight_row<EPI == EPI_SWIGLU, TN>(r, n0, N) * p.K + c * 8;
    else src[i] = X + (size_t)min(m0 + r - BN, M - 1) * p.ldx + c * 8;
  }

  float4v acc[FN][FM];
  acc_zero(acc);
  const int fr = lane & 15, fq = lane >> 4;
  auto stage = [&](int buf, int t) { stage_issue<IPW>(src, (kt0 + t) * GEMM_BK, lds + buf * STAGE, wave); };
  const int nt = kt1 - kt0;
  int issued = 0;
#pragma unroll
  for (int q = 0; q < NBUF - 1; ++q)
    if (q < nt) {
      stage(q, q);
      ++issued;
    }
  for (int t = 0; t < nt; ++t) {
    // stage t has landed once at most (issued - t - 1) newer stages are pending
    // (up to NBUF - 2 in steady state; fewer in the last iterations)
    const int newer = issued - t - 1;
    if (NBUF >= 4 && newer >= 2) wait_vm<IPW * 2>();
    else if (NBUF >= 3 && newer >= 1) wait_vm<IPW>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    // the buffer refilled here was last read in iteration t - 1, which every
    // wave finished before the barrier above
    if (issued < nt) {
      stage(issued % NBUF, issued);
      ++issued;
    }
    const unsigned char* sb = lds + (t % NBUF) * STAGE;
    mfma_step(sb, wn * TN, sb, BN + wm * TM, fr, fq, acc);
  }

  if (S > 1 && !splitk_reduce<FN, FM, NW>(p.ws, p.counters, tile, s, S, reinterpret_cast<int*>(lds), wave, lane, acc))
    return;
  epi_store<EPI>(acc, EpiOut{p.y, p.ldy, p.bias, p.act, nullptr, 0}, m0 + wm * TM, M, n0 + wn * TN, N, 0, fr, fq);
}

template <int WN, int WM, int FN, int FM, int NBUF>
static int sk_launch(const GemmSkParams& p, hipStream_t st) {
  constexpr int BN = 16 * FN * WN, BM = 16 * FM * WM;
  if (p.N % BN || p.K % GEMM_BK || p.S > p.K / GEMM_BK) return (int)hipErrorInvalidValue;
  const long long tiles = (long long)((p.M + BM - 1) / BM) * (p.N / BN);
  const long long grid = tiles * p.S;
  if (grid > 0x7fffffff) return (int)hipErrorInvalidValue;
  dim3 block(64 * WN * WM);
  switch (p.epi) {
    case EPI_SWIGLU:
      if constexpr (FN % 2 == 0) {
        hipLaunchKernelGGL((gemm_sk_kernel<WN, WM, FN, FM, NBUF, EPI_SWIGLU>), dim3(grid), block, 0, st, p);
        break;
      } else {
        return (int)hipErrorInvalidValue;
      }
    case EPI_RESID:
      hipLaunchKernelGGL((gemm_sk_kernel<WN, WM, FN, FM, NBUF, EPI_RESID>), dim3(grid), block, 0, st, p);
      break;
    default:
      hipLaunchKernelGGL((gemm_sk_kernel<WN, WM, FN, FM, NBUF, EPI_BF16>), dim3(grid), block, 0, st, p);
  }
  return (int)hipGetLastError();
}

// The layouts, once: X(layout, WN, WM, FN, FM, NBUF) = WN x WM waves of
// (16 FN features) x (16 FM rows), NBUF stages of (BN + BM) x 128 B.
// (short-K shapes - the Whisper encoder's K = 1280, 20 stages - are bound by
// the bytes one CU keeps in flight: a deeper ring is the lever there)
#define SK_LAYOUTS(X)                                                              \
  X(0, 2, 2, 4, 4, 2)  /* 128 x 128, waves of 64 x 64, 64 KB LDS */                \
  X(1, 2, 2, 4, 2, 2)  /* 128 x  64, waves of 64 x 32, 48 KB */                    \
  X(2, 4, 1, 4, 4, 2)  /* 256 x  64, 80 KB */                                      \
  X(3, 4, 2, 4, 4, 2)  /* 256 x 128, 96 KB */                                      \
  X(4, 2, 2, 4, 2, 3)  /* 128 x  64, 72 KB */                                      \
  X(5, 2, 2, 4, 4, 3)  /* 128 x 128, 96 KB */                                      \
  X(6, 2, 4, 8, 4, 2)  /* 256 x 256, waves of 128 x 64, 128 KB */                  \
  X(7, 2, 2, 2, 2, 2)  /*  64 x  64, waves of 32 x 32, 32 KB */                    \
  X(8, 4, 1, 4, 4, 3)  /* 256 x  64, 120 KB */                                     \
  X(9, 4, 2, 4, 4, 3)  /* 256 x 128, 144 KB: two 48 KB stages in flight per CU */  \
  X(10, 2, 2, 4, 4, 4) /* 128 x 128, 128 KB */                                     \
  X(11, 2, 2, 4, 2, 4) /* 128 x  64, 96 KB */

extern "C" int loqa_gemm_sk(const GemmSkParams* p, hipStream_t st) {
  if (!p || p->M <= 0 || p->S < 1 || p->epi < 0 || p->epi > EPI_RESID || !p->x || !p->w || !p->y)
    return (int)hipErrorInvalidValue;
  if (p->S > 1 && (!p->ws || !p->counters)) return (int)hipErrorInvalidValue;
  if (p->ldx % 8 || p->ldy % 4) return (int)hipErrorInvalidValue;
  if ((p->epi == EPI_SWIGLU && p->bias) || (p->epi != EPI_BF16 && p->act)) return (int)hipErrorInvalidValue;
  switch (p->layout) {
#define X(L, WN, WM, FN, FM, NBUF) \
  case L: return sk_launch<WN, WM, FN, FM, NBUF>(*p, st);
    SK_LAYOUTS(X)
#undef X
    default: return (int)hipErrorInvalidValue;
  }
}

// tile geometry of a layout (features, rows) for the host-side planner
extern "C" int loqa_gemm_sk_dims(int layout, int* bn, int* bm) {
  switch (layout) {
#define X(L, WN, WM, FN, FM, NBUF) \
  case L: *bn = 16 * FN * WN, *bm = 16 * FM * WM; return 0;
    SK_LAYOUTS(X)
#undef X
    default: return (int)hipErrorInvalidValue;
  }
}
