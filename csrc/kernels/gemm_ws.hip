// Row-resident weight-streaming MFMA GEMM for prompt passes:
// Y[M, N] = X[M, K] W[N, K]^T with M up to a few hundred rows (one prefill pass
// of the intent decoder: ~300 - 1200 prompt tokens).
//
// At M ~ 300 a projection is bounded by streaming its weights (gate|up: 235 MB,
// ~45 us at HBM speed) about as much as by its MFMA work, and a square output
// tile either pads M badly (128-row tiles: 384 rows for 300) or re-reads every
// weight tile once per row block. Here a workgroup owns BN = 128 output
// features x ALL the pass's rows (BM = M rounded up to 64, at most 384), so
// every weight byte is read from HBM exactly once and the only re-read operand
// is the small activation block (L2-resident). 8 waves = 2 (features) x 4
// (rows); a wave computes 64 features x BM / 4 rows with 16x16x32 bf16 MFMAs.
//
// The two operands have different latencies, so they are staged at different
// depths (guide §5 "Pipelining across barriers"): weight K-stages (16 KB, from
// HBM) NBW deep, activation K-stages (BM x 128 B, from L2) NBX deep, all by
// global_load_lds with the bank swizzle on the source address, issued
// activation-first so ONE counted vmcnt per step (the newest weight stage may
// stay in flight) retires both; raw s_barrier, never __syncthreads in the loop.
//
// Staging, fragments, the MFMA step, the in-launch split-K reduction and the
// epilogues (EPI_BF16, EPI_SWIGLU, EPI_RESID): see gemm_mfma.h.
//
// Split-K (S > 1): the K range is cut into S chunks, each its own workgroup,
// summed inside the launch by the tile's last arriving chunk (splitk_reduce).
// A workgroup's operand ingestion is (BM + 128) x K/S: at ~300 rows
// the activation block dominates it, so fewer K per workgroup is what lets
// more workgroups than 128-feature tiles share the pass (down: 32 tiles x 8
// chunks). Chunk-major workgroup order: the workgroups of one K chunk (one
// activation slice, L2-resident) run together.
#include "gemm_mfma.h"

struct GemmWsParams {
  const void* x; long long ldx;   // [M, K] bf16 rows
  const void* w;                  // [N, K] bf16 row-major (SwiGLU: gate rows [0, N/2), up [N/2, N))
  int M, N, K;
  int epi, act;                   // act (EPI_BF16): 1 GELU (erf) after the bias
  const float* bias;              // [N] f32 or null (bf16 / resid)
  void* y; long long ldy;         // bf16 output (EPI_RESID: the residual, updated in place)
  int bm;                         // rows per workgroup (multiple of 64, <= 64 * FM of the launch)
  int S;                          // K chunks (>= 1)
  float* ws;                      // S > 1: [tiles][S][bm * 128] f32 partials
  int* counters;                  // S > 1: [tiles] ints, zero on entry (left zero)
};

template <int FM, int NBW, int NBX, int EPI>
__global__ __launch_bounds__(512) void gemm_ws_kernel(GemmWsParams p) {
  constexpr int WN = 2, WM = 4, NW = 8, FN = 4;
  constexpr int TN = 16 * FN, TM = 16 * FM;      // wave tile: 64 features x TM rows
  constexpr int BN = TN * WN, BM = TM * WM;      // 128 x 64 FM
  constexpr int WSTAGE = BN * 128, XSTAGE = BM * 128;
  constexpr int IW = BN / 8 / NW;                // glds per wave per weight stage (2)
  constexpr int IX = BM / 8 / NW;                // glds per wave per activation stage (FM)
  static_assert(IW * 8 * NW == BN && IX * 8 * NW == BM, "stage rows split evenly over the waves");
  static_assert(NBW >= 2 && NBX >= 2 && NBX <= NBW, "stage depths");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[NBW * WSTAGE + NBX * XSTAGE];
  unsigned char* const wl = lds;
  unsigned char* const xl = lds + NBW * WSTAGE;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wn = wave % WN, wm = wave / WN;
  const int M = p.M, N = p.N;
  const int mblocks = (M + p.bm - 1) / p.bm;
  const int tiles = mblocks * (N / BN), S = p.S;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int s = id / tiles, tile = id - s * tiles;
  const int mb = tile % mblocks, nb = tile / mblocks;   // a weight tile's row blocks adjacent
  const int m0 = mb * p.bm, n0 = nb * BN;
  const int KT = p.K / GEMM_BK;
  const int kt0 = (int)(((long long)s * KT) / S), kt1 = (int)(((long long)(s + 1) * KT) / S);
  const int nt = kt1 - kt0;
  const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(p.x);
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(p.w);

  const bf16_t* wsrc[IW];
#pragma unroll
  for (int i = 0; i < IW; ++i) {
    const int r = stage_row(wave * IW + i, lane), c = stage_chunk(r, lane);
    wsrc[i] = W + (size_t)weight_row<EPI == EPI_SWIGLU, TN>(r, n0, N) * p.K + (size_t)kt0 * GEMM_BK + c * 8;
  }
  const bf16_t* xsrc[IX];
#pragma unroll
  for (int i = 0; i < IX; ++i) {
    const int r = stage_row(wave * IX + i, lane), c = stage_chunk(r, lane);
    const int m = min(m0 + min(r, p.bm - 1), M - 1);
    xsrc[i] = X + (size_t)m * p.ldx + (size_t)kt0 * GEMM_BK + c * 8;
  }
  auto stage_w = [&](int kt) { stage_issue<IW>(wsrc, kt * GEMM_BK, wl + (kt % NBW) * WSTAGE, wave); };
  auto stage_x = [&](int kt) { stage_issue<IX>(xsrc, kt * GEMM_BK, xl + (kt % NBX) * XSTAGE, wave); };

  float4v acc[FN][FM];
  acc_zero(acc);
  const int fr = lane & 15, fq = lane >> 4;

  // Issue order, one virtual step v at a time: X(v + NBX - 1), then
  // W(v + NBW - 1). vmcnt retires in issue order, so at the top of step t the
  // wait is for the later-issued of X(t) / W(t); what was issued after it may
  // stay in flight: with NBX = 2 < NBW = 3 that is W(t + 1) (weights get two
  // steps of cover, activations one), with NBX = NBW = 3 it is X(t + 1) and
  // W(t + 1) (two steps for both). Near the end those stages do not exist.
  static_assert(NBW == 3 && (NBX == 2 || NBX == 3), "the counted waits below assume these depths");
  for (int v = -(NBW - 1); v < 0; ++v) {
    if (v + NBX - 1 >= 0 && v + NBX - 1 < nt) stage_x(v + NBX - 1);
    if (v + NBW - 1 < nt) stage_w(v + NBW - 1);
  }
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      if constexpr (NBX == 2) wait_vm<IW>();
      else wait_vm<IW + IX>();
    } else {
      wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
    // the buffers refilled here were last read in step t - 1, which every
    // wave finished before the barrier above
    if (t + NBX - 1 < nt) stage_x(t + NBX - 1);
    if (t + NBW - 1 < nt) stage_w(t + NBW - 1);
    mfma_step(wl + (t % NBW) * WSTAGE, wn * TN, xl + (t % NBX) * XSTAGE, wm * TM, fr, fq, acc);
  }

  if (S > 1 && !splitk_reduce<FN, FM, NW>(p.ws, p.counters, tile, s, S, reinterpret_cast<int*>(lds), wave, lane, acc))
    return;
  epi_store<EPI>(acc, EpiOut{p.y, p.ldy, p.bias, p.act, nullptr, 0}, m0 + wm * TM, min(M, m0 + p.bm),
                 n0 + wn * TN, N, 0, fr, fq);
}

template <int FM, int NBW, int NBX>
static int ws_launch(const GemmWsParams& p, hipStream_t st) {
  const int grid = ((p.M + p.bm - 1) / p.bm) * (p.N / 128) * p.S;
  switch (p.epi) {
    case EPI_SWIGLU:
      hipLaunchKernelGGL((gemm_ws_kernel<FM, NBW, NBX, EPI_SWIGLU>), dim3(grid), dim3(512), 0, st, p);
      break;
    case EPI_RESID:
      hipLaunchKernelGGL((gemm_ws_kernel<FM, NBW, NBX, EPI_RESID>), dim3(grid), dim3(512), 0, st, p);
      break;
    default:
      hipLaunchKernelGGL((gemm_ws_kernel<FM, NBW, NBX, EPI_BF16>), dim3(grid), dim3(512), 0, st, p);
  }
  return (int)hipGetLastError();
}

// depth: 0 = (weight stages 3, activation stages 2), 1 = (3, 3); the LDS of
// (3 * 16 KB + NBX * bm * 128 B) must fit 160 KB (depth 1: bm <= 256).
extern "C" int loqa_gemm_ws(const GemmWsParams* p, int depth, hipStream_t st) {
  if (!p || p->M <= 0 || p->epi < 0 || p->epi > EPI_RESID || !p->x || !p->w || !p->y)
    return (int)hipErrorInvalidValue;
  if (p->N % 128 || p->K % GEMM_BK || p->K < GEMM_BK || p->ldx % 8 || p->ldy % 4 || p->bm < 64 || p->bm % 64 ||
      p->bm > 384 || depth < 0 || depth > 1 || p->S < 1 || p->S > p->K / GEMM_BK)
    return (int)hipErrorInvalidValue;
  if (p->S > 1 && (!p->ws || !p->counters)) return (int)hipErrorInvalidValue;
  if ((p->epi == EPI_SWIGLU && (p->bias || p->act)) || (p->epi == EPI_RESID && p->act))
    return (int)hipErrorInvalidValue;
  const int fm = p->bm / 64;
  if (depth == 1) {
    switch (fm) {
      case 1: return ws_launch<1, 3, 3>(*p, st);
      case 2: return ws_launch<2, 3, 3>(*p, st);
      case 3: return ws_launch<3, 3, 3>(*p, st);
      case 4: return ws_launch<4, 3, 3>(*p, st);
      default: return (int)hipErrorInvalidValue;
    }
  }
  switch (fm) {
    case 1: return ws_launch<1, 3, 2>(*p, st);
    case 2: return ws_launch<2, 3, 2>(*p, st);
    case 3: return ws_launch<3, 3, 2>(*p, st);
    case 4: return ws_launch<4, 3, 2>(*p, st);
    case 5: return ws_launch<5, 3, 2>(*p, st);
    case 6: return ws_launch<6, 3, 2>(*p, st);
    default: return (int)hipErrorInvalidValue;
  }
}
