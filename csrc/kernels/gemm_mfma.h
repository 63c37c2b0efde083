// Device pieces shared by the LDS-tiled MFMA GEMMs (gemm_tile.hip, gemm_sk.hip,
// gemm_ws.hip): Y[M, N] = X[M, K] W[N, K]^T, both operands K-contiguous bf16.
//
// Common structure (guide §5 "Canonical CDNA GEMM", T1/T2/T4):
//   * a wave owns a (16 FN) x (16 FM) output block: FN x FM
//     v_mfma_f32_16x16x32_bf16 tiles with the W fragments as the A operand, so
//     a lane holds 4 consecutive output features of one row (8-byte bf16
//     stores): acc[i][j][r] = C[n = n_base + 16 i + 4 fq + r][m = m_base + 16 j + fr]
//     with fr = lane & 15, fq = lane >> 4;
//   * BK = 64: a stage is rows x 128 B, filled by global_load_lds (16 B per
//     lane, 1 KiB = 8 rows per wave instruction). The LDS image is lane-linear,
//     so the bank swizzle is applied on the SOURCE address: row r's 16-byte
//     chunk c lives in slot c ^ ((r >> 1) & 7). A ds_read_b128 of 16 rows at one
//     chunk then touches 16 distinct (half-row, slot) pairs: conflict-free;
//   * a ring of stages with all but one in flight: the wait before a stage's
//     barrier is a COUNTED vmcnt (the newer stages' DMAs stay in flight across
//     the raw s_barrier; __syncthreads would drain them).
#pragma once
#include "common.h"

#define GEMM_BK 64

// one epilogue numbering for the three kernels (and ops/gemm.py's _EPI)
enum { EPI_BF16 = 0, EPI_SWIGLU = 1, EPI_RESID = 2, EPI_SLABS = 3 };

// s_waitcnt vmcnt(N) with expcnt / lgkmcnt at their maxima (gfx9 encoding:
// vmcnt[3:0] in bits 3:0, vmcnt[5:4] in bits 15:14)
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// ---- staging: lane l of a wave's global_load_lds instruction `inst` (counted
// over the stage) fills row 8 inst + l / 8, slot l % 8, with the source chunk
// that the swizzle puts there
__device__ __forceinline__ int stage_row(int inst, int lane) { return 8 * inst + (lane >> 3); }
__device__ __forceinline__ int stage_chunk(int r, int lane) { return (lane & 7) ^ ((r >> 1) & 7); }

// weight row staged at row r of a workgroup tile that starts at feature n0.
// SwiGLU: each TN-row block (one wave's features) is TN / 2 gate rows + the
// matching TN / 2 up rows (gate rows [0, N/2), up rows [N/2, N) of W)
template <bool SWIGLU, int TN>
__device__ __forceinline__ int weight_row(int r, int n0, int N) {
  if constexpr (SWIGLU) {
    const int blk = r / TN, rr = r - blk * TN;
    const int f = (n0 >> 1) + blk * (TN / 2) + (rr % (TN / 2));
    return rr < TN / 2 ? f : (N >> 1) + f;
  } else {
    return n0 + r;
  }
}

__device__ __forceinline__ void glds16(const bf16_t* g, unsigned char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// one wave's IPW instructions of a stage: src[i] + koff -> dst + (wave IPW + i) KiB
template <int IPW>
__device__ __forceinline__ void stage_issue(const bf16_t* const (&src)[IPW], int koff, unsigned char* dst,
                                            int wave) {
#pragma unroll
  for (int i = 0; i < IPW; ++i) glds16(src[i] + koff, dst + (wave * IPW + i) * 1024);
}

// ---- fragments
__device__ __forceinline__ bf16x8 lds_frag(const unsigned char* base, int row, int c) {
  return *reinterpret_cast<const bf16x8*>(base + row * 128 + 16 * (c ^ ((row >> 1) & 7)));
}

template <int FN, int FM>
__device__ __forceinline__ void acc_zero(float4v (&acc)[FN][FM]) {
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
}

// One BK = 64 step of a wave: W rows wrow + 16 i + fr of the stage at wbase, X
// rows xrow + 16 j + fr of the stage at xbase.
// Half 0's fragments (activations first), then its MFMAs row by row with
// half 1's fragment reads issued between them (sched barriers pin the
// order), then half 1's MFMAs: only half 0's reads are exposed, and at most
// FN + FM + 2 LDS reads are ever outstanding (the 4-bit lgkmcnt: with more
// pending, the waitcnt pass can only wait for all of them).
template <int FN, int FM>
__device__ __forceinline__ void mfma_step(const unsigned char* wbase, int wrow, const unsigned char* xbase,
                                          int xrow, int fr, int fq, float4v (&acc)[FN][FM]) {
  static_assert(FN + FM + 2 <= 15, "outstanding LDS reads exceed lgkmcnt");
  bf16x8 af[2][FN], bfr[2][FM];
#pragma unroll
  for (int j = 0; j < FM; ++j) bfr[0][j] = lds_frag(xbase, xrow + 16 * j + fr, fq);
#pragma unroll
  for (int i = 0; i < FN; ++i) af[0][i] = lds_frag(wbase, wrow + 16 * i + fr, fq);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int i = 0; i < FN; ++i) {
#pragma unroll
    for (int j = 0; j < FM; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][i], bfr[0][j], acc[i][j], 0, 0, 0);
    af[1][i] = lds_frag(wbase, wrow + 16 * i + fr, 4 + fq);
    if (i < FM) bfr[1][i] = lds_frag(xbase, xrow + 16 * i + fr, 4 + fq);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int j = FN; j < FM; ++j) bfr[1][j] = lds_frag(xbase, xrow + 16 * j + fr, 4 + fq);
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1][i], bfr[1][j], acc[i][j], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
}

// gemm_tile's older ordering: both 32-deep halves of the stage are requested
// before the first MFMA, so the second half's LDS reads are in flight under
// the first half's MFMAs
template <int FN, int FM>
__device__ __forceinline__ void mfma_step_upfront(const unsigned char* wbase, int wrow,
                                                  const unsigned char* xbase, int xrow, int fr, int fq,
                                                  float4v (&acc)[FN][FM]) {
  bf16x8 af[2][FN], bfr[2][FM];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
    for (int i = 0; i < FN; ++i) af[sub][i] = lds_frag(wbase, wrow + 16 * i + fr, 4 * sub + fq);
#pragma unroll
    for (int j = 0; j < FM; ++j) bfr[sub][j] = lds_frag(xbase, xrow + 16 * j + fr, 4 * sub + fq);
  }
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[sub][i], bfr[sub][j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  }
}

// ---- in-launch split-K (guide §5 "In-launch split-K reduction"): chunk s of
// S publishes its partial in ws [tiles][S][NW waves][FN FM fragments][64 lanes]
// x 16 B; the tile's LAST workgroup to arrive sums the S partials into acc and
// returns true (the others return false and are done). counters[tile] is zero
// on entry and is left zero. lds_flag: any int of the workgroup's one LDS
// array (guide §5 item 4a) - every wave is past its last LDS read.
// The sum runs in fixed chunk order 0..S-1 over the published partials, this
// workgroup's own read back too: it does not depend on who arrived last, and
// needs no second accumulator array (the 256 x 256 tile has no registers for
// one). No fence, wait or barrier below may move.
template <int FN, int FM>
constexpr int splitk_group() {
  // loads go in groups of up to 16 fragments: the largest divisor of FN whose
  // FM-wide rows fit
  int g = FN;
  while (g > 1 && (FN % g || g * FM > 16)) --g;
  return g;
}

template <int FN, int FM, int NW>
__device__ __forceinline__ bool splitk_reduce(float* ws, int* counters, int tile, int s, int S, int* lds_flag,
                                              int wave, int lane, float4v (&acc)[FN][FM]) {
  constexpr int PER_WAVE = FN * FM * 256;      // floats per wave partial (16 B per lane per fragment)
  float* mine = ws + (((size_t)tile * S + s) * NW + wave) * PER_WAVE;
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j)
      *reinterpret_cast<float4v*>(mine + ((i * FM + j) * 64 + lane) * 4) = acc[i][j];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = __hip_atomic_fetch_add(counters + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t == S - 1;
    if (last) __hip_atomic_store(counters + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *lds_flag = last;
  }
  __syncthreads();
  if (!*lds_flag) return false;
  if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  constexpr int GI = splitk_group<FN, FM>();
  for (int c = 0; c < S; ++c) {
    const float* theirs = ws + (((size_t)tile * S + c) * NW + wave) * PER_WAVE;
#pragma unroll
    for (int i0 = 0; i0 < FN; i0 += GI) {
      float4v v[GI][FM];
#pragma unroll
      for (int i = 0; i < GI; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j)
          v[i][j] = *reinterpret_cast<const float4v*>(theirs + (((i0 + i) * FM + j) * 64 + lane) * 4);
#pragma unroll
      for (int i = 0; i < GI; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i0 + i][j] = c == 0 ? v[i][j] : acc[i0 + i][j] + v[i][j];
    }
  }
  return true;
}

// ---- epilogues, applied once per output element of a wave's block: rows
// m_base + 16 j + fr below m_end, features n_base + 16 i + 4 fq + r.
//   EPI_BF16   y = bf16(acc (+ bias)), optionally GELU (erf) and then + pos
//              (bf16 [pos_rows, N], row m % pos_rows)
//   EPI_SWIGLU y[:, f] = silu(gate_f) * up_f: fragments [0, FN/2) are the gate,
//              [FN/2, FN) the matching up features (weight_row's permutation)
//   EPI_RESID  y = bf16(y + (acc + bias)) in place: one rounding
//   EPI_SLABS  f32 acc to y as [rows, N] f32, row m + slab_row (split-K slabs)
struct EpiOut {
  void* y; long long ldy;
  const float* bias; int act;        // act: 0 none, 1 GELU
  const void* pos; int pos_rows;
};

template <int EPI, int FN, int FM>
__device__ __forceinline__ void epi_store(const float4v (&acc)[FN][FM], const EpiOut& o, int m_base, int m_end,
                                          int n_base, int N, size_t slab_row, int fr, int fq) {
  static_assert(EPI != EPI_SWIGLU || FN % 2 == 0, "SwiGLU pairs gate / up fragments");
  if constexpr (EPI == EPI_SWIGLU) {
    bf16_t* Y = reinterpret_cast<bf16_t*>(o.y);
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int m = m_base + 16 * j + fr;
      if (m >= m_end) continue;
#pragma unroll
      for (int i = 0; i < FN / 2; ++i) {
        const int f = (n_base >> 1) + 16 * i + 4 * fq;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = bf2f(f2bf(acc[i][j][r])), u = bf2f(f2bf(acc[i + FN / 2][j][r]));
          v[r] = g / (1.f + __expf(-g)) * u;
        }
        *reinterpret_cast<uint2*>(Y + (size_t)m * o.ldy + f) =
            make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
      }
    }
  } else if constexpr (EPI == EPI_SLABS) {
    float* part = reinterpret_cast<float*>(o.y);
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int m = m_base + 16 * j + fr;
      if (m >= m_end) continue;
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        const int n = n_base + 16 * i + 4 * fq;
        *reinterpret_cast<float4v*>(part + (slab_row + m) * N + n) = acc[i][j];
      }
    }
  } else {
    bf16_t* Y = reinterpret_cast<bf16_t*>(o.y);
    float4 bv[FN];
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      const int n = n_base + 16 * i + 4 * fq;
      bv[i] = o.bias ? *reinterpret_cast<const float4*>(o.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int m = m_base + 16 * j + fr;
      if (m >= m_end) continue;
      const bf16_t* pr = o.pos ? reinterpret_cast<const bf16_t*>(o.pos) + (size_t)(m % o.pos_rows) * N : nullptr;
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        const int n = n_base + 16 * i + 4 * fq;
        uint2* yp = reinterpret_cast<uint2*>(Y + (size_t)m * o.ldy + n);
        float v[4] = {acc[i][j][0] + bv[i].x, acc[i][j][1] + bv[i].y, acc[i][j][2] + bv[i].z,
                      acc[i][j][3] + bv[i].w};
        if constexpr (EPI == EPI_RESID) {
          const uint2 rv = *yp;
          v[0] += bf2f(rv.x & 0xffff);
          v[1] += bf2f(rv.x >> 16);
          v[2] += bf2f(rv.y & 0xffff);
          v[3] += bf2f(rv.y >> 16);
        } else if (o.act == 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = bf2f(f2bf(v[r]));
            v[r] = 0.5f * t * (1.f + erff(t * 0.70710678118654752f));
          }
        }
        if (pr) {
          const uint2 pv = *reinterpret_cast<const uint2*>(pr + n);
          v[0] = bf2f(f2bf(v[0])) + bf2f(pv.x & 0xffff);
          v[1] = bf2f(f2bf(v[1])) + bf2f(pv.x >> 16);
          v[2] = bf2f(f2bf(v[2])) + bf2f(pv.y & 0xffff);
          v[3] = bf2f(f2bf(v[3])) + bf2f(pv.y >> 16);
        }
        *yp = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
      }
    }
  }
}
