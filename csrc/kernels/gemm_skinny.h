// Decode-shaped GEMM: out^T[N, M] = W[N, K] * x^T[K, M] for M <= 128 tokens
// (SURVEY §2.4 "GEMM/GEMV for skinny M"; guide §5 table row "GEMV / M <= 16 decode
// weights": operand streamed once, straight to VGPRs, deep prefetch).
//
// Weight-streaming bound: every weight byte is read exactly once per decode
// step, so the kernel is shaped for HBM bandwidth, not MFMA rate:
//   * weights are PRE-SHUFFLED once at load time into MFMA fragment order
//     Wp[N/16][K/32][64 lanes][8]: lane l of v_mfma_f32_16x16x32_bf16 holds row
//     (l&15), k-offset 8*(l>>4). One wave load instruction is then 1 KiB
//     contiguous and a wave walks one contiguous 16-row x K stream - full-burst
//     DRAM access instead of 16 scattered 64-byte row segments;
//   * register ping-pong prefetch: the next UNROLL k-steps (UNROLL*RT KiB per
//     wave) are in flight while the current ones feed the MFMAs;
//   * workgroup = 4 waves splitting its (16*RT rows x K/S) item along K, LDS
//     reduce at the end; split-K S keeps >= 2 workgroups per CU; partial sums
//     go to f32 slabs part[S][Mpad][N] that the NEXT kernel sums in its prologue
//     (slab_ops.hip) - deterministic, no atomics, no extra launch.
//
// This header holds the kernels and their launch templates; gemm_skinny.hip
// instantiates the bf16 weight stream and owns the entry points,
// gemm_skinny_fp8.hip instantiates the fp8 (e4m3) weight stream and
// gemm_skinny_mxfp4.hip the MXFP4 (e2m1 + e8m0 block scale) one - three
// translation units, so the sets compile side by side. The format is the FMT
// parameter of the shared pieces: the weight fragment (WFrag), its load
// (load_w), the MFMA step that dequantises it (mma_step) and the launcher.
#pragma once
#include <type_traits>

#include "common.h"

// launch priority of the calling host thread (attn_decode.hip)
extern thread_local int g_loqa_launch_prio;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4v mfma16(const bf16x8& a, const bf16x8& b, const float4v& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// streamed-once weights: non-temporal 16-byte load (8 bf16, or 16 raw fp8 bytes)
__device__ __forceinline__ bf16x8 ldw(const void* p) {
  u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return *reinterpret_cast<bf16x8*>(&v);
}

// fp8 weight stream (OCP e4m3fn bytes, gemm_skinny_fp8.hip): Wp8[N/16][K/64][64
// lanes][16 B]; lane l holds row (l&15), bytes 0-7 = the 8 k values at offset
// 8*(l>>4) of k-step 2j, bytes 8-15 the same of k-step 2j+1. One 16-byte lane
// load is the A fragments of TWO k-steps and stays raw in the prefetch
// registers (half the in-flight weight VGPRs); it is converted to bf16 - exactly,
// every e4m3 value is a bf16 value - when its group is consumed.
typedef unsigned char fp8_t;

// The weight stream's format, the FMT parameter of everything below
enum { WF_BF16 = 0, WF_FP8 = 1, WF_MXFP4 = 2 };

// MXFP4 weight stream (OCP e2m1 elements, one e8m0 scale per 32 k values of a
// row, gemm_skinny_mxfp4.hip): Wp4[N/16][K/128][64 lanes][16 B]; lane l holds
// row (l&15), bytes 4j..4j+3 = the 8 k values at offset 8*(l>>4) of k-step
// 4g+j, ascending, two per byte, the even k in the low nibble. One 16-byte
// lane load is the A fragments of FOUR k-steps and stays raw in the prefetch
// registers (a quarter of the in-flight weight VGPRs); an 8-byte load is two
// k-steps (the layouts whose prefetch group is 2 k-steps).
// Scales: Ws[N/16][K/128][16 rows][4 B], byte j = the e8m0 scale of k-step
// 4g+j: a lane reads one dword per 16-byte weight load, the four lanes of a
// row the same one. A block of 32 is one k-step, so a k-step's A fragment is
// dequantised in registers as e2m1 * 2^(byte - 127), exactly (every such
// product the quantiser emits is a normal bf16), and the accumulator needs no
// scale afterwards.
struct Mx4Ptr {
  const unsigned char* w;   // this lane's 16 bytes of the tile's first 4 k-steps
  const unsigned char* s;   // this lane's row's 4 scale bytes of them
};
template <typename W> constexpr int kFp8 = sizeof(W) == 1;

// 8 e4m3 bytes -> the 8 bf16 of one MFMA A fragment: gfx950's packed
// fp8 -> bf16 convert with scale 1.0, two values per instruction (checked on
// the hardware for all 256 byte values against v_cvt_pk_f32_fp8: exact, NaN
// 0x7f / 0xff stays NaN)
__device__ __forceinline__ bf16x8 cvt_fp8x8(unsigned lo, unsigned hi) {
  typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
  auto cv = [](unsigned v, bool upper) {
    const bf16x2_ r = upper ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, true)
                            : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, false);
    return __builtin_bit_cast(unsigned, r);
  };
  u32x4 r;
  r.x = cv(lo, false);
  r.y = cv(lo, true);
  r.z = cv(hi, false);
  r.w = cv(hi, true);
  return *reinterpret_cast<bf16x8*>(&r);
}

// A fragment of k-step u of a prefetch slot: bf16 - the register itself; fp8 -
// half of raw load u / 2
template <int FMT>
__device__ __forceinline__ bf16x8 wfrag(const bf16x8& raw, int u) {
  if constexpr (FMT == WF_FP8) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(&raw);
    return (u & 1) ? cvt_fp8x8(v.z, v.w) : cvt_fp8x8(v.x, v.y);
  } else {
    return raw;
  }
}

__device__ __forceinline__ bf16x8 ldx(const bf16_t* p) {
  uint4 v = *reinterpret_cast<const uint4*>(p);
  return *reinterpret_cast<bf16x8*>(&v);
}

// workgroup barrier for LDS hand-offs only: waits for this wave's LDS ops, not
// for its outstanding global loads (__syncthreads' release fence would drain
// the weight prefetch)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// 8 e2m1 nibbles (one dword: 8 ascending k values, the even k in the low
// nibble) times 2^(e8m0 - 127) -> the 8 bf16 of one MFMA A fragment: gfx950's
// packed fp4 -> bf16 convert, two values per instruction, byte by byte. The
// scale operand is the f32 whose exponent field is the e8m0 byte. Checked on
// the hardware through the real kernel (tests/test_mxfp4_weights.py, the
// convert probe): byte_sel b converts byte b of the source, its low nibble to
// the low bf16 and its high nibble to the high one; the result is
// e2m1 * 2^(byte - 127) for every scale byte 2..252 (the quantiser's range;
// 0 would be the f32 0.0, not 2^-127, and 255 a NaN - neither is emitted);
// all 16 codes at all 32 nibble positions of a lane load equal the table
// dequantisation bit for bit.
__device__ __forceinline__ bf16x8 cvt_mxfp4x8(unsigned q, unsigned e8m0) {
  typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
  const float sc = __builtin_bit_cast(float, e8m0 << 23);
  u32x4 r;
  r.x = __builtin_bit_cast(unsigned, (bf16x2_)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0));
  r.y = __builtin_bit_cast(unsigned, (bf16x2_)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1));
  r.z = __builtin_bit_cast(unsigned, (bf16x2_)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2));
  r.w = __builtin_bit_cast(unsigned, (bf16x2_)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3));
  return *reinterpret_cast<bf16x8*>(&r);
}

// One prefetch group of weights: U k-steps of RT row tiles.
// NW: 16-byte weight loads per row tile and group (fp8: one per two k-steps)
template <int RT, int U, int FMT = 0>
struct WFrag {
  static constexpr int NW = FMT ? (U + 1) / 2 : U;
  bf16x8 a[NW][RT];
};

// MXFP4: one raw dword (8 nibbles) per k-step and row tile, and the scale
// bytes of the group's k-steps in one register (U = 4: a dword, U = 2: the
// two bytes of its k-steps)
template <int RT, int U>
struct WFrag<RT, U, WF_MXFP4> {
  unsigned q[U][RT];
  unsigned s[RT];
};

// ... and the group's activation fragments (the register form; XL reads them from LDS)
template <int RT, int MT, int U, int FMT = 0>
struct Frag : WFrag<RT, U, FMT> {
  bf16x8 b[U][MT];
};

// wp: this lane's 16 bytes of the tile's first k-step; in elements of W a
// k-step is 512 apart in both formats (fp8: ks even)
template <int RT, int U, int FMT, typename W>
__device__ __forceinline__ void load_w(WFrag<RT, U, FMT>& f, const W* wp, size_t tile_stride, int ks) {
  static_assert(FMT == kFp8<W>, "fragment / weight format mismatch");
#pragma unroll
  for (int u = 0; u < WFrag<RT, U, FMT>::NW; ++u)
#pragma unroll
    for (int i = 0; i < RT; ++i)
      f.a[u][i] = ldw(wp + (size_t)i * tile_stride + (size_t)(ks + u * (FMT ? 2 : 1)) * 512);
}

// MXFP4: tile_stride in bytes of the nibble stream (16 rows x K / 2); the
// scale stream's is a sixteenth of it. A group of 4 k-steps (ks % 4 == 0) is
// one 16-byte load and one scale dword; a group of 2 (ks even) the 8 bytes and
// the 2 scale bytes of its k-steps inside them, so k-steps stay ascending.
template <int RT, int U, int FMT>
__device__ __forceinline__ void load_w(WFrag<RT, U, FMT>& f, const Mx4Ptr wp, size_t tile_stride, int ks) {
  static_assert(FMT == WF_MXFP4 && (U == 4 || U == 2), "MXFP4: prefetch groups of 4 or 2 k-steps");
  const size_t blk = (size_t)(ks >> 2), sub = (size_t)(ks & 3);
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const unsigned char* pw = wp.w + (size_t)i * tile_stride + blk * 1024 + sub * 4;
    const unsigned char* ps = wp.s + (size_t)i * (tile_stride >> 4) + blk * 64 + sub;
    if constexpr (U == 4) {
      const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pw));
      f.q[0][i] = v.x, f.q[1][i] = v.y, f.q[2][i] = v.z, f.q[3][i] = v.w;
      f.s[i] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(ps));
    } else {
      typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(pw));
      f.q[0][i] = v.x, f.q[1][i] = v.y;
      f.s[i] = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(ps));
    }
  }
}

template <int RT, int MT, int U, int FMT>
__device__ __forceinline__ void load_frag_x(Frag<RT, MT, U, FMT>& f, const bf16_t* xp, long long ldx_, int ks) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < MT; ++j) f.b[u][j] = ldx(xp + (size_t)j * 16 * ldx_ + (size_t)(ks + u) * 32);
}

template <int RT, int MT, int U, int FMT, typename WP>
__device__ __forceinline__ void load_frag(Frag<RT, MT, U, FMT>& f, const WP wp, size_t tile_stride,
                                          const bf16_t* xp, long long ldx_, int ks) {
  load_w<RT, U, FMT>(f, wp, tile_stride, ks);
  load_frag_x(f, xp, ldx_, ks);
}

// k-step u of a group against its MT activation fragments. fp8 / MXFP4: this
// k-step's A fragments are dequantised once, here (k-steps stay in ascending
// order). bf16 reads the prefetch registers in place: going through the same
// local copy is not free - it took skinny_fused_kernel<1, 2, 4, 4, act> from
// occupancy 4 to 3 (docs/PERF.md, "Decode GEMM header")
template <int RT, int MT, int U, int FMT>
__device__ __forceinline__ void mma_step(const WFrag<RT, U, FMT>& f, int u, const bf16x8 (&b)[MT],
                                         float4v (&acc)[RT][MT]) {
  bf16x8 deq[FMT ? RT : 1];
  if constexpr (FMT == WF_FP8) {
#pragma unroll
    for (int i = 0; i < RT; ++i) deq[i] = wfrag<1>(f.a[u / 2][i], u);
  } else if constexpr (FMT == WF_MXFP4) {
#pragma unroll
    for (int i = 0; i < RT; ++i) deq[i] = cvt_mxfp4x8(f.q[u][i], (f.s[i] >> (8 * u)) & 0xffu);
  }
  auto a = [&](int i) -> const bf16x8& {
    if constexpr (FMT) return deq[i];
    else return f.a[u][i];
  };
#pragma unroll
  for (int j = 0; j < MT; ++j)
#pragma unroll
    for (int i = 0; i < RT; ++i) acc[i][j] = mfma16(a(i), b[j], acc[i][j]);
}

template <int RT, int MT, int U, int FMT>
__device__ __forceinline__ void mma_frag(const Frag<RT, MT, U, FMT>& f, float4v (&acc)[RT][MT]) {
#pragma unroll
  for (int u = 0; u < U; ++u) mma_step<RT, MT, U, FMT>(f, u, f.b[u], acc);
}

// Ping-pong stream over ng groups of U k-steps from k-step ks0; f0 already
// holds group 0.
// The steady-state loop issues the next group UNCONDITIONALLY before consuming
// the current one: a conditional refill inside the loop body makes the
// consumer block a join point of the refill / no-refill paths, and hipcc's
// waitcnt pass then takes the stricter count of the two (vmcnt(0)) - every
// iteration drained the prefetch and only ONE group was ever in flight.
// (Groups are visited in ascending order. A k-start rotation per workgroup
// measured 5-10 % SLOWER on every shape: the in-step x reuse across
// neighbouring workgroups in L2 matters more.)
template <int RT, int MT, int U, int FMT, typename WP>
__device__ __forceinline__ void stream_k(Frag<RT, MT, U, FMT>& f0, Frag<RT, MT, U, FMT>& f1,
                                         float4v (&acc)[RT][MT], const WP wp,
                                         size_t tile_stride, const bf16_t* xp, long long ldx_,
                                         int ks0, int ng) {
  auto ks = [&](int g) { return ks0 + g * U; };
  // sched_barrier(0) pins each phase: without it the machine scheduler sinks
  // the refill loads between the MFMAs to save registers, collapsing the
  // prefetch distance to 3-5 loads
  int g = 0;
  for (; g + 2 < ng; g += 2) {
    load_frag(f1, wp, tile_stride, xp, ldx_, ks(g + 1));
    __builtin_amdgcn_sched_barrier(0);
    mma_frag(f0, acc);
    __builtin_amdgcn_sched_barrier(0);
    load_frag(f0, wp, tile_stride, xp, ldx_, ks(g + 2));
    __builtin_amdgcn_sched_barrier(0);
    mma_frag(f1, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (g + 1 < ng) {
    load_frag(f1, wp, tile_stride, xp, ldx_, ks(g + 1));
    __builtin_amdgcn_sched_barrier(0);
    mma_frag(f0, acc);
    mma_frag(f1, acc);
  } else {
    mma_frag(f0, acc);
  }
}

// wscale (fp8 only): f32 [N] per-row dequantisation scale, applied as wave 0
// writes its slab
template <int RT, int MT, int U, typename W>
__device__ __forceinline__ void skinny_gemm_body(float4v (&red)[3][RT * MT][64],
                                                 const bf16_t* __restrict__ x, long long ldx_,
                                                 const W* __restrict__ Wp, const float* __restrict__ wscale,
                                                 float* __restrict__ part, int N, int K, int S, int Mpad) {
  constexpr int FMT = kFp8<W>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int KS = K >> 5;                      // k-steps of 32
  const int kw = KS / (S * 4);                // k-steps per wave
  const int ks0 = (s * 4 + wave) * kw;
  const size_t tile_stride = (size_t)KS * 512;  // elements per 16-row tile
  const bf16_t* xp = x + (size_t)(lane & 15) * ldx_ + 8 * (lane >> 4);
  const int ngroups = N / (16 * RT);
  // grid-stride over tile groups: a capped grid (one workgroup per CU) leaves
  // CU slots free for the concurrent decoder stream (see tune_fused_splits)
  for (int tg = blockIdx.x; tg < ngroups; tg += gridDim.x) {
    const int tile0 = tg * RT;                  // first 16-row tile
    const W* wp = Wp + (size_t)tile0 * tile_stride + (size_t)lane * (FMT ? 16 : 8);
    float4v acc[RT][MT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] = (float4v){0.f, 0.f, 0.f, 0.f};

    // ping-pong register prefetch over groups of U k-steps
    Frag<RT, MT, U, FMT> f0, f1;
    load_frag(f0, wp, tile_stride, xp, ldx_, ks0);
    stream_k(f0, f1, acc, wp, tile_stride, xp, ldx_, ks0, kw / U);

    if (wave > 0) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) red[wave - 1][i * MT + j][lane] = acc[i][j];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) {
          float4v v = acc[i][j] + red[0][i * MT + j][lane] + red[1][i * MT + j][lane] +
                      red[2][i * MT + j][lane];
          // C layout (16x16): col = lane&15 (token m), rows n = 4*(lane>>4) + reg
          const int m = j * 16 + (lane & 15);
          const int n = (tile0 + i) * 16 + 4 * (lane >> 4);
          if constexpr (FMT) v *= *reinterpret_cast<const float4v*>(wscale + n);
          *reinterpret_cast<float4v*>(part + ((size_t)s * Mpad + m) * N + n) = v;
        }
    }
    __syncthreads();                            // red is reused by the next group
  }
}

template <int RT, int MT, int U>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(const bf16_t* __restrict__ x, long long ldx_,
                                                          const bf16_t* __restrict__ Wp,
                                                          float* __restrict__ part, int N, int K,
                                                          int S, int Mpad) {
  __shared__ float4v red[3][RT * MT][64];
  skinny_gemm_body<RT, MT, U>(red, x, ldx_, Wp, nullptr, part, N, K, S, Mpad);
}

// the fp8 weight stream: its own kernel name, so the bf16 instances keep theirs
template <int RT, int MT, int U>
__global__ __launch_bounds__(256) void skinny_gemm_fp8_kernel(const bf16_t* __restrict__ x, long long ldx_,
                                                              const fp8_t* __restrict__ Wp,
                                                              const float* __restrict__ wscale,
                                                              float* __restrict__ part, int N, int K,
                                                              int S, int Mpad) {
  __shared__ float4v red[3][RT * MT][64];
  skinny_gemm_body<RT, MT, U>(red, x, ldx_, Wp, wscale, part, N, K, S, Mpad);
}

struct SkinnyArgs {
  const void* x; long long ldx; const void* Wp; const float* wscale; float* part;
  int N, K, S, Mpad, max_wgs;
};

template <int RT, int MT, int U, typename W>
static void launch_skinny_kernel(dim3 grid, const SkinnyArgs& a, hipStream_t st) {
  if constexpr (kFp8<W>)
    hipLaunchKernelGGL((skinny_gemm_fp8_kernel<RT, MT, U>), grid, dim3(256), 0, st, (const bf16_t*)a.x,
                       a.ldx, (const fp8_t*)a.Wp, a.wscale, a.part, a.N, a.K, a.S, a.Mpad);
  else
    hipLaunchKernelGGL((skinny_gemm_kernel<RT, MT, U>), grid, dim3(256), 0, st, (const bf16_t*)a.x,
                       a.ldx, (const bf16_t*)a.Wp, a.part, a.N, a.K, a.S, a.Mpad);
}

// Prefetch groups of 4 k-steps (MT <= 2), of 2 or 1 when the wave's k range
// does not divide. fp8 weights: the same grid and prefetch groups; a wave's k
// range must be even
template <int RT, int MT, typename W>
static int launch_skinny(const SkinnyArgs& a, hipStream_t st) {
  int gx = a.N / (16 * RT);
  if (a.max_wgs > 0 && gx * a.S > a.max_wgs) gx = a.max_wgs / a.S > 0 ? a.max_wgs / a.S : 1;
  dim3 grid(gx, a.S);
  const int kw = a.K / 32 / (a.S * 4);
  if (MT <= 2 && kw % 4 == 0)
    launch_skinny_kernel<RT, MT, (MT <= 2 ? 4 : 2), W>(grid, a, st);
  else if (kw % 2 == 0)
    launch_skinny_kernel<RT, MT, 2, W>(grid, a, st);
  else if constexpr (!kFp8<W>)
    launch_skinny_kernel<RT, MT, 1, W>(grid, a, st);
  else
    return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// Mpad -> (RT, MT) of the plain skinny GEMM, both weight formats
template <typename W>
static int dispatch_skinny(const SkinnyArgs& a, hipStream_t st) {
  if (a.N % (a.Mpad >= 64 ? 64 : 32)) return (int)hipErrorInvalidValue;
  switch (a.Mpad) {
    case 16: return launch_skinny<2, 1, W>(a, st);
    case 32: return launch_skinny<2, 2, W>(a, st);
    case 64: return launch_skinny<4, 4, W>(a, st);
    case 128: return launch_skinny<4, 8, W>(a, st);
    default: return (int)hipErrorInvalidValue;
  }
}

// ============================================================================
// x through LDS (XL): the mid-M form (Mpad 64 / 128: decode steps that carry a
// chunked-prefill slice or long jump-forward runs). At M >= 64 the register
// form above reads Mpad/16 KiB of activation fragments per 1 KiB weight
// fragment, from L2, once per WAVE: at Mpad 64 the activation stream was 4x
// the weight stream and the step took 2.2x the Mpad-16 time. In the XL form
// the 4 waves of a workgroup own 4 row tiles over the SAME k range; each
// U-k-step chunk of x is loaded once per workgroup (256 threads, 16-byte
// pieces, prefetched into registers one chunk ahead) and written to LDS, and
// every wave reads its MFMA B fragments from there (16 B per lane). Weights keep
// the register ping-pong stream (one group of U k-steps in flight).
// LDS image: one 64-B row per (k-step, x row), its four 16-B pieces XOR-swizzled
// by (row >> 1) & 3. ds_read_b128 banks are (a/4) % 64 over four 16-lane groups
// ({0-3,12-15,20-27}, ...) and ds_write_b128 banks (a/4) % 32 over 8-lane groups
// (MI355X_MICROARCH.md, LDS): with the swizzle both the fragment reads (lane l:
// row l & 15, piece l >> 4) and the chunk stores (4 lanes per row) are
// conflict-free. (The earlier 80-B padded rows were conflict-free only under
// 32-bank rules: SQ_LDS_BANK_CONFLICT measured ~1 extra cycle per cycle.)
constexpr int XROW = 32;   // LDS row: 32 k values (64 B), pieces swizzled
__device__ __forceinline__ int xs_piece(int row, int q) { return (q ^ ((row >> 1) & 3)) * 8; }

// one chunk of x: U k-steps x MP rows = MP * U * 4 pieces of 16 B
template <int MP, int U>
struct XRegs {
  static constexpr int NP = (MP * U * 4) / 256;
  uint4 v[NP];
};

// Piece -> thread map: the 4 16-B pieces of a row's k-step fastest, then
// rows, then the chunk's U k-steps. (A whole-line map - a row's U k-steps
// across 4U consecutive lanes - measured 1-2% slower end to end.)
template <int MP, int U>
__device__ __forceinline__ void xc_piece(int idx, int& row, int& u, int& q) {
  q = idx & 3;
  const int rest = idx >> 2;
  row = rest % MP;
  u = rest / MP;
}

template <int MP, int U>
__device__ __forceinline__ void load_xc(XRegs<MP, U>& r, const bf16_t* x, long long ldx_, int ks) {
#pragma unroll
  for (int p = 0; p < XRegs<MP, U>::NP; ++p) {
    int row, u, q;
    xc_piece<MP, U>(p * 256 + (int)threadIdx.x, row, u, q);
    r.v[p] = *reinterpret_cast<const uint4*>(x + (size_t)row * ldx_ + (size_t)(ks + u) * 32 + q * 8);
  }
}

template <int MP, int U>
__device__ __forceinline__ void store_xc(const XRegs<MP, U>& r, bf16_t* xs) {
#pragma unroll
  for (int p = 0; p < XRegs<MP, U>::NP; ++p) {
    int row, u, q;
    xc_piece<MP, U>(p * 256 + (int)threadIdx.x, row, u, q);
    *reinterpret_cast<uint4*>(xs + (size_t)(u * MP + row) * XROW + xs_piece(row, q)) = r.v[p];
  }
}

template <int RT, int MT, int U, int FMT>
__device__ __forceinline__ void mma_xl(const WFrag<RT, U, FMT>& f, float4v (&acc)[RT][MT], const bf16_t* xs,
                                       int lane) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    bf16x8 b[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j)
      b[j] = *reinterpret_cast<const bf16x8*>(xs + (size_t)(u * MT * 16 + j * 16 + (lane & 15)) * XROW +
                                              xs_piece(lane & 15, lane >> 4));
    mma_step(f, u, b, acc);
  }
}

// The XL stream. On entry chunk 0 of x (xr) and weight group 0 (f0) are in
// flight, x issued first, so storing xr waits for x only. Each chunk: issue the
// next chunk's x, then the next weight group (both unconditional, clamped to
// the last chunk: no join point drains the prefetch, see stream_k), consume the
// current chunk from LDS, then (barrier) overwrite LDS with the next chunk.
template <int RT, int MT, int U, int FMT, typename WP>
__device__ __forceinline__ void stream_k_xl(WFrag<RT, U, FMT>& f0, WFrag<RT, U, FMT>& f1, XRegs<MT * 16, U>& xr,
                                            float4v (&acc)[RT][MT], const WP wp,
                                            size_t tile_stride, const bf16_t* x, long long ldx_,
                                            bf16_t* xs, int ks0, int ng, int lane) {
  auto ks = [&](int g) { return ks0 + (g < ng ? g : ng - 1) * U; };
  store_xc<MT * 16, U>(xr, xs);
  lds_barrier();
  int g = 0;
  for (; g + 2 < ng; g += 2) {
    load_xc<MT * 16, U>(xr, x, ldx_, ks(g + 1));
    load_w(f1, wp, tile_stride, ks(g + 1));
    __builtin_amdgcn_sched_barrier(0);
    mma_xl(f0, acc, xs, lane);
    __builtin_amdgcn_sched_barrier(0);
    lds_barrier();
    store_xc<MT * 16, U>(xr, xs);
    lds_barrier();
    load_xc<MT * 16, U>(xr, x, ldx_, ks(g + 2));
    load_w(f0, wp, tile_stride, ks(g + 2));
    __builtin_amdgcn_sched_barrier(0);
    mma_xl(f1, acc, xs, lane);
    __builtin_amdgcn_sched_barrier(0);
    lds_barrier();
    store_xc<MT * 16, U>(xr, xs);
    lds_barrier();
  }
  if (g + 1 < ng) {
    load_xc<MT * 16, U>(xr, x, ldx_, ks(g + 1));
    load_w(f1, wp, tile_stride, ks(g + 1));
    __builtin_amdgcn_sched_barrier(0);
    mma_xl(f0, acc, xs, lane);
    __builtin_amdgcn_sched_barrier(0);
    lds_barrier();
    store_xc<MT * 16, U>(xr, xs);
    lds_barrier();
    mma_xl(f1, acc, xs, lane);
  } else {
    mma_xl(f0, acc, xs, lane);
  }
}

// ============================================================================
// Fused decode GEMMs: the skinny GEMM above with its follow-on op moved into
// the epilogue and the preceding RMSNorm moved into the operand load, so a
// Llama decode layer is 5 launches instead of 10:
//   qkv     : prologue rmsnorm(attn_norm) | epilogue RoPE + paged KV append + q
// (RMSNorm: the norm weight is folded into the weight rows at load time and the
//  per-row 1/rms scale, a property of the row, is applied to the accumulator,
//  so the operand stream stays the plain prefetch pipeline)
//   o       : epilogue residual add + per-tile row sum of squares
//   gate|up : prologue rmsnorm(mlp_norm)  | epilogue silu(gate) * up -> bf16
//   down    : epilogue residual add + per-tile row sum of squares
// Split-K (S > 1) partials are reduced inside the launch by the last arriving
// workgroup of each 32-row tile (guide §5 "in-launch split-K reduction":
// write-through sc1 slab stores -> vmcnt(0) -> barrier -> relaxed agent ticket;
// the reducer takes an agent acquire and sums the S slabs in fixed order, so
// results are bitwise identical to the launch-boundary reduce). The RMSNorm
// scale of a row is rebuilt in every consumer workgroup from the producer's
// per-tile partial sums of squares in a fixed order (deterministic, no atomics).
// Weight rows are permuted at load time so one 32-row tile holds (gate, up)
// feature pairs, or the (c, c + D/2) RoPE pairs of one head.
//
// The epilogue modes (FusedParams::mode; Python passes the numbers). FEPI_, not
// EPI_: gemm_mfma.h numbers the prompt-pass epilogues differently.
enum { FEPI_SILU = 1, FEPI_RESID = 2, FEPI_ROPE = 3, FEPI_ACT = 4 };
enum { NORM_NONE = 0, NORM_RMS = 1, NORM_LN = 2 };

// Host-side parameter block (mirrored by a ctypes.Structure in ops/_lib.py).
struct FusedParams {
  const void* x; long long ldx; const void* Wp; float* part; int* counters;
  int Mpad, N, K, S, mode, norm;
  const float* rowsq_in; const float* rowsum_in; int rowstat_tiles; float eps;
  const float* colsum; const float* bias;
  void* out; long long ldo; int act;
  void* residual; float* rowsq_out; float* rowsum_out;
  const int* positions; const void* cs; void* q_out; void* kc; void* vc; const int* slots;
  int H, Hkv, D, blk;
  int rt;                 // output tile rows / 16 (1, 2; 4 at Mpad 64)
  int wr;                 // waves along the rows (1, or 4 with S == 1; any S with xl)
  int xl;                 // x through LDS (wr == 4; Mpad 32 / 64 / 128)
  int wdtype;             // weight stream: 0 bf16 (Wp), 1 fp8 e4m3fn (Wp = Wp8 bytes + wscale),
                          // 2 MXFP4 (Wp = Wp4 nibble bytes, wscale = the e8m0 scale bytes Ws)
  const float* wscale;    // fp8: f32 [N] per-row dequantisation scale (rows in Wp order)
};


struct FusedArgs {
  const bf16_t* x; long long ldx; const bf16_t* Wp; float* part; int N, K, S, Mpad;
  int* counters;
  const float* rowsq_in; const float* rowsum_in; int rowstat_tiles; float eps;  // norm row stats
  const float* colsum; const float* bias;   // LayerNorm mean correction, output bias (per row of W)
  bf16_t* out; long long ldo; int act;                                        // FEPI_SILU / FEPI_ACT
  bf16_t* residual; float* rowsq_out; float* rowsum_out;                      // FEPI_RESID
  const int* positions; const float2* cs; bf16_t* q_out; bf16_t* kc; bf16_t* vc;
  const int* slots; int H, Hkv, D, blk;                                       // FEPI_ROPE
  int prio;                                     // s_setprio 3 for the launch (attn_decode.hip)
  const float* wscale;                          // fp8 weight stream: per-row scale; MXFP4: the e8m0 bytes
};

// WR: waves along the rows. WR = 1: the 4 waves split the tile's K range
// (LDS reduce); WR = 4: every wave owns its own (16 * RT)-row tile over the
// whole K range of the split - the 4 waves then read the SAME activation
// fragments at about the same time, so x is fetched from L2 once per
// workgroup (L1 hits for the other 3) instead of once per wave, and no
// cross-wave reduction is needed (measured on cold weights, M = 16: the
// gate|up stream went from 48 us to 39 us). WR > 1 requires S == 1.
template <int RT, int MT, int WR>
struct FusedSmem {
  static constexpr int WK = 4 / WR;
  static constexpr int NRED = WK > 1 ? WR * (WK - 1) * RT * MT * 64 : 1;
  static constexpr int NSM = NRED * 4 > 1024 ? NRED * 4 : 1024;   // floats: reduce / prologue / ticket
};

// sred (the first 1024 floats of the workgroup's LDS) in the norm prologue:
// [0, 512) per-thread partial sums of squares, [512, 768) partial row sums,
// then the finished row scales and the row means, up to Mpad 128 rows each
constexpr int SRED_SUM = 512, SRED_SCALE = 768, SRED_MEAN = 896;

// One (16 * RT * WR)-row output tile of the fused GEMM (a workgroup's whole
// GEMM work; `return` = this workgroup's GEMM part is done).
// One long function on purpose: its sections (operand requests, norm prologue,
// k loop, cross-wave and split-K reduce, the scale / norm / bias step and the
// four epilogues) were each tried as a __forceinline__ function over the same
// arrays, and every one of them moved the registers of some instances - one
// to a lower occupancy (docs/PERF.md, "Decode GEMM header").
// The epilogues see one wave's accumulators in the 16x16 MFMA C layout,
// acc[i][j][r] = C[16 * i + nq + r][16 * j + (lane & 15)], nq = 4 * (lane >> 4):
// column = token, rows = 4 consecutive features per lane - the layout the
// prompt-pass GEMMs (gemm_mfma.h) also produce.
template <int RT, int MT, int U, int WR, int MODE, int NORM, int XL, int FMT = 0>
__device__ __forceinline__ void skinny_fused_tile(const FusedArgs& a, float* smem, bf16_t* xs, const int bx,
                                                  const int by) {
  constexpr int WK = 4 / WR;                     // waves along K
  static_assert(!XL || WR == 4, "XL needs the 4 waves along rows");
  // XL + RoPE at MT 8: the RoPE cos/sin operands (RT * MT * 8 VGPRs) are
  // loaded after the k loop instead of being held through it
  constexpr bool EARLY_EPI = !(XL && MODE == FEPI_ROPE && MT > 4);
  float4v* red = reinterpret_cast<float4v*>(smem);
  float* sred = smem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave % WR, wk = wave / WR;
  const int tile = bx * WR + wr;                 // (16 * RT)-row output tile
  const int s = by;                              // K split
  const int KS = a.K >> 5;
  const int kw = KS / (a.S * WK);
  const int ks0 = (s * WK + wk) * kw;
  // elements of W per 16-row tile (MXFP4: bytes of the nibble stream)
  const size_t tile_stride = (size_t)KS * (FMT == WF_MXFP4 ? 256 : 512);
  typedef typename std::conditional<FMT != 0, fp8_t, bf16_t>::type W;
  const auto wp = [&]() {
    const W* p = reinterpret_cast<const W*>(a.Wp) + (size_t)(tile * RT) * tile_stride +
                 (size_t)lane * (FMT ? 16 : 8);
    if constexpr (FMT == WF_MXFP4)   // a.wscale: the e8m0 scale stream
      return Mx4Ptr{p, reinterpret_cast<const unsigned char*>(a.wscale) +
                           (size_t)(tile * RT) * (tile_stride >> 4) + (size_t)(lane & 15) * 4};
    else
      return p;
  }();
  const bf16_t* xp = a.x + (size_t)(lane & 15) * a.ldx + 8 * (lane >> 4);

  // the first weight group is requested before the norm prologue: the row
  // statistics only scale the accumulator, so the stream need not wait for
  // them (the prologue's two L2 round trips then hide under the first fill)
  Frag<RT, MT, XL ? 1 : U, FMT> f0, f1;
  WFrag<RT, XL ? U : 1, FMT> w0, w1;
  XRegs<XL ? MT * 16 : 64, XL ? U : 1> xr;
  const int ng = kw / U;
  if constexpr (XL) {
    load_xc<MT * 16, U>(xr, a.x, a.ldx, ks0);      // x first: storing it waits for x only
    load_w(w0, wp, tile_stride, ks0);
  } else {
    load_frag(f0, wp, tile_stride, xp, a.ldx, ks0);
  }

  // Epilogue operands (residual tile, bias, LayerNorm column sums, RoPE
  // positions / cos-sin / cache slots) are requested now, by the epilogue
  // wave only: their latency hides under the weight stream instead of adding
  // one or two dependent round trips after the last MFMA.
  const int nq = 4 * (lane >> 4);
  uint2 rres[RT][MT];
  float4 bvec[RT], cvec[RT], svec[RT];
  int eslot[MT];
  float2 ecs[RT][MT][4];
  // RoPE epilogue operands: 16-row pair tiles, rows 0-7 = features c..c+7 of
  // the first half, rows 8-15 = their RoPE partners c+D/2..; lanes (l>>4) & 1
  // pick c's 4-row half
  auto load_rope_ops = [&]() {
    const int tph = a.D / 16, nq_t = a.H * tph, nk_t = a.Hkv * tph;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int m = j * 16 + (lane & 15);
      eslot[j] = a.slots[m];
      if (a.cs) {
        const int pos = a.positions[m];
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          const int pt = tile * RT + i;
          if (pt < nq_t + nk_t) {
            const int tt = pt >= nq_t ? pt - nq_t : pt;
            const int c = (tt % tph) * 8 + 4 * ((lane >> 4) & 1);
            const float2* e = a.cs + (size_t)pos * (a.D >> 1) + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) ecs[i][j][r] = e[r];
          }
        }
      }
    }
  };
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    bvec[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    cvec[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    svec[i] = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
    for (int j = 0; j < MT; ++j) rres[i][j] = make_uint2(0u, 0u);
  }
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    eslot[j] = -1;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) ecs[i][j][r] = make_float2(1.f, 0.f);
  }
  if (wk == 0) {
    if constexpr (FMT == WF_FP8) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
        svec[i] = *reinterpret_cast<const float4*>(a.wscale + tile * (16 * RT) + i * 16 + nq);
    }
    if (a.bias) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
        bvec[i] = *reinterpret_cast<const float4*>(a.bias + tile * (16 * RT) + i * 16 + nq);
    }
    if constexpr (NORM == NORM_LN) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
        cvec[i] = *reinterpret_cast<const float4*>(a.colsum + tile * (16 * RT) + i * 16 + nq);
    }
    if constexpr (MODE == FEPI_RESID) {
#pragma unroll
      for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int i = 0; i < RT; ++i)
          rres[i][j] = *reinterpret_cast<const uint2*>(
              a.residual + (size_t)(j * 16 + (lane & 15)) * a.N + tile * (16 * RT) + i * 16 + nq);
    } else if constexpr (MODE == FEPI_ROPE && EARLY_EPI) {
      load_rope_ops();
    }
  }

  float sc[MT], mu[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) sc[j] = 1.f, mu[j] = 0.f;
  if constexpr (NORM != NORM_NONE) {
    // row statistics from the producer's per-tile partial sums (fixed order):
    // RMSNorm scale rsqrt(E[x^2] + eps); LayerNorm also the mean
    const int Mp = a.Mpad, G = 256 / Mp;
    const int m = threadIdx.x % Mp, g = threadIdx.x / Mp;
    // loads issued 16 at a time before any add (a dependent loop would
    // serialise one memory latency per tile)
    float aq = 0.f, as = 0.f;
    for (int base = 0; base < a.rowstat_tiles; base += 16 * G) {
      float vq[16], vs[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int t = base + g + i * G;
        const bool ok = t < a.rowstat_tiles;
        vq[i] = ok ? a.rowsq_in[(size_t)t * Mp + m] : 0.f;
        if constexpr (NORM == NORM_LN) vs[i] = ok ? a.rowsum_in[(size_t)t * Mp + m] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        aq += vq[i];
        if constexpr (NORM == NORM_LN) as += vs[i];
      }
    }
    sred[g * Mp + m] = aq;
    if constexpr (NORM == NORM_LN) sred[SRED_SUM + g * Mp + m] = as;
    lds_barrier();
    if (threadIdx.x < Mp) {
      float tq = 0.f, ts = 0.f;
      for (int q = 0; q < G; ++q) {
        tq += sred[q * Mp + threadIdx.x];
        if constexpr (NORM == NORM_LN) ts += sred[SRED_SUM + q * Mp + threadIdx.x];
      }
      const float mean = ts / (float)a.K;
      const float var = fmaxf(tq / (float)a.K - mean * mean, 0.f);
      sred[SRED_SCALE + threadIdx.x] = rsqrtf(var + a.eps);
      sred[SRED_MEAN + threadIdx.x] = mean;
    }
    lds_barrier();
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      sc[j] = sred[SRED_SCALE + j * 16 + (lane & 15)];
      mu[j] = sred[SRED_MEAN + j * 16 + (lane & 15)];
    }
    lds_barrier();
  }

  float4v acc[RT][MT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = (float4v){0.f, 0.f, 0.f, 0.f};
  if constexpr (XL) {
    stream_k_xl(w0, w1, xr, acc, wp, tile_stride, a.x, a.ldx, xs, ks0, ng, lane);
    if constexpr (MODE == FEPI_ROPE && !EARLY_EPI) load_rope_ops();
  } else {
    stream_k(f0, f1, acc, wp, tile_stride, xp, a.ldx, ks0, ng);
  }

  if constexpr (WK > 1) {
    // red[wr][wk - 1][i * MT + j][lane]
    auto ridx = [&](int q, int ij) { return ((wr * (WK - 1) + q) * RT * MT + ij) * 64 + lane; };
    if (wk > 0) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) red[ridx(wk - 1, i * MT + j)] = acc[i][j];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
          for (int q = 0; q < WK - 1; ++q) acc[i][j] += red[ridx(q, i * MT + j)];
    }
  }
  if ((WR == 1 || XL) && a.S > 1) {
    // publish this split's partial (tile-contiguous slab, sc1 write-through),
    // take a ticket; the last arriver reduces with sc1 loads (no acquire fence:
    // every handed-off byte is stored and loaded sc1, guide §6 Guideline 16).
    // WR == 1: wave 0 holds the workgroup's tile; XL (WR == 4): every wave
    // publishes and tickets its own tile.
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.part, 0, (int)((size_t)(a.N / (16 * RT * WR)) * WR * a.S * RT * MT * 64 * 16), 0x00020000);
    const int slab0 = tile * a.S * RT * MT;
    if (WR > 1 || wave == 0) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
          __builtin_amdgcn_raw_buffer_store_b128(
              __builtin_bit_cast(u32x4, acc[i][j]), rsrc,
              (((slab0 + s * RT * MT) + i * MT + j) * 64 + lane) * 16, 0, 16);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if constexpr (WR > 1) {
      int t = 0;
      if (lane == 0) {
        t = __hip_atomic_fetch_add(&a.counters[tile], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == a.S - 1)
          __hip_atomic_store(&a.counters[tile], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      t = __shfl(t, 0, 64);
      if (t != a.S - 1) return;
    } else {
      __syncthreads();
      if (threadIdx.x == 0) {
        const int t = __hip_atomic_fetch_add(&a.counters[tile], 1, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (t == a.S - 1)
          __hip_atomic_store(&a.counters[tile], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sred[0] = (float)t;
      }
      __syncthreads();
      if ((int)sred[0] != a.S - 1 || wave != 0) return;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // fixed summation order (split 0..S-1) whichever block arrives last
    float4v tot[RT][MT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) tot[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
    // QB slabs per batch, every load issued before the adds (a rolled loop
    // pays one L2 round trip per split); out-of-range slots add exact zeros
    constexpr int QB = (8 / (RT * MT)) > 2 ? 8 / (RT * MT) : 2;
    for (int q0 = 0; q0 < a.S; q0 += QB) {
      float4v v[QB][RT][MT];
#pragma unroll
      for (int qq = 0; qq < QB; ++qq)
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int j = 0; j < MT; ++j)
            v[qq][i][j] = q0 + qq < a.S
                              ? __builtin_bit_cast(float4v, __builtin_amdgcn_raw_buffer_load_b128(
                                                                 rsrc, (((slab0 + (q0 + qq) * RT * MT) + i * MT + j) * 64 + lane) * 16, 0, 16))
                              : float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int qq = 0; qq < QB; ++qq)
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int j = 0; j < MT; ++j) tot[i][j] += v[qq][i][j];
    }
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] = tot[i][j];
  } else if (wk != 0) {
    return;
  }

  // ---- epilogue (the wk == 0 wave of each row tile): acc[i][j] = C[n0 + 4*(lane>>4) + r][m] for i = tile half
  // Norms: the norm weight g is folded into W at load time, so the row scale
  // factors out of the k-sum: RMSNorm  y = s * (W g) x;  LayerNorm
  // y = s * ((W g) x - mean * colsum) with colsum[n] = sum_k (W g)[n][k]; the
  // LayerNorm shift (W b) is folded into the bias.
  // fp8 weights: the K reduction is complete here (cross-wave and split-K), so
  // the per-row dequantisation scale comes first (MXFP4: the block scales
  // went into the A fragments, nothing is left to apply)
  if constexpr (FMT == WF_FP8) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const float4 sv = svec[i];
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        acc[i][j][0] *= sv.x; acc[i][j][1] *= sv.y; acc[i][j][2] *= sv.z; acc[i][j][3] *= sv.w;
      }
    }
  }
  if constexpr (NORM == NORM_RMS) {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] *= sc[j];
  } else if constexpr (NORM == NORM_LN) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const float4 cv = cvec[i];
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        acc[i][j][0] = sc[j] * (acc[i][j][0] - mu[j] * cv.x);
        acc[i][j][1] = sc[j] * (acc[i][j][1] - mu[j] * cv.y);
        acc[i][j][2] = sc[j] * (acc[i][j][2] - mu[j] * cv.z);
        acc[i][j][3] = sc[j] * (acc[i][j][3] - mu[j] * cv.w);
      }
    }
  }
  if (a.bias) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const float4 bv = bvec[i];
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        acc[i][j][0] += bv.x; acc[i][j][1] += bv.y; acc[i][j][2] += bv.z; acc[i][j][3] += bv.w;
      }
    }
  }
  if constexpr (MODE == FEPI_SILU) {
    // 16-row pair tiles (perm_gate_up): rows 0-7 gate, rows 8-15 the matching
    // up rows -> lane l (l < 32) holds gate, lane l ^ 32 its up partner
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int m = j * 16 + (lane & 15);
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float own = bf2f(f2bf(acc[i][j][r]));
          const float oth = __shfl_xor(own, 32, 64);
          o[r] = own / (1.f + __expf(-own)) * oth;
        }
        if (lane < 32) {
          uint2 w2;
          w2.x = pack_bf16x2(o[0], o[1]);
          w2.y = pack_bf16x2(o[2], o[3]);
          *reinterpret_cast<uint2*>(a.out + (size_t)m * a.ldo + (tile * RT + i) * 8 + nq) = w2;
        }
      }
  } else if constexpr (MODE == FEPI_RESID) {
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int m = j * 16 + (lane & 15);
      float sq = 0.f, sm = 0.f;
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        bf16_t* rp = a.residual + (size_t)m * a.N + tile * (16 * RT) + i * 16 + nq;
        const uint2 rv = rres[i][j];
        const float r0 = bf2f(rv.x & 0xffff), r1 = bf2f(rv.x >> 16);
        const float r2 = bf2f(rv.y & 0xffff), r3 = bf2f(rv.y >> 16);
        const float h0 = bf2f(f2bf(acc[i][j][0] + r0)), h1 = bf2f(f2bf(acc[i][j][1] + r1));
        const float h2 = bf2f(f2bf(acc[i][j][2] + r2)), h3 = bf2f(f2bf(acc[i][j][3] + r3));
        uint2 w2;
        w2.x = pack_bf16x2(h0, h1);
        w2.y = pack_bf16x2(h2, h3);
        *reinterpret_cast<uint2*>(rp) = w2;
        sq += h0 * h0 + h1 * h1 + h2 * h2 + h3 * h3;
        sm += h0 + h1 + h2 + h3;
      }
      sq += __shfl_xor(sq, 16, 64);
      sq += __shfl_xor(sq, 32, 64);
      sm += __shfl_xor(sm, 16, 64);
      sm += __shfl_xor(sm, 32, 64);
      if (lane < 16) {
        a.rowsq_out[(size_t)tile * a.Mpad + m] = sq;
        if (a.rowsum_out) a.rowsum_out[(size_t)tile * a.Mpad + m] = sm;
      }
    }
  } else if constexpr (MODE == FEPI_ROPE) {
    // perm_rope_qkv: q / k as 16-row pair tiles (rows 0-7 = first-half features
    // c.., rows 8-15 = partners c+D/2..: lane l and l ^ 32 hold a RoPE pair);
    // v rows in natural order
    const int D = a.D, half = D >> 1, tph = D / 16;
    const int nq_t = a.H * tph, nk_t = a.Hkv * tph;
    const bool lower = lane < 32;
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int pt = tile * RT + i;
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int m = j * 16 + (lane & 15);
        const int slot = eslot[j];
        if (pt < nq_t + nk_t) {
          const bool isk = pt >= nq_t;
          const int tt = isk ? pt - nq_t : pt;
          const int head = tt / tph;
          const int c = (tt - head * tph) * 8 + 4 * ((lane >> 4) & 1) + (lower ? 0 : half);
          float ov[4];
          if (a.cs) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float own = bf2f(f2bf(acc[i][j][r]));
              const float oth = __shfl_xor(own, 32, 64);
              const float2 cs = ecs[i][j][r];
              // lower: x0 cos - x1 sin; upper (own = x1, oth = x0): x1 cos + x0 sin
              ov[r] = own * cs.x + (lower ? -oth : oth) * cs.y;
            }
          } else {  // no rotary embedding (Whisper): plain q / k rows
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = acc[i][j][r];
          }
          uint2 w2;
          w2.x = pack_bf16x2(ov[0], ov[1]);
          w2.y = pack_bf16x2(ov[2], ov[3]);
          if (!isk) {
            *reinterpret_cast<uint2*>(a.q_out + (size_t)m * a.H * D + head * D + c) = w2;
          } else {
            if (slot < 0) continue;
            const int bb = slot / a.blk, o = slot - bb * a.blk;
            *reinterpret_cast<uint2*>(a.kc + (((size_t)bb * a.Hkv + head) * a.blk + o) * D + c) = w2;
          }
        } else {
          if (slot < 0) continue;
          const int bb = slot / a.blk, o = slot - bb * a.blk;
          const int row = (pt - nq_t - nk_t) * 16 + nq;
          const int head = row / D, c = row - head * D;
          uint2 w2;
          w2.x = pack_bf16x2(acc[i][j][0], acc[i][j][1]);
          w2.y = pack_bf16x2(acc[i][j][2], acc[i][j][3]);
          *reinterpret_cast<uint2*>(a.vc + (((size_t)bb * a.Hkv + head) * a.blk + o) * D + c) = w2;
        }
      }
    }
  } else if constexpr (MODE == FEPI_ACT) {
    if (a.act == 2) {
      // f32 output (tensor-parallel partial sums: the all-reduce adds them in
      // f32 before the one bf16 rounding of the residual, as the single-GPU
      // residual epilogue does)
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int m = j * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < RT; ++i)
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + (size_t)m * a.ldo +
                                     tile * (16 * RT) + i * 16 + nq) =
              make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int m = j * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = bf2f(f2bf(acc[i][j][r]));
          o[r] = a.act == 1 ? 0.5f * x * (1.f + erff(x * 0.70710678118654752f)) : x;
        }
        uint2 w2;
        w2.x = pack_bf16x2(o[0], o[1]);
        w2.y = pack_bf16x2(o[2], o[3]);
        *reinterpret_cast<uint2*>(a.out + (size_t)m * a.ldo + tile * (16 * RT) + i * 16 + nq) = w2;
      }
    }
  }
}

template <int RT, int MT, int U, int WR, int MODE, int NORM, int XL = 0>
__global__ __launch_bounds__(256) void skinny_fused_kernel(FusedArgs a) {
  constexpr int SMF = FusedSmem<RT, MT, WR>::NSM + 4;   // + 4: unused pad, kept so every kernel's LDS size stays as measured
  __shared__ __attribute__((aligned(16))) float smem[SMF];
  __shared__ __attribute__((aligned(16))) bf16_t xs[XL ? U * MT * 16 * XROW : 8];
  if (a.prio) __builtin_amdgcn_s_setprio(3);     // kernel argument: wave-uniform
  skinny_fused_tile<RT, MT, U, WR, MODE, NORM, XL>(a, smem, xs, blockIdx.x, blockIdx.y);
}

// the fp8 weight stream: its own kernel name, so the bf16 instances keep theirs
template <int RT, int MT, int U, int WR, int MODE, int NORM, int XL = 0>
__global__ __launch_bounds__(256) void skinny_fused_fp8_kernel(FusedArgs a) {
  constexpr int SMF = FusedSmem<RT, MT, WR>::NSM + 4;
  __shared__ __attribute__((aligned(16))) float smem[SMF];
  __shared__ __attribute__((aligned(16))) bf16_t xs[XL ? U * MT * 16 * XROW : 8];
  if (a.prio) __builtin_amdgcn_s_setprio(3);
  skinny_fused_tile<RT, MT, U, WR, MODE, NORM, XL, 1>(a, smem, xs, blockIdx.x, blockIdx.y);
}

// the MXFP4 weight stream, likewise
template <int RT, int MT, int U, int WR, int MODE, int NORM, int XL = 0>
__global__ __launch_bounds__(256) void skinny_fused_mxfp4_kernel(FusedArgs a) {
  constexpr int SMF = FusedSmem<RT, MT, WR>::NSM + 4;
  __shared__ __attribute__((aligned(16))) float smem[SMF];
  __shared__ __attribute__((aligned(16))) bf16_t xs[XL ? U * MT * 16 * XROW : 8];
  if (a.prio) __builtin_amdgcn_s_setprio(3);
  skinny_fused_tile<RT, MT, U, WR, MODE, NORM, XL, WF_MXFP4>(a, smem, xs, blockIdx.x, blockIdx.y);
}

template <int FMT, int RT, int MT, int U, int WR, int MODE, int NORM, int XL>
static void launch_fused_kernel(dim3 grid, const FusedArgs& a, hipStream_t st) {
  if constexpr (FMT == WF_MXFP4)
    hipLaunchKernelGGL((skinny_fused_mxfp4_kernel<RT, MT, U, WR, MODE, NORM, XL>), grid, dim3(256), 0, st, a);
  else if constexpr (FMT == WF_FP8)
    hipLaunchKernelGGL((skinny_fused_fp8_kernel<RT, MT, U, WR, MODE, NORM, XL>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((skinny_fused_kernel<RT, MT, U, WR, MODE, NORM, XL>), grid, dim3(256), 0, st, a);
}

// One layout (RT, MT, WR, XL) -> its kernel, by the prefetch group U.
// WR = 1 (4 waves along K): groups of 4 k-steps, of 2 or 1 when the wave's k
// range does not divide. (Deeper groups - 8 steps, or a Whisper wave's whole
// 10-step range in one - measured slower in the pipeline, 3.51 -> 3.68 ms per
// LLM step, and were removed: docs/KNOBS.md.)
// (fp8: a 16-byte weight load spans two k-steps, so a wave's k range must be
// even - K % (S * WK * 64) == 0 - and is rejected otherwise. MXFP4: four
// k-steps, K % (S * WK * 128) == 0; the layouts with groups of 2 k-steps take
// the load in 8-byte halves)
// WR = 4: one group size per layout. loqa_skinny_fused admits only
// K % (S * 128) == 0, and WR = 4 without XL only S == 1, so a wave's k range
// is a multiple of 4 k-steps and no smaller group is ever needed; the check
// here keeps a caller that bypasses the entry point from reading past K.
//   register form: at most 2 k-steps per group at Mpad 64 (VGPRs);
//   XL: the group is one LDS chunk, 2 k-steps when the VGPR budget is tight.
template <int RT, int MT, int WR, int XL, int MODE, int NORM, int FMT>
static int launch_fused(const FusedArgs& a, hipStream_t st) {
  constexpr int WK = 4 / WR;
  dim3 grid(a.N / (16 * RT * WR), a.S);
  const int kw = a.K / 32 / (a.S * WK);
  if (FMT == WF_MXFP4 && kw % 4) return (int)hipErrorInvalidValue;
  if constexpr (WR == 4) {
    constexpr int U = XL ? (RT * MT >= 16 ? 2 : 4) : (MT <= 2 ? 4 : 2);
    if (kw % U) return (int)hipErrorInvalidValue;
    launch_fused_kernel<FMT, RT, MT, U, 4, MODE, NORM, XL>(grid, a, st);
  } else if (MT <= 2 && kw % 4 == 0) {   // Mpad 64: at most 2 k-steps per prefetch group (VGPRs)
    launch_fused_kernel<FMT, RT, MT, (MT <= 2 ? 4 : 2), 1, MODE, NORM, 0>(grid, a, st);
  } else if (kw % 2 == 0) {
    launch_fused_kernel<FMT, RT, MT, 2, 1, MODE, NORM, 0>(grid, a, st);
  } else if constexpr (!FMT) {
    launch_fused_kernel<0, RT, MT, 1, 1, MODE, NORM, 0>(grid, a, st);
  } else {
    return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// Every legal layout, as (Mpad, rt, wr, xl) -> launch_fused<RT, MT = Mpad / 16, WR, XL>.
// rt: rows per output tile / 16 (1 or 2, every mode: the paired epilogues pair
// rows inside each 16-row tile through a lane shuffle, so 16-row tiles give
// twice the workgroups without a K split, i.e. without a reduction tail).
// rt 4: 64-row tiles at Mpad 64 (chunked prefill through the compact weights):
// the activation tile is then re-read from L2 by half as many workgroups.
// wr: waves along the rows (1 or 4; 4 only with S == 1, or with xl).
// xl: x through LDS, Mpad 32 / 64 / 128, 4 waves along rows, any split-K.
template <int MODE, int NORM, int FMT>
static int dispatch_shape(const FusedArgs& a, int rt, int wr, int xl, hipStream_t st) {
  auto is = [&](int mpad, int r, int w, int x) { return a.Mpad == mpad && rt == r && wr == w && !xl == !x; };
  if (is(16, 1, 1, 0)) return launch_fused<1, 1, 1, 0, MODE, NORM, FMT>(a, st);
  if (is(16, 1, 4, 0)) return launch_fused<1, 1, 4, 0, MODE, NORM, FMT>(a, st);
  if (is(16, 2, 1, 0)) return launch_fused<2, 1, 1, 0, MODE, NORM, FMT>(a, st);
  if (is(16, 2, 4, 0)) return launch_fused<2, 1, 4, 0, MODE, NORM, FMT>(a, st);
  if (is(32, 1, 1, 0)) return launch_fused<1, 2, 1, 0, MODE, NORM, FMT>(a, st);
  if (is(32, 1, 4, 0)) return launch_fused<1, 2, 4, 0, MODE, NORM, FMT>(a, st);
  if (is(32, 2, 1, 0)) return launch_fused<2, 2, 1, 0, MODE, NORM, FMT>(a, st);
  if (is(32, 2, 4, 0)) return launch_fused<2, 2, 4, 0, MODE, NORM, FMT>(a, st);
  if (is(64, 1, 1, 0)) return launch_fused<1, 4, 1, 0, MODE, NORM, FMT>(a, st);
  if (is(64, 1, 4, 0)) return launch_fused<1, 4, 4, 0, MODE, NORM, FMT>(a, st);
  if (is(64, 2, 1, 0)) return launch_fused<2, 4, 1, 0, MODE, NORM, FMT>(a, st);
  if (is(64, 2, 4, 0)) return launch_fused<2, 4, 4, 0, MODE, NORM, FMT>(a, st);
  if (is(64, 4, 1, 0)) return launch_fused<4, 4, 1, 0, MODE, NORM, FMT>(a, st);
  if (is(64, 4, 4, 0)) return launch_fused<4, 4, 4, 0, MODE, NORM, FMT>(a, st);
  if (is(32, 1, 4, 1)) return launch_fused<1, 2, 4, 1, MODE, NORM, FMT>(a, st);
  if (is(32, 2, 4, 1)) return launch_fused<2, 2, 4, 1, MODE, NORM, FMT>(a, st);
  if (is(64, 1, 4, 1)) return launch_fused<1, 4, 4, 1, MODE, NORM, FMT>(a, st);
  if (is(64, 2, 4, 1)) return launch_fused<2, 4, 4, 1, MODE, NORM, FMT>(a, st);
  if (is(128, 1, 4, 1)) return launch_fused<1, 8, 4, 1, MODE, NORM, FMT>(a, st);
  if (is(128, 2, 4, 1)) return launch_fused<2, 8, 4, 1, MODE, NORM, FMT>(a, st);
  return (int)hipErrorInvalidValue;
}

// fp8 / MXFP4 weights: NORM_NONE and NORM_RMS only (the Llama decode), LayerNorm is rejected
template <int MODE, int FMT>
static int dispatch_norm(const FusedArgs& a, int norm, int rt, int wr, int xl, hipStream_t st) {
  switch (norm) {
    case NORM_NONE: return dispatch_shape<MODE, NORM_NONE, FMT>(a, rt, wr, xl, st);
    case NORM_RMS: return dispatch_shape<MODE, NORM_RMS, FMT>(a, rt, wr, xl, st);
    case NORM_LN:
      if constexpr (!FMT) return dispatch_shape<MODE, NORM_LN, 0>(a, rt, wr, xl, st);
    default: return (int)hipErrorInvalidValue;
  }
}

template <int FMT>
static int dispatch_mode(const FusedArgs& a, int mode, int norm, int rt, int wr, int xl, hipStream_t st) {
  switch (mode) {
    case FEPI_SILU: return dispatch_norm<FEPI_SILU, FMT>(a, norm, rt, wr, xl, st);
    case FEPI_RESID: return dispatch_norm<FEPI_RESID, FMT>(a, norm, rt, wr, xl, st);
    case FEPI_ROPE: return dispatch_norm<FEPI_ROPE, FMT>(a, norm, rt, wr, xl, st);
    case FEPI_ACT: return dispatch_norm<FEPI_ACT, FMT>(a, norm, rt, wr, xl, st);
    default: return (int)hipErrorInvalidValue;
  }
}
