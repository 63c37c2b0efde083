// Device helpers of the row scans over a logits row: the masked argmax modes
// (elementwise.hip) and the beam top-k (beam.hip). Both accumulate a row's
// (max, sum exp) with these functions in the same order, so their
// log-probabilities agree bit for bit.
#pragma once
#include "common.h"

#define ARG_CHUNK 8192
#define ARG_THREADS 256

__device__ __forceinline__ unsigned long long argpack(float v, int idx) {
  const uint32_t bits = __float_as_uint(v);
  const uint32_t key = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return ((unsigned long long)key << 32) | (0xFFFFFFFFu - (uint32_t)idx);
}

__device__ __forceinline__ int argunpack(unsigned long long p, const int* __restrict__ token_ids) {
  if (!p) return -1;
  const int col = (int)(0xFFFFFFFFu - (uint32_t)(p & 0xFFFFFFFFull));
  return token_ids ? token_ids[col] : col;
}

__device__ __forceinline__ void lse_add(float& m, float& s, float x) {
  if (x == -INFINITY) return;     // weight 0 (and keeps inf - inf out of the sum)
  const float d = x - m;          // m == -inf: d = +inf, e = 0, s = 0 * 0 + 1
  const float e = expf(-fabsf(d));
  if (d > 0.f) {
    s = s * e + 1.f;
    m = x;
  } else {
    s += e;
  }
}

// a vector group: the running maximum moves at most once (one rescaling expf),
// then the group's expf are independent of each other
template <int N>
__device__ __forceinline__ void lse_add_group(float& m, float& s, const float (&f)[N],
                                              uint32_t bits) {
  float gm = -INFINITY;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if ((bits >> j) & 1u) gm = fmaxf(gm, f[j]);
  if (gm == -INFINITY) return;    // nothing allowed in the group, or only -inf
  if (gm > m) {
    s *= expf(m - gm);            // m == -inf: s == 0 stays 0
    m = gm;
  }
#pragma unroll
  for (int j = 0; j < N; ++j)
    if ((bits >> j) & 1u) s += expf(f[j] - m);   // m finite: -inf gives 0
}

// s = s * exp(m - mm) + s2 * exp(m2 - mm) with its roundings spelled out. Left
// to -ffp-contract=fast the compiler decides per call site which of the two
// products an fma absorbs, or, where it packs the two multiplies into one
// instruction, that none is, and the bits of the sum follow that choice.
// FMA: the first product rounds, the second is fused (the masked pair inside a
// workgroup); otherwise both products round (the all-column pair, and the
// merge of chunk records). These are the forms the three hand-copied kernels
// had been compiled to; the results are held to those bits.
template <bool FMA>
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  float r;
  if constexpr (FMA) {
    r = fmaf(s2, expf(m2 - mm), s * expf(m - mm));
  } else {
#pragma clang fp contract(off)
    r = s * expf(m - mm) + s2 * expf(m2 - mm);
  }
  // both empty: s == s2 == 0 stays (r is NaN there). A select, not an early
  // return: a merge in the shuffle tree must not become a branch.
  s = mm == -INFINITY ? s : r;
  m = mm;
}

__device__ __forceinline__ float lse_logprob(unsigned long long best, float m, float s) {
  return (best && m != -INFINITY) ? 0.f - logf(s) : -INFINITY;
}

__device__ __forceinline__ float arg_load(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float arg_load(const float* p) { return *p; }
__device__ __forceinline__ void arg_load_group(const bf16_t* p, float (&f)[8]) {
  unpack8(*reinterpret_cast<const uint4*>(p), f);
}
__device__ __forceinline__ void arg_load_group(const float* p, float (&f)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  f[0] = q.x, f[1] = q.y, f[2] = q.z, f[3] = q.w;
}
