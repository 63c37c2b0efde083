// Memory-bound fused elementwise kernels:
//   K1  pcm16 -> f32 conversion fused with the per-utterance sum of squares used
//       by wake-word arbitration RMS (reference: audio_service.go:1048-1101 and
//       :818-852 do these as two per-sample Go loops).
//   K6  bias + GELU (+ sinusoidal position add) epilogue for Whisper conv/MLP.
//   K11 RoPE on q/k + paged KV-cache append (K16), reading the fused QKV GEMM
//       output in place.
//   K14 SwiGLU gate: silu(gate) * up.
//   K15 grammar-masked argmax over the vocabulary (jump-forward JSON decoding).
// All bf16 traffic is 8-16 bytes per lane (guide G13).
#include "common.h"
#include "argscan.h"
#include <float.h>
#include <type_traits>

// ---------------------------------------------------------------- K14 SwiGLU
// in: [T, 2F] = [gate | up], out: [T, F]. 2-D grid (x: 8-wide column vectors,
// y: rows): one 16-byte vector per thread, no per-element 64-bit division (the
// grid-stride form with `i / (F / 8)` ran at 0.8 TB/s on the 318 x 14336
// prefill activations; these kernels are pure streams).
__global__ __launch_bounds__(256) void silu_mul_kernel(const bf16_t* __restrict__ in,
                                                      bf16_t* __restrict__ out, int F) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= (F >> 3)) return;
  const size_t row = blockIdx.y;
  const uint4 gv = reinterpret_cast<const uint4*>(in + row * 2 * F)[c];
  const uint4 uv = reinterpret_cast<const uint4*>(in + row * 2 * F + F)[c];
  float a[8], b[8], o[8];
  unpack8(gv, a);
  unpack8(uv, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = a[j] / (1.f + __expf(-a[j])) * b[j];
  reinterpret_cast<uint4*>(out + row * F)[c] = pack8(o);
}

extern "C" int loqa_silu_mul(const void* in, void* out, long long rows, int F, hipStream_t s) {
  if (F % 8 != 0 || rows <= 0) return (int)hipErrorInvalidValue;
  for (long long r0 = 0; r0 < rows; r0 += 65535) {   // grid.y limit
    const long long n = rows - r0 < 65535 ? rows - r0 : 65535;
    dim3 grid((unsigned)((F / 8 + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(silu_mul_kernel, grid, dim3(256), 0, s, (const bf16_t*)in + r0 * 2 * F,
                       (bf16_t*)out + r0 * F, F);
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ K6 bias+GELU(+pos)
// x[T, F] <- gelu(x + bias) + pos[(t % pos_period), :]   (bias, pos optional);
// 2-D grid as silu_mul
__global__ __launch_bounds__(256) void gelu_bias_kernel(bf16_t* __restrict__ x,
                                                       const bf16_t* __restrict__ bias,
                                                       const bf16_t* __restrict__ pos, int F,
                                                       int pos_period, long long row0) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= (F >> 3)) return;
  const size_t row = (size_t)row0 + blockIdx.y;
  uint4* p = reinterpret_cast<uint4*>(x + row * F) + c;
  float v[8];
  unpack8(*p, v);
  if (bias) {
    float b[8];
    unpack8(reinterpret_cast<const uint4*>(bias)[c], b);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += b[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.5f * v[j] * (1.f + erff(v[j] * 0.70710678118654752f));
  if (pos) {
    float q[8];
    const size_t prow = row % (size_t)pos_period;
    unpack8(reinterpret_cast<const uint4*>(pos + prow * F)[c], q);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += q[j];
  }
  *p = pack8(v);
}

extern "C" int loqa_gelu_bias(void* x, const void* bias, const void* pos, long long rows, int F,
                              int pos_period, hipStream_t s) {
  if (F % 8 != 0 || rows <= 0 || (pos && pos_period <= 0)) return (int)hipErrorInvalidValue;
  for (long long r0 = 0; r0 < rows; r0 += 65535) {   // grid.y limit
    const long long n = rows - r0 < 65535 ? rows - r0 : 65535;
    dim3 grid((unsigned)((F / 8 + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(gelu_bias_kernel, grid, dim3(256), 0, s, (bf16_t*)x, (const bf16_t*)bias,
                       (const bf16_t*)pos, F, pos_period, r0);
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------ K11/K16 RoPE + KV append
// qkv: [T, stride] with q at [0, Hq*D), k at [Hq*D, (Hq+Hkv)*D), v after it.
// q (and k) are rotated in place (NeoX rotate-half pairing i <-> i + D/2);
// k and v are then written to the paged cache [nblocks, Hkv, blk, D] at
// slot = slots[t] (= block * blk + offset). cs == nullptr disables the rotation
// (Whisper decoder, learned positions). slots[t] < 0 skips the append (padding).
__global__ void rope_kv_append_kernel(bf16_t* __restrict__ qkv, int stride,
                                      const int* __restrict__ positions,
                                      const float2* __restrict__ cs, bf16_t* __restrict__ kc,
                                      bf16_t* __restrict__ vc, const int* __restrict__ slots,
                                      int Hq, int Hkv, int D, int blk) {
  const int t = blockIdx.x;
  bf16_t* row = qkv + (size_t)t * stride;
  const int half = D >> 1;
  const int pv = half >> 2;  // 4-element groups per half-head
  const int slot = slots ? slots[t] : -1;
  const float2* csr = cs ? cs + (size_t)positions[t] * half : nullptr;
  const int nq = Hq * pv, nk = Hkv * pv;
  // q and k rotation (k rotation only materialised into the cache).
  for (int i = threadIdx.x; i < nq + nk; i += blockDim.x) {
    const bool isk = i >= nq;
    const int ii = isk ? i - nq : i;
    const int h = ii / pv, c = (ii - h * pv) * 4;
    bf16_t* base = row + (isk ? Hq * D : 0) + h * D;
    uint2 lo = *reinterpret_cast<const uint2*>(base + c);
    uint2 hi = *reinterpret_cast<const uint2*>(base + c + half);
    if (csr) {
      float a[4] = {__uint_as_float(lo.x << 16), __uint_as_float(lo.x & 0xffff0000u),
                    __uint_as_float(lo.y << 16), __uint_as_float(lo.y & 0xffff0000u)};
      float b[4] = {__uint_as_float(hi.x << 16), __uint_as_float(hi.x & 0xffff0000u),
                    __uint_as_float(hi.y << 16), __uint_as_float(hi.y & 0xffff0000u)};
      float ra[4], rb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float2 e = csr[c + j];
        ra[j] = a[j] * e.x - b[j] * e.y;
        rb[j] = b[j] * e.x + a[j] * e.y;
      }
      lo.x = pack_bf16x2(ra[0], ra[1]);
      lo.y = pack_bf16x2(ra[2], ra[3]);
      hi.x = pack_bf16x2(rb[0], rb[1]);
      hi.y = pack_bf16x2(rb[2], rb[3]);
    }
    if (!isk) {
      *reinterpret_cast<uint2*>(base + c) = lo;
      *reinterpret_cast<uint2*>(base + c + half) = hi;
    } else if (slot >= 0) {
      const int b = slot / blk, o = slot - b * blk;
      bf16_t* dst = kc + (((size_t)b * Hkv + h) * blk + o) * D;
      *reinterpret_cast<uint2*>(dst + c) = lo;
      *reinterpret_cast<uint2*>(dst + c + half) = hi;
    }
  }
  if (slot >= 0) {
    const int b = slot / blk, o = slot - b * blk;
    const int dv = D >> 3;
    for (int i = threadIdx.x; i < Hkv * dv; i += blockDim.x) {
      const int h = i / dv, c = (i - h * dv) * 8;
      const uint4 v = *reinterpret_cast<const uint4*>(row + (Hq + Hkv) * D + h * D + c);
      *reinterpret_cast<uint4*>(vc + (((size_t)b * Hkv + h) * blk + o) * D + c) = v;
    }
  }
}

// Same operation, every load of the row issued before any store: the loop form
// above reads, rotates and writes one 4-element group per trip, and its
// in-place q stores keep the compiler from hoisting the next trip's loads, so
// a thread pays one memory round trip per group (5 at Llama-3-8B's 40 heads).
// Here each thread holds up to RK groups (and its V piece) in registers.
template <int RK>
__global__ __launch_bounds__(128) void rope_kv_append_batched_kernel(
    bf16_t* __restrict__ qkv, int stride, const int* __restrict__ positions,
    const float2* __restrict__ cs, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
    const int* __restrict__ slots, int Hq, int Hkv, int D, int blk) {
  const int t = blockIdx.x;
  bf16_t* row = qkv + (size_t)t * stride;
  const int half = D >> 1, pv = half >> 2, dv = D >> 3;
  const int nq = Hq * pv, nk = Hkv * pv;
  uint2 lo[RK], hi[RK];
#pragma unroll
  for (int k = 0; k < RK; ++k) {
    const int i = threadIdx.x + k * 128;
    lo[k] = hi[k] = make_uint2(0u, 0u);
    if (i < nq + nk) {
      const bool isk = i >= nq;
      const int ii = isk ? i - nq : i;
      const int h = ii / pv, c = (ii - h * pv) * 4;
      const bf16_t* base = row + (isk ? Hq * D : 0) + h * D;
      lo[k] = *reinterpret_cast<const uint2*>(base + c);
      hi[k] = *reinterpret_cast<const uint2*>(base + c + half);
    }
  }
  const int slot = slots ? slots[t] : -1;
  const bool vok = slot >= 0 && (int)threadIdx.x < Hkv * dv;
  uint4 vv = make_uint4(0u, 0u, 0u, 0u);
  if (vok) {
    const int h = threadIdx.x / dv, c = (threadIdx.x - h * dv) * 8;
    vv = *reinterpret_cast<const uint4*>(row + (Hq + Hkv) * D + h * D + c);
  }
  const float2* csr = cs ? cs + (size_t)positions[t] * half : nullptr;
  float2 e[RK][4];
#pragma unroll
  for (int k = 0; k < RK; ++k) {
    const int i = threadIdx.x + k * 128;
    const int ii = i >= nq ? i - nq : i;
    const int c = (ii - (ii / pv) * pv) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      e[k][j] = (csr && i < nq + nk) ? csr[c + j] : make_float2(1.f, 0.f);
  }
#pragma unroll
  for (int k = 0; k < RK; ++k) {
    const int i = threadIdx.x + k * 128;
    if (i >= nq + nk) break;
    const bool isk = i >= nq;
    const int ii = isk ? i - nq : i;
    const int h = ii / pv, c = (ii - h * pv) * 4;
    uint2 l = lo[k], u = hi[k];
    if (csr) {
      float a[4] = {__uint_as_float(l.x << 16), __uint_as_float(l.x & 0xffff0000u),
                    __uint_as_float(l.y << 16), __uint_as_float(l.y & 0xffff0000u)};
      float b[4] = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                    __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
      float ra[4], rb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ra[j] = a[j] * e[k][j].x - b[j] * e[k][j].y;
        rb[j] = b[j] * e[k][j].x + a[j] * e[k][j].y;
      }
      l.x = pack_bf16x2(ra[0], ra[1]);
      l.y = pack_bf16x2(ra[2], ra[3]);
      u.x = pack_bf16x2(rb[0], rb[1]);
      u.y = pack_bf16x2(rb[2], rb[3]);
    }
    if (!isk) {
      bf16_t* base = row + h * D;
      *reinterpret_cast<uint2*>(base + c) = l;
      *reinterpret_cast<uint2*>(base + c + half) = u;
    } else if (slot >= 0) {
      const int b = slot / blk, o = slot - b * blk;
      bf16_t* dst = kc + (((size_t)b * Hkv + h) * blk + o) * D;
      *reinterpret_cast<uint2*>(dst + c) = l;
      *reinterpret_cast<uint2*>(dst + c + half) = u;
    }
  }
  if (vok) {
    const int b = slot / blk, o = slot - b * blk;
    const int h = threadIdx.x / dv, c = (threadIdx.x - h * dv) * 8;
    *reinterpret_cast<uint4*>(vc + (((size_t)b * Hkv + h) * blk + o) * D + c) = vv;
  }
}

extern "C" int loqa_rope_kv_append(void* qkv, int stride, const int* positions, const void* cs,
                                   void* kc, void* vc, const int* slots, int T, int Hq, int Hkv,
                                   int D, int blk, hipStream_t s) {
  if (T <= 0) return 0;
  if (D % 8 != 0 || stride < (Hq + 2 * Hkv) * D || (cs && !positions)) return (int)hipErrorInvalidValue;
  if ((Hq + Hkv) * (D / 8) <= 8 * 128 && Hkv * (D / 8) <= 128) {
    hipLaunchKernelGGL(rope_kv_append_batched_kernel<8>, dim3(T), dim3(128), 0, s, (bf16_t*)qkv,
                       stride, positions, (const float2*)cs, (bf16_t*)kc, (bf16_t*)vc, slots, Hq,
                       Hkv, D, blk);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(rope_kv_append_kernel, dim3(T), dim3(128), 0, s, (bf16_t*)qkv, stride,
                     positions, (const float2*)cs, (bf16_t*)kc, (bf16_t*)vc, slots, Hq, Hkv, D,
                     blk);
  return (int)hipGetLastError();
}

// --------------------------------------------- K1 PCM16 -> f32 + sum of squares
// pcm: concatenated int16 samples of S segments (offsets[S+1] in samples).
// out: f32 samples (x / 32767, as audio_service.go:1078), sumsq[S] accumulates.
#define PCM_CHUNK 8192
__global__ void pcm16_f32_sumsq_kernel(const int16_t* __restrict__ pcm, float* __restrict__ out,
                                       const long long* __restrict__ offsets,
                                       float* __restrict__ sumsq) {
  __shared__ float scratch[4];
  const int seg = blockIdx.y;
  const long long beg = offsets[seg], end = offsets[seg + 1];
  const long long c0 = beg + (long long)blockIdx.x * PCM_CHUNK;
  float acc = 0.f;
  if (c0 < end) {
    const long long c1 = min(end, c0 + PCM_CHUNK);
    for (long long i = c0 + threadIdx.x; i < c1; i += blockDim.x) {
      const float f = (float)pcm[i] * (1.0f / 32767.0f);
      out[i] = f;
      acc += f * f;
    }
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0 && c0 < end) atomicAdd(sumsq + seg, acc);
}

extern "C" int loqa_pcm16_f32_sumsq(const void* pcm, float* out, const long long* offsets,
                                    float* sumsq, int nseg, long long max_seg_len, hipStream_t s) {
  if (nseg <= 0) return 0;
  hipError_t e = hipMemsetAsync(sumsq, 0, sizeof(float) * nseg, s);
  if (e != hipSuccess) return (int)e;
  const long long chunks = max_seg_len <= 0 ? 1 : (max_seg_len + PCM_CHUNK - 1) / PCM_CHUNK;
  hipLaunchKernelGGL(pcm16_f32_sumsq_kernel, dim3((unsigned)chunks, nseg), dim3(256), 0, s,
                     (const int16_t*)pcm, out, offsets, sumsq);
  return (int)hipGetLastError();
}

// Padded variant: segment s lands in row s of out [nseg, ld] (the Whisper
// front end's 30 s window), zero beyond the segment - one launch instead of a
// zero-fill plus a copy per utterance.
__global__ void pcm16_f32_pad_kernel(const int16_t* __restrict__ pcm, float* __restrict__ out,
                                     const long long* __restrict__ offsets, float* __restrict__ sumsq,
                                     long long ld) {
  __shared__ float scratch[4];
  const int seg = blockIdx.y;
  const long long beg = offsets[seg], len = min(offsets[seg + 1] - beg, ld);
  const long long c0 = (long long)blockIdx.x * PCM_CHUNK;
  const long long c1 = min(ld, c0 + PCM_CHUNK);
  float* row = out + (size_t)seg * ld;
  float acc = 0.f;
  for (long long i = c0 + threadIdx.x; i < c1; i += blockDim.x) {
    const float f = i < len ? (float)pcm[beg + i] * (1.0f / 32767.0f) : 0.f;
    row[i] = f;
    acc += f * f;
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0 && c0 < len) atomicAdd(sumsq + seg, acc);
}

extern "C" int loqa_pcm16_f32_pad(const void* pcm, float* out, const long long* offsets, float* sumsq,
                                  int nseg, long long ld, hipStream_t s) {
  if (nseg <= 0 || ld <= 0) return nseg < 0 || ld < 0 ? (int)hipErrorInvalidValue : 0;
  hipError_t e = hipMemsetAsync(sumsq, 0, sizeof(float) * nseg, s);
  if (e != hipSuccess) return (int)e;
  const long long chunks = (ld + PCM_CHUNK - 1) / PCM_CHUNK;
  hipLaunchKernelGGL(pcm16_f32_pad_kernel, dim3((unsigned)chunks, nseg), dim3(256), 0, s,
                     (const int16_t*)pcm, out, offsets, sumsq, ld);
  return (int)hipGetLastError();
}

// --------------------------------------------------- K15 grammar-masked argmax
// One row scan in five modes behind loqa_masked_argmax (MODE 0), _lse (1),
// _lse_probe (2), _ts (3) and _sample (4). The modes share the arithmetic and its order, so a higher
// mode returns the lower modes' results bit for bit.
// logits: [B, V] (bf16 if is_bf16 else f32), row stride ld elements.
// mask: [*, W] uint32 bitmask (bit v%32 of word v/32 = token v allowed), or null;
// mask_rows: optional per-row index into the mask table (rows share the
// precomputed grammar-state masks).
// Every mode: out_idx[b] = argmax over the allowed tokens, or -1 when nothing is
// allowed. A candidate is (order-preserving float key << 32 | ~index) folded
// with max: ties resolve to the lowest index like torch.argmax.
// token_ids (optional, int32 [V]): the columns are a gathered subset of the
// vocabulary (the compact sampling head) and out_idx[b] = token_ids[column];
// the record keeps the column, so with ascending ids a tie still goes to the
// lowest token id.
// MODE >= 1: out_logprob[b] = x[winner] - logsumexp(x over the ALLOWED columns),
// the log-softmax of the selected token after the mask. The winner is the
// maximum, so with m = max and s = sum exp(x - m) the result is -log(s): +0.0f
// when the winner is the only allowed token (s == 1); -inf, never NaN, when
// nothing is allowed or the winner is -inf. Every logit is read once and costs
// one expf (online softmax per thread); all arithmetic is f32.
// MODE 2: out_probe[b] = x[b, probe[b]] - logsumexp(x[b, 0..V-1] over ALL
// columns, the mask ignored): the log-softmax of one fixed column before the
// mask (Whisper's log no_speech_prob at the start-of-transcript row). A probing
// row keeps a second pair (am, as) over all columns in the same pass; the mask
// bits only decide whether a term joins the first pair too. The thread that
// meets column probe[b] keeps that logit in px, all others hold -inf, so a max
// over threads and chunk records carries it to the end unchanged. The result is
// (px - am) - logf(as): -inf for a probed logit or a whole row of -inf. A row
// with probe[b] < 0 or >= V writes +0.0f and skips the second sum; the test is
// per row (blockIdx.y), so wave-uniform.
// A row is split over ARG_CHUNK-token workgroups (a 128k vocabulary -> 16 per
// row, so B=16 rows fill the GPU). Each reduces its tokens to one record (8, 16,
// 32, 48 or 64 bytes by mode) in a fixed order: vector groups in column order, the
// shuffle tree 32 -> 1, the waves in wave order. A row of one chunk finishes
// there (SINGLE): one launch, no workspace. A wider row in MODE 0 folds its
// records with atomicMax into a zeroed word per row, which a small launch
// unpacks; in MODE >= 1 it writes them to workspace[b][chunk] and a finalize
// launch merges them in chunk order: no memset, no atomics, bitwise repeatable.
__device__ __forceinline__ float lse_probe_logprob(bool probing, float px, float am, float as) {
  if (!probing) return 0.f;
  if (am == -INFINITY) return -INFINITY;      // every logit -inf (px too)
  return (px - am) - logf(as);                // px == -inf: -inf; as >= 1
}

// a chunk's record, as it lies in LDS and in the workspace
template <int MODE> struct ArgRec;
template <> struct ArgRec<0> { unsigned long long best; };
template <> struct ArgRec<1> { unsigned long long best; float m, s; };
template <> struct ArgRec<2> {
  unsigned long long best;
  float m, s;       // allowed columns
  float am, as;     // all columns (probing rows)
  float px, pad;    // the probed logit, -inf where this record does not hold it
};
template <> struct ArgRec<3> : ArgRec<2> {
  unsigned long long tbest;   // the best allowed timestamp column
  float tm, tsum;             // allowed timestamp columns (ruled rows)
};
template <> struct ArgRec<4> : ArgRec<3> {
  unsigned long long gbest;   // sampling rows: the best Gumbel key below ts_begin
  unsigned long long gtbest;  // ... and among the allowed timestamp columns
};

// MODE 3: Whisper's timestamp rules as a state machine beside the scan. ctl[b]:
// 0 = rules off (the row is MODE 2's, the state untouched), 1 = the window's
// first sampled token, 2 = continue from state[row_slot[b]]. The state word is
// (last + 1) << 2 | f_last << 1 | f_pen: the last timestamp index sampled in the
// window (-1: none), "the last token was a timestamp", "the one before it was
// (or fewer than two tokens are sampled)". Timestamp token k = column
// ts_begin + k, k < ts_count; columns below eot are text, [eot, ts_begin) are
// specials that only the mask governs.
struct TsArgs {
  const int* ctl;
  int* state;
  const int* row_slot;
  int slots, ts_begin, ts_count, eot, max_initial;
};

// What a row may select: columns [x_from, x_to) where the mask has a bit, and
// the timestamp columns [t_from, t_to) whatever their mask bits. A rule-off row
// is [0, V) and no timestamp class, so it scans exactly as MODE 2 does.
struct TsRow {
  int ctl, slot, last, f_last;
  int x_from, x_to, t_from, t_to;
};

__device__ __forceinline__ TsRow ts_row(const TsArgs& t, int b, int V) {
  TsRow r;
  r.ctl = t.ctl[b];
  r.slot = t.row_slot[b];
  if (r.ctl < 1 || r.ctl > 2 || r.slot < 0 || r.slot >= t.slots) r.ctl = 0;
  r.last = -1, r.f_last = 0;
  r.x_from = 0, r.x_to = V, r.t_from = r.t_to = 0;
  if (r.ctl == 0) return r;
  r.x_to = min(V, t.ts_begin);
  int lo = 0, hi = t.max_initial;
  if (r.ctl == 1) {
    r.x_from = r.x_to;                          // a window opens with a timestamp
  } else {
    const int w = t.state[r.slot];
    r.last = (w >> 2) - 1, r.f_last = (w >> 1) & 1;
    const bool f_pen = w & 1;
    hi = t.ts_count - 1;
    lo = r.last < 0 ? 0 : (r.f_last && !f_pen) ? r.last : r.last + 1;
    if (r.f_last && f_pen) lo = hi + 1;                       // a pair is closed: text next
    if (r.f_last && !f_pen) r.x_from = min(t.eot, r.x_to);    // a lone one: a timestamp or EOT
  }
  lo = min(lo, t.ts_count), hi = min(hi, t.ts_count - 1);
  r.t_from = min(V, t.ts_begin + lo);
  r.t_to = max(r.t_from, min(V, t.ts_begin + hi + 1));
  return r;
}

// MODE 4: MODE 3 plus a per-row temperature temp[b] and a random key rng[b]. A
// row with temp[b] == 0 (or not > 0) is MODE 3's bit for bit. A row with
// temp[b] > 0 draws its token by Gumbel-max in the same pass: every column the
// row may select keeps key = fmaf(T, g, x), g = gumbel_noise(rng[b], column),
// and the largest key per class (gbest / gtbest, ties to the lowest column)
// rides along in the record. The greedy quantities are accumulated as in MODE
// 3 and the mass rule is evaluated on them, at temperature 1, before the draw:
// it fires -> the winner is gtbest, else max(gbest, gtbest), a draw from
// Categorical(logits / T) over what the rules leave. The finishing thread loads
// x[winner] and writes its log-probability at temperature 1 (Whisper's
// sum_logprobs), over the timestamps when the rule fired, else over every
// allowed column. ctl == nullptr: every row rule-off, the layout ignored.
struct SampleArgs : TsArgs {
  const float* temp;
  const uint32_t* rng;
  const void* logits;   // the finishing thread's load of x[winner]
  long long ld;
  int is_bf16;
};

__device__ __forceinline__ TsRow ts_row(const SampleArgs& t, int b, int V) {
  if (t.ctl) return ts_row(static_cast<const TsArgs&>(t), b, V);
  TsRow r;
  r.ctl = r.slot = r.f_last = 0, r.last = -1;
  r.x_from = 0, r.x_to = V, r.t_from = r.t_to = 0;
  return r;
}
__device__ __forceinline__ float sample_temp(const SampleArgs& t, int b) { return t.temp[b]; }
__device__ __forceinline__ uint32_t sample_rng(const SampleArgs& t, int b) { return t.rng[b]; }
__device__ __forceinline__ float sample_x(const SampleArgs& t, int b, int col) {
  const size_t i = (size_t)b * t.ld + col;
  return t.is_bf16 ? bf2f(reinterpret_cast<const bf16_t*>(t.logits)[i])
                   : reinterpret_cast<const float*>(t.logits)[i];
}

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// Counter-based standard Gumbel noise of (row key, column): h = fmix32(rng ^
// fmix32(v + 0x9E3779B9)), u = (2 (h >> 9) + 1) / 2^24, an exact f32 strictly
// inside (0, 1), so g = -log(-log u) is finite (about -2.9 .. 16.7). The
// integer part is ops.reference.gumbel_uniform; the two logf and the key's fmaf
// are spelled out with contraction off so the bits do not depend on the call
// site (loqa_gumbel_noise writes g through this function).
__device__ __forceinline__ float gumbel_noise(uint32_t rng, int v) {
#pragma clang fp contract(off)
  const uint32_t h = fmix32(rng ^ fmix32((uint32_t)v + 0x9E3779B9u));
  const float u = (float)(2u * (h >> 9) + 1u) * (1.0f / 16777216.0f);
  const float w = 0.f - logf(u);
  return 0.f - logf(w);
}
__device__ __forceinline__ void gumbel_one(unsigned long long& best, float x, int v, float T,
                                           uint32_t rng) {
  best = max(best, argpack(fmaf(T, gumbel_noise(rng, v), x), v));
}
template <int N>
__device__ __forceinline__ void gumbel_group(unsigned long long& best, const float (&f)[N],
                                             uint32_t bits, int v0, float T, uint32_t rng) {
#pragma unroll
  for (int j = 0; j < N; ++j)
    if ((bits >> j) & 1u) gumbel_one(best, f[j], v0 + j, T, rng);
}

// bit j: column v0 + j lies in [from, to); N <= 8 columns
__device__ __forceinline__ uint32_t range_bits(int v0, int N, int from, int to) {
  const int a = min(max(from - v0, 0), N), e = min(max(to - v0, 0), N);
  return e > a ? ((1u << e) - 1u) & ~((1u << a) - 1u) : 0u;
}

// Whisper's mass rule in f32, its roundings spelled out: with lA / lT the
// logsumexp of every allowed column / of the allowed timestamps and xt the best
// allowed logit below ts_begin, the timestamps win when their log-probability
// mass lT - lA exceeds the best text token's xt - lA. Nothing allowed below
// ts_begin: they win; no timestamp allowed, or an exact tie: they do not.
__device__ __forceinline__ bool ts_fires(bool any_x, bool any_t, float xt, float mA, float sA,
                                         float tm, float tsum) {
#pragma clang fp contract(off)
  const float lA = mA + logf(sA), lT = tm + logf(tsum);
  return any_t && (!any_x || (lT - lA) > (xt - lA));
}

// The running state of a thread, a wave, a chunk or a row: a record and the
// operations on it. `probing` (MODE 2, per row) is the caller's.
template <int MODE>
struct ArgAcc : ArgRec<MODE> {
  __device__ __forceinline__ ArgAcc() {
    this->best = 0;
    if constexpr (MODE >= 1) this->m = -INFINITY, this->s = 0.f;
    if constexpr (MODE >= 2) this->am = this->px = -INFINITY, this->as = this->pad = 0.f;
    if constexpr (MODE >= 3) this->tbest = 0, this->tm = -INFINITY, this->tsum = 0.f;
    if constexpr (MODE == 4) this->gbest = this->gtbest = 0;
  }
  __device__ __forceinline__ ArgAcc(const ArgRec<MODE>& r) : ArgRec<MODE>(r) {}

  // columns v0 .. v0 + N - 1, allowed where bits has a 1
  template <int N>
  __device__ __forceinline__ void group(const float (&f)[N], uint32_t bits, int v0, bool probing,
                                        int pb) {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if ((bits >> j) & 1u) this->best = max(this->best, argpack(f[j], v0 + j));
    if constexpr (MODE >= 1) lse_add_group<N>(this->m, this->s, f, bits);
    if constexpr (MODE >= 2) if (probing) {
      lse_add_group<N>(this->am, this->as, f, (1u << N) - 1u);
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (v0 + j == pb) this->px = f[j];
    }
  }

  // column v (the tail, or a row whose stride keeps vectors unaligned)
  __device__ __forceinline__ void one(float x, int v, bool ok, bool probing, int pb) {
    if (ok) {
      this->best = max(this->best, argpack(x, v));
      if constexpr (MODE >= 1) lse_add(this->m, this->s, x);
    }
    if constexpr (MODE >= 2) if (probing) {
      lse_add(this->am, this->as, x);
      if (v == pb) this->px = x;
    }
  }

  // MODE 3, a ruled row: the allowed timestamp columns of a group / one column
  template <int N>
  __device__ __forceinline__ void tgroup(const float (&f)[N], uint32_t bits, int v0) {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if ((bits >> j) & 1u) this->tbest = max(this->tbest, argpack(f[j], v0 + j));
    lse_add_group<N>(this->tm, this->tsum, f, bits);
  }
  __device__ __forceinline__ void tone(float x, int v) {
    this->tbest = max(this->tbest, argpack(x, v));
    lse_add(this->tm, this->tsum, x);
  }

  // Folds in the record o. FMA: lse_merge's form for the masked pair (the
  // all-column pair has one form). get() fetches each field where it is merged:
  // the field itself, or in the shuffle tree the same field of another lane, so
  // that a probing row's extra shuffles and sums stay one block. `ruled` (MODE
  // 3, per row): the timestamp class is merged too, in the masked pair's form.
  // `sampling` (MODE 4, per row): the two Gumbel bests too.
  template <bool FMA, class Get>
  __device__ __forceinline__ void merge(const ArgRec<MODE>& o, bool probing, bool ruled,
                                        bool sampling, Get get) {
    this->best = max(this->best, get(o.best));
    if constexpr (MODE >= 1) lse_merge<FMA>(this->m, this->s, get(o.m), get(o.s));
    if constexpr (MODE >= 2) if (probing) {
      lse_merge<false>(this->am, this->as, get(o.am), get(o.as));   // <false> at every site
      this->px = fmaxf(this->px, get(o.px));
    }
    if constexpr (MODE >= 3) if (ruled) {
      this->tbest = max(this->tbest, get(o.tbest));
      lse_merge<FMA>(this->tm, this->tsum, get(o.tm), get(o.tsum));
    }
    if constexpr (MODE == 4) if (sampling) {
      this->gbest = max(this->gbest, get(o.gbest));
      if (ruled) this->gtbest = max(this->gtbest, get(o.gtbest));
    }
  }
  template <bool FMA>
  __device__ __forceinline__ void merge(const ArgRec<MODE>& o, bool probing, bool ruled,
                                        bool sampling) {
    merge<FMA>(o, probing, ruled, sampling, [](auto x) { return x; });
  }

  __device__ __forceinline__ void finish(int b, bool probing, const int* __restrict__ token_ids,
                                         int* __restrict__ out_idx, float* __restrict__ out_logprob,
                                         float* __restrict__ out_probe) const {
    out_idx[b] = argunpack(this->best, token_ids);
    if constexpr (MODE >= 1) out_logprob[b] = lse_logprob(this->best, this->m, this->s);
    if constexpr (MODE >= 2)
      out_probe[b] = lse_probe_logprob(probing, this->px, this->am, this->as);
  }

  // MODE 3: a rule-off row finishes as MODE 2 does. A ruled row decides between
  // its two classes by the mass rule; the winner's log-probability is over the
  // timestamps alone when they win (Whisper masks the text then), else over
  // every allowed column. It then writes the row's next state word.
  __device__ __forceinline__ void finish(int b, bool probing, const TsRow& r, const TsArgs& t,
                                         int* __restrict__ out_idx, float* __restrict__ out_logprob,
                                         float* __restrict__ out_probe) const {
    if (r.ctl == 0) {
      finish(b, probing, nullptr, out_idx, out_logprob, out_probe);
      return;
    }
    out_probe[b] = lse_probe_logprob(probing, this->px, this->am, this->as);
    float mA = this->m, sA = this->s;
    lse_merge<false>(mA, sA, this->tm, this->tsum);
    const bool fire = ts_fires(this->best != 0, this->tbest != 0, this->m, mA, sA, this->tm,
                               this->tsum);
    const int col = argunpack(fire ? this->tbest : this->best, nullptr);
    out_idx[b] = col;
    if (col < 0) {                     // nothing allowed: the state stays
      out_logprob[b] = -INFINITY;
      return;
    }
    if (fire)
      out_logprob[b] = lse_logprob(this->tbest, this->tm, this->tsum);
    else                               // x[winner] = m, the maximum below ts_begin
      out_logprob[b] = this->m != -INFINITY ? (this->m - mA) - logf(sA) : -INFINITY;
    const int f_last = col >= t.ts_begin;
    const int last = f_last ? col - t.ts_begin : r.last;
    t.state[r.slot] = ((last + 1) << 2) | (f_last << 1) | (r.ctl == 1 ? 1 : r.f_last);
  }

  // MODE 4: a row with temp[b] == 0 finishes as MODE 3 does. A sampling row's
  // winner is a Gumbel best (see SampleArgs); its log-probability is taken at
  // temperature 1 from the greedy sums, x[winner] loaded here.
  __device__ __forceinline__ void finish(int b, bool probing, const TsRow& r, const SampleArgs& t,
                                         int* __restrict__ out_idx, float* __restrict__ out_logprob,
                                         float* __restrict__ out_probe) const {
    if (!(sample_temp(t, b) > 0.f)) {
      finish(b, probing, r, static_cast<const TsArgs&>(t), out_idx, out_logprob, out_probe);
      return;
    }
    out_probe[b] = lse_probe_logprob(probing, this->px, this->am, this->as);
    float mA = this->m, sA = this->s;
    bool fire = false;
    if (r.ctl != 0) {
      lse_merge<false>(mA, sA, this->tm, this->tsum);
      fire = ts_fires(this->best != 0, this->tbest != 0, this->m, mA, sA, this->tm, this->tsum);
    }
    const int col = argunpack(fire ? this->gtbest : max(this->gbest, this->gtbest), nullptr);
    out_idx[b] = col;
    if (col < 0) {                     // nothing allowed: the state stays
      out_logprob[b] = -INFINITY;
      return;
    }
    const float xw = sample_x(t, b, col);
    const float lm = fire ? this->tm : mA, ls = fire ? this->tsum : sA;
    out_logprob[b] = xw != -INFINITY ? (xw - lm) - logf(ls) : -INFINITY;
    if (r.ctl == 0) return;
    const int f_last = col >= t.ts_begin;
    const int last = f_last ? col - t.ts_begin : r.last;
    t.state[r.slot] = ((last + 1) << 2) | (f_last << 1) | (r.ctl == 1 ? 1 : r.f_last);
  }
};

// SINGLE: gridDim.x == 1 (V <= ARG_CHUNK); the workgroup writes the row's
// results. Otherwise `part` is the zeroed packed word per row (MODE 0) or the
// [B, gridDim.x] chunk records.
// TS: empty below MODE 3 (the kernel's arguments are the lower modes' own), else TsArgs
// (MODE 4: SampleArgs).
template <bool BF16, bool SINGLE, int MODE, class... TS>
__global__ __launch_bounds__(ARG_THREADS) void masked_argmax_kernel(
    const void* __restrict__ logits, long long ld, int V, const uint32_t* __restrict__ mask,
    const int* __restrict__ mask_rows, int W, const int* __restrict__ probe,
    ArgRec<MODE>* __restrict__ part, const int* __restrict__ token_ids, int* __restrict__ out_idx,
    float* __restrict__ out_logprob, float* __restrict__ out_probe, TS... ts) {
  static_assert(sizeof...(TS) == (MODE >= 3 ? 1 : 0), "MODE 3 / 4 take one TsArgs / SampleArgs");
  using T = typename std::conditional<BF16, bf16_t, float>::type;
  constexpr int N = BF16 ? 8 : 4;           // one 16-byte load
  __shared__ ArgRec<MODE> sred[ARG_THREADS / 64];
  const int b = blockIdx.y;
  const int v_begin = blockIdx.x * ARG_CHUNK;
  const int v_end = min(V, v_begin + ARG_CHUNK);
  const uint32_t* m = nullptr;
  if (mask) m = mask + (size_t)(mask_rows ? mask_rows[b] : b) * W;
  int pb = -1;
  if constexpr (MODE >= 2) pb = probe[b];
  const bool probing = pb >= 0 && pb < V;   // false below MODE 2
  TsRow tr;
  if constexpr (MODE >= 3) tr = ts_row(ts..., b, V);
  bool ruled = false;                       // per row too; false below MODE 3
  if constexpr (MODE >= 3) ruled = tr.ctl != 0;
  float temp = 0.f;                         // per row too; MODE 4 alone samples
  uint32_t rng = 0;
  if constexpr (MODE == 4) temp = sample_temp(ts..., b), rng = sample_rng(ts..., b);
  const bool sampling = temp > 0.f;
  const T* row = reinterpret_cast<const T*>(logits) + (size_t)b * ld;
  ArgAcc<MODE> a;
  for (int v0 = v_begin + threadIdx.x * N; v0 < v_end; v0 += ARG_THREADS * N) {
    if (v0 + N <= v_end && (ld % N == 0)) {
      float f[N];
      arg_load_group(row + v0, f);
      const uint32_t all = (1u << N) - 1u;
      uint32_t bits = m ? (m[v0 >> 5] >> (v0 & 31)) & all : all;
      if constexpr (MODE >= 3) if (ruled) bits &= range_bits(v0, N, tr.x_from, tr.x_to);
      a.template group<N>(f, bits, v0, probing, pb);
      if constexpr (MODE == 4) if (sampling) gumbel_group<N>(a.gbest, f, bits, v0, temp, rng);
      if constexpr (MODE >= 3) if (ruled) {
        const uint32_t tbits = range_bits(v0, N, tr.t_from, tr.t_to);
        if (tbits) {
          a.template tgroup<N>(f, tbits, v0);
          if constexpr (MODE == 4) if (sampling) gumbel_group<N>(a.gtbest, f, tbits, v0, temp, rng);
        }
      }
    } else {
      for (int v = v0; v < min(v_end, v0 + N); ++v) {
        bool ok = !m || ((m[v >> 5] >> (v & 31)) & 1u);
        bool tok = false;
        if constexpr (MODE >= 3) if (ruled) {
          ok = ok && v >= tr.x_from && v < tr.x_to;
          tok = v >= tr.t_from && v < tr.t_to;
        }
        if (ok || probing || tok) {
          const float x = arg_load(row + v);
          a.one(x, v, ok, probing, pb);
          if constexpr (MODE >= 3) if (tok) a.tone(x, v);
          if constexpr (MODE == 4) if (sampling) {
            if (ok) gumbel_one(a.gbest, x, v, temp, rng);
            if (tok) gumbel_one(a.gtbest, x, v, temp, rng);
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)   // shuffle tree: <true>, the masked pair's 2nd product fused
    a.template merge<true>(a, probing, ruled, sampling,
                           [o](auto x) { return __shfl_xor(x, o, 64); });
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    // LDS fold: <true>, as the shuffle tree
    for (int i = 1; i < ARG_THREADS / 64; ++i)
      a.template merge<true>(sred[i], probing, ruled, sampling);
    if constexpr (SINGLE && MODE >= 3)   // every thread read the old state before the barrier
      a.finish(b, probing, tr, ts..., out_idx, out_logprob, out_probe);
    else if (SINGLE)
      a.finish(b, probing, token_ids, out_idx, out_logprob, out_probe);
    else if constexpr (MODE == 0) {
      if (a.best) atomicMax(&part[b].best, a.best);
    } else
      part[(size_t)b * gridDim.x + blockIdx.x] = a;
  }
}

// one thread per row: the row's chunk records, merged in chunk order (MODE 0:
// the one packed word that the atomics left)
template <int MODE, class... TS>
__global__ void argmax_finalize_kernel(
    const ArgRec<MODE>* __restrict__ part, int B, int chunks, int V, const int* __restrict__ probe,
    const int* __restrict__ token_ids, int* __restrict__ out_idx, float* __restrict__ out_logprob,
    float* __restrict__ out_probe, TS... ts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int pb = -1;
  if constexpr (MODE >= 2) pb = probe[b];
  const bool probing = pb >= 0 && pb < V;
  TsRow tr;
  if constexpr (MODE >= 3) tr = ts_row(ts..., b, V);
  bool ruled = false;
  if constexpr (MODE >= 3) ruled = tr.ctl != 0;
  bool sampling = false;
  if constexpr (MODE == 4) sampling = sample_temp(ts..., b) > 0.f;
  const ArgRec<MODE>* p = part + (size_t)b * chunks;
  ArgAcc<MODE> a(p[0]);
  for (int c = 1; c < chunks; ++c)   // chunks: <false>
    a.template merge<false>(p[c], probing, ruled, sampling);
  // MODE >= 3: the scan launch has finished, so no workgroup still reads the old state
  if constexpr (MODE >= 3)
    a.finish(b, probing, tr, ts..., out_idx, out_logprob, out_probe);
  else
    a.finish(b, probing, token_ids, out_idx, out_logprob, out_probe);
}

// The argument checks and the SINGLE / chunked dispatch of the five entry
// points; probe, out_logprob and out_probe are null below their mode.
// workspace (device, 8-byte aligned, only touched when V > ARG_CHUNK):
// MODE 0: >= B * 8 bytes, zeroed here; MODE 1 / 2: >= B * ceil(V / ARG_CHUNK)
// * 16 / 32 bytes (MODE 3: 48, MODE 4: 64), no initialisation needed.
template <int MODE, class... TS>
static int masked_argmax(const void* logits, int is_bf16, long long ld, int B, int V,
                         const uint32_t* mask, const int* mask_rows, int W, const int* probe,
                         int* out_idx, float* out_logprob, float* out_probe, void* workspace,
                         const int* token_ids, hipStream_t s, TS... ts) {
  if (B <= 0) return 0;
  if (V <= 0 || (mask && W * 32 < V) || !out_idx) return (int)hipErrorInvalidValue;
  if (MODE >= 1 && (ld < V || !out_logprob)) return (int)hipErrorInvalidValue;
  if (MODE >= 2 && (!probe || !out_probe)) return (int)hipErrorInvalidValue;
  const int chunks = (V + ARG_CHUNK - 1) / ARG_CHUNK;
  const bool single = chunks == 1;
  ArgRec<MODE>* part = (ArgRec<MODE>*)workspace;
  if (!single && !workspace) return (int)hipErrorInvalidValue;
  if (MODE == 0 && !single) {
    hipError_t e = hipMemsetAsync(part, 0, sizeof(ArgRec<0>) * B, s);
    if (e != hipSuccess) return (int)e;
  }
  auto kernel = is_bf16 ? (single ? masked_argmax_kernel<true, true, MODE, TS...>
                                  : masked_argmax_kernel<true, false, MODE, TS...>)
                        : (single ? masked_argmax_kernel<false, true, MODE, TS...>
                                  : masked_argmax_kernel<false, false, MODE, TS...>);
  hipLaunchKernelGGL(kernel, dim3(chunks, B), dim3(ARG_THREADS), 0, s, logits, ld, V, mask,
                     mask_rows, W, probe, single ? nullptr : part, token_ids, out_idx, out_logprob,
                     out_probe, ts...);
  hipError_t e = hipGetLastError();
  if (single || e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((argmax_finalize_kernel<MODE, TS...>), dim3((B + 63) / 64), dim3(64), 0, s,
                     (const ArgRec<MODE>*)part, B, MODE == 0 ? 1 : chunks, V, probe, token_ids,
                     out_idx, out_logprob, out_probe, ts...);
  return (int)hipGetLastError();
}

// token_ids: null, or int32 [V]; probe: int32 [B] (device)
extern "C" int loqa_masked_argmax(const void* logits, int is_bf16, long long ld, int B, int V,
                                  const uint32_t* mask, const int* mask_rows, int W, int* out_idx,
                                  void* workspace, const int* token_ids, hipStream_t s) {
  return masked_argmax<0>(logits, is_bf16, ld, B, V, mask, mask_rows, W, nullptr, out_idx, nullptr,
                          nullptr, workspace, token_ids, s);
}
extern "C" int loqa_masked_argmax_lse(const void* logits, int is_bf16, long long ld, int B, int V,
                                      const uint32_t* mask, const int* mask_rows, int W,
                                      int* out_idx, float* out_logprob, void* workspace,
                                      const int* token_ids, hipStream_t s) {
  return masked_argmax<1>(logits, is_bf16, ld, B, V, mask, mask_rows, W, nullptr, out_idx,
                          out_logprob, nullptr, workspace, token_ids, s);
}
extern "C" int loqa_masked_argmax_lse_probe(const void* logits, int is_bf16, long long ld, int B,
                                            int V, const uint32_t* mask, const int* mask_rows,
                                            int W, const int* probe, int* out_idx,
                                            float* out_logprob, float* out_probe, void* workspace,
                                            const int* token_ids, hipStream_t s) {
  return masked_argmax<2>(logits, is_bf16, ld, B, V, mask, mask_rows, W, probe, out_idx,
                          out_logprob, out_probe, workspace, token_ids, s);
}

// MODE 3 (see TsArgs): ts_ctl, row_slot: int32 [B]; ts_state: int32 [slots],
// read and written in place by the ruled rows, whose slots must differ. The
// columns are the vocabulary itself (no token_ids).
extern "C" int loqa_masked_argmax_ts(const void* logits, int is_bf16, long long ld, int B, int V,
                                     const uint32_t* mask, const int* mask_rows, int W,
                                     const int* probe, const int* ts_ctl, int* ts_state,
                                     const int* row_slot, int slots, int ts_begin, int ts_count,
                                     int eot, int max_initial, int* out_idx, float* out_logprob,
                                     float* out_probe, void* workspace, hipStream_t s) {
  if (B > 0 && (!ts_ctl || !ts_state || !row_slot || slots <= 0 || ts_count <= 0 || eot < 0 ||
                eot > ts_begin || ts_begin > V - ts_count || max_initial < 0))
    return (int)hipErrorInvalidValue;
  const TsArgs t{ts_ctl, ts_state, row_slot, slots, ts_begin, ts_count, eot,
                 min(max_initial, ts_count - 1)};
  return masked_argmax<3>(logits, is_bf16, ld, B, V, mask, mask_rows, W, probe, out_idx,
                          out_logprob, out_probe, workspace, nullptr, s, t);
}

// MODE 4 (see SampleArgs): loqa_masked_argmax_ts plus temp: f32 [B] and rng:
// uint32 [B]. ts_ctl == nullptr: every row rule-off (ts_state, row_slot and the
// layout arguments are ignored), so an engine without timestamps can sample.
// workspace: 64 bytes per (row, chunk).
extern "C" int loqa_masked_argmax_sample(const void* logits, int is_bf16, long long ld, int B,
                                         int V, const uint32_t* mask, const int* mask_rows, int W,
                                         const int* probe, const int* ts_ctl, int* ts_state,
                                         const int* row_slot, int slots, int ts_begin,
                                         int ts_count, int eot, int max_initial, const float* temp,
                                         const unsigned* rng, int* out_idx, float* out_logprob,
                                         float* out_probe, void* workspace, hipStream_t s) {
  if (B > 0 && (!temp || !rng)) return (int)hipErrorInvalidValue;
  if (B > 0 && ts_ctl &&
      (!ts_state || !row_slot || slots <= 0 || ts_count <= 0 || eot < 0 || eot > ts_begin ||
       ts_begin > V - ts_count || max_initial < 0))
    return (int)hipErrorInvalidValue;
  SampleArgs t;
  if (ts_ctl) {
    static_cast<TsArgs&>(t) = TsArgs{ts_ctl, ts_state, row_slot, slots, ts_begin, ts_count, eot,
                                     min(max_initial, ts_count - 1)};
  } else {
    static_cast<TsArgs&>(t) = TsArgs{nullptr, nullptr, nullptr, 0, V, 0, V, 0};
  }
  t.temp = temp, t.rng = rng, t.logits = logits, t.ld = ld, t.is_bf16 = is_bf16;
  return masked_argmax<4>(logits, is_bf16, ld, B, V, mask, mask_rows, W, probe, out_idx,
                          out_logprob, out_probe, workspace, nullptr, s, t);
}

// g[b, v] = gumbel_noise(rng[b], v): the noise of loqa_masked_argmax_sample's draw,
// through the same device function (out: f32 [B, V], contiguous)
__global__ __launch_bounds__(256) void gumbel_noise_kernel(const uint32_t* __restrict__ rng, int V,
                                                           float* __restrict__ out) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < V) out[(size_t)blockIdx.y * V + v] = gumbel_noise(rng[blockIdx.y], v);
}

extern "C" int loqa_gumbel_noise(const unsigned* rng, int B, int V, float* out, hipStream_t s) {
  if (B <= 0 || V <= 0) return B < 0 || V < 0 ? (int)hipErrorInvalidValue : 0;
  if (!rng || !out || B > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(gumbel_noise_kernel, dim3((V + 255) / 256, B), dim3(256), 0, s,
                     (const uint32_t*)rng, V, out);
  return (int)hipGetLastError();
}

// ------------------------------------------------- pipelined decode: step I/O
// A decode step graph exchanges its host data without copy-engine operations
// between graphs (each H2D / D2H copy on the decode stream cost a copy-engine
// hand-off of tens of microseconds between two back-to-back step graphs).
// The host stages a step's metadata in pinned memory; the graph's first node
// reads it zero-copy into the graph's device buffers, and its last node writes
// the sampled tokens zero-copy into a pinned result ring. *ctr counts the step
// graphs launched so far (advanced by the last node), so the staging slot
// (ctr % 2) and result slot (ctr % nres) follow the host's launch order.
__global__ __launch_bounds__(256) void step_fetch_kernel(int* __restrict__ d32,
                                                        const int* __restrict__ h32, int n32,
                                                        int stride32, long long* __restrict__ d64,
                                                        const long long* __restrict__ h64, int n64,
                                                        int stride64, const int* __restrict__ ctr,
                                                        int T, int src_off,
                                                        const int* __restrict__ last_tok) {
  const int slot = ctr[0] & 1;
  const int* src = h32 + (size_t)slot * stride32;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n32; i += gridDim.x * 256) {
    int v = src[i];
    if (i < T) {   // tokens: a staged src slot >= 0 takes that sequence's last sampled token
      const int sl = src[src_off + i];
      // a failed step's sentinel (-1 nothing allowed, -2 collective error)
      // must never become an embedding row index: the host fails those
      // sequences when it reads the step, this one only has to stay in bounds
      if (sl >= 0) v = max(last_tok[sl], 0);
    }
    d32[i] = v;
  }
  const long long* src64 = h64 + (size_t)slot * stride64;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n64; i += gridDim.x * 256) d64[i] = src64[i];
}

// The step's tokens, and NLP (0, 1 or 2) f32 values per sequence (the token
// log-probabilities; the probed log-probability): slot (ctr % nres) of a second
// pinned ring (f32, row stride lp_stride) is a row of planes, lp[i] at [i] and
// lp2[i] at [plane + i]. Every store precedes the fence and the counter store
// that order the tokens.
template <int NLP>
__global__ __launch_bounds__(256) void step_publish_kernel(
    const int* __restrict__ out, const float* __restrict__ lp, const float* __restrict__ lp2, int n,
    int* __restrict__ res, int stride, float* __restrict__ res_lp, int lp_stride, int plane,
    int nres, int* __restrict__ ctr, const int* __restrict__ row_slot, int* __restrict__ last_tok) {
  const int c = ctr[0];
  int* dst = res + (size_t)(c % nres) * stride;
  float* dst_lp = NLP ? res_lp + (size_t)(c % nres) * lp_stride : nullptr;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int v = out[i];
    dst[i] = v;
    if (NLP >= 1) dst_lp[i] = lp[i];
    if (NLP == 2) dst_lp[plane + i] = lp2[i];
    last_tok[row_slot[i]] = v;     // padding rows write the trash slot
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();
    // wrap at 2 * nres (a common multiple of the 2 staging slots and the nres
    // result slots; the host's step number wraps the same way), so the counter
    // never overflows on a long-running hub
    __hip_atomic_store(ctr, (c + 1) % (2 * nres), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// T: token rows at the head of the staged int32 block; src_off: offset of the
// per-token source-slot array in it (see LLMEngine._decode_graph).
extern "C" int loqa_step_fetch(void* d32, const void* h32, int n32, int stride32, void* d64,
                               const void* h64, int n64, int stride64, const int* ctr, int T,
                               int src_off, const int* last_tok, hipStream_t s) {
  if (n32 < 0 || n32 > stride32 || n64 < 0 || n64 > stride64 || src_off + T > n32)
    return (int)hipErrorInvalidValue;
  int blocks = (n32 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 16 ? 16 : blocks);
  hipLaunchKernelGGL(step_fetch_kernel, dim3(blocks), dim3(256), 0, s, (int*)d32, (const int*)h32, n32,
                     stride32, (long long*)d64, (const long long*)h64, n64, stride64, ctr, T, src_off,
                     last_tok);
  return (int)hipGetLastError();
}

// res_lp rows: lp_stride floats, lp at [0, n), lp2 at [plane, plane + n)
template <int NLP>
static int step_publish(const int* out, const float* lp, const float* lp2, int n, void* res,
                        int stride, void* res_lp, int lp_stride, int plane, int nres, int* ctr,
                        const int* row_slot, int* last_tok, hipStream_t s) {
  if (n < 0 || n > stride || nres < 1) return (int)hipErrorInvalidValue;
  if (NLP >= 1 && (!lp || !res_lp)) return (int)hipErrorInvalidValue;
  if (NLP == 1 && n > lp_stride) return (int)hipErrorInvalidValue;
  if (NLP == 2 && (!lp2 || n > plane || plane > lp_stride - n)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(step_publish_kernel<NLP>, dim3(1), dim3(256), 0, s, out, lp, lp2, n, (int*)res,
                     stride, (float*)res_lp, lp_stride, plane, nres, ctr, row_slot, last_tok);
  return (int)hipGetLastError();
}

extern "C" int loqa_step_publish(const int* out, int n, void* res, int stride, int nres, int* ctr,
                                 const int* row_slot, int* last_tok, hipStream_t s) {
  return step_publish<0>(out, nullptr, nullptr, n, res, stride, nullptr, 0, 0, nres, ctr, row_slot,
                         last_tok, s);
}
extern "C" int loqa_step_publish_lp(const int* out, const float* lp, int n, void* res, int stride,
                                    void* res_lp, int lp_stride, int nres, int* ctr,
                                    const int* row_slot, int* last_tok, hipStream_t s) {
  return step_publish<1>(out, lp, nullptr, n, res, stride, res_lp, lp_stride, 0, nres, ctr,
                         row_slot, last_tok, s);
}
extern "C" int loqa_step_publish_lp2(const int* out, const float* lp, const float* lp2, int n,
                                     void* res, int stride, void* res_lp, int lp_stride, int plane,
                                     int nres, int* ctr, const int* row_slot, int* last_tok,
                                     hipStream_t s) {
  return step_publish<2>(out, lp, lp2, n, res, stride, res_lp, lp_stride, plane, nres, ctr,
                         row_slot, last_tok, s);
}

// ---------------------------------------------------------------------------
// Counter-based random init (seeded random-init weights): element
// (r, c) of a [rows, cols] block at (row0, col0) of a conceptual [*, ld] tensor
// gets scale * (u0 + u1 + u2 + u3 - 2) with u_k = fmix32(4 * idx + k + s) / 2^32
// (Irwin-Hall(4): mean 0, variance 1/3 - the caller folds sqrt(3) into scale),
// idx = (row0 + r) * ld + col0 + c. Any shard of a tensor is generated on its
// own, with exactly the values of the unsharded tensor (tensor-parallel ranks
// build their slices without materialising the full model). Integer hashing and
// exact f32 sums: bitwise equal to the CPU path (ops.reference.init_uniform4).
// fmix32 (murmur3's finalizer) is defined above, beside the sampling noise.
__global__ __launch_bounds__(256) void init_uniform4_kernel(bf16_t* __restrict__ out, long long rows,
                                                            int cols, long long ld, long long row0,
                                                            long long col0, uint32_t s, float scale) {
  const long long n = rows * cols;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long r = i / cols, c = i - r * cols;
    const uint32_t idx = (uint32_t)((row0 + r) * ld + col0 + c);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += (float)(fmix32(idx * 4u + (uint32_t)k + s) >> 8) * (1.0f / 16777216.0f);
    out[i] = f2bf((acc - 2.0f) * scale);
  }
}

extern "C" int loqa_init_uniform4(void* out, long long rows, int cols, long long ld, long long row0,
                                  long long col0, unsigned s, float scale, hipStream_t st) {
  if (rows < 0 || cols < 0 || col0 + cols > ld) return (int)hipErrorInvalidValue;
  const long long n = rows * cols;
  if (n == 0) return 0;
  long long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(init_uniform4_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (bf16_t*)out, rows,
                     cols, ld, row0, col0, (uint32_t)s, scale);
  return (int)hipGetLastError();
}
