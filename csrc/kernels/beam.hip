// Beam search on the device (Whisper's BeamSearchDecoder, patience 1):
//   loqa_beam_topk       per logits row: the KB best allowed non-EOT columns with
//                        their log-softmax, and EOT's
//   loqa_beam_merge      per group of beams: the B best (beam, column) pairs by
//                        cumulative score, and which EOT extensions finish
//   loqa_kv_copy_blocks  paged self-attention KV blocks from one sequence's
//                        blocks to another's, every layer, K and V
// One order ranks candidates everywhere: higher score first, then the lower
// source beam, then the lower column.
#include "argscan.h"
#include <type_traits>

#define BEAM_MAX 8

// ------------------------------------------------------------- loqa_beam_topk
// The row scan of the masked argmax (elementwise.hip, MODE 1) with a top-8 list
// in place of the single best: the same ARG_CHUNK chunks, the same thread /
// shuffle-tree / wave / chunk order for (m, s) = (max, sum exp(x - m)) over the
// allowed columns, EOT included, so cand_lp[r, 0] = (m - m) - logf(s) carries
// masked_argmax_lse's bits whenever EOT is not the row's winner.
// A candidate is argpack's (order-preserving float key << 32 | ~column): unique
// per column, its maximum is the largest logit at the lowest column, and the
// logit comes back out of the key. Each thread keeps its 8 best sorted in
// registers; lists merge by insertion (the top 8 of a union of distinct keys
// does not depend on the order of insertion). EOT never enters a list: the
// thread that meets it keeps its logit in ex (-inf elsewhere, and when the
// mask forbids it).
struct BeamRec {
  unsigned long long k[BEAM_MAX];   // sorted, best first; 0 = empty
  float m, s;                       // allowed columns, EOT included
  float ex, pad;                    // EOT's logit where this record holds it
};

struct BeamAcc : BeamRec {
  __device__ __forceinline__ BeamAcc() {
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) this->k[j] = 0;
    this->m = this->ex = -INFINITY;
    this->s = this->pad = 0.f;
  }
  __device__ __forceinline__ BeamAcc(const BeamRec& r) : BeamRec(r) {}

  __device__ __forceinline__ void insert(unsigned long long p) {
    if (p <= this->k[BEAM_MAX - 1]) return;
    this->k[BEAM_MAX - 1] = p;
#pragma unroll
    for (int j = BEAM_MAX - 1; j > 0; --j) {
      const unsigned long long hi = max(this->k[j - 1], this->k[j]);
      const unsigned long long lo = min(this->k[j - 1], this->k[j]);
      this->k[j - 1] = hi;
      this->k[j] = lo;
    }
  }

  template <int N>
  __device__ __forceinline__ void group(const float (&f)[N], uint32_t bits, int v0, int eot) {
    lse_add_group<N>(this->m, this->s, f, bits);
#pragma unroll
    for (int j = 0; j < N; ++j)
      if ((bits >> j) & 1u) {
        if (v0 + j == eot) this->ex = f[j];
        else insert(argpack(f[j], v0 + j));
      }
  }

  __device__ __forceinline__ void one(float x, int v, int eot) {
    lse_add(this->m, this->s, x);
    if (v == eot) this->ex = x;
    else insert(argpack(x, v));
  }

  // get(): the field itself, or in the shuffle tree the same field of another lane
  template <bool FMA, class Get>
  __device__ __forceinline__ void merge(const BeamRec& o, Get get) {
    unsigned long long t[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) t[j] = get(o.k[j]);
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) insert(t[j]);
    lse_merge<FMA>(this->m, this->s, get(o.m), get(o.s));
    this->ex = fmaxf(this->ex, get(o.ex));
  }
  template <bool FMA>
  __device__ __forceinline__ void merge(const BeamRec& o) {
    merge<FMA>(o, [](auto x) { return x; });
  }

  __device__ __forceinline__ float logprob(float x) const {
    return x != -INFINITY ? (x - this->m) - logf(this->s) : -INFINITY;
  }

  __device__ __forceinline__ void finish(int r, int KB, int* __restrict__ cand_id,
                                         float* __restrict__ cand_lp,
                                         float* __restrict__ eot_lp) const {
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) {
      if (j >= KB) break;
      const unsigned long long p = this->k[j];
      const uint32_t key = (uint32_t)(p >> 32);
      const float x = __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
      cand_id[(size_t)r * KB + j] = argunpack(p, nullptr);
      cand_lp[(size_t)r * KB + j] = p ? logprob(x) : -INFINITY;
    }
    eot_lp[r] = logprob(this->ex);
  }
};

template <bool BF16, bool SINGLE>
__global__ __launch_bounds__(ARG_THREADS) void beam_topk_kernel(
    const void* __restrict__ logits, long long ld, int V, const uint32_t* __restrict__ mask,
    const int* __restrict__ mask_rows, int W, int eot, int KB, BeamRec* __restrict__ part,
    int* __restrict__ cand_id, float* __restrict__ cand_lp, float* __restrict__ eot_lp) {
  using T = typename std::conditional<BF16, bf16_t, float>::type;
  constexpr int N = BF16 ? 8 : 4;           // one 16-byte load
  __shared__ BeamRec sred[ARG_THREADS / 64];
  const int b = blockIdx.y;
  const int v_begin = blockIdx.x * ARG_CHUNK;
  const int v_end = min(V, v_begin + ARG_CHUNK);
  const uint32_t* m = nullptr;
  if (mask) m = mask + (size_t)(mask_rows ? mask_rows[b] : b) * W;
  const T* row = reinterpret_cast<const T*>(logits) + (size_t)b * ld;
  BeamAcc a;
  for (int v0 = v_begin + threadIdx.x * N; v0 < v_end; v0 += ARG_THREADS * N) {
    if (v0 + N <= v_end && (ld % N == 0)) {
      float f[N];
      arg_load_group(row + v0, f);
      const uint32_t all = (1u << N) - 1u;
      const uint32_t bits = m ? (m[v0 >> 5] >> (v0 & 31)) & all : all;
      a.template group<N>(f, bits, v0, eot);
    } else {
      for (int v = v0; v < min(v_end, v0 + N); ++v)
        if (!m || ((m[v >> 5] >> (v & 31)) & 1u)) a.one(arg_load(row + v), v, eot);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)   // as the argmax scan: <true> inside a workgroup
    a.template merge<true>(a, [o](auto x) { return __shfl_xor(x, o, 64); });
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < ARG_THREADS / 64; ++i) a.template merge<true>(sred[i]);
    if (SINGLE)
      a.finish(b, KB, cand_id, cand_lp, eot_lp);
    else
      part[(size_t)b * gridDim.x + blockIdx.x] = a;
  }
}

// one thread per row: the row's chunk records, merged in chunk order
__global__ void beam_topk_finalize_kernel(const BeamRec* __restrict__ part, int R, int chunks,
                                          int KB, int* __restrict__ cand_id,
                                          float* __restrict__ cand_lp,
                                          float* __restrict__ eot_lp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= R) return;
  const BeamRec* p = part + (size_t)b * chunks;
  BeamAcc a(p[0]);
  for (int c = 1; c < chunks; ++c) a.template merge<false>(p[c]);   // chunks: <false>
  a.finish(b, KB, cand_id, cand_lp, eot_lp);
}

// logits: [R, V] bf16 / f32, row stride ld; mask: [*, W] packed or null, mask_rows:
// int32 [R] or null; eot < 0 or >= V: no EOT column. cand_id / cand_lp: [R, KB],
// eot_lp: [R]. workspace: R * ceil(V / ARG_CHUNK) * sizeof(BeamRec) (80) bytes,
// 8-byte aligned, touched only when V > ARG_CHUNK, written before it is read.
extern "C" int loqa_beam_topk(const void* logits, int is_bf16, long long ld, int R, int V,
                              const uint32_t* mask, const int* mask_rows, int W, int eot, int KB,
                              int* cand_id, float* cand_lp, float* eot_lp, void* workspace,
                              hipStream_t s) {
  if (R <= 0) return 0;
  if (V <= 0 || ld < V || (mask && W * 32 < V) || KB < 1 || KB > BEAM_MAX || !cand_id ||
      !cand_lp || !eot_lp)
    return (int)hipErrorInvalidValue;
  const int chunks = (V + ARG_CHUNK - 1) / ARG_CHUNK;
  const bool single = chunks == 1;
  BeamRec* part = (BeamRec*)workspace;
  if (!single && !workspace) return (int)hipErrorInvalidValue;
  auto kernel = is_bf16 ? (single ? beam_topk_kernel<true, true> : beam_topk_kernel<true, false>)
                        : (single ? beam_topk_kernel<false, true> : beam_topk_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(chunks, R), dim3(ARG_THREADS), 0, s, logits, ld, V, mask,
                     mask_rows, W, eot, KB, single ? nullptr : part, cand_id, cand_lp, eot_lp);
  hipError_t e = hipGetLastError();
  if (single || e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(beam_topk_finalize_kernel, dim3((R + 63) / 64), dim3(64), 0, s,
                     (const BeamRec*)part, R, chunks, KB, cand_id, cand_lp, eot_lp);
  return (int)hipGetLastError();
}

extern "C" int loqa_beam_topk_record_size() { return (int)sizeof(BeamRec); }

// ------------------------------------------------------------ loqa_beam_merge
// One wave per group g. Lane l < n_src * B holds candidate j = l % B of source
// row g * n_src + l / B; its score is the one f32 add cum_in[g, src] + cand_lp.
// A lane's rank is the number of candidates that come before it in the order
// (score desc, src asc, column asc): the order is total over the valid lanes
// (a column appears once per source row), so ranks 0 .. n_valid - 1 are each
// taken once and the lanes of rank < B write the outputs, one slot each.
__global__ __launch_bounds__(64) void beam_merge_kernel(
    const int* __restrict__ cand_id, const float* __restrict__ cand_lp,
    const float* __restrict__ eot_lp, const float* __restrict__ cum_in, int n_src, int B,
    int* __restrict__ tok, int* __restrict__ parent, float* __restrict__ lp,
    float* __restrict__ cum_out, float* __restrict__ eot_score, int* __restrict__ eot_fin) {
  const int g = blockIdx.x, l = threadIdx.x;
  const int n = n_src * B;
  const int src = l / B, j = l - src * B;
  int col = -1;
  float clp = -INFINITY, score = -INFINITY;
  if (l < n) {
    const size_t i = ((size_t)g * n_src + src) * B + j;
    col = cand_id[i];
    clp = cand_lp[i];
    score = cum_in[(size_t)g * B + src] + clp;
  }
  const bool valid = col >= 0;
  int rank = 0, n_valid = 0;
  for (int i = 0; i < n; ++i) {
    const int ocol = __shfl(col, i, 64);
    const float oscore = __shfl(score, i, 64);
    const int osrc = i / B;
    const bool ov = ocol >= 0;
    const bool before = oscore > score ||
        (oscore == score && (osrc < src || (osrc == src && ocol < col)));
    rank += (ov && before) ? 1 : 0;
    n_valid += ov ? 1 : 0;
  }
  if (valid && rank < B) {
    const size_t o = (size_t)g * B + rank;
    tok[o] = col, parent[o] = src, lp[o] = clp, cum_out[o] = score;
  }
  if (l < B && l >= n_valid) {        // missing candidates
    const size_t o = (size_t)g * B + l;
    tok[o] = -1, parent[o] = -1, lp[o] = -INFINITY, cum_out[o] = -INFINITY;
  }
  // the B-th selected score: held by the lane of rank B - 1 when B candidates exist
  float kth = (valid && rank == B - 1) ? score : -INFINITY;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kth = fmaxf(kth, __shfl_xor(kth, o, 64));
  if (l < B) {
    const float es = l < n_src ? cum_in[(size_t)g * B + l] + eot_lp[(size_t)g * n_src + l]
                               : -INFINITY;
    eot_score[(size_t)g * B + l] = es;
    eot_fin[(size_t)g * B + l] = (l < n_src && (n_valid < B || es > kth)) ? 1 : 0;
  }
}

// cand_id / cand_lp: [G * n_src, B], eot_lp: [G * n_src], cum_in and every
// output: [G, B]; n_src is 1 or B, 2 <= B <= 8 (n_src * B <= 64 lanes).
extern "C" int loqa_beam_merge(const int* cand_id, const float* cand_lp, const float* eot_lp,
                               const float* cum_in, int G, int n_src, int B, int* tok,
                               int* parent, float* lp, float* cum_out, float* eot_score,
                               int* eot_fin, hipStream_t s) {
  if (G <= 0) return 0;
  if (B < 1 || B > BEAM_MAX || (n_src != 1 && n_src != B) || !cand_id || !cand_lp || !eot_lp ||
      !cum_in || !tok || !parent || !lp || !cum_out || !eot_score || !eot_fin)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_merge_kernel, dim3(G), dim3(64), 0, s, cand_id, cand_lp, eot_lp, cum_in,
                     n_src, B, tok, parent, lp, cum_out, eot_score, eot_fin);
  return (int)hipGetLastError();
}

// -------------------------------------------------------- loqa_kv_copy_blocks
// k, v: [L, blocks, block_bytes]; pairs: int32 [P, 2] = (source block,
// destination block), the two sets disjoint (the caller checks), every index in
// [0, blocks). grid (P, L, 2): one workgroup copies one block of K or V of one
// layer in 16-byte vectors.
__global__ __launch_bounds__(256) void kv_copy_blocks_kernel(
    uint4* __restrict__ k, uint4* __restrict__ v, long long layer_vecs, int block_vecs,
    const int* __restrict__ pairs) {
  uint4* base = (blockIdx.z ? v : k) + (size_t)blockIdx.y * layer_vecs;
  const uint4* src = base + (size_t)pairs[2 * blockIdx.x] * block_vecs;
  uint4* dst = base + (size_t)pairs[2 * blockIdx.x + 1] * block_vecs;
  for (int i = threadIdx.x; i < block_vecs; i += 256) dst[i] = src[i];
}

extern "C" int loqa_kv_copy_blocks(void* k, void* v, int L, long long blocks,
                                   long long block_bytes, const int* pairs, int P,
                                   hipStream_t s) {
  if (P <= 0) return 0;
  if (!k || !v || !pairs || L <= 0 || L > 65535 || blocks <= 0 || block_bytes <= 0 ||
      block_bytes % 16 || block_bytes / 16 > 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_copy_blocks_kernel, dim3(P, L, 2), dim3(256), 0, s, (uint4*)k, (uint4*)v,
                     blocks * (block_bytes / 16), (int)(block_bytes / 16), pairs);
  return (int)hipGetLastError();
}
