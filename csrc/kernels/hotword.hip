// Hotword biasing of the Whisper decoder's logits, matched on the device:
//   loqa_hotword_step  per logits row: advance the row's node of a phrase
//                      automaton by the token its sequence sampled last, store
//                      it, and add one boost to every column the node expects
// The automaton is an Aho-Corasick trie whose failure chains the host has
// flattened (engine/hotwords.py), so nothing here walks a chain:
//   hdr  int32 [4]    N (nodes), T (table entries), the bits of the f32 boost, 0
//   off  int32 [N+1]  span n = entries off[n] .. off[n+1]
//   tok  int32 [T]    edge tokens, ascending within a span
//   dst  int32 [T]    edge targets
// Span 0 holds the root's edges, span n > 0 the union of the edges of the
// non-root nodes of n's failure chain (the deepest node's target). So
//   advance(n, t) = t in span(n) ? its dst : t in span(0) ? its dst : 0
//   boosted(n)    = span(n).tok U span(0).tok, every column once.
// Token values are only ever compared: a garbage or negative last token finds
// no edge and lands on the root, and indexes nothing.
#include "common.h"

#define HOTWORD_WG 64

// The index of t in tok[lo .. hi), ascending, or -1. Every lane of the wave
// runs it on the same span: uniform control flow, broadcast loads.
__device__ __forceinline__ int hw_find(const int* __restrict__ tok, int lo, int hi, int t) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int v = tok[mid];
    if (v == t) return mid;
    if (v < t) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// x + boost in f32 on one element. bf16 is widened, added in f32 and rounded to
// nearest even. A NaN is not written at all, so it keeps its bits (what a
// conversion makes of a NaN differs between hosts); -inf + boost is -inf.
template <bool BF16>
__device__ __forceinline__ void hw_add(void* row, int c, float boost) {
  if (BF16) {
    bf16_t* p = (bf16_t*)row + c;
    const float x = bf2f(*p);
    if (x != x) return;
    const uint32_t u = __float_as_uint(x + boost);      // finite or +-inf
    *p = (bf16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  } else {
    float* p = (float*)row + c;
    const float x = *p;
    if (x != x) return;
    *p = x + boost;
  }
}

// grid (B), one wave per row: its lanes stride the node's span, then the root's
// (skipping a root edge the node's span carries too, found by binary search).
// The only writes are the row's boosted columns and hw_state[slot] (lane 0,
// after every lane of this one wave has read it). No atomics.
template <bool BF16>
__global__ __launch_bounds__(HOTWORD_WG) void hotword_step_kernel(
    void* __restrict__ logits, long long ld, int V, const int* __restrict__ ctl,
    const int* __restrict__ row_slot, int* __restrict__ hw_state,
    const int* __restrict__ last_tok, int slots, const int* __restrict__ hdr,
    const int* __restrict__ off, const int* __restrict__ tok, const int* __restrict__ dst,
    int n_cap, int t_cap) {
  const int b = blockIdx.x;
  const int c = ctl[b];
  if (c != 1 && c != 2) return;
  const int s = row_slot[b];
  if ((unsigned)s >= (unsigned)slots) return;      // as ctl = 0
  const int N = hdr[0], T = hdr[1];
  if (N < 1 || N > n_cap || T < 1 || T > t_cap) return;   // no phrases: nothing to do
  const float boost = __int_as_float(hdr[2]);
  // the root's span, clamped to the table (the host writes 0 <= off <= T)
  const int r0 = min(max(off[0], 0), T), r1 = min(max(off[1], r0), T);
  int n = 0;
  if (c == 2) {
    n = hw_state[s];
    if ((unsigned)n >= (unsigned)N) n = 0;
    const int t = last_tok[s];
    int e = -1;
    if (n > 0) {
      const int a0 = min(max(off[n], 0), T), a1 = min(max(off[n + 1], a0), T);
      e = hw_find(tok, a0, a1, t);
    }
    if (e < 0) e = hw_find(tok, r0, r1, t);
    n = e < 0 ? 0 : dst[e];
    if ((unsigned)n >= (unsigned)N) n = 0;
  }
  if (threadIdx.x == 0) hw_state[s] = n;
  void* row = BF16 ? (void*)((bf16_t*)logits + (size_t)b * ld)
                   : (void*)((float*)logits + (size_t)b * ld);
  int a0 = 0, a1 = 0;
  if (n > 0) {
    a0 = min(max(off[n], 0), T);
    a1 = min(max(off[n + 1], a0), T);
    for (int i = a0 + threadIdx.x; i < a1; i += HOTWORD_WG) {
      const int col = tok[i];
      if ((unsigned)col < (unsigned)V) hw_add<BF16>(row, col, boost);
    }
  }
  for (int i = r0 + threadIdx.x; i < r1; i += HOTWORD_WG) {
    const int col = tok[i];
    if ((unsigned)col >= (unsigned)V) continue;
    if (n > 0 && hw_find(tok, a0, a1, col) >= 0) continue;   // boosted above, once
    hw_add<BF16>(row, col, boost);
  }
}

extern "C" int loqa_hotword_wg() { return HOTWORD_WG; }

// logits: [B, >= V] f32 or bf16, row stride ld elements; ctl, row_slot: int32
// [B]; hw_state, last_tok: int32 [slots]; off has n_cap + 1 entries, tok and
// dst t_cap each (the header's N and T are checked against them on the device).
extern "C" int loqa_hotword_step(void* logits, int is_bf16, long long ld, int B, int V,
                                 const int* ctl, const int* row_slot, int* hw_state,
                                 const int* last_tok, int slots, const int* hdr, const int* off,
                                 const int* tok, const int* dst, int n_cap, int t_cap,
                                 hipStream_t s) {
  if (B <= 0) return 0;
  if (!logits || !ctl || !row_slot || !hw_state || !last_tok || !hdr || !off || !tok || !dst ||
      V <= 0 || ld < V || slots <= 0 || n_cap < 1 || t_cap < 1)
    return (int)hipErrorInvalidValue;
  if (is_bf16)
    hipLaunchKernelGGL(hotword_step_kernel<true>, dim3(B), dim3(HOTWORD_WG), 0, s, logits, ld, V,
                       ctl, row_slot, hw_state, last_tok, slots, hdr, off, tok, dst, n_cap, t_cap);
  else
    hipLaunchKernelGGL(hotword_step_kernel<false>, dim3(B), dim3(HOTWORD_WG), 0, s, logits, ld, V,
                       ctl, row_slot, hw_state, last_tok, slots, hdr, off, tok, dst, n_cap, t_cap);
  return (int)hipGetLastError();
}
