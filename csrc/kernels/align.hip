// Word timestamps: Whisper's find_alignment on the device (gfx950).
//
//   loqa_align_record  in the captured decoder step: the cross-attention
//                      queries of the alignment heads -> align_q[slot][a][pos]
//   loqa_align_scores  P[a, r, :] = softmax_f(scale * q[a, r] . k[a, f]), the
//                      window's rows against the encoder K rows read in place
//   loqa_align_cost    normalise over the rows, median filter (7) over the
//                      frames, mean over the heads, negate -> cost[N, F]
//   loqa_dtw           dynamic time warping over cost, backtrace on the device
//
// Definitions: loqa_hub_amd/ops/reference.py (align_scores, align_cost, dtw).
//
// Ordering invariant: record, scores, cost and dtw all run on the engine's ONE
// stream. A step's record launch is stream-ordered before the alignment of the
// window it belongs to, and writes go by (slot, position): a fallback retry, a
// discarded speculative step or a reused slot only overwrites positions whose
// rows the host does not pass to the alignment, or that the next window
// rewrites before its own alignment reads them.
#include "common.h"

#define ALIGN_MAX_HEADS 32

// per-head base pointers, passed by value (a captured step keeps its copy)
struct AlignPtrs {
  const bf16_t* p[ALIGN_MAX_HEADS];
};

// ------------------------------------------------------------------- record
// One thread per (row, head, 16-byte chunk). q[a] points at column head * D of
// the head's layer query buffer [T, ldq].
__global__ void __launch_bounds__(256)
align_record_kernel(AlignPtrs q, int A, int D, long ldq, const int* __restrict__ positions,
                    const int* __restrict__ slots, const int* __restrict__ cu_q,
                    const int* __restrict__ row_slot, int T, int B, bf16_t* __restrict__ align_q,
                    int n_slots, int n_ctx) {
  const int vec = D >> 3;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * A * vec) return;
  const int c = (int)(idx % vec), a = (int)((idx / vec) % A), r = (int)(idx / ((long)vec * A));
  if (slots[r] < 0) return;                     // a padding row
  int b = -1;
  for (int s = 0; s < B; ++s)
    if (cu_q[s] <= r && r < cu_q[s + 1]) { b = s; break; }
  if (b < 0) return;
  const int s = row_slot[b], p = positions[r];
  if ((unsigned)s >= (unsigned)n_slots || (unsigned)p >= (unsigned)n_ctx) return;
  const uint4 v = *reinterpret_cast<const uint4*>(q.p[a] + (long)r * ldq + c * 8);
  *reinterpret_cast<uint4*>(align_q + (((long)s * A + a) * n_ctx + p) * D + c * 8) = v;
}

extern "C" int loqa_align_record(const void* const* q_ptrs, int A, int D, long long ldq,
                                 const int* positions, const int* slots, const int* cu_q,
                                 const int* row_slot, int T, int B, void* align_q, int n_slots,
                                 int n_ctx, hipStream_t stream) {
  if (A < 1 || A > ALIGN_MAX_HEADS || D < 8 || (D & 7) || (ldq & 7) || T < 1 || B < 1)
    return (int)hipErrorInvalidValue;
  AlignPtrs q;
  for (int a = 0; a < ALIGN_MAX_HEADS; ++a) q.p[a] = (const bf16_t*)q_ptrs[a < A ? a : 0];
  const long total = (long)T * A * (D >> 3);
  align_record_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(
      q, A, D, (long)ldq, positions, slots, cu_q, row_slot, T, B, (bf16_t*)align_q, n_slots, n_ctx);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------- scores
// Workgroup = 16 query rows of one head, 4 waves. Phase 1: every wave takes
// frame tiles w, w + 4, ...: one 16 x 16 x D product per tile on
// mfma_f32_16x16x32_bf16 (A operand: lane holds q[row l & 15][8 (l >> 4) + j];
// B operand: k[frame l & 15][8 (l >> 4) + j], both 16-byte loads straight from
// memory), the scaled scores go to P. Phase 2: every wave normalises 4 of the
// rows in place (max, exp, sum, divide; the sum's order is fixed). K rows at or
// beyond F and align_q positions outside ``rows`` are never read.
template <int KS>   // D = 32 KS
__global__ void __launch_bounds__(256)
align_scores_kernel(const bf16_t* __restrict__ align_q, const int* __restrict__ rows, int R,
                    AlignPtrs kp, long ldk, int n_ctx, int F, float scale, float* __restrict__ P) {
  constexpr int D = 32 * KS;
  const int a = blockIdx.y, r0 = blockIdx.x * 16;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  uint4 qf[KS];
  {
    const int r = r0 + lr;
    int pos = r < R ? rows[r] : -1;
    if ((unsigned)pos >= (unsigned)n_ctx) pos = -1;
    const bf16_t* qrow = align_q + ((long)a * n_ctx + (pos < 0 ? 0 : pos)) * D + lk;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[s] = pos < 0 ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4*>(qrow + 32 * s);
  }
  const bf16_t* kbase = kp.p[a];
  float* Pa = P + (long)a * R * F;
  for (int f0 = w * 16; f0 < F; f0 += 64) {
    const int f = f0 + lr;
    float4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const uint4 kf = f < F ? *reinterpret_cast<const uint4*>(kbase + (long)f * ldk + lk + 32 * s)
                             : make_uint4(0, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, qf[s]),
                                                    __builtin_bit_cast(bf16x8, kf), acc, 0, 0, 0);
    }
    // C/D: column (frame) = lane & 15, row = (lane >> 4) * 4 + i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + (lane >> 4) * 4 + i;
      if (r < R && f < F) Pa[(long)r * F + f] = acc[i] * scale;
    }
  }
  __threadfence_block();
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + w * 4 + i;
    if (r >= R) break;                          // wave-uniform
    float* p = Pa + (long)r * F;
    float m = -__builtin_inff();
    for (int f = lane; f < F; f += 64) m = fmaxf(m, p[f]);
    m = wave_max(m);
    float sum = 0.f;
    for (int f = lane; f < F; f += 64) {
      const float e = expf(p[f] - m);
      p[f] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    for (int f = lane; f < F; f += 64) p[f] = p[f] / sum;
  }
}

extern "C" int loqa_align_scores(const void* align_q, const int* rows, int R,
                                 const void* const* k_ptrs, int A, int D, int n_ctx,
                                 long long ldk, int F, float scale, float* P, hipStream_t stream) {
  if (A < 1 || A > ALIGN_MAX_HEADS || R < 1 || F < 1 || (ldk & 7) || (D != 32 && D != 64 && D != 128))
    return (int)hipErrorInvalidValue;
  AlignPtrs kp;
  for (int a = 0; a < ALIGN_MAX_HEADS; ++a) kp.p[a] = (const bf16_t*)k_ptrs[a < A ? a : 0];
  const dim3 grid((R + 15) / 16, A);
  const bf16_t* q = (const bf16_t*)align_q;
  if (D == 32)
    align_scores_kernel<1><<<grid, 256, 0, stream>>>(q, rows, R, kp, (long)ldk, n_ctx, F, scale, P);
  else if (D == 64)
    align_scores_kernel<2><<<grid, 256, 0, stream>>>(q, rows, R, kp, (long)ldk, n_ctx, F, scale, P);
  else
    align_scores_kernel<4><<<grid, 256, 0, stream>>>(q, rows, R, kp, (long)ldk, n_ctx, F, scale, P);
  return (int)hipGetLastError();
}

// --------------------------------------------------------------------- cost
// Workgroup = COST_TILE frames (+ 3 halo frames each side) of every head.
// Phase 1: mean and population std over the R rows of each (head, column), one
// thread per pair, rows in order. Phase 2: every output (row, frame) takes, per
// head in order, the median of its 7 normalised neighbours (reflect padding at
// the edges; F <= 3: the value itself) and averages them over the heads.
#define COST_TILE 32
#define COST_HALO 3
#define COST_COLS (COST_TILE + 2 * COST_HALO)

__device__ __forceinline__ void cswap(float& x, float& y) {
  const float lo = fminf(x, y), hi = fmaxf(x, y);
  x = lo;
  y = hi;
}

// median of 7 (the 4th smallest): Paeth's 13-exchange selection network
__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5,
                                         float v6) {
  cswap(v0, v5); cswap(v0, v3); cswap(v1, v6); cswap(v2, v4); cswap(v0, v1); cswap(v3, v5);
  cswap(v2, v6); cswap(v2, v3); cswap(v3, v6); cswap(v4, v5); cswap(v1, v4); cswap(v1, v3);
  cswap(v3, v4);
  return v3;
}

__global__ void __launch_bounds__(256)
align_cost_kernel(const float* __restrict__ P, int A, int R, int F, int n_lead,
                  float* __restrict__ out) {
  __shared__ float s_mean[ALIGN_MAX_HEADS][COST_COLS];
  __shared__ float s_std[ALIGN_MAX_HEADS][COST_COLS];
  __shared__ int s_col[COST_COLS];              // the frame a halo column reads (reflected)
  const int f0 = blockIdx.x * COST_TILE;
  const bool filt = F > COST_HALO;
  for (int c = threadIdx.x; c < COST_COLS; c += blockDim.x) {
    int g = f0 - COST_HALO + c;
    if (g < 0) g = -g;
    if (g >= F) g = 2 * (F - 1) - g;
    s_col[c] = (g >= 0 && g < F) ? g : -1;      // -1: no output of this tile reads it
  }
  __syncthreads();
  for (int it = threadIdx.x; it < A * COST_COLS; it += blockDim.x) {
    const int a = it / COST_COLS, c = it % COST_COLS, g = s_col[c];
    float mean = 0.f, sd = 0.f;
    if (g >= 0) {
      const float* col = P + (long)a * R * F + g;
      const float first = col[0];
      bool same = true;                         // equal rows: std is 0, not a rounding residue
      float sum = 0.f;
      // (unrolled: the loads of 8 rows are in flight together, the adds stay in row order)
#pragma unroll 8
      for (int r = 0; r < R; ++r) {
        const float v = col[(long)r * F];
        same = same && v == first;
        sum += v;
      }
      mean = sum / (float)R;
      float sq = 0.f;
#pragma unroll 8
      for (int r = 0; r < R; ++r) {
        const float d = col[(long)r * F] - mean;
        sq += d * d;
      }
      sd = same ? 0.f : sqrtf(sq / (float)R);
    }
    s_mean[a][c] = mean;
    s_std[a][c] = sd;
  }
  __syncthreads();
  const int fl = threadIdx.x % COST_TILE, f = f0 + fl;
  if (f >= F) return;
  const int c0 = fl + COST_HALO;                // this frame's own column
  for (int r = n_lead + threadIdx.x / COST_TILE; r < R; r += blockDim.x / COST_TILE) {
    float acc = 0.f;
    for (int a = 0; a < A; ++a) {
      const float* row = P + ((long)a * R + r) * F;
      float v[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int c = filt ? c0 - COST_HALO + k : c0;
        const int g = s_col[c];
        const float sd = s_std[a][c];
        v[k] = (g < 0 || sd == 0.f) ? 0.f : (row[g] - s_mean[a][c]) / sd;
      }
      acc += filt ? median7(v[0], v[1], v[2], v[3], v[4], v[5], v[6]) : v[0];
    }
    out[(long)(r - n_lead) * F + f] = -(acc / (float)A);
  }
}

extern "C" int loqa_align_cost(const float* P, int A, int R, int F, int n_lead, float* out,
                               hipStream_t stream) {
  if (A < 1 || A > ALIGN_MAX_HEADS || R < 1 || F < 1 || n_lead < 0 || n_lead >= R)
    return (int)hipErrorInvalidValue;
  align_cost_kernel<<<(F + COST_TILE - 1) / COST_TILE, 256, 0, stream>>>(P, A, R, F, n_lead, out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------- dtw
// One workgroup, thread i owns DP row i + 1 and walks its columns along the
// anti-diagonal wavefront: at step t it computes cell (i, t - i). It keeps
// c[i][j-1] in a register, takes c[i-1][j] from thread i - 1 (lane shuffle; the
// first lane of a wave reads the previous wave's last lane through LDS, double
// buffered, one barrier per step) and remembers last step's neighbour value as
// c[i-1][j-1]. Each cell is the reference's one f32 add of the same operands,
// so costs and path are the reference's bit for bit. Trace codes (one byte,
// stored by diagonal: [t][i], coalesced) go to LDS when they fit, else to the
// workspace; thread 0 walks the path back and tok_frame leaves through LDS.
#define DTW_MAX_N 448
#define DTW_GROUP 8

__global__ void __launch_bounds__(DTW_MAX_N)
dtw_kernel(const float* __restrict__ x, int N, int M, uint8_t* __restrict__ trace_ws, int lds_trace,
           int* __restrict__ tok_frame, float* __restrict__ total) {
  extern __shared__ uint8_t s_trace[];
  __shared__ float s_edge[2][DTW_MAX_N / 64 + 1];
  __shared__ int s_tok[DTW_MAX_N];
  const int i = threadIdx.x, lane = i & 63, w = i >> 6;
  const int nw = blockDim.x >> 6;
  const float INF = __builtin_inff();
  uint8_t* trace = lds_trace ? s_trace : trace_ws;
  if (i < 2 * (DTW_MAX_N / 64 + 1)) (&s_edge[0][0])[i] = INF;
  s_tok[i] = 0;
  __syncthreads();
  const bool row = i < N;
  const float* xr = x + (long)(row ? i : 0) * M;
  const int T = N + M - 1;
  float cur = INF;                  // this row's last cell c[i][j-1] (c[i][0] = inf)
  float diag = i == 0 ? 0.f : INF;  // c[i-1][j-1]: c[0][0] = 0, every other border cell inf
  float xc[DTW_GROUP], xn[DTW_GROUP];
#pragma unroll
  for (int k = 0; k < DTW_GROUP; ++k) {
    const int j = k - i;
    xc[k] = (row && j >= 0 && j < M) ? xr[j] : 0.f;
  }
  for (int tg = 0; tg < T; tg += DTW_GROUP) {
    // the next group's costs are loaded while this group's cells are computed
#pragma unroll
    for (int k = 0; k < DTW_GROUP; ++k) {
      const int j = tg + DTW_GROUP + k - i;
      xn[k] = (row && j >= 0 && j < M) ? xr[j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < DTW_GROUP; ++k) {
      const int t = tg + k;
      if (t < T) {                              // uniform
        float up = __shfl_up(cur, 1, 64);       // c[i-1][j] (thread i - 1, previous step)
        if (lane == 0) up = w == 0 ? INF : s_edge[(t + 1) & 1][w - 1];
        const int j = t - i;
        if (row && j >= 0 && j < M) {
          const float c0 = diag, c1 = up, c2 = cur;
          float c;
          uint8_t code;
          if (c0 < c1 && c0 < c2) { c = c0; code = 0; }
          else if (c1 < c0 && c1 < c2) { c = c1; code = 1; }
          else { c = c2; code = 2; }
          cur = xc[k] + c;
          diag = up;
          trace[(long)t * N + i] = code;
        }
        if (nw > 1) {
          if (lane == 63) s_edge[t & 1][w] = cur;
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (int k = 0; k < DTW_GROUP; ++k) xc[k] = xn[k];
  }
  if (i == N - 1) *total = cur;
  __threadfence_block();
  __syncthreads();
  if (i == 0) {
    int I = N, J = M;
    for (int guard = 0; (I > 0 || J > 0) && guard < N + M + 2; ++guard) {
      if (I > 0 && J > 0) s_tok[I - 1] = J - 1;   // going back, the last visit is the first cell
      const int code = I == 0 ? 2 : J == 0 ? 1 : trace[(long)(I + J - 2) * N + (I - 1)];
      if (code == 0) { --I; --J; }
      else if (code == 1) --I;
      else --J;
    }
  }
  __syncthreads();
  if (row) tok_frame[i] = s_tok[i];
}

// trace_ws: (N + M - 1) * N bytes (ops.dtw_workspace); unused when the codes fit LDS
extern "C" int loqa_dtw(const float* x, int N, int M, void* trace_ws, int* tok_frame, float* total,
                        hipStream_t stream) {
  if (N < 1 || N > DTW_MAX_N || M < 1) return (int)hipErrorInvalidValue;
  const long long bytes = (long long)(N + M - 1) * N;
  const int lds = bytes <= 48 * 1024;
  dtw_kernel<<<1, (N + 63) / 64 * 64, lds ? (size_t)bytes : 0, stream>>>(
      x, N, M, (uint8_t*)trace_ws, lds, tok_frame, total);
  return (int)hipGetLastError();
}
