// Sample-rate conversion of PCM16: a polyphase windowed-sinc resampler with two
// entry points - loqa_pcm16_resample_pad (ingest: the resampling sibling of
// loqa_pcm16_f32_pad in elementwise.hip, relay audio of any supported rate ->
// padded 16 kHz f32 encoder rows) and loqa_pcm16_resample (reply: the voice's
// PCM16 -> PCM16 at the rate the relays play).
//
// For rate_in -> rate_out: g = gcd, L = rate_out / g, M = rate_in / g. Output
// sample n sits at source time n * M / L: base = (n * M) div L, phase =
// (n * M) mod L, and
//   y[n] = sum_{j < T} x[base - H + j] * tab[phase][j],    H = (T - 1) / 2,
// with zeros outside [0, src_len). tab is the [L][T] f32 table the host builds
// once per rate pair (ops.resample_filter; the Kaiser-windowed sinc of
// ops/reference.py resample_filter, fp64 rounded once to f32). The sum runs in
// tap order as one fma chain, so a sample's bits depend only on n and on the
// utterance - not on the row, chunk or launch it is computed in.
//
// A workgroup owns RS_CHUNK consecutive outputs of one row. n * M needs 64 bits
// for long-form audio (9.6 M outputs x 441), so the chunk's first output is
// placed in 64-bit arithmetic once per workgroup; inside the chunk everything is
// a 32-bit offset from it (i * M + phase0 < 2^21). The chunk's source span,
// x[base0 - H .. base_last + H], is staged through LDS as f32 (exact integers;
// the predicate on [0, src_len) is the only place global PCM is indexed, so no
// lane reads outside the utterance's samples), and every tap is then one LDS
// read, one table read (L2-resident, a broadcast when L = 1) and one fma.
#include "common.h"

#define RS_CHUNK 1024
#define RS_THREADS 256
// LDS span (samples) a chunk may need: 48 kHz -> 8 kHz, the widest supported
// pair, is 1024 * 6 + T (409) = 6553; the launchers check every row against it
#define RS_SPAN 6656

// one descriptor per output row (ops.pcm16_resample_padded fills it): 8 x int64
struct RsRow {
  long long src_first;   // the utterance's first sample in the concatenated PCM
  long long src_len;     // the utterance's source samples
  long long out_first;   // the row's first output index in the utterance's resampled signal
  long long out_len;     // outputs kept in this row (zeros after them)
  long long L, M, T;
  const float* tab;      // [L][T]
};

__host__ __device__ inline long long rs_span(long long L, long long M, long long T) {
  return (L - 1 + (RS_CHUNK - 1) * M) / L + T;
}

// Stage the source span of outputs [n0, n0 + cnt) into s; returns phase0.
__device__ __forceinline__ int rs_stage(const int16_t* __restrict__ x, long long src_len,
                                        long long n0, int cnt, int L, int M, int T, float* s) {
  const long long t0 = n0 * (long long)M;
  const long long base0 = t0 / L;
  const int ph0 = (int)(t0 - base0 * L);
  const int span = (ph0 + (cnt - 1) * M) / L + T;
  const long long lo = base0 - ((T - 1) >> 1);
  for (int i = threadIdx.x; i < span; i += RS_THREADS) {
    const long long j = lo + i;
    s[i] = (j >= 0 && j < src_len) ? (float)x[j] : 0.f;
  }
  __syncthreads();
  return ph0;
}

// Output i of the staged chunk (in source integer units).
__device__ __forceinline__ float rs_output(const float* s, const float* __restrict__ tab, int ph0,
                                           int i, int L, int M, int T) {
  const unsigned t = (unsigned)(ph0 + i * M);
  const unsigned d = t / (unsigned)L;
  const float* h = tab + (size_t)(t - d * (unsigned)L) * T;
  const float* xs = s + d;
  float acc = 0.f;
  for (int j = 0; j < T; ++j) acc = __builtin_fmaf(xs[j], h[j], acc);
  return acc;
}

// Ingest: row r of out [rows, ld] = the utterance's resampled samples
// [out_first, out_first + out_len) * (1 / 32767.f), +0.0 after them; sumsq[r]
// accumulates the squares of the written samples (block sum + one atomicAdd per
// workgroup, as pcm16_f32_pad_kernel). A 16 kHz row is L = M = T = 1 with the
// table {1.0f}: fma(x, 1, 0) = x, so its elements are pcm16_f32_pad_kernel's bits.
__global__ __launch_bounds__(RS_THREADS)
void pcm16_resample_pad_kernel(const int16_t* __restrict__ pcm, float* __restrict__ out,
                               const RsRow* __restrict__ rows, float* __restrict__ sumsq,
                               long long ld) {
  __shared__ float s[RS_SPAN];
  __shared__ float scratch[4];
  const int row = blockIdx.y;
  const RsRow r = rows[row];
  const long long len = min(max(r.out_len, 0LL), ld);
  const long long c0 = (long long)blockIdx.x * RS_CHUNK;
  const int n = (int)(min(ld, c0 + RS_CHUNK) - c0);          // elements written
  const int cnt = (int)min(max(len - c0, 0LL), (long long)n);  // of them resampled
  const int L = (int)r.L, M = (int)r.M, T = (int)r.T;
  int ph0 = 0;
  if (cnt > 0) ph0 = rs_stage(pcm + r.src_first, r.src_len, r.out_first + c0, cnt, L, M, T, s);
  float* dst = out + (size_t)row * ld + c0;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += RS_THREADS) {
    const float f = i < cnt ? rs_output(s, r.tab, ph0, i, L, M, T) * (1.0f / 32767.0f) : 0.f;
    dst[i] = f;
    acc += f * f;
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0 && cnt > 0) atomicAdd(sumsq + row, acc);
}

extern "C" int loqa_pcm16_resample_pad(const void* pcm, float* out, const void* rows,
                                       const long long* rows_host, float* sumsq, int nrows,
                                       long long ld, hipStream_t s) {
  if (nrows <= 0 || ld <= 0) return nrows < 0 || ld < 0 ? (int)hipErrorInvalidValue : 0;
  // rows_host: the same descriptors on the host, checked before anything runs
  for (int i = 0; i < nrows; ++i) {
    const long long* d = rows_host + 8 * (size_t)i;
    if (d[0] < 0 || d[1] < 0 || d[2] < 0 || d[4] < 1 || d[5] < 1 || d[6] < 1 || !(d[6] & 1) ||
        !d[7] || rs_span(d[4], d[5], d[6]) > RS_SPAN || RS_CHUNK * d[5] + d[4] > (1LL << 30))
      return (int)hipErrorInvalidValue;
  }
  hipError_t e = hipMemsetAsync(sumsq, 0, sizeof(float) * nrows, s);
  if (e != hipSuccess) return (int)e;
  const long long chunks = (ld + RS_CHUNK - 1) / RS_CHUNK;
  hipLaunchKernelGGL(pcm16_resample_pad_kernel, dim3((unsigned)chunks, nrows), dim3(RS_THREADS), 0,
                     s, (const int16_t*)pcm, out, (const RsRow*)rows, sumsq, ld);
  return (int)hipGetLastError();
}

// Reply: row b of in [B, max_in] (row stride ld_in) holds n[b] samples (a device
// array the host has not read; clamped to [0, max_in]); row b of out [B, ld_out] gets
// n_out[b] = min(ceil(n[b] * L / M), ld_out) samples - the f32 sum rounded to
// nearest even and saturated to int16 - and zeros after them. n_out is written
// here, by the first workgroup of each row.
__global__ __launch_bounds__(RS_THREADS)
void pcm16_resample_kernel(const int16_t* __restrict__ in, long long ld_in, long long max_in,
                           const void* __restrict__ n_in, int n_is64, int16_t* __restrict__ out,
                           long long ld_out, int* __restrict__ n_out, int L, int M, int T,
                           const float* __restrict__ tab) {
  __shared__ float s[RS_SPAN];
  const int b = blockIdx.y;
  long long src_len = n_is64 ? ((const long long*)n_in)[b] : (long long)((const int*)n_in)[b];
  src_len = min(max(src_len, 0LL), max_in);
  const long long len = min((src_len * L + M - 1) / M, ld_out);
  if (blockIdx.x == 0 && threadIdx.x == 0) n_out[b] = (int)len;
  const long long c0 = (long long)blockIdx.x * RS_CHUNK;
  const int n = (int)(min(ld_out, c0 + RS_CHUNK) - c0);
  const int cnt = (int)min(max(len - c0, 0LL), (long long)n);
  int ph0 = 0;
  if (cnt > 0) ph0 = rs_stage(in + (size_t)b * ld_in, src_len, c0, cnt, L, M, T, s);
  int16_t* dst = out + (size_t)b * ld_out + c0;
  for (int i = threadIdx.x; i < n; i += RS_THREADS) {
    float v = 0.f;
    if (i < cnt) v = fminf(fmaxf(rintf(rs_output(s, tab, ph0, i, L, M, T)), -32768.f), 32767.f);
    dst[i] = (int16_t)(int)v;
  }
}

extern "C" int loqa_pcm16_resample(const void* in, long long ld_in, long long max_in,
                                   const void* n_in, int n_is64, void* out, long long ld_out, int* n_out, int B, int L, int M,
                                   int T, const float* tab, hipStream_t s) {
  if (B <= 0) return B < 0 ? (int)hipErrorInvalidValue : 0;
  if (max_in < 0 || ld_in < max_in || ld_out <= 0 || ld_out >= (1LL << 31) || L < 1 || M < 1 || T < 1 || !(T & 1) ||
      !tab || rs_span(L, M, T) > RS_SPAN || (long long)RS_CHUNK * M + L > (1LL << 30))
    return (int)hipErrorInvalidValue;
  const long long chunks = (ld_out + RS_CHUNK - 1) / RS_CHUNK;
  hipLaunchKernelGGL(pcm16_resample_kernel, dim3((unsigned)chunks, B), dim3(RS_THREADS), 0, s,
                     (const int16_t*)in, ld_in, max_in, n_in, n_is64, (int16_t*)out, ld_out, n_out, L, M, T,
                     tab);
  return (int)hipGetLastError();
}
