// Voice activity detection over the PCM16 the STT upload already holds on the
// device: loqa_vad_energy (per-frame mean square) and loqa_vad_spans (noise
// floor, raw decision, close / open / pad smoothing, speech spans). Every value
// is an integer, so ops/reference.py (vad_energy, vad_spans) gives the same bits.
//
// An utterance is pcm[src_first, src_first + src_len) at `rate`; its frame f
// (20 ms: one encoder position) covers the source samples
//   [f * rate / 50, min(src_len, (f + 1) * rate / 50)),   F = ceil(src_len * 50 / rate),
// and its outputs start at `frame_first` in the frame array E.
//   E[f]   = floor(sum x^2 / count)                        (64-bit sum; E <= 2^30)
//   N[f]   = min(floor_max, min E[g], |g - f| <= W, g in [0, F))
//   raw[f] = E[f] >= level_min && E[f] * 256 > N[f] * ratio_q      (uint64)
// then, each on the result of the one before: close (a non-speech run with
// speech on both sides and fewer than min_silence frames becomes speech), open
// (a speech run of fewer than min_speech frames is removed), pad (a frame within
// `pad` frames of speech becomes speech). The maximal speech runs are the spans.
#include "common.h"
#include <algorithm>
#include <utility>
#include <vector>

#define VAD_EWAVES 4       // energy: one wave per frame, this many frames a workgroup
#define VAD_TILE 1024      // spans: frames per tile = threads of the workgroup
#define VAD_MAX_UTTERANCES 65535   // per launch: the energy grid's y extent
#define VAD_WS_WORDS 6     // spans workspace: int32 words per frame of the longest utterance

// one descriptor per utterance (ops.vad fills it): 4 x int64
struct VadDesc {
  long long src_first, src_len, rate, frame_first;
};

// host copy of the parameters, in this order: 7 x int32
struct VadParams {
  int level_min, floor_max, ratio_q, W, min_speech, min_silence, pad;
};

__host__ __device__ inline long long vad_frames(long long n, long long rate) {
  return (n * 50 + rate - 1) / rate;
}

// ------------------------------------------------------------------- energy
// A wave owns one frame: lanes stride over its samples (2-byte loads: src_first
// is arbitrary, so nothing wider is aligned), each keeps a uint64 partial sum,
// and the wave adds them as two 32-bit halves per shuffle. The loop bounds are
// the only place PCM is indexed and lie inside [0, src_len) of the utterance.
__global__ __launch_bounds__(VAD_EWAVES * WAVE)
void vad_energy_kernel(const int16_t* __restrict__ pcm, const VadDesc* __restrict__ descs,
                       uint32_t* __restrict__ E) {
  const VadDesc d = descs[blockIdx.y];
  const long long F = vad_frames(d.src_len, d.rate);
  const long long f = (long long)blockIdx.x * VAD_EWAVES + (threadIdx.x >> 6);
  if (f >= F) return;                       // wave-uniform
  const int lane = threadIdx.x & 63;
  const long long a = f * d.rate / 50;
  const long long b = min(d.src_len, (f + 1) * d.rate / 50);
  const int16_t* __restrict__ x = pcm + d.src_first;
  unsigned long long acc = 0;
  for (long long i = a + lane; i < b; i += WAVE) {
    const int v = x[i];
    acc += (unsigned)(v * v);               // (-32768)^2 = 2^30 fits
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)acc, o, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(acc >> 32), o, 64);
    acc += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 0) E[d.frame_first + f] = (uint32_t)(acc / (unsigned long long)(b - a));
}

// -------------------------------------------------------------------- spans
enum { VAD_MIN = 0, VAD_MAX = 1, VAD_ADD = 2 };

template <int OP>
__device__ __forceinline__ int vad_op(int a, int b) {
  return OP == VAD_MIN ? min(a, b) : OP == VAD_MAX ? max(a, b) : a + b;
}

// Inclusive scan of one value per thread over the workgroup, continued from
// `carry` (the scan of the tiles before; the same in every thread), which it
// advances by this tile. lds: VAD_TILE / 64 ints.
template <int OP>
__device__ __forceinline__ int vad_scan(int v, int* lds, int& carry) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v = vad_op<OP>(v, t);
  }
  if (lane == WAVE - 1) lds[wid] = v;
  __syncthreads();
  int pre = carry, tot = carry;
#pragma unroll
  for (int i = 0; i < VAD_TILE / WAVE; ++i) {
    const int t = lds[i];
    if (i < wid) pre = vad_op<OP>(pre, t);
    tot = vad_op<OP>(tot, t);
  }
  __syncthreads();
  carry = tot;
  return vad_op<OP>(v, pre);
}

// One smoothing step, in place on s[0, F). With flag = s (close, pad) or !s
// (open): prev[f] = the nearest flagged index <= f (-1: none), a forward
// max-scan kept in P; next[f] = the nearest flagged index >= f (F: none), a
// backward min-scan. A frame's new value needs only its own, prev and next, so
// the backward walk writes s as it goes (a tile reads only frames not yet
// written).
enum { VAD_CLOSE = 0, VAD_OPEN = 1, VAD_PAD = 2 };

template <int MODE>
__device__ __forceinline__ void vad_smooth(int* __restrict__ s, int* __restrict__ P, int F,
                                           int param, int* lds) {
  const int tid = threadIdx.x;
  int carry = -1;
  for (int t0 = 0; t0 < F; t0 += VAD_TILE) {
    const int f = t0 + tid;
    int v = -1;
    if (f < F && (s[f] != 0) == (MODE != VAD_OPEN)) v = f;
    v = vad_scan<VAD_MAX>(v, lds, carry);
    if (f < F) P[f] = v;
  }
  __syncthreads();
  carry = F;
  for (int t0 = 0; t0 < F; t0 += VAD_TILE) {
    const int f = F - 1 - (t0 + tid);
    int cur = 0, v = F;
    if (f >= 0) {
      cur = s[f];
      if ((cur != 0) == (MODE != VAD_OPEN)) v = f;
    }
    const int next = vad_scan<VAD_MIN>(v, lds, carry);
    if (f >= 0) {
      const int prev = P[f];
      int out;
      if (MODE == VAD_CLOSE)
        out = cur || (prev >= 0 && next < F && next - prev - 1 < param);
      else if (MODE == VAD_OPEN)
        out = cur && next - prev - 1 >= param;
      else
        out = cur || (prev >= 0 && f - prev <= param) || (next < F && next - f <= param);
      s[f] = out;
    }
  }
  __syncthreads();
}

// One workgroup per utterance; F has no bound, so every pass walks the frames
// in tiles of VAD_TILE and its arrays live in the caller's workspace (per
// utterance VAD_WS_WORDS * F_max words: two sliding-minimum buffers of 2 F_max,
// s and P of F_max).
//
// Noise floor: X[i] = E[i - We] (UINT_MAX for i < We), We = min(W, F), so
// N[f] = min X[f .. f + 2 We]; A_j[i] = min X[i .. i + 2^j) is built by doubling
// (UINT_MAX beyond the end) and a window of L = 2 We + 1 is the minimum of two
// overlapping A_k, k = floor(log2 L).
__global__ __launch_bounds__(VAD_TILE)
void vad_spans_kernel(const VadDesc* __restrict__ descs, const uint32_t* __restrict__ E,
                      VadParams p, int* __restrict__ ws, long long F_max,
                      int* __restrict__ spans, int cap, int* __restrict__ n_spans,
                      int* __restrict__ speech_frames) {
  __shared__ int lds[VAD_TILE / WAVE];
  const int u = blockIdx.x, tid = threadIdx.x;
  const VadDesc d = descs[u];
  const int F = (int)vad_frames(d.src_len, d.rate);
  if (F == 0) {
    if (tid == 0) n_spans[u] = 0, speech_frames[u] = 0;
    return;
  }
  const uint32_t* __restrict__ Eu = E + d.frame_first;
  int* base = ws + (size_t)u * VAD_WS_WORDS * F_max;
  uint32_t* a = (uint32_t*)base;
  uint32_t* b = (uint32_t*)(base + 2 * F_max);
  int* s = base + 4 * F_max;
  int* P = base + 5 * F_max;

  const int We = min(p.W, F), Lx = F + We, L = 2 * We + 1;
  for (int i = tid; i < Lx; i += VAD_TILE) a[i] = i >= We ? Eu[i - We] : 0xffffffffu;
  __syncthreads();
  const int k = 31 - __clz(L);
  for (int j = 0; j < k; ++j) {
    const int h = 1 << j;
    for (int i = tid; i < Lx; i += VAD_TILE) {
      uint32_t v = a[i];
      if (i + h < Lx) v = min(v, a[i + h]);
      b[i] = v;
    }
    __syncthreads();
    uint32_t* t = a;
    a = b;
    b = t;
  }
  const int off = L - (1 << k);
  for (int f = tid; f < F; f += VAD_TILE) {
    uint32_t n = a[f];
    if (f + off < Lx) n = min(n, a[f + off]);
    n = min(n, (uint32_t)p.floor_max);
    const uint32_t e = Eu[f];
    s[f] = e >= (uint32_t)p.level_min &&
           (unsigned long long)e * 256ull > (unsigned long long)n * (unsigned long long)p.ratio_q;
  }
  __syncthreads();

  vad_smooth<VAD_CLOSE>(s, P, F, p.min_silence, lds);
  vad_smooth<VAD_OPEN>(s, P, F, p.min_speech, lds);
  vad_smooth<VAD_PAD>(s, P, F, p.pad, lds);

  // spans: a run starts where s rises and ends after the frame where it falls;
  // the start's slot is the exclusive count of starts, and the run a frame
  // lies in is the last one started, so an end's slot is the inclusive count - 1
  int* out = spans + (size_t)u * cap * 2;
  int n_start = 0, n_speech = 0;
  for (int t0 = 0; t0 < F; t0 += VAD_TILE) {
    const int f = t0 + tid;
    const int cur = f < F && s[f];
    const int st = cur && (f == 0 || !s[f - 1]);
    const int en = cur && (f == F - 1 || !s[f + 1]);
    const int slot = vad_scan<VAD_ADD>(st, lds, n_start) - 1;
    vad_scan<VAD_ADD>(cur, lds, n_speech);
    if (st && slot < cap) out[2 * slot] = f;
    if (en && slot < cap) out[2 * slot + 1] = f + 1;
  }
  if (tid == 0) n_spans[u] = n_start, speech_frames[u] = n_speech;
}

// ------------------------------------------------------------------ launchers
static const long long VAD_RATES[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000};

// Descriptors (host copy) against the buffers they index: every utterance
// inside pcm (pcm_len < 0: not checked), its frames inside E, no two
// utterances' frames overlapping (the non-empty frame ranges sorted by their
// start: each must begin where the one before has ended). Returns the longest
// utterance's frames, -1 for a bad descriptor.
static long long vad_check(const long long* descs_host, int U, long long pcm_len,
                           long long E_cap) {
  long long F_max = 0;
  std::vector<std::pair<long long, long long>> ranges;
  ranges.reserve(U);
  for (int i = 0; i < U; ++i) {
    const long long* d = descs_host + 4 * (size_t)i;
    bool rate_ok = false;
    for (long long r : VAD_RATES) rate_ok |= d[2] == r;
    if (!rate_ok || d[0] < 0 || d[1] < 0 || d[1] >= (1LL << 40) || d[3] < 0) return -1;
    if (pcm_len >= 0 && (d[0] > pcm_len || d[1] > pcm_len - d[0])) return -1;
    const long long F = vad_frames(d[1], d[2]);
    if (F >= (1LL << 28) || d[3] > E_cap || F > E_cap - d[3]) return -1;
    if (F > 0) ranges.emplace_back(d[3], d[3] + F);
    F_max = F > F_max ? F : F_max;
  }
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i)
    if (ranges[i].first < ranges[i - 1].second) return -1;
  return F_max;
}

// E[frame_first + f] for every frame of every utterance, one launch; nothing
// else of E is written. descs: device [U][4] int64; descs_host: the same on the
// host, checked before anything runs.
extern "C" int loqa_vad_energy(const void* pcm, long long pcm_len, const void* descs,
                               const long long* descs_host, int U, void* E, long long E_cap,
                               hipStream_t s) {
  if (U <= 0) return U < 0 ? (int)hipErrorInvalidValue : 0;
  if (U > VAD_MAX_UTTERANCES || pcm_len < 0 || !descs_host) return (int)hipErrorInvalidValue;
  const long long F_max = vad_check(descs_host, U, pcm_len, E_cap);
  if (F_max < 0) return (int)hipErrorInvalidValue;
  if (F_max == 0) return 0;                 // only empty utterances: nothing to launch
  const long long gx = (F_max + VAD_EWAVES - 1) / VAD_EWAVES;
  hipLaunchKernelGGL(vad_energy_kernel, dim3((unsigned)gx, U), dim3(VAD_EWAVES * WAVE), 0, s,
                     (const int16_t*)pcm, (const VadDesc*)descs, (uint32_t*)E);
  return (int)hipGetLastError();
}

// Words of workspace loqa_vad_spans needs for U utterances of at most F_max frames
// (ops.vad allocates VAD_WS_WORDS = 6 per frame the same way).
static long long vad_ws_words(int U, long long F_max) {
  return (long long)VAD_WS_WORDS * (U > 0 ? U : 0) * (F_max > 1 ? F_max : 1);
}

extern "C" int loqa_vad_tile() { return VAD_TILE; }

// spans [U][cap][2], n_spans [U], speech_frames [U] from E; spans beyond
// n_spans are not written. params: the 7 host ints of VadParams, range-checked
// here as ops.reference.check_vad_params does.
extern "C" int loqa_vad_spans(const void* descs, const long long* descs_host, int U, const void* E,
                              long long E_cap, const int* params, void* ws, long long ws_words,
                              void* spans, int cap, void* n_spans, void* speech_frames,
                              hipStream_t s) {
  if (U <= 0) return U < 0 ? (int)hipErrorInvalidValue : 0;
  if (U > VAD_MAX_UTTERANCES || !descs_host || !params) return (int)hipErrorInvalidValue;
  VadParams p;
  p.level_min = params[0], p.floor_max = params[1], p.ratio_q = params[2], p.W = params[3];
  p.min_speech = params[4], p.min_silence = params[5], p.pad = params[6];
  if (p.level_min < 0 || p.level_min > (1 << 30) || p.floor_max < 0 || p.floor_max > (1 << 30) ||
      p.ratio_q < 256 || p.ratio_q > 2560000 || p.W < 0 || p.W > 3000 || p.min_speech < 1 ||
      p.min_speech > 500 || p.min_silence < 0 || p.min_silence > 500 || p.pad < 0 || p.pad > 500)
    return (int)hipErrorInvalidValue;
  const long long F_max = vad_check(descs_host, U, -1, E_cap);
  if (F_max < 0 || cap < F_max / 2 + 1 || ws_words < vad_ws_words(U, F_max))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(vad_spans_kernel, dim3(U), dim3(VAD_TILE), 0, s, (const VadDesc*)descs,
                     (const uint32_t*)E, p, (int*)ws, F_max > 1 ? F_max : 1, (int*)spans, cap,
                     (int*)n_spans, (int*)speech_frames);
  return (int)hipGetLastError();
}
