// FLAC encoding of reply audio on the device: loqa_flac_encode turns rows of
// PCM16 (the VITS output, or its resampled copy) into one FLAC stream per row -
// mono, 16 bits, a fixed block size, CONSTANT / VERBATIM / FIXED subframes with
// partitioned Rice residuals. ops/reference.py flac_encode is the model; every
// decision below is the integer arithmetic of its flac_frame_plan, so the bytes
// are the model's bytes (docs/ARCHITECTURE.md "FLAC replies" states the rule).
//
// Three launches on the caller's stream, nothing read by the host between them:
//   flac_frame_kernel  grid (frames, rows): one workgroup encodes one frame
//                      into its fixed-stride staging slot and records its bytes
//   flac_scan_kernel   grid (rows): prefix of a row's frame sizes -> each
//                      frame's offset, the 42 header bytes (STREAMINFO with the
//                      min / max frame size and the sample count), out_len
//   flac_pack_kernel   grid (frames, rows): copies a frame behind the header
//
// A frame in the workgroup: the block's samples sit in LDS as int16. Sum |r_o|
// of the five predictor orders are block sums (64-bit: 4096 * 2^19 = 2^31). For
// the finest partition order allowed, the 15 sums of (u >> k) of each partition
// are accumulated in LDS (64-bit: 4096 * 2^21); a coarser order's partitions
// are sums of two children, so the nine orders are priced by halving that
// table. With the order, the partition order and the parameters fixed, an
// exclusive scan of the code lengths gives every sample's bit offset, and each
// thread ORs its codes' stop bit and low bits into a zeroed LDS bit buffer
// (ds_or; the unary zeros are the zeroing). The CRC-16 is linear: every thread
// takes the CRC of its byte chunk, multiplies it by x^(8 * bytes after the
// chunk) modulo the polynomial, and the block XORs the products.
#include "common.h"

#define FL_THREADS 256
#define FL_MAX_BLOCK 4096
#define FL_HEADER 42                 // "fLaC", block header, STREAMINFO
#define FL_MAX_FRAMES 65536          // frame numbers of at most 3 coded bytes
#define FL_PARTS 256                 // partitions of the finest order (2^8)
#define FL_WORDS ((2 * FL_MAX_BLOCK + 15 + 3) / 4 + 2)   // bit buffer, 32-bit words

typedef unsigned long long u64;

__host__ __device__ inline long long fl_slot(int block) { return 2LL * block + 16; }

// residual of order o at sample i (i >= o), |r| <= 16 * 32768
__device__ __forceinline__ int fl_res(const int16_t* s, int i, int o) {
  const int a = s[i];
  if (o == 0) return a;
  const int b = s[i - 1];
  if (o == 1) return a - b;
  const int c = s[i - 2];
  if (o == 2) return a - 2 * b + c;
  const int d = s[i - 3];
  if (o == 3) return a - 3 * b + 3 * c - d;
  return a - 4 * b + 6 * c - 4 * d + s[i - 4];
}

__device__ __forceinline__ unsigned fl_fold(int r) {
  return r >= 0 ? (unsigned)r << 1 : ((unsigned)(-r) << 1) - 1u;
}

__device__ __forceinline__ u64 fl_block_sum(u64 v, u64* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 t = 0;
  for (int i = 0; i < FL_THREADS / 64; ++i) t += scratch[i];
  return t;
}

// exclusive prefix of v over the block; *total gets the block's sum
__device__ __forceinline__ unsigned fl_block_scan(unsigned v, unsigned* scratch, unsigned* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) scratch[wid] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int i = 0; i < FL_THREADS / 64; ++i) {
    if (i < wid) before += scratch[i];
    all += scratch[i];
  }
  *total = all;
  return before + inc - v;
}

// OR the low `width` (<= 16) bits of val into the bit buffer at bit `pos`
// (bit 0 = the MSB of byte 0; a word holds four stream bytes, first byte on top)
__device__ __forceinline__ void fl_put(unsigned* buf, unsigned pos, unsigned val, int width) {
  const unsigned w = pos >> 5;
  const int sh = 32 - (int)(pos & 31) - width;
  if (w >= FL_WORDS) return;
  if (sh >= 0) {
    atomicOr(buf + w, val << sh);
  } else {
    atomicOr(buf + w, val >> -sh);
    if (w + 1 < FL_WORDS) atomicOr(buf + w + 1, val << (32 + sh));
  }
}

__device__ __forceinline__ unsigned fl_byte(const unsigned* buf, int j) {
  return (buf[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu;
}

// a * b in GF(2)[x] modulo x^16 + x^15 + x^2 + 1
__device__ __forceinline__ unsigned fl_gfmul(unsigned a, unsigned b) {
  unsigned r = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    r ^= (b & 1u) ? a : 0u;
    b >>= 1;
    a <<= 1;
    if (a & 0x10000u) a ^= 0x18005u;
  }
  return r;
}

__device__ __forceinline__ long long fl_len(const void* lens, int is64, int b, long long N) {
  const long long n = is64 ? ((const long long*)lens)[b] : (long long)((const int*)lens)[b];
  return min(max(n, 0LL), N);
}

__device__ __forceinline__ int fl_rate_code(int rate) {
  switch (rate) {
    case 8000: return 4;
    case 16000: return 5;
    case 22050: return 6;
    case 24000: return 7;
    case 32000: return 8;
    case 44100: return 9;
    case 48000: return 10;
    default: return 13;              // the rate in Hz follows as 16 bits
  }
}

__global__ __launch_bounds__(FL_THREADS)
void flac_frame_kernel(const int16_t* __restrict__ pcm, long long ld, long long N,
                       const void* __restrict__ lens, int lens64, int rate, int block,
                       int block_code, int frames, uint8_t* __restrict__ staging,
                       int* __restrict__ sizes) {
  __shared__ int16_t s[FL_MAX_BLOCK];
  // the partition sums while the frame is planned, the bit buffer afterwards
  __shared__ u64 arena[FL_PARTS * 15];
  __shared__ uint8_t kall[2 * FL_PARTS];         // k of partition j of order p at 2^p - 1 + j
  __shared__ u64 red[FL_THREADS / 64];
  __shared__ unsigned sred[FL_THREADS / 64];
  __shared__ unsigned hdr[12];
  static_assert(sizeof(arena) >= FL_WORDS * 4, "bit buffer must fit the arena");
  u64* S = arena;
  unsigned* buf = (unsigned*)arena;

  const int tid = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  const long long len = fl_len(lens, lens64, b, N);
  const long long first = (long long)f * block;
  if (first >= len) return;                       // frames past the row write nothing
  const int n = (int)min((long long)block, len - first);
  const int16_t* x = pcm + (size_t)b * ld + first;
  for (int i = tid; i < n; i += FL_THREADS) s[i] = x[i];
  for (int i = tid; i < FL_PARTS * 15; i += FL_THREADS) S[i] = 0;
  __syncthreads();

  // the samples a thread owns: a contiguous run of c
  const int c = (n + FL_THREADS - 1) / FL_THREADS;
  const int i0 = min(tid * c, n), i1 = min(i0 + c, n);

  // ---- the plan: CONSTANT / order / partition order / parameters / VERBATIM
  const int s0 = s[0];
  u64 differ = 0;
  for (int i = i0; i < i1; ++i) differ += s[i] != s0;
  const bool constant = fl_block_sum(differ, red) == 0;

  int order = 0, porder = 0;
  u64 best_bits = 0;
  bool verbatim = false;
  if (!constant) {
    const int omax = min(4, n - 1);
    u64 e[5] = {0, 0, 0, 0, 0};
    for (int i = max(i0, omax); i < i1; ++i) {
#pragma unroll
      for (int o = 0; o < 5; ++o)
        if (o <= omax) e[o] += (u64)abs(fl_res(s, i, o));
    }
    u64 emin = 0;
#pragma unroll
    for (int o = 0; o < 5; ++o) {
      const u64 t = fl_block_sum(e[o], red);
      if (o <= omax && (o == 0 || t < emin)) { emin = t; order = o; }
    }
    // the finest partition order: 2^p divides n and n >> p > order, p <= 8
    int pmax = 0;
    while (pmax < 8 && !(n & ((2 << pmax) - 1)) && (n >> (pmax + 1)) > order) ++pmax;
    {
      const int psize = n >> pmax;
      u64 acc[15];
#pragma unroll
      for (int k = 0; k < 15; ++k) acc[k] = 0;
      int part = -1;
      for (int i = max(i0, order); i < i1; ++i) {
        const int pi = i / psize;
        if (pi != part) {
          if (part >= 0) {
#pragma unroll
            for (int k = 0; k < 15; ++k) atomicAdd(S + part * 15 + k, acc[k]);
          }
#pragma unroll
          for (int k = 0; k < 15; ++k) acc[k] = 0;
          part = pi;
        }
        const unsigned u = fl_fold(fl_res(s, i, order));
#pragma unroll
        for (int k = 0; k < 15; ++k) acc[k] += u >> k;
      }
      if (part >= 0) {
#pragma unroll
        for (int k = 0; k < 15; ++k) atomicAdd(S + part * 15 + k, acc[k]);
      }
    }
    __syncthreads();
    for (int p = pmax; p >= 0; --p) {
      const int parts = 1 << p;
      u64 cost = 0;
      if (tid < parts) {
        const u64 cnt = (u64)((n >> p) - (tid == 0 ? order : 0));
        int kb = 0;
        u64 cb = cnt + S[tid * 15];
#pragma unroll
        for (int k = 1; k < 15; ++k) {
          const u64 t = cnt * (u64)(k + 1) + S[tid * 15 + k];
          if (t < cb) { cb = t; kb = k; }
        }
        kall[parts - 1 + tid] = (uint8_t)kb;
        cost = 4 + cb;
      }
      const u64 bits = fl_block_sum(cost, red);
      if (p == pmax || bits <= best_bits) { best_bits = bits; porder = p; }   // the lowest p on ties
      if (p > 0) {                                 // the parents of this order's partitions
        u64 m[15];
        if (tid < parts / 2) {
#pragma unroll
          for (int k = 0; k < 15; ++k) m[k] = S[(2 * tid) * 15 + k] + S[(2 * tid + 1) * 15 + k];
        }
        __syncthreads();
        if (tid < parts / 2) {
#pragma unroll
          for (int k = 0; k < 15; ++k) S[tid * 15 + k] = m[k];
        }
        __syncthreads();
      }
    }
    verbatim = (u64)(16 * order + 6) + best_bits >= (u64)16 * n;
  }
  __syncthreads();                                  // the sums are dead: the arena becomes the bit buffer
  for (int i = tid; i < FL_WORDS; i += FL_THREADS) buf[i] = 0;

  // ---- the frame header, by one thread
  const bool full = n == block;
  const int num_bytes = f < 0x80 ? 1 : f < 0x800 ? 2 : 3;
  const int rate_code = fl_rate_code(rate);
  const int H = 4 + num_bytes + (full ? 0 : n <= 256 ? 1 : 2) + (rate_code == 13 ? 2 : 0) + 1;
  if (tid == 0) {
    int h = 0;
    hdr[h++] = 0xFF;
    hdr[h++] = 0xF8;
    hdr[h++] = (unsigned)((full ? block_code : n <= 256 ? 6 : 7) << 4 | rate_code);
    hdr[h++] = 0x08;                               // mono, 16 bits
    if (num_bytes == 1) {
      hdr[h++] = (unsigned)f;
    } else if (num_bytes == 2) {
      hdr[h++] = 0xC0u | (unsigned)(f >> 6);
      hdr[h++] = 0x80u | (unsigned)(f & 0x3F);
    } else {
      hdr[h++] = 0xE0u | (unsigned)(f >> 12);
      hdr[h++] = 0x80u | (unsigned)((f >> 6) & 0x3F);
      hdr[h++] = 0x80u | (unsigned)(f & 0x3F);
    }
    if (!full) {
      if (n > 256) hdr[h++] = (unsigned)((n - 1) >> 8);
      hdr[h++] = (unsigned)((n - 1) & 0xFF);
    }
    if (rate_code == 13) {
      hdr[h++] = (unsigned)(rate >> 8) & 0xFFu;
      hdr[h++] = (unsigned)rate & 0xFFu;
    }
    unsigned crc = 0;
    for (int j = 0; j < h; ++j) {
      crc ^= hdr[j];
      for (int t = 0; t < 8; ++t) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xFFu : crc << 1;
    }
    hdr[h++] = crc;
  }
  __syncthreads();                                  // buf zeroed, hdr written
  if (tid < H) fl_put(buf, 8u * tid, hdr[tid], 8);

  // ---- the subframe
  const unsigned body = 8u * H;
  unsigned end_bit;                                 // the frame's bits before padding
  if (constant) {
    if (tid == 0) fl_put(buf, body + 8, (unsigned)s0 & 0xFFFFu, 16);   // type 000000: the byte stays 0
    end_bit = body + 8 + 16;
  } else if (verbatim) {
    if (tid == 0) fl_put(buf, body, 0x02, 8);
    for (int i = i0; i < i1; ++i) fl_put(buf, body + 8 + 16u * i, (unsigned)s[i] & 0xFFFFu, 16);
    end_bit = body + 8 + 16u * n;
  } else {
    if (tid == 0) {
      fl_put(buf, body, (unsigned)(8 | order) << 1, 8);
      fl_put(buf, body + 8 + 16u * order, (unsigned)porder, 6);        // method 00, then the order
    }
    if (tid < order) fl_put(buf, body + 8 + 16u * tid, (unsigned)s[tid] & 0xFFFFu, 16);
    const int psize = n >> porder;
    const uint8_t* ks = kall + (1 << porder) - 1;
    unsigned mine = 0;
    for (int i = max(i0, order); i < i1; ++i) {
      const int part = i / psize;
      const int k = ks[part];
      if (i == max(order, part * psize)) mine += 4;
      mine += (fl_fold(fl_res(s, i, order)) >> k) + 1 + k;
    }
    unsigned total;
    unsigned pos = body + 8 + 16u * order + 6 + fl_block_scan(mine, sred, &total);
    for (int i = max(i0, order); i < i1; ++i) {
      const int part = i / psize;
      const int k = ks[part];
      if (i == max(order, part * psize)) {
        fl_put(buf, pos, (unsigned)k, 4);
        pos += 4;
      }
      const unsigned u = fl_fold(fl_res(s, i, order));
      const unsigned q = u >> k;
      fl_put(buf, pos + q, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
      pos += q + 1 + k;
    }
    end_bit = body + 8 + 16u * order + 6 + total;
  }
  __syncthreads();

  // ---- CRC-16 of the padded frame
  const int nbytes = (int)((end_bit + 7) >> 3);
  const int cb = (nbytes + FL_THREADS - 1) / FL_THREADS;
  const int b0 = min(tid * cb, nbytes), b1 = min(b0 + cb, nbytes);
  unsigned crc = 0;
  for (int j = b0; j < b1; ++j) {
    crc ^= fl_byte(buf, j) << 8;
#pragma unroll
    for (int t = 0; t < 8; ++t) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xFFFFu : crc << 1;
  }
  if (crc) {                                       // times x^(8 * bytes after the chunk)
    unsigned e = 8u * (unsigned)(nbytes - b1), pw = 1, sq = 2;
    while (e) {
      if (e & 1u) pw = fl_gfmul(pw, sq);
      sq = fl_gfmul(sq, sq);
      e >>= 1;
    }
    crc = fl_gfmul(crc, pw);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
  if ((tid & 63) == 0) sred[tid >> 6] = crc;
  __syncthreads();
  if (tid == 0) {
    crc = sred[0] ^ sred[1] ^ sred[2] ^ sred[3];
    fl_put(buf, 8u * nbytes, crc, 16);
    sizes[(size_t)b * frames + f] = nbytes + 2;
  }
  __syncthreads();

  // ---- to the staging slot, whole words (the slot is a multiple of 4 bytes)
  unsigned* dst = (unsigned*)(staging + ((size_t)b * frames + f) * fl_slot(block));
  const int words = (nbytes + 2 + 3) >> 2;
  for (int i = tid; i < words; i += FL_THREADS) dst[i] = __builtin_bswap32(buf[i]);
}

// One workgroup per row: offsets[b][f] = 42 + the bytes of the frames before f,
// the stream header, out_len.
__global__ __launch_bounds__(FL_THREADS)
void flac_scan_kernel(const void* __restrict__ lens, int lens64, long long N, int rate, int block,
                      int frames, const int* __restrict__ sizes, int* __restrict__ offsets,
                      uint8_t* __restrict__ out, long long cap, int* __restrict__ out_len) {
  __shared__ unsigned sred[FL_THREADS / 64];
  __shared__ unsigned smin[FL_THREADS / 64], smax[FL_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const long long len = fl_len(lens, lens64, b, N);
  const int nf = (int)((len + block - 1) / block);
  unsigned carry = 0, mn = 0xFFFFFFFFu, mx = 0;
  for (int base = 0; base < nf; base += FL_THREADS) {
    const int f = base + tid;
    const unsigned v = f < nf ? (unsigned)sizes[(size_t)b * frames + f] : 0u;
    if (f < nf) { mn = min(mn, v); mx = max(mx, v); }
    unsigned total;
    const unsigned ex = fl_block_scan(v, sred, &total);
    if (f < nf) offsets[(size_t)b * frames + f] = (int)(FL_HEADER + carry + ex);
    carry += total;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, (unsigned)__shfl_xor(mn, o, 64));
    mx = max(mx, (unsigned)__shfl_xor(mx, o, 64));
  }
  __syncthreads();
  if ((tid & 63) == 0) { smin[tid >> 6] = mn; smax[tid >> 6] = mx; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < FL_THREADS / 64; ++i) { mn = min(mn, smin[i]); mx = max(mx, smax[i]); }
    if (nf == 0) mn = 0;
    uint8_t* h = out + (size_t)b * cap;
    const uint8_t head[8] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34};
    for (int i = 0; i < 8; ++i) h[i] = head[i];
    h[8] = h[10] = (uint8_t)(block >> 8);
    h[9] = h[11] = (uint8_t)block;
    h[12] = (uint8_t)(mn >> 16); h[13] = (uint8_t)(mn >> 8); h[14] = (uint8_t)mn;
    h[15] = (uint8_t)(mx >> 16); h[16] = (uint8_t)(mx >> 8); h[17] = (uint8_t)mx;
    // 20 bits rate, 3 bits channels - 1, 5 bits (16 - 1), 36 bits samples
    const u64 v = (u64)rate << 44 | (u64)15 << 36 | (u64)len;
    for (int i = 0; i < 8; ++i) h[18 + i] = (uint8_t)(v >> (56 - 8 * i));
    for (int i = 0; i < 16; ++i) h[26 + i] = 0;   // MD5: not computed
    out_len[b] = (int)(FL_HEADER + carry);
  }
}

__global__ __launch_bounds__(FL_THREADS)
void flac_pack_kernel(const void* __restrict__ lens, int lens64, long long N, int block, int frames,
                      const uint8_t* __restrict__ staging, const int* __restrict__ sizes,
                      const int* __restrict__ offsets, uint8_t* __restrict__ out, long long cap) {
  const int f = blockIdx.x, b = blockIdx.y;
  if ((long long)f * block >= fl_len(lens, lens64, b, N)) return;
  const size_t slot = (size_t)b * frames + f;
  const uint8_t* src = staging + slot * fl_slot(block);
  uint8_t* dst = out + (size_t)b * cap + offsets[slot];
  const int bytes = sizes[slot];
  for (int i = threadIdx.x; i < bytes; i += FL_THREADS) dst[i] = src[i];
}

// pcm: int16 [R, N], row stride ld; lens [R] on the device (int32 / int64,
// clamped to [0, N]); out: uint8 [R, cap], cap >= 42 + frames * (2 block + 15);
// out_len: int32 [R]; staging: frames * R slots of 2 block + 16 bytes; sizes,
// offsets: int32 [R, frames]. Everything is checked before the first launch.
extern "C" int loqa_flac_encode(const void* pcm, long long ld, long long N, const void* lens,
                                int lens64, int R, int rate, int block, void* out, long long cap,
                                int* out_len, void* staging, int* sizes, int* offsets,
                                hipStream_t s) {
  if (R <= 0) return R < 0 ? (int)hipErrorInvalidValue : 0;
  int block_code = 0;
  for (int c = 8; c <= 12; ++c)
    if (block == (256 << (c - 8))) block_code = c;
  static const int rates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000};
  bool rate_ok = false;
  for (int r : rates) rate_ok |= r == rate;
  if (!block_code || !rate_ok || N < 0 || ld < N || R > 65535 || (!pcm && N > 0) || !lens || !out || !out_len)
    return (int)hipErrorInvalidValue;
  const long long frames = (N + block - 1) / block;
  if (frames > FL_MAX_FRAMES || cap < FL_HEADER + frames * (2LL * block + 15) || cap >= (1LL << 31))
    return (int)hipErrorInvalidValue;
  if (frames > 0) {
    if (!staging || !sizes || !offsets) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(flac_frame_kernel, dim3((unsigned)frames, R), dim3(FL_THREADS), 0, s,
                       (const int16_t*)pcm, ld, N, lens, lens64, rate, block, block_code,
                       (int)frames, (uint8_t*)staging, sizes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(flac_scan_kernel, dim3(R), dim3(FL_THREADS), 0, s, lens, lens64, N, rate,
                     block, (int)frames, sizes, offsets, (uint8_t*)out, cap, out_len);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || frames == 0) return (int)e;
  hipLaunchKernelGGL(flac_pack_kernel, dim3((unsigned)frames, R), dim3(FL_THREADS), 0, s, lens,
                     lens64, N, block, (int)frames, (const uint8_t*)staging, sizes, offsets,
                     (uint8_t*)out, cap);
  return (int)hipGetLastError();
}
