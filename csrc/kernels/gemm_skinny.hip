// Decode-shaped GEMM entry points and the bf16 weight stream's kernel
// instances (kernels and launch templates: gemm_skinny.h; the fp8 weight
// stream's instances: gemm_skinny_fp8.hip; the MXFP4 one's: gemm_skinny_mxfp4.hip).
#include "gemm_skinny.h"

// x: [Mpad, >=K] bf16 (row stride ldx), rows >= M must be finite (zeros);
// Wp: pre-shuffled weight (loqa_shuffle_weight); part: [S, Mpad, N] f32.
// max_wgs > 0 caps the grid (workgroups loop over tile groups).
extern "C" int loqa_skinny_gemm(const void* x, long long ldx_, const void* Wp, float* part, int Mpad,
                                int N, int K, int S, int max_wgs, hipStream_t st) {
  if (S < 1 || K % (S * 4 * 32) != 0 || ldx_ % 8 != 0 || N % 16 != 0) return (int)hipErrorInvalidValue;
  return dispatch_skinny<bf16_t>(SkinnyArgs{x, ldx_, Wp, nullptr, part, N, K, S, Mpad, max_wgs}, st);
}

// W [N, K] row-major -> Wp[N/16][K/32][64][8] (fragment order of the kernel above)
__global__ void shuffle_weight_kernel(const bf16_t* __restrict__ W, bf16_t* __restrict__ Wp, int N,
                                      int K, long long total_vec) {
  const int KS = K >> 5;
  for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < total_vec;
       v += (long long)gridDim.x * blockDim.x) {
    // destination vector v -> (tile, ks, lane)
    const int lane = (int)(v & 63);
    const long long tk = v >> 6;
    const int ks = (int)(tk % KS);
    const long long t = tk / KS;
    const long long row = t * 16 + (lane & 15);
    const int k = ks * 32 + 8 * (lane >> 4);
    *reinterpret_cast<uint4*>(Wp + v * 8) = *reinterpret_cast<const uint4*>(W + row * K + k);
  }
}

extern "C" int loqa_shuffle_weight(const void* W, void* Wp, int N, int K, hipStream_t st) {
  if (N % 16 || K % 32) return (int)hipErrorInvalidValue;
  const long long tv = (long long)N * K / 8;
  long long blocks = (tv + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(shuffle_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                     (const bf16_t*)W, (bf16_t*)Wp, N, K, tv);
  return (int)hipGetLastError();
}

// the ctypes mirror is held to these two (tests/test_gemm_shared.py): the size,
// and the offset of every field in declaration order (returns the field count;
// writes at most cap offsets)
extern "C" int loqa_skinny_fused_params_size() { return (int)sizeof(FusedParams); }

extern "C" int loqa_skinny_fused_params_offsets(int* out, int cap) {
#define F(f) (int)offsetof(FusedParams, f)
  const int off[] = {F(x), F(ldx), F(Wp), F(part), F(counters), F(Mpad), F(N), F(K), F(S), F(mode),
                     F(norm), F(rowsq_in), F(rowsum_in), F(rowstat_tiles), F(eps), F(colsum), F(bias),
                     F(out), F(ldo), F(act), F(residual), F(rowsq_out), F(rowsum_out), F(positions),
                     F(cs), F(q_out), F(kc), F(vc), F(slots), F(H), F(Hkv), F(D), F(blk), F(rt), F(wr),
                     F(xl), F(wdtype), F(wscale)};
#undef F
  const int n = (int)(sizeof(off) / sizeof(off[0]));
  for (int i = 0; i < n && i < cap; ++i) out[i] = off[i];
  return n;
}

// The kernel argument of a checked parameter block. (FusedArgs' field order is
// the kernel-argument layout the kernels were measured with: it stays.)
static FusedArgs fused_args(const FusedParams& p) {
  FusedArgs a{};
  a.x = (const bf16_t*)p.x, a.ldx = p.ldx, a.Wp = (const bf16_t*)p.Wp, a.wscale = p.wscale;
  a.part = p.part, a.counters = p.counters;
  a.N = p.N, a.K = p.K, a.S = p.S, a.Mpad = p.Mpad;
  a.rowsq_in = p.rowsq_in, a.rowsum_in = p.rowsum_in, a.rowstat_tiles = p.rowstat_tiles, a.eps = p.eps;
  a.colsum = p.colsum, a.bias = p.bias;
  a.out = (bf16_t*)p.out, a.ldo = p.ldo, a.act = p.act;
  a.residual = (bf16_t*)p.residual, a.rowsq_out = p.rowsq_out, a.rowsum_out = p.rowsum_out;
  a.positions = p.positions, a.cs = (const float2*)p.cs, a.slots = p.slots;
  a.q_out = (bf16_t*)p.q_out, a.kc = (bf16_t*)p.kc, a.vc = (bf16_t*)p.vc;
  a.H = p.H, a.Hkv = p.Hkv, a.D = p.D, a.blk = p.blk;
  a.prio = g_loqa_launch_prio;
  return a;
}

// the fp8 weight stream's instances (gemm_skinny_fp8.hip)
int loqa_skinny_fused_fp8_launch(const FusedArgs& a, int mode, int norm, int rt, int wr, int xl,
                                 hipStream_t st);
// the MXFP4 weight stream's instances (gemm_skinny_mxfp4.hip)
int loqa_skinny_fused_mxfp4_launch(const FusedArgs& a, int mode, int norm, int rt, int wr, int xl,
                                   hipStream_t st);

// mode: 1 silu (out [Mpad, ldo >= N/2]), 2 residual (+bias) + row sum-of-squares
// (+ row sums), 3 (RoPE if cs) + paged KV append + q, 4 act(bias + x W^T) -> out
// (act 0 identity, 1 GELU-erf). norm: 1 RMSNorm / 2 LayerNorm of x (the bf16
// residual) with the norm weight folded into Wp; the row statistics come from
// rowstat_tiles partial sums. part: S * Mpad * N f32 scratch (S > 1,
// tile-contiguous slabs); counters: >= N/(16*rt) zeroed ints. Row statistics of
// the residual epilogue are written per (16*rt)-row tile.
// wdtype 1: Wp holds e4m3fn bytes in the fp8 fragment order with the per-row
// scale wscale; no LayerNorm, and every wave's k range must be a whole number
// of 64-wide k-step pairs (K % (S * waves-along-K * 64) == 0).
// wdtype 2: Wp holds MXFP4 nibble bytes in their fragment order and wscale the
// e8m0 scale bytes (one per row and k-step); no LayerNorm, and every wave's k
// range must be a whole number of 128-wide loads
// (K % (S * waves-along-K * 128) == 0).
extern "C" int loqa_skinny_fused(const FusedParams* p, hipStream_t st) {
  const int Mpad = p->Mpad, N = p->N, K = p->K, S = p->S;
  if (S < 1 || K % (S * 128) || p->ldx % 8 || N % 32 ||
      (Mpad != 16 && Mpad != 32 && Mpad != 64 && !(Mpad == 128 && p->xl)))
    return (int)hipErrorInvalidValue;
  if (p->xl && (p->wr != 4 || Mpad < 32 || (p->rt != 1 && p->rt != 2) || N % (64 * p->rt)))
    return (int)hipErrorInvalidValue;
  if (S > 1 && (!p->part || !p->counters)) return (int)hipErrorInvalidValue;
  if (p->norm && (!p->rowsq_in || p->rowstat_tiles < 1)) return (int)hipErrorInvalidValue;
  if (p->norm == NORM_LN && (!p->rowsum_in || !p->colsum)) return (int)hipErrorInvalidValue;
  if (p->mode == FEPI_ROPE && (p->D % 16 || N != (p->H + 2 * p->Hkv) * p->D))
    return (int)hipErrorInvalidValue;
  if ((p->mode == FEPI_SILU || p->mode == FEPI_ACT) && (!p->out || p->ldo % 4))
    return (int)hipErrorInvalidValue;
  if (p->rt != 1 && p->rt != 2 && !(p->rt == 4 && Mpad == 64)) return (int)hipErrorInvalidValue;
  if (p->mode == FEPI_RESID && (!p->residual || !p->rowsq_out)) return (int)hipErrorInvalidValue;
  if (p->wr != 1 && (p->wr != 4 || (S != 1 && !p->xl) || N % (64 * p->rt)))
    return (int)hipErrorInvalidValue;
  if (p->wdtype < 0 || p->wdtype > 2) return (int)hipErrorInvalidValue;
  if (p->wdtype == 2 &&
      (!p->wscale || p->norm == NORM_LN || K % (S * (p->wr == 4 ? 1 : 4) * 128)))
    return (int)hipErrorInvalidValue;
  if (p->wdtype == 1 &&
      (!p->wscale || p->norm == NORM_LN || K % (S * (p->wr == 4 ? 1 : 4) * 64)))
    return (int)hipErrorInvalidValue;
  const FusedArgs a = fused_args(*p);
  if (p->wdtype == 1)
    return loqa_skinny_fused_fp8_launch(a, p->mode, p->norm, p->rt, p->wr, p->xl, st);
  if (p->wdtype == 2)
    return loqa_skinny_fused_mxfp4_launch(a, p->mode, p->norm, p->rt, p->wr, p->xl, st);
  return dispatch_mode<0>(a, p->mode, p->norm, p->rt, p->wr, p->xl, st);
}
