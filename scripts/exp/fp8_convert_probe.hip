// Both fp8 (OCP e4m3fn) -> bf16 conversion sequences the decode GEMMs could use,
// run on all 256 byte values and checked against the format's table on the
// host: v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (the one gemm_skinny.h uses) and
// v_cvt_pk_f32_fp8 + v_perm_b32.
//   hipcc --offload-arch=gfx950 -O2 fp8_convert_probe.hip -o fp8_convert_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <cstring>
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
__global__ void k(unsigned* outA, unsigned* outB) {
  unsigned t = threadIdx.x;           // byte value
  unsigned v = t | (t << 8) | (t << 16) | (t << 24);
  bf2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, false);
  bf2 a2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, true);
  f2 c = __builtin_amdgcn_cvt_pk_f32_fp8(v, false);
  f2 d = __builtin_amdgcn_cvt_pk_f32_fp8(v, true);
  outA[2 * t] = __builtin_bit_cast(unsigned, a);
  outA[2 * t + 1] = __builtin_bit_cast(unsigned, a2);
  outB[2 * t] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, c.y), __builtin_bit_cast(unsigned, c.x), 0x07060302);
  outB[2 * t + 1] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, d.y), __builtin_bit_cast(unsigned, d.x), 0x07060302);
}
static float dec(unsigned b) {  // OCP e4m3fn
  int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
  float v;
  if (e == 15 && m == 7) v = NAN;
  else if (e == 0) v = ldexpf((float)m, -9);
  else v = ldexpf(1.f + m / 8.f, e - 7);
  return s ? -v : v;
}
int main() {
  unsigned *A, *B, hA[512], hB[512];
  if (hipMalloc(&A, 2048) || hipMalloc(&B, 2048)) return 2;
  hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, 0, A, B);
  if (hipDeviceSynchronize()) return 3;
  hipMemcpy(hA, A, 2048, hipMemcpyDeviceToHost); hipMemcpy(hB, B, 2048, hipMemcpyDeviceToHost);
  int badA = 0, badB = 0;
  for (unsigned t = 0; t < 256; ++t) {
    float f = dec(t); unsigned u; memcpy(&u, &f, 4); unsigned want = (u >> 16) * 0x10001u;
    bool nan = std::isnan(f);
    for (int h = 0; h < 2; ++h) {
      unsigned ga = hA[2 * t + h], gb = hB[2 * t + h];
      bool okA = nan ? ((ga & 0x7f80) == 0x7f80 && (ga & 0x7f)) : ga == want;
      bool okB = nan ? ((gb & 0x7f80) == 0x7f80 && (gb & 0x7f)) : gb == want;
      if (!okA) { if (badA++ < 8) printf("A byte %02x h%d got %08x want %08x\n", t, h, ga, want); }
      if (!okB) { if (badB++ < 8) printf("B byte %02x h%d got %08x want %08x\n", t, h, gb, want); }
    }
  }
  printf("scalef32_pk_bf16_fp8 mismatches %d ; cvt_pk_f32_fp8+perm mismatches %d\n", badA, badB);
  return 0;
}
