// Weight-streaming product for wide decode steps: Y[M, N] = X[M, K] W[N, K]^T with 17 <= M <= 64
// rows (one token per sequence at batch 17 .. 64; reference cullavo/arch_cullavo.py:605-636, every
// Linear of the cached forward). gemv.hip covers M <= 16; above it the products run on the training
// tiles' split-K route, which this kernel beats on some of the 7B products only (o and lm_head, gate|up at
// 17 rows: ops.WIDE_TILES_FASTER, DESIGN.md §5 "Wide decode steps"), so the decode step takes it as an opt-in.
//
// What changes against gemv_k is the X traffic. gemv_k loads one X fragment per W fragment and leaves
// X to L2; at M = 64 that is 4 bytes of X from L2 per byte of W from HBM. Here a wave holds RB 16-row
// weight blocks and MB = 2 or 4 16-row X blocks per 32-deep k-step: RB + MB fragment loads feed RB * MB
// v_mfma_f32_16x16x32_bf16, and the L2 reads per weight byte are MB / RB (1 at RB = MB). The price is
// workgroups: one per 16 RB weight rows, so the host picks RB per product (gemv_wide_rb below).
//
// Layout as gemv_k: W fragment = MFMA A operand (lane l: row n0 + 16 rb + (l & 15), 8 k at 8 (l >> 4)),
// X fragment = B operand (row 16 mb + (l & 15), zero for rows >= M), C^T[n][b] in the accumulators.
// The 8 waves of a workgroup split K into contiguous ranges of cdiv(cdiv(K, 32), 8) k-steps; the eight
// partials are summed through LDS in wave order. The order depends on K alone -- not on M, RB or MB --
// so row b of the result is bitwise the same whatever other rows are in the call. No atomics. The
// epilogue is store4 (gemm_common.h): bf16(bf16(bf16(acc) + addend) + residual), or f32 acc.
// OT 1 (x_transform 3): W holds the fused gate|up weight [2N, K]; each 16-row block is 8 gate rows and
// the matching 8 up rows, so the lane pair (l, l + 32) holds g and u of one output, as gemv_k's OT 1.
#include "gemm_common.h"

#include <cstdlib>

namespace {
using namespace cvgemm;

constexpr int kWideWaves = 8;

DEV float wide_silu(float x) { return x / (1.f + __expf(-x)); }  // gemv_silu / swiglu_fwd_k

template <int CT, int RB, int MB, int OT>
__global__ __launch_bounds__(64 * kWideWaves) void gemv_wide_k(GemmArgs p) {
  static_assert(OT == 0 || CT == CULLAVO_DT_BF16, "SwiGLU output: bf16");
  constexpr int NW = kWideWaves;
  constexpr int NB = RB == 4 ? 2 : 4;  // k-steps per batch of loads: NB (RB + MB) fragments in flight
  __shared__ f32x4 red[NW][MB][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * (OT == 1 ? 8 * RB : 16 * RB);
  const int64_t nk = cdiv(p.K, 32);
  const int64_t per = cdiv(nk, NW);
  const u16* wrow[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int64_t row = OT == 1 ? min(n0 + 8 * rb + (r & 7), p.N - 1) + (r >= 8 ? p.N : 0)
                                : min(n0 + 16 * rb + r, p.N - 1);
    wrow[rb] = p.B + row * p.ldb + 8 * g;
  }
  const u16* xrow[MB];
  bool xin[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    xin[mb] = 16 * mb + r < p.M;
    xrow[mb] = p.A + (xin[mb] ? 16 * mb + r : 0) * p.lda + 8 * g;
  }
  f32x4 acc[RB][MB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[rb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ks0 = wave * per, kend = min(nk, ks0 + per);
  // a batch of NB k-steps' loads goes out before any MFMA consumes it. A ring that kept later steps'
  // loads in flight under the MFMAs (124-228 VGPRs against 74-156) measured 5-21 % slower on most of the 7B
  // products (profiles/r21/wide_decode/README_r21_wide.txt); why was not looked into
  for (int64_t j0 = ks0; j0 < kend; j0 += NB) {
    frag8 w[NB][RB], x[NB][MB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int64_t ks = j0 + i;
      const bool in = ks < kend && ks * 32 + 8 * g < p.K;  // this lane's 8 k of the step
      const int64_t off = in ? ks * 32 : 0;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
        w[i][rb] = in ? __builtin_bit_cast(frag8, *reinterpret_cast<const u16x8*>(wrow[rb] + off)) : frag8{};
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int64_t ks = j0 + i;
      const bool in = ks < kend && ks * 32 + 8 * g < p.K;
      const int64_t off = in ? ks * 32 : 0;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        x[i][mb] = (in && xin[mb]) ? __builtin_bit_cast(frag8, *reinterpret_cast<const u16x8*>(xrow[mb] + off)) : frag8{};
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
          acc[rb][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[i][rb], x[i][mb], acc[rb][mb], 0, 0, 0);
  }
  // one pass per weight block: the waves' partials of its MB tiles through LDS, wave mb sums tile mb
  // in wave order and stores rows 16 mb + r
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    if (rb > 0) __syncthreads();  // the previous pass's reads
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) red[wave][mb][lane] = acc[rb][mb];
    __syncthreads();
    if (wave < MB) {
      f32x4 s = red[0][wave][lane];
#pragma unroll
      for (int w2 = 1; w2 < NW; ++w2) s += red[w2][wave][lane];
      const int64_t m = 16 * wave + r;
      if constexpr (OT == 1) {
        // lanes 0-31 hold g of outputs n0 + 8 rb + 4 (lane >> 4) + j, lanes 32-63 the matching u
        f32x4 u;
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = __shfl_xor(s[j], 32);
        const int64_t n = n0 + 8 * rb + 4 * g;
        if (g < 2 && m < p.M && n < p.N) {
          u16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = f2bf(round_bf(wide_silu(round_bf(s[j]))) * round_bf(u[j]));
          *reinterpret_cast<u16x4*>(reinterpret_cast<u16*>(p.C) + m * p.ldc + n) = o;
        }
      } else {
        store4<CT>(p, s, m, n0 + 16 * rb + 4 * g);
      }
    }
  }
}

// Weight blocks per workgroup for a product of `rows` weight rows at MB X blocks. RB = MB reads one
// byte of X from L2 per weight byte; a smaller RB reads MB / RB but keeps more workgroups streaming,
// and on the 7B products the workgroups decided (profiles/r21/wide_decode/products_rb*.txt): the
// N = 4096 products ran 1.7-2.5x faster at RB 1 (256 workgroups) than at RB 4 (64), lm_head
// (501 workgroups at RB 4) 10-35 % faster at RB 4 than at RB 2. So: RB 4 for the widest weights, else
// RB = MB, halved until the grid has a workgroup per CU.
// CULLAVO_GEMV_WIDE_RB (1, 2, 4) is the lab switch (tools/wide_decode_bench.py --rb), read once.
int gemv_wide_rb(int64_t rows, int mb) {
  static const int venv = getenv("CULLAVO_GEMV_WIDE_RB") ? atoi(getenv("CULLAVO_GEMV_WIDE_RB")) : 0;
  if (venv == 1 || venv == 2 || venv == 4) return venv;
  int rb = rows >= 24576 ? 4 : mb;
  while (rb > 1 && cdiv(rows, 16 * rb) < 256) rb /= 2;
  return rb;
}

}  // namespace

extern "C" int cullavo_decode_linear_wide(int x_transform, int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx,
                                          const void* W, int64_t ldw, void* y, int64_t ldy, int y_dtype,
                                          const void* addend, int64_t ld_addend, const void* residual, int64_t ldr,
                                          void* stream) {
  CV_REQUIRE(x_transform == 0 || x_transform == 3, CULLAVO_EINVAL,
             "decode_linear_wide: transform 0 or 3 (1, 2 and 4 are cullavo_decode_linear's, M <= 16)");
  const bool ot = x_transform == 3;
  const bool f32 = y_dtype == CULLAVO_DT_F32;
  CV_REQUIRE(y_dtype == CULLAVO_DT_BF16 || (f32 && !ot), CULLAVO_EINVAL,
             "decode_linear_wide: y is bf16, or f32 with transform 0");
  CV_REQUIRE(!ot || (residual == nullptr && addend == nullptr), CULLAVO_EINVAL,
             "decode_linear_wide: the SwiGLU output takes no residual and no addend");
  CV_REQUIRE(M >= 17 && M <= 64, CULLAVO_EINVAL,
             "decode_linear_wide: 17 <= M <= 64 rows (M <= 16: cullavo_decode_linear)");
  CV_REQUIRE(N > 0 && K > 0, CULLAVO_EINVAL, "decode_linear_wide: N, K > 0");
  CV_REQUIRE(N % 8 == 0 && K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldy % 8 == 0 &&
                 (residual == nullptr || ldr % 8 == 0) && (addend == nullptr || ld_addend % 4 == 0),
             CULLAVO_EINVAL, "decode_linear_wide: sizes and strides must be multiples of 8 (ld_addend: 4)");
  CV_REQUIRE(ldw >= K && ldy >= N && ldx >= K && (residual == nullptr || ldr >= N) &&
                 (addend == nullptr || ld_addend >= N),
             CULLAVO_EINVAL, "decode_linear_wide: leading dimension too small");
  CV_REQUIRE(x != nullptr && W != nullptr && y != nullptr, CULLAVO_EINVAL, "decode_linear_wide: null x, W or y");
  CV_REQUIRE((((uintptr_t)x | (uintptr_t)W | (uintptr_t)y | (uintptr_t)addend | (uintptr_t)residual) & 15) == 0,
             CULLAVO_EINVAL, "decode_linear_wide: pointers must be 16-byte aligned");
  hipStream_t s = CV_STREAM(stream);
  GemmArgs p{};
  p.A = (const u16*)x;
  p.B = (const u16*)W;
  p.C = y;
  p.addend = (const u16*)addend;
  p.ld_add = ld_addend;
  p.residual = (const u16*)residual;
  p.M = M; p.N = N; p.K = K; p.lda = ldx; p.ldb = ldw; p.ldc = ldy; p.ldr = ldr;
  p.alpha = 1.f;
  p.beta = 0.f;
  p.act = CULLAVO_ACT_NONE;
  const int mb = M <= 32 ? 2 : 4;
  const int rb = gemv_wide_rb(ot ? 2 * N : N, mb);
  const unsigned grid = (unsigned)cdiv(N, (ot ? 8 : 16) * rb);
#define WK(RB, MB)                                                                                 \
  if (ot) gemv_wide_k<CULLAVO_DT_BF16, RB, MB, 1><<<grid, 64 * kWideWaves, 0, s>>>(p);              \
  else if (f32) gemv_wide_k<CULLAVO_DT_F32, RB, MB, 0><<<grid, 64 * kWideWaves, 0, s>>>(p);         \
  else gemv_wide_k<CULLAVO_DT_BF16, RB, MB, 0><<<grid, 64 * kWideWaves, 0, s>>>(p);
#define WR(MB) \
  if (rb == 4) { WK(4, MB) } else if (rb == 2) { WK(2, MB) } else { WK(1, MB) }
  if (mb == 2) { WR(2) } else { WR(4) }
#undef WR
#undef WK
  return cullavo_check_launch("decode_linear_wide");
}
