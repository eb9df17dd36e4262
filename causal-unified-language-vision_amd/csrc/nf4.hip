// NF4 (QLoRA's 4-bit NormalFloat) base weights for the LM's decoder layers (reference
// cullavo/load_cullavo.py:66-83: every decoder-layer Linear is bitsandbytes NF4 with bf16 compute;
// lm_head and the projector stay bf16) and the decode step's weight-streaming product on them.
//
// Format (INTEGRATION.md "NF4"): blocks of 64 consecutive k of one weight row; absmax f32 [N, K/64]
// = max |w| of the block; code = the number of code-book midpoints below w / absmax; two codes per
// byte, row-major [N, K/2], element 2i in the high nibble (bitsandbytes' order); dequantised value
// bf16(L[code] * absmax). No double quantisation.
//
// Decode product (nf4_gemv_k): gemv.hip's structure -- one workgroup per 16 weight rows, the waves
// split K, partials summed through LDS in a fixed wave order, store4's epilogue -- on 4.5 bits per
// weight instead of 16. What makes the unpacking fit beside the stream:
//  * the weights are never multiplied by absmax. A lane's 8-byte load is 16 consecutive k of one
//    row and the four lane groups take the four 16-k quarters of one 64-block, so the block's MFMAs
//    see that block alone; they accumulate code-book values into a scratch tile and the block costs
//    four FMAs per lane, acc += absmax * scratch. W is the MFMA's B operand (X the A operand): the
//    output tile's column, hence the lane, is then the weight row the lane loaded, and the scale is
//    ONE register per lane and block, loaded by the lane itself (as the A operand the rows would lie
//    in the four accumulator registers: four scales per lane, fetched across lanes);
//  * code -> bf16 by one 8-byte LDS read per code BYTE: a 256-entry table of both codes' values.
//    The code book is not representable in bf16 (7 mantissa bits against L's 24), so an entry holds
//    hi = bf16(L) and lo = bf16(L - hi) of both codes, L = hi + lo to 2^-18 relative, and the
//    MFMA's 32 k-slots take 8 k as {hi pair, lo pair} x 4 bytes with the X pair repeated: four
//    MFMAs per block (the matrix pipe is idle next to this stream), no per-element VALU.
#include "gemm_common.h"

#include <cstdlib>

namespace {
using namespace cvgemm;

__constant__ float kNf4[16] = {-1.0f,
                               -0.6961928009986877f,
                               -0.5250730514526367f,
                               -0.39491748809814453f,
                               -0.28444138169288635f,
                               -0.18477343022823334f,
                               -0.09105003625154495f,
                               0.0f,
                               0.07958029955625534f,
                               0.16093020141124725f,
                               0.24611230194568634f,
                               0.33791524171829224f,
                               0.44070982933044434f,
                               0.5626170039176941f,
                               0.7229568362236023f,
                               1.0f};

// ---- quantise -----------------------------------------------------------------------------------
// one pass over W: a lane reads 16 B (8 weights), 8 lanes one block, a wave 8 consecutive blocks;
// the block maximum by three xor-shuffles inside the 8-lane group
__global__ __launch_bounds__(256) void nf4_quantize_k(const u16* __restrict__ W, int64_t ldw, int64_t N, int64_t K,
                                                      uint8_t* __restrict__ codes, float* __restrict__ absmax) {
  __shared__ float mid[16];
  if (threadIdx.x < 15) mid[threadIdx.x] = (kNf4[threadIdx.x] + kNf4[threadIdx.x + 1]) * 0.5f;
  __syncthreads();
  const int64_t nblk = K / 64;
  const int64_t gb = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;  // global block index
  const int sub = threadIdx.x & 7;
  const bool in = gb < N * nblk;
  const int64_t row = in ? gb / nblk : 0, blk = in ? gb - row * nblk : 0;
  float v[8];
  if (in) {
    load8(W + row * ldw + blk * 64 + sub * 8, v);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
  }
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
#pragma unroll
  for (int o = 4; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (!in) return;
  unsigned packed = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned c = 7;  // an all-zero block
    if (m != 0.f) {
      const float x = v[j] / m;  // IEEE division
      c = 0;
#pragma unroll
      for (int t = 0; t < 15; ++t) c += x > mid[t] ? 1u : 0u;
    }
    // byte j / 2 of the dword: the even element in the high nibble
    packed |= c << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
  }
  *reinterpret_cast<unsigned*>(codes + row * (K / 2) + blk * 32 + sub * 4) = packed;
  if (sub == 0) absmax[row * nblk + blk] = m;
}

// ---- dequantise ---------------------------------------------------------------------------------
// a lane reads 4 code bytes and writes 8 weights (16 B)
__global__ __launch_bounds__(256) void nf4_dequantize_k(const uint8_t* __restrict__ codes, const float* __restrict__ absmax,
                                                        int64_t N, int64_t K, u16* __restrict__ W, int64_t ldw) {
  __shared__ float book[16];
  if (threadIdx.x < 16) book[threadIdx.x] = kNf4[threadIdx.x];
  __syncthreads();
  const int64_t cpr = K / 8;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= N * cpr) return;
  const int64_t row = q / cpr, c = q - row * cpr;
  const unsigned packed = *reinterpret_cast<const unsigned*>(codes + row * (K / 2) + c * 4);
  const float am = absmax[row * (K / 64) + (c >> 3)];
  u16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned code = (packed >> (8 * (j >> 1) + ((j & 1) ? 0 : 4))) & 15u;
    o[j] = f2bf(book[code] * am);
  }
  *reinterpret_cast<u16x8*>(W + row * ldw + c * 8) = o;
}

// ---- decode product -----------------------------------------------------------------------------
constexpr int kNf4Waves = 8;        // waves per workgroup, K <= 8192
constexpr int kNf4WavesLongK = 16;  // K > 8192 (down_proj)
DEV float nf4_silu(float x) { return x / (1.f + __expf(-x)); }  // gemv.hip gemv_silu

DEV unsigned nf4_pair(float a, float b) { return (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16); }

// NW: waves per workgroup (K split NW ways, contiguous block ranges); NB: 64-blocks per load batch
// and wave (NB x 512 B of codes in flight per wave); OT 1: SwiGLU of the product (gemv.hip OT 1: 8
// gate rows and the matching 8 up rows of the fused [2N, K] weight per workgroup)
// LORA (cullavo_nf4_decode_linear_lora): gemv.hip's fused LoRA term. Wave 0, which writes the tile,
// loads its 16 lora_B rows and the u rows ahead of the code stream and runs the term's two MFMA
// k-steps (lora_term, gemm_common.h) under the first batch; lora_B rows are that MFMA's A operand, so
// lane (r, g) gets t of decode row r and weight rows 4 g .. 4 g + 3, the layout of the reduced tile.
// OT 1: a second fragment set holds the up rows' lora_B (module 1) in tile rows 0-7, so the gate and
// up terms of one output meet in one lane as the reduced g and u do. false: today's kernels.
template <int NW, int NB, int OT, bool LORA = false>
__global__ __launch_bounds__(64 * NW) void nf4_gemv_k(GemmArgs p, const uint8_t* __restrict__ codes,
                                                       const float* __restrict__ absmax) {
  __shared__ u32x2 table[256];  // code byte -> {hi pair, lo pair}; the even element (high nibble) first
  __shared__ __attribute__((aligned(16))) float red[NW][16][16];  // [wave][x row b][weight row c]
  for (int i = threadIdx.x; i < 256; i += 64 * NW) {
    const float a = kNf4[i >> 4], b = kNf4[i & 15];
    const float ah = round_bf(a), bh = round_bf(b);
    table[i] = u32x2{nf4_pair(ah, bh), nf4_pair(a - ah, b - bh)};
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * (OT == 1 ? 8 : 16);
  const int64_t nblk = p.K / 64;
  const int64_t per = cdiv(nblk, NW);
  // this lane's weight row (clamped: the rows past N of a tail workgroup are computed and dropped)
  const int64_t wr = OT == 1 ? min(n0 + (r & 7), p.N - 1) + (r >= 8 ? p.N : 0) : min(n0 + r, p.N - 1);
  const uint8_t* crow = codes + wr * (p.K / 2) + 8 * g;
  const float* arow = absmax + wr * nblk;
  const bool xrow = r < p.M;
  const u16* xp = p.A + (xrow ? r : 0) * p.lda + 16 * g;
  // LORA: wave 0's lora_B and u fragments (OT 1: lb2 / lu2 the up rows' module), and the terms
  frag8 lb[2], lu[2], lb2[2], lu2[2];
  f32x4 lt = {0.f, 0.f, 0.f, 0.f}, lt2 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (LORA) {
    if (wave == 0) {
      const int64_t brow = OT == 1 ? min(n0 + (r & 7), p.N - 1) : min(n0 + r, p.N - 1);
      const u16* up = xrow ? p.lora_u + r * p.ld_lu + (OT == 1 ? 0 : (n0 / p.lora_out) * 64) : nullptr;
      lora_frags(p.lora_b + brow * 64, up, g, lb, lu);
      if constexpr (OT == 1) lora_frags(p.lora_b + (brow + p.N) * 64, xrow ? up + 64 : nullptr, g, lb2, lu2);
    }
  }
  __syncthreads();  // the table
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int64_t b0 = wave * per, bend = min(nblk, b0 + per);
  for (int64_t j0 = b0; j0 < bend; j0 += NB) {
    u32x2 w[NB];
    float am[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const bool in = j0 + i < bend;
      const int64_t blk = in ? j0 + i : b0;
      w[i] = in ? __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(crow + blk * 32)) : u32x2{0u, 0u};
      am[i] = in ? arow[blk] : 0.f;
    }
    if constexpr (LORA) {
      if (wave == 0 && j0 == 0) {  // the adapters' term, under the first code batch's latency
        lt = lora_term(lb, lu, p.lora_scale);
        if constexpr (OT == 1) lt2 = lora_term(lb2, lu2, p.lora_scale);
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const bool in = j0 + i < bend;
      const int64_t blk = in ? j0 + i : b0;
      u32x4 x0 = {0u, 0u, 0u, 0u}, x1 = {0u, 0u, 0u, 0u};
      if (in && xrow) {
        x0 = *reinterpret_cast<const u32x4*>(xp + blk * 64);
        x1 = *reinterpret_cast<const u32x4*>(xp + blk * 64 + 8);
      }
      const unsigned xd[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        // code bytes 2m, 2m + 1 of the lane's 8: k = 64 blk + 16 g + 4 m .. + 3
        const unsigned d = w[i][m >> 1] >> (16 * (m & 1));
        const u32x2 e0 = table[d & 255u], e1 = table[(d >> 8) & 255u];
        const u32x4 wf = {e0[0], e0[1], e1[0], e1[1]};
        const u32x4 xf = {xd[2 * m], xd[2 * m], xd[2 * m + 1], xd[2 * m + 1]};
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(frag8, xf), __builtin_bit_cast(frag8, wf), s, 0,
                                                    0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += am[i] * s[j];
    }
  }
  // lane (r, g) holds C[x row 4 g + j][weight row r]
#pragma unroll
  for (int j = 0; j < 4; ++j) red[wave][4 * g + j][r] = acc[j];
  __syncthreads();
  if (wave == 0) {
    // lane: x row r, weight rows 4 g .. 4 g + 3 (store4's four consecutive columns)
    f32x4 s = *reinterpret_cast<const f32x4*>(&red[0][r][4 * g]);
#pragma unroll
    for (int w2 = 1; w2 < NW; ++w2) s += *reinterpret_cast<const f32x4*>(&red[w2][r][4 * g]);
    if constexpr (OT == 1) {
      // columns 0-7 of the tile are gate rows n0 .., columns 8-15 the matching up rows
      if (g < 2 && r < p.M) {
        f32x4 u = *reinterpret_cast<const f32x4*>(&red[0][r][8 + 4 * g]);
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) u += *reinterpret_cast<const f32x4*>(&red[w2][r][8 + 4 * g]);
        if constexpr (LORA) {  // g and u as the unfused product stores them with its addend
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s[j] = round_bf(round_bf(s[j]) + lt[j]);
            u[j] = round_bf(round_bf(u[j]) + lt2[j]);
          }
        }
        u16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = f2bf(round_bf(nf4_silu(round_bf(s[j]))) * round_bf(u[j]));
        *reinterpret_cast<u16x4*>(reinterpret_cast<u16*>(p.C) + r * p.ldc + n0 + 4 * g) = o;
      }
    } else if constexpr (LORA) {
      store4_lora(p, s, lt, r, n0 + 4 * g);
    } else {
      store4<CULLAVO_DT_BF16>(p, s, r, n0 + 4 * g);
    }
  }
}

}  // namespace

extern "C" int cullavo_nf4_quantize(int64_t N, int64_t K, const void* W, int64_t ldw, void* codes, void* absmax,
                                    void* stream) {
  CV_REQUIRE(N > 0 && K > 0 && K % 64 == 0, CULLAVO_EINVAL, "nf4_quantize: N > 0 and K a positive multiple of 64");
  CV_REQUIRE(ldw >= K && ldw % 8 == 0, CULLAVO_EINVAL, "nf4_quantize: ldw >= K and a multiple of 8");
  CV_REQUIRE(N * (K / 64) <= ((int64_t)1 << 34), CULLAVO_EINVAL, "nf4_quantize: too many blocks");
  const int64_t blocks = N * (K / 64);
  nf4_quantize_k<<<(unsigned)cdiv(blocks * 8, 256), 256, 0, CV_STREAM(stream)>>>(
      (const u16*)W, ldw, N, K, (uint8_t*)codes, (float*)absmax);
  return cullavo_check_launch("nf4_quantize");
}

extern "C" int cullavo_nf4_dequantize(int64_t N, int64_t K, const void* codes, const void* absmax, void* W, int64_t ldw,
                                      void* stream) {
  CV_REQUIRE(N > 0 && K > 0 && K % 64 == 0, CULLAVO_EINVAL, "nf4_dequantize: N > 0 and K a positive multiple of 64");
  CV_REQUIRE(ldw >= K && ldw % 8 == 0, CULLAVO_EINVAL, "nf4_dequantize: ldw >= K and a multiple of 8");
  CV_REQUIRE(N * (K / 8) <= ((int64_t)1 << 39), CULLAVO_EINVAL, "nf4_dequantize: too many elements");
  nf4_dequantize_k<<<(unsigned)cdiv(N * (K / 8), 256), 256, 0, CV_STREAM(stream)>>>(
      (const uint8_t*)codes, (const float*)absmax, N, K, (u16*)W, ldw);
  return cullavo_check_launch("nf4_dequantize");
}


// gemv.hip: the LoRA arguments of the decode products, checked and copied into the argument block
int cvgemm_decode_lora_args(cvgemm::GemmArgs& p, const char* who, int64_t rows, bool swiglu_out, const void* lora_u,
                            int64_t ld_lora_u, const void* lora_b, int64_t lora_out, int lora_r, float lora_scale);

// both entry points: the epilogue's LoRA term is `addend` (materialised) or lora_u / lora_b (fused), not both
static int nf4_decode_linear_impl(int swiglu_out, int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx,
                                  const void* codes, const void* absmax, void* y, int64_t ldy, const void* residual,
                                  int64_t ldr, const void* addend, int64_t ld_add, const void* lora_u,
                                  int64_t ld_lora_u, const void* lora_b, int64_t lora_out, int lora_r,
                                  float lora_scale, void* stream) {
  CV_REQUIRE(swiglu_out == 0 || swiglu_out == 1, CULLAVO_EINVAL, "nf4_decode_linear: swiglu_out 0 or 1");
  CV_REQUIRE(!swiglu_out || (residual == nullptr && addend == nullptr), CULLAVO_EINVAL,
             "nf4_decode_linear: the SwiGLU output takes no residual or addend");
  CV_REQUIRE(M >= 1 && M <= 16 && N > 0 && K > 0, CULLAVO_EINVAL, "nf4_decode_linear: 1 <= M <= 16 rows, N, K > 0");
  CV_REQUIRE(K % 64 == 0, CULLAVO_EINVAL, "nf4_decode_linear: K must be a multiple of 64 (the NF4 block)");
  CV_REQUIRE(N % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && (residual == nullptr || ldr % 8 == 0) &&
                 (addend == nullptr || ld_add % 4 == 0),
             CULLAVO_EINVAL, "nf4_decode_linear: N and strides must be multiples of 8 (addend: 4)");
  CV_REQUIRE(ldx >= K && ldy >= N && (residual == nullptr || ldr >= N) && (addend == nullptr || ld_add >= N),
             CULLAVO_EINVAL, "nf4_decode_linear: leading dimension too small");
  GemmArgs p{};
  p.A = (const u16*)x;
  p.C = y;
  p.residual = (const u16*)residual;
  p.addend = (const u16*)addend;
  p.M = M; p.N = N; p.K = K; p.lda = ldx; p.ldc = ldy; p.ldr = ldr; p.ld_add = ld_add;
  p.alpha = 1.f;
  p.beta = 0.f;
  p.act = CULLAVO_ACT_NONE;
  const bool lora = lora_u != nullptr;
  if (lora) {
    const int rc = cvgemm_decode_lora_args(p, "nf4_decode_linear_lora", swiglu_out ? 2 * N : N, swiglu_out != 0, lora_u,
                                           ld_lora_u, lora_b, lora_out, lora_r, lora_scale);
    if (rc != 0) return rc;
  }
  hipStream_t s = CV_STREAM(stream);
  const unsigned grid = (unsigned)cdiv(N, swiglu_out ? 8 : 16);
  const uint8_t* c = (const uint8_t*)codes;
  const float* a = (const float*)absmax;
  // waves per workgroup (each takes a contiguous range of K / 64 / NW blocks in batches of 8); lab
  // switch CULLAVO_NF4_WAVES = 2 | 4 | 8 | 16, read once per process (as gemv.hip's CULLAVO_GEMV); the
  // fused LoRA term runs on the shapes' own variants only
  static const int wenv = getenv("CULLAVO_NF4_WAVES") ? atoi(getenv("CULLAVO_NF4_WAVES")) : 0;
  const int nw = (!lora && (wenv == 2 || wenv == 4 || wenv == 8 || wenv == 16)) ? wenv
                                                                                 : (K > 8192 ? kNf4WavesLongK : kNf4Waves);
#define NF4_GVL(NW, L)                                                              \
  if (swiglu_out) nf4_gemv_k<NW, 8, 1, L><<<grid, 64 * NW, 0, s>>>(p, c, a);        \
  else nf4_gemv_k<NW, 8, 0, L><<<grid, 64 * NW, 0, s>>>(p, c, a);
#define NF4_GV(NW) NF4_GVL(NW, false)
  if (lora) {
    if (nw == 8) { NF4_GVL(8, true) } else { NF4_GVL(16, true) }
  } else if (nw == 2) { NF4_GV(2) } else if (nw == 4) { NF4_GV(4) } else if (nw == 8) { NF4_GV(8) } else { NF4_GV(16) }
#undef NF4_GV
#undef NF4_GVL
  return cullavo_check_launch("nf4_decode_linear");
}

extern "C" int cullavo_nf4_decode_linear(int swiglu_out, int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx,
                                         const void* codes, const void* absmax, void* y, int64_t ldy,
                                         const void* residual, int64_t ldr, const void* addend, int64_t ld_add,
                                         void* stream) {
  return nf4_decode_linear_impl(swiglu_out, M, N, K, x, ldx, codes, absmax, y, ldy, residual, ldr, addend, ld_add,
                                nullptr, 0, nullptr, 0, 0, 0.f, stream);
}

extern "C" int cullavo_nf4_decode_linear_lora(int swiglu_out, int64_t M, int64_t N, int64_t K, const void* x,
                                              int64_t ldx, const void* codes, const void* absmax, void* y, int64_t ldy,
                                              const void* residual, int64_t ldr, const void* lora_u, int64_t ld_lora_u,
                                              const void* lora_b, int64_t lora_out, int lora_r, float lora_scale,
                                              void* stream) {
  return nf4_decode_linear_impl(swiglu_out, M, N, K, x, ldx, codes, absmax, y, ldy, residual, ldr, nullptr, 0, lora_u,
                                ld_lora_u, lora_b, lora_out, lora_r, lora_scale, stream);
}
