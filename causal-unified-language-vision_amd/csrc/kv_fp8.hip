// FP8 KV cache: the appends that quantise, and the dequantisation to a bf16 slab (format: kv_fp8.h,
// INTEGRATION.md "FP8 KV cache"; decode attention on the codes: decode.hip).
//
// A head row (D = 128 bf16 = 256 B) is held by 16 consecutive lanes, 8 values each from one 16-B
// load: one max over the 16 lanes gives the row's amax and exponent, each lane scales and converts
// its 8 values and stores 8 bytes of codes; lane 0 of the 16 stores the exponent byte. SIM (the
// "fp8_sim" twin): the codes are converted straight back and the dequantised bf16 values go to a
// bf16 cache instead (one 16-B store), nothing else is written.
#include "kv_fp8.h"

namespace {

constexpr int kD = 128;

// the 16 lanes' common exponent byte for values x[8] per lane
DEV int row_exp16(const float* x) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(x[j]));
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 16));
  return fp8_exp_byte(a);
}

// quantise this lane's 8 values of a head row and store them: codes at row8 + l * 8 (and the exponent at
// *ex from lane 0), or SIM: the dequantised bf16 at (u16*)row8 + l * 8
template <bool SIM>
DEV void quant_store(const float* x, void* row8, uint8_t* ex, int l) {
  const int eb = row_exp16(x);
  const float inv = fp8_inv_scale(eb);
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = x[j] * inv;
  const u32x2 codes = fp8_pack8(s);
  if constexpr (SIM) {
    const float sc = fp8_scale(eb);
    float y[8];
    fp8_unpack4(codes[0], y);
    fp8_unpack4(codes[1], y + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] *= sc;
    store8(reinterpret_cast<u16*>(row8) + l * 8, y);
  } else {
    *reinterpret_cast<u32x2*>(reinterpret_cast<uint8_t*>(row8) + l * 8) = codes;
    if (l == 0) *ex = (uint8_t)eb;
  }
}

// kv_append_k / kv_append_ragged_k (decode.hip) with quantisation; q_pad null: the uniform append.
// An item is (row, head, lane of 16): the 16 lanes of a head row sit in one wave and run together
// (the item count and the grid stride are multiples of 16, a padding row skips all 16)
template <bool SIM>
__global__ __launch_bounds__(256) void kv_append_fp8_k(const u16* __restrict__ ks, int64_t ldks,
                                                      const u16* __restrict__ vs, int64_t ldvs, void* kc, void* vc,
                                                      int64_t ld_tok, int64_t ld_b, uint8_t* __restrict__ ke,
                                                      uint8_t* __restrict__ ve, int64_t ld_et, int64_t ld_eb,
                                                      const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ q_pad, int B, int Lnew, int H) {
  const int64_t per_row = (int64_t)H * 16, total = (int64_t)B * Lnew * per_row;
  constexpr int esz = SIM ? 2 : 1;  // bytes per cache element
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per_row;
    const int r = (int)(i % per_row), h = r >> 4, l = r & 15;
    const int b = (int)(row / Lnew), t = (int)(row % Lnew);
    const int pad = q_pad ? max(q_pad[b], 0) : 0;
    if (t < pad) continue;
    const int64_t tok = (int64_t)start[b] + t - pad;
    const int64_t dst = ((int64_t)b * ld_b + tok * ld_tok + (int64_t)h * kD) * esz;
    const int64_t edst = (int64_t)b * ld_eb + tok * ld_et + h;
    float x[8];
    load8(ks + row * ldks + h * kD + l * 8, x);
    quant_store<SIM>(x, reinterpret_cast<uint8_t*>(kc) + dst, SIM ? nullptr : ke + edst, l);
    load8(vs + row * ldvs + h * kD + l * 8, x);
    quant_store<SIM>(x, reinterpret_cast<uint8_t*>(vc) + dst, SIM ? nullptr : ve + edst, l);
  }
}

// rope_append8_k (elementwise.hip) with quantisation: one block per token, the token's (cos, sin)
// pairs once in LDS, q rotated in place with that kernel's arithmetic; lane l of a key head's 16
// holds the rotated dims 8l .. 8l + 7 (the first half's o1 for l < 8, the second half's o2 above:
// each lane loads both halves of its frequency group), rounded to bf16 before amax as cullavo_rope
// would have stored them.
template <bool SIM>
__global__ __launch_bounds__(256) void rope_append_fp8_k(u16* __restrict__ q, int64_t ldq, const u16* __restrict__ k,
                                                        int64_t ldk, const u16* __restrict__ v, int64_t ldv,
                                                        const int64_t* __restrict__ pos, int hq, int hk, float theta,
                                                        void* kc, void* vc, int64_t ld_tok, int64_t ld_b,
                                                        uint8_t* __restrict__ ke, uint8_t* __restrict__ ve,
                                                        int64_t ld_et, int64_t ld_eb,
                                                        const int32_t* __restrict__ start, int Lnew) {
  __shared__ float cs[kD / 2], sn[kD / 2];
  const int64_t t = blockIdx.x;
  constexpr int half = kD / 2, ng = half / 8;
  constexpr int esz = SIM ? 2 : 1;
  if (threadIdx.x < half) {
    const int i = threadIdx.x;
    const float inv_freq = 1.0f / powf(theta, (float)(2 * i) / (float)kD);
    const float ang = (float)pos[t] * inv_freq;
    cs[i] = Elt<u16>::rnd(cosf(ang));
    sn[i] = Elt<u16>::rnd(sinf(ang));
  }
  __syncthreads();
  for (int it = threadIdx.x; it < hq * ng; it += 256) {
    const int h = it / ng, g8 = (it % ng) * 8;
    u16* p1 = q + t * ldq + (int64_t)h * kD + g8;
    float x1[8], x2[8], o1[8], o2[8];
    load8(p1, x1);
    load8(p1 + half, x2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = cs[g8 + j], sv = sn[g8 + j];
      o1[j] = Elt<u16>::rnd(Elt<u16>::rnd(x1[j] * c) + Elt<u16>::rnd(-x2[j] * sv));
      o2[j] = Elt<u16>::rnd(Elt<u16>::rnd(x2[j] * c) + Elt<u16>::rnd(x1[j] * sv));
    }
    store8(p1, o1);
    store8(p1 + half, o2);
  }
  const int b = (int)(t / Lnew), tt = (int)(t % Lnew);
  const int64_t tok = (int64_t)start[b] + tt;
  for (int it = threadIdx.x; it < hk * 16; it += 256) {
    const int h = it >> 4, l = it & 15, g8 = (l & 7) * 8;
    const u16* s1 = k + t * ldk + (int64_t)h * kD + g8;
    float x1[8], x2[8], x[8];
    load8(s1, x1);
    load8(s1 + half, x2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = cs[g8 + j], sv = sn[g8 + j];
      const float o1 = Elt<u16>::rnd(Elt<u16>::rnd(x1[j] * c) + Elt<u16>::rnd(-x2[j] * sv));
      const float o2 = Elt<u16>::rnd(Elt<u16>::rnd(x2[j] * c) + Elt<u16>::rnd(x1[j] * sv));
      x[j] = l < 8 ? o1 : o2;
    }
    const int64_t dst = ((int64_t)b * ld_b + tok * ld_tok + (int64_t)h * kD) * esz;
    const int64_t edst = (int64_t)b * ld_eb + tok * ld_et + h;
    quant_store<SIM>(x, reinterpret_cast<uint8_t*>(kc) + dst, SIM ? nullptr : ke + edst, l);
    load8(v + t * ldv + (int64_t)h * kD + l * 8, x);
    quant_store<SIM>(x, reinterpret_cast<uint8_t*>(vc) + dst, SIM ? nullptr : ve + edst, l);
  }
}

// codes and exponents of rows [0, rows) to bf16: an item is (sequence, row, head, 8 dims), one 8-B
// load and one 16-B store for K and for V
__global__ __launch_bounds__(256) void kv_dequant_fp8_k(const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                       int64_t ld_tok, int64_t ld_b, const uint8_t* __restrict__ ke,
                                                       const uint8_t* __restrict__ ve, int64_t ld_et, int64_t ld_eb,
                                                       u16* __restrict__ ko, u16* __restrict__ vo, int64_t ld_ot,
                                                       int64_t ld_ob, int B, int rows, int H) {
  const int64_t per_row = (int64_t)H * 16, total = (int64_t)B * rows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per_row;
    const int r = (int)(i % per_row), h = r >> 4, l = r & 15;
    const int b = (int)(row / rows), t = (int)(row % rows);
    const int64_t src = (int64_t)b * ld_b + (int64_t)t * ld_tok + h * kD + l * 8;
    const int64_t esrc = (int64_t)b * ld_eb + (int64_t)t * ld_et + h;
    const int64_t dst = (int64_t)b * ld_ob + (int64_t)t * ld_ot + h * kD + l * 8;
    float y[8];
    u32x2 c = *reinterpret_cast<const u32x2*>(kc + src);
    float sc = fp8_scale(ke[esrc]);
    fp8_unpack4(c[0], y);
    fp8_unpack4(c[1], y + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] *= sc;
    store8(ko + dst, y);
    c = *reinterpret_cast<const u32x2*>(vc + src);
    sc = fp8_scale(ve[esrc]);
    fp8_unpack4(c[0], y);
    fp8_unpack4(c[1], y + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] *= sc;
    store8(vo + dst, y);
  }
}

inline bool al16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

int append_fp8(const char* what, const void* k, int64_t ldk, const void* v, int64_t ldv, void* kc, void* vc,
               int64_t ld_tok, int64_t ld_batch, void* ke, void* ve, int64_t ld_etok, int64_t ld_ebatch,
               const int32_t* start, const int32_t* q_pad, bool ragged, int B, int Lnew, int H, int D, int sim,
               void* stream) {
  const std::string w(what);
  CV_REQUIRE(D == kD, CULLAVO_EUNSUPPORTED, w + ": head_dim 128");
  CV_REQUIRE(B >= 0 && Lnew >= 0 && H >= 1, CULLAVO_EINVAL, w + ": B and Lnew must not be negative, H >= 1");
  CV_REQUIRE(k != nullptr && v != nullptr && kc != nullptr && vc != nullptr && start != nullptr, CULLAVO_EINVAL,
             w + ": k / v / caches / start positions");
  CV_REQUIRE(!ragged || q_pad != nullptr, CULLAVO_EINVAL, w + ": q_pad (the padding rows per sequence) is null");
  CV_REQUIRE(sim || (ke != nullptr && ve != nullptr), CULLAVO_EINVAL, w + ": the exponent arrays are null");
  CV_REQUIRE(ldk % 8 == 0 && ldv % 8 == 0 && ldk >= (int64_t)H * D && ldv >= (int64_t)H * D && al16(k, v),
             CULLAVO_EINVAL, w + ": 16-byte aligned k / v rows of at least H*D");
  // codes: byte strides, 16-byte rows (decode attention's loads); sim: a bf16 cache, strides in elements
  const int64_t al = sim ? 8 : 16;
  CV_REQUIRE(ld_tok % al == 0 && ld_batch % al == 0 && ld_tok >= (int64_t)H * D && al16(kc, vc), CULLAVO_EINVAL,
             w + ": 16-byte aligned cache rows of at least H*D");
  CV_REQUIRE(sim || (ld_etok >= H && ld_ebatch >= 0), CULLAVO_EINVAL, w + ": exponent strides");
  if (B == 0 || Lnew == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int64_t work = (int64_t)B * Lnew * H * 16;
  const int g = (int)std::min<int64_t>(cdiv(work, 256), 8192);
  if (sim)
    kv_append_fp8_k<true><<<g, 256, 0, s>>>((const u16*)k, ldk, (const u16*)v, ldv, kc, vc, ld_tok, ld_batch, nullptr,
                                           nullptr, 0, 0, start, q_pad, B, Lnew, H);
  else
    kv_append_fp8_k<false><<<g, 256, 0, s>>>((const u16*)k, ldk, (const u16*)v, ldv, kc, vc, ld_tok, ld_batch,
                                            (uint8_t*)ke, (uint8_t*)ve, ld_etok, ld_ebatch, start, q_pad, B, Lnew, H);
  return cullavo_check_launch(what);
}

}  // namespace

extern "C" int cullavo_kv_append_fp8(const void* k, int64_t ldk, const void* v, int64_t ldv, void* k_codes,
                                     void* v_codes, int64_t ld_tok, int64_t ld_batch, void* k_exp, void* v_exp,
                                     int64_t ld_etok, int64_t ld_ebatch, const int32_t* start, int B, int Lnew, int H,
                                     int D, int sim, void* stream) {
  return append_fp8("kv_append_fp8", k, ldk, v, ldv, k_codes, v_codes, ld_tok, ld_batch, k_exp, v_exp, ld_etok,
                    ld_ebatch, start, nullptr, false, B, Lnew, H, D, sim, stream);
}

extern "C" int cullavo_kv_append_ragged_fp8(const void* k, int64_t ldk, const void* v, int64_t ldv, void* k_codes,
                                            void* v_codes, int64_t ld_tok, int64_t ld_batch, void* k_exp, void* v_exp,
                                            int64_t ld_etok, int64_t ld_ebatch, const int32_t* start,
                                            const int32_t* q_pad, int B, int Lnew, int H, int D, int sim,
                                            void* stream) {
  return append_fp8("kv_append_ragged_fp8", k, ldk, v, ldv, k_codes, v_codes, ld_tok, ld_batch, k_exp, v_exp, ld_etok,
                    ld_ebatch, start, q_pad, true, B, Lnew, H, D, sim, stream);
}

extern "C" int cullavo_rope_kv_append_fp8(void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                          int64_t ldv, const int64_t* position_ids, int64_t tokens, int hq, int hk,
                                          int head_dim, float theta, void* k_codes, void* v_codes, int64_t ld_tok,
                                          int64_t ld_batch, void* k_exp, void* v_exp, int64_t ld_etok,
                                          int64_t ld_ebatch, const int32_t* start, int Lnew, int sim, void* stream) {
  CV_REQUIRE(head_dim == kD, CULLAVO_EUNSUPPORTED, "rope_kv_append_fp8: head_dim 128");
  CV_REQUIRE(Lnew >= 1 && tokens >= 0 && tokens % Lnew == 0 && hq >= 0 && hk >= 1, CULLAVO_EINVAL,
             "rope_kv_append_fp8: tokens = B * Lnew");
  CV_REQUIRE(q != nullptr && k != nullptr && v != nullptr && k_codes != nullptr && v_codes != nullptr &&
                 start != nullptr && position_ids != nullptr,
             CULLAVO_EINVAL, "rope_kv_append_fp8: q / k / v / caches / start / position_ids");
  CV_REQUIRE(sim || (k_exp != nullptr && v_exp != nullptr), CULLAVO_EINVAL,
             "rope_kv_append_fp8: the exponent arrays are null");
  const int64_t al = sim ? 8 : 16;
  CV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ld_tok % al == 0 && ld_batch % al == 0 &&
                 ldq >= (int64_t)hq * kD && ldk >= (int64_t)hk * kD && ldv >= (int64_t)hk * kD &&
                 ld_tok >= (int64_t)hk * kD && al16(q, k, v) && al16(k_codes, v_codes),
             CULLAVO_EINVAL, "rope_kv_append_fp8: 16-byte aligned rows");
  CV_REQUIRE(sim || ld_etok >= hk, CULLAVO_EINVAL, "rope_kv_append_fp8: exponent strides");
  if (tokens == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  if (sim)
    rope_append_fp8_k<true><<<(unsigned)tokens, 256, 0, s>>>((u16*)q, ldq, (const u16*)k, ldk, (const u16*)v, ldv,
                                                            position_ids, hq, hk, theta, k_codes, v_codes, ld_tok,
                                                            ld_batch, nullptr, nullptr, 0, 0, start, Lnew);
  else
    rope_append_fp8_k<false><<<(unsigned)tokens, 256, 0, s>>>((u16*)q, ldq, (const u16*)k, ldk, (const u16*)v, ldv,
                                                             position_ids, hq, hk, theta, k_codes, v_codes, ld_tok,
                                                             ld_batch, (uint8_t*)k_exp, (uint8_t*)v_exp, ld_etok,
                                                             ld_ebatch, start, Lnew);
  return cullavo_check_launch("rope_kv_append_fp8");
}

extern "C" int cullavo_kv_dequant_fp8(const void* k_codes, const void* v_codes, int64_t ld_tok, int64_t ld_batch,
                                      const void* k_exp, const void* v_exp, int64_t ld_etok, int64_t ld_ebatch,
                                      void* k_out, void* v_out, int64_t ld_otok, int64_t ld_obatch, int B, int rows,
                                      int H, int D, void* stream) {
  CV_REQUIRE(D == kD, CULLAVO_EUNSUPPORTED, "kv_dequant_fp8: head_dim 128");
  CV_REQUIRE(B >= 0 && rows >= 0 && H >= 1, CULLAVO_EINVAL, "kv_dequant_fp8: B and rows must not be negative");
  CV_REQUIRE(k_codes != nullptr && v_codes != nullptr && k_out != nullptr && v_out != nullptr, CULLAVO_EINVAL,
             "kv_dequant_fp8: codes / outputs");
  CV_REQUIRE(k_exp != nullptr && v_exp != nullptr, CULLAVO_EINVAL, "kv_dequant_fp8: the exponent arrays are null");
  CV_REQUIRE(ld_tok % 16 == 0 && ld_batch % 16 == 0 && ld_tok >= (int64_t)H * D && al16(k_codes, v_codes) &&
                 ld_otok % 8 == 0 && ld_obatch % 8 == 0 && ld_otok >= (int64_t)H * D && al16(k_out, v_out) &&
                 ld_etok >= H,
             CULLAVO_EINVAL, "kv_dequant_fp8: 16-byte aligned rows of at least H*D");
  if (B == 0 || rows == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int64_t work = (int64_t)B * rows * H * 16;
  const int g = (int)std::min<int64_t>(cdiv(work, 256), 16384);
  kv_dequant_fp8_k<<<g, 256, 0, s>>>((const uint8_t*)k_codes, (const uint8_t*)v_codes, ld_tok, ld_batch,
                                     (const uint8_t*)k_exp, (const uint8_t*)v_exp, ld_etok, ld_ebatch, (u16*)k_out,
                                     (u16*)v_out, ld_otok, ld_obatch, B, rows, H);
  return cullavo_check_launch("kv_dequant_fp8");
}
