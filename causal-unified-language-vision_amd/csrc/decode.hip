// KV-cache decode for generate() (reference cullavo/arch_cullavo.py:
// 605-636 and the HF generate() loop it drives, :341-395).
//
// The cache is preallocated per layer as K, V [B, Lmax, H*D] bf16 (token stride ld_tok, batch
// stride ld_batch). Prefill writes the prompt's rotated keys and values with kv_append; each
// decode step appends one token and runs attn_decode: one query row per (batch, head) against
// keys [kv_start[b], kv_len[b]). Decode attention is HBM-bound (every cached key and value is
// read once per step), so it is split over the keys (flash-decoding): workgroup (chunk, h, b)
// scores kChunk keys with 8 lanes per key (each lane 16 dims, coalesced 256 B rows, all loads in
// flight before use), forms P.V with 16 dim-groups x 16 key-groups of 16 B loads, keeps the
// chunk's max / sum / unnormalised P.V in f32 partials, and a combine kernel rescales and sums
// the chunks in a fixed order (deterministic).
#include "kv_fp8.h"

namespace {

// keys per workgroup: 64 gives the batch-1 step 32 heads x 18 chunks = 576 workgroups at the
// 1088-row prompt (128: 288, about one per CU, each waiting out a longer load ramp)
constexpr int kChunk = 64;
constexpr float kLog2e = 1.4426950408889634f;

__global__ __launch_bounds__(256) void kv_append_k(const u16* __restrict__ ks, int64_t ldks, const u16* __restrict__ vs,
                                                  int64_t ldvs, u16* __restrict__ kc, u16* __restrict__ vc,
                                                  int64_t ld_tok, int64_t ld_b, const int32_t* __restrict__ start,
                                                  int B, int Lnew, int64_t hd) {
  const int64_t per_row = hd / 8, total = (int64_t)B * Lnew * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per_row, c = (i % per_row) * 8;
    const int b = (int)(row / Lnew), t = (int)(row % Lnew);
    const int64_t dst = (int64_t)b * ld_b + (int64_t)(start[b] + t) * ld_tok + c;
    *reinterpret_cast<u16x8*>(kc + dst) = *reinterpret_cast<const u16x8*>(ks + row * ldks + c);
    *reinterpret_cast<u16x8*>(vc + dst) = *reinterpret_cast<const u16x8*>(vs + row * ldvs + c);
  }
}

// kv_append_k for a left-padded [B, Lnew] block (cullavo_kv_append_ragged): row t of sequence b is
// padding when t < q_pad[b] and is not written; the others land at start[b] + t - q_pad[b]
__global__ __launch_bounds__(256) void kv_append_ragged_k(const u16* __restrict__ ks, int64_t ldks,
                                                         const u16* __restrict__ vs, int64_t ldvs,
                                                         u16* __restrict__ kc, u16* __restrict__ vc, int64_t ld_tok,
                                                         int64_t ld_b, const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ q_pad, int B, int Lnew,
                                                         int64_t hd) {
  const int64_t per_row = hd / 8, total = (int64_t)B * Lnew * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / per_row, c = (i % per_row) * 8;
    const int b = (int)(row / Lnew), t = (int)(row % Lnew);
    const int pad = max(q_pad[b], 0);
    if (t < pad) continue;
    const int64_t dst = (int64_t)b * ld_b + (int64_t)(start[b] + t - pad) * ld_tok + c;
    *reinterpret_cast<u16x8*>(kc + dst) = *reinterpret_cast<const u16x8*>(ks + row * ldks + c);
    *reinterpret_cast<u16x8*>(vc + dst) = *reinterpret_cast<const u16x8*>(vs + row * ldvs + c);
  }
}

// ROPE (cullavo_attn_decode_rope): the step's RoPE + KV append fused in front (rope_append8_k's
// arithmetic, elementwise.hip): every workgroup rotates its head's query row itself (q is read, not
// rotated in place), the workgroup whose chunk holds the new row start[b] rotates that row's key,
// writes key and value to the cache and uses them from LDS (its own loads of that row may predate
// the write), and the keys attended are [kv_start[b], start[b] + 1).
struct DecodeRope {
  const u16* k;
  int64_t ldk;
  const u16* v;
  int64_t ldv;
  const int64_t* pos;
  float theta;
  const int32_t* start;
  u16* kc;
  u16* vc;
};

// The FP8 cache (kv_fp8.h): KV_FP8 reads e4m3 codes (Kc, Vc: bytes, ld_tok / ld_b in bytes) and the
// per (token, head) exponent bytes. A lane's 16 dims of a key are one 16-B load, a P.V thread's 8
// dims of a value one 8-B load; codes go to f32 unscaled through the same sums as the bf16 kernel,
// the key's 2^e multiplies the finished score once and the value's 2^e its probability once --
// power-of-two factors that commute with every f32 rounding in range, so the result is bitwise the
// bf16 kernel's on the dequantised cache. With ROPE the new row's workgroup also reduces amax over
// the head for K and V, writes codes and exponents and attends the codes from LDS (the dequantised
// row, what every later step reads). KV_SIM (ROPE only): a bf16 cache that receives the
// dequantised new row; everything else is the bf16 kernel.
constexpr int KV_BF16 = 0, KV_FP8 = 1, KV_SIM = 2;
struct DecodeFp8 {
  const uint8_t* ke;  // K, V exponents [B, Lmax, H]
  const uint8_t* ve;
  int64_t ld_et, ld_eb;
  uint8_t* ke_w;  // ROPE: the same arrays, written at the new row
  uint8_t* ve_w;
};

template <int D, bool ROPE = false, int KV = KV_BF16>
__global__ __launch_bounds__(256) void attn_decode_k(const u16* __restrict__ Q, int64_t ldq, const void* __restrict__ Kc_,
                                                    const void* __restrict__ Vc_, int64_t ld_tok, int64_t ld_b,
                                                    const int32_t* __restrict__ kv_len,
                                                    const int32_t* __restrict__ kv_start, float scale_log2,
                                                    float* __restrict__ part_o, float* __restrict__ part_ml,
                                                    int H, int nchunk, DecodeRope rp = DecodeRope{},
                                                    DecodeFp8 f8 = DecodeFp8{}) {
  static_assert(D == 128, "decode attention is specialised for the LM head_dim");
  static_assert(KV != KV_SIM || ROPE, "the round-trip twin differs from bf16 only where a row is appended");
  constexpr bool FP8 = KV == KV_FP8;
  const u16* Kc = reinterpret_cast<const u16*>(Kc_);
  const u16* Vc = reinterpret_cast<const u16*>(Vc_);
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int t = threadIdx.x;
  const int pnew = ROPE ? rp.start[b] : -1;  // the appended row (ROPE)
  const int len = ROPE ? pnew + 1 : kv_len[b], k_lo = kv_start ? kv_start[b] : 0;
  const int kbeg = c * kChunk, kend = min(len, kbeg + kChunk);
  __shared__ float qs[D];
  __shared__ float ps[kChunk];
  __shared__ float red[8];
  __shared__ float oacc[16][D];
  __shared__ float cs[D / 2], sn[D / 2];
  __shared__ u16 kn[D], vn[D];
  __shared__ __attribute__((aligned(16))) uint8_t kn8[D], vn8[D];  // FP8: the new row's codes
  __shared__ int new_e[2];                                         // and its K, V exponent bytes
  const int64_t pidx = ((int64_t)b * H + h) * nchunk + c;
  if (kbeg >= kend) {  // chunk past this row's length: empty partial
    if (t < D) part_o[pidx * D + t] = 0.f;
    if (t == 0) { part_ml[2 * pidx] = -INFINITY; part_ml[2 * pidx + 1] = 0.f; }
  } else {
    const bool has_new = ROPE && pnew >= kbeg && pnew < kend;
    float nk1 = 0.f, nk2 = 0.f, nv = 0.f;  // KV_FP8 / KV_SIM: the new row's rotated key pair / value
    if constexpr (ROPE) {
      if (t < D / 2) {
        const float inv_freq = 1.0f / powf(rp.theta, (float)(2 * t) / (float)D);
        const float ang = (float)rp.pos[b] * inv_freq;
        cs[t] = Elt<u16>::rnd(cosf(ang));
        sn[t] = Elt<u16>::rnd(sinf(ang));
      }
      __syncthreads();
      // t < 64: the query pair (t, t + 64); 64 <= t < 128 (the new row's chunk): the key pair
      if (t < D / 2 || (has_new && t < D)) {
        const int i = t & (D / 2 - 1);
        const u16* src = t < D / 2 ? Q + (int64_t)b * ldq + (int64_t)h * D : rp.k + (int64_t)b * rp.ldk + (int64_t)h * D;
        const float x1 = bf2f(src[i]), x2 = bf2f(src[i + D / 2]);
        const float o1 = Elt<u16>::rnd(Elt<u16>::rnd(x1 * cs[i]) + Elt<u16>::rnd(-x2 * sn[i]));
        const float o2 = Elt<u16>::rnd(Elt<u16>::rnd(x2 * cs[i]) + Elt<u16>::rnd(x1 * sn[i]));
        if (t < D / 2) {
          qs[i] = o1 * scale_log2;
          qs[i + D / 2] = o2 * scale_log2;
        } else if constexpr (KV == KV_BF16) {
          const int64_t row = (int64_t)b * ld_b + (int64_t)pnew * ld_tok + (int64_t)h * D;
          kn[i] = f2bf(o1);
          kn[i + D / 2] = f2bf(o2);
          rp.kc[row + i] = f2bf(o1);
          rp.kc[row + i + D / 2] = f2bf(o2);
        } else {
          nk1 = o1;
          nk2 = o2;
        }
      }
      if (has_new && t >= D && t < 2 * D) {
        const u16 vv = rp.v[(int64_t)b * rp.ldv + (int64_t)h * D + (t - D)];
        if constexpr (KV == KV_BF16) {
          vn[t - D] = vv;
          rp.vc[(int64_t)b * ld_b + (int64_t)pnew * ld_tok + (int64_t)h * D + (t - D)] = vv;
        } else {
          nv = bf2f(vv);
        }
      }
      if constexpr (KV != KV_BF16) {
        if (has_new) {  // workgroup-uniform: wave 1 holds the rotated key (a pair per lane), waves 2-3 the value
          float a = 0.f;
          if (t >= D / 2 && t < D) a = fmaxf(fabsf(nk1), fabsf(nk2));
          if (t >= D) a = fabsf(nv);
          a = wave_max(a);
          if ((t & 63) == 0) red[t >> 6] = a;
          __syncthreads();
          const int ek = fp8_exp_byte(red[1]), ev = fp8_exp_byte(fmaxf(red[2], red[3]));
          const int64_t row = (int64_t)b * ld_b + (int64_t)pnew * ld_tok + (int64_t)h * D;
          if (t >= D / 2 && t < D) {
            const int i = t - D / 2;
            const unsigned c1 = fp8_code(nk1 * fp8_inv_scale(ek)), c2 = fp8_code(nk2 * fp8_inv_scale(ek));
            if constexpr (FP8) {
              uint8_t* kc8 = reinterpret_cast<uint8_t*>(rp.kc);
              kn8[i] = (uint8_t)c1;
              kn8[i + D / 2] = (uint8_t)c2;
              kc8[row + i] = (uint8_t)c1;
              kc8[row + i + D / 2] = (uint8_t)c2;
            } else {
              const u16 d1 = f2bf(fp8_value(c1) * fp8_scale(ek)), d2 = f2bf(fp8_value(c2) * fp8_scale(ek));
              kn[i] = d1;
              kn[i + D / 2] = d2;
              rp.kc[row + i] = d1;
              rp.kc[row + i + D / 2] = d2;
            }
          } else if (t >= D) {
            const unsigned c = fp8_code(nv * fp8_inv_scale(ev));
            if constexpr (FP8) {
              vn8[t - D] = (uint8_t)c;
              reinterpret_cast<uint8_t*>(rp.vc)[row + (t - D)] = (uint8_t)c;
            } else {
              const u16 d = f2bf(fp8_value(c) * fp8_scale(ev));
              vn[t - D] = d;
              rp.vc[row + (t - D)] = d;
            }
          }
          if constexpr (FP8) {
            if (t == 0) {
              const int64_t erow = (int64_t)b * f8.ld_eb + (int64_t)pnew * f8.ld_et + h;
              new_e[0] = ek;
              new_e[1] = ev;
              f8.ke_w[erow] = (uint8_t)ek;
              f8.ve_w[erow] = (uint8_t)ev;
            }
          }
        }
      }
    } else {
      if (t < D) qs[t] = bf2f(Q[(int64_t)b * ldq + (int64_t)h * D + t]) * scale_log2;
    }
    const u16* Kb = Kc + (int64_t)b * ld_b + (int64_t)h * D;
    const u16* Vb = Vc + (int64_t)b * ld_b + (int64_t)h * D;
    // scores: 8 lanes per key (16 dims each, one 256 B row per key), 32 keys per pass; the K rows
    // and the V rows of P.V (which do not depend on the scores) are all in flight before the first
    // is consumed
    const int sub = t & 7, slot = t >> 3;
    constexpr int kPass = kChunk / 32;
    u16x8 kr[kPass][2];
    u32x4 kq[kPass];     // FP8: the lane's 16 codes of a key
    int ke_b[kPass];     //      and the key's exponent byte
    const uint8_t* Kb8 = reinterpret_cast<const uint8_t*>(Kc_) + (int64_t)b * ld_b + (int64_t)h * D;
    const uint8_t* Vb8 = reinterpret_cast<const uint8_t*>(Vc_) + (int64_t)b * ld_b + (int64_t)h * D;
#pragma unroll
    for (int pass = 0; pass < kPass; ++pass) {
      const int key = min(kbeg + pass * 32 + slot, kend - 1);
      if constexpr (FP8) {
        kq[pass] = *reinterpret_cast<const u32x4*>(Kb8 + (int64_t)key * ld_tok + sub * 16);
        ke_b[pass] = f8.ke[(int64_t)b * f8.ld_eb + (int64_t)key * f8.ld_et + h];
      } else {
        const u16* kp = Kb + (int64_t)key * ld_tok + sub * 16;
        kr[pass][0] = *reinterpret_cast<const u16x8*>(kp);
        kr[pass][1] = *reinterpret_cast<const u16x8*>(kp + 8);
      }
    }
    // P.V: thread (dim group dg of 8 dims, key group kg) sums keys kg, kg+16, ...
    const int dg = t & 15, kg = t >> 4;
    const int nk = kend - kbeg;
    u16x8 vr[kChunk / 16];
    u32x2 vq[kChunk / 16];  // FP8: the thread's 8 codes of a value
    // FP8: thread t < kChunk holds the scale 2^e of value kbeg + t, which multiplies that key's p once
    // (0 outside [kv_start, kend): such a row's exponent is not read either)
    float vscale = 0.f;
    if constexpr (FP8) {
      if (t < kChunk && kbeg + t < kend && kbeg + t >= k_lo)
        vscale = fp8_scale(f8.ve[(int64_t)b * f8.ld_eb + (int64_t)(kbeg + t) * f8.ld_et + h]);
    }
#pragma unroll
    for (int i = 0; i < kChunk / 16; ++i) {
      const int k = min(kg + 16 * i, nk - 1);
      // a key below kv_start has p = 0 and its V row is not read: a free cache row there may hold
      // anything, NaN included (the contract of attn_fwd_cached), and 0 * NaN must not reach the sum.
      // For a finite row this puts 0 * 0 = +0 in place of 0 * v on an accumulator that starts at +0:
      // the same bits.
      if constexpr (FP8) {
        vq[i] = u32x2{};
        if (kbeg + k >= k_lo) vq[i] = *reinterpret_cast<const u32x2*>(Vb8 + (int64_t)(kbeg + k) * ld_tok + dg * 8);
      } else {
        vr[i] = u16x8{};
        if (kbeg + k >= k_lo) vr[i] = *reinterpret_cast<const u16x8*>(Vb + (int64_t)(kbeg + k) * ld_tok + dg * 8);
      }
    }
    __syncthreads();
    if (has_new) {  // the appended row from LDS (this workgroup's own cache write may not be visible)
#pragma unroll
      for (int pass = 0; pass < kPass; ++pass) {
        if (min(kbeg + pass * 32 + slot, kend - 1) == pnew) {
          if constexpr (FP8) {
            kq[pass] = reinterpret_cast<const u32x4*>(kn8)[sub];
            ke_b[pass] = new_e[0];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              kr[pass][0][j] = kn[sub * 16 + j];
              kr[pass][1][j] = kn[sub * 16 + 8 + j];
            }
          }
        }
      }
      if constexpr (FP8) {
        if (kbeg + t == pnew) vscale = fp8_scale(new_e[1]);  // pnew >= kv_start: a row attends itself
      }
#pragma unroll
      for (int i = 0; i < kChunk / 16; ++i) {
        if (kbeg + min(kg + 16 * i, nk - 1) == pnew) {
          if constexpr (FP8) {
            vq[i] = reinterpret_cast<const u32x2*>(vn8)[dg];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) vr[i][j] = vn[dg * 8 + j];
          }
        }
      }
    }
    float qv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) qv[j] = qs[sub * 16 + j];
#pragma unroll
    for (int pass = 0; pass < kPass; ++pass) {
      const int key = kbeg + pass * 32 + slot;
      float acc = 0.f;
      if constexpr (FP8) {  // the same sum over the unscaled code values
        float kf[16];
#pragma unroll
        for (int w = 0; w < 4; ++w) fp8_unpack4(kq[pass][w], kf + 4 * w);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += qv[j] * kf[j] + qv[8 + j] * kf[8 + j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += qv[j] * bf2f(kr[pass][0][j]) + qv[8 + j] * bf2f(kr[pass][1][j]);
      }
      acc += __shfl_xor(acc, 1);
      acc += __shfl_xor(acc, 2);
      acc += __shfl_xor(acc, 4);
      if constexpr (FP8) acc *= fp8_scale(ke_b[pass]);  // the key's scale, once on the finished score
      if (sub == 0) ps[pass * 32 + slot] = (key < kend && key >= k_lo) ? acc : -INFINITY;
    }
    __syncthreads();
    // chunk max and sum (kChunk scores, threads >= kChunk carry -inf / 0)
    const int lane = t & 63, wv = t >> 6;
    const float s = t < kChunk ? ps[t] : -INFINITY;
    float m = wave_max(s);
    if (lane == 0) red[wv] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float p = (s == -INFINITY) ? 0.f : exp2f(s - m);
    __syncthreads();
    if (t < kChunk) ps[t] = FP8 ? p * vscale : p;  // FP8: the value's scale, once on its probability
    float l = wave_sum(p);
    if (lane == 0) red[4 + wv] = l;
    __syncthreads();
    l = red[4] + red[5] + red[6] + red[7];
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kChunk / 16; ++i) {
      const int k = kg + 16 * i;
      const float pk = k < nk ? ps[k] : 0.f;
      if constexpr (FP8) {
        float vf[8];
        fp8_unpack4(vq[i][0], vf);
        fp8_unpack4(vq[i][1], vf + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += pk * vf[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += pk * bf2f(vr[i][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) oacc[kg][dg * 8 + j] = o[j];
    __syncthreads();
    if (t < D) {
      float sum = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) sum += oacc[g][t];
      part_o[pidx * D + t] = sum;
    }
    if (t == 0) { part_ml[2 * pidx] = m; part_ml[2 * pidx + 1] = l; }
  }
}

// Combine: max over the chunks, then the rescaled sums in chunk order (deterministic). Up to
// kCombineRegs chunks (max_len <= 2048) every partial is loaded before the first is used.
constexpr int kCombineRegs = 2048 / kChunk;
template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine_k(const float* __restrict__ part_o,
                                                          const float* __restrict__ part_ml, u16* __restrict__ O,
                                                          int64_t ldo, int H, int nchunk) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const int64_t base = ((int64_t)b * H + h) * nchunk;
  float M = -INFINITY, L = 0.f, acc = 0.f;
  if (nchunk <= kCombineRegs) {
    float mc[kCombineRegs], lc[kCombineRegs], oc[kCombineRegs];
#pragma unroll
    for (int c = 0; c < kCombineRegs; ++c) {
      const bool in = c < nchunk;
      mc[c] = in ? part_ml[2 * (base + c)] : -INFINITY;
      lc[c] = in ? part_ml[2 * (base + c) + 1] : 0.f;
      oc[c] = in ? part_o[(base + c) * D + d] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kCombineRegs; ++c) M = fmaxf(M, mc[c]);
    if (M != -INFINITY) {
#pragma unroll
      for (int c = 0; c < kCombineRegs; ++c) {
        if (mc[c] == -INFINITY) continue;
        const float w = exp2f(mc[c] - M);
        L += w * lc[c];
        acc += w * oc[c];
      }
    }
  } else {
    for (int c = 0; c < nchunk; ++c) M = fmaxf(M, part_ml[2 * (base + c)]);
    if (M != -INFINITY) {
      for (int c = 0; c < nchunk; ++c) {
        const float mc = part_ml[2 * (base + c)];
        if (mc == -INFINITY) continue;
        const float w = exp2f(mc - M);
        L += w * part_ml[2 * (base + c) + 1];
        acc += w * part_o[(base + c) * D + d];
      }
    }
  }
  O[(int64_t)b * ldo + (int64_t)h * D + d] = f2bf(L > 0.f ? acc / L : 0.f);  // no visible key -> 0
}

}  // namespace

extern "C" int cullavo_kv_append(const void* k, int64_t ldk, const void* v, int64_t ldv, void* k_cache,
                                 void* v_cache, int64_t ld_tok, int64_t ld_batch, const int32_t* start, int B,
                                 int Lnew, int64_t hd, void* stream) {
  CV_REQUIRE(hd % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ld_tok % 8 == 0 && ld_batch % 8 == 0, CULLAVO_EINVAL,
             "kv_append: sizes and strides must be multiples of 8");
  CV_REQUIRE(start != nullptr, CULLAVO_EINVAL, "kv_append: start positions");
  if (B == 0 || Lnew == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int64_t work = (int64_t)B * Lnew * (hd / 8);
  const int g = (int)std::min<int64_t>(cdiv(work, 256), 8192);
  kv_append_k<<<g, 256, 0, s>>>((const u16*)k, ldk, (const u16*)v, ldv, (u16*)k_cache, (u16*)v_cache, ld_tok,
                                ld_batch, start, B, Lnew, hd);
  return cullavo_check_launch("kv_append");
}

extern "C" int cullavo_kv_append_ragged(const void* k, int64_t ldk, const void* v, int64_t ldv, void* k_cache,
                                        void* v_cache, int64_t ld_tok, int64_t ld_batch, const int32_t* start,
                                        const int32_t* q_pad, int B, int Lnew, int64_t hd, void* stream) {
  CV_REQUIRE(hd % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ld_tok % 8 == 0 && ld_batch % 8 == 0, CULLAVO_EINVAL,
             "kv_append_ragged: sizes and strides must be multiples of 8");
  CV_REQUIRE(start != nullptr, CULLAVO_EINVAL, "kv_append_ragged: start positions");
  CV_REQUIRE(q_pad != nullptr, CULLAVO_EINVAL, "kv_append_ragged: q_pad (the padding rows per sequence) is null");
  CV_REQUIRE(B >= 0 && Lnew >= 0, CULLAVO_EINVAL, "kv_append_ragged: B and Lnew must not be negative");
  if (B == 0 || Lnew == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int64_t work = (int64_t)B * Lnew * (hd / 8);
  const int g = (int)std::min<int64_t>(cdiv(work, 256), 8192);
  kv_append_ragged_k<<<g, 256, 0, s>>>((const u16*)k, ldk, (const u16*)v, ldv, (u16*)k_cache, (u16*)v_cache, ld_tok,
                                       ld_batch, start, q_pad, B, Lnew, hd);
  return cullavo_check_launch("kv_append_ragged");
}

extern "C" size_t cullavo_attn_decode_workspace(int B, int H, int max_len, int D) {
  const int64_t nchunk = cdiv((int64_t)std::max(max_len, 1), kChunk);
  return (size_t)B * H * nchunk * (D + 2) * sizeof(float);
}

extern "C" int cullavo_attn_decode_rope(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                        int64_t ldv, const int64_t* position_ids, float theta, void* k_cache,
                                        void* v_cache, int64_t ld_tok, int64_t ld_batch, const int32_t* start,
                                        const int32_t* kv_start, void* o, int64_t ldo, int B, int H, int max_len,
                                        int D, float scale, float* workspace, void* stream) {
  CV_REQUIRE(D == 128, CULLAVO_EUNSUPPORTED, "decode attention: head_dim 128");
  CV_REQUIRE(start != nullptr && position_ids != nullptr && workspace != nullptr && k != nullptr && v != nullptr,
             CULLAVO_EINVAL, "decode attention + rope: start / position_ids / workspace / k / v");
  CV_REQUIRE(ld_tok >= (int64_t)H * D && ldq >= (int64_t)H * D && ldk >= (int64_t)H * D && ldv >= (int64_t)H * D &&
                 ldo >= (int64_t)H * D && ld_tok % 8 == 0,
             CULLAVO_EINVAL, "decode attention + rope: strides");
  if (B == 0 || H == 0 || max_len <= 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int nchunk = (int)cdiv((int64_t)max_len, kChunk);
  float* part_o = workspace;
  float* part_ml = workspace + (int64_t)B * H * nchunk * D;
  DecodeRope rp{(const u16*)k, ldk, (const u16*)v, ldv, position_ids, theta, start, (u16*)k_cache, (u16*)v_cache};
  attn_decode_k<128, true><<<dim3(nchunk, H, B), 256, 0, s>>>((const u16*)q, ldq, (const u16*)k_cache,
                                                              (const u16*)v_cache, ld_tok, ld_batch, nullptr,
                                                              kv_start, scale * kLog2e, part_o, part_ml, H, nchunk, rp);
  attn_decode_combine_k<128><<<dim3(H, B), 128, 0, s>>>(part_o, part_ml, (u16*)o, ldo, H, nchunk);
  return cullavo_check_launch("attn_decode_rope");
}

extern "C" int cullavo_attn_decode(const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                   int64_t ld_tok, int64_t ld_batch, const int32_t* kv_len, const int32_t* kv_start,
                                   void* o, int64_t ldo, int B, int H, int max_len, int D, float scale,
                                   float* workspace, void* stream) {
  CV_REQUIRE(D == 128, CULLAVO_EUNSUPPORTED, "decode attention: head_dim 128");
  CV_REQUIRE(kv_len != nullptr && workspace != nullptr, CULLAVO_EINVAL, "decode attention: kv_len / workspace");
  CV_REQUIRE(ld_tok >= (int64_t)H * D && ldq >= (int64_t)H * D && ldo >= (int64_t)H * D && ld_tok % 8 == 0,
             CULLAVO_EINVAL, "decode attention: strides");
  if (B == 0 || H == 0 || max_len <= 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int nchunk = (int)cdiv((int64_t)max_len, kChunk);
  float* part_o = workspace;
  float* part_ml = workspace + (int64_t)B * H * nchunk * D;
  attn_decode_k<128><<<dim3(nchunk, H, B), 256, 0, s>>>((const u16*)q, ldq, (const u16*)k_cache,
                                                        (const u16*)v_cache, ld_tok, ld_batch, kv_len, kv_start,
                                                        scale * kLog2e, part_o, part_ml, H, nchunk);
  attn_decode_combine_k<128><<<dim3(H, B), 128, 0, s>>>(part_o, part_ml, (u16*)o, ldo, H, nchunk);
  return cullavo_check_launch("attn_decode");
}

namespace {
// the argument checks the two FP8 decode-attention entry points share (before any launch)
int decode_fp8_args(const char* what, const void* kc, const void* vc, int64_t ld_tok, int64_t ld_batch, const void* ke,
                    const void* ve, int64_t ld_etok, int64_t ldq, int64_t ldo, int H, int D, bool sim) {
  const std::string w(what);
  CV_REQUIRE(D == 128, CULLAVO_EUNSUPPORTED, w + ": head_dim 128");
  CV_REQUIRE(kc != nullptr && vc != nullptr, CULLAVO_EINVAL, w + ": the caches are null");
  CV_REQUIRE(sim || (ke != nullptr && ve != nullptr), CULLAVO_EINVAL, w + ": the exponent arrays are null");
  const int64_t al = sim ? 8 : 16;  // 16-byte rows: codes in bytes, the round-trip twin's bf16 in elements
  CV_REQUIRE(ld_tok >= (int64_t)H * D && ld_tok % al == 0 && ld_batch % al == 0 &&
                 (((uintptr_t)kc | (uintptr_t)vc) & 15) == 0,
             CULLAVO_EINVAL, w + ": 16-byte aligned cache rows of at least H*D");
  CV_REQUIRE(sim || ld_etok >= H, CULLAVO_EINVAL, w + ": exponent strides");
  CV_REQUIRE(ldq >= (int64_t)H * D && ldo >= (int64_t)H * D, CULLAVO_EINVAL, w + ": strides");
  return CULLAVO_OK;
}
}  // namespace

extern "C" int cullavo_attn_decode_fp8(const void* q, int64_t ldq, const void* k_codes, const void* v_codes,
                                       int64_t ld_tok, int64_t ld_batch, const void* k_exp, const void* v_exp,
                                       int64_t ld_etok, int64_t ld_ebatch, const int32_t* kv_len,
                                       const int32_t* kv_start, void* o, int64_t ldo, int B, int H, int max_len, int D,
                                       float scale, float* workspace, void* stream) {
  if (int rc = decode_fp8_args("attn_decode_fp8", k_codes, v_codes, ld_tok, ld_batch, k_exp, v_exp, ld_etok, ldq, ldo,
                               H, D, false))
    return rc;
  CV_REQUIRE(kv_len != nullptr && workspace != nullptr, CULLAVO_EINVAL, "attn_decode_fp8: kv_len / workspace");
  if (B == 0 || H == 0 || max_len <= 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int nchunk = (int)cdiv((int64_t)max_len, kChunk);
  float* part_o = workspace;
  float* part_ml = workspace + (int64_t)B * H * nchunk * D;
  DecodeFp8 f8{(const uint8_t*)k_exp, (const uint8_t*)v_exp, ld_etok, ld_ebatch, nullptr, nullptr};
  attn_decode_k<128, false, KV_FP8><<<dim3(nchunk, H, B), 256, 0, s>>>((const u16*)q, ldq, k_codes, v_codes, ld_tok,
                                                                       ld_batch, kv_len, kv_start, scale * kLog2e,
                                                                       part_o, part_ml, H, nchunk, DecodeRope{}, f8);
  attn_decode_combine_k<128><<<dim3(H, B), 128, 0, s>>>(part_o, part_ml, (u16*)o, ldo, H, nchunk);
  return cullavo_check_launch("attn_decode_fp8");
}

extern "C" int cullavo_attn_decode_rope_fp8(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                            int64_t ldv, const int64_t* position_ids, float theta, void* k_codes,
                                            void* v_codes, int64_t ld_tok, int64_t ld_batch, void* k_exp, void* v_exp,
                                            int64_t ld_etok, int64_t ld_ebatch, const int32_t* start,
                                            const int32_t* kv_start, void* o, int64_t ldo, int B, int H, int max_len,
                                            int D, float scale, int sim, float* workspace, void* stream) {
  if (int rc = decode_fp8_args("attn_decode_rope_fp8", k_codes, v_codes, ld_tok, ld_batch, k_exp, v_exp, ld_etok, ldq,
                               ldo, H, D, sim != 0))
    return rc;
  CV_REQUIRE(start != nullptr && position_ids != nullptr && workspace != nullptr && k != nullptr && v != nullptr,
             CULLAVO_EINVAL, "attn_decode_rope_fp8: start / position_ids / workspace / k / v");
  CV_REQUIRE(ldk >= (int64_t)H * D && ldv >= (int64_t)H * D, CULLAVO_EINVAL, "attn_decode_rope_fp8: strides");
  if (B == 0 || H == 0 || max_len <= 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  const int nchunk = (int)cdiv((int64_t)max_len, kChunk);
  float* part_o = workspace;
  float* part_ml = workspace + (int64_t)B * H * nchunk * D;
  DecodeRope rp{(const u16*)k, ldk, (const u16*)v, ldv, position_ids, theta, start, (u16*)k_codes, (u16*)v_codes};
  DecodeFp8 f8{(const uint8_t*)k_exp, (const uint8_t*)v_exp, ld_etok, ld_ebatch, (uint8_t*)k_exp, (uint8_t*)v_exp};
  if (sim)
    attn_decode_k<128, true, KV_SIM><<<dim3(nchunk, H, B), 256, 0, s>>>((const u16*)q, ldq, k_codes, v_codes, ld_tok,
                                                                        ld_batch, nullptr, kv_start, scale * kLog2e,
                                                                        part_o, part_ml, H, nchunk, rp, f8);
  else
    attn_decode_k<128, true, KV_FP8><<<dim3(nchunk, H, B), 256, 0, s>>>((const u16*)q, ldq, k_codes, v_codes, ld_tok,
                                                                        ld_batch, nullptr, kv_start, scale * kLog2e,
                                                                        part_o, part_ml, H, nchunk, rp, f8);
  attn_decode_combine_k<128><<<dim3(H, B), 128, 0, s>>>(part_o, part_ml, (u16*)o, ldo, H, nchunk);
  return cullavo_check_launch("attn_decode_rope_fp8");
}
