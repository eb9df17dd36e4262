// Flash attention for the shapes the MFMA kernels of attention.hip do not take: f32 storage
// (the f32 parity mode, SURVEY.md §7 "Hard parts: parity tolerance") and head dims 16 / 32
// (BASELINE config 1: ViT 64/4, LM 128/4). Same contract as cullavo_attn_fwd / _bwd
// (tf:llama/modeling_llama.py:191-214 eager attention with an f32 softmax,
// tf:clip/modeling_clip.py:280-336): lse in natural log, fully masked rows -> zero output and
// lse = +inf, kv_start masks left padding.
//
// Arithmetic is f32 on the VALU with operands staged in LDS (64 keys per block): these shapes
// are test / tiny-model sizes, where the exact f32 chain matters and the FLOPs do not. The
// backward recomputes P from lse (no stored probabilities): delta = rowsum(dO*O), one kernel
// for dK/dV (a workgroup per 64-key block, query blocks of 32 streamed) and one for dQ.
#include "common.h"

namespace {

constexpr int KB = 64;   // keys per block
constexpr int QF = 64;   // query rows per forward / dQ workgroup
constexpr int QB = 32;   // query rows per dK/dV inner block

template <typename T>
DEV void stage_rows(float* dst, int ld_dst, const T* src, int64_t ld_src, int64_t row0, int nrows_valid, int nrows,
                    int D) {
  for (int idx = threadIdx.x; idx < nrows * D; idx += 256) {
    const int r = idx / D, c = idx - r * D;
    dst[r * ld_dst + c] = r < nrows_valid ? Elt<T>::ld(src, (row0 + r) * ld_src + c) : 0.f;
  }
}

// stage_rows with zeros in place of rows r < r_lo as well: the V rows of cache keys below kv_start.
// Their probability is 0, but the output takes fmaf(0, v, o), which a non-finite v turns into NaN;
// for a finite cache fmaf(0, v, o) and fmaf(0, 0, o) are the same value.
template <typename T>
DEV void stage_rows_from(float* dst, int ld_dst, const T* src, int64_t ld_src, int64_t row0, int r_lo,
                         int nrows_valid, int nrows, int D) {
  for (int idx = threadIdx.x; idx < nrows * D; idx += 256) {
    const int r = idx / D, c = idx - r * D;
    dst[r * ld_dst + c] = (r >= r_lo && r < nrows_valid) ? Elt<T>::ld(src, (row0 + r) * ld_src + c) : 0.f;
  }
}

DEV bool visible(int64_t qg, int64_t jg, int Lk, int ks, bool causal) {
  return jg < Lk && jg >= ks && (!causal || jg <= qg);
}

// ---- forward -----------------------------------------------------------------------------------
// thread t: query row r = t >> 2, keys j = part + 4 i (i < 16), output columns part + 4 c
// CACHED (cullavo_attn_fwd_cached; causal): the Lq queries are the last Lq positions of Lk = past +
// Lq keys (query i sees keys <= past + i), K / V are one layer's KV cache, both with token stride
// ldk, sequence b at element offset b * ldv (ldv carries the cache's batch stride); rows >= Lk of
// the cache are never staged, and V rows below kv_start[b] are staged as zeros (stage_rows_from): the
// output is finite whatever those rows hold. lse may then be null. The packed kernel (CACHED false)
// stages every row below Lk: its K / V must be finite below kv_start too.
// RAGGED (cullavo_attn_fwd_ragged; CACHED, causal): Lk is sequence b's own kv_len[b] and the first
// qpad = q_pad[b] queries of its left-padded block are padding -- they see no key (a zero row, lse =
// +inf), and a query block wholly inside the padding stages no key block. Lk - Lq may be negative.
template <typename T, int D, bool CACHED>
__global__ __launch_bounds__(256) void attn_gen_fwd_k(const T* __restrict__ Q, int64_t ldq, const T* __restrict__ K,
                                                      int64_t ldk, const T* __restrict__ V, int64_t ldv,
                                                      T* __restrict__ O, int64_t ldo, float* __restrict__ LSE, int H,
                                                      int Lq, int Lk, float scale, int causal,
                                                      const int32_t* __restrict__ kv_start) {
  constexpr bool RAGGED = false;
  constexpr int qpad = 0;
#include "attn_gen_fwd_body.h"
}

// kv_len[b] clamped to [0, cap] (cap: the rows of a sequence's slab) and q_pad[b] to [0, Lq]: device
// values the host cannot check must not stage rows outside the slab
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_gen_fwd_ragged_k(const T* __restrict__ Q, int64_t ldq,
                                                             const T* __restrict__ K, int64_t ldk,
                                                             const T* __restrict__ V, int64_t ldv,
                                                             T* __restrict__ O, int64_t ldo, float* __restrict__ LSE,
                                                             int H, int Lq, int cap, float scale,
                                                             const int32_t* __restrict__ kv_start,
                                                             const int32_t* __restrict__ kv_len,
                                                             const int32_t* __restrict__ q_pad) {
  constexpr bool CACHED = true, RAGGED = true;
  constexpr int causal = 1;
  const int seq = blockIdx.x / ((int)cdiv(Lq, QF) * H);  // the body's b
  const int Lk = min(max(kv_len[seq], 0), cap);
  const int qpad = q_pad ? min(max(q_pad[seq], 0), Lq) : 0;
#include "attn_gen_fwd_body.h"
}

// ---- backward -----------------------------------------------------------------------------------
// delta[b,h,q] = sum_d dO*O (one wave per row)
template <typename T>
__global__ __launch_bounds__(256) void attn_gen_delta_k(const T* __restrict__ O, int64_t ldo, const T* __restrict__ dO,
                                                        int64_t lddo, float* __restrict__ delta, int H, int Lq,
                                                        int D, int64_t rows) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int q = (int)(row % Lq), h = (int)((row / Lq) % H), b = (int)(row / ((int64_t)Lq * H));
  const int64_t tok = (int64_t)b * Lq + q;
  float acc = 0.f;
  for (int d = lane; d < D; d += 64)
    acc += Elt<T>::ld(dO, tok * lddo + h * D + d) * Elt<T>::ld(O, tok * ldo + h * D + d);
  acc = wave_sum(acc);
  if (lane == 0) delta[row] = acc;
}

// dK, dV of one 64-key block; query blocks of QB rows streamed. Phase 1: thread (query row
// rq = t >> 3, keys j = part + 8 i) computes P and dS into LDS; phase 2: thread (key row
// kr = t >> 2, columns part + 4 c) accumulates dV += P^T dO, dK += dS^T Q.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_gen_bwd_kv_k(const T* __restrict__ Q, int64_t ldq, const T* __restrict__ K,
                                                         int64_t ldk, const T* __restrict__ V, int64_t ldv,
                                                         const T* __restrict__ dO, int64_t lddo,
                                                         const float* __restrict__ LSE,
                                                         const float* __restrict__ DELTA, T* __restrict__ dK,
                                                         int64_t lddk, T* __restrict__ dV, int64_t lddv, int H, int Lq,
                                                         int Lk, float scale, int causal,
                                                         const int32_t* __restrict__ kv_start) {
  constexpr int LD = D + 1;
  extern __shared__ float sm[];
  float* sK = sm;
  float* sV = sK + KB * LD;
  float* sQ = sV + KB * LD;
  float* sdO = sQ + QB * LD;
  float* sP = sdO + QB * LD;       // [QB][KB + 1]
  float* sdS = sP + QB * (KB + 1);  // [QB][KB + 1]
  float* sL = sdS + QB * (KB + 1);  // lse [QB]
  float* sD = sL + QB;              // delta [QB]
  const int nkb = (int)cdiv(Lk, KB);
  const int kb = blockIdx.x % nkb, h = (blockIdx.x / nkb) % H, b = blockIdx.x / (nkb * H);
  const int k0 = kb * KB;
  const int t = threadIdx.x;
  const int ks = kv_start ? kv_start[b] : 0;
  stage_rows<T>(sK, LD, K + h * D, ldk, (int64_t)b * Lk + k0, min(KB, Lk - k0), KB, D);
  stage_rows<T>(sV, LD, V + h * D, ldv, (int64_t)b * Lk + k0, min(KB, Lk - k0), KB, D);
  const int kr = t >> 2, part4 = t & 3;
  float dk[D / 4], dv[D / 4];
#pragma unroll
  for (int c = 0; c < D / 4; ++c) dk[c] = dv[c] = 0.f;
  const int rq = t >> 3, part8 = t & 7;
  const int qstart = causal ? (k0 / QB) * QB : 0;
  for (int q0 = qstart; q0 < Lq; q0 += QB) {
    __syncthreads();
    stage_rows<T>(sQ, LD, Q + h * D, ldq, (int64_t)b * Lq + q0, min(QB, Lq - q0), QB, D);
    stage_rows<T>(sdO, LD, dO + h * D, lddo, (int64_t)b * Lq + q0, min(QB, Lq - q0), QB, D);
    if (t < QB) {
      const int q = q0 + t;
      sL[t] = q < Lq ? LSE[((int64_t)b * H + h) * Lq + q] : INFINITY;
      sD[t] = q < Lq ? DELTA[((int64_t)b * H + h) * Lq + q] : 0.f;
    }
    __syncthreads();
    const int64_t qg = q0 + rq;
#pragma unroll
    for (int i = 0; i < KB / 8; ++i) {
      const int j = part8 + 8 * i;
      float sacc = 0.f, dpacc = 0.f;
      for (int d = 0; d < D; ++d) {
        sacc = fmaf(sQ[rq * LD + d], sK[j * LD + d], sacc);
        dpacc = fmaf(sdO[rq * LD + d], sV[j * LD + d], dpacc);
      }
      const bool ok = qg < Lq && visible(qg, k0 + j, Lk, ks, causal) && sL[rq] != INFINITY;
      const float p = ok ? __expf(sacc * scale - sL[rq]) : 0.f;
      sP[rq * (KB + 1) + j] = p;
      sdS[rq * (KB + 1) + j] = p * (dpacc - sD[rq]);
    }
    __syncthreads();
    for (int r = 0; r < QB; ++r) {
      const float p = sP[r * (KB + 1) + kr], ds = sdS[r * (KB + 1) + kr];
#pragma unroll
      for (int c = 0; c < D / 4; ++c) {
        dv[c] = fmaf(p, sdO[r * LD + part4 + 4 * c], dv[c]);
        dk[c] = fmaf(ds, sQ[r * LD + part4 + 4 * c], dk[c]);
      }
    }
  }
  const int64_t kg = k0 + kr;
  if (kg < Lk) {
    T* dkp = dK + ((int64_t)b * Lk + kg) * lddk + h * D;
    T* dvp = dV + ((int64_t)b * Lk + kg) * lddv + h * D;
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
      Elt<T>::st(dkp, part4 + 4 * c, dk[c] * scale);
      Elt<T>::st(dvp, part4 + 4 * c, dv[c]);
    }
  }
}

// dQ of one 64-row query block, key blocks streamed; thread (row r = t >> 2, keys
// part + 4 i) forms dS, then (row r, columns part + 4 c) accumulates dQ += dS K.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_gen_bwd_q_k(const T* __restrict__ Q, int64_t ldq, const T* __restrict__ K,
                                                        int64_t ldk, const T* __restrict__ V, int64_t ldv,
                                                        const T* __restrict__ dO, int64_t lddo,
                                                        const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                        T* __restrict__ dQ, int64_t lddq, int H, int Lq, int Lk,
                                                        float scale, int causal, const int32_t* __restrict__ kv_start) {
  constexpr int LD = D + 1;
  extern __shared__ float sm[];
  float* sQ = sm;
  float* sdO = sQ + QF * LD;
  float* sK = sdO + QF * LD;
  float* sV = sK + KB * LD;
  float* sdS = sV + KB * LD;  // [QF][KB + 1]
  const int nqb = (int)cdiv(Lq, QF);
  const int qb = blockIdx.x % nqb, h = (blockIdx.x / nqb) % H, b = blockIdx.x / (nqb * H);
  const int q0 = qb * QF;
  const int t = threadIdx.x, r = t >> 2, part = t & 3;
  const int ks = kv_start ? kv_start[b] : 0;
  const int64_t qg = q0 + r;
  stage_rows<T>(sQ, LD, Q + h * D, ldq, (int64_t)b * Lq + q0, min(QF, Lq - q0), QF, D);
  stage_rows<T>(sdO, LD, dO + h * D, lddo, (int64_t)b * Lq + q0, min(QF, Lq - q0), QF, D);
  const float lse = qg < Lq ? LSE[((int64_t)b * H + h) * Lq + qg] : INFINITY;
  const float del = qg < Lq ? DELTA[((int64_t)b * H + h) * Lq + qg] : 0.f;
  float dq[D / 4];
#pragma unroll
  for (int c = 0; c < D / 4; ++c) dq[c] = 0.f;
  const int kend = causal ? min(Lk, q0 + QF) : Lk;
  for (int k0 = 0; k0 < kend; k0 += KB) {
    __syncthreads();
    stage_rows<T>(sK, LD, K + h * D, ldk, (int64_t)b * Lk + k0, min(KB, Lk - k0), KB, D);
    stage_rows<T>(sV, LD, V + h * D, ldv, (int64_t)b * Lk + k0, min(KB, Lk - k0), KB, D);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KB / 4; ++i) {
      const int j = part + 4 * i;
      float sacc = 0.f, dpacc = 0.f;
      for (int d = 0; d < D; ++d) {
        sacc = fmaf(sQ[r * LD + d], sK[j * LD + d], sacc);
        dpacc = fmaf(sdO[r * LD + d], sV[j * LD + d], dpacc);
      }
      const bool ok = qg < Lq && visible(qg, k0 + j, Lk, ks, causal) && lse != INFINITY;
      const float p = ok ? __expf(sacc * scale - lse) : 0.f;
      sdS[r * (KB + 1) + j] = p * (dpacc - del);
    }
    __syncthreads();
    for (int j = 0; j < KB; ++j) {
      const float ds = sdS[r * (KB + 1) + j];
#pragma unroll
      for (int c = 0; c < D / 4; ++c) dq[c] = fmaf(ds, sK[j * LD + part + 4 * c], dq[c]);
    }
  }
  if (qg < Lq) {
    T* qp = dQ + ((int64_t)b * Lq + qg) * lddq + h * D;
#pragma unroll
    for (int c = 0; c < D / 4; ++c) Elt<T>::st(qp, part + 4 * c, dq[c] * scale);
  }
}

template <typename T, int D>
int gen_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
            float* lse, int B, int H, int Lq, int Lk, float scale, int causal, const int32_t* ks, hipStream_t s) {
  constexpr int LD = D + 1;
  const int smem = (QF * LD + 2 * KB * LD + QF * (KB + 1)) * 4;
  static bool once = false;
  if (!once) {
    (void)hipFuncSetAttribute((const void*)attn_gen_fwd_k<T, D, false>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    once = true;
  }
  const unsigned grid = (unsigned)(cdiv(Lq, QF) * H * B);
  attn_gen_fwd_k<T, D, false><<<grid, 256, smem, s>>>((const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (T*)o, ldo, lse,
                                               H, Lq, Lk, scale, causal, ks);
  return cullavo_check_launch("attn_fwd (generic)");
}

template <typename T, int D>
int gen_fwd_cached(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ld_tok, int64_t ld_batch,
                   void* o, int64_t ldo, float* lse, int B, int H, int Lq, int past, float scale, const int32_t* ks,
                   hipStream_t s) {
  constexpr int LD = D + 1;
  const int smem = (QF * LD + 2 * KB * LD + QF * (KB + 1)) * 4;
  static bool once = false;
  if (!once) {
    (void)hipFuncSetAttribute((const void*)attn_gen_fwd_k<T, D, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              smem);
    once = true;
  }
  const unsigned grid = (unsigned)(cdiv(Lq, QF) * H * B);
  // (K, its token stride, V, the batch stride: see the kernel's CACHED note)
  attn_gen_fwd_k<T, D, true><<<grid, 256, smem, s>>>((const T*)q, ldq, (const T*)kc, ld_tok, (const T*)vc, ld_batch,
                                                     (T*)o, ldo, lse, H, Lq, past + Lq, scale, 1, ks);
  return cullavo_check_launch("attn_fwd_cached (generic)");
}

template <typename T, int D>
int gen_fwd_ragged(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ld_tok, int64_t ld_batch,
                   void* o, int64_t ldo, float* lse, int B, int H, int Lq, int cap, float scale, const int32_t* ks,
                   const int32_t* kv_len, const int32_t* q_pad, hipStream_t s) {
  constexpr int LD = D + 1;
  const int smem = (QF * LD + 2 * KB * LD + QF * (KB + 1)) * 4;
  static bool once = false;
  if (!once) {
    (void)hipFuncSetAttribute((const void*)attn_gen_fwd_ragged_k<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              smem);
    once = true;
  }
  const unsigned grid = (unsigned)(cdiv(Lq, QF) * H * B);
  attn_gen_fwd_ragged_k<T, D><<<grid, 256, smem, s>>>((const T*)q, ldq, (const T*)kc, ld_tok, (const T*)vc, ld_batch,
                                                      (T*)o, ldo, lse, H, Lq, cap, scale, ks, kv_len, q_pad);
  return cullavo_check_launch("attn_fwd_ragged (generic)");
}

template <typename T, int D>
int gen_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
            int64_t ldo, const void* dout, int64_t lddo, const float* lse, float* delta, void* dq, int64_t lddq,
            void* dk, int64_t lddk, void* dv, int64_t lddv, int B, int H, int Lq, int Lk, float scale, int causal,
            const int32_t* ks, hipStream_t s) {
  constexpr int LD = D + 1;
  const int smem_kv = (2 * KB * LD + 2 * QB * LD + 2 * QB * (KB + 1) + 2 * QB) * 4;
  const int smem_q = (2 * QF * LD + 2 * KB * LD + QF * (KB + 1)) * 4;
  static bool once = false;
  if (!once) {
    (void)hipFuncSetAttribute((const void*)attn_gen_bwd_kv_k<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              smem_kv);
    (void)hipFuncSetAttribute((const void*)attn_gen_bwd_q_k<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize, smem_q);
    once = true;
  }
  const int64_t rows = (int64_t)B * H * Lq;
  attn_gen_delta_k<T><<<(unsigned)cdiv(rows, 4), 256, 0, s>>>((const T*)o, ldo, (const T*)dout, lddo, delta, H, Lq, D,
                                                               rows);
  attn_gen_bwd_kv_k<T, D><<<(unsigned)(cdiv(Lk, KB) * H * B), 256, smem_kv, s>>>(
      (const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (const T*)dout, lddo, lse, delta, (T*)dk, lddk, (T*)dv,
      lddv, H, Lq, Lk, scale, causal, ks);
  attn_gen_bwd_q_k<T, D><<<(unsigned)(cdiv(Lq, QF) * H * B), 256, smem_q, s>>>(
      (const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (const T*)dout, lddo, lse, delta, (T*)dq, lddq, H, Lq, Lk,
      scale, causal, ks);
  return cullavo_check_launch("attn_bwd (generic)");
}

// f(T{}, std::integral_constant<int, D>{}) for the storage type (float, else bf16 as u16) and the head
// dim the entry points of attention.hip hand over (theirs: f32 storage or D in {16, 32})
template <typename F>
int by_type_and_dim(int dtype, int D, F&& f) {
  auto by_dim = [&](auto t) {
    switch (D) {
      case 16: return f(t, std::integral_constant<int, 16>{});
      case 32: return f(t, std::integral_constant<int, 32>{});
      case 64: return f(t, std::integral_constant<int, 64>{});
      case 128: return f(t, std::integral_constant<int, 128>{});
      default: break;
    }
    cullavo_set_error("attention: head_dim must be 16, 32, 64 or 128");
    return (int)CULLAVO_EUNSUPPORTED;
  };
  return dtype == CULLAVO_DT_F32 ? by_dim(float{}) : by_dim(u16{});
}

}  // namespace

int cullavo_attn_generic_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                             void* o, int64_t ldo, float* lse, int B, int H, int Lq, int Lk, int D, float scale,
                             int causal, const int32_t* ks, int dtype, hipStream_t s) {
  return by_type_and_dim(dtype, D, [&](auto t, auto d) {
    return gen_fwd<decltype(t), decltype(d)::value>(q, ldq, k, ldk, v, ldv, o, ldo, lse, B, H, Lq, Lk, scale, causal,
                                                    ks, s);
  });
}

int cullavo_attn_generic_fwd_cached(const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                    int64_t ld_tok, int64_t ld_batch, void* o, int64_t ldo, float* lse, int B, int H,
                                    int Lq, int past, int D, float scale, const int32_t* ks, int dtype, hipStream_t s) {
  return by_type_and_dim(dtype, D, [&](auto t, auto d) {
    return gen_fwd_cached<decltype(t), decltype(d)::value>(q, ldq, k_cache, v_cache, ld_tok, ld_batch, o, ldo, lse, B,
                                                           H, Lq, past, scale, ks, s);
  });
}

int cullavo_attn_generic_fwd_ragged(const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                    int64_t ld_tok, int64_t ld_batch, void* o, int64_t ldo, float* lse, int B, int H,
                                    int Lq, int cap, int D, float scale, const int32_t* ks, const int32_t* kv_len,
                                    const int32_t* q_pad, int dtype, hipStream_t s) {
  return by_type_and_dim(dtype, D, [&](auto t, auto d) {
    return gen_fwd_ragged<decltype(t), decltype(d)::value>(q, ldq, k_cache, v_cache, ld_tok, ld_batch, o, ldo, lse, B,
                                                           H, Lq, cap, scale, ks, kv_len, q_pad, s);
  });
}

int cullavo_attn_generic_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                             const void* o, int64_t ldo, const void* dout, int64_t lddo, const float* lse,
                             float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                             int B, int H, int Lq, int Lk, int D, float scale, int causal, const int32_t* ks,
                             int dtype, hipStream_t s) {
  return by_type_and_dim(dtype, D, [&](auto t, auto d) {
    return gen_bwd<decltype(t), decltype(d)::value>(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, delta, dq, lddq,
                                                    dk, lddk, dv, lddv, B, H, Lq, Lk, scale, causal, ks, s);
  });
}
