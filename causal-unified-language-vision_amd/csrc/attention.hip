// Flash attention forward/backward for gfx950 (v_mfma_f32_32x32x16_bf16).
//
// Replaces the LM's causal attention (FA2 in the reference: cullavo/load_cullavo.py:72;
// arithmetic of tf:llama/modeling_llama.py:191-214, scale 1/sqrt(128)) and CLIP's non-causal
// attention (tf:clip/modeling_clip.py:280-336, scale 1/8). Tensors are [B, L, H, D] with a
// token stride, i.e. the q/k/v projection outputs are consumed in place.
//
// Forward: a wave owns 32 query rows; the 4 waves of a workgroup share 64-key K/V tiles in
// LDS (double-buffered, register-staged, one barrier per tile). Scores are computed swapped,
// S^T = K Q^T, so every lane owns one query row: the online-softmax row max/sum is 32 register
// ops plus one cross-half shuffle, P^T feeds the P·V MFMA straight from the accumulator
// registers (O^T = V^T P^T) and V^T fragments come from ds_read_b64_tr_b16 transposed reads.
// Backward: kernel A (per 32-key slice per wave: dV = P^T dO, dK = dS^T Q) and kernel B (per
// 32-query slice: dQ = dS K), both recomputing P from the saved log-sum-exp; no atomics, so
// results are bitwise reproducible.
#include "common.h"

#include <vector>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 frag8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr float kLog2e = 1.4426950408889634f;

// bijective XCD-aware block remap (as in gemm.hip; cdna_hip_programming.md §5)
DEV int xcd_remap(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}
constexpr float kLn2 = 0.6931471805599453f;
constexpr int kVmcnt0 = 0x0F70;  // s_waitcnt vmcnt(0) expcnt(7) lgkmcnt(15) (gfx9 encoding)

// bare v_exp_f32: results below 2^-126 flush to zero (softmax weights that small are noise);
// exp2f adds a denormal range fix-up (compare, select, ldexp) around every call
DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// LDS image of a [rows][D] bf16 tile, 16-byte chunk ch of row r. D=128: the dual-use XOR
// image (conflict-free for both the row reads and the tr16 reads, cdna_hip_programming.md
// T10 (b)); D=64: chunk ^ ((r>>1)&7) (row reads conflict-free, tr reads 2-way).
template <int D>
DEV int kv_off(int r, int ch) {
  if (D == 128) return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3)));
  return 128 * r + 16 * (ch ^ ((r >> 1) & 7));
}

// row fragment for a 32x32x16 operand: lane holds T[rbase + (lane&31)][16s + 8h + j]
template <int D>
DEV frag8 row_frag(const char* lds, int rbase, int s, int lane) {
  const int r = rbase + (lane & 31), ch = 2 * s + (lane >> 5);
  return __builtin_bit_cast(frag8, *reinterpret_cast<const u16x8*>(lds + kv_off<D>(r, ch)));
}

// transposed fragment: lane holds T[kb + 8(j>>2) + 4h + (j&3)][d0 + (lane&31)], j = 0..7
// (the k order of an accumulator tile used as the other MFMA operand, guide §3)
template <int D>
DEV frag8 tr_frag(const char* lds, int kb, int d0, int lane) {
  const int h = lane >> 5, i = lane & 15, q = i >> 2, p = i & 3;
  const int dcol = d0 + 16 * ((lane >> 4) & 1);
  const int ch = (dcol >> 3) + (p >> 1);
  const int r0 = kb + 4 * h + q;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + kv_off<D>(r0, ch) + 8 * (p & 1)));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + kv_off<D>(r0 + 8, ch) + 8 * (p & 1)));
  s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(frag8, v);
}

// fragment reads at precomputed LDS addresses (see attn_fwd_k): a row fragment, and a
// transposed fragment from its two ds_read_b64_tr_b16 halves (tr_frag's lo / hi)
// (LDS byte addresses as integers, so a read is one VGPR plus its immediate offset)
typedef __attribute__((address_space(3))) u16x8 lds_u16x8;
DEV unsigned lds_addr(const char* p) { return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p; }
DEV frag8 lds_frag(unsigned a) { return __builtin_bit_cast(frag8, *(const lds_u16x8*)(uintptr_t)a); }
DEV frag8 lds_tr_frag(unsigned lo_a, unsigned hi_a) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)lo_a);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)hi_a);
  s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(frag8, v);
}

// accumulator registers 8s..8s+7 of a 32x32 tile -> bf16 operand fragment
DEV frag8 pack_frag(const f32x16& a, int s) {
  frag8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (__bf16)a[8 * s + j];
  return f;
}

__device__ float g_rescale_thr = 8.f;  // forward's deferred-rescale threshold (cullavo_attn_set_rescale)
// forward kernel (cullavo_attn_set_stage): 4 = attn_fwd_k, the plain LDS-DMA kernel; 7 = the
// software-pipelined attn_fwd_pipe_k, bitwise equal to 4; -1 (default) = 7 (7B layer 151 ->
// 124-128 us, ViT bs-64 layer 148-154 -> 139-144 us alternating on one box,
// profiles/r04/attn/attn_fwd_ab.txt). The register-staged forms 0-3 and the inline-asm form 5 of
// rounds 2-3 left with ABI 6 ("measured, not kept")
int g_fwd_stage = -1;

// global -> registers -> LDS staging of a [ROWS][D] tile of a [L, H, D]-strided tensor (the
// 4-wave backward kernels)
template <int ROWS, int D>
struct Stage {
  static constexpr int kChunks = ROWS * D / 8;
  static constexpr int kPer = kChunks / 256;  // 16-byte chunks per thread
  u16x8 r[kPer];
  DEV void load(const u16* base, int64_t ld, int row0, int nrows) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int q = threadIdx.x + 256 * i;
      const int row = q / (D / 8), ch = q % (D / 8);
      r[i] = (row0 + row < nrows) ? *reinterpret_cast<const u16x8*>(base + (int64_t)(row0 + row) * ld + ch * 8)
                                  : u16x8(0);
    }
  }
  DEV void store(char* lds) const {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int q = threadIdx.x + 256 * i;
      const int row = q / (D / 8), ch = q % (D / 8);
      *reinterpret_cast<u16x8*>(lds + kv_off<D>(row, ch)) = r[i];
    }
  }
};

// Per-tile descriptor staging through registers (the dQ-from-dS^T kernel): the buffer descriptor is
// rebuilt per tile from scalars (base advanced to the tile's first row, num_records covering only
// the rows that exist, so rows past the sequence end read as zeros), every lane keeps ONE
// loop-invariant byte offset, and the i-th chunk's row step (i * rows-per-pass * ld) is the
// instruction's scalar offset: no per-tile VALU address arithmetic, compares or selects.
template <int ROWS, int D>
struct StageT {
  static constexpr int NT = 256;                  // threads of the workgroup
  static constexpr int kPer = ROWS * D / 8 / NT;  // 16-byte chunks per thread
  static constexpr int kPass = NT / (D / 8);      // rows covered by one pass of NT threads
  static_assert(kPer * NT * 8 == ROWS * D && NT % (D / 8) == 0, "tile must split evenly over the threads");
  u16x8 r[kPer];
  DEV static unsigned lane_off(int64_t ld) {
    return (unsigned)(((int64_t)(threadIdx.x / (D / 8)) * ld + (threadIdx.x % (D / 8)) * 8) * 2);
  }
  DEV void load(const u16* base, int64_t ld, int row0, int nrows, unsigned vo) {
    const int left = min(nrows - row0, ROWS);
    const int bytes = left > 0 ? (int)(((int64_t)(left - 1) * ld + D) * 2) : 0;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)row0 * ld), (short)0, bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      r[i] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (int)(i * kPass * ld * 2), 0));
  }
  DEV void store(char* lds) const {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int q = threadIdx.x + NT * i;
      *reinterpret_cast<u16x8*>(lds + kv_off<D>(q / (D / 8), q % (D / 8))) = r[i];
    }
  }
};

// LDS-DMA staging of a [ROWS][D] tile (attn_fwd_k, the 8-wave dK/dV kernel): buffer_load ... lds writes each
// 1 KiB piece lane-linearly (lane i -> byte 16 i of the piece), so the kv_off XOR image is
// produced by permuting the SOURCE chunk: the lane landing in slot s of image row r loads chunk
// s ^ swizzle(r) (the swizzle is an involution). No staging VGPRs and no ds_write: the data goes
// HBM/L2 -> LDS directly. Pieces are dealt round-robin over NW waves; the per-lane offsets are
// loop-invariant (rows relative to the tile origin, which the per-tile descriptor carries, as in
// StageT: rows past the sequence end fall outside num_records and land as zeros).
typedef __attribute__((address_space(3))) void lds_void_t;
// (a free function: the builtin inside a member function made the host pass drop the kernel
// stubs of every instantiation using it, silently -- undefined symbols at load)
DEV void lds_dma16(__amdgpu_buffer_rsrc_t rs, char* lds, unsigned vo) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)lds, 16, vo, 0, 0, 0);
}
template <int ROWS, int D, int NW>
struct StageDMA {
  static constexpr int kRP = 1024 / (2 * D);            // image rows per 1 KiB piece
  static constexpr int kPieces = ROWS / kRP;
  static constexpr int kPer = kPieces / NW;             // pieces per wave
  static_assert(kPer * NW == kPieces, "pieces must split evenly over the waves");
  unsigned vo[kPer];
  DEV void prep(int64_t ld, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int pc = wave + NW * i;
      const int r = pc * kRP + lane / (D / 8), s = lane % (D / 8);
      const int sw = D == 128 ? (((r & 3) << 2) | ((r >> 2) & 3)) : ((r >> 1) & 7);
      vo[i] = (unsigned)(((int64_t)r * ld + (s ^ sw) * 8) * 2);
    }
  }
  DEV void issue(const u16* base, int64_t ld, int row0, int nrows, char* lds, int wave) const {
    const int left = min(nrows - row0, ROWS);
    const int bytes = left > 0 ? (int)(((int64_t)(left - 1) * ld + D) * 2) : 0;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)row0 * ld), (short)0, bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      lds_dma16(rs, lds + (wave + NW * i) * 1024, vo[i]);
  }
};

// StageDMA with one per-lane offset: piece i sits NW * kRP rows (a multiple of 16) below piece 0,
// where the image swizzle (a function of row & 15) repeats, so its source offset is piece 0's
// plus a wave-uniform row step, passed as the instruction's scalar offset (inside the buffer's
// range check like the per-lane part; tests/test_oob_guard.py)
DEV void lds_dma16s(__amdgpu_buffer_rsrc_t rs, char* lds, unsigned vo, int so) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)lds, 16, vo, so, 0, 0);
}
template <int ROWS, int D, int NW>
struct StageDMA1 {
  static constexpr int kRP = 1024 / (2 * D);
  static constexpr int kPer = ROWS / kRP / NW;
  static_assert(kPer * NW * kRP == ROWS && (NW * kRP) % 16 == 0, "pieces must split evenly, 16-row steps");
  unsigned vo;
  DEV void prep(int64_t ld, int wave, int lane) {
    const int r = wave * kRP + lane / (D / 8), s = lane % (D / 8);
    const int sw = D == 128 ? (((r & 3) << 2) | ((r >> 2) & 3)) : ((r >> 1) & 7);
    vo = (unsigned)(((int64_t)r * ld + (s ^ sw) * 8) * 2);
  }
  DEV void issue(const u16* base, int64_t ld, int row0, int nrows, char* lds, int wave) const {
    const int left = min(nrows - row0, ROWS);
    const int bytes = left > 0 ? (int)(((int64_t)(left - 1) * ld + D) * 2) : 0;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)row0 * ld), (short)0, bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < kPer; ++i) lds_dma16s(rs, lds + (wave + NW * i) * 1024, vo, (int)(i * NW * kRP * ld * 2));
  }
};

// Which rows a kernel's sequences own. The backward kernels take it in kv_start's place (a trailing
// template argument SEQ; attn_bwd_dkdv8_k through its included body), as one of
//   const int32_t*  the uniform [B, L] grid: sequence b owns rows b L .. b L + L - 1, the pointer is
//                   kv_start (keys below kv_start[b] are masked; null = none);
//   VarSeq          sequences of unequal length packed back to back (cullavo_attn_*_varlen):
//                   sequence b owns rows start[b] .. start[b] + len[b] - 1, the grid and the lse /
//                   delta rows are sized by max_len, and there is no kv_start.
// The uniform overloads return the kernel's own arguments, so those instantiations compile to the
// code they were before the varlen ones existed (tools/isa_diff.py). len[b] is a device value the
// host cannot check: it is clamped to [0, max_len], so no value indexes lse / delta or the dS^T
// workspace outside sequence b's part. All loads are from workgroup-uniform addresses.
struct VarSeq {
  const int32_t* start;
  const int32_t* len;
  int max_len;
};
template <class SEQ>
constexpr bool kVarlen = std::is_same<SEQ, VarSeq>::value;
DEV int seq_grid_rows(const int32_t*, int L) { return L; }          // rows the grid / lse stride covers
DEV int seq_grid_rows(const VarSeq& s, int) { return s.max_len; }
DEV int seq_grid_rows(int L) { return L; }                          // (attn_delta_k: L in the SEQ's place)
DEV int seq_grid_rows(const VarSeq& s) { return s.max_len; }
DEV int seq_rows(const int32_t*, int, int L) { return L; }          // rows of sequence b
DEV int seq_rows(const VarSeq& s, int b, int) { return min(max(s.len[b], 0), s.max_len); }
DEV int64_t seq_row0(const int32_t*, int b, int L) { return (int64_t)b * L; }  // its first row
DEV int64_t seq_row0(const VarSeq& s, int b, int) { return s.start[b]; }
DEV int seq_kstart(const int32_t* ks, int b) { return ks ? ks[b] : 0; }
DEV int seq_kstart(const VarSeq&, int) { return 0; }
// the kernel argument's type: the uniform grid's kv_start keeps its __restrict__
template <class SEQ>
struct SeqArg { using type = SEQ; };
template <>
struct SeqArg<const int32_t*> { using type = const int32_t* __restrict__; };

// row of accumulator register r of a 32x32 tile for lane half h
DEV int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// a transposed fragment from its two ds_read_b64_tr_b16 halves
DEV frag8 tr_join(const s16x4& lo, const s16x4& hi) {
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(frag8, v);
}

// four row fragments by inline-asm ds_read_b128 / four transposed halves by ds_read_b64_tr_b16
// (issued together), and the counted lgkmcnt wait that ties a group's registers before use
DEV void rd4(s16x8& a, s16x8& b, s16x8& c, s16x8& d, unsigned pa, unsigned pb, unsigned pc, unsigned pd) {
  asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7"
               : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
               : "v"(pa), "v"(pb), "v"(pc), "v"(pd)
               : "memory");
}
template <int CNT>
DEV void tie4(s16x8& a, s16x8& b, s16x8& c, s16x8& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(CNT) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
DEV void rd4t(s16x4& a, s16x4& b, s16x4& c, s16x4& d, unsigned pa, unsigned pb, unsigned pc, unsigned pd) {
  asm volatile("ds_read_b64_tr_b16 %0, %4\n\tds_read_b64_tr_b16 %1, %5\n\tds_read_b64_tr_b16 %2, %6\n\t"
               "ds_read_b64_tr_b16 %3, %7"
               : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
               : "v"(pa), "v"(pb), "v"(pc), "v"(pd)
               : "memory");
}
template <int CNT>
DEV void tie4t(s16x4& a, s16x4& b, s16x4& c, s16x4& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(CNT) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// two V^T fragments (column blocks DT0, DT0 + 1 of a 16-key slice at LDS offset VB) by inline asm,
// tied by a counted lgkmcnt wait: the pipelined forward's P V reads in pairs (fewer registers in
// flight than a whole slice: register pressure made the compiler spill in-flight fragments)
template <int ND, unsigned VB, int DT0>
DEV void tr2_issue(s16x4 (&lo)[2], s16x4 (&hi)[2], const unsigned (&toff)[ND][2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
    asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%4\n\tds_read_b64_tr_b16 %1, %3 offset:%4"
                 : "=&v"(lo[j]), "=&v"(hi[j])
                 : "v"(toff[DT0 + j][0]), "v"(toff[DT0 + j][1]), "n"(VB)
                 : "memory");
}
template <int CNT>
DEV void tr2_tie(s16x4 (&lo)[2], s16x4 (&hi)[2]) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]) : "n"(CNT) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int ND, int DT0>
DEV void tr2_mfma(const s16x4 (&lo)[2], const s16x4 (&hi)[2], const frag8& pf, f32x16 (&o)[ND]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const s16x8 v = __builtin_shufflevector(lo[j], hi[j], 0, 1, 2, 3, 4, 5, 6, 7);
    o[DT0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag8, v), pf, o[DT0 + j], 0, 0, 0);
  }
}

// ============================================================================================
// forward
// ============================================================================================
// The plain kernel (cullavo_attn_set_stage(4)): a tile's three steps in program order, K / V tiles
// by LDS-DMA into a double buffer. The readable statement of the arithmetic; attn_fwd_pipe_k below
// is its bitwise twin and the default.
template <int D, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_fwd_k(const u16* __restrict__ Q, int64_t ldq,
                                                     const u16* __restrict__ K, int64_t ldk,
                                                     const u16* __restrict__ V, int64_t ldv,
                                                     u16* __restrict__ O, int64_t ldo,
                                                     float* __restrict__ LSE, int H, int Lq, int Lk,
                                                     float scale, const int32_t* __restrict__ kv_start) {
  constexpr int KT = 64;                 // keys per tile
  constexpr int TILE = KT * D * 2;       // bytes per K (or V) tile
  constexpr int NS = D / 16;             // k-steps over D
  constexpr int ND = D / 32;             // O^T tiles
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // 1-D grid of (query block, head, batch), XCD-remapped: the query blocks of one (b, h) run
  // on one XCD and share its K/V tiles in L2; heavy causal blocks first within a group
  const int nqb = (Lq + 127) / 128;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qi = lid % nqb, hb = lid / nqb;
  const int qb = CAUSAL ? (nqb - 1 - qi) : qi;
  const int h = hb % H, b = hb / H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
  const int q = qb * 128 + wave * 32 + (lane & 31);
  const int kstart = kv_start ? kv_start[b] : 0;

  const u16* Qb = Q + (int64_t)b * Lq * ldq + (int64_t)h * D;
  const u16* Kb = K + (int64_t)b * Lk * ldk + (int64_t)h * D;
  const u16* Vb = V + (int64_t)b * Lk * ldv + (int64_t)h * D;

  frag8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    u16x8 v = (q < Lq) ? *reinterpret_cast<const u16x8*>(Qb + (int64_t)q * ldq + 16 * s + 8 * hf) : u16x8(0);
    qf[s] = __builtin_bit_cast(frag8, v);
  }

  f32x16 o[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) o[i] = f32x16(0.f);
  float m = -INFINITY, l = 0.f;
  const float c = scale * kLog2e;
  const float rescale_thr = g_rescale_thr;

  // live keys of this lane's query: [kstart, khi)
  const int khi = CAUSAL ? min(Lk, q + 1) : Lk;
  const unsigned kspan = (unsigned)max(khi - kstart, 0);
  int kend = Lk;
  if (CAUSAL) kend = min(Lk, qb * 128 + 128);
  const int ntiles = (kend + KT - 1) / KT;
  const int t0 = kstart / KT;

  StageDMA<KT, D, 4> dk_, dv_;
  dk_.prep(ldk, __builtin_amdgcn_readfirstlane(wave), lane);
  dv_.prep(ldv, __builtin_amdgcn_readfirstlane(wave), lane);
  // K and V of the tile at row0 straight into LDS buffer pair i (K at smem + 2*i*TILE, V right
  // after it)
  auto dma_kv = [&](int row0, int i) {
    const int w = __builtin_amdgcn_readfirstlane(wave);
    dk_.issue(Kb, ldk, row0, Lk, smem + 2 * i * TILE, w);
    dv_.issue(Vb, ldv, row0, Lk, smem + 2 * i * TILE + TILE, w);
  };
  if (t0 < ntiles) dma_kv(t0 * KT, 0);
  // vmcnt(0) the compiler can see on every path: the Q fragments are then known to have
  // landed inside the loop, so the in-loop prefetch of the next K/V tile is not waited for
  // before the first MFMA (hipcc otherwise emits vmcnt(0) there: the prefetch is conditional)
  __builtin_amdgcn_s_waitcnt(kVmcnt0);
  __syncthreads();

  // Per-lane LDS offsets of every fragment read, hoisted out of the tile loop: the swizzle of
  // kv_off depends on row & 15 only, so a fragment at row base kb (kb % 16 == 0) sits at the
  // kb = 0 offset plus 2*D*kb (a constant): each read costs one add to the buffer base instead
  // of recomputing the swizzled address.
  // They are absolute LDS addresses in buffer pair 0; the loop body is instantiated once per
  // buffer pair (CUR = 0 / 1, two tiles per trip), so the pair offset 2*CUR*TILE and every
  // fragment's row base are compile-time immediates of the ds_read (no per-tile address adds).
  const unsigned sbase = lds_addr(smem);
  unsigned roff[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) roff[s] = sbase + kv_off<D>(lane & 31, 2 * s + hf);
  unsigned toff[ND][2];
  {
    const int i = lane & 15, qq = i >> 2, p = i & 3;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const int ch = ((dt * 32 + 16 * ((lane >> 4) & 1)) >> 3) + (p >> 1);
      toff[dt][0] = sbase + TILE + kv_off<D>(4 * hf + qq, ch) + 8 * (p & 1);
      toff[dt][1] = sbase + TILE + kv_off<D>(4 * hf + qq + 8, ch) + 8 * (p & 1);
    }
  }
  const f32x2 c2 = {c, c};
  auto tile = [&](auto cur_c, int t) {
    constexpr int CUR = decltype(cur_c)::value;
    constexpr unsigned PAIR = 2u * CUR * TILE;
    if (t + 1 < ntiles) dma_kv((t + 1) * KT, CUR ^ 1);  // pair CUR^1 was last read before the previous barrier
    // S^T = K Q^T for two 32-key halves
    f32x16 st[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      st[kt] = f32x16(0.f);
#pragma unroll
      for (int s = 0; s < NS; ++s)
        st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag(roff[s] + PAIR + kt * 32 * 2 * D), qf[s], st[kt], 0, 0, 0);
    }
    // mask (boundary tiles only, branch-free), tile max on the raw scores (c > 0)
    const int kbase = t * KT;
    const bool need_mask = (CAUSAL && kbase + KT - 1 > qb * 128) || kbase + KT > Lk || kbase < kstart;
    if (need_mask) {
      // key is live for this lane's query iff kstart <= key < khi: one unsigned compare
      const int koff = kbase + 4 * hf - kstart;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          st[kt][r] = (unsigned)(koff + kt * 32 + acc_row(r, 0)) >= kspan ? -INFINITY : st[kt][r];
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, st[kt][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * c;
    // Deferred rescale (cdna_hip_programming.md T13): the reference max m moves -- and O, l are
    // rescaled by exp2(m_old - m_new) -- only on tiles where some row's max grew by more than
    // g_rescale_thr (log2 units); otherwise P = exp2(s c - m) <= 2^thr against the stale m (f32,
    // and bf16 keeps its relative precision at that scale). LSE = m + log2(l) is exact either
    // way. thr = 0 rescales whenever a max grows: the plain online softmax. Branch-free: alpha = 1
    // on tiles that keep the max (a branch around the O multiplies made hipcc reconcile two O
    // register sets with 64 v_mov_b64 per tile on the common path, more than it skipped).
    const bool grow = __any(tmax > m + rescale_thr);  // wave-uniform
    const float mnew = grow ? fmaxf(m, tmax) : m;
    const float muse = (mnew == -INFINITY) ? 0.f : mnew;
    const float alpha = grow ? fast_exp2(m - muse) : 1.f;
    l *= alpha;
#pragma unroll
    for (int i = 0; i < ND; ++i) o[i] *= alpha;
    m = mnew;
    // P = exp2(s c - m): the scale-and-shift and the row sum two lanes' worth at a time
    // (v_pk_fma_f32 / v_pk_add_f32 on the accumulator's even-aligned register pairs)
    const f32x2 nm2 = {-muse, -muse};
    f32x2 rs2 = {0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2 x = {st[kt][r], st[kt][r + 1]};
        const f32x2 y = __builtin_elementwise_fma(x, c2, nm2);
        const f32x2 pv = {fast_exp2(y[0]), fast_exp2(y[1])};  // exp2(-inf) = 0 for masked keys
        st[kt][r] = pv[0];
        st[kt][r + 1] = pv[1];
        rs2 += pv;
      }
    float rs = rs2[0] + rs2[1];
    rs += __shfl_xor(rs, 32, 64);
    l += rs;
    // O^T += V^T P^T
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag8 pf = pack_frag(st[kt], s);
        const unsigned vb = PAIR + (kt * 32 + 16 * s) * 2 * D;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_tr_frag(toff[dt][0] + vb, toff[dt][1] + vb), pf, o[dt], 0, 0, 0);
      }
    // the next pair's DMA has landed in LDS (vmcnt counts LDS-DMA), then every wave's reads of
    // pair CUR are done before anyone overwrites it; the sched_barrier keeps the tile's MFMAs in
    // front of the wait (hipcc otherwise sinks the last ones below it)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  for (int t = t0; t < ntiles; t += 2) {
    tile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < ntiles) tile(std::integral_constant<int, 1>{}, t + 1);
  }

  if (q < Lq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    u16* Ob = O + ((int64_t)b * Lq + q) * ldo + (int64_t)h * D;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        u16x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = f2bf(o[dt][rr * 4 + j] * inv);
        *reinterpret_cast<u16x4*>(Ob + dt * 32 + 8 * rr + 4 * hf) = w;
      }
    if (hf == 0) LSE[((int64_t)b * H + h) * Lq + q] = l > 0.f ? (m + log2f(l)) * kLn2 : INFINITY;
  }
}

// ============================================================================================
// forward, software-pipelined (the default; cullavo_attn_set_stage(7))
// ============================================================================================
// attn_fwd_k runs a tile's three steps in order -- S = K Q^T on the matrix pipe, the softmax on
// the VALU, P V on the matrix pipe -- so inside a wave the matrix pipe idles through the softmax
// and the VALU through both products. Here iteration t runs tile t's softmax in the issue gaps
// of tile t+1's S MFMAs (independent work: S_{t+1} does not need tile t's max) and of tile t's
// first P V MFMAs. K and V have two-slot rings of their own; K runs one tile ahead of V, so at
// iteration t the K tile t+1 and the V tile t are resident and the DMA of K t+2 / V t+1 lands
// under the iteration (one barrier per tile, as before). Every LDS read is inline asm with a
// counted lgkmcnt wait (the fragment group after the current one stays in flight; hipcc puts a
// vmcnt(0) -- the in-flight LDS-DMA -- in front of the builtin transposed read) and each
// softmax chunk is pinned beside its MFMA group by sched_group_barrier. Per element the
// arithmetic is attn_fwd_k's, in the same order: outputs bitwise equal to its.
// both wave halves' values of a per-query quantity combined (lane l with lane l ^ 32) by one
// v_permlane32_swap on two registers holding x: afterwards one holds the lower half's values in
// both halves, the other the upper half's. Inline asm, so the two operands are two registers: the
// builtin given the same value twice may get one register for both, and then swaps nothing
// useful (both results read back as the lower half: a doubled row sum). The 2 wait states a VALU
// write needs before the swap reads it are the s_nop (cdna_hip_programming.md, permlane hazard).
DEV void swap_halves(unsigned& a, unsigned& b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
DEV float swap_max(float x) {
  unsigned a = __builtin_bit_cast(unsigned, x), b = a;
  swap_halves(a, b);
  return fmaxf(__builtin_bit_cast(float, a), __builtin_bit_cast(float, b));
}
DEV float swap_sum(float x) {
  unsigned a = __builtin_bit_cast(unsigned, x), b = a;
  swap_halves(a, b);
  return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}
// NM MFMAs, each followed by NV VALU instructions (the scheduler's placement of the group's code)
template <int NM, int NV>
DEV void interleave() {
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if (NV > 0) __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);
  }
}
// P = exp2(s c - m) of accumulator registers R0..R0+3 of score tile KT_, the row sum's even /
// odd partials (the pair order of attn_fwd_k's v_pk_add accumulation)
// 2 K row fragments (k-steps S0, S0+1 at LDS byte offset OFF from each lane's roff) by inline-asm
// ds_read_b128, tied by a counted lgkmcnt wait
template <int NS, int S0, unsigned OFF>
DEV void k2_issue(s16x8 (&kf)[2], const unsigned (&roff)[NS]) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(kf[j]) : "v"(roff[S0 + j]), "n"(OFF) : "memory");
}
template <int CNT>
DEV void k2_tie(s16x8 (&kf)[2]) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(kf[0]), "+v"(kf[1]) : "n"(CNT) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int NS, int S0>
DEV void k2_mfma(const s16x8 (&kf)[2], const frag8 (&qf)[NS], f32x16& acc) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag8, kf[j]), qf[S0 + j], acc, 0, 0, 0);
}
// an empty asm on a value: the code computing it cannot sink below this point, and code reading it
// cannot rise above it (hipcc's instruction selection otherwise gathers a whole softmax next to its
// last consumer, out of the MFMA groups it was written beside)
template <class T>
DEV void pin(T& x) {
  asm volatile("" : "+v"(x));
}
template <int KT_, int R0>
DEV void sm_exp4(f32x16 (&sp)[2], float c, float nm, float& rsE, float& rsO) {
  pin(sp[KT_]);
#pragma unroll
  for (int r = R0; r < R0 + 4; r += 2) {
    const float p0 = fast_exp2(__builtin_fmaf(sp[KT_][r], c, nm));
    const float p1 = fast_exp2(__builtin_fmaf(sp[KT_][r + 1], c, nm));
    sp[KT_][r] = p0;
    sp[KT_][r + 1] = p1;
    rsE += p0;
    rsO += p1;
  }
  pin(sp[KT_]);
  pin(rsE);
  pin(rsO);
}

// The kernel's statements are in attn_fwd_pipe_body.h, shared with attn_fwd_cached_k below.
template <int D, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_fwd_pipe_k(const u16* __restrict__ Q, int64_t ldq,
                                                          const u16* __restrict__ K, int64_t ldk,
                                                          const u16* __restrict__ V, int64_t ldv,
                                                          u16* __restrict__ O, int64_t ldo,
                                                          float* __restrict__ LSE, int H, int Lq, int Lk,
                                                          float scale, const int32_t* __restrict__ kv_start) {
  constexpr bool CACHED = false, RAGGED = false, VARLEN = false;
  constexpr int qpad = 0, vl_max = 0, vl_row0 = 0;
#include "attn_fwd_pipe_body.h"
}

// Lq new queries per sequence against the first Lk = past + Lq rows of a KV cache
// (cullavo_attn_fwd_cached): the same statements with a query offset and a K/V batch stride of its
// own. The arguments keep attn_fwd_pipe_k's places: ldk is the cache's token stride (K and V),
// ldv its batch stride.
template <int D>
__global__ __launch_bounds__(256, 2) void attn_fwd_cached_k(const u16* __restrict__ Q, int64_t ldq,
                                                            const u16* __restrict__ K, int64_t ldk,
                                                            const u16* __restrict__ V, int64_t ldv,
                                                            u16* __restrict__ O, int64_t ldo,
                                                            float* __restrict__ LSE, int H, int Lq, int Lk,
                                                            float scale, const int32_t* __restrict__ kv_start) {
  constexpr bool CAUSAL = true, CACHED = true, RAGGED = false, VARLEN = false;
  constexpr int qpad = 0, vl_max = 0, vl_row0 = 0;
#include "attn_fwd_pipe_body.h"
}

// attn_fwd_cached_k with a prefix length per sequence (cullavo_attn_fwd_ragged): the [B, Lq] query
// block is left-padded, sequence b's first q_pad[b] rows are padding and its cache holds kv_len[b]
// rows, the Lq - q_pad[b] new ones included. Query i >= q_pad[b] sits at cache row kv_len[b] - Lq +
// i. Device values cannot be checked on the host: kv_len[b] is clamped to [0, cap] (cap = the rows
// of a sequence's slab, ld_batch / ld_tok) and q_pad[b] to [0, Lq], so no value fetches outside the
// slab. Both are loaded once per workgroup from a uniform address (scalar loads).
template <int D>
__global__ __launch_bounds__(256, 2) void attn_fwd_ragged_k(const u16* __restrict__ Q, int64_t ldq,
                                                            const u16* __restrict__ K, int64_t ldk,
                                                            const u16* __restrict__ V, int64_t ldv,
                                                            u16* __restrict__ O, int64_t ldo,
                                                            float* __restrict__ LSE, int H, int Lq, int cap,
                                                            float scale, const int32_t* __restrict__ kv_start,
                                                            const int32_t* __restrict__ kv_len,
                                                            const int32_t* __restrict__ q_pad) {
  constexpr bool CAUSAL = true, CACHED = true, RAGGED = true, VARLEN = false;
  constexpr int vl_max = 0, vl_row0 = 0;
  const int seq = xcd_remap(blockIdx.x, gridDim.x) / ((Lq + 127) / 128) / H;  // the body's b
  const int Lk = min(max(kv_len[seq], 0), cap);
  const int qpad = q_pad ? min(max(q_pad[seq], 0), Lq) : 0;
#include "attn_fwd_pipe_body.h"
}

// attn_fwd_pipe_k<D, true> over sequences of unequal length packed back to back
// (cullavo_attn_fwd_varlen): sequence b owns rows seq_start[b] .. seq_start[b] + seq_len[b] - 1 of
// Q / K / V / O, the grid and the [B, H, vl_max] lse are sized by the host's bound vl_max.
// seq_len[b] is clamped to [0, vl_max] (a device value: see VarSeq). A workgroup whose query tile
// starts at or beyond the sequence's end exits: workgroup-uniform, before any barrier.
template <int D>
__global__ __launch_bounds__(256, 2) void attn_fwd_varlen_k(const u16* __restrict__ Q, int64_t ldq,
                                                            const u16* __restrict__ K, int64_t ldk,
                                                            const u16* __restrict__ V, int64_t ldv,
                                                            u16* __restrict__ O, int64_t ldo,
                                                            float* __restrict__ LSE, int H, int vl_max, float scale,
                                                            const int32_t* __restrict__ seq_start,
                                                            const int32_t* __restrict__ seq_len) {
  constexpr bool CAUSAL = true, CACHED = false, RAGGED = false, VARLEN = true;
  constexpr int qpad = 0;
  constexpr const int32_t* kv_start = nullptr;
  const int vl_nqb = (vl_max + 127) / 128;
  const int vl_lid = xcd_remap(blockIdx.x, gridDim.x);  // the body's lid, qb and b
  const int seq = vl_lid / vl_nqb / H;
  const int Lq = min(max(seq_len[seq], 0), vl_max), Lk = Lq;
  if ((vl_nqb - 1 - vl_lid % vl_nqb) * 128 >= Lq) return;
  const int64_t vl_row0 = seq_start[seq];
#include "attn_fwd_pipe_body.h"
}

// ============================================================================================
// backward
// ============================================================================================
// delta[b,h,q] = sum_d dO*O  (f32); one 16-lane group per (token, head) row for D=128
// (SEQ: the rows per sequence L, or a VarSeq; the varlen form runs over B max_len rows, reads row
// t < len[b] of sequence b at start[b] + t and skips the rest)
template <int D, class SEQ = int>
__global__ __launch_bounds__(256) void attn_delta_k(const u16* __restrict__ O, int64_t ldo,
                                                    const u16* __restrict__ dO, int64_t lddo,
                                                    float* __restrict__ delta, int B, int H, SEQ sq) {
  constexpr int LPR = D / 8;  // lanes per row
  const int L = seq_grid_rows(sq);
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPR;  // (b, t, h) row
  const int sub = threadIdx.x % LPR;
  int64_t nrows = (int64_t)B * L * H;
  int64_t src = 0;  // varlen: the packed row of (b, t)
  if constexpr (kVarlen<SEQ>) {
    if (row < nrows) {
      const int64_t bt = row / H;
      const int bb = (int)(bt / L), t = (int)(bt % L);
      if (t < seq_rows(sq, bb, L)) src = seq_row0(sq, bb, L) + t;
      else nrows = 0;  // a row past the sequence's end: nothing read, nothing written
    }
  }
  float acc = 0.f;
  if (row < nrows) {
    const int hh = (int)(row % H);
    const int64_t bt = kVarlen<SEQ> ? src : row / H;
    float a[8], d[8];
    load8(O + bt * ldo + (int64_t)hh * D + sub * 8, a);
    load8(dO + bt * lddo + (int64_t)hh * D + sub * 8, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += a[j] * d[j];
  }
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (row < nrows && sub == 0) {
    const int hh = (int)(row % H);
    const int64_t bt = row / H;
    const int64_t bb = bt / L, t = bt % L;
    delta[(bb * H + hh) * L + t] = acc;
  }
}

// Kernel A: dK, dV. A wave owns 32 keys (K, V fragments in registers); the workgroup sweeps
// 32-row query tiles staged in LDS. S = Q K^T and dP = dO V^T keep the key on the lane;
// dV = P^T dO and dK = dS^T Q take P / dS straight from the accumulators (A operand) and
// dO / Q as transposed LDS fragments.
template <int D, bool CAUSAL, class SEQ = const int32_t*>
__global__ __launch_bounds__(256, 1) void attn_bwd_dkdv_k(
    const u16* __restrict__ Q, int64_t ldq, const u16* __restrict__ K, int64_t ldk,
    const u16* __restrict__ V, int64_t ldv, const u16* __restrict__ dO, int64_t lddo,
    const float* __restrict__ LSE, const float* __restrict__ DELTA, u16* __restrict__ dK,
    int64_t lddk, u16* __restrict__ dV, int64_t lddv, int H, int LqG, int LkG, float scale,
    typename SeqArg<SEQ>::type kv_start) {
  constexpr int QT = 32;         // query rows per tile (64-row tiles lost the sweep on both head dims)
  constexpr int NSUB = QT / 32;  // 32-row query sub-tiles per barrier
  constexpr int TILE = QT * D * 2;
  constexpr int NS = D / 16;
  constexpr int ND = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [buf][Q tile | dO tile | lse(32 f32) | delta(32 f32)]
  constexpr int BUF = 2 * TILE + 2 * QT * 4;

  // 1-D grid of (key block, head, batch), XCD-remapped: the key blocks of one (b, h) share
  // its Q / dO tiles in one XCD's L2
  const int nkb = (seq_grid_rows(kv_start, LkG) + 127) / 128;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int kb = lid % nkb, hb = lid / nkb;
  const int h = hb % H, b = hb / H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
  const int key = kb * 128 + wave * 32 + (lane & 31);  // this lane's key (operand column)
  const int kstart = seq_kstart(kv_start, b);
  const int Lq = seq_rows(kv_start, b, LqG), Lk = seq_rows(kv_start, b, LkG);  // this sequence's rows
  if constexpr (kVarlen<SEQ>) if (kb * 128 >= Lk) return;  // a tile past the sequence's end (workgroup-uniform)

  const u16* Qb = Q + seq_row0(kv_start, b, LqG) * ldq + (int64_t)h * D;
  const u16* dOb = dO + seq_row0(kv_start, b, LqG) * lddo + (int64_t)h * D;
  const u16* Kb = K + seq_row0(kv_start, b, LkG) * ldk + (int64_t)h * D;
  const u16* Vb = V + seq_row0(kv_start, b, LkG) * ldv + (int64_t)h * D;
  const float* lseb = LSE + ((int64_t)b * H + h) * seq_grid_rows(kv_start, LqG);
  const float* delb = DELTA + ((int64_t)b * H + h) * seq_grid_rows(kv_start, LqG);

  frag8 kf[NS], vf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool ok = key < Lk;
    kf[s] = __builtin_bit_cast(frag8, ok ? *reinterpret_cast<const u16x8*>(Kb + (int64_t)key * ldk + 16 * s + 8 * hf) : u16x8(0));
    vf[s] = __builtin_bit_cast(frag8, ok ? *reinterpret_cast<const u16x8*>(Vb + (int64_t)key * ldv + 16 * s + 8 * hf) : u16x8(0));
  }
  f32x16 dk[ND], dv[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) { dk[i] = f32x16(0.f); dv[i] = f32x16(0.f); }
  const float c = scale * kLog2e;

  // query tiles that can see this block's keys
  const int kmin = kb * 128;
  int qt0 = CAUSAL ? (kmin / QT) : 0;
  const int nqt = (Lq + QT - 1) / QT;
  const bool block_live = kmin < Lk && (kmin + 128 > kstart);

  Stage<QT, D> sq, sdo;
  // lse / delta of a query tile (threads 0..2QT-1, one value each): loaded together with the
  // tile's Q / dO prefetch and written to LDS with them (not loaded and waited for at the end)
  float aux = 0.f;
  // the next tile's lse / delta: loaded raw and first used when staged after the tile's compute
  // (arithmetic on the loaded value at load time made the compiler wait for it -- and for the
  // in-flight tile prefetch -- at the top of every tile)
  bool aux_in = false;
  auto load_aux = [&](int qt) {
    if (threadIdx.x < 2 * QT) {
      const int qq = qt * QT + (int)threadIdx.x % QT;
      aux_in = qq < Lq;
      aux = (threadIdx.x < QT ? lseb : delb)[min(qq, Lq - 1)];
    }
  };
  auto store_aux = [&](char* buf) {
    if (threadIdx.x < 2 * QT)
      ((float*)(buf + 2 * TILE))[threadIdx.x] = aux_in ? aux : (threadIdx.x < QT ? INFINITY : 0.f);
  };
  if (block_live && qt0 < nqt) {
    sq.load(Qb, ldq, qt0 * QT, Lq);
    sdo.load(dOb, lddo, qt0 * QT, Lq);
    sq.store(smem);
    sdo.store(smem + TILE);
    load_aux(qt0);
    store_aux(smem);
  }
  __builtin_amdgcn_s_waitcnt(kVmcnt0);  // see attn_fwd_k: keeps hipcc from waiting on the prefetch
  __syncthreads();

  for (int qt = qt0; block_live && qt < nqt; ++qt) {
    const int cur = (qt - qt0) & 1;
    char* buf = smem + cur * BUF;
    char* nbuf = smem + (cur ^ 1) * BUF;
    const bool more = qt + 1 < nqt;
    if (more) {
      sq.load(Qb, ldq, (qt + 1) * QT, Lq);
      sdo.load(dOb, lddo, (qt + 1) * QT, Lq);
      load_aux(qt + 1);
    }
    const float* slse = (const float*)(buf + 2 * TILE);
    const float* sdel = slse + QT;
    // S[q][key], dP[q][key] of the NSUB 32-row sub-tiles (independent MFMA chains)
    f32x16 sacc[NSUB], pacc[NSUB];
#pragma unroll
    for (int u = 0; u < NSUB; ++u) { sacc[u] = f32x16(0.f); pacc[u] = f32x16(0.f); }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int u = 0; u < NSUB; ++u) {
        sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<D>(buf, 32 * u, s, lane), kf[s], sacc[u], 0, 0, 0);
        pacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<D>(buf + TILE, 32 * u, s, lane), vf[s], pacc[u], 0, 0, 0);
      }
    // P = exp(S*scale - lse), dS = P * (dP - delta)
#pragma unroll
    for (int u = 0; u < NSUB; ++u)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(slse + 32 * u + 8 * rr + 4 * hf);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sdel + 32 * u + 8 * rr + 4 * hf);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = rr * 4 + j;
          const int qq = qt * QT + 32 * u + 8 * rr + 4 * hf + j;
          float pv = fast_exp2(fmaf(sacc[u][r], c, -l4[j] * kLog2e));
          if ((CAUSAL && key > qq) || key < kstart || key >= Lk || qq >= Lq) pv = 0.f;
          sacc[u][r] = pv;
          pacc[u][r] = pv * (pacc[u][r] - d4[j]);
        }
      }
    // dV += P^T dO ; dK += dS^T Q   (A operand = accumulator, B = transposed LDS fragment);
    // sub-tile order = the 32-row tile order, so every QT sums in the same order
#pragma unroll
    for (int u = 0; u < NSUB; ++u)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag8 pf = pack_frag(sacc[u], s);
        const frag8 df = pack_frag(pacc[u], s);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, tr_frag<D>(buf + TILE, 32 * u + 16 * s, dt * 32, lane), dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, tr_frag<D>(buf, 32 * u + 16 * s, dt * 32, lane), dk[dt], 0, 0, 0);
        }
      }
    if (more) {
      sq.store(nbuf);
      sdo.store(nbuf + TILE);
      store_aux(nbuf);
    }
    __syncthreads();
  }

  // dK/dV[key][d]: register r = key row, lane = d column
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = kb * 128 + wave * 32 + acc_row(r, hf);
      if (kk < Lk) {
        const int d = dt * 32 + (lane & 31);
        dK[(seq_row0(kv_start, b, LkG) + kk) * lddk + (int64_t)h * D + d] = f2bf(dk[dt][r] * scale);
        dV[(seq_row0(kv_start, b, LkG) + kk) * lddv + (int64_t)h * D + d] = f2bf(dv[dt][r]);
      }
    }
}

// Kernel B: dQ. A wave owns 32 query rows (Q, dO fragments in registers, lse/delta per
// lane); the workgroup sweeps 32-key K/V tiles. S^T = K Q^T, dP^T = V dO^T (query on the
// lane), dQ^T += K^T dS^T with K^T as a transposed LDS fragment.
template <int D, bool CAUSAL, int KT, class SEQ = const int32_t*>
__global__ __launch_bounds__(256, 1) void attn_bwd_dq_k(
    const u16* __restrict__ Q, int64_t ldq, const u16* __restrict__ K, int64_t ldk,
    const u16* __restrict__ V, int64_t ldv, const u16* __restrict__ dO, int64_t lddo,
    const float* __restrict__ LSE, const float* __restrict__ DELTA, u16* __restrict__ dQ,
    int64_t lddq, int H, int LqG, int LkG, float scale, typename SeqArg<SEQ>::type kv_start) {
  constexpr int TILE = KT * D * 2;
  constexpr int NSUB = KT / 32;  // 32-key sub-tiles per barrier
  constexpr int NS = D / 16;
  constexpr int ND = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int nqb = (seq_grid_rows(kv_start, LqG) + 127) / 128;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);  // as attn_fwd_k: one (b, h) per XCD range
  const int qi = lid % nqb, hb = lid / nqb;
  const int qb = CAUSAL ? (nqb - 1 - qi) : qi;
  const int h = hb % H, b = hb / H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
  const int q = qb * 128 + wave * 32 + (lane & 31);
  const int kstart = seq_kstart(kv_start, b);
  const int Lq = seq_rows(kv_start, b, LqG), Lk = seq_rows(kv_start, b, LkG);  // this sequence's rows
  if constexpr (kVarlen<SEQ>) if (qb * 128 >= Lq) return;  // a tile past the sequence's end (workgroup-uniform)

  const u16* Qb = Q + seq_row0(kv_start, b, LqG) * ldq + (int64_t)h * D;
  const u16* dOb = dO + seq_row0(kv_start, b, LqG) * lddo + (int64_t)h * D;
  const u16* Kb = K + seq_row0(kv_start, b, LkG) * ldk + (int64_t)h * D;
  const u16* Vb = V + seq_row0(kv_start, b, LkG) * ldv + (int64_t)h * D;

  frag8 qf[NS], of[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool ok = q < Lq;
    qf[s] = __builtin_bit_cast(frag8, ok ? *reinterpret_cast<const u16x8*>(Qb + (int64_t)q * ldq + 16 * s + 8 * hf) : u16x8(0));
    of[s] = __builtin_bit_cast(frag8, ok ? *reinterpret_cast<const u16x8*>(dOb + (int64_t)q * lddo + 16 * s + 8 * hf) : u16x8(0));
  }
  const float lse2 = (q < Lq) ? LSE[((int64_t)b * H + h) * seq_grid_rows(kv_start, LqG) + q] * kLog2e : INFINITY;
  const float del = (q < Lq) ? DELTA[((int64_t)b * H + h) * seq_grid_rows(kv_start, LqG) + q] : 0.f;
  const float c = scale * kLog2e;
  f32x16 dq[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) dq[i] = f32x16(0.f);

  int kend = Lk;
  if (CAUSAL) kend = min(Lk, qb * 128 + 128);
  const int ntiles = (kend + KT - 1) / KT;
  const int t0 = kstart / KT;

  Stage<KT, D> sk, sv;
  // buffer i: K at smem + 2*i*TILE, V right after it
#define bufK(i) (smem + 2 * (i) * TILE)
#define bufV(i) (smem + 2 * (i) * TILE + TILE)
  if (t0 < ntiles) {
    sk.load(Kb, ldk, t0 * KT, Lk);
    sv.load(Vb, ldv, t0 * KT, Lk);
    sk.store(bufK(0));
    sv.store(bufV(0));
  }
  __builtin_amdgcn_s_waitcnt(kVmcnt0);  // see attn_fwd_k: keeps hipcc from waiting on the prefetch
  __syncthreads();
  for (int t = t0; t < ntiles; ++t) {
    const int cur = (t - t0) & 1;
    const bool more = t + 1 < ntiles;
    if (more) {
      sk.load(Kb, ldk, (t + 1) * KT, Lk);
      sv.load(Vb, ldv, (t + 1) * KT, Lk);
    }
    f32x16 st[NSUB], dpt[NSUB];
#pragma unroll
    for (int u = 0; u < NSUB; ++u) { st[u] = f32x16(0.f); dpt[u] = f32x16(0.f); }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int u = 0; u < NSUB; ++u) {
        st[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<D>(bufK(cur), 32 * u, s, lane), qf[s], st[u], 0, 0, 0);
        dpt[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<D>(bufV(cur), 32 * u, s, lane), of[s], dpt[u], 0, 0, 0);
      }
    const int kbase = t * KT;
#pragma unroll
    for (int u = 0; u < NSUB; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kbase + 32 * u + acc_row(r, hf);
        float pv = fast_exp2(fmaf(st[u][r], c, -lse2));
        if (key >= Lk || key < kstart || (CAUSAL && key > q)) pv = 0.f;
        dpt[u][r] = pv * (dpt[u][r] - del);
      }
#pragma unroll
    for (int u = 0; u < NSUB; ++u)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag8 df = pack_frag(dpt[u], s);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
          dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<D>(bufK(cur), 32 * u + 16 * s, dt * 32, lane), df, dq[dt], 0, 0, 0);
      }
    if (more) {
      sk.store(bufK(cur ^ 1));
      sv.store(bufV(cur ^ 1));
    }
    __syncthreads();
  }
  if (q < Lq) {
    u16* dQb = dQ + (seq_row0(kv_start, b, LqG) + q) * lddq + (int64_t)h * D;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        u16x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = f2bf(dq[dt][rr * 4 + j] * scale);
        *reinterpret_cast<u16x4*>(dQb + dt * 32 + 8 * rr + 4 * hf) = w;
      }
  }
}

// ============================================================================================
// backward, 8-wave variants (the default): two waves per SIMD
// ============================================================================================
// The 4-wave kernels above keep one wave per SIMD (their K/V or Q/dO fragments plus two sets of
// 32x32 accumulators need > 256 registers), so every LDS read, exp and wait of a wave sits in
// front of its own MFMAs with nothing to overlap it. Here a workgroup has 8 waves over the same
// 128 keys (dK/dV) or 128 queries (dQ): waves w and w + 4 own the same 32-row slice and split
// the other dimension of every tile between them (query rows 0-31 / 32-63 of the 64-row query
// tile; keys 0-31 / 32-63 of the 64-key tile), so each SIMD runs two waves whose MFMAs cover
// each other's LDS / VALU phases. The pair's partial accumulators are added once at the end
// through LDS (fixed order: half 0 + half 1), so results stay bitwise reproducible.
//   dK/dV: K and V of the workgroup's 128 keys live in LDS for the whole sweep (row fragments
//   re-read per tile instead of 64 registers), Q / dO tiles double-buffered beside them.
//   dQ:    Q / dO fragments in registers, K / V tiles double-buffered in LDS.
template <int ROWS, int D, int NT>
struct StageN {
  static constexpr int kPer = ROWS * D / 8 / NT;  // 16-byte chunks per thread
  u16x8 r[kPer];
  DEV void load(const u16* base, int64_t ld, int row0, int nrows) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int q = threadIdx.x + NT * i;
      const int row = q / (D / 8), ch = q % (D / 8);
      r[i] = (row0 + row < nrows) ? *reinterpret_cast<const u16x8*>(base + (int64_t)(row0 + row) * ld + ch * 8)
                                  : u16x8(0);
    }
  }
  DEV void store(char* lds) const {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int q = threadIdx.x + NT * i;
      const int row = q / (D / 8), ch = q % (D / 8);
      *reinterpret_cast<u16x8*>(lds + kv_off<D>(row, ch)) = r[i];
    }
  }
};

// Q / dO tiles arrive by LDS-DMA (no staging registers or ds_write), and every fragment is read by
// inline asm one step ahead of its MFMAs: 7B layer backward 467.5 -> 449.7 us against the
// register-staged form, bitwise equal (profiles/r05/attn/attn_bwd_stage_ab.txt). DS_OUT: also store
// dS^T[b, h][key][q] for attn_bwd_dq_ds_k (mode 7); the workspace is row-major, ldst = LqP with
// the 128-query block qb at column 128 qb (st_blk = 128).
// The kernel's statements are in attn_bwd_dkdv8_body.h, shared with attn_bwd_dkdv8_varlen_k below (text,
// not a function both call: inlined through a function attn_bwd_dkdv8_k<128, true, true> came out 142
// instructions longer).
template <int D, bool CAUSAL, bool DS_OUT>
__global__ __launch_bounds__(512, 1) void attn_bwd_dkdv8_k(
    const u16* __restrict__ Q, int64_t ldq, const u16* __restrict__ K, int64_t ldk,
    const u16* __restrict__ V, int64_t ldv, const u16* __restrict__ dO, int64_t lddo,
    const float* __restrict__ LSE, const float* __restrict__ DELTA, u16* __restrict__ dK,
    int64_t lddk, u16* __restrict__ dV, int64_t lddv, int H, int LqG, int LkG, float scale,
    const int32_t* __restrict__ kv_start, u16* __restrict__ dST, int64_t ldst, int64_t st_bh, int64_t st_blk) {
  using SEQ = const int32_t*;
#include "attn_bwd_dkdv8_body.h"
}
// packed sequences (cullavo_attn_bwd_varlen): causal, rows and lengths from the VarSeq
template <int D, bool DS_OUT>
__global__ __launch_bounds__(512, 1) void attn_bwd_dkdv8_varlen_k(
    const u16* __restrict__ Q, int64_t ldq, const u16* __restrict__ K, int64_t ldk,
    const u16* __restrict__ V, int64_t ldv, const u16* __restrict__ dO, int64_t lddo,
    const float* __restrict__ LSE, const float* __restrict__ DELTA, u16* __restrict__ dK,
    int64_t lddk, u16* __restrict__ dV, int64_t lddv, int H, float scale, VarSeq kv_start,
    u16* __restrict__ dST, int64_t ldst, int64_t st_bh, int64_t st_blk) {
  using SEQ = VarSeq;
  constexpr bool CAUSAL = true;
  const int LqG = kv_start.max_len, LkG = LqG;
#include "attn_bwd_dkdv8_body.h"
}

// ============================================================================================
// backward dQ from the stored dS (mode 7)
// ============================================================================================
// The 8-wave dK/dV kernel writes dS^T[b, h][key][q] (bf16, the same rounded values its dK
// product consumes) for every (key, query) pair it visits; dQ^T = K^T dS^T then needs no S / dP
// recompute: one product instead of three. A wave owns 32 query columns, the workgroup sweeps
// 64-key tiles up to the causal diagonal with K and dS^T tiles staged in LDS, both operands
// read as transposed fragments (the same k order on both sides). dS^T has LkP =
// round_up(Lk, 128) rows (keys) of LqP = round_up(Lq, 128) queries (cullavo_attn_bwd_workspace).
// K and dS^T tiles are staged through registers (StageT): the LDS-DMA and 4-stage ring forms of
// round 6 moved nothing (130.2 / 129.6 / 130.4 / 131.4 us, profiles/r06/attn/README_r06.txt; the
// ring kernel lives on in tools/lab/dq_ring.inc).
template <int D, bool CAUSAL, class SEQ = const int32_t*>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_ds_k(const u16* __restrict__ K, int64_t ldk,
                                                           const u16* __restrict__ dST, int64_t ldst, int64_t st_bh, int64_t st_blk,
                                                           int LkP, u16* __restrict__ dQ, int64_t lddq, int H,
                                                           int LqG, int LkG, float scale,
                                                           typename SeqArg<SEQ>::type kv_start) {
  constexpr int KT = 64, QB = 128;
  constexpr int TK = KT * D * 2, TS = KT * QB * 2, BUF = TK + TS;
  constexpr int NS = KT / 16, ND = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int nqb = (seq_grid_rows(kv_start, LqG) + QB - 1) / QB;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qi = lid % nqb, hb = lid / nqb;
  const int qb = CAUSAL ? (nqb - 1 - qi) : qi;
  const int h = hb % H, b = hb / H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
  const int q = qb * QB + wave * 32 + (lane & 31);
  const int kstart = seq_kstart(kv_start, b);
  const int Lq = seq_rows(kv_start, b, LqG), Lk = seq_rows(kv_start, b, LkG);  // this sequence's rows
  if constexpr (kVarlen<SEQ>) if (qb * QB >= Lq) return;  // a tile past the sequence's end (workgroup-uniform)
  const u16* Kb = K + seq_row0(kv_start, b, LkG) * ldk + (int64_t)h * D;
  const u16* Sb = dST + ((int64_t)b * H + h) * st_bh + qb * st_blk;

  f32x16 dq[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) dq[i] = f32x16(0.f);
  int kend = Lk;
  if (CAUSAL) kend = min(Lk, qb * QB + QB);
  const int ntiles = (kend + KT - 1) / KT;
  const int t0 = kstart / KT;

  StageT<KT, D> sk;
  StageT<KT, QB> ss;
  const unsigned vok = StageT<KT, D>::lane_off(ldk), vos = StageT<KT, QB>::lane_off(ldst);
  if (t0 < ntiles) {
    sk.load(Kb, ldk, t0 * KT, Lk, vok);
    ss.load(Sb, ldst, t0 * KT, LkP, vos);
    sk.store(smem);
    ss.store(smem + TK);
  }
  __builtin_amdgcn_s_waitcnt(kVmcnt0);
  __syncthreads();
  for (int t = t0; t < ntiles; ++t) {
    char* bK = smem + ((t - t0) & 1) * BUF;
    char* bS = bK + TK;
    const bool more = t + 1 < ntiles;
    if (more) {
      sk.load(Kb, ldk, (t + 1) * KT, Lk, vok);
      ss.load(Sb, ldst, (t + 1) * KT, LkP, vos);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const frag8 bs = tr_frag<QB>(bS, 16 * s, wave * 32, lane);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<D>(bK, 16 * s, dt * 32, lane), bs, dq[dt], 0, 0, 0);
    }
    if (more) {
      char* nK = smem + ((t - t0 + 1) & 1) * BUF;
      sk.store(nK);
      ss.store(nK + TK);
    }
    __syncthreads();
  }
  if (q < Lq) {
    u16* dQb = dQ + (seq_row0(kv_start, b, LqG) + q) * lddq + (int64_t)h * D;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        u16x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = f2bf(dq[dt][rr * 4 + j] * scale);
        *reinterpret_cast<u16x4*>(dQb + dt * 32 + 8 * rr + 4 * hf) = w;
      }
  }
}

int64_t ds_rows(int Lk) { return cdiv(Lk, 128) * 128; }
int64_t ds_cols(int Lq) { return cdiv(Lq, 128) * 128; }

template <typename Kern>
void set_smem(Kern k, int bytes) {
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

template <int D, bool CAUSAL>
int fwd_launch(const u16* q, int64_t ldq, const u16* k, int64_t ldk, const u16* v, int64_t ldv, u16* o,
               int64_t ldo, float* lse, int B, int H, int Lq, int Lk, float scale, const int32_t* ks,
               hipStream_t s) {
  const int smem = 4 * 64 * D * 2;
  static bool once = false;
  if (!once) {
    set_smem(attn_fwd_k<D, CAUSAL>, smem);
    set_smem(attn_fwd_pipe_k<D, CAUSAL>, smem);
    once = true;
  }
  const unsigned grid = (unsigned)(cdiv(Lq, 128) * H * B);
  if (g_fwd_stage == 4)
    attn_fwd_k<D, CAUSAL><<<grid, 256, smem, s>>>(q, ldq, k, ldk, v, ldv, o, ldo, lse, H, Lq, Lk, scale, ks);
  else
    attn_fwd_pipe_k<D, CAUSAL><<<grid, 256, smem, s>>>(q, ldq, k, ldk, v, ldv, o, ldo, lse, H, Lq, Lk, scale, ks);
  return cullavo_check_launch("attn_fwd");
}

template <int D>
int fwd_cached_launch(const u16* q, int64_t ldq, const u16* kc, const u16* vc, int64_t ld_tok, int64_t ld_batch,
                      u16* o, int64_t ldo, float* lse, int B, int H, int Lq, int past, float scale,
                      const int32_t* ks, hipStream_t s) {
  const int smem = 4 * 64 * D * 2;
  static bool once = false;
  if (!once) {
    set_smem(attn_fwd_cached_k<D>, smem);
    once = true;
  }
  const unsigned grid = (unsigned)(cdiv(Lq, 128) * H * B);
  // (K, its token stride, V, the batch stride: the argument places of attn_fwd_pipe_k)
  attn_fwd_cached_k<D><<<grid, 256, smem, s>>>(q, ldq, kc, ld_tok, vc, ld_batch, o, ldo, lse, H, Lq, past + Lq, scale,
                                               ks);
  return cullavo_check_launch("attn_fwd_cached");
}

template <int D>
int fwd_ragged_launch(const u16* q, int64_t ldq, const u16* kc, const u16* vc, int64_t ld_tok, int64_t ld_batch,
                      u16* o, int64_t ldo, float* lse, int B, int H, int Lq, int cap, float scale,
                      const int32_t* ks, const int32_t* kv_len, const int32_t* q_pad, hipStream_t s) {
  const int smem = 4 * 64 * D * 2;
  static bool once = false;
  if (!once) {
    set_smem(attn_fwd_ragged_k<D>, smem);
    once = true;
  }
  const unsigned grid = (unsigned)(cdiv(Lq, 128) * H * B);
  attn_fwd_ragged_k<D><<<grid, 256, smem, s>>>(q, ldq, kc, ld_tok, vc, ld_batch, o, ldo, lse, H, Lq, cap, scale, ks,
                                               kv_len, q_pad);
  return cullavo_check_launch("attn_fwd_ragged");
}

template <int D>
int fwd_varlen_launch(const u16* q, int64_t ldq, const u16* k, int64_t ldk, const u16* v, int64_t ldv, u16* o,
                      int64_t ldo, float* lse, int B, int H, int max_len, float scale, const int32_t* seq_start,
                      const int32_t* seq_len, hipStream_t s) {
  const int smem = 4 * 64 * D * 2;
  static bool once = false;
  if (!once) {
    set_smem(attn_fwd_varlen_k<D>, smem);
    once = true;
  }
  const unsigned grid = (unsigned)(cdiv(max_len, 128) * H * B);
  attn_fwd_varlen_k<D><<<grid, 256, smem, s>>>(q, ldq, k, ldk, v, ldv, o, ldo, lse, H, max_len, scale, seq_start,
                                               seq_len);
  return cullavo_check_launch("attn_fwd_varlen");
}

// backward mode (cullavo_attn_set_bwd_tiles):
//   0 = the 4-wave kernels, 32-row dK/dV tiles and 32-key dQ tiles (the plain pair);
//   2 = as 0 with 64-key dQ tiles, bitwise equal to 0;
//   4 = the 8-wave dK/dV kernel + the 4-wave dQ kernel with 32-key tiles (the recompute path; also
//       what mode 7 runs when no dS^T workspace is given);
//   7 = the 8-wave dK/dV kernel storing dS^T + dQ from it (workspace: B*H*LkP*LqP bf16);
//  -1 = per head dim, see bwd_mode.
// The 64-row dK/dV tiles (modes 1, 3) lost the tile sweep on both head dims and left with ABI 6.
int g_bwd_tiles = -1;

// delta, then the mode's dK/dV kernel, then its dQ kernel (ds: the dS^T workspace of mode 7). ks:
// kv_start of the uniform grid, or the VarSeq of packed sequences (Lq = Lk = its max_len)
template <int D, bool CAUSAL, class SEQ>
int bwd_launch(const u16* q, int64_t ldq, const u16* k, int64_t ldk, const u16* v, int64_t ldv, const u16* o,
               int64_t ldo, const u16* dout, int64_t lddo, const float* lse, float* delta, u16* dq, int64_t lddq,
               u16* dk, int64_t lddk, u16* dv, int64_t lddv, int B, int H, int Lq, int Lk, float scale,
               SEQ ks, int mode, u16* ds, hipStream_t s) {
  // 4-wave dK/dV: 2 x [Q | dO | lse | delta] tiles of 32 rows
  const int smem_a4 = 2 * (2 * 32 * D * 2 + 2 * 32 * 4);
  // 8-wave dK/dV: K, V images (2 x 128 x D) + 2 x [Q | dO | lse | delta] tiles of 64 rows; the pair
  // reduction reuses the front 2 x 4 x 32 x D f32 of it
  const int smem_a8 = std::max(2 * 128 * D * 2 + 2 * (2 * 64 * D * 2 + 2 * 64 * 4), 2 * 4 * 32 * D * 4);
  const int smem_q32 = 4 * 32 * D * 2, smem_q64 = 4 * 64 * D * 2;  // dQ: 2 x [K | V] tiles
  const int smem_qds = 2 * (64 * D * 2 + 64 * 128 * 2);            // dQ from dS^T: 2 x [K | dS^T] tiles
  static bool once = false;
  if (!once) {
    set_smem(attn_bwd_dkdv_k<D, CAUSAL, SEQ>, smem_a4);
    if constexpr (kVarlen<SEQ>) {
      set_smem(attn_bwd_dkdv8_varlen_k<D, false>, smem_a8);
      set_smem(attn_bwd_dkdv8_varlen_k<D, true>, smem_a8);
    } else {
      set_smem(attn_bwd_dkdv8_k<D, CAUSAL, false>, smem_a8);
      set_smem(attn_bwd_dkdv8_k<D, CAUSAL, true>, smem_a8);
    }
    set_smem(attn_bwd_dq_k<D, CAUSAL, 32, SEQ>, smem_q32);
    set_smem(attn_bwd_dq_k<D, CAUSAL, 64, SEQ>, smem_q64);
    set_smem(attn_bwd_dq_ds_k<D, CAUSAL, SEQ>, smem_qds);
    once = true;
  }
  const int64_t rows = (int64_t)B * Lq * H;
  if constexpr (kVarlen<SEQ>)
    attn_delta_k<D, VarSeq><<<(unsigned)cdiv(rows * (D / 8), 256), 256, 0, s>>>(o, ldo, dout, lddo, delta, B, H, ks);
  else
    attn_delta_k<D><<<(unsigned)cdiv(rows * (D / 8), 256), 256, 0, s>>>(o, ldo, dout, lddo, delta, B, H, Lq);
  const unsigned gk = (unsigned)(cdiv(Lk, 128) * H * B), gq = (unsigned)(cdiv(Lq, 128) * H * B);
  // the dS^T workspace is row-major: LkP key rows of LqP queries, 128-query block qb at column 128 qb
  const int64_t LkP = ds_rows(Lk), LqP = ds_cols(Lq);
  if (mode == 7 || mode == 4) {
    u16* st = mode == 7 ? ds : nullptr;
    const int64_t ldst = mode == 7 ? LqP : 0, st_bh = mode == 7 ? LkP * LqP : 0, st_blk = mode == 7 ? 128 : 0;
    if constexpr (kVarlen<SEQ>) {
      static_assert(CAUSAL, "packed sequences are causal");
      if (mode == 7)
        attn_bwd_dkdv8_varlen_k<D, true><<<gk, 512, smem_a8, s>>>(q, ldq, k, ldk, v, ldv, dout, lddo, lse, delta, dk, lddk,
                                                                 dv, lddv, H, scale, ks, st, ldst, st_bh, st_blk);
      else
        attn_bwd_dkdv8_varlen_k<D, false><<<gk, 512, smem_a8, s>>>(q, ldq, k, ldk, v, ldv, dout, lddo, lse, delta, dk, lddk,
                                                                  dv, lddv, H, scale, ks, st, ldst, st_bh, st_blk);
    } else {
      if (mode == 7)
        attn_bwd_dkdv8_k<D, CAUSAL, true><<<gk, 512, smem_a8, s>>>(q, ldq, k, ldk, v, ldv, dout, lddo, lse, delta, dk, lddk,
                                                                  dv, lddv, H, Lq, Lk, scale, ks, st, ldst, st_bh, st_blk);
      else
        attn_bwd_dkdv8_k<D, CAUSAL, false><<<gk, 512, smem_a8, s>>>(q, ldq, k, ldk, v, ldv, dout, lddo, lse, delta, dk, lddk,
                                                                   dv, lddv, H, Lq, Lk, scale, ks, st, ldst, st_bh, st_blk);
    }
  } else
    attn_bwd_dkdv_k<D, CAUSAL, SEQ><<<gk, 256, smem_a4, s>>>(q, ldq, k, ldk, v, ldv, dout, lddo, lse, delta, dk, lddk, dv,
                                                      lddv, H, Lq, Lk, scale, ks);
  if (mode == 7)
    attn_bwd_dq_ds_k<D, CAUSAL, SEQ><<<gq, 256, smem_qds, s>>>(k, ldk, ds, LqP, LkP * LqP, 128, (int)LkP, dq, lddq, H, Lq, Lk,
                                                        scale, ks);
  else if (mode == 2)
    attn_bwd_dq_k<D, CAUSAL, 64, SEQ><<<gq, 256, smem_q64, s>>>(q, ldq, k, ldk, v, ldv, dout, lddo, lse, delta, dq, lddq, H,
                                                         Lq, Lk, scale, ks);
  else
    attn_bwd_dq_k<D, CAUSAL, 32, SEQ><<<gq, 256, smem_q32, s>>>(q, ldq, k, ldk, v, ldv, dout, lddo, lse, delta, dq, lddq, H,
                                                         Lq, Lk, scale, ks);
  return cullavo_check_launch(kVarlen<SEQ> ? "attn_bwd_varlen" : "attn_bwd");
}

}  // namespace

extern "C" int cullavo_attn_set_stage(int stage) {
  const int prev = g_fwd_stage;
  if (stage == -1 || stage == 4 || stage == 7) g_fwd_stage = stage;
  return prev;
}

extern "C" int cullavo_attn_set_rescale(float threshold, float* previous) {
  CV_REQUIRE(threshold >= 0.f && threshold <= 16.f, CULLAVO_EINVAL, "rescale threshold must be in [0, 16]");
  if (previous && hipMemcpyFromSymbol(previous, HIP_SYMBOL(g_rescale_thr), sizeof(float)) != hipSuccess)
    return CULLAVO_EHIP;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_rescale_thr), &threshold, sizeof(float)) != hipSuccess) return CULLAVO_EHIP;
  return CULLAVO_OK;
}

extern "C" int cullavo_attn_set_bwd_tiles(int mode) {
  const int prev = g_bwd_tiles;
  if (mode == -1 || mode == 0 || mode == 2 || mode == 4 || mode == 7) g_bwd_tiles = mode;
  return prev;
}

// The argument checks the attention entry points share, each stated once. Macros, not functions:
// CV_REQUIRE names the entry point it expands in (__func__) and returns from it. They read the entry
// point's own dtype, D, H, Lq, Lk, causal, ldq, ld_tok, ld_batch and ldo.
template <typename... S>
static bool all_x8(S... ld) { return ((ld % 8 == 0) && ...); }
template <typename... S>
static bool all_hold(int64_t row, S... ld) { return ((ld >= row) && ...); }
#define ATTN_REQUIRE_TYPE_AND_DIM()                                                                                \
  CV_REQUIRE(dtype == CULLAVO_DT_BF16 || dtype == CULLAVO_DT_F32, CULLAVO_EUNSUPPORTED, "attention: bf16 / f32"); \
  CV_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, CULLAVO_EUNSUPPORTED, "head_dim must be 16, 32, 64 or 128")
#define ATTN_REQUIRE_CAUSAL_SQUARE() CV_REQUIRE(!causal || Lq == Lk, CULLAVO_EINVAL, "causal attention needs Lq == Lk")
#define ATTN_REQUIRE_STRIDES_X8(...) \
  CV_REQUIRE(all_x8(__VA_ARGS__), CULLAVO_EINVAL, "token strides must be multiples of 8")
#define ATTN_REQUIRE_STRIDES_HOLD_HD(...) \
  CV_REQUIRE(all_hold((int64_t)H * D, __VA_ARGS__), CULLAVO_EINVAL, "token stride smaller than H*D")
#define ATTN_REQUIRE_CACHE_STRIDES()         \
  ATTN_REQUIRE_STRIDES_X8(ldq, ld_tok, ldo); \
  ATTN_REQUIRE_STRIDES_HOLD_HD(ldq, ld_tok, ldo); \
  CV_REQUIRE(ld_batch % 8 == 0, CULLAVO_EINVAL, "the cache's batch stride must be a multiple of 8")
// f32 storage (the parity mode) and the config-1 head dims run the kernels of attn_generic.hip
#define ATTN_GENERIC (dtype == CULLAVO_DT_F32 || D < 64)

extern "C" int cullavo_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                int64_t ldv, void* o, int64_t ldo, float* lse, int B, int H, int Lq, int Lk,
                                int D, float scale, int causal, const int32_t* kv_start, int dtype,
                                void* stream) {
  ATTN_REQUIRE_TYPE_AND_DIM();
  ATTN_REQUIRE_CAUSAL_SQUARE();
  ATTN_REQUIRE_STRIDES_X8(ldq, ldk, ldv, ldo);
  ATTN_REQUIRE_STRIDES_HOLD_HD(ldq, ldk, ldv, ldo);
  if (B == 0 || H == 0 || Lq == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  if (ATTN_GENERIC)
    return cullavo_attn_generic_fwd(q, ldq, k, ldk, v, ldv, o, ldo, lse, B, H, Lq, Lk, D, scale, causal, kv_start,
                                    dtype, s);
  const u16 *Q = (const u16*)q, *K = (const u16*)k, *V = (const u16*)v;
  u16* O = (u16*)o;
  if (D == 128)
    return causal ? fwd_launch<128, true>(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Lq, Lk, scale, kv_start, s)
                  : fwd_launch<128, false>(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Lq, Lk, scale, kv_start, s);
  return causal ? fwd_launch<64, true>(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Lq, Lk, scale, kv_start, s)
                : fwd_launch<64, false>(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Lq, Lk, scale, kv_start, s);
}

extern "C" int cullavo_attn_fwd_cached(const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                       int64_t ld_tok, int64_t ld_batch, void* o, int64_t ldo, float* lse, int B,
                                       int H, int Lq, int past, int D, float scale, const int32_t* kv_start,
                                       int dtype, void* stream) {
  ATTN_REQUIRE_TYPE_AND_DIM();
  CV_REQUIRE(B >= 0 && H >= 0 && Lq >= 0, CULLAVO_EINVAL, "B, H and Lq must not be negative");
  CV_REQUIRE(past >= 0, CULLAVO_EINVAL, "past must not be negative");
  CV_REQUIRE((int64_t)past + Lq <= INT32_MAX, CULLAVO_EINVAL, "past + Lq exceeds the key index range");
  ATTN_REQUIRE_CACHE_STRIDES();
  CV_REQUIRE(ld_batch >= ((int64_t)past + Lq) * ld_tok, CULLAVO_EINVAL,
             "the cache's batch stride is smaller than (past + Lq) rows");
  if (B == 0 || H == 0 || Lq == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  if (ATTN_GENERIC)
    return cullavo_attn_generic_fwd_cached(q, ldq, k_cache, v_cache, ld_tok, ld_batch, o, ldo, lse, B, H, Lq, past, D,
                                           scale, kv_start, dtype, s);
  const u16 *Q = (const u16*)q, *K = (const u16*)k_cache, *V = (const u16*)v_cache;
  u16* O = (u16*)o;
  if (D == 128) return fwd_cached_launch<128>(Q, ldq, K, V, ld_tok, ld_batch, O, ldo, lse, B, H, Lq, past, scale, kv_start, s);
  return fwd_cached_launch<64>(Q, ldq, K, V, ld_tok, ld_batch, O, ldo, lse, B, H, Lq, past, scale, kv_start, s);
}

extern "C" int cullavo_attn_fwd_ragged(const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                       int64_t ld_tok, int64_t ld_batch, void* o, int64_t ldo, float* lse, int B,
                                       int H, int Lq, const int32_t* kv_len, const int32_t* q_pad, int D,
                                       float scale, const int32_t* kv_start, int dtype, void* stream) {
  ATTN_REQUIRE_TYPE_AND_DIM();
  CV_REQUIRE(B >= 0 && H >= 0, CULLAVO_EINVAL, "B and H must not be negative");
  CV_REQUIRE(Lq >= 1, CULLAVO_EINVAL, "attn_fwd_ragged: Lq must be at least 1");
  CV_REQUIRE(kv_len != nullptr, CULLAVO_EINVAL, "attn_fwd_ragged: kv_len (the filled rows per sequence) is null");
  ATTN_REQUIRE_CACHE_STRIDES();
  CV_REQUIRE(ld_batch >= ld_tok, CULLAVO_EINVAL, "the cache's batch stride is smaller than one row");
  if (B == 0 || H == 0) return CULLAVO_OK;
  // the rows of a sequence's slab: the bound the kernel clamps kv_len[b] to
  const int cap = (int)std::min<int64_t>(ld_batch / ld_tok, INT32_MAX - Lq);
  hipStream_t s = CV_STREAM(stream);
  if (ATTN_GENERIC)
    return cullavo_attn_generic_fwd_ragged(q, ldq, k_cache, v_cache, ld_tok, ld_batch, o, ldo, lse, B, H, Lq, cap, D,
                                           scale, kv_start, kv_len, q_pad, dtype, s);
  const u16 *Q = (const u16*)q, *K = (const u16*)k_cache, *V = (const u16*)v_cache;
  u16* O = (u16*)o;
  if (D == 128)
    return fwd_ragged_launch<128>(Q, ldq, K, V, ld_tok, ld_batch, O, ldo, lse, B, H, Lq, cap, scale, kv_start, kv_len,
                                  q_pad, s);
  return fwd_ragged_launch<64>(Q, ldq, K, V, ld_tok, ld_batch, O, ldo, lse, B, H, Lq, cap, scale, kv_start, kv_len,
                               q_pad, s);
}

// default: D=128 (the LM) mode 7 -- in the 7B shape 532 us per layer against 667 for mode 4
// (tools/attn_bench.py), the dQ kernel no longer recomputes S and dP; D=64 (the ViT) mode 2 (647
// vs 797 us for mode 4 at B=64, T=577, H=16: there the 4-wave kernels already hold K/V in registers
// at < 256 VGPRs and the 8-wave LDS re-reads cost more than the second wave hides)
static int bwd_mode(int D) { return g_bwd_tiles >= 0 ? g_bwd_tiles : (D == 128 ? 7 : 2); }

extern "C" size_t cullavo_attn_bwd_workspace(int B, int H, int Lq, int Lk, int D, int dtype) {
  if (dtype != CULLAVO_DT_BF16 || D < 64 || B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || (bwd_mode(D) != 7))
    return 0;
  return (size_t)B * H * ds_rows(Lk) * ds_cols(Lq) * 2;
}

extern "C" int cullavo_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                int64_t ldv, const void* o, int64_t ldo, const void* dout, int64_t lddo,
                                const float* lse, float* delta, void* dq, int64_t lddq, void* dk,
                                int64_t lddk, void* dv, int64_t lddv, int B, int H, int Lq, int Lk, int D,
                                float scale, int causal, const int32_t* kv_start, int dtype, void* stream) {
  return cullavo_attn_bwd_ws(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, delta, dq, lddq, dk, lddk, dv, lddv,
                             B, H, Lq, Lk, D, scale, causal, kv_start, dtype, nullptr, 0, stream);
}

extern "C" int cullavo_attn_bwd_ws(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                   int64_t ldv, const void* o, int64_t ldo, const void* dout, int64_t lddo,
                                   const float* lse, float* delta, void* dq, int64_t lddq, void* dk,
                                   int64_t lddk, void* dv, int64_t lddv, int B, int H, int Lq, int Lk, int D,
                                   float scale, int causal, const int32_t* kv_start, int dtype, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  ATTN_REQUIRE_TYPE_AND_DIM();
  ATTN_REQUIRE_CAUSAL_SQUARE();
  ATTN_REQUIRE_STRIDES_X8(ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv);
  if (B == 0 || H == 0 || Lq == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  if (ATTN_GENERIC)
    return cullavo_attn_generic_bwd(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, delta, dq, lddq, dk, lddk, dv,
                                    lddv, B, H, Lq, Lk, D, scale, causal, kv_start, dtype, s);
  const u16 *Q = (const u16*)q, *K = (const u16*)k, *V = (const u16*)v, *O = (const u16*)o, *dO = (const u16*)dout;
  u16 *dQ = (u16*)dq, *dK = (u16*)dk, *dV = (u16*)dv;
  // mode 7 needs its dS^T workspace; without one the recompute path runs (mode 4: the same dK / dV
  // kernel without the dS^T stores, and the 4-wave dQ kernel)
  int mode = bwd_mode(D);
  u16* ds = (u16*)workspace;
  if (mode == 7 && (ds == nullptr || workspace_bytes < cullavo_attn_bwd_workspace(B, H, Lq, Lk, D, dtype))) mode = 4;
  auto run = [&](auto d_c, auto causal_c) {
    return bwd_launch<decltype(d_c)::value, decltype(causal_c)::value, const int32_t*>(Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse,
                                                                       delta, dQ, lddq, dK, lddk, dV, lddv, B, H, Lq,
                                                                       Lk, scale, kv_start, mode, ds, s);
  };
  using D128 = std::integral_constant<int, 128>;
  using D64 = std::integral_constant<int, 64>;
  if (D == 128) return causal ? run(D128{}, std::true_type{}) : run(D128{}, std::false_type{});
  return causal ? run(D64{}, std::true_type{}) : run(D64{}, std::false_type{});
}

// ---- packed sequences of unequal length (causal, bf16, D 64 / 128) -----------------------------
// seq_start / seq_len are device values, so the host checks only what it holds. With
// cullavo_attn_varlen_set_check(1) the entry points also read both arrays back (a stream
// synchronisation per call: for tests and debugging, off by default) and refuse a length outside
// [0, max_len] or a negative start before anything is launched.
static int g_varlen_check = 0;

extern "C" int cullavo_attn_varlen_set_check(int on) {
  const int prev = g_varlen_check;
  g_varlen_check = on != 0;
  return prev;
}

static int varlen_check_device(const char* fn, const int32_t* seq_start, const int32_t* seq_len, int B, int max_len,
                               hipStream_t s) {
  std::vector<int32_t> host(2 * (size_t)B);
  if (hipMemcpyAsync(host.data(), seq_start, B * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(host.data() + B, seq_len, B * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return cullavo_set_error(std::string(fn) + ": reading seq_start / seq_len back failed"), CULLAVO_EHIP;
  for (int b = 0; b < B; ++b) {
    if (host[B + b] < 0 || host[B + b] > max_len)
      return cullavo_set_error(std::string(fn) + ": max_len is below a sequence's length (or a length is negative)"), CULLAVO_EINVAL;
    if (host[b] < 0) return cullavo_set_error(std::string(fn) + ": a sequence start is negative"), CULLAVO_EINVAL;
  }
  return CULLAVO_OK;
}

#define ATTN_REQUIRE_VARLEN()                                                                                      \
  CV_REQUIRE(dtype == CULLAVO_DT_BF16, CULLAVO_EUNSUPPORTED, "varlen attention: bf16 only");                       \
  CV_REQUIRE(D == 64 || D == 128, CULLAVO_EUNSUPPORTED, "varlen attention: head_dim must be 64 or 128");           \
  CV_REQUIRE(B >= 0 && H >= 0 && max_len >= 0, CULLAVO_EINVAL, "B, H and max_len must not be negative");           \
  CV_REQUIRE(seq_start != nullptr && seq_len != nullptr, CULLAVO_EINVAL, "varlen attention: seq_start or seq_len is null")

extern "C" int cullavo_attn_fwd_varlen(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                       int64_t ldv, void* o, int64_t ldo, float* lse, const int32_t* seq_start,
                                       const int32_t* seq_len, int B, int H, int max_len, int D, float scale,
                                       int dtype, void* stream) {
  ATTN_REQUIRE_VARLEN();
  ATTN_REQUIRE_STRIDES_X8(ldq, ldk, ldv, ldo);
  ATTN_REQUIRE_STRIDES_HOLD_HD(ldq, ldk, ldv, ldo);
  if (B == 0 || H == 0 || max_len == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  if (g_varlen_check) {
    const int rc = varlen_check_device(__func__, seq_start, seq_len, B, max_len, s);
    if (rc != CULLAVO_OK) return rc;
  }
  const u16 *Q = (const u16*)q, *K = (const u16*)k, *V = (const u16*)v;
  u16* O = (u16*)o;
  if (D == 128) return fwd_varlen_launch<128>(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_len, scale, seq_start, seq_len, s);
  return fwd_varlen_launch<64>(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, max_len, scale, seq_start, seq_len, s);
}

extern "C" int cullavo_attn_bwd_varlen(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                       int64_t ldv, const void* o, int64_t ldo, const void* dout, int64_t lddo,
                                       const float* lse, float* delta, void* dq, int64_t lddq, void* dk,
                                       int64_t lddk, void* dv, int64_t lddv, const int32_t* seq_start,
                                       const int32_t* seq_len, int B, int H, int max_len, int D, float scale,
                                       int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  ATTN_REQUIRE_VARLEN();
  ATTN_REQUIRE_STRIDES_X8(ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv);
  ATTN_REQUIRE_STRIDES_HOLD_HD(ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv);
  if (B == 0 || H == 0 || max_len == 0) return CULLAVO_OK;
  hipStream_t s = CV_STREAM(stream);
  if (g_varlen_check) {
    const int rc = varlen_check_device(__func__, seq_start, seq_len, B, max_len, s);
    if (rc != CULLAVO_OK) return rc;
  }
  // as cullavo_attn_bwd_ws: mode 7 without its dS^T workspace runs the recompute path
  int mode = bwd_mode(D);
  u16* ds = (u16*)workspace;
  if (mode == 7 && (ds == nullptr || workspace_bytes < cullavo_attn_bwd_workspace(B, H, max_len, max_len, D, dtype)))
    mode = 4;
  const VarSeq sq{seq_start, seq_len, max_len};
  const u16 *Q = (const u16*)q, *K = (const u16*)k, *V = (const u16*)v, *O = (const u16*)o, *dO = (const u16*)dout;
  u16 *dQ = (u16*)dq, *dK = (u16*)dk, *dV = (u16*)dv;
  if (D == 128)
    return bwd_launch<128, true, VarSeq>(Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse, delta, dQ, lddq, dK, lddk, dV,
                                         lddv, B, H, max_len, max_len, scale, sq, mode, ds, s);
  return bwd_launch<64, true, VarSeq>(Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse, delta, dQ, lddq, dK, lddk, dV,
                                      lddv, B, H, max_len, max_len, scale, sq, mode, ds, s);
}
