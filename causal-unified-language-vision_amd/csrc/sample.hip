// Token sampling for generate() (reference cullavo/arch_cullavo.py:362-365: generate(do_sample=True,
// temperature=0.9, top_k=50, top_p=0.95, ...) and HF's warper order behind it: temperature ->
// top-k -> top-p -> multinomial): one launch per decode step, captured at the end of the decode
// graph, that turns the step's logits into the next step's input token on the device.
//
// One workgroup of 16 waves per row; rows are independent and nothing is written outside the row's
// own slots. Per row:
//   1. x = f32(logit) / temperature (a true division).
//   2. top-k threshold: two-pass 8-bit radix select on the order-preserving 16-bit key of the bf16
//      logit (integer LDS histograms); every token with x >= the k-th largest x survives, ties
//      included (masked_fill(x < kth)), so more than k may survive.
//   3. the tokens strictly above the threshold (at most top_k - 1) go to LDS and are ranked into the
//      canonical order (descending x, ascending id); the run tied at the threshold is kept as
//      (value, count) whatever its length, its j-th member (ascending id) recovered by an ordered
//      count over the row.
//   4. top-p on the f32 softmax of the survivors (accurate expf): a survivor is removed iff the
//      mass of itself and everything after it in canonical order is <= 1 - top_p; the first is
//      always kept; top_p = 1 removes nothing.
//   5. draw: u * (kept mass) against the running sum in canonical order, u from Philox4x32-10
//      keyed by the seed with the counter (step, row_offset); greedy: the lowest-id arg-max.
//   6. bookkeeping: finished rows emit pad_id, a row emitting eos_id becomes finished, the token
//      goes to next_ids[b] and out_tokens[b, step[b]], step[b] += 1.
// Every float reduction is a scan or tree in a fixed order (no float atomics): a row's result is
// bitwise the same from run to run and whatever the batch around it.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 1024;  // top_k <= 1024: at most 1023 tokens strictly above the threshold

// order-preserving 16-bit key of a bf16 (larger value, larger key) and its inverse
DEV unsigned bf_key(u16 b) { return (b & 0x8000u) ? (~(unsigned)b & 0xFFFFu) : ((unsigned)b | 0x8000u); }
DEV u16 key_bf(unsigned k) { return (k & 0x8000u) ? (u16)(k & 0x7FFFu) : (u16)(~k & 0xFFFFu); }
// the same for f32
DEV uint32_t f_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
DEV float key_f(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

// the warped logit; -0 becomes +0 so that equal values have one bit pattern
DEV float warp(u16 bits, float temperature) {
  const float x = bf2f(bits) / temperature;
  return x == 0.f ? 0.f : x;
}

// Philox4x32-10 (Random123 constants)
DEV void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// inclusive scan over the workgroup's threads in thread order (wave shuffles, then the wave totals
// added in wave order: a fixed association); total = the sum over all threads
template <typename T>
DEV T block_scan(T v, T* wtot, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();  // wtot may still be read from an earlier scan
  if (lane == 63) wtot[w] = v;
  __syncthreads();
  T off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const T c = wtot[i];
    if (i < w) off += c;
    tot += c;
  }
  total = tot;
  return v + off;
}

// hist[bin] += 1 for the active lanes, called by whole waves: lanes that share a bin with the
// first pending lane are counted by one LDS add (a few rounds: the high byte of a bf16 key takes
// few values per row), the rest by their own
DEV void hist_add(int* hist, int bin, bool active) {
  const int lane = threadIdx.x & 63;
  bool pending = active;
#pragma unroll 1
  for (int round = 0; round < 4; ++round) {
    const unsigned long long rem = __ballot(pending);
    if (rem == 0) return;
    const int leader = __ffsll((long long)rem) - 1;
    const int lb = __shfl(bin, leader, 64);
    const bool mine = pending && bin == lb;
    const unsigned long long m = __ballot(mine);
    if (lane == leader) atomicAdd(&hist[lb], __popcll(m));
    pending = pending && !mine;
  }
  if (pending) atomicAdd(&hist[bin], 1);
}

// wave 0: the bin (counted from 255 down) in which the cumulative count reaches k, and the count
// in the bins above it
DEV void select_bin(const int* hist, int k, int* out_bin, int* out_above) {
  const int lane = threadIdx.x & 63;
  int c[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { c[j] = hist[255 - (4 * lane + j)]; s += c[j]; }
  int incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  int e = incl - s;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (e < k && e + c[j] >= k) { *out_bin = 255 - (4 * lane + j); *out_above = e; }
    e += c[j];
  }
}

// f(id, bits, active) over the row, every wave running the same number of iterations (f may use
// wave-wide operations): 16-byte loads where the row is 16-byte aligned, then the tail
template <typename F>
DEV void row_pass(const u16* __restrict__ row, int V, F f) {
  const int t = threadIdx.x;
  const int nv = ((reinterpret_cast<uintptr_t>(row) & 15) == 0) ? V / 8 : 0;
  for (int base = 0; base < nv; base += kThreads) {
    const int i = base + t;
    const bool act = i < nv;
    u16x8 q = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) q = *reinterpret_cast<const u16x8*>(row + (int64_t)i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) f(i * 8 + j, q[j], act);
  }
  for (int base = nv * 8; base < V; base += kThreads) {
    const int i = base + t;
    const bool act = i < V;
    f(i, act ? row[i] : (u16)0, act);
  }
}

struct SampleArgs {
  const u16* logits;
  int64_t ldl;
  int V;
  float temperature;
  int top_k;
  float top_p;
  int do_sample;
  uint64_t seed;
  const int64_t* row_offset;
  int64_t* step;
  int64_t eos_id, pad_id;
  uint8_t* finished;
  int64_t* next_ids;
  int64_t* out_tokens;
  int64_t ld_out, n_out;
  int32_t* keep_ids;
  float* keep_probs;
  int32_t* n_keep;
  int64_t cap;
};

__global__ __launch_bounds__(kThreads) void sample_token_k(SampleArgs p) {
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const u16* __restrict__ row = p.logits + (int64_t)b * p.ldl;
  const int V = p.V;
  __shared__ int hist[256];
  __shared__ int sel[4];            // high bin, count above it, low bin, count above it
  __shared__ int n_above_s, tok_s;
  __shared__ unsigned long long ent[kMaxK];  // (descending-x key, id) of the tokens above the threshold
  __shared__ float xs[kMaxK];       // the same in canonical order
  __shared__ int ids[kMaxK];
  __shared__ float pre[kMaxK];      // inclusive running sum of exp(x - max) in canonical order
  __shared__ float wtf[kWaves];
  __shared__ long long wtl[kWaves];
  __shared__ float bxs[kWaves];
  __shared__ int bis[kWaves];

  int drawn = 0;
  if (!p.do_sample) {
    // greedy: the lowest-id arg-max
    float bx = -INFINITY;
    int bi = INT_MAX;
    row_pass(row, V, [&](int id, u16 bits, bool act) {
      const float v = bf2f(bits);
      if (act && (v > bx || (v == bx && id < bi))) { bx = v; bi = id; }
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ox = __shfl_xor(bx, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ox > bx || (ox == bx && oi < bi)) { bx = ox; bi = oi; }
    }
    if (lane == 0) { bxs[w] = bx; bis[w] = bi; }
    __syncthreads();
    bx = bxs[0]; bi = bis[0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i)
      if (bxs[i] > bx || (bxs[i] == bx && bis[i] < bi)) { bx = bxs[i]; bi = bis[i]; }
    drawn = bi == INT_MAX ? 0 : bi;  // a row of NaN
    if (t == 0) {
      if (p.n_keep) p.n_keep[b] = 1;
      if (p.keep_ids && p.cap > 0) { p.keep_ids[(int64_t)b * p.cap] = drawn; p.keep_probs[(int64_t)b * p.cap] = 1.f; }
    }
  } else {
    const int k = min(p.top_k, V);  // V < top_k: every token survives
    // ---- top-k threshold: radix select, high byte then low byte of the key ----
    if (t < 256) hist[t] = 0;
    if (t < 4) sel[t] = 0;
    if (t == 0) { n_above_s = 0; tok_s = 0; }
    __syncthreads();
    row_pass(row, V, [&](int, u16 bits, bool act) { hist_add(hist, (int)(bf_key(bits) >> 8), act); });
    __syncthreads();
    if (w == 0) select_bin(hist, k, &sel[0], &sel[1]);
    __syncthreads();
    const int hi_bin = sel[0], k2 = k - sel[1];
    if (t < 256) hist[t] = 0;
    __syncthreads();
    row_pass(row, V, [&](int, u16 bits, bool act) {
      const unsigned key = bf_key(bits);
      hist_add(hist, (int)(key & 255u), act && (int)(key >> 8) == hi_bin);
    });
    __syncthreads();
    if (w == 0) select_bin(hist, k2, &sel[2], &sel[3]);
    __syncthreads();
    const float xk = warp(key_bf(((unsigned)hi_bin << 8) | (unsigned)sel[2]), p.temperature);
    // ---- the tokens above the threshold into LDS; the tie run is counted ----
    long long my_ties = 0;
    row_pass(row, V, [&](int id, u16 bits, bool act) {
      const float x = warp(bits, p.temperature);
      if (act && x > xk) {
        const int slot = atomicAdd(&n_above_s, 1);
        if (slot < kMaxK)
          ent[slot] = ((unsigned long long)(~f_key(x)) << 32) | (unsigned)id;
      } else if (act && x == xk) {
        ++my_ties;
      }
    });
    long long n_tie_l;
    block_scan<long long>(my_ties, wtl, n_tie_l);  // its barriers also publish ent / n_above_s
    const int n_tie = (int)n_tie_l;
    const int n_above = min(n_above_s, kMaxK - 1);
    // canonical order: rank = the number of entries that come before (keys are distinct)
    if (t < n_above) {
      const unsigned long long my = ent[t];
      int r = 0;
      for (int j = 0; j < n_above; ++j) r += ent[j] < my ? 1 : 0;
      xs[r] = key_f(~(uint32_t)(my >> 32));
      ids[r] = (int)(uint32_t)my;
    }
    __syncthreads();
    // ---- softmax masses in canonical order ----
    const float xmax = n_above ? xs[0] : xk;
    const float e_t = expf(xk - xmax);
    const float e = t < n_above ? expf(xs[t] - xmax) : 0.f;
    float above_mass;
    pre[t] = block_scan<float>(e, wtf, above_mass);
    __syncthreads();
    const float total = above_mass + (float)n_tie * e_t;
    // ---- top-p: a survivor stays iff the mass from itself to the end exceeds 1 - top_p ----
    const bool keep_all = p.top_p >= 1.f;
    const float thr = 1.f - p.top_p;
    long long cnt = 0;  // low half: kept above the threshold; high half: kept members of the run
    if (t < n_above && (keep_all || (total - (t ? pre[t - 1] : 0.f)) / total > thr)) cnt = 1;
    for (int j = t; j < n_tie; j += kThreads)
      if (keep_all || (float)(n_tie - j) * e_t / total > thr) cnt += 1ll << 32;
    long long cnt_tot;
    block_scan<long long>(cnt, wtl, cnt_tot);
    int ka = (int)(cnt_tot & 0xFFFFFFFFll), kt = (int)(cnt_tot >> 32);
    if (ka < n_above) kt = 0;
    if (ka + kt == 0) {  // the first in canonical order always stays
      if (n_above) ka = 1;
      else if (n_tie) kt = 1;
    }
    const int nk = ka + kt;
    const float kept_above = ka ? pre[ka - 1] : 0.f;
    const float mass = kept_above + (float)kt * e_t;
    // ---- the draw: the first token whose running sum exceeds u * mass ----
    uint32_t c[4];
    const int64_t st = p.step[b], ro = p.row_offset ? p.row_offset[b] : (int64_t)b;
    c[0] = (uint32_t)st; c[1] = (uint32_t)((uint64_t)st >> 32);
    c[2] = (uint32_t)ro; c[3] = (uint32_t)((uint64_t)ro >> 32);
    philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const float u = (float)(c[0] >> 8) * 0x1p-24f;
    const float target = u * mass;
    cnt = 0;
    if (t < ka && pre[t] <= target) cnt = 1;
    for (int j = t; j < kt; j += kThreads)
      if (kept_above + (float)(j + 1) * e_t <= target) cnt += 1ll << 32;
    block_scan<long long>(cnt, wtl, cnt_tot);
    int idx = (int)(cnt_tot & 0xFFFFFFFFll) + (int)(cnt_tot >> 32);
    idx = max(0, min(idx, nk - 1));
    const int tie_pick = idx >= ka ? idx - ka : -1;  // the run's member drawn (ascending id), if any
    if (idx < ka) drawn = ids[idx];
    // debug outputs: the kept tokens above the threshold
    if (p.keep_ids && t < ka && t < p.cap) {
      p.keep_ids[(int64_t)b * p.cap + t] = ids[t];
      p.keep_probs[(int64_t)b * p.cap + t] = e / mass;
    }
    if (t == 0 && p.n_keep) p.n_keep[b] = nk;
    // ---- the run's members by ordered count: thread t owns ids [t seg, (t + 1) seg) ----
    if (kt > 0 && (tie_pick >= 0 || p.keep_ids)) {
      const int seg = (V + kThreads - 1) / kThreads;
      const int lo = min(V, t * seg), hi = min(V, lo + seg);
      long long mine = 0;
      for (int i = lo; i < hi; ++i) mine += warp(row[i], p.temperature) == xk ? 1 : 0;
      long long tot;
      long long ord = block_scan<long long>(mine, wtl, tot) - mine;
      for (int i = lo; i < hi; ++i) {
        if (warp(row[i], p.temperature) != xk) continue;
        if (ord == tie_pick) tok_s = i;
        if (p.keep_ids && ord < kt && ka + ord < p.cap) {
          p.keep_ids[(int64_t)b * p.cap + ka + ord] = i;
          p.keep_probs[(int64_t)b * p.cap + ka + ord] = e_t / mass;
        }
        ++ord;
      }
      __syncthreads();
      if (tie_pick >= 0) drawn = tok_s;
    }
  }
  // ---- bookkeeping ----
  if (t == 0) {
    const int64_t st = p.step[b];
    uint8_t fin = p.finished ? p.finished[b] : (uint8_t)0;
    const int64_t tok = fin ? p.pad_id : (int64_t)drawn;
    if (p.eos_id >= 0 && tok == p.eos_id) fin = 1;
    if (p.finished) p.finished[b] = fin;
    p.next_ids[b] = tok;
    if (p.out_tokens && st >= 0 && st < p.n_out) p.out_tokens[(int64_t)b * p.ld_out + st] = tok;
    p.step[b] = st + 1;
  }
}

}  // namespace

extern "C" int cullavo_sample_token(const void* logits, int64_t ldl, int B, int64_t V, int dtype, float temperature,
                                    int top_k, float top_p, int do_sample, uint64_t seed, const int64_t* row_offset,
                                    int64_t* step, int64_t eos_id, int64_t pad_id, uint8_t* finished,
                                    int64_t* next_ids, int64_t* out_tokens, int64_t ld_out, int64_t n_out,
                                    int32_t* keep_ids, float* keep_probs, int32_t* n_keep, int64_t cap, void* stream) {
  CV_REQUIRE(dtype == CULLAVO_DT_BF16, CULLAVO_EINVAL, "bf16 logits only (cached decode is bf16)");
  CV_REQUIRE(V >= 1 && V <= (int64_t)1 << 30, CULLAVO_EINVAL, "V must be in 1 .. 2^30 (32-bit token indices)");
  CV_REQUIRE(top_k >= 1 && top_k <= kMaxK, CULLAVO_EINVAL,
             "top_k must be in 1 .. 1024 (top_k = 0, the full-vocabulary nucleus, is not implemented)");
  CV_REQUIRE(std::isfinite(temperature) && temperature > 0.f, CULLAVO_EINVAL,
             "temperature must be finite and > 0");
  CV_REQUIRE(top_p > 0.f && top_p <= 1.f, CULLAVO_EINVAL, "top_p must be in (0, 1]");
  CV_REQUIRE(B >= 0 && ldl >= V, CULLAVO_EINVAL, "B >= 0 and ldl >= V");
  if (B == 0) return CULLAVO_OK;
  CV_REQUIRE(logits != nullptr && step != nullptr && next_ids != nullptr, CULLAVO_EINVAL,
             "logits / step / next_ids");
  CV_REQUIRE(out_tokens == nullptr || (ld_out >= n_out && n_out >= 0), CULLAVO_EINVAL,
             "out_tokens needs ld_out >= n_out >= 0");
  CV_REQUIRE((keep_ids == nullptr) == (keep_probs == nullptr) && (keep_ids == nullptr || cap >= 1), CULLAVO_EINVAL,
             "keep_ids and keep_probs come together, with cap >= 1");
  SampleArgs a{(const u16*)logits, ldl, (int)V, temperature, top_k, top_p, do_sample, seed, row_offset, step,
               eos_id, pad_id, finished, next_ids, out_tokens, ld_out, n_out, keep_ids, keep_probs, n_keep, cap};
  sample_token_k<<<B, kThreads, 0, CV_STREAM(stream)>>>(a);
  return cullavo_check_launch("sample_token");
}
