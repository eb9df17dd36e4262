// The body of attention.hip's pipelined forward kernels, included once per kernel (inside the
// function, after its `constexpr bool CACHED`): attn_fwd_pipe_k<D, CAUSAL> (CACHED = false) and
// attn_fwd_cached_k<D> (CAUSAL = CACHED = true). It is text, not a function both kernels call:
// inlined through a function the same statements came out with another register assignment, and
// attn_fwd_pipe_k has to stay the code it was, instruction for instruction (tools/isa_diff.py).
//
// CACHED: the Lq queries are the LAST Lq positions of Lk = past + Lq keys (bottom-right aligned:
// query i sees keys <= past + i, past = Lk - Lq), and K / V are one layer's KV cache, both with
// token stride ldk, sequence b at element offset b * ldv (ldv carries the cache's batch stride: its
// capacity, not Lk rows). The LDS-DMA descriptors end at row Lk of the sequence's cache, so the
// free rows behind it are never fetched: in a tile's tail they land as zeros and are masked like
// any key >= Lk. Rows below kv_start[b] never reach a result either, whatever they hold: tiles below
// kv_start / 64 are not fetched, and the V rows of the first tile below kv_start are zeroed in LDS.
//
// RAGGED (attn_fwd_ragged_k, CAUSAL = CACHED = true): the kernel sets Lk = kv_len[b] and qpad =
// q_pad[b] (both workgroup-uniform, scalar registers) before these statements, so every bound above
// is the sequence's own. Queries q < qpad are padding: they load no Q row and see no key (kspan =
// 0), which makes them the zero rows with lse = +inf of any query without a visible key; a query
// tile wholly inside the padding runs no key tile (ntiles = 0: nothing is fetched), a tile that
// holds some padding masks every key tile. past = Lk - Lq may be negative (a short cache behind a
// long pad): queries below -past are padding by construction, kspan = 0 covers bad inputs. With
// RAGGED = false, qpad is the constant 0 and every RAGGED term folds away.
//
// VARLEN (attn_fwd_varlen_k, CAUSAL = true, CACHED = RAGGED = false): sequences of unequal length
// packed back to back. The kernel sets Lq = Lk = seq_len[b] and vl_row0 = seq_start[b] (workgroup-
// uniform) before these statements; the grid and the lse rows are sized by vl_max, the host's upper
// bound of the lengths. Only the base rows and the lse row stride differ from the uniform kernel, so
// a sequence's workgroups run the statements of attn_fwd_pipe_k at B = 1, L = seq_len[b], bit for
// bit. With VARLEN = false, vl_max and vl_row0 are constants and every VARLEN term folds away.
  constexpr int KT = 64;
  constexpr int TILE = KT * D * 2;
  constexpr int NS = D / 16;  // k-steps over D: 8 (D = 128) or 4 (D = 64)
  constexpr int ND = D / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // K slots 0, 1 then V slots 0, 1

  const int nqb = ((VARLEN ? vl_max : Lq) + 127) / 128;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qi = lid % nqb, hb = lid / nqb;
  const int qb = CAUSAL ? (nqb - 1 - qi) : qi;
  const int h = hb % H, b = hb / H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
  const int q = qb * 128 + wave * 32 + (lane & 31);
  const int kstart = kv_start ? kv_start[b] : 0;

  const u16* Qb = Q + (VARLEN ? vl_row0 : (int64_t)b * Lq) * ldq + (int64_t)h * D;
  const u16* Kb = K + (CACHED ? (int64_t)b * ldv : (VARLEN ? vl_row0 : (int64_t)b * Lk) * ldk) + (int64_t)h * D;
  const u16* Vb = V + (VARLEN ? vl_row0 : (int64_t)b * (CACHED ? 1 : Lk)) * ldv + (int64_t)h * D;
  const int64_t ldvt = CACHED ? ldk : ldv;  // V's token stride
  const int past = CACHED ? Lk - Lq : 0;

  frag8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    u16x8 v = (q < Lq && (!RAGGED || q >= qpad)) ? *reinterpret_cast<const u16x8*>(Qb + (int64_t)q * ldq + 16 * s + 8 * hf) : u16x8(0);
    qf[s] = __builtin_bit_cast(frag8, v);
  }
  f32x16 o[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) o[i] = f32x16(0.f);
  float m = -INFINITY, l = 0.f;
  const float c = scale * kLog2e;
  const float rescale_thr = g_rescale_thr;
  // key position of this workgroup's first query: every key <= qlo is visible to all its queries
  const int qlo = past + qb * 128;
  const int khi = CAUSAL ? min(Lk, past + q + 1) : Lk;
  const unsigned kspan = (RAGGED && q < qpad) ? 0u : (unsigned)max(khi - kstart, 0);
  const bool qtile_pad = RAGGED && qb * 128 < qpad;  // the tile holds padding queries: mask every key tile
  int kend = Lk;
  if (CAUSAL) kend = min(Lk, qlo + 128);
  const int ntiles = (RAGGED && qb * 128 + 128 <= qpad) ? 0 : (kend + KT - 1) / KT;
  const int t0 = kstart / KT;

  StageDMA1<KT, D, 4> dk_, dv_;
  const int w = __builtin_amdgcn_readfirstlane(wave);
  dk_.prep(ldk, w, lane);
  dv_.prep(ldvt, w, lane);
  auto dma_k = [&](int t, int slot) { dk_.issue(Kb, ldk, t * KT, Lk, smem + slot * TILE, w); };
  auto dma_v = [&](int t, int slot) { dv_.issue(Vb, ldvt, t * KT, Lk, smem + (2 + slot) * TILE, w); };

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
      toff[dt][0] = sbase + 2 * TILE + kv_off<D>(4 * hf + qq, ch) + 8 * (p & 1);
      toff[dt][1] = sbase + 2 * TILE + kv_off<D>(4 * hf + qq + 8, ch) + 8 * (p & 1);
    }
  }

  // S = K Q^T of the K tile in slot SLOT, plain (prologue): NS groups of 2 fragments (32-key half
  // G / (NS / 2), k-steps 2 (G % (NS / 2)) + 0, 1), two groups in flight
  auto s_plain = [&](auto slot_c, f32x16 (&st)[2]) {
    constexpr unsigned KO = decltype(slot_c)::value * TILE;
    constexpr int HG = NS / 2;
    constexpr unsigned K1 = 32 * 2 * D;
    s16x8 ka[2], kb[2];
    st[0] = f32x16(0.f);
    st[1] = f32x16(0.f);
    auto grp = [&](auto g_c) {
      constexpr int G = decltype(g_c)::value;
      constexpr int CNT = G + 1 < NS ? 2 : 0;
      if constexpr (G % 2 == 0) {
        k2_tie<CNT>(ka);
        k2_mfma<NS, 2 * (G % HG)>(ka, qf, st[G / HG]);
        if constexpr (G + 2 < NS) k2_issue<NS, 2 * ((G + 2) % HG), KO + ((G + 2) / HG) * K1>(ka, roff);
      } else {
        k2_tie<CNT>(kb);
        k2_mfma<NS, 2 * (G % HG)>(kb, qf, st[G / HG]);
        if constexpr (G + 2 < NS) k2_issue<NS, 2 * ((G + 2) % HG), KO + ((G + 2) / HG) * K1>(kb, roff);
      }
    };
    k2_issue<NS, 0, KO>(ka, roff);
    k2_issue<NS, 2 * (1 % HG), KO + (1 / HG) * K1>(kb, roff);
    grp(std::integral_constant<int, 0>{});
    grp(std::integral_constant<int, 1>{});
    grp(std::integral_constant<int, 2>{});
    grp(std::integral_constant<int, 3>{});
    if constexpr (NS == 8) {
      grp(std::integral_constant<int, 4>{});
      grp(std::integral_constant<int, 5>{});
      grp(std::integral_constant<int, 6>{});
      grp(std::integral_constant<int, 7>{});
    }
  };

  // Tile t's mask, row max and rescale decision, run on its scores before tile t's iteration (at
  // the end of iteration t-1, or after the prologue's S): no control flow (the mask and rescale
  // branches) may sit between an inline-asm LDS read and its counted wait, since the compiler
  // may then copy the read's destination registers before the data has landed
  float muse = 0.f;
  float alpha_p = 1.f;  // the pending rescale of l, folded into the next row-sum add
  auto prep = [&](int t, f32x16 (&sp)[2]) {
    const int kbase = t * KT;
    const bool need_mask = (CAUSAL && kbase + KT - 1 > qlo) || kbase + KT > Lk || kbase < kstart || qtile_pad;
    if (need_mask) {
      const int koff = kbase + 4 * hf - kstart;
      if (kbase >= kstart) {
        // koff >= 0: key j of the tile is live iff j < kspan - koff (one compare against a
        // constant per score instead of an add and an unsigned compare)
        const int lim = (int)kspan - koff;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) sp[kt][r] = kt * 32 + acc_row(r, 0) < lim ? sp[kt][r] : -INFINITY;
      } else {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            sp[kt][r] = (unsigned)(koff + kt * 32 + acc_row(r, 0)) >= kspan ? -INFINITY : sp[kt][r];
      }
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, sp[kt][r]);
    tmax = swap_max(tmax) * c;
    const bool grow = __any(tmax > m + rescale_thr);  // wave-uniform
    const float mnew = grow ? fmaxf(m, tmax) : m;
    muse = (mnew == -INFINITY) ? 0.f : mnew;
    alpha_p = 1.f;
    if (grow) {
      const float alpha = fast_exp2(m - muse);
      alpha_p = alpha;
#pragma unroll
      for (int i = 0; i < ND; ++i) o[i] *= alpha;
    }
    m = mnew;
  };

  // one tile: P of sp (tile t, masked scores in registers, decision taken by prep) beside S of
  // tile t+1 (K slot KS, into sn; NEXT = false on the last tile: no S), then P V of tile t (V slot
  // VS), then prep of tile t+1
  auto tile = [&](auto ks_c, auto vs_c, auto next_c, int t, f32x16 (&sp)[2], f32x16 (&sn)[2]) {
    constexpr unsigned KO = decltype(ks_c)::value * TILE;
    constexpr unsigned VO = decltype(vs_c)::value * TILE;
    constexpr bool NEXT = decltype(next_c)::value;
    if constexpr (NEXT) {
      // V slot VS^1 was last read by tile t-1's P V, K slot KS^1 by tile t's S (both before the
      // previous barrier)
      dma_v(t + 1, decltype(vs_c)::value ^ 1);
      if (t + 2 < ntiles) dma_k(t + 2, decltype(ks_c)::value ^ 1);
    }
    // S of tile t+1 in NS groups of 2 MFMAs (K fragments 2 groups in flight), each group's issue
    // gaps carrying one (D = 128) or two (D = 64) of the P chunks 0-7 of tile t
    s16x8 ka[2], kb[2];
    s16x4 la[2], ha[2], lb[2], hb[2];  // P V fragment pairs, two in flight
    constexpr int PG = ND / 2;           // pairs per 16-key slice
    constexpr int NPV = 4 * PG;          // P V groups
    float rsE = 0.f, rsO = 0.f;
    frag8 pf[4];
    const float nm = -muse;
    constexpr unsigned K1 = 32 * 2 * D;  // second 32-key half of the K tile
    constexpr int HG = NS / 2;           // groups per 32-key half
    // P chunk C: registers 4 (C % 4) .. + 3 of score tile C / 4, the packed fragment when a
    // 16-key slice is complete
    auto chunk = [&](auto c_c) {
      constexpr int C = decltype(c_c)::value;
      constexpr int KT_ = C / 4, R0 = (C % 4) * 4;
      sm_exp4<KT_, R0>(sp, c, nm, rsE, rsO);
      if constexpr (R0 == 4 || R0 == 12) {
        pf[2 * KT_ + R0 / 8] = pack_frag(sp[KT_], R0 / 8);
        pin(pf[2 * KT_ + R0 / 8]);
      }
    };
    constexpr int kFill[8] = {6, 8, 6, 8, 6, 8, 6, 8};
    // group G: its MFMAs, its chunk(s), then the reads two groups ahead (or the first P V reads)
    auto group = [&](auto g_c) {
      constexpr int G = decltype(g_c)::value;
      constexpr int S0 = 2 * (G % HG);
      if constexpr (NEXT) {
        if constexpr (G % 2 == 0) {
          k2_tie<G == NS - 1 ? 4 : 2>(ka);
          k2_mfma<NS, S0>(ka, qf, sn[G / HG]);
        } else {
          k2_tie<G == NS - 1 ? 4 : 2>(kb);
          k2_mfma<NS, S0>(kb, qf, sn[G / HG]);
        }
      }
      constexpr int CPG = 8 / NS;  // chunks per group
      chunk(std::integral_constant<int, G * CPG>{});
      if constexpr (CPG == 2) chunk(std::integral_constant<int, G * CPG + 1>{});
      if constexpr (NEXT) interleave<2, kFill[G * CPG] + (CPG == 2 ? kFill[G * CPG + 1] : 0)>();
      if constexpr (G + 2 < NS) {
        if constexpr (NEXT) {
          constexpr unsigned OFF2 = KO + ((G + 2) / HG) * K1;
          if constexpr (G % 2 == 0) k2_issue<NS, 2 * ((G + 2) % HG), OFF2>(ka, roff);
          else k2_issue<NS, 2 * ((G + 2) % HG), OFF2>(kb, roff);
        }
      } else if constexpr (G == NS - 2) {
        tr2_issue<ND, VO, 0>(la, ha, toff);  // P V group 0
      } else {
        tr2_issue<ND, VO + (1 / PG) * 16 * 2 * D, 2 * (1 % PG)>(lb, hb, toff);  // P V group 1
      }
    };
    if constexpr (NEXT) {
      sn[0] = f32x16(0.f);
      sn[1] = f32x16(0.f);
      k2_issue<NS, 0, KO>(ka, roff);
      k2_issue<NS, 2 * (1 % HG), KO + (1 / HG) * K1>(kb, roff);
    }
    group(std::integral_constant<int, 0>{});
    group(std::integral_constant<int, 1>{});
    group(std::integral_constant<int, 2>{});
    group(std::integral_constant<int, 3>{});
    if constexpr (NS == 8) {
      group(std::integral_constant<int, 4>{});
      group(std::integral_constant<int, 5>{});
      group(std::integral_constant<int, 6>{});
      group(std::integral_constant<int, 7>{});
    }
    // P V in NPV pair groups (slice v / PG, column blocks 2 (v % PG) + 0, 1), one group in flight
    // under the current one's MFMAs; the row sum beside the first
    auto pv = [&](auto v_c) {
      constexpr int V = decltype(v_c)::value;
      constexpr int CNT = V + 1 < NPV ? 4 : 0;
      if constexpr (V % 2 == 0) {
        tr2_tie<CNT>(la, ha);
        tr2_mfma<ND, 2 * (V % PG)>(la, ha, pf[V / PG], o);
      } else {
        tr2_tie<CNT>(lb, hb);
        tr2_mfma<ND, 2 * (V % PG)>(lb, hb, pf[V / PG], o);
      }
      if constexpr (V == 0) {
        float rs = rsE + rsO;
        rs = swap_sum(rs);
        // l = l alpha + rs in one rounding, as attn_fwd_k's contracted l *= alpha; ...; l += rs
        // (alpha = 1 when the max held: an exact add)
        l = __builtin_fmaf(l, alpha_p, rs);
        interleave<2, 2>();
      }
      if constexpr (V + 2 < NPV) {
        constexpr unsigned VB = VO + ((V + 2) / PG) * 16 * 2 * D;
        if constexpr (V % 2 == 0) tr2_issue<ND, VB, 2 * ((V + 2) % PG)>(la, ha, toff);
        else tr2_issue<ND, VB, 2 * ((V + 2) % PG)>(lb, hb, toff);
      }
    };
    pv(std::integral_constant<int, 0>{});
    pv(std::integral_constant<int, 1>{});
    pv(std::integral_constant<int, 2>{});
    pv(std::integral_constant<int, 3>{});
    if constexpr (NPV == 8) {
      pv(std::integral_constant<int, 4>{});
      pv(std::integral_constant<int, 5>{});
      pv(std::integral_constant<int, 6>{});
      pv(std::integral_constant<int, 7>{});
    }
    if constexpr (NEXT) {
      prep(t + 1, sn);
      // K t+2 / V t+1 landed (vmcnt counts LDS-DMA), and every wave's reads of the slots they
      // refill next iteration are done
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  };

  f32x16 sa[2], sb[2];
  if (t0 < ntiles) {
    dma_k(t0, 0);
    dma_v(t0, 0);
    if (t0 + 1 < ntiles) dma_k(t0 + 1, 1);
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    __syncthreads();
    if constexpr (CACHED) {
      // kv_start inside tile t0 (workgroup-uniform; absent when kv_start is null or a multiple of 64): the tile
      // came in whole, and its rows below kv_start are cache rows the caller promises nothing about. Their
      // scores are masked by index, but P = 0 times a NaN V row is NaN inside the P V MFMA, so those V rows
      // become zeros here (an image row is 2 D contiguous bytes: the swizzle permutes chunks within a row).
      // The barrier behind prep(t0) orders these stores before tile t0's transposed reads of V slot 0.
      const int zbytes = (kstart - t0 * KT) * 2 * D;
      for (int i = (int)threadIdx.x * 16; i < zbytes; i += 256 * 16)
        *reinterpret_cast<u32x4*>(smem + 2 * TILE + i) = u32x4(0u);
    }
    s_plain(std::integral_constant<int, 0>{}, sa);
    prep(t0, sa);
    __syncthreads();  // K slot 0 is refilled (tile t0 + 2) by the first iteration
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using NT = std::integral_constant<bool, true>;
    using NF = std::integral_constant<bool, false>;
    // tile t: K slot of tile t+1 = (t - t0 + 1) & 1, V slot of tile t = (t - t0) & 1. Pairs of
    // tiles with a successor in a plain loop, the last one or two after it (a loop with the last
    // tile's variant inside it spilled ~95 VGPRs)
    int t = t0;
    for (; t + 2 < ntiles; t += 2) {
      tile(I1{}, I0{}, NT{}, t, sa, sb);
      tile(I0{}, I1{}, NT{}, t + 1, sb, sa);
    }
    if (t + 1 < ntiles) {
      tile(I1{}, I0{}, NT{}, t, sa, sb);
      tile(I0{}, I1{}, NF{}, t + 1, sb, sa);
    } else {
      tile(I1{}, I0{}, NF{}, t, sa, sb);
    }
  }

  // O rows, widened stores (cdna_hip_programming.md T21): lanes l and l ^ 32 hold the two
  // 4-column halves of each 8-column group of the same row; one v_permlane32_swap per dword of a
  // pair of groups (k, k+1) leaves the lower half-wave with columns 8k..8k+7 and the upper with
  // 8k+8..8k+15, one 16-B store each instead of two 8-B stores. The swaps run on every lane (a
  // lane and its partner hold the same query row, so the row guard is uniform across the pair).
  {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    u16* Ob = O + ((VARLEN ? vl_row0 : (int64_t)b * Lq) + q) * ldo + (int64_t)h * D;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int rr = 0; rr < 4; rr += 2) {
        u16x4 wa, wb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wa[j] = f2bf(o[dt][rr * 4 + j] * inv);
          wb[j] = f2bf(o[dt][(rr + 1) * 4 + j] * inv);
        }
        u32x2 a = __builtin_bit_cast(u32x2, wa), bb = __builtin_bit_cast(u32x2, wb);
        unsigned ax = a[0], ay = a[1], bx = bb[0], by = bb[1];
        swap_halves(ax, bx);
        swap_halves(ay, by);
        if (q < Lq) {
          const u32x4 w4 = {ax, ay, bx, by};
          *reinterpret_cast<u32x4*>(Ob + dt * 32 + 8 * rr + 8 * hf) = w4;
        }
      }
    if ((!CACHED || LSE != nullptr) && q < Lq && hf == 0)  // the cached entry point's lse is optional
      LSE[((int64_t)b * H + h) * (VARLEN ? vl_max : Lq) + q] = l > 0.f ? (m + log2f(l)) * kLn2 : INFINITY;
  }
