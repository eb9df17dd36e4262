// The body of attention.hip's 8-wave dK/dV kernels, included once per kernel (inside the function):
// attn_bwd_dkdv8_k<D, CAUSAL, DS_OUT> (SEQ = const int32_t*: the uniform [B, L] grid, kv_start the
// pointer of that name, LqG / LkG its rows per sequence) and attn_bwd_dkdv8_varlen_k<D, DS_OUT> (SEQ =
// VarSeq: kv_start is the packed sequences' description, LqG = LkG = its max_len, CAUSAL = true). Text
// for the reason attn_fwd_pipe_body.h is: attn_bwd_dkdv8_k has to stay the code it was, instruction for
// instruction (tools/isa_diff.py; tests/test_isa_lds_reads.py reads its counted waits).
  constexpr int QT = 64, KB = 128;
  constexpr int TQ = QT * D * 2;          // bytes of a Q (or dO) tile
  constexpr int TK = KB * D * 2;          // bytes of the K (or V) image
  constexpr int NS = D / 16;
  constexpr int ND = D / 32;
  constexpr int BUF = 2 * TQ + 2 * QT * 4;  // [Q | dO | lse(64) | delta(64)]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + TK;
  char* bufs = smem + 2 * TK;

  const int nkb = (seq_grid_rows(kv_start, LkG) + KB - 1) / KB;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int kb = lid % nkb, hb = lid / nkb;
  const int h = hb % H, b = hb / H;
  // wave index through readfirstlane: wave-uniform to the compiler (scalar slice / half branches
  // and row bases)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hf = lane >> 5;
  const int ksl = wave & 3, u = wave >> 2;          // 32-key slice, query half of each tile
  const int key = kb * KB + ksl * 32 + (lane & 31);  // this lane's key
  const int kstart = seq_kstart(kv_start, b);
  const int Lq = seq_rows(kv_start, b, LqG), Lk = seq_rows(kv_start, b, LkG);  // this sequence's rows
  if constexpr (kVarlen<SEQ>) if (kb * 128 >= Lk) return;  // a tile past the sequence's end (workgroup-uniform)
  // live queries of this key: [qlo, qlim) (empty for keys before kstart or past Lk)
  const int qlo = CAUSAL ? key : 0;
  const int qlim = (key < kstart || key >= Lk) ? qlo : Lq;
  const unsigned qspan = (unsigned)max(qlim - qlo, 0);

  const u16* Qb = Q + seq_row0(kv_start, b, LqG) * ldq + (int64_t)h * D;
  const u16* dOb = dO + seq_row0(kv_start, b, LqG) * lddo + (int64_t)h * D;
  const u16* Kb = K + seq_row0(kv_start, b, LkG) * ldk + (int64_t)h * D;
  const u16* Vb = V + seq_row0(kv_start, b, LkG) * ldv + (int64_t)h * D;
  const float* lseb = LSE + ((int64_t)b * H + h) * seq_grid_rows(kv_start, LqG);
  const float* delb = DELTA + ((int64_t)b * H + h) * seq_grid_rows(kv_start, LqG);

  f32x16 dk[ND], dv[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) { dk[i] = f32x16(0.f); dv[i] = f32x16(0.f); }
  const float c = scale * kLog2e;
  const int kmin = kb * KB;
  const int qt0 = CAUSAL ? (kmin / QT) : 0;
  const int nqt = (Lq + QT - 1) / QT;
  const bool block_live = kmin < Lk && (kmin + KB > kstart);

  // Q / dO tiles by LDS-DMA into the swizzled image (as the forward's StageDMA)
  StageDMA<QT, D, 8> dq_, ddo_;
  dq_.prep(ldq, wave, lane);
  ddo_.prep(lddo, wave, lane);
  // per-lane LDS byte offsets of the asm fragment reads (rows relative to a 32-row slice / a
  // 16-key slice: the image swizzle depends on row & 15 only)
  unsigned roff_b[NS], toff_b[ND][2];
  {
#pragma unroll
    for (int s = 0; s < NS; ++s) roff_b[s] = kv_off<D>(lane & 31, 2 * s + (lane >> 5));
    const int i = lane & 15, qq = i >> 2, pp = i & 3;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const int ch = ((dt * 32 + 16 * ((lane >> 4) & 1)) >> 3) + (pp >> 1);
      toff_b[dt][0] = kv_off<D>(4 * hf + qq, ch) + 8 * (pp & 1);
      toff_b[dt][1] = kv_off<D>(4 * hf + qq + 8, ch) + 8 * (pp & 1);
    }
  }
  float aux = 0.f;
  // the next tile's lse / delta: loaded raw and first used when staged after the tile's compute
  // (the lse * log2 e at load time made the compiler wait for the load -- and for the in-flight
  // Q / dO prefetch -- at the top of every tile)
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
      ((float*)(buf + 2 * TQ))[threadIdx.x] =
          threadIdx.x < QT ? (aux_in ? aux * kLog2e : INFINITY) : (aux_in ? aux : 0.f);
  };
  if (block_live) {
    StageN<KB, D, 512> skv;
    skv.load(Kb, ldk, kmin, Lk);
    skv.store(sK);
    skv.load(Vb, ldv, kmin, Lk);
    skv.store(sV);
    if (qt0 < nqt) {
      dq_.issue(Qb, ldq, qt0 * QT, Lq, bufs, wave);
      ddo_.issue(dOb, lddo, qt0 * QT, Lq, bufs + TQ, wave);
      load_aux(qt0);
      store_aux(bufs);
    }
  }
  __builtin_amdgcn_s_waitcnt(kVmcnt0);  // see attn_fwd_k: keeps hipcc from waiting on the prefetch
  __syncthreads();

  for (int qt = qt0; block_live && qt < nqt; ++qt) {
    const int cur = (qt - qt0) & 1;
    char* buf = bufs + cur * BUF;
    char* nbuf = bufs + (cur ^ 1) * BUF;
    const bool more = qt + 1 < nqt;
    if (more) {
      dq_.issue(Qb, ldq, (qt + 1) * QT, Lq, nbuf, wave);  // nbuf was last read before the previous barrier
      ddo_.issue(dOb, lddo, (qt + 1) * QT, Lq, nbuf + TQ, wave);
      load_aux(qt + 1);
    }
    const float* slse = (const float*)(buf + 2 * TQ);
    const float* sdel = slse + QT;
    // S[q][key], dP[q][key] for this wave's 32 query rows of the tile
    f32x16 sacc = f32x16(0.f), pacc = f32x16(0.f);
    {
      // inline-asm fragment reads (a compiler-visible LDS read may alias the next tile's in-flight
      // LDS-DMA, so hipcc would wait vmcnt(0) in front of it), one k-step ahead of the MFMAs: the
      // four reads of step s + 1 are in flight while step s's two MFMAs issue
      const unsigned aq = lds_addr(buf) + 2u * D * 32u * u, ak = lds_addr(sK) + 2u * D * 32u * ksl;
      s16x8 q0, k0, d0, v0, q1, k1, d1, v1;
      __builtin_amdgcn_sched_barrier(0);
      rd4(q0, k0, d0, v0, aq + roff_b[0], ak + roff_b[0], aq + TQ + roff_b[0], ak + TK + roff_b[0]);
#pragma unroll
      for (int st = 0; st < NS; st += 2) {
        rd4(q1, k1, d1, v1, aq + roff_b[st + 1], ak + roff_b[st + 1], aq + TQ + roff_b[st + 1], ak + TK + roff_b[st + 1]);
        tie4<4>(q0, k0, d0, v0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag8, q0), __builtin_bit_cast(frag8, k0), sacc, 0, 0, 0);
        pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag8, d0), __builtin_bit_cast(frag8, v0), pacc, 0, 0, 0);
        if (st + 2 < NS) {
          rd4(q0, k0, d0, v0, aq + roff_b[st + 2], ak + roff_b[st + 2], aq + TQ + roff_b[st + 2], ak + TK + roff_b[st + 2]);
          tie4<4>(q1, k1, d1, v1);
        } else {
          tie4<0>(q1, k1, d1, v1);
        }
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag8, q1), __builtin_bit_cast(frag8, k1), sacc, 0, 0, 0);
        pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag8, d1), __builtin_bit_cast(frag8, v1), pacc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // query qq is live for this lane's key iff qlo <= qq < qlim: one unsigned compare per element
    const int qoff = qt * QT + 32 * u + 4 * hf - qlo;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(slse + 32 * u + 8 * rr + 4 * hf);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(sdel + 32 * u + 8 * rr + 4 * hf);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rr * 4 + j;
        float pv = fast_exp2(fmaf(sacc[r], c, -l4[j]));  // lse staged as lse * log2(e)
        if ((unsigned)(qoff + 8 * rr + j) >= qspan) pv = 0.f;
        sacc[r] = pv;
        pacc[r] = pv * (pacc[r] - d4[j]);
      }
    }
    // dV += P^T dO ; dK += dS^T Q over this wave's 32 query rows
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const frag8 pf = pack_frag(sacc, s);
      const frag8 df = pack_frag(pacc, s);
      if (DS_OUT) {
        // dS^T[key][q] (the bf16 operand of dK) for the dQ kernel: registers 8s..8s+3 / 8s+4..8s+7
        // are query rows 16s + 4hf + 0..3 / 16s + 8 + 4hf + 0..3 of this wave's 32
        const u16x8 w = __builtin_bit_cast(u16x8, df);
        // (128-query block (qt QT) / 128 at st_blk)
        u16* row = dST + ((int64_t)b * H + h) * st_bh + (int64_t)((qt * QT) >> 7) * st_blk + (int64_t)key * ldst +
                   ((qt * QT) & 127) + 32 * u + 16 * s + 4 * hf;
        *reinterpret_cast<u16x4*>(row) = u16x4{w[0], w[1], w[2], w[3]};
        *reinterpret_cast<u16x4*>(row + 8) = u16x4{w[4], w[5], w[6], w[7]};
      }
      {
        // transposed dO / Q fragments by inline asm, one column block ahead of the MFMAs
        const unsigned kb = lds_addr(buf) + 2u * D * (32u * u + 16u * s);
        s16x4 dl0, dh0, ql0, qh0, dl1, dh1, ql1, qh1;
        __builtin_amdgcn_sched_barrier(0);
        rd4t(dl0, dh0, ql0, qh0, kb + TQ + toff_b[0][0], kb + TQ + toff_b[0][1], kb + toff_b[0][0], kb + toff_b[0][1]);
#pragma unroll
        for (int dt = 0; dt < ND; dt += 2) {
          rd4t(dl1, dh1, ql1, qh1, kb + TQ + toff_b[dt + 1][0], kb + TQ + toff_b[dt + 1][1], kb + toff_b[dt + 1][0],
               kb + toff_b[dt + 1][1]);
          tie4t<4>(dl0, dh0, ql0, qh0);
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, tr_join(dl0, dh0), dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, tr_join(ql0, qh0), dk[dt], 0, 0, 0);
          if (dt + 2 < ND) {
            rd4t(dl0, dh0, ql0, qh0, kb + TQ + toff_b[dt + 2][0], kb + TQ + toff_b[dt + 2][1], kb + toff_b[dt + 2][0],
                 kb + toff_b[dt + 2][1]);
            tie4t<4>(dl1, dh1, ql1, qh1);
          } else {
            tie4t<0>(dl1, dh1, ql1, qh1);
          }
          dv[dt + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, tr_join(dl1, dh1), dv[dt + 1], 0, 0, 0);
          dk[dt + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, tr_join(ql1, qh1), dk[dt + 1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (more) store_aux(nbuf);
    // the next tile's DMA landed (MFMAs kept in front of the wait)
    __builtin_amdgcn_sched_barrier(0);
    // DS_OUT: the tile's four dS^T stores (two 8-B stores per 16-query slice, after the DMA in
    // issue order) may stay in flight
    if constexpr (DS_OUT) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // pair reduction: half 1 parks its partial sums in LDS, half 0 adds them and stores
  float* red = (float*)smem;  // [2 (dk, dv)][4 slices][ND][16][64] f32
  auto slot = [&](int which, int dt, int r) { return red + ((((which * 4 + ksl) * ND + dt) * 16 + r) * 64 + lane); };
  __syncthreads();
  if (u == 1) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { *slot(0, dt, r) = dk[dt][r]; *slot(1, dt, r) = dv[dt][r]; }
  }
  __syncthreads();
  if (u == 0) {
    // wave-uniform row base (scalar), one 32-bit lane offset (4 hf rows + column lane & 31);
    // row r's offset acc_row(r, 0) * ld is scalar too, the column block dt * 32 an immediate:
    // one saddr store per element instead of 64-bit address arithmetic per element
    const int k0 = kb * KB + ksl * 32;
    u16* dKr = dK + (seq_row0(kv_start, b, LkG) + k0) * lddk + (int64_t)h * D;
    u16* dVr = dV + (seq_row0(kv_start, b, LkG) + k0) * lddv + (int64_t)h * D;
    const unsigned lk = (unsigned)(4 * hf * lddk + (lane & 31)) * 2u, lv = (unsigned)(4 * hf * lddv + (lane & 31)) * 2u;
    const int left = Lk - k0;  // rows of this slice that exist (>= 32 on all but the last block)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (acc_row(r, hf) < left) {
        u16* pk = dKr + (int64_t)acc_row(r, 0) * lddk;
        u16* pv = dVr + (int64_t)acc_row(r, 0) * lddv;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          *(u16*)((char*)pk + (lk + dt * 64u)) = f2bf((dk[dt][r] + *slot(0, dt, r)) * scale);
          *(u16*)((char*)pv + (lv + dt * 64u)) = f2bf(dv[dt][r] + *slot(1, dt, r));
        }
      }
    }
  }
