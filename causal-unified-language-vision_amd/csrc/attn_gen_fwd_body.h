// The body of attn_generic.hip's forward kernels, included once per kernel (inside the function,
// after its `constexpr bool RAGGED` and `qpad`): attn_gen_fwd_k<T, D, CACHED> (RAGGED = false, qpad
// the constant 0) and attn_gen_fwd_ragged_k<T, D> (CACHED = RAGGED = true, Lk and qpad the
// sequence's own). Text, not a function, for the reason attn_fwd_pipe_body.h gives: the kernels that
// were there keep their code instruction for instruction (tools/isa_diff.py).
  constexpr int LD = D + 1;
  extern __shared__ float sm[];
  float* sQ = sm;
  float* sK = sQ + QF * LD;
  float* sV = sK + KB * LD;
  float* sP = sV + KB * LD;  // [QF][KB + 1]
  const int nqb = (int)cdiv(Lq, QF);
  const int qb = blockIdx.x % nqb, h = (blockIdx.x / nqb) % H, b = blockIdx.x / (nqb * H);
  const int q0 = qb * QF;
  const int t = threadIdx.x, r = t >> 2, part = t & 3;
  const int ks = kv_start ? kv_start[b] : 0;
  const int64_t qg = q0 + r;
  const int past = CACHED ? Lk - Lq : 0;
  const int64_t qpos = past + qg;  // the query's key position
  // sequence b's first K / V row: row b * Lk of the packed [B * Lk] rows, or of its own cache
  const T* Kb = K + (CACHED ? (int64_t)b * ldv : 0) + h * D;
  const T* Vb = V + (CACHED ? (int64_t)b * ldv : 0) + h * D;
  const int64_t krow0 = CACHED ? 0 : (int64_t)b * Lk;
  const int64_t ldvt = CACHED ? ldk : ldv;
  stage_rows<T>(sQ, LD, Q + h * D, ldq, (int64_t)b * Lq + q0, min(QF, Lq - q0), QF, D);
  float m = -INFINITY, l = 0.f;
  float o[D / 4];
#pragma unroll
  for (int c = 0; c < D / 4; ++c) o[c] = 0.f;
  const int kend = (RAGGED && q0 + QF <= qpad) ? 0 : causal ? min(Lk, past + q0 + QF) : Lk;
  for (int k0 = 0; k0 < kend; k0 += KB) {
    __syncthreads();
    stage_rows<T>(sK, LD, Kb, ldk, krow0 + k0, min(KB, Lk - k0), KB, D);
    if (CACHED)  // the cache rows below kv_start may hold anything (attn_generic.hip, stage_rows_from)
      stage_rows_from<T>(sV, LD, Vb, ldvt, krow0 + k0, ks - k0, min(KB, Lk - k0), KB, D);
    else
      stage_rows<T>(sV, LD, Vb, ldvt, krow0 + k0, min(KB, Lk - k0), KB, D);
    __syncthreads();
    float s[KB / 4];
    float bmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < KB / 4; ++i) {
      const int j = part + 4 * i;
      float acc = 0.f;
      for (int d = 0; d < D; ++d) acc = fmaf(sQ[r * LD + d], sK[j * LD + d], acc);
      s[i] = visible(qpos, k0 + j, Lk, ks, causal) && qg < Lq && (!RAGGED || qg >= qpad) ? acc * scale : -INFINITY;
      bmax = fmaxf(bmax, s[i]);
    }
    bmax = fmaxf(bmax, __shfl_xor(bmax, 1, 64));
    bmax = fmaxf(bmax, __shfl_xor(bmax, 2, 64));
    const float mnew = fmaxf(m, bmax);
    const float alpha = mnew == -INFINITY ? 1.f : __expf(m - mnew);
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < KB / 4; ++i) {
      const float p = s[i] == -INFINITY ? 0.f : __expf(s[i] - mnew);
      sP[r * (KB + 1) + part + 4 * i] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 1, 64);
    psum += __shfl_xor(psum, 2, 64);
    l = l * alpha + psum;
    m = mnew;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < D / 4; ++c) o[c] *= alpha;
    for (int j = 0; j < KB; ++j) {
      const float p = sP[r * (KB + 1) + j];
#pragma unroll
      for (int c = 0; c < D / 4; ++c) o[c] = fmaf(p, sV[j * LD + part + 4 * c], o[c]);
    }
  }
  if (qg < Lq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* op = O + ((int64_t)b * Lq + qg) * ldo + h * D;
#pragma unroll
    for (int c = 0; c < D / 4; ++c) Elt<T>::st(op, part + 4 * c, o[c] * inv);
    if ((!CACHED || LSE != nullptr) && part == 0)
      LSE[((int64_t)b * H + h) * Lq + qg] = l > 0.f ? m + __logf(l) : INFINITY;
  }
