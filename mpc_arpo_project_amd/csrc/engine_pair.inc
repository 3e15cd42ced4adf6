// engine_pair.inc -- the two-wave variant of the QP kernel (included by engine.hip inside its
// anonymous namespace, after qp_batch_kernel; it uses that file's device helpers).
//
// One QP instance per 128-thread workgroup: two waves share the instance image in LDS (the same
// image as the one-wave kernel, plus the exchange slots Plan::XCH / XID).  Why (DESIGN.md, Two
// waves per instance): one wave per instance leaves an instance's work a single latency chain; at
// N = 40 the 74 KB image fits two instances per CU, so two of the four SIMDs idle, and at N = 20 the
// LDS caps the CU at four instances = four waves.  With two waves per instance the CU runs twice the
// waves on the same LDS, and every phase but the factorization is split between them:
//   * register state: wave w owns the n-vector slots [w RNH, (w + 1) RNH) and the m-vector slots
//     [w RMH, (w + 1) RMH) of the one-wave kernel's layout (element i on lane i % 64, slot i / 64);
//     every elementwise pass, mat-vec output and Ruiz norm is computed by the owner of its element;
//   * solve steps: the plan is laid out for two waves (Plan::waves == 2: symbolic.cpp packs every
//     target of a step into one half of the segment positions), wave 0 executes positions 0 + 1 of
//     each lane (a pair: one atomic), wave 1 positions 2 and 3; one LDS barrier per step, so every
//     target is summed by one wave in a fixed order (deterministic, like the one-wave kernel);
//   * reductions (norms, certificates, cost scaling, objective): per wave as in the one-wave
//     kernel, then combined through the exchange slots as (wave 0) op (wave 1) -- both waves read
//     the same two values, so every decision (termination, rho update) is identical in both and
//     every barrier is reached by both;
//   * factorization: the elimination chain's steps run on wave 0 (its steps are one 64-lane pass
//     each and latency-bound: splitting them would add a barrier per step and save nothing); wave 1
//     meets it at the barriers around it.
// Barriers are s_waitcnt lgkmcnt(0) + s_barrier: only LDS is shared between the two waves (each
// wave reads back only the global memory it wrote), so the step records' buffer loads stay in
// flight across them.
//
// What this file holds is what only the two-wave kernel has: the half-record solve steps, the
// owner-split factorization, Ruiz passes and MV copy (assemble_and_factor2, scale_problem2,
// scale_finish2), the ADMM loop (solve_instance2) and the kernel.  The wave context Wv with its
// barrier and exchange, and the check path -- ell_load / ell_apply / ell_mv / load_idx /
// ell_absmax_r, compute_residuals, check_termination with both certificates, rho_estimate,
// scale_bounds, store_solution -- are engine.hip's, written once over a wave context and called
// here with Wv (there with One).

// ---- solve steps of one wave: its half of the step record (segments 0 + 1 for wave 0, 2 + 3 for
// wave 1) and its two targets
struct HalfRec {
  uint32_t a[4], b[4];
  uint32_t t0, t1;
};
struct HalfOps {
  typedef HalfRec Rec;
  static constexpr int STRIDE = SOLVE_STEP_WORDS;
  double* v;
  int w;       // wave: record half
  bool fuse;   // segments 0 + 1 are a pair (paired plan, wave 0): one atomic
#ifdef MPCQP_PAIR_CHECKS
  int xid;  // the checked barrier's counters (BAR2_X)
#endif
  __device__ __forceinline__ void load(Rsrc rs, int soff, uint32_t lane, Rec& r) const {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const auto x = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(lane * 16u) + (2 * w + q) * 1024, soff, 0);
      r.a[2 * q] = x[0], r.b[2 * q] = x[1], r.a[2 * q + 1] = x[2], r.b[2 * q + 1] = x[3];
    }
    const auto tg = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(lane * 16u) + 4 * SOLVE_TERM_WORDS + 8 * w, soff, 0);
    r.t0 = tg[0], r.t1 = tg[1];
  }
  __device__ __forceinline__ void step(const Rec& r, int) const {
    double x[4], y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = lds_ld(v, r.a[c]), y[c] = lds_ld(v, r.b[c]);
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
    const double n0 = fma(-x[1], y[1], -(x[0] * y[0]));
    const double n1 = fma(-x[3], y[3], -(x[2] * y[2]));
    if (fuse) {
      lds_add(r.t0, n0 + n1);
    } else {
      lds_add(r.t0, n0);
      lds_add(r.t1, n1);
    }
    LDS_FENCE();
  }
};
// the same with the matrix operands of the next step read during this one (Plan::mat_first; the
// one-wave kernel's solve_step_pf)
__device__ __forceinline__ void half_step_pf(const HalfOps& ops, const HalfRec& r, const HalfRec& nx,
                                             double (&m)[4]) {
  double y[4], mn[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) y[c] = lds_ld(ops.v, r.b[c]);
#pragma unroll
  for (int c = 0; c < 4; ++c) mn[c] = lds_ld(ops.v, nx.a[c]);
  __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
  __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
  const double n0 = fma(-m[1], y[1], -(m[0] * y[0]));
  const double n1 = fma(-m[3], y[3], -(m[2] * y[2]));
  if (ops.fuse) {
    lds_add(r.t0, n0 + n1);
  } else {
    lds_add(r.t0, n0);
    lds_add(r.t1, n1);
  }
  LDS_FENCE();
#pragma unroll
  for (int c = 0; c < 4; ++c) m[c] = mn[c];
}
__device__ __forceinline__ int half_off(int /*n*/, int s) {  // padded table; uniform (step_off)
  return __builtin_amdgcn_readfirstlane(s * (SOLVE_STEP_WORDS * 4));
}
struct HalfPipe {
  HalfRec a, b, c;
};
__device__ __forceinline__ void half_prefetch(const HalfOps& ops, Rsrc rs, int n, uint32_t lane, HalfPipe& p) {
  __builtin_amdgcn_sched_barrier(0);
  ops.load(rs, half_off(n, 0), lane, p.a);
  __builtin_amdgcn_sched_barrier(0);
  ops.load(rs, half_off(n, 1), lane, p.b);
  __builtin_amdgcn_sched_barrier(0);
  ops.load(rs, half_off(n, 2), lane, p.c);
  __builtin_amdgcn_sched_barrier(0);
}
// the step loop of run_body with the barrier of the two waves after every step
#define MPCQP_HSTEP(X)                                      \
  ops.step(p.X, s);                                         \
  BAR2_X(ops.v, ops.xid);                                   \
  if (++s >= n) break;                                      \
  __builtin_amdgcn_sched_barrier(0);                        \
  ops.load(rs, half_off(n, s + 2), lane, p.X);              \
  __builtin_amdgcn_sched_barrier(0);
__device__ __forceinline__ void half_body(const HalfOps& ops, Rsrc rs, int n, uint32_t lane, HalfPipe& p) {
  int s = 0;
  for (;;) {
    MPCQP_HSTEP(a) MPCQP_HSTEP(b) MPCQP_HSTEP(c)
    MPCQP_HSTEP(a) MPCQP_HSTEP(b) MPCQP_HSTEP(c)
    MPCQP_HSTEP(a) MPCQP_HSTEP(b) MPCQP_HSTEP(c)
    MPCQP_HSTEP(a) MPCQP_HSTEP(b) MPCQP_HSTEP(c)
  }
}
#undef MPCQP_HSTEP
#define MPCQP_HPFSTEP(X, Y)                                 \
  half_step_pf(ops, p.X, p.Y, m);                           \
  BAR2_X(ops.v, ops.xid);                                   \
  if (++s >= n) break;                                      \
  __builtin_amdgcn_sched_barrier(0);                        \
  ops.load(rs, half_off(n, s + 2), lane, p.X);              \
  __builtin_amdgcn_sched_barrier(0);
__device__ __forceinline__ void half_body_pf(const HalfOps& ops, Rsrc rs, int n, uint32_t lane, HalfPipe& p) {
  double m[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) m[c] = lds_ld(ops.v, p.a.a[c]);
  int s = 0;
  for (;;) {
    MPCQP_HPFSTEP(a, b) MPCQP_HPFSTEP(b, c) MPCQP_HPFSTEP(c, a)
    MPCQP_HPFSTEP(a, b) MPCQP_HPFSTEP(b, c) MPCQP_HPFSTEP(c, a)
    MPCQP_HPFSTEP(a, b) MPCQP_HPFSTEP(b, c) MPCQP_HPFSTEP(c, a)
    MPCQP_HPFSTEP(a, b) MPCQP_HPFSTEP(b, c) MPCQP_HPFSTEP(c, a)
  }
}
#undef MPCQP_HPFSTEP

// ---- per-wave instance state: the owned slots of Inst
template <int RNH, int RMH>
using Inst2 = Inst<RNH, RMH>;
template <int RNH, int RMH>
using Resid2 = Resid<RNH, RMH>;

// KKT (re)assembly and factorization by both waves (the elimination chain on wave 0)
template <int RNH, int RMH>
__device__ __forceinline__ void assemble_and_factor2(const KParams& p, double* v, const Wv& W,
                                                     const Inst2<RNH, RMH>& S, double sigma) {
  const DevPlan& P = p.pl;
  const int tid = W.lane + 64 * W.w;
  for (int k = tid; k < P.nnzL; k += 128) v[P.LX + k] = 0.0;
  for (int k = tid; k < 64 * P.NKS; k += 128) v[P.DINV + k] = 0.0;
  if (tid < ZERO_BLOCK) v[P.ZERO + tid] = 0.0;
  if (tid == 0) {
    v[P.ONE] = 1.0;
    v[P.MONE] = -1.0;
  }
  BAR2_X(v, p.pl.XID);
  for (int j = tid; j < P.n; j += 128) v[P.slotSig[j]] = sigma;
  BAR2_X(v, p.pl.XID);
  for (int k = tid; k < P.nnzP; k += 128) {
    const double val = v[P.MV + k];
    v[P.slotP[k]] = (P.Pi[k] == P.Pcol[k]) ? val + sigma : val;
  }
  for (int k = tid; k < P.nnzA; k += 128) v[P.slotA[k]] = v[P.MV + P.nnzP + k];
#pragma unroll
  for (int r = 0; r < RMH; ++r) {
    const int i = W.lane + 64 * (r + W.zo);
    if (i < P.m) v[P.slotRho[i]] = -rinv_of(S, r);
  }
  BAR2_X(v, p.pl.XID);
  if (W.w == 0) run_fac<PAIR_PIPE>(P.fac, P.nfac, v, W.lane);
  BAR2_X(v, p.pl.XID);
  for (int k = tid; k < P.nnzL; k += 128) v[P.LX + k] *= v[P.Lcol[k]];
  BAR2_X(v, p.pl.XID);
  if (P.ntail > 0) {
    if (W.w == 0) run_fac<PAIR_PIPE>(P.tail, P.ntail, v, W.lane);
    BAR2_X(v, p.pl.XID);
  }
}

// Ruiz equilibration (scale_problem of the one-wave kernel), owner-split
template <int RNH, int RMH>
__device__ __forceinline__ void scale_problem2(const KParams& p, int inst, const DriftSel& dr, Inst2<RNH, RMH>& S,
                                               double* v, Wv& W, double (&D)[RNH], double (&E)[RMH]) {
  const DevPlan& P = p.pl;
  const int n = P.n, m = P.m, lane = W.lane, tid = lane + 64 * W.w;
  // OSQP's drifted P / q (drift_of, scale_problem of the one-wave kernel)
  const double* P_in = dr.in_b < 0 ? setup_row(p.Px, p.Px_stride, inst) : drift_row(p.Pw, dr.in_b, p.B, P.nnzP, inst);
  const double* q_in = dr.in_b < 0 ? setup_row(p.q, p.q_stride, inst) : drift_row(p.qw, dr.in_b, p.B, n, inst);
  const double* Ax_in = p.Ax + (size_t)inst * P.nnzA;
  const double* l_in = p.l + (size_t)inst * m;
  const double* u_in = p.u + (size_t)inst * m;
  EllIdx<RNH, ELL_KP> iP;
  EllIdx<RNH, ELL_KAT> iAt;
  EllIdx<RMH, ELL_KA> iA;
  load_idx(P.eP, iP, lane, W.xo);
  load_idx(P.eAt, iAt, lane, W.xo);
  load_idx(P.eA, iA, lane, W.zo);
  // this wave's half of the value overlay's rescale operand slots: value slots j in
  // [w 2 JWH, (w + 1) 2 JWH) (value k = 64 j + lane), u16 pairs
  constexpr int JWH = 2 * RNH * 2;  // = 4 RN / 2: the one-wave kernel's JW split in two
  uint32_t ra[JWH], ca[JWH];
  {
    const int j0 = W.w * 2 * JWH;  // first value slot of this wave
#pragma unroll
    for (int q = 0; q < JWH / 2; ++q) {
      ra[2 * q] = ra[2 * q + 1] = ca[2 * q] = ca[2 * q + 1] = 0u;
      const int jg = j0 + 4 * q;  // four u16 slots per 8-byte load
      if (jg < P.SJ) {            // wave-uniform
        const uint2 a = *reinterpret_cast<const uint2*>(P.sra + (size_t)lane * P.SJ + jg);
        const uint2 c = *reinterpret_cast<const uint2*>(P.sca + (size_t)lane * P.SJ + jg);
        ra[2 * q] = a.x, ra[2 * q + 1] = a.y, ca[2 * q] = c.x, ca[2 * q + 1] = c.y;
      }
    }
  }
  if (tid == 0) v[P.S_ZERO] = 0.0;
  {
    const int cnt = P.nnzP + P.nnzA;
    for (int k = tid; k < cnt; k += 128) v[P.S_P + k] = k < P.nnzP ? P_in[k] : Ax_in[k - P.nnzP];
  }
#pragma unroll
  for (int r = 0; r < RNH; ++r) {
    const int j = lane + 64 * (r + W.xo);
    S.q[r] = j < n ? q_in[j] : 0.0;
    D[r] = 1.0;
  }
#pragma unroll
  for (int r = 0; r < RMH; ++r) {
    const int i = lane + 64 * (r + W.zo);
    S.l[r] = i < m ? dmaxd(l_in[i], -OSQP_INFTY) : 0.0;
    S.u[r] = i < m ? dmind(u_in[i], OSQP_INFTY) : 0.0;
    E[r] = 1.0;
  }
  S.c = 1.0;
  double cprev = 1.0;
  double dpc[RNH];
  BAR2_X(v, p.pl.XID);
  const int scaling = uniform_i(set_row(p, inst)->scaling);
  for (int it = 0; it < scaling; ++it) {
    double dp[RNH], da[RNH], er[RMH], dt[RNH], et[RMH];
    if (it == 0) {
      ell_absmax_r<false>(P.eP, iP, 0u, v, dp, W, W.xo);
    } else {
#pragma unroll
      for (int r = 0; r < RNH; ++r) dp[r] = cprev * dpc[r];
    }
    ell_absmax_r<false>(P.eAt, iAt, 0u, v, da, W, W.xo);
    ell_absmax_r<false>(P.eA, iA, 0u, v, er, W, W.zo);
#pragma unroll
    for (int r = 0; r < RNH; ++r) {
      const int j = lane + 64 * (r + W.xo);
      const double d = j < n ? dmaxd(dp[r], da[r]) : 0.0;
      dt[r] = 1. / sqrt(limit_scaling(d));
      if (j < n) v[P.S_DT + j] = dt[r];
    }
#pragma unroll
    for (int r = 0; r < RMH; ++r) {
      const int i = lane + 64 * (r + W.zo);
      const double e = i < m ? er[r] : 0.0;
      et[r] = 1. / sqrt(limit_scaling(e));
      if (i < m) v[P.S_ET + i] = et[r];
    }
    BAR2_X(v, p.pl.XID);  // every column / row factor written before any value is rescaled
    {
      // values k = 64 (j0 + jl) + lane, jl < 2 JWH: this wave's share of scale_pa_r
      const int cnt = P.nnzP + P.nnzA, j0 = W.w * 2 * JWH;
      constexpr int U = 8;
#pragma unroll
      for (int jb = 0; jb < 2 * JWH; jb += U) {
        if (64 * (j0 + jb) >= cnt) break;  // wave-uniform
        double x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jl = jb + u, k = 64 * (j0 + jl) + lane, kc = k < cnt ? k : 0;
          const double f = k < P.nnzP ? cprev : 1.0;
          const uint32_t a = (jl & 1) ? (ra[jl / 2] >> 16) : (ra[jl / 2] & 0xffffu);
          const uint32_t b = (jl & 1) ? (ca[jl / 2] >> 16) : (ca[jl / 2] & 0xffffu);
          x[u] = ((v[P.S_P + kc] * f) * v[a]) * v[b];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = 64 * (j0 + jb + u) + lane;
          if (k < cnt) v[P.S_P + k] = x[u];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RNH; ++r) {
      S.q[r] = dt[r] * S.q[r];
      D[r] = D[r] * dt[r];
    }
#pragma unroll
    for (int r = 0; r < RMH; ++r) E[r] = E[r] * et[r];
    BAR2_X(v, p.pl.XID);  // the rescaled values before the cost normalisation's column norms (and the next
             // pass's factors are not written before every value of this pass is rescaled)
    ell_absmax_r<false>(P.eP, iP, 0u, v, dpc, W, W.xo);
    // vec_mean of the column norms in index order: both waves stage their columns in the D_temp
    // slots (consumed by the rescale above), the exchange's barrier publishes them
    double qmax = 0.0, csum = 0.0;
#pragma unroll
    for (int r = 0; r < RNH; ++r) {
      const int j = lane + 64 * (r + W.xo);
      if (j < n) {
        v[P.S_DT + j] = dpc[r];
        csum = csum + dpc[r];
        qmax = dmaxd(qmax, fabs(S.q[r]));
      }
    }
    const double mine[2] = {wave_sum(csum), wave_max(qmax)};
    const bool ks[2] = {true, false};
    double both[2];
    W.all<2>(p, v, mine, ks, both);  // its barrier publishes both waves' staged norms
    const double inq = limit_scaling(both[1]), T = both[0];
    double c_temp = inq;  // the mean matters only above |q|_inf (scale_problem)
    if (!((T + sum_slack(T, n)) / n < inq)) {
      c_temp = seq_sum(v + P.S_DT, n) / n;
      BAR2_X(v, p.pl.XID);  // both waves' reads before the next pass writes its factors there
    }
    c_temp = limit_scaling(dmaxd(c_temp, inq));
    c_temp = 1. / c_temp;
    cprev = c_temp;
#pragma unroll
    for (int r = 0; r < RNH; ++r) S.q[r] = S.q[r] * c_temp;
    S.c = S.c * c_temp;
  }
  for (int k = tid; k < P.nnzP; k += 128) v[P.S_P + k] = v[P.S_P + k] * cprev;
  // the next solve's unscaled data (scale_problem): D^-1 of this wave's columns in the D_temp slots
  double* const Pw = drift_row(p.Pw, dr.out_b, p.B, P.nnzP, inst);
  double* const qw = drift_row(p.qw, dr.out_b, p.B, n, inst);
  const double cinv = 1. / S.c;
#pragma unroll
  for (int r = 0; r < RNH; ++r) {
    const int j = lane + 64 * (r + W.xo);
    const double di = 1. / D[r];
    if (j < n) {
      v[P.S_DT + j] = di;
      qw[j] = (S.q[r] * cinv) * di;
    }
  }
  BAR2_X(v, p.pl.XID);  // every D^-1 and every final P value before the unscale
  {
    const int j0 = W.w * 2 * JWH;
#pragma unroll
    for (int jl = 0; jl < 2 * JWH; ++jl) {
      if (64 * (j0 + jl) >= P.nnzP) break;  // wave-uniform
      const int k = 64 * (j0 + jl) + lane;
      const uint32_t a = (jl & 1) ? (ra[jl / 2] >> 16) : (ra[jl / 2] & 0xffffu);
      const uint32_t b = (jl & 1) ? (ca[jl / 2] >> 16) : (ca[jl / 2] & 0xffffu);
      if (k < P.nnzP) Pw[k] = ((v[P.S_P + k] * cinv) * v[a]) * v[b];
    }
  }
}

template <int RNH, int RMH>
__device__ __forceinline__ void scale_finish2(const KParams& p, int inst, bool rebound, Inst2<RNH, RMH>& S,
                                              const Slab& sb, double* v, const Wv& W,
                                              const double (&D)[RNH], const double (&E)[RMH]) {
  const DevPlan& P = p.pl;
  const int tid = W.tid();
  scale_bounds(p, inst, rebound, S, sb, W, D, E);
  const int cnt = P.nnzP + P.nnzA;
  for (int k = tid; k < cnt; k += 128) v[P.MV + k] = v[P.S_P + k];
  if (tid == 0) v[P.MVZ] = 0.0;
  BAR2_X(v, p.pl.XID);
}

// MODE: 0 the solve steps split between the waves (Plan::split_steps), 1 the same with the matrix
// operands read one step ahead (Plan::mat_first), 2 every solve step on wave 0 with the one-wave
// kernel's full step records and step loop while wave 1 waits (a plan without the split packing):
// no barrier inside the solves, the other phases still split
template <int RNH, int RMH, bool PAIRED, int MODE>
__device__ __forceinline__ void solve_instance2(const KParams& p, int inst, double* v, double* scr, Wv& W) {
  const DevPlan& P = p.pl;
  const int n = P.n, m = P.m, lane = W.lane;
  const Slab sb = slab_of(P, scr);
  Inst2<RNH, RMH> S;
  const int hs = p.has_state[inst];
  const DriftSel dr = drift_sel(p, inst);
#ifdef MPCQP_TIMING
  unsigned long long tacc[T_NSLOT] = {};
#endif
  T_BEGIN(t_sc);
  {
    double D[RNH], E[RMH];
    scale_problem2<RNH, RMH>(p, inst, dr, S, v, W, D, E);
    scale_finish2<RNH, RMH>(p, inst, dr.rebound, S, sb, v, W, D, E);
    // the drift state after this solve, stored once the scaling has read it (kept to the end of
    // the solve it was an SGPR live across the ADMM loop; the two-wave kernel's other wave has
    // read it before the scaling's barriers)
    if (W.w == 0 && lane == 0) {
      p.dsel[inst] = dr.sel;
      p.pend[inst] = 0;
    }
  }
  T_END(T_SCALE, t_sc);
  const SetRow sr = set_row(p, inst);  // the instance's own settings (KParams::srows)
  S.rho = (hs != 0) ? p.rho_state[inst] : sr->rho;
  set_rho(S);
  T_BEGIN(t_f0);
  assemble_and_factor2<RNH, RMH>(p, v, W, S, sr->sigma);
  T_END(T_FACTOR, t_f0);
  T_COUNT(T_NFACT);

  // ---------------- warm start (own slots)
  const bool warm = uniform_i(sr->warm_start) && hs != 0;
  if (warm && hs == 1) {
#pragma unroll
    for (int r = 0; r < RNH; ++r) {
      const int j = lane + 64 * (r + W.xo);
      S.x[r] = j < n ? p.xs[(size_t)inst * n + j] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < RMH; ++r) {
      const int i = lane + 64 * (r + W.zo);
      S.z[r] = i < m ? p.zs[(size_t)inst * m + i] : 0.0;
      S.y[r] = i < m ? p.ys[(size_t)inst * m + i] : 0.0;
    }
  } else if (warm && hs == 2) {  // osqp_warm_start: scale the user guess, z = A x
#pragma unroll
    for (int r = 0; r < RNH; ++r) {
      const int j = lane + 64 * (r + W.xo);
      S.x[r] = j < n ? S.Dinv[r] * p.xs[(size_t)inst * n + j] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < RMH; ++r) {
      const int i = lane + 64 * (r + W.zo);
      S.y[r] = i < m ? (S.Einv[r] * p.ys[(size_t)inst * m + i]) * S.c : 0.0;
    }
    double* xb = v + P.W;
#pragma unroll
    for (int r = 0; r < RNH; ++r)
      if (lane + 64 * (r + W.xo) < n) xb[lane + 64 * (r + W.xo)] = S.x[r];
    BAR2_X(v, p.pl.XID);
    double az[RMH];
    ell_mv<RMH, ELL_KA>(P.eA, v, xb, az, W, W.zo, W.stage(P, v));
#pragma unroll
    for (int r = 0; r < RMH; ++r) S.z[r] = lane + 64 * (r + W.zo) < m ? az[r] : 0.0;
    BAR2_X(v, p.pl.XID);
  } else {
#pragma unroll
    for (int r = 0; r < RNH; ++r) S.x[r] = 0.0;
#pragma unroll
    for (int r = 0; r < RMH; ++r) S.z[r] = 0.0, S.y[r] = 0.0;
  }
  S.pri_res = S.dua_res = 0.0;

  // ---------------- ADMM
  int wsx[RNH], wsz[RMH];
#pragma unroll
  for (int r = 0; r < RNH; ++r) wsx[r] = (int)P.wsx[lane + 64 * (r + W.xo)];
#pragma unroll
  for (int r = 0; r < RMH; ++r) wsz[r] = (int)P.wsz[lane + 64 * (r + W.zo)];
  constexpr int RN = 2 * RNH, RM = 2 * RMH;
  constexpr int coff = 64 * (RN + RM);
  constexpr int KSH = RNH + RMH;  // diagonal-pass slots of this wave: [w KSH, (w + 1) KSH)
  const int ko = W.w * KSH;
  const uint32_t wcp = P.wcopy[lane], bcp = P.bcopy[lane];
  uint32_t wmx[RNH], wmz[RMH], bmk[KSH];
  constexpr bool W0SOLVE = MODE == 3;
  uint32_t bfm[W0SOLVE ? RN + RM : 1];  // MODE 3: the diagonal pass over every slot, on wave 0
#pragma unroll
  for (int r = 0; r < (W0SOLVE ? RN + RM : 1); ++r) {
    bfm[r] = 0u - ((bcp >> r) & 1u);
    asm volatile("" : "+v"(bfm[r]));
  }
#pragma unroll
  for (int r = 0; r < RNH; ++r) {
    wmx[r] = 0u - ((wcp >> (r + W.xo)) & 1u);
    asm volatile("" : "+v"(wmx[r]));
  }
#pragma unroll
  for (int r = 0; r < RMH; ++r) {
    wmz[r] = 0u - ((wcp >> (RN + r + W.zo)) & 1u);
    asm volatile("" : "+v"(wmz[r]));
  }
#pragma unroll
  for (int r = 0; r < KSH; ++r) {
    bmk[r] = 0u - ((bcp >> (r + ko)) & 1u);
    asm volatile("" : "+v"(bmk[r]));
  }
  auto and_d = [](double x, uint32_t mk) {
    return __hiloint2double((int)((uint32_t)__double2hiint(x) & mk), (int)((uint32_t)__double2loint(x) & mk));
  };
  double sigma = sr->sigma, alpha = sr->alpha, alpha_c = 1.0 - sr->alpha;
  asm volatile("" : "+v"(sigma), "+v"(alpha), "+v"(alpha_c));
  // read once per instance, before the loop, through readfirstlane (the one-wave kernel's)
  const int chk = uniform_i(sr->check_termination);
  int ar_int = uniform_i(sr->adaptive_rho_interval);
  const int ar_on = uniform_i(sr->adaptive_rho);
  if (ar_on && ar_int == 0) ar_int = chk ? 4 * chk : 100;
  if (!ar_on) ar_int = 0;
  int chk_left = chk, ar_left = ar_int;
  int status = MPCQP_UNSOLVED, iter = 0, rho_updates = 0;
  bool can_check = false;
  constexpr bool MATPF = MODE == 1, W0STEPS = MODE == 2 || MODE == 3;
  double dx[RNH], dy[RMH];
  Resid2<RNH, RMH> R;
  HalfPipe sp;
#ifdef MPCQP_PAIR_CHECKS
  const HalfOps hops{v, W.w, PAIRED && W.w == 0, P.XID};
#else
  const HalfOps hops{v, W.w, PAIRED && W.w == 0};
#endif
  Pipe<SolveOps<PAIRED>, PAIR_PIPE> fp;  // MODE 2: wave 0's full step records
  const SolveOps<PAIRED> fops{v};
  const Rsrc rs_fwd = table_rsrc(P.fwd, P.nfwd, SOLVE_STEP_WORDS);
  const Rsrc rs_bwd = table_rsrc(P.bwd, P.nbwd, SOLVE_STEP_WORDS);
  // this wave's 1/D slots of the diagonal pass in registers between factorizations (as the
  // one-wave kernel's DREG; every factorization ends with a barrier)
  constexpr bool DREG = !W0SOLVE;
  double dvr[DREG ? KSH : 1];
  auto load_dinv = [&]() {
    if constexpr (DREG) {
#pragma unroll
      for (int r = 0; r < KSH; ++r) dvr[r] = v[P.DINV + lane + 64 * (r + ko)];
    }
  };
  load_dinv();
  // the loop bounds as opaque SGPR values (the one-wave kernel's max_iter / chk_s / ar_s)
  int max_iter = uniform_i(sr->max_iter);
  const RowTol<false> tol{vector_id(inst)};  // the check blocks load the row where they use it
  int chk_s = chk, ar_s = ar_int;
  asm volatile("" : "+s"(max_iter), "+s"(chk_s), "+s"(ar_s));
  for (iter = 1; iter <= max_iter; ++iter) {
    T_COUNT(T_ITERS);
    T_BEGIN(t_v0);
    if constexpr (W0STEPS) {
      if (W.w == 0) prefetch(rs_fwd, P.nfwd, (uint32_t)lane, fp);
    } else {
      half_prefetch(hops, rs_fwd, P.nfwd, (uint32_t)lane, sp);
    }
    double xp[RNH], zp[RMH], bz[RMH];
#pragma unroll
    for (int r = 0; r < RNH; ++r) {
      xp[r] = S.x[r];
      const double b = fma(sigma, xp[r], -S.q[r]);
      v[wsx[r] + coff] = b;
      v[wsx[r]] = and_d(b, wmx[r]);
    }
#pragma unroll
    for (int r = 0; r < RMH; ++r) {
      zp[r] = S.z[r];
      bz[r] = fma(-rinv_of(S, r), S.y[r], zp[r]);
      v[wsz[r] + coff] = bz[r];
      v[wsz[r]] = and_d(bz[r], wmz[r]);
    }
#ifdef MPCQP_PAIR_CHECKS
    if (W.inj && iter == 1)
      W.inj = 0;  // the injected divergence
    else
#endif
      BAR2_X(v, p.pl.XID);
    T_END(T_VEC, t_v0);
    if constexpr (W0SOLVE) {
      // MODE 3: wave 0 runs forward solve, diagonal pass and backward solve back to back (its
      // LDS operations execute in order: no barrier between them); wave 1 waits at the barrier
      // after the backward solve
      if (W.w == 0) {
        T_BEGIN(t_fw3);
        run_body(rs_fwd, P.nfwd, (uint32_t)lane, fops, fp);
        T_END(T_FWD, t_fw3);
        T_BEGIN(t_v13);
        prefetch(rs_bwd, P.nbwd, (uint32_t)lane, fp);
        double wv[RN + RM], dv[RN + RM];
#pragma unroll
        for (int r = 0; r < RN + RM; ++r) {
          wv[r] = v[P.W + lane + 64 * r];
          dv[r] = v[P.DINV + lane + 64 * r];
        }
#pragma unroll
        for (int r = 0; r < RN + RM; ++r) {
          const double c = wv[r] * dv[r];
          v[P.W + lane + 64 * r + coff] = c;
          v[P.W + lane + 64 * r] = and_d(c, bfm[r]);
        }
        LDS_FENCE();
        T_END(T_VEC, t_v13);
        T_BEGIN(t_bw3);
        run_body(rs_bwd, P.nbwd, (uint32_t)lane, fops, fp);
        T_END(T_BWD, t_bw3);
      }
      BAR2_X(v, p.pl.XID);
    } else {
    T_BEGIN(t_fw);
    if constexpr (W0STEPS) {
      if (W.w == 0) {
        run_body(rs_fwd, P.nfwd, (uint32_t)lane, fops, fp);
        prefetch(rs_bwd, P.nbwd, (uint32_t)lane, fp);
      }
      BAR2_X(v, p.pl.XID);
    } else if constexpr (MATPF) {
      half_body_pf(hops, rs_fwd, P.nfwd, (uint32_t)lane, sp);  // ends with a barrier
    } else {
      half_body(hops, rs_fwd, P.nfwd, (uint32_t)lane, sp);
    }
    T_END(T_FWD, t_fw);
    T_BEGIN(t_v1);
    if constexpr (!W0STEPS) half_prefetch(hops, rs_bwd, P.nbwd, (uint32_t)lane, sp);
    {
      double wv[KSH], dv[KSH];
#pragma unroll
      for (int r = 0; r < KSH; ++r) {
        wv[r] = v[P.W + lane + 64 * (r + ko)];
        if constexpr (DREG)
          dv[r] = dvr[r];
        else
          dv[r] = v[P.DINV + lane + 64 * (r + ko)];
      }
#pragma unroll
      for (int r = 0; r < KSH; ++r) {
        const double c = wv[r] * dv[r];
        v[P.W + lane + 64 * (r + ko) + coff] = c;
        v[P.W + lane + 64 * (r + ko)] = and_d(c, bmk[r]);
      }
    }
    BAR2_X(v, p.pl.XID);
    T_END(T_VEC, t_v1);
    T_BEGIN(t_bw);
    if constexpr (W0STEPS) {
      if (W.w == 0) run_body(rs_bwd, P.nbwd, (uint32_t)lane, fops, fp);
      BAR2_X(v, p.pl.XID);
    } else if constexpr (MATPF) {
      half_body_pf(hops, rs_bwd, P.nbwd, (uint32_t)lane, sp);  // ends with a barrier
    } else {
      half_body(hops, rs_bwd, P.nbwd, (uint32_t)lane, sp);
    }
    T_END(T_BWD, t_bw);
    }  // !W0SOLVE
    T_BEGIN(t_v2);
    double wx[RNH], wz[RMH];
#pragma unroll
    for (int r = 0; r < RNH; ++r) wx[r] = v[wsx[r]];
#pragma unroll
    for (int r = 0; r < RMH; ++r) wz[r] = v[wsz[r]];
    __builtin_amdgcn_sched_group_barrier(0x100, RNH + RMH, 0);
#pragma unroll
    for (int r = 0; r < RNH; ++r) {
      S.x[r] = fma(alpha, wx[r], alpha_c * xp[r]);
      dx[r] = S.x[r] - xp[r];
    }
#pragma unroll
    for (int r = 0; r < RMH; ++r) {
      const double ri = rinv_of(S, r);
      const double zt = fma(ri, wz[r], bz[r]);
      const double zr = fma(alpha, zt, alpha_c * zp[r]);
      S.z[r] = dmind(dmaxd(fma(ri, S.y[r], zr), S.l[r]), S.u[r]);
      dy[r] = rvec_of(S, r) * (zr - S.z[r]);
      S.y[r] = S.y[r] + dy[r];
    }
    LDS_FENCE();
    TSYNC(S.y[0]);
    T_END(T_VEC, t_v2);
    T_BEGIN(t_ck);
    can_check = chk_s && --chk_left == 0;
    if (can_check) chk_left = chk_s;
    const bool adapt = ar_s && --ar_left == 0;
    if (adapt) ar_left = ar_s;
    // the check-time code works on an opaque copy of the lane id: its per-lane addresses are
    // recomputed at each check instead of being hoisted out of the ADMM loop into registers (the
    // one-wave kernel's clane)
    Wv C = W;
    asm volatile("" : "+v"(C.lane));
    if (can_check || adapt) {
      BAR2_X(v, p.pl.XID);  // every wave's solution reads of W done before the residual staging rewrites it
      compute_residuals(p, S, R, v, C TACC_ARG);
      T_COUNT(T_NCHK);
    }
    if (can_check) {
      status = check_termination(p, tol, S, R, dy, dx, sb, v, C, false TACC_ARG);
      if (status != 0) {
        W.ph = C.ph;  // the exchange buffer phase carries on
        break;
      }
      status = MPCQP_UNSOLVED;
    }
    if (adapt) {
      const double rho_new = rho_estimate(p, S, R, v, C);
      const double ar_tol = tol_adaptive_rho(p, tol);
      if (rho_new > S.rho * ar_tol || rho_new < S.rho / ar_tol) {
        S.rho = dmind(dmaxd(rho_new, RHO_MIN), RHO_MAX);
        set_rho(S);
        rho_updates++;
        T_BEGIN(t_f1);
        assemble_and_factor2<RNH, RMH>(p, v, C, S, sigma);
        load_dinv();
#ifdef MPCQP_TIMING
        const unsigned long long dt_f1 = __builtin_amdgcn_s_memtime() - t_f1;
        tacc[T_FACTOR] += dt_f1;
        tacc[T_CHECK] -= dt_f1;
#endif
        T_COUNT(T_NFACT);
      }
    }
    W.ph = C.ph;
    T_END(T_CHECK, t_ck);
  }
  T_BEGIN(t_tl);
  if (!can_check) {
    iter = iter - 1;
    BAR2_X(v, p.pl.XID);
    compute_residuals(p, S, R, v, W TACC_ARG);
    status = check_termination(p, tol, S, R, dy, dx, sb, v, W, false TACC_ARG);
    if (status == 0) status = MPCQP_UNSOLVED;
  }
  if (iter > max_iter) iter = max_iter;
  if (status == MPCQP_UNSOLVED) {
    const int st = check_termination(p, tol, S, R, dy, dx, sb, v, W, true TACC_ARG);
    status = st ? st : MPCQP_MAX_ITER_REACHED;
  }

  store_solution(p, inst, S, sb, v, W, status, iter, rho_updates TTAIL_ARG(t_tl));
  BAR2_X(v, p.pl.XID);  // the image is rewritten by the next instance's scaling
}

// MPCQP_PAIR_WAVES_PER_EU<RNH>: minimum waves per SIMD of the two-wave kernel's register
// allocation -- N = 20 (RNH = 1): 2 (8 waves per CU = 4 instances, <= 256 registers);
// N = 40 (RNH = 2): 1 (2 instances = 4 waves per CU)
template <int RNH>
struct PairWpe {
  static constexpr int value = RNH == 1 ? 2 : 1;
};
template <int RNH, int RMH, bool PAIRED, int MODE>
__global__ void __launch_bounds__(128, PairWpe<RNH>::value) qp_pair_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  if ((uint32_t)(uintptr_t)lds != 0u) __builtin_trap();  // schedule byte addresses assume base 0
  double* v = lds;
  Wv W;
  W.w = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  W.lane = (int)(threadIdx.x & 63u);
  W.xo = W.w * RNH, W.zo = W.w * RMH, W.ph = 0;
#ifdef MPCQP_PAIR_CHECKS
  W.nx = 0;
  W.inj = (blockIdx.x == 0 && W.w == 1) ? g_pair_inject : 0;
  {  // the checked barrier's counters start at 0 (one hardware barrier publishes them)
    int* ck = reinterpret_cast<int*>(v + p.pl.XID);
    if (threadIdx.x == 0) ck[4] = ck[5] = ck[6] = 0;
    LDS_FENCE();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    LDS_FENCE();
  }
#endif
  double* scr = p.scratch + (size_t)blockIdx.x * slab_doubles(p.pl);
  int* xid = reinterpret_cast<int*>(v + p.pl.XID);
#ifdef MPCQP_PAIR_CHECKS
  unsigned int prev = 0xffffffffu;  // the instance this workgroup solved last
#endif
  for (;;) {
    // the first wave takes the next instance (skipping skipped ones) and hands it over in LDS
    if (threadIdx.x == 0) {
      unsigned int inst;
      for (;;) {
        inst = atomicAdd(p.counter, 1u);
        if (inst >= (unsigned int)p.B) break;
        if (p.order) {
          inst = (unsigned int)p.order[inst];
          if (inst >= (unsigned int)p.B) continue;
        }
        if (p.skip && p.skip[inst]) continue;
        break;
      }
      *xid = (int)(inst < (unsigned int)p.B ? inst : p.B);
    }
    BAR2_X(v, p.pl.XID);
    const unsigned int inst = __builtin_amdgcn_readfirstlane((unsigned int)*xid);
#ifdef MPCQP_PAIR_CHECKS
    {
      // diagnostic builds (tests/test_pair_checks.py): both waves read the same instance id and
      // have made the same number of exchanges (so the same buffer phase); a mismatch is reported
      // through the instance's status (MPCQP_PAIR_CHECK_FAILED), not a trap
      // four ints over the hand-off slot XID (allocated as two doubles; ck[0] is wave 0's copy of
      // the id it just read there, the value the slot already holds)
      int* ck = xid;
      // (with the barriers this wave has reached, its own counter ck[4 + w], in the high bits)
      if (W.lane == 0) ck[2 * W.w] = (int)inst, ck[2 * W.w + 1] = W.nx * 2 + W.ph + (ck[4 + W.w] << 12);
      BAR2_X(v, p.pl.XID);
      const bool bad = ck[0] != ck[2] || ck[1] != ck[3] || ck[6] != 0;  // [6]: a barrier timed out
      BAR2_X(v, p.pl.XID);
      // reported on the instance just solved (the divergence happened in or before its solve; a
      // workgroup's last instance has no next one) and on the one taken now, which is not solved
      if (bad && threadIdx.x == 0 && p.info.status) {
        if (prev < (unsigned int)p.B) p.info.status[prev] = -1000;
        if (inst < (unsigned int)p.B) p.info.status[inst] = -1000;
      }
      if (bad) break;
    }
#endif
    if (inst >= (unsigned int)p.B) break;  // identical in both waves
    // an opaque copy of the lane id per instance: per-lane address arithmetic is not hoisted out
    // of the instance loop into registers held for the whole kernel (the one-wave kernel's ilane)
    Wv Wi = W;
    asm volatile("" : "+v"(Wi.lane));
    solve_instance2<RNH, RMH, PAIRED, MODE>(p, (int)inst, v, scr, Wi);
    W.ph = Wi.ph;
#ifdef MPCQP_PAIR_CHECKS
    W.nx = Wi.nx, W.inj = Wi.inj;
    prev = inst;
#endif
  }
}
