// engine_polish.inc -- polishing (OSQP 0.6 polish.c) of a batch's solved instances on the device
// (included by engine.hip inside its anonymous namespace, after engine_pair.inc; it uses that
// file's device helpers and edits none of them: the solve kernels keep their code).
//
// One wave per instance at every horizon -- a polish is one factorization and 1 +
// polish_refine_iter solves, not hundreds of iterations, so the two-wave split buys nothing and a
// two-wave plan's image and full step records run on one wave as they are (run_factor, the
// restarting run_body).  Per instance (DESIGN.md, Polishing):
//   1. the last scaling again, as a bounds-only solve reproduces it: scale_problem / scale_finish on
//      the input of the last scaling (the drift buffer or set-up row dsel names), bitwise the same
//      D, E, c and scaled P, q, A; the unscaled output goes to a per-wave sink (PolishDrift), so
//      nothing a later solve reads is written;
//   2. the carried scaled iterates, and the ADMM solution's residuals (compute_residuals): the
//      values to beat;
//   3. the active sets (form_Ared) as two RM-bit words per lane;
//   4. the reduced KKT on the handle's compiled program: an active row keeps its A entries and gets
//      the diagonal -delta, an inactive one is stored as zeros with the diagonal -1 (it decouples:
//      y_i = 0), P gets +delta where the solve kernels add sigma.  The row activity is staged in the
//      W region (m words) and each lane folds the flags of its A entries' rows (Ai[k]) into one
//      register word before the image is zeroed -- W overlays factor slots;
//   5. rhs = [-q; l | u | 0], solved, then polish_refine_iter rounds of iterative refinement against
//      the unregularised matrix (the residual ELLs, y being 0 on inactive rows);
//   6. z = A x, the normal-cone projection, the residuals and the objective; accepted by OSQP's
//      rule.  On success x, y (unscaled) and the carried xs, zs, ys are overwritten.
// The active-set words, the iterates, the right-hand side and the refinement residual stay in
// registers across the refinement loop; LDS holds the factor image, the staged vectors and the m
// activity words.

// The polish kernel's arguments: the solve kernels' (embedded, so the shared device functions take
// them as they are) and its own.  KParams and DevPlan keep their layout.
struct PParams {
  KParams k;              // k.scratch: [grid][polish_row_doubles], k.x_out / k.y_out: the outputs
  const int32_t* status;  // [B] the status the preceding solve wrote
  mpcqp_polish_info info;
};
// a wave's scratch row: the slab of the solve kernels (D, E, the resident values of a mv_global
// plan), then the sink of scale_problem's unscaled P values and q
__host__ __device__ __forceinline__ size_t polish_row_doubles(int n, int m, int mv_slab, int nnzP) {
  return slab_doubles(n, m, mv_slab) + (((size_t)nnzP + n + 1) & ~size_t(1));
}
// scale_problem's data selection for a polish: the input of the instance's last scaling, and an
// output that goes nowhere (the drift buffers, dsel and pend stay as the solve left them)
struct PolishDrift {
  const double *P_in, *q_in;
  double *P_sink, *q_sink;
  __device__ __forceinline__ const double* in_P(const KParams&, int) const { return P_in; }
  __device__ __forceinline__ const double* in_q(const KParams&, int) const { return q_in; }
  __device__ __forceinline__ double* out_P(const KParams&, int) const { return P_sink; }
  __device__ __forceinline__ double* out_q(const KParams&, int) const { return q_sink; }
};

// compute_obj_val of the scaled x (store_solution's sum)
template <int RN, int RM>
__device__ __forceinline__ double polish_objective(const DevPlan& P, const Inst<RN, RM>& S, double* v,
                                                   const double* mv, int lane) {
  double* xb = v + P.W;
  LDS_FENCE();
#pragma unroll
  for (int r = 0; r < RN; ++r)
    if (lane + 64 * r < P.n) xb[lane + 64 * r] = S.x[r];
  LDS_FENCE();
  double part = 0.0;
  for (int k = lane; k < P.nnzP; k += 64) {
    const int i = P.Pi[k], j = P.Pcol[k];
    const double pk = mv[P.MV + k];
    part += (i == j) ? .5 * pk * xb[i] * xb[i] : pk * xb[i] * xb[j];
  }
#pragma unroll
  for (int r = 0; r < RN; ++r)
    if (lane + 64 * r < P.n) part += S.q[r] * S.x[r];
  const double obj = wave_sum(part) * S.cinv;
  LDS_FENCE();
  return obj;
}

template <int RN, int RM, bool PAIRED>
__device__ __forceinline__ void polish_instance(const PParams& pp, int inst, double* v, double* scr,
                                                int lane) {
  const KParams& p = pp.k;
  const DevPlan& P = p.pl;
  const int n = P.n, m = P.m;
  const Slab sb = slab_of(P, scr);
  double* const sink = scr + slab_doubles(P);
  double* const mv = P.mv_slab ? sb.MV : v;
  One W{lane, mv};
  Inst<RN, RM> S;
#ifdef MPCQP_TIMING
  unsigned long long tacc[T_NSLOT] = {};
#endif
  // ---------------- 1. the last scaling again
  {
    const int sel = __builtin_amdgcn_readfirstlane(p.dsel[inst]);  // -1, 0 or 1 after a solve
    PolishDrift dr;
    dr.P_in = sel < 0 ? setup_row(p.Px, p.Px_stride, inst) : drift_row(p.Pw, sel, p.B, P.nnzP, inst);
    dr.q_in = sel < 0 ? setup_row(p.q, p.q_stride, inst) : drift_row(p.qw, sel, p.B, n, inst);
    dr.P_sink = sink, dr.q_sink = sink + P.nnzP;
    double D[RN], E[RM];
    scale_problem(p, inst, dr, S, v, W, D, E TACC_ARG);
    scale_finish(p, inst, false, S, sb, v, mv, W, D, E);
  }
  // ---------------- 2. the ADMM solution and its residuals
#pragma unroll
  for (int r = 0; r < RN; ++r) {
    const int j = lane + 64 * r;
    S.x[r] = j < n ? p.xs[(size_t)inst * n + j] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    const int i = lane + 64 * r;
    S.z[r] = i < m ? p.zs[(size_t)inst * m + i] : 0.0;
    S.y[r] = i < m ? p.ys[(size_t)inst * m + i] : 0.0;
  }
  S.pri_res = S.dua_res = 0.0;
  Resid<RN, RM> R;
  compute_residuals(p, S, R, v, W TACC_ARG);
  const double pri0 = S.pri_res, dua0 = S.dua_res;
  const double obj0 = polish_objective(P, S, v, mv, lane);
  // ---------------- 3. active sets (form_Ared): bit r of low / upp = row lane + 64 r
  uint32_t low = 0, upp = 0;
  int n_low = 0, n_upp = 0;
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    const bool in = lane + 64 * r < m;
    const bool lo = in && S.z[r] - S.l[r] < -S.y[r];
    const bool up = in && S.u[r] - S.z[r] < S.y[r];
    low |= (lo ? 1u : 0u) << r, upp |= (up ? 1u : 0u) << r;
    n_low += __popcll(__ballot(lo)), n_upp += __popcll(__ballot(up));
  }
  const uint32_t act = low | upp;
  // the instance's own delta and refinement rounds, read where they are used
  const mpcqp_settings* sr = set_row_at_use(p, vector_id(inst));
  const double delta = uniform_d(sr->delta);
  const int refine = uniform_i(sr->polish_refine_iter);
  // ---------------- 4. the reduced KKT, assembled on the full pattern, and its factorization
  uint32_t amask = 0;  // bit j: A entry 64 j + lane lies in an active row
  {
    uint32_t* aw = reinterpret_cast<uint32_t*>(v + P.W);
    LDS_FENCE();
#pragma unroll
    for (int r = 0; r < RM; ++r)
      if (lane + 64 * r < m) aw[lane + 64 * r] = (act >> r) & 1u;
    LDS_FENCE();
#pragma unroll
    for (int j = 0; j < 8 * RN; ++j) {  // nnzA <= 64 SJ <= 512 RN (build_dev_image)
      if (64 * j >= P.nnzA) break;      // wave-uniform
      const int k = 64 * j + lane;
      if (k < P.nnzA && aw[P.Ai[k]] != 0u) amask |= 1u << j;
    }
    LDS_FENCE();
  }
  for (int k = lane; k < P.nnzL; k += 64) v[P.LX + k] = 0.0;
#pragma unroll
  for (int r = 0; r < RN + RM; ++r) v[P.DINV + lane + 64 * r] = 0.0;
  if (lane < ZERO_BLOCK) v[P.ZERO + lane] = 0.0;
  if (lane == 0) {
    v[P.ONE] = 1.0;
    v[P.MONE] = -1.0;
  }
  LDS_FENCE();
  for (int j = lane; j < n; j += 64) v[P.slotSig[j]] = delta;
  LDS_FENCE();
  for (int k = lane; k < P.nnzP; k += 64) {
    const double val = mv[P.MV + k];
    v[P.slotP[k]] = (P.Pi[k] == P.Pcol[k]) ? val + delta : val;
  }
#pragma unroll
  for (int j = 0; j < 8 * RN; ++j) {
    if (64 * j >= P.nnzA) break;
    const int k = 64 * j + lane;
    if (k < P.nnzA) v[P.slotA[k]] = ((amask >> j) & 1u) ? mv[P.MV + P.nnzP + k] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    const int i = lane + 64 * r;
    if (i < m) v[P.slotRho[i]] = ((act >> r) & 1u) ? -delta : -1.0;
  }
  LDS_FENCE();
  run_factor(p, v, lane);
  LDS_FENCE();
  // ---------------- 5. solve and refine
  int wsx[RN], wsz[RM];
#pragma unroll
  for (int r = 0; r < RN; ++r) wsx[r] = (int)P.wsx[lane + 64 * r];
#pragma unroll
  for (int r = 0; r < RM; ++r) wsz[r] = (int)P.wsz[lane + 64 * r];
  constexpr int coff = 64 * (RN + RM);
  const uint32_t wcp = P.wcopy[lane], bcp = P.bcopy[lane];
  auto and_d = [](double x, uint32_t bit) {
    const uint32_t mk = 0u - (bit & 1u);
    return __hiloint2double((int)((uint32_t)__double2hiint(x) & mk), (int)((uint32_t)__double2loint(x) & mk));
  };
  const SolveOps<PAIRED> sops{v};
  const Rsrc rs_fwd = table_rsrc(P.fwd, P.nfwd, SOLVE_STEP_WORDS);
  const Rsrc rs_bwd = table_rsrc(P.bwd, P.nbwd, SOLVE_STEP_WORDS);
  // the right-hand side [-q; l on lower-active rows, u on upper-active ones, 0 elsewhere]
  double bx[RN], bz[RM], sx[RN], sy[RM];
#pragma unroll
  for (int r = 0; r < RN; ++r) bx[r] = lane + 64 * r < n ? -S.q[r] : 0.0, sx[r] = 0.0;
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    bz[r] = ((low >> r) & 1u) ? S.l[r] : (((upp >> r) & 1u) ? S.u[r] : 0.0);
    sy[r] = 0.0;
  }
  double* xb = v + P.W;
  double* yb = v + P.W + n;
  // round 0 solves the right-hand side itself (the residual of the zero vector, exactly); round
  // it >= 1 is iterative_refinement's: the residual against [P A_act'; A_act 0], solved and added
#pragma unroll 1
  for (int it = 0; it <= refine; ++it) {
    double rx[RN], rz[RM];
#pragma unroll
    for (int r = 0; r < RN; ++r) rx[r] = bx[r];
#pragma unroll
    for (int r = 0; r < RM; ++r) rz[r] = bz[r];
    if (it > 0) {
      LDS_FENCE();
      stage_x(W, n, xb, sx);
      LDS_FENCE();
#pragma unroll
      for (int r = 0; r < RM; ++r) yb[lane + 64 * r] = sy[r];  // past m: W padding
      LDS_FENCE();
      double ax[RM], px[RN], aty[RN];
      ell_mv<RM, ELL_KA>(P.eA, mv, xb, ax, W, 0, W.stage(P, v));
      ell_mv<RN, ELL_KP>(P.eP, mv, xb, px, W, 0, W.stage(P, v));
      ell_mv<RN, ELL_KAT>(P.eAt, mv, yb, aty, W, 0, W.stage(P, v));
#pragma unroll
      for (int r = 0; r < RN; ++r) rx[r] = lane + 64 * r < n ? (bx[r] - px[r]) - aty[r] : 0.0;
#pragma unroll
      for (int r = 0; r < RM; ++r) rz[r] = ((act >> r) & 1u) ? bz[r] - ax[r] : 0.0;
      LDS_FENCE();
    }
    // K d = r on the factor: the right-hand side into C, W starting at 0 or at the copy rows'
    // values, forward solve, diagonal pass, backward solve (the ADMM iteration's sequence)
    Pipe<SolveOps<PAIRED>> sp;
    prefetch(rs_fwd, P.nfwd, (uint32_t)lane, sp);
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      v[wsx[r] + coff] = rx[r];
      v[wsx[r]] = and_d(rx[r], wcp >> r);
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      v[wsz[r] + coff] = rz[r];
      v[wsz[r]] = and_d(rz[r], wcp >> (RN + r));
    }
    LDS_FENCE();
    run_body(rs_fwd, P.nfwd, (uint32_t)lane, sops, sp);
    prefetch(rs_bwd, P.nbwd, (uint32_t)lane, sp);
    {
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
        v[P.W + lane + 64 * r] = and_d(c, bcp >> r);
      }
    }
    LDS_FENCE();
    run_body(rs_bwd, P.nbwd, (uint32_t)lane, sops, sp);
    LDS_FENCE();
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const double d = v[wsx[r]];
      sx[r] = lane + 64 * r < n ? sx[r] + d : 0.0;
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const double d = v[wsz[r]];
      sy[r] = ((act >> r) & 1u) ? sy[r] + d : 0.0;
    }
    LDS_FENCE();
  }
  // ---------------- 6. z = A x, the normal-cone projection, residuals, objective, acceptance
#pragma unroll
  for (int r = 0; r < RN; ++r) S.x[r] = sx[r];
  {
    LDS_FENCE();
    stage_x(W, n, xb, S.x);
    LDS_FENCE();
    double ax[RM];
    ell_mv<RM, ELL_KA>(P.eA, mv, xb, ax, W, 0, W.stage(P, v));
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const bool in = lane + 64 * r < m;
      const double t = ax[r] + sy[r];
      const double zc = dmind(dmaxd(t, S.l[r]), S.u[r]);
      S.z[r] = in ? zc : 0.0;
      S.y[r] = in ? t - zc : 0.0;
    }
    LDS_FENCE();
  }
  compute_residuals(p, S, R, v, W TACC_ARG);
  const double pri1 = S.pri_res, dua1 = S.dua_res;
  const double obj1 = polish_objective(P, S, v, mv, lane);
  const bool ok = (pri1 < pri0 && dua1 < dua0) || (pri1 < pri0 && dua0 < 1e-10) ||
                  (dua1 < dua0 && pri0 < 1e-10);
  if (ok) {  // wave-uniform: the unscaled solution and the carried iterates (rho is kept)
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = lane + 64 * r;
      if (j < n) {
        p.x_out[(size_t)inst * n + j] = sb.D[j] * S.x[r];
        p.xs[(size_t)inst * n + j] = S.x[r];
      }
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      if (i < m) {
        p.y_out[(size_t)inst * m + i] = (sb.E[i] * S.y[r]) * S.cinv;
        p.zs[(size_t)inst * m + i] = S.z[r];
        p.ys[(size_t)inst * m + i] = S.y[r];
      }
    }
  }
  if (lane == 0) {
    const mpcqp_polish_info& o = pp.info;
    if (o.status_polish) o.status_polish[inst] = ok ? 1 : -1;
    if (o.obj_val) o.obj_val[inst] = ok ? obj1 : obj0;
    if (o.pri_res) o.pri_res[inst] = ok ? pri1 : pri0;
    if (o.dua_res) o.dua_res[inst] = ok ? dua1 : dua0;
    if (o.n_low) o.n_low[inst] = n_low;
    if (o.n_upp) o.n_upp[inst] = n_upp;
  }
}

// One wave per workgroup on a persistent grid, instances by a grid-stride loop (a polish costs the
// same for every instance: no work counter); the instance image is the workgroup's whole dynamic
// LDS at address 0, the scratch row is the wave's.
template <int RN, int RM, bool PAIRED>
__global__ void __launch_bounds__(64, 1) qp_polish_kernel(PParams pp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = (int)threadIdx.x;
  if ((uint32_t)(uintptr_t)lds != 0u) __builtin_trap();  // schedule byte addresses assume base 0
  double* v = lds;
  const KParams& p = pp.k;
  double* scr = p.scratch + (size_t)blockIdx.x * polish_row_doubles(p.pl.n, p.pl.m, p.pl.mv_slab, p.pl.nnzP);
  for (int inst = (int)blockIdx.x; inst < p.B; inst += (int)gridDim.x) {
    // attempted: solved (OSQP polishes OSQP_SOLVED only), not skipped, carrying that solve's state
    const bool go = __builtin_amdgcn_readfirstlane(pp.status[inst]) == MPCQP_SOLVED &&
                    !(p.skip && __builtin_amdgcn_readfirstlane(p.skip[inst]) != 0) &&
                    __builtin_amdgcn_readfirstlane(p.has_state[inst]) == 1 &&
                    __builtin_amdgcn_readfirstlane(p.dsel[inst]) >= -1;
    if (!go) {
      if (lane == 0 && pp.info.status_polish) pp.info.status_polish[inst] = 0;
      continue;
    }
    int ilane = lane;  // opaque per instance, as in the solve kernels (MPCQP_OPAQUE_LANE_RN)
    asm volatile("" : "+v"(ilane));
    polish_instance<RN, RM, PAIRED>(pp, inst, v, scr, ilane);
    LDS_FENCE();
  }
}

typedef void (*polish_fn)(PParams);
// the instantiation for the plan's register bucket and step kind, as select_kernel chooses
polish_fn select_polish(int n, int m, bool paired) {
  int rn = 0, rm = 0;
  if (!kernel_bucket(n, m, rn, rm)) return nullptr;
  if (rn == 2) return paired ? qp_polish_kernel<2, 4, true> : qp_polish_kernel<2, 4, false>;
#if !defined(MPCQP_DEV20) && !defined(MPCQP_ONLY_SMALL)
  if (rn == 4) return paired ? qp_polish_kernel<4, 8, true> : qp_polish_kernel<4, 8, false>;
#endif
  return nullptr;
}
