// engine_adjoint.inc -- adjoint solves (solution sensitivities) of a batch's solved instances on the
// device (included by engine.hip inside its anonymous namespace, after engine_polish.inc; it uses
// the shared device helpers and that file's PolishDrift / polish_row_doubles, and edits none of
// them: the solve kernels and the polish kernel keep their code).
//
// At a solution with active rows act (lower: b = l, upper: b = u) the reduced KKT system
// K [x; y_act] = [-q; b_act], K = [P A_act'; A_act 0], holds, so for a loss L with gx = dL/dx,
// gy = dL/dy the adjoint K [dx; dy] = [gx; gy_act] (K is symmetric, dy = 0 off act) gives
//   dL/dq = -dx,  dL/dl_i = dy_i (lower-active), dL/du_i = dy_i (upper-active),
//   dL/dA_ij = -(y_i dx_j + dy_i x_j),  dL/dP_ii = -dx_i x_i,  dL/dP_ij = -(dx_i x_j + dx_j x_i)
// (a stored upper entry i < j standing for both halves).  In the engine's scaled space
// (x = D xs, y = E ys / c, Ps = c D P D, As = E A D) Ks = T K T with T = diag(sqrt(c) D, E / sqrt(c)):
// Ks ds = [c D gx; E gy], dx = D dsx, dy = E dsy / c -- no square root appears.
//
// One wave per instance at every horizon, as the polish (a two-wave plan's image runs on one wave).
// Per instance (DESIGN.md, Adjoint solves):
//   1. the last scaling again into a per-wave sink (polish step 1): D, E, c and the scaled P, A;
//   2. the active sets from the carried xs, zs, ys (form_Ared), written out as `act`;
//   3. the reduced KKT with +-delta on the handle's compiled program, factorized ONCE;
//   4. the right-hand-side loop, the kernel's own design point -- the Ruiz passes and the
//      factorization dominate one adjoint, and a gain matrix needs a right-hand side per component
//      of u0: for each of the nrhs right-hand sides the scaled [c D gx; E gy], round 0 plus `refine`
//      rounds of iterative refinement against the unregularised matrix (iterate, right-hand side
//      and residual in registers across the rounds), the residual of the last iterate as a
//      wave-reduced inf-norm relative to the right-hand side's, the unscaling, and the outputs:
//      gq, gl, gu from registers; gPx, gAx by a lane-strided pass over the nonzeros with x, dx, y, dy
//      staged in the W / C regions (free between two solves).
// Nothing a later solve or polish reads is written.

// The adjoint kernel's arguments: the solve kernels' (embedded, so the shared device functions take
// them as they are; k.x_out / k.y_out unused) and its own.  KParams and DevPlan keep their layout.
struct AParams {
  KParams k;              // k.scratch: [grid][polish_row_doubles]
  const int32_t* status;  // [B] the status the solve wrote
  const double *x, *y;    // [B][n], [B][m] the unscaled solution: read, never written
  mpcqp_adjoint_in in;
  mpcqp_adjoint_out out;
};

// an instance that is not attempted: zeros in every requested gradient row, so a caller may sum
__device__ __forceinline__ void adjoint_zero_rows(const AParams& ap, int inst, int lane) {
  const DevPlan& P = ap.k.pl;
  const mpcqp_adjoint_out& o = ap.out;
  for (int k = 0; k < ap.in.nrhs; ++k) {
    const size_t row = (size_t)k * ap.k.B + inst;
    for (int j = lane; j < P.n; j += 64)
      if (o.gq) o.gq[row * P.n + j] = 0.0;
    for (int i = lane; i < P.m; i += 64) {
      if (o.gl) o.gl[row * P.m + i] = 0.0;
      if (o.gu) o.gu[row * P.m + i] = 0.0;
    }
    if (o.gPx)
      for (int e = lane; e < P.nnzP; e += 64) o.gPx[row * P.nnzP + e] = 0.0;
    if (o.gAx)
      for (int e = lane; e < P.nnzA; e += 64) o.gAx[row * P.nnzA + e] = 0.0;
    if (lane == 0 && o.res) o.res[row] = 0.0;
  }
  if (o.act)
    for (int i = lane; i < P.m; i += 64) o.act[(size_t)inst * P.m + i] = 0;
  if (lane == 0 && o.status_adjoint) o.status_adjoint[inst] = 0;
}

template <int RN, int RM, bool PAIRED>
__device__ __forceinline__ void adjoint_instance(const AParams& ap, int inst, double* v, double* scr,
                                                 int lane) {
  const KParams& p = ap.k;
  const DevPlan& P = p.pl;
  const mpcqp_adjoint_out& o = ap.out;
  const int n = P.n, m = P.m;
  const Slab sb = slab_of(P, scr);
  double* const sink = scr + slab_doubles(P);
  double* const mv = P.mv_slab ? sb.MV : v;
  One W{lane, mv};
  Inst<RN, RM> S;
#ifdef MPCQP_TIMING
  unsigned long long tacc[T_NSLOT] = {};
#endif
  // ---------------- 1. the last scaling again: D, E into the slab, c, the scaled [P | A] into MV
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
  // ---------------- 2. active sets (form_Ared) of the carried iterates: bit r = row lane + 64 r
  uint32_t low = 0, upp = 0;
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    const int i = lane + 64 * r;
    const bool in = i < m;
    const double z = in ? p.zs[(size_t)inst * m + i] : 0.0;
    const double y = in ? p.ys[(size_t)inst * m + i] : 0.0;
    const bool lo = in && z - S.l[r] < -y;
    const bool up = in && S.u[r] - z < y;
    low |= (lo ? 1u : 0u) << r, upp |= (up ? 1u : 0u) << r;
    if (in && o.act) o.act[(size_t)inst * m + i] = lo ? (int8_t)-1 : (up ? (int8_t)1 : (int8_t)0);
  }
  const uint32_t act = low | upp;
  const double delta = uniform_d(set_row_at_use(p, vector_id(inst))->delta);
  // ---------------- 3. the reduced KKT on the full pattern (polish step 4), factorized once
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
  // ---------------- 4. the right-hand sides
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
  const int refine = ap.in.refine;
  const bool pattern = o.gPx || o.gAx;
  // the staging of the nonzero pass: x, dx, y, dy over the W and C regions (2 NKP >= 2 (n + m)
  // doubles, contiguous: build_dev_image), both rewritten whole by the next solve's right-hand side
  double* const xb = v + P.W;
  double* const yb = xb + n;  // the refinement's staging of the dual iterate (past m: W padding)
  double* const db = xb + n;
  double* const ys = db + n;
  double* const eb = ys + m;
#pragma unroll 1
  for (int k = 0; k < ap.in.nrhs; ++k) {
    const size_t row = (size_t)k * p.B + inst;
    // the scaled right-hand side [c D gx; E gy on the active rows] and its inf-norm
    double bx[RN], bz[RM], sx[RN], sy[RM];
    double bn = 0.0;
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = lane + 64 * r;
      bx[r] = j < n ? (S.c * sb.D[j]) * ap.in.gx[row * n + j] : 0.0;
      sx[r] = 0.0;
      bn = dmaxd(bn, fabs(bx[r]));
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      bz[r] = (ap.in.gy && ((act >> r) & 1u)) ? sb.E[i] * ap.in.gy[row * m + i] : 0.0;
      sy[r] = 0.0;
      bn = dmaxd(bn, fabs(bz[r]));
    }
    bn = wave_max(bn);
    // round 0 solves the right-hand side itself; round it >= 1 solves the residual against
    // [P A_act'; A_act 0] and adds; the pass after the last round only takes the residual's norm
    double rn = 0.0;
#pragma unroll 1
    for (int it = 0;; ++it) {
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
        for (int r = 0; r < RM; ++r) yb[lane + 64 * r] = sy[r];
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
      if (it > refine) {  // wave-uniform
#pragma unroll
        for (int r = 0; r < RN; ++r) rn = dmaxd(rn, fabs(rx[r]));
#pragma unroll
        for (int r = 0; r < RM; ++r) rn = dmaxd(rn, fabs(rz[r]));
        rn = wave_max(rn);
        break;
      }
      // K d = r on the factor (polish step 5): the right-hand side into C, W starting at 0 or at the
      // copy rows' values, forward solve, diagonal pass, backward solve
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
    if (lane == 0 && o.res) o.res[row] = bn > 0.0 ? rn / bn : 0.0;
    // unscale (dx = D dsx, dy = E dsy / c); gq, gl, gu straight from registers
    LDS_FENCE();
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = lane + 64 * r;
      if (j < n) {
        const double dx = sb.D[j] * sx[r];
        if (o.gq) o.gq[row * n + j] = -dx;
        if (pattern) xb[j] = ap.x[(size_t)inst * n + j], db[j] = dx;
      }
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      if (i < m) {
        const double dy = (sb.E[i] * sy[r]) * S.cinv;  // 0 off the active rows
        if (o.gl) o.gl[row * m + i] = ((low >> r) & 1u) ? dy : 0.0;
        if (o.gu) o.gu[row * m + i] = ((upp >> r) & 1u) ? dy : 0.0;
        if (pattern) ys[i] = ((act >> r) & 1u) ? ap.y[(size_t)inst * m + i] : 0.0, eb[i] = dy;
      }
    }
    LDS_FENCE();
    // the nonzero pass: one entry per lane and trip, its row / column from the structure arrays
    if (o.gPx)
      for (int e = lane; e < P.nnzP; e += 64) {
        const int i = P.Pi[e], j = P.Pcol[e];
        o.gPx[row * P.nnzP + e] = (i == j) ? -(db[i] * xb[i]) : -(db[i] * xb[j] + db[j] * xb[i]);
      }
    if (o.gAx)
      for (int e = lane; e < P.nnzA; e += 64) {
        const int i = P.Ai[e], j = P.Acol[e];
        o.gAx[row * P.nnzA + e] = -(ys[i] * db[j] + eb[i] * xb[j]);
      }
    LDS_FENCE();
  }
  if (lane == 0 && o.status_adjoint) o.status_adjoint[inst] = 1;
}

// One wave per workgroup on a persistent grid, instances by a grid-stride loop (an adjoint costs the
// same for every instance: no work counter); the instance image is the workgroup's whole dynamic
// LDS at address 0, the scratch row is the wave's.
template <int RN, int RM, bool PAIRED>
__global__ void __launch_bounds__(64, 1) qp_adjoint_kernel(AParams ap) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = (int)threadIdx.x;
  if ((uint32_t)(uintptr_t)lds != 0u) __builtin_trap();  // schedule byte addresses assume base 0
  double* v = lds;
  const KParams& p = ap.k;
  double* scr = p.scratch + (size_t)blockIdx.x * polish_row_doubles(p.pl.n, p.pl.m, p.pl.mv_slab, p.pl.nnzP);
  for (int inst = (int)blockIdx.x; inst < p.B; inst += (int)gridDim.x) {
    // attempted: solved, not skipped, carrying that solve's state (the polish's rule)
    const bool go = __builtin_amdgcn_readfirstlane(ap.status[inst]) == MPCQP_SOLVED &&
                    !(p.skip && __builtin_amdgcn_readfirstlane(p.skip[inst]) != 0) &&
                    __builtin_amdgcn_readfirstlane(p.has_state[inst]) == 1 &&
                    __builtin_amdgcn_readfirstlane(p.dsel[inst]) >= -1;
    if (!go) {
      adjoint_zero_rows(ap, inst, lane);
      continue;
    }
    int ilane = lane;  // opaque per instance, as in the solve kernels (MPCQP_OPAQUE_LANE_RN)
    asm volatile("" : "+v"(ilane));
    adjoint_instance<RN, RM, PAIRED>(ap, inst, v, scr, ilane);
    LDS_FENCE();
  }
}

typedef void (*adjoint_fn)(AParams);
// the instantiation for the plan's register bucket and step kind, as select_polish chooses
adjoint_fn select_adjoint(int n, int m, bool paired) {
  int rn = 0, rm = 0;
  if (!kernel_bucket(n, m, rn, rm)) return nullptr;
  if (rn == 2) return paired ? qp_adjoint_kernel<2, 4, true> : qp_adjoint_kernel<2, 4, false>;
#if !defined(MPCQP_DEV20) && !defined(MPCQP_ONLY_SMALL)
  if (rn == 4) return paired ? qp_adjoint_kernel<4, 8, true> : qp_adjoint_kernel<4, 8, false>;
#endif
  return nullptr;
}
