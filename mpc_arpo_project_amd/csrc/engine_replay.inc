// engine_replay.inc -- the adjoint tape and its replay: reverse-mode gradients through many solves
// of one handle (included by engine.hip inside its anonymous namespace, after engine_tangent.inc; it
// uses the shared device helpers and engine_polish.inc's PolishDrift / polish_row_doubles, and edits
// none of them: the solve, polish, adjoint and tangent kernels keep their code).
//
// mpcqp_adjoint reads what the handle carries: the scaled iterates for the active rows, the drift
// buffers for the scaling, the handle's own A, l, u.  A rollout's backward pass comes back to step t
// when the handle is at step T.  So the two things of step t that cannot be had again later are
// recorded right after its solve -- the active rows (adjoint_tape_kernel: one byte per row) and,
// by the caller, the data and the solution -- and qp_replay_kernel does the adjoint solve from that
// record alone.  The handle gives it the compiled plan, the settings rows, a scratch row per wave
// and the stream; no carried array is among its arguments (mpcqp_adjoint_replay nulls them).
//
// One wave per instance at every horizon, as the polish, the adjoint and the tangent.  Per taped
// instance (DESIGN.md, Adjoint tape and replay):
//   1. the equilibration of the taped data from scratch: scale_problem's passes start from the
//      caller's P, q (shared row or the instance's) and A, l, u with D = E = c = 1, the unscaled
//      output goes to the wave's sink, D, E and the scaled [P | A] to the wave's slab / the image.
//      It is the scaling the handle did at the tape point where that started from the set-up data
//      (bitwise: the same passes on the same numbers); where the handle had drifted (OSQP's
//      unscale / rescale between updates of A) it is another equilibration of the same problem, and
//      the gradients agree to rounding, not bitwise;
//   2. the active words from the tape row: one byte per row slot and lane, 64 consecutive bytes per
//      wave load, folded into the two RM-bit words `low` / `upp` the later steps index -- no iterate
//      and no bound is read, the rule was applied when the tape was taken;
//   3. the reduced KKT with +-delta on the handle's compiled program, factorized ONCE;
//   4. the right-hand-side loop of the adjoint: iterate, right-hand side and residual in registers
//      across the refinement rounds, `res` and the outputs as the adjoint takes and writes them.
// Steps 3 and 4 are the adjoint's arithmetic restated, operation for operation: with the same
// scaled matrix and the same active words every output is the adjoint's bit for bit.

// The replay kernel's arguments: the solve kernels' (embedded, so the shared device functions take
// them as they are) with Px / q / Ax / l / u naming the CALLER's arrays and every carried-state
// pointer null, and its own.  KParams and DevPlan keep their layout.
struct RParams {
  KParams k;               // k.scratch: [grid][polish_row_doubles]
  const double *x, *y;     // [B][n], [B][m] the unscaled solution at the tape point
  const int8_t* act;       // [B][m] the tape's active rows
  const int32_t* taped;    // [B] 1: replay the instance
  mpcqp_adjoint_in in;
  mpcqp_adjoint_out out;
};

// The tape: the adjoint's step 2 on the carried scaled iterates, elementwise.  The adjoint's scaled
// bounds are clamp(l) * E and clamp(u) * E of a scaling it redoes from the input of the instance's
// last scaling; the Ruiz passes are bitwise reproducible, so that E is the E the solve stored
// (store_solution: Ecls), and one product per bound gives the adjoint's operands without a pass.
// go is the adjoint kernel's rule.  One thread per row, the row's first thread writes `taped`.
__global__ void adjoint_tape_kernel(const double* zs, const double* ys, const double* E, const double* l,
                                    const double* u, const int32_t* status, const int32_t* skip,
                                    const int32_t* has_state, const int32_t* dsel, int8_t* act,
                                    int32_t* taped, int B, int m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * m) return;
  const size_t b = t / (size_t)m;
  const bool go = status[b] == MPCQP_SOLVED && !(skip && skip[b] != 0) && has_state[b] == 1 && dsel[b] >= -1;
  int8_t a = 0;
  if (go) {
    const double e = E[t], z = zs[t], y = ys[t];
    const double ls = dmaxd(l[t], -OSQP_INFTY) * e, us = dmind(u[t], OSQP_INFTY) * e;
    const bool lo = z - ls < -y, up = us - z < y;
    a = lo ? (int8_t)-1 : (up ? (int8_t)1 : (int8_t)0);
  }
  act[t] = a;
  if (t == b * (size_t)m) taped[b] = go ? 1 : 0;
}

// an instance that is not taped: zeros in every requested gradient row, so a caller may sum
__device__ __forceinline__ void replay_zero_rows(const RParams& rp, int inst, int lane) {
  const DevPlan& P = rp.k.pl;
  const mpcqp_adjoint_out& o = rp.out;
  for (int k = 0; k < rp.in.nrhs; ++k) {
    const size_t row = (size_t)k * rp.k.B + inst;
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
__device__ __forceinline__ void replay_instance(const RParams& rp, int inst, double* v, double* scr,
                                                int lane) {
  const KParams& p = rp.k;
  const DevPlan& P = p.pl;
  const mpcqp_adjoint_out& o = rp.out;
  const int n = P.n, m = P.m;
  const Slab sb = slab_of(P, scr);
  double* const sink = scr + slab_doubles(P);
  double* const mv = P.mv_slab ? sb.MV : v;
  One W{lane, mv};
  double c, cinv;  // the cost scaling and its inverse: all of Inst that outlives step 1
#ifdef MPCQP_TIMING
  unsigned long long tacc[T_NSLOT] = {};
#endif
  // ---------------- 1. the taped data equilibrated from scratch: D, E into the slab, c, the scaled
  // [P | A] into MV.  p.Px / p.q (with their strides) and p.Ax / p.l / p.u are the caller's
  {
    PolishDrift dr;
    dr.P_in = setup_row(p.Px, p.Px_stride, inst);
    dr.q_in = setup_row(p.q, p.q_stride, inst);
    dr.P_sink = sink, dr.q_sink = sink + P.nnzP;
    Inst<RN, RM> S;  // scaled q and bounds die here: the replay reads neither
    double D[RN], E[RM];
    scale_problem(p, inst, dr, S, v, W, D, E TACC_ARG);
    scale_finish(p, inst, false, S, sb, v, mv, W, D, E);
    c = S.c, cinv = S.cinv;
  }
  // ---------------- 2. the active words from the tape: bit r = row lane + 64 r
  uint32_t low = 0, upp = 0;
  {
    const int8_t* const arow = rp.act + (size_t)inst * m;
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      const int a = i < m ? (int)arow[i] : 0;
      low |= (a < 0 ? 1u : 0u) << r, upp |= (a > 0 ? 1u : 0u) << r;
      if (i < m && o.act) o.act[(size_t)inst * m + i] = (int8_t)a;
    }
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
  const int refine = rp.in.refine;
  const bool pattern = o.gPx || o.gAx;
  // the staging of the nonzero pass: x, dx, y, dy over the W and C regions (2 NKP >= 2 (n + m)
  // doubles, contiguous: build_dev_image), both rewritten whole by the next solve's right-hand side
  double* const xb = v + P.W;
  double* const yb = xb + n;  // the refinement's staging of the dual iterate (past m: W padding)
  double* const db = xb + n;
  double* const ys = db + n;
  double* const eb = ys + m;
#pragma unroll 1
  for (int k = 0; k < rp.in.nrhs; ++k) {
    const size_t row = (size_t)k * p.B + inst;
    // the scaled right-hand side [c D gx; E gy on the active rows] and its inf-norm
    double bx[RN], bz[RM], sx[RN], sy[RM];
    double bn = 0.0;
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = lane + 64 * r;
      bx[r] = j < n ? (c * sb.D[j]) * rp.in.gx[row * n + j] : 0.0;
      sx[r] = 0.0;
      bn = dmaxd(bn, fabs(bx[r]));
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      bz[r] = (rp.in.gy && ((act >> r) & 1u)) ? sb.E[i] * rp.in.gy[row * m + i] : 0.0;
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
          const double cw = wv[r] * dv[r];
          v[P.W + lane + 64 * r + coff] = cw;
          v[P.W + lane + 64 * r] = and_d(cw, bcp >> r);
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
        if (pattern) xb[j] = rp.x[(size_t)inst * n + j], db[j] = dx;
      }
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      if (i < m) {
        const double dy = (sb.E[i] * sy[r]) * cinv;  // 0 off the active rows
        if (o.gl) o.gl[row * m + i] = ((low >> r) & 1u) ? dy : 0.0;
        if (o.gu) o.gu[row * m + i] = ((upp >> r) & 1u) ? dy : 0.0;
        if (pattern) ys[i] = ((act >> r) & 1u) ? rp.y[(size_t)inst * m + i] : 0.0, eb[i] = dy;
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

// One wave per workgroup on a persistent grid, instances by a grid-stride loop (a replay costs the
// same for every taped instance: no work counter); the instance image is the workgroup's whole
// dynamic LDS at address 0, the scratch row is the wave's.
template <int RN, int RM, bool PAIRED>
__global__ void __launch_bounds__(64, 1) qp_replay_kernel(RParams rp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = (int)threadIdx.x;
  if ((uint32_t)(uintptr_t)lds != 0u) __builtin_trap();  // schedule byte addresses assume base 0
  double* v = lds;
  const KParams& p = rp.k;
  double* scr = p.scratch + (size_t)blockIdx.x * polish_row_doubles(p.pl.n, p.pl.m, p.pl.mv_slab, p.pl.nnzP);
  for (int inst = (int)blockIdx.x; inst < p.B; inst += (int)gridDim.x) {
    // attempted: what the tape marked, nothing of the handle's state
    if (__builtin_amdgcn_readfirstlane(rp.taped[inst]) == 0) {
      replay_zero_rows(rp, inst, lane);
      continue;
    }
    int ilane = lane;  // opaque per instance, as in the solve kernels (MPCQP_OPAQUE_LANE_RN)
    asm volatile("" : "+v"(ilane));
    replay_instance<RN, RM, PAIRED>(rp, inst, v, scr, ilane);
    LDS_FENCE();
  }
}

typedef void (*replay_fn)(RParams);
// the instantiation for the plan's register bucket and step kind, as select_adjoint chooses
replay_fn select_replay(int n, int m, bool paired) {
  int rn = 0, rm = 0;
  if (!kernel_bucket(n, m, rn, rm)) return nullptr;
  if (rn == 2) return paired ? qp_replay_kernel<2, 4, true> : qp_replay_kernel<2, 4, false>;
#if !defined(MPCQP_DEV20) && !defined(MPCQP_ONLY_SMALL)
  if (rn == 4) return paired ? qp_replay_kernel<4, 8, true> : qp_replay_kernel<4, 8, false>;
#endif
  return nullptr;
}
