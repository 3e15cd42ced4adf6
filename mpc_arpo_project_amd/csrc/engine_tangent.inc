// engine_tangent.inc -- forward sensitivities (tangents) of a batch's solved instances on the
// device (included by engine.hip inside its anonymous namespace, after engine_adjoint.inc; it uses
// the shared device helpers and engine_polish.inc's PolishDrift / polish_row_doubles, and edits none
// of them: the solve, polish and adjoint kernels keep their code).
//
// At a solution with active rows act a perturbation (dq, dl, du, dA, dP) of the data moves it by
//   K [dx; dy_act] = [-(dq + dP x + dA' y); (db - dA x)_act],  K = [P A_act'; A_act 0],
// db_i = dl_i on lower-active rows, du_i on upper-active ones, dy = 0 off act: the adjoint's
// symmetric K with a right-hand side that is assembled here from the perturbation itself.  In the
// engine's scaled space (x = D xs, y = E ys / c, Ps = c D P D, As = E A D) the right-hand side takes
// the adjoint's form [c D r_x; E r_y], and dx = D dsx, dy = E dsy / c -- no square root appears.
//
// One wave per instance at every horizon, as the polish and the adjoint.  Per instance (DESIGN.md,
// Forward sensitivities):
//   1.-3. the adjoint's steps, restated: the last scaling again into the wave's sink, the active words
//      of the carried xs, zs, ys (written out as `act`), the reduced KKT with +-delta on the
//      handle's compiled program, factorized ONCE;
//   4. the direction loop, the kernel's own design point.  The W and C regions of the image are
//      rewritten whole by every solve, so per direction the unscaled x and y (y zeroed off act) are
//      staged again, from the caller's own rows -- read-only, so they serve as the per-instance copy a
//      scratch slab would hold, without the copy and without the 12 (2, 4) / 24 (4, 8) registers
//      a register-held copy costs -- into the W region, and the n + m accumulators are zeroed in
//      the C region.  One lane-strided pass over P's nonzeros and one over A's read dPx / dAx
//      coalesced from global memory exactly once and add dP x, dA' y_act, dA x to the accumulators
//      with LDS atomics (rows and columns collide across lanes); the sums are scaled into registers.
//      Round 0 plus `refine` refinement rounds as the adjoint's; the pass after the last round, which
//      has As dsx and Ps dsx in registers for the residual, also gives dz = A dx + dA x (dA x waits
//      in the lane's own dz row) and dobj.  No right-hand side passes through global memory.
// The accumulation order: a wave's LDS atomics of one instruction are applied in lane order and its
// LDS instructions in issue order (the solve steps rest on both, and the CPU interpretation of the
// device program reproduces them bitwise: emulate.cpp), one wave owns the image, and the passes' trip
// order is fixed -- so the sums, and with them every output, are bitwise the same in every launch.
// Nothing a later solve, polish or adjoint reads is written.

// The tangent kernel's arguments: the solve kernels' (embedded, so the shared device functions take
// them as they are; k.x_out / k.y_out unused) and its own.  KParams and DevPlan keep their layout.
struct TParams {
  KParams k;              // k.scratch: [grid][polish_row_doubles]
  const int32_t* status;  // [B] the status the solve wrote
  const double *x, *y;    // [B][n], [B][m] the unscaled solution: read, never written
  mpcqp_tangent_in in;
  mpcqp_tangent_out out;
};

// an instance that is not attempted: zeros in every requested row
__device__ __forceinline__ void tangent_zero_rows(const TParams& tp, int inst, int lane) {
  const DevPlan& P = tp.k.pl;
  const mpcqp_tangent_out& o = tp.out;
  for (int k = 0; k < tp.in.ndir; ++k) {
    const size_t row = (size_t)k * tp.k.B + inst;
    for (int j = lane; j < P.n; j += 64)
      if (o.dx) o.dx[row * P.n + j] = 0.0;
    for (int i = lane; i < P.m; i += 64) {
      if (o.dy) o.dy[row * P.m + i] = 0.0;
      if (o.dz) o.dz[row * P.m + i] = 0.0;
    }
    if (lane == 0 && o.dobj) o.dobj[row] = 0.0;
    if (lane == 0 && o.res) o.res[row] = 0.0;
  }
  if (o.act)
    for (int i = lane; i < P.m; i += 64) o.act[(size_t)inst * P.m + i] = 0;
  if (lane == 0 && o.status_tangent) o.status_tangent[inst] = 0;
}

template <int RN, int RM, bool PAIRED>
__device__ __forceinline__ void tangent_instance(const TParams& tp, int inst, double* v, double* scr,
                                                 int lane) {
  const KParams& p = tp.k;
  const DevPlan& P = p.pl;
  const mpcqp_tangent_in& in = tp.in;
  const mpcqp_tangent_out& o = tp.out;
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
  const double* qu;  // the unscaled q that scaling started from (dobj)
  {
    const int sel = __builtin_amdgcn_readfirstlane(p.dsel[inst]);  // -1, 0 or 1 after a solve
    PolishDrift dr;
    dr.P_in = sel < 0 ? setup_row(p.Px, p.Px_stride, inst) : drift_row(p.Pw, sel, p.B, P.nnzP, inst);
    dr.q_in = sel < 0 ? setup_row(p.q, p.q_stride, inst) : drift_row(p.qw, sel, p.B, n, inst);
    dr.P_sink = sink, dr.q_sink = sink + P.nnzP;
    qu = dr.q_in;
    double D[RN], E[RM];
    scale_problem(p, inst, dr, S, v, W, D, E TACC_ARG);
    scale_finish(p, inst, false, S, sb, v, mv, W, D, E);
  }
  // ---------------- 2. active sets (form_Ared) of the carried iterates: bit r = row lane + 64 r
  uint32_t low = 0, upp = 0;
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    const int i = lane + 64 * r;
    const bool inr = i < m;
    const double z = inr ? p.zs[(size_t)inst * m + i] : 0.0;
    const double y = inr ? p.ys[(size_t)inst * m + i] : 0.0;
    const bool lo = inr && z - S.l[r] < -y;
    const bool up = inr && S.u[r] - z < y;
    low |= (lo ? 1u : 0u) << r, upp |= (up ? 1u : 0u) << r;
    if (inr && o.act) o.act[(size_t)inst * m + i] = lo ? (int8_t)-1 : (up ? (int8_t)1 : (int8_t)0);
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
  // ---------------- 4. the directions
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
  const int refine = in.refine;
  // The assembly's staging over the W and C regions (2 NKP >= 2 (n + m) doubles, contiguous:
  // build_dev_image): x, y_act, then the accumulators of r_x (n) and dA x (m).  Both regions hold a
  // solve's work vectors only while it runs: the previous direction's last pass has read its
  // staged iterate (xb, yb below) and its long outputs' staging into registers before this one
  // stages, and round 0 rewrites W and C whole from registers after the accumulators are read.
  double* const xb = v + P.W;
  double* const yb = xb + n;  // y_act; in the refinement the dual iterate (past m: W padding)
  const int accx = P.W + n + m, accy = accx + n;  // image indices of the two accumulators
#pragma unroll 1
  for (int k = 0; k < in.ndir; ++k) {
    const size_t row = (size_t)k * p.B + inst;
    // ---- the right-hand side: -(dq + dP x + dA' y_act) and (db - dA x) on the active rows
    LDS_FENCE();
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = lane + 64 * r;
      if (j < n) xb[j] = tp.x[(size_t)inst * n + j], v[accx + j] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      if (i < m) yb[i] = ((act >> r) & 1u) ? tp.y[(size_t)inst * m + i] : 0.0, v[accy + i] = 0.0;
    }
    LDS_FENCE();
    double dob = 0.0;  // the lane's part of x' dP x / 2 + dq' x
    if (in.dPx)
      for (int e = lane; e < P.nnzP; e += 64) {  // both halves of an off-diagonal entry
        const int i = P.Pi[e], j = P.Pcol[e];
        const double d = in.dPx[row * P.nnzP + e];
        const double xi = xb[i], xj = xb[j];
        lds_add((uint32_t)(accx + i) * 8u, d * xj);
        if (i != j) lds_add((uint32_t)(accx + j) * 8u, d * xi);
        dob += (i == j) ? .5 * d * xi * xi : d * xi * xj;
      }
    if (in.dAx) {
#pragma unroll
      for (int jj = 0; jj < 8 * RN; ++jj) {
        if (64 * jj >= P.nnzA) break;  // wave-uniform
        const int e = 64 * jj + lane;
        if (e < P.nnzA) {
          const int i = P.Ai[e], j = P.Acol[e];
          const double d = in.dAx[row * P.nnzA + e];
          lds_add((uint32_t)(accy + i) * 8u, d * xb[j]);                             // dA x, every row
          if ((amask >> jj) & 1u) lds_add((uint32_t)(accx + j) * 8u, d * yb[i]);  // dA' y_act
        }
      }
    }
    LDS_FENCE();
    // scaled [c D r_x; E r_y] into registers, its inf-norm; dA x waits in the dz row for A dx
    double bx[RN], bz[RM], sx[RN], sy[RM];
    double bn = 0.0;
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = lane + 64 * r;
      double t = 0.0;
      if (j < n) {
        const double dq = in.dq ? in.dq[row * n + j] : 0.0;
        dob += dq * xb[j];
        t = -(dq + v[accx + j]);
      }
      bx[r] = j < n ? (S.c * sb.D[j]) * t : 0.0;
      sx[r] = 0.0;
      bn = dmaxd(bn, fabs(bx[r]));
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      const double dax = i < m ? v[accy + i] : 0.0;
      if (i < m && o.dz) o.dz[row * m + i] = dax;
      double db = 0.0;
      if (in.dl && ((low >> r) & 1u)) db = in.dl[row * m + i];
      if (in.du && ((upp >> r) & 1u) && !((low >> r) & 1u)) db = in.du[row * m + i];
      bz[r] = ((act >> r) & 1u) ? sb.E[i] * (db - dax) : 0.0;
      sy[r] = 0.0;
      bn = dmaxd(bn, fabs(bz[r]));
    }
    bn = wave_max(bn);
    // ---- round 0 solves the right-hand side itself; round it >= 1 solves the residual against
    // [P A_act'; A_act 0] and adds; the pass after the last round takes the residual's norm and,
    // from the same products, dz and dobj
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
        if (it > refine) {  // wave-uniform
#pragma unroll
          for (int r = 0; r < RN; ++r) rn = dmaxd(rn, fabs(rx[r]));
#pragma unroll
          for (int r = 0; r < RM; ++r) rn = dmaxd(rn, fabs(rz[r]));
          rn = wave_max(rn);
          // dz = A dx + dA x: As dsx = E A dx.  dobj: (P x + q)' dx = xs' Ps dsx / c + q' dx
          if (o.dz) {
#pragma unroll
            for (int r = 0; r < RM; ++r) {
              const int i = lane + 64 * r;
              if (i < m) o.dz[row * m + i] += ax[r] / sb.E[i];  // the lane's own store above
            }
          }
          if (o.dobj) {
            double part = 0.0;
#pragma unroll
            for (int r = 0; r < RN; ++r) {
              const int j = lane + 64 * r;
              if (j < n) {
                const double Dj = sb.D[j];
                part += ((tp.x[(size_t)inst * n + j] / Dj) * px[r]) * S.cinv + qu[j] * (Dj * sx[r]);
              }
            }
            const double tot = wave_sum(dob + part);
            if (lane == 0) o.dobj[row] = tot;
          }
          break;
        }
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
    // unscale (dx = D dsx, dy = E dsy / c) straight from registers
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = lane + 64 * r;
      if (j < n && o.dx) o.dx[row * n + j] = sb.D[j] * sx[r];
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const int i = lane + 64 * r;
      if (i < m && o.dy) o.dy[row * m + i] = (sb.E[i] * sy[r]) * S.cinv;  // 0 off the active rows
    }
  }
  if (lane == 0 && o.status_tangent) o.status_tangent[inst] = 1;
}

// One wave per workgroup on a persistent grid, instances by a grid-stride loop (a tangent costs the
// same for every instance: no work counter); the instance image is the workgroup's whole dynamic
// LDS at address 0, the scratch row is the wave's.
template <int RN, int RM, bool PAIRED>
__global__ void __launch_bounds__(64, 1) qp_tangent_kernel(TParams tp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = (int)threadIdx.x;
  if ((uint32_t)(uintptr_t)lds != 0u) __builtin_trap();  // schedule byte addresses assume base 0
  double* v = lds;
  const KParams& p = tp.k;
  double* scr = p.scratch + (size_t)blockIdx.x * polish_row_doubles(p.pl.n, p.pl.m, p.pl.mv_slab, p.pl.nnzP);
  for (int inst = (int)blockIdx.x; inst < p.B; inst += (int)gridDim.x) {
    // attempted: solved, not skipped, carrying that solve's state (the polish's rule)
    const bool go = __builtin_amdgcn_readfirstlane(tp.status[inst]) == MPCQP_SOLVED &&
                    !(p.skip && __builtin_amdgcn_readfirstlane(p.skip[inst]) != 0) &&
                    __builtin_amdgcn_readfirstlane(p.has_state[inst]) == 1 &&
                    __builtin_amdgcn_readfirstlane(p.dsel[inst]) >= -1;
    if (!go) {
      tangent_zero_rows(tp, inst, lane);
      continue;
    }
    int ilane = lane;  // opaque per instance, as in the solve kernels (MPCQP_OPAQUE_LANE_RN)
    asm volatile("" : "+v"(ilane));
    tangent_instance<RN, RM, PAIRED>(tp, inst, v, scr, ilane);
    LDS_FENCE();
  }
}

typedef void (*tangent_fn)(TParams);
// the instantiation for the plan's register bucket and step kind, as select_polish chooses
tangent_fn select_tangent(int n, int m, bool paired) {
  int rn = 0, rm = 0;
  if (!kernel_bucket(n, m, rn, rm)) return nullptr;
  if (rn == 2) return paired ? qp_tangent_kernel<2, 4, true> : qp_tangent_kernel<2, 4, false>;
#if !defined(MPCQP_DEV20) && !defined(MPCQP_ONLY_SMALL)
  if (rn == 4) return paired ? qp_tangent_kernel<4, 8, true> : qp_tangent_kernel<4, 8, false>;
#endif
  return nullptr;
}
