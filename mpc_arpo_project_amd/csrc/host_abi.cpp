// host_abi.cpp -- the host-only part of the C ABI (no HIP call): the calling thread's error
// message, default settings and status strings, the planner entry points -- symbolic analysis
// (mpcqp_analyze) and the CPU interpretation of the compiled device program
// (mpcqp_schedule_check) -- and the builder of a plan's device image (build_dev_image,
// dev_plan.hpp: the table blob mpcqp_create uploads, its DevPlan and the plan-consistency checks).
// Linked into libmpcqp.so with the HIP sources; built on its own with
// g++ -fsanitize=address,undefined together with symbolic.cpp, lds_layout.cpp and emulate.cpp for
// the sanitizer check of the host code (tests/test_sanitize.py).
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>

#include "dev_plan.hpp"
#include "host_abi.hpp"

namespace mpcqp {

namespace {
thread_local std::string g_err;
// block caps of the blocked substitution forced by MPCQP_CAPM / MPCQP_CAPW (diagnostics; 0: chosen
// per structure by build_plan_tuned)
int cap_m() { return diag_env_int("MPCQP_CAPM", 0); }
int cap_w() { return diag_env_int("MPCQP_CAPW", 0); }
// matrix operands of the solve steps read one step ahead (MPCQP_MATPF: 0 or 1; Plan::mat_first)
bool matrix_prefetch() { return diag_env_int("MPCQP_MATPF", 0) == 1; }
}  // namespace

int set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int check_settings_row(const mpcqp_settings& s, int row) {
  const std::string at = row >= 0 ? "row " + std::to_string(row) + ": " : "";
  if (s.polish) return set_error(MPCQP_E_UNSUPPORTED, at + "polish is not implemented in this build");
  if (s.scaled_termination)
    return set_error(MPCQP_E_UNSUPPORTED, at + "scaled_termination is not implemented in this build");
  if (s.max_iter <= 0 || s.alpha <= 0 || s.alpha >= 2 || s.sigma <= 0 || s.rho <= 0 ||
      s.scaling < 0 || s.check_termination < 0 || s.eps_abs < 0 || s.eps_rel < 0)
    return set_error(MPCQP_E_INVALID, at + "invalid settings");
  return 0;
}

// waves per instance of the solve kernel (MPCQP_WAVES: 1; 2 = two waves, solve steps split
// between them; 3 = two waves, solve steps on the first; unset or 0: chosen per structure by
// auto_waves; DESIGN.md, Two waves per instance)
int waves_per_instance() {
  const int w = diag_env_int("MPCQP_WAVES", 0);
  return (w == 1 || w == 2 || w == 3) ? w : 0;
}

// The automatic choice: two waves per instance with the solve steps on the first (3) when the
// one-wave image leaves at most two instances per CU -- then two of the CU's four SIMDs would idle,
// and the second wave takes half of the vector passes, checks and Ruiz passes onto them (N = 40:
// +8 % solves/s, profiles/r04/pair2); one wave otherwise (N = 20: four instances per CU, where the
// second wave's barriers cost more than its share saves: -4 %)
int auto_waves(const mpcqp_structure* st) {
  Plan p1;
  if (!build_plan_tuned(st->n, st->m, st->Pp, st->Pi, st->Ap, st->Ai, p1, cap_m(), cap_w(), 163840,
                        4, 1, false))
    return 1;
  const int bytes = ((p1.LDS_N + 1) & ~1) * 8;
  return 163840 / std::max(bytes, 1) <= 2 ? 3 : 1;
}

bool plan_for(const mpcqp_structure* st, Plan& pl) {
  const int w = waves_per_instance();
  return build_plan_tuned(st->n, st->m, st->Pp, st->Pi, st->Ap, st->Ai, pl, cap_m(), cap_w(), 163840,
                          4, w ? w : auto_waves(st), matrix_prefetch());
}

// ---- the device image (dev_plan.hpp) ---------------------------------------------------------
namespace {
// the KM_MREG record tables from the plan's solve records: per step, the terms' vector addresses
// (the operand in the W or C region) + the targets (SolveRecC), and the terms' matrix addresses
// (every other operand: L, N | G | G', ZERO / ONE / MONE); a padding term (both operands zero
// slots) reads its matrix zero from the first and its vector zero from the second
void split_records(const Plan& pl, const std::vector<uint32_t>& rec, int nsteps,
                   std::vector<uint32_t>& vec, std::vector<uint32_t>& mat) {
  auto is_vec = [&](uint32_t byte) {
    const int d = (int)(byte / 8u);
    return (d >= pl.W && d < pl.W + pl.NKP) || (d >= pl.CACC && d < pl.CACC + pl.NKP);
  };
  vec.assign((size_t)nsteps * SOLVEC_STEP_WORDS, 0u);
  mat.assign((size_t)nsteps * SOLVEM_STEP_WORDS, 0u);
  for (int st = 0; st < nsteps; ++st) {
    const uint32_t* r = rec.data() + (size_t)st * SOLVE_STEP_WORDS;
    uint32_t* cv = vec.data() + (size_t)st * SOLVEC_STEP_WORDS;
    uint32_t* cm = mat.data() + (size_t)st * SOLVEM_STEP_WORDS;
    for (int l = 0; l < 64; ++l) {
      for (int c = 0; c < SOLVE_MAXC; ++c) {
        // full record: row q = c / 2 holds lane quads (a_2q, b_2q, a_2q+1, b_2q+1)
        const uint32_t a = r[(c / 2) * 256 + l * 4 + (c % 2) * 2];
        const uint32_t b = r[(c / 2) * 256 + l * 4 + (c % 2) * 2 + 1];
        const bool av = is_vec(a);
        // compact rows: q = c / 4 holds lane quads of terms 4q..4q+3
        cv[(c / 4) * 256 + l * 4 + (c % 4)] = av ? a : b;
        cm[(c / 4) * 256 + l * 4 + (c % 4)] = av ? b : a;
      }
      for (int k = 0; k < 4; ++k) cv[2 * 256 + l * 4 + k] = r[SOLVE_TERM_WORDS + l * 4 + k];
    }
  }
}

// Appends tables to the blob and records where the DevPlan pointer named with each has to point.
// The order of the calls is the layout (which lines share L1 sets: DESIGN.md, Padded schedule tables)
struct ImageBuilder {
  DevImage& img;

  // v and zero_tail zero elements at the next 16-byte boundary, 16 zero bytes behind them
  template <typename T>
  size_t push(const std::vector<T>& v, size_t zero_tail = 0) {
    std::vector<char>& blob = img.blob;
    const size_t off = (blob.size() + 15) & ~size_t(15);
    blob.resize(off + (v.size() + zero_tail) * sizeof(T) + 16);  // resize zero-fills the tail
    if (!v.empty()) memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    return off;
  }
  template <typename T>
  void point(const T* const& field, size_t offset) {
    img.fixups.push_back({(size_t)((const char*)&field - (const char*)&img.dp), offset});
  }
  // pad_words: of a schedule table, the TABLE_PAD_STEPS zero steps behind it (table_rsrc)
  template <typename T>
  void put(const T*& field, const std::vector<T>& v, size_t pad_words = 0) {
    point(field, push(v, pad_words));
  }
  // Two tables that run one after the other (forward then backward solve; factorization then its
  // block-inverse tail), laid out as [A][B][the first TABLE_PAD_STEPS steps of A]: the record
  // pipelines' look-ahead loads past the end of A read B's first steps -- the very lines B's own
  // prefetch loads next, then L1 hits -- and B's read A's, which the next iteration loads.  The
  // restarting pipelines never execute what the look-ahead loads deliver, but a carried pipeline
  // (engine.hip RP_CARRY) does: its look-ahead sets past A are steps 0 and 1 of B's solve, and those
  // past B steps 0 and 1 of A's next one, so the copy behind B has to be A's steps (an A shorter
  // than the pad leaves zero steps there: build_dev_image then refuses the carry-over).  Measured
  // neutral on the N = 20 bench as a layout alone (945k vs 944k solves/s: the shared zero pads were
  // already L1-resident; DESIGN.md, Record traffic).
  void chain(const uint32_t*& fA, const uint32_t*& fB, const std::vector<uint32_t>& A,
             const std::vector<uint32_t>& B, int stride_words) {
    const size_t pad = (size_t)TABLE_PAD_STEPS * stride_words;
    std::vector<uint32_t> all(A);
    all.insert(all.end(), B.begin(), B.end());
    for (size_t k = 0; k < pad; ++k) all.push_back(k < A.size() ? A[k] : 0u);
    const size_t oA = push(all, pad);
    point(fA, oA);
    point(fB, oA + A.size() * sizeof(uint32_t));
  }
  // the residual mat-vecs: table by table across all of them (src and in of each, then every
  // vpos, every pk, every sk), then each one's scalars
  void ells(std::initializer_list<std::pair<EllDev*, const Ell*>> es) {
    for (auto [d, e] : es) put(d->src, e->src), put(d->in, e->in);
    for (auto [d, e] : es) put(d->vpos, e->vpos);
    for (auto [d, e] : es) put(d->pk, e->pk);
    for (auto [d, e] : es) put(d->sk, e->sk);
    for (auto [d, e] : es) {
      d->total = e->total, d->nlong = e->nlong;
      for (int r = 0; r < ELL_MAXR; ++r) d->K[r] = e->K[r], d->off[r] = e->off[r];
      for (int q = 0; q < ELL_MAXLONG; ++q)
        d->long_out[q] = e->long_out[q], d->long_off[q] = e->long_off[q], d->long_cnt[q] = e->long_cnt[q];
    }
  }
};
}  // namespace

int build_dev_image(const Plan& pl, bool mreg, DevImage& img, std::string& err) {
  auto refuse = [&](int code, const char* msg) { return err = msg, code; };
  // the kernel addresses C as W + NKP (an immediate offset): through W's slot plus the
  // compile-time distance 64 (RN + RM)
  if (pl.CACC - pl.W != pl.NKP)
    return refuse(MPCQP_E_UNSUPPORTED, "internal: accumulator region does not follow the solve vector");
  if (pl.nfac < 1 || pl.nfwd < 1 || pl.nbwd < 1) return refuse(MPCQP_E_UNSUPPORTED, "internal: empty schedule");
  if (pl.NKP != 64 * (pl.RN + pl.RM))
    return refuse(MPCQP_E_INVALID, "internal: C region not at the kernel's distance from W");
  if (pl.SJ > 8 * pl.RN)  // the kernel holds 8 RN row / column slots per lane (scale_problem)
    return refuse(MPCQP_E_UNSUPPORTED, "too many matrix values for the scaling registers");
  // the sequential sums stage their terms in the accumulator region C (NKP doubles, free during
  // the checks): a long mat-vec output's products per wave, the certificates' n / m terms
  for (const Ell* e : {&pl.ellA, &pl.ellAt, &pl.ellP}) {
    int tot = 0;  // a mat-vec stages all its long outputs at once (ell_apply)
    for (int L = 0; L < e->nlong; ++L) tot += e->long_cnt[L];
    if (tot > pl.NKP / pl.waves)
      return refuse(MPCQP_E_UNSUPPORTED, "internal: long mat-vec outputs exceed their staging");
  }

  img = DevImage{};
  memset(&img.dp, 0, sizeof img.dp);  // the padding too: a plan's image is the same bytes every time
  ImageBuilder b{img};
  DevPlan& dp = img.dp;
  b.chain(dp.fac, dp.tail, pl.fac, pl.tail, FAC_STEP_WORDS);
  b.chain(dp.fwd, dp.bwd, pl.fwd, pl.bwd, SOLVE_STEP_WORDS);
  // the carried record pipeline executes the look-ahead sets: both counts multiples of three (the
  // rotation then leaves them in the sets the next solve reads first), and no table shorter than
  // the pad, whose copy behind the backward table would be zero-filled
  img.carry = pl.waves == 1 && !pl.mat_first && !pl.mv_global && !mreg && pl.nfwd % 3 == 0 &&
              pl.nbwd % 3 == 0 && pl.nfwd >= TABLE_PAD_STEPS && pl.nbwd >= TABLE_PAD_STEPS;
  b.put(dp.Lcol, pl.Lcol);
  b.put(dp.slotP, pl.slotP), b.put(dp.slotA, pl.slotA);
  b.put(dp.slotRho, pl.slotRho), b.put(dp.slotSig, pl.slotSig);
  b.put(dp.wsx, pl.wsx), b.put(dp.wsz, pl.wsz);
  b.put(dp.Ap, pl.Ap), b.put(dp.Ai, pl.Ai), b.put(dp.Acol, pl.Acol);
  b.put(dp.Arp, pl.Arp), b.put(dp.Ark, pl.Ark), b.put(dp.Arj, pl.Arj);
  b.put(dp.Pi, pl.Pi), b.put(dp.Pcol, pl.Pcol);
  b.put(dp.Psp, pl.Psp), b.put(dp.Psk, pl.Psk), b.put(dp.Pso, pl.Pso);
  b.ells({{&dp.eA, &pl.ellA}, {&dp.eAt, &pl.ellAt}, {&dp.eP, &pl.ellP}});
  b.put(dp.sra, pl.sra), b.put(dp.sca, pl.sca);
  b.put(dp.wcopy, pl.wcopy);
  b.put(dp.bcopy, pl.bcopy);
  std::vector<uint32_t> fwdc, fwdm, bwdc, bwdm;  // empty unless mreg: the pads alone
  if (mreg) {
    split_records(pl, pl.fwd, pl.nfwd, fwdc, fwdm);
    split_records(pl, pl.bwd, pl.nbwd, bwdc, bwdm);
  }
  b.put(dp.fwdc, fwdc, TABLE_PAD_STEPS * SOLVEC_STEP_WORDS), b.put(dp.fwdm, fwdm);
  b.put(dp.bwdc, bwdc, TABLE_PAD_STEPS * SOLVEC_STEP_WORDS), b.put(dp.bwdm, bwdm);

  dp.nfac = pl.nfac, dp.ntail = pl.ntail, dp.nfwd = pl.nfwd, dp.nbwd = pl.nbwd;
  dp.inst_doubles = (pl.LDS_N + 1) & ~1;
  dp.n = pl.n, dp.m = pl.m, dp.nk = pl.nk, dp.nnzP = pl.nnzP, dp.nnzA = pl.nnzA;
  dp.nnzL = pl.nnzL;
  dp.LX = pl.LX, dp.DINV = pl.DINV, dp.W = pl.W, dp.CACC = pl.CACC, dp.ZERO = pl.ZERO;
  dp.ONE = pl.ONE, dp.MONE = pl.MONE, dp.LDS_N = pl.LDS_N, dp.NKS = pl.NKP / 64;
  dp.S_P = pl.S_P, dp.S_A = pl.S_A, dp.S_DT = pl.S_DT, dp.S_ET = pl.S_ET;
  dp.S_ZERO = pl.S_ZERO;
  dp.MV = pl.MV, dp.MVZ = pl.MVZ, dp.mv_slab = pl.mv_slab;
  dp.SJ = pl.SJ;
  dp.XCH = pl.XCH, dp.XID = pl.XID;
  return 0;
}

void rebase(DevImage& img, char* base) {
  for (const auto& [field, offset] : img.fixups) {
    const char* at = base + offset;
    memcpy((char*)&img.dp + field, &at, sizeof at);
  }
}

}  // namespace mpcqp

using namespace mpcqp;

extern "C" {

int mpcqp_version(void) { return 102; }
const char* mpcqp_last_error(void) { return g_err.c_str(); }

const char* mpcqp_status_string(int32_t st) {
  switch (st) {
    case MPCQP_SOLVED: return "solved";
    case MPCQP_SOLVED_INACCURATE: return "solved inaccurate";
    case MPCQP_PRIMAL_INFEASIBLE_INACCURATE: return "primal infeasible inaccurate";
    case MPCQP_DUAL_INFEASIBLE_INACCURATE: return "dual infeasible inaccurate";
    case MPCQP_MAX_ITER_REACHED: return "maximum iterations reached";
    case MPCQP_PRIMAL_INFEASIBLE: return "primal infeasible";
    case MPCQP_DUAL_INFEASIBLE: return "dual infeasible";
    case -5: return "interrupted";
    case -6: return "run time limit reached";
    case MPCQP_NON_CVX: return "problem non convex";
    case MPCQP_UNSOLVED: return "unsolved";
    default: return "unknown";
  }
}

int mpcqp_default_settings(mpcqp_settings* s) {
  if (!s) return set_error(MPCQP_E_INVALID, "null settings");
  s->rho = 0.1;
  s->sigma = 1e-06;
  s->alpha = 1.6;
  s->eps_abs = 1e-3;
  s->eps_rel = 1e-3;
  s->eps_prim_inf = 1e-4;
  s->eps_dual_inf = 1e-4;
  s->delta = 1e-6;
  s->adaptive_rho_tolerance = 5;
  s->max_iter = 4000;
  s->scaling = 10;
  s->adaptive_rho = 1;
  s->adaptive_rho_interval = 0;
  s->polish = 0;
  s->polish_refine_iter = 3;
  s->check_termination = 25;
  s->warm_start = 1;
  s->scaled_termination = 0;
  return 0;
}

int mpcqp_check_settings(const mpcqp_settings* rows, int32_t count) {
  if (!rows) return set_error(MPCQP_E_INVALID, "null settings");
  if (count <= 0) return set_error(MPCQP_E_INVALID, "invalid count");
  for (int32_t i = 0; i < count; ++i)
    if (int rc = check_settings_row(rows[i], i)) return rc;
  return 0;
}

int mpcqp_analyze(const mpcqp_structure* st, int32_t* perm, int32_t* Lp, int32_t* Li,
                  int32_t* nnzL, int32_t* stats) {
  if (!st || !nnzL) return set_error(MPCQP_E_INVALID, "null argument");
  Plan pl;
  if (!plan_for(st, pl)) return set_error(MPCQP_E_UNSUPPORTED, pl.error);
  const int cap = *nnzL;
  *nnzL = pl.nnzL;
  if (perm) std::copy(pl.perm.begin(), pl.perm.end(), perm);
  if (Lp) std::copy(pl.Lp.begin(), pl.Lp.end(), Lp);
  if (Li && cap >= pl.nnzL) std::copy(pl.Li.begin(), pl.Li.end(), Li);
  if (stats) {
    stats[0] = (int32_t)(pl.nfac + pl.ntail);
    stats[1] = (int32_t)pl.nfwd;
    stats[2] = (int32_t)pl.nbwd;
    stats[3] = pl.levels_fwd;
    stats[4] = pl.levels_bwd;
    stats[5] = pl.LDS_N * (int)sizeof(double);
  }
  return 0;
}

int mpcqp_schedule_check(const mpcqp_structure* st, const double* Px, const double* Ax,
                         double sigma, const double* rho_vec, const double* rhs, double* sol,
                         int64_t* model) {
  if (!st || !Px || !Ax || !rho_vec || !rhs || !sol) return set_error(MPCQP_E_INVALID, "null argument");
  Plan pl;  // the plan mpcqp_create would build (MPCQP_WAVES included)
  if (!plan_for(st, pl)) return set_error(MPCQP_E_UNSUPPORTED, pl.error);
  if (model) {
    const LdsModel md = model_lds(pl);
    model[0] = md.read, model[1] = md.atomic, model[2] = md.vec, model[3] = md.floor;
  }
  if (!emulate_kkt_solve(pl, Px, Ax, sigma, rho_vec, rhs, sol))
    return set_error(MPCQP_E_INVALID, "schedule emulation produced a non-finite or unzeroed slot, or changed a 1/D slot");
  return 0;
}

// The compiled device program's factorization and solves on the CPU, factor and solve apart (a
// KKT solver for the oracle's hybrid parity runs: tests/sweep_parity.py, DESIGN.md Parity)
struct mpcqp_emu {
  std::shared_ptr<const Plan> pl;  // shared by clones (read-only)
  std::vector<double> v;
  bool factored = false;
};

int mpcqp_emu_create(const mpcqp_structure* st, mpcqp_emu** out) {
  if (!st || !out) return set_error(MPCQP_E_INVALID, "null argument");
  *out = nullptr;
  auto pl = std::make_shared<Plan>();
  if (!plan_for(st, *pl)) return set_error(MPCQP_E_UNSUPPORTED, pl->error);
  mpcqp_emu* e = new mpcqp_emu();
  e->pl = pl;
  *out = e;
  return 0;
}

int mpcqp_emu_clone(const mpcqp_emu* src, mpcqp_emu** out) {
  if (!src || !out) return set_error(MPCQP_E_INVALID, "null argument");
  mpcqp_emu* e = new mpcqp_emu();
  e->pl = src->pl;
  *out = e;
  return 0;
}

int mpcqp_emu_destroy(mpcqp_emu* e) {
  delete e;
  return 0;
}

int mpcqp_emu_factor(mpcqp_emu* e, const double* Px, const double* Ax, double sigma,
                     const double* rho_vec) {
  if (!e || !Px || !Ax || !rho_vec) return set_error(MPCQP_E_INVALID, "null argument");
  emulate_factor(*e->pl, Px, Ax, sigma, rho_vec, e->v);
  e->factored = true;
  return 0;
}

int mpcqp_emu_solve(mpcqp_emu* e, const double* rhs, double* sol) {
  if (!e || !rhs || !sol) return set_error(MPCQP_E_INVALID, "null argument");
  if (!e->factored) return set_error(MPCQP_E_NODATA, "solve before factor");
  // a non-finite solution is returned as computed (ADMM on an infeasible problem may diverge)
  (void)emulate_solve(*e->pl, e->v, rhs, sol);
  return 0;
}

}  // extern "C"

#ifdef MPCQP_HOST_ONLY_BUILD
// marker of the host-only (sanitizer) build: mpc_arpo_project_amd/_lib.py then binds only the
// host entry points above; never defined in libmpcqp.so
extern "C" int mpcqp_host_only_build(void) { return 1; }
#endif
