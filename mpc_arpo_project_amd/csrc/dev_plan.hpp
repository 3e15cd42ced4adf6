// dev_plan.hpp -- the device image of a plan: the kernel's view of the structure tables (DevPlan,
// part of the kernel arguments) and the host builder that lays them out in one blob (host_abi.cpp).
// Plain C++, no HIP types: the host-only build lays out the same image on a CPU.
#pragma once
#include <utility>

#include "symbolic.hpp"

namespace mpcqp {

constexpr int TABLE_PAD_STEPS = 3;  // zero steps behind every schedule table (engine.hip table_rsrc)
constexpr int MREG_STEPS = 6;  // KM_MREG kernels (engine.hip): forward / backward steps at most
// compact step record: vector addresses of the 8 terms, then the 4 targets (3 rows of 64 lane quads)
constexpr int SOLVEC_STEP_WORDS = 3 * 64 * 4;
constexpr int SOLVEM_STEP_WORDS = 2 * 64 * 4;  // matrix addresses of the 8 terms (2 rows)

struct EllDev {
  const uint16_t *src, *in, *vpos, *sk;
  const uint32_t* pk;  // lane-major packed (vpos, in) terms of the used slots (symbolic.hpp Ell::pk)
  int K[ELL_MAXR], off[ELL_MAXR];
  int total, nlong;
  int long_out[ELL_MAXLONG], long_off[ELL_MAXLONG], long_cnt[ELL_MAXLONG];
};
struct DevPlan {
  EllDev eA, eAt, eP;  // residual mat-vecs (symbolic.hpp Ell)
  const uint32_t *fac, *tail, *fwd, *bwd;  // fixed-stride step records (symbolic.hpp)
  // KM_MREG kernels: the solve records split into vector-operand + target records (fwdc, bwdc) and
  // the matrix operands' LDS addresses (fwdm, bwdm), built on the host (build_dev_image)
  const uint32_t *fwdc, *bwdc, *fwdm, *bwdm;
  int nfac, ntail, nfwd, nbwd;
  const uint16_t* Lcol;    // DINV slot of each L entry's column
  int inst_doubles;        // LDS doubles of the instance image (16-byte aligned)
  const uint16_t *slotP, *slotA, *slotRho, *slotSig, *wsx, *wsz;
  const uint16_t *Ap, *Ai, *Acol, *Arp, *Ark, *Arj, *Pi, *Pcol, *Psp, *Psk, *Pso;
  int n, m, nk, nnzP, nnzA, nnzL;
  int LX, DINV, W, CACC, ZERO, ONE, MONE, LDS_N, S_P, S_A, S_DT, S_ET;
  int NKS;  // 64-lane slots of the padded 1/D, W and C regions (symbolic.hpp NKP / 64 = RN + RM)
  const uint32_t* wcopy;  // per lane: register slots whose W starts at the rhs (symbolic.hpp Plan::wcopy)
  const uint32_t* bcopy;  // per lane: diagonal-pass slots whose W starts at (1/D) W (Plan::bcopy)
  int S_ZERO;
  int MV, MVZ;  // resident scaled values [P | A] (CSC orders) and their zero slot
  int mv_slab;  // doubles of the per-wave slab holding them instead (Plan::mv_global), else 0
  const uint16_t *sra, *sca;  // lane-major row / column scaling slots (symbolic.hpp Plan::sra)
  int SJ;
  int XCH, XID;  // two-wave kernel: exchange slots and the handed-over instance id (Plan::XCH)
};

// Every table of a plan in one blob, the DevPlan's scalars, and where in the blob each of its table
// pointers has to point: null until rebase()
struct DevImage {
  std::vector<char> blob;
  DevPlan dp{};
  std::vector<std::pair<size_t, size_t>> fixups;  // byte offset of a pointer in dp, of its table in blob
  // the solve tables may run as one carried record pipeline (engine.hip RP_CARRY): a one-wave
  // LDS-operand plan whose forward and backward step counts are multiples of three and whose
  // look-ahead loads past either table read real steps of the other
  bool carry = false;
};
// Lays out pl's tables (mreg: with the KM_MREG record tables) and checks the plan against what the
// kernels assume of it: 0, or the MPCQP_E_* code of the failed check with its message in err.
int build_dev_image(const Plan& pl, bool mreg, DevImage& img, std::string& err);
// points img.dp at the copy of img.blob that starts at base (device memory, or the blob itself)
void rebase(DevImage& img, char* base);

}  // namespace mpcqp
