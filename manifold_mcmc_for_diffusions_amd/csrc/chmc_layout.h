// The per-chain device arrays of a context, declared ONCE: for_each_chain_array states, per array, the pointer, the elements
// per chain, the trailing slack, whether chmc_create zeroes it and when it exists at all.  chmc_create allocates by walking
// this list, a half-batch view (set_half) advances every pointer of it to the half's first chain, and the arrays that are
// allocated on first use (ensure_array) take their size from it -- a new array, or a new shape, is edited here and nowhere
// else.  Plain host C++ (no device code, no HIP), included after chmc_core.h; tests/test_device_layout.py states the sizes on
// the CPU through tests/emu/layout_probe.cpp.  The shape comments of Slots and Work (chmc_core.h) repeat this list.
//
// Every array is chain-major: [B][elements per chain], chain c at offset c * (elements per chain).
//
// NOT in the list, because they are not per chain (a view shares them):
//   work.zeros [256], work.nfallback [128], work.ticket (null);
//   work.n_active [12] = [batch | half 0 | half 1] x 4 round slots: the view of half h counts in slots 4 (1 + h) ..;
//   d_y [T] (the observations every chain shares until chmc_set_observations: the per-chain d_yc IS in the list),
//   d_m0 [3 U U + 1] (the block metric every chain shares until chmc_set_metrics: the per-chain d_m0c IS in the list), the block tables d_blk / d_obs2blk / d_blk_full and the work orders d_order / d_order_half /
//   d_order_ident (a view takes its half's order);
//   d_ham [B][4] ([B][3] Hamiltonian terms, or [B] values + [B][3] statistics: not chain-major) and the arrays of the
//   trajectory trees (TreeState, d_tree_*) and the scratch of chmc_gd_objective_device (d_gd), which only whole-batch launches use.
#pragma once
#include <cstddef>
#include "chmc_plan.h"

namespace chmc {

// What a kernel launch sees of a context: the three argument blocks and the per-chain arrays the host hands to kernels one
// by one.  A context IS its whole-batch view (chmc_ctx derives from this); a half-batch view is a copy with every per-chain
// pointer advanced and B = the half's chain count.
struct ChainView {
  Sys sy;
  Slots sl;
  Work w;
  double* d_xobs;          // [B][T][X] Sys::xobs, writable
  int* d_act;              // [B] the step's mask of active chains
  int *d_itf, *d_itb;      // [B] iterations of a step's forward / reverse retraction (inside d_out: alias_step_outputs)
  // allocated on first use (ensure_array):
  double *d_q0, *d_p0;     // [B][Q] n_inner_step > 1: the step's start state (restored when a later inner step fails)
  int* d_ncommit;          // [B] inner steps a chain has completed in the current step
  double *d_qbak, *d_pbak; // [B][Q] chmc_snapshot
  int *d_nsteps, *d_ndone; // [B] per-chain trajectory lengths / steps done (k_traj_chain)
  // allocated by chmc_set_observations only (null, and kAbsent in the list, until then):
  double* d_yc = nullptr;    // [B][T] per-chain observations: Sys::y with Sys::ystride = T
  double* d_sigc = nullptr;  // [B] per-chain fixed observation-noise std: Sys::sigc
  // allocated by chmc_set_metrics only:
  double* d_m0c = nullptr;   // [B][3 U U + 1] per-chain M_0, M_0^-1, chol(M_0), log det(M_0) / 2: Sys::m0 with Sys::m0stride = 3 U U + 1
};

enum ChainArrayKind {
  kPlain = 0,
  kZeroed = 1,  // chmc_create zeroes it
  kLazy = 2,    // null until ensure_array
  kAbsent = 4   // this context does not have it: null
};

// f(pointer, elements per chain, kind, slack): the allocation holds B * (elements per chain) + slack elements.
template <class F>
void for_each_chain_array(ChainView& v, const KernelPlan& plan, size_t npart, F&& f) {
  const Sys& sy = v.sy;
  Slots& sl = v.sl;
  Work& w = v.w;
  const size_t Q = sy.Q, KM = sy.Kmax, RM = sy.RM, U = sy.U, X = sy.X, Z = sy.Z, NV = sy.NV, TRJ = sy.TRJ;
  const size_t steps = (size_t)sy.T * sy.S, ivls = KM * sy.NOBS;  // time steps / observation intervals (padded) per chain
  auto arr = [&](auto*& p, size_t per_chain, int kind = kPlain, size_t slack = 0) { f(p, per_chain, kind, slack); };
  auto only = [](bool exists, int kind = kPlain) { return exists ? kind : (int)kAbsent; };
  // compact form of the stored rows (chmc_core.h, Slots) and the interval sums of the sweeps over it
  const bool pb = plan.pb_allocated;
  // rows of the Newton iterate: 16-row blocks; blocks of at most 8 rows with the MFMA Gram kernel
  const bool jvw = RM > 8 || plan.rows == RowsStoredMfma;

  arr(v.d_xobs, sy.T * X, kZeroed);
  for (int s = 0; s < 2; ++s) {
    arr(sl.q[s], Q, kZeroed, CHMC_Q_PAD), arr(sl.p[s], Q, kZeroed), arr(sl.grad[s], Q, kZeroed), arr(sl.pg[s], Q);
    arr(sl.traj[s], TRJ);
    arr(sl.JuP[s], KM * RM * U), arr(sl.E[s], KM * RM * U);
    arr(sl.Jv[s], RM * NV, kZeroed);
    arr(sl.facD[s], KM * RM * RM);
    arr(sl.facC[s], U * U), arr(sl.Cinv[s], U * U);
    arr(sl.ldb[s], KM), arr(sl.logdet[s], 1);
    arr(sl.PB[s], steps * X * sy.V, only(pb, kZeroed)), arr(sl.LF[s], ivls * RM * X, only(pb, kZeroed));
  }
  arr(w.muF, ivls * X, only(pb)), arr(w.muF2, ivls * X, only(pb));
  arr(w.ivl, ivls * (2 * X * X + X * Z), only(pb));
  arr(w.gcq, ivls * (2 * X * X + X * Z), only(pb && RM > 8)), arr(w.gbw, ivls * (X + 2 * Z), only(pb && RM > 8));
  arr(sl.cur, 1, kZeroed);
  arr(w.trajw, TRJ);
  arr(w.cpad, KM * RM, kZeroed), arr(w.tpad, KM * RM), arr(w.lampad, KM * RM, kZeroed);
  arr(w.cpad2, KM * RM, kZeroed), arr(w.lampad2, KM * RM, kZeroed);
  arr(w.Ew, KM * RM * U), arr(w.Cb, KM * U * U);
  arr(w.sb, KM * U), arr(w.gup, KM * U);
  arr(w.Dw, KM * RM * RM), arr(w.JuL, KM * RM * U);
  arr(w.JvW, RM * NV, only(jvw, kZeroed));
  arr(w.zbP, KM * RM * Z), arr(w.gMb, KM * RM * RM);
  arr(w.gzd, KM * RM * Z), arr(w.gWu, KM * RM * U);
  arr(w.gxdt, KM * RM * X);
  arr(w.sdt, 1, kZeroed), arr(w.cdt, 1, kZeroed);
  arr(w.mu, Q), arr(w.qb, Q, kZeroed, CHMC_Q_PAD), arr(w.pb, Q), arr(w.vin, Q);
  arr(w.Xd, steps * RM * X);
  arr(w.err, 1), arr(w.dt, 1, kZeroed);
  arr(w.ndq, 1);
  arr(w.part, npart * 2);
  arr(w.iters, 1), arr(w.nw, 1), arr(w.ok, 1), arr(w.nstat, 1);
  arr(v.d_act, 1);
  arr(v.d_q0, Q, kLazy), arr(v.d_p0, Q, kLazy), arr(v.d_ncommit, 1, kLazy);
  arr(v.d_qbak, Q, kLazy), arr(v.d_pbak, Q, kLazy);
  arr(v.d_nsteps, 1, kLazy), arr(v.d_ndone, 1, kLazy);
  // per-chain data: no context has them at chmc_create; chmc_set_observations allocates them, and from then on a view
  // advances them like every other array of the list
  arr(v.d_yc, sy.T, only(v.d_yc != nullptr)), arr(v.d_sigc, 1, only(v.d_sigc != nullptr));
  // per-chain block metrics, likewise: chmc_set_metrics allocates the tables
  arr(v.d_m0c, 3 * U * U + 1, only(v.d_m0c != nullptr));
}

// The per-step outputs of chmc_leapfrog_step live in ONE allocation (chmc_ctx::d_out) so that they cross PCIe in a single
// copy: [rev (8 B) | status | iters_fwd | iters_bwd] x B.  The four pointers into it are aliases, not allocations: section by
// section they are chain-major like everything above, so the view that starts at chain c0 is each section's start + c0.
inline size_t step_outputs_words(size_t B) { return B + (3 * B * sizeof(int) + 7) / 8; }  // in 8-byte words
inline void alias_step_outputs(ChainView& v, unsigned long long* out, size_t B, size_t c0) {
  int* const status = reinterpret_cast<int*>(out + B);
  v.w.rev = out + c0, v.w.status = status + c0, v.d_itf = status + B + c0, v.d_itb = status + 2 * B + c0;
}

}  // namespace chmc
