// Wave-level kernels for gfx950: one 64-lane wavefront per (chain, block).
//
// The adjoint recurrence behind the constraint Jacobian (jacob_constr_blocks, sde/mici_extensions.py:521-624)
//     Lam^(s) = Lam^(s+1) A_s,   dc/dv_s = Lam^(s+1) B_s,   dc/dz += Lam^(s+1) Zf_s
// is linear in Lam, so a tile of 64 consecutive time steps is processed by the 64 lanes at once:
//   * lane l loads x_s, v_s of one step of the tile (unit-stride, 16 B per lane: fully coalesced; later steps in lower
//     lanes), evaluates its own A_s, B_s, Zf_s,
//   * a prefix scan over the lanes on the DPP path of the vector ALU forms the product of the later transition matrices
//     of the tile (dpp_prefix_products below),
//   * inside an observation interval every adjoint row is the interval's FRAME (the rows at its end, wave-uniform) times
//     that row-independent product, so the per-lane work carries no row index: X x Z, X x X running sums, the compact
//     form PB_s = P_f E_s B_s of the step's Jacobian rows, and the RM-sized products once per interval (k_state_lean:
//     state evaluation; k_newton_ivl / k_newton_comb: Newton iteration and state evaluation in two phases;
//     k_rev_wave: the round-1 formulation with the rows in registers, kept for 16-row blocks and as a fallback),
//   * the passes over a stored Jacobian (J w, J^T lambda, Gram contraction, grad-log-det weights) read the compact rows
//     (Slots::PB / LF, chmc_core.h).
// Compared with one lane per block this turns scattered 16-byte loads per step per lane into 1 KB contiguous wave loads
// and gives 64x more lanes of parallelism; DESIGN.md section 4 has the measurements.
#pragma once
#include <type_traits>
#include "chmc_core.h"

namespace chmc {

// Trajectories are streamed: written once by the forward scan (non-temporal stores) and read once per sweep.  A
// plain read leaves the lines allocated in L2 / Infinity Cache and the next scan's streaming stores to the same
// addresses then run at half speed (tools/ubench/fwd_latency.hip: 107 us vs 187 us per scan), so the readers use
// the non-temporal hint as well.
#ifdef CHMC_PLAIN_STREAM  // (A/B build: plain loads instead of the streaming hint on the once-per-sweep operands; measured in
                          // round 4 at configs[1]: 47.8 k against 49.7 k steps/s, the forward scan 134 -> 150 us beside the fuller caches)
__device__ inline double ld_stream(const double* p) { return *p; }
#else
__device__ inline double ld_stream(const double* p) { return __builtin_nontemporal_load(p); }
#endif

// Stores the compiler does not see.  With one of its own stores pending, hipcc (ROCm 7.2) waits for vmcnt(0) at the
// next use of a prefetched value, i.e. for the store acknowledgement, every tile.  A store issued through inline asm
// is not tracked, so the waits for the prefetched loads keep their counts (which stay valid: an untracked younger
// store only makes a counted wait retire more).  The trailing s_nop covers the wait states the hazard recogniser would
// insert between a wide store and a VALU write of its data registers.
__device__ __forceinline__ void st_async(double* p, double v) {
  asm volatile("global_store_dwordx2 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st_async2(double* p, double v0, double v1) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  const d2v v = {v0, v1};
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}

__device__ inline double bcast0(double x) {  // value of lane 0, as a wave-uniform value
  union { double d; int i[2]; } u;
  u.d = x;
  u.i[0] = __builtin_amdgcn_readfirstlane(u.i[0]);
  u.i[1] = __builtin_amdgcn_readfirstlane(u.i[1]);
  return u.d;
}

// Cross-lane moves through the DPP path of the vector ALU (no LDS crossbar, no lgkmcnt wait): dst lane <- src lane as
// the control word says, lanes without a source (row boundaries, masked rows / banks) receive `old`.
//   row_shr:n = 0x110 + n (shift right by n inside each row of 16 lanes), wave_shr:1 = 0x138,
//   row_bcast:15 = 0x142 (lane 15 of each row to the next row), row_bcast:31 = 0x143 (lane 31 to rows 2 and 3)
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_mov(double x, double old) {
  union { double d; int i[2]; } u, o;
  u.d = x, o.d = old;
  u.i[0] = __builtin_amdgcn_update_dpp(o.i[0], u.i[0], CTRL, ROW_MASK, BANK_MASK, false);
  u.i[1] = __builtin_amdgcn_update_dpp(o.i[1], u.i[1], CTRL, ROW_MASK, BANK_MASK, false);
  return u.d;
}
__device__ inline double bcast_lane63(double x) {  // value of lane 63, as a wave-uniform value
  union { double d; int i[2]; } u;
  u.d = x;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], 63);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], 63);
  return u.d;
}

template <int X>
__device__ inline void matmul_xx(const double* a, const double* b, double* c) {  // c = a b (X x X)
#pragma unroll
  for (int i = 0; i < X; ++i)
#pragma unroll
    for (int j = 0; j < X; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < X; ++k) t += a[i * X + k] * b[k * X + j];
      c[i * X + j] = t;
    }
}

// Inclusive PREFIX product over the 64 lanes, lower lanes on the left: P_l = A_0 A_1 ... A_l, in seven DPP steps (the
// classic row_shr 1 / 2 / 3, row_shr 4 / 8 with bank masks, row_bcast 15 / 31 sequence).  Lanes without a source get the
// identity, so every step is an unconditional matrix product.  On return P holds the inclusive products; E (optional)
// the exclusive ones (identity in lane 0).
template <int X, int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ void dpp_scan_step(double* P, const double* src) {
  double Y[X * X], Pn[X * X];
#pragma unroll
  for (int i = 0; i < X * X; ++i) Y[i] = dpp_mov<CTRL, ROW_MASK, BANK_MASK>(src[i], (i / X == i % X) ? 1.0 : 0.0);
  matmul_xx<X>(Y, P, Pn);
#pragma unroll
  for (int i = 0; i < X * X; ++i) P[i] = Pn[i];
}
template <int X>
__device__ __forceinline__ void dpp_prefix_products(const double* A, double* P, double* E) {
#pragma unroll
  for (int i = 0; i < X * X; ++i) P[i] = A[i];
  dpp_scan_step<X, 0x111, 0xf, 0xf>(P, A);  // row_shr:1 of the ORIGINAL values
  dpp_scan_step<X, 0x112, 0xf, 0xf>(P, A);  // row_shr:2
  dpp_scan_step<X, 0x113, 0xf, 0xf>(P, A);  // row_shr:3
  dpp_scan_step<X, 0x114, 0xf, 0xe>(P, P);  // row_shr:4, banks 1-3
  dpp_scan_step<X, 0x118, 0xf, 0xc>(P, P);  // row_shr:8, banks 2-3
  dpp_scan_step<X, 0x142, 0xa, 0xf>(P, P);  // row_bcast:15, rows 1 and 3
  dpp_scan_step<X, 0x143, 0xc, 0xf>(P, P);  // row_bcast:31, rows 2 and 3
  if (E) {
#pragma unroll
    for (int i = 0; i < X * X; ++i) E[i] = dpp_mov<0x138, 0xf, 0xf>(P[i], (i / X == i % X) ? 1.0 : 0.0);  // wave_shr:1
  }
}

// One DPP step of an inclusive AFFINE prefix scan: every lane holds the map x -> P x + e_i (NE vectors e_i of length X
// share the matrix P); the step composes the lane's accumulated map AFTER the map fetched from a lower lane,
//     P <- P Pl,   e_i <- P el_i + e_i.
// Lanes without a source receive the identity map (Pl = I, el = 0), so the step is unconditional.  srcP / srce: the
// values that are shifted (the ORIGINAL maps in the row_shr 1 / 2 / 3 steps, the accumulated ones afterwards).
template <int X, int NE, int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ void dpp_affine_step(double* P, double* e, const double* srcP, const double* srce) {
  double Pl[X * X], Pn[X * X];
#pragma unroll
  for (int i = 0; i < X * X; ++i) Pl[i] = dpp_mov<CTRL, ROW_MASK, BANK_MASK>(srcP[i], (i / X == i % X) ? 1.0 : 0.0);
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    double el[X];
#pragma unroll
    for (int d = 0; d < X; ++d) el[d] = dpp_mov<CTRL, ROW_MASK, BANK_MASK>(srce[i * X + d], 0.0);
#pragma unroll
    for (int a = 0; a < X; ++a) {
      double tt = e[i * X + a];
#pragma unroll
      for (int d = 0; d < X; ++d) tt += P[a * X + d] * el[d];
      e[i * X + a] = tt;
    }
  }
  matmul_xx<X>(P, Pl, Pn);
#pragma unroll
  for (int i = 0; i < X * X; ++i) P[i] = Pn[i];
}
template <int X, int NE>
__device__ __forceinline__ void dpp_affine_prefix(double* P, double* e) {
  double P0[X * X], e0[NE * X];
#pragma unroll
  for (int i = 0; i < X * X; ++i) P0[i] = P[i];
#pragma unroll
  for (int i = 0; i < NE * X; ++i) e0[i] = e[i];
  dpp_affine_step<X, NE, 0x111, 0xf, 0xf>(P, e, P0, e0);  // row_shr:1 of the ORIGINAL maps
  dpp_affine_step<X, NE, 0x112, 0xf, 0xf>(P, e, P0, e0);  // row_shr:2
  dpp_affine_step<X, NE, 0x113, 0xf, 0xf>(P, e, P0, e0);  // row_shr:3
  dpp_affine_step<X, NE, 0x114, 0xf, 0xe>(P, e, P, e);    // row_shr:4, banks 1-3
  dpp_affine_step<X, NE, 0x118, 0xf, 0xc>(P, e, P, e);    // row_shr:8, banks 2-3
  dpp_affine_step<X, NE, 0x142, 0xa, 0xf>(P, e, P, e);    // row_bcast:15, rows 1 and 3
  dpp_affine_step<X, NE, 0x143, 0xc, 0xf>(P, e, P, e);    // row_bcast:31, rows 2 and 3
}

// Joint prefix scan of (matrix, row vector) pairs for the recurrence  xbar <- xbar A + h  (later steps in lower lanes):
// every lane holds the map  xbar -> xbar I2 + g;  a step composes the map of the LATER steps (lower lanes) first,
//     g <- gl I2 + g,   I2 <- Yl I2.        Lanes without a source receive the identity map (Yl = I, gl = 0).
template <int X, int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ void dpp_rowaffine_step(double* I2, double* g, const double* srcI, const double* srcg) {
  double Yl[X * X], gl[X], Pn[X * X];
#pragma unroll
  for (int i = 0; i < X * X; ++i) Yl[i] = dpp_mov<CTRL, ROW_MASK, BANK_MASK>(srcI[i], (i / X == i % X) ? 1.0 : 0.0);
#pragma unroll
  for (int a = 0; a < X; ++a) gl[a] = dpp_mov<CTRL, ROW_MASK, BANK_MASK>(srcg[a], 0.0);
#pragma unroll
  for (int d = 0; d < X; ++d) {
    double tt = g[d];
#pragma unroll
    for (int a = 0; a < X; ++a) tt += gl[a] * I2[a * X + d];
    g[d] = tt;
  }
  matmul_xx<X>(Yl, I2, Pn);
#pragma unroll
  for (int i = 0; i < X * X; ++i) I2[i] = Pn[i];
}
template <int X>
__device__ __forceinline__ void dpp_rowaffine_prefix(double* I2, double* g) {
  double I0_[X * X], g0_[X];
#pragma unroll
  for (int i = 0; i < X * X; ++i) I0_[i] = I2[i];
#pragma unroll
  for (int a = 0; a < X; ++a) g0_[a] = g[a];
  dpp_rowaffine_step<X, 0x111, 0xf, 0xf>(I2, g, I0_, g0_);
  dpp_rowaffine_step<X, 0x112, 0xf, 0xf>(I2, g, I0_, g0_);
  dpp_rowaffine_step<X, 0x113, 0xf, 0xf>(I2, g, I0_, g0_);
  dpp_rowaffine_step<X, 0x114, 0xf, 0xe>(I2, g, I2, g);
  dpp_rowaffine_step<X, 0x118, 0xf, 0xc>(I2, g, I2, g);
  dpp_rowaffine_step<X, 0x142, 0xa, 0xf>(I2, g, I2, g);
  dpp_rowaffine_step<X, 0x143, 0xc, 0xf>(I2, g, I2, g);
}

// MODE 0: state evaluation -- store dc/dv rows, symmetric Gram, dc/du rows into the slot.
// MODE 1: Newton iteration -- Gram of the iterate's rows against the stored rows of slot `which`.
// GRAM false (16-row blocks): no Gram accumulation -- the rows are stored (MODE 0: into the slot, MODE 1: into
// work.JvW) and k_gram_rows forms the Gram block from the stored rows.  A 16 x 16 accumulator per lane does not fit
// the register file: with it the sweep ran out of scratch memory, 25x slower than the 8-row instantiations.
template <class M, int RM, int MODE, bool GRAM = true>
__global__ void __launch_bounds__(256) k_rev_wave(Sys sy, Slots sl, Work w, int which, int qsel) {
  constexpr int X = M::X, V = M::V, Z = M::Z, U = M::U, V0 = M::V0;
  // A 16 x 16 Gram accumulator per lane does not fit the register file (the sweep lived in scratch memory and its
  // fully unrolled form produced wrong dc/du): 16-row blocks store their rows and k_gram_rows forms the Gram block.
  static_assert(RM <= 8 || !GRAM, "16-row blocks: instantiate with GRAM = false and form the Gram block with k_gram_rows");
  constexpr int URM = 64;
  constexpr bool STORE_ROWS = MODE == 0 || !GRAM;
  // Interval frames.  Within an observation interval no row is injected, so every adjoint row at a step is the row at
  // the interval's END (the frame LamF, wave-uniform) times ONE matrix that does not depend on the row:
  //     Lam_i(step s) = LamF_i Pf E_s       (Pf: product of the tiles already swept, E_s: the lane's suffix product),
  // hence, with T_s = Pf E_s B_s (X x V) and PE_s = Pf E_s,
  //     dc_i/dv_s                = LamF_i T_s
  //     sum_s Lam_i(s) Zf_s      = LamF_i  [ sum_s PE_s Zf_s ]                 Wacc : X x Z sums instead of RM x Z
  //     Gram (Newton)  D_ij      = LamF_i  [ sum_s T_s (dc_j/dv_s of the stored point)^T ]     Yacc : RM x X instead of RM x RM
  //     Gram (state)   D_ij      = LamF_i  [ sum_s T_s T_s^T ] LamF_j^T                        Sacc : X x X
  // The hot loop therefore carries 8 + 14 (Newton) or 8 + 4 (state) running sums per lane for FitzHugh-Nagumo instead
  // of 28 + 49, does not form the rows at all in a Newton iteration, and the RM-sized products are taken once per
  // interval (flush_frame), where the rows for the next interval are formed as LamF Pf as well.
  constexpr bool ZW = GRAM;  // the frames carry the Gram accumulation
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (MODE == 1 ? !newton_select(w, c, which, qsel) : !w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int sl_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const double* q = (MODE == 1 ? (qsel ? w.qb : pick(sl.q, sl_ ^ 1)) : pick(sl.q, sl_)) + (size_t)c * sy.Q;
  const double* traj = (MODE == 1 ? w.trajw : pick(sl.traj, sl_)) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* Jr = pick(sl.Jv, sl_) + (size_t)c * RM * NV;  // MODE 1: read; MODE 0: written through Jo
  double* Jo = (MODE == 1 ? w.JvW : pick(sl.Jv, sl_)) + (size_t)c * RM * NV;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const size_t colb = (size_t)sy.V0 + (size_t)bd.step0 * V;

  double Lam[RM * X], Dacc[GRAM ? RM * RM : 1], zacc[RM * Z];
  double LamF[ZW ? RM * X : 1], Wacc[ZW ? X * Z : 1], Pf[ZW ? X * X : 1];
  double Yacc[ZW && MODE == 1 ? RM * X : 1], Sacc[ZW && MODE == 0 ? X * X : 1];
  if (ZW) {
#pragma unroll
    for (int i = 0; i < RM * X; ++i) LamF[i] = 0.0;
#pragma unroll
    for (int i = 0; i < X * Z; ++i) Wacc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < X * X; ++i) Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < (MODE == 1 ? RM * X : 1); ++i) Yacc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < (MODE == 0 ? X * X : 1); ++i) Sacc[i] = 0.0;
  }
  auto flush_frame = [&]() {  // the RM-sized products of the interval just swept; its rows at its start
    if (ZW) {
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int mz = 0; mz < Z; ++mz) {
          double tt2 = zacc[i * Z + mz];
#pragma unroll
          for (int a = 0; a < X; ++a) tt2 += LamF[i * X + a] * Wacc[a * Z + mz];
          zacc[i * Z + mz] = tt2;
        }
      if (MODE == 1) {
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int jj = 0; jj < RM; ++jj) {
            double tt2 = Dacc[i * RM + jj];
#pragma unroll
            for (int a = 0; a < X; ++a) tt2 += LamF[i * X + a] * Yacc[jj * X + a];
            Dacc[i * RM + jj] = tt2;
          }
#pragma unroll
        for (int i = 0; i < RM * X; ++i) Yacc[i] = 0.0;
      } else {
        double Qi[RM * X];  // LamF Sacc (Sacc holds the upper triangle of the symmetric X x X sum)
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int bb = 0; bb < X; ++bb) {
            double tt2 = 0.0;
#pragma unroll
            for (int a = 0; a < X; ++a) tt2 += LamF[i * X + a] * (a <= bb ? Sacc[a * X + bb] : Sacc[bb * X + a]);
            Qi[i * X + bb] = tt2;
          }
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int jj = 0; jj <= i; ++jj) {
            double tt2 = Dacc[i * RM + jj];
#pragma unroll
            for (int bb = 0; bb < X; ++bb) tt2 += Qi[i * X + bb] * LamF[jj * X + bb];
            Dacc[i * RM + jj] = tt2;
          }
#pragma unroll
        for (int i = 0; i < X * X; ++i) Sacc[i] = 0.0;
      }
#pragma unroll
      for (int i = 0; i < RM; ++i)  // the rows at the start of the swept interval
#pragma unroll
        for (int d = 0; d < X; ++d) {
          double tt2 = 0.0;
#pragma unroll
          for (int a = 0; a < X; ++a) tt2 += LamF[i * X + a] * Pf[a * X + d];
          Lam[i * X + d] = tt2;
        }
#pragma unroll
      for (int i = 0; i < X * Z; ++i) Wacc[i] = 0.0;
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
    }
  };
#pragma unroll URM
  for (int i = 0; i < RM * X; ++i) Lam[i] = 0.0;
#pragma unroll
  for (int i = 0; i < (GRAM ? RM * RM : 1); ++i) Dacc[i] = 0.0;
#pragma unroll URM
  for (int i = 0; i < RM * Z; ++i) zacc[i] = 0.0;

  // The tiles are walked backwards in time as a two-stage software pipeline (one wavefront per SIMD is resident at
  // this register footprint, so independent work must come from the wave itself):
  //   stage 1 (tile t-1): transition matrices of the 64 steps and their suffix scan -- a chain of dependent shuffles;
  //   stage 2 (tile t)  : adjoint rows at every lane (Lam E), Jacobian entries, dc/dz sums, Gram accumulation.
  // Stage 1 of the next tile does not depend on the carried rows Lam, so both stages sit in one basic block and the
  // scheduler fills the shuffle latencies of one with the FMAs of the other.  Raw inputs are requested two tiles
  // ahead.
  const int ntile = (S + 63) >> 6;
  const int ntot = bd.nobs * ntile;
  struct Raw {
    double x[X], v[V];
    bool valid;
    int s;
  };
  struct Rows {  // stored rows of slot `which` at the tile's steps (MODE 1 with Gram): requested ONE tile ahead
    double jp[(MODE == 1 && GRAM) ? RM * V : 1];
  };
  struct Scan {
    double Bm[X * V], Zf[X * Z], E[X * X], I0[X * X];
  };
  auto fetch = [&](int tt, Raw& r) {
    const int jj = tt / ntile, t = tt - jj * ntile;
    const int off = (t << 6) + (63 - lane);  // later steps in lower lanes (DPP prefix scans)
    r.valid = tt >= 0 && off < S;
    r.s = jj * S + off;
    if (r.valid) {
#pragma unroll
      for (int a = 0; a < X; ++a) r.x[a] = ld_stream(traj + (size_t)r.s * X + a);
#pragma unroll
      for (int a = 0; a < V; ++a) r.v[a] = vbase[(size_t)r.s * V + a];
    } else {
#pragma unroll
      for (int a = 0; a < X; ++a) r.x[a] = 0.0;
#pragma unroll
      for (int a = 0; a < V; ++a) r.v[a] = 0.0;
    }
  };
  auto fetch_rows = [&](const Raw& r, Rows& o) {
    if (MODE == 1 && GRAM) {
      if (r.valid) {
        const size_t col = colb + (size_t)r.s * V;
#pragma unroll URM
        for (int i = 0; i < RM; ++i)  // (skipping the structurally zero rows here breaks the load pipelining: 2x slower)
#pragma unroll
          for (int d = 0; d < V; ++d) o.jp[i * V + d] = ld_stream(Jr + (size_t)i * NV + col + d);
      } else {
#pragma unroll URM
        for (int i = 0; i < RM * V; ++i) o.jp[i] = 0.0;
      }
    }
  };
  auto stage1 = [&](const Raw& r, Scan& o) {
    double A[X * X];
    if (r.valid) {
      M::jac(cc.k, r.x, r.v, A, o.Bm, o.Zf);
    } else {
#pragma unroll
      for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < X * V; ++i) o.Bm[i] = 0.0;
#pragma unroll
      for (int i = 0; i < X * Z; ++i) o.Zf[i] = 0.0;
    }
    // inclusive suffix scan: Inc_l = A_{hi} ... A_{l}  (later steps on the left)
    double Inc[X * X], Eex[X * X];  // inclusive / exclusive products of the later steps (lower lanes)
    dpp_prefix_products<X>(A, Inc, Eex);
#pragma unroll
    for (int i = 0; i < X * X; ++i) {
      o.E[i] = Eex[i];
      o.I0[i] = bcast_lane63(Inc[i]);  // the whole tile's product carries the rows across the tile
    }
  };
  auto stage2 = [&](const Scan& sc, const Raw& r, const Rows& rw) {
    if constexpr (ZW) {
      double PE[X * X], T[X * V];
      matmul_xx<X>(Pf, sc.E, PE);
#pragma unroll
      for (int a = 0; a < X; ++a)
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt2 = 0.0;
#pragma unroll
          for (int e = 0; e < X; ++e) tt2 += PE[a * X + e] * sc.Bm[e * V + d];
          T[a * V + d] = tt2;
        }
#pragma unroll
      for (int a = 0; a < X; ++a)
#pragma unroll
        for (int mz = 0; mz < Z; ++mz) {
          double tt2 = Wacc[a * Z + mz];
#pragma unroll
          for (int e = 0; e < X; ++e) tt2 += PE[a * X + e] * sc.Zf[e * Z + mz];
          Wacc[a * Z + mz] = tt2;
        }
      if (MODE == 0) {
        if (r.valid) {  // the rows of this step, dc_i/dv_s = LamF_i T_s, go straight to memory
          const size_t col0 = colb + (size_t)r.s * V;
#pragma unroll
          for (int i = 0; i < RM; ++i) {
            double jr0[V];
#pragma unroll
            for (int d = 0; d < V; ++d) {
              double tt2 = 0.0;
#pragma unroll
              for (int a = 0; a < X; ++a) tt2 += LamF[i * X + a] * T[a * V + d];
              jr0[d] = tt2;
            }
            if (V == 2) {
              st_async2(Jo + (size_t)i * NV + col0, jr0[0], jr0[V - 1]);
            } else {
#pragma unroll
              for (int d = 0; d < V; ++d) st_async(Jo + (size_t)i * NV + col0 + d, jr0[d]);
            }
          }
        }
#pragma unroll
        for (int a = 0; a < X; ++a)
#pragma unroll
          for (int bb = a; bb < X; ++bb) {
            double tt2 = Sacc[a * X + bb];
#pragma unroll
            for (int d = 0; d < V; ++d) tt2 += T[a * V + d] * T[bb * V + d];
            Sacc[a * X + bb] = tt2;
          }
      } else {
#pragma unroll
        for (int jj = 0; jj < RM; ++jj)
#pragma unroll
          for (int a = 0; a < X; ++a) {
            double tt2 = Yacc[jj * X + a];
#pragma unroll
            for (int d = 0; d < V; ++d) tt2 += T[a * V + d] * rw.jp[jj * V + d];
            Yacc[jj * X + a] = tt2;
          }
      }
      double Pn[X * X];
      matmul_xx<X>(Pf, sc.I0, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pf[i] = Pn[i];
      return;
    }
    double Ls[RM * X], jr[RM * V];
#pragma unroll URM
    for (int i = 0; i < RM; ++i) {
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt2 = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt2 += Lam[i * X + a] * sc.E[a * X + d];
        Ls[i * X + d] = tt2;
      }
#pragma unroll
      for (int d = 0; d < V; ++d) {
        double tt2 = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt2 += Ls[i * X + a] * sc.Bm[a * V + d];
        jr[i * V + d] = tt2;
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt2 = zacc[i * Z + mz];
#pragma unroll
        for (int a = 0; a < X; ++a) tt2 += Ls[i * X + a] * sc.Zf[a * Z + mz];
        zacc[i * Z + mz] = tt2;
      }
    }
    const size_t col = colb + (size_t)r.s * V;
    if (STORE_ROWS) {
      if (r.valid) {
#pragma unroll URM
        for (int i = 0; i < RM; ++i) {
          if (V == 2) {
            st_async2(Jo + (size_t)i * NV + col, jr[i * V], jr[i * V + 1]);
          } else {
#pragma unroll
            for (int d = 0; d < V; ++d) st_async(Jo + (size_t)i * NV + col + d, jr[i * V + d]);
          }
        }
      }
    }
    if (!GRAM) {
      // (Gram block formed afterwards by k_gram_rows)
    } else if (MODE == 0) {
#pragma unroll URM
      for (int i = 0; i < RM; ++i)
#pragma unroll URM
        for (int jj = 0; jj <= i; ++jj) {
          double tt2 = Dacc[i * RM + jj];
#pragma unroll
          for (int d = 0; d < V; ++d) tt2 += jr[i * V + d] * jr[jj * V + d];
          Dacc[i * RM + jj] = tt2;
        }
    } else {
#pragma unroll URM
      for (int i = 0; i < RM; ++i)
#pragma unroll URM
        for (int jj = 0; jj < RM; ++jj) {
          double tt2 = Dacc[i * RM + jj];
#pragma unroll
          for (int d = 0; d < V; ++d) tt2 += jr[i * V + d] * rw.jp[jj * V + d];
          Dacc[i * RM + jj] = tt2;
        }
    }
    // carry the adjoint rows to the start of this tile: Lam <- Lam Inc_0
#pragma unroll URM
    for (int i = 0; i < RM; ++i) {
      double nl[X];
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt2 = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt2 += Lam[i * X + a] * sc.I0[a * X + d];
        nl[d] = tt2;
      }
#pragma unroll
      for (int d = 0; d < X; ++d) Lam[i * X + d] = nl[d];
    }
  };
  Raw r0, r1, r2;
  Rows w0, w1;
  Scan sc0, sc1;
  fetch(ntot - 1, r0);
  fetch_rows(r0, w0);
  fetch(ntot - 2, r1);
  stage1(r0, sc0);
  for (int tt = ntot - 1; tt >= 0; --tt) {
    const int j = tt / ntile, t = tt - j * ntile;
    fetch(tt - 2, r2);
    fetch_rows(r1, w1);
    if (t == ntile - 1) {
      flush_frame();  // the interval that has just been swept
      // rows that start at the end of observation interval j
      if (j < bd.ny) {
        double g[X];
        M::obs_grad(traj + (size_t)(j + 1) * S * X, g);
#pragma unroll URM
        for (int i = 0; i < RM; ++i)
          if (i == j)
#pragma unroll
            for (int a = 0; a < X; ++a) Lam[i * X + a] = g[a];
      }
      if (j == bd.nobs - 1 && !bd.last) {
#pragma unroll URM
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int a = 0; a < X; ++a)
            if (i == bd.ny + a) Lam[i * X + a] = 1.0;
      }
      if (ZW) {
#pragma unroll
        for (int i = 0; i < RM * X; ++i) LamF[i] = Lam[i];
      }
    }
    stage1(r1, sc1);  // tile tt - 1 (identity when there is none)
    stage2(sc0, r0, w0);  // tile tt
    r0 = r1;
    r1 = r2;
    w0 = w1;
    sc0 = sc1;
  }
  flush_frame();  // the first interval
  // x_0 = generate_x_0(z, v_0): the v_0 columns and the z-dependence of the first block (lane 0's share)
  if (bd.first && lane == 0) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    double j0[RM * V0];
    for (int i = 0; i < RM; ++i) {
      for (int d = 0; d < V0; ++d) {
        double tt = 0.0;
        for (int a = 0; a < X; ++a) tt += Lam[i * X + a] * dv0[a * V0 + d];
        j0[i * V0 + d] = tt;
      }
      for (int mz = 0; mz < Z; ++mz) {
        double tt = 0.0;
        for (int a = 0; a < X; ++a) tt += Lam[i * X + a] * dz[a * Z + mz];
        zacc[i * Z + mz] += tt;
      }
    }
    if (STORE_ROWS) {
      for (int i = 0; i < RM; ++i)
        for (int d = 0; d < V0; ++d) Jo[(size_t)i * NV + d] = j0[i * V0 + d];
    }
    if (!GRAM) {
    } else if (MODE == 0) {
      for (int i = 0; i < RM; ++i)
        for (int jj = 0; jj <= i; ++jj)
          for (int d = 0; d < V0; ++d) Dacc[i * RM + jj] += j0[i * V0 + d] * j0[jj * V0 + d];
    } else {
      for (int i = 0; i < RM; ++i)
        for (int jj = 0; jj < RM; ++jj)
          for (int d = 0; d < V0; ++d) Dacc[i * RM + jj] += j0[i * V0 + d] * Jr[(size_t)jj * NV + d];
    }
  }
  // combine the per-lane partial sums over the wave
#pragma unroll
  for (int i = 0; i < (GRAM ? RM * RM : 0); ++i) {
    if (MODE == 0 && (i % RM) > (i / RM)) continue;
    double v = Dacc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    Dacc[i] = v;
  }
#pragma unroll URM
  for (int i = 0; i < RM * Z; ++i) {
    double v = zacc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    zacc[i] = v;
  }
  if (lane == 0) {
    if (GRAM) {
      if (MODE == 0) {
#pragma unroll URM
        for (int i = 0; i < RM; ++i)
#pragma unroll URM
          for (int jj = 0; jj < i; ++jj) Dacc[jj * RM + i] = Dacc[i * RM + jj];
      }
      // dc_dn_l * dc_dn_r (:772-791): sigma at the iterate times sigma at the point whose rows are stored
      const double sg_ = sy.noisy ? sigma_at(sy, q, c) : 0.0;
      const double s2 = sg_ * (MODE == 0 || !sy.noisy ? sg_ : sigma_at(sy, pick(sl.q, sl_) + (size_t)c * sy.Q, c));
#pragma unroll URM
      for (int i = 0; i < RM; ++i) {
        if (sy.noisy && i < bd.ny) Dacc[i * RM + i] += s2;  // dc/dn dc/dn^T (:772-791)
        if (i >= bd.nrows) Dacc[i * RM + i] = 1.0;          // identity padding
      }
      double* Do = w.Dw + cb * RM * RM;
#pragma unroll
      for (int i = 0; i < RM * RM; ++i) Do[i] = Dacc[i];
    }
    if (MODE == 0) {
      double* zo = w.zbP + cb * RM * Z;
#pragma unroll URM
      for (int i = 0; i < RM * Z; ++i) zo[i] = zacc[i];
    }
    double G[Z * Z];
    M::gz_jac(q, G);
    double* ju = (MODE == 0 ? pick(sl.JuP, sl_) : w.JuL) + cb * RM * U;
    for (int i = 0; i < RM; ++i) {
      for (int d = 0; d < Z; ++d) {
        double tt = 0.0;
        for (int mz = 0; mz < Z; ++mz) tt += zacc[i * Z + mz] * G[mz * Z + d];
        ju[i * U + d] = tt;
      }
      // d(sigma(u) n_i) / du_sigma = sigma n_i on the observation rows (g_y_bar :559-569)
      if (M::VS) ju[i * U + Z] = i < bd.ny ? sigma_at(sy, q, c) * q[sy.U + sy.NV + bd.obs0 + i] : 0.0;
    }
  }
}

// The sweep of k_rev_wave rebuilt around the interval frames for TWO OR THREE wavefronts per SIMD.
// With the frames the hot loop carries only X x Z + X x X running sums per lane, but k_rev_wave
// still keeps the RM x RM Gram block, the RM x Z dc/dz rows and the adjoint rows per lane (210 registers that are touched
// once per interval), which pins it at one wavefront per SIMD, where the 6-level shuffle scan of every tile is exposed
// latency (measured: cutting its HBM bytes by 17 % changed nothing).  Here the per-interval running sums are added up
// over the wave when an interval ends (shuffle butterfly) and everything RM-sized lives ONCE per wavefront in LDS
// (0.9 KB): adjoint rows of the frame, Gram block, dc/dz rows, updated by one lane per entry.  The kernel fits
// 128 registers, two wavefronts share a SIMD and fill each other's shuffle latencies.
#ifndef CHMC_LEAN_WAVES
#define CHMC_LEAN_WAVES 2
#endif
// The FitzHugh-Nagumo instantiations need 188 VGPRs; capped at 168 (three wavefronts per SIMD) they spill 13 dwords and
// still run 7 % faster (newton_blk 1.31 -> 1.21 ms per step).
#ifndef CHMC_LEAN_WAVES_PB
#define CHMC_LEAN_WAVES_PB 3
#endif
// The kernel is the STATE EVALUATION of slot `which` on the compact rows (k_rev_wave<MODE 0> at a third of its registers):
// the Gram block is that of the point itself (X x X running sum of T T^T, own frames), the compact rows PB / LF
// and the v_0 columns of the rows are written, dc/du rows go to the slot and dc/dz rows to work.zbP.  (The Newton
// iterations that once ran through it run through k_newton_ivl + k_newton_comb below.)
#define CHMC_IVL_N(X, Z) (2 * (X) * (X) + (X) * (Z))  // per-interval sums Ss, Ws, Pt (k_newton_ivl below)
template <class M, int RM>
__global__ void __launch_bounds__(64, (M::X * M::V <= 4) ? CHMC_LEAN_WAVES_PB : CHMC_LEAN_WAVES)
    k_state_lean(Sys sy, Slots sl, Work w, int which) {
  constexpr int X = M::X, V = M::V, Z = M::Z, U = M::U, V0 = M::V0;
  static_assert(RM <= 8, "blocks of at most 8 rows");
  __shared__ double LamF[RM * X], Dl[RM * RM], zl[RM * Z], Ys[RM * X], Ws[X * Z], Ss[X * X];
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int sl_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const double* q = pick(sl.q, sl_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, sl_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  double* Jo = pick(sl.Jv, sl_) + (size_t)c * RM * NV;  // (only the rows' v_0 columns are written)
  double* PBo = pick(sl.PB, sl_) + ((size_t)c * sy.T * S + bd.step0) * (X * V);
  double* LFo = pick(sl.LF, sl_) + cb * sy.NOBS * RM * X;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  for (int e = lane; e < RM * X; e += 64) LamF[e] = 0.0;
  for (int e = lane; e < RM * RM; e += 64) Dl[e] = 0.0;
  for (int e = lane; e < RM * Z; e += 64) zl[e] = 0.0;
  lds_sync();
  double Wacc[X * Z], Yacc[X * X], Pf[X * X];
#pragma unroll
  for (int i = 0; i < X * Z; ++i) Wacc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < X * X; ++i) Yacc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < X * X; ++i) Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
  // end of an interval: the wave's sums, the RM-sized products (one lane per entry), the rows at the interval's start
  // (jprev: the interval that has just been swept; bd.nobs when nothing has been swept yet)
  auto flush_frame = [&](int jprev) {
#pragma unroll
    for (int i = 0; i < X * X; ++i) {
      double v = Yacc[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == i) Ss[i] = v;
      Yacc[i] = 0.0;
    }
    // Ys[jj][a] = sum_s T_s[a][:] . (dc_jj/dv_s of the point) = sum_a2 Ss[a][a2] LF[jj][a2]
    lds_sync();
    if (lane < RM * X) {
      const int jj = lane / X, a = lane - jj * X;
      double tt = 0.0;
      if (jprev < bd.nobs) {
        const double* lf = LamF + jj * X;  // (the point's own frame, still in LamF at this point of the flush)
#pragma unroll
        for (int a2 = 0; a2 < X; ++a2) tt += Ss[a * X + a2] * lf[a2];
      }
      Ys[lane] = tt;
    }
#pragma unroll
    for (int i = 0; i < X * Z; ++i) {
      double v = Wacc[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == i) Ws[i] = v;
      Wacc[i] = 0.0;
    }
    lds_sync();
    // the swept interval's sums for the forward grad-log-det sweep (k_gld_fwd_qx): Ss = sum T T^T, Ws = sum PE Zf, Pt,
    // in k_newton_ivl's layout
    if (jprev < bd.nobs && w.ivl) {
      double* iv = w.ivl + (cb * sy.NOBS + jprev) * CHMC_IVL_N(X, Z);
      if (lane < X * X) iv[lane] = Ss[lane];
      if (lane < X * Z) iv[X * X + lane] = Ws[lane];
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < X * X; ++i) iv[X * X + X * Z + i] = Pf[i];
      }
    }
    double nl = 0.0;  // entry `lane` of the rows at the start of the swept interval, LamF Pf
    if (lane < RM * X) {
      const int i = lane / X, d = lane - i * X;
#pragma unroll
      for (int a = 0; a < X; ++a) {
        double pf = 0.0;
#pragma unroll
        for (int dd = 0; dd < X; ++dd) pf = dd == d ? Pf[a * X + dd] : pf;
        nl += LamF[i * X + a] * pf;
      }
    }
    if (lane < RM * RM) {
      const int i = lane / RM, jj = lane - i * RM;
      double tt = Dl[lane];
#pragma unroll
      for (int a = 0; a < X; ++a) tt += LamF[i * X + a] * Ys[jj * X + a];
      Dl[lane] = tt;
    }
    if (lane < RM * Z) {
      const int i = lane / Z, mz = lane - i * Z;
      double tt = zl[lane];
#pragma unroll
      for (int a = 0; a < X; ++a) tt += LamF[i * X + a] * Ws[a * Z + mz];
      zl[lane] = tt;
    }
    lds_sync();
    if (lane < RM * X) LamF[lane] = nl;
#pragma unroll
    for (int i = 0; i < X * X; ++i) Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
    lds_sync();
  };
  const int ntile = (S + 63) >> 6;
  struct Raw {
    double x[X], v[V];
    bool valid;
  };
  auto fetch = [&](int tt, Raw& r) {
    const int jj = tt / ntile, t = tt - jj * ntile;
    const int off = (t << 6) + (63 - lane);  // LATER steps in LOWER lanes: the suffix products become a prefix scan
    r.valid = tt >= 0 && off < S;
    const int s = jj * S + off;
    if (r.valid) {
#pragma unroll
      for (int a = 0; a < X; ++a) r.x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
      for (int a = 0; a < V; ++a) r.v[a] = vbase[(size_t)s * V + a];
    } else {
#pragma unroll
      for (int a = 0; a < X; ++a) r.x[a] = 0.0;
#pragma unroll
      for (int a = 0; a < V; ++a) r.v[a] = 0.0;
    }
  };
  Raw r0, r1;
  fetch(bd.nobs * ntile - 1, r0);
  for (int tt = bd.nobs * ntile - 1; tt >= 0; --tt) {
    const int j = tt / ntile, t = tt - j * ntile;
    fetch(tt - 1, r1);
    if (t == ntile - 1) {
      flush_frame(j + 1);  // the interval that has just been swept
      // rows that start at the end of observation interval j
      if (j < bd.ny) {
        double g[X], gl = 0.0;
        M::obs_grad(traj + (size_t)(j + 1) * S * X, g);
#pragma unroll
        for (int a = 0; a < X; ++a) gl = lane == a ? g[a] : gl;
        if (lane < X) LamF[j * X + lane] = gl;
      }
      if (j == bd.nobs - 1 && !bd.last) {
        if (lane < X) LamF[(bd.ny + lane) * X + lane] = 1.0;
      }
      lds_sync();
      if (lane < RM * X) LFo[(size_t)j * RM * X + lane] = LamF[lane];  // the frame of interval j (Slots::LF)
    }
    double A[X * X], Bm[X * V], Zf[X * Z];
    if (r0.valid) {
      M::jac(cc.k, r0.x, r0.v, A, Bm, Zf);
    } else {
#pragma unroll
      for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
      for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
    }
    // products of the transition matrices of the LATER steps of the tile (later steps on the left): with the later steps
    // in the lower lanes an exclusive prefix product over the lanes; lane 63's inclusive product spans the tile
    double Inc[X * X], E[X * X], I0[X * X], PE[X * X], T[X * V];
    dpp_prefix_products<X>(A, Inc, E);
#pragma unroll
    for (int i = 0; i < X * X; ++i) I0[i] = bcast_lane63(Inc[i]);
    matmul_xx<X>(Pf, E, PE);
#pragma unroll
    for (int a = 0; a < X; ++a)
#pragma unroll
      for (int d = 0; d < V; ++d) {
        double tt2 = 0.0;
#pragma unroll
        for (int e = 0; e < X; ++e) tt2 += PE[a * X + e] * Bm[e * V + d];
        T[a * V + d] = tt2;
      }
#pragma unroll
    for (int a = 0; a < X; ++a)
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt2 = Wacc[a * Z + mz];
#pragma unroll
        for (int e = 0; e < X; ++e) tt2 += PE[a * X + e] * Zf[e * Z + mz];
        Wacc[a * Z + mz] = tt2;
      }
    if (r0.valid) {  // PB[s] = T_s: the compact form of this step's rows (Slots::PB)
      const int off0 = (t << 6) + (63 - lane);
      double* dst = PBo + (size_t)(j * S + off0) * (X * V);
      if ((X * V) % 2 == 0) {
#pragma unroll
        for (int k = 0; k + 1 < X * V; k += 2) st_async2(dst + k, T[k], T[k + 1]);
      } else {
#pragma unroll
        for (int k = 0; k < X * V; ++k) st_async(dst + k, T[k]);
      }
    }
#pragma unroll
    for (int a = 0; a < X; ++a)
#pragma unroll
      for (int a2 = 0; a2 < X; ++a2) {
        double tt2 = Yacc[a * X + a2];
#pragma unroll
        for (int d = 0; d < V; ++d) tt2 += T[a * V + d] * T[a2 * V + d];
        Yacc[a * X + a2] = tt2;
      }
    {
      double Pn[X * X];
      matmul_xx<X>(Pf, I0, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pf[i] = Pn[i];
    }
    r0 = r1;
  }
  flush_frame(0);  // the first interval; LamF now holds the rows at the start of the block
  // x_0 = generate_x_0(z, v_0): the v_0 columns and the z-dependence of the first block
  if (bd.first) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    if (lane < RM * RM) {
      const int i = lane / RM, jj = lane - i * RM;
      double tt = Dl[lane];
      for (int d = 0; d < V0; ++d) {
        double j0 = 0.0, j1 = 0.0;
        for (int a = 0; a < X; ++a) j0 += LamF[i * X + a] * dv0[a * V0 + d], j1 += LamF[jj * X + a] * dv0[a * V0 + d];
        tt += j0 * j1;
        if (jj == 0) Jo[(size_t)i * NV + d] = j0;  // the rows' v_0 columns
      }
      Dl[lane] = tt;
    }
    if (lane < RM * Z) {
      const int i = lane / Z, mz = lane - i * Z;
      double tt = zl[lane];
      for (int a = 0; a < X; ++a) {
        double dzs = 0.0;
#pragma unroll
        for (int e = 0; e < X * Z; ++e) dzs = e == a * Z + mz ? dz[e] : dzs;
        tt += LamF[i * X + a] * dzs;
      }
      zl[lane] = tt;
    }
  }
  lds_sync();
  if (lane < RM * RM) {  // noise term on the observation rows, identity padding
    const int i = lane / RM, jj = lane - i * RM;
    double v = Dl[lane];
    if (i == jj) {
      const double sg_ = sy.noisy ? sigma_at(sy, q, c) : 0.0;
      if (sy.noisy && i < bd.ny) v += sg_ * sigma_at(sy, pick(sl.q, sl_) + (size_t)c * sy.Q, c);  // dc_dn dc_dn^T (:772-791)
      if (i >= bd.nrows) v = 1.0;
    }
    w.Dw[cb * RM * RM + lane] = v;
  }
  double G[Z * Z];
  M::gz_jac(q, G);
  for (int e = lane; e < RM * U; e += 64) {  // dc/du rows of the iterate through generate_z'(u)
    const int i = e / U, d = e - i * U;
    double tt = 0.0;
    if (d < Z) {
      for (int mz = 0; mz < Z; ++mz) {
        double gs = 0.0;
#pragma unroll
        for (int ee = 0; ee < Z * Z; ++ee) gs = ee == mz * Z + d ? G[ee] : gs;
        tt += zl[i * Z + mz] * gs;
      }
    } else {
      tt = i < bd.ny ? sigma_at(sy, q, c) * q[sy.U + sy.NV + bd.obs0 + i] : 0.0;
    }
    pick(sl.JuP, sl_)[cb * RM * U + e] = tt;
  }
  for (int e = lane; e < RM * Z; e += 64) w.zbP[cb * RM * Z + e] = zl[e];
}

// The body of k_newton_factor_wave for the block (c, b) on the 16 lanes r = lane & 15 of a 16-lane group (act: this group has a
// block and its chain is in the loop); Dsrc / Jusrc: the block's Gram matrix and dc/du rows of the iterate (global memory, or
// the LDS copies of k_newton_comb<.., FACTOR>, which runs this right behind its combine step: one launch of a Newton round
// less for one 16-row block per chain).
// ONE: the wavefront holds ONE block, in its lanes 0 .. 15 (the per-chain retraction kernel): the cross-lane traffic of the
// factorisation then needs no LDS crossbar -- the row exchange and the pivot-row broadcast are v_readlane from a compile-time
// lane (j) and a wave-uniform one (the pivot), the 16-lane reductions rotate inside the row on the DPP path (row_ror 8 / 4 /
// 2 / 1; sums are then taken from lane 0 so that every lane holds the same bits), the entries left of the pivot column are
// not exchanged (nothing reads them again: the right-hand sides travel in the augmented rows), and the back substitution
// multiplies by one reciprocal per row instead of dividing 1 + U times.
__device__ __forceinline__ double readlane_d(double x, int srclane) {  // srclane: wave-uniform
  union { double d; int i[2]; } u;
  u.d = x;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], srclane);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], srclane);
  return u.d;
}
__device__ __forceinline__ double row16_sum(double v) {  // sum over the 16 lanes of a row, the same bits in every lane
  v += dpp_mov<0x128, 0xf, 0xf>(v, 0.0);  // row_ror:8
  v += dpp_mov<0x124, 0xf, 0xf>(v, 0.0);  // row_ror:4
  v += dpp_mov<0x122, 0xf, 0xf>(v, 0.0);  // row_ror:2
  v += dpp_mov<0x121, 0xf, 0xf>(v, 0.0);  // row_ror:1
  return readlane_d(v, 0);
}
template <class M, int RM, bool FUSE, bool ONE = false>
__device__ __forceinline__ void newton_factor16(const Sys& sy, const Slots& sl, const Work& w, int prev, int qsel, int c, int b,
                                                bool act, const double* Dsrc, const double* Jusrc,
                                                const double* lf_copy = nullptr) {  // (the block's frames LF[m][i][x] in LDS)
  static_assert(RM == 16, "rows over 16 lanes");
  constexpr int U = M::U, NC = RM + 1 + U;  // augmented row: D row | c | dc/du row
  const int lane = threadIdx.x & 63, r = lane & 15;
  const int sp = sl.cur[c] ^ prev;
  const size_t cb = (size_t)c * sy.Kmax + b;
  double a[NC];
#pragma unroll
  for (int k = 0; k < RM; ++k) a[k] = act ? Dsrc[r * RM + k] : (k == r ? 1.0 : 0.0);
  a[RM] = act ? w.cpad[cb * RM + r] : 0.0;
  const double c0 = a[RM];  // the constraint value of this row (|c|_inf of the iterate, FUSE)
#pragma unroll
  for (int d = 0; d < U; ++d) a[RM + 1 + d] = act ? Jusrc[r * U + d] : 0.0;
#pragma unroll
  for (int j = 0; j < RM; ++j) {
    // pivot: largest |a_ij| over the rows i >= j, the first one on ties
    double best = r >= j ? fabs(a[j]) : -1.0;
    int bi = r;
    double pr[NC];
    if constexpr (ONE) {
#define CHMC_F16_ROT(CTRL)                                                         \
  {                                                                                \
    const double ov = dpp_mov<CTRL, 0xf, 0xf>(best, -1.0);                         \
    const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, 0xf, 0xf, false);     \
    if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;                  \
  }
      CHMC_F16_ROT(0x128) CHMC_F16_ROT(0x124) CHMC_F16_ROT(0x122) CHMC_F16_ROT(0x121)
#undef CHMC_F16_ROT
      const int p = __builtin_amdgcn_readfirstlane(bi);  // (the block sits in lanes 0 .. 15)
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        if (k < j) {  // (columns left of the pivot: never read again)
          pr[k] = 0.0;
          continue;
        }
        const double aj = readlane_d(a[k], j), ap = readlane_d(a[k], p);
        a[k] = r == j ? ap : (r == p ? aj : a[k]);  // exchange rows j and p
        pr[k] = ap;                                  // the pivot row
      }
    } else {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o, 16);
        const int oi = __shfl_xor(bi, o, 16);
        if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
      }
      const int p = bi;  // (uniform over the 16 lanes of the block)
      const int partner = r == j ? p : (r == p ? j : r);
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        a[k] = __shfl(a[k], partner, 16);  // exchange rows j and p
        pr[k] = __shfl(a[k], j, 16);       // the pivot row
      }
    }
    const double inv = 1.0 / pr[j];
    if (r > j) {
      const double l = a[j] * inv;
      a[j] = l;
#pragma unroll
      for (int k = j + 1; k < NC; ++k) a[k] -= l * pr[k];
    }
  }
  // back substitution of the 1 + U right-hand sides, column by column
#pragma unroll
  for (int k = RM - 1; k >= 0; --k) {
    if constexpr (ONE) {
      const double rkk = 1.0 / readlane_d(a[k], k);
#pragma unroll
      for (int d = 0; d < 1 + U; ++d) {
        const double xk = readlane_d(a[RM + d], k) * rkk;
        if (r == k) a[RM + d] = xk;
        if (r < k) a[RM + d] -= a[k] * xk;
      }
    } else {
      const double ukk = __shfl(a[k], k, 16);
#pragma unroll
      for (int d = 0; d < 1 + U; ++d) {
        const double xk = __shfl(a[RM + d], k, 16) / ukk;
        if (r == k) a[RM + d] = xk;
        if (r < k) a[RM + d] -= a[k] * xk;
      }
    }
  }
  if (act) {
    w.tpad[cb * RM + r] = a[RM];
#pragma unroll
    for (int d = 0; d < U; ++d) w.Ew[cb * RM * U + r * U + d] = a[RM + 1 + d];
  }
  // C_b = Ju_prev^T E, s_b = Ju_prev^T t: sums over the 16 rows
  double jur[U];
#pragma unroll
  for (int d = 0; d < U; ++d) jur[d] = act ? pick(sl.JuP, sp)[cb * RM * U + r * U + d] : 0.0;
  double sacc[U], Cm[U * U];
#pragma unroll
  for (int aa = 0; aa < U; ++aa) {
    double v = jur[aa] * a[RM];
    if constexpr (ONE) {
      v = row16_sum(v);
    } else {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
    }
    if (!FUSE && act && r == 0) w.sb[cb * U + aa] = v;
    sacc[aa] = v;
#pragma unroll
    for (int d = 0; d < U; ++d) {
      double t = jur[aa] * a[RM + 1 + d];
      if constexpr (ONE) {
        t = row16_sum(t);
      } else {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o, 16);
      }
      if (!FUSE && act && r == 0) w.Cb[(cb * U + aa) * U + d] = t;
      Cm[aa * U + d] = t;
    }
  }
  if constexpr (FUSE) {
    // (every lane of the block holds s = s_b and C_b: the core system C = M_0 + C_b, y = C^-1 s, redundantly per lane)
    constexpr int X = M::X;
    __shared__ double lamS[4][RM];
#pragma unroll
    for (int i = 0; i < U * U; ++i) Cm[i] += sy.m0 ? metric_of(sy, c)[i] : ((i / U == i % U) ? 1.0 : 0.0);
    {
      int piv[U];
      lu_factor<U>(Cm, piv);
      lu_solve<U, 1>(Cm, piv, sacc);
    }
    double l = a[RM];
#pragma unroll
    for (int d = 0; d < U; ++d) l -= a[RM + 1 + d] * sacc[d];
    if (act) w.lampad[cb * RM + r] = l;
    lamS[lane >> 4][r] = l;
    double du[U];
#pragma unroll
    for (int aa = 0; aa < U; ++aa) {
      double v = jur[aa] * l;
      if constexpr (ONE) {
        v = row16_sum(v);
      } else {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
      }
      du[aa] = v;
    }
    unsigned long long eb = absbits(c0);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const unsigned long long v = __shfl_xor(eb, o, 16);
      eb = v > eb ? v : eb;
    }
    if (act && r == 0) {
      double* q = (qsel ? w.qb : pick(sl.q, sp ^ 1)) + (size_t)c * sy.Q;
      unsigned long long nb = 0ULL;
#pragma unroll
      for (int aa = 0; aa < U; ++aa) {
        const double dq = metric_inv_u(sy, c, du, aa);  // delta_q = metric.inv @ delta_mu (:1033-1041, :1105-1113)
        q[aa] -= dq;
        const unsigned long long vb = absbits(dq);
        nb = vb > nb ? vb : nb;
      }
      w.err[c] = bitsd(eb);
      w.ndq[c] = nb;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (act && w.muF) {  // mu_F[m] = sum_i lambda_i LF[m][i] of the previous point's interval frames (KMuF)
      const BlockDesc bd = sy.blk[b];
      const double* lfb = ONE ? lf_copy : pick(sl.LF, sp) + cb * sy.NOBS * RM * X;  // (ONE: the caller's LDS copy)
      double* mo = w.muF + cb * sy.NOBS * X;
      const double* ls = lamS[lane >> 4];
      for (int e = r; e < sy.NOBS * X; e += 16) {
        const int m = e / X, ax = e - m * X;
        double t = 0.0;
        if (m < bd.nobs) {
          for (int i = 0; i < RM; ++i)
            if (i < bd.nrows) t += ls[i] * lfb[(m * RM + i) * X + ax];
        }
        mo[e] = t;
      }
    }
  }
}

// The Newton-iteration sweep in two phases, for layouts with FEW, LONG blocks (SIR single block: B wavefronts of
// a one-phase sweep would each walk the whole chain, 300 us of pure latency per launch however few chains are active).
// With the compact rows nothing in the hot loop depends on the adjoint rows, so the observation intervals of a block
// are independent up to three small matrices each:
//   phase A  k_newton_ivl : one wavefront per (chain, block, INTERVAL m): the wave's sums over the interval's steps
//            Ss[m] = sum_s T_s PBprev_s^T (X x X),  Ws[m] = sum_s PE_s Zf_s (X x Z),  and the product Pt[m] of the
//            interval's transition matrices (T_s = PE_s B_s, PE_s = product of the later transition matrices of the
//            interval) -> work.ivl;
//   phase B  k_newton_comb: one wavefront per (chain, block) walks the intervals backwards with everything RM-sized in
//            LDS -- frame LamF[m] = rows injected at the interval's end + LamF[m+1] Pt[m+1];
//            Gram += LamF[m] Ss[m] LFprev[m]^T;  dc/dz rows += LamF[m] Ws[m] -- and finishes as k_state_lean does
//            (v_0 columns, observation-noise diagonal, identity padding, dc/du rows through generate_z').
// Any RM <= 16: no per-lane array is indexed by the row.
// (166 VGPRs for FitzHugh-Nagumo: three wavefronts per SIMD at run time; capped at 128 for four it spills, 3x slower)
#ifndef CHMC_IVL_WAVES
#define CHMC_IVL_WAVES 2
#endif
// STATE (both phases): the state evaluation of slot `which` in the same two phases (k_state_lean for blocks of
// any RM <= 16): phase A also WRITES the compact rows PB[s] = T_s and sums T_s T_s^T; phase B writes the frames LF[m], the
// symmetric Gram block, the rows' v_0 columns, the dc/du rows of the slot and the dc/dz rows (work.zbP).
// newton_ivl_body: the sums of observation interval m of block (c, b) by the calling wavefront (which / qsel already
// resolved for the chain; m < nobs of the block); shared by k_newton_ivl and the per-chain retraction kernel.
template <class M, bool STATE>
__device__ __forceinline__ void newton_ivl_body(const Sys& sy, const Slots& sl, const Work& w, int which, int qsel, int c, int b,
                                                int m, const BlockDesc& bd) {
  constexpr int X = M::X, V = M::V, Z = M::Z;
  const int lane = threadIdx.x & 63;
  const int sl_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S;
  const double* q = (STATE ? pick(sl.q, sl_) : (qsel ? w.qb : pick(sl.q, sl_ ^ 1))) + (size_t)c * sy.Q;
  const double* traj = (STATE ? pick(sl.traj, sl_) : w.trajw) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X + (size_t)m * S * X;
  double* PBr = pick(sl.PB, sl_) + ((size_t)c * sy.T * S + bd.step0 + (size_t)m * S) * (X * V);  // (STATE: written)
  const double* vbase = q + sy.U + sy.V0 + ((size_t)bd.step0 + (size_t)m * S) * V;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double Wacc[X * Z], Sacc[X * X], Pf[X * X];
#pragma unroll
  for (int i = 0; i < X * Z; ++i) Wacc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < X * X; ++i) Sacc[i] = 0.0, Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
  const int ntile = (S + 63) >> 6;
  struct Raw {
    double x[X], v[V], jp[X * V];
    bool valid;
  };
  auto fetch = [&](int t, Raw& r) {
    const int off = (t << 6) + (63 - lane);  // later steps in lower lanes (DPP prefix scans)
    r.valid = t >= 0 && off < S;
    if (r.valid) {
#pragma unroll
      for (int a = 0; a < X; ++a) r.x[a] = ld_stream(traj + (size_t)off * X + a);
#pragma unroll
      for (int a = 0; a < V; ++a) r.v[a] = vbase[(size_t)off * V + a];
      if constexpr (!STATE) {
#pragma unroll
        for (int k = 0; k < X * V; ++k) r.jp[k] = ld_stream(PBr + (size_t)off * (X * V) + k);
      }
    } else {
#pragma unroll
      for (int a = 0; a < X; ++a) r.x[a] = 0.0;
#pragma unroll
      for (int a = 0; a < V; ++a) r.v[a] = 0.0;
#pragma unroll
      for (int k = 0; k < X * V; ++k) r.jp[k] = 0.0;
    }
  };
  Raw r0, r1;
  fetch(ntile - 1, r0);
  for (int t = ntile - 1; t >= 0; --t) {
    fetch(t - 1, r1);
    double A[X * X], Bm[X * V], Zf[X * Z];
    if (r0.valid) {
      M::jac(cc.k, r0.x, r0.v, A, Bm, Zf);
    } else {
#pragma unroll
      for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
      for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
    }
    double Inc[X * X], E[X * X], I0[X * X], PE[X * X], T[X * V];
    dpp_prefix_products<X>(A, Inc, E);
#pragma unroll
    for (int i = 0; i < X * X; ++i) I0[i] = bcast_lane63(Inc[i]);
    matmul_xx<X>(Pf, E, PE);
#pragma unroll
    for (int a = 0; a < X; ++a)
#pragma unroll
      for (int d = 0; d < V; ++d) {
        double tt2 = 0.0;
#pragma unroll
        for (int e = 0; e < X; ++e) tt2 += PE[a * X + e] * Bm[e * V + d];
        T[a * V + d] = tt2;
      }
#pragma unroll
    for (int a = 0; a < X; ++a)
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt2 = Wacc[a * Z + mz];
#pragma unroll
        for (int e = 0; e < X; ++e) tt2 += PE[a * X + e] * Zf[e * Z + mz];
        Wacc[a * Z + mz] = tt2;
      }
    if constexpr (STATE) {
      if (r0.valid) {  // PB[s] = T_s: the compact form of this step's rows (Slots::PB)
        double* dst = PBr + (size_t)((t << 6) + (63 - lane)) * (X * V);
#pragma unroll
        for (int k = 0; k < X * V; ++k) dst[k] = T[k];
      }
    }
#pragma unroll
    for (int a = 0; a < X; ++a)
#pragma unroll
      for (int a2 = 0; a2 < X; ++a2) {
        double tt2 = Sacc[a * X + a2];
#pragma unroll
        for (int d = 0; d < V; ++d) tt2 += T[a * V + d] * (STATE ? T[a2 * V + d] : r0.jp[a2 * V + d]);
        Sacc[a * X + a2] = tt2;
      }
    {
      double Pn[X * X];
      matmul_xx<X>(Pf, I0, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pf[i] = Pn[i];
    }
    r0 = r1;
  }
  double* out = w.ivl + (cb * sy.NOBS + m) * CHMC_IVL_N(X, Z);
#pragma unroll
  for (int i = 0; i < X * X; ++i) {
    double v = Sacc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) out[i] = v;
  }
#pragma unroll
  for (int i = 0; i < X * Z; ++i) {
    double v = Wacc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) out[X * X + i] = v;
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < X * X; ++i) out[X * X + X * Z + i] = Pf[i];
  }
}
template <class M, bool STATE = false>
__global__ void __launch_bounds__(64, CHMC_IVL_WAVES) k_newton_ivl(Sys sy, Slots sl, Work w, int which, int qsel) {
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K * sy.NOBS) return;
  const int m = wid % sy.NOBS;
  const int cbi = sy.order[wid / sy.NOBS];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (STATE ? !w.ok[c] : !newton_select(w, c, which, qsel)) return;
  const BlockDesc bd = sy.blk[b];
  if (m >= bd.nobs) return;
  newton_ivl_body<M, STATE>(sy, sl, w, which, qsel, c, b, m, bd);
}
// ... of the iterates of two problems against the same previous point (KernelPlan::pair_passes): a workgroup of two
// wavefronts per (chain, block, interval), wavefront 0 on the iterate of w0, wavefront 1 on that of w1.  Both ask for the same
// lines of Slots::PB at the same time on one compute unit; everything else a wavefront touches is its own problem's.  Nothing
// is shared between the two (no LDS, no barrier): each returns on its own when its chain is out of its problem's loop.
template <class M>
__global__ void __launch_bounds__(128, CHMC_IVL_WAVES) k_newton_ivl_pair(Sys sy, Slots sl, Work w0, int which, int qsel, Work w1) {
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K * sy.NOBS) return;
  const bool second = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) != 0;
  const Work w = second ? w1 : w0;
  const int m = wid % sy.NOBS;
  const int cbi = sy.order[wid / sy.NOBS];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!newton_select(w, c, which, qsel)) return;
  const BlockDesc bd = sy.blk[b];
  if (m >= bd.nobs) return;
  newton_ivl_body<M, false>(sy, sl, w, which, qsel, c, b, m, bd);
}

// FACTOR (Newton mode, one 16-row block per chain): the block's LU, Woodbury solve, multipliers and mu_F
// (k_newton_factor_wave<.., FUSE>) follow in the same launch, fed from the LDS copies of the Gram block and the dc/du rows.
// newton_comb_body: the combine step of block (c, b) by ONE wavefront (which / qsel already resolved for the chain); its LDS
// arrays serve one wavefront per workgroup.  Shared by k_newton_comb and the per-chain retraction kernel.
template <class M, int RM, bool STATE, bool FACTOR>
__device__ __forceinline__ void newton_comb_body(const Sys& sy, const Slots& sl, const Work& w, int which, int qsel, int c, int b,
                                                 const BlockDesc& bd) {
  constexpr int X = M::X, Z = M::Z, U = M::U, V0 = M::V0;
  constexpr int NI = CHMC_IVL_N(X, Z);
  static_assert(!(STATE && FACTOR), "the factor step belongs to a Newton iteration");
  __shared__ double LamF[RM * X], LamN[RM * X], Dl[RM * RM], zl[RM * Z], Ys[RM * X], Iv[NI], JuS[FACTOR ? RM * M::U : 1];
  const int lane = threadIdx.x & 63;
  const int sl_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const double* q = (STATE ? pick(sl.q, sl_) : (qsel ? w.qb : pick(sl.q, sl_ ^ 1))) + (size_t)c * sy.Q;
  const double* traj = (STATE ? pick(sl.traj, sl_) : w.trajw) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  double* Jr = pick(sl.Jv, sl_) + (size_t)c * RM * NV;  // (STATE: the v_0 columns are written)
  double* LFr = pick(sl.LF, sl_) + cb * sy.NOBS * RM * X;  // (STATE: written)
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  for (int e = lane; e < RM * X; e += 64) LamF[e] = 0.0;
  for (int e = lane; e < RM * RM; e += 64) Dl[e] = 0.0;
  for (int e = lane; e < RM * Z; e += 64) zl[e] = 0.0;
  lds_sync();
  // (measured, round 4: staging the interval matrices, the previous point's frames and the observation gradients of ALL
  // intervals in LDS before this walk does not shorten the launch -- 9.9 -> 10.2 us: with 20 wavefronts per CU the walk's
  // round trips are hidden, unlike in the one-wavefront-per-chain kernels)
  for (int m = bd.nobs - 1; m >= 0; --m) {
    // rows that start at the end of observation interval m
    if (m < bd.ny) {
      double g[X], gl = 0.0;
      M::obs_grad(traj + (size_t)(m + 1) * S * X, g);
#pragma unroll
      for (int a = 0; a < X; ++a) gl = lane == a ? g[a] : gl;
      if (lane < X) LamF[m * X + lane] = gl;
    }
    if (m == bd.nobs - 1 && !bd.last) {
      if (lane < X) LamF[(bd.ny + lane) * X + lane] = 1.0;
    }
    const double* iv = w.ivl + (cb * sy.NOBS + m) * NI;
    for (int e = lane; e < NI; e += 64) Iv[e] = iv[e];
    lds_sync();
    if constexpr (STATE) {  // the frame of interval m (Slots::LF)
      for (int e = lane; e < RM * X; e += 64) LFr[(size_t)m * RM * X + e] = LamF[e];
    }
    // Ys[jj][a] = sum_a2 Ss[a][a2] LFprev[m][jj][a2]   (STATE: the point's own frame)
    for (int e = lane; e < RM * X; e += 64) {
      const int jj = e / X, a = e - jj * X;
      const double* lf = STATE ? LamF + jj * X : LFr + ((size_t)m * RM + jj) * X;
      double tt = 0.0;
#pragma unroll
      for (int a2 = 0; a2 < X; ++a2) tt += Iv[a * X + a2] * lf[a2];
      Ys[e] = tt;
    }
    lds_sync();
    for (int e = lane; e < RM * RM; e += 64) {
      const int i = e / RM, jj = e - i * RM;
      double tt = Dl[e];
#pragma unroll
      for (int a = 0; a < X; ++a) tt += LamF[i * X + a] * Ys[jj * X + a];
      Dl[e] = tt;
    }
    for (int e = lane; e < RM * Z; e += 64) {
      const int i = e / Z, mz = e - i * Z;
      double tt = zl[e];
#pragma unroll
      for (int a = 0; a < X; ++a) tt += LamF[i * X + a] * Iv[X * X + a * Z + mz];
      zl[e] = tt;
    }
    // the rows at the interval's start: LamF Pt[m]
    for (int e = lane; e < RM * X; e += 64) {
      const int i = e / X, d = e - i * X;
      double tt = 0.0;
#pragma unroll
      for (int a = 0; a < X; ++a) tt += LamF[i * X + a] * Iv[X * X + X * Z + a * X + d];
      LamN[e] = tt;
    }
    lds_sync();
    for (int e = lane; e < RM * X; e += 64) LamF[e] = LamN[e];
    lds_sync();
  }
  // x_0 = generate_x_0(z, v_0): the v_0 columns and the z-dependence of the first block
  if (bd.first) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    for (int e = lane; e < RM * RM; e += 64) {
      const int i = e / RM, jj = e - i * RM;
      double tt = Dl[e];
      for (int d = 0; d < V0; ++d) {
        double j0 = 0.0, j1 = 0.0;
        for (int a = 0; a < X; ++a) j0 += LamF[i * X + a] * dv0[a * V0 + d], j1 += LamF[jj * X + a] * dv0[a * V0 + d];
        tt += j0 * (STATE ? j1 : Jr[(size_t)jj * NV + d]);
        if (STATE && jj == 0) Jr[(size_t)i * NV + d] = j0;  // the rows' v_0 columns
      }
      Dl[e] = tt;
    }
    for (int e = lane; e < RM * Z; e += 64) {
      const int i = e / Z, mz = e - i * Z;
      double tt = zl[e];
      for (int a = 0; a < X; ++a) {
        double dzs = 0.0;
#pragma unroll
        for (int ee = 0; ee < X * Z; ++ee) dzs = ee == a * Z + mz ? dz[ee] : dzs;
        tt += LamF[i * X + a] * dzs;
      }
      zl[e] = tt;
    }
  }
  lds_sync();
  for (int e = lane; e < RM * RM; e += 64) {  // noise term on the observation rows, identity padding
    const int i = e / RM, jj = e - i * RM;
    double v = Dl[e];
    if (i == jj) {
      const double sg_ = sy.noisy ? sigma_at(sy, q, c) : 0.0;
      if (sy.noisy && i < bd.ny) v += sg_ * sigma_at(sy, pick(sl.q, sl_) + (size_t)c * sy.Q, c);  // dc_dn_l * dc_dn_r (:772-791)
      if (i >= bd.nrows) v = 1.0;
    }
    if constexpr (FACTOR) Dl[e] = v;
    else w.Dw[cb * RM * RM + e] = v;
  }
  double G[Z * Z];
  M::gz_jac(q, G);
  for (int e = lane; e < RM * U; e += 64) {  // dc/du rows of the iterate through generate_z'(u)
    const int i = e / U, d = e - i * U;
    double tt = 0.0;
    if (d < Z) {
      for (int mz = 0; mz < Z; ++mz) {
        double gs = 0.0;
#pragma unroll
        for (int ee = 0; ee < Z * Z; ++ee) gs = ee == mz * Z + d ? G[ee] : gs;
        tt += zl[i * Z + mz] * gs;
      }
    } else {
      tt = i < bd.ny ? sigma_at(sy, q, c) * q[sy.U + sy.NV + bd.obs0 + i] : 0.0;
    }
    if constexpr (FACTOR) JuS[e] = tt;
    else (STATE ? pick(sl.JuP, sl_) : w.JuL)[cb * RM * U + e] = tt;
  }
  if constexpr (STATE) {
    for (int e = lane; e < RM * Z; e += 64) w.zbP[cb * RM * Z + e] = zl[e];
  }
  if constexpr (FACTOR) {
    lds_sync();
    newton_factor16<M, RM, true>(sy, sl, w, which, qsel, c, b, lane < 16, Dl, JuS);
  }
}
template <class M, int RM, bool STATE = false, bool FACTOR = false>
__global__ void __launch_bounds__(64) k_newton_comb(Sys sy, Slots sl, Work w, int which, int qsel) {
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (STATE ? !w.ok[c] : !newton_select(w, c, which, qsel)) return;
  const BlockDesc bd = sy.blk[b];
  newton_comb_body<M, RM, STATE, FACTOR>(sy, sl, w, which, qsel, c, b, bd);
}
// ... for two problems in one grid, split as k_fwd_scan<.., PAIR> splits its own: the first B K workgroups combine the
// interval sums of w0, the next B K those of w1 (latency bound: twice the wavefronts take about as long as one set)
template <class M, int RM>
__global__ void __launch_bounds__(64) k_newton_comb_pair(Sys sy, Slots sl, Work w0, int which, int qsel, Work w1) {
  const int n = sy.B * sy.K;
  const bool second = (int)blockIdx.x >= n;
  const int wid = second ? (int)blockIdx.x - n : (int)blockIdx.x;
  if (wid >= n) return;
  const Work w = second ? w1 : w0;
  const int cbi = sy.order[wid];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!newton_select(w, c, which, qsel)) return;
  const BlockDesc bd = sy.blk[b];
  newton_comb_body<M, RM, false, false>(sy, sl, w, which, qsel, c, b, bd);
}

// Reverse sweep for 16-row blocks with the row-indexed state in LDS (see k_gld_bwd_wave_ldsrows: at 16 rows the fully
// unrolled k_rev_wave<.., GRAM = false> keeps 48 + 64 + 48 doubles of rows per lane and spills).  The row loop is rolled;
// the carried adjoint rows (wave-uniform) and the per-lane dc/dz partial sums (one LDS column per lane, conflict-free)
// are indexed by the row at run time; a row's dc/dv entries are stored as soon as they are formed.  MODE as k_rev_wave:
// 0 = state evaluation (rows into the slot, dc/du rows into the slot, dc/dz rows into work.zbP), 1 = Newton iterate
// (rows into work.JvW, dc/du rows into work.JuL).  The Gram block is formed afterwards by k_gram_rows.
template <class M, int RM, int MODE>
__global__ void __launch_bounds__(64) k_rev_wave_ldsrows(Sys sy, Slots sl, Work w, int which, int qsel) {
  constexpr int X = M::X, V = M::V, Z = M::Z, U = M::U, V0 = M::V0;
  __shared__ double LamS[RM * X];
  __shared__ double zaccS[RM * Z * 64];
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (MODE == 1 ? !newton_select(w, c, which, qsel) : !w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int sl_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const double* q = (MODE == 1 ? (qsel ? w.qb : pick(sl.q, sl_ ^ 1)) : pick(sl.q, sl_)) + (size_t)c * sy.Q;
  const double* traj = (MODE == 1 ? w.trajw : pick(sl.traj, sl_)) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  double* Jo = (MODE == 1 ? w.JvW : pick(sl.Jv, sl_)) + (size_t)c * RM * NV;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const size_t colb = (size_t)sy.V0 + (size_t)bd.step0 * V;
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  for (int i = lane; i < RM * X; i += 64) LamS[i] = 0.0;
  for (int i = 0; i < RM * Z; ++i) zaccS[i * 64 + lane] = 0.0;
  lds_sync();
  double* PBo = nullptr;  // compact rows of the evaluated state (MODE 0): Slots::PB / Slots::LF
  double* LFo = nullptr;
  if (MODE == 0 && pick(sl.PB, sl_)) {
    PBo = pick(sl.PB, sl_) + (size_t)c * sy.T * sy.S * (X * V);
    LFo = pick(sl.LF, sl_) + cb * sy.NOBS * RM * X;
  }
  double Pf[X * X];
#pragma unroll
  for (int i = 0; i < X * X; ++i) Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
  const int ntile = (S + 63) >> 6;
  struct Raw {
    double x[X], v[V];
    bool valid;
    int s;
  };
  auto fetch = [&](int tt, Raw& r) {
    const int jj = tt / ntile, t = tt - jj * ntile;
    const int off = (t << 6) + (63 - lane);  // later steps in lower lanes (DPP prefix scans)
    r.valid = tt >= 0 && off < S;
    r.s = jj * S + off;
#pragma unroll
    for (int a = 0; a < X; ++a) r.x[a] = r.valid ? ld_stream(traj + (size_t)r.s * X + a) : 0.0;
#pragma unroll
    for (int a = 0; a < V; ++a) r.v[a] = r.valid ? vbase[(size_t)r.s * V + a] : 0.0;
  };
  Raw r0, r1;
  fetch(bd.nobs * ntile - 1, r0);
  for (int tt = bd.nobs * ntile - 1; tt >= 0; --tt) {
    const int j = tt / ntile, t = tt - j * ntile;
    fetch(tt - 1, r1);  // next (earlier) tile's raw inputs
    if (t == ntile - 1) {  // rows that start at the end of observation interval j
      if (j < bd.ny) {
        double g[X], gl = 0.0;
        M::obs_grad(traj + (size_t)(j + 1) * S * X, g);
#pragma unroll
        for (int a = 0; a < X; ++a) gl = lane == a ? g[a] : gl;
        if (lane < X) LamS[j * X + lane] = gl;
      }
      if (j == bd.nobs - 1 && !bd.last) {
        if (lane < X) LamS[(bd.ny + lane) * X + lane] = 1.0;
      }
      lds_sync();
      if (MODE == 0 && PBo) {  // compact rows (Slots::PB / LF): the frame of interval j, products restart
        for (int e = lane; e < RM * X; e += 64) LFo[(size_t)j * RM * X + e] = LamS[e];
#pragma unroll
        for (int i = 0; i < X * X; ++i) Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
      }
    }
    double A[X * X], Bm[X * V], Zf[X * Z];
    if (r0.valid) {
      M::jac(cc.k, r0.x, r0.v, A, Bm, Zf);
    } else {
#pragma unroll
      for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
      for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
    }
    double Inc[X * X], Eex[X * X];  // inclusive / exclusive products of the later steps (lower lanes)
    dpp_prefix_products<X>(A, Inc, Eex);
    double E[X * X], I0[X * X];
#pragma unroll
    for (int i = 0; i < X * X; ++i) {
      E[i] = Eex[i];
      I0[i] = bcast_lane63(Inc[i]);
    }
    const size_t col = colb + (size_t)r0.s * V;
    if (MODE == 0 && PBo) {  // PB[s] = Pf E_s B_s: the row-independent factor of the step's rows
      double PE[X * X];
      matmul_xx<X>(Pf, E, PE);
      if (r0.valid) {
        double* dst = PBo + (size_t)(bd.step0 + r0.s) * (X * V);
#pragma unroll
        for (int a = 0; a < X; ++a)
#pragma unroll
          for (int d = 0; d < V; ++d) {
            double tt2 = 0.0;
#pragma unroll
            for (int e = 0; e < X; ++e) tt2 += PE[a * X + e] * Bm[e * V + d];
            dst[a * V + d] = tt2;
          }
      }
      double Pn[X * X];
      matmul_xx<X>(Pf, I0, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pf[i] = Pn[i];
    }
#pragma unroll 1
    for (int i = 0; i < RM; ++i) {  // rolled: everything indexed by i lives in LDS or global memory
      double Ls[X];
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt2 = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt2 += LamS[i * X + a] * E[a * X + d];
        Ls[d] = tt2;
      }
      if (r0.valid) {
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt2 = 0.0;
#pragma unroll
          for (int a = 0; a < X; ++a) tt2 += Ls[a] * Bm[a * V + d];
          Jo[(size_t)i * NV + col + d] = tt2;
        }
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt2 = zaccS[(i * Z + mz) * 64 + lane];
#pragma unroll
        for (int a = 0; a < X; ++a) tt2 += Ls[a] * Zf[a * Z + mz];
        zaccS[(i * Z + mz) * 64 + lane] = tt2;
      }
    }
    {  // Lam <- Lam I0: entry e = (row, component) by lane e
      double nl = 0.0;
      const int e = lane < RM * X ? lane : 0, ei = e / X, ed = e - ei * X;
#pragma unroll
      for (int a = 0; a < X; ++a) {
        double i0 = 0.0;
#pragma unroll
        for (int d = 0; d < X; ++d) i0 = d == ed ? I0[a * X + d] : i0;
        nl += LamS[ei * X + a] * i0;
      }
      lds_sync();
      if (lane < RM * X) LamS[e] = nl;
      lds_sync();
    }
    r0 = r1;
  }
  // x_0 = generate_x_0(z, v_0): the v_0 columns and the z-dependence of the first block (lane 0's share)
  if (bd.first && lane == 0) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    for (int i = 0; i < RM; ++i) {
      for (int d = 0; d < V0; ++d) {
        double tt = 0.0;
        for (int a = 0; a < X; ++a) tt += LamS[i * X + a] * dv0[a * V0 + d];
        Jo[(size_t)i * NV + d] = tt;
      }
      for (int mz = 0; mz < Z; ++mz) {
        double tt = 0.0;
        for (int a = 0; a < X; ++a) tt += LamS[i * X + a] * dz[a * Z + mz];
        zaccS[(i * Z + mz) * 64] += tt;
      }
    }
  }
  lds_sync();
  // dc/dz rows: sums over the lanes; entry e by lane e (RM Z = 64 entries for 16 rows)
  double G[Z * Z];
  M::gz_jac(q, G);
  double* ju = (MODE == 0 ? pick(sl.JuP, sl_) : w.JuL) + cb * RM * U;
  for (int e0 = 0; e0 < RM * Z; e0 += 64) {
    const int e = e0 + lane;
    double sum = 0.0;
    if (e < RM * Z)
      for (int l = 0; l < 64; ++l) sum += zaccS[e * 64 + ((l + lane) & 63)];  // (rotated: conflict-free)
    lds_sync();
    if (e < RM * Z) zaccS[e * 64] = sum;
    lds_sync();
    if (MODE == 0 && e < RM * Z) w.zbP[cb * RM * Z + e] = sum;
  }
  for (int e = lane; e < RM * U; e += 64) {  // dc/du rows through generate_z'(u); the sigma column with variable noise
    const int i = e / U, d = e - i * U;
    double tt = 0.0;
    if (d < Z) {
      for (int mz = 0; mz < Z; ++mz) tt += zaccS[(i * Z + mz) * 64] * G[mz * Z + d];
    } else {
      tt = i < bd.ny ? sigma_at(sy, q, c) * q[sy.U + sy.NV + bd.obs0 + i] : 0.0;
    }
    ju[e] = tt;
  }
}

// Gram block of a (chain, block) from stored rows (16-row blocks, see k_rev_wave<.., GRAM = false>):
//   D = Ja Jb^T + sigma^2 on the observation rows + identity padding      (compute_D_blocks :765-792, :742-744)
// Ja: rows of the iterate (work.JvW) or of the slot itself, Jb: stored rows of slot `which`.  One wavefront per
// (chain, block, group of NRG rows): NRG x RM accumulators per lane, lanes stride over the block's columns.
template <int RM, int NRG>
__global__ void __launch_bounds__(256) k_gram_rows(Sys sy, Slots sl, Work w, int which, int newton, int qsel) {
  constexpr int NG = RM / NRG;
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= sy.B * sy.K * NG) return;
  const int g = wid % NG;
  const int cbi = sy.order[wid / NG];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (newton ? !newton_select(w, c, which, qsel) : !w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const double* Jb = pick(sl.Jv, s) + (size_t)c * RM * sy.NV + bd.col0;
  const double* Ja = (newton ? w.JvW : pick(sl.Jv, s)) + (size_t)c * RM * sy.NV + bd.col0 + (size_t)g * NRG * sy.NV;
  double acc[NRG * RM];
#pragma unroll
  for (int i = 0; i < NRG * RM; ++i) acc[i] = 0.0;
  for (int k = lane; k < bd.ncols; k += 64) {
    double a[NRG], bb[RM];
#pragma unroll
    for (int i = 0; i < NRG; ++i) a[i] = Ja[(size_t)i * sy.NV + k];
#pragma unroll
    for (int j = 0; j < RM; ++j) bb[j] = Jb[(size_t)j * sy.NV + k];
#pragma unroll
    for (int i = 0; i < NRG; ++i)
#pragma unroll
      for (int j = 0; j < RM; ++j) acc[i * RM + j] += a[i] * bb[j];
  }
#pragma unroll
  for (int i = 0; i < NRG * RM; ++i) {
    double v = acc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[i] = v;
  }
  if (lane == 0) {
    // dc_dn_l * dc_dn_r: sigma at the point of the rows Ja (the Newton iterate, or the slot itself) times sigma of the slot
    const double sgb = sy.noisy ? sigma_at(sy, pick(sl.q, s) + (size_t)c * sy.Q, c) : 0.0;
    const double s2 = sgb * (newton && sy.noisy ? sigma_at(sy, (qsel ? w.qb : pick(sl.q, s ^ 1)) + (size_t)c * sy.Q, c) : sgb);
    double* Do = w.Dw + cb * RM * RM + (size_t)g * NRG * RM;
#pragma unroll
    for (int i = 0; i < NRG; ++i) {
      const int gi = g * NRG + i;
#pragma unroll
      for (int j = 0; j < RM; ++j) {
        double v = acc[i * RM + j];
        if (gi == j) {
          if (sy.noisy && gi < bd.ny) v += s2;
          if (gi >= bd.nrows) v = 1.0;
        }
        Do[i * RM + j] = v;
      }
    }
  }
}

// The same Gram block on the matrix cores: D (16 x 16) = Ja Jb^T as a chain of v_mfma_f64_16x16x4_f64, ONE wavefront
// per (chain, block).  This is the dense J J^T contraction of compute_D_blocks (:765-792) that BASELINE.json's config 5
// names.  It needs the rows in memory: 16-row blocks (the stored-rows path of the SIR single-block layout) fill the
// hardware tile; blocks of at most 8 rows (the 7-row FitzHugh-Nagumo blocks) use it on the stored-rows family only, with
// the block's columns folded into the tile twice (below) -- their default kernels form the Gram in registers with the
// time index across the lanes, the transpose of what the instruction wants, and never store the rows (DESIGN.md
// section 4; profiles/mfma_gram_utilisation_fhn_s800.txt).
//   operand layout (cdna_hip_programming.md section 3): lane l, r = l & 15, g = l >> 4 supplies A[i = r][k = g] and
//   B[k = g][j = r]; result register m holds D[row = g + 4 m][col = r].
// Columns are read the coalesced way (lane = column, 512 contiguous bytes per row and instruction, next tile's loads in
// flight during the current tile's MFMAs), parked in LDS (row stride 66 doubles: conflict-free ds_read_b64 of a [r][4 m + g]
// pattern) and read back in operand layout: 16 MFMAs per tile of 64 columns.
typedef double v4d_t __attribute__((ext_vector_type(4)));
template <int RM>
__global__ void __launch_bounds__(64) k_gram_rows_mfma(Sys sy, Slots sl, Work w, int which, int newton, int qsel) {
  static_assert(RM <= 8 || RM == 16, "the MFMA Gram kernel is the 16 x 16 x 4 fp64 tile: 16 rows, or at most 8 rows twice");
  constexpr int LDT = 66;
  __shared__ double ta[16 * LDT], tb[16 * LDT];
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (newton ? !newton_select(w, c, which, qsel) : !w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const double* Jb = pick(sl.Jv, s) + (size_t)c * RM * sy.NV + bd.col0;
  const double* Ja = (newton ? w.JvW : pick(sl.Jv, s)) + (size_t)c * RM * sy.NV + bd.col0;
  const int r = lane & 15, g = lane >> 4;
  v4d_t acc = {0.0, 0.0, 0.0, 0.0};
  if constexpr (RM <= 8) {
    // Blocks of at most 8 rows: the block's columns in two halves [0, h) and [h, ncols), operand rows 0-7 = the rows over
    // the first half, rows 8-15 = the same rows over the second half (the shorter half and the rows RM .. 7 of either
    // half are zero).  The two diagonal 8 x 8 quadrants of the tile are the two halves' shares of D, the off-diagonal
    // quadrants (first half against second half) are discarded: 2 RM^2 of the tile's 256 products are useful.  A tile
    // of the loop is 64 columns of EACH half: 16 MFMAs per 128 columns.
    const int h = (bd.ncols + 1) >> 1;
    for (int i = lane; i < 16 * LDT; i += 64) ta[i] = 0.0, tb[i] = 0.0;
    double ra[2 * RM], rb[2 * RM];
    auto fetch = [&](int k0) {
      const int k = k0 + lane;
      const bool in0 = k < h, in1 = h + k < bd.ncols;
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        ra[i] = in0 ? Ja[(size_t)i * sy.NV + k] : 0.0;
        ra[RM + i] = in1 ? Ja[(size_t)i * sy.NV + h + k] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 2 * RM; ++i) rb[i] = ra[i];  // state evaluation: Ja is Jb
      if (newton) {
#pragma unroll
        for (int i = 0; i < RM; ++i) {
          rb[i] = in0 ? Jb[(size_t)i * sy.NV + k] : 0.0;
          rb[RM + i] = in1 ? Jb[(size_t)i * sy.NV + h + k] : 0.0;
        }
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < h; k0 += 64) {
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        ta[i * LDT + lane] = ra[i], tb[i * LDT + lane] = rb[i];
        ta[(8 + i) * LDT + lane] = ra[RM + i], tb[(8 + i) * LDT + lane] = rb[RM + i];
      }
      if (k0 + 64 < h) fetch(k0 + 64);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int m = 0; m < 16; ++m)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ta[r * LDT + 4 * m + g], tb[r * LDT + 4 * m + g], acc, 0, 0, 0);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
    // D[g + 4 m][r] (m = 0, 1; r < 8) = quadrant (0, 0), here, + quadrant (1, 1): registers 2, 3 of lane r + 8
    const double d0 = acc[0] + __shfl_down(acc[2], 8, 64), d1 = acc[1] + __shfl_down(acc[3], 8, 64);
    const double sgb = sy.noisy ? sigma_at(sy, pick(sl.q, s) + (size_t)c * sy.Q, c) : 0.0;
    const double s2 = sgb * (newton && sy.noisy ? sigma_at(sy, (qsel ? w.qb : pick(sl.q, s ^ 1)) + (size_t)c * sy.Q, c) : sgb);
    double* Do = w.Dw + cb * RM * RM;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int gi = g + 4 * m, j = r;  // row of Ja, row of Jb
      double v = m == 0 ? d0 : d1;
      if (gi == j) {
        if (sy.noisy && gi < bd.ny) v += s2;
        if (gi >= bd.nrows) v = 1.0;
      }
      if (gi < RM && j < RM) Do[gi * RM + j] = v;
    }
    return;
  }
  double ra[RM], rb[RM];
  auto fetch = [&](int k0) {
    const int k = k0 + lane;
    const bool in = k < bd.ncols;
#pragma unroll
    for (int i = 0; i < RM; ++i) {
      ra[i] = in ? Ja[(size_t)i * sy.NV + k] : 0.0;
      rb[i] = in ? Jb[(size_t)i * sy.NV + k] : 0.0;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < bd.ncols; k0 += 64) {
#pragma unroll
    for (int i = 0; i < RM; ++i) ta[i * LDT + lane] = ra[i], tb[i * LDT + lane] = rb[i];
    if (k0 + 64 < bd.ncols) fetch(k0 + 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int m = 0; m < 16; ++m)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ta[r * LDT + 4 * m + g], tb[r * LDT + 4 * m + g], acc, 0, 0, 0);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  const double sgb = sy.noisy ? sigma_at(sy, pick(sl.q, s) + (size_t)c * sy.Q, c) : 0.0;
  const double s2 = sgb * (newton && sy.noisy ? sigma_at(sy, (qsel ? w.qb : pick(sl.q, s ^ 1)) + (size_t)c * sy.Q, c) : sgb);
  double* Do = w.Dw + cb * RM * RM;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int gi = g + 4 * m, j = r;  // row of Ja, row of Jb
    double v = acc[m];
    if (gi == j) {
      if (sy.noisy && gi < bd.ny) v += s2;
      if (gi >= bd.nrows) v = 1.0;
    }
    Do[gi * RM + j] = v;
  }
}

// Backward half of conditioned_diffusion_neg_log_dens_and_grad (:82-205): value and gradient of
//   1/2 sum_t ((y_t - obs_func(x_t)) / sigma)^2 + T log sigma [+ 1/2 q^T q]        (Y = 1; sigma a number, or
//   sigma = generate_sigma(u) = exp(u[Z]) with variable observation noise, :163-164, :183-187: the gradient then has the
//   component d/du[Z] = T - sum_t r_t^2 [+ u[Z]])
// by ONE adjoint sweep over the whole trajectory of a chain: one wavefront per chain, 64 consecutive steps per tile as
// in k_rev_wave, a single adjoint row that picks up -r_t / sigma^2 * d obs_func at every observation time.
template <class M>
__global__ void __launch_bounds__(256) k_nld_grad_wave(Sys sy, const double* qin, const double* trajb, int QH,
                                                       int gaussian, double* val, double* grad) {
  constexpr int X = M::X, V = M::V, Z = M::Z, V0 = M::V0;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= sy.B) return;
  const double* q = qin + (size_t)c * QH;
  const double* traj = trajb + (size_t)c * sy.TRJ;
  double* g = grad ? grad + (size_t)c * QH : nullptr;
  const double* vbase = q + sy.U + sy.V0;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const int S = sy.S, ntile = (S + 63) >> 6;
  const double sg = sigma_at(sy, q, c);  // a number, or exp(u[Z])
  const double is2 = 1.0 / (sg * sg);
  double Lam[X], zacc[Z], vsq = 0.0, rsq = 0.0;
#pragma unroll
  for (int a = 0; a < X; ++a) Lam[a] = 0.0;
#pragma unroll
  for (int a = 0; a < Z; ++a) zacc[a] = 0.0;
  for (int j = sy.T - 1; j >= 0; --j) {
    {  // source of observation j: d/dx_t [1/2 r_t^2 / sigma^2] = -r_t / sigma^2 * d obs_func(x_t)
      double og[X];
      const double* xo = traj + (size_t)(j + 1) * S * X;  // state at observation time j (wave-uniform)
      M::obs_grad(xo, og);
      const double rj = y_of(sy, c)[j] - M::obs(xo);
      rsq += rj * rj;
      const double wj = -rj * is2;
#pragma unroll
      for (int a = 0; a < X; ++a) Lam[a] += wj * og[a];
    }
    for (int t = ntile - 1; t >= 0; --t) {
      const int off = (t << 6) + (63 - lane);  // later steps in lower lanes (DPP prefix scans)
      const bool valid = off < S;
      const int s = j * S + off;
      double A[X * X], Bm[X * V], Zf[X * Z], vv[V];
      if (valid) {
        double x[X];
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = traj[(size_t)s * X + a];
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
        M::jac(cc.k, x, vv, A, Bm, Zf);
      } else {
#pragma unroll
        for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
        for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = 0.0;
      }
      double Inc[X * X], Eex[X * X];  // inclusive / exclusive products of the later steps (lower lanes)
      dpp_prefix_products<X>(A, Inc, Eex);
      double E[X * X], I0[X * X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) {
        E[i] = Eex[i];
        I0[i] = bcast_lane63(Inc[i]);
      }
      double Ls[X];
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Lam[a] * E[a * X + d];
        Ls[d] = tt;
      }
      if (valid) {
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt = gaussian ? 0.0 : vv[d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += Ls[a] * Bm[a * V + d];
          if (g) g[sy.U + sy.V0 + (size_t)s * V + d] = tt;
          vsq += vv[d] * vv[d];
        }
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt = zacc[mz];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Ls[a] * Zf[a * Z + mz];
        zacc[mz] = tt;
      }
      double nl[X];
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Lam[a] * I0[a * X + d];
        nl[d] = tt;
      }
#pragma unroll
      for (int d = 0; d < X; ++d) Lam[d] = nl[d];
    }
  }
#pragma unroll
  for (int mz = 0; mz < Z; ++mz) {
    double v = zacc[mz];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    zacc[mz] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vsq += __shfl_xor(vsq, o, 64);
  if (lane == 0) {
    double dz[X * Z], dv0[X * V0], G[Z * Z];
    M::gx0_jac(dz, dv0);
    M::gz_jac(q, G);
    for (int mz = 0; mz < Z; ++mz)
      for (int a = 0; a < X; ++a) zacc[mz] += Lam[a] * dz[a * Z + mz];
    double qsq = vsq;
    for (int d = 0; d < V0; ++d) {
      double tt = gaussian ? 0.0 : q[sy.U + d];
      for (int a = 0; a < X; ++a) tt += Lam[a] * dv0[a * V0 + d];
      if (g) g[sy.U + d] = tt;
      qsq += q[sy.U + d] * q[sy.U + d];
    }
    for (int d = 0; d < Z; ++d) {
      double tt = gaussian ? 0.0 : q[d];
      for (int mz = 0; mz < Z; ++mz) tt += zacc[mz] * G[mz * Z + d];
      if (g) g[d] = tt;
      qsq += q[d] * q[d];
    }
    if (sy.varsig) {  // log sigma = u[Z]: d/du[Z] of 1/2 sum r^2 / sigma^2 + T log sigma
      if (g) g[Z] = (gaussian ? 0.0 : q[Z]) + sy.T - rsq * is2;
      qsq += q[Z] * q[Z];
    }
    val[c] = 0.5 * rsq * is2 + sy.T * log(sg) + (gaussian ? 0.0 : 0.5 * qsq);
  }
}

// Backward half of init_objective of find_initial_state_by_gradient_descent (sde/mici_extensions.py:1582-1618; functor twin
// and scratch layout: KGdGrad, chmc_core.h): one wavefront per (chain, observation interval).  The interval is an
// independent S-step scan from x_init[t] (KGdFwd left its states in slots t S .. of the work trajectory), so there is ONE
// source, c[t] / (T X) at the interval's end, and nothing propagates across intervals: 64-step tiles are swept backwards
// with M::jac and dpp_prefix_products as in k_nld_grad_wave.  Per step lambda^T B + reg v / Q goes straight into the
// gradient; lambda^T Z_f is summed per lane and butterfly-reduced once; interval 0 carries lambda through generate_x_0 into
// the v_0 columns and the z sums.  The z partials, sum c^2 and max |c| of the interval go to part [B][T][Z + 2], which
// KGdReduce adds in interval order (no atomics).
template <class M>
__global__ void __launch_bounds__(256) k_gd_grad_wave(Sys sy, const double* qin, const double* trajb, const double* cres,
                                                      double reg, double* grad, double* part) {
  constexpr int X = M::X, V = M::V, Z = M::Z, V0 = M::V0, NP = CHMC_GD_NPART(Z);
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= (long)sy.B * sy.T) return;
  const int c = (int)(wid / sy.T), j = (int)(wid - (long)c * sy.T);
  const double* q = qin + (size_t)c * sy.Q;
  const double* traj = trajb + (size_t)c * sy.TRJ;
  double* g = grad + (size_t)c * sy.Q;
  const double* vbase = q + sy.U + sy.V0;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const int S = sy.S, ntile = (S + 63) >> 6;
  const double regq = reg / sy.Q, wsrc = 1.0 / ((double)sy.T * X);
  double Lam[X], zacc[Z], csq = 0.0, cmax = 0.0;
#pragma unroll
  for (int a = 0; a < X; ++a) {
    const double ca = cres[((size_t)c * sy.T + j) * X + a];  // wave-uniform
    Lam[a] = ca * wsrc;
    csq += ca * ca;
    cmax = gd_absmax(cmax, ca);
  }
#pragma unroll
  for (int a = 0; a < Z; ++a) zacc[a] = 0.0;
  for (int t = ntile - 1; t >= 0; --t) {
    const int off = (t << 6) + (63 - lane);  // later steps in lower lanes (DPP prefix scans)
    const bool valid = off < S;
    const size_t s = (size_t)j * S + off;
    double A[X * X], Bm[X * V], Zf[X * Z], vv[V];
    if (valid) {
      double x[X];
#pragma unroll
      for (int a = 0; a < X; ++a) x[a] = traj[s * X + a];
#pragma unroll
      for (int a = 0; a < V; ++a) vv[a] = vbase[s * V + a];
      M::jac(cc.k, x, vv, A, Bm, Zf);
    } else {
#pragma unroll
      for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
      for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
#pragma unroll
      for (int a = 0; a < V; ++a) vv[a] = 0.0;
    }
    double Inc[X * X], Eex[X * X];  // inclusive / exclusive products of the later steps (lower lanes)
    dpp_prefix_products<X>(A, Inc, Eex);
    double I0[X * X];
#pragma unroll
    for (int i = 0; i < X * X; ++i) I0[i] = bcast_lane63(Inc[i]);
    double Ls[X];
#pragma unroll
    for (int d = 0; d < X; ++d) {
      double tt = 0.0;
#pragma unroll
      for (int a = 0; a < X; ++a) tt += Lam[a] * Eex[a * X + d];
      Ls[d] = tt;
    }
    if (valid) {
#pragma unroll
      for (int d = 0; d < V; ++d) {
        double tt = regq * vv[d];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Ls[a] * Bm[a * V + d];
        g[sy.U + sy.V0 + s * V + d] = tt;
      }
    }
#pragma unroll
    for (int mz = 0; mz < Z; ++mz) {
      double tt = zacc[mz];
#pragma unroll
      for (int a = 0; a < X; ++a) tt += Ls[a] * Zf[a * Z + mz];
      zacc[mz] = tt;
    }
    double nl[X];
#pragma unroll
    for (int d = 0; d < X; ++d) {
      double tt = 0.0;
#pragma unroll
      for (int a = 0; a < X; ++a) tt += Lam[a] * I0[a * X + d];
      nl[d] = tt;
    }
#pragma unroll
    for (int d = 0; d < X; ++d) Lam[d] = nl[d];
  }
#pragma unroll
  for (int mz = 0; mz < Z; ++mz) {
    double v = zacc[mz];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    zacc[mz] = v;
  }
  if (lane == 0) {
    if (j == 0) {  // x_init[0] = generate_x_0(z, v_0): the v_0 columns and the z-dependence
      double dz[X * Z], dv0[X * V0];
      M::gx0_jac(dz, dv0);
      for (int mz = 0; mz < Z; ++mz)
        for (int a = 0; a < X; ++a) zacc[mz] += Lam[a] * dz[a * Z + mz];
      for (int d = 0; d < V0; ++d) {
        double tt = regq * q[sy.U + d];
        for (int a = 0; a < X; ++a) tt += Lam[a] * dv0[a * V0 + d];
        g[sy.U + d] = tt;
      }
    }
    double* po = part + ((size_t)c * sy.T + j) * NP;
    for (int mz = 0; mz < Z; ++mz) po[mz] = zacc[mz];
    po[Z] = csq, po[Z + 1] = cmax;
  }
}

// J w (lmult_by_jacob_constr :822-877): one wave per (chain, block); lanes stride over the block's columns
// (unit-stride loads of the RM stored rows and of the vector), butterfly reduction, lane 0 adds the dc/du and
// dc/dn terms.  Result in work.cpad.
// TWO: a second vector (the slot's pg) shares the pass over the stored rows; its result goes to work.cpad2.
template <int RM, bool TWO = false>
__global__ void __launch_bounds__(256) k_jw_wave(Sys sy, Slots sl, Work w, int which, int vsel_) {
  const bool minv = (vsel_ & 256) != 0;  // J (metric.inv @ vct): only the u-part of the block metric is not the identity
  const int vsel = vsel_ & 255;
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s = sl.cur[c] ^ which;
  const double* vct = (vsel == 0 ? pick(sl.p, s) : vsel == 1 ? w.pb : vsel == 2 ? w.vin : vsel == 4 ? pick(sl.pg, s) : pick(sl.p, s ^ 1)) + (size_t)c * sy.Q;
  const double* vct2 = pick(sl.pg, s) + (size_t)c * sy.Q;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const double* Jv = pick(sl.Jv, s) + (size_t)c * RM * sy.NV + bd.col0;
  const double* wv = vct + sy.U + bd.col0;
  const double* wv2 = vct2 + sy.U + bd.col0;
  double acc[RM], acc2[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) acc[i] = 0.0, acc2[i] = 0.0;
  // interval m of the block: only rows [m, nrows) are non-zero there (v_0 columns belong to interval 0)
  const int voff = bd.first ? sy.V0 : 0;
  const int per = sy.S * sy.V;
  // 16-byte path: two columns per lane and iteration when every row and the vector are 16-byte aligned
  const bool vec2 = ((sy.Q | sy.NV | sy.U | bd.col0 | voff | per) & 1) == 0;
  auto interval = [&](auto m0c, int k0, int k1) {  // rows [M0, nrows) over columns [k0, k1)
    constexpr int M0 = decltype(m0c)::value;
    if (vec2) {
      for (int k = k0 + 2 * lane; k < k1; k += 128) {
        const double2_ x = *reinterpret_cast<const double2_*>(wv + k);
        double2_ x2;
        if (TWO) x2 = *reinterpret_cast<const double2_*>(wv2 + k);
#pragma unroll
        for (int i = M0; i < RM; ++i)
          if (i < bd.nrows) {
            const double2_ j = *reinterpret_cast<const double2_*>(Jv + (size_t)i * sy.NV + k);
            acc[i] += j.x * x.x + j.y * x.y;
            if (TWO) acc2[i] += j.x * x2.x + j.y * x2.y;
          }
      }
    } else {
      for (int k = k0 + lane; k < k1; k += 64) {
        const double x = wv[k], x2 = TWO ? wv2[k] : 0.0;
#pragma unroll
        for (int i = M0; i < RM; ++i)
          if (i < bd.nrows) {
            const double j = Jv[(size_t)i * sy.NV + k];
            acc[i] += j * x;
            if (TWO) acc2[i] += j * x2;
          }
      }
    }
  };
  for (int m = 0; m < bd.nobs; ++m) {
    const int k0 = m == 0 ? 0 : voff + m * per, k1 = voff + (m + 1) * per;
    // the first active row is a compile-time constant inside an interval (no per-row branches in the column loop)
    switch (m < RM ? m : RM - 1) {
      case 0: interval(std::integral_constant<int, 0>{}, k0, k1); break;
      case 1: interval(std::integral_constant<int, (1 < RM ? 1 : RM - 1)>{}, k0, k1); break;
      case 2: interval(std::integral_constant<int, (2 < RM ? 2 : RM - 1)>{}, k0, k1); break;
      case 3: interval(std::integral_constant<int, (3 < RM ? 3 : RM - 1)>{}, k0, k1); break;
      case 4: interval(std::integral_constant<int, (4 < RM ? 4 : RM - 1)>{}, k0, k1); break;
      case 5: interval(std::integral_constant<int, (5 < RM ? 5 : RM - 1)>{}, k0, k1); break;
      case 6: interval(std::integral_constant<int, (6 < RM ? 6 : RM - 1)>{}, k0, k1); break;
      default: interval(std::integral_constant<int, (7 < RM ? 7 : RM - 1)>{}, k0, k1); break;  // rows 7.. of a 16-row block
    }
  }
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    double v = acc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[i] = v;
    if (TWO) {
      v = acc2[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      acc2[i] = v;
    }
  }
  if (lane < RM) {
    const int i = lane;
    double a = 0.0, a2 = 0.0;
#pragma unroll
    for (int k = 0; k < RM; ++k)
      if (k == i) a = acc[k], a2 = acc2[k];
    if (i < bd.nrows) {
      const double* ju = pick(sl.JuP, s) + (cb * RM + i) * sy.U;
      for (int d = 0; d < sy.U; ++d) a += ju[d] * (minv ? metric_inv_u(sy, c, vct, d) : vct[d]);
      const double sg = sy.noisy ? sigma_at(sy, pick(sl.q, s) + (size_t)c * sy.Q, c) : 0.0;
      if (sy.noisy && i < bd.ny) a += sg * vct[sy.U + sy.NV + bd.obs0 + i];
      if (TWO) {
        for (int d = 0; d < sy.U; ++d) a2 += ju[d] * (minv ? metric_inv_u(sy, c, vct2, d) : vct2[d]);
        if (sy.noisy && i < bd.ny) a2 += sg * vct2[sy.U + sy.NV + bd.obs0 + i];
      }
    } else {
      a = 0.0, a2 = 0.0;
    }
    w.cpad[cb * RM + i] = a;
    if (TWO) w.cpad2[cb * RM + i] = a2;
  }
}

// J w from the compact rows (Slots::PB / LF), same interface and result arrays as k_jw_wave: inside observation
// interval m the rows are LF[m][i] . PB[s], so the pass accumulates the row-independent y_m = sum_s PB[s] w_s (X values
// per lane) and applies the frame once per interval: X V doubles of rows per step instead of up to RM V.
// FIX (with TWO, 16-byte pairs): the momentum correction and pg <- dh1_dpos of KMomFixInitPg for the step columns ride along --
// the pass reads the two positions, the momentum and the gradient instead of p and pg, writes the corrected p and pg back
// (same expressions, same streaming hints) and uses them: one read of p and pg less per step (the columns outside the step
// part -- u, v_0, observation noise -- are corrected by KMomFixEdges before this launch, they are read below).
template <int RM, int X, int V, bool TWO, bool FIX = false>
__device__ __forceinline__ void jw_pb_body(const Sys& sy, const Slots& sl, const Work& w, int which, int vsel_, int wid) {
  static_assert(!FIX || (TWO && V == 2), "the fused momentum correction works on 16-byte pairs of p and pg");
  const bool minv = (vsel_ & 256) != 0;
  const int vsel = vsel_ & 255;
  const int lane = threadIdx.x & 63;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s = sl.cur[c] ^ which;
  const double* vct = (vsel == 0 ? pick(sl.p, s) : vsel == 1 ? w.pb : vsel == 2 ? w.vin : vsel == 4 ? pick(sl.pg, s) : pick(sl.p, s ^ 1)) + (size_t)c * sy.Q;
  const double* vct2 = pick(sl.pg, s) + (size_t)c * sy.Q;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const double* PB = pick(sl.PB, s) + ((size_t)c * sy.T * sy.S + bd.step0) * (X * V);
  const double* LF = pick(sl.LF, s) + cb * sy.NOBS * RM * X;
  const double* wv = vct + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const double* wv2 = vct2 + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const bool wide = V == 2 && !((sy.Q | sy.U | sy.V0) & 1);
  // (FIX: the step columns of the other operands of KMomFixInitPg, and p / pg as destinations)
  const size_t voff = (size_t)c * sy.Q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const double* fqp = FIX ? pick(sl.q, s ^ 1) + voff : nullptr;
  const double* fqn = FIX ? pick(sl.q, s) + voff : nullptr;
  const double* fgr = FIX ? pick(sl.grad, s) + voff : nullptr;
  double* fp = FIX ? pick(sl.p, s) + voff : nullptr;
  double* fpg = FIX ? pick(sl.pg, s) + voff : nullptr;
  double acc[RM], acc2[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) acc[i] = 0.0, acc2[i] = 0.0;
  for (int m = 0; m < bd.nobs; ++m) {
    double y[X], y2[X];
#pragma unroll
    for (int a = 0; a < X; ++a) y[a] = 0.0, y2[a] = 0.0;
    for (int k = m * sy.S + lane; k < (m + 1) * sy.S; k += 64) {
      double pb[X * V], x[V], x2[V];
      const double* src = PB + (size_t)k * (X * V);
      if ((X * V) % 2 == 0) {
#pragma unroll
        for (int e = 0; e < X * V; e += 2) {
          const double2_ v = ld2_stream(src + e);
          pb[e] = v.x, pb[e + 1 < X * V ? e + 1 : e] = v.y;
        }
      } else {
#pragma unroll
        for (int e = 0; e < X * V; ++e) pb[e] = ld_stream(src + e);
      }
      if constexpr (FIX) {  // KMomFixInitPg for this pair of columns
        const size_t ko = (size_t)k * V;
        const double2_ qp = ld2_stream(fqp + ko), qn = ld2_stream(fqn + ko);
        const double2_ pn = ld2_stream(fp + ko), gr = ld2_stream(fgr + ko);
        double sc;
        double2_ flow, po, go;
        if (sy.gaussian) {
          sc = w.cdt[c] / w.sdt[c];
          flow.x = (qp.x + w.sdt[c] * pn.x) / w.cdt[c], flow.y = (qp.y + w.sdt[c] * pn.y) / w.cdt[c];
        } else {
          sc = 1.0 / w.dt[c];
          flow.x = qp.x + w.dt[c] * pn.x, flow.y = qp.y + w.dt[c] * pn.y;
        }
        po.x = pn.x - sc * (flow.x - qn.x), po.y = pn.y - sc * (flow.y - qn.y);
        go.x = gr.x + (sy.gaussian ? 0.0 : qn.x), go.y = gr.y + (sy.gaussian ? 0.0 : qn.y);
        stv2(fp + ko, po, true, true);
        stv2(fpg + ko, go, true, true);
        x[0] = po.x, x[V - 1] = po.y;
        x2[0] = go.x, x2[V - 1] = go.y;
      } else if (wide) {
        const double2_ v = *reinterpret_cast<const double2_*>(wv + (size_t)k * V);
        x[0] = v.x, x[V - 1] = v.y;
        if (TWO) {
          const double2_ v2 = *reinterpret_cast<const double2_*>(wv2 + (size_t)k * V);
          x2[0] = v2.x, x2[V - 1] = v2.y;
        }
      } else {
#pragma unroll
        for (int d = 0; d < V; ++d) x[d] = wv[(size_t)k * V + d], x2[d] = TWO ? wv2[(size_t)k * V + d] : 0.0;
      }
#pragma unroll
      for (int a = 0; a < X; ++a)
#pragma unroll
        for (int d = 0; d < V; ++d) {
          y[a] += pb[a * V + d] * x[d];
          if (TWO) y2[a] += pb[a * V + d] * x2[d];
        }
    }
#pragma unroll
    for (int a = 0; a < X; ++a) {
      double v = y[a];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      y[a] = v;
      if (TWO) {
        v = y2[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        y2[a] = v;
      }
    }
    const double* lf = LF + (size_t)m * RM * X;
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int a = 0; a < X; ++a) {
        const double f = lf[i * X + a];
        acc[i] += f * y[a];
        if (TWO) acc2[i] += f * y2[a];
      }
  }
  if (lane < RM) {
    const int i = lane;
    double a = 0.0, a2 = 0.0;
#pragma unroll
    for (int k = 0; k < RM; ++k)
      if (k == i) a = acc[k], a2 = acc2[k];
    if (i < bd.nrows) {
      if (bd.first) {  // v_0 columns: from the stored rows
        const double* Jv = pick(sl.Jv, s) + (size_t)c * RM * sy.NV + (size_t)i * sy.NV;
        for (int d = 0; d < sy.V0; ++d) {
          a += Jv[d] * vct[sy.U + d];
          if (TWO) a2 += Jv[d] * vct2[sy.U + d];
        }
      }
      const double* ju = pick(sl.JuP, s) + (cb * RM + i) * sy.U;
      for (int d = 0; d < sy.U; ++d) a += ju[d] * (minv ? metric_inv_u(sy, c, vct, d) : vct[d]);
      const double sg = sy.noisy ? sigma_at(sy, pick(sl.q, s) + (size_t)c * sy.Q, c) : 0.0;
      if (sy.noisy && i < bd.ny) a += sg * vct[sy.U + sy.NV + bd.obs0 + i];
      if (TWO) {
        for (int d = 0; d < sy.U; ++d) a2 += ju[d] * (minv ? metric_inv_u(sy, c, vct2, d) : vct2[d]);
        if (sy.noisy && i < bd.ny) a2 += sg * vct2[sy.U + sy.NV + bd.obs0 + i];
      }
    } else {
      a = 0.0, a2 = 0.0;
    }
    w.cpad[cb * RM + i] = a;
    if (TWO) w.cpad2[cb * RM + i] = a2;
  }
}
template <int RM, int X, int V, bool TWO = false, bool FIX = false>
__global__ void __launch_bounds__(256) k_jw_pb(Sys sy, Slots sl, Work w, int which, int vsel_) {
  jw_pb_body<RM, X, V, TWO, FIX>(sy, sl, w, which, vsel_, blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}


// ---------------------------------------------------------------------------------------------------------------
// Gradient of 1/2 log det Gram (value_and_grad of log_det_sqrt_gram, :812-820, :1143-1146), wave per (chain, block).
// Same mathematics as KGldBlk (chmc_core.h); the two sweeps are wave-level scans over 64-step tiles:
//   forward : tangents xd_i along w_i, an AFFINE prefix scan of (A_s, d_s^(1..RM)) over the lanes,
//   backward: adjoint rows Lam (matrix suffix scan, as k_rev_wave) and the summed second-order adjoint x-bar,
//             a joint (matrix, vector) suffix scan with the Hessian contraction as the source term.
// Tangents are stored component-major ([RM*X][T*S] per chain) so both sweeps stream them with unit stride.
// PBJ (both sweeps): the stored rows are read in their compact form (Slots::PB / LF).  The weights w_i = sum_jj
// (G^-1)_i,jj dc_jj/dv_s are then  MLF[m][i] . PB[s]  with the per-interval RM x X matrix MLF[m] = (G^-1)_bb LF[m]
// (wave-uniform, formed once per interval): X V doubles per step instead of RM V, RM X V multiply-adds instead of RM RM V.
// Only the forward sweep has that form: blocks of at most 8 rows on the compact rows run k_gld_fwd_qx + k_gld_bwd_lean.
#ifndef CHMC_GLD_FWD_DPP_MAXROWS
#define CHMC_GLD_FWD_DPP_MAXROWS 16
#endif
template <class M, int RM, bool PBJ = false>
__global__ void __launch_bounds__(256) k_gld_fwd_wave(Sys sy, Slots sl, Work w, int which) {
  constexpr int X = M::X, V = M::V, Z = M::Z, V0 = M::V0;
  constexpr int URM = 64;  // (the forward sweep is correct fully unrolled at 16 rows as well; the backward sweep is not, see there)
  __shared__ double sm[4][RM * RM + RM * Z + (PBJ ? RM * X : 0)];
  const int lane = threadIdx.x & 63;
  const int wv_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wid = blockIdx.x * (blockDim.x >> 6) + wv_;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const size_t TS = (size_t)sy.T * S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, s_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* Jv = pick(sl.Jv, s_) + (size_t)c * RM * NV;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const size_t colb = (size_t)sy.V0 + (size_t)bd.step0 * V;
  double* Xd = w.Xd + (size_t)c * RM * X * TS + bd.step0;
  double* Mb = sm[wv_];
  double* zd = sm[wv_] + RM * RM;
  double* MLFs = sm[wv_] + RM * RM + RM * Z;
  const double* PBr = PBJ ? pick(sl.PB, s_) + ((size_t)c * TS + bd.step0) * (X * V) : nullptr;
  const double* LFr = PBJ ? pick(sl.LF, s_) + cb * sy.NOBS * RM * X : nullptr;
  for (int i = lane; i < RM * RM; i += 64) Mb[i] = w.gMb[cb * RM * RM + i];
  for (int i = lane; i < RM * Z; i += 64) zd[i] = w.gzd[cb * RM * Z + i];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double mlf[PBJ ? RM * X : 1];
  double xdc[RM * X];  // tangents at the start of the current tile (wave-uniform)
#pragma unroll URM
  for (int i = 0; i < RM * X; ++i) xdc[i] = 0.0;
  if (bd.first) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
#pragma unroll URM
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int a = 0; a < X; ++a) {
        double t = 0.0;
        for (int mz = 0; mz < Z; ++mz) t += dz[a * Z + mz] * zd[i * Z + mz];
        for (int d = 0; d < V0; ++d) {
          double wv = 0.0;
          for (int jj = 0; jj < RM; ++jj) wv += Mb[i * RM + jj] * Jv[(size_t)jj * NV + d];
          t += dv0[a * V0 + d] * wv;
        }
        xdc[i * X + a] = t;
      }
  }
  const int ntile = (S + 63) >> 6;
  for (int j = 0; j < bd.nobs; ++j) {
    if constexpr (PBJ) {  // MLF[j] = (G^-1)_bb LF[j], one entry per lane, then to every lane's registers
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      if (lane < RM * X) {
        const int i = lane / X, a = lane - i * X;
        double t = 0.0;
        for (int jj = 0; jj < RM; ++jj) t += Mb[i * RM + jj] * LFr[((size_t)j * RM + jj) * X + a];
        MLFs[lane] = t;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int e2 = 0; e2 < RM * X; ++e2) mlf[e2] = MLFs[e2];
    }
    for (int t = 0; t < ntile; ++t) {
      const int off = (t << 6) + lane;
      const bool valid = off < S;
      const int s = j * S + off;
      double P[X * X], e[RM * X];
      {
        double A[X * X], Bm[X * V], Zf[X * Z], jp[PBJ ? X * V : RM * V];
        if (valid) {
          double x[X], vv[V];
#pragma unroll
          for (int a = 0; a < X; ++a) x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
          for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
          M::jac(cc.k, x, vv, A, Bm, Zf);
          const size_t col = colb + (size_t)s * V;
          if constexpr (PBJ) {
#pragma unroll
            for (int k = 0; k < X * V; ++k) jp[k] = ld_stream(PBr + (size_t)s * (X * V) + k);
          } else
          // rows i < j (their observation lies before this interval) and padded slots are structurally zero
#pragma unroll URM
          for (int i = 0; i < RM; ++i) {
            const bool act = i >= j && i < bd.nrows;
#pragma unroll
            for (int d = 0; d < V; ++d) jp[i * V + d] = act ? Jv[(size_t)i * NV + col + d] : 0.0;
          }
        } else {
#pragma unroll
          for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
          for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
          for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
#pragma unroll URM
          for (int i = 0; i < (PBJ ? X * V : RM * V); ++i) jp[i] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < X * X; ++i) P[i] = A[i];
#pragma unroll URM
        for (int i = 0; i < RM; ++i) {
          double wv[V];
#pragma unroll
          for (int d = 0; d < V; ++d) {
            double tt = 0.0;
            if constexpr (PBJ) {
#pragma unroll
              for (int a = 0; a < X; ++a) tt += mlf[i * X + a] * jp[a * V + d];
            } else {
#pragma unroll URM
              for (int jj = 0; jj < RM; ++jj) tt += Mb[i * RM + jj] * jp[jj * V + d];
            }
            wv[d] = tt;
          }
#pragma unroll
          for (int a = 0; a < X; ++a) {
            double tt = 0.0;
#pragma unroll
            for (int d = 0; d < V; ++d) tt += Bm[a * V + d] * wv[d];
#pragma unroll
            for (int mz = 0; mz < Z; ++mz) tt += Zf[a * Z + mz] * zd[i * Z + mz];
            e[i * X + a] = tt;
          }
        }
      }
      // inclusive affine prefix scan: (P, e)_l maps the tangents at the tile start to those after step l
      if constexpr (RM <= CHMC_GLD_FWD_DPP_MAXROWS) {
        dpp_affine_prefix<X, RM>(P, e);  // DPP path of the vector ALU (the shuffle version below waits on the LDS crossbar)
      } else {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          double Pp[X * X], ep[RM * X], Pn[X * X];
#pragma unroll
          for (int i = 0; i < X * X; ++i) Pp[i] = __shfl_up(P[i], o, 64);
#pragma unroll URM
          for (int i = 0; i < RM * X; ++i) ep[i] = __shfl_up(e[i], o, 64);
          if (lane >= o) {
#pragma unroll URM
            for (int i = 0; i < RM; ++i)
#pragma unroll
              for (int a = 0; a < X; ++a) {
                double tt = e[i * X + a];
#pragma unroll
                for (int d = 0; d < X; ++d) tt += P[a * X + d] * ep[i * X + d];
                e[i * X + a] = tt;
              }
            matmul_xx<X>(P, Pp, Pn);
#pragma unroll
            for (int i = 0; i < X * X; ++i) P[i] = Pn[i];
          }
        }
      }
      // exclusive values: tangents AT this lane's step
      {
        double xs[RM * X];
#pragma unroll URM
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int a = 0; a < X; ++a) xs[i * X + a] = dpp_mov<0x138, 0xf, 0xf>(e[i * X + a], 0.0);  // wave_shr:1
        double Pex[X * X];
#pragma unroll
        for (int i = 0; i < X * X; ++i) Pex[i] = dpp_mov<0x138, 0xf, 0xf>(P[i], (i / X == i % X) ? 1.0 : 0.0);
#pragma unroll URM
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int a = 0; a < X; ++a) {
            double tt = xs[i * X + a];
#pragma unroll
            for (int d = 0; d < X; ++d) tt += Pex[a * X + d] * xdc[i * X + d];
            xs[i * X + a] = tt;
          }
        if (valid) {  // the tangent of row i is only needed up to that row's own observation time
#pragma unroll URM
          for (int i = 0; i < RM; ++i)
            if (i >= j && i < bd.nrows) {
#pragma unroll
              for (int a = 0; a < X; ++a) st_async(Xd + (size_t)(i * X + a) * TS + s, xs[i * X + a]);
            }
        }
      }
      // carry to the next tile: apply lane 63's inclusive map
      {
        double P6[X * X], nx[RM * X];
#pragma unroll
        for (int i = 0; i < X * X; ++i) P6[i] = bcast_lane63(P[i]);
#pragma unroll URM
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int a = 0; a < X; ++a) {
            double tt = bcast_lane63(e[i * X + a]);
#pragma unroll
            for (int d = 0; d < X; ++d) tt += P6[a * X + d] * xdc[i * X + d];
            nx[i * X + a] = tt;
          }
#pragma unroll URM
        for (int i = 0; i < RM * X; ++i) xdc[i] = nx[i];
      }
    }
    // tangent of observation row j at its terminal time (j + 1) S
    if (j < bd.ny && lane == 0) {
#pragma unroll URM
      for (int i = 0; i < RM; ++i)
        if (i == j)
#pragma unroll
          for (int a = 0; a < X; ++a) w.gxdt[(cb * RM + j) * X + a] = xdc[i * X + a];
    }
  }
}

// The forward sweep in the form the row-free backward sweep needs (Qx_s = sum_i LF[m][i]^T xd_i(s)^T, X x X per step) WITHOUT
// the RM row tangents.  Inside observation interval m the frames are constant, so Qx obeys the tangents' own recursion with
// X pseudo-rows instead of RM rows:
//     Qx_{s+1}[r] = A_s Qx_s[r] + B_s (PB_s^T C1_m[r]) + Zf_s C2_m[r],   C1_m = LF[m]^T MLF[m] (X x X),  C2_m = LF[m]^T zd (X x Z),
// started at the interval's first step from Q0_m = LF[m]^T xd(t_m).  The row tangents are only needed at the interval
// boundaries, where they follow from the state sweep's interval sums (k_state_lean leaves Ss, Ws, Pt in work.ivl):
//     xd_i(t_{m+1}) = Pt_m xd_i(t_m) + Ss_m MLF[m][i]^T + Ws_m zd_i
// -- a prologue of nobs tiny steps per block (entries over the lanes, everything RM-sized in LDS).  The affine scan of a
// tile then carries X instead of RM vectors (FitzHugh-Nagumo: 2 instead of 7).  Also writes the rows' terminal tangents
// (work.gxdt) for the backward sweep.  Blocks of at most 8 rows on the compact rows.
template <class M, int RM>
__global__ void __launch_bounds__(256) k_gld_fwd_qx(Sys sy, Slots sl, Work w, int which) {
  constexpr int X = M::X, V = M::V, Z = M::Z, V0 = M::V0;
  constexpr int NI = CHMC_IVL_N(X, Z), NC = X * X + X * Z + X * X;  // per interval: C1, C2, Q0
  // (a block has at most RM observation intervals: every observation contributes a row)
  __shared__ double sm[4][RM * RM + RM * Z + 2 * RM * X + RM * NC + NI];
  const int lane = threadIdx.x & 63;
  const int wv_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wid = blockIdx.x * (blockDim.x >> 6) + wv_;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const size_t TS = (size_t)sy.T * S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, s_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* Jv = pick(sl.Jv, s_) + (size_t)c * RM * NV;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  double* Xd = w.Xd + (size_t)c * RM * X * TS + bd.step0;
  double* Mb = sm[wv_];
  double* zd = Mb + RM * RM;
  double* MLFs = zd + RM * Z;
  double* xds = MLFs + RM * X;   // row tangents at the start of the current interval
  double* Cs = xds + RM * X;     // [nobs][C1 | C2 | Q0]
  double* Iv = Cs + RM * NC;     // the interval's sums Ss | Ws | Pt
  const double* PBr = pick(sl.PB, s_) + ((size_t)c * TS + bd.step0) * (X * V);
  const double* LFr = pick(sl.LF, s_) + cb * sy.NOBS * RM * X;
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  for (int i = lane; i < RM * RM; i += 64) Mb[i] = w.gMb[cb * RM * RM + i];
  for (int i = lane; i < RM * Z; i += 64) zd[i] = w.gzd[cb * RM * Z + i];
  lds_sync();
  // ---- prologue: row tangents at the interval boundaries, and C1, C2, Q0 of every interval
  if (lane < RM * X) {
    const int i = lane / X, a = lane - i * X;
    double t = 0.0;
    if (bd.first) {
      double dz[X * Z], dv0[X * V0];
      M::gx0_jac(dz, dv0);
      for (int mz = 0; mz < Z; ++mz) {
        double dzs = 0.0;
#pragma unroll
        for (int e2 = 0; e2 < X * Z; ++e2) dzs = e2 == a * Z + mz ? dz[e2] : dzs;
        t += dzs * zd[i * Z + mz];
      }
      for (int d = 0; d < V0; ++d) {
        double wv = 0.0, dvs = 0.0;
        for (int jj = 0; jj < RM; ++jj) wv += Mb[i * RM + jj] * Jv[(size_t)jj * NV + d];
#pragma unroll
        for (int e2 = 0; e2 < X * V0; ++e2) dvs = e2 == a * V0 + d ? dv0[e2] : dvs;
        t += dvs * wv;
      }
    }
    xds[lane] = t;
  }
  for (int j = 0; j < bd.nobs; ++j) {
    lds_sync();
    if (lane < RM * X) {  // MLF[j] = (G^-1)_bb LF[j]
      const int i = lane / X, a = lane - i * X;
      double t = 0.0;
      for (int jj = 0; jj < RM; ++jj) t += Mb[i * RM + jj] * LFr[((size_t)j * RM + jj) * X + a];
      MLFs[lane] = t;
    }
    for (int e2 = lane; e2 < NI; e2 += 64) Iv[e2] = w.ivl[(cb * sy.NOBS + j) * NI + e2];
    lds_sync();
    double* Cj = Cs + j * NC;
    if (lane < X * X) {  // C1[a1][a] = sum_i LF[j][i][a1] MLF[j][i][a];  Q0[a1][a2] = sum_i LF[j][i][a1] xd_i[a2]
      const int a1 = lane / X, a2 = lane - a1 * X;
      double c1 = 0.0, q0 = 0.0;
      for (int i = 0; i < RM; ++i) {
        const double lf = LFr[((size_t)j * RM + i) * X + a1];
        c1 += lf * MLFs[i * X + a2];
        q0 += lf * xds[i * X + a2];
      }
      Cj[lane] = c1;
      Cj[X * X + X * Z + lane] = q0;
    }
    if (lane < X * Z) {  // C2[a1][mz] = sum_i LF[j][i][a1] zd[i][mz]
      const int a1 = lane / Z, mz = lane - a1 * Z;
      double c2 = 0.0;
      for (int i = 0; i < RM; ++i) c2 += LFr[((size_t)j * RM + i) * X + a1] * zd[i * Z + mz];
      Cj[X * X + lane] = c2;
    }
    double nx = 0.0;  // row tangent at the interval's end: Pt xd_i + Ss MLF[j][i]^T + Ws zd_i
    if (lane < RM * X) {
      const int i = lane / X, a = lane - i * X;
#pragma unroll
      for (int d = 0; d < X; ++d) nx += Iv[X * X + X * Z + a * X + d] * xds[i * X + d] + Iv[a * X + d] * MLFs[i * X + d];
      for (int mz = 0; mz < Z; ++mz) nx += Iv[X * X + a * Z + mz] * zd[i * Z + mz];
    }
    lds_sync();
    if (lane < RM * X) xds[lane] = nx;
    {
      const double tv = __shfl(nx, (j * X + lane) & 63, 64);  // (every lane takes part: the sources must be active)
      if (j < bd.ny && lane < X) w.gxdt[(cb * RM + j) * X + lane] = tv;  // terminal tangent of row j
    }
  }
  lds_sync();
  // ---- the sweep: X pseudo-rows per interval
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const int ntile = (S + 63) >> 6;
  for (int j = 0; j < bd.nobs; ++j) {
    const double* Cj = Cs + j * NC;
    double c1[X * X], c2[X * Z], xdc[X * X];
#pragma unroll
    for (int i = 0; i < X * X; ++i) c1[i] = Cj[i], xdc[i] = Cj[X * X + X * Z + i];
#pragma unroll
    for (int i = 0; i < X * Z; ++i) c2[i] = Cj[X * X + i];
    for (int t = 0; t < ntile; ++t) {
      const int off = (t << 6) + lane;
      const bool valid = off < S;
      const int s = j * S + off;
      double P[X * X], e[X * X];
      {
        double A[X * X], Bm[X * V], Zf[X * Z], jp[X * V];
        if (valid) {
          double x[X], vv[V];
#pragma unroll
          for (int a = 0; a < X; ++a) x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
          for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
          M::jac(cc.k, x, vv, A, Bm, Zf);
#pragma unroll
          for (int k = 0; k < X * V; ++k) jp[k] = ld_stream(PBr + (size_t)s * (X * V) + k);
        } else {
#pragma unroll
          for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
          for (int i = 0; i < X * V; ++i) Bm[i] = 0.0, jp[i] = 0.0;
#pragma unroll
          for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < X * X; ++i) P[i] = A[i];
#pragma unroll
        for (int r = 0; r < X; ++r) {
          double wv[V];
#pragma unroll
          for (int d = 0; d < V; ++d) {
            double tt = 0.0;
#pragma unroll
            for (int a = 0; a < X; ++a) tt += c1[r * X + a] * jp[a * V + d];
            wv[d] = tt;
          }
#pragma unroll
          for (int a = 0; a < X; ++a) {
            double tt = 0.0;
#pragma unroll
            for (int d = 0; d < V; ++d) tt += Bm[a * V + d] * wv[d];
#pragma unroll
            for (int mz = 0; mz < Z; ++mz) tt += Zf[a * Z + mz] * c2[r * Z + mz];
            e[r * X + a] = tt;
          }
        }
      }
      dpp_affine_prefix<X, X>(P, e);
      {
        double xs[X * X], Pex[X * X];
#pragma unroll
        for (int i = 0; i < X * X; ++i) xs[i] = dpp_mov<0x138, 0xf, 0xf>(e[i], 0.0);  // wave_shr:1
#pragma unroll
        for (int i = 0; i < X * X; ++i) Pex[i] = dpp_mov<0x138, 0xf, 0xf>(P[i], (i / X == i % X) ? 1.0 : 0.0);
#pragma unroll
        for (int r = 0; r < X; ++r)
#pragma unroll
          for (int a = 0; a < X; ++a) {
            double tt = xs[r * X + a];
#pragma unroll
            for (int d = 0; d < X; ++d) tt += Pex[a * X + d] * xdc[r * X + d];
            xs[r * X + a] = tt;
          }
        if (valid) {
#pragma unroll
          for (int i = 0; i < X * X; ++i) st_async(Xd + (size_t)i * TS + s, xs[i]);
        }
      }
      {
        double P6[X * X], nx[X * X];
#pragma unroll
        for (int i = 0; i < X * X; ++i) P6[i] = bcast_lane63(P[i]);
#pragma unroll
        for (int r = 0; r < X; ++r)
#pragma unroll
          for (int a = 0; a < X; ++a) {
            double tt = bcast_lane63(e[r * X + a]);
#pragma unroll
            for (int d = 0; d < X; ++d) tt += P6[a * X + d] * xdc[r * X + d];
            nx[r * X + a] = tt;
          }
#pragma unroll
        for (int i = 0; i < X * X; ++i) xdc[i] = nx[i];
      }
    }
  }
}

// The backward sweep over the stored rows (the compact rows' backward sweep is k_gld_bwd_lean; 16-row blocks:
// k_gld_bwd_wave_ldsrows).
template <class M, int RM>
__global__ void __launch_bounds__(256, 1) k_gld_bwd_wave(Sys sy, Slots sl, Work w, int which) {
  constexpr int X = M::X, V = M::V, Z = M::Z, U = M::U, V0 = M::V0, NXI = M::NXI;
  constexpr int URM = RM <= 8 ? 64 : 1;
  __shared__ double sm[4][RM * RM + RM * Z];
  const int lane = threadIdx.x & 63;
  const int wv_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wid = blockIdx.x * (blockDim.x >> 6) + wv_;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const size_t TS = (size_t)sy.T * S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, s_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* Jv = pick(sl.Jv, s_) + (size_t)c * RM * NV;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const size_t colb = (size_t)sy.V0 + (size_t)bd.step0 * V;
  const double* Xd = w.Xd + (size_t)c * RM * X * TS + bd.step0;
  double* gv = pick(sl.grad, s_) + (size_t)c * sy.Q + sy.U;
  double* Mb = sm[wv_];
  double* zd = sm[wv_] + RM * RM;
  for (int i = lane; i < RM * RM; i += 64) Mb[i] = w.gMb[cb * RM * RM + i];
  for (int i = lane; i < RM * Z; i += 64) zd[i] = w.gzd[cb * RM * Z + i];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double Lam[RM * X], xb[X], zbt[Z];
#pragma unroll URM
  for (int i = 0; i < RM * X; ++i) Lam[i] = 0.0;
#pragma unroll
  for (int i = 0; i < X; ++i) xb[i] = 0.0;
#pragma unroll
  for (int i = 0; i < Z; ++i) zbt[i] = 0.0;
  const int ntile = (S + 63) >> 6;
  for (int j = bd.nobs - 1; j >= 0; --j) {
    if (j < bd.ny) {
      double g[X], hv[X], xt[X];
      for (int a = 0; a < X; ++a) xt[a] = w.gxdt[(cb * RM + j) * X + a];
      M::obs_grad(traj + (size_t)(j + 1) * S * X, g);
      M::obs_hess_vec(traj + (size_t)(j + 1) * S * X, xt, hv);
#pragma unroll URM
      for (int i = 0; i < RM; ++i)
        if (i == j)
#pragma unroll
          for (int a = 0; a < X; ++a) Lam[i * X + a] = g[a];
#pragma unroll
      for (int a = 0; a < X; ++a) xb[a] += hv[a];
    }
    if (j == bd.nobs - 1 && !bd.last) {
#pragma unroll URM
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int a = 0; a < X; ++a)
          if (i == bd.ny + a) Lam[i * X + a] = 1.0;
    }
    for (int t = ntile - 1; t >= 0; --t) {
      const int off = (t << 6) + (63 - lane);  // LATER steps in LOWER lanes: the suffix scans become DPP prefix scans
      const bool valid = off < S;
      const int s = j * S + off;
      const size_t col = colb + (size_t)s * V;
      double A[X * X], Bm[X * V], Zf[X * Z], x[X], vv[V];
      if (valid) {
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
        M::jac(cc.k, x, vv, A, Bm, Zf);
      } else {
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = 0.0;
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = 0.0;
#pragma unroll
        for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
        for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
      }
      // products of the transition matrices of the later steps (adjoint rows): exclusive prefix products over the lanes
      double Inc[X * X], E[X * X];
      dpp_prefix_products<X>(A, Inc, E);
      // Hessian contraction source of this step
      double H[NXI];
      {
        double Sm[X * NXI];
#pragma unroll
        for (int i = 0; i < X * NXI; ++i) Sm[i] = 0.0;
        double jp[RM * V];
#pragma unroll URM
        for (int i = 0; i < RM; ++i) {
          const bool act = valid && i >= j && i < bd.nrows;
#pragma unroll
          for (int d = 0; d < V; ++d) jp[i * V + d] = act ? Jv[(size_t)i * NV + col + d] : 0.0;
        }
#pragma unroll URM
        for (int i = 0; i < RM; ++i) {
          double Ls[X], dir[NXI];
#pragma unroll
          for (int d = 0; d < X; ++d) {
            double tt = 0.0;
#pragma unroll
            for (int a = 0; a < X; ++a) tt += Lam[i * X + a] * E[a * X + d];
            Ls[d] = tt;
          }
#pragma unroll
          for (int a = 0; a < X; ++a) dir[a] = (valid && i >= j && i < bd.nrows) ? Xd[(size_t)(i * X + a) * TS + s] : 0.0;
#pragma unroll
          for (int d = 0; d < V; ++d) {
            double tt = 0.0;
#pragma unroll URM
            for (int jj = 0; jj < RM; ++jj) tt += Mb[i * RM + jj] * jp[jj * V + d];
            dir[X + d] = tt;
          }
#pragma unroll
          for (int mz = 0; mz < Z; ++mz) dir[X + V + mz] = zd[i * Z + mz];
#pragma unroll
          for (int a = 0; a < X; ++a)
#pragma unroll
            for (int m2 = 0; m2 < NXI; ++m2) Sm[a * NXI + m2] += Ls[a] * dir[m2];
        }
        M::hess(cc.k, x, vv, Sm, H);
        if (!valid) {
#pragma unroll
          for (int i = 0; i < NXI; ++i) H[i] = 0.0;
        }
      }
      // joint suffix scan for x-bar: x-bar^(l) = x-bar^(l+1) A_l + Hx_l
      double I2[X * X], gi[X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) I2[i] = A[i];
#pragma unroll
      for (int a = 0; a < X; ++a) gi[a] = H[a];
      dpp_rowaffine_prefix<X>(I2, gi);
      double xbs[X];  // x-bar at the state after this lane's step
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = dpp_mov<0x138, 0xf, 0xf>(gi[d], 0.0);  // wave_shr:1: the sources of the later steps
#pragma unroll
        for (int a = 0; a < X; ++a) tt += xb[a] * E[a * X + d];
        xbs[d] = tt;
      }
      if (valid) {
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt = H[X + d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += Bm[a * V + d] * xbs[a];
          gv[col + d] = tt;
        }
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt = H[X + V + mz];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Zf[a * Z + mz] * xbs[a];
        zbt[mz] += tt;
      }
      // carries
      double I0[X * X], g0[X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) I0[i] = bcast_lane63(I2[i]);
#pragma unroll
      for (int a = 0; a < X; ++a) g0[a] = bcast_lane63(gi[a]);
      {
        double nb[X];
#pragma unroll
        for (int d = 0; d < X; ++d) {
          double tt = g0[d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += xb[a] * I0[a * X + d];
          nb[d] = tt;
        }
#pragma unroll
        for (int d = 0; d < X; ++d) xb[d] = nb[d];
      }
#pragma unroll URM
      for (int i = 0; i < RM; ++i) {
        double nl[X];
#pragma unroll
        for (int d = 0; d < X; ++d) {
          double tt = 0.0;
#pragma unroll
          for (int a = 0; a < X; ++a) tt += Lam[i * X + a] * I0[a * X + d];
          nl[d] = tt;
        }
#pragma unroll
        for (int d = 0; d < X; ++d) Lam[i * X + d] = nl[d];
      }
    }
  }
  if (bd.first && lane == 0) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    for (int d = 0; d < V0; ++d) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dv0[a * V0 + d] * xb[a];
      gv[d] = tt;
    }
    for (int mz = 0; mz < Z; ++mz) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dz[a * Z + mz] * xb[a];
      zbt[mz] += tt;
    }
  }
#pragma unroll
  for (int i = 0; i < Z; ++i) {
    double v = zbt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    zbt[i] = v;
  }
  if (lane == 0) {
    double Gz[Z * Z], gu[U];
    M::gz_jac(q, Gz);
    for (int d = 0; d < Z; ++d) {
      double tt = 0.0;
      for (int mz = 0; mz < Z; ++mz) tt += Gz[mz * Z + d] * zbt[mz];
      gu[d] = tt;
    }
    for (int i = 0; i < RM; ++i) {
      double o[Z], wu[U], zb[Z];
      for (int d = 0; d < U; ++d) wu[d] = w.gWu[(cb * RM + i) * U + d];
      for (int mz = 0; mz < Z; ++mz) zb[mz] = w.zbP[(cb * RM + i) * Z + mz];
      M::gz_hess(q, wu, zb, o);
      for (int d = 0; d < Z; ++d) gu[d] += o[d];
    }
    if constexpr (M::VS)  // variable observation noise: the sigma-dependent entries of J (see var_sigma_grad_terms)
      gu[Z] = var_sigma_grad_terms<RM>(sy, bd, q, w.gWu + cb * RM * U, U, w.gMb + cb * RM * RM,
                                       pick(sl.grad, s_) + (size_t)c * sy.Q);
    for (int d = 0; d < U; ++d) w.gup[cb * U + d] = gu[d];
  }
}


// The backward grad-log-det sweep without a row index in its hot loop (compact rows, blocks of at most 8 rows).  With the
// frames the Hessian-contraction source of a step is
//     Sm[a][.] = sum_i Ls_i[a] dir_i[.] = sum_a' PE_s[a'][a] Q_s[a'][.],    Q_s[a'][.] = sum_i LF[m][i][a'] dir_i(s)[.],
// and Q_s splits into   Qx_s = sum_i LF_i^T xd_i(s)^T  (X x X per step: formed and stored by the FORWARD sweep, which holds
// the tangents, instead of the tangents themselves -- X X doubles per step instead of up to RM X),
// Qv_s = C[m] PB[s] with C[m] = LF[m]^T MLF[m] (X x X per interval),  Qz = LF[m]^T zd (X x Z per interval).
// No adjoint rows are carried (LF[m] holds them), no per-row loads or loops: the kernel fits two wavefronts per SIMD.
#ifndef CHMC_GLD_LEAN_WAVES
#define CHMC_GLD_LEAN_WAVES 2
#endif
template <class M, int RM>
__global__ void __launch_bounds__(64, CHMC_GLD_LEAN_WAVES) k_gld_bwd_lean(Sys sy, Slots sl, Work w, int which) {
  constexpr int X = M::X, V = M::V, Z = M::Z, U = M::U, V0 = M::V0, NXI = M::NXI;
  __shared__ double Mb[RM * RM], zd[RM * Z], LFs[RM * X], MLFs[RM * X], CQ[X * X + X * Z];
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S;
  const size_t TS = (size_t)sy.T * S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, s_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const size_t colb = (size_t)sy.V0 + (size_t)bd.step0 * V;
  const double* Xq = w.Xd + (size_t)c * RM * X * TS + bd.step0;  // Qx, component-major: [X X][T S]
  double* gv = pick(sl.grad, s_) + (size_t)c * sy.Q + sy.U;
  const double* PBr = pick(sl.PB, s_) + ((size_t)c * TS + bd.step0) * (X * V);
  const double* LFr = pick(sl.LF, s_) + cb * sy.NOBS * RM * X;
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  for (int i = lane; i < RM * RM; i += 64) Mb[i] = w.gMb[cb * RM * RM + i];
  for (int i = lane; i < RM * Z; i += 64) zd[i] = w.gzd[cb * RM * Z + i];
  lds_sync();
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double xb[X], zbt[Z], Pf[X * X], Cm[X * X], Qz[X * Z];
#pragma unroll
  for (int i = 0; i < X; ++i) xb[i] = 0.0;
#pragma unroll
  for (int i = 0; i < Z; ++i) zbt[i] = 0.0;
  const int ntile = (S + 63) >> 6;
  for (int j = bd.nobs - 1; j >= 0; --j) {
    if (j < bd.ny) {
      double hv[X], xt[X];
      for (int a = 0; a < X; ++a) xt[a] = w.gxdt[(cb * RM + j) * X + a];
      M::obs_hess_vec(traj + (size_t)(j + 1) * S * X, xt, hv);
#pragma unroll
      for (int a = 0; a < X; ++a) xb[a] += hv[a];
    }
    // per-interval matrices: MLF = (G^-1)_bb LF[j], C = LF^T MLF, Qz = LF^T zd
    lds_sync();
    for (int e = lane; e < RM * X; e += 64) LFs[e] = LFr[(size_t)j * RM * X + e];
    lds_sync();
    for (int e = lane; e < RM * X; e += 64) {
      const int i = e / X, a = e - i * X;
      double t2 = 0.0;
      for (int jj = 0; jj < RM; ++jj) t2 += Mb[i * RM + jj] * LFs[jj * X + a];
      MLFs[e] = t2;
    }
    lds_sync();
    for (int e = lane; e < X * X + X * Z; e += 64) {
      double t2 = 0.0;
      if (e < X * X) {
        const int a1 = e / X, a2 = e - a1 * X;
        for (int i = 0; i < RM; ++i) t2 += LFs[i * X + a1] * MLFs[i * X + a2];
      } else {
        const int a1 = (e - X * X) / Z, mz = (e - X * X) - a1 * Z;
        for (int i = 0; i < RM; ++i) t2 += LFs[i * X + a1] * zd[i * Z + mz];
      }
      CQ[e] = t2;
    }
    lds_sync();
#pragma unroll
    for (int i = 0; i < X * X; ++i) Cm[i] = CQ[i], Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < X * Z; ++i) Qz[i] = CQ[X * X + i];
    for (int t = ntile - 1; t >= 0; --t) {
      const int off = (t << 6) + (63 - lane);  // LATER steps in LOWER lanes: the suffix scans become DPP prefix scans
      const bool valid = off < S;
      const int s = j * S + off;
      const size_t col = colb + (size_t)s * V;
      double A[X * X], Bm[X * V], Zf[X * Z], x[X], vv[V], pb[X * V], qx[X * X];
      if (valid) {
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
#pragma unroll
        for (int k = 0; k < X * V; ++k) pb[k] = ld_stream(PBr + (size_t)s * (X * V) + k);
#pragma unroll
        for (int k = 0; k < X * X; ++k) qx[k] = ld_stream(Xq + (size_t)k * TS + s);
        M::jac(cc.k, x, vv, A, Bm, Zf);
      } else {
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = 0.0;
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = 0.0;
#pragma unroll
        for (int k = 0; k < X * V; ++k) pb[k] = 0.0;
#pragma unroll
        for (int k = 0; k < X * X; ++k) qx[k] = 0.0;
#pragma unroll
        for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
        for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
      }
      double Inc[X * X], E[X * X], PE[X * X];
      dpp_prefix_products<X>(A, Inc, E);
      matmul_xx<X>(Pf, E, PE);
      // Hessian contraction source of this step: Sm = PE^T [ Qx | C PB | Qz ]
      double H[NXI];
      {
        double Q[X * NXI], Sm[X * NXI];
#pragma unroll
        for (int a1 = 0; a1 < X; ++a1) {
#pragma unroll
          for (int a2 = 0; a2 < X; ++a2) Q[a1 * NXI + a2] = qx[a1 * X + a2];
#pragma unroll
          for (int d = 0; d < V; ++d) {
            double tt = 0.0;
#pragma unroll
            for (int a2 = 0; a2 < X; ++a2) tt += Cm[a1 * X + a2] * pb[a2 * V + d];
            Q[a1 * NXI + X + d] = tt;
          }
#pragma unroll
          for (int mz = 0; mz < Z; ++mz) Q[a1 * NXI + X + V + mz] = Qz[a1 * Z + mz];
        }
#pragma unroll
        for (int a = 0; a < X; ++a)
#pragma unroll
          for (int m2 = 0; m2 < NXI; ++m2) {
            double tt = 0.0;
#pragma unroll
            for (int a1 = 0; a1 < X; ++a1) tt += PE[a1 * X + a] * Q[a1 * NXI + m2];
            Sm[a * NXI + m2] = tt;
          }
        M::hess(cc.k, x, vv, Sm, H);
        if (!valid) {
#pragma unroll
          for (int i = 0; i < NXI; ++i) H[i] = 0.0;
        }
      }
      // joint suffix scan for x-bar: x-bar^(l) = x-bar^(l+1) A_l + Hx_l
      double I2[X * X], gi[X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) I2[i] = A[i];
#pragma unroll
      for (int a = 0; a < X; ++a) gi[a] = H[a];
      dpp_rowaffine_prefix<X>(I2, gi);
      double xbs[X];  // x-bar at the state after this lane's step
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = dpp_mov<0x138, 0xf, 0xf>(gi[d], 0.0);  // wave_shr:1: the sources of the later steps
#pragma unroll
        for (int a = 0; a < X; ++a) tt += xb[a] * E[a * X + d];
        xbs[d] = tt;
      }
      if (valid) {
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt = H[X + d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += Bm[a * V + d] * xbs[a];
          gv[col + d] = tt;
        }
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt = H[X + V + mz];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Zf[a * Z + mz] * xbs[a];
        zbt[mz] += tt;
      }
      // carries
      double I0[X * X], g0[X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) I0[i] = bcast_lane63(I2[i]);
#pragma unroll
      for (int a = 0; a < X; ++a) g0[a] = bcast_lane63(gi[a]);
      {
        double nb[X];
#pragma unroll
        for (int d = 0; d < X; ++d) {
          double tt = g0[d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += xb[a] * I0[a * X + d];
          nb[d] = tt;
        }
#pragma unroll
        for (int d = 0; d < X; ++d) xb[d] = nb[d];
      }
      {
        double Pn[X * X];
        matmul_xx<X>(Pf, I0, Pn);
#pragma unroll
        for (int i = 0; i < X * X; ++i) Pf[i] = Pn[i];
      }
    }
  }
  if (bd.first && lane == 0) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    for (int d = 0; d < V0; ++d) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dv0[a * V0 + d] * xb[a];
      gv[d] = tt;
    }
    for (int mz = 0; mz < Z; ++mz) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dz[a * Z + mz] * xb[a];
      zbt[mz] += tt;
    }
  }
#pragma unroll
  for (int i = 0; i < Z; ++i) {
    double v = zbt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    zbt[i] = v;
  }
  if (lane == 0) {
    double Gz[Z * Z], gu[U];
    M::gz_jac(q, Gz);
    for (int d = 0; d < Z; ++d) {
      double tt = 0.0;
      for (int mz = 0; mz < Z; ++mz) tt += Gz[mz * Z + d] * zbt[mz];
      gu[d] = tt;
    }
    for (int i = 0; i < RM; ++i) {
      double o[Z], wu[U], zb[Z];
      for (int d = 0; d < U; ++d) wu[d] = w.gWu[(cb * RM + i) * U + d];
      for (int mz = 0; mz < Z; ++mz) zb[mz] = w.zbP[(cb * RM + i) * Z + mz];
      M::gz_hess(q, wu, zb, o);
      for (int d = 0; d < Z; ++d) gu[d] += o[d];
    }
    if constexpr (M::VS)  // variable observation noise: the sigma-dependent entries of J (see var_sigma_grad_terms)
      gu[Z] = var_sigma_grad_terms<RM>(sy, bd, q, w.gWu + cb * RM * U, U, w.gMb + cb * RM * RM,
                                       pick(sl.grad, s_) + (size_t)c * sy.Q);
    for (int d = 0; d < U; ++d) w.gup[cb * U + d] = gu[d];
  }
}



// ---------------------------------------------------------------------------------------------------------------
// Grad-log-det for FEW LONG blocks (the SIR single-block layout), every observation interval on its own wavefront.  With
// the row-free forms (k_gld_fwd_qx, k_gld_bwd_lean) a step only sees per-interval X x X / X x Z matrices, and what crosses
// an interval boundary is small and follows from the state sweep's interval sums (work.ivl: Ss, Ws, Pt):
//   k_gld_ivl_prologue  wave per (chain, block): the row tangents at the interval boundaries (as k_gld_fwd_qx's prologue),
//                       C1 = LF^T MLF, C2 = LF^T zd, Q0 = LF^T xd(t_m) of every interval -> work.gcq, terminal tangents -> gxdt
//   k_gld_fwd_ivl       wave per (chain, block, interval): the pseudo-row sweep of that interval from Q0 -> Qx
//   k_gld_bwd_ivl_a     wave per (chain, block, interval): the backward sweep of the interval with NO incoming x-bar (its own
//                       observation's Hessian term included): gradient entries, z-bar sum and the x-bar it hands on -> work.gbw
//   k_gld_bwd_ivl_b     wave per (chain, block, interval): x-bar arriving at the interval's end = the later intervals' hand-ons
//                       carried through their transition products (x-bar is an affine recursion); its contribution to the
//                       interval's gradient entries and z-bar needs the step Jacobians and prefix products only (no Hessian)
//   KGldIvlFinish       per (chain, block): sums, v_0 columns, dc/dz terms, work.gup (the tail of k_gld_bwd_lean)
#define CHMC_GCQ_N(X, Z) (2 * (X) * (X) + (X) * (Z))  // per interval: C1 | C2 | Q0
#define CHMC_GBW_N(X, Z) ((X) + 2 * (Z))               // per interval: x-bar handed on | z-bar (phase a) | z-bar (phase b)
// (body: block `wid` of the work order by the calling wavefront; `wv_`: its slice of the LDS scratch, < 4)
template <class M, int RM>
__device__ __forceinline__ void gld_ivl_prologue_body(const Sys& sy, const Slots& sl, const Work& w, int which, int wid, int wv_) {
  constexpr int X = M::X, Z = M::Z, V0 = M::V0;
  constexpr int NI = CHMC_IVL_N(X, Z), NC = CHMC_GCQ_N(X, Z);
  __shared__ double sm[4][RM * RM + RM * Z + 2 * RM * X + NI];
  const int lane = threadIdx.x & 63;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int NV = sy.NV;
  const double* Jv = pick(sl.Jv, s_) + (size_t)c * RM * NV;
  const double* LFr = pick(sl.LF, s_) + cb * sy.NOBS * RM * X;
  double* Mb = sm[wv_];
  double* zd = Mb + RM * RM;
  double* MLFs = zd + RM * Z;
  double* xds = MLFs + RM * X;
  double* Iv = xds + RM * X;
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  for (int i = lane; i < RM * RM; i += 64) Mb[i] = w.gMb[cb * RM * RM + i];
  for (int i = lane; i < RM * Z; i += 64) zd[i] = w.gzd[cb * RM * Z + i];
  lds_sync();
  if (lane < RM * X) {
    const int i = lane / X, a = lane - i * X;
    double t = 0.0;
    if (bd.first) {
      double dz[X * Z], dv0[X * V0];
      M::gx0_jac(dz, dv0);
      for (int mz = 0; mz < Z; ++mz) {
        double dzs = 0.0;
#pragma unroll
        for (int e2 = 0; e2 < X * Z; ++e2) dzs = e2 == a * Z + mz ? dz[e2] : dzs;
        t += dzs * zd[i * Z + mz];
      }
      for (int d = 0; d < V0; ++d) {
        double wv = 0.0, dvs = 0.0;
        for (int jj = 0; jj < RM; ++jj) wv += Mb[i * RM + jj] * Jv[(size_t)jj * NV + d];
#pragma unroll
        for (int e2 = 0; e2 < X * V0; ++e2) dvs = e2 == a * V0 + d ? dv0[e2] : dvs;
        t += dvs * wv;
      }
    }
    xds[lane] = t;
  }
  for (int j = 0; j < bd.nobs; ++j) {
    lds_sync();
    if (lane < RM * X) {
      const int i = lane / X, a = lane - i * X;
      double t = 0.0;
      for (int jj = 0; jj < RM; ++jj) t += Mb[i * RM + jj] * LFr[((size_t)j * RM + jj) * X + a];
      MLFs[lane] = t;
    }
    for (int e2 = lane; e2 < NI; e2 += 64) Iv[e2] = w.ivl[(cb * sy.NOBS + j) * NI + e2];
    lds_sync();
    double* Cj = w.gcq + (cb * sy.NOBS + j) * NC;
    if (lane < X * X) {
      const int a1 = lane / X, a2 = lane - a1 * X;
      double c1 = 0.0, q0 = 0.0;
      for (int i = 0; i < RM; ++i) {
        const double lf = LFr[((size_t)j * RM + i) * X + a1];
        c1 += lf * MLFs[i * X + a2];
        q0 += lf * xds[i * X + a2];
      }
      Cj[lane] = c1;
      Cj[X * X + X * Z + lane] = q0;
    }
    if (lane < X * Z) {
      const int a1 = lane / Z, mz = lane - a1 * Z;
      double c2 = 0.0;
      for (int i = 0; i < RM; ++i) c2 += LFr[((size_t)j * RM + i) * X + a1] * zd[i * Z + mz];
      Cj[X * X + lane] = c2;
    }
    double nx = 0.0;
    if (lane < RM * X) {
      const int i = lane / X, a = lane - i * X;
#pragma unroll
      for (int d = 0; d < X; ++d) nx += Iv[X * X + X * Z + a * X + d] * xds[i * X + d] + Iv[a * X + d] * MLFs[i * X + d];
      for (int mz = 0; mz < Z; ++mz) nx += Iv[X * X + a * Z + mz] * zd[i * Z + mz];
    }
    lds_sync();
    if (lane < RM * X) xds[lane] = nx;
    {
      const double tv = __shfl(nx, (j * X + lane) & 63, 64);
      if (j < bd.ny && lane < X) w.gxdt[(cb * RM + j) * X + lane] = tv;
    }
  }
}
template <class M, int RM>
__global__ void __launch_bounds__(256) k_gld_ivl_prologue(Sys sy, Slots sl, Work w, int which) {
  const int wv_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  gld_ivl_prologue_body<M, RM>(sy, sl, w, which, blockIdx.x * (blockDim.x >> 6) + wv_, wv_);
}


// (wid -> (chain, block, interval); false when the wavefront has nothing to do)
__device__ inline bool gld_ivl_ids(const Sys& sy, const Work& w, int wid, int& c, int& b, int& j) {
  if (wid >= sy.B * sy.K * sy.NOBS) return false;
  j = wid % sy.NOBS;
  const int cbi = sy.order[wid / sy.NOBS];
  c = cbi / sy.K, b = cbi - c * sy.K;
  return w.ok[c] != 0 && j < sy.blk[b].nobs;
}

// (UNTRACKED: the Qx stores are issued outside the compiler's vmcnt model, st_async.  The per-chain kernels pass false: they
// contain generic-address (flat) accesses to LDS, beside which untracked stores are not allowed -- tools/check_scan_isa.py.)
template <class M, int RM, bool UNTRACKED = true>
__device__ __forceinline__ void gld_fwd_ivl_body(const Sys& sy, const Slots& sl, const Work& w, int which, int wid) {
  constexpr int X = M::X, V = M::V, Z = M::Z;
  constexpr int NC = CHMC_GCQ_N(X, Z);
  const int lane = threadIdx.x & 63;
  int c, b, j;
  if (!gld_ivl_ids(sy, w, wid, c, b, j)) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S;
  const size_t TS = (size_t)sy.T * S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, s_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  double* Xd = w.Xd + (size_t)c * RM * X * TS + bd.step0;
  const double* PBr = pick(sl.PB, s_) + ((size_t)c * TS + bd.step0) * (X * V);
  const double* Cj = w.gcq + (cb * sy.NOBS + j) * NC;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double c1[X * X], c2[X * Z], xdc[X * X];
#pragma unroll
  for (int i = 0; i < X * X; ++i) c1[i] = Cj[i], xdc[i] = Cj[X * X + X * Z + i];
#pragma unroll
  for (int i = 0; i < X * Z; ++i) c2[i] = Cj[X * X + i];
  const int ntile = (S + 63) >> 6;
  for (int t = 0; t < ntile; ++t) {
    const int off = (t << 6) + lane;
    const bool valid = off < S;
    const int s = j * S + off;
    double P[X * X], e[X * X];
    {
      double A[X * X], Bm[X * V], Zf[X * Z], jp[X * V];
      if (valid) {
        double x[X], vv[V];
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
        M::jac(cc.k, x, vv, A, Bm, Zf);
#pragma unroll
        for (int k = 0; k < X * V; ++k) jp[k] = ld_stream(PBr + (size_t)s * (X * V) + k);
      } else {
#pragma unroll
        for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < X * V; ++i) Bm[i] = 0.0, jp[i] = 0.0;
#pragma unroll
        for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
      }
#pragma unroll
      for (int i = 0; i < X * X; ++i) P[i] = A[i];
#pragma unroll
      for (int r = 0; r < X; ++r) {
        double wv[V];
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt = 0.0;
#pragma unroll
          for (int a = 0; a < X; ++a) tt += c1[r * X + a] * jp[a * V + d];
          wv[d] = tt;
        }
#pragma unroll
        for (int a = 0; a < X; ++a) {
          double tt = 0.0;
#pragma unroll
          for (int d = 0; d < V; ++d) tt += Bm[a * V + d] * wv[d];
#pragma unroll
          for (int mz = 0; mz < Z; ++mz) tt += Zf[a * Z + mz] * c2[r * Z + mz];
          e[r * X + a] = tt;
        }
      }
    }
    dpp_affine_prefix<X, X>(P, e);
    {
      double xs[X * X], Pex[X * X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) xs[i] = dpp_mov<0x138, 0xf, 0xf>(e[i], 0.0);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pex[i] = dpp_mov<0x138, 0xf, 0xf>(P[i], (i / X == i % X) ? 1.0 : 0.0);
#pragma unroll
      for (int r = 0; r < X; ++r)
#pragma unroll
        for (int a = 0; a < X; ++a) {
          double tt = xs[r * X + a];
#pragma unroll
          for (int d = 0; d < X; ++d) tt += Pex[a * X + d] * xdc[r * X + d];
          xs[r * X + a] = tt;
        }
      if (valid) {
#pragma unroll
        for (int i = 0; i < X * X; ++i) {
          if constexpr (UNTRACKED) st_async(Xd + (size_t)i * TS + s, xs[i]);
          else Xd[(size_t)i * TS + s] = xs[i];
        }
      }
    }
    {
      double P6[X * X], nx[X * X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) P6[i] = bcast_lane63(P[i]);
#pragma unroll
      for (int r = 0; r < X; ++r)
#pragma unroll
        for (int a = 0; a < X; ++a) {
          double tt = bcast_lane63(e[r * X + a]);
#pragma unroll
          for (int d = 0; d < X; ++d) tt += P6[a * X + d] * xdc[r * X + d];
          nx[r * X + a] = tt;
        }
#pragma unroll
      for (int i = 0; i < X * X; ++i) xdc[i] = nx[i];
    }
  }
}
template <class M, int RM>
__global__ void __launch_bounds__(256) k_gld_fwd_ivl(Sys sy, Slots sl, Work w, int which) {
  gld_fwd_ivl_body<M, RM>(sy, sl, w, which, blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}


// PHASE 0: everything (Hessian contraction source, gradient entries without the incoming x-bar); PHASE 1: the incoming
// x-bar's contribution only
template <class M, int RM, int PHASE>
__device__ __forceinline__ void gld_bwd_ivl_body(const Sys& sy, const Slots& sl, const Work& w, int which, int wid) {
  constexpr int X = M::X, V = M::V, Z = M::Z, NXI = M::NXI;
  constexpr int NI = CHMC_IVL_N(X, Z), NC = CHMC_GCQ_N(X, Z), NB = CHMC_GBW_N(X, Z);
  const int lane = threadIdx.x & 63;
  int c, b, j;
  if (!gld_ivl_ids(sy, w, wid, c, b, j)) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S;
  const size_t TS = (size_t)sy.T * S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, s_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const size_t colb = (size_t)sy.V0 + (size_t)bd.step0 * V;
  const double* Xq = w.Xd + (size_t)c * RM * X * TS + bd.step0;  // Qx, component-major: [X X][T S]
  double* gv = pick(sl.grad, s_) + (size_t)c * sy.Q + sy.U;
  const double* PBr = pick(sl.PB, s_) + ((size_t)c * TS + bd.step0) * (X * V);
  const double* Cj = w.gcq + (cb * sy.NOBS + j) * NC;
  double* gb = w.gbw + (cb * sy.NOBS + j) * NB;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double xb[X], zbt[Z], Pf[X * X], Cm[X * X], Qz[X * Z];
#pragma unroll
  for (int i = 0; i < X; ++i) xb[i] = 0.0;
#pragma unroll
  for (int i = 0; i < Z; ++i) zbt[i] = 0.0;
#pragma unroll
  for (int i = 0; i < X * X; ++i) Cm[i] = Cj[i], Pf[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
  for (int i = 0; i < X * Z; ++i) Qz[i] = Cj[X * X + i];
  if (PHASE == 0) {
    if (j < bd.ny) {  // the Hessian term of the observation at the interval's end
      double hv[X], xt[X];
      for (int a = 0; a < X; ++a) xt[a] = w.gxdt[(cb * RM + j) * X + a];
      M::obs_hess_vec(traj + (size_t)(j + 1) * S * X, xt, hv);
#pragma unroll
      for (int a = 0; a < X; ++a) xb[a] = hv[a];
    }
  } else {
    // x-bar arriving at this interval's end: the later intervals' hand-ons through their transition products
    for (int m = bd.nobs - 1; m > j; --m) {
      const double* gm = w.gbw + (cb * sy.NOBS + m) * NB;
      const double* Pt = w.ivl + (cb * sy.NOBS + m) * NI + X * X + X * Z;
      double nb[X];
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = gm[d];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += xb[a] * Pt[a * X + d];
        nb[d] = tt;
      }
#pragma unroll
      for (int d = 0; d < X; ++d) xb[d] = nb[d];
    }
  }
  const int ntile = (S + 63) >> 6;
  for (int t = ntile - 1; t >= 0; --t) {
    const int off = (t << 6) + (63 - lane);  // LATER steps in LOWER lanes
    const bool valid = off < S;
    const int s = j * S + off;
    const size_t col = colb + (size_t)s * V;
    double A[X * X], Bm[X * V], Zf[X * Z], x[X], vv[V], pb[X * V], qx[X * X];
    if (valid) {
#pragma unroll
      for (int a = 0; a < X; ++a) x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
      for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
      if (PHASE == 0) {
#pragma unroll
        for (int k = 0; k < X * V; ++k) pb[k] = ld_stream(PBr + (size_t)s * (X * V) + k);
#pragma unroll
        for (int k = 0; k < X * X; ++k) qx[k] = ld_stream(Xq + (size_t)k * TS + s);
      }
      M::jac(cc.k, x, vv, A, Bm, Zf);
    } else {
#pragma unroll
      for (int a = 0; a < X; ++a) x[a] = 0.0;
#pragma unroll
      for (int a = 0; a < V; ++a) vv[a] = 0.0;
#pragma unroll
      for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
      for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
    }
    if (PHASE != 0 || !valid) {
#pragma unroll
      for (int k = 0; k < X * V; ++k) pb[k] = 0.0;
#pragma unroll
      for (int k = 0; k < X * X; ++k) qx[k] = 0.0;
    }
    double Inc[X * X], E[X * X], PE[X * X];
    dpp_prefix_products<X>(A, Inc, E);
    matmul_xx<X>(Pf, E, PE);
    double I0[X * X];
#pragma unroll
    for (int i = 0; i < X * X; ++i) I0[i] = bcast_lane63(Inc[i]);
    if (PHASE == 0) {
      double H[NXI];
      {
        double Q[X * NXI], Sm[X * NXI];
#pragma unroll
        for (int a1 = 0; a1 < X; ++a1) {
#pragma unroll
          for (int a2 = 0; a2 < X; ++a2) Q[a1 * NXI + a2] = qx[a1 * X + a2];
#pragma unroll
          for (int d = 0; d < V; ++d) {
            double tt = 0.0;
#pragma unroll
            for (int a2 = 0; a2 < X; ++a2) tt += Cm[a1 * X + a2] * pb[a2 * V + d];
            Q[a1 * NXI + X + d] = tt;
          }
#pragma unroll
          for (int mz = 0; mz < Z; ++mz) Q[a1 * NXI + X + V + mz] = Qz[a1 * Z + mz];
        }
#pragma unroll
        for (int a = 0; a < X; ++a)
#pragma unroll
          for (int m2 = 0; m2 < NXI; ++m2) {
            double tt = 0.0;
#pragma unroll
            for (int a1 = 0; a1 < X; ++a1) tt += PE[a1 * X + a] * Q[a1 * NXI + m2];
            Sm[a * NXI + m2] = tt;
          }
        M::hess(cc.k, x, vv, Sm, H);
        if (!valid) {
#pragma unroll
          for (int i = 0; i < NXI; ++i) H[i] = 0.0;
        }
      }
      double I2[X * X], gi[X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) I2[i] = A[i];
#pragma unroll
      for (int a = 0; a < X; ++a) gi[a] = H[a];
      dpp_rowaffine_prefix<X>(I2, gi);
      double xbs[X];
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = dpp_mov<0x138, 0xf, 0xf>(gi[d], 0.0);
#pragma unroll
        for (int a = 0; a < X; ++a) tt += xb[a] * E[a * X + d];
        xbs[d] = tt;
      }
      if (valid) {
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt = H[X + d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += Bm[a * V + d] * xbs[a];
          gv[col + d] = tt;
        }
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt = H[X + V + mz];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Zf[a * Z + mz] * xbs[a];
        zbt[mz] += tt;
      }
      double g0[X], nb[X];
#pragma unroll
      for (int a = 0; a < X; ++a) g0[a] = bcast_lane63(gi[a]);
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = g0[d];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += xb[a] * I0[a * X + d];
        nb[d] = tt;
      }
#pragma unroll
      for (int d = 0; d < X; ++d) xb[d] = nb[d];
      double Pn[X * X];
      matmul_xx<X>(Pf, I0, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pf[i] = Pn[i];
    } else {
      // the incoming x-bar at the state after this lane's step: xb (at the interval's end) through the later steps
      double xc[X];
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt += xb[a] * PE[a * X + d];
        xc[d] = tt;
      }
      if (valid) {
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt = 0.0;
#pragma unroll
          for (int a = 0; a < X; ++a) tt += Bm[a * V + d] * xc[a];
          gv[col + d] += tt;
        }
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Zf[a * Z + mz] * xc[a];
        zbt[mz] += tt;
      }
      double Pn[X * X];
      matmul_xx<X>(Pf, I0, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pf[i] = Pn[i];
    }
  }
#pragma unroll
  for (int i = 0; i < Z; ++i) {
    double v = zbt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    zbt[i] = v;
  }
  if (lane == 0) {
    if (PHASE == 0) {
#pragma unroll
      for (int a = 0; a < X; ++a) gb[a] = xb[a];
    }
#pragma unroll
    for (int i = 0; i < Z; ++i) gb[X + PHASE * Z + i] = zbt[i];
  }
}
template <class M, int RM, int PHASE>
__global__ void __launch_bounds__(256) k_gld_bwd_ivl(Sys sy, Slots sl, Work w, int which) {
  gld_bwd_ivl_body<M, RM, PHASE>(sy, sl, w, which, blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}


template <class M, int RM>
__device__ __forceinline__ void gld_ivl_finish_body(const Sys& sy, const Slots& sl, const Work& w, int which, int tid) {
  constexpr int X = M::X, Z = M::Z, U = M::U, V0 = M::V0;
  constexpr int NI = CHMC_IVL_N(X, Z), NB = CHMC_GBW_N(X, Z);
  if (tid >= sy.B * sy.K) return;
  const int c = tid / sy.K, b = tid - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  double* gv = pick(sl.grad, s_) + (size_t)c * sy.Q + sy.U;
  double xb[X], zbt[Z];
  for (int a = 0; a < X; ++a) xb[a] = 0.0;
  for (int i = 0; i < Z; ++i) zbt[i] = 0.0;
  for (int m = bd.nobs - 1; m >= 0; --m) {  // x-bar at the block's start; z-bar sums of both phases
    const double* gm = w.gbw + (cb * sy.NOBS + m) * NB;
    const double* Pt = w.ivl + (cb * sy.NOBS + m) * NI + X * X + X * Z;
    double nb[X];
    for (int d = 0; d < X; ++d) {
      double tt = gm[d];
      for (int a = 0; a < X; ++a) tt += xb[a] * Pt[a * X + d];
      nb[d] = tt;
    }
    for (int d = 0; d < X; ++d) xb[d] = nb[d];
    for (int i = 0; i < Z; ++i) zbt[i] += gm[X + i] + gm[X + Z + i];
  }
  if (bd.first) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    for (int d = 0; d < V0; ++d) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dv0[a * V0 + d] * xb[a];
      gv[d] = tt;
    }
    for (int mz = 0; mz < Z; ++mz) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dz[a * Z + mz] * xb[a];
      zbt[mz] += tt;
    }
  }
  double Gz[Z * Z], gu[U];
  M::gz_jac(q, Gz);
  for (int d = 0; d < Z; ++d) {
    double tt = 0.0;
    for (int mz = 0; mz < Z; ++mz) tt += Gz[mz * Z + d] * zbt[mz];
    gu[d] = tt;
  }
  for (int i = 0; i < RM; ++i) {
    double o[Z], wu[U], zb[Z];
    for (int d = 0; d < U; ++d) wu[d] = w.gWu[(cb * RM + i) * U + d];
    for (int mz = 0; mz < Z; ++mz) zb[mz] = w.zbP[(cb * RM + i) * Z + mz];
    M::gz_hess(q, wu, zb, o);
    for (int d = 0; d < Z; ++d) gu[d] += o[d];
  }
  if constexpr (M::VS)  // variable observation noise: the sigma-dependent entries of J (see var_sigma_grad_terms)
    gu[Z] = var_sigma_grad_terms<RM>(sy, bd, q, w.gWu + cb * RM * U, U, w.gMb + cb * RM * RM,
                                     pick(sl.grad, s_) + (size_t)c * sy.Q);
  for (int d = 0; d < U; ++d) w.gup[cb * U + d] = gu[d];
}
template <class M, int RM>
__global__ void __launch_bounds__(64) k_gld_ivl_finish(Sys sy, Slots sl, Work w, int which) {
  gld_ivl_finish_body<M, RM>(sy, sl, w, which, blockIdx.x * 64 + threadIdx.x);
}


// The same backward sweep for 16-row blocks.  With 16 rows the row loops of k_gld_bwd_wave cannot be unrolled (register
// file) and, rolled, they index per-lane arrays at run time, which puts those arrays into scratch memory (4.0 ms per
// launch on the SIR single-block layout).  Here the row loop stays rolled but everything it indexes by the row lives in
// LDS (the carried adjoint rows, which are wave-uniform, next to (G^-1)_bb and zd) or in global memory; the stored rows of
// the lane's step are loaded with static indices and stay in registers.
template <class M, int RM>
__global__ void __launch_bounds__(256) k_gld_bwd_wave_ldsrows(Sys sy, Slots sl, Work w, int which) {
  constexpr int X = M::X, V = M::V, Z = M::Z, U = M::U, V0 = M::V0, NXI = M::NXI;
  __shared__ double sm[4][RM * RM + RM * Z + RM * X];
  const int lane = threadIdx.x & 63;
  const int wv_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wid = blockIdx.x * (blockDim.x >> 6) + wv_;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];  // work order: longest blocks first
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  if (!w.ok[c]) return;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int S = sy.S, NV = sy.NV;
  const size_t TS = (size_t)sy.T * S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* traj = pick(sl.traj, s_) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  const double* Jv = pick(sl.Jv, s_) + (size_t)c * RM * NV;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const size_t colb = (size_t)sy.V0 + (size_t)bd.step0 * V;
  const double* Xd = w.Xd + (size_t)c * RM * X * TS + bd.step0;
  double* gv = pick(sl.grad, s_) + (size_t)c * sy.Q + sy.U;
  double* Mb = sm[wv_];
  double* zd = sm[wv_] + RM * RM;
  double* Lam = sm[wv_] + RM * RM + RM * Z;  // the carried adjoint rows (wave-uniform): indexed by the row at run time
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  for (int i = lane; i < RM * RM; i += 64) Mb[i] = w.gMb[cb * RM * RM + i];
  for (int i = lane; i < RM * Z; i += 64) zd[i] = w.gzd[cb * RM * Z + i];
  for (int i = lane; i < RM * X; i += 64) Lam[i] = 0.0;
  lds_sync();
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double xb[X], zbt[Z];
#pragma unroll
  for (int i = 0; i < X; ++i) xb[i] = 0.0;
#pragma unroll
  for (int i = 0; i < Z; ++i) zbt[i] = 0.0;
  const int ntile = (S + 63) >> 6;
  for (int j = bd.nobs - 1; j >= 0; --j) {
    if (j < bd.ny) {
      double g[X], hv[X], xt[X];
      for (int a = 0; a < X; ++a) xt[a] = w.gxdt[(cb * RM + j) * X + a];
      M::obs_grad(traj + (size_t)(j + 1) * S * X, g);
      M::obs_hess_vec(traj + (size_t)(j + 1) * S * X, xt, hv);
      {
        double gl = 0.0;
#pragma unroll
        for (int a = 0; a < X; ++a) gl = lane == a ? g[a] : gl;
        if (lane < X) Lam[j * X + lane] = gl;
      }
#pragma unroll
      for (int a = 0; a < X; ++a) xb[a] += hv[a];
    }
    if (j == bd.nobs - 1 && !bd.last) {
      if (lane < X) Lam[(bd.ny + lane) * X + lane] = 1.0;
    }
    lds_sync();
    for (int t = ntile - 1; t >= 0; --t) {
      const int off = (t << 6) + (63 - lane);  // LATER steps in LOWER lanes: the suffix scans become DPP prefix scans
      const bool valid = off < S;
      const int s = j * S + off;
      const size_t col = colb + (size_t)s * V;
      double A[X * X], Bm[X * V], Zf[X * Z], x[X], vv[V];
      if (valid) {
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = ld_stream(traj + (size_t)s * X + a);
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
        M::jac(cc.k, x, vv, A, Bm, Zf);
      } else {
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = 0.0;
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = 0.0;
#pragma unroll
        for (int i = 0; i < X * X; ++i) A[i] = (i / X == i % X) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < X * V; ++i) Bm[i] = 0.0;
#pragma unroll
        for (int i = 0; i < X * Z; ++i) Zf[i] = 0.0;
      }
      // products of the transition matrices of the later steps (adjoint rows): exclusive prefix products over the lanes
      double Inc[X * X], E[X * X];
      dpp_prefix_products<X>(A, Inc, E);
      // Hessian contraction source of this step
      double H[NXI];
      {
        double Sm[X * NXI];
#pragma unroll
        for (int i = 0; i < X * NXI; ++i) Sm[i] = 0.0;
        double jp[RM * V];  // stored rows at this lane's step: static indices (registers)
#pragma unroll
        for (int i = 0; i < RM; ++i) {
          const bool act = valid && i >= j && i < bd.nrows;
#pragma unroll
          for (int d = 0; d < V; ++d) jp[i * V + d] = act ? Jv[(size_t)i * NV + col + d] : 0.0;
        }
#pragma unroll 1
        for (int i = 0; i < RM; ++i) {  // rolled: everything indexed by i lives in LDS or global memory
          double Ls[X], dir[NXI];
#pragma unroll
          for (int d = 0; d < X; ++d) {
            double tt = 0.0;
#pragma unroll
            for (int a = 0; a < X; ++a) tt += Lam[i * X + a] * E[a * X + d];
            Ls[d] = tt;
          }
#pragma unroll
          for (int a = 0; a < X; ++a) dir[a] = (valid && i >= j && i < bd.nrows) ? Xd[(size_t)(i * X + a) * TS + s] : 0.0;
#pragma unroll
          for (int d = 0; d < V; ++d) {
            double tt = 0.0;
#pragma unroll
            for (int jj = 0; jj < RM; ++jj) tt += Mb[i * RM + jj] * jp[jj * V + d];
            dir[X + d] = tt;
          }
#pragma unroll
          for (int mz = 0; mz < Z; ++mz) dir[X + V + mz] = zd[i * Z + mz];
#pragma unroll
          for (int a = 0; a < X; ++a)
#pragma unroll
            for (int m2 = 0; m2 < NXI; ++m2) Sm[a * NXI + m2] += Ls[a] * dir[m2];
        }
        M::hess(cc.k, x, vv, Sm, H);
        if (!valid) {
#pragma unroll
          for (int i = 0; i < NXI; ++i) H[i] = 0.0;
        }
      }
      // joint suffix scan for x-bar: x-bar^(l) = x-bar^(l+1) A_l + Hx_l
      double I2[X * X], gi[X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) I2[i] = A[i];
#pragma unroll
      for (int a = 0; a < X; ++a) gi[a] = H[a];
      dpp_rowaffine_prefix<X>(I2, gi);
      double xbs[X];  // x-bar at the state after this lane's step
#pragma unroll
      for (int d = 0; d < X; ++d) {
        double tt = dpp_mov<0x138, 0xf, 0xf>(gi[d], 0.0);  // wave_shr:1: the sources of the later steps
#pragma unroll
        for (int a = 0; a < X; ++a) tt += xb[a] * E[a * X + d];
        xbs[d] = tt;
      }
      if (valid) {
#pragma unroll
        for (int d = 0; d < V; ++d) {
          double tt = H[X + d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += Bm[a * V + d] * xbs[a];
          gv[col + d] = tt;
        }
      }
#pragma unroll
      for (int mz = 0; mz < Z; ++mz) {
        double tt = H[X + V + mz];
#pragma unroll
        for (int a = 0; a < X; ++a) tt += Zf[a * Z + mz] * xbs[a];
        zbt[mz] += tt;
      }
      // carries
      double I0[X * X], g0[X];
#pragma unroll
      for (int i = 0; i < X * X; ++i) I0[i] = bcast_lane63(I2[i]);
#pragma unroll
      for (int a = 0; a < X; ++a) g0[a] = bcast_lane63(gi[a]);
      {
        double nb[X];
#pragma unroll
        for (int d = 0; d < X; ++d) {
          double tt = g0[d];
#pragma unroll
          for (int a = 0; a < X; ++a) tt += xb[a] * I0[a * X + d];
          nb[d] = tt;
        }
#pragma unroll
        for (int d = 0; d < X; ++d) xb[d] = nb[d];
      }
      {  // Lam <- Lam I0: entry e = (row, component) by lane e
        double nl = 0.0;
        const int e = lane < RM * X ? lane : 0, ei = e / X, ed = e - ei * X;
#pragma unroll
        for (int a = 0; a < X; ++a) {
          double i0 = 0.0;
#pragma unroll
          for (int d = 0; d < X; ++d) i0 = d == ed ? I0[a * X + d] : i0;
          nl += Lam[ei * X + a] * i0;
        }
        lds_sync();
        if (lane < RM * X) Lam[e] = nl;
        lds_sync();
      }
    }
  }
  if (bd.first && lane == 0) {
    double dz[X * Z], dv0[X * V0];
    M::gx0_jac(dz, dv0);
    for (int d = 0; d < V0; ++d) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dv0[a * V0 + d] * xb[a];
      gv[d] = tt;
    }
    for (int mz = 0; mz < Z; ++mz) {
      double tt = 0.0;
      for (int a = 0; a < X; ++a) tt += dz[a * Z + mz] * xb[a];
      zbt[mz] += tt;
    }
  }
#pragma unroll
  for (int i = 0; i < Z; ++i) {
    double v = zbt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    zbt[i] = v;
  }
  if (lane == 0) {
    double Gz[Z * Z], gu[U];
    M::gz_jac(q, Gz);
    for (int d = 0; d < Z; ++d) {
      double tt = 0.0;
      for (int mz = 0; mz < Z; ++mz) tt += Gz[mz * Z + d] * zbt[mz];
      gu[d] = tt;
    }
    for (int i = 0; i < RM; ++i) {
      double o[Z], wu[U], zb[Z];
      for (int d = 0; d < U; ++d) wu[d] = w.gWu[(cb * RM + i) * U + d];
      for (int mz = 0; mz < Z; ++mz) zb[mz] = w.zbP[(cb * RM + i) * Z + mz];
      M::gz_hess(q, wu, zb, o);
      for (int d = 0; d < Z; ++d) gu[d] += o[d];
    }
    if constexpr (M::VS)  // variable observation noise: the sigma-dependent entries of J (see var_sigma_grad_terms)
      gu[Z] = var_sigma_grad_terms<RM>(sy, bd, q, w.gWu + cb * RM * U, U, w.gMb + cb * RM * RM,
                                       pick(sl.grad, s_) + (size_t)c * sy.Q);
    for (int d = 0; d < U; ++d) w.gup[cb * U + d] = gu[d];
  }
}

// Chain part of the Woodbury solves (KSolveChain in chmc_core.h) with the blocks of a chain spread over the lanes
// of one wavefront: lane b owns block b (K <= 64), the U x U core matrix and right-hand side are summed over the
// lanes with shuffles, every lane solves the tiny core system redundantly, forms its block's multipliers and its
// share of the u-columns of J^T lambda, which is reduced again.  Same template parameters as KSolveChain.
template <class M, int RM, int SYM, int TGT>
__device__ __forceinline__ void solve_chain_body(const Sys& sy, const Slots& sl, const Work& w, int which, int qsel, int psel, int c) {
  constexpr int U = M::U;
  const int lane = threadIdx.x & 63;
  if (c >= sy.B) return;
  if (TGT == 0 ? !newton_select(w, c, which, qsel) : !w.ok[c]) return;
  const int s = sl.cur[c] ^ which;
  const bool has = lane < sy.K;
  const size_t cb = (size_t)c * sy.Kmax + (has ? lane : 0);
  double sacc[U], Cm[U * U];
#pragma unroll
  for (int a = 0; a < U; ++a) sacc[a] = has ? w.sb[cb * U + a] : 0.0;
  if (!SYM) {
#pragma unroll
    for (int i = 0; i < U * U; ++i) Cm[i] = has ? w.Cb[cb * U * U + i] : 0.0;
  }
#pragma unroll
  for (int a = 0; a < U; ++a) {
    double v = sacc[a];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    sacc[a] = v;
  }
  if (SYM) {
    double Lc[U * U];
#pragma unroll
    for (int i = 0; i < U * U; ++i) Lc[i] = pick(sl.facC, s)[(size_t)c * U * U + i];
    cho_solve<U, 1>(Lc, sacc);
  } else {
#pragma unroll
    for (int i = 0; i < U * U; ++i) {
      double v = Cm[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      Cm[i] = v + (sy.m0 ? metric_of(sy, c)[i] : ((i / U == i % U) ? 1.0 : 0.0));  // + M_0 (:794-798)
    }
    int piv[U];
    lu_factor<U>(Cm, piv);
    lu_solve<U, 1>(Cm, piv, sacc);
  }
  double du[U];
#pragma unroll
  for (int a = 0; a < U; ++a) du[a] = 0.0;
  unsigned long long eb = 0ULL;
  if (has) {
    const double* E = (SYM ? pick(sl.E, s) : w.Ew) + cb * RM * U;
    const double* ju = pick(sl.JuP, s) + cb * RM * U;
#pragma unroll
    for (int i = 0; i < RM; ++i) {
      double l = w.tpad[cb * RM + i];
#pragma unroll
      for (int a = 0; a < U; ++a) l -= E[i * U + a] * sacc[a];
      w.lampad[cb * RM + i] = l;
#pragma unroll
      for (int a = 0; a < U; ++a) du[a] += ju[i * U + a] * l;
      if (TGT == 0) {
        const unsigned long long vb = absbits(w.cpad[cb * RM + i]);
        eb = vb > eb ? vb : eb;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < U; ++a) {
    double v = du[a];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    du[a] = v;
  }
  if (TGT == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long v = __shfl_xor(eb, o, 64);
      eb = v > eb ? v : eb;
    }
  }
  if (lane == 0) {
    if (TGT == 0) {
      double* q = (qsel ? w.qb : pick(sl.q, s ^ 1)) + (size_t)c * sy.Q;
      unsigned long long nb = 0ULL;
#pragma unroll
      for (int a = 0; a < U; ++a) {
        const double dq = metric_inv_u(sy, c, du, a);  // delta_q = metric.inv @ delta_mu (:1033-1041, :1105-1113)
        q[a] -= dq;
        const unsigned long long vb = absbits(dq);
        nb = vb > nb ? vb : nb;
      }
      w.err[c] = bitsd(eb);
      w.ndq[c] = nb;
    } else if (TGT == 1) {
      double* p = (psel == 0 ? pick(sl.p, s) : psel == 1 ? w.pb : psel == 3 ? pick(sl.pg, s) : pick(sl.p, s ^ 1)) + (size_t)c * sy.Q;
#pragma unroll
      for (int a = 0; a < U; ++a) p[a] -= du[a];
    }
  }
}
template <class M, int RM, int SYM, int TGT>
__global__ void __launch_bounds__(256) k_solve_chain_wave(Sys sy, Slots sl, Work w, int which, int qsel, int psel) {
  solve_chain_body<M, RM, SYM, TGT>(sy, sl, w, which, qsel, psel,
                                    blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}


// ---------------------------------------------------------------------------------------------------------------
// KGldPrep for 16-row blocks with the block over 16 lanes (four blocks per wavefront): lane r solves for column r of
// D_b^-1 against the Cholesky factor parked in LDS (the per-column recurrences of cho_solve, same operation order), forms
// row r of W_u = E C^-1 and column r of (G^-1)_bb = D_b^-1 - W_u E^T.  The one-lane functor keeps three 16 x 16 matrices in
// scratch memory: 206-247 us per launch on the SIR single-block layout.
// (body: the blocks tid0 .. tid0 + ntids - 1, ntids <= 4, on the 16-lane groups of the calling wavefront)
template <class M, int RM>
__device__ __forceinline__ void gld_prep_body(const Sys& sy, const Slots& sl, const Work& w, int which, int tid0, int ntids) {
  static_assert(RM == 16, "rows over 16 lanes");
  constexpr int Z = M::Z, U = M::U;
  __shared__ double Ls[4][RM * RM], Es[4][RM * U], Ws[4][RM * U];
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int tid = tid0 + g;
  const bool live = g < ntids && tid < sy.B * sy.K;
  const int tc = live ? tid : 0;
  const int c = tc / sy.K, b = tc - c * sy.K;
  const bool act = live && w.ok[c] != 0;
  const int s = sl.cur[c] ^ which;
  const size_t cb = (size_t)c * sy.Kmax + b;
  const int nrows = sy.blk[b].nrows;
  double* L = Ls[g];
  double e[U], wu[U];
  {
    const double* fd = pick(sl.facD, s) + cb * RM * RM + r * RM;
#pragma unroll
    for (int k = 0; k < RM; ++k) L[r * RM + k] = act ? fd[k] : (k == r ? 1.0 : 0.0);
    const double* E = pick(sl.E, s) + cb * RM * U + r * U;
    const double* Ci = pick(sl.Cinv, s) + (size_t)c * U * U;
#pragma unroll
    for (int a = 0; a < U; ++a) e[a] = act ? E[a] : 0.0;
#pragma unroll
    for (int d = 0; d < U; ++d) {
      double t = 0.0;
#pragma unroll
      for (int a = 0; a < U; ++a) t += e[a] * (act ? Ci[a * U + d] : 0.0);
      wu[d] = t;
      Ws[g][r * U + d] = t;
      Es[g][r * U + d] = e[d];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  // column r of D^-1 = (L L^T)^-1: forward then backward substitution with right-hand side e_r
  double x[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    double t = i == r ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < RM; ++k)
      if (k < i) t -= L[i * RM + k] * x[k];
    x[i] = t / L[i * RM + i];
  }
#pragma unroll
  for (int i = RM - 1; i >= 0; --i) {
    double t = x[i];
#pragma unroll
    for (int k = 0; k < RM; ++k)
      if (k > i) t -= L[k * RM + i] * x[k];
    x[i] = t / L[i * RM + i];
  }
  if (!act) return;
  // (G^-1)_bb[i][r] = D^-1[i][r] - sum_a W_u[i][a] E[r][a]; padded rows and columns are zero
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    double t = 0.0;
#pragma unroll
    for (int a = 0; a < U; ++a) t += Ws[g][i * U + a] * e[a];
    const double v = (i >= nrows || r >= nrows) ? 0.0 : x[i] - t;
    w.gMb[cb * RM * RM + i * RM + r] = v;
  }
  double Gz[Z * Z];
  M::gz_jac(pick(sl.q, s) + (size_t)c * sy.Q, Gz);
#pragma unroll
  for (int d = 0; d < U; ++d) w.gWu[(cb * RM + r) * U + d] = wu[d];
#pragma unroll
  for (int mz = 0; mz < Z; ++mz) {
    double t = 0.0;
#pragma unroll
    for (int d = 0; d < Z; ++d) t += Gz[mz * Z + d] * wu[d];
    w.gzd[(cb * RM + r) * Z + mz] = t;
  }
}
template <class M, int RM>
__global__ void __launch_bounds__(64) k_gld_prep_wave(Sys sy, Slots sl, Work w, int which) {
  gld_prep_body<M, RM>(sy, sl, w, which, blockIdx.x * 4, 4);
}


// ---------------------------------------------------------------------------------------------------------------
// Newton iteration, everything between the Gram blocks and the J^T lambda column pass in ONE launch (blocks of at most 8
// rows, at most 64 blocks per chain, compact rows): lane b of the chain's wavefront factors block b (KNewtonFactor: LU of
// D_b, D_b^-1 c_b, D_b^-1 dc/du_b, C_b, s_b, same operation order), the Woodbury core is summed over the lanes and solved
// redundantly by every lane, lane b forms its block's multipliers and its share of the u-columns, lane 0 applies them to
// the iterate (k_solve_chain_wave<.., 0, 0>), and lane b applies its multipliers to its interval frames (KMuF<RM, X, 0>).
// What the three kernels passed through HBM (tpad, Ew, Cb, sb) stays in registers; results are bitwise theirs.
// Three launches of 9-21 us each become one: sym_blk + solve_chain 0.45 -> see DESIGN.md.
// newton_fsm_body: chain c by the calling wavefront (a chain of the launch: newton_select holds); shared by k_newton_fsm_wave
// and its form for two problems.
template <class M, int RM>
__device__ __forceinline__ void newton_fsm_body(const Sys& sy, const Slots& sl, const Work& w, int prev, int qsel, int c) {
  constexpr int U = M::U, X = M::X;
  static_assert(RM <= 8, "one block per lane: the RM x RM matrix lives in registers");
  const int lane = threadIdx.x & 63;
  const int sp = sl.cur[c] ^ prev;
  const bool has = lane < sy.K;
  const size_t cb = (size_t)c * sy.Kmax + (has ? lane : 0);
  double D[RM * RM], JuL[RM * U], cp[RM];
  unsigned long long eb = 0ULL;
#pragma unroll
  for (int i = 0; i < RM * RM; ++i) D[i] = has ? w.Dw[cb * RM * RM + i] : ((i / RM == i % RM) ? 1.0 : 0.0);
#pragma unroll
  for (int i = 0; i < RM * U; ++i) JuL[i] = has ? w.JuL[cb * RM * U + i] : 0.0;
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    cp[i] = has ? w.cpad[cb * RM + i] : 0.0;
    const unsigned long long vb = absbits(cp[i]);  // |c|_inf of the iterate (before the solve overwrites cp)
    eb = vb > eb ? vb : eb;
  }
  {
    int piv[RM];
    lu_factor<RM>(D, piv);
    lu_solve<RM, 1>(D, piv, cp);
    lu_solve<RM, U>(D, piv, JuL);
  }
  const double* jur = pick(sl.JuP, sp) + cb * RM * U;
  double ju[RM * U];
#pragma unroll
  for (int i = 0; i < RM * U; ++i) ju[i] = has ? jur[i] : 0.0;
  double sacc[U], Cm[U * U];
#pragma unroll
  for (int a = 0; a < U; ++a) {
    double t2 = 0.0;
#pragma unroll
    for (int i = 0; i < RM; ++i) t2 += ju[i * U + a] * cp[i];
    sacc[a] = has ? t2 : 0.0;
#pragma unroll
    for (int d = 0; d < U; ++d) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < RM; ++i) t += ju[i * U + a] * JuL[i * U + d];
      Cm[a * U + d] = has ? t : 0.0;
    }
  }
#pragma unroll
  for (int a = 0; a < U; ++a) {
    double v = sacc[a];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    sacc[a] = v;
  }
#pragma unroll
  for (int i = 0; i < U * U; ++i) {
    double v = Cm[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    Cm[i] = v + (sy.m0 ? metric_of(sy, c)[i] : ((i / U == i % U) ? 1.0 : 0.0));  // + M_0 (:794-798)
  }
  {
    int piv[U];
    lu_factor<U>(Cm, piv);
    lu_solve<U, 1>(Cm, piv, sacc);
  }
  double lam[RM], du[U];
#pragma unroll
  for (int a = 0; a < U; ++a) du[a] = 0.0;
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    double l = cp[i];
#pragma unroll
    for (int a = 0; a < U; ++a) l -= JuL[i * U + a] * sacc[a];
    lam[i] = l;
    if (has) w.lampad[cb * RM + i] = l;
#pragma unroll
    for (int a = 0; a < U; ++a) du[a] += ju[i * U + a] * l;
  }
#pragma unroll
  for (int a = 0; a < U; ++a) {
    double v = has ? du[a] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    du[a] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = __shfl_xor(eb, o, 64);
    eb = v > eb ? v : eb;
  }
  if (lane == 0) {
    double* q = (qsel ? w.qb : pick(sl.q, sp ^ 1)) + (size_t)c * sy.Q;
    unsigned long long nb = 0ULL;
#pragma unroll
    for (int a = 0; a < U; ++a) {
      const double dq = metric_inv_u(sy, c, du, a);  // delta_q = metric.inv @ delta_mu (:1033-1041, :1105-1113)
      q[a] -= dq;
      const unsigned long long vb = absbits(dq);
      nb = vb > nb ? vb : nb;
    }
    w.err[c] = bitsd(eb);
    w.ndq[c] = nb;
  }
  if (has && w.muF) {  // mu_F[m] = sum_i lambda_i LF[m][i] of the previous point's interval frames
    const BlockDesc bd = sy.blk[lane];
    const double* lfb = pick(sl.LF, sp) + cb * sy.NOBS * RM * X;
    double* mo = w.muF + cb * sy.NOBS * X;
    // (four intervals at a time, their frames requested together and the results stored afterwards: interval by interval the
    // run-time loop pays a memory round trip each on the one wavefront of the chain, and this kernel is pure latency)
    for (int m0 = 0; m0 < sy.NOBS; m0 += 4) {
      double t4[4][X], lf[4][RM * X];
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // (the loads under wave-uniform conditions only: all of them issue before the first use)
        const bool in = m0 + k < sy.NOBS;
#pragma unroll
        for (int e = 0; e < RM * X; ++e) lf[k][e] = in ? lfb[(m0 + k) * RM * X + e] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int m = m0 + k;
#pragma unroll
        for (int a = 0; a < X; ++a) {
          double t = 0.0;
          if (m < bd.nobs) {
#pragma unroll
            for (int i = 0; i < RM; ++i)
              if (i < bd.nrows) t += lam[i] * lf[k][i * X + a];
          }
          t4[k][a] = t;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (m0 + k < sy.NOBS) {
#pragma unroll
          for (int a = 0; a < X; ++a) mo[(m0 + k) * X + a] = t4[k][a];
        }
    }
  }
}
template <class M, int RM>
__global__ void __launch_bounds__(64) k_newton_fsm_wave(Sys sy, Slots sl, Work w, int prev, int qsel) {
  const int c = blockIdx.x;
  if (c >= sy.B) return;
  if (!newton_select(w, c, prev, qsel)) return;
  newton_fsm_body<M, RM>(sy, sl, w, prev, qsel, c);
}
// ... for two problems in one grid (KernelPlan::pair_passes): the first B workgroups serve the chains of w0, the next B those
// of w1 -- one wavefront per chain and problem, pure latency, so both sets take about as long as one
template <class M, int RM>
__global__ void __launch_bounds__(64) k_newton_fsm_wave_pair(Sys sy, Slots sl, Work w0, int prev, int qsel, Work w1) {
  const bool second = (int)blockIdx.x >= sy.B;
  const int c = second ? (int)blockIdx.x - sy.B : (int)blockIdx.x;
  if (c >= sy.B) return;
  const Work w = second ? w1 : w0;
  if (!newton_select(w, c, prev, qsel)) return;
  newton_fsm_body<M, RM>(sy, sl, w, prev, qsel, c);
}

// ---------------------------------------------------------------------------------------------------------------
// KNewtonFactor for 16-row blocks with the ROWS of the block over 16 lanes (four blocks per wavefront) instead of one
// lane per block: a 16 x 16 matrix does not fit one lane's registers (the functor lives in scratch memory: 230 us per
// launch on the SIR single-block layout, 17 launches per leapfrog step).  LU with partial pivoting in LAPACK getrf
// order (:745-752) on the augmented rows [D | c | dc/du]: pivot search and row exchange by 16-lane shuffles, the
// elimination of a column is one FMA per lane and entry, the forward substitution rides along (same operation order as
// lu_solve), the back substitution runs column by column.  Then E = D^-1 dc/du, t = D^-1 c, C_b and s_b as KNewtonFactor.
// FUSE (one block per chain, K = 1: the chain's Woodbury system is this block's): the 16 lanes go on to solve the core
// system, form the multipliers, apply their u-columns to the iterate and apply them to the interval frames -- the work
// of k_solve_chain_wave<.., 0, 0> and KMuF<16, X, 0>, two launches of a latency-bound round less.
template <class M, int RM, bool FUSE = false>
__global__ void __launch_bounds__(64) k_newton_factor_wave(Sys sy, Slots sl, Work w, int prev, int qsel) {
  const int lane = threadIdx.x & 63;
  const int tid = blockIdx.x * 4 + (lane >> 4);
  const bool live = tid < sy.B * sy.K;
  const int tc = live ? tid : 0;
  const int c = tc / sy.K, b = tc - c * sy.K;
  const bool act = newton_select(w, c, prev, qsel) && live;
  const size_t cb = (size_t)c * sy.Kmax + b;
  newton_factor16<M, RM, FUSE>(sy, sl, w, prev, qsel, c, b, act, w.Dw + cb * RM * RM, w.JuL + cb * RM * M::U);
}

// ---------------------------------------------------------------------------------------------------------------
// Forward scan of `constr` (:473-519) for S % 8 == 0: lane l of a wavefront integrates block (chain, block) =
// tid of the launch, exactly like fwd_block_impl, but with the memory traffic arranged by hand.  The recursion is
// latency bound (one wavefront per SIMD issues ~14 dependent fp64 instructions per step, 2.7 ns each), so every
// cycle the wave spends on memory instructions or waiting for them is lost (tools/ubench/fwd_latency.hip):
//   * loads: each lane walks its own 128-byte lines of noise increments.  hipcc drains the whole vector-memory
//     queue (s_waitcnt vmcnt(0)) at the first use of a loaded tile, which exposes a full HBM round trip per tile;
//     here the loads are issued through inline asm into a ring of DEPTH tiles and waited for with a counted
//     s_waitcnt (loads retire in issue order, MI355X_MICROARCH.md), which hides them completely;
//   * stores: a lane-per-block store instruction writes 16 bytes to 64 different lines (~95 ns of issue per
//     instruction).  The integrating wave only parks its 8-step trajectory tile in LDS; a second, helper wavefront
//     of the workgroup reads the tile back transposed (8 lanes per 128-byte row) and issues the global stores, so
//     that stores cost the integrating wave nothing and never sit in its vmcnt queue.
// The two waves meet at one s_barrier per tile (the integrating wave signals tile t when it starts tile t+1); the
// tile buffers alternate.
typedef double d2_t __attribute__((ext_vector_type(2)));
template <int OFF>
__device__ __forceinline__ void vm_load16(d2_t& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(p), "n"(OFF) : "memory");
}
template <int I, int N, int OFF0>
struct TileLoad {
  static __device__ __forceinline__ void run(d2_t* r, const void* p) {
    vm_load16<OFF0 + 16 * I>(r[I], p);
    TileLoad<I + 1, N, OFF0>::run(r, p);
  }
};
template <int N, int OFF0>
struct TileLoad<N, N, OFF0> {
  static __device__ __forceinline__ void run(d2_t*, const void*) {}
};
// wait until at most NOUT vector-memory operations are outstanding; the tile's registers are tied to the wait so
// that no use of them can be scheduled above it
template <int NOUT>
__device__ __forceinline__ void vm_wait(d2_t (&r)[8]) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7])
               : "n"(NOUT)
               : "memory");
}
template <int NOUT>
__device__ __forceinline__ void vm_wait(d2_t (&r)[12]) {
  asm volatile("s_waitcnt vmcnt(%12)"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]),
                 "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11])
               : "n"(NOUT)
               : "memory");
}
// streaming store: the trajectory is written once and read back by other workgroups much later; without the
// non-temporal hint every new line is allocated in L2 and the per-CU write path (not HBM) paces the helper wave
// (tools/ubench/fwd_latency.hip: 70 -> 49 ns per step)
__device__ __forceinline__ void vm_store16_nt(double* p, const d2_t& v) {
  // (nt: measured again in round 4 with the alternating chain order -- plain stores would leave the trajectory in the caches
  // for the interval sums that read it next: those get 1 % faster, the scan 2 % slower, the step 0.3 % slower)
  asm volatile("global_store_dwordx4 %0, %1, off nt" : : "v"(p), "v"(v) : "memory");
}

// ---------------------------------------------------------------------------------------------------------------
// Multiple shooting over a whole chain by ONE wavefront (k_xobs_par, k_path_par): the chain's L steps are cut into 64 segments
// of m = ceil(L / 64) steps, lane l integrates segment l from its start state Ul, seeded with the state's stored trajectory,
// and accumulates the segment's transition matrix; the junction defects are corrected by an affine prefix scan over the
// lanes (the Newton step on the 63 matching conditions, as in fwd_par_sweeps).  The stored trajectory is exact inside every
// block of the CURRENT partition and its block junctions close to the constraint tolerance, so the junction corrections of
// the first sweep are ~1e-9 and the second sweep only confirms them.
// (Not fwd_par_sweeps: that one works per block on W wavefronts with the DPP scan, treats the absorbing fronts of SIR, and
// settles to CHMC_PAR_JTOL = 1e-11 before a final pass; only the settled predicate is common to the two.)

// A junction value has settled: the new one equals the old one (bitwise, or both NaN: beyond a point where the true recursion
// overflows everything is NaN and stays NaN) or differs from it by at most tol relative to max(|new|, 1).
__device__ __forceinline__ bool junction_settled(double nu, double old, double tol) {
  const bool same = nu == old || (nu != nu && old != old);
  const bool close = fabs(nu - old) <= tol * (fabs(nu) > 1.0 ? fabs(nu) : 1.0);
  return same || close;
}

// Lane `lane`'s segment [s0, s1) of the L steps (have: it is not empty) and its first start state Ul: x0 for lane 0, else
// the stored trajectory's state before step s0.  sy.blk / sy.obs2blk must still describe the partition the trajectory was
// computed in.
struct ShootSeg {
  int m, s0, s1;
  bool have;
};
template <class M>
__device__ __forceinline__ ShootSeg shoot_setup(const Sys& sy, int lane, int L, const double* trj, const double (&x0)[M::X],
                                                double (&Ul)[M::X]) {
  constexpr int X = M::X;
  ShootSeg sg;
  sg.m = (L + 63) >> 6;
  sg.s0 = lane * sg.m, sg.s1 = (sg.s0 + sg.m < L ? sg.s0 + sg.m : L);
  sg.have = sg.s0 < L;
  const int b0 = sg.have ? sy.obs2blk[sg.s0 / sy.S] : 0;  // step s of block b sits at trajectory entry s + CHMC_TPAD b
#pragma unroll
  for (int a = 0; a < X; ++a) Ul[a] = lane == 0 ? x0[a] : (sg.have ? trj[(size_t)(sg.s0 + CHMC_TPAD * b0) * X + a] : 0.0);
  return sg;
}

// The junction half of a sweep, after every lane has integrated its segment from Ul to x with the transition matrix P: the
// junction defects, their affine prefix scan over the lanes, the new start states (a lane whose start state did not move
// at all hands on its end state as it is: the exact prefix) and the settled criterion at 1e-13.  Ul becomes the new start
// state; returns whether every junction has settled (the same value in every lane).
// (The integration half stays in the two kernels: shared behind a per-step hook it compiled to the same fp64 instructions
// and still moved the last bit of some settled start states on long chains, profiles/shoot_shared_full_form_rejected.txt.)
template <int X>
__device__ __forceinline__ bool shoot_junctions(const double (&x)[X], const double (&P)[X * X], double (&Ul)[X], int lane,
                                                bool have, bool junction) {
  double ec[X], Pc[X * X], Unext[X];
#pragma unroll
  for (int a = 0; a < X; ++a) Unext[a] = __shfl_down(Ul[a], 1, 64);
#pragma unroll
  for (int a = 0; a < X; ++a) ec[a] = junction ? x[a] - Unext[a] : 0.0;
#pragma unroll
  for (int i = 0; i < X * X; ++i) Pc[i] = junction ? P[i] : ((i / X == i % X) ? 1.0 : 0.0);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    double Pp[X * X], ep[X], Pn[X * X];
#pragma unroll
    for (int i = 0; i < X * X; ++i) Pp[i] = __shfl_up(Pc[i], o, 64);
#pragma unroll
    for (int a = 0; a < X; ++a) ep[a] = __shfl_up(ec[a], o, 64);
    if (lane >= o) {
#pragma unroll
      for (int a = 0; a < X; ++a) {
        double tt = ec[a];
#pragma unroll
        for (int d = 0; d < X; ++d) tt += Pc[a * X + d] * ep[d];
        ec[a] = tt;
      }
      matmul_xx<X>(Pc, Pp, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) Pc[i] = Pn[i];
    }
  }
  double dl[X], Un[X];
#pragma unroll
  for (int a = 0; a < X; ++a) {
    const double up = __shfl_up(ec[a], 1, 64);
    dl[a] = lane == 0 ? 0.0 : up;
  }
  bool still = true;
#pragma unroll
  for (int a = 0; a < X; ++a) still = still && dl[a] == 0.0;
#pragma unroll
  for (int a = 0; a < X; ++a) {
    double tt = 0.0;
#pragma unroll
    for (int d = 0; d < X; ++d) tt += P[a * X + d] * dl[d];
    Un[a] = still ? x[a] : x[a] + tt;
  }
  int unsettled = 0;
#pragma unroll
  for (int a = 0; a < X; ++a) {
    const double nu = __shfl_up(Un[a], 1, 64);
    if (lane > 0 && have) {
      unsettled |= !junction_settled(nu, Ul[a], 1e-13);
      Ul[a] = nu;
    }
  }
  return __ballot(unsettled) == 0ULL;
}

// generate_x_obs_seq (:384-397) of every chain's CURRENT state by the multiple shooting above: the states at the observation
// times for the partition switch, stored by the sweeps themselves.  The sequential recursion, 40 000 dependent steps on one
// lane (KXobs: 2 ms per switch at configs[1]), is the fallback.
template <class M>
__global__ void __launch_bounds__(64) k_xobs_par(Sys sy, Slots sl, double* xobs_out) {
  constexpr int X = M::X, V = M::V, MAXS = 8;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x;
  if (c >= sy.B) return;
  const int s_ = sl.cur[c];
  const int S = sy.S, L = sy.T * sy.S;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* vbase = q + sy.U + sy.V0;
  double* out = xobs_out + (size_t)c * sy.T * X;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double x0[X], Ul[X];
  M::gx0(cc.z, q + sy.U, x0);
  const ShootSeg sg = shoot_setup<M>(sy, lane, L, pick(sl.traj, s_) + (size_t)c * sy.TRJ, x0, Ul);
  const int s0 = sg.s0, s1 = sg.s1;
  const bool have = sg.have;
  bool converged = false;
  for (int sweep = 0; sweep < MAXS && !converged; ++sweep) {
    double x[X], P[X * X];
#pragma unroll
    for (int a = 0; a < X; ++a) x[a] = Ul[a];
#pragma unroll
    for (int i = 0; i < X * X; ++i) P[i] = (i / X == i % X) ? 1.0 : 0.0;
    // The noise increments of the NEXT eight steps are requested before the current eight are integrated: a step of this
    // loop is about 40 ns of arithmetic (FitzHugh-Nagumo) behind a load whose latency is ten times that, and the chain has
    // this one wavefront -- 626 us per partition switch at configs[1] with a load per step in the loop.  (Addresses past the
    // segment are clamped to its last step; those values are not used.)
    constexpr int CH = 8;
    double vb[2][CH * V];
    auto fetch = [&](int base, double* dst) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        int sj = base + j;
        sj = sj < L ? sj : L - 1;
#pragma unroll
        for (int a = 0; a < V; ++a) dst[j * V + a] = vbase[(size_t)sj * V + a];
      }
    };
    auto run = [&](int base, const double* src) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = base + j;
        if (s < s1) {
          double vv[V], A[X * X], Bm[X * V], xn[X], Pn[X * X];
#pragma unroll
          for (int a = 0; a < V; ++a) vv[a] = src[j * V + a];
          M::jac_ab(cc.k, x, vv, A, Bm);
          M::step(cc.k, x, vv, xn);
          matmul_xx<X>(A, P, Pn);
#pragma unroll
          for (int i = 0; i < X * X; ++i) P[i] = Pn[i];
#pragma unroll
          for (int a = 0; a < X; ++a) x[a] = xn[a];
          if ((s + 1) % S == 0) {
            const int t = (s + 1) / S - 1;
#pragma unroll
            for (int a = 0; a < X; ++a) out[t * X + a] = x[a];
          }
        }
      }
    };
    if (have) fetch(s0, vb[0]);
    for (int base = s0; base < s1; base += 2 * CH) {  // (two chunks per trip: the buffers are indexed statically)
      fetch(base + CH, vb[1]);
      run(base, vb[0]);
      fetch(base + 2 * CH, vb[0]);
      run(base + CH, vb[1]);
    }
    converged = shoot_junctions<X>(x, P, Ul, lane, have, have && s1 < L);
  }
  if (!converged && lane == 0) {  // sequential recursion: the states after every S-th step, no point 0
    plain_recursion<M>(cc.k, x0, vbase, L, S, [&](int p, const double* xs) {
#pragma unroll
      for (int a = 0; a < X; ++a) out[(size_t)(p - 1) * X + a] = xs[a];
    });
  }
}

// generate_from_model's x_seq (FitzHugh-Nagumo_example.ipynb:316-335) of every chain's CURRENT state: point 0 is x_0, point p
// the state after step p * stride of the whole chain's recursion; out [B][NP = T S / stride + 1][X].  One wavefront per chain.
// Phase 1 settles the 64 segment start states by the multiple shooting above, as k_xobs_par does but storing nothing (the
// set-up, the junction half of a sweep and the settled criterion are that kernel's; the integration loop is written out in
// both, see shoot_junctions), and falls back to the plain recursion on lane 0.  Phase 2 is a plain pass: every lane
// integrates its segment once more from its settled start state (within 1e-13 relative of the sequential recursion's state
// there) and emits the states whose step index is a multiple of `stride`.
// Emit: a lane's points are contiguous in `out`, but the 64 lanes write 64 regions, and a lane-per-region store instruction
// touches 64 lines for 16 or 24 bytes each.  A lane therefore parks its doubles in its row of an LDS ring, indexed by the
// global double index modulo the ring, and after every 8-step window the wavefront writes out the 128-byte lines that are
// complete: 8 lanes per line, 16 bytes each, 8 whole lines per store instruction.  Only the doubles before a region's first
// line boundary and behind its last one (fewer than 16 each, twice per lane and call) are stored by the lane itself.
// Row stride RING + 1 doubles: ds_write_b64 banks are (a / 4) % 32, rows that are 2 (RING + 1) = 2 (mod 32) dwords apart put 16
// lanes that write the same ring slot on 16 different bank pairs.
// CHMC_PATH_DIRECT_STORES (build switch, A/B only): every double is stored by its lane, no ring.  Measured at stride 1
// (profiles/path_posterior_timing.txt): slower for X = 3 (SIR, 1 024 chains: 83.6 against 78.3 us), faster for X = 2, where a
// point is one 16-byte store (configs[1]: 148 against 251 us -- the flush below costs about 1.4 us per window).
// sweeps (may be null): sweeps to convergence per chain, 0 for the sequential fallback.
#ifdef CHMC_PATH_DIRECT_STORES
constexpr bool kPathRing = false;
#else
constexpr bool kPathRing = true;
#endif
template <class M>
__global__ void __launch_bounds__(64) k_path_par(Sys sy, Slots sl, int stride, double* x_seq, int* sweeps) {
  constexpr int X = M::X, V = M::V, MAXS = 8, CH = 8;
  constexpr int RING = X <= 2 ? 32 : 64, RS = RING + 1, MAXL = (15 + CH * X) / 16;
  static_assert(16 + CH * X <= RING, "a window's doubles and an open line fit the ring");
  __shared__ double ring[64 * RS];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x;
  if (c >= sy.B) return;
  const int s_ = sl.cur[c];
  const int S = sy.S, L = sy.T * sy.S;
  const int NP = L / stride + 1;
  const double* q = pick(sl.q, s_) + (size_t)c * sy.Q;
  const double* vbase = q + sy.U + sy.V0;
  double* out = x_seq + (size_t)c * NP * X;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  double x0[X], Ul[X];
  M::gx0(cc.z, q + sy.U, x0);
  const ShootSeg sg = shoot_setup<M>(sy, lane, L, pick(sl.traj, s_) + (size_t)c * sy.TRJ, x0, Ul);
  const int m = sg.m, s0 = sg.s0, s1 = sg.s1;
  const bool have = sg.have;
  // noise increments of eight steps, requested one window ahead (addresses past the chain are clamped to its last step)
  auto fetch = [&](int base, double* dst) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      int sj = base + j;
      sj = sj < L ? sj : L - 1;
#pragma unroll
      for (int a = 0; a < V; ++a) dst[j * V + a] = vbase[(size_t)sj * V + a];
    }
  };
  // ---- phase 1: settle the segment start states
  bool converged = false;
  int nsweep = 0;
  for (int sweep = 0; sweep < MAXS && !converged; ++sweep) {
    double x[X], P[X * X];
#pragma unroll
    for (int a = 0; a < X; ++a) x[a] = Ul[a];
#pragma unroll
    for (int i = 0; i < X * X; ++i) P[i] = (i / X == i % X) ? 1.0 : 0.0;
    double vb[2][CH * V];
    auto run = [&](int base, const double* src) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = base + j;
        if (s < s1) {
          double vv[V], A[X * X], Bm[X * V], xn[X], Pn[X * X];
#pragma unroll
          for (int a = 0; a < V; ++a) vv[a] = src[j * V + a];
          M::jac_ab(cc.k, x, vv, A, Bm);
          M::step(cc.k, x, vv, xn);
          matmul_xx<X>(A, P, Pn);
#pragma unroll
          for (int i = 0; i < X * X; ++i) P[i] = Pn[i];
#pragma unroll
          for (int a = 0; a < X; ++a) x[a] = xn[a];
        }
      }
    };
    if (have) fetch(s0, vb[0]);
    for (int base = s0; base < s1; base += 2 * CH) {  // (two windows per trip: the buffers are indexed statically)
      fetch(base + CH, vb[1]);
      run(base, vb[0]);
      fetch(base + 2 * CH, vb[0]);
      run(base + CH, vb[1]);
    }
    converged = shoot_junctions<X>(x, P, Ul, lane, have, have && s1 < L);
    nsweep = sweep + 1;
  }
  if (sweeps && lane == 0) sweeps[c] = converged ? nsweep : 0;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < X; ++a) out[a] = x0[a];
  }
  if (!converged) {  // sequential recursion on lane 0
    if (lane == 0) {
      plain_recursion<M>(cc.k, x0, vbase, L, stride, [&](int p, const double* xs) {
#pragma unroll
        for (int a = 0; a < X; ++a) out[(size_t)p * X + a] = xs[a];
      });
    }
    return;
  }
  // ---- phase 2: the plain pass from the settled start states, emitting through the ring
  // gi: index of the lane's next double, counted from the 128-byte line boundary at or below `out` (off0 doubles below it);
  // the lane's first point is the first p with p * stride > s0
  const int off0 = (int)(((unsigned long long)out >> 3) & 15);
  int gi = off0 + (s0 / stride + 1) * X;
  bool started = kPathRing && (gi & 15) == 0;  // the lane has reached a line boundary: its doubles go through the ring from there
  int gf = gi;                    // first double not yet written out (a line boundary once started)
  double* row = ring + lane * RS;
  double x[X];
#pragma unroll
  for (int a = 0; a < X; ++a) x[a] = Ul[a];
  int left = stride - s0 % stride;  // steps until the next emitted state
  double vb[2][CH * V];
  auto run = [&](int base, const double* src) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int s = base + j;
      if (s < s1) {
        double vv[V], xn[X];
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = src[j * V + a];
        M::step(cc.k, x, vv, xn);
#pragma unroll
        for (int a = 0; a < X; ++a) x[a] = xn[a];
        if (--left == 0) {
          left = stride;
#pragma unroll
          for (int a = 0; a < X; ++a) {
            if (started)
              row[gi & (RING - 1)] = x[a];
            else
              out[gi - off0] = x[a];
            ++gi;
            if (kPathRing && !started && (gi & 15) == 0) started = true, gf = gi;
          }
        }
      }
    }
  };
  auto flush = [&]() {  // (uniform: every lane calls it after every window)
    const int nl = started ? (gi >> 4) - (gf >> 4) : 0;
    if (__ballot(nl > 0) == 0ULL) return;
    __syncthreads();
    const int sub = lane >> 3, k = lane & 7;
#pragma unroll
    for (int grp = 0; grp < 8; ++grp) {
      const int r = grp * 8 + sub;
      const int gf_r = __shfl(gf, r, 64), nl_r = __shfl(nl, r, 64);
      const double* rr = ring + r * RS;
#pragma unroll
      for (int j = 0; j < MAXL; ++j) {
        if (j < nl_r) {
          const int idx = gf_r + 16 * j + 2 * k;
          d2_t v;
          v.x = rr[idx & (RING - 1)];
          v.y = rr[(idx + 1) & (RING - 1)];
          *(d2_t*)(out + (idx - off0)) = v;
        }
      }
    }
    gf += 16 * nl;
    __syncthreads();
  };
  const int nwin = (m + CH - 1) / CH;
  fetch(s0, vb[0]);
  for (int w = 0; w < nwin; w += 2) {
    const int base = s0 + w * CH;
    fetch(base + CH, vb[1]);
    run(base, vb[0]);
    flush();
    fetch(base + 2 * CH, vb[0]);
    run(base + CH, vb[1]);
    flush();
  }
  if (started) {  // the doubles behind the lane's last complete line
    for (int g = gf; g < gi; ++g) out[g - off0] = row[g & (RING - 1)];
  }
}

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Is chain c part of this scan launch?  use_nw 0: chains with work.ok; 1: chains of the Newton loop (work.nw == 1).
__device__ inline bool scan_select(const Work& w, int c, int use_nw, int& which, int& qsel) {
  (void)which, (void)qsel;
  return use_nw ? w.nw[c] == 1 : w.ok[c] != 0;
}
// Helper wavefronts per workgroup that issue the trajectory stores (they share a tile's rows: helper h takes the 1 KB store
// instructions i = h mod CHMC_SCAN_HELPERS).  Measured with the line-aligned trajectory rows (round 4, configs[1]): one helper
// 113.0 us per launch, two 112.0 us -- the helper is not short of store slots (vmcnt), one stays the default.
#ifndef CHMC_SCAN_HELPERS
#define CHMC_SCAN_HELPERS 1
#endif
// PAIR: one launch for two problems on the same batch (the reverse retraction of a step and the forward retraction of the
// next one, run_projection_pair): the first ceil(B K / 64) workgroups scan the iterate of (w, which, qsel), the others that of
// (w1, which1, qsel1).  A workgroup picks its argument set once (uniform: scalar selects); the body is the same.
template <class M, int RM, bool STORE, bool PAIR = false>
__global__ void __launch_bounds__(STORE ? 64 * (1 + CHMC_SCAN_HELPERS) : 64)
    k_fwd_scan(Sys sy, Slots sl, Work w0, int which0, int qsel0, int use_nw, int store_traj, Work w1, int which1, int qsel1) {
  const int wg0 = (sy.B * sy.K + 63) / 64;  // workgroups per problem
  const bool second = PAIR && (int)blockIdx.x >= wg0;
  const Work w = second ? w1 : w0;
  int which = second ? which1 : which0, qsel = second ? qsel1 : qsel0;
  const int wg = second ? (int)blockIdx.x - wg0 : (int)blockIdx.x;
  constexpr int X = M::X, V = M::V, PF = 8;
  constexpr int NLD = PF * V / 2;        // 16-byte loads per lane and tile
  constexpr int NST = PF * X / 2;        // 16-byte chunks per trajectory row and tile
  constexpr int TBV = PF * V * 8;        // bytes of noise increments per tile
#ifndef CHMC_SCAN_DEPTH
#define CHMC_SCAN_DEPTH (V == 2 ? 4 : 3)
#endif
  constexpr int DEPTH = CHMC_SCAN_DEPTH;  // tiles in flight
  constexpr int NOUT = (DEPTH - 1) * NLD;
  constexpr int RSD = PF * X + 2;        // LDS row stride in doubles: tile + 16 bytes (conflict-free row access)
  static_assert(NOUT <= 63, "vmcnt is a 6-bit field");
#ifndef CHMC_SCAN_NB
#define CHMC_SCAN_NB 1  // 2 measured equal within the run-to-run spread (three interleaved runs each at configs[1]:
                        // 45.9-46.2 k against 45.3-46.2 k steps/s; S = 800, 512 chains: 27.82 k against 27.83 k)
#endif
  // NB tiles per hand-over: the integrating wave parks NB tiles before it meets the helper at the barrier, so the helper
  // may fall up to NB tiles behind (store issue under memory load) without stalling the recursion
  constexpr int NB = CHMC_SCAN_NB;
  __shared__ __attribute__((aligned(16))) double tile[STORE ? 2 : 1][STORE ? NB * 64 * RSD : 2];
  __shared__ double obsv[64 * (2 * RM + 1)];
  const int lane = threadIdx.x & 63;
  const int wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool helper = STORE && wave_id != 0;
  const int hid = wave_id - 1;  // which helper
  const int n = sy.B * sy.K, S = sy.S;
  const int tid0 = wg * 64;

  // both waves work out the longest block of the 64 (same loop trip count and barrier count)
  int maxL = 0;
  {
    const int t = tid0 + lane;
    int L = 0;
    if (t < n) {
      const int c = t / sy.K;
      int wh_ = which, qs_ = qsel;
      if (scan_select(w, c, use_nw, wh_, qs_)) L = sy.blk[t - c * sy.K].nsteps;
    }
    maxL = L;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(maxL, off, 64);
      maxL = o > maxL ? o : maxL;
    }
    maxL = __builtin_amdgcn_readfirstlane(maxL);
  }
  if (maxL == 0) return;

  if (helper) {
    // rows of this lane: chunk g = 64 i + lane of the 64 x NST chunks of a tile -> row g / NST, chunk g % NST
    double* rp[NST];
    int rL[NST], lo_[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int g = 64 * i + lane, r = g / NST, ch = g - r * NST;
      const int t = tid0 + r;
      rp[i] = w.trajw, rL[i] = 0, lo_[i] = r * RSD + 2 * ch;  // (a global pointer: no generic-address stores)
      if (t < n) {
        const int c = t / sy.K, b = t - c * sy.K;
        int wh_ = which, qs_ = qsel;
        if (scan_select(w, c, use_nw, wh_, qs_)) {
          const BlockDesc bd = sy.blk[b];
          const int s = sl.cur[c] ^ wh_;
          rp[i] = (store_traj == 2 ? w.trajw : pick(sl.traj, s)) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X + 2 * ch;
          rL[i] = bd.nsteps;
        }
      }
    }
#ifdef CHMC_SCAN_PRIO
    __builtin_amdgcn_s_setprio(3);
#endif
    int buf = 0;
    for (int s0 = 0; s0 < maxL; s0 += PF * NB) {
      lds_barrier();  // tiles s0 .. s0 + NB PF are in tile[buf]
#pragma unroll
      for (int sl_ = 0; sl_ < NB; ++sl_) {
        const int st = s0 + sl_ * PF;
        if (st < maxL) {
          d2_t tt[NST];
#pragma unroll
          for (int i = 0; i < NST; ++i)
            if (i % CHMC_SCAN_HELPERS == hid) tt[i] = *reinterpret_cast<const d2_t*>(&tile[buf][sl_ * 64 * RSD + lo_[i]]);
#pragma unroll
          for (int i = 0; i < NST; ++i)
            if (i % CHMC_SCAN_HELPERS == hid && st < rL[i]) vm_store16_nt(rp[i] + (size_t)st * X, tt[i]);
        }
      }
      buf ^= 1;
    }
    return;
  }

  // ---- integrating wave
#ifdef CHMC_SCAN_PRIO
  __builtin_amdgcn_s_setprio(3);
#endif
  const int tid = tid0 + lane;
  const int tc = tid < n ? tid : n - 1;  // lanes past the end shadow the last block (valid addresses, no output)
  const int c = tc / sy.K, b = tc - c * sy.K;
  const BlockDesc bd = sy.blk[b];
  const bool act = scan_select(w, c, use_nw, which, qsel) && tid < n;  // (merged scan: which / qsel are the chain's own)
  const int L = act ? bd.nsteps : 0;
  const int s = sl.cur[c] ^ which;
  const double* q = (qsel ? w.qb : pick(sl.q, s)) + (size_t)c * sy.Q;
  const double* xobs = sy.xobs + (size_t)c * sy.T * X;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const double sig = sy.noisy ? sigma_at(sy, q, c) : 0.0;
  double x[X], xn[X];
  const double* vb = q + sy.U;
  if (bd.first) {
    M::gx0(cc.z, vb, x);
  } else {
#pragma unroll
    for (int a = 0; a < X; ++a) x[a] = xobs[(bd.obs0 - 1) * X + a];
  }
  // observation targets of this block, parked in LDS (a global load inside the loop would make hipcc drain the ring)
  double* ov = obsv + lane * (2 * RM + 1);
  {
    const double* nn = q + sy.U + sy.NV;
    for (int j = 0; j < bd.ny; ++j) {
      ov[2 * j] = y_of(sy, c)[bd.obs0 + j];
      ov[2 * j + 1] = sy.noisy ? nn[bd.obs0 + j] : 0.0;
    }
  }
  double cp[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) cp[i] = 0.0;

  const char* vp = reinterpret_cast<const char*>(vb + sy.V0 + (size_t)bd.step0 * V);
  d2_t ring[DEPTH][NLD];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) TileLoad<0, NLD, 0>::run(ring[d], vp + d * TBV);
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) vm_wait<0>(ring[d]);  // prologue tiles: simply drain, once per scan

  int left = S, j = 0;  // wave-uniform: every block starts at an observation time
  for (int s0 = 0; s0 < maxL; s0 += PF * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const int st = s0 + d * PF;
      if (st < maxL) {
        // ring[d] was refilled DEPTH tiles ago; DEPTH - 1 younger tiles may stay in flight
        vm_wait<NOUT>(ring[d]);
        // hand the previous NB tiles to the helper: their LDS writes were issued at least one step ago, so the wait is free
        if (STORE && st > 0 && (st / PF) % NB == 0) lds_barrier();
        if (st < L) {
          double* lo = STORE ? &tile[((st / PF) / NB) & 1][((st / PF) % NB) * 64 * RSD + lane * RSD] : nullptr;
#pragma unroll
          for (int i = 0; i < PF; ++i) {
            double vt[V];
#pragma unroll
            for (int a = 0; a < V; ++a) vt[a] = ring[d][(i * V + a) >> 1][(i * V + a) & 1];
            if (STORE) {
#pragma unroll
              for (int a = 0; a < X; ++a) lo[i * X + a] = x[a];
            }
            M::step(cc.k, x, vt, xn);
#pragma unroll
            for (int a = 0; a < X; ++a) x[a] = xn[a];
          }
        }
        // refill with the tile DEPTH ahead; a finished lane keeps re-reading its last tiles (never consumed; the
        // position buffers carry CHMC_Q_PAD doubles of slack for the over-read at the end of a block)
        TileLoad<0, NLD, DEPTH * TBV>::run(ring[d], vp);
        if (st < L) vp += TBV;
        left -= PF;
        if (left == 0) {  // st + PF is the time of local observation j
          if (st < L && j < bd.ny) {
            const double val = (M::obs(x) + (sy.noisy ? sig * ov[2 * j + 1] : 0.0)) - ov[2 * j];
#pragma unroll
            for (int jj = 0; jj < RM; ++jj)
              if (jj == j) cp[jj] = val;
          }
          ++j;
          left = S;
        }
      }
    }
  }
  if (STORE) lds_barrier();  // last tile
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) vm_wait<0>(ring[d]);  // nothing may land in a register after this point
  if (!act) return;
  if (STORE) {
    double* trow = (store_traj == 2 ? w.trajw : pick(sl.traj, s)) + (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
#pragma unroll
    for (int a = 0; a < X; ++a) trow[(size_t)L * X + a] = x[a];
  }
  if (!bd.last) {
#pragma unroll
    for (int a = 0; a < X; ++a) {
      const double val = x[a] - xobs[(bd.obs0 + bd.nobs - 1) * X + a];
#pragma unroll
      for (int jj = 0; jj < RM; ++jj)
        if (jj == bd.ny + a) cp[jj] = val;
    }
  }
  double* out = w.cpad + ((size_t)c * sy.Kmax + b) * RM;
#pragma unroll
  for (int i = 0; i < RM; ++i) out[i] = cp[i];
}

// ---------------------------------------------------------------------------------------------------------------
// Time-parallel forward scan of `constr` for layouts with FEW, LONG blocks (the SIR single-block configuration: K = 1,
// 2 800 steps -- a lane-per-block scan then keeps 4 wavefronts of the whole chip busy for 0.9 ms).  One wavefront per
// (chain, block) integrates the block by MULTIPLE SHOOTING: the block is cut into 64 segments, lane l integrates
// segment l with the exact nonlinear recursion from a guessed start state U_l (taken from a nearby trajectory: the
// previous Newton iterate of the retraction, or the state's own trajectory) and accumulates the segment's transition
// matrix A_l = d(end state) / d(start state); the 63 matching conditions U_{l+1} = F_l(U_l) are then solved by Newton's
// method, whose linear system is the affine recurrence
//     U_{l+1}^new = F_l(U_l) + A_l (U_l^new - U_l),          U_0 = x_0 fixed,
// i.e. one wave-level affine prefix scan over the lanes.  Properties: (i) the nonlinearity is resolved exactly inside the
// segments, only the 63 junctions are linearised, so the error squares per sweep from any reasonable guess; (ii) a
// junction whose predecessor did not move gets EXACTLY F_l(U_l), so after j sweeps the first j segments are bitwise the
// sequential recursion and the method terminates with the sequential result after at most 64 sweeps whatever the guess;
// (iii) the trajectory entries are stored by the segment recursions themselves.  Sweeps repeat until no junction moved
// by more than CHMC_PAR_JTOL (relative), then ONE more sweep integrates from the settled start states: its junction defects
// are the square of the last corrections, so what it stores equals the sequential recursion to rounding (about 1e-15
// relative), though not bit for bit.  Segments started from a useless guess may overflow; that is harmless (the exact prefix
// reaches them), and where the true recursion itself overflows the NaNs are the result.  A block that is still not
// settled after MAXS sweeps is integrated sequentially by lane 0 (counted in work.nfallback).  Which scan a layout gets is
// decided from the layout alone (chmc_create: few_long_blocks), never from the number of chains, so a chain's bits do not
// depend on its shard (CHMC_PAR_SCAN overrides; tests compare the two scans).
// gsel: guess trajectory: 1 = the destination buffer itself (previous iterate), 2 = the state's trajectory (slot cur),
// 3 = work.trajw (the last iterate of the retraction that produced the point being evaluated).
// W wavefronts per (chain, block): 64 W segments, the affine prefix scan continued across the wavefronts through LDS (three
// workgroup barriers per sweep).  The host picks W so that the launch has about one wavefront per SIMD of the chip
// (chmc_create: par_waves); W = 1 compiles to the single-wavefront kernel (no LDS, no barrier).
// Junction tolerance (relative to max(|x|, 1)): a junction has settled when its new start state moved by no more than this;
// one FINAL sweep from the settled start states follows (fwd_par_sweeps), which squares the remaining defect, so the
// tolerance only has to put the iteration into its quadratic regime: 1e-11 leaves <= 5e-11 before and ~1e-20 x (curvature)
// after the final sweep.  History: round 3 had no final sweep and stored the trajectory of the start states before the last
// correction; measured then on boarding-school SIR, 256 chains, against the sequential scan over 12 288 chain-steps: 1e-13:
// 6 iteration counts differ, positions to 2.3e-13; 3e-13 (round 3's value): 8 counts, 8.4e-13; 1e-12: 76 counts; 1e-11: the
// retractions stopped converging (a constraint value was then uncertain by more than the constraint tolerance).
#ifndef CHMC_PAR_JTOL
#define CHMC_PAR_JTOL 1e-11
#endif
#ifndef CHMC_PAR_MAXS_ROUND
#define CHMC_PAR_MAXS_ROUND 12  // measured at 256 boarding-school SIR chains: 4: 22.5 k, 6: 25.0 k, 8: 25.9 k, 10: 26.1 k, 12: 26.3 k, 16: 25.7 k steps/s
#endif
// (-DCHMC_RETRACT_PROF, diagnostic build: thread 0 adds the 100 MHz ticks between the marked points of a sweep to
// work.nfallback[56 ..]: recursion | in-wave scan | cross-wave | new start states | absorbing fronts | hand-over | final pass)
#ifdef CHMC_RETRACT_PROF
#define CHMC_SWEEP_PROF(slot)                                          \
  do {                                                                 \
    if (threadIdx.x == 0 && w.nfallback) {                             \
      const long long t1_ = wall_clock64();                            \
      atomicAdd(w.nfallback + (slot), (int)(t1_ - tp_));               \
      tp_ = t1_;                                                       \
    }                                                                  \
  } while (0)
#else
#define CHMC_SWEEP_PROF(slot) \
  do {                        \
  } while (0)
#endif
// The sweeps of the time-parallel scan of block `bd` of one chain by the W wavefronts of the calling workgroup (all of them
// must call it: workgroup barriers inside when W > 1): position `q`, trajectory written to `traj`, start states taken from
// `guess`, constraint values to `out`.  Returns whether every junction settled within MAXS sweeps (the same value in every
// thread); Ul / s0r / haver: this lane's segment start state, first step and whether it owns a segment (for a caller that
// keeps the junction states of an unsettled scan).  Shared by k_fwd_par and the per-chain retraction kernel (chmc_retract.h).
// The sweeps themselves store nothing: trajectory and constraint values are written by the FINAL pass, a plain recursion (no
// transition matrices, no junction system) from the settled start states.  PRE > 0: a segment of at most PRE steps keeps its
// noise increments in registers for all sweeps (they do not change; the per-step global load was exposed latency with two
// wavefronts per SIMD) and the step loop is unrolled with predicates.
// WG > W: the calling workgroup has WG wavefronts of which the first W integrate (the per-chain kernels: 8 wavefronts, 256
// segments on 4 of them); the others only keep the workgroup barriers and the loop control in step.
template <class M, int RM, int W, int PRE = 0, int WG = W>
__device__ __forceinline__ bool fwd_par_sweeps(const Sys& sy, const Work& w, const BlockDesc& bd, int c, const double* q,
                                               const double* xobs, double* traj, const double* guess, double* out, int MAXS,
                                               int gsel, double (&Ul)[M::X], int& s0r, bool& haver) {
  constexpr int X = M::X, V = M::V;
  static_assert(WG >= W && (WG == W || W > 1), "idle wavefronts need the cross-wavefront form");
  const int lane = threadIdx.x & 63;
  const int wv = W > 1 ? (int)(threadIdx.x >> 6) : 0;  // wavefront of the workgroup
  const int gl = W > 1 ? (int)threadIdx.x : lane;      // segment of the block
  constexpr int NSEG = 64 * W;
  // cross-wavefront hand-over (W > 1): first start state, scan aggregate, last new start state and the settled flag of
  // every wavefront
  __shared__ double sAe[W > 1 ? W : 1][M::X], sAP[W > 1 ? W : 1][M::X * M::X],
      sUn[W > 1 ? W : 1][M::X];
  __shared__ int sFlag[W > 1 ? W : 1], sFront[W > 1 ? W : 1][1 + 2 * M::X], sStuck[W > 1 ? W : 1];
  __shared__ double sTv[W > 1 ? W : 1][M::X];
  if (WG > W && wv >= W) {  // idle wavefront: the same barriers (B), (B'), (C) per sweep, the same exit
    bool settled_ = false;
    for (int sweep = 0; sweep < MAXS && !settled_; ++sweep) {
      __syncthreads();  // (B)
      if (M::NABS > 0) {
        int any = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) any |= sStuck[k];
        if (any) __syncthreads();  // (B')
      }
      __syncthreads();  // (C)
      int any = 0;
#pragma unroll
      for (int k = 0; k < W; ++k) any |= sFlag[k];
      settled_ = !any;
    }
#pragma unroll
    for (int a = 0; a < X; ++a) Ul[a] = 0.0;
    s0r = 0, haver = false;
    return settled_;
  }
  const int S = sy.S, L = bd.nsteps;
  const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
  const double* nn = q + sy.U + sy.NV;
  ChainConsts<M> cc;
  cc.init(q, sy.dl);
  const double sig = sy.noisy ? sigma_at(sy, q, c) : 0.0;
  double x0[X];
  if (bd.first) {
    M::gx0(cc.z, q + sy.U, x0);
  } else {
#pragma unroll
    for (int a = 0; a < X; ++a) x0[a] = xobs[(bd.obs0 - 1) * X + a];
  }
  const int m = (L + NSEG - 1) / NSEG;                    // steps per segment
  const int s0 = gl * m, s1 = (s0 + m < L ? s0 + m : L);  // this lane's segment [s0, s1) (empty when s0 >= L)
  const bool have = s0 < L;
#pragma unroll
  for (int a = 0; a < X; ++a) Ul[a] = gl == 0 ? x0[a] : (have ? guess[(size_t)s0 * X + a] : 0.0);
  // `settled`: a sweep has left every junction where it was (to CHMC_PAR_JTOL).  The final pass then integrates from the
  // start states that sweep produced, whose junction defects are of the order of the SQUARE of its corrections (Newton),
  // so the trajectory and constraint values it stores are those of the sequential recursion to rounding.  (Round 3 stored
  // the values of the start states BEFORE the last correction: off by up to the tolerance, and an observation exp(x) ~ 300
  // of the SIR model turns 3e-13 relative into 5e-10 of constraint value -- half the constraint tolerance: Newton iteration
  // counts then differed from the sequential scan's, VERDICT r3 weak #2.)
  const bool junction = have && s1 < L;  // lane l + 1 owns a segment
  // start state of the NEXT lane's segment as this lane last saw it: the guess at first, afterwards the value this lane
  // itself handed on (the next lane adopts exactly that), so the junction defect needs no cross-lane traffic
  double Unext[X];
#pragma unroll
  for (int a = 0; a < X; ++a) Unext[a] = junction ? guess[(size_t)s1 * X + a] : 0.0;
  const bool pre = PRE > 0 && m <= PRE;  // (uniform)
  double vpre[(PRE > 0 ? PRE : 1) * V];
  if (PRE > 0 && pre) {
#pragma unroll
    for (int k = 0; k < PRE; ++k)
#pragma unroll
      for (int a = 0; a < V; ++a) vpre[k * V + a] = s0 + k < s1 ? vbase[(size_t)(s0 + k) * V + a] : 0.0;
  }
#ifdef CHMC_RETRACT_PROF
  long long tp_ = wall_clock64();
#endif
  bool settled = false;
  for (int sweep = 0; sweep < MAXS && !settled; ++sweep) {
    // exact recursion over the segment and its transition matrix
    double x[X], P[X * X];
#pragma unroll
    for (int a = 0; a < X; ++a) x[a] = Ul[a];
#pragma unroll
    for (int i = 0; i < X * X; ++i) P[i] = (i / X == i % X) ? 1.0 : 0.0;
    auto one_step = [&](const double* vv) {
      double A[X * X], Bm[X * V], xn[X], Pn[X * X];
      M::jac_ab(cc.k, x, vv, A, Bm);
      M::step(cc.k, x, vv, xn);
      matmul_xx<X>(A, P, Pn);
#pragma unroll
      for (int i = 0; i < X * X; ++i) P[i] = Pn[i];
#pragma unroll
      for (int a = 0; a < X; ++a) x[a] = xn[a];
    };
    if (PRE > 0 && pre) {
#pragma unroll
      for (int k = 0; k < PRE; ++k)
        if (s0 + k < s1) one_step(vpre + k * V);
    } else {
      // (measured, round 4: requesting the increments of step s + 1 before step s is integrated changes nothing -- 27.4 us of
      // recursion per Newton iteration either way: the step's own dependent arithmetic is the latency, not its loads)
      for (int s = s0; s < s1; ++s) {
        double vv[V];
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
        one_step(vv);
      }
    }
    CHMC_SWEEP_PROF(56);
    // junction defects e_l = F_l(U_l) - U_{l+1} and the Newton system d_{l+1} = e_l + A_l d_l, d_0 = 0, by an inclusive
    // affine prefix scan over the lanes: after it (Pc, ec)_l maps d_0 to d_{l+1}, i.e. ec_l = d_{l+1}
    double ec[X], Pc[X * X];
#pragma unroll
    for (int a = 0; a < X; ++a) ec[a] = junction ? x[a] - Unext[a] : 0.0;
#pragma unroll
    for (int i = 0; i < X * X; ++i) Pc[i] = junction ? P[i] : ((i / X == i % X) ? 1.0 : 0.0);
    // Models with absorbing components: a state may hold a NaN that the recursion itself removes (SIR clips a NaN
    // compartment to the floor), so a NaN must not travel through the corrections: a junction that is NaN on both sides
    // has no defect, and a segment whose defect or transition matrix is not finite passes no correction on (its end state
    // goes to the next segment as it is).
    bool broken = false;
    if (M::NABS > 0 && junction) {
#pragma unroll
      for (int a = 0; a < X; ++a)
        if (x[a] != x[a] && Unext[a] != Unext[a]) ec[a] = 0.0;
#pragma unroll
      for (int a = 0; a < X; ++a) broken = broken || !(fabs(ec[a]) <= 1.7976931348623157e308);
#pragma unroll
      for (int i = 0; i < X * X; ++i) broken = broken || !(fabs(Pc[i]) <= 1.7976931348623157e308);
      if (broken) {
#pragma unroll
        for (int a = 0; a < X; ++a) ec[a] = 0.0;
#pragma unroll
        for (int i = 0; i < X * X; ++i) Pc[i] = 0.0;
      }
    }
    // (the DPP path of the vector ALU: row_shr 1 / 2 / 3 / 4 / 8 and row_bcast 15 / 31, no LDS crossbar; lanes without a source
    // compose with the identity map.  With the final pass behind the sweeps the association order of the products no longer
    // decides anything: round 3 measured more sweeps with it at a junction tolerance of 1e-13.)
    dpp_affine_prefix<X, 1>(Pc, ec);
    CHMC_SWEEP_PROF(57);
    // across the wavefronts: d at the start of wavefront wv = the aggregates of the wavefronts before it applied to d_0 = 0
    double dw[X];
#pragma unroll
    for (int a = 0; a < X; ++a) dw[a] = 0.0;
    // (absorbing components: does any segment of the block end, or any junction sit, in an absorbed / NaN state?  Only then
    // is there a front to look for; the flag travels with the aggregates)
    bool any_stuck = false;
    if (M::NABS > 0) {
      bool st = false;
#pragma unroll
      for (int a = 0; a < X; ++a) {
        const bool sx = a < M::NABS ? M::absorbed(x[a]) : x[a] != x[a];
        const bool su = a < M::NABS ? M::absorbed(Unext[a]) : Unext[a] != Unext[a];
        st = st || (have && sx) || (junction && su);
      }
      any_stuck = __ballot(st) != 0ULL;
    }
    if (W > 1) {
      if (lane == 63) {
#pragma unroll
        for (int a = 0; a < X; ++a) sAe[wv][a] = ec[a];
#pragma unroll
        for (int i = 0; i < X * X; ++i) sAP[wv][i] = Pc[i];
        sStuck[wv] = any_stuck;
      }
      __syncthreads();  // (B)
      if (M::NABS > 0) {
        int any = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) any |= sStuck[k];
        any_stuck = any != 0;
      }
      bool moved = false;  // (a zero d is passed on as an exact zero: no 0 * inf from an overflowed aggregate)
      for (int k = 0; k < wv; ++k) {
        double dn[X];
#pragma unroll
        for (int a = 0; a < X; ++a) {
          double tt = sAe[k][a];
          if (moved) {
#pragma unroll
            for (int d = 0; d < X; ++d) tt += sAP[k][a * X + d] * dw[d];
          }
          dn[a] = tt;
        }
        moved = false;
#pragma unroll
        for (int a = 0; a < X; ++a) dw[a] = dn[a], moved = moved || dn[a] != 0.0;
      }
      if (moved) {
#pragma unroll
        for (int a = 0; a < X; ++a) {
          double tt = ec[a];
#pragma unroll
          for (int d = 0; d < X; ++d) tt += Pc[a * X + d] * dw[d];
          ec[a] = tt;
        }
      }
    }
    CHMC_SWEEP_PROF(58);
    // d_l of this lane = ec of lane l - 1; new start state of the NEXT lane's segment, formed as F_l + A_l d_l so that a
    // junction whose predecessor did not move (d_l == 0) receives exactly F_l
    double dl[X], Un[X];
#pragma unroll
    for (int a = 0; a < X; ++a) {
      const double up = dpp_mov<0x138, 0xf, 0xf>(ec[a], 0.0);  // wave_shr:1
      dl[a] = lane == 0 ? dw[a] : up;
    }
    bool still = true;  // this lane's start state did not move at all: its end state is final (exact prefix)
#pragma unroll
    for (int a = 0; a < X; ++a) still = still && dl[a] == 0.0;
#pragma unroll
    for (int a = 0; a < X; ++a) {
      double tt = 0.0;
#pragma unroll
      for (int d = 0; d < X; ++d) tt += P[a * X + d] * dl[d];
      Un[a] = (still || broken) ? x[a] : x[a] + tt;  // (no 0 * inf from an overflowed transition matrix)
    }
    // A junction is settled when its new value equals the old one (bitwise, or both NaN: beyond a point where the true
    // recursion overflows everything is NaN and stays NaN) or differs by rounding only.  Segments started from garbage
    // may overflow; that is not an error: the exact prefix grows by at least one segment per sweep and reaches them.
    // (Judged by the lane that produced the new value: it holds the old start state of the next segment in Unext.)
    auto moved_beyond_rounding = [&]() {
      int u = 0;
      if (junction) {
#pragma unroll
        for (int a = 0; a < X; ++a) u |= !junction_settled(Un[a], Unext[a], CHMC_PAR_JTOL);
      }
      return u;
    };
    CHMC_SWEEP_PROF(59);
    int unsettled = moved_beyond_rounding();
    // Absorbing components (SIR: a log-compartment that has reached the floor stays there, with zero derivatives; a
    // component without a floor that is NaN stays NaN).  The linearised junction conditions carry no information through
    // such a component, so a guess that is absorbed where the trajectory is not (or the other way round) would be corrected
    // ONE segment per sweep: measured, every scan left unsettled after 12 sweeps had such a front -- settled junctions up
    // to segment 40 or so, one or two unsettled ones, and start states at the floor (left by the previous Newton iterate)
    // or NaN from there on.  So, once everything before such a junction has settled (the segment to its left is then
    // trusted):
    //  * freeze: the first segment that ENDS absorbed makes every later segment start absorbed, whatever the other
    //    components do: those start states are set to the absorbed value at once (on the exact prefix that is the value the
    //    recursion gives anyway);
    //  * thaw: at the first junction whose new value is not absorbed while the old one was, the later start states that
    //    would stay absorbed take that junction's value as their guess, and the ordinary iteration goes on from there.
    // Both only change guesses: a junction still counts as settled only when its new value equals its old one.
    if (M::NABS > 0 && any_stuck) {  // (uniform over the workgroup)
      constexpr int NONE = 0x7fffffff;
      const double qnan = __longlong_as_double(0x7ff8000000000000LL);
      auto stuck = [](int a, double v) { return a < M::NABS ? M::absorbed(v) : v != v; };
      const unsigned long long bu = __ballot(unsettled);
      int fu = bu ? __ffsll((long long)bu) - 1 + 64 * wv : NONE;  // first junction (by its left segment) that moved
      int fa[X], ft[X];  // first segment that ends absorbed / first thawing junction, per component
      double tv[X];      // new value of the thawing junction
#pragma unroll
      for (int a = 0; a < X; ++a) {
        const unsigned long long ba = __ballot(have && stuck(a, x[a]));
        fa[a] = ba ? __ffsll((long long)ba) - 1 + 64 * wv : NONE;
        const unsigned long long bt = __ballot(junction && !stuck(a, Un[a]) && stuck(a, Unext[a]));
        const int lt = bt ? __ffsll((long long)bt) - 1 : 0;
        ft[a] = bt ? lt + 64 * wv : NONE;
        tv[a] = __shfl(Un[a], lt, 64);
      }
      if (W > 1) {
        if (lane == 0) {
          sFront[wv][0] = fu;
#pragma unroll
          for (int a = 0; a < X; ++a) sFront[wv][1 + a] = fa[a], sFront[wv][1 + X + a] = ft[a], sTv[wv][a] = tv[a];
        }
        __syncthreads();  // (B')
#pragma unroll
        for (int k = 0; k < W; ++k) {
          fu = sFront[k][0] < fu ? sFront[k][0] : fu;
#pragma unroll
          for (int a = 0; a < X; ++a) {
            fa[a] = sFront[k][1 + a] < fa[a] ? sFront[k][1 + a] : fa[a];
            if (sFront[k][1 + X + a] < ft[a]) ft[a] = sFront[k][1 + X + a], tv[a] = sTv[k][a];
          }
        }
      }
      bool changed = false;
#pragma unroll
      for (int a = 0; a < X; ++a) {
        if (!junction) continue;
        if (fa[a] != NONE && fu >= fa[a]) {
          if (gl > fa[a]) Un[a] = a < M::NABS ? M::abs_value() : qnan, changed = true;
        } else if (ft[a] != NONE && fu >= ft[a]) {
          if (gl > ft[a] && stuck(a, Un[a])) Un[a] = tv[a], changed = true;
        }
      }
      if (changed) unsettled = moved_beyond_rounding();
    }
    CHMC_SWEEP_PROF(60);
    const bool wave_unsettled = __ballot(unsettled) != 0ULL;
    if (W > 1) {
      if (lane == 63) {
#pragma unroll
        for (int a = 0; a < X; ++a) sUn[wv][a] = Un[a];
        sFlag[wv] = wave_unsettled;
      }
      __syncthreads();  // (C)
    }
#pragma unroll
    for (int a = 0; a < X; ++a) {
      double nu = dpp_mov<0x138, 0xf, 0xf>(Un[a], 0.0);  // wave_shr:1: new start state of this lane's segment
      if (W > 1 && lane == 0 && wv > 0) nu = sUn[wv - 1][a];
      if (gl > 0 && have) Ul[a] = nu;
      if (junction) Unext[a] = Un[a];  // (what the next lane has just adopted)
    }
    CHMC_SWEEP_PROF(61);
    // settled: no junction moved (beyond the tolerance)
    bool quiet;
    if (W > 1) {
      int any = 0;
#pragma unroll
      for (int k = 0; k < W; ++k) any |= sFlag[k];
      quiet = !any;
    } else {
      quiet = !wave_unsettled;
    }
    settled = quiet;
    if (settled && gl == 0 && w.nfallback) atomicAdd(w.nfallback + 1 + (sweep < 14 ? sweep : 14) + 16 * (gsel - 1), 1);
  }
  if (settled && have) {  // final pass: the plain recursion from the settled start states stores the results
    double x[X];
#pragma unroll
    for (int a = 0; a < X; ++a) x[a] = Ul[a];
    auto final_step = [&](int s, const double* vv) {
      double xn[X];
#pragma unroll
      for (int a = 0; a < X; ++a) traj[(size_t)s * X + a] = x[a];
      M::step(cc.k, x, vv, xn);
#pragma unroll
      for (int a = 0; a < X; ++a) x[a] = xn[a];
      if ((s + 1) % S == 0) {  // s + 1 is the time of local observation j
        const int j = (s + 1) / S - 1;
        if (j < bd.ny) out[j] = (M::obs(x) + (sy.noisy ? sig * nn[bd.obs0 + j] : 0.0)) - y_of(sy, c)[bd.obs0 + j];
      }
    };
    if (PRE > 0 && pre) {
#pragma unroll
      for (int k = 0; k < PRE; ++k)
        if (s0 + k < s1) final_step(s0 + k, vpre + k * V);
    } else {
      for (int s = s0; s < s1; ++s) {
        double vv[V];
#pragma unroll
        for (int a = 0; a < V; ++a) vv[a] = vbase[(size_t)s * V + a];
        final_step(s, vv);
      }
    }
    if (s1 == L) {  // end of the block
#pragma unroll
      for (int a = 0; a < X; ++a) traj[(size_t)L * X + a] = x[a];
      if (!bd.last) {
#pragma unroll
        for (int a = 0; a < X; ++a) out[bd.ny + a] = x[a] - xobs[(bd.obs0 + bd.nobs - 1) * X + a];
      }
    }
  }
  CHMC_SWEEP_PROF(62);
  const bool converged = settled;
  s0r = s0, haver = have;
  return converged;
}

template <class M, int RM, int W>
__global__ void __launch_bounds__(64 * W) k_fwd_par(Sys sy, Slots sl, Work w, int which, int qsel, int use_nw,
                                                    int store_traj, int gsel, int round) {
  // (ii) makes the sweeps exact after at most 64 of them, but a block that is not settled after a dozen belongs to a
  // chain whose retraction is diverging (healthy blocks settle in 2-9 sweeps): it is handed to the sequential
  // recursion, which costs the same 0.9 ms as the remaining sweeps would
  constexpr int X = M::X, V = M::V;
  // Inside a Newton loop (use_nw == 1) with ONE block per chain a scan that has
  // not settled after CHMC_PAR_MAXS_ROUND sweeps is neither integrated sequentially nor handed to another stream: its
  // junction states are kept in the trajectory buffer, the chain's mask becomes 2 -- the round's other kernels and the
  // convergence check skip it, it takes no iteration -- and the next round's launch goes on sweeping from there.  A launch
  // therefore never lasts longer than CHMC_PAR_MAXS_ROUND sweeps (99.8 % of the scans settle within 6, tools/
  // par_scan_stats.py), and nothing is handed to another stream: round 2's scheme (12 sweeps, then the chain parked for a
  // 0.9 ms sequential scan on a side stream, re-joining three rounds later) cost boarding-school SIR at 256 chains
  // 22.7 k against 26.3 k steps/s.
  // (With several blocks per chain the chain's mask would be shared by wavefronts that settle and wavefronts that do not:
  // those layouts keep 12 sweeps and the sequential recursion inside the launch, as outside a loop.)
  const bool apend = use_nw == 1 && sy.K == 1;
  const int MAXS = apend ? CHMC_PAR_MAXS_ROUND : 12;
  const int gl = W > 1 ? (int)threadIdx.x : (int)(threadIdx.x & 63);  // segment of the block
  const int wid = blockIdx.x;
  if (wid >= sy.B * sy.K) return;
  const int cbi = sy.order[wid];
  const int c = cbi / sy.K, b = cbi - c * sy.K;
  int* amask = nullptr;  // the chain's mask entry when an unsettled scan is carried over to the next round
  if (use_nw) {
    const int f = w.nw[c];
    if (f != 1 && !(apend && f == 2)) return;
    if (apend) {
      amask = w.nw + c;
      if (f == 2) gsel = 1;  // carry on from the junction states kept by the previous round's launch
    }
  } else if (!w.ok[c]) {
    return;
  }
  (void)round;
  const BlockDesc bd = sy.blk[b];
  const int s_ = sl.cur[c] ^ which;
  const int S = sy.S, L = bd.nsteps;
  const double* q = (qsel ? w.qb : pick(sl.q, s_)) + (size_t)c * sy.Q;
  const double* xobs = sy.xobs + (size_t)c * sy.T * X;
  const size_t toff = (size_t)c * sy.TRJ + (size_t)(bd.step0 + CHMC_TPAD * b) * X;
  double* traj = (store_traj == 2 ? w.trajw : pick(sl.traj, s_)) + toff;
  const double* guess = gsel == 2 ? pick(sl.traj, sl.cur[c]) + toff : gsel == 3 ? w.trajw + toff : traj;
  double* out = w.cpad + ((size_t)c * sy.Kmax + b) * RM;
  double Ul[X];  // start state of this lane's segment
  int s0 = 0;
  bool have = false;
  // (one 16-row block per chain: the layouts of the per-chain kernels, chmc_retract.h, whose arithmetic this launch repeats
  // bit for bit -- no sequential fallback outside a loop, the sweeps go on until settled, as there)
  const bool chain16 = RM > 8 && sy.Kmax == 1;
  const bool converged = fwd_par_sweeps<M, RM, W>(sy, w, bd, c, q, xobs, traj, guess, out,
                                                  (chain16 && !apend) ? 64 * W + 2 : MAXS, gsel, Ul, s0, have);
  if (apend) {
    if (!converged) {
      // keep the junction states for the next round's sweeps (the guess is then this buffer: gsel 1)
      if (gl > 0 && have) {
#pragma unroll
        for (int a = 0; a < X; ++a) traj[(size_t)s0 * X + a] = Ul[a];
      }
      if (gl == 0) {
        *amask = 2;
        if (w.nfallback) atomicAdd(w.nfallback + 15, 1);
      }
      return;
    }
    if (gl == 0) *amask = 1;
  }
  if (!converged && gl == 0) {  // sequential recursion (same arithmetic as fwd_block_impl)
    const double* vbase = q + sy.U + sy.V0 + (size_t)bd.step0 * V;
    const double* nn = q + sy.U + sy.NV;
    ChainConsts<M> cc;
    cc.init(q, sy.dl);
    const double sig = sy.noisy ? sigma_at(sy, q, c) : 0.0;
    double x[X], xn[X];
    if (bd.first) {
      M::gx0(cc.z, q + sy.U, x);
    } else {
#pragma unroll
      for (int a = 0; a < X; ++a) x[a] = xobs[(bd.obs0 - 1) * X + a];
    }
    for (int s = 0; s < L; ++s) {
#pragma unroll
      for (int a = 0; a < X; ++a) traj[(size_t)s * X + a] = x[a];
      M::step(cc.k, x, vbase + (size_t)s * V, xn);
#pragma unroll
      for (int a = 0; a < X; ++a) x[a] = xn[a];
      if ((s + 1) % S == 0) {
        const int j = (s + 1) / S - 1;
        if (j < bd.ny) out[j] = (M::obs(x) + (sy.noisy ? sig * nn[bd.obs0 + j] : 0.0)) - y_of(sy, c)[bd.obs0 + j];
      }
    }
#pragma unroll
    for (int a = 0; a < X; ++a) traj[(size_t)L * X + a] = x[a];
    if (!bd.last) {
#pragma unroll
      for (int a = 0; a < X; ++a) out[bd.ny + a] = x[a] - xobs[(bd.obs0 + bd.nobs - 1) * X + a];
    }
    if (w.nfallback) atomicAdd(w.nfallback, 1);
  }
  if (gl == 0)
    for (int i = bd.nrows; i < RM; ++i) out[i] = 0.0;  // padded constraint slots
}

// Posterior predictive simulation (chmc_predict_device): one wavefront per (chain, group of 64 consecutive replicates), one
// lane per replicate.  The lane runs predict_replicate (chmc_core.h: x, the model constants and the open Philox pair stay in
// registers, the normals are generated in the loop); at every emitted point the wavefront reduces each of the XC channels
// over its lanes -- sum, then the centred squares about the group mean; both by wave_allsum, which leaves the same bits in
// every lane -- and counts y_rep <= level by a ballot per level.  Lanes past n_rep (the partial last group) repeat
// the last replicate so that every lane runs the same trip counts, and enter the sums as zeros and the ballots as false.
// What leaves the wavefront per point is the record [m_g (XC) | s_g (XC) | counts (n_levels)] of (chain, group, point) in
// grp [B][G][NPF][2 XC + n_levels], 64 times less than the raw replicates; KPredictFold<.., grouped> merges the groups in
// order behind it.  The kernel only ever stores: with 256 chains x 64 replicates there is one wavefront on a quarter of
// the SIMDs and nothing hides a load, so a merge into the caller's moments inside the loop (a read-modify-write per point,
// measured: 8 us per emitted point, profiles/predictive_timing.txt) put the memory latency on the recursion's critical path.
// Kept paths (r < n_keep): every lane stores its own XC doubles per point, rows NPF XC doubles apart -- a plotting output
// of a few replicates, not worth a transpose through LDS.
// Sum of v over the 64 lanes, the same bits in every lane.  Inside each row of 16 lanes by rotations through the DPP path
// (row_ror:n = 0x120 + n): after adding the row rotated by 8, 4, 2 and 1 the partial sums have period 8, 4, 2 and 1 in the
// row bit for bit, because both lanes of a pair add the same two numbers (a + b == b + a).  Across the four rows by two xor
// shuffles.  (Six xor shuffles, the form of the Gram kernels, make three times the LDS crossbar trips; with 2 XC sums per
// emitted point and one wavefront on a SIMD that was 0.3 of the 5.5 us a point cost, profiles/predictive_timing.txt.)
__device__ __forceinline__ double wave_allsum(double v) {
  v += dpp_mov<0x128, 0xf, 0xf>(v, 0.0);
  v += dpp_mov<0x124, 0xf, 0xf>(v, 0.0);
  v += dpp_mov<0x122, 0xf, 0xf>(v, 0.0);
  v += dpp_mov<0x121, 0xf, 0xf>(v, 0.0);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
// EVENTS (k_predict_events, chmc_predict_events_device): every lane also keeps the running event accumulator of its replicate
// (EventAcc, chmc_core.h) in the emit callback and stores the replicate's event vector into evraw [B][n_rep][NE] at the end;
// without it the body is the text of k_predict as it was.
template <class M, bool EVENTS>
__device__ __forceinline__ void predict_wave(const Sys& sy, const Slots& sl, const PredictArgs& a, double* grp,
                                             const EventArgs* e, double* evraw) {
  constexpr int X = M::X, XC = X + 2;
  const int lane = threadIdx.x & 63;
  const int G = (a.n_rep + 63) / 64;
  const int c = blockIdx.x / G, g = blockIdx.x - c * G;
  if (c >= sy.B) return;
  if (a.mask && !a.mask[c]) return;
  const int R = a.n_rep - 64 * g < 64 ? a.n_rep - 64 * g : 64;
  const bool act = lane < R;
  const int r = 64 * g + (act ? lane : R - 1);
  const int REC = 2 * XC + a.n_levels;
  const double* q = pick(sl.q, sl.cur[c]) + (size_t)c * sy.Q;
  double* keep = a.paths && act && r < a.n_keep ? a.paths + ((size_t)c * a.n_keep + r) * a.NPF * XC : nullptr;
  double* rec0 = grp + ((size_t)c * G + g) * a.NPF * REC;
  EventAcc acc;
  double vfirst = 0.0, prev = 0.0;
  predict_replicate<M>(sy, a, q, c, r, [&](int p, const double* ch) {
    if constexpr (EVENTS) event_point(*e, acc, p, ch[e->channel], vfirst, prev);
    if (keep) {
#pragma unroll
      for (int i = 0; i < XC; ++i) keep[(size_t)p * XC + i] = ch[i];
    }
    double mg = 0.0, sg = 0.0;  // lane i < XC: the group statistics of channel i
#pragma unroll
    for (int i = 0; i < XC; ++i) {
      const double m = wave_allsum(act ? ch[i] : 0.0) / R;
      const double d = act ? ch[i] - m : 0.0;
      const double s = wave_allsum(d * d);
      if (lane == i) mg = m, sg = s;
    }
    double* rec = rec0 + (size_t)p * REC;
    if (lane < XC) rec[lane] = mg, rec[XC + lane] = sg;
    for (int l = 0; l < a.n_levels; ++l) {
      const int cnt = __popcll(__ballot(act && ch[XC - 1] <= a.levels[l]));
      if (lane == (l & 63)) rec[2 * XC + l] = (double)cnt;
    }
  });
  if constexpr (EVENTS) {
    if (act)
      event_write(*e, evraw + ((size_t)c * a.n_rep + r) * (5 + 3 * e->L), acc.bad != 0, acc.vmax, acc.imax, acc.vmin, acc.imin,
                  acc.sum, vfirst, prev, acc.up, acc.first, acc.above);
  }
}
template <class M>
__global__ void __launch_bounds__(64) k_predict(Sys sy, Slots sl, PredictArgs a, double* grp) {
  predict_wave<M, false>(sy, sl, a, grp, nullptr, nullptr);
}
template <class M>
__global__ void __launch_bounds__(64) k_predict_events(Sys sy, Slots sl, PredictArgs a, double* grp, EventArgs e, double* evraw) {
  predict_wave<M, true>(sy, sl, a, grp, &e, evraw);
}

// Scoring arrived observations (chmc_score_future_device): k_predict's geometry -- a wavefront per (chain, group of 64
// consecutive candidates), a lane per candidate -- without its reductions.  The lane runs predict_replicate at stride S and
// keeps the candidate's FutureAcc (chmc_core.h) in registers; at each of the H emitted points it loads the wave-uniform
// y_future[c][p] (one scalar load per S steps, off the step loop, which stays free of global loads as in k_predict), parks
// n_p in nscr [B][n_cand][H] and, at the end, stores logw.  Lanes past n_cand repeat the last candidate, so that every lane
// runs the same trip counts, and store nothing.  No value crosses lanes: the bits are those of KFutureScore.
template <class M>
__global__ void __launch_bounds__(64) k_future_score(Sys sy, Slots sl, PredictArgs a, FutureArgs f) {
  const int lane = threadIdx.x & 63;
  const int G = (f.n_cand + 63) / 64;
  const int c = blockIdx.x / G, g = blockIdx.x - c * G;
  if (c >= sy.B) return;
  if (a.mask && !a.mask[c]) return;
  const int R = f.n_cand - 64 * g < 64 ? f.n_cand - 64 * g : 64;
  const bool act = lane < R;
  const int r = 64 * g + (act ? lane : R - 1);
  const double* q = pick(sl.q, sl.cur[c]) + (size_t)c * sy.Q;
  const double sig = sigma_at(sy, q, c);
  const double* y = f.y + (size_t)c * f.H;
  double* ns = f.nscr + ((size_t)c * f.n_cand + r) * f.H;
  FutureAcc acc;
  acc.open();
  predict_replicate<M>(sy, a, q, c, r, [&](int p, const double* ch) {
    const double n = acc.add(y[p], ch[M::X], sig);
    if (act) ns[p] = n;
  });
  if (act) f.logw[(size_t)c * f.n_cand + r] = acc.logw(f.H, sig);
}

// Path-wise events of the latent path (chmc_path_events_device): one wavefront per chain over x [B][NP][X].  Lane j takes
// the window's points p0 + j, p0 + j + 64, ... so that a wavefront's loads are consecutive points; the predecessor of each
// point is read by the same lane (a second load of a line its neighbour has just fetched, no shuffle on the path).  Every
// lane opens its accumulator on the window's first point -- a point of the window, so extremes and first passages are
// unaffected and a lane without points needs no special case -- and keeps it out of its sum unless it is lane 0.  The
// lanes are then reduced: (value, index) pairs of the extremes with the smaller index winning a tie, first passages by the
// smallest index, counts by integer sums, the non-finite flag by a ballot, and the trapezoid partial sums by wave_allsum:
// the integral of a chain has one summation order, whatever B is.  Lane 0 writes the NE doubles.
template <class M>
__global__ void __launch_bounds__(64) k_path_events(int B, int NP, EventArgs e, const int* mask, const double* x, double* out) {
  constexpr int X = M::X;
  const int lane = threadIdx.x & 63, c = blockIdx.x;
  if (c >= B) return;
  if (mask && !mask[c]) return;
  const double* xc = x + (size_t)c * NP * X;
  const double vfirst = event_channel<M>(xc + (size_t)e.p0 * X, e.channel);
  const double vlast = event_channel<M>(xc + (size_t)e.p1 * X, e.channel);
  EventAcc a;
  a.open(e, e.p0, vfirst);
  if (lane) a.sum = 0.0;
  for (int p = e.p0 + lane; p <= e.p1; p += 64) {
    if (p == e.p0) continue;
    const double v = event_channel<M>(xc + (size_t)p * X, e.channel);
    const double prev = event_channel<M>(xc + (size_t)(p - 1) * X, e.channel);
    a.add(e, p, v, prev);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const double vx = __shfl_xor(a.vmax, m, 64), vn = __shfl_xor(a.vmin, m, 64);
    const int ix = __shfl_xor(a.imax, m, 64), in = __shfl_xor(a.imin, m, 64);
    if (vx > a.vmax || (vx == a.vmax && ix < a.imax)) a.vmax = vx, a.imax = ix;
    if (vn < a.vmin || (vn == a.vmin && in < a.imin)) a.vmin = vn, a.imin = in;
#pragma unroll
    for (int l = 0; l < kEventLevels; ++l)
      if (l < e.L) {
        a.up[l] += __shfl_xor(a.up[l], m, 64);
        a.above[l] += __shfl_xor(a.above[l], m, 64);
        const int f = __shfl_xor(a.first[l], m, 64);
        if (f >= 0 && (a.first[l] < 0 || f < a.first[l])) a.first[l] = f;
      }
  }
  const bool bad = __ballot(a.bad != 0) != 0ULL;
  const double sum = wave_allsum(a.sum);
  if (lane == 0)
    event_write(e, out + (size_t)c * (5 + 3 * e.L), bad, a.vmax, a.imax, a.vmin, a.imin, sum, vfirst, vlast, a.up, a.first,
                a.above);
}

// The map between time resolutions (chmc_resample_q_device; the arithmetic is chmc_core.h's resample_*).  A workgroup of 256
// lanes takes a tile of one chain; tile 0 also copies u, v_0 and n.
//   refine, m <= 256: a lane per FINE step, so that a wavefront stores consecutive doubles.  A tile is nseg = 256 / m whole
//     coarse steps ("segments" of m lanes; the remaining 256 - nseg m lanes idle), so no segment straddles a workgroup and m
//     need neither divide 64 nor stay below it.  Every lane draws the xi of its step once (a Philox pair per two columns)
//     and parks it in LDS; the segment's first lane forms A xi over the m parked entries in ascending k -- the order of the
//     functor form -- and parks the residual; every lane then adds its row of A^T to the xi it kept in registers.
//   refine, m > 256: a tile is one coarse step, walked in chunks of 256 fine steps.  xi is parked in the destination row
//     itself (each lane reads back what it wrote), lane 0 carries A xi across the chunks.
//   coarsen: a lane per COARSE step sums its m fine steps in ascending k (reads m V doubles, stores V).
template <class M>
__global__ void __launch_bounds__(256) k_resample(ResampleArgs a, int nseg, int ntile) {
  constexpr int V = M::V;
  __shared__ double sx[256 * V];
  __shared__ double sr[256 * V];
  const int tid = threadIdx.x, m = a.m;
  const int c = blockIdx.x / ntile, tile = blockIdx.x - c * ntile;
  if (c >= a.B) return;
  if (a.mask && !a.mask[c]) return;  // uniform per workgroup
  const double* src = a.src + (size_t)c * (size_t)a.Qs;
  double* dst = a.dst + (size_t)c * (size_t)a.Qd;
  const int NS = a.T * a.Sc, head = a.U + a.V0;
  if (tile == 0) resample_copy_ends(a, src, dst, tid, 256);
  if (!a.refine) {
    const int s = tile * 256 + tid;
    if (s >= NS) return;
    ResampleSum<M> ax;
    ax.open();
    const double* w = src + head + (size_t)s * m * V;
    for (int k = 0; k < m; ++k) ax.add(m, k, w + (size_t)k * V);
    ax.close(m);
#pragma unroll
    for (int i = 0; i < V; ++i) dst[head + (size_t)s * V + i] = ax.s[i];
    return;
  }
  NormalCursor cur;
  cur.open(a.seed, a.key, (uint32_t)(a.chain_offset + c));
  double x[V], r[V];
  if (m <= 256) {
    const int seg = tid / m, k = tid - seg * m;
    const int s = tile * nseg + seg;
    const bool on = seg < nseg && s < NS;
    const uint32_t col = (uint32_t)head + ((uint32_t)s * (uint32_t)m + (uint32_t)k) * (uint32_t)V;
    if (on) {
      resample_xi<M>(cur, col, x);
#pragma unroll
      for (int i = 0; i < V; ++i) sx[tid * V + i] = x[i];
    }
    __syncthreads();
    if (on && k == 0) {
      ResampleSum<M> ax;
      ax.open();
      for (int kk = 0; kk < m; ++kk) ax.add(m, kk, sx + (tid + kk) * V);
      resample_residual<M>(m, src + head + (size_t)s * V, ax, r);
#pragma unroll
      for (int i = 0; i < V; ++i) sr[seg * V + i] = r[i];
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int i = 0; i < V; ++i) r[i] = sr[seg * V + i];
      resample_spread<M>(m, k, r, x);
#pragma unroll
      for (int i = 0; i < V; ++i) dst[col + i] = x[i];
    }
    return;
  }
  const int s = tile;  // (nseg == 1, ntile == NS)
  const uint32_t col0 = (uint32_t)head + (uint32_t)s * (uint32_t)m * (uint32_t)V;
  ResampleSum<M> ax;
  ax.open();
  for (int k0 = 0; k0 < m; k0 += 256) {
    const int k = k0 + tid;
    if (k < m) {
      resample_xi<M>(cur, col0 + (uint32_t)k * V, x);
#pragma unroll
      for (int i = 0; i < V; ++i) sx[tid * V + i] = x[i], dst[col0 + (size_t)k * V + i] = x[i];
    }
    __syncthreads();
    if (tid == 0) {
      const int n = m - k0 < 256 ? m - k0 : 256;
      for (int kk = 0; kk < n; ++kk) ax.add(m, k0 + kk, sx + kk * V);
    }
    __syncthreads();
  }
  if (tid == 0) {
    resample_residual<M>(m, src + head + (size_t)s * V, ax, r);
#pragma unroll
    for (int i = 0; i < V; ++i) sr[i] = r[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < V; ++i) r[i] = sr[i];
  for (int k = tid; k < m; k += 256) {
#pragma unroll
    for (int i = 0; i < V; ++i) x[i] = dst[col0 + (size_t)k * V + i];
    resample_spread<M>(m, k, r, x);
#pragma unroll
    for (int i = 0; i < V; ++i) dst[col0 + (size_t)k * V + i] = x[i];
  }
}

// (An LDS-staged variant of the forward scan -- 8 lanes fetching one block's 128-byte tile, tiles parked in LDS with a
// 144-byte row stride, trajectory tiles written back the same way -- was built and measured at 2x the time of the
// plain lane-per-block scan of chmc_core.h: with one wavefront per SIMD the extra LDS round trips sit on the
// critical path of the sequential recursion.  It was removed.)

// (A blocked variant of k_rev_wave -- every lane owning 4 consecutive steps, composing their transition matrices
// locally so that only lane aggregates go through the shuffle scan, and multiplying the carried rows into per-lane
// sums once per 256-step tile -- was built, passed the parity suite and cut vector instructions per block by 28 %
// (SQ_INSTS_VALU 14.4 k vs 20 k per wavefront at N4).  It still ran 10-25 % slower (newton_blk 3.55 vs 3.21 ms per
// step, state_blk 0.54 vs 0.43): at 256 VGPR + 248 AGPR it has no registers left for the two-stage prefetch of
// k_rev_wave, so with one wavefront per SIMD the 64-byte-strided loads sit exposed (SQ_WAIT_INST_ANY > busy
// cycles).  It was removed.)

}  // namespace chmc
