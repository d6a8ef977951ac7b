// The pass layer: which kernel runs a pass of chmc_api.inc's sequencing for the context's plan (chmc_plan.h).  Included by
// chmc_api.inc once chmc_ctx, dispatch() / Inst and part_plan() are defined.  One function per pass; it takes the context and
// the selectors the kernels take, switches on the plan and returns what the sequencing needs to know afterwards.  Passes that
// are the same functors in both builds come first; the others are written twice under the ONE #ifdef of the sequencing: over
// the wave kernels of chmc_wave.h / chmc_retract.h (the library) and over the generic functors of chmc_core.h (the host
// emulation of tests/emu/, whose plan -- PlanInput::wave_kernels = false -- selects the stored rows and no per-chain layout).

// The per-chain kernels (k_retract_chain, k_traj_chain; retract_waves / traj_waves in chmc_api.inc) are instantiated for the SIR
// models only: they are sized to SIR's 75 KB of LDS.  A FitzHugh-Nagumo layout with one 16-row block per chain (T <= 14) always
// runs the batched path of the same plan, so CHMC_RETRACT_KERNEL=1/2 changes nothing there.
// The gate is written twice and the two must agree: chain_kernel_model (run time, on chmc_config::model) decides whether a
// call takes the per-chain path, kChainKernels (compile time, on the model type `dispatch` selects for that id) decides
// which instantiations exist.  `dispatch` maps CHMC_MODEL_SIR to SirModel / SirVsModel and nothing else to them, and both
// carry SirModel::ID -- held below, so a model id that drifts from its type's ID does not compile rather than launching nothing.
static_assert(SirModel::ID == CHMC_MODEL_SIR && SirVsModel::ID == CHMC_MODEL_SIR && FhnModel::ID == CHMC_MODEL_FHN &&
                  FhnVsModel::ID == CHMC_MODEL_FHN && FhnNbModel::ID == CHMC_MODEL_FHN_NOTEBOOK,
              "chain_kernel_model and kChainKernels gate the per-chain kernels on the same models");
static bool chain_kernel_model(const chmc_ctx* c) { return c->model == CHMC_MODEL_SIR; }
template <class M, int RM>
constexpr bool kChainKernels = RM == 16 && M::ID == CHMC_MODEL_SIR;

// J^T lambda column pass over the stored rows: two columns per work item with 16-byte accesses when every offset is even
template <int RM, int TGT>
static void update(const Sys& sy, const Slots& sl, const Work& w, int which, int qsel, int psel) {
  if (sy.Q % 2 == 0 && sy.NV % 2 == 0 && sy.U % 2 == 0 && sy.V0 % 2 == 0 && sy.V % 2 == 0 && sy.NCOL % 2 == 0)
    launch_colmax(KUpdate<RM, TGT, 2>{sy, sl, w, which, qsel, psel}, sy.NCOL / 2, sy.B, 4);
  else
    launch_colmax(KUpdate<RM, TGT, 1>{sy, sl, w, which, qsel, psel}, sy.NCOL, sy.B, 4);
}
// J^T lambda update by the row family (KernelPlan::rows): `update` over the stored rows, or
// J^T lambda from the compact rows: mu_F (KMuF), then the column pass (KUpdatePB), one step per work item; a full launch
// moves 0.66 GB in 125 us = 5.2 TB/s, the streaming rate of this part.
// have_mu_f: the Newton sweep has formed mu_F
// (flow_rev, fwd_qb, fwd_hfrac: KUpdatePB's members of those names, with its defaults)
template <class M, int RM, int TGT>
static void jt_lambda(chmc_ctx* c, int which, int qsel, int psel, bool have_mu_f = false, int flow_rev = 0,
                      double* fwd_qb = nullptr, double fwd_hfrac = 0.0) {
  const Sys& sy = c->sy;
  if (c->plan.rows != RowsCompact) return update<RM, TGT>(sy, c->sl, c->w, which, qsel, psel);
  if (!have_mu_f) launch(KMuF<RM, M::X, TGT>{sy, c->sl, c->w, which}, (long)sy.B * sy.K * sy.NOBS * M::X, 5);
  launch_colmax(KUpdatePB<RM, M::X, M::V, TGT>{sy, c->sl, c->w, which, qsel, psel, flow_rev, fwd_qb, fwd_hfrac},
                sy.T * sy.S + sy.V0 + (sy.noisy ? sy.T : 0), sy.B, 4);
}

// the latent path by the plain recursion, one work item per chain (KPath): of the caller's positions `q`, or of the current
// states (null) where no time-parallel pass is available; it reports no sweeps (0)
template <class M>
static void path_seq(chmc_ctx* c, const double* q, int stride, double* out, int* sweeps) {
  if (sweeps) dev_zero(sweeps, sizeof(int) * c->sy.B);
  launch(KPath<M>{c->sy, c->sl, q, stride, out}, c->sy.B, 7), c->diag[11]++;
}

// chmc_predict_device: the library's scratch for the replicates' channels or group statistics, grown on demand
static double* predict_scratch(chmc_ctx* c, size_t n) {
  if (c->d_pred_cap < n) c->d_pred = alloc<double>(c, n), c->d_pred_cap = n;
  return c->d_pred;
}
// the moments' second pass (KPredictFold): the replicates are counted, then every (chain, point) merges the call's groups
template <class M>
static void predict_fold(chmc_ctx* c, const PredictArgs& a, int grouped, const double* src, long long* n, double* mean, double* m2,
                         long long* cdf) {
  KPredictFold<M> f{a.NPF, a.n_rep, a.n_levels, 0, grouped, a.mask, a.levels, src, n, mean, m2, cdf};
  launch(f, c->sy.B, 8);
  f.phase = 1;
  launch(f, (long)c->sy.B * a.NPF, 8);
}
// the predictive by the generic functors: a work item per (chain, replicate) writes the raw channels, the fold sums them in
// replicate order.  e (null: chmc_predict_device): the replicates' event vectors go to evraw as well
template <class M>
static void predict_seq(chmc_ctx* c, const PredictArgs& a, const EventArgs* e, double* evraw, long long* n, double* mean,
                        double* m2, long long* cdf) {
  double* raw = predict_scratch(c, (size_t)c->sy.B * a.n_rep * a.NPF * (M::X + 2));
  const long tasks = (long)c->sy.B * a.n_rep;
  if (e)
    launch(KPredict<M, true>{c->sy, c->sl, a, raw, *e, evraw}, tasks, 7);
  else
    launch(KPredict<M, false>{c->sy, c->sl, a, raw, {}, nullptr}, tasks, 7);
  c->diag[13]++;
  predict_fold<M>(c, a, 0, raw, n, mean, m2, cdf);
}
// the events' fold of both forms (KEventFold)
static void event_fold(chmc_ctx* c, const PredictArgs& a, const EventArgs& e, const double* evraw, long long* en, double* emean,
                       double* em2) {
  const int NE = 5 + 3 * e.L;
  launch(KEventFold{NE, a.n_rep, a.mask, evraw, en, emean, em2}, (long)c->sy.B * NE, 8);
}
// the latent-path events by the generic functor: one work item per chain
template <class M>
static void path_events_seq(chmc_ctx* c, int NP, const EventArgs& e, const int* mask, const double* x, double* out) {
  launch(KPathEvents<M>{NP, e, mask, x, out}, c->sy.B, 7), c->diag[15]++;
}
// chmc_score_future_device by the generic functor: a work item per (chain, candidate); counted with the predictive's
// functor form (every diagnostics slot is taken)
template <class M>
static void future_seq(chmc_ctx* c, const PredictArgs& a, const FutureArgs& f) {
  launch(KFutureScore<M>{c->sy, c->sl, a, f}, (long)c->sy.B * f.n_cand, 7), c->diag[13]++;
}
// score, pick and tail of both forms: a work item per chain (KFuturePick), then the picked candidates' normals, a work item
// per (chain, component pair) (KFutureTail)
static void future_pick(chmc_ctx* c, const PredictArgs& a, const FutureArgs& f, unsigned long long key, double* log_pred,
                        int* picked, double* tail) {
  const long long nv = (long long)a.HS * c->sy.V, ld = nv + f.H;
  launch(KFuturePick{f, a.seed, key, a.chain_offset, a.mask, log_pred, picked, tail, ld, nv}, c->sy.B, 8);
  if (tail) launch(KFutureTail{a.seed, a.key0, a.chain_offset, a.mask, picked, nv, ld, tail}, (long)(c->sy.B * ((nv + 1) / 2)), 8);
}
// the map between time resolutions by the generic functor: one work item per (chain, coarse step)
template <class M>
static void resample_seq(chmc_ctx* c, const ResampleArgs& a) {
  (void)c;
  launch(KResample<M>{a}, (long)a.B * a.T * a.Sc, 8);
}
// chmc_set_state_project_device: the observed coordinate of the scanned x_obs_seq `xs` pinned to the data, a work item per
// (chain, observation), then the chains' defects and the mask without the chains that could not be pinned.  Once per rung
// and a handful of flops per work item: the functor form in both builds.  `scr`: [B][T] dobs, [B][T] pok, [B] defect, [B] pinfail
template <class M>
static void pin_obs(chmc_ctx* c, int* act, const double* xs, double* scr) {
  const Sys& sy = c->sy;
  const size_t bt = (size_t)sy.B * sy.T;
  launch(KPinObs<M>{sy, act, xs, c->d_xobs, scr, scr + bt}, (long)bt, 8);
  launch(KPinChain{sy.T, act, scr, scr + bt, scr + 2 * bt, scr + 2 * bt + sy.B}, sy.B);
}

#ifdef CHMC_WAVE_KERNELS
constexpr bool kWaveKernels = true;  // PlanInput::wave_kernels of every context of this build
// chmc_predict_device: a wavefront per (chain, group of 64 replicates) where the library keeps the compact rows (the
// default; path_scan's rule) leaves the groups' statistics to the fold; CHMC_COMPACT_ROWS=0 runs the functor form, the A/B
// partner.  e (chmc_predict_events_device; null: none): the EVENTS instantiation of the wave kernel, by the same rule
template <class M>
static void predict_pass(chmc_ctx* c, const PredictArgs& a, const EventArgs* e, double* evraw, long long* n, double* mean,
                         double* m2, long long* cdf) {
  if (!c->plan.pb_allocated) return predict_seq<M>(c, a, e, evraw, n, mean, m2, cdf);
  const int G = (a.n_rep + 63) / 64;
  double* grp = predict_scratch(c, (size_t)c->sy.B * G * a.NPF * (2 * (M::X + 2) + a.n_levels));
  if (e)
    launch_blocks(k_predict_events<M>, (long)c->sy.B * G, 64, 7, c->sy, c->sl, a, grp, *e, evraw);
  else
    launch_blocks(k_predict<M>, (long)c->sy.B * G, 64, 7, c->sy, c->sl, a, grp);
  c->diag[12]++;
  predict_fold<M>(c, a, 1, grp, n, mean, m2, cdf);
}
// chmc_score_future_device: the functor form unless CHMC_FUTURE_WAVE=1 asks for the wave kernel -- a wavefront per (chain,
// group of 64 candidates), counted with the predictive wave kernel -- where predict_pass's rule allows it (the compact rows
// are allocated; KernelPlan::future_wave).  Bitwise equal; the functor form was the faster one at every measured shape
// (profiles/future_score_timing.txt), so it is the default
template <class M>
static void future_pass(chmc_ctx* c, const PredictArgs& a, const FutureArgs& f) {
  if (!c->plan.future_wave) return future_seq<M>(c, a, f);
  launch_blocks(k_future_score<M>, (long)c->sy.B * ((f.n_cand + 63) / 64), 64, 7, c->sy, c->sl, a, f), c->diag[12]++;
}
// chmc_path_events_device: a wavefront per chain where the library keeps the compact rows (path_scan's rule), the functor
// form under CHMC_COMPACT_ROWS=0
template <class M>
static void path_events_pass(chmc_ctx* c, int NP, const EventArgs& e, const int* mask, const double* x, double* out) {
  if (!c->plan.pb_allocated) return path_events_seq<M>(c, NP, e, mask, x, out);
  launch_blocks(k_path_events<M>, (long)c->sy.B, 64, 7, c->sy.B, NP, e, mask, x, out), c->diag[14]++;
}
// chmc_resample_q_device: workgroups of 256 lanes over tiles of a chain where the library keeps the compact rows
// (path_scan's rule), the functor form under CHMC_COMPACT_ROWS=0.  A tile: 256 coarse steps (coarsening), 256 / m whole
// coarse steps (refinement by m <= 256: a lane per fine step), one coarse step (m > 256)
template <class M>
static void resample_pass(chmc_ctx* c, const ResampleArgs& a) {
  if (!c->plan.pb_allocated) return resample_seq<M>(c, a);
  const long NS = (long)a.T * a.Sc;
  const int nseg = !a.refine ? 256 : a.m <= 256 ? 256 / a.m : 1;
  const long ntile = (NS + nseg - 1) / nseg;
  launch_blocks(k_resample<M>, (long)a.B * ntile, 256, 8, a, nseg, (int)ntile);
}
// chain-level Woodbury solve: one wavefront per chain up to 64 blocks
template <class M, int RM, int SYM, int TGT>
static void solve_chain(const Sys& sy, const Slots& sl, const Work& w, int which, int qsel, int psel) {
  if (sy.K <= 64)
    launch_wave(k_solve_chain_wave<M, RM, SYM, TGT>, (long)sy.B, 5, sy, sl, w, which, qsel, psel);
  else
    launch(KSolveChain<M, RM, SYM, TGT>{sy, sl, w, which, qsel, psel}, sy.B, 5);
}

// time-parallel forward scan (k_fwd_par) on `waves` wavefronts per workgroup (par_waves_for / CHMC_CHAIN_SCAN_WAVES: 1, 2 or 4)
template <class M, int RM, class... Args>
static void fwd_par(int waves, long n, Args... args) {
  if (waves == 4)
    launch_blocks(k_fwd_par<M, RM, 4>, n, 256, 7, args...);
  else if (waves == 2)
    launch_blocks(k_fwd_par<M, RM, 2>, n, 128, 7, args...);
  else
    launch_blocks(k_fwd_par<M, RM, 1>, n, 64, 7, args...);
}
// forward scan (KernelPlan::fwd); gsel: guess trajectory for the time-parallel scan (k_fwd_par; 0: none available ->
// sequential scan, KernelPlan::fwd_cold).  Returns the number of scan launches.
// (Measured and rejected for the sequential scan, round 3: giving every scan workgroup a CU of its own with 56 KB of dynamic
// LDS padding -- 512 chains, S = 800: 439 against 392 us per scan.  The scan's time doubles from 80 to 160 wavefronts because
// it is then bound by the memory system, not by two wavefronts sharing a SIMD: 10 240 lanes x 32 B per step in 128-byte lines
// that belong to 64 different streams per wave instruction = 2.8-3.3 TB/s, DESIGN.md section 4.)
template <class M, int RM>
static int fwd(chmc_ctx* c, int which, int qsel, int use_nw, int store, int gsel) {
  const Sys& sy = c->sy;
  stagger_wait();  // half-batches: this half's scan runs after the other half's latest one
  const FwdScan scan = gsel != 0 ? c->plan.fwd : c->plan.fwd_cold;
  if (scan == FwdPar) {
    // few long blocks: Newton on the trajectory, one wavefront per (chain, block); a scan that stores nothing
    // (quasi-Newton) iterates on the work trajectory
    fwd_par<M, RM>(c->plan.fwd_waves, (long)sy.B * sy.K, sy, c->sl, c->w, which, qsel, use_nw, store ? store : 2, gsel, c->round);
  } else if (scan == FwdWave) {
    if (store)
      launch_blocks(k_fwd_scan<M, RM, true>, ((long)sy.B * sy.K + 63) / 64, 64 * (1 + CHMC_SCAN_HELPERS), 7, sy, c->sl, c->w, which,
                    qsel, use_nw, store, c->w, 0, 0);
    else
      launch_blocks(k_fwd_scan<M, RM, false>, ((long)sy.B * sy.K + 63) / 64, 64, 7, sy, c->sl, c->w, which, qsel, use_nw, store,
                    c->w, 0, 0);
  } else {
    launch(KFwd<M, RM>{sy, c->sl, c->w, which, qsel, use_nw, store}, (long)sy.B * sy.K, 7);
  }
  stagger_record();
  return 1;
}
// ... of the chains in the Newton loops of two problems, c->w and w1, with the same (which, qsel): ONE launch of twice the
// workgroups (the lock-step round path never scans in parallel in time: KernelPlan::pair_retractions)
template <class M, int RM>
static int fwd_pair(chmc_ctx* c, const Work& w1, int which, int qsel, int store) {
  const Sys& sy = c->sy;
  if (c->plan.fwd_cold == FwdWave) {
    const long wg = ((long)sy.B * sy.K + 63) / 64;
    if (store)
      launch_blocks(k_fwd_scan<M, RM, true, true>, 2 * wg, 64 * (1 + CHMC_SCAN_HELPERS), 7, sy, c->sl, c->w, which, qsel, 1, store,
                    w1, which, qsel);
    else
      launch_blocks(k_fwd_scan<M, RM, false, true>, 2 * wg, 64, 7, sy, c->sl, c->w, which, qsel, 1, store, w1, which, qsel);
    return 1;
  }
  launch(KFwd<M, RM>{sy, c->sl, c->w, which, qsel, 1, store}, (long)sy.B * sy.K, 7);
  launch(KFwd<M, RM>{sy, c->sl, w1, which, qsel, 1, store}, (long)sy.B * sy.K, 7);
  return 2;
}

// state sweep of slot `which` behind its forward scan (PartitionPlan::state): Jacobian sweep, Gram blocks, block factors
template <class M, int RM>
static void state_sweep(chmc_ctx* c, int which) {
  const Sys& sy = c->sy;
  const StateSweep state = part_plan(c).state;
  const long nbk = (long)sy.B * sy.K;
  if constexpr (RM > 8) {
    switch (state) {
      case StateIvlComb:  // few long 16-row blocks: interval-parallel sums, then one combine per block (compact rows only)
        launch_blocks(k_newton_ivl<M, true>, nbk * sy.NOBS, 64, 2, sy, c->sl, c->w, which, 0);
        launch_blocks(k_newton_comb<M, RM, true>, nbk, 64, 2, sy, c->sl, c->w, which, 0);
        break;
      case StateIvlCombWg:  // one block per chain: the per-chain kernels' combine (all threads) + 16-lane Cholesky, E, C_b
        launch_blocks(k_newton_ivl<M, true>, nbk * sy.NOBS, 64, 2, sy, c->sl, c->w, which, 0);
        launch_blocks(k_newton_comb_wg<M, RM, CHMC_RETRACT_WAVES, true>, (long)sy.B, 64 * CHMC_RETRACT_WAVES, 2, sy, c->sl,
                      c->w, which, 0);
        break;
      case StateLdsrowsGramMfma:  // store the rows, then the Gram block from the stored rows
        launch_blocks(k_rev_wave_ldsrows<M, RM, 0>, nbk, 64, 2, sy, c->sl, c->w, which, 0);
        launch_blocks(k_gram_rows_mfma<RM>, nbk, 64, 2, sy, c->sl, c->w, which, 0, 0), c->diag[0]++;
        break;
      default:  // StateLdsrowsGram
        launch_blocks(k_rev_wave_ldsrows<M, RM, 0>, nbk, 64, 2, sy, c->sl, c->w, which, 0);
        launch_wave(k_gram_rows<RM, 4>, nbk * (RM / 4), 2, sy, c->sl, c->w, which, 0, 0), c->diag[1]++;
    }
  } else {
    switch (state) {
      case StateLean:  // the state sweep at three wavefronts per SIMD (compact rows)
        launch_blocks(k_state_lean<M, RM>, nbk, 64, 2, sy, c->sl, c->w, which);
        break;
      case StateRevStoreGramMfma:  // store the rows, then the Gram block from the stored rows on the matrix cores
        launch_wave(k_rev_wave<M, RM, 0, false>, nbk, 2, sy, c->sl, c->w, which, 0);
        launch_blocks(k_gram_rows_mfma<RM>, nbk, 64, 2, sy, c->sl, c->w, which, 0, 0), c->diag[0]++;
        break;
      default:  // StateRevWave
        launch_wave(k_rev_wave<M, RM, 0>, nbk, 2, sy, c->sl, c->w, which, 0);
    }
  }
  if (state != StateIvlCombWg)  // (k_newton_comb_wg<.., STATE> has factored the block)
    launch(KStateFactor<M, RM>{sy, c->sl, c->w, which}, nbk, 9);
}
// grad-log-det sweeps of slot `which` (PartitionPlan::gld), between KStateChain and KGldChain
template <class M, int RM>
static void gld_sweeps(chmc_ctx* c, int which) {
  const Sys& sy = c->sy;
  const long nbk = (long)sy.B * sy.K;
  if constexpr (RM > 8)  // 16-row blocks: the block over 16 lanes (a 16 x 16 inverse per lane lives in scratch memory)
    launch_blocks(k_gld_prep_wave<M, RM>, ((long)sy.B * sy.K + 3) / 4, 64, 9, sy, c->sl, c->w, which);
  else
    launch(KGldPrep<M, RM>{sy, c->sl, c->w, which}, (long)sy.B * sy.K, 9);
  switch (part_plan(c).gld) {
    case GldQxLean:  // blocks of at most 8 rows: row-free backward sweep on Qx written by the forward sweep
      if constexpr (RM <= 8) {
        // forward sweep on X pseudo-rows (Qx directly; the row tangents only at the interval boundaries, from the state
        // sweep's interval sums in work.ivl)
        launch_wave(k_gld_fwd_qx<M, RM>, nbk, 3, sy, c->sl, c->w, which);
        launch_blocks(k_gld_bwd_lean<M, RM>, nbk, 64, 3, sy, c->sl, c->w, which);
      }
      break;
    case GldIvl:  // few long 16-row blocks: the row-free sweeps, every observation interval on its own wavefront
      if constexpr (RM > 8) {
        const long niv = nbk * sy.NOBS;
        launch_wave(k_gld_ivl_prologue<M, RM>, nbk, 3, sy, c->sl, c->w, which);
        launch_wave(k_gld_fwd_ivl<M, RM>, niv, 3, sy, c->sl, c->w, which);
        launch_wave(k_gld_bwd_ivl<M, RM, 0>, niv, 3, sy, c->sl, c->w, which);
        launch_wave(k_gld_bwd_ivl<M, RM, 1>, niv, 3, sy, c->sl, c->w, which);
        launch_blocks(k_gld_ivl_finish<M, RM>, (nbk + 63) / 64, 64, 3, sy, c->sl, c->w, which);
      }
      break;
    case GldCompactFwdStored:  // 16-row blocks, large batches: the weights from the compact rows (DPP affine scan)
      if constexpr (RM > 8) {
        launch_wave(k_gld_fwd_wave<M, RM, true>, nbk, 3, sy, c->sl, c->w, which);
        launch_wave(k_gld_bwd_wave_ldsrows<M, RM>, nbk, 3, sy, c->sl, c->w, which);
      }
      break;
    case GldStored:
      launch_wave(k_gld_fwd_wave<M, RM>, nbk, 3, sy, c->sl, c->w, which);
      if constexpr (RM > 8) {
        launch_wave(k_gld_bwd_wave_ldsrows<M, RM>, nbk, 3, sy, c->sl, c->w, which);
      } else {
        launch_wave(k_gld_bwd_wave<M, RM>, nbk, 3, sy, c->sl, c->w, which);
      }
      break;
  }
}

// Newton sweep of the iterate against the rows of slot `prev` (PartitionPlan::newton), with the block factorisations.
// Returns `solved`: the sweep went on to solve the chain's core system and to form lambda and mu_F.
template <class M, int RM>
static bool newton_sweep(chmc_ctx* c, int prev, int qsel) {
  const Sys& sy = c->sy;
  const NewtonSweep sweep = part_plan(c).newton;
  // (these sweeps go on to factor the blocks, solve the chain's core system and form lambda and mu_F)
  const bool solved = sweep == NewtonIvlFsm || sweep == Newton16IvlCombFactor || sweep == Newton16IvlCombWg;
  const long nbk = (long)sy.B * sy.K;
  if constexpr (RM > 8) {
    switch (sweep) {
      // two-phase sweep on the compact rows: interval-parallel sums, then one combine per block
      case Newton16IvlCombWg:  // (the per-chain kernels' combine + LU on 16 lanes: the same bits as k_retract_chain)
        launch_blocks(k_newton_ivl<M>, nbk * sy.NOBS, 64, 1, sy, c->sl, c->w, prev, qsel);
        launch_blocks(k_newton_comb_wg<M, RM, CHMC_RETRACT_WAVES, false>, (long)sy.B, 64 * CHMC_RETRACT_WAVES, 1, sy,
                      c->sl, c->w, prev, qsel);
        break;
      case Newton16IvlCombFactor:  // one block per chain (the SIR single-block layout)
        launch_blocks(k_newton_ivl<M>, nbk * sy.NOBS, 64, 1, sy, c->sl, c->w, prev, qsel);
        launch_blocks(k_newton_comb<M, RM, false, true>, nbk, 64, 1, sy, c->sl, c->w, prev, qsel);
        break;
      case Newton16IvlComb:
        launch_blocks(k_newton_ivl<M>, nbk * sy.NOBS, 64, 1, sy, c->sl, c->w, prev, qsel);
        launch_blocks(k_newton_comb<M, RM>, nbk, 64, 1, sy, c->sl, c->w, prev, qsel);
        break;
      case Newton16LdsrowsGramMfma:
        launch_blocks(k_rev_wave_ldsrows<M, RM, 1>, nbk, 64, 1, sy, c->sl, c->w, prev, qsel);
        launch_blocks(k_gram_rows_mfma<RM>, nbk, 64, 1, sy, c->sl, c->w, prev, 1, qsel), c->diag[0]++;
        break;
      default:  // Newton16LdsrowsGram
        launch_blocks(k_rev_wave_ldsrows<M, RM, 1>, nbk, 64, 1, sy, c->sl, c->w, prev, qsel);
        launch_wave(k_gram_rows<RM, 4>, nbk * (RM / 4), 1, sy, c->sl, c->w, prev, 1, qsel), c->diag[1]++;
    }
    // rows over 16 lanes (a 16 x 16 matrix per lane lives in scratch memory)
    if (!solved) launch_blocks(k_newton_factor_wave<M, RM>, (nbk + 3) / 4, 64, 9, sy, c->sl, c->w, prev, qsel);
  } else {
    switch (sweep) {
      // two phases (interval-parallel sums + per-block combine): 25 600 seven-tile wavefronts balance better over the
      // SIMDs than 5 120 thirty-five-tile ones and the hot loop has no per-interval flush
      case NewtonIvlFsm:
      case NewtonIvlComb:
        launch_blocks(k_newton_ivl<M>, nbk * sy.NOBS, 64, 1, sy, c->sl, c->w, prev, qsel);
        launch_blocks(k_newton_comb<M, RM>, nbk, 64, 1, sy, c->sl, c->w, prev, qsel);
        break;
      case NewtonRevStoreGramMfma:  // the iterate's rows into work.JvW, Gram block against the stored rows by MFMA
        launch_wave(k_rev_wave<M, RM, 1, false>, nbk, 1, sy, c->sl, c->w, prev, qsel);
        launch_blocks(k_gram_rows_mfma<RM>, nbk, 64, 1, sy, c->sl, c->w, prev, 1, qsel), c->diag[0]++;
        break;
      default:  // NewtonRevWave
        launch_wave(k_rev_wave<M, RM, 1>, nbk, 1, sy, c->sl, c->w, prev, qsel);
    }
    if (solved)  // block LU, Woodbury solve, u-columns and mu_F in one launch (wave per chain)
      launch_blocks(k_newton_fsm_wave<M, RM>, (long)sy.B, 64, 5, sy, c->sl, c->w, prev, qsel), c->diag[4]++;
    else
      launch(KNewtonFactor<M, RM>{sy, c->sl, c->w, prev}, nbk, 9), c->diag[5]++;
  }
  return solved;
}
// ... and J^T lambda update of the iterates of two problems, c->w and w1, against the rows of the same slot `prev`
// (KernelPlan::pair_passes: compact rows, at most 8 row slots, NewtonIvlFsm -- the sweep has solved and formed mu_F): one
// launch per pass for both.  Interval sums: a workgroup of two wavefronts per interval, one per problem, on the same PB
// lines; combine and solve: both problems' wavefronts in one grid; update: one work item per step loads PB once for both
// iterates (96 instead of 128 bytes per step and pair).
template <class M, int RM>
static void newton_sweep_pair(chmc_ctx* c, const Work& w1, int prev, int qsel) {
  const Sys& sy = c->sy;
  const long nbk = (long)sy.B * sy.K;
  if constexpr (RM <= 8) {
    launch_blocks(k_newton_ivl_pair<M>, nbk * sy.NOBS, 128, 1, sy, c->sl, c->w, prev, qsel, w1);
    launch_blocks(k_newton_comb_pair<M, RM>, 2 * nbk, 64, 1, sy, c->sl, c->w, prev, qsel, w1);
    launch_blocks(k_newton_fsm_wave_pair<M, RM>, 2 * (long)sy.B, 64, 5, sy, c->sl, c->w, prev, qsel, w1), c->diag[4]++;
  }
}
template <class M, int RM>
static void jt_lambda_pair(chmc_ctx* c, const Work& w1, int prev, int qsel) {
  const Sys& sy = c->sy;
  if constexpr (RM <= 8)
    launch_colmax_pair(KUpdatePBPair<RM, M::X, M::V>{sy, c->sl, c->w, w1, prev, qsel}, sy.T * sy.S + sy.V0 + (sy.noisy ? sy.T : 0),
                       sy.B, 4);
}

// J v -> cpad for the vector `vsel` selects, from the compact rows or from the stored rows of slot `which`
template <class M, int RM>
static void jw(chmc_ctx* c, int which, int vsel, bool compact) {
  const Sys& sy = c->sy;
  if (compact)
    launch_wave(k_jw_pb<RM, M::X, M::V>, (long)sy.B * sy.K, 6, sy, c->sl, c->w, which, vsel);
  else
    launch_wave(k_jw_wave<RM>, (long)sy.B * sy.K, 6, sy, c->sl, c->w, which, vsel);  // J M^-1 p
}
// P(q) applied to the slot's momentum and to pg in one pass over the Jacobian rows (project_momentum_and_kick_direction)
static void project_pair(chmc_ctx* c, int which, bool fix_in_jw, bool flow_rev, double* fwd_qb, double fwd_hfrac) {
  const Sys& sy = c->sy;
  dispatch(c, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    // J p -> cpad, J pg -> cpad2 from one read of the compact rows (16-row blocks: PB / LF are written beside the stored
    // rows; 9 instead of 48 doubles per step) or of the stored rows
    switch (part_plan(c).jp) {
      case JpPbWg:  // one block per chain: the interval sums over the wavefronts of a workgroup (k_traj_chain's form)
        if constexpr (RM > 8)
          launch_blocks(k_jw_pb_wg<RM, M::X, M::V, CHMC_RETRACT_WAVES>, (long)sy.B, 64 * CHMC_RETRACT_WAVES, 6, sy, c->sl, c->w,
                        which);
        break;
      case JpPb:
        if constexpr (RM <= 8 && M::V == 2) {
          if (fix_in_jw) {
            launch_wave(k_jw_pb<RM, M::X, M::V, true, true>, (long)sy.B * sy.K, 6, sy, c->sl, c->w, which, 256);
            break;
          }
        }
        launch_wave(k_jw_pb<RM, M::X, M::V, true>, (long)sy.B * sy.K, 6, sy, c->sl, c->w, which, 256);
        break;
      case JpWave:
        launch_wave(k_jw_wave<RM, true>, (long)sy.B * sy.K, 6, sy, c->sl, c->w, which, 256);
        break;
    }
    // two Woodbury solves on views of the work arrays instead of copies between them: the first writes the multipliers of
    // p straight into lampad2, the second takes J pg from cpad2
    Work w1 = c->w, w2 = c->w;
    w1.lampad = c->w.lampad2;
    w2.cpad = c->w.cpad2;
    launch(KSymBlk<M, RM>{sy, c->sl, w1, which, 0}, (long)sy.B * sy.K, 9);
    solve_chain<M, RM, 1, 1>(sy, c->sl, w1, which, 0, 0);  // multipliers of p (and its u columns) -> lampad2
    launch(KSymBlk<M, RM>{sy, c->sl, w2, which, 0}, (long)sy.B * sy.K, 9);
    solve_chain<M, RM, 1, 1>(sy, c->sl, w2, which, 0, 3);  // multipliers of pg (and its u columns) -> lampad
    if (flow_rev)
      jt_lambda<M, RM, 3>(c, which, 0, 0, false, 1, fwd_qb, fwd_hfrac);
    else
      jt_lambda<M, RM, 3>(c, which, 0, 0);
  });
}

// chmc_switch_partition: the stored trajectories seed a time-parallel pass over the whole chain
template <class M>
static void xobs_par(chmc_ctx* c) {
  launch_blocks(k_xobs_par<M>, (long)c->sy.B, 64, 0, c->sy, c->sl, c->d_xobs);
}
// chmc_generate_x_seq*: the latent path of the current states by the time-parallel pass where chmc_switch_partition has one
// (compact rows allocated and a state set: the stored trajectories seed it), else -- and for a caller's q, which has no
// stored trajectory -- by the plain recursion
template <class M>
static void path_scan(chmc_ctx* c, const double* q, int stride, double* out, int* sweeps) {
  if (q || !(c->plan.pb_allocated && c->have_state)) return path_seq<M>(c, q, stride, out, sweeps);
  launch_blocks(k_path_par<M>, (long)c->sy.B, 64, 7, c->sy, c->sl, stride, out, sweeps), c->diag[10]++;
}
// the comparator target (nld_core): forward scan of the whole chain as the one block of `sf` (KernelPlan::nld), adjoint sweep
template <class M, int RM>
static void nld_sweeps(chmc_ctx* c, const Sys& sf, int QH, int use_gaussian_splitting, double* grad_dev) {
  const Sys& sy = c->sy;
  if (c->plan.nld == FwdPar) {
    Sys sp = sf;
    sp.order = c->d_order_ident;
    fwd_par<M, RM>(c->plan.nld_waves, (long)sy.B, sp, c->sl, c->w, 0, 1, 0, 2, 1, 0);
  } else if (c->plan.nld == FwdWave)
    launch_blocks(k_fwd_scan<M, RM, true>, ((long)sy.B + 63) / 64, 64 * (1 + CHMC_SCAN_HELPERS), 7, sf, c->sl, c->w, 0, 1, 0, 2, c->w, 0, 0);
  else
    launch(KFullScan<M>{sy, c->w.qb, c->w.trajw, QH}, sy.B, 7);
  launch_wave(k_nld_grad_wave<M>, (long)sy.B, 0, sy, c->w.qb, c->w.trajw, QH, use_gaussian_splitting, c->d_ham, grad_dev);
}
// chmc_gd_objective_device: the backward half, one wavefront per (chain, interval) task
template <class M>
static void gd_grad(chmc_ctx* c, long tasks, const double* q, const double* cres, double reg_coeff, double* g, double* part) {
  launch_wave(k_gd_grad_wave<M>, tasks, 0, c->sy, q, (const double*)c->w.trajw, cres, reg_coeff, g, part);
}

// The per-chain kernels, one workgroup of `waves` wavefronts per chain (chain_kernel_waves: CHMC_RETRACT_WAVES or 4); args:
// the kernel's arguments.  Instantiated where kChainKernels holds; retract_waves / traj_waves return 0 elsewhere.
template <class M, int RM, class... Args>
static void retract_chain(int waves, long n, Args... args) {
  if constexpr (kChainKernels<M, RM>) {
    if (waves == 4)
      launch_blocks(k_retract_chain<M, RM, 4>, n, 256, 1, args...);
    else
      launch_blocks(k_retract_chain<M, RM, CHMC_RETRACT_WAVES>, n, 64 * CHMC_RETRACT_WAVES, 1, args...);
  }
}
template <class M, int RM, class... Args>
static void traj_chain(int waves, long n, Args... args) {
  if constexpr (kChainKernels<M, RM>) {
    if (waves == 4)
      launch_blocks(k_traj_chain<M, RM, 4>, n, 256, 1, args...);
    else
      launch_blocks(k_traj_chain<M, RM, CHMC_RETRACT_WAVES>, n, 64 * CHMC_RETRACT_WAVES, 1, args...);
  }
}

#else  // the host emulation: generic functors over the stored rows
constexpr bool kWaveKernels = false;
// a pass no emulation plan selects: reaching it is a bug of the sequencing or of make_plan, never a silent no-op
[[noreturn]] static void no_wave_kernels(const char* pass) {
  fprintf(stderr, "chmc host emulation: %s needs the wave kernels; no plan without them selects it\n", pass);
  abort();
}

template <class M, int RM, int SYM, int TGT>
static void solve_chain(const Sys& sy, const Slots& sl, const Work& w, int which, int qsel, int psel) {
  launch(KSolveChain<M, RM, SYM, TGT>{sy, sl, w, which, qsel, psel}, sy.B, 5);
}
// forward scans: only those that store nothing (a quasi-Newton round's constraint values) -- KStateBlk and KNewtonBlk
// integrate the point themselves
template <class M, int RM>
static int fwd(chmc_ctx* c, int which, int qsel, int use_nw, int store, int) {
  if (store) return 0;
  launch(KFwd<M, RM>{c->sy, c->sl, c->w, which, qsel, use_nw, store}, (long)c->sy.B * c->sy.K, 7);
  return 1;
}
// (two functor launches in place of the merged one)
template <class M, int RM>
static int fwd_pair(chmc_ctx* c, const Work& w1, int which, int qsel, int store) {
  const Sys& sy = c->sy;
  if (store) return 0;
  launch(KFwd<M, RM>{sy, c->sl, c->w, which, qsel, 1, store}, (long)sy.B * sy.K, 7);
  launch(KFwd<M, RM>{sy, c->sl, w1, which, qsel, 1, store}, (long)sy.B * sy.K, 7);
  return 2;
}
template <class M, int RM>
static void state_sweep(chmc_ctx* c, int which) {
  launch(KStateBlk<M, RM>{c->sy, c->sl, c->w, which}, (long)c->sy.B * c->sy.K, 2);
}
template <class M, int RM>
static void gld_sweeps(chmc_ctx* c, int which) {
  launch(KGldBlk<M, RM>{c->sy, c->sl, c->w, which}, (long)c->sy.B * c->sy.K, 3);
}
template <class M, int RM>
static bool newton_sweep(chmc_ctx* c, int prev, int qsel) {
  launch(KNewtonBlk<M, RM>{c->sy, c->sl, c->w, prev, qsel}, (long)c->sy.B * c->sy.K, 1);
  return false;
}
// (two calls of the single pass each in place of the merged launches; no emulation plan has pair_passes)
template <class M, int RM>
static void newton_sweep_pair(chmc_ctx* c, const Work& w1, int prev, int qsel) {
  const Work w0 = c->w;
  for (int p = 0; p < 2; ++p) {
    c->w = p ? w1 : w0;
    if (!newton_sweep<M, RM>(c, prev, qsel)) solve_chain<M, RM, 0, 0>(c->sy, c->sl, c->w, prev, qsel, 0);
  }
  c->w = w0;
}
template <class M, int RM>
static void jt_lambda_pair(chmc_ctx* c, const Work& w1, int prev, int qsel) {
  const Work w0 = c->w;
  jt_lambda<M, RM, 0>(c, prev, qsel, 0);
  c->w = w1;
  jt_lambda<M, RM, 0>(c, prev, qsel, 0);
  c->w = w0;
}
template <class M, int RM>
static void jw(chmc_ctx* c, int which, int vsel, bool) {
  launch(KJw<RM>{c->sy, c->sl, c->w, which, vsel}, (long)c->sy.B * c->sy.K * RM, 6);
}
static void project_momentum(chmc_ctx* c, int which, int vsel, int psel);
static void project_pair(chmc_ctx* c, int which, bool, bool, double*, double) {
  project_momentum(c, which, 0, 0);
  project_momentum(c, which, 4, 3);
}
template <class M>
static void gd_grad(chmc_ctx* c, long tasks, const double* q, const double* cres, double reg_coeff, double* g, double* part) {
  launch(KGdGrad<M>{c->sy, q, c->w.trajw, cres, reg_coeff, g, part}, tasks);
}
// unreachable: the plan allocates no compact rows (k_xobs_par), nld_core refuses the call first, no layout is eligible for the
// per-chain kernels
template <class M>
static void xobs_par(chmc_ctx*) { no_wave_kernels("the partition switch's time-parallel pass"); }
template <class M>
static void path_scan(chmc_ctx* c, const double* q, int stride, double* out, int* sweeps) {
  path_seq<M>(c, q, stride, out, sweeps);
}
template <class M>
static void predict_pass(chmc_ctx* c, const PredictArgs& a, const EventArgs* e, double* evraw, long long* n, double* mean,
                         double* m2, long long* cdf) {
  predict_seq<M>(c, a, e, evraw, n, mean, m2, cdf);
}
template <class M>
static void future_pass(chmc_ctx* c, const PredictArgs& a, const FutureArgs& f) {
  future_seq<M>(c, a, f);
}
template <class M>
static void path_events_pass(chmc_ctx* c, int NP, const EventArgs& e, const int* mask, const double* x, double* out) {
  path_events_seq<M>(c, NP, e, mask, x, out);
}
template <class M>
static void resample_pass(chmc_ctx* c, const ResampleArgs& a) {
  resample_seq<M>(c, a);
}
template <class M, int RM>
static void nld_sweeps(chmc_ctx*, const Sys&, int, int, double*) { no_wave_kernels("the comparator target"); }
template <class M, int RM, class... Args>
static void retract_chain(int, long, Args...) { no_wave_kernels("the per-chain retraction"); }
template <class M, int RM, class... Args>
static void traj_chain(int, long, Args...) { no_wave_kernels("the per-chain trajectory"); }
#endif
