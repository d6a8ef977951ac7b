// Which kernel runs for which pass: decided here, once per context, from the layout and the environment switches.
// Plain host C++ (no device code, no HIP): chmc_api.inc stores the KernelPlan in the context, its sequencing and the passes
// of chmc_passes.inc (the launch sites) switch on it; tests/test_kernel_plan.py states the table on the CPU through tests/emu/plan_probe.cpp.
//
// The library has TWO complete sets of kernels for the passes over a point's Jacobian (RowFamily); every other round-1 /
// round-2 variant has been removed (round 3):
//   compact rows (default)   Slots::PB / LF; Newton sweep = k_newton_ivl + k_newton_comb (+ k_newton_fsm_wave), state sweep =
//                            k_state_lean, grad-log-det = k_gld_fwd_qx + k_gld_bwd_lean, J p = k_jw_pb,
//                            J^T lambda = KMuF + KUpdatePB; 16-row blocks: rows stored as well (state sweep
//                            k_rev_wave_ldsrows + k_gram_rows) unless the blocks are few (interval-parallel sweeps)
//   stored rows              round 1's kernels over Slots::Jv: k_rev_wave / k_rev_wave_ldsrows, k_gram_rows, k_gld_fwd_wave +
//                            k_gld_bwd_wave(_ldsrows), k_jw_wave, KUpdate -- kept as the independent second implementation
//                            the full-size A/B test compares against (tests/test_hip_parity.py)
//   stored rows, MFMA Gram   the Gram block on the matrix cores (v_mfma_f64_16x16x4_f64, k_gram_rows_mfma) instead of with
//                            vector FMAs; it contracts rows in memory, so it puts the 16-row Newton sweep on the stored-rows
//                            kernels and selects the whole stored-rows family for blocks of at most 8 rows (the sweeps
//                            k_rev_wave<.., GRAM = false> store the rows, the state's into Slots::Jv, the Newton iterate's into
//                            work.JvW, and accumulate no Gram block).  Measurements: DESIGN.md section 4,
//                            profiles/mfma_gram_utilisation_fhn_s800.txt
//
// Environment switches -- EVERY variable the library reads, all of them in read_switches(); each is exercised by a GPU test.
//   latched by the first chmc_create of the process:
//   CHMC_COMPACT_ROWS=0     the stored-rows family everywhere (the A/B partner of the default)
//   CHMC_GRAM_MFMA=1        the stored-rows family with the MFMA Gram kernel
//   read by chmc_create:
//   CHMC_PAR_SCAN=0/1       time-parallel forward scan off / forced (default: at most 4 blocks per chain, >= 1024 steps; the
//                           comparator target's scan reads it at every call)
//   CHMC_PAR_WAVES=1/2/4    wavefronts per (chain, block) of that scan (default: from the block length; likewise)
//   CHMC_ROW_SPLIT=1/2/4    16-row state evaluation: 1 = stored-rows sweeps, otherwise interval-parallel (default: <= 4 blocks)
//   CHMC_HALVES=2           two overlapped half-batches per step
//   read on entry to every call on a context:
//   CHMC_NO_FWD_SCAN        (set) generic functor instead of the hand-scheduled forward scan
//   CHMC_STEP_FUSIONS=0     the momentum correction and the reverse flow of a step as passes of their own instead of inside
//                           the J p / J^T lambda passes (same bits)
//   CHMC_RETRACT_KERNEL=0/1/2  one 16-row block per chain: batched launches / one workgroup of 8 wavefronts per chain / of 4
//                           wavefronts (two chains per compute unit).  Default: 8 up to one chain per compute unit, 4 up to
//                           four, batched beyond; all three give the same bits.  The per-chain kernels are instantiated for the
//                           SIR models only: a FitzHugh-Nagumo layout with one 16-row block per chain always runs the batched
//                           launches of the same plan and the switch is a no-op there (retract_waves / traj_waves, chmc_api.inc)
//   CHMC_PAIR_RETRACT=0/1   chmc_leapfrog_steps: 0 = every retraction in a Newton loop of its own; 1 = the reverse retraction of
//                           step i and the forward retraction of step i + 1 advance round for round in one loop with one
//                           forward-scan launch per round for both (KernelPlan::pair_retractions).  Default: paired while the
//                           merged launch still has a compute unit per workgroup (pair_this_call); both give the same bits
//   CHMC_PAIR_PASSES=0      a paired loop launches every pass behind the scan once per problem instead of once for both
//                           (KernelPlan::pair_passes; the A/B partner of the merged passes, same bits)
//   CHMC_FUTURE_WAVE=1      chmc_score_future_device runs its wave kernel (k_future_score) where the compact rows are allocated
//                           (KernelPlan::future_wave) instead of the functor form (KFutureScore), the default because it was the
//                           faster one at every measured shape: the A/B partner on the SAME state and
//                           start state -- CHMC_COMPACT_ROWS=0 also changes the stepping kernels and the path scan, and with them
//                           the inputs at rounding level; same bits
#pragma once
#include <climits>
#include <cstdlib>

#ifndef CHMC_RETRACT_WAVES
#define CHMC_RETRACT_WAVES 8  // (chmc_retract.h; repeated for builds without the wave kernels)
#endif
#ifndef CHMC_CHAIN_SCAN_WAVES
#define CHMC_CHAIN_SCAN_WAVES 4  // (chmc_retract.h, likewise)
#endif
static_assert(CHMC_CHAIN_SCAN_WAVES == 1 || CHMC_CHAIN_SCAN_WAVES == 2 || CHMC_CHAIN_SCAN_WAVES == 4,
              "k_fwd_par is launched with 1, 2 or 4 wavefronts per workgroup (fwd_par in chmc_passes.inc)");
#ifndef CHMC_CHAIN_WG4_MAX_PER_CU
#define CHMC_CHAIN_WG4_MAX_PER_CU 4  // (chains per CU up to which two 4-wavefront workgroups per CU match or beat batched launches)
#endif

namespace chmc {

constexpr int kSwitchUnset = INT_MIN;
struct Switches {
  bool compact_rows = true, gram_mfma = false;
  int par_scan = kSwitchUnset, par_waves = kSwitchUnset, row_split = 0, halves = 1;
  bool no_fwd_scan = false, step_fusions = true;
  int retract_kernel = kSwitchUnset, pair_retract = kSwitchUnset;
  bool pair_passes = true;
  bool future_wave = false;
};
inline Switches read_switches() {
  auto env = [](const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
  };
  static const bool compact_rows = env("CHMC_COMPACT_ROWS", 1) != 0, gram_mfma = env("CHMC_GRAM_MFMA", 0) != 0;
  Switches s;
  s.compact_rows = compact_rows, s.gram_mfma = gram_mfma;
  s.par_scan = env("CHMC_PAR_SCAN", kSwitchUnset), s.par_waves = env("CHMC_PAR_WAVES", kSwitchUnset);
  s.row_split = env("CHMC_ROW_SPLIT", 0), s.halves = env("CHMC_HALVES", 1);
  s.no_fwd_scan = getenv("CHMC_NO_FWD_SCAN") != nullptr, s.step_fusions = env("CHMC_STEP_FUSIONS", 1) != 0;
  s.retract_kernel = env("CHMC_RETRACT_KERNEL", kSwitchUnset);
  s.pair_retract = env("CHMC_PAIR_RETRACT", kSwitchUnset);
  s.pair_passes = env("CHMC_PAIR_PASSES", 1) != 0;
  s.future_wave = env("CHMC_FUTURE_WAVE", 0) == 1;
  return s;
}

// What the plan is decided from: the LAYOUT (blocks per chain, block length, rows) -- never the number of chains in the
// context -- so a chain's bits do not depend on the shard it runs in: N ranks of B / N chains reproduce one rank of B chains
// chain for chain (tests/test_hip_parity.py::test_results_do_not_depend_on_the_shard_size).
struct PlanInput {
  int rmt;               // row slots per block: 6, 7, 8 or 16
  int num_partition;
  int K[2];              // blocks per chain, per partition
  int longest;           // steps of the longest block of any partition
  int chain_steps;       // T S: the one block of the comparator target's scan
  bool s_tiles8;         // S % 8 == 0: the hand-scheduled forward scan has its 8-step tiles
  int V;                 // noise increments per step
  bool even_dims;        // Q, U, V0 and NV all even (16-byte pairs of p and pg)
  bool gaussian;         // Gaussian splitting
  bool wave_kernels;     // CHMC_WAVE_KERNELS: without them every pass is a generic functor over the stored rows
  Switches sw;           // as read by chmc_create
  Switches call;         // as read on entry to the current call: no_fwd_scan, step_fusions, retract_kernel, pair_retract,
                         // pair_passes, future_wave; the comparator's scan
};

enum RowFamily { RowsCompact, RowsStored, RowsStoredMfma };
enum FwdScan { FwdPar /* k_fwd_par<W> */, FwdWave /* k_fwd_scan */, FwdFunctor /* KFwd; comparator: KFullScan */ };
enum StateSweep {
  StateLean,             // k_state_lean
  StateIvlComb,          // k_newton_ivl<STATE> + k_newton_comb<STATE>
  StateIvlCombWg,        // k_newton_ivl<STATE> + k_newton_comb_wg<STATE> (one block per chain; factors the block as well)
  StateLdsrowsGram,      // k_rev_wave_ldsrows + k_gram_rows
  StateLdsrowsGramMfma,  // k_rev_wave_ldsrows + k_gram_rows_mfma
  StateRevWave,          // k_rev_wave
  StateRevStoreGramMfma  // k_rev_wave<.., GRAM = false> + k_gram_rows_mfma
};
enum NewtonSweep {  // sweep of the iterate, block factorisation, chain solve
  NewtonIvlFsm,            // k_newton_ivl + k_newton_comb, k_newton_fsm_wave (LU, Woodbury solve, u-columns, mu_F)
  NewtonIvlComb,           // k_newton_ivl + k_newton_comb, KNewtonFactor, chain solve
  NewtonRevWave,           // k_rev_wave, KNewtonFactor, chain solve
  NewtonRevStoreGramMfma,  // k_rev_wave<.., GRAM = false> + k_gram_rows_mfma, KNewtonFactor, chain solve
  Newton16IvlCombWg,       // k_newton_ivl + k_newton_comb_wg (combine, LU on 16 lanes, solve: the bits of k_retract_chain)
  Newton16IvlCombFactor,   // k_newton_ivl + k_newton_comb<.., FACTOR> (one block per chain: factors, solves, forms lambda, mu_F)
  Newton16IvlComb,         // k_newton_ivl + k_newton_comb, k_newton_factor_wave, chain solve
  Newton16LdsrowsGram,     // k_rev_wave_ldsrows + k_gram_rows, k_newton_factor_wave, chain solve
  Newton16LdsrowsGramMfma  // k_rev_wave_ldsrows + k_gram_rows_mfma, k_newton_factor_wave, chain solve
};
enum GldSweep {
  GldQxLean,            // k_gld_fwd_qx + k_gld_bwd_lean (row-free)
  GldIvl,               // k_gld_ivl_prologue, k_gld_fwd_ivl, k_gld_bwd_ivl<0>, <1>, k_gld_ivl_finish (row-free, wavefront per interval)
  GldCompactFwdStored,  // k_gld_fwd_wave<.., compact weights> + k_gld_bwd_wave_ldsrows
  GldStored             // k_gld_fwd_wave + k_gld_bwd_wave (16-row blocks: _ldsrows)
};
enum JpPass { JpPb /* k_jw_pb */, JpPbWg /* k_jw_pb_wg: the pair (J p, J pg) only */, JpWave /* k_jw_wave */ };

struct PartitionPlan {
  StateSweep state;
  NewtonSweep newton;
  GldSweep gld;
  JpPass jp;
  bool rebuild_rows;   // the state sweep leaves Slots::Jv unwritten: entry points that hand rows out rebuild them (ensure_rows)
  bool retract_chain;  // layout of k_retract_chain: whether it runs is the call's choice (chain_kernel_waves)
  bool traj_chain;     // ... and of k_traj_chain
};
struct KernelPlan {
  RowFamily rows;      // RowsCompact: J^T lambda = KMuF + KUpdatePB, otherwise KUpdate
  bool pb_allocated;   // Slots::PB / LF exist (16-row blocks with the MFMA Gram keep them beside the stored rows); with them,
                       // chmc_switch_partition seeds a time-parallel pass (k_xobs_par) from the stored trajectories
  bool par_scan;       // time-parallel forward scans: a chain may sit a round out (run_projection), always one batch
  FwdScan fwd;         // forward scan with a guess trajectory
  FwdScan fwd_cold;    // ... with none
  int fwd_waves;       // wavefronts per (chain, block) of FwdPar
  FwdScan nld;         // the comparator target's scan (one block per chain)
  int nld_waves;
  bool mom_fix_in_jp;       // a step's momentum correction (KMomFixInitPg) rides in the J p pass (k_jw_pb<.., FIX>)
  bool rev_flow_in_update;  // the reverse flow of the reversibility check (KFlow) rides in the J^T lambda pass (KUpdatePB<.., 3>)
  int retract_kernel;       // CHMC_RETRACT_KERNEL of this call
  // Inside a trajectory (chmc_leapfrog_steps, one n_steps for all chains) the reverse retraction of step i -- the
  // reversibility check -- and the forward retraction of step i + 1 are independent Newton loops against the same point q':
  // they advance round for round in ONE lock-step loop, and each round's forward scan is one launch for both (k_fwd_scan<..,
  // PAIR>: twice the lanes at the latency of one scan).  Lock-step round path only: not the per-chain kernel layouts
  // (k_retract_chain / k_traj_chain), not two half-batches, and not the time-parallel scan -- its first sweep takes the
  // state slot's trajectory as its guess, which before the commit of step i is not the one the unpaired step i + 1 starts
  // from, and a chain's bits must not depend on the pairing.  With the wave kernels only where the scan is k_fwd_scan (the
  // generic functor has no merged launch: two launches would save nothing), unless CHMC_PAIR_RETRACT=1 asks for it.  Whether a
  // call pairs is then pair_this_call's choice.
  bool pair_retractions;
  int pair_retract;         // CHMC_PAIR_RETRACT of this call
  // A round of a paired loop in which both problems still iterate runs the passes behind the scan ONCE for both as well
  // (newton_sweep_pair, jt_lambda_pair in chmc_passes.inc): both are Newton sweeps and J^T lambda updates against the same
  // compact rows Slots::PB / LF of the proposal slot, so one work item / workgroup serves both iterates from one read of
  // them, and the latency-bound combine and solve kernels carry both problems' wavefronts in one grid.  Compact rows in
  // blocks of at most 8 row slots with the one-launch solve (NewtonIvlFsm: at most 64 blocks per chain) in every partition;
  // every other plan, and CHMC_PAIR_PASSES=0, keeps one launch per problem and pass.  Same bits either way.
  bool pair_passes;
  bool future_wave;    // chmc_score_future_device: k_future_score (CHMC_FUTURE_WAVE=1, and predict_pass's rule: the compact rows
                       // are allocated) instead of the functor form
  PartitionPlan part[2];
};

// Wavefronts per (chain, block) of the time-parallel scan, with at least 16 steps per segment.  Measured on boarding-school
// SIR (2 800 steps), lock-step Newton loop of round 3, steps/s for 1 / 2 / 4 wavefronts per chain: 256 chains 32.6 k / 35.5 k /
// 31.5 k, 512 chains 54.6 k / 54.7 k / -- (a sweep over 22 steps per lane takes 17.5 us, over 11 steps 11.3 us: the prefix
// scan across the lanes and the workgroup barriers do not shrink with the segments).  CHMC_PAR_WAVES overrides (1, 2, 4).
inline int par_waves_for(int env, long longest) {
  if (env == 1 || env == 2 || env == 4) return env;
  return longest >= 4096 ? 4 : longest >= 2048 ? 2 : 1;
}
// Few long blocks per chain (the SIR single-block layout: 1 x 2 800 steps): the time-parallel scan and the interval-parallel
// 16-row state evaluation; many short blocks (FitzHugh-Nagumo: 20 x 2 000): lanes / wavefronts per block already fill the chip.
inline bool few_long_blocks(int nblocks_per_chain, long longest) { return nblocks_per_chain <= 4 && longest >= 1024; }

inline KernelPlan make_plan(const PlanInput& in) {
  const Switches& sw = in.sw;
  KernelPlan pl{};
  const bool rows16 = in.rmt > 8;
  const int kmax = in.K[0] > in.K[in.num_partition - 1] ? in.K[0] : in.K[in.num_partition - 1];
  // One 16-row block per chain (the boarding-school SIR layout): the layouts of the per-chain kernels (chmc_retract.h).  Their
  // batched (lock-step) path runs the same per-chain arithmetic bit for bit: scans of CHMC_CHAIN_SCAN_WAVES wavefronts per
  // chain, the workgroup-parallel combine with the 16-lane factorisations, J p over the wavefronts.
  const bool chain16_layout = kmax == 1 && rows16;

  const bool compact = in.wave_kernels && sw.compact_rows && !sw.gram_mfma;
  pl.rows = compact ? RowsCompact : sw.gram_mfma ? RowsStoredMfma : RowsStored;
  pl.pb_allocated = compact || (in.wave_kernels && sw.compact_rows && rows16);

  // Time-parallel forward scan: pays when a lane-per-block scan leaves the chip empty for a long recursion, i.e. for few
  // long blocks per chain.  Decided from the layout alone: whatever the number of chains (1 024 blocks of 2 800 steps: 0.9 ms
  // for the sequential scan on 16 wavefronts against three or four sweeps of 27 us per wavefront).
  // (one 16-row block per chain on the compact rows: always, whatever the block length -- the per-chain kernels integrate
  // that way, and the batched path of these layouts does the same arithmetic)
  pl.par_scan = sw.par_scan != kSwitchUnset ? sw.par_scan != 0
                                            : few_long_blocks(kmax, in.longest) || (chain16_layout && sw.compact_rows && !sw.gram_mfma);
  pl.fwd_waves = chain16_layout && sw.par_waves == kSwitchUnset ? CHMC_CHAIN_SCAN_WAVES : par_waves_for(sw.par_waves, in.longest);
  // hand-scheduled wave kernel when the steps per observation tile by 8, the generic functor otherwise
  pl.fwd_cold = in.wave_kernels && in.s_tiles8 && !in.call.no_fwd_scan ? FwdWave : FwdFunctor;
  pl.fwd = in.wave_kernels && pl.par_scan ? FwdPar : pl.fwd_cold;
  // The comparator target: one block of T S steps per chain.  A lane-per-chain scan keeps B / 64 wavefronts busy for T S
  // dependent steps (0.93 ms for the 2 800 steps of the boarding-school SIR chains, 2.8 ms for 40 000 FitzHugh-Nagumo steps) --
  // for up to 1 024 chains the time-parallel scan does it in a few sweeps.
  const bool nld_par = in.call.par_scan != kSwitchUnset ? in.call.par_scan != 0 : few_long_blocks(1, in.chain_steps);
  pl.nld = nld_par ? FwdPar : in.s_tiles8 ? FwdWave : FwdFunctor;
  pl.nld_waves = par_waves_for(in.call.par_waves, in.chain_steps);

  // Element-wise passes of a step folded into their neighbours on the compact rows (the same bits):
  //  * the momentum correction: blocks with at most 8 rows, two noise increments per step and even dimensions;
  //  * the reverse flow: blocks with at most 8 rows, standard splitting only (hipcc contracts the rotation q cos - p sin of the
  //    Gaussian splitting differently inside the column pass -- equal to rounding, not bitwise; the switch must not change a bit).
  const bool step_fusions = pl.pb_allocated && in.call.step_fusions && !rows16;
  pl.mom_fix_in_jp = step_fusions && in.V == 2 && in.even_dims;
  pl.rev_flow_in_update = step_fusions && !in.gaussian;
  pl.future_wave = pl.pb_allocated && in.call.future_wave;
  pl.retract_kernel = in.call.retract_kernel;
  pl.pair_retract = in.call.pair_retract;
  pl.pair_retractions = in.call.pair_retract != 0 && sw.halves != 2 && pl.fwd != FwdPar &&
                        (!in.wave_kernels || pl.fwd_cold == FwdWave || in.call.pair_retract == 1);

  for (int p = 0; p < in.num_partition; ++p) {
    PartitionPlan& pp = pl.part[p];
    const int K = in.K[p];
    // 16-row blocks, state evaluation: with at most 4 blocks per chain the interval-parallel sweeps on the compact rows (a
    // wavefront per observation interval), otherwise the stored-rows sweeps with one wavefront per block (many blocks per
    // chain: those fill the chip by themselves).  CHMC_ROW_SPLIT overrides (1: stored rows; 2, 4: interval-parallel).
    const bool split = sw.row_split == 1 ? false : (sw.row_split == 2 || sw.row_split == 4) ? true : K <= 4;
    const bool ivl16 = rows16 && compact && split;
    const bool chain16 = chain16_layout && ivl16;
    if (rows16) {
      pp.state = chain16 ? StateIvlCombWg : ivl16 ? StateIvlComb : sw.gram_mfma ? StateLdsrowsGramMfma : StateLdsrowsGram;
      pp.newton = chain16 ? Newton16IvlCombWg
                  : compact ? (K == 1 ? Newton16IvlCombFactor : Newton16IvlComb)
                  : sw.gram_mfma ? Newton16LdsrowsGramMfma : Newton16LdsrowsGram;
      pp.gld = ivl16 ? GldIvl : compact ? GldCompactFwdStored : GldStored;
    } else {
      pp.state = compact ? StateLean : sw.gram_mfma ? StateRevStoreGramMfma : StateRevWave;
      // (at most 64 blocks per chain: k_newton_fsm_wave, a wavefront per chain)
      pp.newton = compact ? (K <= 64 ? NewtonIvlFsm : NewtonIvlComb) : sw.gram_mfma ? NewtonRevStoreGramMfma : NewtonRevWave;
      pp.gld = compact ? GldQxLean : GldStored;
    }
    pp.jp = chain16 ? JpPbWg : compact ? JpPb : JpWave;
    pp.rebuild_rows = compact && (!rows16 || ivl16);
    // NOTE (inconsistent, kept as it was): eligibility ignores CHMC_PAR_SCAN, CHMC_PAR_WAVES and CHMC_ROW_SPLIT, although
    // the per-chain kernels always scan in parallel on CHMC_CHAIN_SCAN_WAVES wavefronts and combine per workgroup -- with
    // one of those switches pinned, the batched path computes other bits and the choice by chains per CU shows.  The fix is
    // to require `chain16 && pl.par_scan && pl.fwd_waves == CHMC_CHAIN_SCAN_WAVES` here.
    pp.retract_chain = compact && rows16 && K == 1;
    pp.traj_chain = pp.retract_chain && ivl16;
    if (pp.retract_chain) pl.pair_retractions = false;
  }
  pl.pair_passes = pl.pair_retractions && in.call.pair_passes && in.wave_kernels && pl.rows == RowsCompact && in.rmt <= 8;
  for (int p = 0; p < in.num_partition; ++p) pl.pair_passes = pl.pair_passes && pl.part[p].newton == NewtonIvlFsm;
  return pl;
}

// Per-chain kernels against batched launches: the one choice made per call.  Wavefronts per chain of k_retract_chain /
// k_traj_chain (0: the batched path).  8 while every chain has a CU to itself (two wavefronts per SIMD work on ONE chain); 4 up
// to four chains per CU: two workgroups -- two chains -- then share a CU (one wavefront per SIMD each, the same 256 registers;
// 75 KB of LDS each), and each chain's phases fill the other's barrier and latency gaps; batched launches with 3 - 4
// wavefronts per SIMD beyond that.  The arithmetic does not depend on the number of wavefronts (every sum is formed by one
// thread or one wavefront in a fixed order; the scan has its 256 segments on four wavefronts either way), nor on the
// execution model (tests/test_hip_parity.py::test_per_chain_kernels_equal_the_batched_path_bitwise).
// Boarding-school SIR, steps/s by chains per GPU (8 wavefronts | 4 wavefronts | batched), profiles/r04c_bench_sir_*:
//   256: 84.0 k | 75.9 k | 69.0 k     512: 97.1 k | 121.7 k | 103.3 k     1 024: 99.2 k | 122.8 k | 120.2 k     2 048: 106.7 k |
//   137.7 k | 140.2 k.   CHMC_RETRACT_KERNEL=0 / 1 / 2 forces batched / 8 / 4.
inline int chain_kernel_waves(const KernelPlan& pl, bool eligible, int B, int num_cus, bool newton, bool half_batches) {
  if (!eligible || !newton || half_batches) return 0;
  const int want = pl.retract_kernel != kSwitchUnset ? pl.retract_kernel
                   : B <= num_cus ? 1 : B <= CHMC_CHAIN_WG4_MAX_PER_CU * num_cus ? 2 : 0;
  return want == 1 ? CHMC_RETRACT_WAVES : want == 2 ? 4 : 0;
}

// Paired retractions against a loop per retraction: the other choice made per call -- like the one above a pure scheduling
// decision, the bits are the same either way (tests/test_pair_retractions.py), so it may look at the batch.  The merged scan
// launch has 2 ceil(B K / 64) workgroups, and it keeps the latency of a single scan only while each of them has a compute
// unit to itself: measured on one box (steps/s, paired | unpaired), FitzHugh-Nagumo S = 400, 256 chains
// (160 workgroups on 256 compute units): 55.4-56.3 k | 53.2-53.7 k; S = 800, 512 chains (320 workgroups): 31.0 k | 32.4 k --
// the scans of two workgroups that share a compute unit take as long as two scans, and the second problem's passes are no
// longer free.  Without the wave kernels (the host emulation of the tests) there is no merged launch to fit: always paired.
// CHMC_PAIR_RETRACT=1 pairs whatever the batch.
inline bool pair_this_call(const KernelPlan& pl, bool wave_kernels, int B, int K, int num_cus) {
  if (!pl.pair_retractions) return false;
  if (pl.pair_retract == 1 || !wave_kernels) return true;
  return 2 * (((long)B * K + 63) / 64) <= num_cus;
}

}  // namespace chmc
