// Host side of the C ABI (include/chmc.h): context, device memory, kernel sequencing.
// Included by chmc.hip (HIP backend) after the backend primitives are defined:
//   dev_alloc / dev_free / dev_zero / h2d / d2h / d2d / dev_sync / launch(functor, n) / CHMC_BACKEND_NAME
// (tests/emu/ compiles the same text over a host backend to unit-test this sequencing logic without a GPU;
// the shipped library has no such path.)
#include <string>
#include <algorithm>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <thread>
#include <type_traits>
#include "../../include/chmc.h"
#include "chmc_plan.h"
#include "chmc_layout.h"

using namespace chmc;

static thread_local std::string g_err;
static int fail(const std::string& m) {
  g_err = m;
  return -1;
}
#include CHMC_BACKEND_HEADER

struct chmc_ctx : ChainView {  // sy, sl, w and the per-chain arrays handed to kernels one by one: chmc_layout.h
  // Streams, poll slots and events of the backend are thread_local: a context belongs to the host thread that created it
  // (SURVEY 8b "one ctx per (device, stream); not re-entrant"); every entry point checks that instead of running on another
  // thread's (missing) streams.
  std::thread::id owner = std::this_thread::get_id();
  chmc_config cfg;
  int model, RMt, part, num_partition, npart_sum;
  int K[2], C[2];
  std::vector<BlockDesc> hblk[2];
  BlockDesc* d_blk[2];
  int* d_obs2blk[2];
  int* d_order[2];  // wave -> (chain, block) work order of the wave-per-block kernels, longest blocks first
  double *d_y, *d_ham;
  unsigned long long* d_out = nullptr;  // [rev | status | iters_fwd | iters_bwd] x B (alias_step_outputs)
  BlockDesc* d_blk_full = nullptr;       // one block spanning all observations (chmc_neg_log_dens_and_grad)
  int* d_order_ident = nullptr;          // identity work order [B] for that one-block-per-chain layout
  unsigned long long* d_fill_keys = nullptr;  // chmc_fill_normal*: [B][2] (stream, draw) of the listed rows, then [B] ints: the rows
  double* d_gd = nullptr;  // chmc_gd_objective_device: [B][T][X] c, [B][T][Z + 2] interval partials, [B][2] chain sums (whole-batch launches only)
  double* d_place = nullptr;  // chmc_set_state_project_device: [B][T][X] scanned x_obs_seq, [B][T] dobs, [B][T] pok, [B] defect, [B] pinfail, [B] moved
  bool mom_tangent = false;  // every chain's momentum is known to lie in the cotangent space of its current point
  bool snap_tangent = false; // ... at the time of chmc_snapshot
  bool have_state = false;   // a chain state has been set (chmc_set_metric then refreshes its cached factors)
  double* d_m0 = nullptr;    // [3 U U + 1] M_0, M_0^-1, chol(M_0), log det(M_0) / 2 of the block metric every chain shares
  double *d_tree_part = nullptr, *d_tree_out = nullptr;  // chmc_tree_leaf: workgroup partials, per-chain results
  int* d_tree_mask = nullptr;                            // [2][B] run, take
  int* d_path_ints = nullptr;       // chmc_generate_x_seq* / chmc_path_stats_update_device: [2][B] sweeps, mask
  double* d_path_out = nullptr;     // chmc_generate_x_seq: staging of the host form's output, d_path_cap doubles
  size_t d_path_cap = 0;
  double* d_pred = nullptr;         // chmc_predict_device: the replicates' raw channels or group statistics, d_pred_cap doubles
  size_t d_pred_cap = 0;
  double* d_pred_x = nullptr;       // ... [B][T + 1][X] the chains' paths at the observation times (the forecast's start state)
  double* d_pred_lev = nullptr;     // ... the CDF levels, d_pred_lev_cap doubles
  size_t d_pred_lev_cap = 0;
  double* d_pred_ev = nullptr;      // chmc_predict_events_device: [NPF] point times, then the raw events where the caller keeps none
  size_t d_pred_ev_cap = 0;
  double* d_fut = nullptr;          // chmc_score_future_device: [B][H] y_future, [B] log_pred, [B] ints picked (padded to doubles),
  size_t d_fut_cap = 0;             // then [B][n_cand][H] the candidates' n and, where the caller keeps none, [B][n_cand] logw
  TreeState tree{};                                     // chmc_tree_begin / _subtree / _step: per-chain tree decisions
  bool have_tree = false;
  bool rows_fresh = false;  // Slots::Jv holds the full rows of the current states (see ensure_rows)
  std::vector<unsigned char> h_out;
  std::vector<void*> allocs;
  long long counters[8];
  PlanInput plan_in{};  // layout and switches the kernel plan is decided from (chmc_plan.h)
  KernelPlan plan{};    // which kernel runs for which pass; the per-partition part is plan.part[part]
  long long diag[16] = {0};  // launches by kernel family: [0] k_gram_rows_mfma, [1] k_gram_rows, [2] k_retract_chain, [3] k_traj_chain,
                              // [4] k_newton_fsm_wave, [5] KNewtonFactor (blocks of at most 8 rows), [6] rounds whose forward scan
                              // served two problems (one k_fwd_scan<.., PAIR> launch), [7] forward-scan launches of the
                              // lock-step Newton loop (run_lockstep), [8] rounds it enqueued, per problem, [9] rounds of a paired
                              // call whose passes behind the scan served two problems as well (KernelPlan::pair_passes: interval
                              // sums, combine, solve and J^T lambda update one launch each; a subset of [6]), [10] launches of
                              // the time-parallel path scan, [11] of the sequential one (KPath), [12] of the predictive wave
                              // kernel, [13] of its functor form (KPredict), [14] of the path-events wave kernel, [15] of its
                              // functor form (KPathEvents)
  // Paired retractions (KernelPlan::pair_retractions): the second problem of a paired run_lockstep call -- the forward
  // retraction of the NEXT step -- works in a Work of its own: every array a round's kernels, KNewtonBegin, KCheck or KNewtonEnd
  // write (pair_alloc), everything they only read shared with `w`.  Whole batch only, allocated on first use.
  Work pw{};
  int* d_itf_next = nullptr;  // [B] its iteration counts: the next step's iters_fwd
  bool have_pair = false;
  bool pair_ready = false;    // the last step ran that loop: the next step of the trajectory adopts its result
  // two half-batches on two streams (chmc_leapfrog_step): chain ranges [hc0[h], hc0[h] + hB[h]) and their work orders
  int round = 0;                   // round of the current Newton loop
  int halves = 1;                  // 1: the step runs as one batch; 2: as two overlapped half-batches
  int hB[2] = {0, 0}, hc0[2] = {0, 0};
  int* d_order_half[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [partition][half]
  void* comm = nullptr;                     // RCCL communicator of chmc_comm_init (ncclComm_t)
  int comm_rank = 0, comm_world = 1;
  int last_n_inner = 1;
  int proj_rounds[2] = {0, 0}, proj_stable[2] = {0, 0};  // rounds the last forward / reverse retraction needed; how often in a row
                                                          // (by a problem's direction, alone or paired; half-batches leave it alone)
  int num_cus = 256;                            // compute units of the device (per-chain kernels: up to 2 chains per CU)
  std::vector<double> last_dt;     // last uploaded step sizes
  std::vector<int> last_active;
  bool last_active_null = true;
};

template <class T_>
static T_* alloc(chmc_ctx* c, size_t n) {
  T_* p = (T_*)dev_alloc(n * sizeof(T_));
  c->allocs.push_back(p);
  return p;
}
// chmc_create: every array of the list (chmc_layout.h) that this context has from the start
static void alloc_chain_arrays(chmc_ctx* c) {
  const size_t B = c->sy.B;
  for_each_chain_array(*c, c->plan, c->npart_sum, [&](auto*& p, size_t per_chain, int kind, size_t slack) {
    using T_ = std::remove_reference_t<decltype(*p)>;
    p = nullptr;
    if (kind & (kLazy | kAbsent)) return;
    p = alloc<T_>(c, B * per_chain + slack);
    if (kind & kZeroed) dev_zero(p, sizeof(T_) * (B * per_chain + slack));
  });
}
// ... and one that is allocated on first use (whole-batch view only)
template <class T_>
static void ensure_array(chmc_ctx* c, T_*& want) {
  if (want) return;
  const size_t B = c->sy.B;
  for_each_chain_array(*c, c->plan, c->npart_sum, [&](auto*& p, size_t per_chain, int, size_t slack) {
    if ((void*)&p == (void*)&want) want = alloc<T_>(c, B * per_chain + slack);
  });
}

// wave -> (chain, block) work order of `chains` chains, longest blocks first, on the device (`slack` spare entries)
static int* upload_work_order(chmc_ctx* c, const std::vector<BlockDesc>& blk, int chains, int slack) {
  const int K = (int)blk.size();
  std::vector<int> order((size_t)chains * K);
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return blk[a % K].nsteps > blk[b % K].nsteps; });
  int* d = alloc<int>(c, order.size() + slack);
  if (!order.empty()) h2d(d, order.data(), sizeof(int) * order.size());
  return d;
}

// block shape tables (sde/mici_extensions.py:321-351; rows :406-411)
static void build_partition(chmc_ctx* c, int p, int init) {
  const chmc_config& g = c->cfg;
  const int T = g.num_obs, R = g.num_obs_per_subseq, S = g.num_steps_per_obs;
  const int X = c->sy.X, V = c->sy.V, V0 = c->sy.V0;
  std::vector<int> sizes;
  if (R <= 0 || R >= T) {
    sizes.push_back(T);
  } else {
    int num_full = (T - init) / R, num_rem = (T - init) % R;
    int num_middle = num_rem == 0 ? num_full - 1 : num_full;
    int final_ = num_rem == 0 ? R : num_rem;
    sizes.push_back(init);
    for (int i = 0; i < num_middle; ++i) sizes.push_back(R);
    sizes.push_back(final_);
  }
  int obs = 0, row = 0;
  for (size_t b = 0; b < sizes.size(); ++b) {
    BlockDesc B;
    memset(&B, 0, sizeof(B));
    B.obs0 = obs, B.nobs = sizes[b], B.first = b == 0, B.last = b + 1 == sizes.size();
    B.ny = (B.last || g.noisy) ? B.nobs : B.nobs - 1;
    B.nrows = B.ny + (B.last ? 0 : X);
    B.row0 = row;
    B.step0 = obs * S, B.nsteps = B.nobs * S;
    B.col0 = B.first ? 0 : V0 + B.step0 * V;
    B.ncols = B.nsteps * V + (B.first ? V0 : 0);
    row += B.nrows, obs += B.nobs;
    c->hblk[p].push_back(B);
  }
  c->K[p] = (int)sizes.size();
  c->C[p] = row;
}

// A half-batch "view": the same structures with every per-chain array advanced to the half's first chain and B = the
// half's chain count.  Every array is chain-major, so a kernel launched on a view works on that chain range only and
// the two halves of a step touch disjoint memory (their active-chain counters included).
using ViewSave = ChainView;
static ViewSave save_view(const chmc_ctx* c) { return *c; }
static void restore_view(chmc_ctx* c, const ViewSave& f) { static_cast<ChainView&>(*c) = f; }
static void set_half(chmc_ctx* c, const ViewSave& f, int h) {
  const size_t c0 = (size_t)c->hc0[h];
  ChainView& v = *c;
  v = f;
  for_each_chain_array(v, c->plan, c->npart_sum, [&](auto*& p, size_t per_chain, int, size_t) {
    if (p) p += c0 * per_chain;
  });
  alias_step_outputs(v, c->d_out, f.sy.B, c0);
  v.sy.B = c->hB[h];
  v.sy.xobs = v.d_xobs;
  if (v.d_yc) v.sy.y = v.d_yc;  // (shared data: stride 0, every view reads d_y)
  v.sy.sigc = v.d_sigc;
  if (v.sy.m0stride) v.sy.m0 = v.d_m0c;  // (shared metric: stride 0, every view reads d_m0)
  v.sy.order = c->d_order_half[c->part][h];
  v.w.n_active = f.w.n_active + 4 * (1 + h);
  use_stream(h);
}

static void select_partition(chmc_ctx* c, int p) {
  c->part = p;
  c->sy.K = c->K[p];
  c->sy.C = c->C[p];
  c->sy.blk = c->d_blk[p];
  c->sy.obs2blk = c->d_obs2blk[p];
  c->sy.order = c->d_order[p];
}

// The instantiation of a context: model type and row slots per block (RM), as the tag type `dispatch` hands to its callee.
template <class M_, int RM_>
struct Inst {
  using M = M_;
  static constexpr int RM = RM_;
};
// (model, varsig, RMt) -> (M, RM): calls f(Inst<M, RM>{}) for the context's instantiation.  The launch sites below are generic
// lambdas (or function templates on <M, RM>) that read the two off the tag.
template <class F>
static void dispatch(const chmc_ctx* ctx, F&& f) {
  const int rmt = ctx->RMt;
  if (ctx->sy.varsig) {  // variable observation noise: dim_u = dim_z + 1
    if (ctx->model == CHMC_MODEL_FHN) {
      if (rmt == 8) f(Inst<FhnVsModel, 8>{});
      else f(Inst<FhnVsModel, 16>{});
    } else {
      if (rmt == 8) f(Inst<SirVsModel, 8>{});
      else f(Inst<SirVsModel, 16>{});
    }
  } else if (ctx->model == CHMC_MODEL_FHN) {
    if (rmt == 7) f(Inst<FhnModel, 7>{});
    else if (rmt == 6) f(Inst<FhnModel, 6>{});
    else if (rmt == 8) f(Inst<FhnModel, 8>{});
    else f(Inst<FhnModel, 16>{});
  } else if (ctx->model == CHMC_MODEL_FHN_NOTEBOOK) {
    if (rmt == 6) f(Inst<FhnNbModel, 6>{});
    else if (rmt == 8) f(Inst<FhnNbModel, 8>{});
    else f(Inst<FhnNbModel, 16>{});
  } else {
    if (rmt == 8) f(Inst<SirModel, 8>{});
    else f(Inst<SirModel, 16>{});
  }
}

// Kernel families, environment switches and the choice of a kernel per pass: chmc_plan.h.  chmc_create decides the plan, every
// entry point refreshes the part that hangs on a per-call switch (CHMC_ENTER), the passes (chmc_passes.inc) switch on it.
static const PartitionPlan& part_plan(const chmc_ctx* c) { return c->plan.part[c->part]; }
static void refresh_plan(chmc_ctx* c) {
  c->plan_in.call = read_switches();
  c->plan = make_plan(c->plan_in);
}
// One function per pass: the only text that differs between the library and the host emulation.
#include "chmc_passes.inc"

extern "C" const char* chmc_last_error(void) { return g_err.c_str(); }
extern "C" const char* chmc_backend(void) { return CHMC_BACKEND_NAME; }

extern "C" int chmc_create(const chmc_config* cfg, chmc_ctx** out) {
  if (!cfg || !out) return fail("chmc_create: null argument");
  if (cfg->model != CHMC_MODEL_FHN && cfg->model != CHMC_MODEL_SIR && cfg->model != CHMC_MODEL_FHN_NOTEBOOK)
    return fail("chmc_create: unknown model id");
  if (cfg->num_obs < 1 || cfg->num_steps_per_obs < 1 || cfg->num_chains < 1) return fail("chmc_create: bad sizes");
  if (!cfg->y_seq) return fail("chmc_create: y_seq is null");
  if (cfg->noisy == 1 && !(cfg->sigma > 0.0)) return fail("chmc_create: noisy observations need sigma > 0");
  if (cfg->noisy < 0 || cfg->noisy > 2) return fail("chmc_create: noisy must be 0 (noiseless), 1 (fixed sigma) or 2 (sigma = generate_sigma(u))");
  if (cfg->noisy == 2 && cfg->model == CHMC_MODEL_FHN_NOTEBOOK)
    return fail("chmc_create: the notebook model has no generate_sigma (noiseless observations)");
  if (cfg->num_obs_per_subseq == 1 && cfg->num_obs > 1)  // the second partition would open with 1 // 2 = 0 observations (:327)
    return fail("chmc_create: num_obs_per_subseq must be at least 2 (or <= 0 / >= num_obs for a single sub-sequence)");
  if (dev_init(cfg->device)) return fail(std::string("chmc_create: ") + g_err);
  chmc_ctx* c = new chmc_ctx();
  c->num_cus = dev_num_cus();
  c->cfg = *cfg;
  c->cfg.y_seq = nullptr;
  c->model = cfg->model;
  memset(c->counters, 0, sizeof(c->counters));
  Sys& sy = c->sy;
  memset(&sy, 0, sizeof(sy));
  const bool fhn = cfg->model == CHMC_MODEL_FHN || cfg->model == CHMC_MODEL_FHN_NOTEBOOK;
  sy.X = fhn ? FhnModel::X : SirModel::X, sy.V = fhn ? FhnModel::V : SirModel::V;
  sy.Z = fhn ? FhnModel::Z : SirModel::Z, sy.V0 = fhn ? FhnModel::V0 : SirModel::V0;
  sy.varsig = cfg->noisy == 2;  // generate_sigma callable (:353-358): u gets the component log sigma
  sy.U = sy.Z + sy.varsig;
  sy.B = cfg->num_chains, sy.T = cfg->num_obs, sy.S = cfg->num_steps_per_obs;
  sy.noisy = cfg->noisy != 0, sy.gaussian = cfg->use_gaussian_splitting != 0;
  sy.dl = cfg->obs_interval / cfg->num_steps_per_obs;
  sy.sigma = cfg->noisy == 1 ? cfg->sigma : 0.0;
  sy.NV = sy.V0 + sy.T * sy.S * sy.V;
  sy.NCOL = sy.NV + (sy.noisy ? sy.T : 0);
  sy.Q = sy.U + sy.NCOL;
  const int R = cfg->num_obs_per_subseq;
  if (R <= 0 || R >= sy.T) {
    c->num_partition = 1;
    build_partition(c, 0, sy.T);
  } else {
    c->num_partition = 2;
    build_partition(c, 0, R);
    build_partition(c, 1, R / 2);
  }
  int rmax = 0, kmax = 0, nobsmax = 1;
  for (int p = 0; p < c->num_partition; ++p) {
    for (auto& b : c->hblk[p]) {
      rmax = b.nrows > rmax ? b.nrows : rmax;
      nobsmax = b.nobs > nobsmax ? b.nobs : nobsmax;
    }
    kmax = c->K[p] > kmax ? c->K[p] : kmax;
  }
  sy.NOBS = nobsmax;
  if (rmax > 16) {
    delete c;
    return fail("chmc_create: blocks with more than 16 constraint rows are not supported");
  }
  c->RMt = rmax <= 8 ? 8 : 16;
  if (fhn && !sy.varsig && (rmax == 6 || (rmax == 7 && cfg->model == CHMC_MODEL_FHN))) c->RMt = rmax;  // R = 5 with noisy (7) / noiseless (6) observations (BASELINE configs 1-3, 5): exact row count, no padded slot
  sy.RM = c->RMt, sy.Kmax = kmax, sy.TRJ = (sy.T * sy.S + CHMC_TPAD * kmax) * sy.X;
  const size_t B = sy.B;
  c->hB[0] = sy.B / 2, c->hB[1] = sy.B - sy.B / 2, c->hc0[0] = 0, c->hc0[1] = sy.B / 2;
  for (int p = 0; p < c->num_partition; ++p) {
    c->d_blk[p] = alloc<BlockDesc>(c, c->K[p]);
    h2d(c->d_blk[p], c->hblk[p].data(), sizeof(BlockDesc) * c->K[p]);
    std::vector<int> o2b(sy.T);
    for (int b = 0; b < c->K[p]; ++b)
      for (int t = 0; t < c->hblk[p][b].nobs; ++t) o2b[c->hblk[p][b].obs0 + t] = b;
    c->d_obs2blk[p] = alloc<int>(c, sy.T);
    h2d(c->d_obs2blk[p], o2b.data(), sizeof(int) * sy.T);
    // Work order of the wave-per-(chain, block) kernels.  Workgroups are dispatched in index order and every SIMD
    // holds one of these wavefronts, so a launch is a list schedule: with the blocks in (chain, block) order the
    // short first / last sub-sequences of partition 1 land anywhere and the last round runs a few long blocks on an
    // otherwise idle chip (partition-1 steps were 7 % slower than partition-0 steps for the same total work).
    // Longest-processing-time-first puts the short blocks at the end, where they fill the tail.
    c->d_order[p] = upload_work_order(c, c->hblk[p], sy.B, 0);
    // the same list schedule for the chains of one half-batch
    for (int h = 0; h < 2; ++h) c->d_order_half[p][h] = upload_work_order(c, c->hblk[p], c->hB[h], 1);
  }
  {
    PlanInput& in = c->plan_in;
    in.rmt = c->RMt, in.num_partition = c->num_partition, in.K[0] = c->K[0], in.K[1] = c->K[c->num_partition - 1];
    in.longest = 0;
    for (int p = 0; p < c->num_partition; ++p)
      for (auto& bl : c->hblk[p]) in.longest = bl.nsteps > in.longest ? bl.nsteps : in.longest;
    in.chain_steps = sy.T * sy.S, in.s_tiles8 = sy.S % 8 == 0;
    in.V = sy.V, in.even_dims = !((sy.Q | sy.U | sy.V0 | sy.NV) & 1), in.gaussian = sy.gaussian;
    in.wave_kernels = kWaveKernels;
    in.sw = in.call = read_switches();
    c->plan = make_plan(in);
  }
  {
    // CHMC_HALVES=2: run every leapfrog step as two overlapped half-batches.  Bitwise equal to the one-batch step, but
    // measured SLOWER at 256 chains per GPU (26.0 k against 28.4 k steps/s: the forward scan's trajectory stores stall
    // under the other half's memory traffic, DESIGN.md section 7) and equal at 512, so one batch is the default.
    c->halves = (c->plan_in.sw.halves == 2 && sy.B >= 2) ? 2 : 1;
    // (One 16-row block per chain: the retraction runs per chain in its own workgroup (k_retract_chain), there is no
    // lock-step loop to overlap; one block per chain with the time-parallel scan: a handful of wavefronts per half-batch.
    // Always one batch.)
    if (kmax == 1 && (c->plan.par_scan || c->RMt > 8)) c->halves = 1;
  }
  c->d_y = alloc<double>(c, sy.T);
  h2d(c->d_y, cfg->y_seq, sizeof(double) * sy.T);
  c->npart_sum = rowsum_groups(sy.Q);
  alloc_chain_arrays(c);  // every per-chain array: chmc_layout.h
  // the comparator target's time-parallel scan (nld_core) takes a row's work trajectory as its guess: the first call of a
  // context sees the cold guess chmc_adam_begin_tries_device deals out (zeros), not whatever the allocation held
  dev_zero(c->w.trajw, sizeof(double) * B * sy.TRJ);
  sy.y = c->d_y, sy.xobs = c->d_xobs;
  c->d_out = alloc<unsigned long long>(c, step_outputs_words(B));
  alias_step_outputs(*c, c->d_out, B, 0);
  Work& w = c->w;
  w.n_active = alloc<int>(c, 12);  // [batch | half 0 | half 1] x 4 round slots
  {
    double* z = alloc<double>(c, 256);
    dev_zero(z, sizeof(double) * 256);
    w.zeros = z;
  }
  w.nfallback = alloc<int>(c, 128);  // [0] sequential fallbacks; [1 + sweeps + 16 (gsel - 1)] histogram of sweeps to convergence;
  dev_zero(w.nfallback, sizeof(int) * 128);  // [48 .. 79] phase ticks of the per-chain kernels in the diagnostic build (CHMC_RETRACT_PROF)
  c->d_ham = alloc<double>(c, B * 4);  // [B][3] Hamiltonian terms; chmc_adam_objective_device: values [B] + statistics [B][3]
  select_partition(c, 0);
  if (dev_sync()) {
    std::string e = g_err;
    chmc_destroy(c);
    return fail("chmc_create: " + e);
  }
  *out = c;
  return 0;
}

extern "C" int chmc_comm_destroy(chmc_ctx* ctx);
extern "C" void chmc_destroy(chmc_ctx* c) {
  if (!c) return;
  if (c->comm) chmc_comm_destroy(c);  // a communicator of chmc_comm_init is released with the context
  for (void* p : c->allocs) dev_free(p);
  delete c;
}

extern "C" int chmc_get_dims(const chmc_ctx* c, int* d) {
  if (!c || !d) return fail("chmc_get_dims: null argument");
  const Sys& s = c->sy;
  int v[16] = {s.B, s.Q, s.NV, s.U, s.X, s.T, s.S, c->num_partition, s.RM, s.Kmax,
               c->C[0], c->num_partition > 1 ? c->C[1] : 0, c->K[0], c->num_partition > 1 ? c->K[1] : 0, s.V, s.V0};
  memcpy(d, v, sizeof(v));
  return 0;
}
extern "C" int chmc_get_blocks(const chmc_ctx* c, int p, int* out) {
  if (!c || !out || p < 0 || p >= c->num_partition) return fail("chmc_get_blocks: bad argument");
  memcpy(out, c->hblk[p].data(), sizeof(BlockDesc) * c->K[p]);
  return 0;
}
extern "C" int chmc_get_counters(const chmc_ctx* c, long long* out8) {
  if (!c || !out8) return fail("chmc_get_counters: null argument");
  memcpy(out8, c->counters, sizeof(c->counters));  // host-side counts only: no device access, no synchronisation
  return 0;
}

// ------------------------------------------------------------------------------------------------------------
static void begin_all(chmc_ctx* c, const double* d_dt, const int* d_active, double dt_scale = 1.0) {
  launch(KBegin{c->w, d_active, d_dt, dt_scale}, c->sy.B);
}

// jacob_constr_blocks + chol_gram_blocks + log_det + grad_log_det at slot `which` (the one value_and_grad call
// of grad_log_det_sqrt_gram that fills all of the reference's state caches, :1173-1184)
// traj_guess: 3 when work.trajw holds the trajectory of the retraction's last iterate towards this point (the
// time-parallel scan then needs a single sweep), 0 when nothing close is known (sequential scan)
// With the compact rows the state sweeps that need no stored rows do not write the rows of the step columns at all
// (PartitionPlan::rebuild_rows): the per-operator entry points that hand rows to the caller rebuild them on demand.
static void ensure_rows(chmc_ctx* c) {
  if (!part_plan(c).rebuild_rows || c->rows_fresh) return;
  const Sys& sy = c->sy;
  dispatch(c, [&](auto inst) {
    using M = typename decltype(inst)::M;
    launch(KRowsFromPB<decltype(inst)::RM, M::X, M::V>{sy, c->sl}, (long)sy.B * sy.T * sy.S, 2);
  });
  c->rows_fresh = true;
}
static void state_eval_core(chmc_ctx* c, int which, bool with_grad = true, int traj_guess = 0) {
  const Sys& sy = c->sy;
  c->rows_fresh = false;
  dispatch(c, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    fwd<M, RM>(c, which, 0, 0, 1, traj_guess);
    state_sweep<M, RM>(c, which);
    launch(KStateChain<M>{sy, c->sl, c->w, which}, sy.B);
    if (!with_grad) return;  // an inner h2-flow step that is not the last needs J and the Gram factors only (mici _step_b)
    gld_sweeps<M, RM>(c, which);
    launch(KGldChain<M>{sy, c->sl, c->w, which}, sy.B);
  });
  c->counters[0]++, c->counters[1]++, c->counters[3]++, c->counters[4] += with_grad ? 1 : 0;
}

static void project_momentum(chmc_ctx* c, int which, int vsel, int psel);
// Everything the reference caches on a state (state_eval_core) plus the projected kick direction
// pg = P(q) dh1_dpos(q).  A(h): p <- P(q)[p - h dh1_dpos(q)] (mici ConstrainedLeapfrogIntegrator._step_a) is linear in
// p and P is idempotent, so for a momentum that is already tangent at q it equals p - h pg: with pg attached to the
// state, a leapfrog step needs ONE pass over the stored Jacobian rows for its momentum projections (at the new
// point, shared between P p and pg) instead of three.
static void state_eval(chmc_ctx* c, int which) {
  const Sys& sy = c->sy;
  state_eval_core(c, which);
  launch(KInitPg{sy, c->sl, c->w, which}, (long)sy.B * sy.Q, 8);
  project_momentum(c, which, 4, 3);
}
// P(q) applied in place to the slot's momentum and to pg (initialised to dh1_dpos) in one pass over the Jacobian rows
// fix_in_jw / flow_rev: the step's momentum correction / reverse flow ride in this pass (KernelPlan::mom_fix_in_jp,
// rev_flow_in_update)
// fwd_qb: with flow_rev, the forward-flowed point of the next step as well (KUpdatePB::fwd_qb, paired retractions)
static void project_momentum_and_kick_direction(chmc_ctx* c, int which, bool init_pg, bool fix_in_jw = false,
                                                bool flow_rev = false, double* fwd_qb = nullptr, double fwd_hfrac = 0.0) {
  const Sys& sy = c->sy;
  if (init_pg) launch(KInitPg{sy, c->sl, c->w, which}, (long)sy.B * sy.Q, 8);
  project_pair(c, which, fix_in_jw, flow_rev, fwd_qb, fwd_hfrac);
}

// p -= J^T G^-1 J p with J, G of slot `which`; p selected by (vsel, psel) (project_onto_cotangent_space :1243-1254)
static void project_momentum(chmc_ctx* c, int which, int vsel, int psel) {
  const Sys& sy = c->sy;
  dispatch(c, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    jw<M, RM>(c, which, vsel | 256, c->plan.rows == RowsCompact);
    launch(KSymBlk<M, RM>{sy, c->sl, c->w, which, 0}, (long)sy.B * sy.K, 9);
    solve_chain<M, RM, 1, 1>(sy, c->sl, c->w, which, 0, psel);
    jt_lambda<M, RM, 1>(c, which, 0, psel);
  });
}

// One Newton / quasi-Newton iteration (:1023-1045, :1088-1117) in two parts.  prev: slot with J(q_prev) and its factors;
// qsel 0: iterate is the other slot's q, 1: work.qb.
// iteration_scan: the forward scan of the iterate (constraint values; Newton: its trajectory into work.trajw).
// use_nw 1: the chains of the loop (work.nw).
static void iteration_scan(chmc_ctx* c, int newton, int prev, int qsel, int fwd_guess, int use_nw) {
  dispatch(c, [&](auto inst) {
    c->diag[7] += fwd<typename decltype(inst)::M, decltype(inst)::RM>(c, prev ^ 1, qsel, use_nw, newton ? 2 : 0, fwd_guess);
  });
}
// ... of the iterates of two problems with the same (prev, qsel), c->w and w1, in one launch
static void iteration_scan_pair(chmc_ctx* c, int newton, int prev, int qsel, const Work& w1) {
  dispatch(c, [&](auto inst) {
    c->diag[7] += fwd_pair<typename decltype(inst)::M, decltype(inst)::RM>(c, w1, prev ^ 1, qsel, newton ? 2 : 0);
  });
  c->diag[6]++;
}
// iteration_after_scan: Jacobian sweep of the iterate against the previous point's rows, block factorisations, Woodbury
// solve, J^T lambda update of the iterate (masked by work.nw == 1)
// (Tried and rejected, round 3: KCheck riding on the update pass through a last-workgroup ticket -- 5 launches per round instead
// of 6, but update 116 -> 177 us per launch and 44.8 k -> 41.9 k steps/s; that code was removed, see docs/history.md.)
static void iteration_after_scan(chmc_ctx* c, int newton, int prev, int qsel) {
  const Sys& sy = c->sy;
  dispatch(c, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    bool solved = false;  // the sweep has solved the chain's core system and formed lambda and mu_F as well
    if (newton) {
      solved = newton_sweep<M, RM>(c, prev, qsel);
      if (!solved) solve_chain<M, RM, 0, 0>(sy, c->sl, c->w, prev, qsel, 0);
    } else {
      launch(KSymBlk<M, RM>{sy, c->sl, c->w, prev, 1}, (long)sy.B * sy.K, 9);
      solve_chain<M, RM, 1, 0>(sy, c->sl, c->w, prev, qsel, 0);
    }
    jt_lambda<M, RM, 0>(c, prev, qsel, 0, solved);
  });
}
// ... of a Newton round of two problems with the same (prev, qsel), c->w and w1, every pass one launch for both
// (KernelPlan::pair_passes)
static void iteration_after_scan_pair(chmc_ctx* c, int prev, int qsel, const Work& w1) {
  dispatch(c, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    newton_sweep_pair<M, RM>(c, w1, prev, qsel);
    jt_lambda_pair<M, RM>(c, w1, prev, qsel);
  });
  c->diag[9]++;
}

// The solver of a retraction as the entry points receive it (include/chmc.h)
struct Solver {
  int newton;  // 1: Newton, 0: quasi-Newton
  double ctol, ptol, dtol;
  int max_iters;
};

// One set of chains in the lock-step loop below: the whole batch, a half-batch, or one of two paired retractions.
struct Problem {
  const ViewSave* view = nullptr;  // a half-batch: set_half(c, *view, half) makes it the active view, with its stream and its
  int half = 0;                    // n_active slots
  const Work* work = nullptr;      // a paired problem: this Work becomes c->w
  int* iters = nullptr;            // where a chain's iteration count is added when its loop ends (KCheck, KNewtonEnd; KAddIters):
  int count_dir = -1;              // this array, or else the ACTIVE view's d_itf (0) / d_itb (1); -1: nowhere
  int dir = -1;                    // its index into proj_rounds / proj_stable (0 forward, 1 reverse); -1: never predicts
};

// Newton / quasi-Newton loop (:999-1135) of n = 1 or 2 problems, every chain of a problem in lock step, the problems in lock
// step on the host.  Leaves per-chain iters / err / ndq / nstat in each problem's work arrays.
//   one problem: the active view (whole batch) on the current stream;
//   two half-batch views: parts of one batch, each on its own stream (chmc_leapfrog_step with two halves);
//   two paired problems (`mergeable`): the reverse retraction of step i on c->w and the forward retraction of step i + 1 on
//     c->pw (its iterate pw.qb holds the forward-flowed point, KPairFlow), on the one stream.  Both are loops against the
//     proposal slot's point (prev = 1) on an iterate in a work array (qsel = 1), so one forward scan serves both.
// Round `it`, in this order:
//   1. every problem whose prediction is due (below) waits for its count of round it - 1 and stops if nobody is left;
//   2. mergeable and both still iterating: ONE forward scan for both (iteration_scan_pair) and, where the plan has pair_passes
//      and the loop is Newton's, sweep, solve and update one launch per pass for both (iteration_after_scan_pair);
//   3. per problem still iterating, in index order: its own scan and passes unless 2. served it, then its check (KCheck),
//      which from round 1 on publishes the count of chains still iterating to the problem's pinned poll slot 2 i + (it & 1)
//      from its last workgroup (no copy packet behind it; A/B on one box, three interleaved runs each: configs[1]
//      46.3-46.8 k -> 46.7-47.1 k steps/s, SIR unchanged).  KCheck also adds a finished loop's iteration count to the step's
//      counter and clears the next round's counter: no memset between the rounds;
//   4. per problem, the count of round it - 1 is examined while the device runs round it.
// Every kernel of a round is masked per chain (work.nw), so a round enqueued for chains that have all finished is a handful
// of empty launches.  The host therefore never waits for the count of round `it` before round `it + 1` is queued.  (Waiting
// first costs a 30 us stream bubble per round.)  The first count examined is that of the second round: no chain satisfies the
// position tolerance after one update of an h2-flowed point.
// Speculation has a price when the batch is regular: the round enqueued behind the last real one is empty (six launches).
// When the last few retractions of a problem's direction all ended after the same number of rounds (FitzHugh-Nagumo at
// configs[1]: always 4), the host does not speculate at that point: it waits for that round's count first and stops if nobody
// is left (one host wake-up instead of an empty round: the same 30 us, but 12 launches fewer per step and the launched rounds
// equal the rounds that had work).  Irregular batches (SIR) keep speculating; half-batches never predict and leave
// proj_rounds / proj_stable alone.  A predicting problem that ends with fewer than `expect` rounds records `expect`, whichever
// read-back ended it: the one-batch loop's rule, under which every recorded benchmark ran, so a paired problem is enqueued for
// exactly the rounds a loop of its own would have been.  (Whether recording the shorter count is the better rule is a
// separate question.)
// Counters: diag[8] counts enqueued rounds per problem; counters[6] a round that had work, once per paired problem but once
// for a batch or its two halves.
static void run_lockstep(chmc_ctx* c, const Solver& s, int prev, int qsel, const Problem* pr, int n, bool mergeable) {
  const Sys& sy = c->sy;
  auto enter = [&](int i) {
    if (pr[i].view) set_half(c, *pr[i].view, pr[i].half);
    if (pr[i].work) c->w = *pr[i].work;
  };
  // (read at every use: d_itf / d_itb are those of the half-batch view that is active then)
  auto iters_dst = [&](int i) {
    const int dir = pr[i].count_dir;
    return pr[i].iters ? pr[i].iters : dir < 0 ? nullptr : (dir ? c->d_itb : c->d_itf);
  };
  const bool one_batch = !mergeable;  // the problems are parts of one batch: a round counts once
  bool done[2] = {true, true}, predict[2] = {false, false};
  int rounds_done[2] = {0, 0};
  for (int i = 0; i < n; ++i) {
    enter(i);
    if (sy.B > 0) launch(KNewtonBegin{c->w}, sy.B);
    done[i] = sy.B <= 0;
    predict[i] = pr[i].dir >= 0 && c->proj_stable[pr[i].dir] >= 3 && c->proj_rounds[pr[i].dir] >= 2;
  }
  // Time-parallel scans with one block per chain do not wait for a chain they cannot settle within a few sweeps: the chain
  // sits the round out (mask 2, k_fwd_par) and its scan goes on in the next round's launch.  Rounds are therefore not
  // iterations: the loop gets up to 64 / CHMC_PAR_MAXS_ROUND + 1 rounds per iteration (KCheck enforces max_iters per chain).
  const bool carry = c->plan.fwd == FwdPar && sy.K == 1;
  const int max_rounds = carry ? 12 * (s.max_iters + 1) : s.max_iters;
  for (int it = 0; it < max_rounds && !(done[0] && done[1]); ++it) {
    for (int i = 0; i < n; ++i)  // (the count of round it - 1 was requested in that round)
      if (!done[i] && predict[i] && it >= c->proj_rounds[pr[i].dir] && poll_end(2 * i + ((it - 1) & 1)) == 0) done[i] = true;
    if (done[0] && done[1]) break;
    c->round = it;
    const bool both = mergeable && !done[0] && !done[1];
    const bool merged = both && s.newton && c->plan.pair_passes;
    if (both) {
      enter(0);
      iteration_scan_pair(c, s.newton, prev, qsel, *pr[1].work);
      if (merged) iteration_after_scan_pair(c, prev, qsel, *pr[1].work);
    }
    int worked = 0;
    for (int i = 0; i < n; ++i) {
      if (done[i]) continue;
      enter(i);
      // (first round: the state's own trajectory is the scan's guess; later ones: the previous iterate's)
      if (!both) iteration_scan(c, s.newton, prev, qsel, it == 0 ? 2 : 1, 1);
      if (!merged) iteration_after_scan(c, s.newton, prev, qsel);
      const KCheck chk{c->w, s.ctol, s.ptol, s.dtol, s.max_iters, sy.B, iters_dst(i), it & 3};
      if (it >= 1) launch_publish(chk, sy.B, c->w.n_active + (it & 3), 2 * i + (it & 1));
      else launch(chk, sy.B);
      c->diag[8]++;
      if (it == 0) worked++;
    }
    for (int i = 0; i < n && it >= 1; ++i) {
      if (done[i]) continue;
      if (it >= 2 && poll_end(2 * i + ((it - 1) & 1)) == 0) {  // round it - 1 left no chain active: round it was empty
        done[i] = true;  // (its pending read-back lands before any later one of the same stream: no need to wait for it)
        continue;
      }
      worked++;
      rounds_done[i] = it + 1;
      if (it + 1 >= max_rounds) poll_end(2 * i + (it & 1));  // drain the last read-back before the slots are reused
    }
    c->counters[6] += one_batch ? worked > 0 : worked;
  }
  for (int i = 0; i < n; ++i) {
    if (pr[i].dir >= 0) {
      int& expect = c->proj_rounds[pr[i].dir];
      int& stable = c->proj_stable[pr[i].dir];
      if (predict[i] && done[i] && rounds_done[i] < expect) rounds_done[i] = expect;
      stable = rounds_done[i] == expect ? stable + 1 : 0;
      expect = rounds_done[i];
    }
    enter(i);  // a chain the host left in the loop is a failure, never a silent success
    if (sy.B > 0) launch(KNewtonEnd{c->w, iters_dst(i)}, sy.B);
  }
  c->round = 0;
}

// One 16-row block per chain on the compact rows (the SIR single-block layout): the whole Newton retraction of a chain in one
// launch, one workgroup per chain (k_retract_chain, chmc_retract.h) -- no rounds, no read-backs, every chain iterates exactly
// as long as it needs.  The batched path of these layouts does the same per-chain arithmetic bit for bit (k_fwd_par with the
// same segmentation, k_newton_comb_wg, k_jw_pb_wg: tests/test_hip_parity.py::test_per_chain_kernels_equal_the_batched_path_
// bitwise), so which of the two runs is a pure scheduling decision:
// chain_kernel_waves (chmc_plan.h).
static int retract_waves(const chmc_ctx* c, int newton, const void* views) {
  return chain_kernel_waves(c->plan, part_plan(c).retract_chain && chain_kernel_model(c), c->sy.B, c->num_cus, newton != 0,
                            views != nullptr);
}
// ... and whole leapfrog steps -- whole trajectories -- of a chain in one launch (k_traj_chain): the same layouts with the
// interval-parallel 16-row state evaluation, one inner h2-flow step, momenta known to be tangent, one batch.
static int traj_waves(const chmc_ctx* c, int n_inner, int newton) {
  const bool eligible = part_plan(c).traj_chain && chain_kernel_model(c) && n_inner == 1 && c->mom_tangent && c->halves == 1;
  return chain_kernel_waves(c->plan, eligible, c->sy.B, c->num_cus, newton != 0, false);
}
// One retraction of the active view (views == nullptr) or of its two half-batches: the per-chain kernel where the plan has
// one, else the lock-step loop.  count_dir: Problem::count_dir.
static void run_projection(chmc_ctx* c, const Solver& s, int prev, int qsel, const ViewSave* views = nullptr,
                           int count_dir = -1) {
  const Sys& sy = c->sy;
  if (const int waves = retract_waves(c, s.newton, views)) {
    int* const iters_dst = count_dir < 0 ? nullptr : (count_dir ? c->d_itb : c->d_itf);
    dispatch(c, [&](auto inst) {
      retract_chain<typename decltype(inst)::M, decltype(inst)::RM>(waves, (long)sy.B, sy, c->sl, c->w, prev, qsel, s.ctol, s.ptol,
                                                                     s.dtol, s.max_iters, iters_dst);
    });
    c->counters[6]++;  // (one launch that lasts as long as its slowest chain iterates)
    c->diag[2]++;
    return;
  }
  Problem pr[2];
  for (int h = 0; h < 2; ++h) pr[h].view = views, pr[h].half = h, pr[h].count_dir = count_dir, pr[h].dir = views ? -1 : prev & 1;
  run_lockstep(c, s, prev, qsel, pr, views ? 2 : 1, false);
}

// The arrays of the second problem's Work (chmc_ctx::pw), sized as chmc_layout.h sizes their counterparts.  Not in that list:
// only the whole-batch view has them, as with the arrays of the trajectory trees.
static void pair_alloc(chmc_ctx* c) {
  if (c->have_pair) return;
  const Sys& sy = c->sy;
  const size_t B = sy.B, KM = sy.Kmax, RM = sy.RM, U = sy.U, X = sy.X, Z = sy.Z, ivls = KM * sy.NOBS;
  Work& w = c->pw;
  w = c->w;
  auto zeroed = [&](size_t n) {
    double* p = alloc<double>(c, n);
    dev_zero(p, sizeof(double) * n);
    return p;
  };
  w.qb = zeroed(B * sy.Q + CHMC_Q_PAD);
  w.trajw = alloc<double>(c, B * sy.TRJ);
  w.cpad = zeroed(B * KM * RM), w.tpad = alloc<double>(c, B * KM * RM), w.lampad = zeroed(B * KM * RM);
  w.Ew = alloc<double>(c, B * KM * RM * U), w.Cb = alloc<double>(c, B * KM * U * U), w.sb = alloc<double>(c, B * KM * U);
  w.Dw = alloc<double>(c, B * KM * RM * RM), w.JuL = alloc<double>(c, B * KM * RM * U), w.zbP = alloc<double>(c, B * KM * RM * Z);
  if (c->plan.pb_allocated) {
    w.muF = alloc<double>(c, B * ivls * X);
    w.ivl = alloc<double>(c, B * ivls * (2 * X * X + X * Z));
  }
  w.err = alloc<double>(c, B), w.ndq = alloc<unsigned long long>(c, B);
  w.iters = alloc<int>(c, B), w.nw = alloc<int>(c, B), w.nstat = alloc<int>(c, B), w.ok = alloc<int>(c, B), w.status = alloc<int>(c, B);
  w.n_active = alloc<int>(c, 4);  // its own round slots
  c->d_itf_next = alloc<int>(c, B);
  c->have_pair = true;
}

// The reverse retraction of step i (problem 0: that of run_projection(.., 1, 1, nullptr, 1), on c->w) beside the forward
// retraction of step i + 1 (problem 1, on c->pw, counting into d_itf_next) as the two mergeable problems of run_lockstep.
// Returns on problem 0's Work.
static void run_projection_pair(chmc_ctx* c, const Solver& s) {
  const Work wk[2] = {c->w, c->pw};
  Problem pr[2];
  pr[0].work = &wk[0], pr[0].count_dir = 1, pr[0].dir = 1;
  pr[1].work = &wk[1], pr[1].iters = c->d_itf_next, pr[1].dir = 0;
  run_lockstep(c, s, 1, 1, pr, 2, true);
  c->w = wk[0];
}

static int check_ctx(const chmc_ctx* c, const char* fn) {
  if (!c) return fail(std::string(fn) + ": null context");
  if (c->owner != std::this_thread::get_id())
    return fail(std::string(fn) + ": a context must be driven by the host thread that created it");
  return 0;
}
#define CHMC_ENTER(fn)                 \
  if (check_ctx(ctx, fn)) return -1;   \
  refresh_plan(ctx);                   \
  use_stream(-1);                      \
  if (dev_set(ctx->cfg.device)) return fail(std::string(fn) + ": " + g_err);
#define CHMC_LEAVE(fn)                                                 \
  if (dev_sync()) return fail(std::string(fn) + ": " + g_err);        \
  return 0;

// diagnostics (include/chmc.h): [0 .. 63] the counters of the time-parallel forward scan (see chmc_create),
// [64 ..] launches by kernel family
extern "C" int chmc_get_diagnostics(chmc_ctx* ctx, long long* out80) {
  CHMC_ENTER("chmc_get_diagnostics")
  if (!out80) return fail("chmc_get_diagnostics: null output");
  int ps[80];
  d2h(ps, ctx->w.nfallback, sizeof(ps));
  for (int i = 0; i < 64; ++i) out80[i] = ps[i];
  for (int i = 0; i < 16; ++i) out80[64 + i] = ctx->diag[i];
#ifdef CHMC_RETRACT_PROF
  for (int i = 4; i < 16; ++i) out80[64 + i] = ps[64 + i - 4];  // diagnostic build: phase ticks of k_traj_chain
#endif
  CHMC_LEAVE("chmc_get_diagnostics")
}

extern "C" int chmc_set_state(chmc_ctx* ctx, const double* q, const double* p, const double* x_obs, int partition) {
  CHMC_ENTER("chmc_set_state")
  if (!q || !x_obs) return fail("chmc_set_state: q and x_obs_seq are required");
  if (partition < 0 || partition >= ctx->num_partition) return fail("chmc_set_state: partition out of range");
  const Sys& sy = ctx->sy;
  const size_t n = sizeof(double) * (size_t)sy.B * sy.Q;
  dev_zero(ctx->sl.cur, sizeof(int) * sy.B);
  h2d(ctx->sl.q[0], q, n);
  if (p) h2d(ctx->sl.p[0], p, n);
  else dev_zero(ctx->sl.p[0], n);
  h2d(ctx->d_xobs, x_obs, sizeof(double) * (size_t)sy.B * sy.T * sy.X);
  select_partition(ctx, partition);
  begin_all(ctx, nullptr, nullptr);
  state_eval(ctx, 0);
  ctx->have_state = true;
  ctx->mom_tangent = p == nullptr;  // a zero momentum is tangent, a given one is the caller's business
  CHMC_LEAVE("chmc_set_state")
}

extern "C" int chmc_init_linear_interpolation(chmc_ctx* ctx, const double* u, const double* v_0,
                                              const double* x_obs_seq_init, int partition) {
  CHMC_ENTER("chmc_init_linear_interpolation")
  if (!u || !v_0 || !x_obs_seq_init) return fail("chmc_init_linear_interpolation: u, v_0 and x_obs_seq_init are required");
  if (partition < 0 || partition >= ctx->num_partition)
    return fail("chmc_init_linear_interpolation: partition out of range");
  const Sys& sy = ctx->sy;
  // staging in work buffers that the state evaluation below does not touch before they have been consumed
  double* d_u = ctx->w.pb;
  double* d_v0 = ctx->w.pb + (size_t)sy.B * sy.U;
  h2d(d_u, u, sizeof(double) * (size_t)sy.B * sy.U);
  h2d(d_v0, v_0, sizeof(double) * (size_t)sy.B * sy.V0);
  h2d(ctx->d_xobs, x_obs_seq_init, sizeof(double) * (size_t)sy.B * sy.T * sy.X);
  dev_zero(ctx->sl.cur, sizeof(int) * sy.B);
  dev_zero(ctx->sl.p[0], sizeof(double) * (size_t)sy.B * sy.Q);
  if (ctx->model == CHMC_MODEL_FHN)
    launch(KInitInterp<FhnModel>{sy, ctx->sl.q[0], d_u, d_v0, ctx->d_xobs}, (long)sy.B * sy.T * sy.S);
  else if (ctx->model == CHMC_MODEL_FHN_NOTEBOOK)
    launch(KInitInterp<FhnNbModel>{sy, ctx->sl.q[0], d_u, d_v0, ctx->d_xobs}, (long)sy.B * sy.T * sy.S);
  else
    launch(KInitInterp<SirModel>{sy, ctx->sl.q[0], d_u, d_v0, ctx->d_xobs}, (long)sy.B * sy.T * sy.S);
  select_partition(ctx, partition);
  begin_all(ctx, nullptr, nullptr);
  state_eval(ctx, 0);
  ctx->have_state = true;
  ctx->mom_tangent = true;  // zero momentum
  CHMC_LEAVE("chmc_init_linear_interpolation")
}

// gather the current state slot of every chain into contiguous device buffers (work.qb / work.pb)
struct KGatherState {
  Sys sy;
  Slots sl;
  double *qo, *po;
  CHMC_HD void operator()(int tid) const {
    const int c = tid / sy.Q;
    const int s = sl.cur[c];
    if (qo) qo[tid] = pick(sl.q, s)[tid];
    if (po) po[tid] = pick(sl.p, s)[tid];
  }
};
struct KScatterMom {
  Sys sy;
  Slots sl;
  const double* pi;
  CHMC_HD void operator()(int tid) const {
    const int c = tid / sy.Q;
    sl.p[sl.cur[c]][tid] = pi[tid];
  }
};
struct KGatherSlotVec {  // per-chain slot-selected copy of a [B][stride] array
  Slots sl;
  const double* a0;
  const double* a1;
  double* out;
  long stride;
  CHMC_HD void operator()(int tid) const {
    const int c = (int)(tid / stride);
    out[tid] = (sl.cur[c] ? a1 : a0)[tid];
  }
};

extern "C" int chmc_get_state(chmc_ctx* ctx, double* q, double* p, double* x_obs, int* partition) {
  CHMC_ENTER("chmc_get_state")
  const Sys& sy = ctx->sy;
  const size_t n = sizeof(double) * (size_t)sy.B * sy.Q;
  launch(KGatherState{sy, ctx->sl, q ? ctx->w.qb : nullptr, p ? ctx->w.pb : nullptr}, (long)sy.B * sy.Q);
  if (q) d2h(q, ctx->w.qb, n);
  if (p) d2h(p, ctx->w.pb, n);
  if (x_obs) d2h(x_obs, ctx->d_xobs, sizeof(double) * (size_t)sy.B * sy.T * sy.X);
  if (partition) *partition = ctx->part;
  CHMC_LEAVE("chmc_get_state")
}
// Per-chain observations: d_yc [B][T] and d_sigc [B] are entries of the per-chain list (chmc_layout.h) that no context has
// until this call; afterwards Sys::y strides by T and sigma_at reads the chain's own value.
extern "C" int chmc_set_observations(chmc_ctx* ctx, const double* y_seq, const double* sigma) {
  CHMC_ENTER("chmc_set_observations")
  if (!y_seq) return fail("chmc_set_observations: y_seq is null");
  Sys& sy = ctx->sy;
  if (sigma) {
    if (ctx->cfg.noisy != 1)
      return fail("chmc_set_observations: a per-chain sigma needs a context with a fixed noise level (noisy == 1)");
    for (int c = 0; c < sy.B; ++c)
      if (!(sigma[c] > 0.0)) return fail("chmc_set_observations: every sigma must be > 0");
  }
  ensure_array(ctx, ctx->d_yc);
  h2d(ctx->d_yc, y_seq, sizeof(double) * (size_t)sy.B * sy.T);
  sy.y = ctx->d_yc, sy.ystride = sy.T;
  if (sigma) {
    ensure_array(ctx, ctx->d_sigc);
    h2d(ctx->d_sigc, sigma, sizeof(double) * (size_t)sy.B);
    sy.sigc = ctx->d_sigc;
  }
  // the constraint changed: nothing cached on the chain states holds any more
  ctx->have_state = ctx->have_tree = ctx->pair_ready = ctx->rows_fresh = false;
  ctx->mom_tangent = ctx->snap_tangent = false;
  CHMC_LEAVE("chmc_set_observations")
}
extern "C" int chmc_get_observations(chmc_ctx* ctx, double* y_seq, double* sigma) {
  CHMC_ENTER("chmc_get_observations")
  const Sys& sy = ctx->sy;
  const size_t B = sy.B, T = sy.T;
  if (y_seq) {
    if (ctx->d_yc) {
      d2h(y_seq, ctx->d_yc, sizeof(double) * B * T);
    } else {  // the shared sequence, once per chain
      d2h(y_seq, ctx->d_y, sizeof(double) * T);
      for (size_t c = 1; c < B; ++c) memcpy(y_seq + c * T, y_seq, sizeof(double) * T);
    }
  }
  if (sigma) {
    if (ctx->d_sigc) d2h(sigma, ctx->d_sigc, sizeof(double) * B);
    else std::fill(sigma, sigma + B, sy.sigma);  // (0 without a fixed noise level: noiseless, or exp(u[Z]))
  }
  CHMC_LEAVE("chmc_get_observations")
}

extern "C" int chmc_get_state_device(chmc_ctx* ctx, void* q_dev, void* p_dev) {
  CHMC_ENTER("chmc_get_state_device")
  const Sys& sy = ctx->sy;
  launch(KGatherState{sy, ctx->sl, (double*)q_dev, (double*)p_dev}, (long)sy.B * sy.Q);
  CHMC_LEAVE("chmc_get_state_device")
}
extern "C" int chmc_set_momentum(chmc_ctx* ctx, const double* p) {
  CHMC_ENTER("chmc_set_momentum")
  if (!p) return fail("chmc_set_momentum: null momentum");
  const Sys& sy = ctx->sy;
  h2d(ctx->w.pb, p, sizeof(double) * (size_t)sy.B * sy.Q);
  launch(KScatterMom{sy, ctx->sl, ctx->w.pb}, (long)sy.B * sy.Q);
  ctx->mom_tangent = false;
  CHMC_LEAVE("chmc_set_momentum")
}
extern "C" int chmc_set_momentum_device(chmc_ctx* ctx, const void* p_dev) {
  CHMC_ENTER("chmc_set_momentum_device")
  if (!p_dev) return fail("chmc_set_momentum_device: null momentum");
  const Sys& sy = ctx->sy;
  launch(KScatterMom{sy, ctx->sl, (const double*)p_dev}, (long)sy.B * sy.Q);
  ctx->mom_tangent = false;
  CHMC_LEAVE("chmc_set_momentum_device")
}

// metric = blockdiag(M_0, identity) (sde/mici_extensions.py:303-315); see include/chmc.h
// One chain's table h [3 U U + 1] = M_0, M_0^-1, lower Cholesky factor, log det(M_0) / 2 from M0 [U][U]; null, or what is
// wrong with the matrix.
static const char* metric_table(const double* M0, int U, double* h) {
  double* Mh = h;
  double* W = Mh + U * U;
  double* L = W + U * U;
  for (int i = 0; i < U * U; ++i) Mh[i] = M0[i], L[i] = 0.0;
  for (int i = 0; i < U; ++i)
    for (int j = 0; j < i; ++j)
      if (!(std::fabs(M0[i * U + j] - M0[j * U + i]) <= 1e-12 * (std::fabs(M0[i * U + i]) + std::fabs(M0[j * U + j]))))
        return "is not symmetric";
  double hld = 0.0;
  for (int j = 0; j < U; ++j) {  // lower Cholesky factor
    double d = M0[j * U + j];
    for (int k = 0; k < j; ++k) d -= L[j * U + k] * L[j * U + k];
    if (!(d > 0.0)) return "is not positive definite";
    L[j * U + j] = std::sqrt(d);
    hld += std::log(L[j * U + j]);
    for (int i = j + 1; i < U; ++i) {
      double t = M0[i * U + j];
      for (int k = 0; k < j; ++k) t -= L[i * U + k] * L[j * U + k];
      L[i * U + j] = t / L[j * U + j];
    }
  }
  for (int c = 0; c < U; ++c) {  // M_0^-1, column by column
    double y[8];
    for (int i = 0; i < U; ++i) {
      double t = (i == c) ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) t -= L[i * U + k] * y[k];
      y[i] = t / L[i * U + i];
    }
    for (int i = U - 1; i >= 0; --i) {
      double t = y[i];
      for (int k = i + 1; k < U; ++k) t -= L[k * U + i] * W[k * U + c];
      W[i * U + c] = t / L[i * U + i];
    }
  }
  h[3 * U * U] = hld;
  return nullptr;
}
// the metric changed: tangency is with respect to it, and the factors, log-determinant, gradient and kick direction of the
// current state depend on M_0
static void metric_changed(chmc_ctx* ctx) {
  ctx->mom_tangent = false;
  if (ctx->have_state) {
    begin_all(ctx, nullptr, nullptr);
    state_eval(ctx, 0);
  }
}
extern "C" int chmc_set_metric(chmc_ctx* ctx, const double* M0) {
  CHMC_ENTER("chmc_set_metric")
  Sys& sy = ctx->sy;
  const int U = sy.U;
  if (!M0) {
    sy.m0 = nullptr, sy.m0stride = 0;
  } else {
    if (sy.gaussian) return fail("chmc_set_metric: only the identity metric can be used with Gaussian splitting");
    if (U > 8) return fail("chmc_set_metric: dim_u must be at most 8");
    std::vector<double> h(3 * (size_t)U * U + 1);
    if (const char* what = metric_table(M0, U, h.data())) return fail(std::string("chmc_set_metric: M_0 ") + what);
    if (!ctx->d_m0) ctx->d_m0 = alloc<double>(ctx, h.size());
    h2d(ctx->d_m0, h.data(), sizeof(double) * h.size());
    sy.m0 = ctx->d_m0, sy.m0stride = 0;  // (every chain reads the one table, also after chmc_set_metrics)
  }
  metric_changed(ctx);
  CHMC_LEAVE("chmc_set_metric")
}
// Per-chain block metrics: d_m0c [B][3 U U + 1] is an entry of the per-chain list (chmc_layout.h) that no context has until
// this call; afterwards Sys::m0 strides by the table size and metric_of reads the chain's own table.
extern "C" int chmc_set_metrics(chmc_ctx* ctx, const double* M0) {
  CHMC_ENTER("chmc_set_metrics")
  if (!M0) return fail("chmc_set_metrics: M0 is null");
  Sys& sy = ctx->sy;
  const int U = sy.U;
  if (sy.gaussian) return fail("chmc_set_metrics: only the identity metric can be used with Gaussian splitting");
  if (U > 8) return fail("chmc_set_metrics: dim_u must be at most 8");
  const size_t n = 3 * (size_t)U * U + 1;
  std::vector<double> h((size_t)sy.B * n);
  for (int c = 0; c < sy.B; ++c)
    if (const char* what = metric_table(M0 + (size_t)c * U * U, U, h.data() + c * n))
      return fail("chmc_set_metrics: M_0 of chain " + std::to_string(c) + " " + what);
  ensure_array(ctx, ctx->d_m0c);
  h2d(ctx->d_m0c, h.data(), sizeof(double) * h.size());
  sy.m0 = ctx->d_m0c, sy.m0stride = (int)n;
  metric_changed(ctx);
  CHMC_LEAVE("chmc_set_metrics")
}
extern "C" int chmc_get_metric(chmc_ctx* ctx, double* M0) {
  CHMC_ENTER("chmc_get_metric")
  if (!M0) return fail("chmc_get_metric: null output");
  const Sys& sy = ctx->sy;
  const size_t B = sy.B, UU = (size_t)sy.U * sy.U, n = 3 * UU + 1;
  if (!sy.m0) {  // the identity
    for (size_t c = 0; c < B; ++c)
      for (size_t i = 0; i < UU; ++i) M0[c * UU + i] = (i / sy.U == i % sy.U) ? 1.0 : 0.0;
  } else if (sy.m0stride) {
    std::vector<double> h(B * n);
    d2h(h.data(), ctx->d_m0c, sizeof(double) * h.size());
    for (size_t c = 0; c < B; ++c) memcpy(M0 + c * UU, h.data() + c * n, sizeof(double) * UU);
  } else {  // the shared matrix, once per chain
    d2h(M0, ctx->d_m0, sizeof(double) * UU);
    for (size_t c = 1; c < B; ++c) memcpy(M0 + c * UU, M0, sizeof(double) * UU);
  }
  CHMC_LEAVE("chmc_get_metric")
}

extern "C" int chmc_sample_momentum(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw,
                                    int chain_offset) {
  CHMC_ENTER("chmc_sample_momentum")
  const Sys& sy = ctx->sy;
  launch(KNormalFill{sy, ctx->sl, seed, draw, chain_offset}, (long)sy.B * ((sy.Q + 1) / 2), 8);
  if (sy.m0) launch(KMetricSqrtU{sy, ctx->sl}, sy.B);  // metric.sqrt @ n (:1257)
  begin_all(ctx, nullptr, nullptr);
  project_momentum(ctx, 0, 0, 0);
  ctx->mom_tangent = true;
  CHMC_LEAVE("chmc_sample_momentum")
}

// ---- minimal caller support (SURVEY.md 8f #2): snapshot / restore of chain states for a Metropolis accept step
struct KSnapshot {
  Sys sy;
  Slots sl;
  double *qb, *pb;
  int restore;
  const int* mask;
  CHMC_HD void operator()(int tid) const {
    const int c = tid / sy.Q;
    const int s = sl.cur[c];
    if (!restore) {
      qb[tid] = pick(sl.q, s)[tid];
      pb[tid] = pick(sl.p, s)[tid];
    } else if (mask[c]) {
      pick(sl.q, s)[tid] = qb[tid];
      pick(sl.p, s)[tid] = pb[tid];
    }
  }
};
extern "C" int chmc_snapshot(chmc_ctx* ctx) {
  CHMC_ENTER("chmc_snapshot")
  const Sys& sy = ctx->sy;
  ensure_array(ctx, ctx->d_qbak), ensure_array(ctx, ctx->d_pbak);
  launch(KSnapshot{sy, ctx->sl, ctx->d_qbak, ctx->d_pbak, 0, nullptr}, (long)sy.B * sy.Q, 8);
  ctx->snap_tangent = ctx->mom_tangent;
  CHMC_LEAVE("chmc_snapshot")
}
extern "C" int chmc_restore(chmc_ctx* ctx, const int* mask) {
  CHMC_ENTER("chmc_restore")
  if (!mask) return fail("chmc_restore: null mask");
  if (!ctx->d_qbak) return fail("chmc_restore: no snapshot has been taken");
  const Sys& sy = ctx->sy;
  h2d(ctx->d_act, mask, sizeof(int) * sy.B);
  ctx->last_active_null = true;
  ctx->last_active.clear();
  launch(KSnapshot{sy, ctx->sl, ctx->d_qbak, ctx->d_pbak, 1, ctx->d_act}, (long)sy.B * sy.Q, 8);
  begin_all(ctx, nullptr, ctx->d_act);  // re-evaluate the state caches of the restored chains only
  state_eval(ctx, 0);
  ctx->mom_tangent = ctx->mom_tangent && ctx->snap_tangent;
  CHMC_LEAVE("chmc_restore")
}
extern "C" int chmc_restore_device(chmc_ctx* ctx, const void* q_dev, const void* p_dev, const int* mask,
                                   int momentum_is_tangent) {
  CHMC_ENTER("chmc_restore_device")
  if (!mask || !q_dev || !p_dev) return fail("chmc_restore_device: q_dev, p_dev and mask are required");
  const Sys& sy = ctx->sy;
  h2d(ctx->d_act, mask, sizeof(int) * sy.B);
  ctx->last_active_null = true;
  ctx->last_active.clear();
  launch(KSnapshot{sy, ctx->sl, const_cast<double*>((const double*)q_dev), const_cast<double*>((const double*)p_dev), 1,
                   ctx->d_act}, (long)sy.B * sy.Q, 8);
  begin_all(ctx, nullptr, ctx->d_act);  // re-evaluate the state caches of the restored chains only
  state_eval(ctx, 0);
  ctx->mom_tangent = ctx->mom_tangent && momentum_is_tangent != 0;
  CHMC_LEAVE("chmc_restore_device")
}
extern "C" int chmc_tree_leaf(chmc_ctx* ctx, const int* run, const int* take, void* sub_prop_q_dev, void* sub_sum_dev,
                              void* ck_p_dev, void* ck_sum_dev, void* ck_end_dev, int store_slot, int check_lo, int n_check,
                              double* out) {
  CHMC_ENTER("chmc_tree_leaf")
  if (!run || !take || !sub_prop_q_dev || !sub_sum_dev || !ck_p_dev || !ck_sum_dev || (n_check > 0 && !out))
    return fail("chmc_tree_leaf: null argument");
  if (n_check < 0 || n_check > CHMC_TREE_MAXCHK || check_lo < 0 || store_slot < -1)
    return fail("chmc_tree_leaf: checkpoint range out of bounds");
  const Sys& sy = ctx->sy;
  const int ng = rowsum_groups(sy.Q), nacc = 6 * n_check;
  if (!ctx->d_tree_part) {
    ctx->d_tree_part = alloc<double>(ctx, (size_t)sy.B * ng * CHMC_ROWSUM_MAX);
    ctx->d_tree_out = alloc<double>(ctx, (size_t)sy.B * CHMC_ROWSUM_MAX);
    ctx->d_tree_mask = alloc<int>(ctx, 2 * (size_t)sy.B);
  }
  h2d(ctx->d_tree_mask, run, sizeof(int) * sy.B);
  h2d(ctx->d_tree_mask + sy.B, take, sizeof(int) * sy.B);
  launch_rowsum(KTreeLeaf{sy, ctx->sl, ctx->d_tree_mask, ctx->d_tree_mask + sy.B, (double*)sub_prop_q_dev,
                          (double*)sub_sum_dev, (double*)ck_p_dev, (double*)ck_sum_dev, (double*)ck_end_dev, store_slot,
                          check_lo, n_check},
                sy.Q, sy.B, nacc, ctx->d_tree_part, 8);
  if (nacc) {
    launch(KTreeLeafFinish{sy, ctx->sl, ctx->d_tree_mask, ctx->d_tree_part, ng, nacc, ctx->d_tree_out, (double*)ck_end_dev,
                           check_lo},
           sy.B);
    d2h(out, ctx->d_tree_out, sizeof(double) * (size_t)sy.B * nacc);
  } else {
    dev_sync();  // the caller's buffers are final when the call returns
  }
  CHMC_LEAVE("chmc_tree_leaf")
}
extern "C" int chmc_get_head(chmc_ctx* ctx, int n, double* out) {
  CHMC_ENTER("chmc_get_head")
  const Sys& sy = ctx->sy;
  if (!out || n < 1 || n > sy.Q) return fail("chmc_get_head: bad argument");
  std::vector<int> cur(sy.B);
  d2h(cur.data(), ctx->sl.cur, sizeof(int) * sy.B);
  for (int ch = 0; ch < sy.B; ++ch)
    d2h(out + (size_t)ch * n, ctx->sl.q[cur[ch]] + (size_t)ch * sy.Q, sizeof(double) * n);
  CHMC_LEAVE("chmc_get_head")
}

// x at the observation times of every chain's current state, sequentially (KXobs)
static void update_x_obs(chmc_ctx* ctx) {
  const Sys& sy = ctx->sy;
  dispatch(ctx, [&](auto inst) { launch(KXobs<typename decltype(inst)::M>{sy, ctx->sl, ctx->d_xobs}, sy.B); });
}
extern "C" int chmc_update_x_obs_seq(chmc_ctx* ctx) {
  CHMC_ENTER("chmc_update_x_obs_seq")
  update_x_obs(ctx);
  CHMC_LEAVE("chmc_update_x_obs_seq")
}
extern "C" int chmc_switch_partition(chmc_ctx* ctx) {
  CHMC_ENTER("chmc_switch_partition")
  // the stored trajectories (valid for the partition we are leaving) seed a time-parallel pass over the whole chain
  // (the stored-rows family keeps round 1's sequential pass: the A/B test then covers both)
  const bool par = ctx->plan.pb_allocated && ctx->have_state;
  if (par) dispatch(ctx, [&](auto inst) { xobs_par<typename decltype(inst)::M>(ctx); });
  select_partition(ctx, (ctx->part + 1) % ctx->num_partition);
  if (!par) update_x_obs(ctx);
  begin_all(ctx, nullptr, nullptr);
  state_eval(ctx, 0);
  ctx->mom_tangent = false;  // the momentum was tangent to the other partition's constraint set
  CHMC_LEAVE("chmc_switch_partition")
}

// the latent path (include/chmc.h): path_scan picks the pass; q_dev null = current states
static int path_check(chmc_ctx* ctx, const char* fn, int stride, bool current) {
  if (stride < 1 || ctx->sy.S % stride != 0)
    return fail(std::string(fn) + ": stride must be at least 1 and divide num_steps_per_obs");
  if (current && !ctx->have_state) return fail(std::string(fn) + ": no state has been set");
  return 0;
}
// a call's chain mask on the device: d_path_ints ([2][B], allocated on first use) holds the sweeps, then the mask
static int* path_mask(chmc_ctx* ctx, const int* mask) {
  if (!ctx->d_path_ints) ctx->d_path_ints = alloc<int>(ctx, 2 * (size_t)ctx->sy.B);
  if (!mask) return nullptr;
  int* d_mask = ctx->d_path_ints + ctx->sy.B;
  h2d(d_mask, mask, sizeof(int) * ctx->sy.B);
  return d_mask;
}
static void path_run(chmc_ctx* ctx, const double* q_dev, int stride, double* out_dev, int* sweeps) {
  path_mask(ctx, nullptr);
  dispatch(ctx, [&](auto inst) { path_scan<typename decltype(inst)::M>(ctx, q_dev, stride, out_dev, sweeps ? ctx->d_path_ints : nullptr); });
  if (sweeps) d2h(sweeps, ctx->d_path_ints, sizeof(int) * ctx->sy.B);
}
extern "C" int chmc_generate_x_seq(chmc_ctx* ctx, const double* q, int stride, double* x_seq, int* sweeps) {
  CHMC_ENTER("chmc_generate_x_seq")
  if (!x_seq) return fail("chmc_generate_x_seq: null output");
  if (path_check(ctx, "chmc_generate_x_seq", stride, q == nullptr)) return -1;
  const Sys& sy = ctx->sy;
  const size_t n = (size_t)sy.B * (sy.T * sy.S / stride + 1) * sy.X;
  if (ctx->d_path_cap < n) ctx->d_path_out = alloc<double>(ctx, n), ctx->d_path_cap = n;
  if (q) h2d(ctx->w.qb, q, sizeof(double) * (size_t)sy.B * sy.Q);
  path_run(ctx, q ? ctx->w.qb : nullptr, stride, ctx->d_path_out, sweeps);
  d2h(x_seq, ctx->d_path_out, sizeof(double) * n);
  CHMC_LEAVE("chmc_generate_x_seq")
}
extern "C" int chmc_generate_x_seq_device(chmc_ctx* ctx, int stride, void* x_seq_dev, int* sweeps) {
  CHMC_ENTER("chmc_generate_x_seq_device")
  if (!x_seq_dev) return fail("chmc_generate_x_seq_device: null output");
  if (path_check(ctx, "chmc_generate_x_seq_device", stride, true)) return -1;
  path_run(ctx, nullptr, stride, (double*)x_seq_dev, sweeps);
  CHMC_LEAVE("chmc_generate_x_seq_device")
}
extern "C" int chmc_path_stats_update_device(chmc_ctx* ctx, int stride, const int* mask, void* x_seq_dev, void* n_dev,
                                             void* mean_dev, void* m2_dev) {
  CHMC_ENTER("chmc_path_stats_update_device")
  if (!x_seq_dev || !n_dev || !mean_dev || !m2_dev) return fail("chmc_path_stats_update_device: null argument");
  if (path_check(ctx, "chmc_path_stats_update_device", stride, true)) return -1;
  const Sys& sy = ctx->sy;
  const int NP = sy.T * sy.S / stride + 1;
  path_run(ctx, nullptr, stride, (double*)x_seq_dev, nullptr);
  const int* d_mask = path_mask(ctx, mask);
  dispatch(ctx, [&](auto inst) {
    using M = typename decltype(inst)::M;
    const KPathWelford<M> f{NP, 0, d_mask, (const double*)x_seq_dev, (long long*)n_dev, (double*)mean_dev, (double*)m2_dev};
    KPathWelford<M> g = f;
    g.phase = 1;
    launch(f, sy.B, 8);
    launch(g, (long)sy.B * NP, 8);
  });
  CHMC_LEAVE("chmc_path_stats_update_device")
}

// posterior predictive simulation (include/chmc.h): predict_pass picks the kernel
static int predict_check(const chmc_ctx* ctx, const char* fn, int horizon, int stride, int origin) {
  if (horizon < 1) return fail(std::string(fn) + ": horizon must be at least 1");
  if (stride < 1 || ctx->sy.S % stride != 0)
    return fail(std::string(fn) + ": stride must be at least 1 and divide num_steps_per_obs");
  if (origin != 0 && origin != 1) return fail(std::string(fn) + ": origin must be 0 (forecast) or 1 (replication)");
  if ((long long)horizon * ctx->sy.S * (ctx->sy.V + 1) >= (1LL << 31))
    return fail(std::string(fn) + ": horizon too long for the 32-bit counter of the normal stream");
  return 0;
}
// the times of a call's NPF points: t0 + p stride dl, p = 1 .. NPF, t0 the last observation's time (origin 0) or 0
static void predict_times(const chmc_ctx* ctx, int NPF, int stride, int origin, double* times) {
  const double t0 = origin == 0 ? ctx->sy.T * ctx->cfg.obs_interval : 0.0;
  for (int p = 1; p <= NPF; ++p) times[p - 1] = t0 + p * (stride * ctx->sy.dl);
}
// a forecast's arguments: the keyed streams of (seed, draw), the steps and points, and for origin 0 the start state x_T --
// the last point of the path of the current states at the observation times, scanned HERE into d_pred_x
static PredictArgs forecast_args(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset, int horizon,
                                 int stride, int origin, int n_rep) {
  const Sys& sy = ctx->sy;
  PredictArgs a{};
  a.seed = seed, a.key0 = CHMC_PREDICT_DRAW | (draw << 16);
  a.chain_offset = chain_offset, a.HS = horizon * sy.S, a.stride = stride, a.NPF = a.HS / stride;
  a.n_rep = n_rep;
  if (origin == 0) {
    if (!ctx->d_pred_x) ctx->d_pred_x = alloc<double>(ctx, (size_t)sy.B * (sy.T + 1) * sy.X);
    path_run(ctx, nullptr, sy.S, ctx->d_pred_x, nullptr);
    a.xstart = ctx->d_pred_x + (size_t)sy.T * sy.X, a.xld = (long long)(sy.T + 1) * sy.X;
  }
  return a;
}
extern "C" int chmc_predict_points(const chmc_ctx* ctx, int horizon, int stride, int origin, int* n_points, double* times) {
  if (!ctx) return fail("chmc_predict_points: null context");
  if (!n_points) return fail("chmc_predict_points: null output");
  if (predict_check(ctx, "chmc_predict_points", horizon, stride, origin)) return -1;
  *n_points = horizon * ctx->sy.S / stride;
  if (times) predict_times(ctx, *n_points, stride, origin, times);
  return 0;
}
// the events of a chmc_predict_events_device call (null: chmc_predict_device)
struct PredictEventCall {
  int channel, p0, p1, n_thresholds;
  const double* thresholds;
  void *events_dev, *en_dev, *emean_dev, *em2_dev;
};
static int event_thresholds(const std::string& fn, int L, const double* th, EventArgs& e) {
  if (L < 0 || L > kEventLevels) return fail(fn + ": the number of thresholds must be in [0, 8]");
  if (L > 0 && !th) return fail(fn + ": thresholds must not be null");
  for (int l = 0; l < L; ++l) {
    if (!(th[l] == th[l]) || (l && !(th[l] > th[l - 1]))) return fail(fn + ": thresholds must be increasing");
    e.theta[l] = th[l];
  }
  e.L = L;
  return 0;
}
static int predict_call(chmc_ctx* ctx, const char* name, unsigned long long seed, unsigned long long draw, int chain_offset,
                        int horizon, int stride, int origin, int n_rep, const int* mask, int n_levels, const double* levels,
                        void* n_dev, void* mean_dev, void* m2_dev, void* cdf_dev, void* paths_dev, int n_keep,
                        const PredictEventCall* ev) {
  CHMC_ENTER(name)
  const std::string fn = name;
  if (!n_dev || !mean_dev || !m2_dev) return fail(fn + ": null argument");
  if (predict_check(ctx, fn.c_str(), horizon, stride, origin)) return -1;
  if (!ctx->have_state) return fail(fn + ": no state has been set");
  if (n_rep < 1 || n_rep > 65536) return fail(fn + ": n_rep must be in [1, 65536]");
  if ((long long)ctx->sy.B * n_rep >= (1LL << 31) || (long long)ctx->sy.B * (horizon * ctx->sy.S / stride) >= (1LL << 31))
    return fail(fn + ": chains x replicates and chains x points must stay below 2^31");
  if (n_keep < 0 || n_keep > n_rep) return fail(fn + ": n_keep must be in [0, n_rep]");
  if (draw >= (1ULL << 45)) return fail(fn + ": draw must be below 2^45");
  if (n_levels < 0) return fail(fn + ": n_levels must not be negative");
  if (n_levels > 0 && (!levels || !cdf_dev)) return fail(fn + ": n_levels > 0 needs levels and cdf_dev");
  for (int l = 1; l < n_levels; ++l)
    if (!(levels[l] > levels[l - 1])) return fail(fn + ": levels must be increasing");
  const Sys& sy = ctx->sy;
  EventArgs e{};
  if (ev) {
    const int NPF = horizon * sy.S / stride;
    if (!ev->en_dev || !ev->emean_dev || !ev->em2_dev) return fail(fn + ": null argument");
    if (ev->channel < 0 || ev->channel > sy.X + 1) return fail(fn + ": channel must be in [0, X + 1]");
    if (ev->p0 < 0 || ev->p1 < ev->p0 || ev->p1 >= NPF) return fail(fn + ": window must satisfy 0 <= p0 <= p1 < n_points");
    if (event_thresholds(fn, ev->n_thresholds, ev->thresholds, e)) return -1;
    e.channel = ev->channel, e.p0 = ev->p0, e.p1 = ev->p1, e.h = stride * sy.dl;
  }
  PredictArgs a = forecast_args(ctx, seed, draw, chain_offset, horizon, stride, origin, n_rep);
  a.n_keep = paths_dev ? n_keep : 0, a.n_levels = n_levels;
  a.paths = a.n_keep ? (double*)paths_dev : nullptr;
  a.mask = path_mask(ctx, mask);
  if (n_levels > 0) {
    if (ctx->d_pred_lev_cap < (size_t)n_levels)
      ctx->d_pred_lev = alloc<double>(ctx, (size_t)n_levels), ctx->d_pred_lev_cap = (size_t)n_levels;
    h2d(ctx->d_pred_lev, levels, sizeof(double) * n_levels);
    a.levels = ctx->d_pred_lev;
  }
  double* evraw = nullptr;
  if (ev) {  // the point times, as chmc_predict_points gives them, and the replicates' raw events (the caller's buffer or scratch)
    const int NE = 5 + 3 * e.L;
    const size_t n_ev = ev->events_dev ? 0 : (size_t)sy.B * n_rep * NE;
    if (ctx->d_pred_ev_cap < a.NPF + n_ev)
      ctx->d_pred_ev = alloc<double>(ctx, a.NPF + n_ev), ctx->d_pred_ev_cap = a.NPF + n_ev;
    std::vector<double> times(a.NPF);
    predict_times(ctx, a.NPF, stride, origin, times.data());
    h2d(ctx->d_pred_ev, times.data(), sizeof(double) * a.NPF);
    e.times = ctx->d_pred_ev;
    evraw = ev->events_dev ? (double*)ev->events_dev : ctx->d_pred_ev + a.NPF;
  }
  dispatch(ctx, [&](auto inst) {
    predict_pass<typename decltype(inst)::M>(ctx, a, ev ? &e : nullptr, evraw, (long long*)n_dev, (double*)mean_dev,
                                             (double*)m2_dev, (long long*)cdf_dev);
  });
  if (ev) event_fold(ctx, a, e, evraw, (long long*)ev->en_dev, (double*)ev->emean_dev, (double*)ev->em2_dev);
  CHMC_LEAVE(name)
}
extern "C" int chmc_predict_device(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset,
                                   int horizon, int stride, int origin, int n_rep, const int* mask, int n_levels,
                                   const double* levels, void* n_dev, void* mean_dev, void* m2_dev, void* cdf_dev,
                                   void* paths_dev, int n_keep) {
  return predict_call(ctx, "chmc_predict_device", seed, draw, chain_offset, horizon, stride, origin, n_rep, mask, n_levels,
                      levels, n_dev, mean_dev, m2_dev, cdf_dev, paths_dev, n_keep, nullptr);
}
extern "C" int chmc_predict_events_device(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset,
                                          int horizon, int stride, int origin, int n_rep, const int* mask, int n_levels,
                                          const double* levels, void* n_dev, void* mean_dev, void* m2_dev, void* cdf_dev,
                                          void* paths_dev, int n_keep, int channel, int p0, int p1, int n_thresholds,
                                          const double* thresholds, void* events_dev, void* en_dev, void* emean_dev,
                                          void* em2_dev) {
  const PredictEventCall ev{channel, p0, p1, n_thresholds, thresholds, events_dev, en_dev, emean_dev, em2_dev};
  return predict_call(ctx, "chmc_predict_events_device", seed, draw, chain_offset, horizon, stride, origin, n_rep, mask,
                      n_levels, levels, n_dev, mean_dev, m2_dev, cdf_dev, paths_dev, n_keep, &ev);
}

// scoring observations that arrived behind the fit (include/chmc.h): the forecast candidates of chmc_predict_device at
// stride S weighed by y_future; future_pass picks the kernel, future_pick scores, picks and fills the tail; ONE read-back of
// [B] log_pred and [B] picked
extern "C" int chmc_score_future_device(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset,
                                        int horizon, const double* y_future, int n_cand, const int* mask, double* log_pred,
                                        int* picked, void* logw_dev, void* tail_dev) {
  CHMC_ENTER("chmc_score_future_device")
  const std::string fn = "chmc_score_future_device";
  if (!y_future || !log_pred) return fail(fn + ": null argument");
  const Sys& sy = ctx->sy;
  if (predict_check(ctx, fn.c_str(), horizon, sy.S, 0)) return -1;
  if (!ctx->have_state) return fail(fn + ": no state has been set");
  if (!sy.noisy)
    return fail(fn + ": a context without observation noise is not supported (the weights are degenerate there and placing "
                     "the state is a projection; out of scope)");
  if (n_cand < 1 || n_cand > 65536) return fail(fn + ": n_cand must be in [1, 65536]");
  if ((long long)sy.B * n_cand >= (1LL << 31) || (long long)sy.B * ((long long)horizon * sy.S * sy.V + horizon) >= (1LL << 31))
    return fail(fn + ": chains x candidates and chains x tail length must stay below 2^31");
  if (draw >= (1ULL << 45)) return fail(fn + ": draw must be below 2^45");
  if (chain_offset < 0) return fail(fn + ": negative chain_offset");
  const size_t nBH = (size_t)sy.B * horizon;
  for (size_t i = 0; i < nBH; ++i)
    if (!(y_future[i] - y_future[i] == 0.0)) return fail(fn + ": y_future must be finite");
  // scratch: y | log_pred | picked | n of every candidate | logw where the caller keeps none
  const size_t nB = (size_t)sy.B, nC = nB * n_cand, nI = (nB + 1) / 2;
  const size_t need = nBH + nB + nI + nC * horizon + (logw_dev ? 0 : nC);
  if (ctx->d_fut_cap < need) ctx->d_fut = alloc<double>(ctx, need), ctx->d_fut_cap = need;
  double* d_y = ctx->d_fut;
  double* d_lp = d_y + nBH;
  int* d_pk = reinterpret_cast<int*>(d_lp + nB);
  h2d(d_y, y_future, sizeof(double) * nBH);
  PredictArgs a = forecast_args(ctx, seed, draw, chain_offset, horizon, sy.S, 0, n_cand);  // (x_T as the forecast takes it)
  a.mask = path_mask(ctx, mask);
  FutureArgs f{};
  f.H = horizon, f.n_cand = n_cand, f.y = d_y;
  f.nscr = d_lp + nB + nI;
  f.logw = logw_dev ? (double*)logw_dev : f.nscr + nC * horizon;
  dispatch(ctx, [&](auto inst) { future_pass<typename decltype(inst)::M>(ctx, a, f); });
  future_pick(ctx, a, f, CHMC_FUTURE_DRAW | draw, d_lp, d_pk, (double*)tail_dev);
  std::vector<double> h(nB + nI);
  d2h(h.data(), d_lp, sizeof(double) * (nB + nI));
  const int* hp = reinterpret_cast<const int*>(h.data() + nB);
  for (int c = 0; c < sy.B; ++c) {
    if (mask && !mask[c]) continue;
    log_pred[c] = h[c];
    if (picked) picked[c] = hp[c];
  }
  CHMC_LEAVE("chmc_score_future_device")
}

// path-wise events of a path buffer (include/chmc.h): path_events_pass picks the kernel
extern "C" int chmc_path_events_device(chmc_ctx* ctx, const void* x_seq_dev, int n_points, int stride, int channel, int p0,
                                       int p1, int n_thresholds, const double* thresholds, const int* mask, void* events_dev) {
  CHMC_ENTER("chmc_path_events_device")
  const std::string fn = "chmc_path_events_device";
  if (!x_seq_dev || !events_dev) return fail(fn + ": null argument");
  const Sys& sy = ctx->sy;
  if (stride < 1 || sy.S % stride != 0) return fail(fn + ": stride must be at least 1 and divide num_steps_per_obs");
  if (channel < 0 || channel > sy.X) return fail(fn + ": channel must be in [0, X]");
  if (n_points < 1 || (long long)sy.B * n_points >= (1LL << 31)) return fail(fn + ": n_points must be positive, chains x points below 2^31");
  if (p0 < 0 || p1 < p0 || p1 >= n_points) return fail(fn + ": window must satisfy 0 <= p0 <= p1 < n_points");
  EventArgs e{};
  if (event_thresholds(fn, n_thresholds, thresholds, e)) return -1;
  e.channel = channel, e.p0 = p0, e.p1 = p1, e.h = stride * sy.dl;
  const int* d_mask = path_mask(ctx, mask);
  dispatch(ctx, [&](auto inst) {
    path_events_pass<typename decltype(inst)::M>(ctx, n_points, e, d_mask, (const double*)x_seq_dev, (double*)events_dev);
  });
  CHMC_LEAVE("chmc_path_events_device")
}


// padded [B][Kmax][RM] <-> packed [B][C] conversion of block-row vectors (host side, small)
static void unpad_rows(const chmc_ctx* c, const std::vector<double>& pad, double* out, int ncomp) {
  const Sys& sy = c->sy;
  const auto& bl = c->hblk[c->part];
  for (int ch = 0; ch < sy.B; ++ch)
    for (int b = 0; b < sy.K; ++b)
      for (int i = 0; i < bl[b].nrows; ++i)
        for (int a = 0; a < ncomp; ++a)
          out[((size_t)ch * sy.C + bl[b].row0 + i) * ncomp + a] = pad[(((size_t)ch * sy.Kmax + b) * sy.RM + i) * ncomp + a];
}
static void pad_rows(const chmc_ctx* c, const double* in, std::vector<double>& pad) {
  const Sys& sy = c->sy;
  const auto& bl = c->hblk[c->part];
  pad.assign((size_t)sy.B * sy.Kmax * sy.RM, 0.0);
  for (int ch = 0; ch < sy.B; ++ch)
    for (int b = 0; b < sy.K; ++b)
      for (int i = 0; i < bl[b].nrows; ++i) pad[((size_t)ch * sy.Kmax + b) * sy.RM + i] = in[(size_t)ch * sy.C + bl[b].row0 + i];
}
static void fetch_padded(chmc_ctx* c, const double* dev, double* out, int ncomp) {
  const Sys& sy = c->sy;
  std::vector<double> pad((size_t)sy.B * sy.Kmax * sy.RM * ncomp);
  d2h(pad.data(), dev, sizeof(double) * pad.size());
  unpad_rows(c, pad, out, ncomp);
}
// copy a slot-selected per-chain array to the host
static void fetch_slot(chmc_ctx* c, double* const a[2], double* host, size_t stride, double* staging) {
  const Sys& sy = c->sy;
  launch(KGatherSlotVec{c->sl, a[0], a[1], staging, (long)stride}, (long)sy.B * (long)stride);
  d2h(host, staging, sizeof(double) * (size_t)sy.B * stride);
}

extern "C" int chmc_constr(chmc_ctx* ctx, double* cvec) {
  CHMC_ENTER("chmc_constr")
  if (!cvec) return fail("chmc_constr: null output");
  const Sys& sy = ctx->sy;
  begin_all(ctx, nullptr, nullptr);
  dispatch(ctx, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    launch(KFwd<M, RM>{sy, ctx->sl, ctx->w, 0, 0, 0, 0}, (long)sy.B * sy.K, 7);
  });
  ctx->counters[0]++;
  fetch_padded(ctx, ctx->w.cpad, cvec, 1);
  CHMC_LEAVE("chmc_constr")
}
extern "C" int chmc_jacob_constr_blocks(chmc_ctx* ctx, double* dc_du, double* dc_dv) {
  CHMC_ENTER("chmc_jacob_constr_blocks")
  const Sys& sy = ctx->sy;
  if (dc_du) {
    std::vector<double> pad((size_t)sy.B * sy.Kmax * sy.RM * sy.U);
    launch(KGatherSlotVec{ctx->sl, ctx->sl.JuP[0], ctx->sl.JuP[1], ctx->w.Ew, (long)sy.Kmax * sy.RM * sy.U},
           (long)sy.B * sy.Kmax * sy.RM * sy.U);
    d2h(pad.data(), ctx->w.Ew, sizeof(double) * pad.size());
    unpad_rows(ctx, pad, dc_du, sy.U);
  }
  if (dc_dv) {
    ensure_rows(ctx);
    // staging through Xd (>= RM*NV doubles per chain because T*S*RM*X >= RM*(V0 + T*S*V) does not hold in
    // general): copy slot by slot instead
    std::vector<int> cur(sy.B);
    d2h(cur.data(), ctx->sl.cur, sizeof(int) * sy.B);
    const size_t st = (size_t)sy.RM * sy.NV;
    for (int ch = 0; ch < sy.B; ++ch) d2h(dc_dv + ch * st, ctx->sl.Jv[cur[ch]] + ch * st, sizeof(double) * st);
  }
  CHMC_LEAVE("chmc_jacob_constr_blocks")
}
extern "C" int chmc_chol_gram_blocks(chmc_ctx* ctx, double* chol_C, double* chol_D) {
  CHMC_ENTER("chmc_chol_gram_blocks")
  const Sys& sy = ctx->sy;
  std::vector<int> cur(sy.B);
  d2h(cur.data(), ctx->sl.cur, sizeof(int) * sy.B);
  for (int ch = 0; ch < sy.B; ++ch) {
    if (chol_C)
      d2h(chol_C + (size_t)ch * sy.U * sy.U, ctx->sl.facC[cur[ch]] + (size_t)ch * sy.U * sy.U, sizeof(double) * sy.U * sy.U);
    if (chol_D)
      for (int b = 0; b < sy.K; ++b)
        d2h(chol_D + ((size_t)ch * sy.K + b) * sy.RM * sy.RM,
            ctx->sl.facD[cur[ch]] + ((size_t)ch * sy.Kmax + b) * sy.RM * sy.RM, sizeof(double) * sy.RM * sy.RM);
  }
  CHMC_LEAVE("chmc_chol_gram_blocks")
}
extern "C" int chmc_log_det_sqrt_gram(chmc_ctx* ctx, double* out) {
  CHMC_ENTER("chmc_log_det_sqrt_gram")
  if (!out) return fail("chmc_log_det_sqrt_gram: null output");
  fetch_slot(ctx, ctx->sl.logdet, out, 1, ctx->w.err);
  CHMC_LEAVE("chmc_log_det_sqrt_gram")
}
extern "C" int chmc_grad_log_det_sqrt_gram(chmc_ctx* ctx, double* grad) {
  CHMC_ENTER("chmc_grad_log_det_sqrt_gram")
  if (!grad) return fail("chmc_grad_log_det_sqrt_gram: null output");
  fetch_slot(ctx, ctx->sl.grad, grad, ctx->sy.Q, ctx->w.qb);
  CHMC_LEAVE("chmc_grad_log_det_sqrt_gram")
}
extern "C" int chmc_lmult_by_jacob_constr(chmc_ctx* ctx, const double* vct, double* out) {
  CHMC_ENTER("chmc_lmult_by_jacob_constr")
  if (!vct || !out) return fail("chmc_lmult_by_jacob_constr: null argument");
  const Sys& sy = ctx->sy;
  ensure_rows(ctx);
  h2d(ctx->w.vin, vct, sizeof(double) * (size_t)sy.B * sy.Q);
  begin_all(ctx, nullptr, nullptr);
  dispatch(ctx, [&](auto inst) { jw<typename decltype(inst)::M, decltype(inst)::RM>(ctx, 0, 2, false); });
  fetch_padded(ctx, ctx->w.cpad, out, 1);
  CHMC_LEAVE("chmc_lmult_by_jacob_constr")
}
// u-columns of J^T lambda for the per-op API (the fused paths fold them into KSolveChain)
struct KJtLamU {
  Sys sy;
  Slots sl;
  Work w;
  CHMC_HD void operator()(int c) const {
    const int s = sl.cur[c];
    for (int a = 0; a < sy.U; ++a) {
      double t = 0.0;
      for (int b = 0; b < sy.K; ++b)
        for (int i = 0; i < sy.RM; ++i)
          t += pick(sl.JuP, s)[(((size_t)c * sy.Kmax + b) * sy.RM + i) * sy.U + a] * w.lampad[((size_t)c * sy.Kmax + b) * sy.RM + i];
      w.pb[(size_t)c * sy.Q + a] = t;
    }
  }
};
extern "C" int chmc_rmult_by_jacob_constr(chmc_ctx* ctx, const double* vct, double* out) {
  CHMC_ENTER("chmc_rmult_by_jacob_constr")
  if (!vct || !out) return fail("chmc_rmult_by_jacob_constr: null argument");
  const Sys& sy = ctx->sy;
  ensure_rows(ctx);
  std::vector<double> pad;
  pad_rows(ctx, vct, pad);
  h2d(ctx->w.lampad, pad.data(), sizeof(double) * pad.size());
  begin_all(ctx, nullptr, nullptr);
  dispatch(ctx, [&](auto inst) { update<decltype(inst)::RM, 2>(sy, ctx->sl, ctx->w, 0, 0, 0); });
  launch(KJtLamU{sy, ctx->sl, ctx->w}, sy.B);
  d2h(out, ctx->w.pb, sizeof(double) * (size_t)sy.B * sy.Q);
  CHMC_LEAVE("chmc_rmult_by_jacob_constr")
}
extern "C" int chmc_lmult_by_inv_gram(chmc_ctx* ctx, const double* vct, double* out) {
  CHMC_ENTER("chmc_lmult_by_inv_gram")
  if (!vct || !out) return fail("chmc_lmult_by_inv_gram: null argument");
  const Sys& sy = ctx->sy;
  std::vector<double> pad;
  pad_rows(ctx, vct, pad);
  h2d(ctx->w.cpad, pad.data(), sizeof(double) * pad.size());
  begin_all(ctx, nullptr, nullptr);
  dispatch(ctx, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    launch(KSymBlk<M, RM>{sy, ctx->sl, ctx->w, 0, 0}, (long)sy.B * sy.K, 9);
    solve_chain<M, RM, 1, 2>(sy, ctx->sl, ctx->w, 0, 0, 0);
  });
  fetch_padded(ctx, ctx->w.lampad, out, 1);
  CHMC_LEAVE("chmc_lmult_by_inv_gram")
}
extern "C" int chmc_normal_space_component(chmc_ctx* ctx, const double* vct, double* out) {
  CHMC_ENTER("chmc_normal_space_component")
  if (!vct || !out) return fail("chmc_normal_space_component: null argument");
  const Sys& sy = ctx->sy;
  ensure_rows(ctx);
  h2d(ctx->w.vin, vct, sizeof(double) * (size_t)sy.B * sy.Q);
  begin_all(ctx, nullptr, nullptr);
  dispatch(ctx, [&](auto inst) {
    using M = typename decltype(inst)::M;
    constexpr int RM = decltype(inst)::RM;
    jw<M, RM>(ctx, 0, 2 | 256, false);
    launch(KSymBlk<M, RM>{sy, ctx->sl, ctx->w, 0, 0}, (long)sy.B * sy.K, 9);
    solve_chain<M, RM, 1, 2>(sy, ctx->sl, ctx->w, 0, 0, 0);
    update<RM, 2>(sy, ctx->sl, ctx->w, 0, 0, 0);
  });
  launch(KJtLamU{sy, ctx->sl, ctx->w}, sy.B);
  d2h(out, ctx->w.pb, sizeof(double) * (size_t)sy.B * sy.Q);
  CHMC_LEAVE("chmc_normal_space_component")
}
extern "C" int chmc_project_onto_cotangent_space(chmc_ctx* ctx) {
  CHMC_ENTER("chmc_project_onto_cotangent_space")
  begin_all(ctx, nullptr, nullptr);
  project_momentum(ctx, 0, 0, 0);
  ctx->mom_tangent = true;
  CHMC_LEAVE("chmc_project_onto_cotangent_space")
}
// conditioned_diffusion_neg_log_dens_and_grad (:82-205) for the positions staged in work.qb; values into ctx->d_ham [B],
// gradient (optional) into grad_dev [B][U + NV]
static int nld_core(chmc_ctx* ctx, int use_gaussian_splitting, double* grad_dev) {
  if (!ctx->plan_in.wave_kernels) return fail("chmc_neg_log_dens_and_grad: not available in the host emulation build");
  const Sys& sy = ctx->sy;
  const int QH = sy.U + sy.NV;
  // the whole chain as ONE block of T observations: the forward-scan kernel then integrates the full trajectory
  Sys sf = sy;
  if (!ctx->d_blk_full) {
    BlockDesc bf{};
    bf.obs0 = 0, bf.nobs = sy.T, bf.first = 1, bf.last = 1, bf.row0 = 0, bf.nrows = 0, bf.ny = 0;
    bf.col0 = 0, bf.ncols = sy.NV, bf.step0 = 0, bf.nsteps = sy.T * sy.S;
    ctx->d_blk_full = alloc<BlockDesc>(ctx, 1);
    h2d(ctx->d_blk_full, &bf, sizeof(BlockDesc));
  }
  sf.K = 1, sf.Kmax = 1, sf.Q = QH, sf.blk = ctx->d_blk_full;
  // One block of T S steps per chain: a lane-per-chain scan keeps B / 64 wavefronts busy for T S dependent steps (0.93 ms
  // for the 2 800 steps of the boarding-school SIR chains, 2.8 ms for 40 000 FitzHugh-Nagumo steps) -- for up to 1 024 chains
  // the time-parallel scan (multiple shooting over 64 segments, k_fwd_par) does it in a few sweeps, seeded with the work
  // trajectory of the previous call (the Adam-based initial-state finder and the HMC comparator evaluate nearby points
  // call after call; a useless guess only costs sweeps).  KernelPlan::nld, from this call's CHMC_PAR_SCAN / CHMC_PAR_WAVES.
  const bool par = ctx->plan.nld == FwdPar;
  if (par && !ctx->d_order_ident) {
    std::vector<int> id(sy.B);
    for (int i = 0; i < sy.B; ++i) id[i] = i;
    ctx->d_order_ident = alloc<int>(ctx, sy.B);
    h2d(ctx->d_order_ident, id.data(), sizeof(int) * sy.B);
  }
  begin_all(ctx, nullptr, nullptr);  // every chain active
  dispatch(ctx, [&](auto inst) {
    nld_sweeps<typename decltype(inst)::M, decltype(inst)::RM>(ctx, sf, QH, use_gaussian_splitting, grad_dev);
  });
  return 0;
}
extern "C" int chmc_neg_log_dens_and_grad(chmc_ctx* ctx, const double* q, int use_gaussian_splitting, double* value,
                                          double* grad) {
  CHMC_ENTER("chmc_neg_log_dens_and_grad")
  const Sys& sy = ctx->sy;
  if (!q || !value) return fail("chmc_neg_log_dens_and_grad: q and value are required");
  if (!sy.noisy) return fail("chmc_neg_log_dens_and_grad: needs observation noise (the density is degenerate without)");
  const size_t n = sizeof(double) * (size_t)sy.B * (sy.U + sy.NV);
  h2d(ctx->w.qb, q, n);
  if (nld_core(ctx, use_gaussian_splitting, grad ? ctx->w.pb : nullptr)) return -1;
  d2h(value, ctx->d_ham, sizeof(double) * sy.B);
  if (grad) d2h(grad, ctx->w.pb, n);
  CHMC_LEAVE("chmc_neg_log_dens_and_grad")
}
// the same with the positions and the gradient in device memory (the caller's buffers): nothing but the B values
// crosses PCIe
extern "C" int chmc_neg_log_dens_and_grad_device(chmc_ctx* ctx, const void* q_dev, int use_gaussian_splitting,
                                                 double* value, void* grad_dev) {
  CHMC_ENTER("chmc_neg_log_dens_and_grad_device")
  const Sys& sy = ctx->sy;
  if (!q_dev || !value) return fail("chmc_neg_log_dens_and_grad_device: q_dev and value are required");
  if (!sy.noisy) return fail("chmc_neg_log_dens_and_grad_device: needs observation noise (the density is degenerate without)");
  d2d(ctx->w.qb, q_dev, sizeof(double) * (size_t)sy.B * (sy.U + sy.NV));
  if (nld_core(ctx, use_gaussian_splitting, (double*)grad_dev)) return -1;
  d2h(value, ctx->d_ham, sizeof(double) * sy.B);
  CHMC_LEAVE("chmc_neg_log_dens_and_grad_device")
}
// Adam-based initial states, device-resident loop (init.py): objective + gradient of chmc_neg_log_dens_and_grad_device and the
// row statistics of the restart rules in one call and one read-back of [B][3]
extern "C" int chmc_adam_objective_device(chmc_ctx* ctx, const void* u_v_dev, void* grad_dev, double* out3) {
  CHMC_ENTER("chmc_adam_objective_device")
  const Sys& sy = ctx->sy;
  if (!u_v_dev || !grad_dev || !out3) return fail("chmc_adam_objective_device: null argument");
  if (!sy.noisy) return fail("chmc_adam_objective_device: needs observation noise");
  const int n = sy.U + sy.NV;
  d2d(ctx->w.qb, u_v_dev, sizeof(double) * (size_t)sy.B * n);
  if (nld_core(ctx, 0, (double*)grad_dev)) return -1;
  launch_rowsum(KAdamRow{(const double*)u_v_dev, (const double*)grad_dev, n}, n, sy.B, 2, ctx->w.part, 8);
  launch(KAdamStats{ctx->w.part, ctx->d_ham, rowsum_groups(n), ctx->d_ham + sy.B}, sy.B);
  d2h(out3, ctx->d_ham + sy.B, sizeof(double) * (size_t)sy.B * 3);
  CHMC_LEAVE("chmc_adam_objective_device")
}
extern "C" int chmc_adam_update_device(chmc_ctx* ctx, void* u_v_dev, void* m_dev, void* v_dev, const void* grad_dev,
                                       const double* coef, double b1, double b2, double eps) {
  CHMC_ENTER("chmc_adam_update_device")
  const Sys& sy = ctx->sy;
  if (!u_v_dev || !m_dev || !v_dev || !grad_dev || !coef) return fail("chmc_adam_update_device: null argument");
  const int n = sy.U + sy.NV;
  h2d(ctx->d_ham, coef, sizeof(double) * (size_t)sy.B * 2);
  launch(KAdamUpdate{(double*)u_v_dev, (double*)m_dev, (double*)v_dev, (const double*)grad_dev, ctx->d_ham, n, b1, b2, eps},
         (long)sy.B * n, 8);
  CHMC_LEAVE("chmc_adam_update_device")
}
// Keyed normal draws (KNormalFillRows): the listed rows' (stream, draw) keys and indices go up in one copy.  Checks shared by
// chmc_fill_normal_device, chmc_fill_normal and chmc_adam_begin_tries_device: every row in [0, B), none listed twice.
static int upload_row_keys(chmc_ctx* ctx, const char* fn, int n_rows, const int* rows, const int* stream,
                           const unsigned long long* draw, const int** rows_dev) {
  const int B = ctx->sy.B;
  if (n_rows < 0 || n_rows > B) return fail(std::string(fn) + ": n_rows out of range");
  if (n_rows && (!rows || !stream || !draw)) return fail(std::string(fn) + ": null argument");
  std::vector<unsigned long long> h((size_t)B * 3, 0ULL);
  int* hr = reinterpret_cast<int*>(h.data() + (size_t)B * 2);
  std::vector<char> seen(B, 0);
  for (int r = 0; r < n_rows; ++r) {
    if (rows[r] < 0 || rows[r] >= B) return fail(std::string(fn) + ": row index out of range");
    if (seen[rows[r]]) return fail(std::string(fn) + ": a row is listed twice");
    seen[rows[r]] = 1;
    h[2 * r] = (unsigned long long)(unsigned)stream[r], h[2 * r + 1] = draw[r], hr[r] = rows[r];
  }
  if (!ctx->d_fill_keys) ctx->d_fill_keys = alloc<unsigned long long>(ctx, (size_t)B * 3);
  if (n_rows) h2d(ctx->d_fill_keys, h.data(), sizeof(unsigned long long) * h.size());
  *rows_dev = reinterpret_cast<const int*>(ctx->d_fill_keys + (size_t)B * 2);
  return 0;
}
static int fill_rows(chmc_ctx* ctx, const char* fn, unsigned long long seed, int n_rows, const int* rows_dev, int n_cols,
                     double* dst_dev, long long ld) {
  const long npair = ((long)n_cols + 1) / 2;
  if ((long)n_rows * npair > 0x7fffffffL) return fail(std::string(fn) + ": too many values for one call");
  const int wide = ld % 2 == 0 && n_cols % 2 == 0 && (reinterpret_cast<uintptr_t>(dst_dev) & 15) == 0;
  launch(KNormalFillRows{seed, rows_dev, ctx->d_fill_keys, n_cols, dst_dev, ld, wide}, (long)n_rows * npair, 8);
  return 0;
}
extern "C" int chmc_fill_normal_device(chmc_ctx* ctx, unsigned long long seed, int n_rows, const int* rows, const int* stream,
                                       const unsigned long long* draw, int n_cols, void* dst_dev, long ld) {
  CHMC_ENTER("chmc_fill_normal_device")
  if (!dst_dev) return fail("chmc_fill_normal_device: null argument");
  if (n_cols < 0 || ld < n_cols) return fail("chmc_fill_normal_device: need 0 <= n_cols <= ld");
  const int* rows_dev = nullptr;
  if (upload_row_keys(ctx, "chmc_fill_normal_device", n_rows, rows, stream, draw, &rows_dev)) return -1;
  if (fill_rows(ctx, "chmc_fill_normal_device", seed, n_rows, rows_dev, n_cols, (double*)dst_dev, ld)) return -1;
  CHMC_LEAVE("chmc_fill_normal_device")
}
// host-pointer twin: the same kernel into a compact scratch [n_rows][n_cols], copied back row by row (padding and unlisted
// rows of dst are not touched)
extern "C" int chmc_fill_normal(chmc_ctx* ctx, unsigned long long seed, int n_rows, const int* rows, const int* stream,
                                const unsigned long long* draw, int n_cols, double* dst, long ld) {
  CHMC_ENTER("chmc_fill_normal")
  if (!dst) return fail("chmc_fill_normal: null argument");
  if (n_cols < 0 || ld < n_cols) return fail("chmc_fill_normal: need 0 <= n_cols <= ld");
  const int* rows_dev = nullptr;
  if (upload_row_keys(ctx, "chmc_fill_normal", n_rows, rows, stream, draw, &rows_dev)) return -1;
  if (n_rows == 0 || n_cols == 0) return 0;
  // (the scratch rows are 0 .. n_rows - 1: an identity row list behind the uploaded one)
  std::vector<int> ident(n_rows);
  for (int r = 0; r < n_rows; ++r) ident[r] = r;
  const size_t n = (size_t)n_rows * n_cols;
  double* scratch = (double*)dev_alloc(sizeof(double) * n + sizeof(int) * (size_t)n_rows);
  int* ident_dev = reinterpret_cast<int*>(scratch + n);
  h2d(ident_dev, ident.data(), sizeof(int) * (size_t)n_rows);
  int rc = fill_rows(ctx, "chmc_fill_normal", seed, n_rows, ident_dev, n_cols, scratch, n_cols);
  std::vector<double> h(n);
  if (!rc) d2h(h.data(), scratch, sizeof(double) * n);
  if (dev_sync()) rc = fail(std::string("chmc_fill_normal: ") + g_err);
  dev_free(scratch);
  if (rc) return -1;
  for (int r = 0; r < n_rows; ++r) memcpy(dst + (size_t)rows[r] * (size_t)ld, h.data() + (size_t)r * n_cols, sizeof(double) * (size_t)n_cols);
  return 0;
}
// A prior draw per chain and the data it generates (include/chmc.h): q = keyed N(0, I), x_obs_seq = its path at the observation
// times, y = KSimObs of the two -- the chain then sits on the manifold of its own data, at an exact draw from its posterior.
extern "C" int chmc_simulate_observations_device(chmc_ctx* ctx, unsigned long long seed, int chain_offset, int partition) {
  CHMC_ENTER("chmc_simulate_observations_device")
  if (partition < 0 || partition >= ctx->num_partition)
    return fail("chmc_simulate_observations_device: partition out of range");
  if (chain_offset < 0) return fail("chmc_simulate_observations_device: negative chain_offset");
  Sys& sy = ctx->sy;
  const int B = sy.B;
  if ((long long)B * sy.T > 0x7fffffffLL) return fail("chmc_simulate_observations_device: too many observations for one call");
  std::vector<int> rows(B), stream(B);
  std::vector<unsigned long long> draw(B, CHMC_SIMULATE_DRAW);
  for (int c = 0; c < B; ++c) rows[c] = c, stream[c] = chain_offset + c;
  const int* rows_dev = nullptr;
  if (upload_row_keys(ctx, "chmc_simulate_observations_device", B, rows.data(), stream.data(), draw.data(), &rows_dev)) return -1;
  dev_zero(ctx->sl.cur, sizeof(int) * B);
  if (fill_rows(ctx, "chmc_simulate_observations_device", seed, B, rows_dev, sy.Q, ctx->sl.q[0], sy.Q)) return -1;
  dev_zero(ctx->sl.p[0], sizeof(double) * (size_t)B * sy.Q);
  update_x_obs(ctx);  // x_obs_seq of the draws
  ensure_array(ctx, ctx->d_yc);
  dispatch(ctx, [&](auto inst) {
    launch(KSimObs<typename decltype(inst)::M>{sy, ctx->sl, ctx->d_xobs, ctx->d_yc}, (long)B * sy.T, 8);
  });
  sy.y = ctx->d_yc, sy.ystride = sy.T;
  ctx->have_tree = ctx->pair_ready = ctx->snap_tangent = false;
  select_partition(ctx, partition);
  begin_all(ctx, nullptr, nullptr);
  state_eval(ctx, 0);
  ctx->have_state = true;
  ctx->mom_tangent = true;  // zero momentum
  CHMC_LEAVE("chmc_simulate_observations_device")
}
// The map between time resolutions (include/chmc.h): positions of a context with S_src steps per interval -> positions of
// this one; resample_pass picks the kernel
extern "C" int chmc_resample_q_device(chmc_ctx* ctx, const void* q_src_dev, int S_src, unsigned long long seed,
                                      unsigned long long draw, int chain_offset, const int* mask, void* q_dst_dev) {
  CHMC_ENTER("chmc_resample_q_device")
  const std::string fn = "chmc_resample_q_device";
  if (!q_src_dev || !q_dst_dev) return fail(fn + ": null argument");
  if (S_src < 1) return fail(fn + ": S_src must be at least 1");
  if (draw >= (1ULL << 45)) return fail(fn + ": draw must be below 2^45");
  if (chain_offset < 0) return fail(fn + ": negative chain_offset");
  const Sys& sy = ctx->sy;
  const int S_big = S_src > sy.S ? S_src : sy.S, S_small = S_src > sy.S ? sy.S : S_src;
  if (S_big % S_small != 0)
    return fail(fn + ": S_src and the context's num_steps_per_obs must be in an integer ratio (non-integer ratios are not supported)");
  const int NT = sy.noisy ? sy.T : 0;
  const long long Qs = (long long)sy.U + sy.V0 + (long long)sy.T * S_src * sy.V + NT;
  if (Qs > 0x7fffffffLL || (long long)sy.B * sy.T * S_big > 0x7fffffffLL) return fail(fn + ": too many steps for one call");
  if (S_src == sy.S) {  // a copy of the rows asked for
    for (int c0 = 0; c0 < sy.B;) {
      int c1 = c0;
      while (c1 < sy.B && (!mask || mask[c1])) ++c1;
      if (c1 > c0) d2d((double*)q_dst_dev + (size_t)c0 * sy.Q, (const double*)q_src_dev + (size_t)c0 * sy.Q, sizeof(double) * (size_t)(c1 - c0) * sy.Q);
      c0 = c1 + 1;
    }
    CHMC_LEAVE("chmc_resample_q_device")
  }
  ResampleArgs a{};
  a.seed = seed, a.key = CHMC_RESAMPLE_DRAW | draw, a.chain_offset = chain_offset;
  a.B = sy.B, a.U = sy.U, a.V0 = sy.V0, a.T = sy.T, a.NT = NT;
  a.Sc = S_small, a.m = S_big / S_small, a.refine = sy.S > S_src;
  a.Qs = Qs, a.Qd = sy.Q;
  a.src = (const double*)q_src_dev, a.dst = (double*)q_dst_dev;
  a.mask = path_mask(ctx, mask);
  dispatch(ctx, [&](auto inst) { resample_pass<typename decltype(inst)::M>(ctx, a); });
  CHMC_LEAVE("chmc_resample_q_device")
}
// A position placed on the manifold of the chain's data through its observation-noise part (include/chmc.h): the sequence
// of chmc_simulate_observations_device with n solved for in place of y -- the path scan from q, one small per-chain kernel
// (KSolveNoise), then chmc_set_state's evaluation
extern "C" int chmc_set_state_solve_noise_device(chmc_ctx* ctx, const void* q_dev, int partition, double* moved) {
  CHMC_ENTER("chmc_set_state_solve_noise_device")
  const std::string fn = "chmc_set_state_solve_noise_device";
  if (!q_dev) return fail(fn + ": null argument");
  if (partition < 0 || partition >= ctx->num_partition) return fail(fn + ": partition out of range");
  const Sys& sy = ctx->sy;
  if (!sy.noisy)
    return fail(fn + ": a context without observation noise is not supported (x_obs_seq is part of the constraint there; "
                     "chmc_set_state_project_device places a refined state in it)");
  const size_t n = sizeof(double) * (size_t)sy.B * sy.Q;
  dev_zero(ctx->sl.cur, sizeof(int) * sy.B);
  d2d(ctx->sl.q[0], q_dev, n);
  dev_zero(ctx->sl.p[0], n);
  update_x_obs(ctx);  // x_obs_seq of the given positions
  dispatch(ctx, [&](auto inst) { launch(KSolveNoise<typename decltype(inst)::M>{sy, ctx->sl, ctx->d_xobs, ctx->d_ham}, sy.B, 8); });
  if (moved) d2h(moved, ctx->d_ham, sizeof(double) * sy.B);
  select_partition(ctx, partition);
  begin_all(ctx, nullptr, nullptr);
  state_eval(ctx, 0);
  ctx->have_state = true;
  ctx->mom_tangent = true;  // zero momentum
  CHMC_LEAVE("chmc_set_state_solve_noise_device")
}
// "Deal a try into a row" for the device-resident finder (init.py): keyed start points, zero moments and gradient, and the
// row's carried scan guess back to the cold guess of a new context, so that every evaluation of a try depends on that try's
// own (point, previous iterate) only, whichever row it runs in and whatever ran there before
extern "C" int chmc_adam_begin_tries_device(chmc_ctx* ctx, unsigned long long seed, int n_rows, const int* rows,
                                            const int* stream, const unsigned long long* draw, void* u_v_dev, void* m_dev,
                                            void* v_dev, void* grad_dev) {
  CHMC_ENTER("chmc_adam_begin_tries_device")
  const Sys& sy = ctx->sy;
  if (!u_v_dev || !m_dev || !v_dev || !grad_dev) return fail("chmc_adam_begin_tries_device: null argument");
  if (!sy.noisy) return fail("chmc_adam_begin_tries_device: needs observation noise");
  const int n = sy.U + sy.NV;
  const int* rows_dev = nullptr;
  if (upload_row_keys(ctx, "chmc_adam_begin_tries_device", n_rows, rows, stream, draw, &rows_dev)) return -1;
  if (fill_rows(ctx, "chmc_adam_begin_tries_device", seed, n_rows, rows_dev, n, (double*)u_v_dev, n)) return -1;
  const long long span = (long long)sy.TRJ > n ? (long long)sy.TRJ : n;
  if ((long long)n_rows * span > 0x7fffffffLL) return fail("chmc_adam_begin_tries_device: too many rows for one call");
  launch(KBeginTries{rows_dev, (double*)m_dev, (double*)v_dev, (double*)grad_dev, n, ctx->w.trajw, (long long)sy.TRJ, span},
         (long)n_rows * span, 8);
  CHMC_LEAVE("chmc_adam_begin_tries_device")
}
// find_initial_state_by_gradient_descent (sde/mici_extensions.py:1550-1676), device-resident loop (init.py): objective,
// gradient with respect to ALL of q and the row statistics of its try rules in one call and one read-back of [B][3].
// Forward half KGdFwd, backward half k_gd_grad_wave (HIP) / KGdGrad (host emulation), chain level KGdReduce.
extern "C" int chmc_gd_objective_device(chmc_ctx* ctx, const void* q_dev, const void* xo_dev, double reg_coeff, void* grad_dev,
                                        double* out3) {
  CHMC_ENTER("chmc_gd_objective_device")
  const Sys& sy = ctx->sy;
  if (!q_dev || !xo_dev || !grad_dev || !out3) return fail("chmc_gd_objective_device: null argument");
  const long long tasks = (long long)sy.B * sy.T;
  if (tasks > 0x7fffffffLL) return fail("chmc_gd_objective_device: too many (chain, interval) tasks for one call");
  const size_t ncres = (size_t)tasks * sy.X;
  if (!ctx->d_gd) ctx->d_gd = alloc<double>(ctx, ncres + (size_t)tasks * CHMC_GD_NPART(sy.Z) + (size_t)sy.B * 2);
  const double *q = (const double*)q_dev, *xo = (const double*)xo_dev;
  double *g = (double*)grad_dev, *cres = ctx->d_gd, *part = ctx->d_gd + ncres;
  double* stat = part + (size_t)tasks * CHMC_GD_NPART(sy.Z);  // [B][2] = 1/2 mean(c^2), max |c|
  dispatch(ctx, [&](auto inst) {
    using M = typename decltype(inst)::M;
    launch(KGdFwd<M>{sy, q, xo, ctx->w.trajw, cres}, (long)tasks, 7);
    gd_grad<M>(ctx, (long)tasks, q, cres, reg_coeff, g, part);
    launch(KGdReduce<M>{sy, q, part, reg_coeff, g, stat}, sy.B);
  });
  launch_rowsum(KAdamRow{q, g, sy.Q}, sy.Q, sy.B, 2, ctx->w.part, 8);
  launch(KGdStats{ctx->w.part, stat, rowsum_groups(sy.Q), sy.Q, reg_coeff, ctx->d_ham}, sy.B);
  d2h(out3, ctx->d_ham, sizeof(double) * (size_t)sy.B * 3);
  CHMC_LEAVE("chmc_gd_objective_device")
}
// chmc_adam_update_device over an explicit number of columns (the same kernel): that finder's parameters are all of q
extern "C" int chmc_adam_update_cols_device(chmc_ctx* ctx, int n_cols, void* x_dev, void* m_dev, void* v_dev,
                                            const void* grad_dev, const double* coef, double b1, double b2, double eps) {
  CHMC_ENTER("chmc_adam_update_cols_device")
  const Sys& sy = ctx->sy;
  if (!x_dev || !m_dev || !v_dev || !grad_dev || !coef) return fail("chmc_adam_update_cols_device: null argument");
  if (n_cols < 0 || (long long)sy.B * n_cols > 0x7fffffffLL) return fail("chmc_adam_update_cols_device: n_cols out of range");
  h2d(ctx->d_ham, coef, sizeof(double) * (size_t)sy.B * 2);
  launch(KAdamUpdate{(double*)x_dev, (double*)m_dev, (double*)v_dev, (const double*)grad_dev, ctx->d_ham, n_cols, b1, b2, eps},
         (long)sy.B * n_cols, 8);
  CHMC_LEAVE("chmc_adam_update_cols_device")
}
extern "C" int chmc_hamiltonian(chmc_ctx* ctx, double* h) {
  CHMC_ENTER("chmc_hamiltonian")
  if (!h) return fail("chmc_hamiltonian: null output");
  const Sys& sy = ctx->sy;
  launch_rowsum(KNormRow{sy, ctx->sl}, sy.Q, sy.B, 2, ctx->w.part, 8);  // [B][npart_sum][2] partial sums of q.q, p.p
  launch(KHamiltonian{sy, ctx->sl, ctx->w, ctx->npart_sum, ctx->d_ham}, sy.B);
  d2h(h, ctx->d_ham, sizeof(double) * (size_t)sy.B * 3);
  CHMC_LEAVE("chmc_hamiltonian")
}

struct KMuFromMove {  // mu / dt, or mu / sin(dt) with Gaussian splitting (:1060-1063, :1132-1135); mu = q_in - q_out
  Sys sy;
  Slots sl;
  Work w;
  const double* q_in;
  CHMC_HD void operator()(int tid) const {
    const int c = tid / sy.Q;
    const double dt = w.dt[c];
    const int col = tid - c * sy.Q;
    double d = q_in[tid] - sl.q[sl.cur[c] ^ 1][tid];
    if (sy.m0 && col < sy.U) {  // the multiplier term is metric @ (position move) (:1033-1041, :1105-1113)
      d = 0.0;
      for (int b = 0; b < sy.U; ++b)
        d += metric_of(sy, c)[col * sy.U + b] * (q_in[(size_t)c * sy.Q + b] - sl.q[sl.cur[c] ^ 1][(size_t)c * sy.Q + b]);
    }
    w.mu[tid] = d / (sy.gaussian ? sin(dt) : dt);
  }
};
struct KCopyToOther {  // other slot's q = src
  Sys sy;
  Slots sl;
  const double* src;
  CHMC_HD void operator()(int tid) const {
    const int c = tid / sy.Q;
    sl.q[sl.cur[c] ^ 1][tid] = src[tid];
  }
};
struct KGatherOtherQ {
  Sys sy;
  Slots sl;
  double* out;
  CHMC_HD void operator()(int tid) const {
    const int c = tid / sy.Q;
    out[tid] = sl.q[sl.cur[c] ^ 1][tid];
  }
};

extern "C" int chmc_project(chmc_ctx* ctx, int newton, const double* q, const double* dt, double ctol, double ptol,
                            double dtol, int max_iters, double* q_out, double* mu_out, int* iters, double* norm_dq,
                            double* err, int* status) {
  CHMC_ENTER("chmc_project")
  if (!q || !dt) return fail("chmc_project: q and dt are required");
  if (max_iters < 0) return fail("chmc_project: max_iters < 0");
  const Sys& sy = ctx->sy;
  const size_t n = sizeof(double) * (size_t)sy.B * sy.Q;
  h2d(ctx->w.vin, q, n);
  h2d(ctx->w.err, dt, sizeof(double) * sy.B);  // staging for dt
  ctx->last_dt.clear();                        // the step-size cache of chmc_leapfrog_step is now stale
  begin_all(ctx, ctx->w.err, nullptr);
  launch(KCopyToOther{sy, ctx->sl, ctx->w.vin}, (long)sy.B * sy.Q);
  run_projection(ctx, Solver{newton, ctol, ptol, dtol, max_iters}, 0, 0);
  if (mu_out) {
    launch(KMuFromMove{sy, ctx->sl, ctx->w, ctx->w.vin}, (long)sy.B * sy.Q);
    d2h(mu_out, ctx->w.mu, n);
  }
  if (q_out) {
    launch(KGatherOtherQ{sy, ctx->sl, ctx->w.vin}, (long)sy.B * sy.Q);
    d2h(q_out, ctx->w.vin, n);
  }
  if (iters) d2h(iters, ctx->w.iters, sizeof(int) * sy.B);
  if (err) d2h(err, ctx->w.err, sizeof(double) * sy.B);
  if (norm_dq) d2h(norm_dq, ctx->w.ndq, sizeof(double) * sy.B);
  if (status) d2h(status, ctx->w.nstat, sizeof(int) * sy.B);
  CHMC_LEAVE("chmc_project")
}

// The projection step of find_initial_state_by_gradient_descent (:1654-1669) for the chains of ctx->d_act, whose current
// slots hold (row of q_dev, zero momentum) with their x_obs_seq in the context, partition 0: the state is evaluated, the
// position is projected from it with dt = 1 by the solver of chmc_project, and a converged point replaces the state's
// position (and the row of q_out, where given).  Afterwards d_act holds the chains that converged; their caches are the
// caller's to re-evaluate.  Shared by chmc_gd_project_device and chmc_set_state_project_device.
static void project_rows(chmc_ctx* ctx, const double* q_dev, double* q_out, const Solver& so, int* st, int* iters, double* err) {
  const Sys& sy = ctx->sy;
  begin_all(ctx, nullptr, ctx->d_act);  // the state caches of the masked chains only
  state_eval(ctx, 0);
  const std::vector<double> ones(sy.B, 1.0);
  h2d(ctx->w.err, ones.data(), sizeof(double) * sy.B);  // staging for dt
  ctx->last_dt.clear();                                 // the step-size cache of chmc_leapfrog_step is now stale
  begin_all(ctx, ctx->w.err, ctx->d_act);
  launch(KCopyToOther{sy, ctx->sl, q_dev}, (long)sy.B * sy.Q);
  run_projection(ctx, so, 0, 0);
  d2h(st, ctx->w.nstat, sizeof(int) * sy.B);
  if (iters) d2h(iters, ctx->w.iters, sizeof(int) * sy.B);
  if (err) d2h(err, ctx->w.err, sizeof(double) * sy.B);
  launch(KGdConverged{ctx->w, ctx->d_act}, sy.B);
  launch(KGdAdopt{sy, ctx->sl, ctx->d_act, q_out}, (long)sy.B * sy.Q, 8);
}
// chmc_gd_project_device (include/chmc.h): the masked chains' states become (q_dev row, zero momentum, xo_dev row, partition
// 0), project_rows, and the caches of the chains that moved onto the manifold
extern "C" int chmc_gd_project_device(chmc_ctx* ctx, const int* mask, void* q_dev, const void* xo_dev, int newton, double ctol,
                                      double ptol, double dtol, int max_iters, int* status, int* iters, double* err) {
  CHMC_ENTER("chmc_gd_project_device")
  if (!mask || !q_dev || !xo_dev) return fail("chmc_gd_project_device: mask, q_dev and xo_dev are required");
  if (max_iters < 0) return fail("chmc_gd_project_device: max_iters < 0");
  if (!ctx->have_state || ctx->part != 0)
    return fail("chmc_gd_project_device: the context must hold a state in partition 0 in every row");
  const Sys& sy = ctx->sy;
  h2d(ctx->d_act, mask, sizeof(int) * sy.B);
  ctx->last_active_null = true;
  ctx->last_active.clear();
  launch(KGdSetRows{sy, ctx->sl, (const double*)q_dev, (const double*)xo_dev, ctx->d_xobs, ctx->d_act}, (long)sy.B * sy.Q, 8);
  std::vector<int> st(sy.B);
  project_rows(ctx, (const double*)q_dev, (double*)q_dev, Solver{newton, ctol, ptol, dtol, max_iters}, st.data(), iters, err);
  begin_all(ctx, nullptr, ctx->d_act);  // ... and of the chains that moved onto the manifold
  state_eval(ctx, 0);
  if (dev_sync()) return fail(std::string("chmc_gd_project_device: ") + g_err);
  for (int c = 0; c < sy.B; ++c) {
    if (status) status[c] = mask[c] ? st[c] : CHMC_INACTIVE;
    if (!mask[c]) {
      if (iters) iters[c] = 0;
      if (err) err[c] = 0.0;
    }
  }
  return 0;
}
// A position placed on the manifold of the chain's data WITHOUT observation noise (include/chmc.h): x_obs_seq scanned from
// the row itself (KXobs, as chmc_set_state_solve_noise_device), its observed coordinate pinned to the data (pin_obs), the
// projection of chmc_gd_project_device from that state (project_rows), x_obs_seq again from the projected path, and the
// caches in the partition asked for.
extern "C" int chmc_set_state_project_device(chmc_ctx* ctx, const void* q_dev, int partition, const int* mask, int newton,
                                             double ctol, double ptol, double dtol, int max_iters, int* status, int* iters,
                                             double* defect, double* moved) {
  CHMC_ENTER("chmc_set_state_project_device")
  const std::string fn = "chmc_set_state_project_device";
  if (!q_dev) return fail(fn + ": null argument");
  if (partition < 0 || partition >= ctx->num_partition) return fail(fn + ": partition out of range");
  if (max_iters < 0) return fail(fn + ": max_iters < 0");
  const Sys& sy = ctx->sy;
  if (sy.noisy)
    return fail(fn + ": a context with observation noise places a position exactly and without a solver: "
                     "use chmc_set_state_solve_noise_device");
  const int B = sy.B;
  std::vector<int> m(B, 1);
  bool all = true;
  if (mask)
    for (int c = 0; c < B; ++c) m[c] = mask[c] != 0, all = all && m[c];
  if (!all && !ctx->have_state) return fail(fn + ": a context that holds no state yet takes all chains (mask NULL or all non-zero)");
  if ((long long)B * sy.T * sy.X > 0x7fffffffLL) return fail(fn + ": too many observations for one call");
  const size_t nxo = (size_t)B * sy.T * sy.X, bt = (size_t)B * sy.T;
  if (!ctx->d_place) ctx->d_place = alloc<double>(ctx, nxo + 2 * bt + 3 * (size_t)B);
  double *xs = ctx->d_place, *scr = xs + nxo, *d_defect = scr + 2 * bt, *d_moved = d_defect + 2 * (size_t)B;
  // a partial call leaves the other chains' positions, momenta and x_obs_seq alone; their caches are evaluated again below
  // whenever the call passes through another partition than the one they were evaluated in
  const bool whole = all || ctx->part != 0 || partition != 0;
  const bool tangent = all || (ctx->mom_tangent && ctx->part == partition);
  select_partition(ctx, 0);
  if (all) dev_zero(ctx->sl.cur, sizeof(int) * B);
  h2d(ctx->d_act, m.data(), sizeof(int) * B);
  ctx->last_active_null = true;
  ctx->last_active.clear();
  ctx->have_tree = ctx->pair_ready = false;
  launch(KGdSetRows{sy, ctx->sl, (const double*)q_dev, nullptr, ctx->d_xobs, ctx->d_act}, (long)B * sy.Q, 8);
  dispatch(ctx, [&](auto inst) {
    using M = typename decltype(inst)::M;
    launch(KXobs<M>{sy, ctx->sl, xs}, B);  // x_obs_seq of the given positions
    pin_obs<M>(ctx, ctx->d_act, xs, scr);
  });
  std::vector<double> hd(2 * (size_t)B), hm(B, 0.0);
  d2h(hd.data(), d_defect, sizeof(double) * 2 * (size_t)B);  // defect, pinfail
  std::vector<int> st(B), it(B);
  project_rows(ctx, (const double*)q_dev, nullptr, Solver{newton, ctol, ptol, dtol, max_iters}, st.data(), it.data(), nullptr);
  dev_zero(d_moved, sizeof(double) * B);
  launch_colmax(KPlacedMoved{sy, ctx->sl, ctx->d_act, (const double*)q_dev, reinterpret_cast<unsigned long long*>(d_moved)}, sy.Q, B, 8);
  d2h(hm.data(), d_moved, sizeof(double) * B);
  dispatch(ctx, [&](auto inst) { launch(KXobs<typename decltype(inst)::M>{sy, ctx->sl, xs}, B); });  // ... of the projected ones
  launch(KCopyXobsRows{sy.T * sy.X, ctx->d_act, xs, ctx->d_xobs}, (long)nxo, 8);
  h2d(ctx->d_act, m.data(), sizeof(int) * B);
  select_partition(ctx, partition);
  begin_all(ctx, nullptr, whole ? nullptr : ctx->d_act);
  state_eval(ctx, 0);
  ctx->have_state = true;
  ctx->mom_tangent = tangent;  // zero momentum in the call's chains
  if (dev_sync()) return fail(fn + ": " + g_err);
  for (int c = 0; c < B; ++c) {
    const bool pinfail = hd[B + c] != 0.0;
    if (status) status[c] = !m[c] ? CHMC_INACTIVE : pinfail ? 2 : st[c];
    if (iters) iters[c] = m[c] && !pinfail ? it[c] : 0;
    if (defect) defect[c] = m[c] ? hd[c] : 0.0;
    if (moved) moved[c] = m[c] ? hm[c] : 0.0;
  }
  return 0;
}

struct KInnerRestore {  // failed chains that had completed inner steps: back to the step's start state
  Sys sy;
  Slots sl;
  const double *q0, *p0;
  const int* mask;
  CHMC_HD void operator()(int tid) const {
    const int c = tid / sy.Q;
    if (!mask[c]) return;
    const int s = sl.cur[c];
    pick(sl.q, s)[tid] = q0[tid];
    pick(sl.p, s)[tid] = p0[tid];
  }
};

// chmc_leapfrog_step in two parts: step_enqueue puts the whole step on the stream (the Newton loops wait for their
// active-chain counts only), step_finish fetches the per-chain outputs.  `active_dev`: a device-resident mask used
// instead of the host array (chmc_tree_step: the chains of a trajectory tree that are still running).
struct StepOptions {
  // the per-chain trajectory kernel (traj_waves) takes that many steps per chain in the one launch and leaves the steps done in
  // ctx->d_ndone; every other path takes ONE step and ignores them
  const int* n_steps_host = nullptr;
  int n_steps_all = 1;
  bool want_n_done = false;
  bool skip_end_kick = false;  // the next step of the trajectory applies this step's closing A(dt/2) with its opening one
  bool pending_kick = false;   // ... and this step owes the one of the step before
  // the forward retraction of the NEXT step of the trajectory runs beside this step's reverse one (run_projection_pair); that
  // step then opens by adopting the result instead of flowing and retracting
  bool pair_next = false;
};
static int step_enqueue(chmc_ctx* ctx, const double* dt, const int* active, const int* active_dev, int n_inner, const Solver& s,
                        double rev_tol, const StepOptions& opt = StepOptions{}) {
  const Sys& sy = ctx->sy;
  const int* const n_steps_host = opt.n_steps_host;
  const bool pending_kick = opt.pending_kick, pair_next = opt.pair_next;
  const bool adopt = pending_kick && ctx->pair_ready;
  ctx->pair_ready = false;
  if (pair_next) pair_alloc(ctx);
  // dt / active change rarely between consecutive steps of a trajectory: upload only when they do
  const double* d_dt = nullptr;
  if (ctx->last_dt.size() != (size_t)sy.B || ctx->last_n_inner != n_inner ||
      memcmp(ctx->last_dt.data(), dt, sizeof(double) * sy.B) != 0) {
    h2d(ctx->w.err, dt, sizeof(double) * sy.B);
    ctx->last_dt.assign(dt, dt + sy.B);
    ctx->last_n_inner = n_inner;
    d_dt = ctx->w.err;
  }
  const int* d_active = nullptr;
  if (active_dev) {
    d2d(ctx->d_act, active_dev, sizeof(int) * sy.B);
    ctx->last_active_null = true;  // (the cached host mask no longer describes d_act)
    ctx->last_active.clear();
    d_active = ctx->d_act;
  } else if (active) {
    if (ctx->last_active_null || memcmp(ctx->last_active.data(), active, sizeof(int) * sy.B) != 0) {
      h2d(ctx->d_act, active, sizeof(int) * sy.B);
      ctx->last_active.assign(active, active + sy.B);
      ctx->last_active_null = false;
    }
    d_active = ctx->d_act;
  } else {
    ctx->last_active_null = true;
  }
  if (n_inner > 1) ensure_array(ctx, ctx->d_q0), ensure_array(ctx, ctx->d_p0), ensure_array(ctx, ctx->d_ncommit);
  if (const int waves = traj_waves(ctx, n_inner, s.newton)) {
    ensure_array(ctx, ctx->d_nsteps), ensure_array(ctx, ctx->d_ndone);
    if (n_steps_host) h2d(ctx->d_nsteps, n_steps_host, sizeof(int) * sy.B);
    begin_all(ctx, d_dt ? ctx->w.err : nullptr, d_active ? ctx->d_act : nullptr, 1.0);
    dev_zero(ctx->d_itf, sizeof(int) * sy.B), dev_zero(ctx->d_itb, sizeof(int) * sy.B);
    dispatch(ctx, [&](auto inst) {
      traj_chain<typename decltype(inst)::M, decltype(inst)::RM>(
          waves, (long)sy.B, sy, ctx->sl, ctx->w, n_steps_host ? ctx->d_nsteps : nullptr, opt.n_steps_all, s.ctol, s.ptol, s.dtol,
          s.max_iters, rev_tol, ctx->d_itf, ctx->d_itb, opt.want_n_done ? ctx->d_ndone : nullptr);
    });
    ctx->rows_fresh = false;
    ctx->diag[3]++;
    const int ns = n_steps_host ? 1 : opt.n_steps_all;  // (counters: evaluations per chain of a full-length trajectory)
    ctx->counters[0] += ns, ctx->counters[1] += ns, ctx->counters[3] += ns, ctx->counters[4] += ns, ctx->counters[6] += 2 * ns;
    return 0;
  }
  // The step is a sequence of phases per batch; with two half-batches every phase is enqueued for half 0 on its
  // stream, then for half 1 on the other, and the two Newton loops advance in lock step (run_projection).  The halves
  // are chain ranges of the same arrays, so nothing but the streams is shared; the forward scans of the two halves are
  // kept out of phase (fwd), which puts one half's latency-bound scan, factorisations and checks under the other
  // half's reverse sweeps and column passes.
  //
  // mici _step_b with n_inner_step inner steps of dt_i = dt / n_inner_step: work.dt holds dt_i, the two half-kicks of
  // _step_a use n_inner_step / 2 of it.  Between inner steps the new point becomes state_prev, i.e. the proposal slot
  // becomes the state slot (KCommitInner); only the last inner step evaluates dh1_dpos (gradient of the log-determinant).
  const bool two = ctx->halves == 2;
  const ViewSave full = save_view(ctx);
  const int nh = two ? 2 : 1;
  const double kick = 0.5 * n_inner;
  auto enter = [&](int h) {
    if (two) set_half(ctx, full, h);
  };
  if (two) streams_fork();
  for (int h = 0; h < nh; ++h) {
    enter(h);
    begin_all(ctx, d_dt ? ctx->w.err : nullptr, d_active ? ctx->d_act : nullptr, 1.0 / n_inner);
    dev_zero(ctx->d_itf, sizeof(int) * sy.B), dev_zero(ctx->d_itb, sizeof(int) * sy.B);
    if (n_inner > 1) {
      dev_zero(ctx->d_ncommit, sizeof(int) * sy.B);
      launch(KGatherState{sy, ctx->sl, ctx->d_q0, ctx->d_p0}, (long)sy.B * sy.Q, 8);
    }
  }
  for (int i = 0; i < n_inner; ++i) {
    const bool last = i == n_inner - 1;
    for (int h = 0; h < nh; ++h) {
      enter(h);
      if (i > 0) {
        // later inner steps start from a point whose momentum was projected there: plain h2 flow into the proposal slot
        launch_rows(KFlow{sy, ctx->sl, ctx->w, 0, 0, 0, 1.0}, sy.Q, sy.B, 8);
      } else if (ctx->mom_tangent) {
        // A(dt/2): proposal.p = P(q)[ state.p - dt/2 dh1_dpos(state) ] = state.p - dt/2 pg for a tangent momentum;
        // B: h2 flow from the state with the kicked momentum
        // (pending_kick: the step before, of the same trajectory, left its closing A(dt/2) to this pass)
        if (adopt) {
          launch_rows(KPairAdopt{sy, ctx->sl, ctx->w, kick, ctx->pw.qb}, sy.Q, sy.B, 8);
          launch(KPairAdoptStatus{ctx->w, ctx->pw, ctx->d_itf, ctx->d_itf_next}, sy.B);
        } else if (pending_kick) {
          launch_rows(KKick2FlowPg{sy, ctx->sl, ctx->w, kick}, sy.Q, sy.B, 8);
        } else {
          launch_rows(KKickFlowPg{sy, ctx->sl, ctx->w, kick}, sy.Q, sy.B, 8);
        }
      } else {
        launch(KKick{sy, ctx->sl, ctx->w, 0, 1, kick}, (long)sy.B * sy.Q, 8);
        project_momentum(ctx, 0, 3, 2);
        launch_rows(KFlow{sy, ctx->sl, ctx->w, 0, 0, 1, 1.0}, sy.Q, sy.B, 8);
      }
    }
    if (!adopt)
      run_projection(ctx, s, 0, 0, two ? &full : nullptr, 0);  // retraction onto the manifold
    for (int h = 0; h < nh; ++h) {
      enter(h);
      state_eval_core(ctx, 1, last, 3);  // J, factors, log det at the new point; on the last inner step dh1_dpos as well
      // momentum correction; pg <- dh1_dpos (for the step columns inside the J p pass where that is possible)
      const bool fix_in_jw = last && ctx->plan.mom_fix_in_jp;
      if (fix_in_jw)
        launch_rows(KMomFixEdges{KMomFixInitPg{sy, ctx->sl, ctx->w, 1}}, sy.U + sy.V0 + (sy.Q - sy.U - sy.NV), sy.B, 8);
      else
        launch_rows(KMomFixInitPg{sy, ctx->sl, ctx->w, 1}, sy.Q, sy.B, 8);
      const bool flow_in_update = last && ctx->plan.rev_flow_in_update;
      if (last)  // P p and pg = P dh1_dpos, one pass over the new Jacobian rows
        project_momentum_and_kick_direction(ctx, 1, false, fix_in_jw, flow_in_update, pair_next ? ctx->pw.qb : nullptr, kick);
      else
        project_momentum(ctx, 1, 0, 0);  // (pg of an intermediate point is never used)
      // reverse retraction from the new point and reversibility check (the reverse flow: in the J^T lambda pass where that is
      // possible, the u-part here)
      launch_rows(KFlow{sy, ctx->sl, ctx->w, 1, 1, 0, -1.0}, flow_in_update ? sy.U : sy.Q, sy.B, 8);
      if (pair_next) {  // ... and the forward flow of the next step into the second problem's iterate, likewise
        launch(KPairBegin{ctx->w, ctx->pw, ctx->d_itf_next}, sy.B);
        launch_rows(KPairFlow{sy, ctx->sl, ctx->w, kick, ctx->pw.qb}, flow_in_update ? sy.U : sy.Q, sy.B, 8);
      }
    }
    if (pair_next) {
      run_projection_pair(ctx, s);
      ctx->pair_ready = true;
    } else {
      run_projection(ctx, s, 1, 1, two ? &full : nullptr, 1);
    }
    for (int h = 0; h < nh; ++h) {
      enter(h);
      launch_colmax(KRevDiff{sy, ctx->sl, ctx->w}, (sy.Q + 1) / 2, sy.B, 8);
      launch(KRevCheck{ctx->w, rev_tol}, sy.B);
      if (last) {
        // A(dt/2) at the new point: the momentum was projected there above, so P(p - dt/2 dh1_dpos) = p - dt/2 pg
        if (!opt.skip_end_kick) launch_rows(KKickPg{sy, ctx->sl, ctx->w, 1, 0, kick}, sy.Q, sy.B, 8);
        launch(KCommit{ctx->sl, ctx->w}, sy.B);
      } else {
        launch(KCommitInner{ctx->sl, ctx->w, ctx->d_ncommit}, sy.B);
      }
    }
  }
  if (two) {
    restore_view(ctx, full);
    streams_join();
    const int extra = n_inner;  // (state_eval_core ran once per half and inner step)
    ctx->counters[0] -= extra, ctx->counters[1] -= extra, ctx->counters[3] -= extra, ctx->counters[4] -= 1;
  }
  return 0;
}
static void step_finish(chmc_ctx* ctx, bool masked, int n_inner, int* status, int* iters_fwd, int* iters_bwd,
                        double* rev_err) {
  const Sys& sy = ctx->sy;
  bool any_failed = false;
  {  // one copy for the four per-chain outputs
    const size_t nb = (size_t)sy.B * (sizeof(double) + 3 * sizeof(int));
    ctx->h_out.resize(nb);
    d2h(ctx->h_out.data(), ctx->d_out, nb);
    const unsigned char* h = ctx->h_out.data();
    if (rev_err) memcpy(rev_err, h, sizeof(double) * sy.B);
    h += sizeof(double) * sy.B;
    if (status) memcpy(status, h, sizeof(int) * sy.B);
    if (iters_fwd) memcpy(iters_fwd, h + sizeof(int) * sy.B, sizeof(int) * sy.B);
    if (iters_bwd) memcpy(iters_bwd, h + 2 * sizeof(int) * sy.B, sizeof(int) * sy.B);
    const int* st = reinterpret_cast<const int*>(h);
    for (int c = 0; c < sy.B; ++c) any_failed = any_failed || st[c] > 0;
    if (n_inner > 1 && any_failed) {
      // a chain that failed after it had completed inner steps sits at an intermediate point: put the step's start
      // state back and re-evaluate its caches (a failed step leaves the chain state alone)
      std::vector<int> nc(sy.B), mask(sy.B);
      d2h(nc.data(), ctx->d_ncommit, sizeof(int) * sy.B);
      bool any = false;
      for (int c = 0; c < sy.B; ++c) any = (mask[c] = st[c] > 0 && nc[c] > 0) || any;
      if (any) {
        h2d(ctx->d_act, mask.data(), sizeof(int) * sy.B);
        ctx->last_active_null = true;
        ctx->last_active.clear();
        launch(KInnerRestore{sy, ctx->sl, ctx->d_q0, ctx->d_p0, ctx->d_act}, (long)sy.B * sy.Q, 8);
        // (work.dt keeps dt_i: the cached step sizes stay valid)
        launch(KBegin{ctx->w, ctx->d_act, nullptr, 1.0}, sy.B);
        state_eval(ctx, 0);
        // KBegin has overwritten the statuses of the step: put them back (they were copied to the host above)
        h2d(ctx->w.status, st, sizeof(int) * sy.B);
      }
    }
  }
  ctx->counters[5]++;
  // accepted chains: projected at the new point; failed chains keep their momentum; chains masked out by `active`
  // were not touched at all.  (A failed chain of a step that started from unprojected momenta keeps an unprojected one.)
  ctx->mom_tangent = ctx->mom_tangent || (!masked && !any_failed);
}
extern "C" int chmc_leapfrog_step(chmc_ctx* ctx, const double* dt, const int* active, int n_inner, int newton,
                                  double ctol, double ptol, double dtol, int max_iters, double rev_tol, int* status,
                                  int* iters_fwd, int* iters_bwd, double* rev_err) {
  CHMC_ENTER("chmc_leapfrog_step")
  if (!dt) return fail("chmc_leapfrog_step: dt is required");
  if (n_inner < 1) return fail("chmc_leapfrog_step: n_inner_step must be at least 1");
  if (step_enqueue(ctx, dt, active, nullptr, n_inner, Solver{newton, ctol, ptol, dtol, max_iters}, rev_tol)) return -1;
  step_finish(ctx, active != nullptr, n_inner, status, iters_fwd, iters_bwd, rev_err);
  CHMC_LEAVE("chmc_leapfrog_step")
}

// ------------------------------------------------------------------------------------------------------------
// chmc_leapfrog_steps: whole trajectories.  The reference integrates one chain at a time (scripts/utils.py:351-363): an
// integrator error ends THAT chain's trajectory (Mici's integration transitions: `for s in range(n_step): state =
// integrator.step(state)` inside a try).  Here: batched steps, a chain whose step fails sits out the rest of the call.
// (Round 3 also had an asynchronous per-chain-phase engine behind this entry point -- chains in different phases sharing
// launches through device-side masks.  It lost to the lock-step batch at every BASELINE shape (41 k vs 48 k steps/s at
// configs[1], 49 k vs 51 k at SIR) and was removed in round 4, when the per-chain retraction kernel (chmc_retract.h) gave
// single-block layouts what the engine was after -- every chain iterating as long as IT needs -- without launches.)
extern "C" int chmc_leapfrog_steps(chmc_ctx* ctx, const double* dt, const int* active, const int* n_steps, int n_steps_all,
                                   int n_inner, int newton, double ctol, double ptol, double dtol, int max_iters,
                                   double rev_tol, int* n_done, int* status, int* iters_fwd, int* iters_bwd, double* rev_err) {
  CHMC_ENTER("chmc_leapfrog_steps")
  if (!dt) return fail("chmc_leapfrog_steps: dt is required");
  if (n_inner < 1) return fail("chmc_leapfrog_steps: n_inner_step must be at least 1");
  if (!n_steps && n_steps_all < 0) return fail("chmc_leapfrog_steps: negative number of steps");
  const Sys& sy = ctx->sy;
  const int B = sy.B;
  const Solver s{newton, ctol, ptol, dtol, max_iters};
  if (traj_waves(ctx, n_inner, newton)) {
    // one launch: every chain walks its own steps in its own workgroup (k_traj_chain) and stops at its first failed step
    int longest = n_steps_all;
    if (n_steps) {
      longest = 0;
      for (int c = 0; c < B; ++c) longest = n_steps[c] > longest ? n_steps[c] : longest;
    }
    StepOptions opt;
    opt.n_steps_host = n_steps, opt.n_steps_all = longest, opt.want_n_done = true;
    if (step_enqueue(ctx, dt, active, nullptr, n_inner, s, rev_tol, opt)) return -1;
    std::vector<int> nd(B), st(B);
    d2h(nd.data(), ctx->d_ndone, sizeof(int) * B);
    step_finish(ctx, active != nullptr, 1, st.data(), iters_fwd, iters_bwd, rev_err);
    long long tot = 0;
    for (int c = 0; c < B; ++c) {
      if (st[c] < 0) nd[c] = 0;
      tot += nd[c] + (st[c] > 0);
    }
    if (n_done) memcpy(n_done, nd.data(), sizeof(int) * B);
    if (status) memcpy(status, st.data(), sizeof(int) * B);
    ctx->counters[5] += longest > 0 ? longest - 1 : 0;  // (step_finish has counted one batched step)
    (void)tot;
    CHMC_LEAVE("chmc_leapfrog_steps")
  }
  // chmc_leapfrog_step's batched steps; a chain whose step fails sits out the rest of the call
  std::vector<int> act(B), left(B), nd(B, 0), st_out(B, 0), itf(B, 0), itb(B, 0), st(B), f(B), b(B);
  std::vector<double> rv(B, 0.0), r1(B);
  int longest = 0;
  for (int c = 0; c < B; ++c) {
    act[c] = active ? (active[c] != 0) : 1;
    left[c] = act[c] ? (n_steps ? n_steps[c] : n_steps_all) : 0;
    if (left[c] < 0) left[c] = 0;
    st_out[c] = act[c] ? 0 : -1;
    longest = left[c] > longest ? left[c] : longest;
  }
  // Every chain takes the same number of steps (the integration transitions' case): the closing A(dt/2) of a step and the
  // opening A(dt/2) + flow of the next are one pass over the vectors (KKick2FlowPg) -- a chain that runs step k + 1 has
  // completed step k, and a chain whose step k + 1 fails keeps the fully kicked momentum that pass wrote back.  Needs a
  // momentum known to be tangent (the opening pass is then KKickFlowPg), one inner step and no block metric.
  const bool fuse_kicks = !n_steps && n_inner == 1 && !sy.m0;
  bool pending = false;
  for (int k = 0; k < longest; ++k) {
    std::vector<int> run(B);
    bool any = false;
    for (int c = 0; c < B; ++c) any = (run[c] = act[c] && left[c] > 0) || any;
    if (!any) break;
    const bool skip = fuse_kicks && ctx->mom_tangent && k + 1 < longest;
    // ... and the forward retraction of step k + 1 runs beside the reverse retraction of step k (KernelPlan::pair_retractions):
    // under the same conditions, where the merged scan launch fits the chip (pair_this_call, chmc_plan.h; the same bits)
    const bool pair = skip && ctx->halves == 1 && pair_this_call(ctx->plan, ctx->plan_in.wave_kernels, B, sy.K, ctx->num_cus);
    StepOptions opt;
    opt.skip_end_kick = skip, opt.pending_kick = pending, opt.pair_next = pair;
    if (step_enqueue(ctx, dt, run.data(), nullptr, n_inner, s, rev_tol, opt)) return -1;
    pending = skip;
    step_finish(ctx, true, n_inner, st.data(), f.data(), b.data(), r1.data());
    for (int c = 0; c < B; ++c) {
      if (!run[c]) continue;
      itf[c] += f[c], itb[c] += b[c];
      if (st[c] == 0 || st[c] == 3) rv[c] = r1[c];  // (the last step that reached the reversibility check)
      if (st[c] == 0) {
        nd[c] += 1, left[c] -= 1;
      } else {
        st_out[c] = st[c], left[c] = 0;
      }
    }
  }
  if (n_done) memcpy(n_done, nd.data(), sizeof(int) * B);
  if (status) memcpy(status, st_out.data(), sizeof(int) * B);
  if (iters_fwd) memcpy(iters_fwd, itf.data(), sizeof(int) * B);
  if (iters_bwd) memcpy(iters_bwd, itb.data(), sizeof(int) * B);
  if (rev_err) memcpy(rev_err, rv.data(), sizeof(double) * B);
  CHMC_LEAVE("chmc_leapfrog_steps")
}

// ---- the dynamic transition's per-chain decisions on the device (include/chmc.h)
static void tree_alloc(chmc_ctx* ctx) {
  if (ctx->have_tree) return;
  const int B = ctx->sy.B;
  TreeState& t = ctx->tree;
  t.h0 = alloc<double>(ctx, B), t.sub_logw = alloc<double>(ctx, B), t.sum_acc = alloc<double>(ctx, B), t.u = alloc<double>(ctx, B);
  t.alive = alloc<int>(ctx, B), t.run = alloc<int>(ctx, B), t.take = alloc<int>(ctx, B), t.n_step = alloc<int>(ctx, B);
  t.failed = alloc<int>(ctx, B), t.diverged = alloc<int>(ctx, B), t.n_running = alloc<int>(ctx, 1);
  t.logw = alloc<double>(ctx, B), t.u2 = alloc<double>(ctx, B);
  t.fwd = alloc<int>(ctx, B), t.at_pos = alloc<int>(ctx, B), t.at_neg = alloc<int>(ctx, B), t.moved = alloc<int>(ctx, B);
  t.depth = alloc<int>(ctx, B), t.done = alloc<int>(ctx, B), t.acc = alloc<int>(ctx, B), t.need = alloc<int>(ctx, B);
  t.counts = alloc<int>(ctx, 2);
  if (!ctx->d_tree_part) {
    const int ng = rowsum_groups(ctx->sy.Q);
    ctx->d_tree_part = alloc<double>(ctx, (size_t)B * ng * CHMC_ROWSUM_MAX);
    ctx->d_tree_out = alloc<double>(ctx, (size_t)B * CHMC_ROWSUM_MAX);
    ctx->d_tree_mask = alloc<int>(ctx, 2 * (size_t)B);
  }
  ctx->have_tree = true;
}
static void hamiltonian_enqueue(chmc_ctx* ctx) {
  const Sys& sy = ctx->sy;
  launch_rowsum(KNormRow{sy, ctx->sl}, sy.Q, sy.B, 2, ctx->w.part, 8);
  launch(KHamiltonian{sy, ctx->sl, ctx->w, ctx->npart_sum, ctx->d_ham}, sy.B);
}
extern "C" int chmc_tree_begin(chmc_ctx* ctx, double* h0) {
  CHMC_ENTER("chmc_tree_begin")
  tree_alloc(ctx);
  hamiltonian_enqueue(ctx);
  launch(KTreeBegin{ctx->tree, ctx->d_ham}, ctx->sy.B);
  if (h0) d2h(h0, ctx->tree.h0, sizeof(double) * ctx->sy.B);
  CHMC_LEAVE("chmc_tree_begin")
}
extern "C" int chmc_tree_subtree(chmc_ctx* ctx) {
  CHMC_ENTER("chmc_tree_subtree")
  if (!ctx->have_tree) return fail("chmc_tree_subtree: chmc_tree_begin has not been called");
  launch(KTreeSubBegin{ctx->tree}, ctx->sy.B);
  CHMC_LEAVE("chmc_tree_subtree")
}
extern "C" int chmc_tree_step(chmc_ctx* ctx, const double* dt, int n_inner, int newton, double ctol, double ptol,
                              double dtol, int max_iters, double rev_tol, const double* u_leaf, double max_delta_h,
                              void* sub_prop_q_dev, void* sub_sum_dev, void* ck_p_dev, void* ck_sum_dev, void* ck_end_dev,
                              int store_slot, int check_lo, int n_check, int* n_running) {
  CHMC_ENTER("chmc_tree_step")
  if (!ctx->have_tree) return fail("chmc_tree_step: chmc_tree_begin has not been called");
  if (!dt || !u_leaf || !sub_prop_q_dev || !sub_sum_dev || !ck_p_dev || !ck_sum_dev || !n_running)
    return fail("chmc_tree_step: null argument");
  if (n_inner < 1) return fail("chmc_tree_step: n_inner_step must be at least 1");
  if (n_check < 0 || n_check > CHMC_TREE_MAXCHK || check_lo < 0 || store_slot < -1)
    return fail("chmc_tree_step: checkpoint range out of bounds");
  const Sys& sy = ctx->sy;
  TreeState& t = ctx->tree;
  h2d(t.u, u_leaf, sizeof(double) * sy.B);
  if (step_enqueue(ctx, dt, nullptr, t.run, n_inner, Solver{newton, ctol, ptol, dtol, max_iters}, rev_tol)) return -1;
  hamiltonian_enqueue(ctx);
  launch(KTreeDecide{t, ctx->w.status, ctx->d_ham, max_delta_h}, sy.B);
  const int ng = rowsum_groups(sy.Q), nacc = 6 * n_check;
  launch_rowsum(KTreeLeaf{sy, ctx->sl, t.run, t.take, (double*)sub_prop_q_dev, (double*)sub_sum_dev, (double*)ck_p_dev,
                          (double*)ck_sum_dev, (double*)ck_end_dev, store_slot, check_lo, n_check},
                sy.Q, sy.B, nacc, ctx->d_tree_part, 8);
  if (nacc) {
    launch(KTreeLeafFinish{sy, ctx->sl, t.run, ctx->d_tree_part, ng, nacc, ctx->d_tree_out, (double*)ck_end_dev, check_lo},
           sy.B);
    launch(KTreeTurn{t, ctx->d_tree_out, nacc}, sy.B);
  }
  launch(KTreeCount{t, sy.B}, 1);
  step_finish(ctx, true, n_inner, nullptr, nullptr, nullptr, nullptr);  // (n_inner_step > 1: failed chains are put back)
  d2h(n_running, t.n_running, sizeof(int));
  CHMC_LEAVE("chmc_tree_step")
}
// ---- the per-doubling logic on the device (include/chmc.h)
extern "C" int chmc_tree_doubling_begin(chmc_ctx* ctx, const double* u_dir, const void* neg_q_dev, const void* neg_p_dev,
                                        const void* pos_q_dev, const void* pos_p_dev, void* sub_sum_dev, int* n_alive) {
  CHMC_ENTER("chmc_tree_doubling_begin")
  if (!ctx->have_tree) return fail("chmc_tree_doubling_begin: chmc_tree_begin has not been called");
  if (!u_dir || !neg_q_dev || !neg_p_dev || !pos_q_dev || !pos_p_dev || !sub_sum_dev || !n_alive)
    return fail("chmc_tree_doubling_begin: null argument");
  const Sys& sy = ctx->sy;
  TreeState& t = ctx->tree;
  h2d(t.u2, u_dir, sizeof(double) * sy.B);
  dev_zero(t.counts, sizeof(int) * 2);
  launch(KTreeDoubleBegin{t}, sy.B);
  dev_zero(sub_sum_dev, sizeof(double) * (size_t)sy.B * sy.Q);
  int cnt[2] = {0, 0};
  d2h(cnt, t.counts, sizeof(cnt));
  *n_alive = cnt[0];
  if (cnt[1] > 0) {
    // chains that extend their tree from the edge the context is not on: that edge's state comes back from the tree
    // vectors and its caches are re-evaluated (one batched evaluation per doubling at most); its momentum is tangent
    launch(KTreeRestoreEdge{sy, ctx->sl, t, (const double*)neg_q_dev, (const double*)neg_p_dev, (const double*)pos_q_dev,
                            (const double*)pos_p_dev}, (long)sy.B * sy.Q, 8);
    ctx->last_active_null = true;
    ctx->last_active.clear();
    begin_all(ctx, nullptr, t.need);
    state_eval(ctx, 0);
  }
  CHMC_LEAVE("chmc_tree_doubling_begin")
}
extern "C" int chmc_tree_doubling_end(chmc_ctx* ctx, const double* u_accept, int depth, void* prop_q_dev,
                                      const void* sub_prop_q_dev, void* sum_mom_dev, const void* sub_sum_dev, void* neg_q_dev,
                                      void* neg_p_dev, void* pos_q_dev, void* pos_p_dev, int* n_alive) {
  CHMC_ENTER("chmc_tree_doubling_end")
  if (!ctx->have_tree) return fail("chmc_tree_doubling_end: chmc_tree_begin has not been called");
  if (!u_accept || !prop_q_dev || !sub_prop_q_dev || !sum_mom_dev || !sub_sum_dev || !neg_q_dev || !neg_p_dev ||
      !pos_q_dev || !pos_p_dev || !n_alive)
    return fail("chmc_tree_doubling_end: null argument");
  const Sys& sy = ctx->sy;
  TreeState& t = ctx->tree;
  h2d(t.u2, u_accept, sizeof(double) * sy.B);
  launch(KTreeDoubleDecide{t, depth}, sy.B);
  const int ng = rowsum_groups(sy.Q);
  launch_rowsum(KTreeDoubleRows{sy, ctx->sl, t, (double*)prop_q_dev, (double*)sum_mom_dev, (double*)neg_q_dev,
                                (double*)neg_p_dev, (double*)pos_q_dev, (double*)pos_p_dev, (const double*)sub_prop_q_dev,
                                (const double*)sub_sum_dev},
                sy.Q, sy.B, 2, ctx->d_tree_part, 8);
  dev_zero(t.counts, sizeof(int) * 2);
  launch(KTreeDoubleFinish{t, ctx->d_tree_part, ng}, sy.B);
  int cnt[2] = {0, 0};
  d2h(cnt, t.counts, sizeof(cnt));
  *n_alive = cnt[0];
  CHMC_LEAVE("chmc_tree_doubling_end")
}
extern "C" int chmc_tree_get_doubling(chmc_ctx* ctx, int* moved, int* depth, double* logw) {
  CHMC_ENTER("chmc_tree_get_doubling")
  if (!ctx->have_tree) return fail("chmc_tree_get_doubling: chmc_tree_begin has not been called");
  const TreeState& t = ctx->tree;
  if (moved) d2h(moved, t.moved, sizeof(int) * ctx->sy.B);
  if (depth) d2h(depth, t.depth, sizeof(int) * ctx->sy.B);
  if (logw) d2h(logw, t.logw, sizeof(double) * ctx->sy.B);
  CHMC_LEAVE("chmc_tree_get_doubling")
}
extern "C" int chmc_tree_get(chmc_ctx* ctx, int* alive, int* run, int* n_step, int* failed, int* diverged, double* sub_logw,
                             double* sum_acc) {
  CHMC_ENTER("chmc_tree_get")
  if (!ctx->have_tree) return fail("chmc_tree_get: chmc_tree_begin has not been called");
  const size_t ni = sizeof(int) * ctx->sy.B, nd = sizeof(double) * ctx->sy.B;
  const TreeState& t = ctx->tree;
  if (alive) d2h(alive, t.alive, ni);
  if (run) d2h(run, t.run, ni);
  if (n_step) d2h(n_step, t.n_step, ni);
  if (failed) d2h(failed, t.failed, ni);
  if (diverged) d2h(diverged, t.diverged, ni);
  if (sub_logw) d2h(sub_logw, t.sub_logw, nd);
  if (sum_acc) d2h(sum_acc, t.sum_acc, nd);
  CHMC_LEAVE("chmc_tree_get")
}
extern "C" int chmc_tree_set_alive(chmc_ctx* ctx, const int* alive) {
  CHMC_ENTER("chmc_tree_set_alive")
  if (!ctx->have_tree || !alive) return fail("chmc_tree_set_alive: no tree / null argument");
  h2d(ctx->tree.alive, alive, sizeof(int) * ctx->sy.B);
  CHMC_LEAVE("chmc_tree_set_alive")
}

// ------------------------------------------------------------------------------------------------------------
// The one collective of the chain-parallel layer (SURVEY.md 8b / 8e): an all-gather of per-chain samples over RCCL.
// RCCL is bound at first use with dlopen (the library a PyTorch process has already loaded is reused), so that
// libchmc_hip.so has no link-time dependency on it.
#ifdef CHMC_WAVE_KERNELS
#include <dlfcn.h>
#include <rccl/rccl.h>
namespace {
struct Rccl {
  void* h = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclCommUserRank) CommUserRank = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl g_rccl;
int rccl_load() {
  if (g_rccl.h) return 0;
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;  // an instance that is already in the process (PyTorch's) under any of its names first
  for (int i = 0; !h && i < 3; ++i) h = dlopen(names[i], RTLD_NOW | RTLD_NOLOAD);
  for (int i = 0; !h && i < 3; ++i) h = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
  if (!h) return fail(std::string("RCCL not found: ") + dlerror());
  g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
  g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
  g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(h, "ncclAllGather");
  g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
  g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
  g_rccl.CommCount = (decltype(g_rccl.CommCount))dlsym(h, "ncclCommCount");
  g_rccl.CommUserRank = (decltype(g_rccl.CommUserRank))dlsym(h, "ncclCommUserRank");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy)
    return fail("RCCL library lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy");
  g_rccl.h = h;
  return 0;
}
int rccl_fail(const char* what, ncclResult_t r) {
  return fail(std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error"));
}
}  // namespace

extern "C" int chmc_comm_unique_id(void* id128) {
  if (!id128) return fail("chmc_comm_unique_id: null argument");
  if (rccl_load()) return -1;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclResult_t r = g_rccl.GetUniqueId((ncclUniqueId*)id128);
  return r == ncclSuccess ? 0 : rccl_fail("ncclGetUniqueId", r);
}
extern "C" int chmc_comm_init(chmc_ctx* ctx, const void* id128, int rank, int world) {
  CHMC_ENTER("chmc_comm_init")
  if (!id128 || world < 1 || rank < 0 || rank >= world) return fail("chmc_comm_init: bad argument");
  if (ctx->comm) return fail("chmc_comm_init: the context already has a communicator");
  if (rccl_load()) return -1;
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclComm_t comm = nullptr;
  ncclResult_t r = g_rccl.CommInitRank(&comm, world, id, rank);
  if (r != ncclSuccess) return rccl_fail("ncclCommInitRank", r);
  ctx->comm = comm, ctx->comm_rank = rank, ctx->comm_world = world;
  return 0;
}
extern "C" int chmc_gather_samples(chmc_ctx* ctx, const void* local_dev, long count, void* gathered_dev) {
  CHMC_ENTER("chmc_gather_samples")
  if (!ctx->comm) return fail("chmc_gather_samples: chmc_comm_init has not been called");
  if (!local_dev || !gathered_dev || count < 1) return fail("chmc_gather_samples: bad argument");
  ncclResult_t r = g_rccl.AllGather(local_dev, gathered_dev, (size_t)count, ncclDouble, (ncclComm_t)ctx->comm, g_stream);
  if (r != ncclSuccess) return rccl_fail("ncclAllGather", r);
  CHMC_LEAVE("chmc_gather_samples")
}
extern "C" int chmc_comm_info(chmc_ctx* ctx, int* world, int* rank) {
  CHMC_ENTER("chmc_comm_info")
  if (!ctx->comm) return fail("chmc_comm_info: chmc_comm_init has not been called");
  if (!g_rccl.CommCount || !g_rccl.CommUserRank) return fail("chmc_comm_info: the RCCL library lacks ncclCommCount / ncclCommUserRank");
  int n = 0, r = 0;
  ncclResult_t e = g_rccl.CommCount((ncclComm_t)ctx->comm, &n);
  if (e != ncclSuccess) return rccl_fail("ncclCommCount", e);
  e = g_rccl.CommUserRank((ncclComm_t)ctx->comm, &r);
  if (e != ncclSuccess) return rccl_fail("ncclCommUserRank", e);
  if (world) *world = n;
  if (rank) *rank = r;
  return 0;
}
extern "C" int chmc_comm_destroy(chmc_ctx* ctx) {
  CHMC_ENTER("chmc_comm_destroy")
  if (ctx->comm) {
    dev_sync();
    g_rccl.CommDestroy((ncclComm_t)ctx->comm);
    ctx->comm = nullptr, ctx->comm_world = 1, ctx->comm_rank = 0;
  }
  return 0;
}
#else
extern "C" int chmc_comm_unique_id(void*) { return fail("chmc_comm_unique_id: not available in the host emulation build"); }
extern "C" int chmc_comm_init(chmc_ctx*, const void*, int, int) { return fail("chmc_comm_init: not available in the host emulation build"); }
extern "C" int chmc_gather_samples(chmc_ctx*, const void*, long, void*) { return fail("chmc_gather_samples: not available in the host emulation build"); }
extern "C" int chmc_comm_info(chmc_ctx*, int*, int*) { return fail("chmc_comm_info: not available in the host emulation build"); }
extern "C" int chmc_comm_destroy(chmc_ctx*) { return 0; }
#endif
