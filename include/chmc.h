/* chmc.h -- C ABI of the MI355X-native batched constrained-HMC leapfrog library (libchmc_hip.so).
 *
 * The reference (thiery-lab/manifold-mcmc-for-diffusions) has no FFI of its own: its hot path is a set of
 * JAX-jitted closures behind Mici's duck-typed System / Integrator / projection-solver protocol.  Each entry
 * point below therefore replaces one of those closures / methods (file:line relative to the reference tree),
 * batched over `num_chains` independent chains.  All arrays are fp64, C-contiguous, chain-major; host
 * pointers unless the name ends in `_device`.  The caller owns its buffers for the duration of a call; the
 * context owns all device memory.  A context is bound to one device / one stream and is not re-entrant.
 *
 * Return value: 0 on success, <0 on API misuse or a HIP error (text via chmc_last_error()).  Numerical
 * outcomes are per-chain status codes, never a non-zero return.
 */
#ifndef CHMC_H
#define CHMC_H
#ifdef __cplusplus
extern "C" {
#endif

/* model ids: which `forward_func / generate_z / generate_x_0 / obs_func` set is compiled in
 * (sde/example_models/fhn.py, sde/example_models/sir.py) */
#define CHMC_MODEL_FHN 0
#define CHMC_MODEL_SIR 1
#define CHMC_MODEL_FHN_NOTEBOOK 2 /* FitzHugh-Nagumo with the priors of FitzHugh-Nagumo_example.ipynb (cells 7-18) */

/* per-chain status of a projection / leapfrog step (exception classes of the reference):
 *   0 ok
 *   1 ConvergenceError "did not converge"           sde/mici_extensions.py:1398-1402, 1472-1476
 *   2 ConvergenceError "diverged" (|c| > dtol, NaN) sde/mici_extensions.py:1393-1397, 1467-1471
 *   3 NonReversibleStepError                        mici ConstrainedLeapfrogIntegrator._step_b
 *  -1 chain was not active in the call */
#define CHMC_OK 0
#define CHMC_NOT_CONVERGED 1
#define CHMC_DIVERGED 2
#define CHMC_NON_REVERSIBLE 3
#define CHMC_INACTIVE (-1)

typedef struct chmc_ctx chmc_ctx;

/* Arguments of ConditionedDiffusionConstrainedSystem.__init__ (sde/mici_extensions.py:211-228) that can cross
 * a C ABI; the model callables are replaced by `model`.  The metric argument (identity, or block diagonal with a dense
 * dim_u x dim_u first block, :279-315) is set with chmc_set_metric. */
typedef struct chmc_config {
  int model;                  /* CHMC_MODEL_* */
  int num_obs;                /* T = y_seq.shape[0] (dim_y = 1) */
  int num_steps_per_obs;      /* S */
  int num_obs_per_subseq;     /* R; 0 or >= T: no partitioning (:321-324).  A block has its observation rows plus dim_x state
                               * rows (none in the last block) and at most 16 rows, for every model: R <= 14 with noisy, 15 with
                               * noiseless FitzHugh-Nagumo observations; R <= 13 / 14 for SIR.  chmc_create refuses more
                               * ("... not supported").  Row slots per block (dims[8] = RM): 6, 7 or 8 for blocks of at most 8
                               * rows, 16 for blocks of 9 to 16 rows */
  int noisy;                  /* generate_sigma (:353-358): 0 None (noiseless observations), 1 a number (`sigma`),
                               * 2 the model's generate_sigma_y(u) = exp(u[dim_z]) (fhn.py:46-47, sir.py:92-93):
                               * variable observation noise, dim_u = dim_z + 1, q = [u(dim_u) | v_0 | v_seq | n] */
  int use_gaussian_splitting; /* :273-278 */
  int num_chains;             /* B */
  int device;                 /* HIP device ordinal */
  double obs_interval;
  double sigma;               /* fixed observation-noise std (generate_sigma given as a Number, :354-358); noisy == 1 only */
  const double* y_seq;        /* [T]: shared by every chain (a data set and a fixed sigma per chain: chmc_set_observations) */
} chmc_config;

int chmc_create(const chmc_config* cfg, chmc_ctx** out);
void chmc_destroy(chmc_ctx* ctx);
const char* chmc_last_error(void);
const char* chmc_backend(void); /* "hip:gfx950" */

/* dims[16] = {B, Q, NV, U, X, T, S, num_partition, RM, Kmax, C(part 0), C(part 1), K(part 0), K(part 1), V, V0} */
int chmc_get_dims(const chmc_ctx* ctx, int* dims);
/* blocks of a partition (sde/mici_extensions.py:321-351): 12 ints per block
 * {obs0, nobs, first, last, row0, nrows, ny, col0, ncols, step0, nsteps, 0} */
int chmc_get_blocks(const chmc_ctx* ctx, int partition, int* out);

/* ---- chain state: ConditionedDiffusionHamiltonianState (sde/mici_extensions.py:1285-1320) ------------- */
/* Sets pos [B][Q], mom [B][Q] (may be NULL), x_obs_seq [B][T][X], partition, and evaluates everything the
 * reference caches on a state (jacob_constr_blocks, chol_gram_blocks, log_det_sqrt_gram, grad_log_det_sqrt_gram,
 * :1151-1184). */
int chmc_set_state(chmc_ctx* ctx, const double* q, const double* p, const double* x_obs_seq, int partition);
int chmc_get_state(chmc_ctx* ctx, double* q, double* p, double* x_obs_seq, int* partition);
/* Per-chain observations: many data sets of one shape (model, T, S, R) in one context.  chmc_create gives every chain the
 * same y_seq [T] and the same sigma; chmc_set_observations gives chain c the row y_seq[c] of y_seq [B][T] and, with
 * sigma != NULL, the fixed observation-noise std sigma[c] (sigma [B], every entry > 0).
 *   sigma is accepted in a context with noisy == 1 only.  NULL keeps the noise level(s) the context has.  With noisy == 0
 *   (no observation noise) or noisy == 2 (sigma = exp(u[dim_z]) stays a function of the chain's own u) only y_seq is per
 *   chain, and a non-NULL sigma is an error.
 *   The call INVALIDATES the chain state: the constraint function changed, so the caller sets or initialises a state
 *   afterwards (chmc_set_state, chmc_init_linear_interpolation, a finder), as after chmc_create.
 *   Calling it again replaces the data.  Every entry point then works with the chain's own data -- the constraint and all
 *   operators, the steps, trajectories and trees, the path scans, and row c of chmc_neg_log_dens_and_grad* /
 *   chmc_adam_objective_device (row c is judged against chain c's data).  A chain's results are bitwise those of a
 *   context that holds its (y, sigma) as shared data.
 * chmc_get_observations returns what the kernels use: y_seq [B][T] and sigma [B] (either may be NULL); in a context that
 * never had per-chain data the shared values, once per chain (sigma = 0 where noisy != 1). */
int chmc_set_observations(chmc_ctx* ctx, const double* y_seq, const double* sigma);
int chmc_get_observations(chmc_ctx* ctx, double* y_seq, double* sigma);
/* Data simulated from a prior draw, per chain, on the device.  For every chain c:
 *   pos = [u | v_0 | v_seq | n] ~ N(0, I): the keyed normals of chmc_fill_normal* for (seed, stream = chain_offset + c,
 *   draw = CHMC_SIMULATE_DRAW), so the data of a chain do not depend on how the chains are sharded;
 *   x_obs_seq = the path of that position at the observation times;
 *   y_c[t] = obs_func(x(t_obs)) + sigma_c n_t   (without the noise term for noisy == 0; sigma_c = exp(u[dim_z]) for
 *   noisy == 2, else the chain's fixed noise level: the context's, or the one chmc_set_observations gave it);
 *   mom = 0, the given partition, and the state caches evaluated, like chmc_set_state.
 * The data become the chain's observations as with chmc_set_observations (chmc_get_observations returns them).  Afterwards
 * the constraint is zero by construction: every chain sits on the manifold of its own data, at an exact draw from its own
 * posterior (simulation-based calibration needs no initial-state finder and no burn-in). */
#define CHMC_SIMULATE_DRAW (1ULL << 62) /* (momentum refresh: the transition number; the finders: 2^63 | ...) */
int chmc_simulate_observations_device(chmc_ctx* ctx, unsigned long long seed, int chain_offset, int partition);
/* Carrying positions between time resolutions: a context's num_steps_per_obs S is fixed at chmc_create, this call maps
 * positions of a context with S_src steps per observation interval to positions of `ctx` (the DESTINATION; S_dst = its S),
 * same model, T and noisy.  q_src_dev [B][U + V0 + T S_src V + (noisy ? T : 0)], q_dst_dev [B][Q], two distinct device
 * buffers.  u, v_0 and n are copied; v_seq is mapped per coarse step, which covers the m fine steps k = 0 .. m - 1:
 *   Euler-Maruyama components (SIR's three):       a = m^-1/2 sum_k a_k
 *   strong-order-1.5 pairs (a, b) = (v[j], v[dim_noise + j]) (both FitzHugh-Nagumo models, one pair), from
 *   Delta W = sqrt(delta) a = sum_k Delta W_k and
 *   Delta Z = delta^3/2 (a + b / sqrt 3) / 2 = sum_k Delta Z_k + h sum_k (m - 1 - k) Delta W_k   (h = delta / m):
 *                                                  a = m^-1/2 sum_k a_k
 *                                                  b = m^-3/2 sum_k [sqrt(3) (m - 1 - 2 k) a_k + b_k]
 *   These rows form A, one row per coarse normal, one column per fine normal of the coarse step, A A^T = I.
 *   S_src = m S_dst (m >= 2):  coarsening  v = A w; deterministic, seed and draw are ignored.
 *   S_dst = m S_src (m >= 2):  refinement  w = xi + A^T (v - A xi) with fresh xi ~ N(0, I): A w = v exactly -- the fine
 *     sequence drives a refinement of the SAME Brownian path -- and w ~ N(0, I) whenever v is.  xi of destination
 *     component j of chain c is column j of the keyed row of chmc_fill_normal* for (seed, stream = chain_offset + c,
 *     draw = CHMC_RESAMPLE_DRAW | draw), draw < 2^45 (the columns of u, v_0 and n go unused): bit 60 is disjoint from the
 *     momentum refresh, CHMC_PREDICT_DRAW (bit 61), CHMC_SIMULATE_DRAW (bit 62) and the finders (bit 63).
 *   S_src = S_dst:  a copy.  Any other ratio is an error; m need not be a power of two and may exceed 64.
 * The sums over k in A xi and A w are formed in ascending k whatever the launch geometry, so a chain's result depends on
 * (seed, draw, chain_offset + c) and its own row alone: any sharding gives the same bits.  Rows of chains with mask[c] == 0
 * (host [B]; NULL = all chains) are not touched.  The chain state of `ctx` is neither read nor changed.
 * Errors: NULL buffers, S_src < 1, S_src and S_dst not in an integer ratio, draw >= 2^45, chain_offset < 0. */
#define CHMC_RESAMPLE_DRAW (1ULL << 60)
int chmc_resample_q_device(chmc_ctx* ctx, const void* q_src_dev, int S_src, unsigned long long seed,
                           unsigned long long draw, int chain_offset, const int* mask, void* q_dst_dev);
/* A refined position is not on the fine manifold: the fine path differs from the coarse one by the discretisation error at
 * the observation times.  With observation noise (noisy == 1 or 2) the constraint fixes n, so the point is placed exactly,
 * without a solver.  For every chain c, from row c of q_dev [B][Q] (device):
 *   x_obs_seq = the path of the row at the observation times (scanned from q itself, never from a stored x_obs_seq);
 *   n_t := (y_t - obs_func(x(t_obs))) / sigma_c   (sigma_c: the context's, the chain's own after chmc_set_observations,
 *   or exp(u[dim_z]) for noisy == 2); pos = the row with this n; mom = 0, the given partition, and the state caches
 *   evaluated as by chmc_set_state: the state is bitwise that of chmc_set_state(q', NULL, x_obs', partition) for the
 *   q', x_obs' chmc_get_state returns.  Every observation row and every state row of the constraint is zero to rounding.
 *   moved[c] = max_t |n_t new - n_t given| (host [B]; may be NULL).
 * A context WITHOUT observation noise (noisy == 0) is not supported and returns an error: there x_obs_seq must satisfy
 * obs_func(x) = y and is part of the constraint's definition, so closing the defect is a projection, not a substitution:
 * chmc_set_state_project_device below. */
int chmc_set_state_solve_noise_device(chmc_ctx* ctx, const void* q_dev, int partition, double* moved);
/* The same placement WITHOUT observation noise (noisy == 0; a noisy context returns an error that names
 * chmc_set_state_solve_noise_device).  For every chain c with mask[c] != 0 (host [B]; NULL = all chains), from row c of
 * q_dev [B][Q] (device; never written):
 *   1. x_obs_seq = the path of the row at the observation times, scanned from q itself as above.
 *   2. defect[c] = max_t |y_t - obs_func(x_t)| (y_t: the chain's own after chmc_set_observations); then every x_t moves along
 *      obs_grad until the observation holds: x <- x + g (y - obs(x)) / (g . g), at most 8 rounds, done when
 *      |y - obs(x)| <= 8 eps max(1, |y|) -- one round for the linear obs_func of both FitzHugh-Nagumo models, Newton on exp
 *      for SIR.  A chain with an observation that does not get there or is not finite (SIR with y <= 0) gets status 2 and
 *      the solver is not run for it.
 *   3. The state (row, mom = 0, the pinned x_obs_seq, partition 0) is evaluated and the row is projected from it
 *      (state_prev = state, dt = 1) by the solver of chmc_project with the given settings: the sequence of
 *      chmc_gd_project_device.  On convergence the projected point becomes the chain's position.
 *   4. x_obs_seq of the converged chains is scanned again from the projected path, and the caches are evaluated in the given
 *      partition (for partition 1, the evaluation chmc_switch_partition ends with).  mom = 0.
 * The result is bitwise the state of chmc_set_state(q', NULL, x_obs', partition) for the q', x_obs' chmc_get_state returns.
 * Outputs (host [B], each may be NULL): status = the codes of chmc_project (CHMC_INACTIVE for chains outside the mask),
 * iters, defect, moved[c] = max_j |q placed - q given| (0 unless converged).
 * A chain that did not converge keeps the pinned, unprojected state: off the manifold and flagged by its status; the caller
 * retries it (another row under `mask`) or refuses to go on.  Chains outside the mask keep position, momentum and x_obs_seq;
 * the context as a whole ends in `partition`, and where the call passes through another partition than the one they were
 * evaluated in, their caches are evaluated again from those.  A context that holds no state yet takes all chains only.
 * A chain's result depends on its own row and data alone: any sharding gives the same bits.
 * Errors: NULL q_dev, partition out of range, max_iters < 0, a noisy context, a partial mask without a state. */
int chmc_set_state_project_device(chmc_ctx* ctx, const void* q_dev, int partition, const int* mask, int newton,
                                  double constraint_tol, double position_tol, double divergence_tol, int max_iters,
                                  int* status, int* iters, double* defect, double* moved);
/* find_initial_state_by_linear_interpolation (sde/mici_extensions.py:1479-1547) for all chains at once, on the
 * device: given u [B][U], v_0 [B][V0] and full states at the observation times x_obs_seq_init [B][T][X]
 * (generate_x_obs_seq_init of the scripts), solves per time step for the noise increments that make the discretised
 * path interpolate linearly between them (solve_for_v_seq :1503-1526), sets pos = [u | v_0 | v_seq | n = 0],
 * mom = 0, x_obs_seq = x_obs_seq_init and evaluates the state caches, like chmc_set_state. */
int chmc_init_linear_interpolation(chmc_ctx* ctx, const double* u, const double* v_0, const double* x_obs_seq_init,
                                   int partition);
/* system.metric = PositiveDefiniteBlockDiagonalMatrix((DensePositiveDefiniteMatrix(M_0), IdentityMatrix()))
 * (sde/mici_extensions.py:279-315): M_0 [U][U] symmetric positive definite acts on the u-part of the state, the rest
 * of the metric is the identity; NULL restores the identity metric.  Enters get_M_0_matrix (:794-798) in the Woodbury
 * cores, log_det_sqrt_metric_0 (:305-310, :809), delta_q = metric.inv @ delta_mu in both solvers (:1033-1041,
 * :1105-1113), h2 / dh2_dmom / h2_flow (:1202-1231), normal_space_component (:1243-1250) and sample_momentum
 * (:1256-1259).  Refreshes the cached factors of the current state when one has been set; the momentum is kept as it
 * is (project it again if it has to be tangent with respect to the new metric).  Errors: Gaussian splitting (the
 * reference raises ValueError :293-300), M_0 not symmetric positive definite. */
int chmc_set_metric(chmc_ctx* ctx, const double* M_0);
/* One M_0 per chain: M_0 [B][U][U], chain c's metric is blockdiag(M_0[c], identity) -- many posteriors in one context
 * (chmc_set_observations) whose global parameters u have different scales, each with the metric the reference's
 * OnlineBlockDiagonalMetricAdapter (scripts/utils.py, sde/mici_extensions.py:279-315) would give a system of its own.  The
 * interface knows nothing of groups: a caller with one matrix per group passes M[groups].  Every matrix is validated as
 * chmc_set_metric validates its one (symmetric positive definite, dim_u <= 8, no Gaussian splitting :293-300); the error
 * names the first offending chain and the context keeps the metric it had.  Like chmc_set_metric the call refreshes the
 * cached factors of the current state and keeps the momentum.  A chain's results are bitwise those of a context that holds
 * its matrix as the shared metric.  A later chmc_set_metric(ctx, M_0) returns every chain to one shared matrix, and
 * chmc_set_metric(ctx, NULL) to the identity.
 * chmc_get_metric writes the matrix each chain uses, M_0 [B][U][U]: the shared one once per chain, or the identity. */
int chmc_set_metrics(chmc_ctx* ctx, const double* M_0);
int chmc_get_metric(chmc_ctx* ctx, double* M_0);
/* One leaf of a batched dynamic-integration (no-U-turn) tree (the caller of integrator.step in the reference:
 * mici.transitions.MultinomialDynamicIntegrationTransition, scripts/utils.py:292-301), fused into one pass over the state
 * the last chmc_leapfrog_step produced.  The tree vectors stay with the caller as device buffers (plain pointers:
 * sub_prop_q, sub_sum [B][Q]; ck_p, ck_sum, ck_end [D][B][Q]).  For every chain with run[c] != 0:
 *   sub_sum += mom;  sub_prop_q = pos if take[c];  ck_p[store_slot], ck_sum[store_slot] = mom, sub_sum (store_slot >= 0);
 * and for the n_check nested sub-tree spans that end at this leaf (span k starts at the leaf recorded in checkpoint
 * check_lo + k; slot check_lo holds the largest span, and the span of slot check_lo + k + 1 is the right half of span k):
 *   out[c][6k], out[c][6k + 1] = dh_dmom(ck_p[check_lo + k]) . rho, dh_dmom(mom) . rho with rho = sub_sum -
 *   ck_sum[check_lo + k] + ck_p[check_lo + k] (momentum sum of the span): the two sides of the no-U-turn criterion
 *   (dh_dmom = metric.inv @ mom :1204-1208);
 *   with ck_end != NULL, for k < n_check - 1 (spans of four leaves or more), Mici's additional sub-tree checks
 *   (do_extra_subtree_checks, the transition's default) across the two halves of the span -- first leaf a, last leaf m
 *   of the left half, first leaf m + 1 of the right half, this leaf b:
 *   out[c][6k + 2], out[c][6k + 3] = dh_dmom(p_a) . rho1, dh_dmom(p_{m+1}) . rho1, rho1 = momenta of a..m plus p_{m+1};
 *   out[c][6k + 4], out[c][6k + 5] = dh_dmom(p_m) . rho2, dh_dmom(p_b) . rho2,     rho2 = momenta of m+1..b plus p_m;
 *   afterwards ck_end[check_lo] = mom (this leaf ends the left half of the next larger span starting at slot check_lo).
 *   Entries that are not computed are 0.
 * out is [B][6 n_check] on the host (zeros for chains that did not run; may be NULL when n_check == 0); n_check <= 10.
 * Sums are formed in a fixed order (no atomics).  run / take are host arrays (take is decided by the caller from
 * chmc_hamiltonian of the same state: multinomial sampling of the sub-tree's proposal); chmc_tree_step is the variant
 * that takes these decisions on the device. */
int chmc_tree_leaf(chmc_ctx* ctx, const int* run, const int* take, void* sub_prop_q_dev, void* sub_sum_dev,
                   void* ck_p_dev, void* ck_sum_dev, void* ck_end_dev, int store_slot, int check_lo, int n_check,
                   double* out);
/* The per-chain decisions of the same transition taken on the device, so that a leaf of the batched trees costs one
 * call and one 4-byte read-back instead of three host round trips (mici _build_tree's base case and its termination
 * logic, scripts/utils.py:292-301).  The library keeps per chain: h0 (Hamiltonian at the tree's root), alive (the tree
 * can still grow), run (the chain takes part in the current sub-tree), the sub-tree's multinomial log weight, the
 * number of leaves, the sum of the leaves' acceptance probabilities min(1, exp(h0 - h)), and the integrator-error /
 * divergence flags.
 *   chmc_tree_begin    h0 = Hamiltonian of the current states (returned in h0[B] if not NULL), alive = isfinite(h0),
 *                      counters and flags cleared;
 *   chmc_tree_set_alive overrides alive[B] (the caller ends a chain's tree on its whole-tree criterion);
 *   chmc_tree_subtree  run = alive, sub-tree weight = 0 (log weight -inf);
 *   chmc_tree_step     for the chains with run != 0: one chmc_leapfrog_step (same arguments), then
 *                      integrator error (status != 0) -> failed, alive = run = 0; else delta_h = h - h0 > max_delta_h or
 *                      NaN -> diverged, alive = run = 0; else the leaf joins the sub-tree: n_step += 1, sum_acc +=
 *                      min(1, exp(h0 - h)), weight += exp(-h), take = u_leaf[c] < exp(-h) / weight; then the
 *                      bookkeeping of chmc_tree_leaf with these run / take (same buffers and slot arguments), and a
 *                      negative criterion value on any checked span sets alive = run = 0 (no-U-turn termination).
 *                      *n_running = number of chains with run != 0 afterwards;
 *   chmc_tree_get      per-chain state to the host (any pointer may be NULL). */
int chmc_tree_begin(chmc_ctx* ctx, double* h0);
int chmc_tree_set_alive(chmc_ctx* ctx, const int* alive);
int chmc_tree_subtree(chmc_ctx* ctx);
int chmc_tree_step(chmc_ctx* ctx, const double* dt, int n_inner_step, int newton, double constraint_tol, double position_tol,
                   double divergence_tol, int max_iters, double reverse_check_tol, const double* u_leaf, double max_delta_h,
                   void* sub_prop_q_dev, void* sub_sum_dev, void* ck_p_dev, void* ck_sum_dev, void* ck_end_dev,
                   int store_slot, int check_lo, int n_check, int* n_running);
int chmc_tree_get(chmc_ctx* ctx, int* alive, int* run, int* n_step, int* failed, int* diverged, double* sub_logw,
                  double* sum_acc);
/* The per-doubling logic of the same transition on the device (mici MultinomialDynamicIntegrationTransition.sample: the
 * loop over tree depths around _build_tree), so that a doubling costs two calls with an 8-byte read-back each instead of
 * per-chain host logic on [B][Q] vectors.  The tree vectors stay the caller's device buffers [B][Q].
 *   chmc_tree_doubling_begin  for every live chain: direction fwd = u_dir[c] < 0.5; if the context's chain state sits on
 *                             the other tree edge, the edge (neg or pos q, p) is copied into the state and its caches
 *                             are re-evaluated; a new sub-tree begins (chmc_tree_subtree), sub_sum = 0.
 *                             *n_alive = chains whose tree can still grow (0: the transition is over).
 *   (2^depth chmc_tree_step calls with dt = +-step_size by the same comparison)
 *   chmc_tree_doubling_end    for every chain whose sub-tree completed (run != 0): biased progressive sampling, the
 *                             sub-tree's proposal replaces the tree's if u_accept[c] < min(1, exp(sub_logw - logw));
 *                             logw = logaddexp(logw, sub_logw); sum_mom += sub_sum; the chain's current state becomes
 *                             the tree's edge on the side of the doubling; then the no-U-turn criterion on the whole tree,
 *                             dh_dmom(neg edge) . sum_mom < 0 or dh_dmom(pos edge) . sum_mom < 0 -> alive = 0 (sums in a
 *                             fixed order).  *n_alive as above.
 *   chmc_tree_get_doubling    per chain: whether the proposal moved, doublings completed, log weight of the tree. */
int chmc_tree_doubling_begin(chmc_ctx* ctx, const double* u_dir, const void* neg_q_dev, const void* neg_p_dev,
                             const void* pos_q_dev, const void* pos_p_dev, void* sub_sum_dev, int* n_alive);
int chmc_tree_doubling_end(chmc_ctx* ctx, const double* u_accept, int depth, void* prop_q_dev, const void* sub_prop_q_dev,
                           void* sum_mom_dev, const void* sub_sum_dev, void* neg_q_dev, void* neg_p_dev, void* pos_q_dev,
                           void* pos_p_dev, int* n_alive);
int chmc_tree_get_doubling(chmc_ctx* ctx, int* moved, int* depth, double* logw);
int chmc_set_momentum(chmc_ctx* ctx, const double* p);
int chmc_get_state_device(chmc_ctx* ctx, void* q_dev, void* p_dev);  /* device-to-device copies */
int chmc_set_momentum_device(chmc_ctx* ctx, const void* p_dev);
/* system.sample_momentum(state, rng) (:1256-1259) with a device-side counter-based generator: mom = P(q) n,
 * n ~ N(0, I) from Philox4x32-10 keyed by `seed`, counter (component pair, `draw`, chain_offset + chain): the
 * stream of a chain does not depend on how chains are sharded over GPUs. */
int chmc_sample_momentum(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset);
/* Caller support for an accept / reject step around a trajectory (the role of Mici's transitions, which keep the
 * start state and discard a rejected or failed trajectory): device-side copy of (pos, mom) and masked restore
 * (mask [B], non-zero = restore; the state caches of restored chains are re-evaluated).  chmc_get_head copies the
 * first n components of every chain's position ([B][n]: u and v_0 live there, cf. trace_func of the scripts). */
int chmc_snapshot(chmc_ctx* ctx);
int chmc_restore(chmc_ctx* ctx, const int* mask);
/* The same from caller-held device buffers q_dev, p_dev [B][Q] (e.g. the tree edges of a dynamic transition): chains
 * with mask != 0 get (pos, mom) from the buffers and their state caches re-evaluated; momentum_is_tangent tells the
 * library whether those momenta lie in the cotangent space of their positions (see chmc_leapfrog_step). */
int chmc_restore_device(chmc_ctx* ctx, const void* q_dev, const void* p_dev, const int* mask, int momentum_is_tangent);
int chmc_get_head(chmc_ctx* ctx, int n, double* out);
/* system.update_x_obs_seq(state) (:1240-1241, :384-397) */
int chmc_update_x_obs_seq(chmc_ctx* ctx);
/* SwitchPartitionTransition.sample (:1279-1282): partition = (partition + 1) % num_partition, update x_obs_seq,
 * re-evaluate the state caches */
int chmc_switch_partition(chmc_ctx* ctx);
/* The latent path x(t) of every chain: generate_from_model's x_seq (FitzHugh-Nagumo_example.ipynb:316-335), the one function
 * of that notebook the samplers' head traces cannot give.  For a stride >= 1 that divides num_steps_per_obs,
 * NP = num_obs * num_steps_per_obs / stride + 1 points per chain: point 0 is x_0 = generate_x_0(generate_z(u), v_0), point p
 * the state after step p * stride of the recursion from x_0 over the whole chain; observation time t (1-based) is point
 * t * num_steps_per_obs / stride.  x_seq is [B][NP][X].
 *   q != NULL (host [B][Q]): the path of those positions, one sequential recursion per chain.
 *   q == NULL: the path of the chains' current states.  Where the library keeps the compact rows (CHMC_COMPACT_ROWS, the
 *   default) the stored trajectories of the states seed a time-parallel pass over the whole chain, as in
 *   chmc_switch_partition; the result equals the sequential recursion to rounding.  sweeps (host [B], may be NULL): sweeps
 *   that pass needed per chain, 0 where the sequential recursion ran.
 * Errors: stride < 1 or not a divisor of num_steps_per_obs; no state set (q == NULL). */
int chmc_generate_x_seq(chmc_ctx* ctx, const double* q, int stride, double* x_seq, int* sweeps);
/* The same for the current states into a caller-held device buffer x_seq_dev [B][NP][X] (FitzHugh-Nagumo_example.ipynb:316-335). */
int chmc_generate_x_seq_device(chmc_ctx* ctx, int stride, void* x_seq_dev, int* sweeps);
/* Running posterior moments of the path (the bands the notebook draws from stored generate_from_model outputs,
 * FitzHugh-Nagumo_example.ipynb:316-335 and :401, without storing the draws): the path of the current states goes to the
 * scratch buffer x_seq_dev [B][NP][X], then every chain with mask[c] != 0 (host [B]; NULL = all) folds it into its moments by
 * Welford's recurrence over the X state components and obs_func(x) (X + 1 channels):
 *   n[c] += 1;  d = v - mean;  mean += d / n[c];  m2 += d (v - mean).
 * n_dev [B] (long long), mean_dev, m2_dev [B][NP][X + 1] are the caller's device buffers, zero before the first call; the
 * buffers of chains with mask[c] == 0 are not touched. */
int chmc_path_stats_update_device(chmc_ctx* ctx, int stride, const int* mask, void* x_seq_dev, void* n_dev, void* mean_dev,
                                  void* m2_dev);

/* Posterior predictive simulation on the device: forecasts beyond the last observation and replicated data sets, folded into
 * running moments per chain.  For chain c with current position q = [u | v_0 | v_seq | n], z = generate_z(u) and
 * dl = obs_interval / S, replicate r = 0 .. n_rep - 1 integrates horizon * S steps of the model's one-step map from
 *   origin = 0 (forecast):    x_T, the state after step T S of the chain's path as chmc_generate_x_seq* defines it (the
 *                             path is rebuilt from q by the path scan, never read from a possibly stale x_obs_seq, so the call is
 *                             right after leapfrog steps with no partition switch in between); point p has time
 *                             T obs_interval + p stride dl,
 *   origin = 1 (replication): x_0 = generate_x_0(z, v_0); point p has time p stride dl (horizon = T, stride = S: a
 *                             replicated data set for a posterior predictive check),
 * driven by fresh normals w_r = [v (horizon S V) | eps (NPF)] and emits the NPF = horizon S / stride points p = 1 .. NPF
 * (stride >= 1 divides S).  Normals 2 j, 2 j + 1 of w_r are the pair j of the keyed stream of chmc_fill_normal*:
 *   (seed, stream = chain_offset + c, draw_key = CHMC_PREDICT_DRAW | (draw << 16) | r),   draw < 2^45, n_rep <= 65536,
 * disjoint from the momentum refresh (small draw indices), CHMC_SIMULATE_DRAW (bit 62) and the finders (bit 63).  Without
 * observation noise (noisy == 0) w_r has no eps part.
 * Channels per point, XC = X + 2: the X state components, obs_func(x), and y_rep = obs_func(x) + sigma_c eps_p with
 * sigma_c the chain's observation-noise std (the context's, the chain's own after chmc_set_observations, or exp(u[Z]) with
 * variable noise); noisy == 0: y_rep = obs_func(x).
 * Running moments per (chain, point, channel): n_dev [B] (long long, counts replicate paths), mean_dev, m2_dev
 * [B][NPF][XC] are the caller's device buffers, zero before the first call.  One call merges its replicates in groups of 64
 * consecutive replicates, in group order (the last group may be partial): for a group of R_g values v,
 *   m_g = sum(v) / R_g,  s_g = sum((v - m_g)^2),  then Chan's merge
 *   n' = n + R_g;  d = m_g - mean;  mean += d R_g / n';  m2 += s_g + d^2 n R_g / n'.
 * Non-finite values are not filtered: a replicate that leaves the finite range makes that point's mean and m2 (and every
 * later point's it reaches) non-finite from then on, and counts in no CDF level.
 * Predictive CDF of y_rep: with n_levels > 0 and levels (host, n_levels increasing doubles),
 *   cdf_dev [B][NPF][n_levels] (long long) += #{r : y_rep_r <= levels[l]}.
 * Kept paths: paths_dev [B][n_keep][NPF][XC] receives the first n_keep <= n_rep replicates of this call (overwritten by
 * every call); n_keep = 0 or a NULL pointer keeps none.
 * mask (host [B], NULL = all): no buffer of a chain with mask[c] == 0 is touched.
 * A chain's outputs depend on (seed, draw, chain_offset + c), its own state and data alone -- not on B, the other chains or
 * the launch geometry: any sharding of the chains gives the same bits.
 * Errors: no state set; horizon < 1; stride < 1 or not a divisor of num_steps_per_obs; origin not 0 or 1; n_rep outside
 * [1, 65536]; n_keep outside [0, n_rep]; draw >= 2^45; n_levels < 0, or n_levels > 0 with NULL levels or cdf_dev; levels
 * not increasing; a NULL n_dev, mean_dev or m2_dev.
 * chmc_predict_points: NPF into *n_points and, where times != NULL, the NPF point times. */
#define CHMC_PREDICT_DRAW (1ULL << 61)
int chmc_predict_points(const chmc_ctx* ctx, int horizon, int stride, int origin, int* n_points, double* times);
int chmc_predict_device(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset, int horizon,
                        int stride, int origin, int n_rep, const int* mask, int n_levels, const double* levels, void* n_dev,
                        void* mean_dev, void* m2_dev, void* cdf_dev, void* paths_dev, int n_keep);

/* Scoring observations that arrived behind the fit, and a state for the longer record.  A context's num_obs T is fixed at
 * chmc_create; this call, on the context that holds the fit of y_1..T, weighs forecast candidates by the H = horizon
 * observations y_future [B][H] (host) that arrived next.  For chain c, with sigma_c as chmc_predict_device defines it:
 *   candidates  r = 0 .. n_cand - 1 is forecast replicate r of chmc_predict_device(seed, draw, chain_offset, horizon,
 *               stride = S, origin = 0): the same start state x_T (rebuilt from the position by the path scan, never read
 *               from x_obs_seq), the same keyed stream (seed, chain_offset + c, CHMC_PREDICT_DRAW | draw << 16 | r) and the
 *               same recursion, so o_p^r = obs_func(x) at point p = 1 .. H has the same bits; the eps part of the stream is
 *               not used.
 *   weights     n_p^r = (y_future[c][p-1] - o_p^r) / sigma_c;
 *               logw_r = -1/2 sum_p (n_p^r)^2 - H (log sigma_c + 1/2 log 2 pi), the sum in ascending p (each term added by
 *               one fused multiply-add, the affine map by another); a candidate with a non-finite o_p has logw_r = -inf.
 *   score       m = max_r logw_r;  s = sum_r exp(logw_r - m) in ascending r, always in that one order;
 *               log_pred[c] = m + log s - log n_cand  = log p(y_{T+1..T+H} | y_{1..T}, this draw), by n_cand replicates.
 *               Every candidate -inf: log_pred[c] = -inf, picked[c] = -1, and the chain's tail_dev row is not written.
 *   pick        z = normal 0 of the keyed row (seed, chain_offset + c, CHMC_FUTURE_DRAW | draw) of chmc_fill_normal*;
 *               u = Phi(z) = 1/2 erfc(-z / sqrt 2); picked[c] = the smallest r whose running sum of exp(logw_r' - m) over
 *               r' <= r exceeds u s (if rounding leaves none: the last candidate with a finite weight) -- a candidate drawn in
 *               proportion to its weight.
 *   tail        row c of tail_dev [B][H S V + H] = [ v of the picked candidate: the H S V step normals, the bits
 *               chmc_fill_normal* returns for its key | n_p of the picked candidate (H) ].  Spliced behind the chain's
 *               [u | v_0 | v_seq] and [n], it is a position of the context with T + H observations whose observation-noise
 *               part already solves the new constraint rows to rounding (chmc_set_state_solve_noise_device places it).
 * Bit 59: CHMC_FUTURE_DRAW | draw, draw < 2^45, has bits 60 - 63 clear and is therefore disjoint from CHMC_RESAMPLE_DRAW
 * (bit 60), CHMC_PREDICT_DRAW (bit 61; its draw << 16 reaches bit 60 but never clears bit 61), CHMC_SIMULATE_DRAW (bit 62)
 * and the finders (bit 63); the momentum refresh uses the transition number, far below 2^59.
 * log_pred [B] and picked [B] (may be NULL) are host arrays; logw_dev [B][n_cand] (may be NULL) receives the weights;
 * tail_dev may be NULL.  mask (host [B], NULL = all): no buffer of a chain with mask[c] == 0, nor its log_pred / picked
 * entry, is touched.  A chain's outputs depend on (seed, draw, chain_offset + c), its own state and its own data alone: any
 * sharding of the chains gives the same bits.  The chain state is not changed.
 * Two forms: a work item per (chain, candidate) (KFutureScore, the default: the faster one at every measured shape, DESIGN.md
 * section 4.13) and, under CHMC_FUTURE_WAVE=1 where the compact rows are allocated, a wavefront per (chain, group of 64
 * candidates) with a lane per candidate (k_future_score).  Neither reduces over candidates and both use the same
 * accumulator, so the two forms give the same bits.
 * Errors: no state set; noisy == 0 (not supported: without observation noise the weights are degenerate, and the state
 * would be placed by the projection of chmc_set_state_project_device, not through n); horizon < 1; n_cand outside [1, 65536];
 * draw >= 2^45; chain_offset < 0; a NULL y_future or log_pred; a non-finite y_future. */
#define CHMC_FUTURE_DRAW (1ULL << 59)
int chmc_score_future_device(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset, int horizon,
                             const double* y_future, int n_cand, const int* mask, double* log_pred, int* picked,
                             void* logw_dev, void* tail_dev);

/* Path-wise event summaries on the device: functionals of one whole path (its peak and the time of it, first passages,
 * up-crossings, integrals), which no pointwise summary gives.
 * The event vector.  Inputs: one channel's values v_p at the points p0 <= p <= p1 (an inclusive window of point indices),
 * the point times t_p with constant spacing h, and L increasing thresholds theta_0 < ... < theta_{L-1}, 0 <= L <= 8.
 * NE = 5 + 3 L doubles, in this order:
 *   max, t_max     max_p v_p and the time of the FIRST point attaining it
 *   min, t_min     min_p v_p and the time of the FIRST point attaining it
 *   integral       h (sum_{p = p0 .. p1} v_p - (v_p0 + v_p1) / 2), the trapezoid rule; 0 for a one-point window
 *   then per threshold l = 0 .. L - 1:
 *   upcross_l      #{p0 < p <= p1 : v_{p-1} < theta_l <= v_p}, as a double
 *   t_first_l      the time of the first p in [p0, p1] with v_p >= theta_l; NaN if there is none
 *   time_above_l   h #{p0 < p <= p1 : v_p >= theta_l}
 * If any v_p of the window is not finite, all NE entries are NaN.  Values outside the window never matter.
 *
 * chmc_path_events_device: the events of the latent path.  x_seq_dev [B][n_points][X] is any path buffer on the device, for
 * example the scratch of chmc_path_stats_update_device / chmc_generate_x_seq_device at the same stride; point p has time
 * t_p = p h with h = stride dl, dl = obs_interval / num_steps_per_obs.  channel in [0, X]: a state component, or X for
 * obs_func(x).  thresholds: host, n_thresholds doubles.  events_dev [B][NE] receives the event vectors; mask (host [B],
 * NULL = all): the row of a chain with mask[c] == 0 is not touched.
 * With the compact rows allocated (the default) a wavefront per chain reduces the window (k_path_events: the integral's
 * per-lane partial sums are added in one fixed order), under CHMC_COMPACT_ROWS=0 a work item per chain takes the points in
 * order (KPathEvents); the two may differ in `integral` by rounding alone, every other entry is identical.  A chain's
 * events depend on its own path alone: any sharding of the chains gives the same bits.
 * Errors: NULL buffers; stride < 1 or not a divisor of num_steps_per_obs; channel outside [0, X]; n_points < 1; a window
 * that is not 0 <= p0 <= p1 < n_points; n_thresholds outside [0, 8]; thresholds NULL or not increasing.
 *
 * chmc_predict_events_device: chmc_predict_device (same arguments, same keyed streams, same replicate paths; it leaves the
 * same moments, CDF counts and kept paths, bit for bit) which also evaluates the event vector of every replicate.
 * channel in [0, X + 1] (X + 1: y_rep); the window is over the emitted points, 0-based and inclusive, 0 <= p0 <= p1 < NPF;
 * the times are those of chmc_predict_points and h = stride dl.
 *   events_dev [B][n_rep][NE]  the replicates' event vectors of this call (overwritten by every call); NULL keeps none.
 *   en_dev [B][NE] (long long), emean_dev, em2_dev [B][NE]: running moments per chain and entry over the FINITE values,
 *   the caller's device buffers, zero before the first call.  One call merges, per entry, its groups of 64 consecutive
 *   replicates in group order, as the predictive moments above: with R_g the number of finite values v of the group
 *   (a group with none merges nothing), m_g = sum(v) / R_g, s_g = sum((v - m_g)^2), both sums in replicate order, then
 *   Chan's merge with the entry's own count n = en.  So P(threshold l reached in the window) = en[t_first_l] / n_dev.
 * Both forms of the predictive evaluate a replicate's events by the same code on the replicate's own path and share the fold,
 * and a chain's events depend on (seed, draw, chain_offset + c), its own state and data alone: any sharding gives the same bits.
 * Errors: those of chmc_predict_device, and: channel outside [0, X + 1]; a bad window; n_thresholds outside [0, 8];
 * thresholds NULL or not increasing; a NULL en_dev, emean_dev or em2_dev. */
int chmc_path_events_device(chmc_ctx* ctx, const void* x_seq_dev, int n_points, int stride, int channel, int p0, int p1,
                            int n_thresholds, const double* thresholds, const int* mask, void* events_dev);
int chmc_predict_events_device(chmc_ctx* ctx, unsigned long long seed, unsigned long long draw, int chain_offset, int horizon,
                               int stride, int origin, int n_rep, const int* mask, int n_levels, const double* levels,
                               void* n_dev, void* mean_dev, void* m2_dev, void* cdf_dev, void* paths_dev, int n_keep,
                               int channel, int p0, int p1, int n_thresholds, const double* thresholds, void* events_dev,
                               void* en_dev, void* emean_dev, void* em2_dev);

/* ---- per-op entry points, evaluated at the current state ------------------------------------------------
 * Internally the library keeps the dc/dv rows of a state in a compact factored form (per step a row-independent X x V
 * matrix, per observation interval the RM x X adjoint frame; DESIGN.md section 4 "Compact rows") and the stepping path
 * never writes the full rows of blocks with at most 8 rows (nor of few 16-row blocks per chain).  The entry points below that return rows or multiply by them
 * rebuild the row-slot array first (one extra pass, only when called); results are the same to rounding.
 *
 * Environment switches: the table of every variable the library reads, and when, is in csrc/chmc_plan.h (read_switches is
 * the one place that reads them).  Defaults are chosen from the layout (blocks per chain, block length, rows) alone, never
 * from the number of chains -- the one exception, the execution model of single-block layouts (CHMC_RETRACT_KERNEL), chooses
 * between bit-identical paths; the per-chain kernels it selects exist for the SIR models only, a FitzHugh-Nagumo layout with
 * one 16-row block per chain always runs the batched launches and the switch is a no-op there --, so a chain's results do not depend on the shard it runs in (bitwise:
 * tests/test_hip_parity.py::test_results_do_not_depend_on_the_shard_size).  Pinning a switch to a non-default value changes
 * bits at the rounding level (summation order; the time-parallel scan equals the sequential recursion to about 1e-15
 * relative after its final sweep, not bitwise), never statuses. */
int chmc_constr(chmc_ctx* ctx, double* c);                                  /* :473-519, :1151-1155  [B][C] */
/* :521-624, :1157-1161.  dc_du [B][C][U]; dc_dv [B][RM][NV] row-slot layout (slot i = row i of the block that
 * owns the column); dc/dn is sigma on observation rows (:601-608). */
int chmc_jacob_constr_blocks(chmc_ctx* ctx, double* dc_du, double* dc_dv);
int chmc_chol_gram_blocks(chmc_ctx* ctx, double* chol_C, double* chol_D);   /* :626-687  [B][U][U], [B][K][RM][RM] */
int chmc_log_det_sqrt_gram(chmc_ctx* ctx, double* out);                     /* :800-820, :1169-1171  [B] */
int chmc_grad_log_det_sqrt_gram(chmc_ctx* ctx, double* grad);               /* :1143-1146, :1173-1184  [B][Q] */
int chmc_lmult_by_jacob_constr(chmc_ctx* ctx, const double* vct, double* out);   /* :822-877  [B][Q] -> [B][C] */
int chmc_rmult_by_jacob_constr(chmc_ctx* ctx, const double* vct, double* out);   /* :879-913  [B][C] -> [B][Q] */
int chmc_lmult_by_inv_gram(chmc_ctx* ctx, const double* vct, double* out);       /* :915-942  [B][C] -> [B][C] */
int chmc_normal_space_component(chmc_ctx* ctx, const double* vct, double* out);  /* :983-993, :1243-1250 */
int chmc_project_onto_cotangent_space(chmc_ctx* ctx);  /* :1252-1254, in place on the state's momentum */
int chmc_hamiltonian(chmc_ctx* ctx, double* h);        /* :1186-1202  [B][3] = {h1 + h2, q.q/2, p.p/2} */

/* conditioned_diffusion_neg_log_dens_and_grad (sde/mici_extensions.py:82-205), the target of the reference's
 * unconstrained-HMC comparator, for B independent points: q [B][QH], QH = U + V0 + T S V (no observation-noise part),
 *   value [B] = 1/2 sum_t ((y_t - obs_func(x_t)) / sigma)^2 + T log sigma (+ 1/2 q.q unless use_gaussian_splitting),
 *   grad [B][QH] (may be NULL).  Needs a context with observation noise; does not touch the chain states. */
int chmc_neg_log_dens_and_grad(chmc_ctx* ctx, const double* q, int use_gaussian_splitting, double* value, double* grad);
/* The same with q_dev [B][U + V0 + T S V] and grad_dev (may be NULL) in device memory; `value` [B] on the host. */
int chmc_neg_log_dens_and_grad_device(chmc_ctx* ctx, const void* q_dev, int use_gaussian_splitting, double* value,
                                      void* grad_dev);
/* The device-resident loop of find_initial_state_by_gradient_descent_noisy_system (sde/mici_extensions.py:1679-1801; its
 * objective :1706-1737 is the comparator's target for a fixed sigma): one Adam iteration is these two calls.
 * chmc_adam_objective_device: objective and gradient at u_v_dev [B][U + V0 + T S V] (gradient into grad_dev) and, in one
 *   read-back, out3 [B][3] = objective, |u_v|^2, 1 if every gradient entry is finite (else 0): what the restart rules
 *   (:1745-1765) need of the chain.
 * chmc_adam_update_device: the Adam step (jax.example_libraries.optimizers.adam, :1740) in place on u_v_dev, m_dev, v_dev:
 *   moments of every chain (non-finite gradient entries count as 0), parameters of chain c moved by
 *   coef[c][1] * m / (sqrt(v * coef[c][0]) + eps), coef [B][2] on the host = {1 / (1 - b2^t), lr / (1 - b1^t) or 0}. */
int chmc_adam_objective_device(chmc_ctx* ctx, const void* u_v_dev, void* grad_dev, double* out3);
int chmc_adam_update_device(chmc_ctx* ctx, void* u_v_dev, void* m_dev, void* v_dev, const void* grad_dev,
                            const double* coef, double b1, double b2, double eps);
/* Keyed normal draws on the device: the start points and restart points of the same finder (sde/mici_extensions.py:1743-1765
 * draws them from one NumPy generator in the order the tries happen to start) as a function of (seed, stream, draw) alone.
 * Writes n_cols standard normals into each of the n_rows listed rows of a caller-owned [B][ld] fp64 buffer: row rows[r]
 * gets the Philox4x32-10 + Box-Muller stream of chmc_sample_momentum with counter (component pair, low word of draw[r],
 * stream[r], high word of draw[r]) and key `seed` -- i.e. the unprojected normals the momentum refresh draws for global
 * chain stream[r] at draw index draw[r].  rows, stream, draw [n_rows] are host arrays; rows in [0, B), none twice
 * (n_rows = 0 is allowed); columns n_cols .. ld - 1 and unlisted rows are not touched.  A value does not depend on the row
 * it lands in, on the other rows listed, on B or on the launch geometry.  The finder uses stream = chain_offset + chain and
 * draw = 2^63 | try: the high bit keeps its draws disjoint from the momentum refresh, whose draw index is the transition
 * number.  chmc_fill_normal is the host-pointer twin (dst [B][ld] on the host): the same kernel and a copy back, so a
 * draw has one set of bits per backend. */
int chmc_fill_normal_device(chmc_ctx* ctx, unsigned long long seed, int n_rows, const int* rows, const int* stream,
                            const unsigned long long* draw, int n_cols, void* dst_dev, long ld);
int chmc_fill_normal(chmc_ctx* ctx, unsigned long long seed, int n_rows, const int* rows, const int* stream,
                     const unsigned long long* draw, int n_cols, double* dst, long ld);
/* "Deal a try into a row" of the device-resident loop: for every listed row of u_v_dev, m_dev, v_dev, grad_dev
 * [B][U + V0 + T S V], u_v = the keyed normals of (seed, stream[r], draw[r]) as above (replacing rng.standard_normal of
 * :1743-1765 plus an upload), m = v = grad = 0, and the row's carried scan guess -- the work trajectory that the
 * time-parallel scan of chmc_adam_objective_device / chmc_neg_log_dens_and_grad[_device] (layouts with T S >= 1024) would
 * otherwise inherit from whatever was evaluated in that row before -- is reset to the cold guess (zeros) a new context
 * starts from.  Afterwards every evaluation of the try depends on the try's own (point, previous iterate) only: its bits
 * do not depend on the row, on the batch, or on the tries that used the row earlier. */
int chmc_adam_begin_tries_device(chmc_ctx* ctx, unsigned long long seed, int n_rows, const int* rows, const int* stream,
                                 const unsigned long long* draw, void* u_v_dev, void* m_dev, void* v_dev, void* grad_dev);
/* The device-resident loop of find_initial_state_by_gradient_descent (sde/mici_extensions.py:1550-1676), the generic finder:
 * any partition, noisy or noiseless observations, every model.  One Adam iteration is chmc_gd_objective_device +
 * chmc_adam_update_cols_device; a try that gets within coarse_tol calls chmc_gd_project_device.
 * chmc_gd_objective_device: init_objective (:1582-1618) and its gradient with respect to ALL of q at q_dev [B][Q], given
 *   x_obs_seq_init in xo_dev [B][T][X]:
 *     c[t] = x_S(z(u), v_subseq[t]; start x_init[t]) - xo[t],  x_init[0] = generate_x_0(z, v_0), x_init[t] = xo[t - 1] (a constant),
 *     objective = 1/2 mean(c^2) + 1/2 reg_coeff mean(q^2)      (means over the T X entries of c and the Q entries of q);
 *   the observation-noise part n and a variable-sigma u[Z] only receive the regulariser's reg_coeff q / Q.  Gradient into
 *   grad_dev [B][Q]; in one read-back out3 [B][3] = objective, max |c|, 1 if the objective and every gradient entry are
 *   finite (else 0).  The T intervals of a chain are independent scans: a work item per (chain, interval), the intervals'
 *   sums added in interval order (no atomics), so a row's results depend on the row's own (q, xo) only -- not on B, the row
 *   index or the other rows.  Works in a noiseless context (unlike chmc_adam_objective_device); does not touch the chain
 *   states.
 * chmc_adam_update_cols_device: chmc_adam_update_device (:1625, jax.example_libraries.optimizers.adam) on buffers of
 *   [B][n_cols] (this finder: n_cols = Q); same kernel, same coef [B][2].
 * chmc_gd_project_device: the projection of :1654-1669 for the chains with mask[c] != 0.  The chain's state becomes
 *   (pos = row c of q_dev, mom = 0, x_obs_seq = row c of xo_dev, partition 0) with the state caches evaluated, and that
 *   position is projected from that state (state_prev = state) with dt = 1 by the solver chmc_project runs (newton,
 *   tolerances and max_iters as there).  On convergence the projected point is written back into row c of q_dev and becomes
 *   the chain's state (caches re-evaluated); otherwise row c of q_dev is left alone (the chain's state stays the one
 *   projected from).  Chains with mask[c] == 0 keep their state and their row.  status [B]: chmc_project's codes (-1 for
 *   unmasked chains); iters, err [B] (0 for unmasked chains); any of the three may be NULL.  The context must hold a state
 *   in partition 0 in every row before the first call (chmc_set_state; a state at u = 0 is finite for every model). */
int chmc_gd_objective_device(chmc_ctx* ctx, const void* q_dev, const void* xo_dev, double reg_coeff, void* grad_dev,
                             double* out3);
int chmc_adam_update_cols_device(chmc_ctx* ctx, int n_cols, void* x_dev, void* m_dev, void* v_dev, const void* grad_dev,
                                 const double* coef, double b1, double b2, double eps);
int chmc_gd_project_device(chmc_ctx* ctx, const int* mask, void* q_dev, const void* xo_dev, int newton, double constraint_tol,
                           double position_tol, double divergence_tol, int max_iters, int* status, int* iters, double* err);

/* Projection solvers (newton != 0: newton_projection :1065-1135 with its host wrapper :1405-1476;
 * newton == 0: quasi_newton_projection :999-1063 / :1323-1402).  Projects the points q [B][Q] onto the manifold
 * along the rows of the constraint Jacobian at the CURRENT state (= `state_prev` of the reference).
 * Outputs: q_out [B][Q]; mu_out [B][Q] = mu/dt (mu/sin dt with Gaussian splitting); iters, norm_dq, err, status [B].
 * The state itself is not modified. */
int chmc_project(chmc_ctx* ctx, int newton, const double* q, const double* dt, double constraint_tol,
                 double position_tol, double divergence_tol, int max_iters, double* q_out, double* mu_out,
                 int* iters, double* norm_dq, double* err, int* status);

/* One ConstrainedLeapfrogIntegrator.step per chain (mici 0.1.10): A(dt/2) B(dt) A(dt/2); B = n_inner_step inner steps
 * of dt / n_inner_step (scripts/utils.py:131-136 --num-inner-h2-step), each with forward projection, momentum
 * projection at the new point, reverse projection and reversibility check; dh1_dpos is evaluated at the last new point
 * only.  dt [B] = state.dir * step_size; active [B] (NULL: all).  A chain whose step fails -- in whichever inner step --
 * keeps its state (Mici discards the partial step).  iters_fwd / iters_bwd are summed over the inner steps, rev_err is
 * that of the last inner step a chain ran.
 * The two half-kicks A(dt/2): p <- P(q)[p - dt/2 dh1_dpos(q)] use the projected kick direction P(q) dh1_dpos(q) that
 * the library keeps with every evaluated state: for a momentum already in the cotangent space (after
 * chmc_sample_momentum, chmc_project_onto_cotangent_space or a previous step) P(q)[p - h g] = p - h P(q) g, which
 * saves two of the three passes over the stored Jacobian rows; a momentum set through chmc_set_state /
 * chmc_set_momentum(_device), or carried across chmc_switch_partition, takes the full projection as in the reference. */
int chmc_leapfrog_step(chmc_ctx* ctx, const double* dt, const int* active, int n_inner_step, int newton,
                       double constraint_tol, double position_tol, double divergence_tol, int max_iters,
                       double reverse_check_tol, int* status, int* iters_fwd, int* iters_bwd, double* rev_err);

/* A whole integration trajectory per chain: up to n_steps[c] (n_steps == NULL: n_steps_all for every chain) consecutive
 * ConstrainedLeapfrogIntegrator.step calls of the chains with active[c] != 0, the loop a Mici integration transition
 * runs around integrator.step (mici.transitions: `for s in range(n_step): state = integrator.step(state)`, ended by
 * an IntegratorError; scripts/utils.py:284-301).  Semantics per chain = chmc_leapfrog_step applied repeatedly: a chain
 * whose step fails keeps the state its last successful step produced, reports that step's status and takes no further
 * steps.  Outputs [B]: n_done (successful steps), status (0: all steps done; 1 / 2 / 3: the failing step's code; -1:
 * inactive), iters_fwd / iters_bwd (Newton iterations summed over the chain's steps, the failing one included), rev_err
 * (reverse-check distance of the last step that reached the check).
 * Implemented as one batched chmc_leapfrog_step per step over the chains still running (tests/test_trajectories.py: bitwise
 * the host loop).  For layouts with one 16-row block per chain every retraction inside those steps already runs per chain,
 * in the chain's own workgroup, for as many Newton iterations as THAT chain needs (k_retract_chain; lax.while_loop
 * :1119-1131).  (Round 3's asynchronous per-chain-phase engine behind this entry point lost to the batched steps at every
 * BASELINE shape and was removed in round 4.) */
int chmc_leapfrog_steps(chmc_ctx* ctx, const double* dt, const int* active, const int* n_steps, int n_steps_all,
                        int n_inner_step, int newton, double constraint_tol, double position_tol, double divergence_tol,
                        int max_iters, double reverse_check_tol, int* n_done, int* status, int* iters_fwd, int* iters_bwd,
                        double* rev_err);

/* The single collective of a chain-sharded run: chains are independent, every rank (one process per
 * GPU) steps its own contiguous shard with no communication, and a sampling segment ends with ONE all-gather of the
 * traced per-chain samples over RCCL / xGMI.  (The reference runs its chains sequentially in one process,
 * scripts/utils.py:351-363; there is no reference collective to mirror.)
 *   chmc_comm_unique_id : rank 0 creates the 128-byte RCCL id and hands it to the other ranks by whatever means the
 *                         launcher has (file, MPI, torch.distributed.broadcast_object_list ...)
 *   chmc_comm_init      : every rank, same id; creates the context's communicator (collective call)
 *   chmc_gather_samples : local_dev [count] doubles of this rank -> gathered_dev [world][count] on EVERY rank, rank-major
 *                         (equal shards); both are device buffers of the caller; enqueued on the context's stream and
 *                         complete when the call returns
 *   chmc_comm_info      : world size and rank READ BACK from the communicator (ncclCommCount / ncclCommUserRank): what a
 *                         launcher prints to show that the ranks it started really joined one RCCL communicator
 *   chmc_comm_destroy   : releases the communicator (chmc_destroy does the same for a context that still owns one).
 * N > 1 ranks have been rehearsed with gloo on CPU only so far (tests/test_distributed_gloo.py); see INTEGRATION.md. */
int chmc_comm_unique_id(void* id128);
int chmc_comm_init(chmc_ctx* ctx, const void* id128, int rank, int world);
int chmc_gather_samples(chmc_ctx* ctx, const void* local_dev, long count, void* gathered_dev);
int chmc_comm_info(chmc_ctx* ctx, int* world, int* rank);
int chmc_comm_destroy(chmc_ctx* ctx);

/* evaluation counters since creation: {constr, jacob_constr_blocks, lu_jacob_product_blocks, chol_gram_blocks,
 * grad_log_det_sqrt_gram, leapfrog_step calls, newton rounds launched (a launch of the per-chain retraction kernel counts
 * as one), 0 (reserved)} (cf. _call_counts, :1451-1461).
 * Host-side counts: the call does not touch the device. */
int chmc_get_counters(const chmc_ctx* ctx, long long* out8);

/* diagnostics of the kernel paths taken since creation (tests assert with them that an optional kernel family ran):
 *   out80[0]       blocks the time-parallel forward scan handed to its sequential fallback
 *   out80[1 .. 63] histogram of sweeps to convergence of the time-parallel scan (1 + sweeps + 16 (guess kind - 1)), [15] parked
 *   out80[64]      launches of the fp64-MFMA Gram kernel (v_mfma_f64_16x16x4_f64; CHMC_GRAM_MFMA=1: 16-row blocks, and blocks
 *                  of at most 8 rows on the stored-rows family)
 *   out80[65]      launches of the vector-FMA Gram kernel over stored rows (16-row blocks)
 *   out80[66]      launches of the per-chain retraction kernel (k_retract_chain: one 16-row block per chain, SIR models only)
 *   out80[67]      launches of the per-chain trajectory kernel (k_traj_chain: whole leapfrog steps of such a chain)
 *   out80[68]      launches of k_newton_fsm_wave or of its form for two problems (blocks of at most 8 rows, at most 64 blocks per chain: block LU, Woodbury
 *                  solve and mu_F of a Newton round in one launch, a wavefront per chain)
 *   out80[69]      launches of KNewtonFactor for blocks of at most 8 rows (the unfused Newton round: more than 64 blocks per
 *                  chain, or the stored-rows families; the chain solve and mu_F follow as launches of their own)
 *   out80[70]      rounds of the lock-step Newton loops whose forward scan served two problems at once: the reverse
 *                  retraction of a trajectory's step and the forward retraction of its next step (one merged scan launch;
 *                  CHMC_PAIR_RETRACT=0 switches the pairing off)
 *   out80[71]      forward-scan launches of the lock-step Newton loops (a merged launch counts once)
 *   out80[72]      rounds those loops enqueued, counted per problem: with the hand-scheduled scan, [71] = [72] - [70]
 *   out80[73]      rounds among those of [70] whose passes behind the scan served both problems as well: interval sums,
 *                  combine, solve and J^T lambda update one launch each for the pair (compact rows in blocks of at most 8 row
 *                  slots, at most 64 blocks per chain; CHMC_PAIR_PASSES=0 keeps one launch per problem and pass)
 *   out80[74]      launches of the time-parallel path scan (k_path_par: chmc_generate_x_seq* / chmc_path_stats_update_device
 *                  on the current states with the compact rows allocated)
 *   out80[75]      launches of the sequential path scan (KPath: a caller's q, or CHMC_COMPACT_ROWS=0)
 *   out80[76]      launches of the predictive wave kernel (k_predict, k_predict_events: chmc_predict_device /
 *                  chmc_predict_events_device with the compact rows on), and of k_future_score (chmc_score_future_device under
 *                  CHMC_FUTURE_WAVE=1: the same recursion and geometry; no slot is free for a counter of its own)
 *   out80[77]      launches of the predictive functor form (KPredict<M, EVENTS>: CHMC_COMPACT_ROWS=0), and of
 *                  KFutureScore (chmc_score_future_device's default)
 *   out80[78]      launches of the path-events wave kernel (k_path_events: chmc_path_events_device, compact rows on)
 *   out80[79]      launches of the path-events functor form (KPathEvents: CHMC_COMPACT_ROWS=0)
 * Synchronises the context's stream. */
int chmc_get_diagnostics(chmc_ctx* ctx, long long* out80);

/* ---- measurement: HIP events recorded on the library's own stream around every kernel launch ------------- */
/* kernel classes: 0 other, 1 newton_blk (constr + Jacobian + Gram/LU of a Newton iteration), 2 state_blk
 * (Jacobian store + Gram + Cholesky), 3 grad_log_det_blk, 4 update (J^T lambda column pass), 5 solve_chain,
 * 6 jacob_vec (J w), 7 constr (forward scan only), 8 element-wise, 9 sym_blk */
#define CHMC_NUM_KERNEL_CLASSES 10
int chmc_profile_enable(int on);  /* 0 stop, 1 all classes, else bit mask (1 << class); resets the accumulators */
int chmc_profile_stride(int every); /* time every `every`-th launch of a profiled class only (default 1); an event pair costs ~30 us of stream bubbles */
int chmc_profile_get(double* ms, long long* launches);  /* [CHMC_NUM_KERNEL_CLASSES] each; synchronises */

#ifdef __cplusplus
}
#endif
#endif
