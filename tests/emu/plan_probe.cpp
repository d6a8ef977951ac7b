// TEST-ONLY: the kernel plan (csrc/chmc_plan.h) of a layout as integers, for tests/test_kernel_plan.py.  The wave kernels
// are assumed compiled in (the plan of the shipped library); the switches come from the environment, as in the library.
#include "../../manifold_mcmc_for_diffusions_amd/csrc/chmc_plan.h"

// in:  rmt, num_partition, K[0], K[1], longest, chain_steps, S % 8 == 0, V, even dims, gaussian, chains, compute units
// out: rows, pb_allocated, par_scan, fwd, fwd_cold, fwd_waves, nld, nld_waves, mom_fix_in_jp, rev_flow_in_update,
//      per partition (7 each): state, newton, gld, jp, rebuild_rows, wavefronts per chain of k_retract_chain / k_traj_chain
//      for a Newton retraction of the whole batch (0: batched launches)
extern "C" int chmc_plan_probe(const int* in, int* out) {
  using namespace chmc;
  PlanInput pi{};
  pi.rmt = in[0], pi.num_partition = in[1], pi.K[0] = in[2], pi.K[1] = in[3], pi.longest = in[4], pi.chain_steps = in[5];
  pi.s_tiles8 = in[6] != 0, pi.V = in[7], pi.even_dims = in[8] != 0, pi.gaussian = in[9] != 0, pi.wave_kernels = true;
  pi.sw = pi.call = read_switches();
  const KernelPlan pl = make_plan(pi);
  int n = 0;
  out[n++] = pl.rows, out[n++] = pl.pb_allocated, out[n++] = pl.par_scan, out[n++] = pl.fwd, out[n++] = pl.fwd_cold;
  out[n++] = pl.fwd_waves, out[n++] = pl.nld, out[n++] = pl.nld_waves, out[n++] = pl.mom_fix_in_jp;
  out[n++] = pl.rev_flow_in_update;
  for (int p = 0; p < pi.num_partition; ++p) {
    const PartitionPlan& pp = pl.part[p];
    out[n++] = pp.state, out[n++] = pp.newton, out[n++] = pp.gld, out[n++] = pp.jp, out[n++] = pp.rebuild_rows;
    out[n++] = chain_kernel_waves(pl, pp.retract_chain, in[10], in[11], true, false);
    out[n++] = chain_kernel_waves(pl, pp.traj_chain, in[10], in[11], true, false);
  }
  return n;
}
