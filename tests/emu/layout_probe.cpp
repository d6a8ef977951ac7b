// TEST-ONLY: the list of per-chain device arrays (csrc/chmc_layout.h) of a layout as integers, for
// tests/test_device_layout.py.  The switches come from the environment, as in the library.
#define CHMC_HD
#include "../../manifold_mcmc_for_diffusions_amd/csrc/chmc_core.h"
#include "../../manifold_mcmc_for_diffusions_amd/csrc/chmc_layout.h"

// in:  T, S, noisy, U, X, V, Z, V0, Kmax, RM, NOBS, groups of the row sums (work.part), wave kernels compiled in
// out: [0 .. 4] elements per chain of Slots::PB[0], Slots::LF[0], work.gcq, work.gbw, work.JvW (0: the context has none);
//      then per array of the list: elements per chain, slack, bytes per element, kind (ChainArrayKind)
// returns the number of arrays
extern "C" int chmc_layout_probe(const int* in, long long* out) {
  using namespace chmc;
  ChainView v{};
  Sys& sy = v.sy;
  sy.T = in[0], sy.S = in[1], sy.noisy = in[2], sy.U = in[3], sy.X = in[4], sy.V = in[5], sy.Z = in[6], sy.V0 = in[7];
  sy.Kmax = in[8], sy.RM = in[9], sy.NOBS = in[10];
  sy.NV = sy.V0 + sy.T * sy.S * sy.V, sy.NCOL = sy.NV + (sy.noisy ? sy.T : 0), sy.Q = sy.U + sy.NCOL;
  sy.TRJ = (sy.T * sy.S + CHMC_TPAD * sy.Kmax) * sy.X;
  PlanInput pi{};  // (the list depends on KernelPlan::pb_allocated and ::rows only: row slots, switches, wave kernels)
  pi.rmt = sy.RM, pi.num_partition = 1, pi.K[0] = pi.K[1] = sy.Kmax, pi.wave_kernels = in[12] != 0;
  pi.sw = pi.call = read_switches();
  const KernelPlan pl = make_plan(pi);
  for (int i = 0; i < 5; ++i) out[i] = 0;
  int n = 0;
  for_each_chain_array(v, pl, (size_t)in[11], [&](auto*& p, size_t per_chain, int kind, size_t slack) {
    const void* const five[5] = {&v.sl.PB[0], &v.sl.LF[0], &v.w.gcq, &v.w.gbw, &v.w.JvW};
    for (int i = 0; i < 5; ++i)
      if ((const void*)&p == five[i] && !(kind & kAbsent)) out[i] = (long long)per_chain;
    long long* o = out + 5 + 4 * n++;
    o[0] = (long long)per_chain, o[1] = (long long)slack, o[2] = (long long)sizeof(*p), o[3] = kind;
  });
  return n;
}
