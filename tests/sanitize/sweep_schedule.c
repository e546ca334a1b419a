/* Prints what the sweep schedule helpers of the host layer (csrc/pmg_internal.h, csrc/pmg_mgmc_internal.h) give, for
   tests/test_sweep_schedule.py to compare with the Python statement of the same contract.  Host only: no device call. */
#include "../../parmgmc_amd/csrc/pmg_mgmc_internal.h"

int main(void)
{
  const int      types[3] = {PMG_SOR_FORWARD_SWEEP, PMG_SOR_BACKWARD_SWEEP, PMG_SOR_SYMMETRIC_SWEEP};
  const int32_t  itss[3]  = {0, 1, 3};
  const uint64_t c0s[4]   = {0u, 5u, 0xffffffffull, 0xfffffffffffffffeull};
  for (int t = 0; t < 3; ++t)
    for (int i = 0; i < 3; ++i)
      for (int noisy = 0; noisy < 2; ++noisy)
        for (int c = 0; c < 4; ++c) {
          pmg_sweep_iter it = pmg_sweep_begin(types[t], itss[i], noisy, c0s[c]);
          printf("S %d %d %d %llu :", types[t], (int)itss[i], noisy, (unsigned long long)c0s[c]);
          int64_t n = 0;
          while (pmg_sweep_next(&it)) {
            if (it.index != n++) return 2;
            printf(" %d:%llu", it.dir, (unsigned long long)it.sweep);
          }
          if (pmg_sweep_next(&it)) return 3; /* stays at the end */
          printf(" ; %llu\n", (unsigned long long)it.ctr);
        }
  for (int t = 0; t < 3; ++t) printf("N %d : %d\n", types[t], pmg_sweep_ndir(types[t]));
  const int32_t ncs[3] = {1, 2, 5};
  for (int dir = PMG_SOR_FORWARD_SWEEP; dir <= PMG_SOR_BACKWARD_SWEEP; ++dir)
    for (int k = 0; k < 3; ++k) {
      printf("C %d %d :", dir, (int)ncs[k]);
      for (int32_t cc = 0; cc < ncs[k]; ++cc) printf(" %d", (int)pmg_sweep_color(dir, ncs[k], cc));
      printf("\n");
    }
  struct pmg_mgmc_s h;
  memset(&h, 0, sizeof h);
  for (int t = 0; t < 3; ++t)
    for (h.nu = 1; h.nu <= 2; ++h.nu)
      for (h.coarse_type = 0; h.coarse_type <= 1; ++h.coarse_type)
        for (h.coarse_its = 1; h.coarse_its <= 3; h.coarse_its += 2)
          for (int l = 0; l < 3; ++l) {
            h.sweep_type = types[t];
            printf("L %d %d %d %d %d : %d %d\n", types[t], h.nu, h.coarse_type, h.coarse_its, l, pmg_mgmc_i_leg_sweeps(&h, l), pmg_mgmc_i_level_sweeps(&h, l));
          }
  printf("sweep_schedule ok\n");
  return 0;
}
