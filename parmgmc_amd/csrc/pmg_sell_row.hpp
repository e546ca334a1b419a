// The row sum of the sliced-ELL sweeps (kernels_csr.hip, kernels_blockgibbs.hip): one lane, one row, entries column-major with
// lane stride 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Off-diagonal part of one row: sum -= a_j y[c_j] in storage order.  The entries are fetched in batches of SELL_BATCH:
// all value / column loads of a batch are issued together, then all gathers y[c_j], and only then the dependent
// subtractions run.  A plain `for j` loop compiles to load c -> wait -> load y[c] -> wait per entry, i.e. 2 w serial
// memory latencies per row -- a 63 000-row colour of the refined L-shape mesh took 7 us, all of it latency.
// The slice width w is wave-uniform, so the guards are scalar branches; a batch reads the slice's last column again
// instead of running past it (a valid address whose value is not used).  Same terms, same order: same bits.
constexpr int SELL_BATCH = 8;
__device__ __forceinline__ double sell_row_sum(double sum, int w, const double *__restrict__ v, const int32_t *__restrict__ c, const double *y)
{
  for (int j0 = 0; j0 < w; j0 += SELL_BATCH) {
    double  a[SELL_BATCH], yv[SELL_BATCH];
    int32_t cj[SELL_BATCH];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) {
      const int64_t jj = (int64_t)min(j0 + q, w - 1) * 64;
      a[q]             = v[jj];
      cj[q]            = c[jj];
    }
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) yv[q] = y[cj[q]];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q)
      if (j0 + q < w) sum = sum - a[q] * yv[q];
  }
  return sum;
}
