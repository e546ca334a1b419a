// The moment arithmetic of the chain statistics, one copy for kernels_chainstats.hip (moments of the samples y) and
// kernels_rbstats.hip (moments of the conditional means m): the balanced tree over the lane slots of a row, the
// two-pass moments of a chunk of up to 64 chains, the parking of chunk results and the Chan/Golub/LeVeque merge.  The order of
// every sum is stated in kernels_chainstats.hip; it is a function of the number of chains alone.
#ifndef PMG_CHAIN_MOMENTS_HPP
#define PMG_CHAIN_MOMENTS_HPP
#include <hip/hip_runtime.h>

namespace pmg_moments {

// balanced tree over the LPR lanes of a row, neighbours first; every lane ends with the same bits
template <int LPR>
__device__ __forceinline__ double row_tree(double v)
{
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// (Nb, mb, Mb) merged into (N, m, M)
__device__ __forceinline__ void merge(double N, double &m, double &M, double Nb, double mb, double Mb)
{
  const double d = mb - m, Np = N + Nb;
  m = m + (d * Nb) / Np;
  M = M + (Mb + (((d * d) * N) * Nb) / Np);
}

// mean and sum of squared deviations over the cnt chains of one chunk: v is this lane's value (+0.0 in a slot without a chain,
// live = false there); second pass over the registers, not a sum of squares.  Every lane of the wavefront must call it.
template <int LPR>
__device__ __forceinline__ void chunk_moments(double v, bool live, double cnt, double &cm, double &cM2)
{
  cm             = row_tree<LPR>(v) / cnt;
  const double d = live ? v - cm : 0.0;
  cM2            = row_tree<LPR>(d * d);
}

// The step's batch (bm, bM2) after chunk k of a row whose chains are walked in chunks of 64 by one wavefront (lpr = 64): chunk
// 0 is the batch, chunk k > 0 is merged into what p[0..1] (LDS, this row's slot) holds of the `seen` chains before it; all but
// the last chunk are parked there by lane 0.
__device__ __forceinline__ void chunk_batch(double *p, int k, bool last, int lane, double seen, double cnt, double cm, double cM2, double &bm, double &bM2)
{
  bm = cm, bM2 = cM2;
  if (k > 0) {
    bm = p[0], bM2 = p[1];
    merge(seen, bm, bM2, cnt, cm, cM2);
  }
  if (!last && lane == 0) p[0] = bm, p[1] = bM2;
}

} // namespace pmg_moments
#endif
