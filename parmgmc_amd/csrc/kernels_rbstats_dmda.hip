// Rao-Blackwellised running statistics of the chains on a DMDA grid, matrix-free (gfx950): kernels_rbstats.hip on the operator
// of pmg_grid_create / pmg_mat_create_dmda (MatAssembleShiftedLaplaceFD, src/problems.c:14-75, and its 3-D analogue) without a
// matrix.  Rows in DMDA natural order, row = i + nx * (j + ny * k); Y[row * C + c], chain fastest.  No index or value array is
// read: the coefficients of a row follow from (i, j, k) in registers.
//
// ARITHMETIC: the bits of kernels_rbstats.hip on the assembled operator.  Per row and chain, every product, sum and quotient
// rounded on its own (-ffp-contract=off), hinv2 = 1.0 / ((nx - 1) * (nx - 1)) and kappa * kappa formed on the host:
//     s = 0.0;  s = s + (-hinv2) * y_j       over the in-domain neighbours in stored order (k-1) (j-1) (i-1) (i+1) (j+1) (k+1)
//     r = b_i - s                            (b_i = 0.0 without a right-hand side)
//     w = 0.0;  w = w + (B_ik * S_k) * (t_kc - B_ik * y_ic),  k ascending;   r = r - w        (only with Q = A + B S B^T)
//     m = r / q_i                            (one division)
// Without a low-rank term q_i = kappa * kappa, then + hinv2 once per in-domain neighbour by repeated addition, formed in
// registers (the addends are equal, so only their number matters); with one, q_i is read from the array the host formed.
// The moments of m are merged by pmg_chain_moments.hpp with the lane mapping kernels_rbstats.hip uses for the same C.  No
// floating-point atomics; the order of every sum is fixed by (nx, ny, nz, C) alone.
//
// C = 1 (march_kernel): one lane per point of an x-y plane, 256 consecutive points of the plane per block (lines are walked
// along x, a wavefront may span the end of one line and the start of the next), marching through `zsteps` planes.  The lane
// carries its own values of planes k-1 and k in registers and loads plane k+1 once: the z neighbours are never fetched a
// second time, whatever the caches hold (DESIGN 4b's finding for 513^3).  The x and y neighbours are plain 8-byte loads of
// plane k at p -+ 1 and p -+ nx: other lanes of the same or a neighbouring wavefront load the same lines as their own values
// in the same plane step, so they hit.  Every access is one double wide: lines of 2^k + 1 grids start 8-byte aligned only.
//
// C > 1 (chains_kernel): the lane mapping of kernels_rbstats.hip -- lpr = C rounded up to a power of two (at most 64) lanes
// share a row, G = 64 / lpr rows per wavefront at a time, chains beyond 64 in chunks of 64 by the same wavefront with the
// moments of the chunks read so far parked in LDS; neighbour segments are Y[j * C + c].  Untuned.
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"
#include "pmg_chain_moments.hpp"

namespace {

constexpr int MAXRPW = 256;  // as kernels_rbstats.hip: rows per wavefront when the chains are chunked
constexpr int MAXBLK = 2048; // blocks of one march before a wavefront takes a second plane
constexpr int ZMIN   = 8;    // planes a wavefront marches at least (where the grid has them): 2 of ZMIN + 2 plane loads are re-reads

using pmg_moments::chunk_batch;
using pmg_moments::chunk_moments;
using pmg_moments::merge;

inline int lpr_log2_of(int32_t C) // as kernels_chainstats.hip
{
  int l = 0;
  while (l < 6 && (1 << l) < C) ++l;
  return l;
}

// r - w of the file header for row `row` and chain c; yi = Y[row * C + c]
__device__ __forceinline__ double lowrank_term(const pmgk_rbstats_dmda_op &A, int64_t n, int64_t row, int64_t C, int c, double yi, double r)
{
  double w = 0.0;
  for (int j = 0; j < A.k; ++j) {
    const double bij = A.B[row + n * j];
    w                = w + (bij * A.S[j]) * (A.T[(int64_t)j * C + c] - bij * yi);
  }
  return r - w;
}

// C = 1.  STORE: Mout = m, nothing recorded.  Otherwise m is merged into (mean, M2), which hold N samples per row.
template <bool STORE>
__global__ __launch_bounds__(256) void march_kernel(pmgk_rbstats_dmda_op A, int zsteps, int nbp, double N, const double *__restrict__ Y, double *__restrict__ mean, double *__restrict__ M2, double *__restrict__ Mout)
{
  const int64_t P  = (int64_t)A.nx * A.ny, n = P * A.nz;
  const int     kc = (int)(blockIdx.x / (unsigned)nbp), pb = (int)(blockIdx.x % (unsigned)nbp);
  const int64_t p  = (int64_t)pb * 256 + threadIdx.x;
  if (p >= P) return; // no barrier and no cross-lane exchange below
  const int    j = (int)((uint32_t)p / (uint32_t)A.nx), i = (int)p - j * A.nx;
  const int    k0 = kc * zsteps, k1 = min(A.nz, k0 + zsteps);
  const bool   hw = i > 0, he = i < A.nx - 1, hs = j > 0, hn = j < A.ny - 1;
  const double nh = -A.hinv2;
  const bool   first = N == 0.0;
  double       qxy   = A.kk; // the in-plane part of q: the additions of equal addends commute
  if (hs) qxy = qxy + A.hinv2;
  if (hw) qxy = qxy + A.hinv2;
  if (hn) qxy = qxy + A.hinv2;
  if (he) qxy = qxy + A.hinv2;
  int64_t row = p + P * k0;
  double  ym = k0 > 0 ? Y[row - P] : 0.0, yc = Y[row];
  for (int k = k0; k < k1; ++k, row += P) {
    const bool   hd = k > 0, hu = k < A.nz - 1;
    const double yu = hu ? Y[row + P] : 0.0;
    const double ys = hs ? Y[row - A.nx] : 0.0, yw = hw ? Y[row - 1] : 0.0;
    const double ye = he ? Y[row + 1] : 0.0, yn = hn ? Y[row + A.nx] : 0.0;
    double       s  = 0.0;
    if (hd) s = s + nh * ym;
    if (hs) s = s + nh * ys;
    if (hw) s = s + nh * yw;
    if (he) s = s + nh * ye;
    if (hn) s = s + nh * yn;
    if (hu) s = s + nh * yu;
    double r = (A.b ? A.b[row] : 0.0) - s;
    double q;
    if (A.k > 0) {
      r = lowrank_term(A, n, row, 1, 0, yc, r);
      q = A.q[row];
    } else {
      q = qxy;
      if (hd) q = q + A.hinv2;
      if (hu) q = q + A.hinv2;
    }
    const double m = r / q;
    if (STORE) {
      Mout[row] = m;
    } else {
      double cm, cM2;
      chunk_moments<1>(m, true, 1.0, cm, cM2); // what kernels_rbstats.hip does at lpr = 1
      double mo = first ? 0.0 : mean[row], vo = first ? 0.0 : M2[row];
      merge(N, mo, vo, 1.0, cm, cM2);
      mean[row] = mo;
      M2[row]   = vo;
    }
    ym = yc, yc = yu;
  }
}

// the conditional mean of row `row` for chain c, C > 1
__device__ __forceinline__ double cond_mean(const pmgk_rbstats_dmda_op &A, int64_t n, int64_t row, int64_t C, int c, const double *__restrict__ Y)
{
  const uint32_t P = (uint32_t)A.nx * (uint32_t)A.ny;
  const int      k = (int)((uint32_t)row / P);
  const uint32_t p = (uint32_t)row - (uint32_t)k * P;
  const int      j = (int)(p / (uint32_t)A.nx), i = (int)p - j * A.nx;
  const bool     hd = k > 0, hs = j > 0, hw = i > 0, he = i < A.nx - 1, hn = j < A.ny - 1, hu = k < A.nz - 1;
  const double   nh = -A.hinv2;
  const double   yd = hd ? Y[(row - P) * C + c] : 0.0, ys = hs ? Y[(row - A.nx) * C + c] : 0.0, yw = hw ? Y[(row - 1) * C + c] : 0.0;
  const double   ye = he ? Y[(row + 1) * C + c] : 0.0, yn = hn ? Y[(row + A.nx) * C + c] : 0.0, yu = hu ? Y[(row + P) * C + c] : 0.0;
  double         s  = 0.0;
  if (hd) s = s + nh * yd;
  if (hs) s = s + nh * ys;
  if (hw) s = s + nh * yw;
  if (he) s = s + nh * ye;
  if (hn) s = s + nh * yn;
  if (hu) s = s + nh * yu;
  double r = (A.b ? A.b[row] : 0.0) - s;
  if (A.k > 0) return lowrank_term(A, n, row, C, c, Y[row * C + c], r) / A.q[row];
  double q = A.kk;
  if (hd) q = q + A.hinv2;
  if (hs) q = q + A.hinv2;
  if (hw) q = q + A.hinv2;
  if (he) q = q + A.hinv2;
  if (hn) q = q + A.hinv2;
  if (hu) q = q + A.hinv2;
  return r / q;
}

// C > 1: the row loop of kernels_rbstats.hip's rbstats_kernel on the stencil
template <int LPRL, bool STORE>
__global__ __launch_bounds__(256) void chains_kernel(pmgk_rbstats_dmda_op A, int32_t C, int iters, double N, const double *__restrict__ Y, double *__restrict__ mean, double *__restrict__ M2, double *__restrict__ Mout)
{
  constexpr int     LPR = 1 << LPRL, G = 64 / LPR;
  __shared__ double parked[LPRL == 6 && !STORE ? 4 * MAXRPW * 2 : 2]; // (mean, M2) of the chunks read so far, per row of a wavefront
  const int     lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> LPRL, cl = lane & (LPR - 1);
  const int64_t n      = (int64_t)A.nx * A.ny * A.nz;
  const int64_t row0   = ((int64_t)blockIdx.x * 4 + wv) * ((int64_t)iters * G);
  const int     chunks = LPRL == 6 ? (C + 63) / 64 : 1;
  const bool    first  = N == 0.0;
  for (int k = 0; k < chunks; ++k) {
    const int    c    = k * 64 + cl;
    const bool   live = c < C, last = k == chunks - 1;
    const double cnt  = (double)min(64, C - k * 64), seen = 64.0 * k; // chains of this chunk, of the chunks before it
    for (int it = 0; it < iters; ++it) {
      const int64_t row = row0 + (int64_t)it * G + g;
      double        m   = 0.0; // a slot without a chain or a row enters the tree as +0.0
      if (live && row < n) m = cond_mean(A, n, row, C, c, Y);
      if (STORE) {
        if (live && row < n) Mout[row * C + c] = m;
      } else {
        double cm, cM2;
        chunk_moments<LPR>(m, live, cnt, cm, cM2); // all 64 lanes
        double bm = cm, bM2 = cM2;
        if (LPRL == 6 && chunks > 1) // G = 1: the wavefront's rows are `it`
          chunk_batch(parked + (wv * MAXRPW + it) * 2, k, last, lane, seen, cnt, cm, cM2, bm, bM2);
        if (last && cl == 0 && row < n) {
          double mo = first ? 0.0 : mean[row], vo = first ? 0.0 : M2[row];
          merge(N, mo, vo, (double)C, bm, bM2);
          mean[row] = mo;
          M2[row]   = vo;
        }
      }
    }
    if (!STORE && chunks > 1) __syncthreads(); // parked is reused by the next chunk; uniform over the block
  }
}

template <int LPRL>
void launch(bool store, unsigned nb, hipStream_t st, const pmgk_rbstats_dmda_op &A, int32_t C, int iters, double N, const double *Y, double *mean, double *M2, double *Mout)
{
  if (store) hipLaunchKernelGGL((chains_kernel<LPRL, true>), dim3(nb), dim3(256), 0, st, A, C, iters, N, Y, mean, M2, Mout);
  else hipLaunchKernelGGL((chains_kernel<LPRL, false>), dim3(nb), dim3(256), 0, st, A, C, iters, N, Y, mean, M2, Mout);
}

int run(bool store, const pmgk_rbstats_dmda_op *A, int32_t C, double N, const double *Y, double *mean, double *M2, double *Mout, void *stream)
{
  if (A->nx <= 0 || A->ny <= 0 || A->nz <= 0 || C <= 0) return 0;
  if (A->k < 0 || A->k > 64 || (int64_t)A->nx * A->ny * A->nz > INT32_MAX) return 1;
  const hipStream_t st = (hipStream_t)stream;
  int32_t           iters, nb;
  pmgk_rbstats_dmda_geometry(A->nx, A->ny, A->nz, C, &iters, &nb);
  if (C == 1) {
    const int nbp = (int)(((int64_t)A->nx * A->ny + 255) / 256);
    if (store) hipLaunchKernelGGL((march_kernel<true>), dim3((unsigned)nb), dim3(256), 0, st, *A, iters, nbp, N, Y, mean, M2, Mout);
    else hipLaunchKernelGGL((march_kernel<false>), dim3((unsigned)nb), dim3(256), 0, st, *A, iters, nbp, N, Y, mean, M2, Mout);
    return hipGetLastError() == hipSuccess ? 0 : 1;
  }
  switch (lpr_log2_of(C)) {
  case 1: launch<1>(store, (unsigned)nb, st, *A, C, iters, N, Y, mean, M2, Mout); break;
  case 2: launch<2>(store, (unsigned)nb, st, *A, C, iters, N, Y, mean, M2, Mout); break;
  case 3: launch<3>(store, (unsigned)nb, st, *A, C, iters, N, Y, mean, M2, Mout); break;
  case 4: launch<4>(store, (unsigned)nb, st, *A, C, iters, N, Y, mean, M2, Mout); break;
  case 5: launch<5>(store, (unsigned)nb, st, *A, C, iters, N, Y, mean, M2, Mout); break;
  default: launch<6>(store, (unsigned)nb, st, *A, C, iters, N, Y, mean, M2, Mout); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace

/* The launch geometry of one update or cond_mean, from (nx, ny, nz, C) only.  C = 1: *iters = the planes a wavefront marches
   through, *nblocks = ceil(nx ny / 256) blocks per plane x ceil(nz / *iters) plane ranges.  C > 1: pmgk_rbstats_geometry's
   rows per wavefront = *iters * (64 / lpr) and blocks, on n = nx ny nz. */
extern "C" void pmgk_rbstats_dmda_geometry(int32_t nx, int32_t ny, int32_t nz, int32_t nchains, int32_t *iters, int32_t *nblocks)
{
  const int64_t P = (int64_t)nx * ny;
  if (nchains > 1) {
    pmgk_rbstats_geometry(P * nz, nchains, iters, nblocks);
    return;
  }
  const int64_t nbp = (P + 255) / 256;
  int64_t       ranges = (MAXBLK + nbp - 1) / nbp; /* plane ranges that fill MAXBLK blocks */
  if (ranges > nz) ranges = nz;
  int64_t zs = (nz + ranges - 1) / ranges;
  if (zs < ZMIN) zs = ZMIN;
  if (zs > nz) zs = nz;
  *iters   = (int32_t)zs;
  *nblocks = (int32_t)(nbp * ((nz + zs - 1) / zs));
}

/* one step: as pmgk_rbstats_update; with A->k > 0, A->q must hold the conditional precisions and A->T = B^T Y (k x C) */
extern "C" int pmgk_rbstats_dmda_update(const pmgk_rbstats_dmda_op *A, int32_t nchains, double count, const double *Y, double *mean, double *M2, void *stream)
{
  return run(false, A, nchains, count, Y, mean, M2, NULL, stream);
}

/* M (n x C, the layout of Y) = the conditional means of Y */
extern "C" int pmgk_rbstats_dmda_cond_mean(const pmgk_rbstats_dmda_op *A, int32_t nchains, const double *Y, double *M, void *stream)
{
  return run(true, A, nchains, 0.0, Y, NULL, NULL, M, stream);
}
