// Rao-Blackwellised running statistics of the chains on the device (gfx950).  For x ~ N(Q^-1 b, Q^-1) every sample y gives the
// conditional mean of each unknown given all the others in closed form,
//     m_i = E[x_i | x_-i] = (b_i - sum_{j != i} Q_ij y_j) / Q_ii,      E[x_i] = E[m_i],      Var[x_i] = 1 / Q_ii + Var[m_i],
// and the moments of m estimate the marginal mean and variance with less Monte Carlo error than the moments of y (the simple
// Rao-Blackwellised estimator of Siden et al. 2018).  ONE launch per step reads the matrix and the step's n x C sample array Y,
// forms m in registers and merges its moments into the running (mean, M2) of every row: m is never written to memory.
//
// Layout and lane mapping: kernels_chains.hip's.  Y[row * C + c], chain fastest; lpr = C rounded up to a power of two (at most
// 64) lanes share a row and a wavefront serves G = 64 / lpr rows at a time.  The lanes of a row walk the row's stored
// off-diagonal entries together: colidx and vals are one address for the lpr lanes (a broadcast), the gathers Y[col * C + c]
// one contiguous segment of 8 * min(C, 64) bytes.  The loads of a batch of 8 entries are issued before its gathers and those
// before the dependent sums.  Rows of different length in one wavefront (lpr < 64) wait for the longest.  Chains beyond 64 are
// taken in chunks of 64 by the SAME wavefront, chunk loop outermost, the moments of the chunks read so far parked in LDS.
//
// ARITHMETIC per row i and chain c, every product, sum and quotient rounded on its own (-ffp-contract=off):
//     s = 0.0;  s = s + a_ij * y_jc          over the stored off-diagonal entries of row i in stored order
//     r = b_i - s                            (b_i = 0.0 without a right-hand side)
//     w = 0.0;  w = w + (B_ik * S_k) * (t_kc - B_ik * y_ic),  k ascending;   r = r - w        (only with Q = A + B S B^T)
//     m = r / q_i                            (one division; q_i = a_ii, or a_ii + sum_k S_k * (B_ik * B_ik) formed on the host)
// t = B^T y per chain comes from pmgk_lrc_btx_chains (kernels_lrc_chains.hip states its order of summation).
// The moments of m_0 .. m_{C-1} are merged exactly as kernels_chainstats.hip merges those of y_0 .. y_{C-1}: the same balanced
// tree over the lane slots, second pass over (m_c - bm)^2, chunks of 64 chains, Chan/Golub/LeVeque merge -- one copy of that
// code, pmg_chain_moments.hpp.  No floating-point atomics; the order of every sum is fixed by (matrix, C) alone.
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"
#include "pmg_chain_moments.hpp"

namespace {

constexpr int BATCH  = 8;    // entries of a row whose loads are in flight together (as sell_row_sum_chains)
constexpr int MAXRPW = 256;  // rows per wavefront when the chains are chunked (their moments wait in LDS)
constexpr int MAXBLK = 2048; // blocks of one update before a wavefront takes a second row group (8192 wavefronts: 8 per SIMD of 256 compute units)

using pmg_moments::chunk_batch;
using pmg_moments::chunk_moments;
using pmg_moments::merge;

inline int lpr_log2_of(int32_t C) // as kernels_chainstats.hip
{
  int l = 0;
  while (l < 6 && (1 << l) < C) ++l;
  return l;
}

// the conditional mean of row `row` for chain c (the file header states every rounding)
__device__ __forceinline__ double cond_mean(const pmgk_rbstats_op &A, int64_t row, int64_t C, int c, const double *__restrict__ Y)
{
  const int32_t beg = A.rowptr[row], end = A.rowptr[row + 1];
  double        s   = 0.0;
  for (int32_t j0 = beg; j0 < end; j0 += BATCH) {
    double  a[BATCH], yv[BATCH];
    int32_t cj[BATCH];
#pragma unroll
    for (int q = 0; q < BATCH; ++q) {
      const int32_t jj = min(j0 + q, end - 1); // in [beg, end): the loop runs only for beg < end
      a[q]             = A.vals[jj];
      cj[q]            = A.cols[jj];
    }
#pragma unroll
    for (int q = 0; q < BATCH; ++q) yv[q] = Y[(int64_t)cj[q] * C + c];
#pragma unroll
    for (int q = 0; q < BATCH; ++q)
      if (j0 + q < end) s = s + a[q] * yv[q];
  }
  double r = (A.b ? A.b[row] : 0.0) - s;
  if (A.k > 0) {
    const double yi = Y[row * C + c];
    double       w  = 0.0;
    for (int j = 0; j < A.k; ++j) {
      const double bij = A.B[row + A.n * j];
      w                = w + (bij * A.S[j]) * (A.T[(int64_t)j * C + c] - bij * yi);
    }
    r = r - w;
  }
  return r / A.q[row];
}

// STORE: Mout = m, nothing recorded.  Otherwise the moments of m are merged into (mean, M2), which hold N samples per row.
template <int LPRL, bool STORE>
__global__ __launch_bounds__(256) void rbstats_kernel(pmgk_rbstats_op A, int32_t C, int iters, double N, const double *__restrict__ Y, double *__restrict__ mean, double *__restrict__ M2, double *__restrict__ Mout)
{
  constexpr int     LPR = 1 << LPRL, G = 64 / LPR;
  __shared__ double parked[LPRL == 6 && !STORE ? 4 * MAXRPW * 2 : 2]; // (mean, M2) of the chunks read so far, per row of a wavefront
  const int     lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> LPRL, cl = lane & (LPR - 1);
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
      if (live && row < A.n) m = cond_mean(A, row, C, c, Y);
      if (STORE) {
        if (live && row < A.n) Mout[row * C + c] = m;
      } else {
        double cm, cM2;
        chunk_moments<LPR>(m, live, cnt, cm, cM2); // all 64 lanes: the row loop above has ended for every lane
        double bm = cm, bM2 = cM2;
        if (LPRL == 6 && chunks > 1) // G = 1: the wavefront's rows are `it`
          chunk_batch(parked + (wv * MAXRPW + it) * 2, k, last, lane, seen, cnt, cm, cM2, bm, bM2);
        if (last && cl == 0 && row < A.n) {
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

__global__ __launch_bounds__(256) void rbstats_fields_kernel(int64_t n, double Nm1, const double *__restrict__ q, const double *__restrict__ mean, const double *__restrict__ M2, double *__restrict__ mean_out, double *__restrict__ var_out)
{
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  if (mean_out) mean_out[r] = mean[r];
  if (var_out) var_out[r] = 1.0 / q[r] + M2[r] / Nm1;
}

template <int LPRL>
void launch(bool store, unsigned nb, hipStream_t st, const pmgk_rbstats_op &A, int32_t C, int iters, double N, const double *Y, double *mean, double *M2, double *Mout)
{
  if (store) hipLaunchKernelGGL((rbstats_kernel<LPRL, true>), dim3(nb), dim3(256), 0, st, A, C, iters, N, Y, mean, M2, Mout);
  else hipLaunchKernelGGL((rbstats_kernel<LPRL, false>), dim3(nb), dim3(256), 0, st, A, C, iters, N, Y, mean, M2, Mout);
}

int run(bool store, const pmgk_rbstats_op *A, int32_t C, double N, const double *Y, double *mean, double *M2, double *Mout, void *stream)
{
  if (A->n <= 0 || C <= 0) return 0;
  if (A->k < 0 || A->k > 64) return 1;
  const hipStream_t st = (hipStream_t)stream;
  int32_t           iters, nb;
  pmgk_rbstats_geometry(A->n, C, &iters, &nb);
  switch (lpr_log2_of(C)) {
  case 0: launch<0>(store, (unsigned)nb, st, *A, C, iters, N, Y, mean, M2, Mout); break;
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

/* rows per wavefront = iters * (64 / lpr) and the number of blocks (4 wavefronts each) of one update or cond_mean: (n, C) only */
extern "C" void pmgk_rbstats_geometry(int64_t n, int32_t nchains, int32_t *iters, int32_t *nblocks)
{
  const int64_t rbi = 4 * (int64_t)(64 >> lpr_log2_of(nchains)); /* rows of a block per iteration */
  const int64_t nbi = (n + rbi - 1) / rbi;
  int64_t       it  = (nbi + MAXBLK - 1) / MAXBLK;
  if (it < 1) it = 1;
  if (nchains > 64 && it > MAXRPW) it = MAXRPW;
  *iters   = (int32_t)it;
  *nblocks = (int32_t)((nbi + it - 1) / it);
}

/* one step: the moments of the conditional means of Y's C samples per row merged into mean / M2 (n each), which hold `count`
   samples per row; with A->k > 0, A->T must hold B^T Y (k x C) */
extern "C" int pmgk_rbstats_update(const pmgk_rbstats_op *A, int32_t nchains, double count, const double *Y, double *mean, double *M2, void *stream)
{
  return run(false, A, nchains, count, Y, mean, M2, NULL, stream);
}

/* M (n x C, the layout of Y) = the conditional means of Y */
extern "C" int pmgk_rbstats_cond_mean(const pmgk_rbstats_op *A, int32_t nchains, const double *Y, double *M, void *stream)
{
  return run(true, A, nchains, 0.0, Y, NULL, NULL, M, stream);
}

/* mean_out = mean, var_out = 1 / q + M2 / (count - 1) (two quotients and one sum, each rounded); either output may be NULL */
extern "C" int pmgk_rbstats_fields(int64_t n, double count, const double *q, const double *mean, const double *M2, double *mean_out, double *var_out, void *stream)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(rbstats_fields_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, count - 1.0, q, mean, M2, mean_out, var_out);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
