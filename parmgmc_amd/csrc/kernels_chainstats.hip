// Running statistics of the chains on the device (gfx950): ONE pass over a step's n x C sample array Y updates the running mean
// and sum of squared deviations of every row over all samples seen (MS_ComputeMeanAndVar, src/ms.c:221-251; the benchmark's
// Welford loop, examples/benchmark/main.cc:151-175) and forms the quantities of interest t[q][c] = sum_r w_q[r] Y[r, c] of every
// chain (the VecSum / VecDot of examples/ex7.c:45-46).  Y is read from memory exactly once.
//
// Layout and lane mapping: kernels_chains.hip's.  Y[row * C + c], chain fastest; lpr = C rounded up to a power of two (at most
// 64) lanes share a row, a wavefront serves G = 64 / lpr rows at a time and keeps RW = 8 such row groups in flight; chains
// beyond 64 are taken in chunks of 64 by the SAME wavefront (chunk loop outermost, the row statistics of a chunk parked in LDS),
// so that a row's statistics are complete when its last chunk has been read.
//
// ORDER OF EVERY SUM -- a function of (n, C) alone (pmgk_chainstats_geometry has no other input):
//   row sum and sum of squared deviations over the chains of a chunk: the balanced binary tree over the lpr lane slots of the
//     row, neighbours first (slot i with i ^ 1, then i ^ 2, ...; slots c >= C hold +0.0).  Both operands of every node are
//     exchanged, so all lanes of the row hold the same bits.
//   chunk:  cm = s / cnt, cM2 = tree of (y_c - cm)^2 (second pass over the registers, not a sum of squares), cnt = chains of the
//     chunk.  The step's batch (C, bm, bM2) is chunk 0 merged with chunks 1, 2, ... in that order by the pairwise formula below
//     (for C <= 64 there is one chunk: bm = (sum_c y_c) / C, bM2 = sum_c (y_c - bm)^2).
//   merge of (Nb, mb, Mb) into (N, m, M):  d = mb - m;  N' = N + Nb;  m = m + (d * Nb) / N';  M = M + (Mb + (((d * d) * N) * Nb) / N');
//     Chan/Golub/LeVeque; with C = 1 it is Welford's update.  The first step starts from N = 0, m = 0, M = 0.
//   QOI: rows are cut into blocks of 4 * rpw rows (rpw = iters * G * RW rows per wavefront, iters from the geometry).  Lane
//     (g, c) of wavefront v of block B adds w[r] * Y[r, c] (two roundings) from 0.0 over the rows r = (4 B + v) rpw + j G + g,
//     j = 0, 1, ... ascending; the G lanes of a chain are combined by the balanced tree over g (g with g ^ 1 first), the four
//     wavefronts as (v0 + v1) + (v2 + v3).  The block values are summed by chainstats_reduce_kernel: slot l < 64 adds blocks l,
//     l + 64, ... from 0.0 ascending, the 64 slots are combined by the shuffle-down tree (offsets 32, 16, ... 1).
// No floating-point atomics anywhere; -ffp-contract=off as the rest of the library.
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"
#include "pmg_chain_moments.hpp"

namespace {

constexpr int RW     = 8;                        // row groups a wavefront keeps in flight
constexpr int MAXQ   = PMGK_CHAINSTATS_MAX_QOI;  // accumulators a lane carries
constexpr int MAXRPW = 256;                      // rows per wavefront when the chains are chunked (their statistics wait in LDS)
constexpr int MAXBLK = 1024;                     // blocks of the update for C <= 64: every wavefront resident at once

inline int lpr_log2_of(int32_t C)
{
  int l = 0;
  while (l < 6 && (1 << l) < C) ++l;
  return l;
}

// the tree over the lane slots, the chunk moments and the merge: pmg_chain_moments.hpp, shared with kernels_rbstats.hip
using pmg_moments::chunk_batch;
using pmg_moments::chunk_moments;
using pmg_moments::merge;

template <int LPRL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void chainstats_update_kernel(int64_t n, int32_t C, int nq, pmgk_chainstats_qoi Q, int iters, double N, const double *__restrict__ Y, double *__restrict__ mean, double *__restrict__ M2, double *__restrict__ partial)
{
  constexpr int     LPR = 1 << LPRL, G = 64 / LPR, RWI = G * RW;
  __shared__ double red[4][MAXQ][64];
  __shared__ double parked[LPRL == 6 ? 4 * MAXRPW * 2 : 2]; // (mean, M2) of the chunks read so far, per row of a wavefront
  const int     lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> LPRL, cl = lane & (LPR - 1);
  const int64_t row0   = ((int64_t)blockIdx.x * 4 + wv) * ((int64_t)iters * RWI);
  const int     chunks = LPRL == 6 ? (C + 63) / 64 : 1;
  const bool    first  = N == 0.0;
  for (int k = 0; k < chunks; ++k) {
    const int    c    = k * 64 + cl;
    const bool   live = c < C;
    const double cnt  = (double)min(64, C - k * 64), seen = 64.0 * k; // chains of this chunk, of the chunks before it
    double       acc[MAXQ];
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) acc[q] = 0.0;
    for (int it = 0; it < iters; ++it) {
      const int64_t rb = row0 + (int64_t)it * RWI + g;
      double        y[RW], mo[RW], vo[RW];
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const int64_t row = rb + i * G;
        y[i]              = live && row < n ? Y[row * C + c] : 0.0;
      }
      const bool last = k == chunks - 1;
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const int64_t row = rb + i * G;
        const bool    ld  = last && !first && cl == 0 && row < n;
        mo[i]             = ld ? mean[row] : 0.0;
        vo[i]             = ld ? M2[row] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < MAXQ; ++q)
        if (q < nq) {
          const double *w = Q.w[q];
          if (w) {
            double wr[RW];
#pragma unroll
            for (int i = 0; i < RW; ++i) wr[i] = rb + i * G < n ? w[rb + i * G] : 0.0;
#pragma unroll
            for (int i = 0; i < RW; ++i) acc[q] = acc[q] + wr[i] * y[i];
          } else {
#pragma unroll
            for (int i = 0; i < RW; ++i) acc[q] = acc[q] + y[i];
          }
        }
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const int64_t row = rb + i * G;
        double        cm, cM2;
        chunk_moments<LPR>(y[i], live, cnt, cm, cM2);
        double bm = cm, bM2 = cM2;
        if (LPRL == 6 && chunks > 1) // G = 1: the wavefront's rows are it * RW + i
          chunk_batch(parked + ((wv * MAXRPW) + it * RW + i) * 2, k, last, lane, seen, cnt, cm, cM2, bm, bM2);
        if (last && cl == 0 && row < n) {
          merge(N, mo[i], vo[i], (double)C, bm, bM2);
          mean[row] = mo[i];
          M2[row]   = vo[i];
        }
      }
    }
    if (nq > 0) { // uniform over the block
#pragma unroll
      for (int q = 0; q < MAXQ; ++q)
        if (q < nq) {
          double v = acc[q];
#pragma unroll
          for (int o = LPR; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
          if (g == 0) red[wv][q][cl] = v;
        }
      __syncthreads();
      for (int t = threadIdx.x; t < nq * LPR; t += 256) {
        const int q = t >> LPRL, cc = t & (LPR - 1), ch = k * 64 + cc;
        if (ch < C) partial[((int64_t)blockIdx.x * nq + q) * C + ch] = (red[0][q][cc] + red[1][q][cc]) + (red[2][q][cc] + red[3][q][cc]);
      }
    }
    __syncthreads(); // red and parked are reused by the next chunk
  }
}

// out[q * qstride + c] = sum over the nb block values of (q, c); block (4 chains, QOI blockIdx.y), 64 slots per chain
__global__ __launch_bounds__(256) void chainstats_reduce_kernel(int nb, int nq, int32_t C, const double *__restrict__ partial, double *__restrict__ out, int64_t qstride)
{
  __shared__ double red[64][4];
  const int l = threadIdx.x >> 2, cc = threadIdx.x & 3, q = blockIdx.y;
  const int c = blockIdx.x * 4 + cc;
  double    a = 0.0;
  if (c < C)
    for (int b = l; b < nb; b += 64) a = a + partial[((int64_t)b * nq + q) * C + c];
  red[l][cc] = a;
  __syncthreads();
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    if (l < o) red[l][cc] = red[l][cc] + red[l + o][cc];
    __syncthreads();
  }
  if (l == 0 && c < C) out[(int64_t)q * qstride + c] = red[0][cc];
}

__global__ __launch_bounds__(256) void chainstats_fields_kernel(int64_t n, double Nm1, const double *__restrict__ mean, const double *__restrict__ M2, double *__restrict__ mean_out, double *__restrict__ var_out)
{
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  if (mean_out) mean_out[r] = mean[r];
  if (var_out) var_out[r] = M2[r] / Nm1;
}

template <int LPRL>
void launch_update(unsigned nb, hipStream_t st, int64_t n, int32_t C, int nq, const pmgk_chainstats_qoi &Q, int iters, double N, const double *Y, double *mean, double *M2, double *partial)
{
  hipLaunchKernelGGL((chainstats_update_kernel<LPRL>), dim3(nb), dim3(256), 0, st, n, C, nq, Q, iters, N, Y, mean, M2, partial);
}

} // namespace

/* rows per wavefront = iters * (64 / lpr) * 8 and the number of blocks (4 wavefronts each) of one update: (n, C) only */
extern "C" void pmgk_chainstats_geometry(int64_t n, int32_t nchains, int32_t *iters, int32_t *nblocks)
{
  const int     lprl = lpr_log2_of(nchains);
  const int64_t rbi  = 4 * (int64_t)(64 >> lprl) * RW; /* rows of a block per iteration */
  const int64_t nbi  = (n + rbi - 1) / rbi;
  int64_t       it   = (nbi + MAXBLK - 1) / MAXBLK;
  if (it < 1) it = 1;
  if (nchains > 64 && it > MAXRPW / RW) it = MAXRPW / RW;
  *iters   = (int32_t)it;
  *nblocks = (int32_t)((nbi + it - 1) / it);
}

/* one step: mean / M2 (n each) merged with the C samples of every row, Q->w[q] . Y[:, c] into trace_step[q * qstride + c];
   count = samples merged before this step; partial: nblocks * nqoi * C doubles */
extern "C" int pmgk_chainstats_update(int64_t n, int32_t nchains, int nqoi, const pmgk_chainstats_qoi *Q, double count, const double *Y, double *mean, double *M2, double *partial, double *trace_step, int64_t qstride, void *stream)
{
  if (n <= 0 || nchains <= 0) return 0;
  if (nqoi < 0 || nqoi > MAXQ) return 1;
  const hipStream_t st = (hipStream_t)stream;
  int32_t           iters, nb;
  pmgk_chainstats_geometry(n, nchains, &iters, &nb);
  switch (lpr_log2_of(nchains)) {
  case 0: launch_update<0>((unsigned)nb, st, n, nchains, nqoi, *Q, iters, count, Y, mean, M2, partial); break;
  case 1: launch_update<1>((unsigned)nb, st, n, nchains, nqoi, *Q, iters, count, Y, mean, M2, partial); break;
  case 2: launch_update<2>((unsigned)nb, st, n, nchains, nqoi, *Q, iters, count, Y, mean, M2, partial); break;
  case 3: launch_update<3>((unsigned)nb, st, n, nchains, nqoi, *Q, iters, count, Y, mean, M2, partial); break;
  case 4: launch_update<4>((unsigned)nb, st, n, nchains, nqoi, *Q, iters, count, Y, mean, M2, partial); break;
  case 5: launch_update<5>((unsigned)nb, st, n, nchains, nqoi, *Q, iters, count, Y, mean, M2, partial); break;
  default: launch_update<6>((unsigned)nb, st, n, nchains, nqoi, *Q, iters, count, Y, mean, M2, partial); break;
  }
  if (nqoi > 0) hipLaunchKernelGGL(chainstats_reduce_kernel, dim3((unsigned)((nchains + 3) / 4), (unsigned)nqoi), dim3(256), 0, st, nb, nqoi, nchains, partial, trace_step, qstride);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

/* mean_out = mean, var_out = M2 / (count - 1); either output may be NULL */
extern "C" int pmgk_chainstats_fields(int64_t n, double count, const double *mean, const double *M2, double *mean_out, double *var_out, void *stream)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(chainstats_fields_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, count - 1.0, mean, M2, mean_out, var_out);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
