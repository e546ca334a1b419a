// Many independent chains per launch on the sliced-ELL (AIJ) path (gfx950): the colour sweep, the residual, the layout
// permutations, the CSR transfer products and the coarse exact sampler of kernels_csr.hip / kernels_dense.hip, each
// advancing C chains of ONE operator in one launch.
//
// Layout: a multi-chain vector holds n x C doubles with the chain index fastest, element (row, chain) at row * C + chain.
// Lanes span the chains of a row: with lpr = lanes per row (C rounded up to a power of two, at most 64), a wavefront
// serves 64 / lpr consecutive rows, and chains beyond 64 go to blockIdx.y.  The matrix entries, idiag, sqrtdiag, orig
// and a shared right-hand side are the same address for all lanes of a row (one fetch per row), and every gather
// Y[col * C + c] is one contiguous segment of 8 * min(C, 64) bytes per row.
//
// Bit identity: every (row, chain) pair runs the single-chain kernel's arithmetic for that row with that chain's noise
// key -- same terms, same order, same roundings (built with -ffp-contract=off like the rest), so column c of a chains
// call equals the single-chain call with seed = keys[c].
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"
#define PMG_RNG_LITERALS // as in kernels_csr.hip
#define PMG_RNG_TU chains
#include "pmg_rng.hpp"

namespace {

constexpr int SELL_BATCH = 8; // as sell_row_sum: the loads of a batch, then its gathers, then the dependent arithmetic

struct lane_map {
  int lpr_log2; // log2 of the lanes that share one row
  int chunks;   // blockIdx.y extent: chain chunks of 64
};

inline lane_map map_chains(int32_t C)
{
  lane_map m{0, (C + 63) / 64};
  if (C >= 64) m.lpr_log2 = 6;
  else
    while ((1 << m.lpr_log2) < C) ++m.lpr_log2;
  return m;
}

// off-diagonal part of row `l` of its slice for chain c: sum -= a_j Y[col_j * C + c] in storage order
__device__ __forceinline__ double sell_row_sum_chains(double sum, int w, const double *__restrict__ v, const int32_t *__restrict__ cl, const double *Y, int64_t C, int c)
{
  for (int j0 = 0; j0 < w; j0 += SELL_BATCH) {
    double  a[SELL_BATCH], yv[SELL_BATCH];
    int32_t cj[SELL_BATCH];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) {
      const int64_t jj = (int64_t)min(j0 + q, w - 1) * 64;
      a[q]             = v[jj];
      cj[q]            = cl[jj];
    }
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) yv[q] = Y[(int64_t)cj[q] * C + c];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q)
      if (j0 + q < w) sum = sum - a[q] * yv[q];
  }
  return sum;
}

// Right-hand sides: chain stride bcs = 0 is ONE vector shared by all chains (b[row]), bcs = 1 one per chain (b[row * C + c]).
__device__ __forceinline__ int64_t b_index(int row, int64_t C, int c, int bcs) { return bcs ? (int64_t)row * C + c : (int64_t)row; }

// one colour: rows row0 .. row0 + nrows - 1 of the layout (whole slices, so a wavefront never straddles two slices and the
// slice width stays wave-uniform)
template <bool NOISY>
__global__ __launch_bounds__(256) void sell_color_sweep_chains_kernel(pmgk_sell S, int row0, int nrows, int lpr_log2, int32_t C, double one_minus_omega, const uint64_t *__restrict__ keys, uint64_t sweep, const double *__restrict__ b, int bcs, double *Y)
{
  __shared__ pmg::LogTabEntry s_logtab[NOISY ? 4 * PMG_LOGTAB_SIZE : 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q0   = (blockIdx.x * 4 + wv) << (6 - lpr_log2); // first row of this wavefront inside the colour
  if (q0 >= nrows) return;
  const pmg::LogTabEntry *tab = s_logtab + (NOISY ? wv * PMG_LOGTAB_SIZE : 0);
  if (NOISY) pmg::load_log_table_wave(s_logtab + wv * PMG_LOGTAB_SIZE, lane); // every lane of the wave provides its entry
  const int c = blockIdx.y * 64 + (lane & ((1 << lpr_log2) - 1));
  if (c >= C) return;
  const int     row  = row0 + q0 + (lane >> lpr_log2); // < row0 + nrows: nrows is a multiple of 64, q0 of 64 / lpr
  const int     s    = row >> 6, l = row & 63;
  const int64_t off  = S.soff[s];
  const int     w    = __builtin_amdgcn_readfirstlane(S.swidth[s]);
  const int     org  = S.orig[row];
  const int64_t yi   = (int64_t)row * C + c;
  double        sum  = b[b_index(row, C, c, bcs)];
  const double  yold = Y[yi], idg = S.idiag[row];
  if (NOISY) {
    const uint64_t key  = keys[c];
    const uint32_t uorg = org < 0 ? 0u : (uint32_t)(S.noise_row0 + org);
    double         z0, z1;
    pmg::normal_pair(uorg >> 1, 0u, (uint32_t)sweep, (uint32_t)(sweep >> 32), (uint32_t)key, (uint32_t)(key >> 32), tab, z0, z1);
    const double xi = (uorg & 1u) ? z1 : z0;
    sum             = xi * S.sqrtdiag[row] + sum;
  }
  sum = sell_row_sum_chains(sum, w, S.vals + off + l, S.cols + off + l, Y, C, c);
  if (org >= 0) Y[yi] = one_minus_omega * yold + idg * sum;
}

// R = b - A Y over all slices, sell_residual_kernel's order of terms (off-diagonal sum from 0, diagonal term last)
__global__ __launch_bounds__(256) void sell_residual_chains_kernel(pmgk_sell S, int lpr_log2, int32_t C, const double *__restrict__ b, int bcs, const double *__restrict__ Y, double *__restrict__ R)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q0   = (blockIdx.x * 4 + wv) << (6 - lpr_log2);
  const int c    = blockIdx.y * 64 + (lane & ((1 << lpr_log2) - 1));
  if (q0 >= S.nslices * 64 || c >= C) return;
  const int      row = q0 + (lane >> lpr_log2);
  const int      s   = row >> 6, l = row & 63;
  const int64_t  off = S.soff[s];
  const int      w   = __builtin_amdgcn_readfirstlane(S.swidth[s]);
  const double  *v   = S.vals + off + l;
  const int32_t *cl  = S.cols + off + l;
  double         sum = 0.0;
  for (int j0 = 0; j0 < w; j0 += SELL_BATCH) {
    double  a[SELL_BATCH], yv[SELL_BATCH];
    int32_t cj[SELL_BATCH];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) {
      const int64_t jj = (int64_t)min(j0 + q, w - 1) * 64;
      a[q]             = v[jj];
      cj[q]            = cl[jj];
    }
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) yv[q] = Y[(int64_t)cj[q] * C + c];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q)
      if (j0 + q < w) sum = sum + a[q] * yv[q];
  }
  const int64_t yi = (int64_t)row * C + c;
  sum              = sum + S.diag[row] * Y[yi];
  R[yi]            = S.orig[row] >= 0 ? b[b_index(row, C, c, bcs)] - sum : 0.0;
}

// natural (n x C; chain stride bcs as above) -> layout (ld x C); pad rows get 0
__global__ __launch_bounds__(256) void permute_in_chains_kernel(int32_t ld, const int32_t *__restrict__ orig, int lpr_log2, int32_t C, const double *__restrict__ nat, int bcs, double *__restrict__ perm)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = t >> lpr_log2;
  const int     c = blockIdx.y * 64 + (int)(t & ((1 << lpr_log2) - 1));
  if (r >= ld || c >= C) return;
  const int o    = orig[r];
  perm[r * C + c] = o >= 0 ? nat[b_index(o, C, c, bcs)] : 0.0;
}

__global__ __launch_bounds__(256) void permute_out_chains_kernel(int32_t ld, const int32_t *__restrict__ orig, int lpr_log2, int32_t C, const double *__restrict__ perm, double *__restrict__ nat)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = t >> lpr_log2;
  const int     c = blockIdx.y * 64 + (int)(t & ((1 << lpr_log2) - 1));
  if (r >= ld || c >= C) return;
  const int o = orig[r];
  if (o >= 0) nat[(int64_t)o * C + c] = perm[r * C + c];
}

// Y[rowpos[r]] (+)= sum_k vals[k] X[colidx[k]] per chain, csr_spmv_rows_kernel's batches and order of terms
template <bool ACC>
__global__ __launch_bounds__(256) void csr_spmv_rows_chains_kernel(int32_t nrows, const int32_t *__restrict__ rowpos, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ vals, int lpr_log2, int32_t C, const double *__restrict__ X, double *__restrict__ Y, double *__restrict__ zero)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = t >> lpr_log2;
  const int     c = blockIdx.y * 64 + (int)(t & ((1 << lpr_log2) - 1));
  if (r >= nrows || c >= C) return;
  const int     k0 = rowptr[r], k1 = rowptr[r + 1];
  const int64_t o  = (int64_t)rowpos[r] * C + c;
  double        yo = 0.0;
  if (ACC) yo = Y[o];
  double sum = 0.0;
  for (int kb = k0; kb < k1; kb += SELL_BATCH) {
    double  a[SELL_BATCH], xv[SELL_BATCH];
    int32_t cj[SELL_BATCH];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) {
      const int kk = min(kb + q, k1 - 1);
      a[q]         = vals[kk];
      cj[q]        = colidx[kk];
    }
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q) xv[q] = X[(int64_t)cj[q] * C + c];
#pragma unroll
    for (int q = 0; q < SELL_BATCH; ++q)
      if (kb + q < k1) sum = sum + a[q] * xv[q];
  }
  Y[o] = ACC ? yo + sum : sum;
  if (zero) zero[o] = 0.0;
}

// Xi[i * C + c] = entry i of fill_normal_rows_kernel's stream (keys[c], sweep): pair q gives entries 2q (cos) and 2q+1 (sin)
__global__ __launch_bounds__(256) void fill_normal_rows_chains_kernel(int64_t n, int lpr_log2, int32_t C, const uint64_t *__restrict__ keys, uint64_t sweep, double *__restrict__ Xi)
{
  __shared__ pmg::LogTabEntry s_logtab[PMG_LOGTAB_SIZE];
  pmg::load_log_table(s_logtab);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t q = t >> lpr_log2;
  const int     c = blockIdx.y * 64 + (int)(t & ((1 << lpr_log2) - 1));
  if (2 * q >= n || c >= C) return;
  const uint64_t key = keys[c];
  double         z0, z1;
  pmg::normal_pair((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)sweep, (uint32_t)(sweep >> 32), (uint32_t)key, (uint32_t)(key >> 32), s_logtab, z0, z1);
  Xi[2 * q * C + c] = z0;
  if (2 * q + 1 < n) Xi[(2 * q + 1) * C + c] = z1;
}

// Out = M X (+ Add) for the lower or upper triangle of the row-major n x n matrix M on C right-hand sides.  One block per
// row of M, one wavefront per group of TRI_CG chains: a lane reads its four entries of the row once and applies them to the
// group's chains.  Per chain the arithmetic is tri_gemv_kernel's: lane `lane` accumulates columns kb + 2 lane, +1, +128,
// +129 into four fma sums, then (s0 + s1) + (s2 + s3) and the shuffle-down reduction over the 64 lanes.
constexpr int TRI_CG = 8;
template <bool UPPER>
__global__ __launch_bounds__(256) void tri_gemv_chains_kernel(int32_t n, const double *__restrict__ M, int32_t C, const double *__restrict__ X, const double *__restrict__ Add, double *__restrict__ Out)
{
  const int lane = threadIdx.x & 63;
  const int c0   = (blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6)) * TRI_CG;
  if (c0 >= C) return; // whole wavefronts
  const int     i   = blockIdx.x;
  const int     k0  = UPPER ? i : 0, k1 = UPPER ? n : i + 1;
  const double *row = M + (int64_t)i * n;
  double        s[4][TRI_CG];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int j = 0; j < TRI_CG; ++j) s[p][j] = 0.0;
  for (int kb = k0; kb < k1; kb += 256) {
    const int ka = kb + 2 * lane, kc = ka + 128;
    const int kk[4] = {ka, ka + 1, kc, kc + 1};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (kk[p] >= k1) continue;
      const double  m = row[kk[p]];
      const double *x = X + (int64_t)kk[p] * C + c0;
#pragma unroll
      for (int j = 0; j < TRI_CG; ++j)
        if (c0 + j < C) s[p][j] = fma(m, x[j], s[p][j]);
    }
  }
#pragma unroll
  for (int j = 0; j < TRI_CG; ++j) {
    double v = (s[0][j] + s[1][j]) + (s[2][j] + s[3][j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0 && c0 + j < C) {
      const int64_t o = (int64_t)i * C + c0 + j;
      Out[o]          = Add ? v + Add[o] : v;
    }
  }
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : 1; }

// blocks of 256 threads over `rows` rows with 2^lpr_log2 lanes per row
inline dim3 row_grid(int64_t rows, const lane_map &m) { return dim3((unsigned)((rows * (1 << m.lpr_log2) + 255) / 256), (unsigned)m.chunks); }

} // namespace

extern "C" int pmgk_sell_color_sweep_chains(const pmgk_sell *S, int slice0, int nsl, double omega, int noisy, const uint64_t *keys, uint64_t sweep, int32_t nchains, const double *b, int bcs, double *Y, void *stream)
{
  if (nsl <= 0 || nchains <= 0) return 0;
  const lane_map m    = map_chains(nchains);
  const int      rows = nsl * 64;
  const dim3     grid = row_grid(rows, m), block(256);
  const double   om1  = 1. - omega;
  if (noisy) hipLaunchKernelGGL((sell_color_sweep_chains_kernel<true>), grid, block, 0, (hipStream_t)stream, *S, slice0 * 64, rows, m.lpr_log2, nchains, om1, keys, sweep, b, bcs, Y);
  else hipLaunchKernelGGL((sell_color_sweep_chains_kernel<false>), grid, block, 0, (hipStream_t)stream, *S, slice0 * 64, rows, m.lpr_log2, nchains, om1, keys, sweep, b, bcs, Y);
  return launch_status();
}

extern "C" int pmgk_sell_residual_chains(const pmgk_sell *S, int32_t nchains, const double *b, int bcs, const double *Y, double *R, void *stream)
{
  if (S->nslices <= 0 || nchains <= 0) return 0;
  const lane_map m = map_chains(nchains);
  hipLaunchKernelGGL(sell_residual_chains_kernel, row_grid((int64_t)S->nslices * 64, m), dim3(256), 0, (hipStream_t)stream, *S, m.lpr_log2, nchains, b, bcs, Y, R);
  return launch_status();
}

extern "C" int pmgk_permute_in_chains(int32_t ld, const int32_t *orig, int32_t nchains, const double *nat, int bcs, double *perm, void *stream)
{
  if (ld <= 0 || nchains <= 0) return 0;
  const lane_map m = map_chains(nchains);
  hipLaunchKernelGGL(permute_in_chains_kernel, row_grid(ld, m), dim3(256), 0, (hipStream_t)stream, ld, orig, m.lpr_log2, nchains, nat, bcs, perm);
  return launch_status();
}

extern "C" int pmgk_permute_out_chains(int32_t ld, const int32_t *orig, int32_t nchains, const double *perm, double *nat, void *stream)
{
  if (ld <= 0 || nchains <= 0) return 0;
  const lane_map m = map_chains(nchains);
  hipLaunchKernelGGL(permute_out_chains_kernel, row_grid(ld, m), dim3(256), 0, (hipStream_t)stream, ld, orig, m.lpr_log2, nchains, perm, nat);
  return launch_status();
}

extern "C" int pmgk_csr_spmv_rows_chains(int32_t nrows, const int32_t *rowpos, const int32_t *rowptr, const int32_t *colidx, const double *vals, int32_t nchains, const double *X, double *Y, int accumulate, double *zero, void *stream)
{
  if (nrows <= 0 || nchains <= 0) return 0;
  const lane_map m    = map_chains(nchains);
  const dim3     grid = row_grid(nrows, m), block(256);
  if (accumulate) hipLaunchKernelGGL((csr_spmv_rows_chains_kernel<true>), grid, block, 0, (hipStream_t)stream, nrows, rowpos, rowptr, colidx, vals, m.lpr_log2, nchains, X, Y, zero);
  else hipLaunchKernelGGL((csr_spmv_rows_chains_kernel<false>), grid, block, 0, (hipStream_t)stream, nrows, rowpos, rowptr, colidx, vals, m.lpr_log2, nchains, X, Y, zero);
  return launch_status();
}

extern "C" int pmgk_fill_normal_rows_chains(int64_t n, int32_t nchains, const uint64_t *keys, uint64_t sweep, double *Xi, void *stream)
{
  if (n <= 0 || nchains <= 0) return 0;
  const lane_map m = map_chains(nchains);
  hipLaunchKernelGGL(fill_normal_rows_chains_kernel, row_grid((n + 1) / 2, m), dim3(256), 0, (hipStream_t)stream, n, m.lpr_log2, nchains, keys, sweep, Xi);
  return launch_status();
}

extern "C" int pmgk_tri_gemv_chains(int32_t n, int upper, const double *M, int32_t nchains, const double *X, const double *Add, double *Out, void *stream)
{
  if (n <= 0 || nchains <= 0) return 0;
  const int  groups = (nchains + TRI_CG - 1) / TRI_CG, wpb = groups < 4 ? groups : 4;
  const dim3 grid((unsigned)n, (unsigned)((groups + wpb - 1) / wpb)), block(64 * wpb);
  if (upper) hipLaunchKernelGGL((tri_gemv_chains_kernel<true>), grid, block, 0, (hipStream_t)stream, n, M, nchains, X, Add, Out);
  else hipLaunchKernelGGL((tri_gemv_chains_kernel<false>), grid, block, 0, (hipStream_t)stream, n, M, nchains, X, Add, Out);
  return launch_status();
}
