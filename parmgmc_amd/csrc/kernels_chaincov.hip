// Covariance over the chains on the device (gfx950): err = ||C_step - Sigma||_F / ||Sigma||_F of one step's n x C sample array Y
// with C_step the unbiased covariance over the chains (SampleMean / SampleCovariance / EstimateCovarianceMatErrors,
// src/stats.c:55-117; the study of examples/ex6.c:168-193), as a symmetric rank-C update on v_mfma_f64_16x16x4_f64 followed by a
// norm.  In the error path the covariance is never written to memory: a workgroup keeps its 32 x 32 tile in accumulators,
// subtracts the Sigma tile and leaves ONE double per tile.
//
// Layout: Y[row * K + k], k (the chain) fastest, natural rows -- what pmg_*_sample_chains write.  Sigma and the matrix output are
// n x n row-major (symmetric).  Only the lower-triangle tile grid (ti >= tj, 32 x 32 tiles, T = ceil(n / 32), T (T + 1) / 2
// workgroups) is computed.  A and B operands of the tile product are both rows of Y: a workgroup of four wavefronts stages
// chunks of 64 k of its two row panels through LDS (row stride 66 doubles: the 32 lanes of a ds_read_b64 group read rows
// lane & 15 at k and k + 1, banks 2 * row + k, all different), subtracting the row mean while staging (centred products, not
// E[y y^T] - m m^T) and zero-filling rows >= n and k >= K; the next chunk's loads are in flight during the MFMAs of this one.
// Wavefront v takes k in [16 v, 16 v + 16) of every chunk, so a workgroup splits K four ways (n = 1024 has only 528 tiles).
// f64 MFMA operand maps (kernels_dense.hip, pinned by the Cholesky tests): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4]
// [col = lane & 15], C/D col = lane & 15, row = (lane >> 4) + 4 * reg.
//
// ORDER OF EVERY SUM -- a function of (n, K) alone:
//   row mean: lane l of the row's wavefront adds Y[row, l], Y[row, l + 64], ... from 0.0 ascending; the 64 lanes are combined
//     by the balanced tree, neighbours first (l with l ^ 1, then l ^ 2, ...); mean = sum / K.
//   tile element (r, s): wavefront v accumulates, from 0.0, one MFMA per group of four k {64 j + 16 v + 4 q + (0..3)},
//     j = 0, 1, ... outermost, q = 0..3 (groups that start at k >= K are skipped; inside a group the instruction's own fixed
//     order); the four wavefronts are combined through LDS as (v0 + v1) + (v2 + v3); the sum is divided by K - 1.
//   tile partial: thread t of 256 adds d^2 (two roundings), d = C_rs - Sigma_rs, from 0.0 over accumulator slots i = (t >> 6) +
//     4 j, j = 0..3, lane t & 63 (elements outside the matrix count 0.0); the 256 thread values are combined by the LDS tree
//     (t with t + 128, then t + 64, ... t + 1); off-diagonal tiles are doubled (exact).  Diagonal tiles are computed in full.
//   step: thread t of 256 adds the tile partials t, t + 256, ... from 0.0 ascending (tiles numbered ti (ti + 1) / 2 + tj), the
//     same LDS tree; err = sqrt(sum) / ||Sigma||_F.  ||Sigma||_F is the same two-stage sum over the squared entries of Sigma.
// No floating-point atomics anywhere; -ffp-contract=off as the rest of the library.  Two runs give the same bits, on any stream.
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int TB = 32;     // tile edge
constexpr int KC = 64;     // k per staged chunk
constexpr int LDP = KC + 2; // row stride of a staged panel (doubles)

// tile number -> (ti >= tj), row-major enumeration of the lower triangle
__device__ __forceinline__ void tile_of(int tile, int &ti, int &tj)
{
  int i = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= tile) ++i;
  while (i * (i + 1) / 2 > tile) --i;
  ti = i, tj = tile - i * (i + 1) / 2;
}

// blk[0] = tree over the 256 thread values (t with t + 128 first)
__device__ __forceinline__ double block_tree(double v, double *blk)
{
  const int t = threadIdx.x;
  blk[t]      = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o >= 1; o >>= 1) {
    if (t < o) blk[t] = blk[t] + blk[t + o];
    __syncthreads();
  }
  return blk[0];
}

__global__ __launch_bounds__(256) void chaincov_mean_kernel(int32_t n, int32_t K, const double *__restrict__ Y, double *__restrict__ mean)
{
  const int lane = threadIdx.x & 63;
  const int row  = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return; // whole wavefronts
  const double *y = Y + (int64_t)row * K;
  double        s = 0.0;
  for (int k = lane; k < K; k += 64) s = s + y[k];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o, 64);
  if (lane == 0) mean[row] = s / (double)K;
}

// OUT = false: partial[tile] = sum over the tile of (acc / denom - Sigma)^2 (doubled off the diagonal)
// OUT = true:  Cout (n x n, both triangles) = acc / denom
template <bool OUT>
__global__ __launch_bounds__(256) void chaincov_syrk_kernel(int32_t n, int32_t K, const double *__restrict__ Y, const double *__restrict__ mean, double denom, const double *__restrict__ Sigma, double *__restrict__ partial, double *__restrict__ Cout)
{
  __shared__ double sm[2 * TB * LDP]; // the two panels; afterwards the 4 x 16 x 64 accumulators of the wavefronts
  __shared__ double blk[256];
  static_assert(2 * TB * LDP >= 4 * 16 * 64, "the accumulators fit the panels' LDS");
  double   *As = sm, *Bs = sm + TB * LDP;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lk = lane >> 4;
  int       ti, tj;
  tile_of((int)blockIdx.x, ti, tj);
  // staging: thread t carries k = t & 63 of rows (t >> 6) + 4 p, p = 0..7, of both panels
  const int kk = t & 63, r0 = t >> 6;
  double    mA[8], mB[8], ya[8], yb[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int ga = ti * TB + r0 + 4 * p, gb = tj * TB + r0 + 4 * p;
    mA[p]        = mean && ga < n ? mean[ga] : 0.0;
    mB[p]        = mean && gb < n ? mean[gb] : 0.0;
  }
  auto load = [&](int kb) {
    const int  k  = kb + kk;
    const bool kl = k < K;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int ga = ti * TB + r0 + 4 * p, gb = tj * TB + r0 + 4 * p;
      ya[p]        = kl && ga < n ? Y[(int64_t)ga * K + k] - mA[p] : 0.0;
      yb[p]        = kl && gb < n ? Y[(int64_t)gb * K + k] - mB[p] : 0.0;
    }
  };
  v4d acc[2][2] = {};
  load(0);
  for (int kb = 0; kb < K; kb += KC) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      As[(r0 + 4 * p) * LDP + kk] = ya[p];
      Bs[(r0 + 4 * p) * LDP + kk] = yb[p];
    }
    __syncthreads();
    if (kb + KC < K) load(kb + KC);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k0 = 16 * wv + 4 * q;
      if (kb + k0 < K) { // uniform over the wavefront
        const int    k  = k0 + lk;
        const double a0 = As[lr * LDP + k], a1 = As[(16 + lr) * LDP + k];
        const double b0 = Bs[lr * LDP + k], b1 = Bs[(16 + lr) * LDP + k];
        acc[0][0]       = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1]       = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0]       = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1]       = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    __syncthreads(); // the panels are overwritten by the next chunk (and by the accumulators after the last)
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sm[(wv * 16 + (a * 2 + b) * 4 + reg) * 64 + lane] = acc[a][b][reg];
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int    i = wv + 4 * j; // accumulator slot (a, b, reg)
    const double v = (sm[i * 64 + lane] + sm[(16 + i) * 64 + lane]) + (sm[(32 + i) * 64 + lane] + sm[(48 + i) * 64 + lane]);
    const int    a = i >> 3, b = (i >> 2) & 1, reg = i & 3;
    const int    gr = ti * TB + 16 * a + lk + 4 * reg, gc = tj * TB + 16 * b + lr;
    const double c  = v / denom;
    if (OUT) {
      if (gr < n && gc < n && (ti != tj || gr >= gc)) { // a diagonal tile writes its lower half and mirrors it: exactly symmetric
        Cout[(int64_t)gr * n + gc] = c;
        Cout[(int64_t)gc * n + gr] = c;
      }
    } else {
      const double d = gr < n && gc < n ? c - Sigma[(int64_t)gr * n + gc] : 0.0;
      s              = s + d * d;
    }
  }
  if (!OUT) {
    const double tot = block_tree(s, blk);
    if (t == 0) partial[blockIdx.x] = ti != tj ? 2.0 * tot : tot;
  }
}

// partial[tile] = sum of the squared entries of the tile of Sigma (doubled off the diagonal)
__global__ __launch_bounds__(256) void chaincov_sqnorm_kernel(int32_t n, const double *__restrict__ Sigma, double *__restrict__ partial)
{
  __shared__ double blk[256];
  const int         t = threadIdx.x;
  int               ti, tj;
  tile_of((int)blockIdx.x, ti, tj);
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int    e = t + 256 * j, gr = ti * TB + (e >> 5), gc = tj * TB + (e & 31);
    const double d = gr < n && gc < n ? Sigma[(int64_t)gr * n + gc] : 0.0;
    s              = s + d * d;
  }
  const double tot = block_tree(s, blk);
  if (t == 0) partial[blockIdx.x] = ti != tj ? 2.0 * tot : tot;
}

// out[0] = sqrt(sum of the tile partials) (/ norm[0])
__global__ __launch_bounds__(256) void chaincov_reduce_kernel(int ntiles, const double *__restrict__ partial, const double *__restrict__ norm, double *__restrict__ out)
{
  __shared__ double blk[256];
  double            s = 0.0;
  for (int i = threadIdx.x; i < ntiles; i += 256) s = s + partial[i];
  const double tot = block_tree(s, blk);
  if (threadIdx.x == 0) out[0] = norm ? sqrt(tot) / norm[0] : sqrt(tot);
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : 1; }

} // namespace

/* tiles of the lower triangle = workgroups of the tile kernels = doubles of `partial` */
extern "C" int pmgk_chaincov_ntiles(int32_t n)
{
  const int T = (n + TB - 1) / TB;
  return T * (T + 1) / 2;
}

/* mean[r] = (sum_k Y[r, k]) / K */
extern "C" int pmgk_chaincov_means(int32_t n, int32_t K, const double *Y, double *mean, void *stream)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(chaincov_mean_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n, K, Y, mean);
  return launch_status();
}

/* partial[tile] of || (Y - mean)(Y - mean)^T / denom - Sigma ||_F^2; mean == NULL: no centring */
extern "C" int pmgk_chaincov_syrk_error(int32_t n, int32_t K, const double *Y, const double *mean, double denom, const double *Sigma, double *partial, void *stream)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL((chaincov_syrk_kernel<false>), dim3((unsigned)pmgk_chaincov_ntiles(n)), dim3(256), 0, (hipStream_t)stream, n, K, Y, mean, denom, Sigma, partial, (double *)nullptr);
  return launch_status();
}

/* Cout (n x n row-major, both triangles) = (Y - mean)(Y - mean)^T / denom */
extern "C" int pmgk_chaincov_syrk_matrix(int32_t n, int32_t K, const double *Y, const double *mean, double denom, double *Cout, void *stream)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL((chaincov_syrk_kernel<true>), dim3((unsigned)pmgk_chaincov_ntiles(n)), dim3(256), 0, (hipStream_t)stream, n, K, Y, mean, denom, (const double *)nullptr, (double *)nullptr, Cout);
  return launch_status();
}

extern "C" int pmgk_chaincov_sqnorm_tiles(int32_t n, const double *Sigma, double *partial, void *stream)
{
  if (n <= 0) return 0;
  hipLaunchKernelGGL(chaincov_sqnorm_kernel, dim3((unsigned)pmgk_chaincov_ntiles(n)), dim3(256), 0, (hipStream_t)stream, n, Sigma, partial);
  return launch_status();
}

/* out[0] = sqrt(sum_i partial[i]) / norm[0] (norm == NULL: no division) */
extern "C" int pmgk_chaincov_reduce(int ntiles, const double *partial, const double *norm, double *out, void *stream)
{
  hipLaunchKernelGGL(chaincov_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ntiles, partial, norm, out);
  return launch_status();
}
