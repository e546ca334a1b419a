// Integrated autocorrelation time of many series on the device (gfx950): IACT with AutoWindow(c = 5) of the reference
// (src/iact.c:17-92, restated on the host by pmg_iact, pmg_diag.c:73-108) for every column of X (n x S, series fastest,
// X[t * ld + s]: a window of a pmg_chainstats trace).  The autocorrelation is formed directly, lag block by lag block, and the
// scan of a series stops at the first block that holds its window: n * (window + LAG_BLOCK) multiply-adds per series, not n^2.
//
// Two kernels.
//   iact_transpose_kernel: 32 x 32 tiles through LDS, Z[s * n + t] = X[t * ld + s]: every later read of a series is contiguous.
//   iact_scan_kernel: one workgroup of LB = PMGK_IACT_LAG_BLOCK lanes per series.  Phase A centres the series in place in Z.
//     Phase B takes the lags in blocks [kb, kb + LB), lane j owning lag k = kb + j.  Time runs in tiles of TILE steps: the tile
//     z[t0 .. t0 + TILE) and the shifted tile z[t0 + kb .. t0 + kb + TILE + LB) (a halo of one lag block) are staged in LDS, zero
//     where the index reaches n; z_t is then an LDS broadcast and z_{t + k} a read of consecutive doubles over the lanes.  After
//     a block lane 0 continues the running sum of rho in lag order and tests the window rule; the block loop ends at the first
//     hit (or once nacf lags have been written).
//
// ORDER OF EVERY SUM -- a function of (n, k) alone:
//   mean:  slot j < LB adds x_t from 0.0 over t = j, j + LB, ... ascending; the LB slots are combined by the tree with the far
//     half first (slot j with j + LB/2, then j + LB/4, ... j + 1); m = sum / n;  z_t = x_t - m.
//   c_k = sum_{t < n - k} z_t z_{t+k}:  four accumulators, accumulator r takes t = r, r + 4, r + 8, ... ascending from 0.0, each
//     term by one fused multiply-add (a single rounding per term); c_k = (a0 + a1) + (a2 + a3).  Terms with t + k >= n enter as
//     z * (+0.0) and leave the accumulators unchanged.
//   rho_k = c_k / c_0;  P_k = P_{k-1} + rho_k in lag order, k = 0, 1, ... (src/iact.c:85-86);  T_k = 2 P_k - 1.
//   window = first k with (double)k >= 5 T_k;  tau = T_window;  valid = 500 tau <= n.
// No floating-point atomics; nothing depends on the stream, on max_lag, on nacf or on the other series of the call.
#include <hip/hip_runtime.h>
#include <math.h>
#include "pmg_kernels.h"

namespace {

constexpr int LB   = PMGK_IACT_LAG_BLOCK; // lags per block = lanes of the scan workgroup
constexpr int TILE = 1024;                // time steps staged per tile: 8 (TILE + TILE + LB) = 18 KiB of LDS
constexpr int TT   = 32;                  // edge of a transpose tile
static_assert(LB >= 64 && LB <= 512 && (LB & (LB - 1)) == 0, "the lag block is a power of two between 64 and 512");
static_assert(TILE % LB == 0 && TILE % 4 == 0, "the staging loops and the four accumulators tile the time tile");

__global__ __launch_bounds__(256) void iact_transpose_kernel(int64_t n, int32_t S, const double *__restrict__ X, int64_t ld, double *__restrict__ Z)
{
  __shared__ double tile[TT][TT + 1];
  const int     tx = threadIdx.x & (TT - 1), ty = threadIdx.x >> 5;
  const int64_t t0 = (int64_t)blockIdx.x * TT;
  const int32_t s0 = (int32_t)blockIdx.y * TT;
  for (int r = ty; r < TT; r += 256 / TT) {
    const int64_t t = t0 + r;
    const int32_t s = s0 + tx;
    tile[r][tx]     = t < n && s < S ? X[t * ld + s] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < TT; r += 256 / TT) {
    const int32_t s = s0 + r;
    const int64_t t = t0 + tx;
    if (s < S && t < n) Z[(int64_t)s * n + t] = tile[tx][r];
  }
}

__global__ __launch_bounds__(LB) void iact_scan_kernel(int64_t n, int32_t S, double *__restrict__ Z, int32_t max_lag, int32_t nacf, double *__restrict__ acf, double *__restrict__ tau, int32_t *__restrict__ window, int32_t *__restrict__ valid)
{
  __shared__ double za[TILE];      // z[t0 + i]
  __shared__ double zb[TILE + LB]; // z[t0 + kb + i]
  __shared__ double red[LB];
  __shared__ int    go_on;
  const int     j = threadIdx.x;
  const int32_t s = (int32_t)blockIdx.x;
  double       *z = Z + (int64_t)s * n;

  // phase A: the mean in its fixed order, the series centred in place (every lane rewrites the entries it summed)
  double acc = 0.0;
  for (int64_t t = j; t < n; t += LB) acc = acc + z[t];
  red[j] = acc;
  __syncthreads();
  for (int o = LB / 2; o >= 1; o >>= 1) {
    if (j < o) red[j] = red[j] + red[j + o];
    __syncthreads();
  }
  const double m = red[0] / (double)n;
  for (int64_t t = j; t < n; t += LB) z[t] = z[t] - m;
  __threadfence_block();
  __syncthreads();

  // phase B
  const bool    limited = max_lag > 0 && (int64_t)max_lag < n - 1;
  const int64_t klim    = limited ? (int64_t)max_lag : n - 1; // the last lag the window rule is tested at
  const int64_t kacf    = acf ? (int64_t)nacf - 1 : -1;       // the last lag whose rho is written
  double        c0 = 0.0, P = 0.0, T0 = 0.0, Tlim = 0.0, tau_w = 0.0; // P .. tau_w: lane 0 only
  int64_t       w     = 0;
  bool          found = false;
  for (int64_t kb = 0;; kb += LB) {
    const int64_t k  = kb + j;
    const int64_t nt = n - kb; // terms of the block's first lag: the longest sum of the block
    double        a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int64_t t0 = 0; t0 < nt; t0 += TILE) {
      __syncthreads(); // the tile before this one has been consumed
      for (int i = j; i < TILE; i += LB) {
        const int64_t t = t0 + i;
        za[i]           = t < n ? z[t] : 0.0;
      }
      for (int i = j; i < TILE + LB; i += LB) {
        const int64_t u = t0 + kb + i;
        zb[i]           = u < n ? z[u] : 0.0;
      }
      __syncthreads();
      const int64_t left = nt - t0;
      const int     len  = left < TILE ? (int)((left + 3) & ~(int64_t)3) : TILE; // zb is zero from `left` on
      for (int i = 0; i < len; i += 4) {
        a0 = fma(za[i], zb[i + j], a0);
        a1 = fma(za[i + 1], zb[i + 1 + j], a1);
        a2 = fma(za[i + 2], zb[i + 2 + j], a2);
        a3 = fma(za[i + 3], zb[i + 3 + j], a3);
      }
    }
    const double c = (a0 + a1) + (a2 + a3);
    red[j]         = c;
    __syncthreads();
    if (kb == 0) {
      c0 = red[0];
      if (!(c0 != 0.0) || !isfinite(c0)) { // what the host gives for 0 / 0 (uniform over the workgroup)
        if (acf)
          for (int64_t q = j; q < nacf; q += LB) acf[q * S + s] = NAN;
        if (j == 0) tau[s] = NAN, window[s] = (int32_t)(n - 1), valid[s] = 0;
        return;
      }
    }
    __syncthreads(); // red[0] has been read by every lane
    const double rho = c / c0;
    if (k <= kacf) acf[k * S + s] = rho;
    red[j] = rho;
    __syncthreads();
    if (j == 0) {
      if (!found)
        for (int q = 0; q < LB && kb + q <= klim; ++q) {
          const int64_t kk = kb + q;
          P                = P + red[q];
          const double T   = 2 * P - 1;
          if (kk == 0) T0 = T;
          if (kk == klim) Tlim = T;
          if ((double)kk >= 5 * T) {
            found = true, w = kk, tau_w = T;
            break;
          }
        }
      const int64_t next = kb + LB;
      go_on              = next <= n - 1 && ((!found && next <= klim) || next <= kacf);
    }
    __syncthreads();
    if (!go_on) break;
  }
  if (j == 0) {
    if (found) tau[s] = tau_w, window[s] = (int32_t)w, valid[s] = 500 * tau_w <= (double)n;
    else if (limited) tau[s] = Tlim, window[s] = -1, valid[s] = 0;
    else tau[s] = T0, window[s] = 0, valid[s] = 500 * T0 <= (double)n; // no lag qualifies: the host's window 0
  }
}

} // namespace

/* Z[s * n + t] = X[t * ld + s]; Z holds n * nseries doubles */
extern "C" int pmgk_iact_transpose(int64_t n, int32_t nseries, const double *X, int64_t ld, double *Z, void *stream)
{
  if (n <= 0 || nseries <= 0) return 0;
  const int64_t bt = (n + TT - 1) / TT, bs = ((int64_t)nseries + TT - 1) / TT;
  if (bt > 0x7fffffff || bs > 65535) return 1;
  hipLaunchKernelGGL(iact_transpose_kernel, dim3((unsigned)bt, (unsigned)bs), dim3(256), 0, (hipStream_t)stream, n, nseries, X, ld, Z);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

/* centres every series of Z in place, then tau / window / valid (nseries each) and, with acf != NULL, acf[k * nseries + s], k < nacf */
extern "C" int pmgk_iact_scan(int64_t n, int32_t nseries, double *Z, int32_t max_lag, int32_t nacf, double *acf, double *tau, int32_t *window, int32_t *valid, void *stream)
{
  if (n <= 0 || nseries <= 0) return 0;
  if (n > 0x7fffffff || max_lag < 0 || (acf && (nacf < 0 || nacf > n))) return 1;
  hipLaunchKernelGGL(iact_scan_kernel, dim3((unsigned)nseries), dim3(LB), 0, (hipStream_t)stream, n, nseries, Z, max_lag, nacf, acf, tau, window, valid);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
