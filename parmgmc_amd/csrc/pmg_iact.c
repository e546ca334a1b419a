/* Integrated autocorrelation time of every chain on the device: the third consumer of pmg_*_sample_chains (C11 host side).
 *
 * Replaces, for traces that live on the device, the loop "pmg_iact per chain on a downloaded trace": IACT of the reference
 * (src/iact.c:73-92; examples/ex2.c:107; the benchmark's "Measure IACT" loop) with AutoWindow(c = 5) (:49-71) on the
 * autocorrelation of :17-47, which is formed directly instead of through an FFT and only as far as the window needs it.
 * All argument checks run before any device work.  The scratch -- the series transposed and centred (n x nseries doubles) and
 * the per-series results -- lives for one call: allocated once the checks have passed, freed on every path out.  The
 * arithmetic and its order are stated in kernels_iact.hip.
 */
#include "pmg_internal.h"

_Static_assert(PMG_IACT_LAG_BLOCK == PMGK_IACT_LAG_BLOCK, "the public constant is the kernel's");

static pmg_status iact_check(int64_t n, int32_t nseries, const double *X_dev, int64_t ld, int32_t max_lag, const double *tau_host, int32_t nacf, const double *acf_dev)
{
  PMG_CHECK(X_dev, PMG_ERR_ARG_NULL, "null series array");
  PMG_CHECK(tau_host, PMG_ERR_ARG_NULL, "null output array");
  PMG_CHECK(n >= 2, PMG_ERR_ARG_OUTOFRANGE, "Too few data points"); /* src/iact.c:79 */
  PMG_CHECK(n <= INT32_MAX, PMG_ERR_ARG_OUTOFRANGE, "n = %lld: the window is a 32-bit lag", (long long)n);
  PMG_CHECK(nseries >= 1, PMG_ERR_ARG_OUTOFRANGE, "nseries = %d", nseries);
  PMG_CHECK(nseries <= 32 * 65535, PMG_ERR_ARG_OUTOFRANGE, "nseries = %d exceeds %d", nseries, 32 * 65535);
  PMG_CHECK(n <= ((int64_t)1 << 34) / nseries, PMG_ERR_ARG_OUTOFRANGE, "a scratch of %lld x %d doubles exceeds 128 GiB", (long long)n, nseries);
  PMG_CHECK(ld >= nseries, PMG_ERR_ARG_OUTOFRANGE, "leading dimension %lld below the %d series", (long long)ld, nseries);
  PMG_CHECK(max_lag >= 0, PMG_ERR_ARG_OUTOFRANGE, "max_lag = %d", max_lag);
  PMG_CHECK(!acf_dev || (nacf >= 0 && nacf <= n), PMG_ERR_ARG_OUTOFRANGE, "nacf = %d outside [0, %lld]", nacf, (long long)n);
  return PMG_SUCCESS;
}

static pmg_status iact_run(int64_t n, int32_t S, const double *X_dev, int64_t ld, int32_t max_lag, double *tau_host, int32_t *window_host, int32_t *valid_host, int32_t nacf, double *acf_dev, void *stream)
{
  if (!acf_dev || nacf == 0) acf_dev = NULL, nacf = 0;
  const size_t off_w = sizeof(double) * (size_t)S, off_v = off_w + sizeof(int32_t) * (size_t)S, rbytes = off_v + sizeof(int32_t) * (size_t)S;
  double      *Z = NULL;
  char        *res = NULL, *host = (char *)malloc(rbytes);
  pmg_status   st = host ? PMG_SUCCESS : pmg_set_error(PMG_ERR_MEM, __FILE__, __LINE__, "out of host memory");
  if (!st) st = pmg_dev_alloc((void **)&Z, sizeof(double) * (size_t)n * (size_t)S);
  if (!st) st = pmg_dev_alloc((void **)&res, rbytes);
  if (!st && pmgk_iact_transpose(n, S, X_dev, ld, Z, stream)) st = pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "kernel launch failed: pmgk_iact_transpose");
  if (!st && pmgk_iact_scan(n, S, Z, max_lag, nacf, acf_dev, (double *)res, (int32_t *)(res + off_w), (int32_t *)(res + off_v), stream)) st = pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "kernel launch failed: pmgk_iact_scan");
  if (!st) {
    hipError_t e = hipMemcpyAsync(host, res, rbytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) st = pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "copying the results: %s", hipGetErrorString(e));
  } else if (Z) (void)hipStreamSynchronize((hipStream_t)stream); /* a launched kernel may still use the scratch */
  if (!st) {
    memcpy(tau_host, host, off_w);
    if (window_host) memcpy(window_host, host + off_w, sizeof(int32_t) * (size_t)S);
    if (valid_host) memcpy(valid_host, host + off_v, sizeof(int32_t) * (size_t)S);
  }
  pmg_dev_free(res);
  pmg_dev_free(Z);
  free(host);
  return st;
}

pmg_status pmg_iact_chains(int64_t n, int32_t nseries, const double *X_dev, int64_t ld, int32_t max_lag, double *tau_host, int32_t *window_host, int32_t *valid_host, int32_t nacf, double *acf_dev, void *stream)
{
  PMG_CALL(iact_check(n, nseries, X_dev, ld, max_lag, tau_host, nacf, acf_dev));
  return iact_run(n, nseries, X_dev, ld, max_lag, tau_host, window_host, valid_host, nacf, acf_dev, stream);
}

pmg_status pmg_chainstats_iact(pmg_chainstats cs, int32_t q, int32_t first, int32_t count, int32_t max_lag, double *tau_host, int32_t *window_host, int32_t *valid_host, int32_t nacf, double *acf_dev, void *stream)
{
  PMG_CHECK(cs, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(tau_host, PMG_ERR_ARG_NULL, "null output array");
  const double *X = NULL;
  int32_t       C = 0;
  PMG_CALL(pmg_chainstats_trace_window(cs, q, first, count, &X, &C)); /* q and the window against what has been recorded */
  PMG_CHECK(count >= 2, PMG_ERR_ARG_OUTOFRANGE, "Too few data points"); /* src/iact.c:79 */
  PMG_CALL(iact_check(count, C, X, C, max_lag, tau_host, nacf, acf_dev));
  PMG_HIP(hipDeviceSynchronize()); /* updates may have been enqueued on any stream */
  return iact_run(count, C, X, C, max_lag, tau_host, window_host, valid_host, nacf, acf_dev, stream);
}
