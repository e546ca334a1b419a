/* Covariance error over the chains on the device: the ex6 consumer of pmg_*_sample_chains (C11 host side).
 *
 * Replaces, for chains that live on the device, what examples/ex6.c:168-193 does with EstimateCovarianceMatErrors
 * (src/stats.c:94-117): per sample index the unbiased covariance over the chains (SampleMean :55-61, SampleCovariance :63-84,
 * 1 / (chains - 1) at :78) against a dense reference in the relative Frobenius norm (:110-112).  The reference Sigma lives on
 * the device, n x n row-major: formed from a pmg_chol handle's L^-1 as W^T W (DenseInverse, src/stats.c:8-31, without the
 * host), or copied from the host at the first update.  The handle owns Sigma, its norm, the row means, the tile scratch
 * and the error trace (max_steps doubles).  All argument checks run before any device work.  The arithmetic and its order are
 * stated in kernels_chaincov.hip.
 */
#include "pmg_internal.h"

#define CC_MAXN 4096 /* pmg_estimate_covariance_errors' limit */

struct pmg_chaincov_s {
  int32_t n, C, max_steps, steps, ntiles;
  void   *stream;     /* what the callback launches on (it carries none) */
  double *Sigma_host; /* create_dense: waits here for the first update */
  double *Sigma, *norm, *mean, *partial, *errs;
  int     allocated;
};

static pmg_status cc_check_sizes(int32_t n, int32_t nchains, int32_t max_steps)
{
  PMG_CHECK(n >= 1, PMG_ERR_ARG_OUTOFRANGE, "n = %d", n);
  PMG_CHECK(n <= CC_MAXN, PMG_ERR_SUP, "dense covariance diagnostics are meant for small problems (n = %d)", n);
  PMG_CHECK(nchains >= 2, PMG_ERR_ARG_OUTOFRANGE, "%d chains: the covariance over the chains needs two", nchains);
  PMG_CALL(pmg_chains_size_check(n, nchains));
  PMG_CHECK(max_steps >= 1, PMG_ERR_ARG_OUTOFRANGE, "max_steps = %d", max_steps);
  return PMG_SUCCESS;
}

static pmg_status cc_new(int32_t n, int32_t nchains, int32_t max_steps, pmg_chaincov *out)
{
  pmg_chaincov h = (pmg_chaincov)calloc(1, sizeof(*h));
  PMG_CHECK(h, PMG_ERR_MEM, "out of memory");
  h->n = n, h->C = nchains, h->max_steps = max_steps, h->ntiles = pmgk_chaincov_ntiles(n);
  *out = h;
  return PMG_SUCCESS;
}

/* everything on the device but Sigma's values; then ||Sigma||_F once Sigma is there */
static pmg_status cc_alloc(pmg_chaincov h)
{
  const size_t nn = (size_t)h->n * (size_t)h->n;
  PMG_CALL(pmg_dev_alloc((void **)&h->Sigma, sizeof(double) * nn));
  PMG_CALL(pmg_dev_alloc((void **)&h->norm, sizeof(double)));
  PMG_CALL(pmg_dev_alloc((void **)&h->mean, sizeof(double) * (size_t)h->n));
  PMG_CALL(pmg_dev_alloc((void **)&h->partial, sizeof(double) * (size_t)h->ntiles));
  PMG_CALL(pmg_dev_alloc((void **)&h->errs, sizeof(double) * (size_t)h->max_steps));
  return PMG_SUCCESS;
}

static pmg_status cc_norm(pmg_chaincov h, void *stream)
{
  PMG_KERNEL(pmgk_chaincov_sqnorm_tiles(h->n, h->Sigma, h->partial, stream)); /* MatNorm(Q, NORM_FROBENIUS), src/stats.c:105 */
  PMG_KERNEL(pmgk_chaincov_reduce(h->ntiles, h->partial, NULL, h->norm, stream));
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_create_chol(pmg_chol ch, int32_t nchains, int32_t max_steps, pmg_chaincov *cc)
{
  PMG_CHECK(cc, PMG_ERR_ARG_NULL, "null handle pointer");
  *cc = NULL;
  PMG_CHECK(ch, PMG_ERR_ARG_NULL, "null Cholesky handle");
  const int32_t n = pmg_chol_size(ch);
  PMG_CALL(cc_check_sizes(n, nchains, max_steps));
  pmg_chaincov h = NULL;
  PMG_CALL(cc_new(n, nchains, max_steps, &h));
  pmg_status st = cc_alloc(h);
  /* Sigma = L^-T L^-1 = W^T W: row i of (L^-1)^T holds column i of W, so Sigma is the uncentred rank-n product of its rows */
  if (!st && pmgk_chaincov_syrk_matrix(n, n, pmg_chol_inverse_factor_upper(ch), NULL, 1.0, h->Sigma, NULL)) st = pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "kernel launch failed");
  if (!st) st = cc_norm(h, NULL);
  if (!st && hipDeviceSynchronize() != hipSuccess) st = pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "forming the reference covariance failed"); /* ch may go now */
  if (st) {
    pmg_chaincov_destroy(&h);
    return st;
  }
  h->allocated = 1;
  *cc = h;
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_create_dense(int32_t n, const double *Sigma_host, int32_t nchains, int32_t max_steps, pmg_chaincov *cc)
{
  PMG_CHECK(cc, PMG_ERR_ARG_NULL, "null handle pointer");
  *cc = NULL;
  PMG_CALL(cc_check_sizes(n, nchains, max_steps));
  PMG_CHECK(Sigma_host, PMG_ERR_ARG_NULL, "null reference matrix");
  pmg_chaincov h = NULL;
  PMG_CALL(cc_new(n, nchains, max_steps, &h));
  const size_t bytes = sizeof(double) * (size_t)n * (size_t)n;
  h->Sigma_host      = (double *)malloc(bytes);
  if (!h->Sigma_host) {
    free(h);
    PMG_FAIL(PMG_ERR_MEM, "out of host memory for the %d x %d reference", n, n);
  }
  memcpy(h->Sigma_host, Sigma_host, bytes);
  *cc = h;
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_destroy(pmg_chaincov *cc)
{
  if (!cc || !*cc) return PMG_SUCCESS;
  pmg_chaincov h = *cc;
  free(h->Sigma_host);
  pmg_dev_free(h->Sigma), pmg_dev_free(h->norm), pmg_dev_free(h->mean), pmg_dev_free(h->partial), pmg_dev_free(h->errs);
  free(h);
  *cc = NULL;
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_set_stream(pmg_chaincov h, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  h->stream = stream;
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_reset(pmg_chaincov h)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  if (h->allocated) PMG_HIP(hipDeviceSynchronize()); /* updates in flight on any stream still write the trace */
  h->steps = 0;
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_get_count(pmg_chaincov h, int32_t *steps)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(steps, PMG_ERR_ARG_NULL, "null output");
  *steps = h->steps;
  return PMG_SUCCESS;
}

static pmg_status cc_prepare(pmg_chaincov h, void *stream)
{
  if (h->allocated) return PMG_SUCCESS;
  PMG_CALL(cc_alloc(h));
  PMG_HIP(hipMemcpy(h->Sigma, h->Sigma_host, sizeof(double) * (size_t)h->n * (size_t)h->n, hipMemcpyHostToDevice));
  free(h->Sigma_host);
  h->Sigma_host = NULL;
  PMG_CALL(cc_norm(h, stream));
  h->allocated = 1;
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_update(pmg_chaincov h, const double *Y_dev, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(Y_dev, PMG_ERR_ARG_NULL, "null sample array");
  PMG_CHECK(h->steps < h->max_steps, PMG_ERR_ARG_OUTOFRANGE, "the handle was created for %d steps", h->max_steps);
  PMG_CALL(cc_prepare(h, stream));
  PMG_KERNEL(pmgk_chaincov_means(h->n, h->C, Y_dev, h->mean, stream));                                                 /* SampleMean, src/stats.c:55-61 */
  PMG_KERNEL(pmgk_chaincov_syrk_error(h->n, h->C, Y_dev, h->mean, (double)(h->C - 1), h->Sigma, h->partial, stream)); /* :63-84, :110 */
  PMG_KERNEL(pmgk_chaincov_reduce(h->ntiles, h->partial, h->norm, h->errs + h->steps, stream));                        /* :111-112 */
  h->steps++;
  return PMG_SUCCESS;
}

int pmg_chaincov_callback(int32_t it, const double *Y_nat_dev, int32_t n, int32_t nchains, void *ctx)
{
  (void)it;
  pmg_chaincov h = (pmg_chaincov)ctx;
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle as callback context");
  PMG_CHECK(n == h->n && nchains == h->C, PMG_ERR_ARG_SIZ, "samples of %d rows x %d chains for a handle of %d x %d", n, nchains, h->n, h->C);
  return pmg_chaincov_update(h, Y_nat_dev, h->stream);
}

pmg_status pmg_chaincov_covariance(pmg_chaincov h, const double *Y_dev, double *C_dev, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(Y_dev && C_dev, PMG_ERR_ARG_NULL, "null array");
  PMG_CALL(cc_prepare(h, stream));
  PMG_KERNEL(pmgk_chaincov_means(h->n, h->C, Y_dev, h->mean, stream));
  PMG_KERNEL(pmgk_chaincov_syrk_matrix(h->n, h->C, Y_dev, h->mean, (double)(h->C - 1), C_dev, stream));
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_get_errors(pmg_chaincov h, int32_t first, int32_t count, double *errs_host)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(first >= 0 && count >= 0 && first <= h->steps && count <= h->steps - first, PMG_ERR_ARG_OUTOFRANGE, "steps [%d, %d + %d) outside the %d recorded", first, first, count, h->steps);
  PMG_CHECK(errs_host || count == 0, PMG_ERR_ARG_NULL, "null output array");
  if (count == 0) return PMG_SUCCESS;
  PMG_HIP(hipDeviceSynchronize()); /* updates may have been enqueued on any stream */
  PMG_HIP(hipMemcpy(errs_host, h->errs + first, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  return PMG_SUCCESS;
}

pmg_status pmg_chaincov_get_reference(pmg_chaincov h, double *Sigma_host)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(Sigma_host, PMG_ERR_ARG_NULL, "null output array");
  const size_t bytes = sizeof(double) * (size_t)h->n * (size_t)h->n;
  if (!h->allocated) memcpy(Sigma_host, h->Sigma_host, bytes); /* create_dense before the first update */
  else PMG_HIP(hipMemcpy(Sigma_host, h->Sigma, bytes, hipMemcpyDeviceToHost));
  return PMG_SUCCESS;
}
