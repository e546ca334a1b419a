/* Rao-Blackwellised running statistics of the chains on the device (C11 host side): the marginal mean and variance of every
 * unknown of x ~ N(Q^-1 b, Q^-1) from the conditional means m_i = (b_i - sum_{j != i} Q_ij y_j) / Q_ii of the samples instead of
 * the samples themselves -- what MS_ComputeMeanAndVar (src/ms.c:221-251) and the benchmark's Welford loop
 * (examples/benchmark/main.cc:151-175) report, with the exact part 1 / Q_ii of the variance taken out of the Monte Carlo sum.
 * The handle owns a copy of the matrix in natural numbering (the off-diagonal entries of every row in stored order, the
 * diagonal apart), the low-rank factors, and mean and M2 (n doubles each) on the device.  Creation and every argument check run
 * without a device; device memory, the matrix upload included, is allocated by the first update or cond_mean.  The arithmetic
 * and its order are stated in kernels_rbstats.hip.
 * A DMDA handle (pmg_rbstats_create_dmda) holds no matrix: the operator of pmg_grid_create is (nx, ny, nz, kappa), its diagonal
 * comes from rb_diag and the launches go to kernels_rbstats_dmda.hip, which gives the bits of the CSR kernel on the assembled
 * operator.  Everything that does not touch the matrix is one copy for both kinds.
 */
#include <math.h>
#include "pmg_internal.h"

/* Weak references: this file is also linked, without the kernels, into host-only programs that bring launchers of their own for
   the CSR kernels only (tests/sanitize/rbstats_san.c).  The library always holds kernels_rbstats_dmda.hip; where the two
   launchers are absent a DMDA handle's update and cond_mean fail with PMG_ERR_SUP (rb_launch), they do not fall back. */
extern int pmgk_rbstats_dmda_update(const pmgk_rbstats_dmda_op *A, int32_t nchains, double count, const double *Y, double *mean, double *M2, void *stream) __attribute__((weak));
extern int pmgk_rbstats_dmda_cond_mean(const pmgk_rbstats_dmda_op *A, int32_t nchains, const double *Y, double *M, void *stream) __attribute__((weak));

struct pmg_rbstats_s {
  int64_t n, nnz; /* nnz: stored entries of the matrix as given, the diagonal included */
  int32_t C, k, steps;
  void   *stream; /* what the callbacks launch on (they carry none) */
  /* host: off-diagonal CSR, a_ii, q_i = Q_ii, B (n x k column-major), S */
  int32_t *rowptr_h, *cols_h;
  double  *vals_h, *diag_h, *q_h, *B_h, S_h[64];
  const double *b_dev; /* borrowed; NULL: zero */
  /* device */
  int32_t *rowptr, *cols;
  double  *vals, *q, *B, *S, *T, *partial, *mean, *M2;
  int      allocated, lr_dirty; /* lr_dirty: q / B / S on the device are not the host's */
  /* a DMDA handle: no rowptr / cols / vals / diag_h; kk = kappa * kappa, hinv2 = 1.0 / ((nx - 1) * (nx - 1)) */
  int     dmda;
  int32_t nx, ny, nz;
  double  kk, hinv2;
};

/* a_rr: the stored diagonal entry, or that of MatAssembleShiftedLaplaceFD (kappa * kappa, then + hinv2 once per in-domain
   neighbour by repeated addition; the addends are equal, so the order of the neighbours does not matter) */
static double rb_diag(const struct pmg_rbstats_s *h, size_t r)
{
  if (!h->dmda) return h->diag_h[r];
  const size_t  P = (size_t)h->nx * (size_t)h->ny;
  const int32_t k = (int32_t)(r / P), j = (int32_t)((r % P) / (size_t)h->nx), i = (int32_t)(r % (size_t)h->nx);
  const int     cnt = (k > 0) + (j > 0) + (i > 0) + (k < h->nz - 1) + (j < h->ny - 1) + (i < h->nx - 1);
  double        d   = h->kk;
  for (int a = 0; a < cnt; ++a) d += h->hinv2;
  return d;
}

pmg_status pmg_rbstats_destroy(pmg_rbstats *rb)
{
  if (!rb || !*rb) return PMG_SUCCESS;
  pmg_rbstats h = *rb;
  free(h->rowptr_h), free(h->cols_h), free(h->vals_h), free(h->diag_h), free(h->q_h), free(h->B_h);
  pmg_dev_free(h->rowptr), pmg_dev_free(h->cols), pmg_dev_free(h->vals), pmg_dev_free(h->q), pmg_dev_free(h->B), pmg_dev_free(h->S);
  pmg_dev_free(h->T), pmg_dev_free(h->partial), pmg_dev_free(h->mean), pmg_dev_free(h->M2);
  free(h);
  *rb = NULL;
  return PMG_SUCCESS;
}

/* the checks of pmg_mcsor_setup (rowptr monotone, columns in range, a stored diagonal: same codes) and a diagonal > 0 and
   finite; fills the off-diagonal copy */
static pmg_status rb_copy_matrix(pmg_rbstats h, const int32_t *rowptr, const int32_t *colidx, const double *vals)
{
  const int32_t n = (int32_t)h->n;
  int64_t       w = 0;
  for (int32_t r = 0; r < n; ++r) {
    PMG_CHECK(rowptr[r + 1] >= rowptr[r], PMG_ERR_ARG_WRONG, "rowptr not monotone at row %d", r);
    int found     = 0;
    h->rowptr_h[r] = (int32_t)w;
    for (int32_t j = rowptr[r]; j < rowptr[r + 1]; ++j) {
      const int32_t c = colidx[j];
      PMG_CHECK(c >= 0 && c < n, PMG_ERR_ARG_OUTOFRANGE, "column %d out of range in row %d", c, r);
      if (c == r) {
        PMG_CHECK(!found, PMG_ERR_ARG_WRONG, "row %d stores its diagonal entry twice", r);
        found        = 1;
        h->diag_h[r] = vals[j];
      } else {
        h->cols_h[w] = c, h->vals_h[w] = vals[j];
        ++w;
      }
    }
    PMG_CHECK(found, PMG_ERR_ARG_WRONG, "row %d has no stored diagonal entry", r);
    PMG_CHECK(isfinite(h->diag_h[r]) && h->diag_h[r] > 0.0, PMG_ERR_ARG_WRONG, "row %d has the diagonal entry %g: a conditional precision must be positive and finite", r, h->diag_h[r]);
    h->q_h[r] = h->diag_h[r];
  }
  h->rowptr_h[n] = (int32_t)w;
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_create_csr(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, int32_t nchains, pmg_rbstats *rb)
{
  PMG_CHECK(rb, PMG_ERR_ARG_NULL, "null handle pointer");
  *rb = NULL;
  PMG_CHECK(n >= 1, PMG_ERR_ARG_OUTOFRANGE, "n = %d", n);
  PMG_CALL(pmg_chains_size_check(n, nchains));
  PMG_CHECK(rowptr && colidx && vals, PMG_ERR_ARG_NULL, "null CSR array");
  PMG_CHECK(rowptr[0] >= 0 && rowptr[n] >= rowptr[0], PMG_ERR_ARG_WRONG, "rowptr runs from %d to %d", rowptr[0], rowptr[n]);
  pmg_rbstats h = (pmg_rbstats)calloc(1, sizeof(*h));
  PMG_CHECK(h, PMG_ERR_MEM, "out of memory");
  h->n = n, h->C = nchains, h->nnz = (int64_t)rowptr[n] - rowptr[0];
  const size_t nz = (size_t)(h->nnz > 0 ? h->nnz : 1);
  h->rowptr_h     = (int32_t *)malloc(sizeof(int32_t) * ((size_t)n + 1));
  h->cols_h       = (int32_t *)malloc(sizeof(int32_t) * nz);
  h->vals_h       = (double *)malloc(sizeof(double) * nz);
  h->diag_h       = (double *)malloc(sizeof(double) * (size_t)n);
  h->q_h          = (double *)malloc(sizeof(double) * (size_t)n);
  pmg_status st   = h->rowptr_h && h->cols_h && h->vals_h && h->diag_h && h->q_h ? PMG_SUCCESS : pmg_set_error(PMG_ERR_MEM, __FILE__, __LINE__, "out of memory");
  if (!st) st = rb_copy_matrix(h, rowptr, colidx, vals);
  if (st) {
    pmg_rbstats_destroy(&h);
    return st;
  }
  *rb = h;
  return PMG_SUCCESS;
}

/* The operator of pmg_grid_create / pmg_mat_create_dmda / pmg_mgmc_create_dmda on an nx x ny x nz vertex grid (nz = 1: the
   reference's 2-D matrix), rows in DMDA natural order, matrix-free.  The size checks of pmg_mat_create_dmda, then
   nx ny nz <= INT32_MAX and nchains >= 1. */
pmg_status pmg_rbstats_create_dmda(int32_t nx, int32_t ny, int32_t nz, double kappa, int32_t nchains, pmg_rbstats *rb)
{
  PMG_CHECK(rb, PMG_ERR_ARG_NULL, "null handle pointer");
  *rb = NULL;
  PMG_CHECK(nx >= 2 && ny >= 1 && nz >= 1, PMG_ERR_ARG_OUTOFRANGE, "grid %d x %d x %d", nx, ny, nz);
  PMG_CHECK((int64_t)nx * ny <= INT32_MAX && (int64_t)nx * ny * nz <= INT32_MAX, PMG_ERR_ARG_OUTOFRANGE, "grid %d x %d x %d has more than %d points", nx, ny, nz, INT32_MAX);
  const int64_t n = (int64_t)nx * ny * nz;
  PMG_CALL(pmg_chains_size_check(n, nchains));
  PMG_CHECK(isfinite(kappa * kappa), PMG_ERR_ARG_WRONG, "kappa = %g: a conditional precision must be positive and finite", kappa);
  pmg_rbstats h = (pmg_rbstats)calloc(1, sizeof(*h));
  PMG_CHECK(h, PMG_ERR_MEM, "out of memory");
  h->dmda = 1, h->nx = nx, h->ny = ny, h->nz = nz;
  h->n = n, h->C = nchains, h->nnz = 0;
  h->kk    = kappa * kappa;
  h->hinv2 = 1.0 / (double)((int64_t)(nx - 1) * (nx - 1)); /* the integer product first (src/problems.c:24) */
  h->q_h   = (double *)malloc(sizeof(double) * (size_t)n);
  if (!h->q_h) {
    pmg_rbstats_destroy(&h);
    return pmg_set_error(PMG_ERR_MEM, __FILE__, __LINE__, "out of memory");
  }
  for (size_t r = 0; r < (size_t)n; ++r) h->q_h[r] = rb_diag(h, r);
  *rb = h;
  return PMG_SUCCESS;
}

/* Q = A + B S B^T: B n x k column-major in the matrix's row numbering, S the k diagonal entries (as pmg_mcsor_set_lowrank);
   q_i = a_ii + sum_k S_k * (B_ik * B_ik), k ascending.  k = 0 removes the term. */
pmg_status pmg_rbstats_set_lowrank(pmg_rbstats h, int32_t k, const double *B_host, const double *S_host)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(k >= 0 && k <= 64, PMG_ERR_ARG_OUTOFRANGE, "rank k = %d (0..64 supported)", k);
  PMG_CHECK(k == 0 || (B_host && S_host), PMG_ERR_ARG_NULL, "null low-rank factor");
  const size_t n = (size_t)h->n;
  for (size_t r = 0; r < n; ++r) { /* before anything changes */
    double q = rb_diag(h, r);
    for (int32_t j = 0; j < k; ++j) q = q + S_host[j] * (B_host[r + n * (size_t)j] * B_host[r + n * (size_t)j]);
    PMG_CHECK(isfinite(q) && q > 0.0, PMG_ERR_ARG_WRONG, "row %zu has the conditional precision %g with the low-rank term: it must be positive and finite", r, q);
  }
  if (h->allocated) PMG_HIP(hipDeviceSynchronize()); /* as pmg_rbstats_reset: the moments of another Q are forgotten */
  h->steps  = 0;
  double *B = NULL;
  if (k > 0) {
    B = (double *)malloc(sizeof(double) * n * (size_t)k);
    PMG_CHECK(B, PMG_ERR_MEM, "out of memory");
    memcpy(B, B_host, sizeof(double) * n * (size_t)k);
    memcpy(h->S_h, S_host, sizeof(double) * (size_t)k);
  }
  free(h->B_h);
  h->B_h = B, h->k = k;
  for (size_t r = 0; r < n; ++r) {
    double q = rb_diag(h, r);
    for (int32_t j = 0; j < k; ++j) q = q + h->S_h[j] * (B[r + n * (size_t)j] * B[r + n * (size_t)j]);
    h->q_h[r] = q;
  }
  h->lr_dirty = 1; /* uploaded by the next update or cond_mean */
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_set_rhs(pmg_rbstats h, const double *b_dev)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  h->b_dev = b_dev;
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_set_stream(pmg_rbstats h, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  h->stream = stream;
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_reset(pmg_rbstats h)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  if (h->allocated) PMG_HIP(hipDeviceSynchronize()); /* updates in flight on any stream still write the fields */
  h->steps = 0; /* the first update of a fresh count starts from (0, 0, 0) without reading the fields */
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_get_count(pmg_rbstats h, int32_t *steps, int64_t *samples)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  if (steps) *steps = h->steps;
  if (samples) *samples = (int64_t)h->steps * h->C;
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_get_cond_precision(pmg_rbstats h, double *q_host)
{
  PMG_CHECK(h && q_host, PMG_ERR_ARG_NULL, "null argument");
  memcpy(q_host, h->q_h, sizeof(double) * (size_t)h->n);
  return PMG_SUCCESS;
}

/* the matrix (12 bytes per stored entry), Y once (neighbour gathers counted as cache hits), b, q, and mean / M2 read and
   written; with a low-rank term B, and Y once more for B^T Y.  A DMDA handle reads no matrix, b only where one is set and q
   only with a low-rank term (kernels_rbstats_dmda.hip forms it in registers otherwise). */
pmg_status pmg_rbstats_get_algorithmic_bytes(pmg_rbstats h, double *bytes)
{
  PMG_CHECK(h && bytes, PMG_ERR_ARG_NULL, "null argument");
  if (h->dmda) {
    *bytes = 8.0 * (double)h->n * h->C + 32.0 * (double)h->n + (h->b_dev ? 8.0 * (double)h->n : 0.0);
    if (h->k > 0) *bytes += 8.0 * (double)h->n + 8.0 * (double)h->n * h->k + 8.0 * (double)h->n * h->C;
    return PMG_SUCCESS;
  }
  *bytes = 12.0 * (double)h->nnz + 8.0 * (double)h->n * h->C + 48.0 * (double)h->n;
  if (h->k > 0) *bytes += 8.0 * (double)h->n * h->k + 8.0 * (double)h->n * h->C;
  return PMG_SUCCESS;
}

static pmg_status rb_prepare(pmg_rbstats h, void *stream)
{
  const size_t n = (size_t)h->n;
  if (!h->allocated) {
    if (!h->dmda) {
      PMG_CALL(pmg_dev_upload((void **)&h->rowptr, h->rowptr_h, sizeof(int32_t) * (n + 1)));
      const size_t nz = (size_t)h->rowptr_h[n];
      if (nz) {
        PMG_CALL(pmg_dev_upload((void **)&h->cols, h->cols_h, sizeof(int32_t) * nz));
        PMG_CALL(pmg_dev_upload((void **)&h->vals, h->vals_h, sizeof(double) * nz));
      }
    }
    PMG_CALL(pmg_dev_alloc((void **)&h->q, sizeof(double) * n));
    PMG_CALL(pmg_dev_alloc((void **)&h->mean, sizeof(double) * n));
    PMG_CALL(pmg_dev_alloc((void **)&h->M2, sizeof(double) * n));
    h->allocated = h->lr_dirty = 1;
  }
  if (h->lr_dirty) {
    PMG_HIP(hipStreamSynchronize((hipStream_t)stream)); /* a launch that reads the old factors may be in flight */
    if (h->stream != stream) PMG_HIP(hipStreamSynchronize((hipStream_t)h->stream));
    pmg_dev_free(h->B), pmg_dev_free(h->S), pmg_dev_free(h->T), pmg_dev_free(h->partial);
    h->B = h->S = h->T = h->partial = NULL;
    PMG_HIP(hipMemcpy(h->q, h->q_h, sizeof(double) * n, hipMemcpyHostToDevice));
    if (h->k > 0) {
      const size_t kc = (size_t)h->k * (size_t)h->C;
      PMG_CALL(pmg_dev_upload((void **)&h->B, h->B_h, sizeof(double) * n * (size_t)h->k));
      PMG_CALL(pmg_dev_upload((void **)&h->S, h->S_h, sizeof(double) * (size_t)h->k));
      PMG_CALL(pmg_dev_alloc((void **)&h->T, sizeof(double) * kc));
      PMG_CALL(pmg_dev_alloc((void **)&h->partial, sizeof(double) * kc * (size_t)pmgk_lrc_btx_chains_nblocks(h->n, 0)));
    }
    h->lr_dirty = 0;
  }
  return PMG_SUCCESS;
}

/* the fused launch of one step on a prepared handle: M_dev = NULL merges the moments of the conditional means, otherwise they
   are stored there */
static pmg_status rb_launch(pmg_rbstats h, const double *Y_dev, double *M_dev, void *stream)
{
  const double count = (double)h->steps * (double)h->C;
  if (h->dmda) {
    PMG_CHECK(pmgk_rbstats_dmda_update && pmgk_rbstats_dmda_cond_mean, PMG_ERR_SUP, "this program was linked without kernels_rbstats_dmda.hip");
    const pmgk_rbstats_dmda_op A = {h->nx, h->ny, h->nz, h->kk, h->hinv2, h->q, h->b_dev, h->k, h->B, h->S, h->T};
    if (M_dev) PMG_KERNEL(pmgk_rbstats_dmda_cond_mean(&A, h->C, Y_dev, M_dev, stream));
    else PMG_KERNEL(pmgk_rbstats_dmda_update(&A, h->C, count, Y_dev, h->mean, h->M2, stream));
    return PMG_SUCCESS;
  }
  const pmgk_rbstats_op A = {h->n, h->rowptr, h->cols, h->vals, h->q, h->b_dev, h->k, h->B, h->S, h->T};
  if (M_dev) PMG_KERNEL(pmgk_rbstats_cond_mean(&A, h->C, Y_dev, M_dev, stream));
  else PMG_KERNEL(pmgk_rbstats_update(&A, h->C, count, Y_dev, h->mean, h->M2, stream));
  return PMG_SUCCESS;
}

/* T = B^T Y per chain, the summation order of pmgk_lrc_btx_chains */
static pmg_status rb_bty(pmg_rbstats h, const double *Y_dev, void *stream)
{
  if (h->k > 0) PMG_KERNEL(pmgk_lrc_btx_chains(h->n, NULL, h->k, h->B, h->n, Y_dev, h->C, h->partial, NULL, h->T, stream));
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_update(pmg_rbstats h, const double *Y_dev, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(Y_dev, PMG_ERR_ARG_NULL, "null sample array");
  PMG_CHECK(h->steps < INT32_MAX, PMG_ERR_ARG_OUTOFRANGE, "the step count is full");
  PMG_CALL(rb_prepare(h, stream));
  PMG_CALL(rb_bty(h, Y_dev, stream));
  PMG_CALL(rb_launch(h, Y_dev, NULL, stream));
  h->steps++;
  return PMG_SUCCESS;
}

pmg_status pmg_rbstats_cond_mean(pmg_rbstats h, const double *Y_dev, double *M_dev, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(Y_dev && M_dev, PMG_ERR_ARG_NULL, "null sample or output array");
  PMG_CHECK(Y_dev != M_dev, PMG_ERR_ARG_WRONG, "the conditional means cannot overwrite the samples they are gathered from");
  PMG_CALL(rb_prepare(h, stream));
  PMG_CALL(rb_bty(h, Y_dev, stream));
  PMG_CALL(rb_launch(h, Y_dev, M_dev, stream));
  return PMG_SUCCESS;
}

int pmg_rbstats_callback(int32_t it, const double *Y_nat_dev, int32_t n, int32_t nchains, void *ctx)
{
  (void)it;
  pmg_rbstats h = (pmg_rbstats)ctx;
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle as callback context");
  PMG_CHECK(n == h->n && nchains == h->C, PMG_ERR_ARG_SIZ, "samples of %d rows x %d chains for a handle of %lld x %d", n, nchains, (long long)h->n, h->C);
  return pmg_rbstats_update(h, Y_nat_dev, h->stream);
}

int pmg_rbstats_sample_callback(int32_t it, const double *y_nat_dev, int32_t n, void *ctx) { return pmg_rbstats_callback(it, y_nat_dev, n, 1, ctx); }

pmg_status pmg_rbstats_get_fields(pmg_rbstats h, double *mean_dev, double *var_dev, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK((int64_t)h->steps * h->C >= 2, PMG_ERR_ARG_WRONGSTATE, "Need at least 2 samples for variance computation"); /* src/ms.c:233 */
  PMG_CHECK(mean_dev || var_dev, PMG_ERR_ARG_NULL, "null output fields");
  PMG_KERNEL(pmgk_rbstats_fields(h->n, (double)h->steps * (double)h->C, h->q, h->mean, h->M2, mean_dev, var_dev, stream));
  return PMG_SUCCESS;
}
