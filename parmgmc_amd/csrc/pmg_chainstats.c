/* Running statistics of the chains on the device: the consumer of pmg_*_sample_chains (C11 host side).
 *
 * Replaces what the reference's drivers do with their chains on the host:
 *   - MS_ComputeMeanAndVar (src/ms.c:221-251) and the benchmark's Welford loop (examples/benchmark/main.cc:151-175): mean and
 *     unbiased variance of every row over all samples -- here over steps x chains samples, merged step by step on the device;
 *   - the sample callback of examples/ex7.c:40-52 (VecSum / VecDot per sample) and GelmanRubin (ex7.c:61-93).
 * The handle owns mean and M2 (n doubles each), the QOI weights, the block scratch of the update and the trace
 * nqoi x max_steps x nchains, all on the device and allocated at the first call that needs them: creation and every argument
 * check run without a device.  The arithmetic and its order are stated in kernels_chainstats.hip.
 */
#include "pmg_internal.h"

#define CS_MAXQ PMGK_CHAINSTATS_MAX_QOI
_Static_assert(PMG_CHAINSTATS_MAX_QOI == PMGK_CHAINSTATS_MAX_QOI, "the public cap is the kernel's");

struct pmg_chainstats_s {
  int64_t n;
  int32_t C, nq, max_steps, steps;
  void   *stream;          /* what the callbacks launch on (they carry none) */
  double *w_host[CS_MAXQ]; /* NULL: all ones */
  int     w_dirty[CS_MAXQ];
  double *w_dev[CS_MAXQ];
  double *mean, *M2, *partial, *trace;
  int     allocated;
};

pmg_status pmg_chainstats_create(int32_t n, int32_t nchains, int32_t nqoi, int32_t max_steps, pmg_chainstats *cs)
{
  PMG_CHECK(cs, PMG_ERR_ARG_NULL, "null handle pointer");
  *cs = NULL;
  PMG_CHECK(n >= 1, PMG_ERR_ARG_OUTOFRANGE, "n = %d", n);
  PMG_CALL(pmg_chains_size_check(n, nchains));
  PMG_CHECK(nqoi >= 0 && nqoi <= CS_MAXQ, PMG_ERR_ARG_OUTOFRANGE, "nqoi = %d outside [0, %d]", nqoi, CS_MAXQ);
  PMG_CHECK(max_steps >= 1, PMG_ERR_ARG_OUTOFRANGE, "max_steps = %d", max_steps);
  PMG_CHECK(nqoi == 0 || (int64_t)max_steps <= ((int64_t)1 << 34) / ((int64_t)nqoi * nchains), PMG_ERR_ARG_OUTOFRANGE, "a trace of %d x %d x %d doubles exceeds 128 GiB", nqoi, max_steps, nchains);
  pmg_chainstats h = (pmg_chainstats)calloc(1, sizeof(*h));
  PMG_CHECK(h, PMG_ERR_MEM, "out of memory");
  h->n = n, h->C = nchains, h->nq = nqoi, h->max_steps = max_steps;
  *cs = h;
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_destroy(pmg_chainstats *cs)
{
  if (!cs || !*cs) return PMG_SUCCESS;
  pmg_chainstats h = *cs;
  for (int q = 0; q < CS_MAXQ; ++q) {
    free(h->w_host[q]);
    pmg_dev_free(h->w_dev[q]);
  }
  pmg_dev_free(h->mean), pmg_dev_free(h->M2), pmg_dev_free(h->partial), pmg_dev_free(h->trace);
  free(h);
  *cs = NULL;
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_set_qoi(pmg_chainstats h, int32_t q, const double *w_host)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(q >= 0 && q < h->nq, PMG_ERR_ARG_OUTOFRANGE, "QOI %d outside [0, %d)", q, h->nq);
  if (!w_host) {
    free(h->w_host[q]);
    h->w_host[q] = NULL;
  } else {
    if (!h->w_host[q]) h->w_host[q] = (double *)malloc(sizeof(double) * (size_t)h->n);
    PMG_CHECK(h->w_host[q], PMG_ERR_MEM, "out of memory");
    memcpy(h->w_host[q], w_host, sizeof(double) * (size_t)h->n);
  }
  h->w_dirty[q] = 1; /* uploaded by the next update */
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_set_stream(pmg_chainstats h, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  h->stream = stream;
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_reset(pmg_chainstats h)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  if (h->allocated) PMG_HIP(hipDeviceSynchronize()); /* updates in flight on any stream still write the fields */
  h->steps = 0; /* the first update of a fresh count starts from (0, 0, 0) without reading the fields */
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_get_count(pmg_chainstats h, int32_t *steps, int64_t *samples)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  if (steps) *steps = h->steps;
  if (samples) *samples = (int64_t)h->steps * h->C;
  return PMG_SUCCESS;
}

static pmg_status cs_prepare(pmg_chainstats h, void *stream)
{
  if (!h->allocated) {
    int32_t iters, nb;
    pmgk_chainstats_geometry(h->n, h->C, &iters, &nb);
    PMG_CALL(pmg_dev_alloc((void **)&h->mean, sizeof(double) * (size_t)h->n));
    PMG_CALL(pmg_dev_alloc((void **)&h->M2, sizeof(double) * (size_t)h->n));
    PMG_CALL(pmg_dev_alloc((void **)&h->partial, sizeof(double) * (size_t)nb * (size_t)h->nq * (size_t)h->C));
    PMG_CALL(pmg_dev_alloc((void **)&h->trace, sizeof(double) * (size_t)h->nq * (size_t)h->max_steps * (size_t)h->C));
    h->allocated = 1;
  }
  for (int q = 0; q < h->nq; ++q)
    if (h->w_dirty[q]) {
      PMG_HIP(hipStreamSynchronize((hipStream_t)stream)); /* an update that reads the old weights may be in flight */
      if (h->stream != stream) PMG_HIP(hipStreamSynchronize((hipStream_t)h->stream));
      if (!h->w_host[q]) {
        pmg_dev_free(h->w_dev[q]);
        h->w_dev[q] = NULL;
      } else {
        if (!h->w_dev[q]) PMG_CALL(pmg_dev_alloc((void **)&h->w_dev[q], sizeof(double) * (size_t)h->n));
        PMG_HIP(hipMemcpy(h->w_dev[q], h->w_host[q], sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice));
      }
      h->w_dirty[q] = 0;
    }
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_update(pmg_chainstats h, const double *Y_dev, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(Y_dev, PMG_ERR_ARG_NULL, "null sample array");
  PMG_CHECK(h->steps < h->max_steps, PMG_ERR_ARG_OUTOFRANGE, "the handle was created for %d steps", h->max_steps);
  PMG_CALL(cs_prepare(h, stream));
  pmgk_chainstats_qoi Q;
  for (int q = 0; q < CS_MAXQ; ++q) Q.w[q] = q < h->nq ? h->w_dev[q] : NULL;
  const int64_t qstride = (int64_t)h->max_steps * h->C;
  PMG_KERNEL(pmgk_chainstats_update(h->n, h->C, h->nq, &Q, (double)h->steps * (double)h->C, Y_dev, h->mean, h->M2, h->partial, h->trace + (int64_t)h->steps * h->C, qstride, stream));
  h->steps++;
  return PMG_SUCCESS;
}

int pmg_chainstats_callback(int32_t it, const double *Y_nat_dev, int32_t n, int32_t nchains, void *ctx)
{
  (void)it;
  pmg_chainstats h = (pmg_chainstats)ctx;
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle as callback context");
  PMG_CHECK(n == h->n && nchains == h->C, PMG_ERR_ARG_SIZ, "samples of %d rows x %d chains for a handle of %lld x %d", n, nchains, (long long)h->n, h->C);
  return pmg_chainstats_update(h, Y_nat_dev, h->stream);
}

int pmg_chainstats_sample_callback(int32_t it, const double *y_nat_dev, int32_t n, void *ctx) { return pmg_chainstats_callback(it, y_nat_dev, n, 1, ctx); }

pmg_status pmg_chainstats_get_fields(pmg_chainstats h, double *mean_dev, double *var_dev, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK((int64_t)h->steps * h->C >= 2, PMG_ERR_ARG_WRONGSTATE, "Need at least 2 samples for variance computation"); /* src/ms.c:233 */
  PMG_CHECK(mean_dev || var_dev, PMG_ERR_ARG_NULL, "null output fields");
  PMG_KERNEL(pmgk_chainstats_fields(h->n, (double)h->steps * (double)h->C, h->mean, h->M2, mean_dev, var_dev, stream));
  return PMG_SUCCESS;
}

static pmg_status cs_window(pmg_chainstats h, int32_t q, int32_t first, int32_t count)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(q >= 0 && q < h->nq, PMG_ERR_ARG_OUTOFRANGE, "QOI %d outside [0, %d)", q, h->nq);
  PMG_CHECK(first >= 0 && count >= 0 && first <= h->steps && count <= h->steps - first, PMG_ERR_ARG_OUTOFRANGE, "steps [%d, %d + %d) outside the %d recorded", first, first, count, h->steps);
  return PMG_SUCCESS;
}

/* the recorded steps [first, first + count) of QOI q where they lie: count x nchains device doubles, chain fastest (borrowed;
   NULL while nothing has been recorded).  For pmg_chainstats_iact (pmg_iact.c). */
pmg_status pmg_chainstats_trace_window(pmg_chainstats h, int32_t q, int32_t first, int32_t count, const double **X_dev, int32_t *nchains)
{
  PMG_CALL(cs_window(h, q, first, count));
  *X_dev   = h->trace ? h->trace + ((int64_t)q * h->max_steps + first) * h->C : NULL;
  *nchains = h->C;
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_get_trace(pmg_chainstats h, int32_t q, int32_t first, int32_t count, double *vals_host)
{
  PMG_CALL(cs_window(h, q, first, count));
  PMG_CHECK(vals_host || count == 0, PMG_ERR_ARG_NULL, "null output array");
  if (count == 0) return PMG_SUCCESS;
  PMG_HIP(hipStreamSynchronize((hipStream_t)h->stream));
  PMG_HIP(hipDeviceSynchronize()); /* updates may have been enqueued on any stream */
  PMG_HIP(hipMemcpy(vals_host, h->trace + ((int64_t)q * h->max_steps + first) * h->C, sizeof(double) * (size_t)count * (size_t)h->C, hipMemcpyDeviceToHost));
  return PMG_SUCCESS;
}

/* GelmanRubin (examples/ex7.c:61-93) term by term in its order; vals[i * n + j] = value j of chain i */
pmg_status pmg_gelman_rubin(int32_t chains, int64_t n, const double *vals_host, double *gr)
{
  PMG_CHECK(chains >= 2, PMG_ERR_ARG_OUTOFRANGE, "%d chains: the between-chain variance needs two", chains);
  PMG_CHECK(n >= 2, PMG_ERR_ARG_OUTOFRANGE, "%lld values per chain: the within-chain variance needs two", (long long)n);
  PMG_CHECK(vals_host && gr, PMG_ERR_ARG_NULL, "null argument");
  double *means = (double *)calloc(2 * (size_t)chains, sizeof(double));
  PMG_CHECK(means, PMG_ERR_MEM, "out of memory");
  double *vars = means + chains, mean = 0, B = 0, W = 0;
  for (int32_t i = 0; i < chains; ++i)
    for (int64_t j = 0; j < n; ++j) means[i] += 1. / n * vals_host[i * n + j];
  for (int32_t i = 0; i < chains; ++i) mean += 1. / chains * means[i];
  for (int32_t i = 0; i < chains; ++i) B += n / (chains - 1.) * (means[i] - mean) * (means[i] - mean);
  for (int32_t i = 0; i < chains; ++i)
    for (int64_t j = 0; j < n; ++j) vars[i] += 1. / (n - 1.) * (vals_host[i * n + j] - means[i]) * (vals_host[i * n + j] - means[i]);
  for (int32_t i = 0; i < chains; ++i) W += 1. / chains * vars[i];
  *gr = ((n - 1.) / n * W + 1. / n * B) / W;
  free(means);
  return PMG_SUCCESS;
}

pmg_status pmg_chainstats_rhat(pmg_chainstats h, int32_t q, int32_t first, int32_t count, double *gr)
{
  PMG_CALL(cs_window(h, q, first, count));
  PMG_CHECK(h->C >= 2, PMG_ERR_ARG_OUTOFRANGE, "%d chains: the between-chain variance needs two", h->C);
  PMG_CHECK(count >= 2, PMG_ERR_ARG_OUTOFRANGE, "%d steps: the within-chain variance needs two", count);
  PMG_CHECK(gr, PMG_ERR_ARG_NULL, "null argument");
  const size_t nv = (size_t)count * (size_t)h->C;
  double      *t  = (double *)malloc(2 * nv * sizeof(double));
  PMG_CHECK(t, PMG_ERR_MEM, "out of memory");
  pmg_status s = pmg_chainstats_get_trace(h, q, first, count, t);
  if (!s) {
    for (int32_t j = 0; j < count; ++j) /* step-major -> the reference's vals[chain][step] */
      for (int32_t i = 0; i < h->C; ++i) t[nv + (size_t)i * count + j] = t[(size_t)j * h->C + i];
    s = pmg_gelman_rubin(h->C, count, t + nv, gr);
  }
  free(t);
  return s;
}
