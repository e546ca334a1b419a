/* AddressSanitizer + UndefinedBehaviorSanitizer run of the host part of the matrix-free Rao-Blackwellised statistics handle
 * (pmg_rbstats_create_dmda in csrc/pmg_rbstats.c): creation, every argument check, the formation of q with and without a
 * low-rank term, the byte model, and destruction after a failed creation.  Built and run by tests/test_rbstats_dmda_host.py
 * with gcc -fsanitize=address,undefined -ffp-contract=off together with pmg_rbstats.c and pmg_chains_common.c; nothing is
 * preloaded.  The device layer is replaced by the stubs below, which end the program when they are reached: none of the calls
 * made here may touch a device.  A finding or a failed check ends with a non-zero status. */
#include <math.h>
#include <stdarg.h>
#include "../../parmgmc_amd/csrc/pmg_internal.h"

static char g_msg[512];
pmg_status  pmg_set_error(pmg_status code, const char *file, int line, const char *fmt, ...)
{
  va_list ap;
  (void)file, (void)line;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}

#define REQUIRE(cond) \
  do { \
    if (!(cond)) { \
      fprintf(stderr, "rbstats_dmda_host.c:%d: %s failed (last message: %s)\n", __LINE__, #cond, g_msg); \
      exit(1); \
    } \
  } while (0)

#define REACHED(name) \
  do { \
    fprintf(stderr, "rbstats_dmda_host.c: the device layer was reached: %s\n", name); \
    exit(2); \
  } while (0)

/* ---- the device layer: never reached ---- */
hipError_t  hipDeviceSynchronize(void) { REACHED("hipDeviceSynchronize"); }
hipError_t  hipStreamSynchronize(hipStream_t s) { (void)s; REACHED("hipStreamSynchronize"); }
hipError_t  hipMemcpy(void *d, const void *s, size_t b, hipMemcpyKind k) { (void)d, (void)s, (void)b, (void)k; REACHED("hipMemcpy"); }
hipError_t  hipMemcpyAsync(void *d, const void *s, size_t b, hipMemcpyKind k, hipStream_t st) { (void)d, (void)s, (void)b, (void)k, (void)st; REACHED("hipMemcpyAsync"); }
const char *hipGetErrorString(hipError_t e) { (void)e; return "stub"; }
pmg_status  pmg_dev_alloc(void **p, size_t bytes) { (void)p, (void)bytes; REACHED("pmg_dev_alloc"); }
pmg_status  pmg_dev_upload(void **p, const void *host, size_t bytes) { (void)p, (void)host, (void)bytes; REACHED("pmg_dev_upload"); }
void        pmg_dev_free(void *p) { if (p) REACHED("pmg_dev_free of a device pointer"); }
pmg_status  pmg_devbuf_reserve(pmg_devbuf *b, size_t bytes, void *stream) { (void)b, (void)bytes, (void)stream; REACHED("pmg_devbuf_reserve"); }
void        pmg_devbuf_free(pmg_devbuf *b) { (void)b; REACHED("pmg_devbuf_free"); }
int         pmgk_lrc_btx_chains_nblocks(int64_t n, int compact) { (void)n, (void)compact; REACHED("pmgk_lrc_btx_chains_nblocks"); }
int pmgk_lrc_btx_chains(int64_t n, const int64_t *rows, int k, const double *M, int64_t ldm, const double *Y, int32_t nchains, double *partial, const double *scale, double *out, void *stream)
{
  (void)n, (void)rows, (void)k, (void)M, (void)ldm, (void)Y, (void)nchains, (void)partial, (void)scale, (void)out, (void)stream;
  REACHED("pmgk_lrc_btx_chains");
}
int pmgk_rbstats_update(const pmgk_rbstats_op *A, int32_t C, double count, const double *Y, double *mean, double *M2, void *stream)
{
  (void)A, (void)C, (void)count, (void)Y, (void)mean, (void)M2, (void)stream;
  REACHED("pmgk_rbstats_update");
}
int pmgk_rbstats_cond_mean(const pmgk_rbstats_op *A, int32_t C, const double *Y, double *M, void *stream)
{
  (void)A, (void)C, (void)Y, (void)M, (void)stream;
  REACHED("pmgk_rbstats_cond_mean");
}
int pmgk_rbstats_fields(int64_t n, double count, const double *q, const double *mean, const double *M2, double *mean_out, double *var_out, void *stream)
{
  (void)n, (void)count, (void)q, (void)mean, (void)M2, (void)mean_out, (void)var_out, (void)stream;
  REACHED("pmgk_rbstats_fields");
}
int pmgk_rbstats_dmda_update(const pmgk_rbstats_dmda_op *A, int32_t C, double count, const double *Y, double *mean, double *M2, void *stream)
{
  (void)A, (void)C, (void)count, (void)Y, (void)mean, (void)M2, (void)stream;
  REACHED("pmgk_rbstats_dmda_update");
}
int pmgk_rbstats_dmda_cond_mean(const pmgk_rbstats_dmda_op *A, int32_t C, const double *Y, double *M, void *stream)
{
  (void)A, (void)C, (void)Y, (void)M, (void)stream;
  REACHED("pmgk_rbstats_dmda_cond_mean");
}

/* the diagonal of MatAssembleShiftedLaplaceFD (src/problems.c:14-75) and its 3-D analogue, written out independently */
static double want_diag(int nx, int ny, int nz, double kappa, int i, int j, int k)
{
  const double hinv2 = 1. / ((nx - 1) * (nx - 1));
  double       d     = kappa * kappa;
  if (k > 0) d += hinv2;
  if (j > 0) d += hinv2;
  if (i > 0) d += hinv2;
  if (k < nz - 1) d += hinv2;
  if (j < ny - 1) d += hinv2;
  if (i < nx - 1) d += hinv2;
  return d;
}

static void check_grid(int nx, int ny, int nz, double kappa, int nchains)
{
  const size_t n  = (size_t)nx * (size_t)ny * (size_t)nz;
  pmg_rbstats  rb = NULL;
  REQUIRE(pmg_rbstats_create_dmda(nx, ny, nz, kappa, nchains, &rb) == PMG_SUCCESS && rb);
  double *q = malloc(sizeof(double) * n), *q2 = malloc(sizeof(double) * n); /* exactly n: a write past the end is a finding */
  REQUIRE(q && q2);
  REQUIRE(pmg_rbstats_get_cond_precision(rb, q) == PMG_SUCCESS);
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) REQUIRE(q[i + (size_t)nx * (j + (size_t)ny * k)] == want_diag(nx, ny, nz, kappa, i, j, k));
  double by = -1.0;
  REQUIRE(pmg_rbstats_get_algorithmic_bytes(rb, &by) == PMG_SUCCESS && by == 8.0 * n * nchains + 32.0 * n);
  REQUIRE(pmg_rbstats_set_rhs(rb, (const double *)0x1000) == PMG_SUCCESS); /* borrowed, never read here */
  REQUIRE(pmg_rbstats_get_algorithmic_bytes(rb, &by) == PMG_SUCCESS && by == 8.0 * n * nchains + 40.0 * n);
  /* a low-rank term of rank 3 with a zero row: q = a_ii + sum_k S_k * (B_ik * B_ik), k ascending */
  const int kr = 3;
  double   *B  = malloc(sizeof(double) * n * kr), S[3] = {2.0, 0.5, 11.0};
  REQUIRE(B);
  for (size_t r = 0; r < n; ++r)
    for (int c = 0; c < kr; ++c) B[r + n * c] = r == n / 2 ? 0.0 : sin(1.0 + (double)r * 0.37 + c) / sqrt((double)n);
  REQUIRE(pmg_rbstats_set_lowrank(rb, kr, B, S) == PMG_SUCCESS);
  REQUIRE(pmg_rbstats_get_cond_precision(rb, q2) == PMG_SUCCESS);
  for (size_t r = 0; r < n; ++r) {
    double w = q[r];
    for (int c = 0; c < kr; ++c) w = w + S[c] * (B[r + n * c] * B[r + n * c]);
    REQUIRE(q2[r] == w);
  }
  REQUIRE(q2[n / 2] == q[n / 2]);
  REQUIRE(pmg_rbstats_get_algorithmic_bytes(rb, &by) == PMG_SUCCESS && by == 8.0 * n * nchains + 40.0 * n + 8.0 * n + 8.0 * n * kr + 8.0 * n * nchains);
  /* refused terms change nothing */
  REQUIRE(pmg_rbstats_set_lowrank(rb, -1, B, S) == PMG_ERR_ARG_OUTOFRANGE);
  REQUIRE(pmg_rbstats_set_lowrank(rb, 65, B, S) == PMG_ERR_ARG_OUTOFRANGE);
  REQUIRE(pmg_rbstats_set_lowrank(rb, kr, NULL, S) == PMG_ERR_ARG_NULL);
  double Sbad[3] = {2.0, INFINITY, 11.0};
  REQUIRE(pmg_rbstats_set_lowrank(rb, kr, B, Sbad) == PMG_ERR_ARG_WRONG);
  double Sneg[3] = {-1e6 * (double)n, 0.5, 11.0};
  REQUIRE(pmg_rbstats_set_lowrank(rb, kr, B, Sneg) == PMG_ERR_ARG_WRONG);
  REQUIRE(pmg_rbstats_get_cond_precision(rb, q) == PMG_SUCCESS);
  for (size_t r = 0; r < n; ++r) REQUIRE(q[r] == q2[r]);
  REQUIRE(pmg_rbstats_set_lowrank(rb, 0, NULL, NULL) == PMG_SUCCESS);
  REQUIRE(pmg_rbstats_get_cond_precision(rb, q) == PMG_SUCCESS);
  REQUIRE(q[0] == want_diag(nx, ny, nz, kappa, 0, 0, 0) && q[n - 1] == want_diag(nx, ny, nz, kappa, nx - 1, ny - 1, nz - 1));
  /* the callbacks refuse other sizes before anything is launched; nothing has been recorded */
  REQUIRE(pmg_rbstats_callback(0, (const double *)0x1000, (int32_t)n - 1, nchains, rb) == PMG_ERR_ARG_SIZ);
  REQUIRE(pmg_rbstats_callback(0, (const double *)0x1000, (int32_t)n, nchains + 1, rb) == PMG_ERR_ARG_SIZ);
  REQUIRE(pmg_rbstats_get_fields(rb, (double *)0x1000, (double *)0x1000, NULL) == PMG_ERR_ARG_WRONGSTATE);
  REQUIRE(pmg_rbstats_update(rb, NULL, NULL) == PMG_ERR_ARG_NULL);
  REQUIRE(pmg_rbstats_cond_mean(rb, (const double *)0x1000, (double *)0x1000, NULL) == PMG_ERR_ARG_WRONG);
  REQUIRE(pmg_rbstats_reset(rb) == PMG_SUCCESS); /* nothing allocated: no synchronisation */
  int32_t steps = -1;
  int64_t samples = -1;
  REQUIRE(pmg_rbstats_get_count(rb, &steps, &samples) == PMG_SUCCESS && steps == 0 && samples == 0);
  free(B), free(q), free(q2);
  REQUIRE(pmg_rbstats_destroy(&rb) == PMG_SUCCESS && rb == NULL);
}

int main(void)
{
  pmg_rbstats rb = (pmg_rbstats)0x10; /* a failed creation leaves NULL, and destroying that is a no-op */
  REQUIRE(pmg_rbstats_create_dmda(5, 4, 3, 1.0, 1, NULL) == PMG_ERR_ARG_NULL);
  REQUIRE(pmg_rbstats_create_dmda(1, 4, 3, 1.0, 1, &rb) == PMG_ERR_ARG_OUTOFRANGE && rb == NULL);
  REQUIRE(pmg_rbstats_destroy(&rb) == PMG_SUCCESS && rb == NULL);
  REQUIRE(pmg_rbstats_create_dmda(1, 4, 3, 1.0, 0, &rb) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "grid")); /* the grid before the chains */
  REQUIRE(pmg_rbstats_create_dmda(-7, 4, 3, 1.0, 1, &rb) == PMG_ERR_ARG_OUTOFRANGE);
  REQUIRE(pmg_rbstats_create_dmda(5, 0, 3, 1.0, 1, &rb) == PMG_ERR_ARG_OUTOFRANGE);
  REQUIRE(pmg_rbstats_create_dmda(5, 4, 0, 1.0, 1, &rb) == PMG_ERR_ARG_OUTOFRANGE);
  REQUIRE(pmg_rbstats_create_dmda(2048, 2048, 512, 1.0, 1, &rb) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "points")); /* 2^31 */
  REQUIRE(pmg_rbstats_create_dmda(65536, 65536, 1, 1.0, 1, &rb) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "points")); /* 2^32: wraps to 0 in 32 bits */
  REQUIRE(pmg_rbstats_create_dmda(INT32_MAX, INT32_MAX, INT32_MAX, 1.0, 1, &rb) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "points"));
  REQUIRE(pmg_rbstats_create_dmda(65536, 65536, 1, 1.0, 0, &rb) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "points")); /* the size before the chains */
  REQUIRE(pmg_rbstats_create_dmda(5, 4, 3, 1.0, 0, &rb) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "nchains"));
  REQUIRE(pmg_rbstats_create_dmda(5, 4, 3, 1.0, -2, &rb) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "nchains"));
  REQUIRE(pmg_rbstats_create_dmda(5, 4, 3, NAN, 1, &rb) == PMG_ERR_ARG_WRONG && rb == NULL);
  REQUIRE(pmg_rbstats_create_dmda(5, 4, 3, 1e200, 1, &rb) == PMG_ERR_ARG_WRONG && rb == NULL);
  REQUIRE(pmg_rbstats_destroy(&rb) == PMG_SUCCESS);
  REQUIRE(pmg_rbstats_destroy(NULL) == PMG_SUCCESS);
  check_grid(2, 2, 1, 0.1, 1);
  check_grid(5, 4, 3, 0.1, 3);
  check_grid(9, 9, 1, 1.0 / 3.0, 1);
  check_grid(17, 17, 17, 0.1, 65);
  check_grid(2, 1, 1, 0.0, 1); /* kappa = 0: the one neighbour makes q positive */
  printf("rbstats_dmda_host ok\n");
  return 0;
}
