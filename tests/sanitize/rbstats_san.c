/* AddressSanitizer + UndefinedBehaviorSanitizer run of the host paths of the Rao-Blackwellised statistics group
 * (parmgmc_amd/csrc/pmg_rbstats.c with pmg_common.c) that need no device: the copy of the matrix (the diagonal taken out of
 * rows stored in any order, rows without off-diagonal entries, columns stored twice), every rejected matrix, the low-rank
 * factors set, replaced and removed, the conditional precisions, and every rejected call -- none of which may reach a kernel
 * launcher: the launchers are stubs here that count how often they are reached.  Built and run by
 * tests/test_sanitize_rbstats.py with gcc -fsanitize=address,undefined on the CPU; a finding aborts with a non-zero status. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "parmgmc_hip.h"

static int reached = 0;
#define LAUNCHER(name, ...) int name(__VA_ARGS__) { ++reached; return 1; }
LAUNCHER(pmgk_rbstats_update, const void *A, int32_t C, double cnt, const double *Y, double *m, double *M2, void *st)
LAUNCHER(pmgk_rbstats_cond_mean, const void *A, int32_t C, const double *Y, double *M, void *st)
LAUNCHER(pmgk_rbstats_fields, int64_t n, double cnt, const double *q, const double *m, const double *M2, double *mo, double *vo, void *st)
LAUNCHER(pmgk_lrc_btx_chains, int64_t n, const int64_t *rows, int k, const double *M, int64_t ldm, const double *Y, int32_t C, double *p, const double *s, double *o, void *st)
LAUNCHER(pmgk_lrc_btx_chains_nblocks, int64_t n, int compact)
LAUNCHER(pmgk_fill_normal_rows, int64_t n, uint64_t seed, uint64_t sweep, double *xi, void *st)
LAUNCHER(pmgk_stream_triad, int64_t n, const double *a, const double *b, double *c, void *st)
pmg_status pmg_chains_size_check(int64_t ld, int32_t nchains) { return ld >= 1 && nchains >= 1 ? PMG_SUCCESS : PMG_ERR_ARG_OUTOFRANGE; } /* pmg_mcsor.c's, not part of this program */

static int failures = 0;
#define EXPECT(call, code, text) \
  do { \
    const pmg_status s_ = (call); \
    if (s_ != (code) || ((text) && !strstr(pmg_last_error_string(), (text)))) { \
      printf("line %d: status %d (want %d), message \"%s\"\n", __LINE__, (int)s_, (int)(code), pmg_last_error_string()); \
      ++failures; \
    } \
  } while (0)
#define REQUIRE(cond) \
  do { \
    if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), ++failures; \
  } while (0)

int main(void)
{
  enum { N = 5, C = 3, K = 2 };
  /* row 0: diagonal last, columns descending; row 1: no off-diagonal entry; row 2: column 0 stored twice; row 3: diagonal first;
     row 4: diagonal in the middle.  The arrays are heap blocks of exactly their size, so that a read past them is a finding. */
  const int32_t rp_[N + 1] = {0, 3, 4, 8, 10, 13}, ci_[13] = {4, 2, 0, 1, 0, 2, 0, 3, 3, 2, 0, 4, 2};
  const double  v_[13] = {-1, -0.5, 4, 3, -0.25, 5, -0.25, -1, 6, -1, -1, 7, -0.5};
  int32_t *rp = malloc(sizeof rp_), *ci = malloc(sizeof ci_);
  double  *v = malloc(sizeof v_), *q = malloc(sizeof(double) * N), *B = malloc(sizeof(double) * N * K), *S = malloc(sizeof(double) * K);
  memcpy(rp, rp_, sizeof rp_), memcpy(ci, ci_, sizeof ci_), memcpy(v, v_, sizeof v_);
  const double *Y = (const double *)(uintptr_t)0x2000; /* never dereferenced */
  double       *M = (double *)(uintptr_t)0x4000;
  pmg_rbstats   h = NULL;

  /* creation */
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_create_csr(0, rp, ci, v, C, &h), PMG_ERR_ARG_OUTOFRANGE, "n = 0");
  EXPECT(pmg_rbstats_create_csr(INT32_MIN, rp, ci, v, C, &h), PMG_ERR_ARG_OUTOFRANGE, NULL);
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, 0, &h), PMG_ERR_ARG_OUTOFRANGE, NULL);
  EXPECT(pmg_rbstats_create_csr(N, NULL, ci, v, C, &h), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_create_csr(N, rp, NULL, v, C, &h), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, NULL, C, &h), PMG_ERR_ARG_NULL, NULL);
  REQUIRE(h == NULL);
  /* rejected matrices: each defect in turn, then repaired */
  ci[3] = 0; /* row 1 loses its diagonal */
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_ERR_ARG_WRONG, "row 1 has no stored diagonal");
  ci[3] = 1;
  ci[0] = 0; /* row 0 stores it twice */
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_ERR_ARG_WRONG, "twice");
  ci[0] = 4;
  for (int t = 0; t < 4; ++t) {
    const double bad[4] = {0.0, -6.0, NAN, INFINITY};
    v[8]                = bad[t];
    EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_ERR_ARG_WRONG, "positive and finite");
  }
  v[8]  = 6;
  ci[12] = N;
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_ERR_ARG_OUTOFRANGE, "column 5 out of range in row 4");
  ci[12] = -1;
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_ERR_ARG_OUTOFRANGE, "out of range");
  ci[12] = 2;
  rp[2]  = 2;
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_ERR_ARG_WRONG, "monotone");
  rp[2] = 4;
  rp[0] = -1;
  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_ERR_ARG_WRONG, "rowptr runs");
  rp[0] = 0;
  REQUIRE(h == NULL);

  EXPECT(pmg_rbstats_create_csr(N, rp, ci, v, C, &h), PMG_SUCCESS, NULL);
  REQUIRE(h != NULL);
  memset(rp, 0x7f, sizeof rp_), memset(ci, 0x7f, sizeof ci_), memset(v, 0x7f, sizeof v_); /* the handle keeps copies */
  EXPECT(pmg_rbstats_get_cond_precision(h, q), PMG_SUCCESS, NULL);
  REQUIRE(q[0] == 4 && q[1] == 3 && q[2] == 5 && q[3] == 6 && q[4] == 7);
  double bytes = 0;
  EXPECT(pmg_rbstats_get_algorithmic_bytes(h, &bytes), PMG_SUCCESS, NULL);
  REQUIRE(bytes == 12.0 * 13 + 8.0 * N * C + 48.0 * N);

  /* the low-rank term: set, rejected (nothing changes), replaced by a smaller one, removed */
  for (int i = 0; i < N * K; ++i) B[i] = 0.5 * (i % N);
  S[0] = 2, S[1] = 4;
  EXPECT(pmg_rbstats_set_lowrank(NULL, K, B, S), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_set_lowrank(h, -1, B, S), PMG_ERR_ARG_OUTOFRANGE, "rank");
  EXPECT(pmg_rbstats_set_lowrank(h, 65, B, S), PMG_ERR_ARG_OUTOFRANGE, "rank");
  EXPECT(pmg_rbstats_set_lowrank(h, K, NULL, S), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_set_lowrank(h, K, B, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_set_lowrank(h, K, B, S), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_get_cond_precision(h, q), PMG_SUCCESS, NULL);
  REQUIRE(q[0] == 4 && q[1] == 3 + 2 * 0.25 + 4 * 0.25 && q[4] == 7 + 2 * 4.0 + 4 * 4.0);
  S[1] = -40; /* row 4: 7 + 8 - 160 */
  EXPECT(pmg_rbstats_set_lowrank(h, K, B, S), PMG_ERR_ARG_WRONG, "positive and finite");
  S[1] = NAN;
  EXPECT(pmg_rbstats_set_lowrank(h, K, B, S), PMG_ERR_ARG_WRONG, "positive and finite");
  EXPECT(pmg_rbstats_get_cond_precision(h, q), PMG_SUCCESS, NULL);
  REQUIRE(q[4] == 7 + 2 * 4.0 + 4 * 4.0);
  EXPECT(pmg_rbstats_get_algorithmic_bytes(h, &bytes), PMG_SUCCESS, NULL);
  REQUIRE(bytes == 12.0 * 13 + 16.0 * N * C + 48.0 * N + 8.0 * N * K);
  EXPECT(pmg_rbstats_set_lowrank(h, 1, B, S), PMG_SUCCESS, NULL); /* reads one column of B and one entry of S */
  EXPECT(pmg_rbstats_get_cond_precision(h, q), PMG_SUCCESS, NULL);
  REQUIRE(q[4] == 7 + 2 * 4.0);
  EXPECT(pmg_rbstats_set_lowrank(h, 0, NULL, NULL), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_get_cond_precision(h, q), PMG_SUCCESS, NULL);
  REQUIRE(q[4] == 7);

  /* every rejected call of the rest of the group */
  int32_t steps = -1;
  int64_t samples = -1;
  EXPECT(pmg_rbstats_set_rhs(NULL, Y), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_set_rhs(h, Y), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_set_rhs(h, NULL), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_set_stream(NULL, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_set_stream(h, NULL), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_update(NULL, Y, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_update(h, NULL, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_cond_mean(NULL, Y, M, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_cond_mean(h, NULL, M, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_cond_mean(h, Y, NULL, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_cond_mean(h, Y, (double *)(uintptr_t)Y, NULL), PMG_ERR_ARG_WRONG, "overwrite");
  EXPECT(pmg_rbstats_callback(0, Y, N, C, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_callback(0, Y, N + 1, C, h), PMG_ERR_ARG_SIZ, "6 rows x 3 chains");
  EXPECT(pmg_rbstats_callback(0, Y, N, C + 1, h), PMG_ERR_ARG_SIZ, NULL);
  EXPECT(pmg_rbstats_callback(0, Y, INT32_MIN, INT32_MAX, h), PMG_ERR_ARG_SIZ, NULL);
  EXPECT(pmg_rbstats_callback(0, NULL, N, C, h), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_sample_callback(0, Y, N, h), PMG_ERR_ARG_SIZ, NULL);
  EXPECT(pmg_rbstats_sample_callback(0, Y, N, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_reset(NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_reset(h), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_get_count(NULL, &steps, &samples), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_get_count(h, &steps, &samples), PMG_SUCCESS, NULL);
  REQUIRE(steps == 0 && samples == 0);
  EXPECT(pmg_rbstats_get_count(h, NULL, NULL), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_get_fields(NULL, M, M, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_get_fields(h, M, M, NULL), PMG_ERR_ARG_WRONGSTATE, "at least 2 samples");
  EXPECT(pmg_rbstats_get_cond_precision(NULL, q), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_get_cond_precision(h, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_get_algorithmic_bytes(NULL, &bytes), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_get_algorithmic_bytes(h, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_rbstats_destroy(&h), PMG_SUCCESS, NULL);
  REQUIRE(h == NULL);
  EXPECT(pmg_rbstats_destroy(&h), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_destroy(NULL), PMG_SUCCESS, NULL);

  /* one row, one entry: the smallest matrix */
  const int32_t rp1[2] = {0, 1}, ci1[1] = {0};
  const double  v1[1]  = {2.5};
  EXPECT(pmg_rbstats_create_csr(1, rp1, ci1, v1, 1, &h), PMG_SUCCESS, NULL);
  EXPECT(pmg_rbstats_get_cond_precision(h, q), PMG_SUCCESS, NULL);
  REQUIRE(q[0] == 2.5);
  EXPECT(pmg_rbstats_destroy(&h), PMG_SUCCESS, NULL);

  free(rp), free(ci), free(v), free(q), free(B), free(S);
  if (reached) ++failures, printf("%d launcher calls on paths that need no device\n", reached);
  if (failures) return 1;
  printf("rbstats_san ok\n");
  return 0;
}
