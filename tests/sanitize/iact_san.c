/* AddressSanitizer + UndefinedBehaviorSanitizer run of the argument-check paths of the device IACT entry points
 * (parmgmc_amd/csrc/pmg_iact.c with pmg_chainstats.c and pmg_common.c): every rejected call returns its code and message
 * without reaching a kernel launcher -- the launchers are stubs here that count how often they are reached.  Built and run by
 * tests/test_sanitize_iact.py with gcc -fsanitize=address,undefined on the CPU; a finding aborts with a non-zero status. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "parmgmc_hip.h"

static int reached = 0;
#define LAUNCHER(name, ...) int name(__VA_ARGS__) { ++reached; return 1; }
typedef struct { const double *w[PMG_CHAINSTATS_MAX_QOI]; } san_qoi;
LAUNCHER(pmgk_iact_transpose, int64_t n, int32_t S, const double *X, int64_t ld, double *Z, void *st)
LAUNCHER(pmgk_iact_scan, int64_t n, int32_t S, double *Z, int32_t ml, int32_t na, double *acf, double *tau, int32_t *w, int32_t *v, void *st)
LAUNCHER(pmgk_chainstats_update, int64_t n, int32_t C, int nq, const san_qoi *Q, double cnt, const double *Y, double *m, double *M2, double *p, double *t, int64_t qs, void *st)
LAUNCHER(pmgk_chainstats_fields, int64_t n, double cnt, const double *m, const double *M2, double *mo, double *vo, void *st)
LAUNCHER(pmgk_fill_normal_rows, int64_t n, uint64_t seed, uint64_t sweep, double *xi, void *st)
LAUNCHER(pmgk_stream_triad, int64_t n, const double *a, const double *b, double *c, void *st)
void pmgk_chainstats_geometry(int64_t n, int32_t C, int32_t *iters, int32_t *nb) { (void)n; (void)C; ++reached; *iters = *nb = 1; }
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

int main(void)
{
  enum { S = 4 };
  double        tau[S];
  int32_t       win[S], val[S];
  const double *X   = (const double *)(uintptr_t)0x2000; /* never dereferenced */
  double       *acf = (double *)(uintptr_t)0x4000;
  for (int i = 0; i < S; ++i) tau[i] = -7.0, win[i] = val[i] = -7;

  EXPECT(pmg_iact_chains(100, S, NULL, S, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_iact_chains(100, S, X, S, 0, NULL, win, val, 0, NULL, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_iact_chains(1, S, X, S, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "Too few data points");
  EXPECT(pmg_iact_chains(-5, S, X, S, 0, tau, NULL, NULL, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "Too few data points");
  EXPECT(pmg_iact_chains((int64_t)1 << 31, 1, X, 1, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "32-bit");
  EXPECT(pmg_iact_chains(INT64_MAX, S, X, S, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, NULL);
  EXPECT(pmg_iact_chains(100, 0, X, S, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "nseries");
  EXPECT(pmg_iact_chains(100, INT32_MIN, X, S, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "nseries");
  EXPECT(pmg_iact_chains(100, INT32_MAX, X, INT32_MAX, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "nseries");
  EXPECT(pmg_iact_chains((int64_t)1 << 30, 1 << 20, X, 1 << 20, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "scratch");
  EXPECT(pmg_iact_chains(100, S, X, S - 1, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "leading dimension");
  EXPECT(pmg_iact_chains(100, S, X, INT64_MIN, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "leading dimension");
  EXPECT(pmg_iact_chains(100, S, X, S, -1, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "max_lag");
  EXPECT(pmg_iact_chains(100, S, X, S, INT32_MIN, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "max_lag");
  EXPECT(pmg_iact_chains(100, S, X, S, 0, tau, win, val, -1, acf, NULL), PMG_ERR_ARG_OUTOFRANGE, "nacf");
  EXPECT(pmg_iact_chains(100, S, X, S, 0, tau, win, val, 101, acf, NULL), PMG_ERR_ARG_OUTOFRANGE, "nacf");

  pmg_chainstats h = NULL;
  EXPECT(pmg_chainstats_create(10, S, 2, 30, &h), PMG_SUCCESS, NULL);
  EXPECT(pmg_chainstats_iact(NULL, 0, 0, 2, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_chainstats_iact(h, 0, 0, 2, 0, NULL, win, val, 0, NULL, NULL), PMG_ERR_ARG_NULL, NULL);
  EXPECT(pmg_chainstats_iact(h, -1, 0, 0, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "QOI");
  EXPECT(pmg_chainstats_iact(h, 2, 0, 0, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "QOI");
  EXPECT(pmg_chainstats_iact(h, INT32_MAX, 0, 0, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "QOI");
  EXPECT(pmg_chainstats_iact(h, 0, 0, 2, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "recorded");
  EXPECT(pmg_chainstats_iact(h, 1, 1, 0, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "recorded");
  EXPECT(pmg_chainstats_iact(h, 1, -1, 2, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "recorded");
  EXPECT(pmg_chainstats_iact(h, 1, 0, -1, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "recorded");
  EXPECT(pmg_chainstats_iact(h, 1, INT32_MAX, INT32_MAX, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "recorded");
  EXPECT(pmg_chainstats_iact(h, 1, INT32_MIN, INT32_MAX, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "recorded");
  EXPECT(pmg_chainstats_iact(h, 0, 0, 0, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "Too few data points");
  EXPECT(pmg_chainstats_iact(h, 1, 0, 0, -1, tau, NULL, NULL, 5, acf, NULL), PMG_ERR_ARG_OUTOFRANGE, "Too few data points");
  EXPECT(pmg_chainstats_destroy(&h), PMG_SUCCESS, NULL);
  EXPECT(pmg_chainstats_create(10, S, 0, 30, &h), PMG_SUCCESS, NULL);
  EXPECT(pmg_chainstats_iact(h, 0, 0, 0, 0, tau, win, val, 0, NULL, NULL), PMG_ERR_ARG_OUTOFRANGE, "QOI");
  EXPECT(pmg_chainstats_destroy(&h), PMG_SUCCESS, NULL);

  for (int i = 0; i < S; ++i)
    if (tau[i] != -7.0 || win[i] != -7 || val[i] != -7) ++failures, printf("a rejected call wrote output %d\n", i);
  if (reached) ++failures, printf("%d launcher calls on argument-check paths\n", reached);
  if (failures) return 1;
  printf("iact_san ok\n");
  return 0;
}
