/* AddressSanitizer + UndefinedBehaviorSanitizer run of the host part of the coloured block Gibbs sampler
 * (csrc/pmg_blockgibbs_host.c): colouring, interior / exterior split, packing, Cholesky factors and their inverses, and every
 * error path.  Built and run by tests/test_blockgibbs_host.py with gcc -fsanitize=address,undefined -ffp-contract=off
 * together with that one file; nothing is preloaded, no device call is made.  A finding or a failed check ends with a
 * non-zero status.
 *
 * Bounds (u = 2^-53, gamma(k) = k u / (1 - k u); the first is factor_bound of tests/chol_edge_refs.py, the others are the
 * classical ones of the same kind for a triangular inverse by forward substitution):
 *   ||A_PP - L L^T||_F <= gamma(m + 1) trace(A_PP)
 *   |L W - I|          <= gamma(m) |L| |W|                 componentwise (every column of W solves L w = e_j)
 *   ||W L - I||_F      <= C_FWD m u ||W||_F ||L||_F         (C_FWD = 8; ||W||_F ||L||_F bounds the condition number of L) */
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
      fprintf(stderr, "blockgibbs_host.c:%d: %s failed (last message: %s)\n", __LINE__, #cond, g_msg); \
      exit(1); \
    } \
  } while (0)

static const double U = 0x1p-53;
static double       gam(int k) { return k * U / (1.0 - k * U); }

typedef struct {
  int32_t  n, *rp, *ci;
  double  *v;
} csr;

static void csr_free(csr *A) { free(A->rp), free(A->ci), free(A->v); }

/* symmetric banded matrix, every entry of the band stored, strictly diagonally dominant */
static csr banded(int32_t n, int32_t hb)
{
  csr A = {n, calloc((size_t)n + 1, sizeof(int32_t)), malloc(sizeof(int32_t) * (size_t)n * (2 * (size_t)hb + 1)), malloc(sizeof(double) * (size_t)n * (2 * (size_t)hb + 1))};
  REQUIRE(A.rp && A.ci && A.v);
  int32_t k = 0;
  for (int32_t r = 0; r < n; ++r) {
    double  sum = 0.0;
    int32_t dk  = -1;
    for (int32_t c = r - hb < 0 ? 0 : r - hb; c <= r + hb && c < n; ++c) {
      A.ci[k] = c;
      if (c == r) dk = k;
      else {
        const int32_t lo = r < c ? r : c, hi = r < c ? c : r;
        A.v[k] = -(0.1 + (double)((lo * 31 + hi * 17) % 97) / 107.0);
        sum += fabs(A.v[k]);
      }
      ++k;
    }
    A.v[dk]     = sum + 1.0;
    A.rp[r + 1] = k;
  }
  return A;
}

/* 5-point shifted Laplacian on an nx x ny grid */
static csr laplace(int32_t nx, int32_t ny)
{
  const int32_t n = nx * ny;
  csr           A = {n, calloc((size_t)n + 1, sizeof(int32_t)), malloc(sizeof(int32_t) * 5 * (size_t)n), malloc(sizeof(double) * 5 * (size_t)n)};
  REQUIRE(A.rp && A.ci && A.v);
  int32_t k = 0;
  for (int32_t j = 0; j < ny; ++j)
    for (int32_t i = 0; i < nx; ++i) {
      if (j > 0) A.ci[k] = i + nx * (j - 1), A.v[k++] = -1.0;
      if (i > 0) A.ci[k] = i - 1 + nx * j, A.v[k++] = -1.0;
      A.ci[k] = i + nx * j, A.v[k++] = 4.25;
      if (i < nx - 1) A.ci[k] = i + 1 + nx * j, A.v[k++] = -1.0;
      if (j < ny - 1) A.ci[k] = i + nx * (j + 1), A.v[k++] = -1.0;
      A.rp[i + nx * j + 1] = k;
    }
  return A;
}

static int stored(const csr *A, int32_t r, int32_t c)
{
  for (int32_t k = A->rp[r]; k < A->rp[r + 1]; ++k)
    if (A->ci[k] == c) return 1;
  return 0;
}

static int in_block(const int32_t *bp, const int32_t *br, int32_t p, int32_t row)
{
  for (int32_t s = bp[p]; s < bp[p + 1]; ++s)
    if (br[s] == row) return 1;
  return 0;
}

/* the conflict rule, by brute force */
static int conflict(const csr *A, const int32_t *bp, const int32_t *br, int32_t p, int32_t q)
{
  for (int32_t s = bp[p]; s < bp[p + 1]; ++s)
    for (int32_t t = bp[q]; t < bp[q + 1]; ++t)
      if (br[s] == br[t] || stored(A, br[s], br[t]) || stored(A, br[t], br[s])) return 1;
  return 0;
}

/* everything a plan promises, against the matrix and the blocks it was built from */
static void check_plan(const csr *A, int32_t nb, const int32_t *bp, const int32_t *br, const int32_t *pos_of_row, int32_t ld, int first_fit, const pmg_bg_plan *pl)
{
  REQUIRE(pl->n == A->n && pl->nblocks == nb && pl->nslots == bp[nb] && pl->ld == (pos_of_row ? ld : A->n));
  /* colours: valid, and (default rule) first-fit in block order */
  for (int32_t p = 0; p < nb; ++p) {
    REQUIRE(pl->colors[p] >= 0 && pl->colors[p] < pl->ncolors);
    unsigned char taken[PMG_BG_MAX_BLOCK * 64] = {0};
    for (int32_t q = 0; q < nb; ++q)
      if (q != p && conflict(A, bp, br, p, q)) {
        REQUIRE(pl->colors[q] != pl->colors[p]);
        if (q < p && pl->colors[q] < (int32_t)sizeof taken) taken[pl->colors[q]] = 1;
      }
    if (first_fit) {
      REQUIRE(!taken[pl->colors[p]]);
      for (int32_t c = 0; c < pl->colors[p]; ++c) REQUIRE(taken[c]);
    }
  }
  /* tiles: every slot sits in a tile of its block's colour and of the smallest width that holds the block, its block's lanes
     are consecutive from a multiple of the width; lanes without a slot have no position */
  int64_t nlive = 0;
  for (int64_t t = 0; t < (int64_t)pl->ntiles * 64; ++t) nlive += pl->pos[t] >= 0;
  REQUIRE(nlive == pl->nslots);
  int64_t next_total = 0;
  for (int32_t p = 0; p < nb; ++p) {
    const int32_t m = bp[p + 1] - bp[p], g = m <= 8 ? 8 : m <= 16 ? 16 : m <= 32 ? 32 : 64;
    const int32_t tl0 = pl->slot_tile_lane[bp[p]], t = tl0 / 64;
    REQUIRE(t >= pl->ctile[pl->colors[p]] && t < pl->ctile[pl->colors[p] + 1]);
    REQUIRE(pl->tile_g[t] == g && (tl0 % 64) % g == 0);
    for (int32_t i = 0; i < m; ++i) {
      const int32_t s = bp[p] + i, row = br[s], tl = pl->slot_tile_lane[s], l = tl % 64;
      REQUIRE(tl == tl0 + i && pl->slot[tl] == s && pl->pos[tl] == (pos_of_row ? pos_of_row[row] : row));
      /* interior and exterior entries partition the row; the exterior ones keep the storage order, then pads of value 0 at a valid position */
      int32_t ni = 0, ne = 0;
      for (int32_t k = A->rp[row]; k < A->rp[row + 1]; ++k) {
        if (in_block(bp, br, p, A->ci[k])) {
          ++ni;
          continue;
        }
        REQUIRE(ne < pl->tile_ew[t]);
        const int64_t e = pl->tile_eoff[t] + (int64_t)ne * 64 + l;
        REQUIRE(pl->evals[e] == A->v[k] && pl->ecols[e] == (pos_of_row ? pos_of_row[A->ci[k]] : A->ci[k]));
        ++ne;
      }
      REQUIRE(ni == pl->slot_nint[s] && ne == pl->slot_next[s] && ni + ne == A->rp[row + 1] - A->rp[row]);
      next_total += ne;
      for (int32_t j = ne; j < pl->tile_ew[t]; ++j) {
        const int64_t e = pl->tile_eoff[t] + (int64_t)j * 64 + l;
        REQUIRE(pl->evals[e] == 0.0 && pl->ecols[e] >= 0 && pl->ecols[e] < pl->ld);
      }
    }
    /* the factors */
    const double *L = pl->L + pl->woff[p], *W = pl->W + pl->woff[p];
    double        ef = 0.0, tr = 0.0, nW = 0.0, nL = 0.0, eWL = 0.0;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        double a = 0.0; /* A_PP from the lower triangle */
        const int32_t hi = i > j ? i : j, lo = i > j ? j : i;
        for (int32_t k = A->rp[br[bp[p] + hi]]; k < A->rp[br[bp[p] + hi] + 1]; ++k)
          if (A->ci[k] == br[bp[p] + lo]) a = A->v[k];
        long double llt = 0.0L, lw = 0.0L, alw = 0.0L, wl = 0.0L;
        for (int k = 0; k < m; ++k) {
          llt += (long double)L[i * m + k] * L[j * m + k];
          lw += (long double)L[i * m + k] * W[k * m + j];
          alw += fabsl((long double)L[i * m + k] * W[k * m + j]);
          wl += (long double)W[i * m + k] * L[k * m + j];
        }
        ef += (double)((a - llt) * (a - llt));
        if (i == j) tr += a;
        nW += W[i * m + j] * W[i * m + j];
        nL += L[i * m + j] * L[i * m + j];
        eWL += (double)((wl - (i == j)) * (wl - (i == j)));
        REQUIRE(fabsl(lw - (i == j)) <= gam(m) * alw + 4 * U * (i == j)); /* (+ the rounding of the comparison itself) */
        if (j > i) REQUIRE(L[i * m + j] == 0.0 && W[i * m + j] == 0.0);
        /* the packed rows: M = W^T W summed over k ascending, and W^T; zero outside the block */
        double acc = 0.0;
        for (int k = 0; k < m; ++k) acc = acc + W[k * m + i] * W[k * m + j];
        const int64_t e = pl->tile_foff[t] + (int64_t)j * 64 + tl0 % 64 + i;
        REQUIRE(pl->M[e] == acc && pl->WT[e] == W[j * m + i]);
      }
    REQUIRE(sqrt(ef) <= gam(m + 1) * tr);
    REQUIRE(sqrt(eWL) <= 8.0 * m * U * sqrt(nW) * sqrt(nL));
    for (int i = 0; i < g; ++i) /* pad rows and pad columns of the block's square */
      for (int j = 0; j < g; ++j)
        if (i >= m || j >= m) REQUIRE(pl->M[pl->tile_foff[t] + (int64_t)j * 64 + tl0 % 64 + i] == 0.0 && pl->WT[pl->tile_foff[t] + (int64_t)j * 64 + tl0 % 64 + i] == 0.0);
  }
  REQUIRE(next_total == pl->nnz_ext);
  for (int32_t t = 0; t < pl->ntiles; ++t) REQUIRE(pl->tile_foff[t + 1] - pl->tile_foff[t] == 64 * (int64_t)pl->tile_g[t] && pl->tile_eoff[t + 1] - pl->tile_eoff[t] == 64 * (int64_t)pl->tile_ew[t]);
}

int main(void)
{
  pmg_bg_plan pl;
  /* 1. vertex stars of the 9 x 9 Laplacian (overlapping, 3 to 5 rows), first-fit, no layout */
  {
    csr      A  = laplace(9, 9);
    int32_t *bp = malloc(sizeof(int32_t) * ((size_t)A.n + 1));
    REQUIRE(bp);
    memcpy(bp, A.rp, sizeof(int32_t) * ((size_t)A.n + 1));
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, A.n, bp, A.ci, 0, NULL, 0, NULL, &pl) == PMG_SUCCESS);
    check_plan(&A, A.n, bp, A.ci, NULL, 0, 1, &pl);
    int32_t *user = malloc(sizeof(int32_t) * (size_t)A.n);
    REQUIRE(user);
    memcpy(user, pl.colors, sizeof(int32_t) * (size_t)A.n);
    const int32_t nc = pl.ncolors;
    pmg_bg_plan_free(&pl);
    /* the same colouring handed in by the user, with a layout that reverses the rows and has ld > n */
    int32_t *pos = malloc(sizeof(int32_t) * (size_t)A.n);
    REQUIRE(pos);
    for (int32_t r = 0; r < A.n; ++r) pos[r] = A.n + 10 - r;
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, A.n, bp, A.ci, nc + 2, user, A.n + 20, pos, &pl) == PMG_SUCCESS); /* two colours without a block */
    REQUIRE(pl.ncolors == nc + 2 && pl.ctile[nc] == pl.ctile[nc + 2]);
    check_plan(&A, A.n, bp, A.ci, pos, A.n + 20, 0, &pl);
    pmg_bg_plan_free(&pl);
    /* an invalid user colouring: blocks 0 and 1 overlap */
    user[1] = user[0];
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, A.n, bp, A.ci, nc, user, 0, NULL, &pl) == PMG_ERR_ARG_WRONG);
    REQUIRE(strstr(g_msg, "blocks 0 and 1"));
    user[1] = nc; /* a colour outside [0, ncolors) */
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, A.n, bp, A.ci, nc, user, 0, NULL, &pl) == PMG_ERR_ARG_OUTOFRANGE);
    /* bad layouts */
    pos[3] = pos[4];
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, A.n, bp, A.ci, 0, NULL, A.n + 20, pos, &pl) == PMG_ERR_ARG_WRONG);
    pos[3] = A.n + 20;
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, A.n, bp, A.ci, 0, NULL, A.n + 20, pos, &pl) == PMG_ERR_ARG_OUTOFRANGE);
    free(pos), free(user), free(bp);
    csr_free(&A);
  }
  /* 2. consecutive-row blocks of every width class on a banded matrix (310 rows of blocks on 300 rows: the last two overlap),
        first-fit; then on a tridiagonal matrix, mixed by a user colouring of two colours that each hold every width */
  {
    csr           A       = banded(300, 70);
    const int32_t sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64}, nb = 16;
    int32_t       bp[17] = {0}, br[310], k = 0, row = 0;
    for (int32_t p = 0; p < nb; ++p) {
      const int32_t r0 = row + sizes[p] <= 300 ? row : 300 - sizes[p];
      for (int32_t i = 0; i < sizes[p]; ++i) br[k + i] = r0 + i;
      k += sizes[p];
      row += sizes[p];
      bp[p + 1] = k;
    }
    REQUIRE(k == 310 && br[309] == 299);
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, nb, bp, br, 0, NULL, 0, NULL, &pl) == PMG_SUCCESS);
    check_plan(&A, nb, bp, br, NULL, 0, 1, &pl);
    pmg_bg_plan_free(&pl);
    /* a narrow band: only neighbouring blocks conflict, two colours hold every width */
    csr     T = banded(300, 1);
    int32_t two[16];
    for (int32_t p = 0; p < nb; ++p) two[p] = p % 2;
    REQUIRE(pmg_bg_plan_build(T.n, T.rp, T.ci, T.v, nb, bp, br, 2, two, 0, NULL, &pl) == PMG_SUCCESS);
    check_plan(&T, nb, bp, br, NULL, 0, 0, &pl);
    REQUIRE(pl.ncolors == 2);
    pmg_bg_plan_free(&pl);
    /* an indefinite block: the diagonal of row 160 (block 13, rows 150 .. 182) made negative */
    for (int32_t q = T.rp[160]; q < T.rp[161]; ++q)
      if (T.ci[q] == 160) T.v[q] = -1.0;
    REQUIRE(pmg_bg_plan_build(T.n, T.rp, T.ci, T.v, nb, bp, br, 0, NULL, 0, NULL, &pl) == PMG_ERR_MAT_CH_ZRPVT);
    REQUIRE(strstr(g_msg, "block 13") && strstr(g_msg, "order 11"));
    REQUIRE(!pl.colors && !pl.W); /* nothing left behind */
    csr_free(&T);
    /* block errors */
    int32_t bp1[2] = {0, 65}, br1[65];
    for (int32_t i = 0; i < 65; ++i) br1[i] = i;
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 1, bp1, br1, 0, NULL, 0, NULL, &pl) == PMG_ERR_SUP && strstr(g_msg, "65 rows"));
    int32_t bp2[3] = {0, 2, 2};
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 2, bp2, br1, 0, NULL, 0, NULL, &pl) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "block 1 is empty"));
    int32_t bp3[2] = {0, 3}, br3[3] = {5, 300, 6};
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 1, bp3, br3, 0, NULL, 0, NULL, &pl) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "row 300"));
    br3[1] = -1;
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 1, bp3, br3, 0, NULL, 0, NULL, &pl) == PMG_ERR_ARG_OUTOFRANGE);
    br3[1] = 5;
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 1, bp3, br3, 0, NULL, 0, NULL, &pl) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "twice"));
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, -1, bp3, br3, 0, NULL, 0, NULL, &pl) == PMG_ERR_ARG_OUTOFRANGE);
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 1, NULL, br3, 0, NULL, 0, NULL, &pl) == PMG_ERR_ARG_NULL);
    /* matrix errors */
    const int32_t keep = A.ci[7];
    A.ci[7]            = 300;
    br3[1]             = 7;
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 1, bp3, br3, 0, NULL, 0, NULL, &pl) == PMG_ERR_ARG_OUTOFRANGE && strstr(g_msg, "column 300"));
    A.ci[7] = keep;
    /* no block at all, and an empty matrix */
    int32_t bp0[1] = {0};
    REQUIRE(pmg_bg_plan_build(A.n, A.rp, A.ci, A.v, 0, bp0, NULL, 0, NULL, 0, NULL, &pl) == PMG_SUCCESS && pl.ntiles == 0 && pl.ncolors == 0);
    pmg_bg_plan_free(&pl);
    REQUIRE(pmg_bg_plan_build(0, bp0, NULL, NULL, 0, bp0, NULL, 0, NULL, 0, NULL, &pl) == PMG_SUCCESS);
    pmg_bg_plan_free(&pl);
    csr_free(&A);
  }
  /* 3. a one-sided pattern: row 0 stores an entry in column 5, row 5 stores none in column 0 -- still a conflict */
  {
    int32_t rp[7] = {0, 2, 3, 4, 5, 6, 7}, ci[7] = {0, 5, 1, 2, 3, 4, 5}, bp[3] = {0, 1, 2}, br[2] = {0, 5};
    double  v[7]  = {2.0, -0.5, 2.0, 2.0, 2.0, 2.0, 2.0};
    REQUIRE(pmg_bg_plan_build(6, rp, ci, v, 2, bp, br, 0, NULL, 0, NULL, &pl) == PMG_SUCCESS);
    REQUIRE(pl.ncolors == 2 && pl.colors[0] == 0 && pl.colors[1] == 1);
    pmg_bg_plan_free(&pl);
    int32_t same[2] = {0, 0}, rev[3] = {0, 1, 2}, brr[2] = {5, 0};
    REQUIRE(pmg_bg_plan_build(6, rp, ci, v, 2, bp, br, 1, same, 0, NULL, &pl) == PMG_ERR_ARG_WRONG);
    REQUIRE(pmg_bg_plan_build(6, rp, ci, v, 2, rev, brr, 1, same, 0, NULL, &pl) == PMG_ERR_ARG_WRONG); /* seen from the other block */
  }
  printf("blockgibbs_host ok\n");
  return 0;
}
