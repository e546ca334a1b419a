/* Host sparse tools of the MGMC set-up (C11): what PETSc does on the host for PCGAMGMC's geometric hierarchy --
 * DMCreateInterpolation's Q1 interpolation, R = P^T, the Galerkin product A_c = P^T A P (-pc_mg_galerkin both, injected at
 * src/pc_gamgmc.c:345-349), B_{l-1} = P_l^T B_l (src/pc_gamgmc.c:177) -- and the class-stencil form of the resulting 27-point
 * operators.  Host memory only: nothing here calls the HIP runtime or a kernel launcher, so the file also runs in the
 * stand-alone sanitizer program (tests/sanitize/host_san.c). */
#include "pmg_mgmc_internal.h"

void pmg_hcsr_free(hcsr *m)
{
  free(m->rp);
  free(m->ci);
  free(m->v);
  memset(m, 0, sizeof *m);
}

/* nr x nc with room for nnz entries; rowptr zeroed */
static pmg_status hcsr_alloc(hcsr *m, int64_t nr, int64_t nc, int64_t nnz)
{
  m->nr = (int32_t)nr;
  m->nc = (int32_t)nc;
  m->rp = (int32_t *)calloc((size_t)nr + 1, sizeof(int32_t));
  m->ci = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1));
  m->v  = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
  PMG_CHECK(m->rp && m->ci && m->v, PMG_ERR_MEM, "out of host memory");
  return PMG_SUCCESS;
}

pmg_status pmg_hcsr_dup(const hcsr *A, hcsr *out)
{
  const size_t nnz = (size_t)A->rp[A->nr];
  PMG_CALL(hcsr_alloc(out, A->nr, A->nc, (int64_t)nnz));
  memcpy(out->rp, A->rp, sizeof(int32_t) * ((size_t)A->nr + 1));
  memcpy(out->ci, A->ci, sizeof(int32_t) * nnz);
  memcpy(out->v, A->v, sizeof(double) * nnz);
  return PMG_SUCCESS;
}

/* Q1 interpolation from the (ncx,ncy,ncz) grid to the (nfx,nfy,nfz) grid, natural ordering, columns ascending.
   Per direction: fine 2I coincides with coarse I (weight 1), fine 2I+1 lies midway (1/2, 1/2); a direction with
   one point is not coarsened. */
pmg_status pmg_hier_q1_interp(const int32_t nf[3], const int32_t nc[3], hcsr *P)
{
  const int64_t nrow = (int64_t)nf[0] * nf[1] * nf[2];
  /* count */
  int64_t nnz = 0;
  int64_t cnt[3][2]; /* per direction: number of fine points with 1 / 2 contributions */
  for (int d = 0; d < 3; ++d) {
    if (nf[d] == nc[d]) {
      cnt[d][0] = nf[d];
      cnt[d][1] = 0;
    } else {
      cnt[d][0] = (nf[d] + 1) / 2;
      cnt[d][1] = nf[d] / 2;
    }
  }
  nnz   = (cnt[0][0] + 2 * cnt[0][1]) * (cnt[1][0] + 2 * cnt[1][1]) * (cnt[2][0] + 2 * cnt[2][1]);
  PMG_CALL(hcsr_alloc(P, nrow, nc[0] * nc[1] * nc[2], nnz));
  int64_t p = 0;
  for (int k = 0; k < nf[2]; ++k)
    for (int j = 0; j < nf[1]; ++j)
      for (int i = 0; i < nf[0]; ++i) {
        const int f[3] = {i, j, k};
        int       c0[3], m[3];
        double    w[3][2];
        for (int d = 0; d < 3; ++d) {
          if (nf[d] == nc[d]) { c0[d] = f[d]; m[d] = 1; w[d][0] = 1.0; }
          else if ((f[d] & 1) == 0) { c0[d] = f[d] / 2; m[d] = 1; w[d][0] = 1.0; }
          else { c0[d] = f[d] / 2; m[d] = 2; w[d][0] = 0.5; w[d][1] = 0.5; }
        }
        P->rp[i + (int64_t)nf[0] * (j + (int64_t)nf[1] * k)] = (int32_t)p;
        for (int c = 0; c < m[2]; ++c)
          for (int bq = 0; bq < m[1]; ++bq)
            for (int a = 0; a < m[0]; ++a) {
              P->ci[p] = (c0[0] + a) + nc[0] * ((c0[1] + bq) + nc[1] * (c0[2] + c));
              P->v[p]  = w[0][a] * w[1][bq] * w[2][c];
              ++p;
            }
      }
  P->rp[nrow] = (int32_t)p;
  return PMG_SUCCESS;
}

pmg_status pmg_hcsr_transpose(const hcsr *A, hcsr *T)
{
  const int32_t nnz = A->rp[A->nr];
  PMG_CALL(hcsr_alloc(T, A->nc, A->nr, nnz));
  for (int32_t k = 0; k < nnz; ++k) T->rp[A->ci[k] + 1]++;
  for (int32_t r = 0; r < T->nr; ++r) T->rp[r + 1] += T->rp[r];
  int32_t *fill = (int32_t *)malloc(sizeof(int32_t) * (size_t)(T->nr > 0 ? T->nr : 1));
  PMG_CHECK(fill, PMG_ERR_MEM, "out of host memory");
  memcpy(fill, T->rp, sizeof(int32_t) * (size_t)T->nr);
  for (int32_t r = 0; r < A->nr; ++r)
    for (int32_t k = A->rp[r]; k < A->rp[r + 1]; ++k) {
      const int32_t q = fill[A->ci[k]]++;
      T->ci[q]        = r;
      T->v[q]         = A->v[k];
    }
  free(fill);
  return PMG_SUCCESS;
}

void pmg_hier_laplace_rows(int32_t nx, int32_t ny, int32_t nz, double kappa, double h2, rowsrc *s)
{
  memset(s, 0, sizeof *s);
  s->nx    = nx;
  s->ny    = ny;
  s->nz    = nz;
  s->kappa = kappa;
  s->h2    = h2;
  for (int nn = 0; nn < 8; ++nn) {
    double dgl = kappa * kappa;
    for (int q = 0; q < nn; ++q) dgl += h2;
    s->diag[nn] = dgl;
  }
}

/* row `row` into cols/vals (room for maxrow entries); its length, or -1 when it does not fit */
static int rowsrc_get(const rowsrc *s, int32_t row, int maxrow, int32_t *cols, double *vals)
{
  if (s->A) {
    const int32_t a = s->A->rp[row], n = s->A->rp[row + 1] - a;
    if (n > maxrow) return -1;
    memcpy(cols, s->A->ci + a, sizeof(int32_t) * (size_t)n);
    memcpy(vals, s->A->v + a, sizeof(double) * (size_t)n);
    return n;
  }
  if (maxrow < 7) return -1;
  const int32_t i = row % s->nx, j = (row / s->nx) % s->ny, k = row / (s->nx * s->ny);
  int           n = 0, nn = (k > 0) + (j > 0) + (i > 0) + (i < s->nx - 1) + (j < s->ny - 1) + (k < s->nz - 1);
  if (k > 0) { cols[n] = row - s->nx * s->ny; vals[n++] = -s->h2; }
  if (j > 0) { cols[n] = row - s->nx; vals[n++] = -s->h2; }
  if (i > 0) { cols[n] = row - 1; vals[n++] = -s->h2; }
  cols[n] = row; vals[n++] = s->diag[nn];
  if (i < s->nx - 1) { cols[n] = row + 1; vals[n++] = -s->h2; }
  if (j < s->ny - 1) { cols[n] = row + s->nx; vals[n++] = -s->h2; }
  if (k < s->nz - 1) { cols[n] = row + s->nx * s->ny; vals[n++] = -s->h2; }
  return n;
}

static int cmp_i32(const void *a, const void *b) { return (*(const int32_t *)a > *(const int32_t *)b) - (*(const int32_t *)a < *(const int32_t *)b); }

/* C = P^T A P, fused: for coarse row I, for i in R_I, for (j,a) in A_i, for (J,p) in P_j: C[I,J] += r a p */
typedef struct {
  double  *d; /* acc[nc], vals[maxrow] */
  int32_t *i; /* mark[nc], list[nc], cols[maxrow] */
} rap_work;

static pmg_status rap_rows(const rowsrc *A, int maxrow, const hcsr *P, const hcsr *R, hcsr *Cm, rap_work *w)
{
  const int32_t nc  = P->nc;
  size_t        cap = (size_t)nc * 32 + 64;
  const size_t  mr  = (size_t)(maxrow > 0 ? maxrow : 0);
  PMG_CALL(hcsr_alloc(Cm, nc, nc, (int64_t)cap));
  w->d = (double *)calloc((size_t)nc + mr + 1, sizeof(double));
  w->i = (int32_t *)malloc(sizeof(int32_t) * (2 * (size_t)nc + mr + 1));
  PMG_CHECK(w->d && w->i, PMG_ERR_MEM, "out of host memory in the Galerkin product");
  double  *acc = w->d, *vals = w->d + nc;
  int32_t *mark = w->i, *list = mark + nc, *cols = list + nc;
  for (int32_t q = 0; q < nc; ++q) mark[q] = -1;
  size_t nnz = 0;
  for (int32_t I = 0; I < nc; ++I) {
    int32_t nl = 0;
    for (int32_t kr = R->rp[I]; kr < R->rp[I + 1]; ++kr) {
      const int32_t i  = R->ci[kr];
      const double  rv = R->v[kr];
      const int     na = rowsrc_get(A, i, maxrow, cols, vals);
      PMG_CHECK(na >= 0, PMG_ERR_ARG_SIZ, "row %d of the fine operator has more than %d entries", i, maxrow);
      for (int ka = 0; ka < na; ++ka) {
        const int32_t j  = cols[ka];
        const double  ra = rv * vals[ka];
        for (int32_t kp = P->rp[j]; kp < P->rp[j + 1]; ++kp) {
          const int32_t J = P->ci[kp];
          if (mark[J] != I) {
            mark[J]    = I;
            list[nl++] = J;
            acc[J]     = 0.0;
          }
          acc[J] += ra * P->v[kp];
        }
      }
    }
    qsort(list, (size_t)nl, sizeof(int32_t), cmp_i32);
    if (nnz + (size_t)nl > cap) {
      cap          = (cap + (size_t)nl) * 2;
      int32_t *ci2 = (int32_t *)realloc(Cm->ci, sizeof(int32_t) * cap);
      if (ci2) Cm->ci = ci2;
      double *v2 = (double *)realloc(Cm->v, sizeof(double) * cap);
      if (v2) Cm->v = v2;
      PMG_CHECK(ci2 && v2, PMG_ERR_MEM, "out of host memory in the Galerkin product");
    }
    for (int32_t q = 0; q < nl; ++q) {
      Cm->ci[nnz] = list[q];
      Cm->v[nnz]  = acc[list[q]];
      ++nnz;
    }
    PMG_CHECK(nnz < 2147483647u, PMG_ERR_ARG_OUTOFRANGE, "coarse operator exceeds 32-bit nonzero count");
    Cm->rp[I + 1] = (int32_t)nnz;
  }
  return PMG_SUCCESS;
}

pmg_status pmg_hier_galerkin_rap(const rowsrc *A, int maxrow, const hcsr *P, const hcsr *R, hcsr *Cm)
{
  rap_work         w  = {NULL, NULL};
  const pmg_status st = rap_rows(A, maxrow, P, R, Cm, &w);
  free(w.d);
  free(w.i);
  return st;
}

/* Bc = R Bf = P^T Bf column by column (MatTransposeMatMult(Ip, Bf), src/pc_gamgmc.c:177) */
pmg_status pmg_hier_restrict_B(const hcsr *R, int32_t k, int32_t nf, const double *Bf, double **Bc_out)
{
  double *Bc = (double *)malloc(sizeof(double) * (size_t)R->nr * k);
  PMG_CHECK(Bc, PMG_ERR_MEM, "out of host memory");
  for (int32_t c = 0; c < k; ++c) {
    const double *bf = Bf + (size_t)nf * c;
    double       *bc = Bc + (size_t)R->nr * c;
    for (int32_t r = 0; r < R->nr; ++r) {
      double acc = 0.0;
      for (int32_t q = R->rp[r]; q < R->rp[r + 1]; ++q) acc += R->v[q] * bf[R->ci[q]];
      bc[r] = acc;
    }
  }
  *Bc_out = Bc;
  return PMG_SUCCESS;
}

/* Try to express the CSR operator of a structured level as 27 position-class stencils; returns 1 if every row equals
   its class stencil bit for bit (always the case for Galerkin operators of the constant-coefficient fine operator),
   0 otherwise (the caller keeps the sliced-ELL form). */
/* class-stencil table of a structured 27-point (9-point) matrix on an nx*ny*nz grid: coef[27*cls + e] and which
   classes occur; returns 0 when the matrix is not of that form (a row is not the full in-domain 27-box, or two points
   of one position class have different rows) */
int pmg_hier_st27_extract(int nx, int ny, int nz, const hcsr *A, double *coef /* [27*27] */, int *have /* [27] */)
{
  memset(coef, 0, sizeof(double) * 27 * 27);
  memset(have, 0, sizeof(int) * 27);
  for (int32_t k = 0; k < nz; ++k)
    for (int32_t j = 0; j < ny; ++j)
      for (int32_t i = 0; i < nx; ++i) {
        const int32_t row = i + nx * (j + ny * k);
        const int     cls = (i == 0 ? 0 : (i == nx - 1 ? 2 : 1)) + 3 * (j == 0 ? 0 : (j == ny - 1 ? 2 : 1)) + 9 * (k == 0 ? 0 : (k == nz - 1 ? 2 : 1));
        double        loc[27];
        memset(loc, 0, sizeof loc);
        int32_t expect = 0;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx)
              if (i + dx >= 0 && i + dx < nx && j + dy >= 0 && j + dy < ny && k + dz >= 0 && k + dz < nz) ++expect;
        if (A->rp[row + 1] - A->rp[row] != expect) return 0; /* not the full in-domain 27-box */
        for (int32_t q = A->rp[row]; q < A->rp[row + 1]; ++q) {
          const int32_t c = A->ci[q], ci = c % nx, cj = (c / nx) % ny, ck = c / (nx * ny);
          const int     dx = ci - i, dy = cj - j, dz = ck - k;
          if (dx < -1 || dx > 1 || dy < -1 || dy > 1 || dz < -1 || dz > 1) return 0;
          loc[9 * (dz + 1) + 3 * (dy + 1) + (dx + 1)] = A->v[q];
        }
        if (!have[cls]) {
          memcpy(coef + 27 * cls, loc, sizeof loc);
          have[cls] = 1;
        } else if (memcmp(coef + 27 * cls, loc, sizeof loc) != 0) {
          return 0;
        }
      }
  return 1;
}

/* ---- hierarchy from class-stencil tables ----------------------------------------------------------------------
   The Galerkin operators of the constant-coefficient grid operator are class stencils whose 27 x 27 tables do not
   depend on the grid size, so they are computed on a small PROXY hierarchy with the same coefficients (same kappa,
   same h2 = 1/(nx-1)^2 of the true grid, as many levels, 2^levels + 1 points per refined direction at most): the
   Galerkin products of the true 10^7..10^8-row matrices never have to be formed, and a z-slab of a multi-device run
   needs nothing but its own planes.  Bit-identical to the tables extracted from the full products (the same entries
   are summed in the same order for every point of a class; tests compare both set-ups).
   dims[l] = the true extents of level l (0 = coarsest), h2 the TRUE grid's 1/(nx-1)^2 (src/problems.c:24); *ok = 0
   when the grid has no such proxy or an operator is not a class stencil (the caller forms the full products). */
static pmg_status proxy_tables(int nlevels, const int32_t (*dims)[3], double kappa, double h2, st27_table *tab, int *ok, hcsr *w /* [4], the caller's to free */)
{
  hcsr *P = &w[0], *R = &w[1], *Ac = &w[2], *Aprev = &w[3];
  const int top = nlevels - 1;
  int32_t   pd[64][3];
  PMG_CHECK(nlevels >= 2 && nlevels <= 64, PMG_ERR_ARG_OUTOFRANGE, "%d levels", nlevels);
  for (int q = 0; q < 3; ++q) {
    const int32_t tn  = dims[top][q];
    const int64_t cap = ((int64_t)1 << (nlevels < 20 ? nlevels : 20)) + 1;
    pd[top][q]        = tn == 1 ? 1 : (int32_t)(tn < cap ? tn : cap);
  }
  for (int l = top; l >= 1; --l)
    for (int q = 0; q < 3; ++q) pd[l - 1][q] = dims[l][q] == dims[l - 1][q] ? pd[l][q] : (pd[l][q] - 1) / 2 + 1; /* coarsened in the true hierarchy <=> coarsened here */
  for (int l = top; l >= 0; --l) /* every position class of the true level must exist on the proxy level */
    for (int q = 0; q < 3; ++q)
      if (pd[l][q] != dims[l][q] && pd[l][q] < 3) return PMG_SUCCESS;
  rowsrc src;
  pmg_hier_laplace_rows(pd[top][0], pd[top][1], pd[top][2], kappa, h2, &src);
  int good = 1;
  for (int l = top; l >= 1 && good; --l) {
    PMG_CALL(pmg_hier_q1_interp(pd[l], pd[l - 1], P));
    PMG_CALL(pmg_hcsr_transpose(P, R));
    rowsrc sl = src;
    if (l < top) sl.A = Aprev;
    PMG_CALL(pmg_hier_galerkin_rap(&sl, l == top ? 7 : 64, P, R, Ac));
    good = pmg_hier_st27_extract(pd[l - 1][0], pd[l - 1][1], pd[l - 1][2], Ac, tab[l - 1].coef, tab[l - 1].have);
    pmg_hcsr_free(P);
    pmg_hcsr_free(R);
    pmg_hcsr_free(Aprev);
    hcsr_move(Aprev, Ac);
  }
  *ok = good;
  return PMG_SUCCESS;
}

pmg_status pmg_hier_stencil_tables(int nlevels, const int32_t (*dims)[3], double kappa, double h2, st27_table *tab /* [nlevels-1], level l < top */, int *ok)
{
  hcsr w[4];
  memset(w, 0, sizeof w);
  *ok                 = 0;
  const pmg_status st = proxy_tables(nlevels, dims, kappa, h2, tab, ok, w);
  for (int q = 0; q < 4; ++q) pmg_hcsr_free(&w[q]);
  return st;
}

/* assembled CSR of a class-stencil operator on the full nx*ny*nz grid (for the dense coarse factorisation) */
pmg_status pmg_hier_st27_to_csr(int nx, int ny, int nz, const st27_table *t, hcsr *A)
{
  const int32_t n = nx * ny * nz;
  PMG_CALL(hcsr_alloc(A, n, n, (int64_t)n * 27));
  int32_t nnz = 0;
  for (int32_t k = 0; k < nz; ++k)
    for (int32_t j = 0; j < ny; ++j)
      for (int32_t i = 0; i < nx; ++i) {
        const int32_t row = i + nx * (j + ny * k);
        const int     cls = (i == 0 ? 0 : (i == nx - 1 ? 2 : 1)) + 3 * (j == 0 ? 0 : (j == ny - 1 ? 2 : 1)) + 9 * (k == 0 ? 0 : (k == nz - 1 ? 2 : 1));
        A->rp[row]        = nnz;
        int e             = 0;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx, ++e)
              if (i + dx >= 0 && i + dx < nx && j + dy >= 0 && j + dy < ny && k + dz >= 0 && k + dz < nz) {
                A->ci[nnz]  = row + dx + nx * (dy + ny * dz);
                A->v[nnz++] = t->coef[27 * cls + e];
              }
      }
  A->rp[n] = nnz;
  return PMG_SUCCESS;
}

/* parity colouring (i&1) + 2(j&1) + 4(k&1), compressed to consecutive colours: valid for the 9/27-point box (red-black is
   not a valid colouring of a 27-point stencil) */
void pmg_hier_parity_colouring(int32_t nx, int32_t ny, int32_t nz, int32_t *col)
{
  int present[8] = {0}, remap[8], ncol = 0;
  for (int32_t k = 0; k < nz; ++k)
    for (int32_t j = 0; j < ny; ++j)
      for (int32_t i = 0; i < nx; ++i) present[(i & 1) + 2 * (j & 1) + 4 * (k & 1)] = 1;
  for (int q = 0; q < 8; ++q) remap[q] = present[q] ? ncol++ : -1;
  for (int32_t k = 0; k < nz; ++k)
    for (int32_t j = 0; j < ny; ++j)
      for (int32_t i = 0; i < nx; ++i) col[i + nx * (j + ny * k)] = remap[(i & 1) + 2 * (j & 1) + 4 * (k & 1)];
}
