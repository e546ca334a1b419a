/* Host part of the coloured block Gibbs sampler (C11): what the reference does per patch inside PCASM's multiplicative loop
 * with a `cholsampler` sub-PC (examples/ex13.py:11-22) -- extracting A_PP, dpotrf('L') of it (src/pc_chols.c:174-194), keeping
 * the factor for the solves and the noise (src/pc_chols.c:220-260) -- done once for every block, plus what the device sweep
 * needs: a colouring of the blocks, the split of every block row into interior and exterior entries, and the packing of blocks
 * into wavefront tiles (kernels_blockgibbs.hip).  Host memory only: nothing here calls the HIP runtime or a kernel launcher, so
 * the file also runs in the stand-alone sanitizer program (tests/sanitize/blockgibbs_host.c).  Built with -ffp-contract=off:
 * every a * b + c below is two roundings, and the tests restate M = W^T W from the W this file returns. */
#include "pmg_internal.h"
#include <math.h>

void pmg_bg_plan_free(pmg_bg_plan *pl)
{
  free(pl->colors), free(pl->ctile), free(pl->tile_g), free(pl->tile_ew), free(pl->tile_foff), free(pl->tile_eoff);
  free(pl->pos), free(pl->slot), free(pl->M), free(pl->WT), free(pl->evals), free(pl->ecols);
  free(pl->woff), free(pl->W), free(pl->L), free(pl->slot_nint), free(pl->slot_next), free(pl->slot_tile_lane);
  memset(pl, 0, sizeof *pl);
}

static size_t at_least_one(int64_t k) { return (size_t)(k > 0 ? k : 1); }

pmg_status pmg_bg_check_blocks(int32_t n, int32_t nblocks, const int32_t *blockptr, const int32_t *blockrows)
{
  PMG_CHECK(n >= 0, PMG_ERR_ARG_OUTOFRANGE, "n = %d", n);
  PMG_CHECK(nblocks >= 0, PMG_ERR_ARG_OUTOFRANGE, "nblocks = %d", nblocks);
  PMG_CHECK(blockptr && (blockrows || blockptr[nblocks] == 0), PMG_ERR_ARG_NULL, "null block array");
  PMG_CHECK(blockptr[0] == 0, PMG_ERR_ARG_WRONG, "blockptr[0] = %d", blockptr[0]);
  for (int32_t p = 0; p < nblocks; ++p) {
    const int64_t m = (int64_t)blockptr[p + 1] - blockptr[p];
    PMG_CHECK(m > 0, PMG_ERR_ARG_OUTOFRANGE, "block %d is empty", p);
    PMG_CHECK(m <= PMG_BG_MAX_BLOCK, PMG_ERR_SUP, "block %d has %lld rows: at most %d are supported (the dense path of src/pc_chols.c:33-35)", p, (long long)m, PMG_BG_MAX_BLOCK);
  }
  int32_t *seen = (int32_t *)malloc(sizeof(int32_t) * at_least_one(n)); /* the last block that listed the row */
  PMG_CHECK(seen, PMG_ERR_MEM, "out of host memory");
  for (int32_t r = 0; r < n; ++r) seen[r] = -1;
  for (int32_t p = 0; p < nblocks; ++p)
    for (int32_t s = blockptr[p]; s < blockptr[p + 1]; ++s) {
      const int32_t r = blockrows[s];
      if (r < 0 || r >= n || seen[r] == p) {
        const int twice = r >= 0 && r < n;
        free(seen);
        if (twice) PMG_FAIL(PMG_ERR_ARG_OUTOFRANGE, "row %d is listed twice in block %d", r, p);
        PMG_FAIL(PMG_ERR_ARG_OUTOFRANGE, "row %d of block %d is outside [0, %d)", r, p, n);
      }
      seen[r] = p;
    }
  free(seen);
  return PMG_SUCCESS;
}

/* ---- the conflict graph ------------------------------------------------------------------------------------------------
   Blocks p and q conflict if they share a row, or if a row of one has a stored entry in a column of the other (either
   direction, so the transposed pattern is walked too).  visit(p, q, ctx) is called for every conflicting q != p, possibly
   several times. */
typedef struct {
  int32_t        n, nblocks;
  const int32_t *rowptr, *colidx, *blockptr, *blockrows;
  int32_t       *rb_ptr, *rb_idx; /* row -> the blocks that list it */
  int32_t       *tp_ptr, *tp_idx; /* column -> the rows that store an entry in it */
} bg_graph;

static void graph_free(bg_graph *g) { free(g->rb_ptr), free(g->rb_idx), free(g->tp_ptr), free(g->tp_idx); }

static pmg_status graph_build(bg_graph *g)
{
  const int32_t n = g->n, nslots = g->blockptr[g->nblocks], nnz = g->rowptr[n];
  g->rb_ptr = (int32_t *)calloc((size_t)n + 2, sizeof(int32_t));
  g->rb_idx = (int32_t *)malloc(sizeof(int32_t) * at_least_one(nslots));
  g->tp_ptr = (int32_t *)calloc((size_t)n + 2, sizeof(int32_t));
  g->tp_idx = (int32_t *)malloc(sizeof(int32_t) * at_least_one(nnz));
  PMG_CHECK(g->rb_ptr && g->rb_idx && g->tp_ptr && g->tp_idx, PMG_ERR_MEM, "out of host memory");
  /* counting sort, twice: offsets shifted by one so that the fill pass leaves rb_ptr[r] = first entry of row r */
  for (int32_t s = 0; s < nslots; ++s) ++g->rb_ptr[g->blockrows[s] + 2];
  for (int32_t k = 0; k < nnz; ++k) ++g->tp_ptr[g->colidx[k] + 2];
  for (int32_t r = 0; r < n; ++r) {
    g->rb_ptr[r + 2] += g->rb_ptr[r + 1];
    g->tp_ptr[r + 2] += g->tp_ptr[r + 1];
  }
  for (int32_t p = 0; p < g->nblocks; ++p)
    for (int32_t s = g->blockptr[p]; s < g->blockptr[p + 1]; ++s) g->rb_idx[g->rb_ptr[g->blockrows[s] + 1]++] = p;
  for (int32_t r = 0; r < n; ++r)
    for (int32_t k = g->rowptr[r]; k < g->rowptr[r + 1]; ++k) g->tp_idx[g->tp_ptr[g->colidx[k] + 1]++] = r;
  return PMG_SUCCESS;
}

typedef int (*bg_visit_fn)(int32_t p, int32_t q, void *ctx); /* nonzero stops the walk */

static int graph_row_blocks(const bg_graph *g, int32_t p, int32_t row, bg_visit_fn visit, void *ctx)
{
  for (int32_t t = g->rb_ptr[row]; t < g->rb_ptr[row + 1]; ++t)
    if (g->rb_idx[t] != p && visit(p, g->rb_idx[t], ctx)) return 1;
  return 0;
}

static int graph_neighbours(const bg_graph *g, int32_t p, bg_visit_fn visit, void *ctx)
{
  for (int32_t s = g->blockptr[p]; s < g->blockptr[p + 1]; ++s) {
    const int32_t r = g->blockrows[s];
    if (graph_row_blocks(g, p, r, visit, ctx)) return 1;
    for (int32_t k = g->rowptr[r]; k < g->rowptr[r + 1]; ++k)
      if (graph_row_blocks(g, p, g->colidx[k], visit, ctx)) return 1;
    for (int32_t k = g->tp_ptr[r]; k < g->tp_ptr[r + 1]; ++k)
      if (graph_row_blocks(g, p, g->tp_idx[k], visit, ctx)) return 1;
  }
  return 0;
}

typedef struct {
  const int32_t *colors;
  int32_t       *mark; /* first-fit: mark[c] = p when a coloured neighbour of p has colour c */
  int32_t        clash;
} bg_color_ctx;

static int visit_mark(int32_t p, int32_t q, void *ctx)
{
  bg_color_ctx *c = (bg_color_ctx *)ctx;
  if (c->colors[q] >= 0) c->mark[c->colors[q]] = p;
  return 0;
}

static int visit_check(int32_t p, int32_t q, void *ctx)
{
  bg_color_ctx *c = (bg_color_ctx *)ctx;
  if (c->colors[q] != c->colors[p]) return 0;
  c->clash = q;
  return 1;
}

static pmg_status color_blocks(const bg_graph *g, int32_t user_ncolors, const int32_t *user_colors, int32_t *colors, int32_t *ncolors)
{
  const int32_t nb = g->nblocks;
  bg_color_ctx  c  = {colors, NULL, -1};
  if (user_colors) {
    PMG_CHECK(user_ncolors >= 0, PMG_ERR_ARG_OUTOFRANGE, "ncolors = %d", user_ncolors);
    for (int32_t p = 0; p < nb; ++p) {
      PMG_CHECK(user_colors[p] >= 0 && user_colors[p] < user_ncolors, PMG_ERR_ARG_OUTOFRANGE, "colour %d of block %d is outside [0, %d)", user_colors[p], p, user_ncolors);
      colors[p] = user_colors[p];
    }
    *ncolors = user_ncolors;
  } else {
    c.mark = (int32_t *)malloc(sizeof(int32_t) * ((size_t)nb + 1));
    PMG_CHECK(c.mark, PMG_ERR_MEM, "out of host memory");
    for (int32_t p = 0; p <= nb; ++p) c.mark[p] = -1;
    for (int32_t p = 0; p < nb; ++p) colors[p] = -1;
    int32_t nc = 0;
    for (int32_t p = 0; p < nb; ++p) {
      graph_neighbours(g, p, visit_mark, &c);
      int32_t col = 0;
      while (c.mark[col] == p) ++col;
      colors[p] = col;
      if (col + 1 > nc) nc = col + 1;
    }
    free(c.mark);
    *ncolors = nc;
  }
  /* whatever the rule, like pmg_mcsor_setup: two blocks of one colour are swept in one launch */
  for (int32_t p = 0; p < nb; ++p)
    PMG_CHECK(!graph_neighbours(g, p, visit_check, &c), PMG_ERR_ARG_WRONG, "blocks %d and %d share a row or are coupled by a stored entry but share colour %d: the %s colouring is not a colouring of the blocks", p, c.clash, colors[p], user_colors ? "user" : "first-fit");
  return PMG_SUCCESS;
}

/* ---- one block: A_PP (lower triangle) -> L -> W = L^-1, all row-major m x m ------------------------------------------------ */
static pmg_status factor_block(int32_t p, int m, double *L, double *W)
{
  /* unblocked dpotrf('L'), column by column (dpotf2's order) */
  for (int j = 0; j < m; ++j) {
    double d = L[j * m + j];
    for (int k = 0; k < j; ++k) d = d - L[j * m + k] * L[j * m + k];
    PMG_CHECK(d > 0.0, PMG_ERR_MAT_CH_ZRPVT, "block %d: the leading minor of order %d is not positive definite (pivot %g)", p, j + 1, d); /* src/pc_chols.c:190; NaN fails too */
    const double ljj = sqrt(d);
    L[j * m + j]     = ljj;
    for (int i = j + 1; i < m; ++i) {
      double s = L[i * m + j];
      for (int k = 0; k < j; ++k) s = s - L[i * m + k] * L[j * m + k];
      L[i * m + j] = s / ljj;
    }
  }
  /* W = L^-1 by forward substitution on the columns of the identity */
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < m; ++i) {
      if (i < j) {
        W[i * m + j] = 0.0;
        continue;
      }
      double s = i == j ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s = s - L[i * m + k] * W[k * m + j];
      W[i * m + j] = s / L[i * m + i];
    }
  return PMG_SUCCESS;
}

static int padded_width(int m) { return m <= 8 ? 8 : m <= 16 ? 16 : m <= 32 ? 32 : 64; }

static pmg_status plan_build(const bg_graph *g, const double *vals, int32_t user_ncolors, const int32_t *user_colors, const int32_t *pos_of_row, pmg_bg_plan *pl)
{
  const int32_t n = g->n, nb = g->nblocks, nslots = g->blockptr[nb];
  pl->colors = (int32_t *)malloc(sizeof(int32_t) * at_least_one(nb));
  PMG_CHECK(pl->colors, PMG_ERR_MEM, "out of host memory");
  PMG_CALL(color_blocks(g, user_ncolors, user_colors, pl->colors, &pl->ncolors));
  const int32_t nc = pl->ncolors;

  /* tiles: inside a colour the blocks of padded width 8, then 16, 32, 64, each group in block order, 64 / g blocks per tile */
  int32_t *cnt = (int32_t *)calloc(at_least_one((int64_t)nc * 4), sizeof(int32_t)); /* blocks of (colour, width class) */
  int32_t *first = (int32_t *)calloc(at_least_one((int64_t)nc * 4) + 1, sizeof(int32_t)); /* first tile of the group */
  pl->ctile = (int32_t *)calloc((size_t)nc + 1, sizeof(int32_t));
  if (!cnt || !first || !pl->ctile) {
    free(cnt), free(first);
    PMG_FAIL(PMG_ERR_MEM, "out of host memory");
  }
#define WCLASS(m) ((m) <= 8 ? 0 : (m) <= 16 ? 1 : (m) <= 32 ? 2 : 3)
  for (int32_t p = 0; p < nb; ++p) ++cnt[pl->colors[p] * 4 + WCLASS(g->blockptr[p + 1] - g->blockptr[p])];
  for (int32_t q = 0; q < nc * 4; ++q) {
    const int per = 64 / (8 << (q & 3));
    first[q + 1]  = first[q] + (cnt[q] + per - 1) / per;
    cnt[q]        = 0; /* from here on: blocks of the group placed so far */
  }
  for (int32_t c = 0; c <= nc; ++c) pl->ctile[c] = first[c * 4];
  const int32_t ntiles = pl->ntiles = first[nc * 4];

  pl->tile_g         = (int32_t *)calloc(at_least_one(ntiles), sizeof(int32_t));
  pl->tile_ew        = (int32_t *)calloc(at_least_one(ntiles), sizeof(int32_t));
  pl->tile_foff      = (int64_t *)calloc((size_t)ntiles + 1, sizeof(int64_t));
  pl->tile_eoff      = (int64_t *)calloc((size_t)ntiles + 1, sizeof(int64_t));
  pl->pos            = (int32_t *)malloc(sizeof(int32_t) * at_least_one((int64_t)ntiles * 64));
  pl->slot           = (int32_t *)calloc(at_least_one((int64_t)ntiles * 64), sizeof(int32_t));
  pl->woff           = (int64_t *)calloc((size_t)nb + 1, sizeof(int64_t));
  pl->slot_nint      = (int32_t *)calloc(at_least_one(nslots), sizeof(int32_t));
  pl->slot_next      = (int32_t *)calloc(at_least_one(nslots), sizeof(int32_t));
  pl->slot_tile_lane = (int32_t *)calloc(at_least_one(nslots), sizeof(int32_t));
  int32_t *loc       = (int32_t *)malloc(sizeof(int32_t) * at_least_one(n)); /* local index of a row in the current block, else -1 */
  if (!pl->tile_g || !pl->tile_ew || !pl->tile_foff || !pl->tile_eoff || !pl->pos || !pl->slot || !pl->woff || !pl->slot_nint || !pl->slot_next || !pl->slot_tile_lane || !loc) {
    free(cnt), free(first), free(loc);
    PMG_FAIL(PMG_ERR_MEM, "out of host memory");
  }
  for (int64_t t = 0; t < (int64_t)ntiles * 64; ++t) pl->pos[t] = -1;
  for (int32_t r = 0; r < n; ++r) loc[r] = -1;

  /* place the blocks; count interior and exterior entries; tile widths */
  for (int32_t p = 0; p < nb; ++p) {
    const int32_t s0 = g->blockptr[p], m = g->blockptr[p + 1] - s0;
    const int     q = pl->colors[p] * 4 + WCLASS(m), gw = padded_width(m), per = 64 / gw;
    const int32_t tile = first[q] + cnt[q] / per, lane0 = (cnt[q] % per) * gw;
    ++cnt[q];
    pl->tile_g[tile] = gw;
    pl->woff[p + 1]  = pl->woff[p] + (int64_t)m * m;
    for (int32_t i = 0; i < m; ++i) loc[g->blockrows[s0 + i]] = i;
    for (int32_t i = 0; i < m; ++i) {
      const int32_t r = g->blockrows[s0 + i], tl = tile * 64 + lane0 + i;
      pl->pos[tl]                = pos_of_row ? pos_of_row[r] : r;
      pl->slot[tl]               = s0 + i;
      pl->slot_tile_lane[s0 + i] = tl;
      int32_t ni = 0;
      for (int32_t k = g->rowptr[r]; k < g->rowptr[r + 1]; ++k) ni += loc[g->colidx[k]] >= 0;
      pl->slot_nint[s0 + i] = ni;
      pl->slot_next[s0 + i] = g->rowptr[r + 1] - g->rowptr[r] - ni;
      pl->nnz_ext += pl->slot_next[s0 + i];
      if (pl->slot_next[s0 + i] > pl->tile_ew[tile]) pl->tile_ew[tile] = pl->slot_next[s0 + i];
    }
    for (int32_t i = 0; i < m; ++i) loc[g->blockrows[s0 + i]] = -1;
  }
#undef WCLASS
  free(cnt), free(first);
  for (int32_t t = 0; t < ntiles; ++t) {
    pl->tile_foff[t + 1] = pl->tile_foff[t] + (int64_t)pl->tile_g[t] * 64;
    pl->tile_eoff[t + 1] = pl->tile_eoff[t] + (int64_t)pl->tile_ew[t] * 64;
  }
  const int64_t ftot = pl->tile_foff[ntiles], etot = pl->tile_eoff[ntiles], wtot = pl->woff[nb];
  pl->M     = (double *)calloc(at_least_one(ftot), sizeof(double));
  pl->WT    = (double *)calloc(at_least_one(ftot), sizeof(double));
  pl->evals = (double *)calloc(at_least_one(etot), sizeof(double));
  pl->ecols = (int32_t *)malloc(sizeof(int32_t) * at_least_one(etot));
  pl->W     = (double *)calloc(at_least_one(wtot), sizeof(double));
  pl->L     = (double *)calloc(at_least_one(wtot), sizeof(double));
  if (!pl->M || !pl->WT || !pl->evals || !pl->ecols || !pl->W || !pl->L) {
    free(loc);
    PMG_FAIL(PMG_ERR_MEM, "out of host memory");
  }
  /* pad entries of the exterior part: value 0 at the lane's own position, in lanes without a row at the tile's first row's
     (lane 0 of a tile always has one) */
  for (int32_t t = 0; t < ntiles; ++t)
    for (int32_t j = 0; j < pl->tile_ew[t]; ++j)
      for (int l = 0; l < 64; ++l) pl->ecols[pl->tile_eoff[t] + (int64_t)j * 64 + l] = pl->pos[t * 64 + l] >= 0 ? pl->pos[t * 64 + l] : pl->pos[t * 64];

  pmg_status st = PMG_SUCCESS;
  for (int32_t p = 0; p < nb && !st; ++p) {
    const int32_t s0 = g->blockptr[p], m = g->blockptr[p + 1] - s0;
    double       *L = pl->L + pl->woff[p], *W = pl->W + pl->woff[p];
    for (int32_t i = 0; i < m; ++i) loc[g->blockrows[s0 + i]] = i;
    for (int32_t i = 0; i < m; ++i) {
      const int32_t r = g->blockrows[s0 + i], tl = pl->slot_tile_lane[s0 + i], t = tl / 64, l = tl % 64;
      int32_t       je = 0;
      for (int32_t k = g->rowptr[r]; k < g->rowptr[r + 1]; ++k) {
        const int32_t c = g->colidx[k], j = loc[c];
        if (j >= 0) {
          if (j <= i) L[i * m + j] = vals[k]; /* the lower triangle only, as dpotrf('L') reads it */
        } else {
          pl->evals[pl->tile_eoff[t] + (int64_t)je * 64 + l] = vals[k];
          pl->ecols[pl->tile_eoff[t] + (int64_t)je * 64 + l] = pos_of_row ? pos_of_row[c] : c;
          ++je;
        }
      }
    }
    for (int32_t i = 0; i < m; ++i) loc[g->blockrows[s0 + i]] = -1;
    st = factor_block(p, m, L, W);
    if (st) break;
    /* the lane of local row i holds row i of M = W^T W and of W^T, entry j at foff + j * 64 + lane */
    const int32_t tl0 = pl->slot_tile_lane[s0], t = tl0 / 64;
    for (int32_t i = 0; i < m; ++i)
      for (int32_t j = 0; j < m; ++j) {
        double acc = 0.0;
        for (int32_t k = 0; k < m; ++k) acc = acc + W[k * m + i] * W[k * m + j];
        const int64_t e = pl->tile_foff[t] + (int64_t)j * 64 + tl0 % 64 + i;
        pl->M[e]        = acc;
        pl->WT[e]       = W[j * m + i];
      }
  }
  free(loc);
  return st;
}

pmg_status pmg_bg_plan_build(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, int32_t nblocks, const int32_t *blockptr, const int32_t *blockrows, int32_t user_ncolors, const int32_t *user_colors, int32_t ld, const int32_t *pos_of_row, pmg_bg_plan *pl)
{
  memset(pl, 0, sizeof *pl);
  PMG_CALL(pmg_bg_check_blocks(n, nblocks, blockptr, blockrows));
  PMG_CHECK(rowptr && (colidx || rowptr[n] == 0) && (vals || rowptr[n] == 0), PMG_ERR_ARG_NULL, "null CSR array");
  PMG_CHECK(rowptr[0] == 0, PMG_ERR_ARG_WRONG, "rowptr[0] = %d", rowptr[0]);
  for (int32_t r = 0; r < n; ++r) {
    PMG_CHECK(rowptr[r + 1] >= rowptr[r], PMG_ERR_ARG_WRONG, "rowptr not monotone at row %d", r);
    for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) PMG_CHECK(colidx[k] >= 0 && colidx[k] < n, PMG_ERR_ARG_OUTOFRANGE, "column %d out of range in row %d", colidx[k], r);
  }
  if (pos_of_row) {
    PMG_CHECK(ld >= n, PMG_ERR_ARG_OUTOFRANGE, "layout length %d for %d rows", ld, n);
    unsigned char *used = (unsigned char *)calloc(at_least_one(ld), 1);
    PMG_CHECK(used, PMG_ERR_MEM, "out of host memory");
    for (int32_t r = 0; r < n; ++r) {
      const int32_t q = pos_of_row[r];
      if (q < 0 || q >= ld || used[q]) {
        free(used);
        PMG_FAIL(q < 0 || q >= ld ? PMG_ERR_ARG_OUTOFRANGE : PMG_ERR_ARG_WRONG, "position %d of row %d is outside [0, %d) or taken by another row", q, r, ld);
      }
      used[q] = 1;
    }
    free(used);
  }
  pl->n       = n;
  pl->ld      = pos_of_row ? ld : n;
  pl->nblocks = nblocks;
  pl->nslots  = blockptr[nblocks];
  bg_graph   g  = {n, nblocks, rowptr, colidx, blockptr, blockrows, NULL, NULL, NULL, NULL};
  pmg_status st = graph_build(&g);
  if (!st) st = plan_build(&g, vals, user_ncolors, user_colors, pos_of_row, pl);
  graph_free(&g);
  if (st) pmg_bg_plan_free(pl);
  return st;
}
