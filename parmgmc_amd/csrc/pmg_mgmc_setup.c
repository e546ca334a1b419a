/* Multigrid Monte Carlo sampler: handle construction, options and the set-up of the hierarchy -- host side (C11).
 *
 * Three set-up routines behind pmg_mgmc_setup, each a body that owns its temporaries through one setup_scratch:
 *   setup_user_body      a hierarchy handed over level by level (whole or by row blocks): sliced-ELL levels, CSR transfers
 *   setup_stencil_body   DMDA default: class-stencil tables from the proxy hierarchy, matrix-free Q1 transfers, z-slabs
 *   setup_galerkin_body  DMDA with the full Galerkin products on the host (keep_host, PMG_MG_FULL_GALERKIN / _NO_STENCIL /
 *                        _CSR_TRANSFERS, or a grid whose coarse operators are no class stencils)
 * Each body gives every level its kind and transfer kind (mg_kind, mg_transfer) where it builds the level; nothing assigns them
 * afterwards.  The setters write the inputs h->in, the bodies read them, pmg_mgmc_i_free_inputs releases them after a successful
 * set-up.  The host sparse tools they call are in pmg_hier_host.c, the cycle that runs on the result in pmg_mgmc.c.
 */
#include "pmg_mgmc_internal.h"
#include <math.h>

/* a handle of `levels` empty levels with PCGAMGMC's defaults */
static pmg_status mgmc_alloc(int32_t levels, pmg_mgmc *out)
{
  pmg_mgmc h = (pmg_mgmc)calloc(1, sizeof *h);
  PMG_CHECK(h, PMG_ERR_MEM, "out of host memory");
  h->lv = (mg_level *)calloc((size_t)levels, sizeof(mg_level));
  h->in = (mg_level_in *)calloc((size_t)levels, sizeof(mg_level_in));
  if (!h->lv || !h->in) {
    free(h->lv);
    free(h->in);
    free(h);
    PMG_FAIL(PMG_ERR_MEM, "out of host memory");
  }
  h->nlevels     = levels;
  h->omega       = 1.0;
  h->nu          = 1;                     /* -mg_levels_ksp_max_it 1, src/pc_gamgmc.c:324-328 */
  h->scaled      = 0;                     /* -mg_levels_pc_type sorgibbs, :330-334            */
  h->sweep_type  = PMG_SOR_FORWARD_SWEEP;
  h->coarse_type = 0;                     /* -mg_coarse_pc_type cholsampler, :336-342         */
  h->coarse_its  = 1;
  *out           = h;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_create_dmda(int32_t nx, int32_t ny, int32_t nz, double kappa, int32_t levels, pmg_mgmc *out)
{
  PMG_CHECK(out, PMG_ERR_ARG_NULL, "null output handle");
  *out = NULL;
  PMG_CHECK(levels >= 2, PMG_ERR_ARG_OUTOFRANGE, "need at least 2 levels (got %d)", levels);
  PMG_CHECK(nx >= 3 && ny >= 1 && nz >= 1, PMG_ERR_ARG_OUTOFRANGE, "grid %d x %d x %d", nx, ny, nz);
  pmg_mgmc h;
  PMG_CALL(mgmc_alloc(levels, &h));
  h->kappa = kappa;
  int32_t d[3]   = {nx, ny, nz};
  for (int l = levels - 1; l >= 0; --l) {
    h->lv[l].nx = d[0];
    h->lv[l].ny = d[1];
    h->lv[l].nz = d[2];
    h->lv[l].n  = d[0] * d[1] * d[2];
    h->lv[l].nzl = d[2];
    if (l > 0)
      for (int q = 0; q < 3; ++q)
        if (d[q] > 1) {
          if ((d[q] - 1) % 2 != 0 || d[q] < 3) {
            const int32_t bad = d[q];
            free(h->lv);
            free(h->in);
            free(h);
            PMG_FAIL(PMG_ERR_ARG_SIZ, "level %d has %d points in direction %d: vertex-centred 2:1 coarsening needs (n-1) even and n >= 3 on every refined level (use 2^k+1 points)", l, bad, q);
          }
          d[q] = (d[q] - 1) / 2 + 1;
        }
  }
  h->n_io = nx * ny * nz;
  *out    = h;
  return PMG_SUCCESS;
}

/* The same sampler on z-slabs of the DMDA, one rank per device (the reference distributes every PCMG
   level over all MPI ranks and lets GAMG reduce the coarse grids to rank 0, src/pc_chols.c:38-47,272-282):
     - `g` is this rank's slab of the fine operator (pmg_grid_create with kz0 = cuts[rank], nz = cuts[rank+1] - kz0),
       `dist` the halo transport created on it; both stay the caller's;
     - a coarse plane K belongs to the owner of fine plane 2K, so coarse levels inherit the partition with no data
       motion; per level and cycle there is the sweeps' halo (one plane per z-parity phase and side) and one halo of
       the residual for the restriction; the prolongation also fills the fine ghost planes, from the coarse ghost
       planes, so it needs no exchange;
     - levels with at most PMG_MG_REPLICATE_BELOW (default 2^19) unknowns, or with fewer planes than ranks, are
       REPLICATED: their right-hand side is all-gathered once and every rank runs the remaining coarse part of the
       cycle redundantly -- the noise is a function of (seed, counter, global index), so all ranks compute the same
       bits and no scatter is needed on the way up.
   Samples are bit-identical to the single-device sampler for any number of ranks. */
pmg_status pmg_mgmc_create_dmda_slab(int32_t nx, int32_t ny, int32_t nz, double kappa, int32_t levels, pmg_grid g, pmg_dist dist, const int32_t *cuts, pmg_mgmc *out)
{
  PMG_CHECK(out && g && dist && cuts, PMG_ERR_ARG_NULL, "null argument");
  PMG_CALL(pmg_mgmc_create_dmda(nx, ny, nz, kappa, levels, out));
  pmg_mgmc   h  = *out;
  pmg_status st = pmg_dist_get_info(dist, &h->rank, &h->nranks, NULL);
  pmgk_grid_layout L;
  if (!st) st = pmg_grid_get_kernel_layout(g, &L);
  if (!st && (cuts[0] != 0 || cuts[h->nranks] != nz)) st = pmg_set_error(PMG_ERR_ARG_WRONG, __FILE__, __LINE__, "cuts must run from 0 to nz = %d", nz);
  if (!st && (L.nx != nx || L.ny != ny || L.nzg != nz || L.kz0 != cuts[h->rank] || L.nz != cuts[h->rank + 1] - cuts[h->rank])) st = pmg_set_error(PMG_ERR_ARG_SIZ, __FILE__, __LINE__, "the grid slab does not match cuts[%d..%d] of a %d x %d x %d grid", h->rank, h->rank + 1, nx, ny, nz);
  const int top = levels - 1;
  if (!st) {
    h->cuts = (int32_t *)malloc(sizeof(int32_t) * (size_t)levels * (size_t)(h->nranks + 1));
    if (!h->cuts) st = pmg_set_error(PMG_ERR_MEM, __FILE__, __LINE__, "out of host memory");
  }
  if (!st) {
    const int nr1 = h->nranks + 1;
    memcpy(h->cuts + (size_t)top * nr1, cuts, sizeof(int32_t) * (size_t)nr1);
    for (int l = top; l >= 1 && !st; --l) {
      if (h->lv[l].nz == h->lv[l - 1].nz) st = pmg_set_error(PMG_ERR_SUP, __FILE__, __LINE__, "z-slabs need a grid that is coarsened in z on every level");
      for (int r = 0; r < nr1; ++r) h->cuts[(size_t)(l - 1) * nr1 + r] = (h->cuts[(size_t)l * nr1 + r] + 1) / 2; /* plane K <-> fine plane 2K */
    }
    for (int r = 0; r < h->nranks && !st; ++r)
      if (cuts[r + 1] <= cuts[r]) st = pmg_set_error(PMG_ERR_ARG_WRONG, __FILE__, __LINE__, "rank %d owns no plane", r);
  }
  if (st) {
    pmg_mgmc_destroy(out);
    return st;
  }
  h->dist          = dist;
  h->lv[top].g     = g;
  h->lv[top].kz0   = L.kz0;
  h->lv[top].nzl   = L.nz;
  h->n_io          = nx * ny * L.nz;
  return PMG_SUCCESS;
}

/* A hierarchy handed over level by level: what PCGAMGMC finds inside PETSc's PCMG/PCGAMG after PCSetUp -- the
   level operators (PCMGGetSmoother + PCGetOperators) and interpolations (PCMGGetInterpolation), reference
   src/pc_gamgmc.c:165-176 -- e.g. a GAMG hierarchy of an unstructured P1 matrix.  Every level is swept with the
   sliced-ELL multicolour kernel (greedy colouring), transfers are CSR products. */
pmg_status pmg_mgmc_create_hierarchy(int32_t levels, pmg_mgmc *out)
{
  PMG_CHECK(out, PMG_ERR_ARG_NULL, "null output handle");
  *out = NULL;
  PMG_CHECK(levels >= 2 && levels <= 64, PMG_ERR_ARG_OUTOFRANGE, "levels = %d", levels);
  pmg_mgmc h;
  PMG_CALL(mgmc_alloc(levels, &h));
  h->user_hier = 1;
  *out           = h;
  return PMG_SUCCESS;
}

static void hcsr_borrow(hcsr *m, int32_t nr, int32_t nc, const int32_t *rp, const int32_t *ci, const double *v) /* borrowed, only read */
{
  m->nr = nr;
  m->nc = nc;
  m->rp = (int32_t *)rp;
  m->ci = (int32_t *)ci;
  m->v  = (double *)v;
}

pmg_status pmg_mgmc_set_level_operator(pmg_mgmc h, int32_t level, int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals)
{
  PMG_CHECK(h && rowptr && colidx && vals, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(h->user_hier && !h->is_setup, PMG_ERR_ARG_WRONGSTATE, "level operators belong to pmg_mgmc_create_hierarchy, before set-up");
  PMG_CHECK(level >= 0 && level < h->nlevels && n >= 1, PMG_ERR_ARG_OUTOFRANGE, "level %d, n %d", level, n);
  mg_level *Lv = &h->lv[level];
  Lv->n        = n;
  Lv->nx       = n;
  Lv->ny = Lv->nz = 1;
  hcsr_borrow(&h->in[level].A_user, n, n, rowptr, colidx, vals);
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_set_level_interpolation(pmg_mgmc h, int32_t level, int32_t nrows, int32_t ncols, const int32_t *rowptr, const int32_t *colidx, const double *vals)
{
  PMG_CHECK(h && rowptr && colidx && vals, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(h->user_hier && !h->is_setup, PMG_ERR_ARG_WRONGSTATE, "interpolations belong to pmg_mgmc_create_hierarchy, before set-up");
  PMG_CHECK(level >= 1 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  hcsr_borrow(&h->in[level].P_user, nrows, ncols, rowptr, colidx, vals);
  return PMG_SUCCESS;
}

/* ---- caller-supplied hierarchy distributed by ROW BLOCKS (the reference runs PCGAMGMC on any MATMPIAIJ,
   src/pc_gamgmc.c:157-223; MCSORApply_MPIAIJ src/mc_sor.c:298-381 is the level sampler) --------------------------------
   Every rank describes ITS rows:
   * level 0 (coarsest, exact sampler): the whole matrix on every rank (pmg_mgmc_set_level_operator) -- it is factored
     redundantly, the restricted right-hand side is all-gathered by the row blocks `coarse_starts`;
   * level l >= 1: pmg_mgmc_set_level_operator with the rank's rows in LOCAL numbering (owned rows 0 .. nowned-1 in the
     order of the global rows row0 .. row0+nowned-1, entries in the order of the global CSR row, then one identity row
     per ghost), and pmg_mgmc_set_level_rowblock with a globally valid distance-1 colouring of the owned rows and the
     ghost-update plan of pmg_distmcsor_create in LOCAL ROW indices;
   * pmg_mgmc_set_level_interpolation(l): the owned rows of P_l, columns in the local numbering of level l-1 (global
     indices for l-1 = 0); pmg_mgmc_set_level_restriction(l): the rows of R_l = P_l^T that this rank owns on level l-1,
     columns in the local numbering of level l, entries by ascending global fine row (the order of a transposition).
   Noise is keyed on global rows and every row keeps its global entry order: the chain is the single-device chain of
   pmg_mgmc_create_hierarchy bit for bit; with a low-rank update (pmg_mgmc_set_lowrank: this rank's rows of B) to rounding. */
pmg_status pmg_mgmc_set_rowblock_transport(pmg_mgmc h, pmg_dist dist, const int64_t *coarse_starts)
{
  PMG_CHECK(h && dist && coarse_starts, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(!pmg_mgmc_i_has_blocks(h), PMG_ERR_SUP, "row blocks on a hierarchy with block smoothing (pmg_mgmc_set_level_blocks) are not supported");
  PMG_CHECK(h->user_hier && !h->is_setup, PMG_ERR_ARG_WRONGSTATE, "row blocks belong to pmg_mgmc_create_hierarchy, before set-up");
  int32_t rank, nranks;
  PMG_CALL(pmg_dist_get_info(dist, &rank, &nranks, NULL));
  PMG_CHECK(nranks >= 1 && nranks <= 64, PMG_ERR_ARG_OUTOFRANGE, "%d ranks", nranks);
  free(h->rb_c0_starts);
  h->rb_c0_starts = (int64_t *)malloc(sizeof(int64_t) * ((size_t)nranks + 1));
  PMG_CHECK(h->rb_c0_starts, PMG_ERR_MEM, "out of host memory");
  memcpy(h->rb_c0_starts, coarse_starts, sizeof(int64_t) * ((size_t)nranks + 1));
  for (int r = 0; r < nranks; ++r) PMG_CHECK(coarse_starts[r] <= coarse_starts[r + 1], PMG_ERR_ARG_WRONG, "coarse row blocks must be ascending");
  PMG_CHECK(coarse_starts[0] == 0, PMG_ERR_ARG_WRONG, "coarse row blocks must start at 0");
  h->rb_dist = dist;
  h->rank    = rank;
  h->nranks  = nranks;
  return PMG_SUCCESS;
}

static void *dup_bytes(const void *src, size_t bytes)
{
  void *p = malloc(bytes ? bytes : 1);
  if (p && bytes) memcpy(p, src, bytes);
  return p;
}

pmg_status pmg_mgmc_set_level_rowblock(pmg_mgmc h, int32_t level, int64_t row0, int32_t nowned, int32_t ncolors, const int32_t *colors_owned, const int64_t *send_ptr, const int32_t *send_idx, const int64_t *counts, const int64_t *recv_ptr, const int32_t *recv_src, const int32_t *recv_idx)
{
  PMG_CHECK(h && colors_owned && send_ptr && counts && recv_ptr, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(!pmg_mgmc_i_has_blocks(h), PMG_ERR_SUP, "row-block levels on a hierarchy with block smoothing (pmg_mgmc_set_level_blocks) are not supported");
  PMG_CHECK(h->user_hier && !h->is_setup && h->rb_dist, PMG_ERR_ARG_WRONGSTATE, "call pmg_mgmc_set_rowblock_transport first, before set-up");
  PMG_CHECK(level >= 1 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d (the coarsest level is replicated)", level);
  PMG_CHECK(row0 >= 0 && nowned >= 0 && ncolors >= 1, PMG_ERR_ARG_OUTOFRANGE, "row0 %lld, %d owned rows, %d colours", (long long)row0, nowned, ncolors);
  mg_level_in *in  = &h->in[level];
  const size_t nc1 = (size_t)ncolors + 1, ns = (size_t)send_ptr[ncolors], nr = (size_t)recv_ptr[ncolors];
  PMG_CHECK((ns == 0 || send_idx) && (nr == 0 || (recv_src && recv_idx)), PMG_ERR_ARG_NULL, "null index list");
  free(in->rb_colors), free(in->rb_send_ptr), free(in->rb_recv_ptr), free(in->rb_counts), free(in->rb_send_idx), free(in->rb_recv_src), free(in->rb_recv_idx);
  in->rb_colors   = (int32_t *)dup_bytes(colors_owned, sizeof(int32_t) * (size_t)nowned);
  in->rb_send_ptr = (int64_t *)dup_bytes(send_ptr, sizeof(int64_t) * nc1);
  in->rb_recv_ptr = (int64_t *)dup_bytes(recv_ptr, sizeof(int64_t) * nc1);
  in->rb_counts   = (int64_t *)dup_bytes(counts, sizeof(int64_t) * (size_t)ncolors * (size_t)h->nranks);
  in->rb_send_idx = (int32_t *)dup_bytes(send_idx, sizeof(int32_t) * ns);
  in->rb_recv_src = (int32_t *)dup_bytes(recv_src, sizeof(int32_t) * nr);
  in->rb_recv_idx = (int32_t *)dup_bytes(recv_idx, sizeof(int32_t) * nr);
  PMG_CHECK(in->rb_colors && in->rb_send_ptr && in->rb_recv_ptr && in->rb_counts && in->rb_send_idx && in->rb_recv_src && in->rb_recv_idx, PMG_ERR_MEM, "out of host memory");
  in->rb         = 1;
  in->rb_row0    = row0;
  in->rb_nowned  = nowned;
  in->rb_ncolors = ncolors;
  return PMG_SUCCESS;
}

/* Block Gibbs smoothing of one level of a caller-supplied hierarchy: the multiplicative patch smoother of examples/ex13.py:11-22
   (PCASM multiplicative around -sub_pc_type cholsampler, src/pc_chols.c:174-194,220-260,284-287) as that level's smoother.
   The blocks are copied; block_colors NULL = first-fit.  They are checked at set-up, against the level's operator. */
pmg_status pmg_mgmc_set_level_blocks(pmg_mgmc h, int32_t level, int32_t nblocks, const int32_t *blockptr, const int32_t *blockrows, int32_t ncolors, const int32_t *block_colors)
{
  PMG_CHECK(h && blockptr, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(h->user_hier, PMG_ERR_SUP, "block smoothing needs a caller-supplied hierarchy (pmg_mgmc_create_hierarchy): DMDA handles are not supported");
  PMG_CHECK(!h->is_setup, PMG_ERR_ARG_WRONGSTATE, "set the blocks of a level before pmg_mgmc_setup");
  PMG_CHECK(level >= 0 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  PMG_CHECK(nblocks >= 0 && (blockrows || blockptr[nblocks] == 0), PMG_ERR_ARG_OUTOFRANGE, "%d blocks", nblocks);
  PMG_CHECK(!h->rb_dist && !h->in[level].rb, PMG_ERR_SUP, "block smoothing of row-block distributed hierarchies is not supported");
  PMG_CHECK(h->omega == 1.0, PMG_ERR_SUP, "block smoothing with omega = %g: a block sweep has no relaxation parameter", h->omega);
  PMG_CHECK(!h->lrc_k, PMG_ERR_SUP, "block smoothing of a hierarchy with a low-rank update (pmg_mgmc_set_lowrank) is not supported");
  mg_level_in *in = &h->in[level];
  free(in->bg_blockptr), free(in->bg_blockrows), free(in->bg_colors);
  in->bg_blockptr  = (int32_t *)dup_bytes(blockptr, sizeof(int32_t) * ((size_t)nblocks + 1));
  in->bg_blockrows = (int32_t *)dup_bytes(blockrows, sizeof(int32_t) * (size_t)(blockptr[nblocks] > 0 ? blockptr[nblocks] : 0));
  in->bg_colors    = block_colors ? (int32_t *)dup_bytes(block_colors, sizeof(int32_t) * (size_t)nblocks) : NULL;
  PMG_CHECK(in->bg_blockptr && in->bg_blockrows && (in->bg_colors || !block_colors), PMG_ERR_MEM, "out of host memory");
  in->bg_nblocks = nblocks;
  in->bg_ncolors = ncolors;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_set_level_restriction(pmg_mgmc h, int32_t level, int32_t nrows, int32_t ncols, const int32_t *rowptr, const int32_t *colidx, const double *vals)
{
  PMG_CHECK(h && rowptr && colidx && vals, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(h->user_hier && !h->is_setup, PMG_ERR_ARG_WRONGSTATE, "restrictions belong to pmg_mgmc_create_hierarchy, before set-up");
  PMG_CHECK(level >= 1 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  hcsr_borrow(&h->in[level].R_user, nrows, ncols, rowptr, colidx, vals);
  return PMG_SUCCESS;
}

/* the narrowed copies of 64-bit index arrays (NULL where the caller's were 32-bit already): the level adopts them when
   the setter took the matrix, otherwise they are freed */
static pmg_status adopt_narrowed(pmg_status st, int32_t **rp_slot, int32_t **ci_slot, int32_t *rpo, int32_t *cio)
{
  free(st ? rpo : *rp_slot);
  free(st ? cio : *ci_slot);
  if (!st) *rp_slot = rpo, *ci_slot = cio;
  return st;
}

/* pmg_mgmc_set_level_operator / _interpolation for either PetscInt width: idx_width = sizeof(PetscInt) * 8 */
pmg_status pmg_mgmc_set_level_operator_idx(pmg_mgmc h, int32_t level, int64_t n, const void *rowptr, const void *colidx, const double *vals, int idx_width)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(level >= 0 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  const int32_t *rp, *ci;
  int32_t       *rpo, *cio;
  PMG_CALL(pmg_narrow_csr(n, n, rowptr, colidx, idx_width, &rp, &ci, &rpo, &cio));
  return adopt_narrowed(pmg_mgmc_set_level_operator(h, level, (int32_t)n, rp, ci, vals), &h->in[level].A_rp_own, &h->in[level].A_ci_own, rpo, cio);
}

pmg_status pmg_mgmc_set_level_interpolation_idx(pmg_mgmc h, int32_t level, int64_t nrows, int64_t ncols, const void *rowptr, const void *colidx, const double *vals, int idx_width)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(level >= 1 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  const int32_t *rp, *ci;
  int32_t       *rpo, *cio;
  PMG_CALL(pmg_narrow_csr(nrows, ncols, rowptr, colidx, idx_width, &rp, &ci, &rpo, &cio));
  return adopt_narrowed(pmg_mgmc_set_level_interpolation(h, level, (int32_t)nrows, (int32_t)ncols, rp, ci, vals), &h->in[level].P_rp_own, &h->in[level].P_ci_own, rpo, cio);
}

pmg_status pmg_mgmc_set_smoother(pmg_mgmc h, int scaled, double omega, int sweep_type, int32_t its)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(!h->is_setup, PMG_ERR_ARG_WRONGSTATE, "set the smoother before pmg_mgmc_setup");
  PMG_CHECK(pmg_sweep_type_ok(sweep_type), PMG_ERR_SUP, "Only forward, backward and symmetric sweep supported");
  PMG_CHECK(scaled || omega == 1.0, PMG_ERR_SUP, "sorgibbs smoothing requires omega = 1");
  PMG_CHECK(its >= 1 && (uint32_t)its * 4u <= MG_DRAWS_PER_SAMPLE, PMG_ERR_ARG_OUTOFRANGE, "smoothing iterations %d", its);
  PMG_CHECK(omega == 1.0 || !pmg_mgmc_i_has_blocks(h), PMG_ERR_SUP, "omega = %g on a hierarchy with block smoothing: a block sweep has no relaxation parameter", omega);
  h->scaled     = scaled;
  h->omega      = omega;
  h->sweep_type = sweep_type;
  h->nu         = its;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_set_coarse(pmg_mgmc h, int type, int32_t its)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(!h->is_setup, PMG_ERR_ARG_WRONGSTATE, "set the coarse sampler before pmg_mgmc_setup");
  PMG_CHECK(type == 0 || type == 1, PMG_ERR_ARG_OUTOFRANGE, "coarse sampler type %d", type);
  PMG_CHECK(its >= 1 && (uint32_t)its * 2u <= MG_DRAWS_PER_SAMPLE, PMG_ERR_ARG_OUTOFRANGE, "coarse iterations %d", its);
  h->coarse_type = type;
  h->coarse_its  = its;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_set_correction_form(pmg_mgmc h, int literal)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  h->correction_form = literal != 0;
  return PMG_SUCCESS;
}

/* on = 0: the cycle forms r = b - A x and b_c = P^T r with two kernels on every level, a low-rank term is subtracted
   from r before the restriction -- the reference's operation order (src/pc_gamgmc.c:194, PCMG's residual then
   MatRestrict).  Default (1): grid levels fuse the two and subtract a low-rank term in restricted form. */
pmg_status pmg_mgmc_set_fused_transfers(pmg_mgmc h, int on)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(!h->is_setup || !h->dist, PMG_ERR_ARG_WRONGSTATE, "z-slab hierarchies decide this at set-up");
  h->no_fused = !on;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_set_coloring(pmg_mgmc h, int rule)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(!h->is_setup, PMG_ERR_ARG_WRONGSTATE, "the colouring rule must be chosen before set-up");
  PMG_CHECK(rule == PMG_COLORING_GREEDY || rule == PMG_COLORING_ITERATED, PMG_ERR_ARG_OUTOFRANGE, "colouring rule %d: greedy or iterated expected", rule);
  h->aij_coloring = rule;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_set_keep_host(pmg_mgmc h, int keep)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  h->keep_host = keep;
  return PMG_SUCCESS;
}

/* MATLRC fine-level operator A + B S B^T (MatCreateLRC in examples/ex4.c; PCSetUp_GAMGMC builds the hierarchy from
   the base matrix A, src/pc_gamgmc.c:282-286).  PCGAMGMC_SetUpHierarchy (src/pc_gamgmc.c:157-196) then gives every
   level l the operator A_l + B_l S B_l^T with B_{l-1} = P_l^T B_l, for the level sampler AND the level residual; the
   coarse Cholesky sampler factors the explicit sum (src/pc_chols.c:119-153).  B is n_fine x k column-major in the
   finest level's natural numbering, S the k diagonal entries; both are copied.  Call before pmg_mgmc_setup. */
pmg_status pmg_mgmc_set_lowrank(pmg_mgmc h, int32_t k, const double *B_host, const double *S_host)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(!h->is_setup, PMG_ERR_ARG_WRONGSTATE, "set the low-rank update before pmg_mgmc_setup");
  PMG_CHECK(k >= 0 && k <= 64, PMG_ERR_ARG_OUTOFRANGE, "rank k = %d (0..64 supported)", k);
  PMG_CHECK(k == 0 || !pmg_mgmc_i_has_blocks(h), PMG_ERR_SUP, "a low-rank update on a hierarchy with block smoothing (pmg_mgmc_set_level_blocks) is not supported");
  free(h->lrc_B);
  free(h->lrc_S);
  h->lrc_B = h->lrc_S = NULL;
  h->lrc_k = 0;
  if (k == 0) return PMG_SUCCESS;
  PMG_CHECK(B_host && S_host, PMG_ERR_ARG_NULL, "null low-rank factor");
  const int32_t n = h->dist ? h->n_io : h->lv[h->nlevels - 1].n; /* z-slabs: the rows of this rank's planes */
  PMG_CHECK(n > 0, PMG_ERR_ARG_WRONGSTATE, "set the finest level operator before the low-rank update");
  h->lrc_B = (double *)malloc(sizeof(double) * (size_t)n * k);
  h->lrc_S = (double *)malloc(sizeof(double) * (size_t)k);
  PMG_CHECK(h->lrc_B && h->lrc_S, PMG_ERR_MEM, "out of host memory");
  memcpy(h->lrc_B, B_host, sizeof(double) * (size_t)n * k);
  memcpy(h->lrc_S, S_host, sizeof(double) * (size_t)k);
  h->lrc_k = k;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_get_num_levels(pmg_mgmc h, int32_t *levels)
{
  PMG_CHECK(h && levels, PMG_ERR_ARG_NULL, "null argument");
  *levels = h->nlevels;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_get_level_dims(pmg_mgmc h, int32_t level, int32_t *nx, int32_t *ny, int32_t *nz)
{
  PMG_CHECK(h && nx && ny && nz, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(level >= 0 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  *nx = h->lv[level].nx;
  *ny = h->lv[level].ny;
  *nz = h->lv[level].nz;
  return PMG_SUCCESS;
}

/* which = 0: Galerkin operator of `level` (< finest); which = 1: interpolation from level-1 to `level` (>= 1).
   Call with NULL arrays to query nrows/nnz.  Needs pmg_mgmc_set_keep_host(h, 1) before set-up. */
pmg_status pmg_mgmc_get_level_matrix(pmg_mgmc h, int32_t level, int which, int32_t *nrows, int32_t *nnz, int32_t *rowptr, int32_t *colidx, double *vals)
{
  PMG_CHECK(h && nrows && nnz, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(h->is_setup && h->keep_host, PMG_ERR_ARG_WRONGSTATE, "needs pmg_mgmc_set_keep_host(h,1) and pmg_mgmc_setup");
  PMG_CHECK(level >= 0 && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  const hcsr *M = which == 0 ? &h->lv[level].A_host : &h->lv[level].P_host;
  PMG_CHECK(M->rp, PMG_ERR_ARG_OUTOFRANGE, "level %d has no such matrix", level);
  *nrows = M->nr;
  *nnz   = M->rp[M->nr];
  if (rowptr) memcpy(rowptr, M->rp, sizeof(int32_t) * ((size_t)M->nr + 1));
  if (colidx) memcpy(colidx, M->ci, sizeof(int32_t) * (size_t)*nnz);
  if (vals) memcpy(vals, M->v, sizeof(double) * (size_t)*nnz);
  return PMG_SUCCESS;
}

/* kind: 0 = grid level (colour-partitioned cvec), 1 = class-stencil level, 2 = sliced-ELL level, 3 = dense coarsest level;
   ld = vector length, off = position of natural index 0 for kinds 1 and 3 (plane-padded natural order), else 0 */
pmg_status pmg_mgmc_get_level_layout(pmg_mgmc h, int32_t level, int32_t *kind, int64_t *ld, int64_t *off)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 0, &Lv));
  if (kind) switch (Lv->kind) {
    case MG_LV_GRID:
    case MG_LV_GRID_SLAB: *kind = 0; break;
    case MG_LV_ST27: *kind = 1; break;
    case MG_LV_SELL:
    case MG_LV_ROWBLOCK: *kind = 2; break;
    case MG_LV_EXACT: *kind = 3; break;
    }
  if (ld) *ld = Lv->ld;
  if (off) *off = Lv->padded ? Lv->off : 0;
  return PMG_SUCCESS;
}

/* the 27 x 27 class table and the per-class noise scale of a class-stencil level, as the kernels use them */
pmg_status pmg_mgmc_get_level_stencil(pmg_mgmc h, int32_t level, double *coef_host, double *sqrtdiag_host)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 0, &Lv));
  PMG_CHECK(Lv->kind == MG_LV_ST27, PMG_ERR_ARG_WRONGSTATE, "level %d is not a class-stencil level", level);
  if (coef_host) PMG_HIP(hipMemcpy(coef_host, Lv->st_coef, sizeof(double) * 27 * 27, hipMemcpyDeviceToHost));
  if (sqrtdiag_host) PMG_HIP(hipMemcpy(sqrtdiag_host, h->scaled ? Lv->st_sqrtd_scaled : Lv->st_sqrtd, sizeof(double) * 27, hipMemcpyDeviceToHost));
  return PMG_SUCCESS;
}

/* plane-padded natural layout; pos (may be NULL): natural index -> layout position */
static void level_set_padded(mg_level *Lv, int32_t *pos)
{
  Lv->padded = 1;
  Lv->off    = (int64_t)Lv->nx * Lv->ny;
  Lv->ld     = (int64_t)Lv->nx * Lv->ny * ((int64_t)Lv->nzl + 2);
  for (int32_t q = 0; pos && q < Lv->n; ++q) pos[q] = q + (int32_t)Lv->off;
}

/* upload a class-stencil table and make Lv a class-stencil level (owned planes kz0 .. kz0+nzl-1 of its nz) */
static pmg_status st27_install(mg_level *Lv, const double *coef, const int *have, double omega)
{
  double       dg[27], idg[27], sq[27], sqs[27];
  const double sc = sqrt((2 - omega) / omega);
  for (int c = 0; c < 27; ++c) {
    dg[c] = have[c] ? coef[27 * c + 13] : 1.0;
    const double t = 1.0 / dg[c];
    idg[c]         = t * omega;            /* MCSORUpdateIDiag, src/mc_sor.c:114-124 */
    sq[c]          = sqrt(fabs(dg[c]));    /* src/pc_mcgibbs.c:149 */
    sqs[c]         = sq[c] * sc;
  }
  PMG_CALL(pmg_dev_upload((void **)&Lv->st_coef, coef, sizeof(double) * 27 * 27));
  PMG_CALL(pmg_dev_upload((void **)&Lv->st_idiag, idg, sizeof idg));
  PMG_CALL(pmg_dev_upload((void **)&Lv->st_sqrtd, sq, sizeof sq));
  PMG_CALL(pmg_dev_upload((void **)&Lv->st_sqrtd_scaled, sqs, sizeof sqs));
  Lv->st.nx    = Lv->nx;
  Lv->st.ny    = Lv->ny;
  Lv->st.nz    = Lv->nzl;
  Lv->st.kz0   = Lv->kz0;
  Lv->st.nzg   = Lv->nz;
  Lv->st.coef  = Lv->st_coef;
  Lv->st.idiag = Lv->st_idiag;
  Lv->kind     = MG_LV_ST27;
  return PMG_SUCCESS;
}

/* Try to express the CSR operator of a structured level as 27 position-class stencils: the level is installed as an
   MG_LV_ST27 level if every row equals its class stencil bit for bit (always the case for Galerkin operators of the
   constant-coefficient fine operator); otherwise it is left as it was (the caller keeps the sliced-ELL form). */
static pmg_status st27_from_csr(mg_level *Lv, const hcsr *A, double omega)
{
  double coef[27 * 27];
  int    have[27];
  return pmg_hier_st27_extract(Lv->nx, Lv->ny, Lv->nz, A, coef, have) ? st27_install(Lv, coef, have, omega) : PMG_SUCCESS;
}

/* deterministic sweep of a class-stencil level as a pmg_det_sweep_fn: the cycle's own sweep without its noise */
typedef struct {
  pmg_mgmc  h;
  mg_level *Lv;
} level_ref;

static pmg_status st27_det_sweep(void *ctx, int dir, const double *b, double *y, void *stream)
{
  const level_ref *c = (const level_ref *)ctx;
  return pmg_mgmc_i_st27_dir_sweep(c->h, c->Lv, dir, 0, b, y, 0, NULL, stream);
}

/* deterministic sweep of the fine level of a z-slab hierarchy; sum of k-vectors over the ranks */
static pmg_status dist_det_sweep(void *ctx, int dir, const double *b, double *y, void *stream)
{
  return pmg_dist_apply_cvec(((pmg_mgmc)ctx)->dist, b, y, dir, stream);
}
static pmg_status mg_reduce(void *ctx, double *vals_dev, int count, void *stream)
{
  return pmg_dist_allreduce_sum(((pmg_mgmc)ctx)->dist, vals_dev, count, stream);
}

/* MatCreateLRC(Ac, Bc, Sf) + KSPSetOperators on the level sampler (src/pc_gamgmc.c:178, :185-187): B_nat is the
   level's n x k block in natural numbering */
static pmg_status level_attach_lrc(pmg_mgmc h, mg_level *Lv, const double *B_nat)
{
  switch (Lv->kind) {
  case MG_LV_GRID:
  case MG_LV_GRID_SLAB: return pmg_grid_set_lowrank(Lv->g, h->lrc_k, B_nat, h->lrc_S); /* (a slab hierarchy attaches on the device: stencil_attach_lowrank) */
  case MG_LV_SELL:
  case MG_LV_ROWBLOCK: return pmg_mcsor_set_lowrank(Lv->mc, h->lrc_k, B_nat, h->lrc_S); /* (a row block attaches to its pmg_distmcsor on the device) */
  case MG_LV_ST27: {
    int64_t *pos = (int64_t *)malloc(sizeof(int64_t) * (size_t)Lv->n);
    PMG_CHECK(pos, PMG_ERR_MEM, "out of host memory");
    for (int32_t q = 0; q < Lv->n; ++q) pos[q] = q + Lv->off;
    level_ref  ref = {h, Lv};
    pmg_status st  = pmg_lrc_build(&Lv->lrc, h->lrc_k, Lv->ld, Lv->n, B_nat, pos, h->lrc_S, st27_det_sweep, &ref);
    free(pos);
    return st;
  }
  case MG_LV_EXACT: break; /* the update goes into the factored matrix */
  }
  return PMG_SUCCESS;
}

static pmg_status upload_transfer(const hcsr *M, const int32_t *rowpos_of, const int32_t *colpos_of, int32_t **rowpos, int32_t **rowptr, int32_t **col, double **val)
{
  const int32_t nnz = M->rp[M->nr];
  int32_t      *rp  = (int32_t *)malloc(sizeof(int32_t) * (size_t)(M->nr > 0 ? M->nr : 1));
  int32_t      *cc  = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1));
  PMG_CHECK(rp && cc, PMG_ERR_MEM, "out of host memory");
  for (int32_t r = 0; r < M->nr; ++r) rp[r] = rowpos_of[r];
  for (int32_t k = 0; k < nnz; ++k) cc[k] = colpos_of[M->ci[k]];
  pmg_status st = pmg_dev_upload((void **)rowpos, rp, sizeof(int32_t) * (size_t)M->nr);
  if (!st) st = pmg_dev_upload((void **)rowptr, M->rp, sizeof(int32_t) * ((size_t)M->nr + 1));
  if (!st) st = pmg_dev_upload((void **)col, cc, sizeof(int32_t) * (size_t)nnz);
  if (!st) st = pmg_dev_upload((void **)val, M->v, sizeof(double) * (size_t)nnz);
  free(rp);
  free(cc);
  return st;
}

/* ---- set-up temporaries --------------------------------------------------------------------------------------------
   Whatever a set-up routine allocates that is not a field of the handle lives here, so that its body may leave through
   PMG_CALL / PMG_CHECK anywhere: pmg_mgmc_setup releases the scratch whatever the body's status.  A failed set-up leaves
   the handle partly built with is_setup == 0; pmg_mgmc_destroy releases that. */
typedef struct {
  int         nlevels;
  int32_t   **pos;             /* [nlevels]: natural index -> layout position */
  hcsr        P, R, Ac, Aprev; /* transfers and operators of the level pair at hand */
  double     *Bcur;            /* host: level-l block of the low-rank factor, natural numbering */
  int         Bcur_owned;      /* 0 while it is the handle's lrc_B (the finest level) */
  double     *Bdev, *Bdev2;    /* device: that block in the level's layout; the next coarser one while it is formed (or a staging column) */
  void       *tmp;             /* host: index lists and staging of the step at hand (setup_tmp) */
  st27_table *tab;             /* [nlevels-1]: class-stencil tables from the proxy hierarchy */
} setup_scratch;

static void setup_release(setup_scratch *s)
{
  for (int l = 0; l < s->nlevels && s->pos; ++l) free(s->pos[l]);
  free(s->pos);
  pmg_hcsr_free(&s->P);
  pmg_hcsr_free(&s->R);
  pmg_hcsr_free(&s->Ac);
  pmg_hcsr_free(&s->Aprev);
  if (s->Bcur_owned) free(s->Bcur);
  pmg_dev_free(s->Bdev);
  pmg_dev_free(s->Bdev2);
  free(s->tmp);
  free(s->tab);
}

/* zero-filled host scratch; the previous one is dropped */
static void *setup_tmp(setup_scratch *s, size_t bytes)
{
  free(s->tmp);
  return s->tmp = calloc(bytes ? bytes : 1, 1);
}

/* the scratch takes over the next coarser level's block */
static void setup_own_B(setup_scratch *s, double *B)
{
  if (s->Bcur_owned) free(s->Bcur);
  s->Bcur       = B;
  s->Bcur_owned = 1;
}

static void setup_next_Bdev(setup_scratch *s)
{
  pmg_dev_free(s->Bdev);
  s->Bdev  = s->Bdev2;
  s->Bdev2 = NULL;
}


/* B_{l-1} = P_l^T B_l on the host (s->R = P_l^T) and the MATLRC operator of level l-1, src/pc_gamgmc.c:177-187 */
static pmg_status setup_restrict_attach_B(pmg_mgmc h, setup_scratch *s, const mg_level *U, mg_level *Cc)
{
  double *Bc = NULL;
  PMG_CALL(pmg_hier_restrict_B(&s->R, h->lrc_k, U->n, s->Bcur, &Bc));
  setup_own_B(s, Bc);
  return level_attach_lrc(h, Cc, s->Bcur);
}

/* sliced-ELL level sampler from a host CSR in natural numbering, coloured by `rule` (PMG_COLORING_USER: by `colors`); a
   row block keys its noise on the global row.  Fills ld, A_nnz and pos (natural row -> layout position). */
static pmg_status level_make_sell(pmg_mgmc h, int l, const hcsr *A, int rule, const int32_t *colors, int32_t *pos)
{
  mg_level          *Lv = &h->lv[l];
  const mg_level_in *in = &h->in[l];
  PMG_CALL(pmg_mcsor_create_csr(Lv->n, A->rp, A->ci, A->v, &Lv->mc));
  PMG_CALL(pmg_mcsor_set_natural_order(Lv->mc, 1));
  Lv->A_nnz = A->rp[Lv->n];
  PMG_CALL(pmg_mcsor_set_coloring(Lv->mc, rule, colors));
  if (in->rb) PMG_CALL(pmg_mcsor_set_noise_row_offset(Lv->mc, in->rb_row0));
  PMG_CALL(pmg_mcsor_set_omega(Lv->mc, h->omega));
  PMG_CALL(pmg_mcsor_set_sweep_type(Lv->mc, h->sweep_type));
  PMG_CALL(pmg_mcsor_setup(Lv->mc));
  int32_t ld32;
  PMG_CALL(pmg_mcsor_layout_len(Lv->mc, &ld32));
  Lv->ld = ld32;
  PMG_CALL(pmg_mcsor_get_layout(Lv->mc, pos));
  if (!in->bg_blockptr) return PMG_SUCCESS;
  /* block smoothing: the same operator, vectors in the layout just built */
  PMG_CHECK(h->omega == 1.0 && !h->lrc_k && !in->rb, PMG_ERR_SUP, "level with block smoothing: omega = 1, no low-rank update and no row block");
  PMG_CALL(pmg_blockgibbs_create_csr(Lv->n, A->rp, A->ci, A->v, in->bg_nblocks, in->bg_blockptr, in->bg_blockrows, &Lv->bg));
  if (in->bg_colors) PMG_CALL(pmg_blockgibbs_set_coloring(Lv->bg, in->bg_ncolors, in->bg_colors));
  PMG_CALL(pmg_blockgibbs_set_layout(Lv->bg, ld32, pos));
  return pmg_blockgibbs_setup(Lv->bg);
}

/* the level vectors b, x, r, the second iterate where the out-of-place sweeps want one, and the outer chain's pair in the
   finest level's layout; all zero-filled (pmg_dev_alloc): ghost planes and layout padding stay zero */
static pmg_status alloc_level_vectors(pmg_mgmc h)
{
  for (int l = 0; l < h->nlevels; ++l) {
    mg_level *Lv = &h->lv[l];
    PMG_CALL(pmg_dev_alloc((void **)&Lv->b, sizeof(double) * (size_t)Lv->ld));
    PMG_CALL(pmg_dev_alloc((void **)&Lv->x, sizeof(double) * (size_t)Lv->ld));
    PMG_CALL(pmg_dev_alloc((void **)&Lv->r, sizeof(double) * (size_t)Lv->ld));
    if (pmg_mgmc_i_level_wants_x2(Lv)) PMG_CALL(pmg_dev_alloc((void **)&Lv->x2, sizeof(double) * (size_t)Lv->ld));
  }
  const size_t top_bytes = sizeof(double) * (size_t)h->lv[h->nlevels - 1].ld;
  PMG_CALL(pmg_dev_alloc((void **)&h->y_lay, top_bytes));
  PMG_CALL(pmg_dev_alloc((void **)&h->b_lay, top_bytes));
  return PMG_SUCCESS;
}

/* ---- caller-supplied hierarchy ---------------------------------------------------------------------------------- */

/* the shapes of level l of a caller-supplied hierarchy; on l == 0 also where the row blocks begin */
static pmg_status user_level_check(pmg_mgmc h, int l)
{
  const int top = h->nlevels - 1;
  const mg_level    *Lv = &h->lv[l];
  const mg_level_in *in = &h->in[l];
  PMG_CHECK(in->A_user.rp, PMG_ERR_ARG_WRONGSTATE, "level %d has no operator", l);
  PMG_CHECK(!in->bg_blockptr || l >= 1 || h->coarse_type == 1, PMG_ERR_ARG_WRONG, "level 0 has blocks but is sampled exactly: block smoothing applies to a Gibbs coarse level (pmg_mgmc_set_coarse)");
  if (h->rb_dist) { /* row blocks from level rb_fold upwards; the levels below are replicated (the coarsest sampled exactly) */
    if (l == 0) {
      h->rb_fold = 1;
      while (h->rb_fold <= top && !h->in[h->rb_fold].rb) ++h->rb_fold;
      PMG_CHECK(h->rb_fold <= top, PMG_ERR_ARG_WRONGSTATE, "row-block hierarchy without a row-block level (pmg_mgmc_set_level_rowblock)");
      PMG_CHECK(h->rb_c0_starts[h->nranks] == h->lv[h->rb_fold - 1].n, PMG_ERR_ARG_SIZ, "the row blocks of the highest replicated level cover %lld rows, level %d has %d", (long long)h->rb_c0_starts[h->nranks], h->rb_fold - 1, h->lv[h->rb_fold - 1].n);
    }
    PMG_CHECK(l < h->rb_fold ? !in->rb : in->rb, PMG_ERR_ARG_WRONGSTATE, "row-block hierarchy: level %d %s", l, l < h->rb_fold ? "lies below a replicated level and must be replicated too" : "has no row block (pmg_mgmc_set_level_rowblock)");
    PMG_CHECK(h->coarse_type == 0, PMG_ERR_SUP, "row-block hierarchies: exact coarse sampler");
    if (l >= h->rb_fold) {
      PMG_CHECK(in->P_user.rp && in->R_user.rp && in->P_user.nr == in->rb_nowned && in->P_user.nc == h->lv[l - 1].n && in->R_user.nc == Lv->n, PMG_ERR_ARG_SIZ, "level %d: interpolation rows = owned rows, its columns and the restriction's in local numbering", l);
      PMG_CHECK(in->R_user.nr == (l == h->rb_fold ? (int32_t)(h->rb_c0_starts[h->rank + 1] - h->rb_c0_starts[h->rank]) : h->in[l - 1].rb_nowned), PMG_ERR_ARG_SIZ, "level %d: the restriction has one row per owned row of level %d", l, l - 1);
      return PMG_SUCCESS;
    }
  }
  PMG_CHECK(l == 0 || (in->P_user.rp && in->P_user.nr == Lv->n && in->P_user.nc == h->lv[l - 1].n), PMG_ERR_ARG_SIZ, "interpolation of %slevel %d missing or of the wrong shape", h->rb_dist ? "the replicated " : "", l);
  return PMG_SUCCESS;
}

/* the sampler of a row-block level: the caller's global colouring on the owned rows, the ghost rows in a colour of their own
   that is never swept; then the ghost-update plan in layout positions */
static pmg_status user_level_rowblock(pmg_mgmc h, int l, setup_scratch *s)
{
  mg_level          *Lv = &h->lv[l];
  const mg_level_in *in = &h->in[l];
  PMG_CHECK(in->rb_nowned <= Lv->n, PMG_ERR_ARG_SIZ, "level %d: %d owned rows of %d local rows", l, in->rb_nowned, Lv->n);
  int32_t *col = (int32_t *)setup_tmp(s, sizeof(int32_t) * (size_t)Lv->n);
  PMG_CHECK(col, PMG_ERR_MEM, "out of host memory");
  for (int32_t r = 0; r < Lv->n; ++r) col[r] = r < in->rb_nowned ? in->rb_colors[r] : in->rb_ncolors;
  Lv->rb_nowned = in->rb_nowned;
  PMG_CALL(level_make_sell(h, l, &in->A_user, PMG_COLORING_USER, col, s->pos[l]));
  const int64_t  ns = in->rb_send_ptr[in->rb_ncolors], nr = in->rb_recv_ptr[in->rb_ncolors];
  const int32_t *pos = s->pos[l];
  int32_t       *sp = (int32_t *)setup_tmp(s, sizeof(int32_t) * (size_t)(ns + nr + 2));
  PMG_CHECK(sp, PMG_ERR_MEM, "out of host memory");
  int32_t *rp = sp + ns + 1;
  for (int64_t q = 0; q < ns; ++q) {
    PMG_CHECK(in->rb_send_idx[q] >= 0 && in->rb_send_idx[q] < in->rb_nowned, PMG_ERR_ARG_OUTOFRANGE, "level %d: send row %d is not an owned row", l, in->rb_send_idx[q]);
    sp[q] = pos[in->rb_send_idx[q]];
  }
  for (int64_t q = 0; q < nr; ++q) {
    PMG_CHECK(in->rb_recv_idx[q] >= in->rb_nowned && in->rb_recv_idx[q] < Lv->n, PMG_ERR_ARG_OUTOFRANGE, "level %d: receive row %d is not a ghost row", l, in->rb_recv_idx[q]);
    rp[q] = pos[in->rb_recv_idx[q]];
  }
  return pmg_distmcsor_create(Lv->mc, h->rb_dist, in->rb_ncolors, in->rb_send_ptr, sp, in->rb_counts, in->rb_recv_ptr, in->rb_recv_src, rp, &Lv->dm);
}

/* row blocks: B_{l-1} = P_l^T B_l column by column on the device, with the V-cycle's own restriction (s->Bdev: level l's
   block in its layout, zero on the ghost rows); the block of the highest replicated level goes on to the host */
static pmg_status user_rowblock_restrict_B(pmg_mgmc h, int l, setup_scratch *s)
{
  mg_level    *U = &h->lv[l], *Cc = &h->lv[l - 1];
  const size_t k = (size_t)h->lrc_k;
  PMG_CALL(pmg_dev_alloc((void **)&s->Bdev2, sizeof(double) * (size_t)Cc->ld * k));
  for (int32_t c = 0; c < h->lrc_k; ++c) {
    double *bf = s->Bdev + (size_t)U->ld * c, *bc = s->Bdev2 + (size_t)Cc->ld * c;
    PMG_CALL(pmg_distmcsor_refresh_layout(U->dm, bf, NULL)); /* the rows of P^T read other ranks' rows of B */
    PMG_KERNEL(pmgk_csr_spmv_rows(U->R_nrows, U->R_rowpos, U->R_rowptr, U->R_col, U->R_val, bf, bc, 0, NULL, NULL));
    if (l == h->rb_fold) PMG_CALL(pmg_mgmc_i_rb_fold_allgather(h, bc, NULL)); /* the replicated level below takes the whole column */
  }
  /* (the refresh left copies on the ghost rows of the fine block, which counts every row once: it is dropped here) */
  setup_next_Bdev(s);
  if (l > h->rb_fold) return pmg_distmcsor_set_lowrank_dev(Cc->dm, h->lrc_k, s->Bdev, h->lrc_S);
  /* the highest replicated level: its whole block goes to the host in natural numbering, where the replicated levels below take over */
  double *Bl = (double *)setup_tmp(s, sizeof(double) * (size_t)Cc->ld * k), *B0 = (double *)malloc(sizeof(double) * (size_t)Cc->n * k);
  setup_own_B(s, B0);
  PMG_CHECK(Bl && B0, PMG_ERR_MEM, "out of host memory");
  PMG_HIP(hipMemcpy(Bl, s->Bdev, sizeof(double) * (size_t)Cc->ld * k, hipMemcpyDeviceToHost));
  for (int32_t c = 0; c < h->lrc_k; ++c)
    for (int32_t r = 0; r < Cc->n; ++r) B0[(size_t)Cc->n * c + r] = Bl[(size_t)Cc->ld * c + s->pos[l - 1][r]];
  if (l - 1 == 0) return pmg_chol_create_csr_lowrank(Cc->n, h->in[0].A_user.rp, h->in[0].A_user.ci, h->in[0].A_user.v, h->lrc_k, s->Bcur, h->lrc_S, &h->chol);
  return level_attach_lrc(h, Cc, s->Bcur);
}

static pmg_status setup_user_body(pmg_mgmc h, setup_scratch *s)
{
  const int top = h->nlevels - 1;
  int32_t **pos = s->pos;
  for (int l = 0; l <= top; ++l) {
    mg_level          *Lv = &h->lv[l];
    const mg_level_in *in = &h->in[l];
    PMG_CALL(user_level_check(h, l));
    pos[l] = (int32_t *)malloc(sizeof(int32_t) * (size_t)Lv->n);
    PMG_CHECK(pos[l], PMG_ERR_MEM, "out of host memory");
    Lv->kind     = in->rb ? MG_LV_ROWBLOCK : (l > 0 || h->coarse_type == 1 ? MG_LV_SELL : MG_LV_EXACT);
    Lv->transfer = l > 0 ? MG_TR_CSR : MG_TR_NONE;
    switch (Lv->kind) {
    case MG_LV_ROWBLOCK: PMG_CALL(user_level_rowblock(h, l, s)); break;
    case MG_LV_SELL: PMG_CALL(level_make_sell(h, l, &in->A_user, h->aij_coloring, NULL, pos[l])); break; /* PMG_COLORING_GREEDY unless pmg_mgmc_set_coloring said otherwise */
    case MG_LV_EXACT:
      Lv->ld = Lv->n;
      for (int32_t q = 0; q < Lv->n; ++q) pos[l][q] = q;
      if (!h->lrc_k) PMG_CALL(pmg_chol_create_csr(Lv->n, in->A_user.rp, in->A_user.ci, in->A_user.v, &h->chol));
      break;
    case MG_LV_GRID:
    case MG_LV_GRID_SLAB:
    case MG_LV_ST27: break; /* DMDA hierarchies only */
    }
  }
  s->Bcur = h->lrc_B; /* level-l block of the low-rank factor, natural numbering (owned by h at the top) */
  if (h->lrc_k && h->rb_dist) { /* row blocks: the block in the level's LAYOUT on the device, zero on the ghost rows */
    mg_level *T  = &h->lv[top];
    double   *Bl = (double *)setup_tmp(s, sizeof(double) * (size_t)T->ld * (size_t)h->lrc_k);
    PMG_CHECK(Bl, PMG_ERR_MEM, "out of host memory");
    for (int32_t c = 0; c < h->lrc_k; ++c)
      for (int32_t r = 0; r < T->rb_nowned; ++r) Bl[(size_t)T->ld * c + pos[top][r]] = s->Bcur[(size_t)T->n * c + r];
    PMG_CALL(pmg_dev_upload((void **)&s->Bdev, Bl, sizeof(double) * (size_t)T->ld * (size_t)h->lrc_k));
    PMG_CALL(pmg_distmcsor_set_lowrank_dev(T->dm, h->lrc_k, s->Bdev, h->lrc_S));
  } else if (h->lrc_k) PMG_CALL(level_attach_lrc(h, &h->lv[top], s->Bcur));
  for (int l = top; l >= 1; --l) {
    mg_level          *U = &h->lv[l], *Cc = &h->lv[l - 1];
    const mg_level_in *in = &h->in[l], *cin = &h->in[l - 1];
    const int          rb = U->kind == MG_LV_ROWBLOCK;
    if (!rb) PMG_CALL(pmg_hcsr_transpose(&in->P_user, &s->R));
    if (h->lrc_k && !rb) { /* B_{l-1} = P_l^T B_l, src/pc_gamgmc.c:177-178 */
      PMG_CALL(setup_restrict_attach_B(h, s, U, Cc));
      if (Cc->kind == MG_LV_EXACT) PMG_CALL(pmg_chol_create_csr_lowrank(Cc->n, cin->A_user.rp, cin->A_user.ci, cin->A_user.v, h->lrc_k, s->Bcur, h->lrc_S, &h->chol));
    }
    U->P_nrows = in->P_user.nr;
    U->R_nrows = rb ? in->R_user.nr : s->R.nr;
    PMG_CALL(upload_transfer(&in->P_user, pos[l], pos[l - 1], &U->P_rowpos, &U->P_rowptr, &U->P_col, &U->P_val));
    U->P_nnz = in->P_user.rp[in->P_user.nr];
    if (!rb) PMG_CALL(upload_transfer(&s->R, pos[l - 1], pos[l], &U->R_rowpos, &U->R_rowptr, &U->R_col, &U->R_val));
    else /* the caller's rows of P^T: owned rows of level l-1 (on the replicated coarsest level: this rank's block of the global rows) */
      PMG_CALL(upload_transfer(&in->R_user, pos[l - 1] + (l == h->rb_fold ? h->rb_c0_starts[h->rank] : 0), pos[l], &U->R_rowpos, &U->R_rowptr, &U->R_col, &U->R_val));
    if (rb && l == h->rb_fold && l - 1 >= 1) { /* the replicated level below keeps its vectors in a sliced-ELL layout: all-gather through natural order */
      int32_t *iota = (int32_t *)setup_tmp(s, sizeof(int32_t) * (size_t)Cc->n);
      PMG_CHECK(iota, PMG_ERR_MEM, "out of host memory");
      for (int32_t q = 0; q < Cc->n; ++q) iota[q] = q;
      PMG_CALL(pmg_dev_upload((void **)&h->rb_fold_pos, pos[l - 1], sizeof(int32_t) * (size_t)Cc->n));
      PMG_CALL(pmg_dev_upload((void **)&h->rb_fold_iota, iota, sizeof(int32_t) * (size_t)Cc->n));
      PMG_CALL(pmg_dev_alloc((void **)&h->rb_fold_buf, sizeof(double) * (size_t)Cc->n));
    }
    pmg_hcsr_free(&s->R);
    if (h->lrc_k && rb) PMG_CALL(user_rowblock_restrict_B(h, l, s));
  }
  PMG_CALL(alloc_level_vectors(h));
  h->n_io     = h->lv[top].n; /* the caller's vectors: one entry per (local) row of the finest level */
  h->is_setup = 1;
  return PMG_SUCCESS;
}

/* ---- DMDA hierarchy from the full Galerkin products --------------------------------------------------------------- */

static pmg_status setup_galerkin_body(pmg_mgmc h, setup_scratch *s, int no_stencil, int csr_transfers)
{
  const int top = h->nlevels - 1;
  int32_t **pos = s->pos; /* natural index -> layout position per level */
  /* finest level: matrix-free grid operator */
  mg_level *F = &h->lv[top];
  F->kind     = MG_LV_GRID;
  PMG_CALL(pmg_grid_create(F->nx, F->ny, F->nz, 0, F->nz, h->kappa, &F->g));
  h->own_grid = 1;
  PMG_CALL(pmg_grid_set_omega(F->g, h->omega));
  PMG_CALL(pmg_grid_set_sweep_type(F->g, h->sweep_type));
  PMG_CALL(pmg_grid_cvec_len(F->g, &F->ld));
  PMG_CHECK(F->ld < 2147483647, PMG_ERR_ARG_OUTOFRANGE, "fine level layout exceeds 32-bit positions");
  int64_t *p64 = (int64_t *)setup_tmp(s, sizeof(int64_t) * (size_t)F->n);
  pos[top]     = (int32_t *)malloc(sizeof(int32_t) * (size_t)F->n);
  PMG_CHECK(p64 && pos[top], PMG_ERR_MEM, "out of host memory");
  PMG_CALL(pmg_grid_get_layout(F->g, p64));
  for (int32_t q = 0; q < F->n; ++q) pos[top][q] = (int32_t)p64[q];
  rowsrc src;
  pmg_hier_laplace_rows(F->nx, F->ny, F->nz, h->kappa, 1. / ((F->nx - 1) * (F->nx - 1)) /* src/problems.c:24 */, &src);
  s->Bcur = h->lrc_B; /* level-l block of the low-rank factor, natural numbering (owned by h at the top) */
  if (h->lrc_k) PMG_CALL(level_attach_lrc(h, F, s->Bcur));
  for (int l = top; l >= 1; --l) {
    mg_level     *U = &h->lv[l], *Cc = &h->lv[l - 1];
    const int32_t nf[3] = {U->nx, U->ny, U->nz}, ncd[3] = {Cc->nx, Cc->ny, Cc->nz};
    PMG_CALL(pmg_hier_q1_interp(nf, ncd, &s->P));
    PMG_CALL(pmg_hcsr_transpose(&s->P, &s->R));
    rowsrc sl = src;
    if (l < top) sl.A = &s->Aprev;
    PMG_CALL(pmg_hier_galerkin_rap(&sl, l == top ? 7 : 64, &s->P, &s->R, &s->Ac));
    /* coarse level operator object: a class-stencil level if the operator is one, else a sliced-ELL level under the parity
       colouring; the Cholesky level keeps padded natural order */
    const int is_coarsest = (l - 1 == 0), sampled = !is_coarsest || h->coarse_type == 1;
    pos[l - 1]            = (int32_t *)malloc(sizeof(int32_t) * (size_t)Cc->n);
    PMG_CHECK(pos[l - 1], PMG_ERR_MEM, "out of host memory");
    Cc->kind = sampled ? MG_LV_SELL : MG_LV_EXACT;
    if (sampled && !no_stencil) PMG_CALL(st27_from_csr(Cc, &s->Ac, h->omega)); /* an MG_LV_ST27 level where the operator allows */
    if (Cc->kind != MG_LV_SELL) level_set_padded(Cc, pos[l - 1]);
    else {
      int32_t *col = (int32_t *)setup_tmp(s, sizeof(int32_t) * (size_t)Cc->n);
      PMG_CHECK(col, PMG_ERR_MEM, "out of host memory");
      pmg_hier_parity_colouring(Cc->nx, Cc->ny, Cc->nz, col);
      PMG_CALL(level_make_sell(h, l - 1, &s->Ac, PMG_COLORING_USER, col, pos[l - 1]));
    }
    if (h->lrc_k) PMG_CALL(setup_restrict_attach_B(h, s, U, Cc));
    if (is_coarsest && h->coarse_type == 0) PMG_CALL(pmg_chol_create_csr_lowrank(Cc->n, s->Ac.rp, s->Ac.ci, s->Ac.v, h->lrc_k, s->Bcur, h->lrc_S, &h->chol));
    /* transfers: matrix-free Q1 kernels from the grid level and between natural-order levels, CSR products in
       layout numbering otherwise */
    if (U->kind == MG_LV_GRID && !csr_transfers) {
      U->transfer = MG_TR_Q1_GRID;
      if (!Cc->padded) PMG_CALL(pmg_dev_upload((void **)&U->cpos_dev, pos[l - 1], sizeof(int32_t) * (size_t)Cc->n));
    } else if (U->kind == MG_LV_ST27 && Cc->padded && !csr_transfers) U->transfer = MG_TR_Q1_NAT;
    else {
      U->transfer = MG_TR_CSR;
      U->P_nrows = s->P.nr;
      U->R_nrows = s->R.nr;
      PMG_CALL(upload_transfer(&s->P, pos[l], pos[l - 1], &U->P_rowpos, &U->P_rowptr, &U->P_col, &U->P_val));
      U->P_nnz = s->P.rp[s->P.nr];
      PMG_CALL(upload_transfer(&s->R, pos[l - 1], pos[l], &U->R_rowpos, &U->R_rowptr, &U->R_col, &U->R_val));
    }
    pmg_hcsr_free(&s->R);
    if (h->keep_host) { /* for inspection: the interpolation itself, a deep copy of the operator */
      hcsr_move(&U->P_host, &s->P);
      PMG_CALL(pmg_hcsr_dup(&s->Ac, &Cc->A_host));
    } else pmg_hcsr_free(&s->P);
    pmg_hcsr_free(&s->Aprev);
    hcsr_move(&s->Aprev, &s->Ac);
  }
  PMG_CALL(alloc_level_vectors(h));
  h->is_setup = 1;
  return PMG_SUCCESS;
}

/* ---- DMDA hierarchy from class-stencil tables --------------------------------------------------------------------- */

/* MATLRC operators of a class-stencil hierarchy (PCGAMGMC_SetUpHierarchy, src/pc_gamgmc.c:157-196): the factor B of the
   finest level is restricted level by level ON THE DEVICE, column by column, with the restriction kernels of the
   V-cycle (B_{l-1} = P_l^T B_l, :177), every level sampler gets A_l + B_l S B_l^T; the coarsest block is left in s->Bcur in
   natural numbering for the dense factorisation (src/pc_chols.c:119-153). */
static pmg_status stencil_attach_lowrank(pmg_mgmc h, setup_scratch *s)
{
  const int     top = h->nlevels - 1, k = h->lrc_k;
  mg_level     *F   = &h->lv[top];
  const int32_t nrows = h->dist ? h->n_io : F->n;
  PMG_CALL(pmg_dev_alloc((void **)&s->Bdev, sizeof(double) * (size_t)F->ld * k));
  PMG_CALL(pmg_dev_alloc((void **)&s->Bdev2, sizeof(double) * (size_t)nrows));
  for (int c = 0; c < k; ++c) { /* natural host column (this rank's planes) -> cvec */
    PMG_HIP(hipMemcpy(s->Bdev2, h->lrc_B + (size_t)nrows * c, sizeof(double) * (size_t)nrows, hipMemcpyHostToDevice));
    PMG_CALL(pmg_grid_to_cvec(F->g, s->Bdev2, s->Bdev + (size_t)F->ld * c, NULL));
  }
  PMG_HIP(hipDeviceSynchronize());
  pmg_dev_free(s->Bdev2);
  s->Bdev2 = NULL;
  if (h->dist) PMG_CALL(pmg_lrc_build_dev(&F->lrc, k, F->ld, s->Bdev, h->lrc_S, dist_det_sweep, h, F->distributed ? mg_reduce : NULL, h)); /* the slab sweeps run in pmg_dist: the update is applied around them here */
  else PMG_CALL(pmg_grid_set_lowrank_dev(F->g, k, s->Bdev, h->lrc_S));
  for (int l = top; l >= 1; --l) {
    mg_level *Lv = &h->lv[l], *Cc = &h->lv[l - 1];
    PMG_CALL(pmg_dev_alloc((void **)&s->Bdev2, sizeof(double) * (size_t)Cc->ld * k));
    for (int c = 0; c < k; ++c) PMG_CALL(pmg_mgmc_i_restrict(h, l, s->Bdev + (size_t)Lv->ld * c, s->Bdev2 + (size_t)Cc->ld * c, NULL)); /* B_{l-1} = P_l^T B_l */
    PMG_HIP(hipDeviceSynchronize());
    setup_next_Bdev(s);
    if (Cc->kind == MG_LV_ST27) { /* a sampled level (not the Cholesky level) */
      level_ref ref = {h, Cc};
      PMG_CALL(pmg_lrc_build_dev(&Cc->lrc, k, Cc->ld, s->Bdev, h->lrc_S, st27_det_sweep, &ref, Cc->distributed ? mg_reduce : NULL, h));
    }
  }
  /* coarsest block to the host, natural numbering (the padded layout minus its ghost planes) */
  mg_level *C0 = &h->lv[0];
  double   *B0 = (double *)malloc(sizeof(double) * (size_t)C0->n * k);
  setup_own_B(s, B0);
  PMG_CHECK(B0, PMG_ERR_MEM, "out of host memory");
  for (int c = 0; c < k; ++c) PMG_HIP(hipMemcpy(B0 + (size_t)C0->n * c, s->Bdev + (size_t)C0->ld * c + C0->off, sizeof(double) * (size_t)C0->n, hipMemcpyDeviceToHost));
  return PMG_SUCCESS;
}

/* z-slab grid level l: whether the cycle may fuse residual and restriction there (Lv->rr_slab, with the two-plane
   buffers of the iterate).  Every rank needs two planes (it hands its second and second-to-last ones to the neighbours) and a coarse plane of its own -- decided from the cuts, identically on every rank -- AND the
   kernel must accept this rank's own slab (limits that depend on the local layout: slabs differ by a plane).  Every
   rank dry-runs the kernel's predicate on its slab and the ranks agree with one all-reduce: a rank that would be
   refused in the cycle (after its peers had entered the next halo) makes all of them keep the two-kernel form */
static pmg_status slab_agree_fused_rr(pmg_mgmc h, int l)
{
  mg_level *Lv = &h->lv[l];
  if (!(Lv->kind == MG_LV_GRID_SLAB && Lv->distributed && Lv->transfer == MG_TR_Q1_GRID && !Lv->cpos_dev && !h->no_fused && (!h->lrc_k || (mg_level_cycle_lrc(h, l) && mg_level_cycle_lrc(h, l - 1))) && pmg_switch(PMG_SW_GRID_FUSED_RR_SLAB))) return PMG_SUCCESS;
  const int32_t *fc = h->cuts + (size_t)l * (size_t)(h->nranks + 1), *cc = h->cuts + (size_t)(l - 1) * (size_t)(h->nranks + 1);
  int            ok = 1;
  for (int r = 0; r < h->nranks; ++r) ok = ok && fc[r + 1] - fc[r] >= 2 && cc[r + 1] - cc[r] >= 1;
  if (ok) {
    pmgk_st27_dims CD = level_dims(&h->lv[l - 1]);
    CD.kz0            = cc[h->rank];
    CD.nz             = cc[h->rank + 1] - cc[h->rank];
    double  mine      = pmg_grid_residual_restrict_applies(Lv->g, &CD, 1, 1) ? 1.0 : 0.0, all = 0.0;
    double *flag      = NULL;
    PMG_CALL(pmg_dev_alloc((void **)&flag, sizeof(double)));
    pmg_status st = hipMemcpy(flag, &mine, sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? PMG_SUCCESS : pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "upload failed");
    if (!st) st = pmg_dist_allreduce_sum(h->dist, flag, 1, NULL);
    if (!st && hipMemcpy(&all, flag, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) st = pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "download failed");
    pmg_dev_free(flag);
    PMG_CALL(st);
    ok = all == (double)h->nranks;
  }
  if (ok) {
    int64_t own, ghost, np;
    PMG_CALL(pmg_grid_halo_plane(Lv->g, 0, 0, &own, &ghost, &np));
    PMG_CALL(pmg_dev_alloc((void **)&Lv->y2lo, sizeof(double) * 2 * (size_t)np));
    PMG_CALL(pmg_dev_alloc((void **)&Lv->y2hi, sizeof(double) * 2 * (size_t)np));
    Lv->rr_slab = 1;
  }
  return PMG_SUCCESS;
}

/* set-up from class-stencil tables (s->tab): every level below the grid level is a class-stencil level in padded natural
   order, transfers are the matrix-free Q1 kernels, the coarsest level is factored from the expanded table */
static pmg_status setup_stencil_body(pmg_mgmc h, setup_scratch *s)
{
  const st27_table *tab = s->tab;
  const int top = h->nlevels - 1;
  mg_level *F   = &h->lv[top];
  F->kind       = h->dist ? MG_LV_GRID_SLAB : MG_LV_GRID;
  F->transfer   = MG_TR_Q1_GRID;
  if (!F->g) {
    PMG_CALL(pmg_grid_create(F->nx, F->ny, F->nz, 0, F->nz, h->kappa, &F->g));
    h->own_grid = 1;
  }
  PMG_CALL(pmg_grid_set_omega(F->g, h->omega));
  PMG_CALL(pmg_grid_set_sweep_type(F->g, h->sweep_type));
  PMG_CALL(pmg_grid_cvec_len(F->g, &F->ld));
  if (h->dist) { /* which levels stay distributed */
    const int nr1 = h->nranks + 1;
    int64_t   cap = 0, rep = pmg_switch_wide(PMG_SW_MG_REPLICATE_BELOW); /* default 2^19 */
    PMG_CALL(pmg_dist_get_info(h->dist, NULL, NULL, &cap));
    F->distributed = h->nranks > 1;
    int replicated = !F->distributed;
    for (int l = top - 1; l >= 0; --l) {
      mg_level      *Lv = &h->lv[l];
      const int32_t *c  = h->cuts + (size_t)l * nr1;
      int            minplanes = 1 << 30;
      for (int r = 0; r < h->nranks; ++r) minplanes = c[r + 1] - c[r] < minplanes ? c[r + 1] - c[r] : minplanes;
      if (!replicated && (Lv->n <= rep || minplanes < 1 || l == 0)) replicated = 1;
      if (replicated) {
        PMG_CHECK(!h->lv[l + 1].distributed || Lv->n <= cap, PMG_ERR_SUP, "level %d (%d unknowns) has to be replicated but exceeds the exchange capacity (%lld): use more levels", l, Lv->n, (long long)cap);
      } else {
        Lv->distributed = 1;
        Lv->kz0         = c[h->rank];
        Lv->nzl         = c[h->rank + 1] - c[h->rank];
      }
    }
  }
  for (int l = top - 1; l >= 0; --l) {
    mg_level *Lv = &h->lv[l];
    level_set_padded(Lv, NULL);
    if (l > 0 || h->coarse_type == 1) PMG_CALL(st27_install(Lv, tab[l].coef, tab[l].have, h->omega));
    else Lv->kind = MG_LV_EXACT;
    if (l > 0) Lv->transfer = MG_TR_Q1_NAT;
  }
  if (h->lrc_k) PMG_CALL(stencil_attach_lowrank(h, s)); /* leaves the coarsest block in s->Bcur */
  if (h->coarse_type == 0) {
    mg_level *C0 = &h->lv[0];
    PMG_CHECK(!C0->distributed, PMG_ERR_SUP, "the Cholesky level must not be distributed");
    PMG_CALL(pmg_hier_st27_to_csr(C0->nx, C0->ny, C0->nz, &tab[0], &s->Ac));
    PMG_CALL(pmg_chol_create_csr_lowrank(C0->n, s->Ac.rp, s->Ac.ci, s->Ac.v, h->lrc_k, s->Bcur, h->lrc_S, &h->chol));
  }
  PMG_CALL(alloc_level_vectors(h));
  for (int l = 1; l <= top; ++l) PMG_CALL(slab_agree_fused_rr(h, l));
  h->is_setup = 1;
  return PMG_SUCCESS;
}

/* the DMDA routes.  PMG_MG_FULL_GALERKIN, PMG_MG_NO_STENCIL and PMG_MG_CSR_TRANSFERS are read here, once per set-up */
static pmg_status setup_dmda_body(pmg_mgmc h, setup_scratch *s)
{
  const int top = h->nlevels - 1;
  const int full_galerkin = pmg_switch(PMG_SW_MG_FULL_GALERKIN), no_stencil = pmg_switch(PMG_SW_MG_NO_STENCIL), csr_transfers = pmg_switch(PMG_SW_MG_CSR_TRANSFERS);
  if (h->dist) PMG_CHECK(!h->keep_host, PMG_ERR_SUP, "host copies of the level matrices are a single-device feature");
  if (h->dist || (!h->keep_host && !full_galerkin && !no_stencil && !csr_transfers)) {
    /* class-stencil tables from the proxy hierarchy: no product with the full-size matrices */
    int32_t dims[64][3];
    int     ok = 0;
    PMG_CHECK(h->nlevels <= 64, PMG_ERR_ARG_OUTOFRANGE, "too many levels");
    for (int l = 0; l <= top; ++l) dims[l][0] = h->lv[l].nx, dims[l][1] = h->lv[l].ny, dims[l][2] = h->lv[l].nz;
    s->tab = (st27_table *)malloc(sizeof(st27_table) * (size_t)top);
    PMG_CHECK(s->tab, PMG_ERR_MEM, "out of host memory");
    PMG_CALL(pmg_hier_stencil_tables(h->nlevels, dims, h->kappa, 1. / ((h->lv[top].nx - 1) * (h->lv[top].nx - 1)) /* src/problems.c:24, the TRUE grid's spacing */, s->tab, &ok));
    if (ok) return setup_stencil_body(h, s);
    PMG_CHECK(!h->dist, PMG_ERR_SUP, "the coarse operators of this grid are not class stencils; z-slabs need them");
  }
  return setup_galerkin_body(h, s, no_stencil, csr_transfers);
}

pmg_status pmg_mgmc_setup(pmg_mgmc h)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  if (h->is_setup) return PMG_SUCCESS;
  setup_scratch s = {0};
  s.nlevels     = h->nlevels;
  s.pos         = (int32_t **)calloc((size_t)h->nlevels, sizeof(int32_t *));
  pmg_status st = s.pos ? PMG_SUCCESS : pmg_set_error(PMG_ERR_MEM, __FILE__, __LINE__, "out of host memory");
  if (!st) st = h->user_hier ? setup_user_body(h, &s) : setup_dmda_body(h, &s);
  setup_release(&s);
  if (!st) pmg_mgmc_i_free_inputs(h); /* a failed set-up keeps them */
  return st;
}

void pmg_mgmc_i_free_inputs(pmg_mgmc h)
{
  for (int l = 0; l < h->nlevels && h->in; ++l) {
    mg_level_in *in = &h->in[l];
    free(in->A_rp_own), free(in->A_ci_own), free(in->P_rp_own), free(in->P_ci_own);
    free(in->rb_colors), free(in->rb_send_ptr), free(in->rb_recv_ptr), free(in->rb_counts), free(in->rb_send_idx), free(in->rb_recv_src), free(in->rb_recv_idx);
    free(in->bg_blockptr), free(in->bg_blockrows), free(in->bg_colors);
    memset(in, 0, sizeof *in); /* the borrowed matrices with them */
  }
}

pmg_status pmg_mgmc_destroy(pmg_mgmc *hp)
{
  if (!hp || !*hp) return PMG_SUCCESS;
  pmg_mgmc h = *hp;
  for (int l = 0; l < h->nlevels; ++l) {
    mg_level *Lv = &h->lv[l];
    if (h->own_grid) pmg_grid_destroy(&Lv->g); /* (a slab's grid is the caller's, set up or not) */
    pmg_distmcsor_destroy(&Lv->dm);
    pmg_mcsor_destroy(&Lv->mc);
    pmg_blockgibbs_destroy(&Lv->bg);
    pmg_dev_free(Lv->b);
    pmg_dev_free(Lv->x);
    pmg_dev_free(Lv->r);
    pmg_dev_free(Lv->x2);
    pmg_dev_free(Lv->y2lo);
    pmg_dev_free(Lv->y2hi);
    pmg_dev_free(Lv->cpos_dev);
    pmg_dev_free(Lv->st_coef);
    pmg_dev_free(Lv->st_idiag);
    pmg_dev_free(Lv->st_sqrtd);
    pmg_dev_free(Lv->st_sqrtd_scaled);
    pmg_lrc_destroy(&Lv->lrc);
    pmg_dev_free(Lv->P_rowpos);
    pmg_dev_free(Lv->P_rowptr);
    pmg_dev_free(Lv->P_col);
    pmg_dev_free(Lv->P_val);
    pmg_dev_free(Lv->R_rowpos);
    pmg_dev_free(Lv->R_rowptr);
    pmg_dev_free(Lv->R_col);
    pmg_dev_free(Lv->R_val);
    pmg_hcsr_free(&Lv->A_host);
    pmg_hcsr_free(&Lv->P_host);
  }
  pmg_mgmc_i_free_inputs(h);
  free(h->in);
  pmg_mgmc_i_free_chains(h);
  pmg_chol_destroy(&h->chol);
  pmg_dev_free(h->y_lay);
  pmg_dev_free(h->b_lay);
  pmg_dev_free(h->eta_batch);
  free(h->lrc_B);
  free(h->lrc_S);
  free(h->cuts);
  free(h->rb_c0_starts);
  pmg_dev_free(h->rb_fold_pos);
  pmg_dev_free(h->rb_fold_iota);
  pmg_dev_free(h->rb_fold_buf);
  free(h->lv);
  free(h);
  *hp = NULL;
  return PMG_SUCCESS;
}
