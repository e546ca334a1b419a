/* Multigrid Monte Carlo sampler on a DMDA hierarchy -- host side (C11).
 *
 * Mirrors PCGAMGMC with `-pc_gamgmc_mg_type mg` (reference src/pc_gamgmc.c) together with the part of PETSc's PCMG
 * it drives (third party, restated from PETSc's documented semantics -- parity unpinned by any reference fixture):
 *   - hierarchy: vertex-centred 2:1 coarsening nc = (nf-1)/2 + 1, Q1 (bi/tri-linear) interpolation as DMDA's
 *     DMCreateInterpolation builds it, restriction R = P^T, Galerkin coarse operators A_c = P^T A P
 *     (-pc_mg_galerkin both, injected at src/pc_gamgmc.c:345-349);
 *   - level "smoothers" = Gibbs samplers (default sorgibbs, KSPRICHARDSON, max_it 1: src/pc_gamgmc.c:318-334),
 *     coarse "solver" = exact Cholesky sampler (src/pc_gamgmc.c:336-342) or Gibbs sweeps (examples/ex1.c:35);
 *   - one V-cycle: pre-smooth, r = b - A x, b_c = P^T r, recurse from x_c = 0, x += P x_c, post-smooth;
 *   - the outer chain in correction form, PCApplyRichardson_GAMGMC (src/pc_gamgmc.c:227-264):
 *     first iteration from a zero guess y = MG(b), afterwards w = b - A y, y += MG(w); callback per sample.
 * The finest level is the matrix-free red-black grid operator (pmg_grid).  The coarser levels of a DMDA hierarchy are
 * class-stencil levels by default: the 9/27-point Galerkin operators as 27 x 27 position-class tables, vectors in
 * plane-padded natural order, swept under the 4/8-colour parity colouring (red-black is not a valid colouring of a
 * 27-point stencil), with matrix-free Q1 transfers between them and from the grid level, and the exact coarse sampler
 * on the expanded table.  Sliced-ELL levels with CSR transfers in layout numbering serve caller-supplied (AIJ)
 * hierarchies, whole or by row blocks, and the DMDA routes behind PMG_MG_NO_STENCIL / PMG_MG_CSR_TRANSFERS /
 * PMG_MG_FULL_GALERKIN and pmg_mgmc_set_keep_host.  z-slab hierarchies add a halo per sweep phase and fold into
 * replicated coarse levels.
 *
 * This file is the cycle: a level's kind (mg_kind, set once by the set-up) selects its sampler and residual, its transfer kind
 * the restriction and prolongation; level_path decides what remains open from cycle to cycle, mg_vcycle launches them,
 * pmg_mgmc_get_algorithmic_bytes charges them, pmg_mgmc_sample runs the outer chain.  The hierarchy is built in
 * pmg_mgmc_setup.c (host sparse tools: pmg_hier_host.c); the multi-chain cycle is pmg_mgmc_chains.c, the single-kernel
 * diagnostics pmg_mgmc_level.c; pmg_mgmc_internal.h holds what they share.
 */
#include "pmg_mgmc_internal.h"

/* the phase-fused out-of-place sweep and the paired residual (kernels_stencil27_pair.hip) serve class-stencil levels
   that live on one device; PMG_ST27_PAIR=0 keeps the one-launch-per-colour kernels (same bits) */
static int st27_use_pair(const mg_level *Lv) { return pmg_switch(PMG_SW_ST27_PAIR) && Lv->kind == MG_LV_ST27 && !Lv->distributed && Lv->kz0 == 0 && Lv->nzl == Lv->nz; }

/* the same kernels on the z-slab of a distributed class-stencil level: one launch per z-parity phase instead of four, the
   halo of the boundary planes behind each as before; PMG_ST27_PAIR_SLAB=0 keeps the per-colour kernels (same bits; probes:
   2 = paired residual only, 3 = paired sweeps only) */
static int st27_use_pair_slab(const mg_level *Lv) { return pmg_switch(PMG_SW_ST27_PAIR_SLAB) && Lv->kind == MG_LV_ST27 && Lv->distributed; }

/* the level's own iterate is swept out of place, into Lv->x2 */
int pmg_mgmc_i_st27_out_of_place(const mg_level *Lv) { return Lv->x2 && st27_use_pair(Lv); }

/* the second iterate buffer of those kernels: which levels get one at set-up */
int pmg_mgmc_i_level_wants_x2(const mg_level *Lv) { return st27_use_pair(Lv) || st27_use_pair_slab(Lv); }

/* one directional sweep of a class-stencil level on (b, *x): in place, or out of place into Lv->x2 followed by a swap of
   the two buffers when x is the level's own iterate */
static void st27_swap(mg_level *Lv)
{
  double *t = Lv->x;
  Lv->x     = Lv->x2;
  Lv->x2    = t;
}

static pmg_status st27_one_sweep(mg_level *Lv, const pmgk_st27 *S, int backward, double omega, int noisy, uint64_t seed, uint64_t sweep, const double *b, int x_is_zero, void *stream)
{
  if (pmg_mgmc_i_st27_out_of_place(Lv)) {
    /* x_is_zero: the iterate is the zero vector and has NOT been stored (level_iterate_is_unset): the sweep neither reads it
       nor needs the memset */
    PMG_KERNEL(pmgk_st27_sweep_pp(S, backward, omega, noisy, seed, sweep, b, x_is_zero ? NULL : Lv->x, Lv->x2, stream));
    st27_swap(Lv);
    return PMG_SUCCESS;
  }
  PMG_KERNEL(pmgk_st27_sweep(S, backward, omega, noisy, seed, sweep, b, Lv->x, stream));
  return PMG_SUCCESS;
}

/* a vector of the highest replicated level of a row-block hierarchy, of which every rank has computed the rows of its block
   (coarse row blocks rb_c0_starts): all ranks end up with all rows.  The coarsest level keeps natural order (one all-gather
   in place); a sliced-ELL level goes through natural order: gather my block, all-gather, scatter everything. */
pmg_status pmg_mgmc_i_rb_fold_allgather(pmg_mgmc h, double *v, void *stream)
{
  int64_t cnts[64];
  for (int r = 0; r < h->nranks; ++r) cnts[r] = h->rb_c0_starts[r + 1] - h->rb_c0_starts[r];
  if (!h->rb_fold_pos) return pmg_dist_allgather(h->rb_dist, v, h->rb_c0_starts, cnts, stream);
  const int64_t s0 = h->rb_c0_starts[h->rank], n = h->rb_c0_starts[h->nranks];
  PMG_KERNEL(pmgk_gather_idx(cnts[h->rank], h->rb_fold_pos + s0, v, h->rb_fold_buf + s0, stream));
  PMG_CALL(pmg_dist_allgather(h->rb_dist, h->rb_fold_buf, h->rb_c0_starts, cnts, stream));
  PMG_KERNEL(pmgk_scatter_idx(n, h->rb_fold_iota, h->rb_fold_pos, h->rb_fold_buf, v, stream));
  return PMG_SUCCESS;
}

/* z-neighbour halo of a vector of a distributed level: the boundary planes travel to the neighbours' ghost planes */
pmg_status pmg_mgmc_i_halo_level(pmg_mgmc h, mg_level *Lv, double *v, void *stream)
{
  if (!Lv->distributed) return PMG_SUCCESS;
  const double *slo[2], *shi[2];
  double       *rlo[2], *rhi[2];
  int64_t       n[2];
  switch (Lv->kind) {
  case MG_LV_GRID_SLAB: /* cvec: one block per colour */
    for (int c = 0; c < 2; ++c) {
      int64_t own, ghost;
      PMG_CALL(pmg_grid_halo_plane(Lv->g, c, 0, &own, &ghost, &n[c]));
      slo[c] = v + own;
      rlo[c] = v + ghost;
      PMG_CALL(pmg_grid_halo_plane(Lv->g, c, 1, &own, &ghost, &n[c]));
      shi[c] = v + own;
      rhi[c] = v + ghost;
    }
    return pmg_dist_exchange(h->dist, 2, slo, n, rlo, n, shi, n, rhi, n, stream);
  case MG_LV_ST27: /* padded natural order: one plane below, one above */
    n[0]   = Lv->off;
    slo[0] = v + Lv->off;
    rlo[0] = v;
    shi[0] = v + Lv->off * Lv->nzl;
    rhi[0] = v + Lv->off * ((int64_t)Lv->nzl + 1);
    return pmg_dist_exchange(h->dist, 1, slo, n, rlo, n, shi, n, rhi, n, stream);
  case MG_LV_EXACT:
  case MG_LV_GRID:
  case MG_LV_SELL:
  case MG_LV_ROWBLOCK: break; /* never z-slabs */
  }
  return PMG_SUCCESS;
}

/* `its` samples of a level sampler whose low-rank update is applied around the sweeps HERE (class-stencil levels, the grid
   level of a z-slab hierarchy): noise term, directional sweep (the part that differs), repair, halo */
typedef pmg_status (*mg_dir_sweep)(pmg_mgmc h, mg_level *Lv, int dir, const double *rhs, uint64_t seed, uint64_t *ctr, void *stream);

typedef struct {
  pmg_mgmc     h;
  mg_level    *Lv;
  mg_dir_sweep sweep;
  uint64_t     seed, *ctr;
} mg_sweep_args;

/* the level's directional sweep as a pmg_det_sweep_fn: it sweeps the level's own iterate and advances the level's counter */
static pmg_status mg_one_sweep(void *ctx, int dir, const double *rhs, double *x, void *stream)
{
  const mg_sweep_args *a = (const mg_sweep_args *)ctx;
  (void)x;
  return a->sweep(a->h, a->Lv, dir, rhs, a->seed, a->ctr, stream);
}

static pmg_status mg_lowrank_sweeps(pmg_mgmc h, int l, int its, mg_dir_sweep sweep, uint64_t seed, uint64_t *ctr, void *stream)
{
  mg_level      *Lv = &h->lv[l];
  pmg_lrc        lr = mg_level_cycle_lrc(h, l);
  mg_sweep_args  a  = {h, Lv, sweep, seed, ctr};
  pmg_sweep_iter it = pmg_sweep_begin(h->sweep_type, its, 1, *ctr);
  while (pmg_sweep_next(&it)) {
    PMG_CALL(pmg_lrc_dir_sweep(lr, 1, it.dir, seed, *ctr, mg_one_sweep, &a, Lv->b, &Lv->x, stream)); /* an out-of-place sweep swaps Lv->x */
    if (lr) PMG_CALL(pmg_mgmc_i_halo_level(h, Lv, Lv->x, stream)); /* the repair changed boundary planes */
  }
  return PMG_SUCCESS;
}

/* class-stencil level (same draw numbering as pmg_mcsor_sample_layout); on a z-slab the two z-parity phases of a sweep are
   separated by a halo of the boundary planes.  The set-up builds the levels' low-rank updates with the deterministic form */
pmg_status pmg_mgmc_i_st27_dir_sweep(pmg_mgmc h, mg_level *Lv, int dir, int noisy, const double *rhs, double *y, uint64_t seed, uint64_t *ctr, void *stream)
{
  const int backward = dir == PMG_SOR_BACKWARD_SWEEP;
  pmgk_st27 S        = Lv->st;
  S.sqrtdiag         = h->scaled ? Lv->st_sqrtd_scaled : Lv->st_sqrtd;
  if (!noisy) seed = 0;
  const uint64_t draw = noisy ? *ctr : 0;
  if (!Lv->distributed) {
    if (!noisy) PMG_KERNEL(pmgk_st27_sweep(&S, backward, h->omega, 0, seed, draw, rhs, y, stream));
    else {
      PMG_CALL(st27_one_sweep(Lv, &S, backward, h->omega, 1, seed, (*ctr)++, rhs, Lv->x_unset, stream));
      Lv->x_unset = 0;
    }
    return PMG_SUCCESS;
  }
  const int pp  = noisy && Lv->x2 && st27_use_pair_slab(Lv) && pmg_switch(PMG_SW_ST27_PAIR_SLAB) != 2; /* out of place: x2 <- sweep(x), phase by phase, then the buffers swap */
  double   *out = !noisy ? y : (pp ? Lv->x2 : Lv->x);
  for (int phase = 0; phase < 2; ++phase) {
    if (pp) PMG_KERNEL(pmgk_st27_sweep_pp_phase(&S, backward, phase, h->omega, 1, seed, draw, rhs, Lv->x, out, stream));
    else PMG_KERNEL(pmgk_st27_sweep_phase(&S, backward, phase, h->omega, noisy, seed, draw, rhs, out, stream));
    PMG_CALL(pmg_mgmc_i_halo_level(h, Lv, out, stream));
  }
  if (noisy) ++*ctr;
  if (pp) st27_swap(Lv);
  return PMG_SUCCESS;
}

static pmg_status st27_dir_sweep(pmg_mgmc h, mg_level *Lv, int dir, const double *rhs, uint64_t seed, uint64_t *ctr, void *stream)
{
  return pmg_mgmc_i_st27_dir_sweep(h, Lv, dir, 1, rhs, NULL, seed, ctr, stream);
}

/* grid level of a z-slab hierarchy: one slab sweep (leaves the ghost planes current) */
static pmg_status slab_dir_sweep(pmg_mgmc h, mg_level *Lv, int dir, const double *rhs, uint64_t seed, uint64_t *ctr, void *stream)
{
  return pmg_dist_sample_cvec(h->dist, rhs, Lv->x, 1, h->scaled, dir, seed, *ctr, ctr, stream);
}

/* `its` samples of a level smoothed by block sweeps (pmg_mgmc_set_level_blocks): the slot stream of the level's key, one draw
   counter per directional sweep like every other level sampler.  The sweep reads the iterate outside each block, so it needs the
   zero guess STORED: a sliced-ELL level gets it from the fill kernel or from the restriction into it (x_zeroed: every row of the
   level is a row of P^T, the layout padding is zero since the allocation and is never written). */
static pmg_status mg_block_sweeps(pmg_mgmc h, mg_level *Lv, int its, uint64_t seed, uint64_t *ctr, void *stream)
{
  pmg_sweep_iter it = pmg_sweep_begin(h->sweep_type, its, 1, *ctr);
  while (pmg_sweep_next(&it)) PMG_CALL(pmg_blockgibbs_dir_sweep(Lv->bg, it.dir, 1, seed, it.sweep, NULL, Lv->b, Lv->x, stream));
  *ctr = it.ctr;
  return PMG_SUCCESS;
}

/* one smoothing leg of level l on (Lv->b, Lv->x): `its` samples of the level's sampler (nu; coarse_its on level 0, where the exact
   sampler draws its one sample whatever `its`).  The set-up's checks keep the grid and row-block kinds off level 0 */
static pmg_status mg_smooth(pmg_mgmc h, int l, int its, uint64_t seed, uint64_t *ctr, void *stream)
{
  mg_level      *Lv  = &h->lv[l];
  const uint64_t key = level_seed(seed, l);
  switch (Lv->kind) {
  case MG_LV_EXACT: return pmg_chol_sample(h->chol, Lv->b + Lv->off, Lv->x + Lv->off, 1, key, *ctr, stream);
  case MG_LV_GRID: return pmg_grid_sample_cvec(Lv->g, Lv->b, Lv->x, its, h->scaled, key, *ctr, ctr, stream);
  case MG_LV_GRID_SLAB:
    if (mg_level_cycle_lrc(h, l)) return mg_lowrank_sweeps(h, l, its, slab_dir_sweep, key, ctr, stream);
    return pmg_dist_sample_cvec(h->dist, Lv->b, Lv->x, its, h->scaled, h->sweep_type, key, *ctr, ctr, stream); /* leaves the ghost planes current */
  case MG_LV_ST27: return mg_lowrank_sweeps(h, l, its, st27_dir_sweep, key, ctr, stream);
  case MG_LV_SELL:
    if (Lv->bg) return mg_block_sweeps(h, Lv, its, key, ctr, stream);
    return pmg_mcsor_sample_layout(Lv->mc, Lv->b, Lv->x, its, h->scaled, key, *ctr, ctr, stream);
  case MG_LV_ROWBLOCK: return pmg_distmcsor_sample_layout(Lv->dm, Lv->b, Lv->x, its, h->scaled, h->sweep_type, key, *ctr, ctr, stream); /* refreshes the ghost rows first, leaves them current */
  }
  return PMG_SUCCESS;
}

/* r = b - A_l x by the level's residual kernel; the low-rank term of an update the LEVEL holds (mg_level_cycle_lrc) is the caller's */
static pmg_status mg_residual(mg_level *Lv, int pair, const double *b, const double *x, double *r, void *stream)
{
  switch (Lv->kind) {
  case MG_LV_GRID:
  case MG_LV_GRID_SLAB: return pmg_grid_residual_cvec(Lv->g, b, x, r, stream);
  case MG_LV_ST27:
    if (pair) PMG_KERNEL(pmgk_st27_residual_pair(&Lv->st, b, x, r, stream));
    else PMG_KERNEL(pmgk_st27_residual(&Lv->st, b, x, r, stream));
    return PMG_SUCCESS;
  case MG_LV_SELL: return pmg_mcsor_residual_layout(Lv->mc, b, x, r, stream);
  case MG_LV_ROWBLOCK: return pmg_distmcsor_residual_layout(Lv->dm, b, x, r, stream); /* + the all-reduced low-rank term */
  case MG_LV_EXACT: break;
  }
  PMG_FAIL(PMG_ERR_PLIB, "an exactly sampled level has no residual kernel");
}

/* Level l distributed, level l - 1 replicated (the fold): a rank restricts into the coarse planes it owns -- CD becomes
   those planes, the vector is returned shifted to them (plane K of the full-size vector = plane K - kz0 of the shifted
   one) -- and an all-gather of the planes completes the vector on every rank */
static double *fold_own_planes(pmg_mgmc h, int l, pmgk_st27_dims *CD, double *b_coarse)
{
  const int32_t *cc = h->cuts + (size_t)(l - 1) * (size_t)(h->nranks + 1);
  CD->kz0           = cc[h->rank];
  CD->nz            = cc[h->rank + 1] - cc[h->rank];
  return b_coarse + h->lv[l - 1].off * CD->kz0;
}

static pmg_status fold_allgather(pmg_mgmc h, int l, double *b_coarse, void *stream)
{
  const mg_level *Cc = &h->lv[l - 1];
  const int32_t  *cc = h->cuts + (size_t)(l - 1) * (size_t)(h->nranks + 1);
  int64_t         offs[64], cnts[64];
  PMG_CHECK(h->nranks <= 64, PMG_ERR_ARG_OUTOFRANGE, "too many ranks");
  for (int r = 0; r < h->nranks; ++r) {
    offs[r] = Cc->off * ((int64_t)cc[r] + 1);
    cnts[r] = Cc->off * (int64_t)(cc[r + 1] - cc[r]);
  }
  return pmg_dist_allgather(h->dist, b_coarse, offs, cnts, stream);
}

/* b_coarse = P_l^T r_fine (MatRestrict).  A z-slab restricts into the coarse planes it owns (K with fine plane 2K on
   this rank) and needs r on its ghost planes for that (one halo of r); into a replicated coarse level the owned part is
   followed by an all-gather.  r_fine's ghost planes are overwritten. */
pmg_status pmg_mgmc_i_restrict(pmg_mgmc h, int l, double *r_fine, double *b_coarse, void *stream)
{
  mg_level      *Lv = &h->lv[l], *Cc = &h->lv[l - 1];
  pmgk_st27_dims CD   = level_dims(Cc);
  const int      fold = Lv->distributed && !Cc->distributed; /* distributed -> replicated */
  if (Lv->distributed) PMG_CALL(pmg_mgmc_i_halo_level(h, Lv, r_fine, stream));
  double *bc = fold ? fold_own_planes(h, l, &CD, b_coarse) : b_coarse;
  switch (Lv->transfer) {
  case MG_TR_NONE: break;
  case MG_TR_Q1_GRID: {
    pmgk_grid_layout GL;
    PMG_CALL(pmg_grid_get_kernel_layout(Lv->g, &GL));
    PMG_KERNEL(pmgk_q1_restrict(&GL, &CD, Lv->cpos_dev, r_fine, bc, stream));
    break;
  }
  case MG_TR_Q1_NAT: {
    const pmgk_st27_dims FD = level_dims(Lv);
    PMG_KERNEL(pmgk_st27_restrict(&FD, &CD, r_fine, bc, stream));
    break;
  }
  case MG_TR_CSR: {
    const int rowblock = Lv->kind == MG_LV_ROWBLOCK;
    if (rowblock) PMG_CALL(pmg_distmcsor_refresh_layout(Lv->dm, r_fine, stream)); /* the rows of P^T read r on other ranks' rows */
    /* inside a cycle on one device the restriction also sets the zero guess of a sliced-ELL coarse level: its rows are the rows of P^T, the
       padding of the layout is never written (zero since the allocation) -- one fill kernel less per level (PMG_MG_FUSED_ZERO=0) */
    double *zero = pmg_switch(PMG_SW_MG_FUSED_ZERO) && !h->dist && !rowblock && Cc->kind == MG_LV_SELL && b_coarse == Cc->b && Lv->R_nrows == Cc->n ? Cc->x : NULL;
    PMG_KERNEL(pmgk_csr_spmv_rows(Lv->R_nrows, Lv->R_rowpos, Lv->R_rowptr, Lv->R_col, Lv->R_val, r_fine, b_coarse, 0, zero, stream));
    if (zero) Cc->x_zeroed = 1;
    if (rowblock && l == h->rb_fold) PMG_CALL(pmg_mgmc_i_rb_fold_allgather(h, b_coarse, stream)); /* the replicated level below: every rank needs the whole right-hand side */
    break;
  }
  }
  if (fold) PMG_CALL(fold_allgather(h, l, b_coarse, stream));
  return PMG_SUCCESS;
}

/* z-slab grid level: b_coarse = P^T (b - A x) in one kernel.  The residual on the two ghost planes needs x two planes deep:
   every rank sends its second and second-to-last planes (both colours, one exchange) into the neighbours' y2 buffers; b is
   current on its ghost planes (pmg_mgmc_sample exchanges them once per call: in-place form only).  The coarse planes
   this rank owns, the fold into a replicated coarse level and the all-gather behind it are those of pmg_mgmc_i_restrict. */
static pmg_status mg_residual_restrict_slab(pmg_mgmc h, int l, void *stream)
{
  mg_level      *Lv = &h->lv[l], *Cc = &h->lv[l - 1];
  pmgk_st27_dims CD   = level_dims(Cc);
  const int      fold = !Cc->distributed;
  const double  *slo[2], *shi[2];
  double        *rlo[2], *rhi[2];
  int64_t        n[2];
  for (int c = 0; c < 2; ++c) {
    int64_t own, ghost;
    PMG_CALL(pmg_grid_halo_plane(Lv->g, c, 0, &own, &ghost, &n[c]));
    slo[c] = Lv->x + own + n[c]; /* plane 1 */
    rlo[c] = Lv->y2lo + (int64_t)c * n[c];
    PMG_CALL(pmg_grid_halo_plane(Lv->g, c, 1, &own, &ghost, &n[c]));
    shi[c] = Lv->x + own - n[c]; /* plane nz - 2 */
    rhi[c] = Lv->y2hi + (int64_t)c * n[c];
  }
  PMG_CALL(pmg_dist_exchange(h->dist, 2, slo, n, rlo, n, shi, n, rhi, n, stream));
  double *bc   = fold ? fold_own_planes(h, l, &CD, Cc->b) : Cc->b;
  int     done = 0;
  PMG_CALL(pmg_grid_residual_restrict(Lv->g, Lv->b, Lv->x, Lv->kz0 > 0 ? Lv->y2lo : NULL, Lv->kz0 + Lv->nzl < Lv->nz ? Lv->y2hi : NULL, &CD, bc, &done, stream));
  PMG_CHECK(done, PMG_ERR_PLIB, "level %d: the fused residual + restriction refused a slab the set-up had accepted", l);
  if (mg_level_cycle_lrc(h, l)) PMG_CALL(pmg_lrc_residual_sub_restricted(mg_level_cycle_lrc(h, l), mg_level_cycle_lrc(h, l - 1), Lv->x, Cc->b, stream)); /* - P^T B S B^T x = - B_{l-1} (S B^T x); B^T x summed over the ranks */
  if (fold) PMG_CALL(fold_allgather(h, l, Cc->b, stream));
  return PMG_SUCCESS;
}

/* x_fine += P_l e_coarse (MatInterpolateAdd).  only_color (grid level): -1 = both colours, else just that one. */
pmg_status pmg_mgmc_i_prolong_add(pmg_mgmc h, int l, const double *e_coarse, double *x_fine, int only_color, void *stream)
{
  mg_level *Lv = &h->lv[l], *Cc = &h->lv[l - 1];
  /* a z-slab also interpolates onto its in-domain ghost planes (from its coarse planes + coarse ghost planes): the
     same arithmetic the owner does, so the fine ghost planes stay current without an exchange */
  const int glo = Lv->distributed && Lv->kz0 > 0, ghi = Lv->distributed && Lv->kz0 + Lv->nzl < Lv->nz;
  const pmgk_st27_dims FD = level_dims(Lv), CD = level_dims(Cc);
  switch (Lv->transfer) {
  case MG_TR_NONE: break;
  case MG_TR_Q1_GRID: {
    pmgk_grid_layout GL;
    PMG_CALL(pmg_grid_get_kernel_layout(Lv->g, &GL));
    PMG_KERNEL(pmgk_q1_prolong_add(&GL, &CD, Lv->cpos_dev, -glo, Lv->nzl + glo + ghi, only_color, e_coarse, x_fine, stream));
    break;
  }
  case MG_TR_Q1_NAT: PMG_KERNEL(pmgk_st27_prolong_add(&FD, &CD, Lv->kz0 - glo, Lv->nzl + glo + ghi, e_coarse, x_fine, stream)); break;
  case MG_TR_CSR: PMG_KERNEL(pmgk_csr_spmv_rows(Lv->P_nrows, Lv->P_rowpos, Lv->P_rowptr, Lv->P_col, Lv->P_val, e_coarse, x_fine, 1, NULL, stream)); break;
  }
  return PMG_SUCCESS;
}

/* The noise terms B (sqrt(S) o eta) of a cycle need one draw of k numbers per directional sweep and level
   (src/pc_mcgibbs.c:130-134) -- a launch of one wavefront in front of every sweep, ~2 us each on the cycle's critical path
   (timing probe without them: 0.732 -> 0.715 ms per 257^3 k = 3 sample).  Which (seed, counter) every sweep of the cycle
   will ask for is known when the cycle starts: they are all drawn by ONE launch here and handed to the levels' updates,
   which take them when the sweep asks with a matching (seed, counter) and draw themselves otherwise.  Same numbers either
   way.  Single device only; PMG_LRC_BATCH=0 switches it off. */
#define MG_ETA_STRIDE 64
static pmg_status mg_draw_lowrank_noise(pmg_mgmc h, uint64_t seed, const uint64_t *ctr, int on, void *stream)
{
  if (!h->eta_batch_mode) h->eta_batch_mode = pmg_switch(PMG_SW_LRC_BATCH) ? 1 : -1;
  const int env = h->eta_batch_mode > 0;
  const int top = h->nlevels - 1;
  uint64_t  seeds[PMGK_NORMAL_BATCH_MAX], ctrs[PMGK_NORMAL_BATCH_MAX];
  int       first[64], count[64], nslots = 0;
  pmg_lrc   any = NULL;
  for (int l = 0; l <= top; ++l) {
    pmg_lrc lr = mg_level_path_lrc(h, l);
    first[l] = count[l] = 0;
    if (!lr) continue;
    pmg_lrc_preset_eta(lr, 0, 0, 0, NULL, 0); /* forget the last cycle's */
    if (!on || !env || h->dist || !pmg_lrc_is_local(lr) || pmg_lrc_rank(lr) > MG_ETA_STRIDE) continue;
    const int n = pmg_mgmc_i_level_sweeps(h, l);
    if (n <= 0 || nslots + n > PMGK_NORMAL_BATCH_MAX) continue;
    first[l] = nslots;
    count[l] = n;
    for (int i = 0; i < n; ++i) {
      seeds[nslots + i] = pmg_lrc_noise_seed(level_seed(seed, l));
      ctrs[nslots + i]  = ctr[l] + (uint64_t)i;
    }
    nslots += n;
    any = lr;
  }
  if (!nslots) return PMG_SUCCESS;
  if (!h->eta_batch) PMG_CALL(pmg_dev_alloc((void **)&h->eta_batch, sizeof(double) * MG_ETA_STRIDE * PMGK_NORMAL_BATCH_MAX));
  PMG_KERNEL(pmgk_fill_normal_batch(nslots, pmg_lrc_rank(any), seeds, ctrs, pmg_lrc_sqrtS(any), h->eta_batch, MG_ETA_STRIDE, stream)); /* S is the same on every level (src/pc_gamgmc.c:170-176) */
  for (int l = 0; l <= top; ++l)
    if (count[l]) pmg_lrc_preset_eta(mg_level_path_lrc(h, l), level_seed(seed, l), ctr[l], count[l], h->eta_batch + (size_t)first[l] * MG_ETA_STRIDE, MG_ETA_STRIDE);
  return PMG_SUCCESS;
}

/* The kernels one V-cycle runs on level l, decided HERE and nowhere else: mg_vcycle launches what this says,
   pmg_mgmc_get_algorithmic_bytes charges it.  A pure function, not a table of the set-up: the correction form and, on
   one device, the fused transfers may be switched afterwards, and top_has_guess changes from cycle to cycle. */
enum { MG_GUESS_KEEP, MG_GUESS_FILL, MG_GUESS_UNSET };  /* the iterate a level starts from: its own | zero, stored by a fill kernel (or by the CSR restriction into it, x_zeroed) | zero, NOT stored: the first out-of-place sweep is told */
enum { MG_RR_TWO, MG_RR_FUSED, MG_RR_FUSED_SLAB };      /* residual, then restriction | b_{l-1} = P^T (b - A x) in one pass on one device | the same on a z-slab */
typedef struct {
  pmg_lrc lrc;                   /* mg_level_path_lrc: the low-rank update the level's sampler applies with the cycle's help, NULL if none */
  double  rows;                  /* owned unknowns */
  int     zero_guess;            /* MG_GUESS_* (level 0: in front of the Gibbs sweeps; the exact sampler takes no guess) */
  int     rr;                    /* MG_RR_*, l >= 1 */
  int     rr_lowrank_restricted; /* the residual's low-rank term is subtracted in restricted form behind the fused kernel: - P^T B S B^T x = - B_{l-1} (S B^T x) */
  int     residual_pair;         /* class-stencil level: the paired residual kernel */
  int     prolong_colour;        /* -1: interpolate onto both colours, else onto this one only */
} mg_path;

static mg_path level_path(const struct pmg_mgmc_s *h, int l, int top_has_guess)
{
  const mg_level *Lv = &h->lv[l];
  mg_path         p  = {mg_level_path_lrc(h, l), level_rows(Lv), MG_GUESS_FILL, MG_RR_TWO, 0, 0, -1};
  if (l == 0 ? h->coarse_type == 0 : (l == h->nlevels - 1 && top_has_guess)) p.zero_guess = MG_GUESS_KEEP;
  else if (l >= 1 && pmg_mgmc_i_st27_out_of_place(Lv) && h->nu >= 1) p.zero_guess = MG_GUESS_UNSET; /* (also under a low-rank update: the noise term changes b, the repair acts on the swept iterate) */
  p.residual_pair = st27_use_pair(Lv) || (st27_use_pair_slab(Lv) && pmg_switch(PMG_SW_ST27_PAIR_SLAB) != 3);
  if (l == 0) return p;
  const mg_level *Cc = &h->lv[l - 1];
  if (Lv->transfer == MG_TR_Q1_GRID && !Lv->cpos_dev && !h->no_fused) {
    /* z-slab: agreed by the ranks at set-up, and b's ghost planes are current in the in-place form only (pmg_mgmc_sample).
       One device: a local update on both levels and the kernel's own gate, which the launcher asks first as well */
    const pmgk_st27_dims CD = level_dims(Cc);
    if (Lv->distributed) p.rr = Lv->rr_slab && !h->correction_form ? MG_RR_FUSED_SLAB : MG_RR_TWO;
    else if ((!p.lrc || (pmg_lrc_is_local(p.lrc) && Cc->kind == MG_LV_ST27 && pmg_lrc_is_local(mg_level_cycle_lrc(h, l - 1)))) && pmg_grid_residual_restrict_applies(Lv->g, &CD, 0, 0)) p.rr = MG_RR_FUSED;
  }
  p.rr_lowrank_restricted = p.rr != MG_RR_TWO && p.lrc;
  /* with omega = 1 a colour sweep never reads the old values of the colour it updates (the (1-omega) x term is
     gone), so the colour the post-smoother visits first needs no correction: it is overwritten unread */
  if (Lv->transfer == MG_TR_Q1_GRID && h->omega == 1.0 && h->nu >= 1 && !pmg_switch(PMG_SW_MG_PROLONG_BOTH)) p.prolong_colour = h->sweep_type == PMG_SOR_BACKWARD_SWEEP ? 0 : 1;
  return p;
}

/* the residual kernel the cycle runs on level l, on the caller's vectors (level diagnostics) */
pmg_status pmg_mgmc_i_level_residual(pmg_mgmc h, int l, const double *b, const double *x, double *r, void *stream)
{
  return mg_residual(&h->lv[l], level_path(h, l, 0).residual_pair, b, x, r, stream);
}

static pmg_status mg_zero_guess(mg_level *Lv, int how, void *stream)
{
  if (how == MG_GUESS_UNSET) Lv->x_unset = 1;
  else if (how == MG_GUESS_FILL && !Lv->x_zeroed) PMG_KERNEL(pmgk_fill_zero(Lv->x, Lv->ld, stream));
  Lv->x_zeroed = 0;
  return PMG_SUCCESS;
}

/* one multiplicative V-cycle on lv[top].b -> lv[top].x; x starts at zero on every level below the top, and on the
   top level too unless top_has_guess */
static pmg_status mg_vcycle(pmg_mgmc h, uint64_t seed, uint64_t sample, int top_has_guess, void *stream)
{
  const int top = h->nlevels - 1;
  uint64_t  ctr[64];
  mg_path   path[64];
  PMG_CHECK(h->nlevels <= 64, PMG_ERR_ARG_OUTOFRANGE, "too many levels");
  for (int l = 0; l <= top; ++l) {
    ctr[l]  = sample * MG_DRAWS_PER_SAMPLE;
    path[l] = level_path(h, l, top_has_guess);
    h->lv[l].x_zeroed = 0; /* (a cycle that ended in an error may have left one set) */
  }
  if (h->lrc_k > 0) PMG_CALL(mg_draw_lowrank_noise(h, seed, ctr, 1, stream));
  for (int l = top; l >= 1; --l) {
    mg_level      *Lv = &h->lv[l], *Cc = &h->lv[l - 1];
    const mg_path *p  = &path[l];
    PMG_CALL(mg_zero_guess(Lv, p->zero_guess, stream));
    pmg_lrc_expect_residual(p->lrc, 1); /* the last repair of the pre-smoothing also starts the residual's low-rank term */
    const pmg_status sst = mg_smooth(h, l, h->nu, seed, &ctr[l], stream);
    pmg_lrc_expect_residual(p->lrc, sst == PMG_SUCCESS); /* (an error: forget) */
    PMG_CALL(sst);
    switch (p->rr) {
    case MG_RR_FUSED: {
      const pmgk_st27_dims CD = level_dims(Cc);
      int                  done = 0;
      PMG_CALL(pmg_grid_residual_restrict(Lv->g, Lv->b, Lv->x, NULL, NULL, &CD, Cc->b, &done, stream));
      PMG_CHECK(done, PMG_ERR_PLIB, "level %d: the fused residual + restriction refused a level its own gate had accepted", l);
      if (p->rr_lowrank_restricted) PMG_CALL(pmg_lrc_residual_sub_restricted(p->lrc, mg_level_cycle_lrc(h, l - 1), Lv->x, Cc->b, stream));
      break;
    }
    case MG_RR_FUSED_SLAB: PMG_CALL(mg_residual_restrict_slab(h, l, stream)); break;
    default:
      PMG_CALL(mg_residual(Lv, p->residual_pair, Lv->b, Lv->x, Lv->r, stream));
      if (mg_level_cycle_lrc(h, l)) PMG_CALL(pmg_lrc_residual_sub(mg_level_cycle_lrc(h, l), Lv->x, Lv->r, stream)); /* PCMGSetResidual(..., As[l]), src/pc_gamgmc.c:194 */
      PMG_CALL(pmg_mgmc_i_restrict(h, l, Lv->r, Cc->b, stream));
    }
  }
  PMG_CALL(mg_zero_guess(&h->lv[0], path[0].zero_guess, stream));
  PMG_CALL(mg_smooth(h, 0, h->coarse_its, seed, &ctr[0], stream));
  for (int l = 1; l <= top; ++l) {
    PMG_CALL(pmg_mgmc_i_prolong_add(h, l, h->lv[l - 1].x, h->lv[l].x, path[l].prolong_colour, stream));
    pmg_lrc_expect_residual(path[l].lrc, 0); /* no residual behind the post-smoothing */
    PMG_CALL(mg_smooth(h, l, h->nu, seed, &ctr[l], stream));
  }
  if (h->lrc_k > 0) PMG_CALL(mg_draw_lowrank_noise(h, seed, ctr, 0, stream)); /* nothing outside this cycle takes its noise terms */
  return PMG_SUCCESS;
}

/* ALGORITHMIC bytes of ONE sample as the cycle above is built (what bench.py's V-cycle lines divide by their time):
   every launch of mg_vcycle / pmg_mgmc_sample counted with the operands it must read and write once, per level --
   this rank's owned unknowns N_l; halos, memsets of skipped zero fills and cache re-reads are NOT counted.
     grid sweep (matrix-free 7-point)     24 N per directional sweep (32 N at omega != 1): read y, b, write y
     class-stencil sweep (27 x 27 table)  24 N; 16 N for the zero-guess pre-sweep of the out-of-place kernel (x not read)
     sliced-ELL sweep                     12 nnz + 40 N
     block sweep (set_level_blocks)       pmg_blockgibbs_get_algorithmic_bytes: factors as stored + 12 nnz_ext + 28 per slot
     zero fill of a level iterate         8 N (skipped where the zero-guess sweep applies)
     grid residual + restriction fused    16 N + 8 N_c;  unfused: residual 24 N, restriction 8 N + 8 N_c
     class-stencil residual, restriction  24 N, 8 N + 8 N_c;  sliced-ELL: 12 nnz + 28 N, 12 nnz_P + 12 N_c + 8 N
     prolongation                         grid, omega = 1: ONE colour, 8 N + 8 N_c; otherwise 16 N + 8 N_c;
                                          CSR: 12 nnz_P + 20 N + 8 N_c
     exact coarse sample                  8 N_0^2 (two triangles) ; Gibbs coarse: its sweeps
     literal correction form              + outer residual 24 N and update 24 N on the finest level, + its zero fill
     low-rank update per directional sweep on ns support rows: noise term (8 k + 24) ns, repair (16 k + 24) ns;
                                          residual term (8 k + 8) ns + (8 k + 16) ns' (ns' = ns unrestricted, coarse rows restricted)
   per_level (may be NULL): nlevels entries, the smoothing / residual / transfer bytes charged to the level they run on
   (a transfer is charged to its FINE level). */
static pmg_status level_kernel_bytes(const struct pmg_mgmc_s *h, const mg_level *Lv, double N, double Nc, double *sweep /* one directional sweep */, double *rr_two /* residual, then restriction */)
{
  *sweep = *rr_two = 0.0;
  switch (Lv->kind) {
  case MG_LV_EXACT: break; /* no sweeps: 8 N^2 */
  case MG_LV_GRID:
  case MG_LV_GRID_SLAB:
  case MG_LV_ST27:
    *sweep  = (Lv->kind == MG_LV_ST27 || h->omega == 1.0 ? 24.0 : 32.0) * N;
    *rr_two = 24.0 * N + 8.0 * N + 8.0 * Nc;
    break;
  case MG_LV_SELL:
  case MG_LV_ROWBLOCK:
    *sweep  = 12.0 * (double)Lv->A_nnz + 40.0 * N;
    *rr_two = 12.0 * (double)Lv->A_nnz + 28.0 * N + 12.0 * (double)Lv->P_nnz + 12.0 * Nc + 8.0 * N;
    if (Lv->bg) return pmg_blockgibbs_get_algorithmic_bytes(Lv->bg, sweep);
    break;
  }
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_get_algorithmic_bytes(pmg_mgmc h, double *total, double *per_level)
{
  PMG_CHECK(h && total, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(h->is_setup, PMG_ERR_ARG_WRONGSTATE, "call pmg_mgmc_setup first");
  const int    top  = h->nlevels - 1;
  *total            = 0.0;
  for (int l = 0; l <= top; ++l) {
    const mg_level *Lv = &h->lv[l];
    const mg_path   p  = level_path(h, l, !h->correction_form);
    const double    N  = p.rows;
    int32_t         k = 0, kc = 0;
    int64_t         ns = 0, nc = 0; /* support rows of the level's update, of the next coarser level's */
    int             lr_dense = 0, cdense = 0;
    /* a rank whose slab or block misses B's support launches none of the low-rank kernels: ns = 0, no bytes */
    if (p.lrc) pmg_lrc_get_sizes(p.lrc, &k, &ns, &lr_dense);
    if (lr_dense) ns = (int64_t)N; /* dense factors: every row of the level */
    const double Nc = l >= 1 ? level_rows(&h->lv[l - 1]) : 0.0;
    double       sweep, rr_two;
    PMG_CALL(level_kernel_bytes(h, Lv, N, Nc, &sweep, &rr_two));
    const double lrsw  = p.lrc ? ((8.0 * k + 24.0) + (16.0 * k + 24.0)) * (double)ns : 0.0;
    const double lrres = p.lrc ? (8.0 * k + 8.0) * (double)ns + (8.0 * k + 16.0) * (double)ns : 0.0; /* unrestricted residual term */
    double       by    = p.zero_guess == MG_GUESS_FILL ? 8.0 * N : (p.zero_guess == MG_GUESS_UNSET ? -8.0 * N : 0.0); /* the zero fill / the first sweep does not read x */
    if (l == 0) {
      by += Lv->kind == MG_LV_EXACT ? 8.0 * N * N : pmg_mgmc_i_level_sweeps(h, l) * (sweep + lrsw);
    } else {
      const pmg_lrc clr = p.rr_lowrank_restricted ? mg_level_cycle_lrc(h, l - 1) : NULL; /* the coarse update the restricted residual term runs over */
      by += pmg_mgmc_i_level_sweeps(h, l) * (sweep + lrsw);
      by += p.rr != MG_RR_TWO ? 16.0 * N + 8.0 * Nc : rr_two;
      if (clr) pmg_lrc_get_sizes(clr, &kc, &nc, &cdense);
      if (clr && !cdense) by += (8.0 * k + 8.0) * (double)ns + (8.0 * k + 16.0) * (double)nc;
      else by += lrres;
      switch (Lv->transfer) {
      case MG_TR_NONE: break;
      case MG_TR_Q1_GRID:
      case MG_TR_Q1_NAT: by += (p.prolong_colour >= 0 ? 8.0 : 16.0) * N + 8.0 * Nc; break;
      case MG_TR_CSR: by += 12.0 * (double)Lv->P_nnz + 20.0 * N + 8.0 * Nc; break;
      }
      if (l == top && h->correction_form) by += 48.0 * N + lrres;
    }
    if (per_level) per_level[l] = by;
    *total += by;
  }
  return PMG_SUCCESS;
}

/* the caller's vector of the finest level into (to = 1) or out of the level's layout */
static pmg_status lvl_permute(mg_level *Lv, int to, const double *in, double *out, void *stream)
{
  switch (Lv->kind) {
  case MG_LV_GRID:
  case MG_LV_GRID_SLAB: return to ? pmg_grid_to_cvec(Lv->g, in, out, stream) : pmg_grid_from_cvec(Lv->g, in, out, stream);
  case MG_LV_SELL:
  case MG_LV_ROWBLOCK: return to ? pmg_mcsor_to_layout(Lv->mc, in, out, stream) : pmg_mcsor_from_layout(Lv->mc, in, out, stream);
  case MG_LV_ST27:
  case MG_LV_EXACT: break;
  }
  PMG_FAIL(PMG_ERR_PLIB, "the finest level is a grid or a sliced-ELL level");
}

pmg_status pmg_mgmc_sample(pmg_mgmc h, const double *b_nat, double *y_nat, int32_t its, int guesszero, uint64_t seed, uint64_t counter0, uint64_t *counter_out, pmg_sample_callback cb, void *cbctx, void *stream)
{
  PMG_CHECK(h && b_nat && y_nat, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(h->is_setup, PMG_ERR_ARG_WRONGSTATE, "call pmg_mgmc_setup first");
  PMG_CHECK(its >= 0, PMG_ERR_ARG_OUTOFRANGE, "its = %d", its);
  mg_level    *F     = &h->lv[h->nlevels - 1];
  const size_t bytes = sizeof(double) * (size_t)F->ld;
  PMG_CALL(lvl_permute(F, 1, b_nat, h->b_lay, stream));
  PMG_CALL(lvl_permute(F, 1, y_nat, h->y_lay, stream));
  if (h->correction_form && F->distributed) PMG_CALL(pmg_mgmc_i_halo_level(h, F, h->y_lay, stream)); /* the outer residual reads the ghost planes of y */
  if (level_path(h, h->nlevels - 1, 1).rr == MG_RR_FUSED_SLAB) PMG_CALL(pmg_mgmc_i_halo_level(h, F, h->b_lay, stream)); /* the fused residual + restriction reads b on the ghost planes */
  if (h->correction_form && F->kind == MG_LV_ROWBLOCK) PMG_CALL(pmg_distmcsor_refresh_layout(F->dm, h->y_lay, stream)); /* ... the ghost rows of a row block */
  for (int32_t it = 0; it < its; ++it) {
    if (!h->correction_form) {
      /* The cycle run IN PLACE on (b, y): a stationary linear sweep satisfies S(b, y) = y + S(b - A y, 0) with the
         same noise, so "w = b - A y; y += MG(w)" (src/pc_gamgmc.c:253-256) and the V-cycle started from the guess y
         are the same chain up to rounding -- without the outer residual, the axpy and a memset (about 15 % of a
         sample).  pmg_mgmc_set_correction_form(mg, 1) selects the literal form. */
      double *sb = F->b, *sx = F->x;
      F->b       = h->b_lay;
      F->x       = h->y_lay;
      pmg_status st = mg_vcycle(h, seed, counter0 + (uint64_t)it, !(it == 0 && guesszero), stream);
      F->b          = sb;
      F->x          = sx;
      PMG_CALL(st);
    } else if (it == 0 && guesszero) { /* y = MG(b), src/pc_gamgmc.c:243-246 */
      PMG_HIP(hipMemcpyAsync(F->b, h->b_lay, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
      PMG_CALL(mg_vcycle(h, seed, counter0 + (uint64_t)it, 0, stream));
      PMG_HIP(hipMemcpyAsync(h->y_lay, F->x, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    } else { /* w = b - A y; work = MG(w); y += work, src/pc_gamgmc.c:253-256 */
      PMG_CALL(mg_residual(F, 0, h->b_lay, h->y_lay, F->b, stream));
      if (mg_level_cycle_lrc(h, h->nlevels - 1)) PMG_CALL(pmg_lrc_residual_sub(mg_level_cycle_lrc(h, h->nlevels - 1), h->y_lay, F->b, stream)); /* z-slabs */
      PMG_CALL(mg_vcycle(h, seed, counter0 + (uint64_t)it, 0, stream));
      PMG_KERNEL(pmgk_axpy(F->ld, 1.0, F->x, h->y_lay, stream));
    }
    if (cb) { /* pg->scb(it, y, ctx), src/pc_gamgmc.c:258 */
      PMG_CALL(lvl_permute(F, 0, h->y_lay, y_nat, stream));
      const int rc = cb(it, y_nat, h->n_io, cbctx);
      if (rc != 0 && counter_out) *counter_out = counter0 + (uint64_t)it + 1; /* y holds sample it: a resumed chain draws the next noise */
      PMG_CHECK(rc == 0, rc, "sample callback returned %d", rc);
    }
  }
  PMG_CALL(lvl_permute(F, 0, h->y_lay, y_nat, stream));
  if (counter_out) *counter_out = counter0 + (uint64_t)its;
  return PMG_SUCCESS;
}
