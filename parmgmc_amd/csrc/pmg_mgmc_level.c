/* Single-kernel entry points of one level of the MGMC sampler -- host side (C11).  Diagnostics: the full-size parity
   tests run ONE kernel of the V-cycle on caller-supplied vectors in the level's own layout and compare sampled rows with
   the oracle. */
#include "pmg_mgmc_internal.h"

pmg_status pmg_mgmc_i_level_checked(pmg_mgmc h, int32_t level, int need_coarser, mg_level **Lv)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(h->is_setup, PMG_ERR_ARG_WRONGSTATE, "call pmg_mgmc_setup first");
  PMG_CHECK(!h->dist, PMG_ERR_SUP, "level diagnostics are a single-device feature");
  PMG_CHECK(level >= (need_coarser ? 1 : 0) && level < h->nlevels, PMG_ERR_ARG_OUTOFRANGE, "level %d", level);
  *Lv = &h->lv[level];
  return PMG_SUCCESS;
}

/* ONE directional sweep of the level sampler (all colours) with the raw (seed, counter) pair */
pmg_status pmg_mgmc_level_sweep(pmg_mgmc h, int32_t level, int backward, int noisy, uint64_t seed, uint64_t counter, const double *b_lvl, double *x_lvl, void *stream)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 0, &Lv));
  PMG_CHECK(b_lvl && x_lvl, PMG_ERR_ARG_NULL, "null vector");
  if (Lv->bg) return pmg_blockgibbs_dir_sweep(Lv->bg, backward ? PMG_SOR_BACKWARD_SWEEP : PMG_SOR_FORWARD_SWEEP, noisy != 0, seed, counter, NULL, b_lvl, x_lvl, stream); /* the block sweep the cycle runs */
  PMG_CHECK(Lv->kind == MG_LV_ST27, PMG_ERR_SUP, "level %d: only class-stencil levels (use pmg_grid_* / pmg_mcsor_* for the others)", level);
  pmgk_st27 S = Lv->st;
  S.sqrtdiag  = h->scaled ? Lv->st_sqrtd_scaled : Lv->st_sqrtd;
  if (pmg_mgmc_i_st27_out_of_place(Lv)) { /* the production kernel: out of place into the level's second buffer, then copied back */
    PMG_KERNEL(pmgk_st27_sweep_pp(&S, backward != 0, h->omega, noisy != 0, seed, counter, b_lvl, x_lvl, Lv->x2, stream));
    PMG_HIP(hipMemcpyAsync(x_lvl, Lv->x2, sizeof(double) * (size_t)Lv->ld, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PMG_SUCCESS;
  }
  PMG_KERNEL(pmgk_st27_sweep(&S, backward != 0, h->omega, noisy != 0, seed, counter, b_lvl, x_lvl, stream));
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_level_residual(pmg_mgmc h, int32_t level, const double *b_lvl, const double *x_lvl, double *r_lvl, void *stream)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 0, &Lv));
  PMG_CHECK(b_lvl && x_lvl && r_lvl, PMG_ERR_ARG_NULL, "null vector");
  switch (Lv->kind) {
  case MG_LV_GRID:
  case MG_LV_GRID_SLAB:
  case MG_LV_ST27: return pmg_mgmc_i_level_residual(h, level, b_lvl, x_lvl, r_lvl, stream);
  case MG_LV_SELL:
  case MG_LV_ROWBLOCK: return pmg_mcsor_residual_layout(Lv->mc, b_lvl, x_lvl, r_lvl, stream); /* (of a row block: the local rows, no exchange) */
  case MG_LV_EXACT: break;
  }
  PMG_FAIL(PMG_ERR_SUP, "level %d has no residual kernel", level);
}

/* b_coarse (level-1) = P^T r_fine (level); x_fine (level) += P e_coarse (level-1), both colours */
pmg_status pmg_mgmc_level_restrict(pmg_mgmc h, int32_t level, double *r_fine, double *b_coarse, void *stream)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 1, &Lv));
  PMG_CHECK(r_fine && b_coarse, PMG_ERR_ARG_NULL, "null vector");
  return pmg_mgmc_i_restrict(h, level, r_fine, b_coarse, stream);
}

/* the V-cycle's fused step b_coarse = P^T (b - A x) on a grid level; PMG_ERR_SUP where the cycle runs the two steps */
pmg_status pmg_mgmc_level_residual_restrict(pmg_mgmc h, int32_t level, const double *b_lvl, const double *x_lvl, double *b_coarse, void *stream)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 1, &Lv));
  PMG_CHECK(b_lvl && x_lvl && b_coarse, PMG_ERR_ARG_NULL, "null vector");
  int done = 0;
  if (Lv->kind == MG_LV_GRID && Lv->transfer == MG_TR_Q1_GRID && !Lv->cpos_dev && !mg_level_sampler_lrc(h, level)) { /* (level_checked: no z-slabs here) */
    const pmgk_st27_dims CD = level_dims(&h->lv[level - 1]);
    PMG_CALL(pmg_grid_residual_restrict(Lv->g, b_lvl, x_lvl, NULL, NULL, &CD, b_coarse, &done, stream));
  }
  PMG_CHECK(done, PMG_ERR_SUP, "level %d: no fused residual + restriction (z-slab, low-rank update, permuted or semicoarsened coarse level)", level);
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_level_prolong_add(pmg_mgmc h, int32_t level, const double *e_coarse, double *x_fine, void *stream)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 1, &Lv));
  PMG_CHECK(e_coarse && x_fine, PMG_ERR_ARG_NULL, "null vector");
  return pmg_mgmc_i_prolong_add(h, level, e_coarse, x_fine, -1, stream);
}

/* the MATLRC update of a level (src/pc_gamgmc.c:157-196), single device: held by the grid object on the grid level, by the
   level on class-stencil levels; a sliced-ELL level's sampler keeps its own to itself (PMG_ERR_ARG_WRONGSTATE here) */
static pmg_status level_lrc(pmg_mgmc h, int32_t level, int need_coarser, mg_level **Lv, pmg_lrc *l)
{
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, need_coarser, Lv));
  *l = mg_level_path_lrc(h, level);
  PMG_CHECK(*l, PMG_ERR_ARG_WRONGSTATE, "level %d carries no low-rank update", level);
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_level_lowrank_factors(pmg_mgmc h, int32_t level, int32_t *k, int64_t *ns, int64_t *rows_host, double *B_host, double *Bb_fwd_host, double *Bb_bwd_host)
{
  mg_level *Lv;
  pmg_lrc   l;
  PMG_CALL(level_lrc(h, level, 0, &Lv, &l));
  return pmg_lrc_get_compact(l, k, ns, rows_host, B_host, Bb_fwd_host, Bb_bwd_host);
}

/* what the low-rank passes of a level run over, on every kind of level: the rank, the number of rows (the support rows of the row-compact form, every row of the dense form: *dense = 1) */
pmg_status pmg_mgmc_level_lowrank_sizes(pmg_mgmc h, int32_t level, int32_t *k, int64_t *rows, int *dense)
{
  mg_level *Lv;
  PMG_CALL(pmg_mgmc_i_level_checked(h, level, 0, &Lv));
  pmg_lrc l = mg_level_sampler_lrc(h, level);
  PMG_CHECK(l, PMG_ERR_ARG_WRONGSTATE, "level %d carries no low-rank update", level);
  pmg_lrc_get_sizes(l, k, rows, dense);
  if (dense && *dense && rows) *rows = (int64_t)level_rows(Lv);
  return PMG_SUCCESS;
}

/* y -= Bb (B^T y) with the level's factors, MCSORPostSOR_LRC (src/mc_sor.c:101-112) */
pmg_status pmg_mgmc_level_lowrank_post(pmg_mgmc h, int32_t level, int backward, double *y_lvl, void *stream)
{
  mg_level *Lv;
  pmg_lrc   l;
  PMG_CALL(level_lrc(h, level, 0, &Lv, &l));
  PMG_CHECK(y_lvl, PMG_ERR_ARG_NULL, "null vector");
  return pmg_lrc_post(l, backward ? PMG_SOR_BACKWARD_SWEEP : PMG_SOR_FORWARD_SWEEP, y_lvl, stream);
}

/* the low-rank part of the level residual (PCMGSetResidual on the MATLRC operator, src/pc_gamgmc.c:194):
   restricted = 0: out (this level's layout) -= B_l (S B_l^T x);  restricted = 1: out (the next coarser level's layout)
   -= B_{l-1} (S B_l^T x), the form the cycle uses behind the fused residual + restriction */
pmg_status pmg_mgmc_level_lowrank_residual_sub(pmg_mgmc h, int32_t level, int restricted, const double *x_lvl, double *out, void *stream)
{
  mg_level *Lv, *Cc;
  pmg_lrc   l, lc;
  PMG_CALL(level_lrc(h, level, restricted, &Lv, &l));
  PMG_CHECK(x_lvl && out, PMG_ERR_ARG_NULL, "null vector");
  if (!restricted) return pmg_lrc_residual_sub(l, x_lvl, out, stream);
  PMG_CALL(level_lrc(h, level - 1, 0, &Cc, &lc));
  return pmg_lrc_residual_sub_restricted(l, lc, x_lvl, out, stream);
}

