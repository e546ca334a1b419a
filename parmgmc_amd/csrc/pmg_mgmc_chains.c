/* Many chains per call (pmg_mgmc_sample_chains): hierarchies of sliced-ELL levels on one device -- host side (C11).
   The V-cycle of mg_vcycle restricted to what such a hierarchy runs -- level sampler = pmg_mcsor sweeps, residual, CSR
   restriction / prolongation, exact or Gibbs coarse level -- on ld x C level vectors (chain fastest), each step one launch
   for all chains (kernels_chains.hip).  Column c performs the single-chain cycle's operations in the same order with the keys
   level_seed(seeds[c], l) and the same counters: pmg_mgmc_sample on that column with seed = seeds[c], bit for bit. */
#include "pmg_mgmc_internal.h"

void pmg_mgmc_i_free_chains(pmg_mgmc h)
{
  for (int l = 0; l < h->nlevels && h->ch_b; ++l) {
    pmg_dev_free(h->ch_b[l]);
    pmg_dev_free(h->ch_x[l]);
    pmg_dev_free(h->ch_r[l]);
  }
  free(h->ch_b);
  free(h->ch_x);
  free(h->ch_r);
  pmg_dev_free(h->ch_Y);
  pmg_dev_free(h->ch_bs);
  pmg_dev_free(h->ch_xi);
  pmg_dev_free(h->ch_v);
  pmg_dev_free(h->ch_B);
  pmg_keybuf_free(&h->ch_keys);
  h->ch_b = h->ch_x = h->ch_r = NULL;
  h->ch_Y = h->ch_bs = h->ch_xi = h->ch_v = h->ch_B = NULL;
  h->ch_cap = h->ch_B_cap = 0;
}

static pmg_status mgmc_chains_workspace(pmg_mgmc h, int32_t C, void *stream)
{
  if (C <= h->ch_cap) return PMG_SUCCESS;
  PMG_HIP(hipStreamSynchronize((hipStream_t)stream)); /* the old buffers may still be in use */
  pmg_keybuf keys = h->ch_keys; /* kept: its own growth rule */
  memset(&h->ch_keys, 0, sizeof h->ch_keys);
  pmg_mgmc_i_free_chains(h);
  h->ch_keys = keys;
  const int L = h->nlevels;
  h->ch_b = (double **)calloc((size_t)L, sizeof(double *));
  h->ch_x = (double **)calloc((size_t)L, sizeof(double *));
  h->ch_r = (double **)calloc((size_t)L, sizeof(double *));
  PMG_CHECK(h->ch_b && h->ch_x && h->ch_r, PMG_ERR_MEM, "out of host memory");
  for (int l = 0; l < L; ++l) {
    const size_t bytes = sizeof(double) * (size_t)h->lv[l].ld * (size_t)C;
    PMG_CALL(pmg_dev_alloc((void **)&h->ch_b[l], bytes));
    PMG_CALL(pmg_dev_alloc((void **)&h->ch_x[l], bytes));
    PMG_CALL(pmg_dev_alloc((void **)&h->ch_r[l], bytes));
  }
  const mg_level *F = &h->lv[L - 1];
  PMG_CALL(pmg_dev_alloc((void **)&h->ch_Y, sizeof(double) * (size_t)F->ld * (size_t)C));
  PMG_CALL(pmg_dev_alloc((void **)&h->ch_bs, sizeof(double) * (size_t)F->ld));
  if (h->coarse_type == 0) {
    PMG_CALL(pmg_dev_alloc((void **)&h->ch_xi, sizeof(double) * (size_t)h->lv[0].n * (size_t)C));
    PMG_CALL(pmg_dev_alloc((void **)&h->ch_v, sizeof(double) * (size_t)h->lv[0].n * (size_t)C));
  }
  h->ch_cap = C;
  return PMG_SUCCESS;
}

/* one V-cycle on C chains: top level right-hand side btop (chain stride bcs: 0 = the shared vector, 1 = per chain) and iterate
   xtop; every level below starts from zero, the top level too unless top_has_guess (mg_vcycle's rules) */
static pmg_status mg_vcycle_chains(pmg_mgmc h, int32_t C, const uint64_t *keys, const double *btop, int bcs_top, double *xtop, uint64_t sample, int top_has_guess, void *stream)
{
  const int top = h->nlevels - 1;
  uint64_t  ctr[64];
  int       zeroed[64];
  for (int l = 0; l <= top; ++l) {
    ctr[l]    = sample * MG_DRAWS_PER_SAMPLE;
    zeroed[l] = 0;
  }
  for (int l = top; l >= 1; --l) {
    mg_level     *Lv  = &h->lv[l];
    const double *b   = l == top ? btop : h->ch_b[l];
    const int     bcs = l == top ? bcs_top : 1;
    double       *x   = l == top ? xtop : h->ch_x[l];
    if ((l < top || !top_has_guess) && !zeroed[l]) PMG_KERNEL(pmgk_fill_zero(x, Lv->ld * C, stream));
    PMG_CALL(pmg_mcsor_sweeps_chains(Lv->mc, C, keys + (size_t)l * C, 1, h->scaled, h->nu, ctr[l], &ctr[l], b, bcs, x, stream));
    PMG_CALL(pmg_mcsor_residual_chains(Lv->mc, C, b, bcs, x, h->ch_r[l], stream));
    /* b_{l-1} = P^T r, which also sets the coarse level's zero guess where one is needed (as mg_restrict does) */
    const int needs_zero = l - 1 >= 1 || h->coarse_type != 0;
    PMG_KERNEL(pmgk_csr_spmv_rows_chains(Lv->R_nrows, Lv->R_rowpos, Lv->R_rowptr, Lv->R_col, Lv->R_val, C, h->ch_r[l], h->ch_b[l - 1], 0, needs_zero ? h->ch_x[l - 1] : NULL, stream));
    zeroed[l - 1] = needs_zero;
  }
  if (h->coarse_type == 0) PMG_CALL(pmg_chol_sample_chains(h->chol, C, keys, ctr[0], h->ch_b[0], h->ch_x[0], h->ch_xi, h->ch_v, stream));
  else {
    if (!zeroed[0]) PMG_KERNEL(pmgk_fill_zero(h->ch_x[0], h->lv[0].ld * C, stream));
    PMG_CALL(pmg_mcsor_sweeps_chains(h->lv[0].mc, C, keys, 1, h->scaled, h->coarse_its, ctr[0], &ctr[0], h->ch_b[0], 1, h->ch_x[0], stream));
  }
  for (int l = 1; l <= top; ++l) {
    mg_level     *Lv  = &h->lv[l];
    const double *b   = l == top ? btop : h->ch_b[l];
    const int     bcs = l == top ? bcs_top : 1;
    double       *x   = l == top ? xtop : h->ch_x[l];
    PMG_KERNEL(pmgk_csr_spmv_rows_chains(Lv->P_nrows, Lv->P_rowpos, Lv->P_rowptr, Lv->P_col, Lv->P_val, C, h->ch_x[l - 1], x, 1, NULL, stream)); /* x += P e */
    PMG_CALL(pmg_mcsor_sweeps_chains(Lv->mc, C, keys + (size_t)l * C, 1, h->scaled, h->nu, ctr[l], &ctr[l], b, bcs, x, stream));
  }
  return PMG_SUCCESS;
}

/* checks of pmg_mgmc_sample_chains / pmg_mgmc_get_algorithmic_bytes_chains; the argument and support checks come before the
   set-up check, and nothing here touches the device */
static pmg_status mgmc_chains_check(pmg_mgmc h, int32_t C)
{
  PMG_CHECK(h->user_hier, PMG_ERR_SUP, "multi-chain sampling of DMDA hierarchies (pmg_mgmc_create_dmda*) is not supported: one chain already fills the device there");
  PMG_CHECK(!h->rb_dist, PMG_ERR_SUP, "multi-chain sampling of row-block distributed hierarchies is not supported");
  PMG_CHECK(!h->lrc_k, PMG_ERR_SUP, "multi-chain sampling of a hierarchy with a low-rank (MATLRC) update is not supported");
  PMG_CHECK(h->is_setup, PMG_ERR_ARG_WRONGSTATE, "call pmg_mgmc_setup first");
  for (int l = 0; l < h->nlevels; ++l) {
    const mg_level *Lv = &h->lv[l];
    PMG_CHECK(!Lv->dm && !Lv->is_grid && !Lv->is_st27 && (Lv->mc || (l == 0 && h->coarse_type == 0)), PMG_ERR_SUP, "level %d is not a sliced-ELL level: not supported by the multi-chain cycle", l);
    if (Lv->mc) PMG_CALL(pmg_mcsor_chains_supported(Lv->mc));
    PMG_CALL(pmg_chains_size_check(Lv->ld, C));
  }
  return PMG_SUCCESS;
}

/* the chains loop: right-hand side b_nat shared (bcs = 0, n values) or one per chain (bcs = 1, n x C, chain fastest) */
static pmg_status mgmc_chains_run(pmg_mgmc h, int32_t C, const uint64_t *seeds, const double *b_nat, int bcs, double *Y_nat, int32_t its, int guesszero, uint64_t counter0, uint64_t *counter_out, pmg_chains_callback cb, void *cbctx, void *stream)
{
  PMG_CHECK(h, PMG_ERR_ARG_NULL, "null handle");
  PMG_CHECK(C >= 1, PMG_ERR_ARG_OUTOFRANGE, "nchains = %d", C);
  PMG_CHECK(seeds && b_nat && Y_nat, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(its >= 0, PMG_ERR_ARG_OUTOFRANGE, "its = %d", its);
  PMG_CALL(mgmc_chains_check(h, C));
  const int top = h->nlevels - 1;
  mg_level *F   = &h->lv[top];
  PMG_CALL(mgmc_chains_workspace(h, C, stream));
  if (bcs && C > h->ch_B_cap) { /* after the workspace: growing it frees this buffer too */
    PMG_HIP(hipStreamSynchronize((hipStream_t)stream));
    pmg_dev_free(h->ch_B);
    h->ch_B     = NULL;
    h->ch_B_cap = 0;
    PMG_CALL(pmg_dev_alloc((void **)&h->ch_B, sizeof(double) * (size_t)F->ld * (size_t)C));
    h->ch_B_cap = C;
  }
  uint64_t *kh = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)h->nlevels * (size_t)C);
  PMG_CHECK(kh, PMG_ERR_MEM, "out of host memory");
  for (int l = 0; l <= top; ++l)
    for (int32_t c = 0; c < C; ++c) kh[(size_t)l * C + c] = level_seed(seeds[c], l);
  const pmg_status kst = pmg_keybuf_set(&h->ch_keys, kh, (int64_t)h->nlevels * C, stream);
  free(kh);
  PMG_CALL(kst);
  const uint64_t *keys = h->ch_keys.dev;
  const int32_t  *orig = pmg_mcsor_orig_dev(F->mc);
  const int64_t   nel  = F->ld * C;
  const double   *btop = bcs ? h->ch_B : h->ch_bs;
  if (bcs) PMG_KERNEL(pmgk_permute_in_chains(F->ld, orig, C, b_nat, 1, h->ch_B, stream));
  else PMG_KERNEL(pmgk_permute_in(F->ld, orig, b_nat, h->ch_bs, stream));
  PMG_KERNEL(pmgk_permute_in_chains(F->ld, orig, C, Y_nat, 1, h->ch_Y, stream));
  for (int32_t it = 0; it < its; ++it) {
    const uint64_t sample = counter0 + (uint64_t)it;
    if (!h->correction_form || (it == 0 && guesszero)) /* in place on (b, Y), pmg_mgmc_sample's default; or Y = MG(b) (src/pc_gamgmc.c:243-246) */
      PMG_CALL(mg_vcycle_chains(h, C, keys, btop, bcs, h->ch_Y, sample, !h->correction_form && !(it == 0 && guesszero), stream));
    else { /* w = b - A y; work = MG(w); y += work, src/pc_gamgmc.c:253-256 */
      PMG_CALL(pmg_mcsor_residual_chains(F->mc, C, btop, bcs, h->ch_Y, h->ch_b[top], stream));
      PMG_CALL(mg_vcycle_chains(h, C, keys, h->ch_b[top], 1, h->ch_x[top], sample, 0, stream));
      PMG_KERNEL(pmgk_axpy(nel, 1.0, h->ch_x[top], h->ch_Y, stream));
    }
    if (cb) {
      PMG_KERNEL(pmgk_permute_out_chains(F->ld, orig, C, h->ch_Y, Y_nat, stream));
      const int rc = cb(it, Y_nat, F->n, C, cbctx);
      PMG_CHECK(rc == 0, rc, "sample callback returned %d", rc);
    }
  }
  PMG_KERNEL(pmgk_permute_out_chains(F->ld, orig, C, h->ch_Y, Y_nat, stream));
  if (counter_out) *counter_out = counter0 + (uint64_t)its;
  return PMG_SUCCESS;
}

pmg_status pmg_mgmc_sample_chains(pmg_mgmc h, int32_t C, const uint64_t *seeds, const double *b_nat, double *Y_nat, int32_t its, int guesszero, uint64_t counter0, uint64_t *counter_out, pmg_chains_callback cb, void *cbctx, void *stream)
{
  return mgmc_chains_run(h, C, seeds, b_nat, 0, Y_nat, its, guesszero, counter0, counter_out, cb, cbctx, stream);
}

/* pmg_mgmc_sample_chains with one right-hand side per chain (B_nat n x C, chain fastest): column c = pmg_mgmc_sample with b = B[:, c] */
pmg_status pmg_mgmc_sample_chains_rhs(pmg_mgmc h, int32_t C, const uint64_t *seeds, const double *B_nat, double *Y_nat, int32_t its, int guesszero, uint64_t counter0, uint64_t *counter_out, pmg_chains_callback cb, void *cbctx, void *stream)
{
  return mgmc_chains_run(h, C, seeds, B_nat, 1, Y_nat, its, guesszero, counter0, counter_out, cb, cbctx, stream);
}

/* ALGORITHMIC bytes of ONE V-cycle of pmg_mgmc_sample_chains advancing all C chains, each launch counted once with its operands
   (per level N rows, nnz stored entries of the operator, nnz_P of the interpolation, N_c rows of the next coarser level).
   Operands every chain shares -- matrix, idiag, sqrtdiag, diag, orig, the shared b, P, W -- count once; iterates, residuals and
   per-chain right-hand sides count C times:
     sliced-ELL sweep, shared b           12 nnz + 24 N + 16 N C    (idiag + sqrtdiag + b once; read and write Y per chain)
     sliced-ELL sweep, per-chain b        12 nnz + 16 N + 24 N C
     residual                             12 nnz + 12 N + 16 N C, + 8 N (shared b) or 8 N C (per-chain b)
     zero fill of a level iterate         8 N C
     restriction P^T r                    12 nnz_P + 8 N_c + 8 N C + 8 N_c C
     prolongation x += P e                12 nnz_P + 8 N + 16 N C + 8 N_c C
     exact coarse sample                  8 N_0^2 (two triangles of W) + 48 N_0 C (noise, L^-1 b + xi, the sample)
     Gibbs coarse                         zero fill + its sweeps with per-chain b
     literal correction form              + outer residual (shared b) and the update y += x (24 N C) on the finest level
   The top level of the in-place form keeps its guess (no zero fill) and sweeps with the shared b; below the top every
   right-hand side is per chain.  per_level (may be NULL): nlevels entries, transfers charged to their fine level. */
pmg_status pmg_mgmc_get_algorithmic_bytes_chains(pmg_mgmc h, int32_t C, double *total, double *per_level)
{
  PMG_CHECK(h && total, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(C >= 1, PMG_ERR_ARG_OUTOFRANGE, "nchains = %d", C);
  PMG_CALL(mgmc_chains_check(h, C));
  const int    top  = h->nlevels - 1;
  const int    ndir = h->sweep_type == PMG_SOR_SYMMETRIC_SWEEP ? 2 : 1;
  const double nsw  = (double)h->nu * ndir, Cd = (double)C;
  *total            = 0.0;
  for (int l = 0; l <= top; ++l) {
    const mg_level *Lv  = &h->lv[l];
    const double    N   = (double)Lv->n, nnz = (double)Lv->A_nnz;
    const double    swp = 12.0 * nnz + 16.0 * N + 24.0 * N * Cd; /* per-chain b */
    double          by  = 0.0;
    if (l == 0) by = h->coarse_type == 0 ? 8.0 * N * N + 48.0 * N * Cd : 8.0 * N * Cd + h->coarse_its * ndir * swp;
    else {
      const double Nc     = (double)h->lv[l - 1].n, nnzP = (double)Lv->P_nnz;
      const int    shared = l == top && !h->correction_form;
      by += 2.0 * nsw * (shared ? 12.0 * nnz + 24.0 * N + 16.0 * N * Cd : swp);
      if (!shared) by += 8.0 * N * Cd;                                                   /* zero fill */
      by += 12.0 * nnz + 12.0 * N + 16.0 * N * Cd + (shared ? 8.0 * N : 8.0 * N * Cd); /* residual */
      by += 12.0 * nnzP + 8.0 * Nc + 8.0 * N * Cd + 8.0 * Nc * Cd;                     /* restriction */
      by += 12.0 * nnzP + 8.0 * N + 16.0 * N * Cd + 8.0 * Nc * Cd;                     /* prolongation */
      if (l == top && h->correction_form) by += (12.0 * nnz + 12.0 * N + 16.0 * N * Cd + 8.0 * N) + 24.0 * N * Cd;
    }
    if (per_level) per_level[l] = by;
    *total += by;
  }
  return PMG_SUCCESS;
}
