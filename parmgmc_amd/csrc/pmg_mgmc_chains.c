/* Many chains per call (pmg_mgmc_sample_chains): hierarchies of sliced-ELL levels on one device -- host side (C11).
   The V-cycle of mg_vcycle restricted to what such a hierarchy runs -- level sampler = pmg_mcsor sweeps, residual, CSR
   restriction / prolongation, exact or Gibbs coarse level -- on ld x C level vectors (chain fastest), each step one launch
   for all chains (kernels_chains.hip).  Column c performs the single-chain cycle's operations in the same order with the keys
   level_seed(seeds[c], l) and the same counters: pmg_mgmc_sample on that column with seed = seeds[c], bit for bit.
   A hierarchy with a low-rank update (pmg_mgmc_set_lowrank: MATLRC levels, src/pc_gamgmc.c:157-196) runs, per directional sweep of a
   level that has one, the noise term + B_l (sqrt(S) o eta_c) on the right-hand side, the colour sweeps, the repair y -= Bb (B^T y);
   its residual gets - B_l (S o (B_l^T x)) before the restriction (pmg_mcsor_residual_layout's unrestricted form).  The noise terms
   of a cycle are drawn by one launch; every such right-hand side is the cycle's own and takes the term in place (pmg_lrc.c). */
#include "pmg_mgmc_internal.h"

void pmg_mgmc_i_free_chains(pmg_mgmc h)
{
  for (int l = 0; l < 3 * h->nlevels && h->ch_b; ++l) pmg_devbuf_free(&h->ch_b[l]); /* ch_b, ch_x, ch_r: one array (mgmc_chains_workspace) */
  free(h->ch_b);
  h->ch_b = h->ch_x = h->ch_r = NULL;
  pmg_devbuf_free(&h->ch_Y);
  pmg_devbuf_free(&h->ch_bs);
  pmg_devbuf_free(&h->ch_xi);
  pmg_devbuf_free(&h->ch_v);
  pmg_devbuf_free(&h->ch_B);
  pmg_devbuf_free(&h->ch_eta);
  pmg_keybuf_free(&h->ch_keys);
}

static pmg_status mgmc_chains_workspace(pmg_mgmc h, int32_t C, void *stream)
{
  if (!h->ch_b) { /* first chains call: the three level arrays, empty, in one host allocation */
    h->ch_b = (pmg_devbuf *)calloc(3 * (size_t)h->nlevels, sizeof(pmg_devbuf));
    PMG_CHECK(h->ch_b, PMG_ERR_MEM, "out of host memory");
    h->ch_x = h->ch_b + h->nlevels;
    h->ch_r = h->ch_x + h->nlevels;
  }
  for (int l = 0; l < h->nlevels; ++l) {
    const size_t bytes = sizeof(double) * (size_t)h->lv[l].ld * (size_t)C;
    PMG_CALL(pmg_devbuf_reserve(&h->ch_b[l], bytes, stream));
    PMG_CALL(pmg_devbuf_reserve(&h->ch_x[l], bytes, stream));
    PMG_CALL(pmg_devbuf_reserve(&h->ch_r[l], bytes, stream));
  }
  const size_t top = sizeof(double) * (size_t)h->lv[h->nlevels - 1].ld;
  PMG_CALL(pmg_devbuf_reserve(&h->ch_Y, top * (size_t)C, stream));
  PMG_CALL(pmg_devbuf_reserve(&h->ch_bs, top, stream));
  if (h->coarse_type == 0) {
    PMG_CALL(pmg_devbuf_reserve(&h->ch_xi, sizeof(double) * (size_t)h->lv[0].n * (size_t)C, stream));
    PMG_CALL(pmg_devbuf_reserve(&h->ch_v, sizeof(double) * (size_t)h->lv[0].n * (size_t)C, stream));
  }
  return PMG_SUCCESS;
}

/* every noise term sqrt(S) o eta of one cycle in ONE launch (mg_draw_lowrank_noise on chains): slot first[l] + d holds the k x C
   numbers of level l's directional sweep with counter ctr[l] + d, from the keys pmg_lrc_noise_seed(level_seed(seeds[c], l)) */
static pmg_status chains_draw_lowrank_noise(pmg_mgmc h, int32_t C, const uint64_t *keys, const uint64_t *ctr, int *first, void *stream)
{
  pmgk_lrc_noise_plan plan;
  pmg_lrc             any    = NULL;
  int                 nslots = 0;
  plan.n = 0;
  for (int l = 0; l < h->nlevels; ++l) {
    pmg_lrc   lr = mg_level_sampler_lrc(h, l);
    const int n  = pmg_mgmc_i_level_sweeps(h, l);
    first[l]     = nslots;
    if (!lr || n <= 0) continue;
    plan.level[plan.n] = l;
    plan.first[plan.n] = nslots;
    plan.ctr0[plan.n]  = ctr[l];
    ++plan.n;
    nslots += n;
    any = lr;
  }
  if (!nslots) return PMG_SUCCESS;
  const int k = pmg_lrc_rank(any);
  PMG_CALL(pmg_devbuf_reserve(&h->ch_eta, sizeof(double) * (size_t)nslots * (size_t)k * (size_t)C, stream));
  PMG_KERNEL(pmgk_lrc_noise_batch_chains(nslots, k, C, keys, pmg_lrc_noise_seed(0), &plan, pmg_lrc_sqrtS(any), h->ch_eta.p, stream)); /* S is the same on every level (src/pc_gamgmc.c:170-176) */
  return PMG_SUCCESS;
}

/* one smoothing leg (`its` samples) of level l's sampler from draw number *done of the cycle on: plain sweeps on (b, bcs), or, on a level with a
   low-rank update, on bown -- the same right-hand side as ld x C doubles the cycle may write (the noise term goes in and out) */
static pmg_status chains_smooth(pmg_mgmc h, int l, int32_t C, const uint64_t *keys, int its, uint64_t *ctr, int first, int *done, const double *b, int bcs, double *bown, double *x, void *stream)
{
  mg_level *Lv = &h->lv[l];
  pmg_lrc   lr = mg_level_sampler_lrc(h, l);
  if (!lr) return pmg_mcsor_sweeps_chains(Lv->mc, C, keys + (size_t)l * C, 1, h->scaled, its, *ctr, ctr, b, bcs, x, stream);
  const int64_t kc = (int64_t)pmg_lrc_rank(lr) * C;
  PMG_CALL(pmg_mcsor_sweeps_lowrank_chains(Lv->mc, C, keys + (size_t)l * C, h->scaled, its, *ctr, ctr, (const double *)h->ch_eta.p + (int64_t)(first + *done) * kc, kc, bown, x, stream));
  *done += pmg_mgmc_i_leg_sweeps(h, l);
  return PMG_SUCCESS;
}

/* one V-cycle on C chains: top level right-hand side btop (chain stride bcs: 0 = the shared vector, 1 = per chain) and iterate
   xtop; every level below starts from zero, the top level too unless top_has_guess (mg_vcycle's rules).  btop_own: btop as
   ld x C doubles the cycle may write, for the sweeps of a top level with a low-rank update (btop itself where bcs = 1) */
static pmg_status mg_vcycle_chains(pmg_mgmc h, int32_t C, const uint64_t *keys, const double *btop, int bcs_top, double *btop_own, double *xtop, uint64_t sample, int top_has_guess, void *stream)
{
  const int top = h->nlevels - 1;
  uint64_t  ctr[64];
  int       zeroed[64], first[64], done[64];
  PMG_CHECK(h->nlevels <= 64, PMG_ERR_ARG_OUTOFRANGE, "too many levels");
  for (int l = 0; l <= top; ++l) {
    ctr[l]    = sample * MG_DRAWS_PER_SAMPLE;
    zeroed[l] = done[l] = first[l] = 0;
  }
  if (h->lrc_k > 0) PMG_CALL(chains_draw_lowrank_noise(h, C, keys, ctr, first, stream));
  for (int l = top; l >= 1; --l) {
    mg_level     *Lv  = &h->lv[l];
    const double *b   = l == top ? btop : h->ch_b[l].p;
    const int     bcs = l == top ? bcs_top : 1;
    double       *x   = l == top ? xtop : h->ch_x[l].p;
    if ((l < top || !top_has_guess) && !zeroed[l]) PMG_KERNEL(pmgk_fill_zero(x, Lv->ld * C, stream));
    PMG_CALL(chains_smooth(h, l, C, keys, h->nu, &ctr[l], first[l], &done[l], b, bcs, l == top ? btop_own : h->ch_b[l].p, x, stream));
    PMG_CALL(pmg_mcsor_residual_chains(Lv->mc, C, b, bcs, x, h->ch_r[l].p, stream)); /* with the low-rank term of a MATLRC level, src/pc_gamgmc.c:194 */
    /* b_{l-1} = P^T r, which also sets the coarse level's zero guess where one is needed (as mg_restrict does) */
    const int needs_zero = l - 1 >= 1 || h->coarse_type != 0;
    PMG_KERNEL(pmgk_csr_spmv_rows_chains(Lv->R_nrows, Lv->R_rowpos, Lv->R_rowptr, Lv->R_col, Lv->R_val, C, h->ch_r[l].p, h->ch_b[l - 1].p, 0, needs_zero ? h->ch_x[l - 1].p : NULL, stream));
    zeroed[l - 1] = needs_zero;
  }
  if (h->coarse_type == 0) PMG_CALL(pmg_chol_sample_chains(h->chol, C, keys, ctr[0], h->ch_b[0].p, h->ch_x[0].p, h->ch_xi.p, h->ch_v.p, stream));
  else {
    if (!zeroed[0]) PMG_KERNEL(pmgk_fill_zero(h->ch_x[0].p, h->lv[0].ld * C, stream));
    PMG_CALL(chains_smooth(h, 0, C, keys, h->coarse_its, &ctr[0], first[0], &done[0], h->ch_b[0].p, 1, h->ch_b[0].p, h->ch_x[0].p, stream));
  }
  for (int l = 1; l <= top; ++l) {
    mg_level     *Lv  = &h->lv[l];
    const double *b   = l == top ? btop : h->ch_b[l].p;
    const int     bcs = l == top ? bcs_top : 1;
    double       *x   = l == top ? xtop : h->ch_x[l].p;
    PMG_KERNEL(pmgk_csr_spmv_rows_chains(Lv->P_nrows, Lv->P_rowpos, Lv->P_rowptr, Lv->P_col, Lv->P_val, C, h->ch_x[l - 1].p, x, 1, NULL, stream)); /* x += P e */
    PMG_CALL(chains_smooth(h, l, C, keys, h->nu, &ctr[l], first[l], &done[l], b, bcs, l == top ? btop_own : h->ch_b[l].p, x, stream));
  }
  return PMG_SUCCESS;
}

/* checks of pmg_mgmc_sample_chains / pmg_mgmc_get_algorithmic_bytes_chains; the argument and support checks come before the
   set-up check, and nothing here touches the device */
static pmg_status mgmc_chains_check(pmg_mgmc h, int32_t C)
{
  PMG_CHECK(h->user_hier, PMG_ERR_SUP, "multi-chain sampling of DMDA hierarchies (pmg_mgmc_create_dmda*) is not supported: one chain already fills the device there");
  PMG_CHECK(!h->rb_dist, PMG_ERR_SUP, "multi-chain sampling of row-block distributed hierarchies is not supported");
  PMG_CHECK(!pmg_mgmc_i_has_blocks(h), PMG_ERR_SUP, "multi-chain sampling of a hierarchy with block smoothing (pmg_mgmc_set_level_blocks) is not supported");
  PMG_CHECK(!h->lrc_k || h->is_setup, PMG_ERR_SUP, "multi-chain sampling of a hierarchy with a low-rank (MATLRC) update: whether its levels carry the update is known after pmg_mgmc_setup only");
  PMG_CHECK(h->is_setup, PMG_ERR_ARG_WRONGSTATE, "call pmg_mgmc_setup first");
  for (int l = 0; l < h->nlevels; ++l) {
    const mg_level *Lv = &h->lv[l];
    PMG_CHECK(Lv->kind == MG_LV_SELL || Lv->kind == MG_LV_EXACT, PMG_ERR_SUP, "level %d is not a sliced-ELL level: not supported by the multi-chain cycle", l);
    if (Lv->kind == MG_LV_SELL) PMG_CALL(pmg_mcsor_chains_supported(Lv->mc));
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
  if (bcs) PMG_CALL(pmg_devbuf_reserve(&h->ch_B, sizeof(double) * (size_t)F->ld * (size_t)C, stream));
  uint64_t *kh = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)h->nlevels * (size_t)C);
  PMG_CHECK(kh, PMG_ERR_MEM, "out of host memory");
  for (int l = 0; l <= top; ++l)
    for (int32_t c = 0; c < C; ++c) kh[(size_t)l * C + c] = level_seed(seeds[c], l);
  const pmg_status kst = pmg_keybuf_set(&h->ch_keys, kh, (int64_t)h->nlevels * C, stream);
  free(kh);
  PMG_CALL(kst);
  const uint64_t *keys = h->ch_keys.dev.p;
  const int32_t  *orig = pmg_mcsor_orig_dev(F->mc);
  const int64_t   nel  = F->ld * C;
  const double   *btop = bcs ? h->ch_B.p : h->ch_bs.p;
  /* a top level with a low-rank update sweeps on a right-hand side the noise term can go onto: the library's copy of a per-chain
     B, or the shared b spread over ch_b[top] ONCE per call -- the term goes in and out bit for bit.  (The literal form's own cycles
     run on ch_b[top] = w, which then replaces the spread b: that one is needed for its = 0 with guesszero only.) */
  const int lrtop = mg_level_sampler_lrc(h, top) != NULL;
  double   *bown  = !lrtop ? NULL : (bcs ? h->ch_B.p : h->ch_b[top].p);
  if (lrtop && !bcs && its > 0 && (!h->correction_form || guesszero)) PMG_KERNEL(pmgk_permute_in_chains(F->ld, orig, C, b_nat, 0, h->ch_b[top].p, stream));
  if (bcs) PMG_KERNEL(pmgk_permute_in_chains(F->ld, orig, C, b_nat, 1, h->ch_B.p, stream));
  else PMG_KERNEL(pmgk_permute_in(F->ld, orig, b_nat, h->ch_bs.p, stream));
  PMG_KERNEL(pmgk_permute_in_chains(F->ld, orig, C, Y_nat, 1, h->ch_Y.p, stream));
  for (int32_t it = 0; it < its; ++it) {
    const uint64_t sample = counter0 + (uint64_t)it;
    if (!h->correction_form || (it == 0 && guesszero)) /* in place on (b, Y), pmg_mgmc_sample's default; or Y = MG(b) (src/pc_gamgmc.c:243-246) */
      PMG_CALL(mg_vcycle_chains(h, C, keys, btop, bcs, bown, h->ch_Y.p, sample, !h->correction_form && !(it == 0 && guesszero), stream));
    else { /* w = b - A y; work = MG(w); y += work, src/pc_gamgmc.c:253-256 */
      PMG_CALL(pmg_mcsor_residual_chains(F->mc, C, btop, bcs, h->ch_Y.p, h->ch_b[top].p, stream));
      PMG_CALL(mg_vcycle_chains(h, C, keys, h->ch_b[top].p, 1, h->ch_b[top].p, h->ch_x[top].p, sample, 0, stream));
      PMG_KERNEL(pmgk_axpy(nel, 1.0, h->ch_x[top].p, h->ch_Y.p, stream));
    }
    if (cb) {
      PMG_KERNEL(pmgk_permute_out_chains(F->ld, orig, C, h->ch_Y.p, Y_nat, stream));
      const int rc = cb(it, Y_nat, F->n, C, cbctx);
      PMG_CHECK(rc == 0, rc, "sample callback returned %d", rc);
    }
  }
  PMG_KERNEL(pmgk_permute_out_chains(F->ld, orig, C, h->ch_Y.p, Y_nat, stream));
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
   right-hand side is per chain.  per_level (may be NULL): nlevels entries, transfers charged to their fine level.
   A level with a LOW-RANK update (rank k; n = its ns support rows, or all N rows in the dense form; idx = 8 n, the row positions,
   0 in the dense form; nb = ceil(n / 1024), dense ceil(N / 4096), blocks of B^T y) adds per launch, B_l, Bb_l and the rows once,
   k-vectors and touched iterate rows C times:
     noise term in place                  8 k n + idx + 8 k C + 24 n C       (B_l, eta; b read + written, the old entries kept)
     update  U(restore)                   8 k n + idx + 8 k C + 16 n C, + 16 n C with the restore (kept entries read, b written)
     B^T y block sums                     8 k n + idx + 8 n C + 8 nb k C
     reduction  R(scale)                  8 nb k C + 8 k C, + 8 k with the scale S
     one workgroup  F(restore, scale)     16 k n + idx + 24 n C, + 16 n C with the restore, + 8 k with the scale
     repair  = F(1, 0) on a support of one block (compact, n <= 1024), else block sums + R(0) + U(1)
     residual term = F(0, 1) there, else block sums + R(1) + U(0)
   per cycle:  s_l (noise term + repair) with s_l = 2 nu ndir directional sweeps (coarse_its ndir on a Gibbs coarsest level), one
   residual term on every level above the coarsest, a second one on the finest level of the literal form (the outer residual),
   8 k C s_l + 8 C for the level's share of the cycle's ONE noise launch (its draws, its keys) and 8 k once for sqrt(S), charged to
   the finest level.  The top level of the in-place form sweeps on the spread copy of b: each of its 2 nu ndir sweeps is a
   per-chain-b sweep (+ 8 N C - 8 N); spreading b is once per call, not per cycle, and not counted. */
static double chains_lowrank_bytes(pmg_mgmc h, int l, double Cd)
{
  pmg_lrc lr = mg_level_sampler_lrc(h, l);
  if (!lr) return 0.0;
  const int top = h->nlevels - 1;
  int32_t   k;
  int64_t   ns;
  int       dense;
  pmg_lrc_get_sizes(lr, &k, &ns, &dense);
  const double K = k, N = (double)h->lv[l].n, n = dense ? N : (double)ns, idx = dense ? 0.0 : 8.0 * n;
  const double nb = dense ? (double)((h->lv[l].n + 4095) / 4096) : (double)((ns + 1023) / 1024), s = pmg_mgmc_i_level_sweeps(h, l);
  const double noise = 8.0 * K * n + idx + 8.0 * K * Cd + 24.0 * n * Cd, upd = 8.0 * K * n + idx + 8.0 * K * Cd + 16.0 * n * Cd;
  const double btx = 8.0 * K * n + idx + 8.0 * n * Cd + 8.0 * nb * K * Cd, red = 8.0 * nb * K * Cd + 8.0 * K * Cd, one = 16.0 * K * n + idx + 24.0 * n * Cd;
  const int    fused  = pmg_lrc_chains_fused(lr);
  const double repair = fused ? one + 16.0 * n * Cd : btx + red + upd + 16.0 * n * Cd;
  const double resid  = fused ? one + 8.0 * K : btx + red + 8.0 * K + upd;
  double       by     = s * (noise + repair) + 8.0 * K * Cd * s + 8.0 * Cd;
  if (l >= 1) by += resid;
  if (l == top) by += 8.0 * K + (h->correction_form ? resid : 2.0 * h->nu * pmg_sweep_ndir(h->sweep_type) * (8.0 * N * Cd - 8.0 * N));
  return by;
}

pmg_status pmg_mgmc_get_algorithmic_bytes_chains(pmg_mgmc h, int32_t C, double *total, double *per_level)
{
  PMG_CHECK(h && total, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(C >= 1, PMG_ERR_ARG_OUTOFRANGE, "nchains = %d", C);
  PMG_CALL(mgmc_chains_check(h, C));
  const int    top  = h->nlevels - 1;
  const double Cd   = (double)C;
  *total            = 0.0;
  for (int l = 0; l <= top; ++l) {
    const mg_level *Lv  = &h->lv[l];
    const double    N   = (double)Lv->n, nnz = (double)Lv->A_nnz;
    const double    swp = 12.0 * nnz + 16.0 * N + 24.0 * N * Cd; /* per-chain b */
    double          by  = 0.0;
    if (l == 0) by = h->coarse_type == 0 ? 8.0 * N * N + 48.0 * N * Cd : 8.0 * N * Cd + pmg_mgmc_i_level_sweeps(h, l) * swp;
    else {
      const double Nc     = (double)h->lv[l - 1].n, nnzP = (double)Lv->P_nnz;
      const int    shared = l == top && !h->correction_form;
      by += pmg_mgmc_i_level_sweeps(h, l) * (shared ? 12.0 * nnz + 24.0 * N + 16.0 * N * Cd : swp);
      if (!shared) by += 8.0 * N * Cd;                                                   /* zero fill */
      by += 12.0 * nnz + 12.0 * N + 16.0 * N * Cd + (shared ? 8.0 * N : 8.0 * N * Cd); /* residual */
      by += 12.0 * nnzP + 8.0 * Nc + 8.0 * N * Cd + 8.0 * Nc * Cd;                     /* restriction */
      by += 12.0 * nnzP + 8.0 * N + 16.0 * N * Cd + 8.0 * Nc * Cd;                     /* prolongation */
      if (l == top && h->correction_form) by += (12.0 * nnz + 12.0 * N + 16.0 * N * Cd + 8.0 * N) + 24.0 * N * Cd;
    }
    by += chains_lowrank_bytes(h, l, Cd);
    if (per_level) per_level[l] = by;
    *total += by;
  }
  return PMG_SUCCESS;
}
