/* Coloured block Gibbs sampler -- the handle (C11): keeps the caller's blocks and options, has pmg_blockgibbs_host.c build the
 * plan at set-up, uploads it and launches one kernel per block colour (kernels_blockgibbs.hip).
 *
 * Replaces, per patch, PCSetUp_CholSampler's dense factorisation (reference src/pc_chols.c:174-194), PCApply_CholSampler's
 * solve + noise (:220-260) and its Richardson wrapper (:284-287), in the multiplicative patch loop examples/ex13.py:11-22
 * composes with PCASM. */
#include "pmg_internal.h"

struct pmg_blockgibbs_s {
  /* borrowed host CSR (valid until setup) */
  int32_t        n;
  const int32_t *rowptr, *colidx;
  const double  *vals;
  /* owned copies of what the caller described */
  int32_t  nblocks, *blockptr, *blockrows;
  int32_t  user_ncolors, *user_colors;
  int32_t  ld, *pos_of_row;
  int      type;
  /* set-up products */
  int             is_setup;
  pmg_bg_plan     plan; /* host: colours, tile ranges, W; the packed arrays are freed once they are on the device */
  pmgk_blockgibbs K;    /* device */
  double          bytes;
  pmg_keybuf      ch_keys; /* the noise keys of the last chains call: the only per-object state of the chains entry points */
};

#define BG_SETUP(bg) PMG_CHECK((bg)->is_setup, PMG_ERR_ARG_WRONGSTATE, "call pmg_blockgibbs_setup first")
#define BG_NOT_SETUP(bg, what) PMG_CHECK(!(bg)->is_setup, PMG_ERR_ARG_WRONGSTATE, what " must be chosen before pmg_blockgibbs_setup")

static pmg_status copy_i32(int32_t **dst, const int32_t *src, int64_t count)
{
  free(*dst);
  *dst = (int32_t *)malloc(sizeof(int32_t) * (size_t)(count > 0 ? count : 1));
  PMG_CHECK(*dst, PMG_ERR_MEM, "out of host memory");
  if (count > 0) memcpy(*dst, src, sizeof(int32_t) * (size_t)count);
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_create_csr(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, int32_t nblocks, const int32_t *blockptr, const int32_t *blockrows, pmg_blockgibbs *out)
{
  PMG_CHECK(out, PMG_ERR_ARG_NULL, "null output handle");
  *out = NULL;
  PMG_CHECK(n >= 0, PMG_ERR_ARG_OUTOFRANGE, "n = %d", n);
  PMG_CHECK(rowptr && (colidx || rowptr[n] == 0) && (vals || rowptr[n] == 0), PMG_ERR_ARG_NULL, "null CSR array");
  PMG_CALL(pmg_bg_check_blocks(n, nblocks, blockptr, blockrows));
  pmg_blockgibbs bg = (pmg_blockgibbs)calloc(1, sizeof *bg);
  PMG_CHECK(bg, PMG_ERR_MEM, "out of host memory");
  bg->n       = n;
  bg->rowptr  = rowptr;
  bg->colidx  = colidx;
  bg->vals    = vals;
  bg->nblocks = nblocks;
  bg->type    = PMG_SOR_FORWARD_SWEEP;
  pmg_status st = copy_i32(&bg->blockptr, blockptr, (int64_t)nblocks + 1);
  if (!st) st = copy_i32(&bg->blockrows, blockrows, blockptr[nblocks]);
  if (st) {
    pmg_blockgibbs_destroy(&bg);
    return st;
  }
  *out = bg;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_set_coloring(pmg_blockgibbs bg, int32_t ncolors, const int32_t *block_colors)
{
  PMG_CHECK(bg, PMG_ERR_ARG_NULL, "null block Gibbs handle");
  BG_NOT_SETUP(bg, "the colouring");
  if (!block_colors) { /* back to first-fit */
    free(bg->user_colors);
    bg->user_colors = NULL;
    return PMG_SUCCESS;
  }
  PMG_CHECK(ncolors >= 0, PMG_ERR_ARG_OUTOFRANGE, "ncolors = %d", ncolors);
  PMG_CALL(copy_i32(&bg->user_colors, block_colors, bg->nblocks));
  bg->user_ncolors = ncolors;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_set_layout(pmg_blockgibbs bg, int32_t ld, const int32_t *pos_of_row)
{
  PMG_CHECK(bg, PMG_ERR_ARG_NULL, "null block Gibbs handle");
  BG_NOT_SETUP(bg, "the layout");
  PMG_CHECK(pos_of_row || bg->n == 0, PMG_ERR_ARG_NULL, "null position array");
  PMG_CHECK(ld >= bg->n, PMG_ERR_ARG_OUTOFRANGE, "layout length %d for %d rows", ld, bg->n);
  PMG_CALL(copy_i32(&bg->pos_of_row, pos_of_row, bg->n));
  bg->ld = ld;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_set_sweep_type(pmg_blockgibbs bg, int type)
{
  PMG_CHECK(bg, PMG_ERR_ARG_NULL, "null block Gibbs handle");
  PMG_CHECK(pmg_sweep_type_ok(type), PMG_ERR_SUP, "Only forward, backward and symmetric sweep supported"); /* src/mc_sor.c:427 */
  bg->type = type;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_get_sweep_type(pmg_blockgibbs bg, int *type)
{
  PMG_CHECK(bg && type, PMG_ERR_ARG_NULL, "null argument");
  *type = bg->type;
  return PMG_SUCCESS;
}

static void bg_free_device(pmg_blockgibbs bg)
{
  pmg_dev_free((void *)bg->K.tile_g), pmg_dev_free((void *)bg->K.tile_ew), pmg_dev_free((void *)bg->K.tile_foff), pmg_dev_free((void *)bg->K.tile_eoff);
  pmg_dev_free((void *)bg->K.pos), pmg_dev_free((void *)bg->K.slot), pmg_dev_free((void *)bg->K.M), pmg_dev_free((void *)bg->K.WT);
  pmg_dev_free((void *)bg->K.evals), pmg_dev_free((void *)bg->K.ecols);
  memset(&bg->K, 0, sizeof bg->K);
}

pmg_status pmg_blockgibbs_setup(pmg_blockgibbs bg)
{
  PMG_CHECK(bg, PMG_ERR_ARG_NULL, "null block Gibbs handle");
  if (bg->is_setup) return PMG_SUCCESS; /* the borrowed CSR was released after the first set-up */
  pmg_bg_plan *pl = &bg->plan;
  PMG_CALL(pmg_bg_plan_build(bg->n, bg->rowptr, bg->colidx, bg->vals, bg->nblocks, bg->blockptr, bg->blockrows, bg->user_ncolors, bg->user_colors, bg->ld, bg->pos_of_row, pl));
  const size_t nt = (size_t)pl->ntiles, ftot = (size_t)pl->tile_foff[nt], etot = (size_t)pl->tile_eoff[nt];
  /* the byte model of one noisy directional sweep */
  bg->bytes     = 2.0 * 8.0 * (double)ftot + 12.0 * (double)pl->nnz_ext + 28.0 * (double)pl->nslots;
  pmg_status st = pmg_dev_upload((void **)&bg->K.tile_g, pl->tile_g, sizeof(int32_t) * nt);
  if (!st) st = pmg_dev_upload((void **)&bg->K.tile_ew, pl->tile_ew, sizeof(int32_t) * nt);
  if (!st) st = pmg_dev_upload((void **)&bg->K.tile_foff, pl->tile_foff, sizeof(int64_t) * (nt + 1));
  if (!st) st = pmg_dev_upload((void **)&bg->K.tile_eoff, pl->tile_eoff, sizeof(int64_t) * (nt + 1));
  if (!st) st = pmg_dev_upload((void **)&bg->K.pos, pl->pos, sizeof(int32_t) * nt * 64);
  if (!st) st = pmg_dev_upload((void **)&bg->K.slot, pl->slot, sizeof(int32_t) * nt * 64);
  if (!st) st = pmg_dev_upload((void **)&bg->K.M, pl->M, sizeof(double) * ftot);
  if (!st) st = pmg_dev_upload((void **)&bg->K.WT, pl->WT, sizeof(double) * ftot);
  if (!st) st = pmg_dev_upload((void **)&bg->K.evals, pl->evals, sizeof(double) * etot);
  if (!st) st = pmg_dev_upload((void **)&bg->K.ecols, pl->ecols, sizeof(int32_t) * etot);
  if (st) {
    bg_free_device(bg);
    pmg_bg_plan_free(pl);
    return st;
  }
  /* on the device now; the host keeps the colours, the tile ranges and W */
  free(pl->M), free(pl->WT), free(pl->evals), free(pl->ecols), free(pl->L), free(pl->pos), free(pl->slot);
  pl->M = pl->WT = pl->evals = pl->L = NULL;
  pl->ecols = pl->pos = pl->slot = NULL;
  bg->is_setup = 1;
  bg->rowptr = bg->colidx = NULL;
  bg->vals                = NULL;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_get_num_colors(pmg_blockgibbs bg, int32_t *ncolors)
{
  PMG_CHECK(bg && ncolors, PMG_ERR_ARG_NULL, "null argument");
  BG_SETUP(bg);
  *ncolors = bg->plan.ncolors;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_get_coloring(pmg_blockgibbs bg, int32_t *block_colors)
{
  PMG_CHECK(bg && block_colors, PMG_ERR_ARG_NULL, "null argument");
  BG_SETUP(bg);
  if (bg->nblocks) memcpy(block_colors, bg->plan.colors, sizeof(int32_t) * (size_t)bg->nblocks);
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_get_num_slots(pmg_blockgibbs bg, int32_t *nslots)
{
  PMG_CHECK(bg && nslots, PMG_ERR_ARG_NULL, "null argument");
  BG_SETUP(bg);
  *nslots = bg->plan.nslots;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_get_block_factor(pmg_blockgibbs bg, int32_t p, int32_t *m, double *W_host)
{
  PMG_CHECK(bg && m, PMG_ERR_ARG_NULL, "null argument");
  BG_SETUP(bg);
  PMG_CHECK(p >= 0 && p < bg->nblocks, PMG_ERR_ARG_OUTOFRANGE, "block %d of %d", p, bg->nblocks);
  *m = bg->blockptr[p + 1] - bg->blockptr[p];
  if (W_host) memcpy(W_host, bg->plan.W + bg->plan.woff[p], sizeof(double) * (size_t)(*m) * (size_t)(*m));
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_get_algorithmic_bytes(pmg_blockgibbs bg, double *bytes)
{
  PMG_CHECK(bg && bytes, PMG_ERR_ARG_NULL, "null argument");
  BG_SETUP(bg);
  *bytes = bg->bytes;
  return PMG_SUCCESS;
}

/* one direction over all block colours; mode as pmgk_blockgibbs_color_sweep */
pmg_status pmg_blockgibbs_dir_sweep(pmg_blockgibbs bg, int dir, int mode, uint64_t seed, uint64_t sweep, const double *xi_slots, const double *b, double *y, void *stream)
{
  const pmg_bg_plan *pl = &bg->plan;
  int                rc = 0;
  for (int32_t cc = 0; cc < pl->ncolors && !rc; ++cc) {
    const int32_t c = pmg_sweep_color(dir, pl->ncolors, cc);
    rc = pmgk_blockgibbs_color_sweep(&bg->K, pl->ctile[c], pl->ctile[c + 1] - pl->ctile[c], mode, seed, sweep, xi_slots, b, y, stream);
  }
  PMG_KERNEL(rc);
  return PMG_SUCCESS;
}

static pmg_status bg_sweeps(pmg_blockgibbs bg, int32_t its, int noisy, uint64_t seed, uint64_t counter0, uint64_t *counter_out, const double *b, double *y, void *stream)
{
  pmg_sweep_iter it = pmg_sweep_begin(bg->type, its, noisy, counter0);
  while (pmg_sweep_next(&it)) PMG_CALL(pmg_blockgibbs_dir_sweep(bg, it.dir, noisy, seed, it.sweep, NULL, b, y, stream));
  if (counter_out) *counter_out = it.ctr;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_apply(pmg_blockgibbs bg, const double *b, double *y, void *stream)
{
  PMG_CHECK(bg && b && y, PMG_ERR_ARG_NULL, "null argument");
  BG_SETUP(bg);
  return bg_sweeps(bg, 1, 0, 0, 0, NULL, b, y, stream);
}

pmg_status pmg_blockgibbs_sample(pmg_blockgibbs bg, const double *b, double *y, int32_t its, uint64_t seed, uint64_t counter0, uint64_t *counter_out, void *stream)
{
  PMG_CHECK(bg && b && y, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(its >= 0, PMG_ERR_ARG_OUTOFRANGE, "its = %d", its);
  BG_SETUP(bg);
  return bg_sweeps(bg, its, 1, seed, counter0, counter_out, b, y, stream);
}

pmg_status pmg_blockgibbs_sweep_xi(pmg_blockgibbs bg, int backward, const double *xi_slots, const double *b, double *y, void *stream)
{
  PMG_CHECK(bg && b && y && (xi_slots || (bg->is_setup && !bg->plan.nslots)), PMG_ERR_ARG_NULL, "null argument");
  BG_SETUP(bg);
  return pmg_blockgibbs_dir_sweep(bg, backward ? PMG_SOR_BACKWARD_SWEEP : PMG_SOR_FORWARD_SWEEP, 2, 0, 0, xi_slots, b, y, stream);
}

/* ---- many chains per launch -------------------------------------------------------------------------------------------
   Y is len x C doubles, chain fastest, in the handle's own indexing (rows, or positions after pmg_blockgibbs_set_layout): the
   vectors are in their layout already, so there is no permutation and no iterate workspace.  One launch per block colour
   sweeps every chain (kernels_blockgibbs_chains.hip); column c follows the single-chain path with key keys[c]. */

static int64_t bg_len(pmg_blockgibbs bg) { return bg->pos_of_row ? bg->ld : bg->n; }

/* one direction over all block colours on C chains; mode as pmgk_blockgibbs_color_sweep, bcs = chain stride of b (0 | 1) */
pmg_status pmg_blockgibbs_dir_sweep_chains(pmg_blockgibbs bg, int dir, int mode, int32_t C, const uint64_t *keys_dev, uint64_t sweep, const double *Xi, const double *b, int bcs, double *Y, void *stream)
{
  const pmg_bg_plan *pl = &bg->plan;
  int                rc = 0;
  for (int32_t cc = 0; cc < pl->ncolors && !rc; ++cc) {
    const int32_t c = pmg_sweep_color(dir, pl->ncolors, cc);
    rc = pmgk_blockgibbs_color_sweep_chains(&bg->K, pl->ctile[c], pl->ctile[c + 1] - pl->ctile[c], mode, C, keys_dev, sweep, Xi, b, bcs, Y, stream);
  }
  PMG_KERNEL(rc);
  return PMG_SUCCESS;
}

/* the checks of every chains entry point, before any device work: NULL, ranges, sizes, state -- in this order */
static pmg_status bg_chains_args(pmg_blockgibbs bg, int32_t C, int need_seeds, const uint64_t *seeds, const void *xi, int need_xi, const double *b, const double *Y, int32_t its)
{
  PMG_CHECK(bg, PMG_ERR_ARG_NULL, "null block Gibbs handle");
  PMG_CHECK(b && Y && (seeds || !need_seeds) && (xi || !need_xi || (bg->is_setup && !bg->plan.nslots)), PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(C >= 1, PMG_ERR_ARG_OUTOFRANGE, "nchains = %d", C);
  PMG_CHECK(its >= 0, PMG_ERR_ARG_OUTOFRANGE, "its = %d", its);
  PMG_CALL(pmg_chains_size_check(bg_len(bg), C));
  BG_SETUP(bg);
  return PMG_SUCCESS;
}

static pmg_status bg_chains_run(pmg_blockgibbs bg, int32_t C, const uint64_t *seeds, int noisy, const double *b, int bcs, double *Y, int32_t its, uint64_t counter0, uint64_t *counter_out, pmg_chains_callback cb, void *cbctx, void *stream)
{
  PMG_CALL(bg_chains_args(bg, C, noisy, seeds, NULL, 0, b, Y, its));
  if (noisy) PMG_CALL(pmg_keybuf_set(&bg->ch_keys, seeds, C, stream));
  const int      ndir = pmg_sweep_ndir(bg->type);
  pmg_sweep_iter it   = pmg_sweep_begin(bg->type, its, noisy, counter0);
  while (pmg_sweep_next(&it)) {
    PMG_CALL(pmg_blockgibbs_dir_sweep_chains(bg, it.dir, noisy, C, noisy ? bg->ch_keys.dev.p : NULL, it.sweep, NULL, b, bcs, Y, stream));
    if (cb && (it.index + 1) % ndir == 0) { /* a sample is complete */
      const int rc = cb((int32_t)(it.index / ndir), Y, (int32_t)bg_len(bg), C, cbctx);
      PMG_CHECK(rc == 0, rc, "sample callback returned %d", rc);
    }
  }
  if (counter_out) *counter_out = it.ctr;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_apply_chains(pmg_blockgibbs bg, int32_t nchains, const double *b, double *Y, void *stream)
{
  return bg_chains_run(bg, nchains, NULL, 0, b, 0, Y, 1, 0, NULL, NULL, NULL, stream);
}

pmg_status pmg_blockgibbs_sample_chains(pmg_blockgibbs bg, int32_t nchains, const uint64_t *seeds, const double *b, double *Y, int32_t its, uint64_t counter0, uint64_t *counter_out, pmg_chains_callback cb, void *cbctx, void *stream)
{
  return bg_chains_run(bg, nchains, seeds, 1, b, 0, Y, its, counter0, counter_out, cb, cbctx, stream);
}

pmg_status pmg_blockgibbs_sample_chains_rhs(pmg_blockgibbs bg, int32_t nchains, const uint64_t *seeds, const double *B, double *Y, int32_t its, uint64_t counter0, uint64_t *counter_out, pmg_chains_callback cb, void *cbctx, void *stream)
{
  return bg_chains_run(bg, nchains, seeds, 1, B, 1, Y, its, counter0, counter_out, cb, cbctx, stream);
}

pmg_status pmg_blockgibbs_sweep_xi_chains(pmg_blockgibbs bg, int32_t nchains, int backward, const double *Xi_slots, const double *b, double *Y, void *stream)
{
  PMG_CALL(bg_chains_args(bg, nchains, 0, NULL, Xi_slots, 1, b, Y, 0));
  return pmg_blockgibbs_dir_sweep_chains(bg, backward ? PMG_SOR_BACKWARD_SWEEP : PMG_SOR_FORWARD_SWEEP, 2, nchains, NULL, 0, Xi_slots, b, 0, Y, stream);
}

/* one noisy directional sweep on C chains; operands every chain shares (factors, exterior entries, positions, a shared b) count once */
pmg_status pmg_blockgibbs_get_algorithmic_bytes_chains(pmg_blockgibbs bg, int32_t nchains, int per_chain_rhs, double *bytes)
{
  PMG_CHECK(bg && bytes, PMG_ERR_ARG_NULL, "null argument");
  PMG_CHECK(nchains >= 1, PMG_ERR_ARG_OUTOFRANGE, "nchains = %d", nchains);
  BG_SETUP(bg);
  const pmg_bg_plan *pl = &bg->plan;
  const double       ns = (double)pl->nslots, C = (double)nchains;
  *bytes = 2.0 * 8.0 * (double)pl->tile_foff[pl->ntiles] + 12.0 * (double)pl->nnz_ext + 4.0 * ns + 8.0 * ns * (per_chain_rhs ? C : 1.0) + 16.0 * ns * C;
  return PMG_SUCCESS;
}

pmg_status pmg_blockgibbs_destroy(pmg_blockgibbs *bg)
{
  if (!bg || !*bg) return PMG_SUCCESS;
  pmg_keybuf_free(&(*bg)->ch_keys);
  bg_free_device(*bg);
  pmg_bg_plan_free(&(*bg)->plan);
  free((*bg)->blockptr), free((*bg)->blockrows), free((*bg)->user_colors), free((*bg)->pos_of_row);
  free(*bg);
  *bg = NULL;
  return PMG_SUCCESS;
}
