/* Host-side internals of libparmgmc_hip (C11). */
#ifndef PMG_INTERNAL_H
#define PMG_INTERNAL_H
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/parmgmc_hip.h"
#include "pmg_kernels.h"
#include "pmg_switch.h"

#define PMG_VERSION_STRING "0.1.0"

/* Records file:line + message for pmg_last_error_string() and returns `code` (PetscCheck analogue:
   reference code raises through PetscCheck(cond, comm, PETSC_ERR_*, fmt...), e.g. src/mc_sor.c:427). */
pmg_status pmg_set_error(pmg_status code, const char *file, int line, const char *fmt, ...);

#define PMG_FAIL(code, ...) return pmg_set_error((code), __FILE__, __LINE__, __VA_ARGS__)
#define PMG_CHECK(cond, code, ...) \
  do { \
    if (!(cond)) return pmg_set_error((code), __FILE__, __LINE__, __VA_ARGS__); \
  } while (0)
/* PetscCall analogue */
#define PMG_CALL(expr) \
  do { \
    pmg_status pmg_s_ = (expr); \
    if (pmg_s_) return pmg_s_; \
  } while (0)
#define PMG_HIP(expr) \
  do { \
    hipError_t pmg_e_ = (expr); \
    if (pmg_e_ != hipSuccess) return pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "%s: %s", #expr, hipGetErrorString(pmg_e_)); \
  } while (0)
#define PMG_KERNEL(expr) \
  do { \
    if ((expr) != 0) return pmg_set_error(PMG_ERR_GPU, __FILE__, __LINE__, "kernel launch failed: %s", #expr); \
  } while (0)

static inline int pmg_sweep_type_ok(int t) { return t == PMG_SOR_FORWARD_SWEEP || t == PMG_SOR_BACKWARD_SWEEP || t == PMG_SOR_SYMMETRIC_SWEEP; }

/* ---- the sweep schedule of every sampler: "`its` samples of sweep type `type`, starting at draw counter counter0" ----
   A symmetric sample is a forward, then a backward directional sweep (src/mc_sor.c:223-232).  Every noisy directional
   sweep takes the next draw counter, so a symmetric sample draws twice (src/pc_mcgibbs.c:172-181).  A forward sweep visits
   the colours in ascending, a backward one in descending order (src/mc_sor.c:256-289, :317, :344).
     pmg_sweep_iter it = pmg_sweep_begin(type, its, noisy, counter0);
     while (pmg_sweep_next(&it)) ... one directional sweep it.dir with draw counter it.sweep ...
     if (counter_out) *counter_out = it.ctr; */
typedef struct {
  int      type, noisy;
  int64_t  total, index; /* directional sweeps of the call; the current one's number, from 0 */
  uint64_t counter0;
  int      dir;   /* PMG_SOR_FORWARD_SWEEP or PMG_SOR_BACKWARD_SWEEP */
  uint64_t sweep; /* counter0 + index: the draw counter of a noisy sweep (a deterministic sweep reads none) */
  uint64_t ctr;   /* what the call hands back through counter_out: behind the last noisy sweep so far */
} pmg_sweep_iter;

static inline int pmg_sweep_ndir(int type) { return type == PMG_SOR_SYMMETRIC_SWEEP ? 2 : 1; }

static inline pmg_sweep_iter pmg_sweep_begin(int type, int32_t its, int noisy, uint64_t counter0)
{
  const pmg_sweep_iter it = {type, noisy, (int64_t)its * pmg_sweep_ndir(type), -1, counter0, type, counter0, counter0};
  return it;
}

static inline int pmg_sweep_next(pmg_sweep_iter *it) /* 0 at the end */
{
  if (it->index + 1 >= it->total) return 0;
  ++it->index;
  it->dir   = it->type != PMG_SOR_SYMMETRIC_SWEEP ? it->type : (it->index % 2 == 0 ? PMG_SOR_FORWARD_SWEEP : PMG_SOR_BACKWARD_SWEEP);
  it->sweep = it->counter0 + (uint64_t)it->index;
  if (it->noisy) it->ctr = it->sweep + 1;
  return 1;
}

/* the cc-th colour a directional sweep visits */
static inline int32_t pmg_sweep_color(int dir, int32_t ncolors, int32_t cc) { return dir == PMG_SOR_FORWARD_SWEEP ? cc : ncolors - 1 - cc; }

#define PMG_CHECK_UNSCALED_NOISE(noisy, scaled, omega) PMG_CHECK(!(noisy) || (scaled) || (omega) == 1.0, PMG_ERR_SUP, "the unscaled (sorgibbs) noise requires omega = 1 (src/pc_sorgibbs.c:94)")

pmg_status pmg_grid_set_lowrank_dev(pmg_grid g, int32_t k, const double *B_cvec_dev, const double *S_host);
pmg_status pmg_grid_sweep_color_halo_cvec(pmg_grid g, int color, int noisy, int scaled, uint64_t seed, uint64_t counter, const pmgk_grid_halo *halo, const double *b, double *y, void *stream);
pmg_status pmg_grid_sweep_color_faces_cvec(pmg_grid g, int color, int noisy, int scaled, uint64_t seed, uint64_t counter, const pmgk_grid_halo *halo, const double *b, double *y, void *stream);
/* kernel-side description of a grid object (internal) */
pmg_status pmg_grid_get_kernel_layout(pmg_grid g, pmgk_grid_layout *L);
/* residual and Q1 restriction fused; *done = 0 when the fused kernel does not apply (the caller runs the two steps) */
int32_t    pmg_grid_line_stride(int32_t nx, int32_t ny, int32_t nzg); /* doubles per line of a colour array */
int        pmg_grid_residual_restrict_applies(pmg_grid g, const pmgk_st27_dims *C, int have_lo2, int have_hi2);
pmg_status pmg_grid_residual_restrict(pmg_grid g, const double *b, const double *y, const double *ylo2, const double *yhi2, const pmgk_st27_dims *C, double *b_coarse, int *done, void *stream);

#define PMG_XCH_MAXSEG 4
/* low-rank (MATLRC) helper shared by pmg_mcsor and pmg_grid (pmg_lrc.c); vectors in the sampler's layout */
typedef struct pmg_lrc_s *pmg_lrc;
typedef pmg_status (*pmg_det_sweep_fn)(void *ctx, int dir, const double *b_lay, double *y_lay, void *stream);
/* what a sampler's directional sweep needs besides (dir, b, y): the usual context of a pmg_det_sweep_fn */
typedef struct {
  void    *obj; /* the sampler */
  int      noisy, scaled;
  uint64_t seed, sweep;
} pmg_sweep_args;
typedef pmg_status (*pmg_lrc_reduce_fn)(void *ctx, double *vals_dev, int count, void *stream);
pmg_status pmg_lrc_build_dev(pmg_lrc *out, int32_t k, int64_t ld, const double *B_lay_dev, const double *S_host, pmg_det_sweep_fn det, void *ctx, pmg_lrc_reduce_fn reduce, void *rctx);
pmg_status pmg_lrc_build(pmg_lrc *out, int32_t k, int64_t ld, int32_t n, const double *B_nat_host, const int64_t *pos, const double *S_host, pmg_det_sweep_fn det, void *ctx);
pmg_status pmg_lrc_rhs(pmg_lrc l, const double *b_lay, uint64_t seed, uint64_t counter, const double **beff, void *stream);
pmg_status pmg_lrc_rhs_done(pmg_lrc l, void *stream); /* after the sweep that used the vector pmg_lrc_rhs returned */
pmg_status pmg_lrc_post(pmg_lrc l, int dir, double *y_lay, void *stream);
/* one directional sweep of an operator with an optional update (l = NULL: the sweep alone).  The sweep itself is sweep_fn(ctx, dir, rhs,
   *y_lay, stream): ctx->sor(...) then ctx->postsor(...) of src/mc_sor.c:223-236, with the extra noise term of PrepareRHS_LRC
   (src/pc_mcgibbs.c:130-140) on rhs when the sweep is a noisy one.  *y_lay is read again behind the sweep, which may swap the iterate's buffers */
pmg_status pmg_lrc_dir_sweep(pmg_lrc l, int noisy, int dir, uint64_t seed, uint64_t counter, pmg_det_sweep_fn sweep_fn, void *ctx, const double *b_lay, double *const *y_lay, void *stream);
pmg_status pmg_lrc_residual_sub(pmg_lrc l, const double *x_lay, double *r_lay, void *stream);
pmg_status pmg_lrc_residual_sub_restricted(pmg_lrc l_fine, pmg_lrc l_coarse, const double *x_fine_lay, double *b_coarse_lay, void *stream);
void       pmg_lrc_preset_eta(pmg_lrc l, uint64_t seed, uint64_t counter0, int n, const double *eta_dev, int64_t stride); /* noise terms drawn ahead */
uint64_t      pmg_lrc_noise_seed(uint64_t seed);
const double *pmg_lrc_sqrtS(pmg_lrc l); /* device, k entries */
int           pmg_lrc_rank(pmg_lrc l);
void       pmg_lrc_expect_residual(pmg_lrc l, int on); /* the sweeps that follow are in front of a residual of the same vector */
int        pmg_lrc_is_local(pmg_lrc l);
void       pmg_lrc_get_sizes(pmg_lrc l, int32_t *k, int64_t *ns, int *dense); /* ns = 0: none of B's support on this rank */
pmg_status pmg_lrc_get_compact(pmg_lrc l, int32_t *k, int64_t *ns, int64_t *rows_host, double *B_host, double *Bbf_host, double *Bbb_host);
pmg_lrc    pmg_grid_lrc(pmg_grid g); /* the grid operator's low-rank update, NULL if none (borrowed) */
void       pmg_lrc_destroy(pmg_lrc *l);
/* the noise term and the repair on C chains (ld x C, chain fastest): pmg_lrc_rhs into out (b chain stride b_cs) / pmg_lrc_post per column */
pmg_status pmg_lrc_rhs_chains(pmg_lrc l, int32_t nchains, const uint64_t *keys_dev, uint64_t counter, const double *b_lay, int b_cs, double *out_lay, void *stream);
pmg_status pmg_lrc_post_chains(pmg_lrc l, int32_t nchains, int dir, double *Y_lay, void *stream);
/* the forms of the chains V-cycle: the noise term (eta_dev k x C, drawn) IN PLACE on a right-hand side the cycle owns, the repair
   that puts the entries under it back, the residual's term R -= B (S o (B^T X)); 1: one launch each for the last two */
pmg_status pmg_lrc_rhs_inplace_chains(pmg_lrc l, int32_t nchains, const double *eta_dev, double *B_lay, void *stream);
pmg_status pmg_lrc_post_restore_chains(pmg_lrc l, int32_t nchains, int dir, double *Y_lay, void *stream);
pmg_status pmg_lrc_residual_sub_chains(pmg_lrc l, int32_t nchains, const double *X_lay, double *R_lay, void *stream);
int        pmg_lrc_chains_fused(pmg_lrc l);
pmg_status pmg_mcsor_set_idiag_by_division(pmg_mcsor mc, int on); /* PCPARSOR's idiag = omega / d */
pmg_status pmg_mcsor_set_natural_order(pmg_mcsor mc, int on); /* no locality renumbering inside the colours (hierarchy levels) */
/* pmg_parsor.c: data-flow form of PCPARSOR's multi-rank sweep; the four arrays are malloc'ed, the caller frees them */
pmg_status pmg_parsor_build_dataflow(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, int32_t nparts, const int32_t *row_starts, const int32_t *proccols_in, int32_t **e_rowptr, int32_t **e_colidx, double **e_vals, int32_t **e_colors, int32_t *nlevels_out, int32_t *proccols_out, int32_t *classes_out);
int        pmg_invert_small(int k, double *a_colmajor, double *inv); /* Gauss-Jordan, partial pivoting; a is overwritten; nonzero = singular */

pmg_status pmg_narrow_csr(int64_t nrows, int64_t ncols, const void *rowptr, const void *colidx, int idx_width, const int32_t **rp, const int32_t **ci, int32_t **rp_own, int32_t **ci_own);
/* trace ranges named like the reference's PetscLogEvents (src/parmgmc.c:118-127) */
#define PMG_EVENT_MULTICOL_SOR "MulticolSOR"
#define PMG_EVENT_VEC_SET_RANDOM_NORMAL "VecSetRandN"
void pmg_trace_begin(const char *name);
void pmg_trace_end(void);
/* device allocation helpers (zero-filled) */
pmg_status pmg_dev_alloc(void **p, size_t bytes); /* zero-filled; the fill has finished on return */
pmg_status pmg_dev_zero(void *p, size_t bytes);   /* zero fill, finished on return */
pmg_status pmg_dev_upload(void **p, const void *host, size_t bytes);
void       pmg_dev_free(void *p);
/* a device buffer that grows: the workspaces whose size follows the chain count.  Zero-filled whenever (re)allocated; reserve
   with bytes <= cap makes no HIP call, a growing one synchronises `stream` first; a failed one leaves {NULL, 0} */
typedef struct {
  void  *p;
  size_t cap; /* bytes */
} pmg_devbuf;
pmg_status pmg_devbuf_reserve(pmg_devbuf *b, size_t bytes, void *stream);
void       pmg_devbuf_free(pmg_devbuf *b);

/* shared by every multi-chain entry point (pmg_chains_common.c): a device copy of C noise keys, uploaded only when they change */
typedef struct {
  pmg_devbuf dev;
  uint64_t  *host; /* the keys of the last upload; as long as dev */
  int64_t    n;
} pmg_keybuf;
pmg_status pmg_keybuf_set(pmg_keybuf *k, const uint64_t *keys, int64_t n, void *stream);
void       pmg_keybuf_free(pmg_keybuf *k);
/* ld rows of nchains chains: PMG_ERR_ARG_OUTOFRANGE when the element count or the chain count exceeds what the launches index */
pmg_status pmg_chains_size_check(int64_t ld, int32_t nchains);
/* building blocks of the chains V-cycle on layout vectors (n x C, chain fastest; bcs = chain stride of b: 0 shared, 1 per chain) */
pmg_status pmg_mcsor_sweeps_chains(pmg_mcsor mc, int32_t nchains, const uint64_t *keys_dev, int noisy, int scaled, int32_t its, uint64_t counter0, uint64_t *counter_out, const double *b_lay, int bcs, double *Y_lay, void *stream);
pmg_status pmg_mcsor_residual_chains(pmg_mcsor mc, int32_t nchains, const double *b_lay, int bcs, const double *Y_lay, double *R_lay, void *stream);
pmg_status pmg_mcsor_chains_supported(pmg_mcsor mc); /* PMG_ERR_SUP for what the chains kernels do not carry */
pmg_lrc    pmg_mcsor_lrc(pmg_mcsor mc); /* the operator's low-rank update, NULL if none (borrowed) */
/* pmg_mcsor_sweeps_chains (noisy) on an operator with a low-rank update: directional sweep i of the call takes its noise term from
   eta_dev + i * eta_stride (k x C, drawn) onto B_lay (ld x C, the caller's own: written and put back) and is followed by the repair */
pmg_status pmg_mcsor_sweeps_lowrank_chains(pmg_mcsor mc, int32_t nchains, const uint64_t *keys_dev, int scaled, int32_t its, uint64_t counter0, uint64_t *counter_out, const double *eta_dev, int64_t eta_stride, double *B_lay, double *Y_lay, void *stream);
const int32_t *pmg_mcsor_orig_dev(pmg_mcsor mc);      /* layout -> natural row map on the device (-1 in pad rows) */
/* pmg_chol.c: the exact sample y = L^-T (L^-1 b + xi) on C right-hand sides; Xi, V: n x C work arrays */
pmg_status pmg_chol_sample_chains(pmg_chol ch, int32_t nchains, const uint64_t *keys_dev, uint64_t counter, const double *B, double *Y, double *Xi, double *V, void *stream);
/* the handle's size and its (L^-1)^T: device, n x n row-major, zero below the diagonal (borrowed) */
int32_t       pmg_chol_size(pmg_chol ch);
const double *pmg_chol_inverse_factor_upper(pmg_chol ch);

/* pmg_chainstats.c: steps [first, first + count) of QOI q of the trace on the device, count x nchains, chain fastest (borrowed) */
pmg_status pmg_chainstats_trace_window(pmg_chainstats cs, int32_t q, int32_t first, int32_t count, const double **X_dev, int32_t *nchains);

/* pmg_rowblock.c */
void pmg_mcsor_adopt_arrays(pmg_mcsor mc, int32_t *rowptr, int32_t *colidx, double *vals);

/* pmg_blockgibbs_host.c: everything pmg_blockgibbs_setup does on the host -- block extraction, the conflict graph and its
   colouring, W_p = L_p^-1 of every block, the interior / exterior split of every block row, the packing into wavefront tiles
   (kernels_blockgibbs.hip).  Host arrays only, freed by pmg_bg_plan_free.
   A tile is one wavefront: 64 / g blocks of padded width g, lane (q, i) = q * g + i owns local row i of its q-th block. */
#define PMG_BG_MAX_BLOCK 64
typedef struct {
  int32_t  n, ld, nblocks, nslots, ncolors, ntiles;
  int32_t *colors;    /* [nblocks] */
  int32_t *ctile;     /* [ncolors + 1] first tile of every colour */
  int32_t *tile_g;    /* [ntiles] padded block width: 8, 16, 32 or 64 */
  int32_t *tile_ew;   /* [ntiles] exterior entries per lane (the widest row of the tile) */
  int64_t *tile_foff; /* [ntiles + 1] first factor entry, g * 64 per tile: entry j of lane l at foff + j * 64 + l */
  int64_t *tile_eoff; /* [ntiles + 1] first exterior entry, ew * 64 per tile, laid out the same way */
  int32_t *pos;       /* [ntiles * 64] vector position of the lane's row, -1 in lanes without a row */
  int32_t *slot;      /* [ntiles * 64] the lane's slot blockptr[p] + i (0 in lanes without a row) */
  double  *M, *WT;    /* [tile_foff[ntiles]] rows of W^T W and of W^T, zero outside the block */
  double  *evals;     /* [tile_eoff[ntiles]] exterior entries in the row's storage order, then pad entries of value 0 */
  int32_t *ecols;     /* their vector positions (pad entries: a valid position) */
  int64_t *woff;      /* [nblocks + 1] block p's W at W + woff[p], row-major m x m */
  double  *W, *L;     /* L (same layout) is what the factorisation left: kept for the host tests */
  int32_t *slot_nint, *slot_next; /* [nslots] stored entries of the slot's row inside / outside its block */
  int32_t *slot_tile_lane;        /* [nslots] tile * 64 + lane of the slot */
  int64_t  nnz_ext;
} pmg_bg_plan;
/* user_colors NULL: first-fit over the blocks in block order.  pos_of_row NULL: position = row, ld = n. */
pmg_status pmg_bg_plan_build(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, int32_t nblocks, const int32_t *blockptr, const int32_t *blockrows, int32_t user_ncolors, const int32_t *user_colors, int32_t ld, const int32_t *pos_of_row, pmg_bg_plan *out);
void       pmg_bg_plan_free(pmg_bg_plan *pl);
/* the argument checks of pmg_blockgibbs_create_csr */
pmg_status pmg_bg_check_blocks(int32_t n, int32_t nblocks, const int32_t *blockptr, const int32_t *blockrows);
/* pmg_blockgibbs.c: one directional sweep over all block colours of a handle that is set up; mode as pmgk_blockgibbs_color_sweep */
pmg_status pmg_blockgibbs_dir_sweep(pmg_blockgibbs bg, int dir, int mode, uint64_t seed, uint64_t sweep, const double *xi_slots, const double *b, double *y, void *stream);
/* the same on C chains: vectors in the handle's layout, len x C, chain fastest; keys on the device (mode 1), Xi nslots x C (mode 2),
   bcs = chain stride of b (0: one shared vector, 1: len x C).  What a chains V-cycle would call on a block level. */
pmg_status pmg_blockgibbs_dir_sweep_chains(pmg_blockgibbs bg, int dir, int mode, int32_t C, const uint64_t *keys_dev, uint64_t sweep, const double *Xi, const double *b, int bcs, double *Y, void *stream);

#endif
