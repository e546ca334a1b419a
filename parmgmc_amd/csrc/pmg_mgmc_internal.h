/* What the translation units of the MGMC sampler share (C11): the handle, its levels, the host CSR type of the set-up and
 * the few functions that cross files.
 *   pmg_hier_host.c    pure host sparse tools of the set-up (no device call: they also run under the host sanitizer program)
 *   pmg_mgmc_setup.c   handle construction, setters, the three set-up routines, getters of set-up data, destroy
 *   pmg_mgmc.c         the V-cycle, its byte model and pmg_mgmc_sample
 *   pmg_mgmc_chains.c  the multi-chain cycle
 *   pmg_mgmc_level.c   single-kernel entry points of one level (diagnostics)
 * A level has ONE kind (mg_kind: which sampler and residual it runs, who holds its low-rank update, how its vectors are laid
 * out) and ONE transfer kind (mg_transfer: how it restricts into and interpolates from the next coarser level).  The set-up
 * assigns both, once; every dispatch on them is a switch without a default, so that -Wswitch names the place a new kind
 * forgets.  What the caller hands in before set-up (mg_level_in, h->in) is apart from what the cycle reads afterwards
 * (mg_level, h->lv) and is released when the set-up has succeeded.
 * Everything declared here is internal to the library: PMG_HIDDEN keeps it out of the exported symbols. */
#ifndef PMG_MGMC_INTERNAL_H
#define PMG_MGMC_INTERNAL_H
#include "pmg_internal.h"

#define PMG_HIDDEN __attribute__((visibility("hidden")))

/* host CSR, natural numbering, columns ascending; a zeroed one is empty */
typedef struct {
  int32_t  nr, nc;
  int32_t *rp, *ci;
  double  *v;
} hcsr;

/* kind of a level          sampler (mg_smooth)                    residual (mg_residual)          low-rank update held by        vectors
   MG_LV_EXACT      pmg_chol_sample (coarsest, Cholesky)   none                            the factored sum                natural order: padded (DMDA), ld = n (caller's)
   MG_LV_GRID       pmg_grid_sample_cvec                   pmg_grid_residual_cvec          the grid object                 colour-partitioned cvec
   MG_LV_GRID_SLAB  pmg_dist_sample_cvec (built on a       pmg_grid_residual_cvec          the level (Lv->lrc): the cycle  cvec of the slab
                    pmg_dist, any rank count)                                              brackets the slab sweeps
   MG_LV_ST27       class-stencil sweeps (one device or    pmgk_st27_residual[_pair]       the level (Lv->lrc)             plane-padded natural order
                    z-slab: `distributed`)
   MG_LV_SELL       pmg_mcsor_sample_layout, or block      pmg_mcsor_residual_layout       the pmg_mcsor object            sliced-ELL layout
                    sweeps where Lv->bg
   MG_LV_ROWBLOCK   pmg_distmcsor_sample_layout            pmg_distmcsor_residual_layout   the pmg_distmcsor object        sliced-ELL layout, ghost rows last */
typedef enum { MG_LV_EXACT, MG_LV_GRID, MG_LV_GRID_SLAB, MG_LV_ST27, MG_LV_SELL, MG_LV_ROWBLOCK } mg_kind;
/* transfers between level l and l - 1, held by level l: none (level 0) | matrix-free Q1 from a grid level (cpos_dev: the coarse
   level is permuted, else padded natural) | matrix-free Q1 between two levels in padded natural order | CSR products in layout numbering */
typedef enum { MG_TR_NONE, MG_TR_Q1_GRID, MG_TR_Q1_NAT, MG_TR_CSR } mg_transfer;

typedef struct {
  mg_kind     kind;     /* assigned by the set-up bodies, */
  mg_transfer transfer; /* and by nothing after them */
  int32_t   nx, ny, nz, n; /* global extents */
  int32_t   kz0, nzl;      /* owned planes (0, nz on a single device and on replicated levels) */
  int       padded;        /* plane-padded natural layout (class-stencil levels, Cholesky level): element (i,j,k) at off + i + nx (j + ny (k - kz0)) */
  int64_t   off;           /* = nx*ny when padded */
  int       distributed;   /* z-slab level of a multi-device hierarchy */
  pmg_grid  g;
  pmg_mcsor mc;
  int64_t   ld;
  double   *b, *x, *r;
  int       x_zeroed; /* the restriction kernel has set the zero guess already */
  int       x_unset; /* the iterate is zero but the memset was skipped: the next out-of-place sweep starts from NULL */
  double   *y2lo, *y2hi; /* z-slab grid level: the iterate's planes kz0 - 2 and kz0 + nz + 1 (colour 0 plane, colour 1 plane) for the fused residual + restriction */
  int       rr_slab;     /* ... which every rank can run (agreed from the slab cuts) */
  double   *x2; /* second buffer of the out-of-place class-stencil sweep (single-device levels): x and x2 swap after every directional sweep */
  /* transfers to the next coarser level, in layout numbering on the device */
  int32_t  P_nrows, R_nrows;
  int32_t *cpos_dev; /* MG_TR_Q1_GRID onto a permuted coarse level: layout position of every point of that level (NULL: padded natural) */
  /* class-stencil form of a structured Galerkin level (natural-order vectors) */
  pmgk_st27 st;
  double   *st_coef, *st_idiag, *st_sqrtd, *st_sqrtd_scaled;
  pmg_lrc   lrc; /* MATLRC update of a class-stencil or slab grid level (mg_level_cycle_lrc); the other kinds keep theirs inside g / mc / dm */
  int32_t *P_rowpos, *P_rowptr, *P_col, *R_rowpos, *R_rowptr, *R_col;
  double  *P_val, *R_val;
  /* optional host copies (natural numbering) for inspection */
  hcsr A_host, P_host;
  int32_t       rb_nowned; /* row block: the owned rows, first among the n local rows */
  pmg_distmcsor dm;
  int64_t       A_nnz, P_nnz; /* stored entries of a sliced-ELL level's operator / of its CSR interpolation (traffic accounting) */
  pmg_blockgibbs bg; /* block smoothing of an MG_LV_SELL level (pmg_mgmc_set_level_blocks): on the level's operator, in the layout of `mc` */
} mg_level;

/* What the caller hands in for one level before set-up.  The setters write it, the set-up bodies read it, and
   pmg_mgmc_i_free_inputs empties it when a set-up has succeeded: nothing after set-up reads it. */
typedef struct {
  hcsr     A_user, P_user; /* caller-supplied hierarchy: borrowed host CSR */
  hcsr     R_user;         /* row block: rows of the restriction INTO the next coarser level that this rank owns there (borrowed) */
  int32_t *A_rp_own, *A_ci_own, *P_rp_own, *P_ci_own; /* 32-bit copies of 64-bit PetscInt arrays (owned) */
  /* ROW BLOCK of a distributed hierarchy (pmg_mgmc_set_level_rowblock sets rb): A_user is this rank's rows in
     LOCAL numbering -- owned rows first, then one identity row per ghost (every row of another rank that this rank's operator,
     restriction or the finer level's interpolation reads); copies of the plan lists, from which set-up builds `dm` */
  int      rb;
  int32_t  rb_nowned, rb_ncolors;
  int64_t  rb_row0;
  int32_t *rb_colors, *rb_send_idx, *rb_recv_src, *rb_recv_idx;
  int64_t *rb_send_ptr, *rb_recv_ptr, *rb_counts;
  /* block smoothing (pmg_mgmc_set_level_blocks): copies of the caller's blocks, from which set-up builds `bg` */
  int32_t  bg_nblocks, bg_ncolors, *bg_blockptr, *bg_blockrows, *bg_colors;
} mg_level_in;

struct pmg_mgmc_s {
  int          nlevels;
  mg_level    *lv; /* lv[0] = coarsest */
  mg_level_in *in; /* [nlevels] */
  double    kappa, omega;
  int       nu, scaled, sweep_type;
  int       coarse_type, coarse_its; /* 0 = cholsampler, 1 = Gibbs sweeps */
  int       keep_host, is_setup, user_hier;
  int       no_fused;        /* 1: residual and restriction as two kernels everywhere (pmg_mgmc_set_fused_transfers(mg, 0)) */
  int       correction_form; /* 1: w = b - A y, y += MG(w) literally (src/pc_gamgmc.c:253-256); 0: the same cycle run in place on (b, y) */
  pmg_chol  chol;
  double   *y_lay, *b_lay;
  /* MATLRC fine operator A + B S B^T (host copies until set-up; src/pc_gamgmc.c:157-196) */
  int32_t   lrc_k;
  double   *lrc_B, *lrc_S;
  int       aij_coloring; /* rule of the AIJ levels (pmg_mgmc_set_coloring); PMG_COLORING_GREEDY = 0 */
  double   *eta_batch; /* device: the low-rank noise terms of one cycle, drawn together (mg_draw_lowrank_noise) */
  int       eta_batch_mode; /* 0: not asked yet, 1: on, -1: PMG_LRC_BATCH=0 when this sampler ran its first cycle */
  int       own_grid; /* the fine grid operator was created here (not handed in with a slab) */
  /* multi-device: z-slabs of the fine grid, one rank per device (borrowed dist object); cuts[l*(nranks+1) + r] =
     first plane of rank r on level l */
  pmg_dist  dist;
  int32_t   rank, nranks;
  int32_t  *cuts;
  int32_t   n_io; /* length of the caller's fine-level vectors (the owned planes) */
  /* row-block distributed caller-supplied hierarchy: transport (borrowed) and the row blocks of the replicated coarsest level */
  pmg_dist  rb_dist;
  int64_t  *rb_c0_starts; /* row blocks of the highest REPLICATED level (rb_fold - 1): who restricts which of its rows */
  int       rb_fold;      /* lowest row-block level; the levels below are replicated on every rank */
  int32_t  *rb_fold_pos, *rb_fold_iota; /* device: layout position of natural row q of level rb_fold - 1, and 0, 1, 2, ... */
  double   *rb_fold_buf;                /* device: that level's vector in natural order (the all-gather buffer) */
  /* multi-chain workspace (pmg_mgmc_sample_chains): every buffer allocated on first use, grows with the chain count C */
  pmg_devbuf *ch_b, *ch_x, *ch_r; /* [nlevels], one host array made by the first chains call: level vectors of ld x C doubles, chain fastest */
  pmg_devbuf  ch_Y, ch_bs;        /* the chains' iterate and the shared right-hand side in the finest level's layout */
  pmg_devbuf  ch_xi, ch_v;        /* exact coarse sampler: noise and L^-1 b + xi, n_0 x C */
  pmg_keybuf  ch_keys;            /* level_seed(seeds[c], l) at l * C + c */
  pmg_devbuf  ch_B;               /* one right-hand side per chain in the finest level's layout (pmg_mgmc_sample_chains_rhs), ld x C */
  pmg_devbuf  ch_eta;             /* the low-rank noise terms of one cycle: (directional sweeps of the levels with an update) x k x C */
};

typedef struct {
  double coef[27 * 27];
  int    have[27];
} st27_table;

#define MG_DRAWS_PER_SAMPLE 64u

/* row generator: either a stored CSR or the matrix-free 7-point operator of src/problems.c:14-75 */
typedef struct {
  const hcsr *A;
  int32_t     nx, ny, nz;
  double      kappa, h2, diag[8];
} rowsrc;

/* *to takes over *from's arrays */
static inline void hcsr_move(hcsr *to, hcsr *from)
{
  *to = *from;
  memset(from, 0, sizeof *from);
}

/* per-level noise seed: levels draw from independent streams */
static inline uint64_t level_seed(uint64_t seed, int level) { return seed + 0x9E3779B97F4A7C15ull * (uint64_t)(level + 1); }

/* directional sweeps of ONE smoothing leg of level l (nu samples; coarse_its on a Gibbs coarsest level, none on an exactly sampled
   one), and of one whole cycle (pre- and post-smoothing above the coarsest level).  The batched noise draws of a cycle and the
   sweeps that later ask for them count with these two, as do the byte models */
static inline int pmg_mgmc_i_leg_sweeps(const struct pmg_mgmc_s *h, int l) { return (l >= 1 ? h->nu : (h->coarse_type != 0 ? h->coarse_its : 0)) * pmg_sweep_ndir(h->sweep_type); }
static inline int pmg_mgmc_i_level_sweeps(const struct pmg_mgmc_s *h, int l) { return (l >= 1 ? 2 : 1) * pmg_mgmc_i_leg_sweeps(h, l); }

/* some level is smoothed by block sweeps (before set-up: is asked to be) */
static inline int pmg_mgmc_i_has_blocks(const struct pmg_mgmc_s *h)
{
  for (int l = 0; l < h->nlevels; ++l)
    if (h->is_setup ? h->lv[l].bg != NULL : h->in[l].bg_blockptr != NULL) return 1;
  return 0;
}

/* owned unknowns: a z-slab's planes, a row block's rows */
static inline double level_rows(const mg_level *Lv)
{
  switch (Lv->kind) {
  case MG_LV_GRID:
  case MG_LV_GRID_SLAB:
  case MG_LV_ST27: return (double)Lv->nx * Lv->ny * Lv->nzl;
  case MG_LV_ROWBLOCK: return (double)Lv->rb_nowned;
  case MG_LV_SELL:
  case MG_LV_EXACT: break; /* (never distributed) */
  }
  return (double)Lv->n;
}

static inline pmgk_st27_dims level_dims(const mg_level *Lv) { return (pmgk_st27_dims){Lv->nx, Lv->ny, Lv->nzl, Lv->kz0, Lv->nz}; }

/* the low-rank update the level's SAMPLER applies, NULL if none */
static inline pmg_lrc mg_level_sampler_lrc(const struct pmg_mgmc_s *h, int l)
{
  const mg_level *Lv = &h->lv[l];
  switch (Lv->kind) {
  case MG_LV_GRID: return pmg_grid_lrc(Lv->g);
  case MG_LV_GRID_SLAB:
  case MG_LV_ST27: return Lv->lrc;
  case MG_LV_SELL: return pmg_mcsor_lrc(Lv->mc);
  case MG_LV_ROWBLOCK: /* the pmg_distmcsor object's, which hands none out */
  case MG_LV_EXACT: break; /* the factor is that of the explicit sum */
  }
  return NULL;
}

/* mg_path.lrc and the level diagnostics: the sampler's update where it is open to the cycle -- which hands it the batched noise,
   announces the residual and charges its passes -- and to pmg_mgmc_level_lowrank_*.  A sliced-ELL sampler applies its own inside
   its pmg_mcsor calls */
static inline pmg_lrc mg_level_path_lrc(const struct pmg_mgmc_s *h, int l) { return h->lv[l].kind == MG_LV_SELL ? NULL : mg_level_sampler_lrc(h, l); }

/* the update whose noise bracket and residual term the CYCLE applies itself: the one the level holds.  The samplers of the other
   kinds bracket their own sweeps, and their residual calls subtract the term */
static inline pmg_lrc mg_level_cycle_lrc(const struct pmg_mgmc_s *h, int l)
{
  const mg_level *Lv = &h->lv[l];
  switch (Lv->kind) {
  case MG_LV_GRID_SLAB:
  case MG_LV_ST27: return Lv->lrc;
  case MG_LV_EXACT:
  case MG_LV_GRID:
  case MG_LV_SELL:
  case MG_LV_ROWBLOCK: break;
  }
  return NULL;
}

/* ---- pmg_hier_host.c: host memory only.  A function that fails leaves its output matrix partly allocated: it stays the
   caller's to release with pmg_hcsr_free, which accepts that state. */
PMG_HIDDEN void       pmg_hcsr_free(hcsr *m);
PMG_HIDDEN pmg_status pmg_hcsr_dup(const hcsr *A, hcsr *out);
PMG_HIDDEN pmg_status pmg_hcsr_transpose(const hcsr *A, hcsr *T);
PMG_HIDDEN pmg_status pmg_hier_q1_interp(const int32_t nf[3], const int32_t nc[3], hcsr *P);
PMG_HIDDEN void       pmg_hier_laplace_rows(int32_t nx, int32_t ny, int32_t nz, double kappa, double h2, rowsrc *s);
PMG_HIDDEN pmg_status pmg_hier_galerkin_rap(const rowsrc *A, int maxrow, const hcsr *P, const hcsr *R, hcsr *Cm);
PMG_HIDDEN pmg_status pmg_hier_restrict_B(const hcsr *R, int32_t k, int32_t nf, const double *Bf, double **Bc_out);
PMG_HIDDEN int        pmg_hier_st27_extract(int nx, int ny, int nz, const hcsr *A, double *coef /* [27*27] */, int *have /* [27] */);
PMG_HIDDEN pmg_status pmg_hier_st27_to_csr(int nx, int ny, int nz, const st27_table *t, hcsr *A);
PMG_HIDDEN pmg_status pmg_hier_stencil_tables(int nlevels, const int32_t (*dims)[3] /* [nlevels], 0 = coarsest */, double kappa, double h2, st27_table *tab /* [nlevels-1] */, int *ok);
PMG_HIDDEN void       pmg_hier_parity_colouring(int32_t nx, int32_t ny, int32_t nz, int32_t *col /* [nx*ny*nz] */);

/* ---- pmg_mgmc.c: the pieces of the cycle that the set-up (low-rank blocks restricted with the cycle's own kernels) and
   the level diagnostics run too */
PMG_HIDDEN int        pmg_mgmc_i_st27_out_of_place(const mg_level *Lv); /* the level's own iterate is swept out of place, into Lv->x2 */
PMG_HIDDEN int        pmg_mgmc_i_level_wants_x2(const mg_level *Lv);    /* the set-up gives the level a second iterate buffer */
PMG_HIDDEN pmg_status pmg_mgmc_i_halo_level(pmg_mgmc h, mg_level *Lv, double *v, void *stream);
/* one directional sweep of a class-stencil level.  noisy: the cycle's, on (rhs, the level's own iterate) with draw *ctr, which it
   advances; out of place where the level has a second buffer (the two then swap).  Not noisy: in place on the caller's (rhs, y),
   the level's iterate, buffers and counter untouched (seed and ctr are not read) */
PMG_HIDDEN pmg_status pmg_mgmc_i_st27_dir_sweep(pmg_mgmc h, mg_level *Lv, int dir, int noisy, const double *rhs, double *y, uint64_t seed, uint64_t *ctr, void *stream);
PMG_HIDDEN pmg_status pmg_mgmc_i_rb_fold_allgather(pmg_mgmc h, double *v, void *stream);
PMG_HIDDEN pmg_status pmg_mgmc_i_level_residual(pmg_mgmc h, int l, const double *b, const double *x, double *r, void *stream);
PMG_HIDDEN pmg_status pmg_mgmc_i_restrict(pmg_mgmc h, int l, double *r_fine, double *b_coarse, void *stream);
PMG_HIDDEN pmg_status pmg_mgmc_i_prolong_add(pmg_mgmc h, int l, const double *e_coarse, double *x_fine, int only_color, void *stream);
/* ---- pmg_mgmc_setup.c, pmg_mgmc_chains.c, pmg_mgmc_level.c */
PMG_HIDDEN void       pmg_mgmc_i_free_inputs(pmg_mgmc h); /* releases what h->in owns and zeroes the rest */
PMG_HIDDEN void       pmg_mgmc_i_free_chains(pmg_mgmc h);
PMG_HIDDEN pmg_status pmg_mgmc_i_level_checked(pmg_mgmc h, int32_t level, int need_coarser, mg_level **Lv);

#endif
