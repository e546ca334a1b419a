// Low-rank (Woodbury) pieces of kernels_lrc.hip on MANY CHAINS per launch (gfx950): the repair y -= Bb (B^T y) of the
// sampler on A + B S B^T, its noise term B (sqrt(S) o eta), and the products of PCWOODBURY, each for C chains of one operator.
//
// Layout: multi-chain vectors are n x C doubles, chain fastest (kernels_chains.hip), and so are the k-vectors of the chains
// (k x C, element (column j, chain c) at j * C + c).  Lanes run along the chains of a row: B, Bb, G and the row positions are
// one broadcast load per row, Y[row * C + c] one contiguous segment.
//
// Bit identity: every (column, chain) pair adds its terms in the order of the single-chain kernel, so column c of a result
// equals the single-chain call on that column.
//   B^T y: blocks of 256 * R rows (R = 16 dense, PMG_LRC_RPT compact); slot t < 256 runs an fma chain from 0.0 over the rows
//          t, t + 256, ... of its block; a wavefront's 64 slots are combined by the shuffle-down tree (offsets 32 ... 1), the
//          four wavefronts as (w0 + w1) + (w2 + w3).  Here a lane owns one chain, so a wavefront covers 64 / lpr slots at a
//          time (lpr = lanes per chain group): the tree is rebuilt exactly -- its node of offset o over slot i is the sum of
//          the nodes (i, 2o) and (i + o, 2o), and the leaves taken in bit-reversed order make every node a contiguous run of
//          leaves.  A lane group sums one run in registers, the groups are combined by shuffles over whole groups.
//   block sums (lrc_reduce_kernel): virtual lane l adds blocks l, l + 64, ... from 0.0, then the same tree, then the scale.
//   updates (lrc_axpy_cols_kernel, lrc_axpy_rows_kernel): fma chain over the columns from 0.0, out = in + sign * s.
//   noise (fill_normal_rows_kernel<true>): pair q of the row stream (key, sweep) gives entries 2q and 2q + 1, times sqrt(S).
//
// The V-cycle of the chains (pmg_mgmc_chains.c) runs these in fewer launches, same sums:
//   lrc_noise_batch_chains_kernel  every noise term of one cycle (level, draw, column, chain) from the cycle's key table;
//   lrc_axpy_chains_kernel         with save_out the noise term goes onto a right-hand side IN PLACE and the old entries are
//                                  kept (nr x C); with restore they go back in the repair's update pass over the same rows;
//   lrc_small_chains_kernel        a support of one block of rows: B^T y, its (one-block) reduction with the scale and the
//                                  update that consumes it by ONE workgroup per chunk of 64 chains, the k x 64 sums in LDS.
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"
#define PMG_RNG_LITERALS // as in kernels_lrc.hip
#define PMG_RNG_TU lrc_chains
#include "pmg_rng.hpp"

namespace {

constexpr int KB = 4; // columns of B^T y formed per pass over a block's rows of Y

inline int lpr_log2_of(int32_t C)
{
  int l = 0;
  while (l < 6 && (1 << l) < C) ++l;
  return l;
}
inline unsigned chunks_of(int32_t C) { return (unsigned)((C + 63) / 64); }

__device__ __forceinline__ int bitrev6(int m) { return (int)(__builtin_bitreverse32((uint32_t)m) >> 26); }

// The node of the 64-leaf shuffle-down tree over the leaves m0 .. m0 + L - 1 (leaf m = slot bitrev6(m)); leaf(slot, v)
// writes the KB slot values.  Left + right, as s_i + s_{i+off}.
template <int L, class Leaf>
__device__ __forceinline__ void tree_node(int m0, const Leaf &leaf, double (&v)[KB])
{
  if constexpr (L == 1) leaf(bitrev6(m0), v);
  else {
    double r[KB];
    tree_node<L / 2>(m0, leaf, v);
    tree_node<L / 2>(m0 + L / 2, leaf, r);
#pragma unroll
    for (int j = 0; j < KB; ++j) v[j] = v[j] + r[j];
  }
}

struct kvals {
  double v[KB];
};

// one slot of a block of B^T y for chain c: the fma chains over the rows q0 + slot + 256 i, i < R, q < n, of the columns j0 ..
// j0 + KB - 1 (< k).  Not inlined: the tree calls it up to 64 times per lane, and unrolled copies made the build take minutes.
template <int R, bool ROWS>
__device__ __noinline__ kvals btx_slot(int slot, int64_t q0, int64_t n, const int64_t *__restrict__ rows, int k, int j0, const double *__restrict__ M, int64_t ldm, const double *__restrict__ Y, int32_t C, int c, bool live)
{
  int64_t q[R];
  double  y[R];
  kvals   s;
#pragma unroll
  for (int i = 0; i < R; ++i) q[i] = q0 + slot + 256 * i;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int64_t row = q[i] < n ? (ROWS ? rows[q[i]] : q[i]) : -1;
    y[i]              = live && row >= 0 ? Y[row * C + c] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    s.v[j] = 0.0;
    if (j0 + j < k) {
      const double *col = M + ldm * (int64_t)(j0 + j);
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (q[i] < n) s.v[j] = fma(col[q[i]], y[i], s.v[j]);
    }
  }
  return s;
}

// The sums of block blk of B^T y for the chunk of 64 chains blockIdx.y: store(j, cc, sum) is called once per column j < k and
// chain blockIdx.y * 64 + cc < C with block blk's sum of M[q + ldm j] * Y[row(q) * C + c] over its 256 * R rows q < n, row(q) =
// rows[q] (compact form) or q (dense form).  256 threads; LPRL = log2 lanes per chain group.  Ends behind a barrier.
template <int R, bool ROWS, int LPRL, class Store>
__device__ __forceinline__ void btx_block(int64_t blk, int64_t n, const int64_t *__restrict__ rows, int k, const double *__restrict__ M, int64_t ldm, const double *__restrict__ Y, int32_t C, double (&red)[4][KB][64], const Store &store)
{
  constexpr int LPR = 1 << LPRL, G = 64 / LPR; // lanes per group, groups per wavefront; a group sums LPR leaves
  const int     lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> LPRL, cl = lane & (LPR - 1);
  const int     c    = blockIdx.y * 64 + cl;
  const bool    live = c < C;
  const int64_t q0   = blk * (256 * R) + 64 * wv;
  for (int j0 = 0; j0 < k; j0 += KB) {
    auto leaf = [&](int slot, double (&s)[KB]) {
      const kvals r = btx_slot<R, ROWS>(slot, q0, n, rows, k, j0, M, ldm, Y, C, c, live);
#pragma unroll
      for (int j = 0; j < KB; ++j) s[j] = r.v[j];
    };
    double v[KB];
    tree_node<LPR>(g * LPR, leaf, v);
#pragma unroll
    for (int d = 1; d < G; d <<= 1)
#pragma unroll
      for (int j = 0; j < KB; ++j) v[j] = v[j] + __shfl_down(v[j], d * LPR, 64);
    if (g == 0)
#pragma unroll
      for (int j = 0; j < KB; ++j) red[wv][j][cl] = v[j];
    __syncthreads();
    if (threadIdx.x < KB * LPR) {
      const int j = threadIdx.x >> LPRL, cc = threadIdx.x & (LPR - 1);
      if (j0 + j < k && (int)blockIdx.y * 64 + cc < C) store(j0 + j, cc, (red[0][j][cc] + red[1][j][cc]) + (red[2][j][cc] + red[3][j][cc]));
    }
    __syncthreads();
  }
}

// partial[((blk * k) + j) * C + c] = block blk's sum (btx_block).  Block (blockIdx.x, blockIdx.y = chunk of 64 chains)
template <int R, bool ROWS, int LPRL>
__global__ __launch_bounds__(256) void lrc_btx_chains_kernel(int64_t n, const int64_t *__restrict__ rows, int k, const double *__restrict__ M, int64_t ldm, const double *__restrict__ Y, int32_t C, double *__restrict__ partial)
{
  __shared__ double red[4][KB][64];
  btx_block<R, ROWS, LPRL>((int64_t)blockIdx.x, n, rows, k, M, ldm, Y, C, red, [&](int j, int cc, double v) { partial[((int64_t)blockIdx.x * k + j) * C + blockIdx.y * 64 + cc] = v; });
}

// One workgroup per chunk of 64 chains on a support of ONE block of rows (ns <= 256 * 4): w = scale o (Mc^T Y) as
// lrc_btx_chains_kernel + lrc_reduce_chains_kernel form it from a single block sum p (0.0 + p: the virtual lane's chain, the
// other leaves of the tree add + 0.0, which changes nothing any more; then the scale), kept in LDS, and out[rows[q] * C + c] +=
// sign * sum_j M2[q + ns j] w[j][c] as lrc_axpy_chains_kernel (in = out).  out may be Y: every read of Y is in front of the
// barriers, and a chunk touches its own chains only.  restore: rdst[rows[q] * C + c] = restore[q * C + c] in the same pass.
template <int LPRL>
__global__ __launch_bounds__(256) void lrc_small_chains_kernel(int64_t ns, const int64_t *__restrict__ rows, int k, const double *__restrict__ Mc, const double *Y, int32_t C, const double *__restrict__ scale, const double *__restrict__ M2, double sign, double *out, const double *__restrict__ restore, double *rdst)
{
  constexpr int LPR = 1 << LPRL;
  __shared__ double red[4][KB][64];
  __shared__ double w[64][64]; // [column][chain of the chunk]
  btx_block<4, true, LPRL>(0, ns, rows, k, Mc, ns, Y, C, red, [&](int j, int cc, double p) {
    const double a = 0.0 + p;
    w[j][cc]       = scale ? scale[j] * a : a;
  });
  const int cc = threadIdx.x & (LPR - 1), c = blockIdx.y * 64 + cc;
  if (c >= C) return;
  for (int64_t q = threadIdx.x >> LPRL; q < ns; q += 256 >> LPRL) {
    double s = 0.0;
    for (int j = 0; j < k; ++j) s = fma(M2[q + ns * j], w[j][cc], s);
    const int64_t o = rows[q] * C + c;
    out[o]          = out[o] + sign * s;
    if (restore) rdst[o] = restore[q * C + c];
  }
}

// out[j * C + c] = scale[j] * (sum of the nb block sums of column j, chain c) in lrc_reduce_kernel's order; one thread per (j, c)
__global__ __launch_bounds__(256) void lrc_reduce_chains_kernel(int nb, int k, int32_t C, const double *__restrict__ partial, const double *__restrict__ scale, double *__restrict__ out)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)k * C) return;
  const int j = (int)(t / C), c = (int)(t % C);
  auto leaf = [&](int l, double (&s)[KB]) {
    double a = 0.0;
    for (int b = l; b < nb; b += 64) a += partial[((int64_t)b * k + j) * C + c];
    s[0] = a;
#pragma unroll
    for (int i = 1; i < KB; ++i) s[i] = 0.0;
  };
  double v[KB];
  tree_node<64>(0, leaf, v);
  out[t] = scale ? scale[j] * v[0] : v[0];
}

// out[row(q) * C + c] = in[row(q) (* C + c)] + sign * sum_j M[q + ldm j] coef[j * C + c], q < nr; row(q) = rows[q] or q.
// in may be out (the repair); in_cs = 0: one vector shared by the chains.  save_out != NULL: save_out[q * C + c] = the value of
// in that was read (the noise term in place); restore != NULL: rdst[row(q) * C + c] = restore[q * C + c] (it goes back).
template <bool ROWS>
__global__ __launch_bounds__(256) void lrc_axpy_chains_kernel(int64_t nr, const int64_t *__restrict__ rows, int k, const double *__restrict__ M, int64_t ldm, const double *__restrict__ coef, double sign, const double *in, int in_cs, double *out, int lpr_log2, int32_t C, double *__restrict__ save_out, const double *__restrict__ restore, double *rdst)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = t >> lpr_log2;
  const int     c = blockIdx.y * 64 + (int)(t & ((1 << lpr_log2) - 1));
  if (q >= nr || c >= C) return;
  const int64_t r = ROWS ? rows[q] : q;
  double        s = 0.0;
  for (int j = 0; j < k; ++j) s = fma(M[q + ldm * j], coef[(int64_t)j * C + c], s);
  const int64_t o = r * C + c;
  const double  v = in[in_cs ? o : r];
  if (save_out) save_out[q * C + c] = v;
  out[o] = v + sign * s;
  if (restore) rdst[o] = restore[q * C + c];
}

// eta[j * C + c] = entry j of the row stream (keys[c] + tag, sweep) times sqrtS[j], j < k
__global__ __launch_bounds__(256) void lrc_noise_chains_kernel(int k, int lpr_log2, int32_t C, const uint64_t *__restrict__ keys, uint64_t tag, uint64_t sweep, const double *__restrict__ sqrtS, double *__restrict__ eta)
{
  __shared__ pmg::LogTabEntry s_logtab[PMG_LOGTAB_SIZE];
  pmg::load_log_table(s_logtab);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = t >> lpr_log2;
  const int     c = blockIdx.y * 64 + (int)(t & ((1 << lpr_log2) - 1));
  if (2 * q >= k || c >= C) return;
  const uint64_t key = keys[c] + tag;
  double         z0, z1;
  pmg::normal_pair((uint32_t)q, 0u, (uint32_t)sweep, (uint32_t)(sweep >> 32), (uint32_t)key, (uint32_t)(key >> 32), s_logtab, z0, z1);
  eta[2 * q * C + c] = z0 * sqrtS[2 * q];
  if (2 * q + 1 < k) eta[(2 * q + 1) * C + c] = z1 * sqrtS[2 * q + 1];
}

// The noise terms of one cycle: slot s = plan.first[i] + d is draw d of entry i (a level with an update), eta[(s * k + j) * C + c]
// = entry j of the row stream (keys[plan.level[i] * C + c] + tag, plan.ctr0[i] + d) times sqrtS[j]: lrc_noise_chains_kernel's
// numbers for that level's keys and that counter.  blockIdx.z = slot.
__global__ __launch_bounds__(256) void lrc_noise_batch_chains_kernel(int k, int lpr_log2, int32_t C, const uint64_t *__restrict__ keys, uint64_t tag, pmgk_lrc_noise_plan plan, const double *__restrict__ sqrtS, double *__restrict__ eta)
{
  __shared__ pmg::LogTabEntry s_logtab[PMG_LOGTAB_SIZE];
  pmg::load_log_table(s_logtab);
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = t >> lpr_log2;
  const int     c = blockIdx.y * 64 + (int)(t & ((1 << lpr_log2) - 1)), slot = blockIdx.z;
  if (2 * q >= k || c >= C) return;
  int i = 0;
  while (i + 1 < plan.n && plan.first[i + 1] <= slot) ++i;
  const uint64_t key = keys[(int64_t)plan.level[i] * C + c] + tag, sweep = plan.ctr0[i] + (uint64_t)(slot - plan.first[i]);
  double         z0, z1;
  pmg::normal_pair((uint32_t)q, 0u, (uint32_t)sweep, (uint32_t)(sweep >> 32), (uint32_t)key, (uint32_t)(key >> 32), s_logtab, z0, z1);
  double *e          = eta + (int64_t)slot * k * C;
  e[2 * q * C + c] = z0 * sqrtS[2 * q];
  if (2 * q + 1 < k) e[(2 * q + 1) * C + c] = z1 * sqrtS[2 * q + 1];
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : 1; }

template <int R, bool ROWS>
void launch_btx(dim3 grid, int lprl, hipStream_t st, int64_t n, const int64_t *rows, int k, const double *M, int64_t ldm, const double *Y, int32_t C, double *partial)
{
  switch (lprl) {
  case 0: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 0>), grid, dim3(256), 0, st, n, rows, k, M, ldm, Y, C, partial); break;
  case 1: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 1>), grid, dim3(256), 0, st, n, rows, k, M, ldm, Y, C, partial); break;
  case 2: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 2>), grid, dim3(256), 0, st, n, rows, k, M, ldm, Y, C, partial); break;
  case 3: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 3>), grid, dim3(256), 0, st, n, rows, k, M, ldm, Y, C, partial); break;
  case 4: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 4>), grid, dim3(256), 0, st, n, rows, k, M, ldm, Y, C, partial); break;
  case 5: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 5>), grid, dim3(256), 0, st, n, rows, k, M, ldm, Y, C, partial); break;
  default: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 6>), grid, dim3(256), 0, st, n, rows, k, M, ldm, Y, C, partial); break;
  }
}

} // namespace

/* blocks of the chains B^T y: those of pmgk_lrc_btx (rows == NULL, n rows) or pmgk_lrc_btx_rows (n support rows) */
extern "C" int pmgk_lrc_btx_chains_nblocks(int64_t n, int compact) { return compact ? pmgk_lrc_rows_nblocks(n) : pmgk_lrc_nblocks(n); }

/* out (k x C) = scale o (M^T Y) per chain, through partial (nblocks * k * C doubles); rows != NULL: the compact form (M is
   n x k over the support rows, Y indexed at rows[q]) */
extern "C" int pmgk_lrc_btx_chains(int64_t n, const int64_t *rows, int k, const double *M, int64_t ldm, const double *Y, int32_t nchains, double *partial, const double *scale, double *out, void *stream)
{
  if (n <= 0 || k <= 0 || nchains <= 0) return 0;
  if (k > 64 || (rows && pmgk_lrc_rows_per_block() != 256 * 4)) return 1;
  const hipStream_t st   = (hipStream_t)stream;
  const int         nb   = pmgk_lrc_btx_chains_nblocks(n, rows != NULL);
  const dim3        grid = dim3((unsigned)nb, chunks_of(nchains));
  const int         lprl = lpr_log2_of(nchains);
  if (rows) launch_btx<4, true>(grid, lprl, st, n, rows, k, M, ldm, Y, nchains, partial);
  else launch_btx<16, false>(grid, lprl, st, n, rows, k, M, ldm, Y, nchains, partial);
  const int64_t nt = (int64_t)k * nchains;
  hipLaunchKernelGGL(lrc_reduce_chains_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, nb, k, nchains, partial, scale, out);
  return launch_status();
}

/* pmgk_lrc_axpy_chains that also keeps what it read (save_out, nr x C) and / or puts saved entries back (rdst at the rows = restore) */
extern "C" int pmgk_lrc_axpy_save_chains(int64_t nr, const int64_t *rows, int k, const double *M, int64_t ldm, const double *coef, double sign, const double *in, int in_cs, double *out, int32_t nchains, double *save_out, const double *restore, double *rdst, void *stream)
{
  if (nr <= 0 || nchains <= 0) return 0;
  const int  lprl = lpr_log2_of(nchains);
  const dim3 grid((unsigned)((nr * (1 << lprl) + 255) / 256), chunks_of(nchains));
  if (rows) hipLaunchKernelGGL((lrc_axpy_chains_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, nr, rows, k, M, ldm, coef, sign, in, in_cs, out, lprl, nchains, save_out, restore, rdst);
  else hipLaunchKernelGGL((lrc_axpy_chains_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, nr, rows, k, M, ldm, coef, sign, in, in_cs, out, lprl, nchains, save_out, restore, rdst);
  return launch_status();
}

extern "C" int pmgk_lrc_axpy_chains(int64_t nr, const int64_t *rows, int k, const double *M, int64_t ldm, const double *coef, double sign, const double *in, int in_cs, double *out, int32_t nchains, void *stream)
{
  return pmgk_lrc_axpy_save_chains(nr, rows, k, M, ldm, coef, sign, in, in_cs, out, nchains, NULL, NULL, NULL, stream);
}

/* one launch for out[rows] += sign * M2 (scale o (Mc^T Y)) per chain on a support of one block of rows (ns <= pmgk_lrc_rows_per_block(),
   Mc and M2 ns x k): the bits of pmgk_lrc_btx_chains + pmgk_lrc_axpy_chains.  out may be Y; restore as pmgk_lrc_axpy_save_chains */
extern "C" int pmgk_lrc_small_chains(int64_t ns, const int64_t *rows, int k, const double *Mc, const double *Y, int32_t nchains, const double *scale, const double *M2, double sign, double *out, const double *restore, double *rdst, void *stream)
{
  if (ns <= 0 || k <= 0 || nchains <= 0) return 0;
  if (k > 64 || !rows || ns > 256 * 4 || pmgk_lrc_rows_per_block() != 256 * 4) return 1;
  const hipStream_t st = (hipStream_t)stream;
  const dim3        grid(1, chunks_of(nchains));
  switch (lpr_log2_of(nchains)) {
  case 0: hipLaunchKernelGGL((lrc_small_chains_kernel<0>), grid, dim3(256), 0, st, ns, rows, k, Mc, Y, nchains, scale, M2, sign, out, restore, rdst); break;
  case 1: hipLaunchKernelGGL((lrc_small_chains_kernel<1>), grid, dim3(256), 0, st, ns, rows, k, Mc, Y, nchains, scale, M2, sign, out, restore, rdst); break;
  case 2: hipLaunchKernelGGL((lrc_small_chains_kernel<2>), grid, dim3(256), 0, st, ns, rows, k, Mc, Y, nchains, scale, M2, sign, out, restore, rdst); break;
  case 3: hipLaunchKernelGGL((lrc_small_chains_kernel<3>), grid, dim3(256), 0, st, ns, rows, k, Mc, Y, nchains, scale, M2, sign, out, restore, rdst); break;
  case 4: hipLaunchKernelGGL((lrc_small_chains_kernel<4>), grid, dim3(256), 0, st, ns, rows, k, Mc, Y, nchains, scale, M2, sign, out, restore, rdst); break;
  case 5: hipLaunchKernelGGL((lrc_small_chains_kernel<5>), grid, dim3(256), 0, st, ns, rows, k, Mc, Y, nchains, scale, M2, sign, out, restore, rdst); break;
  default: hipLaunchKernelGGL((lrc_small_chains_kernel<6>), grid, dim3(256), 0, st, ns, rows, k, Mc, Y, nchains, scale, M2, sign, out, restore, rdst); break;
  }
  return launch_status();
}

/* eta (nslots x k x C) = every noise term of the plan's slots in one launch (slot s at eta + s * k * C) */
extern "C" int pmgk_lrc_noise_batch_chains(int nslots, int k, int32_t nchains, const uint64_t *keys, uint64_t tag, const pmgk_lrc_noise_plan *plan, const double *sqrtS, double *eta, void *stream)
{
  if (nslots <= 0 || k <= 0 || nchains <= 0) return 0;
  if (nslots > 65535 || plan->n < 1 || plan->n > PMGK_LRC_NOISE_PLAN_MAX) return 1;
  const int  lprl = lpr_log2_of(nchains);
  const dim3 grid((unsigned)(((int64_t)(k + 1) / 2 * (1 << lprl) + 255) / 256), chunks_of(nchains), (unsigned)nslots);
  hipLaunchKernelGGL(lrc_noise_batch_chains_kernel, grid, dim3(256), 0, (hipStream_t)stream, k, lprl, nchains, keys, tag, *plan, sqrtS, eta);
  return launch_status();
}

extern "C" int pmgk_lrc_noise_chains(int k, int32_t nchains, const uint64_t *keys, uint64_t tag, uint64_t sweep, const double *sqrtS, double *eta, void *stream)
{
  if (k <= 0 || nchains <= 0) return 0;
  const int  lprl = lpr_log2_of(nchains);
  const dim3 grid((unsigned)(((int64_t)(k + 1) / 2 * (1 << lprl) + 255) / 256), chunks_of(nchains));
  hipLaunchKernelGGL(lrc_noise_chains_kernel, grid, dim3(256), 0, (hipStream_t)stream, k, lprl, nchains, keys, tag, sweep, sqrtS, eta);
  return launch_status();
}
