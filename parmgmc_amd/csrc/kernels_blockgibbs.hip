// Coloured block Gibbs sweep (gfx950): one launch updates every block of one block colour,
//
//   y_P <- A_PP^-1 (b_P - A_{P,rest} y_rest) + L_P^-T xi_P,    A_PP = L_P L_P^T,
//
// the patch update PCASM's multiplicative loop composes from a one-iteration Richardson around the dense Cholesky sampler
// (reference examples/ex13.py:11-22; src/pc_chols.c:174-194 factor, :220-260 the two triangular solves and the noise,
// :284-287 the Richardson wrapper), and with xi = 0 one step of multiplicative Schwarz.
//
// A wavefront is a tile of 64 / G blocks of padded width G in {8, 16, 32, 64} (pmg_blockgibbs_host.c packs them): lane
// (q, i) = q * G + i owns local row i of the tile's q-th block, so a 5-row star patch takes 8 lanes, not 64.  Per lane:
//   1. r_i = b[p_i] - sum a_k y[col_k] over the row's stored entries OUTSIDE the block, in storage order (sell_row_sum on the
//      tile's column-major exterior entries; columns are vector positions, so a layout costs nothing here);
//   2. r (and xi) go through the wavefront's LDS line, 64 doubles each;
//   3. y_i = sum_j M_ij r_j (+ sum_j (W^T)_ij xi_j), M = W^T W, W = L^-1: every lane forms its own row serially in j = 0 .. G-1
//      from zero -- no cross-lane reduction, so the result can be restated bit for bit -- reading M and W^T column-major from
//      the tile (entry j of lane l at foff + j * 64 + l: coalesced), zero outside the block.
// Lanes without a row (pad rows of a block, pad blocks of a tile) run every step with r = xi = 0 and are masked at the store
// only.  Rows in no block are never written.  The blocks of one colour share no row and no stored coupling, so the launch
// has no race.
#include <hip/hip_runtime.h>
#include "pmg_kernels.h"
#define PMG_RNG_LITERALS // as kernels_csr.hip: no scalar loads in the middle of the row sum
#define PMG_RNG_TU blockgibbs
#include "pmg_rng.hpp"
#include "pmg_sell_row.hpp"

namespace {

enum { BG_DET = 0, BG_DRAW = 1, BG_XI = 2 }; // no noise; normals drawn in registers; normals read from xi_slots (diagnostic)

// acc_i = sum_j F[j * 64 + lane] * x[j], j ascending from zero, x the block's line in LDS
__device__ __forceinline__ double block_row(int g, const double *__restrict__ F, const double *x)
{
  double acc = 0.0;
  for (int j0 = 0; j0 < g; j0 += 8) { // g is a multiple of 8: the eight loads of a batch are issued together
    double f[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) f[q] = F[(int64_t)(j0 + q) * 64];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc = acc + f[q] * x[j0 + q];
  }
  return acc;
}

template <int MODE>
__global__ __launch_bounds__(256) void blockgibbs_color_kernel(pmgk_blockgibbs B, int tile0, int ntiles, uint32_t key0, uint32_t key1, uint64_t sweep, const double *__restrict__ xi_slots, const double *__restrict__ b, double *y)
{
  __shared__ pmg::LogTabEntry s_logtab[MODE == BG_DRAW ? 4 * PMG_LOGTAB_SIZE : 1];
  __shared__ double           s_line[4][2][64];
  const int                   lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int                   tl   = blockIdx.x * (blockDim.x >> 6) + wv;
  if (tl >= ntiles) return; // the whole wavefront: every exchange below stays inside one wavefront
  if (MODE == BG_DRAW) pmg::load_log_table_wave(s_logtab + wv * PMG_LOGTAB_SIZE, lane);
  const int     t    = tile0 + tl;
  const int     g    = __builtin_amdgcn_readfirstlane(B.tile_g[t]);
  const int     ew   = __builtin_amdgcn_readfirstlane(B.tile_ew[t]);
  const int64_t foff = B.tile_foff[t], eoff = B.tile_eoff[t];
  const int     pos  = B.pos[(int64_t)t * 64 + lane];
  const bool    live = pos >= 0;
  double        sum  = live ? b[pos] : 0.0;
  double        xi   = 0.0;
  if (MODE != BG_DET) {
    const uint32_t s = (uint32_t)B.slot[(int64_t)t * 64 + lane]; // slot stream: element s of the row stream (kernels_csr.hip:67-72)
    if (MODE == BG_DRAW) {
      double z0, z1;
      pmg::normal_pair(s >> 1, 0u, (uint32_t)sweep, (uint32_t)(sweep >> 32), key0, key1, s_logtab + wv * PMG_LOGTAB_SIZE, z0, z1);
      xi = (s & 1u) ? z1 : z0;
    } else xi = xi_slots[s];
    if (!live) xi = 0.0;
  }
  sum = sell_row_sum(sum, ew, B.evals + eoff + lane, B.ecols + eoff + lane, y);
  if (!live) sum = 0.0; // whatever a pad entry read: the factor's zero columns must meet a finite value
  double *line_r = s_line[wv][0], *line_x = s_line[wv][1];
  line_r[lane] = sum;
  if (MODE != BG_DET) line_x[lane] = xi;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int base = lane & ~(g - 1); // first lane of my block
  double    out  = block_row(g, B.M + foff + lane, line_r + base);
  if (MODE != BG_DET) out = out + block_row(g, B.WT + foff + lane, line_x + base);
  if (live) y[pos] = out;
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : 1; }

} // namespace

// mode 0: xi = 0 (pmg_blockgibbs_apply); 1: the slot stream of (seed, sweep); 2: xi_slots[slot] (pmg_blockgibbs_sweep_xi)
extern "C" int pmgk_blockgibbs_color_sweep(const pmgk_blockgibbs *B, int tile0, int ntiles, int mode, uint64_t seed, uint64_t sweep, const double *xi_slots, const double *b, double *y, void *stream)
{
  if (ntiles <= 0) return 0;
  if (mode == BG_XI && !xi_slots) return 1;
  const dim3 block(256), grid((ntiles + 3) / 4);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  if (mode == BG_DET) hipLaunchKernelGGL((blockgibbs_color_kernel<BG_DET>), grid, block, 0, (hipStream_t)stream, *B, tile0, ntiles, k0, k1, sweep, xi_slots, b, y);
  else if (mode == BG_DRAW) hipLaunchKernelGGL((blockgibbs_color_kernel<BG_DRAW>), grid, block, 0, (hipStream_t)stream, *B, tile0, ntiles, k0, k1, sweep, xi_slots, b, y);
  else if (mode == BG_XI) hipLaunchKernelGGL((blockgibbs_color_kernel<BG_XI>), grid, block, 0, (hipStream_t)stream, *B, tile0, ntiles, k0, k1, sweep, xi_slots, b, y);
  else return 1;
  return launch_status();
}
