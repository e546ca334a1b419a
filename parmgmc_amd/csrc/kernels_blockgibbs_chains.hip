// Coloured block Gibbs sweep on C chains of one operator (gfx950): one launch updates every block of one block colour in every
// chain.  The plan is the one kernels_blockgibbs.hip reads (pmgk_blockgibbs: tiles, pos, slot, M, WT, evals, ecols), the vectors
// are len x C doubles with the chain index fastest, element (position, chain) at pos * C + chain.
//
// Mapping.  A workgroup is ONE wavefront = one tile (64 / G blocks of padded width G, lane (q, i) = q * G + i owns local row i of
// the tile's q-th block, as in the single-chain kernel) times one CHUNK of CB = 8 consecutive chains, which the lane carries in
// registers.  The grid is one-dimensional, 8 * band * ny workgroups with band = ceil(ntiles / 8): workgroup id serves tile
// (id % 8) * band + (id / 8) / ny and chunk (id / 8) % ny (further chunks, beyond the launch limit only, in a loop of stride ny),
// see the comment in the kernel.  What does not depend on the chain -- pos, slot, every exterior (a_k, col_k), every factor
// entry M[j][lane] / WT[j][lane] -- is loaded once per chunk and applied to CB accumulators; every exterior gather, the
// right-hand side of the per-chain form, the injected normals and the store are CB contiguous doubles at idx * C + c0.  A
// further chunk reads the factors again, 4 KiB per factor and tile of 5-point stars, from the L2 its neighbour chunk has filled.
//
// Bit identity.  Per (slot, chain) the operations of blockgibbs_color_kernel in its order: r starts from b; the exterior entries
// are subtracted in storage order, sum - a_k * y, pad entries included; out = sum_j M_ij r_j from zero over j ascending, products
// and sums rounded separately (-ffp-contract=off); the same sum over (W^T)_ij xi_j is added as one further addition; xi is
// element s & 1 of normal_pair(s >> 1, 0, sweep_lo, sweep_hi, key_lo, key_hi) with key = keys[chain].  Every lane forms its own
// row serially: no cross-lane reduction.  That also rules out the f64 MFMA for the row product: it fuses the multiply and the add.
//
// LDS.  r and xi of a chunk pass through two lines of CB x 64 doubles, CHAIN-major: element (chain c, lane l) at c * 64 + l --
// 4 KiB each, 8 KiB per workgroup (+ 1 KiB log table when normals are drawn).  A lane writes line[c][lane]: 64 consecutive
// doubles per instruction, no bank conflict.  In the row product every lane of a block reads the same line[c][base + j] (a
// broadcast) and the 64 / G blocks of a tile read addresses G * 8 bytes apart, >= 64 bytes, all inside one 512-byte row of the
// line: 8 distinct 8-byte words on 8 distinct bank pairs for G = 8.  No conflict for any G, without padding (a lane-major line
// [lane][c] would put the blocks G * CB * 8 bytes apart, a multiple of the 256-byte bank row: 64 / G-way).
//
// Access width.  With C even and all vectors 16-byte aligned (VEC) a row's chunk is loaded and stored as four 16-byte accesses,
// each aligned because idx * C + c0 is even; otherwise rows are only 8-byte aligned and every access is a plain 8-byte one.
// Tail chunk.  nc = min(CB, C - c0) is uniform over the workgroup; every load and store of column c is under c < nc (for VEC,
// nc is even and pairs are whole): nothing is read or written past column C - 1.  Unused columns compute on zeros.
// Synchronisation.  The only early exit is a whole wavefront (= workgroup) past the colour's last tile, before any LDS access;
// there is no lane-divergent control flow around the LDS exchange, which stays inside the wavefront (fence + wave barrier, as in
// the single-chain kernel; once more at the end of a chunk, before the next one overwrites the lines).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "pmg_kernels.h"
#define PMG_RNG_LITERALS // as kernels_csr.hip
#define PMG_RNG_TU blockgibbs_chains
#include "pmg_rng.hpp"

namespace {

enum { BG_DET = 0, BG_DRAW = 1, BG_XI = 2 }; // as kernels_blockgibbs.hip
constexpr int CB = 8;                        // chains per chunk
constexpr int IB = 8;                        // exterior entries whose values and columns are loaded together (SELL_BATCH of the single-chain kernel)
constexpr int EB = 4;                        // exterior entries whose gathers are in flight together (EB * CB doubles per lane)

// entries j0 .. j0 + IB - 1 of the lane's exterior row (ew >= 1); past the tile's width the last entry again (a valid address, not used)
__device__ __forceinline__ void load_entries(double (&a)[IB], int32_t (&cj)[IB], const double *__restrict__ ev, const int32_t *__restrict__ ec, int j0, int ew)
{
#pragma unroll
  for (int q = 0; q < IB; ++q) {
    const int64_t jj = (int64_t)min(j0 + q, ew - 1) * 64;
    a[q]             = ev[jj];
    cj[q]            = ec[jj];
  }
}

// v[c] = p[c] for c < nc, 0 beyond
template <bool VEC>
__device__ __forceinline__ void load_chunk(double (&v)[CB], const double *p, int nc)
{
  if (VEC) {
#pragma unroll
    for (int c = 0; c < CB; c += 2) {
      double2 t = make_double2(0.0, 0.0);
      if (c < nc) t = *reinterpret_cast<const double2 *>(p + c);
      v[c]     = t.x;
      v[c + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < CB; ++c) v[c] = c < nc ? p[c] : 0.0;
  }
}

template <bool VEC>
__device__ __forceinline__ void store_chunk(double *p, const double (&v)[CB], int nc)
{
  if (VEC) {
#pragma unroll
    for (int c = 0; c < CB; c += 2)
      if (c < nc) *reinterpret_cast<double2 *>(p + c) = make_double2(v[c], v[c + 1]);
  } else {
#pragma unroll
    for (int c = 0; c < CB; ++c)
      if (c < nc) p[c] = v[c];
  }
}

// acc[c] = sum_j F[j * 64 + lane] * x[c][j], j ascending from zero (block_row of the single-chain kernel per chain); x = the
// block's first element of the chain-major line
__device__ __forceinline__ void block_row_chains(double (&acc)[CB], int g, const double *__restrict__ F, const double *x)
{
#pragma unroll
  for (int c = 0; c < CB; ++c) acc[c] = 0.0;
  for (int j0 = 0; j0 < g; j0 += 8) { // g is a multiple of 8
    double f[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) f[q] = F[(int64_t)(j0 + q) * 64];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int c = 0; c < CB; ++c) acc[c] = acc[c] + f[q] * x[c * 64 + j0 + q];
  }
}

__device__ __forceinline__ void wave_lds_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(64) void blockgibbs_color_chains_kernel(pmgk_blockgibbs B, int tile0, int ntiles, int band, int32_t C, int nchunks, int ny, const uint64_t *__restrict__ keys, uint64_t sweep, const double *__restrict__ Xi, const double *__restrict__ b, int bcs, double *Y)
{
  __shared__ pmg::LogTabEntry s_logtab[MODE == BG_DRAW ? PMG_LOGTAB_SIZE : 1];
  __shared__ double           s_r[CB * 64];
  __shared__ double           s_x[MODE != BG_DET ? CB * 64 : 1];
  const int                   lane = threadIdx.x;
  // workgroup -> (tile, first chunk): workgroups are dealt round-robin over the 8 XCDs, so workgroups id and id + 8 share an L2.
  // XCD x takes the band of tiles [x * band, (x + 1) * band) with all their chunks, the chunks of a tile next to each other:
  // neighbouring blocks of a colour gather the same exterior rows, and the chunks of a tile read the same factors.  For speed
  // only: any placement gives the same result.
  const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
  const int tl  = xcd * band + k / ny;
  if (tl >= ntiles) return; // the whole wavefront, before any exchange
  if (MODE == BG_DRAW) pmg::load_log_table_wave(s_logtab, lane);
  const int      t    = tile0 + tl;
  const int      g    = __builtin_amdgcn_readfirstlane(B.tile_g[t]);
  const int      ew   = __builtin_amdgcn_readfirstlane(B.tile_ew[t]);
  const int64_t  foff = B.tile_foff[t], eoff = B.tile_eoff[t];
  const int      pos  = B.pos[(int64_t)t * 64 + lane];
  const bool     live = pos >= 0;
  const int64_t  prow = (int64_t)(live ? pos : 0) * C; // 64-bit: pos * C passes 2^31
  const uint32_t s    = MODE != BG_DET ? (uint32_t)B.slot[(int64_t)t * 64 + lane] : 0u;
  const double  *ev   = B.evals + eoff + lane;
  const int32_t *ec   = B.ecols + eoff + lane;
  const int      base = lane & ~(g - 1); // first lane of my block
  for (int chunk = k % ny; chunk < nchunks; chunk += ny) {
    const int c0 = chunk * CB;
    const int nc = min(CB, C - c0);
    // the first batch of exterior entries is requested before the normals are drawn: its latency passes under the arithmetic
    double  a[IB]  = {};
    int32_t cj[IB] = {};
    if (ew > 0) load_entries(a, cj, ev, ec, 0, ew); // a tile of whole components has no exterior entry at all
    // 1. the normals
    if (MODE == BG_XI) {
      double xv[CB];
      load_chunk<VEC>(xv, Xi + (int64_t)s * C + c0, live ? nc : 0);
#pragma unroll
      for (int c = 0; c < CB; ++c) s_x[c * 64 + lane] = xv[c];
    }
    if (MODE == BG_DRAW) {
#pragma unroll 1
      for (int c = 0; c < CB; ++c) {
        double xi = 0.0;
        if (c < nc) { // uniform
          const uint64_t key = keys[c0 + c];
          double         z0, z1;
          pmg::normal_pair(s >> 1, 0u, (uint32_t)sweep, (uint32_t)(sweep >> 32), (uint32_t)key, (uint32_t)(key >> 32), s_logtab, z0, z1);
          xi = (s & 1u) ? z1 : z0;
          if (!live) xi = 0.0;
        }
        s_x[c * 64 + lane] = xi;
      }
    }
    // 2. r = b - sum a_k y[col_k] over the exterior entries, in storage order
    double sum[CB];
    if (bcs) {
      load_chunk<VEC>(sum, b + prow + c0, live ? nc : 0);
    } else {
      const double bv = live ? b[pos] : 0.0;
#pragma unroll
      for (int c = 0; c < CB; ++c) sum[c] = bv;
    }
    for (int j0 = 0; j0 < ew; j0 += IB) {
      if (j0) load_entries(a, cj, ev, ec, j0, ew);
#pragma unroll
      for (int h = 0; h < IB; h += EB) { // the gathers of EB entries are in flight together
        double yv[EB][CB];
#pragma unroll
        for (int q = 0; q < EB; ++q) load_chunk<VEC>(yv[q], Y + (int64_t)cj[h + q] * C + c0, j0 + h < ew ? nc : 0);
#pragma unroll
        for (int q = 0; q < EB; ++q)
          if (j0 + h + q < ew) {
#pragma unroll
            for (int c = 0; c < CB; ++c) sum[c] = sum[c] - a[h + q] * yv[q][c];
          }
      }
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) s_r[c * 64 + lane] = live ? sum[c] : 0.0; // whatever a pad entry read: the factor's zero columns must meet a finite value
    wave_lds_sync();
    // 3. the row of W^T W (and of W^T)
    double out[CB];
    block_row_chains(out, g, B.M + foff + lane, s_r + base);
    if (MODE != BG_DET) {
      double nz[CB];
      block_row_chains(nz, g, B.WT + foff + lane, s_x + base);
#pragma unroll
      for (int c = 0; c < CB; ++c) out[c] = out[c] + nz[c];
    }
    store_chunk<VEC>(Y + prow + c0, out, live ? nc : 0);
    wave_lds_sync(); // the next chunk writes the lines this one has read
  }
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : 1; }

template <int MODE>
int launch(const pmgk_blockgibbs *B, int tile0, int ntiles, int32_t C, const uint64_t *keys, uint64_t sweep, const double *Xi, const double *b, int bcs, double *Y, void *stream)
{
  const int  nchunks = (C + CB - 1) / CB;
  const int  band    = (ntiles + 7) / 8;                                                                // tiles per XCD
  const int  ny      = (int)std::min<int64_t>(nchunks, std::max<int64_t>(1, ((int64_t)1 << 30) / (8 * (int64_t)band))); // chunks side by side; the rest in the kernel's loop
  const dim3 block(64), grid(8u * (unsigned)band * (unsigned)ny);
  // 16-byte accesses need even rows on 16-byte aligned vectors (a shared b is read 8 bytes at a time either way)
  const uintptr_t al  = (uintptr_t)Y | (MODE == BG_XI ? (uintptr_t)Xi : 0) | (bcs ? (uintptr_t)b : 0);
  const bool      vec = (C % 2 == 0) && (al % 16 == 0);
  if (vec) hipLaunchKernelGGL((blockgibbs_color_chains_kernel<MODE, true>), grid, block, 0, (hipStream_t)stream, *B, tile0, ntiles, band, C, nchunks, ny, keys, sweep, Xi, b, bcs, Y);
  else hipLaunchKernelGGL((blockgibbs_color_chains_kernel<MODE, false>), grid, block, 0, (hipStream_t)stream, *B, tile0, ntiles, band, C, nchunks, ny, keys, sweep, Xi, b, bcs, Y);
  return launch_status();
}

} // namespace

// tiles [tile0, tile0 + ntiles) on C chains.  mode as pmgk_blockgibbs_color_sweep: 0 no noise, 1 the slot stream of (keys_dev[c],
// sweep), 2 Xi_slots[slot * C + c]; bcs = chain stride of b (0: one shared vector, 1: len x C)
extern "C" int pmgk_blockgibbs_color_sweep_chains(const pmgk_blockgibbs *B, int tile0, int ntiles, int mode, int32_t C, const uint64_t *keys_dev, uint64_t sweep, const double *Xi_slots, const double *b, int bcs, double *Y, void *stream)
{
  if (ntiles <= 0) return 0;
  if (C < 1 || (mode == BG_XI && !Xi_slots) || (mode == BG_DRAW && !keys_dev)) return 1;
  if (mode == BG_DET) return launch<BG_DET>(B, tile0, ntiles, C, keys_dev, sweep, Xi_slots, b, bcs, Y, stream);
  if (mode == BG_DRAW) return launch<BG_DRAW>(B, tile0, ntiles, C, keys_dev, sweep, Xi_slots, b, bcs, Y, stream);
  if (mode == BG_XI) return launch<BG_XI>(B, tile0, ntiles, C, keys_dev, sweep, Xi_slots, b, bcs, Y, stream);
  return 1;
}
