/* What the multi-chain entry points of every object share (MCSOR, the chains V-cycle, Woodbury, block Gibbs, the statistics
   handles): the device copy of the chains' noise keys and the size check of an ld x C launch. */
#include "pmg_internal.h"

pmg_status pmg_keybuf_set(pmg_keybuf *k, const uint64_t *keys, int64_t n, void *stream)
{
  if (k->n == n && n > 0 && !memcmp(k->host, keys, sizeof(uint64_t) * (size_t)n)) return PMG_SUCCESS;
  const size_t bytes = sizeof(uint64_t) * (size_t)n;
  /* one synchronisation either way: launches in flight may still read the keys; the host copy is the source of the last upload */
  if (bytes > k->dev.cap) {
    k->n = 0;
    PMG_CALL(pmg_devbuf_reserve(&k->dev, bytes, stream));
    free(k->host);
    k->host = (uint64_t *)malloc(bytes);
    if (!k->host) {
      pmg_devbuf_free(&k->dev);
      PMG_FAIL(PMG_ERR_MEM, "out of host memory");
    }
  } else PMG_HIP(hipStreamSynchronize((hipStream_t)stream));
  memcpy(k->host, keys, bytes);
  k->n = n;
  PMG_HIP(hipMemcpyAsync(k->dev.p, k->host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return PMG_SUCCESS;
}

void pmg_keybuf_free(pmg_keybuf *k)
{
  pmg_devbuf_free(&k->dev);
  free(k->host);
  memset(k, 0, sizeof *k);
}

/* the launches index ld x C elements with 64-bit offsets; grids of 256-thread blocks over them and chunks of 64 chains in
   blockIdx.y must stay inside the launch limits */
pmg_status pmg_chains_size_check(int64_t ld, int32_t nchains)
{
  PMG_CHECK(nchains >= 1, PMG_ERR_ARG_OUTOFRANGE, "nchains = %d", nchains);
  PMG_CHECK(nchains <= 64 * 65535, PMG_ERR_ARG_OUTOFRANGE, "nchains = %d exceeds %d", nchains, 64 * 65535);
  PMG_CHECK(ld <= ((int64_t)1 << 40) / nchains, PMG_ERR_ARG_OUTOFRANGE, "%lld rows x %d chains exceed 2^40 elements", (long long)ld, nchains);
  return PMG_SUCCESS;
}
