/* The PMG_* environment switches of the native library: one id per row of the table in pmg_switch.c, which alone calls
   getenv.  A PROCESS row is parsed at its first read and then fixed for the life of the process; a LIVE row is parsed at
   every read, and the caller decides when that is (an object's build, a set-up, a sampler's first cycle).  C and HIP. */
#ifndef PMG_SWITCH_H
#define PMG_SWITCH_H
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { /* in the order of the table's rows: the PROCESS rows, then the LIVE rows */
  PMG_SW_GRID_PACKED, PMG_SW_GRID_BANDED, PMG_SW_GRID_TAIL, PMG_SW_GRID_FLAT, PMG_SW_GRID_PLANE_PAIR,
  PMG_SW_GRID_FUSED_RR, PMG_SW_GRID_RR_CHUNK, PMG_SW_GRID_RR_SYNC,
  PMG_SW_TRANSFER_GENERIC, PMG_SW_ST27_PHASE_MAX_PLANE, PMG_SW_ST27_PACK_REMAINDER, PMG_SW_ST27_PAIR, PMG_SW_ST27_PAIR_SLAB,
  PMG_SW_MG_FUSED_ZERO, PMG_SW_MG_PROLONG_BOTH, PMG_SW_SELL_LOCALITY, PMG_SW_DISTMCSOR_REFRESH_BY_COLOUR, PMG_SW_TRACE,
  PMG_SW_GRID_SX_ALIGN, PMG_SW_GRID_FUSED_RR_SLAB,
  PMG_SW_MG_REPLICATE_BELOW, PMG_SW_MG_FULL_GALERKIN, PMG_SW_MG_NO_STENCIL, PMG_SW_MG_CSR_TRANSFERS,
  PMG_SW_LRC_FUSED, PMG_SW_LRC_RESTORE, PMG_SW_LRC_REDUCE, PMG_SW_LRC_BTY, PMG_SW_LRC_DENSE, PMG_SW_LRC_BATCH, PMG_SW_IPC_DEBUG,
  PMG_SW_COUNT
} pmg_switch_id;

/* The latch of the PROCESS rows.  The sampler objects may be used from several host threads: the value is stored first,
   then its flag with release order, and a reader loads the flag with acquire order (the compilers' C11-model builtins,
   since <stdatomic.h> cannot be included from C++17).  Two threads that race on a first read both parse the same string. */
extern long long     pmg_switch_value[PMG_SW_COUNT];
extern unsigned char pmg_switch_latched[PMG_SW_COUNT];

/* Parses the row's variable now (a PROCESS row that is already latched returns its value) and latches a PROCESS row;
   *is_set, where asked for, tells a variable that exists from one that does not. */
long long pmg_switch_parse(pmg_switch_id id, int *is_set);

/* A latched PROCESS row costs one flag load and one array load, no call: this is what the launchers read per launch. */
static inline long long pmg_switch_wide(pmg_switch_id id)
{
  if (__atomic_load_n(&pmg_switch_latched[id], __ATOMIC_ACQUIRE)) return __atomic_load_n(&pmg_switch_value[id], __ATOMIC_RELAXED);
  return pmg_switch_parse(id, 0);
}
static inline int pmg_switch(pmg_switch_id id) { return (int)pmg_switch_wide(id); }

/* 1 and *value where the variable exists, 0 and *value untouched where it does not (LIVE rows): "unset" is no integer */
static inline int pmg_switch_if_set(pmg_switch_id id, int *value)
{
  int             set;
  const long long v = pmg_switch_parse(id, &set);
  if (set) *value = (int)v;
  return set;
}

#ifdef __cplusplus
}
#endif
#endif
