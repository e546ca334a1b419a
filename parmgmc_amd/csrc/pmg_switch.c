/* The table of the PMG_* environment switches (pmg_switch.h): name, parse kind, default, read time.  Plain C11, no HIP and
   nothing of the rest of the library.  A new switch is one id in pmg_switch.h, one row here, one line of INTEGRATION.md
   section 5 and a test that holds it to the default's results (tests/test_runtime_switch_inventory.py asks for all four). */
#include "pmg_switch.h"
#include <stdlib.h>

enum { PRESENT, INT, CHAR0 }; /* 1 if the variable exists (empty counts) | atoll, the default when unset | first character, 0 when unset or empty */
enum { PROCESS, LIVE };

static const struct { const char *name; int kind; long long dflt; int when; } pmg_switch_row[PMG_SW_COUNT] = {
  [PMG_SW_GRID_PACKED]                 = {"PMG_GRID_PACKED", INT, 2, PROCESS}, /* 0 = never, 1 = always, 2 = by lane efficiency */
  [PMG_SW_GRID_BANDED]                 = {"PMG_GRID_BANDED", INT, 1, PROCESS},
  [PMG_SW_GRID_TAIL]                   = {"PMG_GRID_TAIL", INT, 1, PROCESS},
  [PMG_SW_GRID_FLAT]                   = {"PMG_GRID_FLAT", INT, 1, PROCESS},
  [PMG_SW_GRID_PLANE_PAIR]             = {"PMG_GRID_PLANE_PAIR", INT, 1, PROCESS},
  [PMG_SW_GRID_FUSED_RR]               = {"PMG_GRID_FUSED_RR", INT, 1, PROCESS},
  [PMG_SW_GRID_RR_CHUNK]               = {"PMG_GRID_RR_CHUNK", INT, 0, PROCESS},
  [PMG_SW_GRID_RR_SYNC]                = {"PMG_GRID_RR_SYNC", INT, -1, PROCESS}, /* -1 = by grid size */
  [PMG_SW_TRANSFER_GENERIC]            = {"PMG_TRANSFER_GENERIC", PRESENT, 0, PROCESS},
  [PMG_SW_ST27_PHASE_MAX_PLANE]        = {"PMG_ST27_PHASE_MAX_PLANE", INT, 1100, PROCESS},
  [PMG_SW_ST27_PACK_REMAINDER]         = {"PMG_ST27_PACK_REMAINDER", INT, 1, PROCESS},
  [PMG_SW_ST27_PAIR]                   = {"PMG_ST27_PAIR", INT, 1, PROCESS},
  [PMG_SW_ST27_PAIR_SLAB]              = {"PMG_ST27_PAIR_SLAB", INT, 1, PROCESS}, /* probes: 2 = paired residual only, 3 = paired sweeps only */
  [PMG_SW_MG_FUSED_ZERO]               = {"PMG_MG_FUSED_ZERO", INT, 1, PROCESS},
  [PMG_SW_MG_PROLONG_BOTH]             = {"PMG_MG_PROLONG_BOTH", PRESENT, 0, PROCESS},
  [PMG_SW_SELL_LOCALITY]               = {"PMG_SELL_LOCALITY", INT, 1, PROCESS}, /* 0 = never, 2 = always */
  [PMG_SW_DISTMCSOR_REFRESH_BY_COLOUR] = {"PMG_DISTMCSOR_REFRESH_BY_COLOUR", PRESENT, 0, PROCESS},
  [PMG_SW_TRACE]                       = {"PMG_TRACE", CHAR0, 0, PROCESS},
  [PMG_SW_GRID_SX_ALIGN]               = {"PMG_GRID_SX_ALIGN", INT, 0, LIVE}, /* no default: unset is the size rule of pmg_grid_line_stride (pmg_switch_if_set) */
  [PMG_SW_GRID_FUSED_RR_SLAB]          = {"PMG_GRID_FUSED_RR_SLAB", INT, 1, LIVE},
  [PMG_SW_MG_REPLICATE_BELOW]          = {"PMG_MG_REPLICATE_BELOW", INT, 1 << 19, LIVE}, /* 64-bit: pmg_switch_wide */
  [PMG_SW_MG_FULL_GALERKIN]            = {"PMG_MG_FULL_GALERKIN", PRESENT, 0, LIVE},
  [PMG_SW_MG_NO_STENCIL]               = {"PMG_MG_NO_STENCIL", PRESENT, 0, LIVE},
  [PMG_SW_MG_CSR_TRANSFERS]            = {"PMG_MG_CSR_TRANSFERS", PRESENT, 0, LIVE},
  [PMG_SW_LRC_FUSED]                   = {"PMG_LRC_FUSED", CHAR0, 0, LIVE}, /* '1': both fusions; '2': the noise term only; '3': the restore only */
  [PMG_SW_LRC_RESTORE]                 = {"PMG_LRC_RESTORE", CHAR0, 0, LIVE},
  [PMG_SW_LRC_REDUCE]                  = {"PMG_LRC_REDUCE", CHAR0, 0, LIVE},
  [PMG_SW_LRC_BTY]                     = {"PMG_LRC_BTY", CHAR0, 0, LIVE},
  [PMG_SW_LRC_DENSE]                   = {"PMG_LRC_DENSE", PRESENT, 0, LIVE},
  [PMG_SW_LRC_BATCH]                   = {"PMG_LRC_BATCH", INT, 1, LIVE},
  [PMG_SW_IPC_DEBUG]                   = {"PMG_IPC_DEBUG", PRESENT, 0, LIVE},
};

long long     pmg_switch_value[PMG_SW_COUNT];
unsigned char pmg_switch_latched[PMG_SW_COUNT];

long long pmg_switch_parse(pmg_switch_id id, int *is_set)
{
  const int   latch = pmg_switch_row[id].when == PROCESS;
  const char *e     = getenv(pmg_switch_row[id].name);
  if (is_set) *is_set = e != NULL;
  if (latch && __atomic_load_n(&pmg_switch_latched[id], __ATOMIC_ACQUIRE)) return __atomic_load_n(&pmg_switch_value[id], __ATOMIC_RELAXED);
  const int       kind = pmg_switch_row[id].kind;
  const long long v    = kind == PRESENT ? e != NULL : kind == CHAR0 ? (e ? (unsigned char)e[0] : 0) : e ? atoll(e) : pmg_switch_row[id].dflt;
  if (latch) {
    __atomic_store_n(&pmg_switch_value[id], v, __ATOMIC_RELAXED);
    __atomic_store_n(&pmg_switch_latched[id], 1, __ATOMIC_RELEASE);
  }
  return v;
}
