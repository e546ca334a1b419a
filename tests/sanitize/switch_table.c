/* Prints what the switch accessors (csrc/pmg_switch.h) return for every row of the table in csrc/pmg_switch.c, for
   tests/test_switch_table.py to compare with the expressions the call sites used before there was a table.  Host only.
     switch_table            every value of the set in turn: PROCESS rows latch, so the program re-executes itself once per
                             value (no device here, so exec is harmless); then the two read times
     switch_table threads    eight threads first-read every PROCESS row at once (built with -fsanitize=thread) */
#define _GNU_SOURCE
#include "../../parmgmc_amd/csrc/pmg_switch.c" /* the table itself is static: the names and read times come from it */
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

static const char *const values[] = {NULL, "", "0", "1", "2", "3", "4", "16", "400", "1000000000", "x"};
enum { NVALUES = sizeof values / sizeof values[0], NTHREADS = 8 };

static void set_all(const char *v)
{
  for (int id = 0; id < PMG_SW_COUNT; ++id)
    if ((v ? setenv(pmg_switch_row[id].name, v, 1) : unsetenv(pmg_switch_row[id].name)) != 0) _exit(4);
}

static void set_one(pmg_switch_id id, const char *v)
{
  if ((v ? setenv(pmg_switch_row[id].name, v, 1) : unsetenv(pmg_switch_row[id].name)) != 0) _exit(4);
}

static pthread_barrier_t barrier;
static long long         seen[NTHREADS][PMG_SW_COUNT];

static void *first_reads(void *arg)
{
  long long *mine = (long long *)arg;
  pthread_barrier_wait(&barrier);
  for (int id = 0; id < PMG_SW_COUNT; ++id)
    if (pmg_switch_row[id].when == PROCESS) mine[id] = pmg_switch_wide((pmg_switch_id)id);
  return NULL;
}

int main(int argc, char **argv)
{
  if (argc > 1 && !strcmp(argv[1], "threads")) {
    pthread_t th[NTHREADS];
    set_all("3");
    if (pthread_barrier_init(&barrier, NULL, NTHREADS)) return 5;
    for (int t = 0; t < NTHREADS; ++t)
      if (pthread_create(&th[t], NULL, first_reads, seen[t])) return 5;
    for (int t = 0; t < NTHREADS; ++t) pthread_join(th[t], NULL);
    for (int id = 0; id < PMG_SW_COUNT; ++id) {
      if (pmg_switch_row[id].when != PROCESS) continue;
      for (int t = 1; t < NTHREADS; ++t)
        if (seen[t][id] != seen[0][id]) return 6;
      printf("T %s : %lld\n", pmg_switch_row[id].name, seen[0][id]);
    }
    printf("switch_table ok\n");
    return 0;
  }
  const int stage = argc > 1 ? atoi(argv[1]) : 0;
  if (stage < NVALUES) { /* one value of the set for every variable, in a process that has read none of them yet */
    set_all(values[stage]);
    for (int id = 0; id < PMG_SW_COUNT; ++id) {
      int       got = -7, set;
      const int was_set = pmg_switch_if_set((pmg_switch_id)id, &got);
      (void)pmg_switch_parse((pmg_switch_id)id, &set);
      if (set != was_set || (!was_set && got != -7)) return 7;
      printf("V %d %s %s : %lld %d %d\n", stage, pmg_switch_row[id].name, pmg_switch_row[id].when == PROCESS ? "PROCESS" : "LIVE", pmg_switch_wide((pmg_switch_id)id), pmg_switch((pmg_switch_id)id), was_set);
    }
    fflush(stdout);
    char next[16];
    snprintf(next, sizeof next, "%d", stage + 1);
    char *args[] = {argv[0], next, NULL};
    execv("/proc/self/exe", args);
    return 8;
  }
  /* the two read times.  A PROCESS row keeps its first value whatever the environment does afterwards, and a second row,
     first read only after the change, sees the new value: the latch is per row */
  set_all("0");
  printf("P PMG_GRID_PACKED first : %d\n", pmg_switch(PMG_SW_GRID_PACKED));
  set_all("1");
  printf("P PMG_GRID_PACKED after_setenv : %d\n", pmg_switch(PMG_SW_GRID_PACKED));
  printf("P PMG_GRID_BANDED first : %d\n", pmg_switch(PMG_SW_GRID_BANDED));
  set_all(NULL);
  printf("P PMG_GRID_PACKED after_unsetenv : %d\n", pmg_switch(PMG_SW_GRID_PACKED));
  printf("P PMG_GRID_BANDED after_unsetenv : %d\n", pmg_switch(PMG_SW_GRID_BANDED));
  printf("P PMG_GRID_TAIL first : %d\n", pmg_switch(PMG_SW_GRID_TAIL));
  for (int id = 0; id < PMG_SW_COUNT; ++id) { /* a LIVE row follows every change */
    if (pmg_switch_row[id].when != LIVE) continue;
    printf("L %s :", pmg_switch_row[id].name);
    const char *seq[] = {"1", "0", NULL, "2", ""};
    for (unsigned q = 0; q < sizeof seq / sizeof seq[0]; ++q) {
      set_one((pmg_switch_id)id, seq[q]);
      printf(" %lld", pmg_switch_wide((pmg_switch_id)id));
    }
    printf("\n");
  }
  printf("switch_table ok\n");
  return 0;
}
