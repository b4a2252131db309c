// Which kernel a filtered scan round runs: scan_plan() maps (index format, queries, width, switches) to a ScanPlan and does nothing
// else -- no launch, no HIP call, no global written, no pointer dereferenced.  Scan::filter_step (search.hip) launches what it returns;
// om_debug_scan_plan returns the plan alone, so the table is testable on a machine without a GPU, and om_debug_sim_stream launches the
// stream instantiation it names over a caller's buffers.  DESIGN.md 4f lists the rules in the order they are tested here.
#pragma once
#include "kernels.h"

struct ScanSwitches {
  int gen7;         // OM_OPT_SCAN_GEN7: 1 the persistent kernels (generation 7 for wide batches, the register-resident stream for small
                    // ones); 0 the tile-at-a-time kernels of generations 2 and 6
};

// every switch the planner reads, read once per call
static ScanSwitches scan_switches() { return ScanSwitches{om_option(OM_OPT_SCAN_GEN7)}; }

#define SCAN_KSTEP 64            // index columns per K step of the stream kernels (one 128-byte LDS row of 16-bit values)
#define SCAN_NKMAX32_NARROW 12   // K steps compiled into the 32-query stream kernel: 256 <= d <= 768 ...
#define SCAN_NKMAX32_WIDE 16     // ... and 832 <= d <= 1024
#define SCAN_NKMAX16 32          // K steps compiled into the 16-query stream kernel: 1088 <= d <= 2048

// What the planner decided.  family: OM_SCAN_FAMILY_*.  For the two stream families: qblock = queries per resident block (32: on
// 32 x 32 x 16 MFMAs, 16: on 16 x 16 x 32), nb = resident blocks per workgroup (1 | 2 | 4: 4 / nb waves share a block and a unit's 128
// rows), nkmax = K steps compiled in (query registers: qblock * nkmax * 64 * 2 bytes per wave).  The other families leave them 0.
struct ScanPlan { int family, qblock, nb, nkmax; };

static ScanPlan scan_plan(bool half, int64_t nq, int d, const ScanSwitches sw) {
  ScanPlan p = {OM_SCAN_FAMILY_GENERIC, 0, 0, 0};
  auto stream = [&](int family, int qblock, int nkmax) {
    const int64_t blocks = (nq + qblock - 1) / qblock;
    p.family = family; p.qblock = qblock; p.nb = blocks <= 1 ? 1 : blocks <= 2 ? 2 : 4; p.nkmax = nkmax;
    return p;
  };
  // 1. more than one 128-query tile: the 256 x 256 kernels (generation 7 / 7c / 7c16 over whole tiles, generation 6 for the ragged
  //    tail and with the switch off: filter_step's own sub-choice), in both index formats
  if (nq > 128) { p.family = OM_SCAN_FAMILY_WIDE; return p; }
  // 2. the float32 index, the switch off, no whole K step: the 128-query tile of generation 2
  if (!half || !sw.gen7 || nq < 1 || d < SCAN_KSTEP || d % SCAN_KSTEP != 0) return p;
  const int nk = d / SCAN_KSTEP;
  // 3. fewer than four K steps: the split append of the stream kernels has no retire point inside a tile
  if (nk < 4) return p;
  // 4. the query block(s) of a workgroup resident in registers, one pass over the index at stream speed
  if (nk <= SCAN_NKMAX32_NARROW) return stream(OM_SCAN_FAMILY_STREAM32, 32, SCAN_NKMAX32_NARROW);
  if (nk <= SCAN_NKMAX32_WIDE) return stream(OM_SCAN_FAMILY_STREAM32, 32, SCAN_NKMAX32_WIDE);
  // 5. wider rows: a 32-query block no longer fits a wave's registers, a 16-query block does up to d = 2048 -- at most 64 queries
  if (nk <= SCAN_NKMAX16 && nq <= 64) return stream(OM_SCAN_FAMILY_STREAM16, 16, SCAN_NKMAX16);
  return p;
}
