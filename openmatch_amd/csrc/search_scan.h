// The scan kernels of the exact search (search_scan.hip) as the rest of the search code sees them: two functions, no kernel symbol.
#pragma once
#include "search_keys.h"

// The dynamic-LDS attribute of every scan kernel: host calls, made once (a capturing stream must not meet them).
int scan_attrs();

// One launch of the table row that (plan, l.kernel, half) names: the l.rows index rows at `rows` ([l.rows, d], float32 or -- half -- 16-bit,
// ids from row_base) against the queries, on l.grid workgroups with l.group as the kernel's last integer argument; survivors are
// appended to keys / cnt.  l.row0 is the caller's: `rows` and `row_base` already name the launch's first row.
int scan_launch(const ScanPlan& plan, const ScanLaunch& l, bool half, const ScanSwitches& sw, const void* rows, uint32_t row_base,
                const void* queries, int64_t nq, int d, const float* thr, u64* keys, unsigned* cnt, hipStream_t s);
