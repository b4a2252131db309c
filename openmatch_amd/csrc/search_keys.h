// What the two units of the exact search share (search.hip: the list kernels and the host chain; search_scan.hip: the scan kernels):
// the 64-bit key of a candidate and the capacity of a list.
#pragma once
#include "kernels.h"
#include "search_plan.h"

#define SORT_CAP 8192      // keys one workgroup sorts in LDS (64 KiB)
static_assert(SORT_CAP == SEARCH_SORT_CAP, "search_plan.h schedules for this list size");

typedef unsigned long long u64;

__host__ __device__ inline u64 pack_key(float score, uint32_t payload) {
  return ((u64)f32_orderable(score) << 32) | (u64)(uint32_t)~payload;
}
__host__ __device__ inline float key_score(u64 k) { return orderable_f32((uint32_t)(k >> 32)); }
__host__ __device__ inline uint32_t key_payload(u64 k) { return ~(uint32_t)k; }
