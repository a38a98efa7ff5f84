// The hash grid's level table on the host, free of HIP headers: common.hpp includes it for every kernel file, and the host check
// programs under tools/ (plain g++ with sanitizers, no GPU) compile it as it stands.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../include/dns_hip.h"

namespace dns {

constexpr int MAX_DYN_LDS = 160 * 1024;      // gfx950: 160 KiB of LDS per CU, all of it available to one workgroup

// Device-side copy of the level table, passed by value as a kernel argument.
struct GridLevels {
  uint32_t n_levels;
  float scale[DNS_MAX_LEVELS];
  uint32_t resolution[DNS_MAX_LEVELS];
  uint32_t size[DNS_MAX_LEVELS];
  uint32_t offset[DNS_MAX_LEVELS];
  uint32_t hashed[DNS_MAX_LEVELS];
};

inline GridLevels to_levels(const DnsGridMeta* m) {
  GridLevels g;
  g.n_levels = m->n_levels;
  for (uint32_t l = 0; l < DNS_MAX_LEVELS; ++l) {
    g.scale[l] = m->scale[l];
    g.resolution[l] = m->resolution[l];
    g.size[l] = m->size[l];
    g.offset[l] = m->offset[l];
    g.hashed[l] = m->hashed[l];
  }
  return g;
}

// tcnn GridEncoding constructor arithmetic:
//   scale = exp2(l * log2(pls)) * base - 1;  res = ceilf(scale) + 1;
// tcnn evaluates `scale` in float32 with CUDA's exp2f, whose last bits no other platform reproduces; at the
// finest level the exact value is an integer (desired_resolution - 1), so one ulp flips the resolution.  The
// table is therefore DEFINED here as the float64 value rounded once to float32 (finest level = exactly
// desired_resolution - 1), computed on the host only and handed to every kernel and to the oracle's check.
//   size  = min(next_multiple(res^3, 8), 2^log2_T);
//   dense index while the running stride stays <= size, hashed once it exceeds it.
// The body of dns_grid_meta_init (host.cpp), which checks the arguments' ranges first; false: the table exceeds 2^31 rows.
inline bool grid_meta_fill(DnsGridMeta* meta, uint32_t n_levels, uint32_t n_features, uint32_t log2_hashmap_size,
                           uint32_t base_resolution, double per_level_scale) {
  memset(meta, 0, sizeof(*meta));
  meta->n_levels = n_levels;
  meta->n_features = n_features;
  meta->log2_hashmap_size = log2_hashmap_size;
  meta->base_resolution = base_resolution;
  meta->per_level_scale = (float)per_level_scale;
  const double log2_pls = log2(per_level_scale);
  const uint32_t T = 1u << log2_hashmap_size;
  uint64_t offset = 0;
  for (uint32_t l = 0; l < n_levels; ++l) {
    volatile double e = exp2((double)l * log2_pls);      // volatile: no fused contraction into the mul/sub below
    volatile double m = e * (double)base_resolution;
    const float scale = (float)(m - 1.0);
    const uint32_t res = (uint32_t)ceilf(scale) + 1u;
    uint64_t dense = (uint64_t)res * res * res;
    dense = (dense + 7u) / 8u * 8u;
    const uint32_t size = dense < T ? (uint32_t)dense : T;
    uint32_t stride = 1;
    for (int d = 0; d < 3 && stride <= size; ++d) stride *= res;   // uint32 wrap, as tcnn
    meta->scale[l] = scale;
    meta->resolution[l] = res;
    meta->size[l] = size;
    meta->offset[l] = (uint32_t)offset;
    meta->hashed[l] = size < stride ? 1u : 0u;
    offset += size;
    if (!(offset < (1ull << 31))) return false;
  }
  meta->total_rows = (uint32_t)offset;
  return true;
}

}  // namespace dns
