// What the two channels-last convolutions -- the image stem (stem.hip, stem_tile.hpp) and the general one (lpips.hip, conv_plan.hpp)
// -- have in common, free of HIP headers: the shape of a workgroup's output tile and the map from an accumulator element of
// v_mfma_f32_32x32x2_f32 to its output.  stem_tile.hpp and conv_plan.hpp re-export these names into their namespaces; the kernels
// stay two.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DNS_TILE_HD __host__ __device__ inline
#else
#define DNS_TILE_HD inline
#endif

namespace dns {
namespace convt {

constexpr int THREADS = 256;                       // 4 waves
constexpr int WAVES = 4;
constexpr int TILE_W = 32;                         // output pixels of one matrix tile (M = 32) along x
constexpr int ROWS_PER_WAVE = 2;                   // matrix tiles per wave: consecutive output rows
constexpr int TILE_H = WAVES * ROWS_PER_WAVE;      // 8 output rows per workgroup

// Accumulator element -> output: wave `wave`'s matrix tile `mt` is the tile's output row row_of(wave, mt); register r of lane l holds
// the pixel acc_pixel(r, l) of that row and the channel acc_channel(l) (+ 32 for the second N block): the C/D map of the 32x32 forms
DNS_TILE_HD int row_of(int wave, int mt) { return wave * ROWS_PER_WAVE + mt; }
DNS_TILE_HD int acc_pixel(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
DNS_TILE_HD int acc_channel(int lane) { return lane & 31; }

#if defined(__HIPCC__)
typedef float f32x16 __attribute__((ext_vector_type(16)));
// ReLU that keeps a NaN (IEEE 754-2019 maximum; fmaxf returns 0 for a NaN), as in the MLP kernels
__device__ __forceinline__ float relu(float a) { return __builtin_elementwise_maximum(a, 0.f); }
#endif

}  // namespace convt
}  // namespace dns
