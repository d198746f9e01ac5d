// hrt_refine_tile_bits.h -- the mask arithmetic of the tile-masked refinement (hrt_refine_tiles, DESIGN.md §2 S18,
// §33): the bits of a pixel mask that belong to one row of an 8x8 tile, and from them the tile's selected pixels.
// Shared by the kernel (hrt_refine.hip refine_tile_bits) and a plain C++ test program
// (tests/cpp/refine_tile_bits_test.cpp): no HIP header is needed to compile it.
//
// The mask is hrt_refine's: pixel i = x + y W is bit i & 31 of word i >> 5, ceil(W H / 32) words; the bits of the
// last word beyond the image are ignored.  Tile (tx, ty) holds the real pixels x in [8 tx, min(8 tx + 8, W)),
// y in [8 ty, min(8 ty + 8, H)).  A tile row's bits start at bit y W + 8 tx: they can straddle two words, be cut
// short at the image's right edge, and lie in the last word beside ignored bits.  Only words that hold a real
// pixel's bit are read.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HRT_TILE_FN __host__ __device__ inline
#else
#define HRT_TILE_FN inline
#endif

namespace hrt {

// The real pixels of tile column tx in one row: min(8, W - 8 tx)   (8 tx < W).
HRT_TILE_FN uint32_t tile_row_pixels(uint32_t width, uint32_t tx) {
  const uint32_t left = width - 8u * tx;
  return left < 8u ? left : 8u;
}

// The mask bits of row y's pixels in tile column tx, pixel 8 tx + k in bit k; the bits from tile_row_pixels up are 0.
HRT_TILE_FN uint32_t tile_row_bits(const uint32_t* mask, uint32_t width, uint32_t y, uint32_t tx) {
  const uint32_t n = tile_row_pixels(width, tx);
  const uint64_t first = (uint64_t)y * width + 8u * tx;  // the row's first bit; its last, first + n - 1, is a pixel's
  const uint64_t w0 = first >> 5;
  const uint32_t sh = (uint32_t)(first & 31u);
  uint32_t v = mask[w0] >> sh;
  if (sh + n > 32u) v |= mask[w0 + 1] << (32u - sh);  // (sh > 24 here: the shift is 1..7)
  return v & ((1u << n) - 1u);
}

// The selected real pixels of tile (tx, ty) of a width x height image, and (*real) its real pixels.
HRT_TILE_FN uint32_t tile_selected_pixels(const uint32_t* mask, uint32_t width, uint32_t height, uint32_t tx, uint32_t ty,
                                          uint32_t* real) {
  const uint32_t y1 = 8u * ty + 8u < height ? 8u * ty + 8u : height;
  uint32_t count = 0;
  for (uint32_t y = 8u * ty; y < y1; ++y) {
    uint32_t v = tile_row_bits(mask, width, y, tx);
    for (; v; v &= v - 1u) ++count;
  }
  *real = (y1 - 8u * ty) * tile_row_pixels(width, tx);
  return count;
}

}  // namespace hrt
