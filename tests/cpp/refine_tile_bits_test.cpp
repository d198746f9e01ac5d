// The mask arithmetic of the tile-masked refinement (epq_raytracer_amd/csrc/hrt_refine_tile_bits.h, shared with the
// refine_tile_bits kernel) against a bit-by-bit loop: every width 1..70 and height 1..17 with masks that are all zero,
// all one, a single bit at every position, and random, each with zeros and with garbage in the unused bits of the last
// word.  Every mask lives in a heap block of exactly its words, so that the sanitizer build
// (tests/test_refine_tiles_bits.py) sees a read past either end.
//
//   refine_tile_bits_test                 the self-check; prints the number of cases, exits 1 at the first mismatch
//   refine_tile_bits_test <in> <out>      in: records {u32 w, u32 h, mask words}; out: per record {u32 selected pixels,
//                                         u32 selected tiles, u32 their real pixels, the tile bitmap's words}
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hrt_refine_tile_bits.h"

namespace {

struct Result {
  uint32_t selected = 0, tiles_selected = 0, traced = 0;
  std::vector<uint32_t> bits;
  bool operator==(const Result& o) const {
    return selected == o.selected && tiles_selected == o.tiles_selected && traced == o.traced && bits == o.bits;
  }
};

// what the kernel computes, tile by tile, through the shared header
Result by_header(const uint32_t* mask, uint32_t w, uint32_t h) {
  const uint32_t tx = (w + 7) / 8, ty = (h + 7) / 8;
  Result r;
  r.bits.assign((tx * ty + 31) / 32, 0u);
  for (uint32_t t = 0; t < tx * ty; ++t) {
    uint32_t real = 0;
    const uint32_t sel = hrt::tile_selected_pixels(mask, w, h, t % tx, t / tx, &real);
    r.selected += sel;
    if (sel) {
      r.bits[t >> 5] |= 1u << (t & 31u);
      ++r.tiles_selected;
      r.traced += real;
    }
  }
  return r;
}

// the specification, pixel by pixel
Result by_pixels(const uint32_t* mask, uint32_t w, uint32_t h) {
  const uint32_t tx = (w + 7) / 8, ty = (h + 7) / 8;
  Result r;
  r.bits.assign((tx * ty + 31) / 32, 0u);
  std::vector<uint32_t> real(tx * ty, 0u);
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      const uint32_t i = x + y * w, t = x / 8 + (y / 8) * tx;
      ++real[t];
      if ((mask[i >> 5] >> (i & 31u)) & 1u) {
        ++r.selected;
        r.bits[t >> 5] |= 1u << (t & 31u);
      }
    }
  for (uint32_t t = 0; t < tx * ty; ++t)
    if ((r.bits[t >> 5] >> (t & 31u)) & 1u) {
      ++r.tiles_selected;
      r.traced += real[t];
    }
  return r;
}

uint32_t rng_state = 0x9E3779B9u;
uint32_t rng() {  // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

uint64_t cases = 0;
bool check(const std::vector<uint32_t>& words, uint32_t w, uint32_t h, const char* what) {
  // exactly the mask's words on the heap, once as they are and once with garbage in the last word's unused bits
  const uint32_t n = w * h, nw = (n + 31) / 32;
  for (int garbage = 0; garbage < 2; ++garbage) {
    uint32_t* m = static_cast<uint32_t*>(std::malloc(nw * sizeof(uint32_t)));
    if (!m) return false;
    for (uint32_t i = 0; i < nw; ++i) m[i] = words[i];
    if (n % 32) {
      const uint32_t spare = 0xFFFFFFFFu << (n % 32);
      m[nw - 1] = (m[nw - 1] & ~spare) | (garbage ? (rng() | 0x80000000u) & spare : 0u);
    }
    const bool ok = by_header(m, w, h) == by_pixels(m, w, h);
    std::free(m);
    ++cases;
    if (!ok) {
      std::fprintf(stderr, "refine_tile_bits_test: %s mask differs at %u x %u (garbage %d)\n", what, w, h, garbage);
      return false;
    }
  }
  return true;
}

int self_check() {
  for (uint32_t w = 1; w <= 70; ++w)
    for (uint32_t h = 1; h <= 17; ++h) {
      const uint32_t n = w * h, nw = (n + 31) / 32;
      std::vector<uint32_t> words(nw, 0u);
      if (!check(words, w, h, "the all-zero")) return 1;
      words.assign(nw, 0xFFFFFFFFu);
      if (!check(words, w, h, "the all-one")) return 1;
      for (uint32_t i = 0; i < n; ++i) {
        words.assign(nw, 0u);
        words[i >> 5] = 1u << (i & 31u);
        if (!check(words, w, h, "a single-bit")) return 1;
      }
      for (int round = 0; round < 4; ++round) {
        for (uint32_t& v : words) v = round < 2 ? rng() : rng() & rng() & rng() & rng();  // dense, then sparse
        if (!check(words, w, h, "a random")) return 1;
      }
    }
  std::printf("refine_tile_bits_test: %llu masks agree with the bit-by-bit loop\n", (unsigned long long)cases);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return self_check();
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 3;
  uint32_t wh[2];
  while (std::fread(wh, 4, 2, in) == 2) {
    if (wh[0] == 0 || wh[1] == 0 || wh[0] > 4096 || wh[1] > 4096) return 4;
    std::vector<uint32_t> words(((size_t)wh[0] * wh[1] + 31) / 32);
    if (std::fread(words.data(), 4, words.size(), in) != words.size()) return 4;
    const Result r = by_header(words.data(), wh[0], wh[1]);
    const uint32_t head[3] = {r.selected, r.tiles_selected, r.traced};
    std::fwrite(head, 4, 3, out);
    std::fwrite(r.bits.data(), 4, r.bits.size(), out);
  }
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 3;
}
