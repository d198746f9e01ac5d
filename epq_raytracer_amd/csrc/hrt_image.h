// hrt_image.h -- launch interface of the image passes (hrt_image.hip): clear, the progressive accumulator
// (assets/image_combiner.glsl), fold records, format conversion, the present pass and row-tile assembly.
//
// An image crosses this interface as one pointer plus its format: f32 = float4 texels (HRT_MODE_RGBA32F),
// else packed RGBA8 words.  The typed pointers are recovered inside the launchers only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_raytrace.h"

namespace hrt {

hipError_t launch_clear(void* img, bool f32, size_t npix, hipStream_t stream);
// image_combiner.glsl for one frame: cur <- fold of nw as frame `frame` (frame 0 does not read cur)
hipError_t launch_accumulate(void* cur, const void* nw, bool f32, size_t npix, uint32_t frame, hipStream_t stream);
// the nf frames of a stack (image f at f * npix) folded into the accumulator as frames frame0 + f
hipError_t launch_accumulate_frames(void* cur, const void* stack, bool f32, size_t npix, uint32_t nf, uint32_t frame0,
                                    hipStream_t stream);
// The fold of launch_accumulate_frames (store) or its chain in registers only (!store) with one fold record
// per frame: frame f's counts are ADDED to ring[(slot0 + f) % HRT_FOLD_RECORD_RING], which the caller zeroed
// on the stream before (changed_pixels, max_delta and abs_delta_sum; the host keeps the frame numbers).
// real_pix <= npix: the pixels that count.  nf <= HRT_FOLD_RECORD_RING.  A single-frame fold is nf == 1
// with the trace image as the stack.  The grid is sized by num_cus, not by npix.
hipError_t launch_fold_records(void* cur, const void* stack, bool f32, size_t npix, size_t real_pix, uint32_t nf,
                               uint32_t frame0, bool store, hrt_fold_record* ring, uint32_t slot0, uint32_t num_cus,
                               hipStream_t stream);
// format conversion for hrt_read_image: dst <- src in the other format (src_f32: float4 -> RGBA8 words)
hipError_t launch_convert(const void* src, bool src_f32, void* dst, size_t npix, hipStream_t stream);
// The present pass (hrt_present): the target of width x height pixels of 4 bytes, rows pitch bytes apart
// (dst 4-byte aligned, pitch a multiple of 4); bgra: bytes 0 and 2 of each pixel swapped.
struct PresentTarget {
  unsigned char* dst;
  uint32_t width, height, pitch, bgra;
};
// target(x, y) = the ws x hs image's texel (((2x+1) ws) div (2 width), hs - 1 - ((2y+1) hs) div (2 height)):
// present_rows at the image's own size, else present_nearest
hipError_t launch_present(const void* src, bool f32, uint32_t ws, uint32_t hs, const PresentTarget& t,
                          hipStream_t stream);
// The gathered present: the full width x height image as the root of a row-tile group holds it after the
// gather -- parts blocks of local_rows x width pixels in part order, global row y in block
// (y / row_tile) % parts (hrt_present_map.h).  launch_present's rule over the full image, read straight
// from the blocks.
struct GatheredImage {
  const void* src;
  bool f32;
  uint32_t width, height, row_tile, parts, local_rows;
};
hipError_t launch_present_gathered(const GatheredImage& g, const PresentTarget& t, hipStream_t stream);
// launch_accumulate on a w x h image (t of the same size) whose kernel also writes the folded pixel to t
hipError_t launch_accumulate_present(void* cur, const void* nw, bool f32, uint32_t w, uint32_t h, uint32_t frame,
                                     const PresentTarget& t, hipStream_t stream);
// Row-tile framebuffer assembly: gathered = parts x local_rows rows (rank-major), frame = height rows of
// row_words 4-byte words; global row y comes from part (y / row_tile) % parts (hip_raytrace.h partition).
hipError_t launch_assemble_rows(const uint32_t* gathered, uint32_t* frame, uint32_t row_words, uint32_t height,
                                uint32_t local_rows, uint32_t row_tile, uint32_t parts, hipStream_t stream);

}  // namespace hrt
