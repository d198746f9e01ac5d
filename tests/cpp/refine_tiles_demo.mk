# refine_tiles_demo: tile-masked refinement through the C++ host mirror (include/hrt_app.hpp) against the in-tree
# libhip_raytrace.so; built by __graft_entry__.build() so that the GPU box runs the same binary
# (tests/test_gpu_refine_tiles.py).  refine_tile_bits_test: the HIP-free mask arithmetic
# (epq_raytracer_amd/csrc/hrt_refine_tile_bits.h) against a bit-by-bit loop, plain and under ASan + UBSan
# (tests/test_refine_tiles_bits.py).  Run from this directory: make -f refine_tiles_demo.mk [clean]
ROOT := $(abspath ../..)
LIB := $(ROOT)/epq_raytracer_amd/lib
CSRC := $(ROOT)/epq_raytracer_amd/csrc
CXX ?= g++
all: refine_tiles_demo refine_tile_bits_test refine_tile_bits_test_san
refine_tiles_demo: refine_tiles_demo.cpp $(ROOT)/include/hrt_app.hpp $(ROOT)/include/hip_raytrace.h $(ROOT)/include/hrt_host.h $(LIB)/libhip_raytrace.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(LIB) -lhip_raytrace \
		-Wl,-rpath,'$$ORIGIN/../../epq_raytracer_amd/lib'
refine_tile_bits_test: refine_tile_bits_test.cpp $(CSRC)/hrt_refine_tile_bits.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(CSRC) $< -o $@
refine_tile_bits_test_san: refine_tile_bits_test.cpp $(CSRC)/hrt_refine_tile_bits.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o $@
clean:
	rm -f refine_tiles_demo refine_tile_bits_test refine_tile_bits_test_san
.PHONY: all clean
