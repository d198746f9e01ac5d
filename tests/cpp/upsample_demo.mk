# upsample_demo: guided upsampling through the C++ host mirror (include/hrt_app.hpp) against the in-tree
# libhip_raytrace.so; built by __graft_entry__.build() so that the GPU box runs the same binary
# (tests/test_gpu_upsample.py).  Its hit arrays and target are device buffers: it links the HIP runtime for
# hipMalloc / hipMemcpy / hipFree.  upsample_map_test: the HIP-free coordinate arithmetic
# (epq_raytracer_amd/csrc/hrt_upsample_map.h) as a stand-alone program, plain and under ASan + UBSan
# (tests/test_upsample_ref.py).  Run from this directory: make -f upsample_demo.mk [clean]
ROOT := $(abspath ../..)
LIB := $(ROOT)/epq_raytracer_amd/lib
CSRC := $(ROOT)/epq_raytracer_amd/csrc
ROCM ?= /opt/rocm
CXX ?= g++
all: upsample_demo upsample_map_test upsample_map_test_san
upsample_demo: upsample_demo.cpp $(ROOT)/include/hrt_app.hpp $(ROOT)/include/hip_raytrace.h $(ROOT)/include/hrt_host.h $(LIB)/libhip_raytrace.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(LIB) -lhip_raytrace -L$(ROCM)/lib -lamdhip64 \
		-Wl,-rpath,'$$ORIGIN/../../epq_raytracer_amd/lib' -Wl,-rpath,$(ROCM)/lib
upsample_map_test: upsample_map_test.cpp $(CSRC)/hrt_upsample_map.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -I$(CSRC) $< -o $@
upsample_map_test_san: upsample_map_test.cpp $(CSRC)/hrt_upsample_map.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o $@
clean:
	rm -f upsample_demo upsample_map_test upsample_map_test_san
.PHONY: all clean
