# resolve_demo: temporal upsampling through the C++ host mirror (include/hrt_app.hpp) against the in-tree
# libhip_raytrace.so; built by __graft_entry__.build() so that the GPU box runs the same binary
# (tests/test_gpu_resolve.py).  resolve_map_test: the HIP-free coordinate arithmetic
# (epq_raytracer_amd/csrc/hrt_resolve_map.h) as a stand-alone program, plain and under ASan + UBSan
# (tests/test_resolve_ref.py).  Run from this directory: make -f resolve_demo.mk [clean]
ROOT := $(abspath ../..)
LIB := $(ROOT)/epq_raytracer_amd/lib
CSRC := $(ROOT)/epq_raytracer_amd/csrc
ROCM ?= /opt/rocm
CXX ?= g++
all: resolve_demo resolve_map_test resolve_map_test_san
resolve_demo: resolve_demo.cpp $(ROOT)/include/hrt_app.hpp $(ROOT)/include/hip_raytrace.h $(ROOT)/include/hrt_host.h $(LIB)/libhip_raytrace.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(LIB) -lhip_raytrace -L$(ROCM)/lib -lamdhip64 \
		-Wl,-rpath,'$$ORIGIN/../../epq_raytracer_amd/lib' -Wl,-rpath,$(ROCM)/lib
resolve_map_test: resolve_map_test.cpp $(CSRC)/hrt_resolve_map.h $(CSRC)/hrt_upsample_map.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -I$(CSRC) $< -o $@
resolve_map_test_san: resolve_map_test.cpp $(CSRC)/hrt_resolve_map.h $(CSRC)/hrt_upsample_map.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o $@
clean:
	rm -f resolve_demo resolve_map_test resolve_map_test_san
.PHONY: all clean
