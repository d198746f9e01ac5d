# refine_demo: adaptive refinement through the C++ host mirror (include/hrt_app.hpp) against the in-tree
# libhip_raytrace.so; built by __graft_entry__.build() so that the GPU box runs the same binary
# (tests/test_gpu_refine.py).  Its hit array is a device buffer: it links the HIP runtime for
# hipMalloc / hipMemcpy / hipFree.  Run from this directory: make -f refine_demo.mk [clean]
ROOT := $(abspath ../..)
LIB := $(ROOT)/epq_raytracer_amd/lib
ROCM ?= /opt/rocm
CXX ?= g++
refine_demo: refine_demo.cpp $(ROOT)/include/hrt_app.hpp $(ROOT)/include/hip_raytrace.h $(ROOT)/include/hrt_host.h $(LIB)/libhip_raytrace.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(LIB) -lhip_raytrace -L$(ROCM)/lib -lamdhip64 \
		-Wl,-rpath,'$$ORIGIN/../../epq_raytracer_amd/lib' -Wl,-rpath,$(ROCM)/lib
clean:
	rm -f refine_demo
.PHONY: clean
