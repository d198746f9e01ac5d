# radiance_demo: radiance queries through the C++ host mirror (include/hrt_app.hpp) against the in-tree
# libhip_raytrace.so; built by __graft_entry__.build() so that the GPU box runs the same binary
# (tests/test_gpu_radiance.py).  Run from this directory: make -f radiance_demo.mk [clean]
ROOT := $(abspath ../..)
LIB := $(ROOT)/epq_raytracer_amd/lib
CXX ?= g++
radiance_demo: radiance_demo.cpp $(ROOT)/include/hrt_app.hpp $(ROOT)/include/hip_raytrace.h $(ROOT)/include/hrt_host.h $(LIB)/libhip_raytrace.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(LIB) -lhip_raytrace -Wl,-rpath,'$$ORIGIN/../../epq_raytracer_amd/lib'
clean:
	rm -f radiance_demo
.PHONY: clean
