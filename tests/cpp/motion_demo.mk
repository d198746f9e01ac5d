# motion_demo: object motion in the temporal history through the C++ host mirror (include/hrt_app.hpp) against the
# in-tree libhip_raytrace.so; built by __graft_entry__.build() so that the GPU box runs the same binary
# (tests/test_gpu_motion.py).  motion_map_test: the HIP-free coordinate arithmetic
# (epq_raytracer_amd/csrc/hrt_motion_map.h) as a stand-alone program, plain and under ASan + UBSan
# (tests/test_motion_ref.py).  Run from this directory: make -f motion_demo.mk [clean]
ROOT := $(abspath ../..)
LIB := $(ROOT)/epq_raytracer_amd/lib
CSRC := $(ROOT)/epq_raytracer_amd/csrc
ROCM ?= /opt/rocm
CXX ?= g++
all: motion_demo motion_map_test motion_map_test_san
motion_demo: motion_demo.cpp $(ROOT)/include/hrt_app.hpp $(ROOT)/include/hip_raytrace.h $(ROOT)/include/hrt_host.h $(LIB)/libhip_raytrace.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(ROOT)/include $< -o $@ -L$(LIB) -lhip_raytrace -L$(ROCM)/lib -lamdhip64 \
		-Wl,-rpath,'$$ORIGIN/../../epq_raytracer_amd/lib' -Wl,-rpath,$(ROCM)/lib
motion_map_test: motion_map_test.cpp $(CSRC)/hrt_motion_map.h
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -I$(CSRC) $< -o $@
motion_map_test_san: motion_map_test.cpp $(CSRC)/hrt_motion_map.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I$(CSRC) $< -o $@
clean:
	rm -f motion_demo motion_map_test motion_map_test_san
.PHONY: all clean
