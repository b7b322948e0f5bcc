# Test-only libraries of the key loop's forms of core/fe.h (LEAN products with an addend), beside the Makefile of the
# older test libraries.
#   libleantest.so  host build (g++) of the header (leanmul_shim.cpp; tests/test_leanmul.py)
#   libleandev.so   its device build, one input per lane (leanmul_dev.hip; tests/test_gpu_leanmul.py)
# usage: make -C tests/native -f leanmul.mk
CXX ?= g++
CXXFLAGS ?= -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -I../../include
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../vgen_amd/csrc
HDRS := $(wildcard $(CSRC)/core/*.h)

all: libleantest.so libleandev.so

# (written beside their names and renamed into place: a test of another pytest worker may load a library while its rule runs)
libleantest.so: leanmul_shim.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -shared -o $@.tmp leanmul_shim.cpp
	mv -f $@.tmp $@

libleandev.so: leanmul_dev.hip $(HDRS)
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-pass-failed -o $@.tmp leanmul_dev.hip -Wl,-rpath,/opt/rocm/lib
	mv -f $@.tmp $@

clean:
	rm -f libleantest.so libleandev.so
