# Test-only libraries of the onion format (Tor v3, the Ed25519 walk), beside the Makefile of the older test libraries; same flags.
#   libonniontest.so       host build (g++) of what the kernels evaluate for the format - core/ed_walk.h and core/filter_eval.h
#                          filter_eval_onion - over the product's host sources (onion_shim.cpp; tests/test_onion.py)
#   libvgen_fake_onion.so  the host scan loop (scanner.cpp, cabi.cpp) over the CPU stand-in of the runtime with onion contexts added
#                          (onion_rt.cpp, which includes fake_rt.cpp as it is): the C ABI without a device (tests/test_onion_scan_host.py)
#   onion_selftest         a stand-alone program over the same host sources built with -fsanitize=address,undefined (onion_selftest.cpp)
#   libonniondev.so        device build (hipcc, gfx950) of the format's single-source core functions, one input per lane, with the product's
#                          host sources for the filter compiler (onion_dev.hip; tests/test_gpu_onion.py)
# usage: make -C tests/native -f onion.mk
CXX ?= g++
CXXFLAGS ?= -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -I../../include
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../vgen_amd/csrc
HDRS := $(wildcard $(CSRC)/core/*.h $(CSRC)/host/*.h $(CSRC)/device/*.h)
HOST := $(CSRC)/host/host_ec.cpp $(CSRC)/host/encode.cpp $(CSRC)/host/regex_dfa.cpp $(CSRC)/host/filter.cpp $(CSRC)/host/pattern_info.cpp $(CSRC)/host/provider.cpp
HOOKBUILD := ../../build/hooks
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas -I../../include -Wno-pass-failed

all: libonniontest.so libvgen_fake_onion.so onion_selftest libonniondev.so

libonniontest.so: onion_shim.cpp $(HOST) $(HDRS)
	$(CXX) $(CXXFLAGS) -shared -o $@.tmp onion_shim.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

FAKE_FLAGS := -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -Wno-unused-parameter -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include

libvgen_fake_onion.so: onion_rt.cpp fake_rt.cpp $(CSRC)/scanner.cpp $(CSRC)/cabi.cpp $(HOST) $(HDRS) $(CSRC)/runtime.h
	$(CXX) $(FAKE_FLAGS) -shared -o $@.tmp onion_rt.cpp $(CSRC)/scanner.cpp $(CSRC)/cabi.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

onion_selftest: onion_selftest.cpp $(HOST) $(HDRS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -I../../include -fsanitize=address,undefined -fno-sanitize-recover=all -o $@.tmp onion_selftest.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

$(HOOKBUILD)/onion_dev.o: onion_dev.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# (linked beside its name and renamed into place: a test of another pytest worker may load the library while this rule runs)
libonniondev.so: $(HOOKBUILD)/onion_dev.o $(HOST)
	$(HIPCC) --offload-arch=gfx950 -O2 -std=c++17 -fPIC -I../../include -shared -o $@.tmp $^ -lpthread -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined
	mv -f $@.tmp $@

clean:
	rm -f libonniontest.so libvgen_fake_onion.so onion_selftest libonniondev.so $(HOOKBUILD)/onion_dev.o
