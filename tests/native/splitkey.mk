# Test-only libraries of the split-key search, beside the Makefile of the older test libraries; same flags.
#   libsplitkeytest.so     host build (g++) of vg::host_seq_points with a base point over the product's host sources
#                          (splitkey_shim.cpp; tests/test_splitkey.py)
#   libvgen_fake_split.so  the host scan loop (scanner.cpp, cabi.cpp) over the CPU stand-in of the runtime with split-key dispatches
#                          added (splitkey_rt.cpp, which includes fake_rt.cpp as it is): the C ABI without a device
#                          (tests/test_splitkey_scan_host.py)
# usage: make -C tests/native -f splitkey.mk
CXX ?= g++
CXXFLAGS ?= -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -I../../include
CSRC := ../../vgen_amd/csrc
HDRS := $(wildcard $(CSRC)/core/*.h $(CSRC)/host/*.h $(CSRC)/device/*.h)
HOST := $(CSRC)/host/host_ec.cpp $(CSRC)/host/encode.cpp $(CSRC)/host/regex_dfa.cpp $(CSRC)/host/filter.cpp $(CSRC)/host/pattern_info.cpp $(CSRC)/host/provider.cpp

all: libsplitkeytest.so libvgen_fake_split.so

# (linked beside its name and renamed into place: a test of another pytest worker may load the library while this rule runs)
libsplitkeytest.so: splitkey_shim.cpp $(HOST) $(HDRS)
	$(CXX) $(CXXFLAGS) -shared -o $@.tmp splitkey_shim.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

FAKE_FLAGS := -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -Wno-unused-parameter -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include

libvgen_fake_split.so: splitkey_rt.cpp fake_rt.cpp $(CSRC)/scanner.cpp $(CSRC)/cabi.cpp $(HOST) $(HDRS) $(CSRC)/runtime.h
	$(CXX) $(FAKE_FLAGS) -shared -o $@.tmp splitkey_rt.cpp $(CSRC)/scanner.cpp $(CSRC)/cabi.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

clean:
	rm -f libsplitkeytest.so libvgen_fake_split.so
