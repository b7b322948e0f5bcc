# Test-only libraries of the Nostr format (x-only keys), beside the Makefile of the older test libraries; same flags.
#   libnostrtest.so  host build (g++) of what the kernels evaluate for the format - core/filter_eval.h filter_eval_npub, core/dfa_eval.h
#                    dfa_match_npub - over the product's host sources (nostr_shim.cpp; tests/test_nostr.py)
#   libvgen_fake_nostr.so  the host scan loop (scanner.cpp, cabi.cpp) over the CPU stand-in of the runtime with Nostr contexts added
#                    (nostr_rt.cpp, which includes fake_rt.cpp as it is): the C ABI without a device (tests/test_nostr_scan_host.py)
#   libxonlydev.so   driver of vg::launch_seq_fwd / vg::launch_seq_bwd for the format over the product's own build/lib/device/kernels.o
#                    (the shipped code objects, not a second compilation), on crafted offset tables (xonly_dev.hip; tests/test_gpu_nostr.py)
# usage: make -C tests/native -f nostr.mk
CXX ?= g++
CXXFLAGS ?= -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -I../../include
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../vgen_amd/csrc
HDRS := $(wildcard $(CSRC)/core/*.h $(CSRC)/host/*.h $(CSRC)/device/*.h)
HOST := $(CSRC)/host/host_ec.cpp $(CSRC)/host/encode.cpp $(CSRC)/host/regex_dfa.cpp $(CSRC)/host/filter.cpp $(CSRC)/host/pattern_info.cpp $(CSRC)/host/provider.cpp
LIBBUILD := ../../build/lib
HOOKBUILD := ../../build/hooks
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas -I../../include -Wno-pass-failed

all: libnostrtest.so libvgen_fake_nostr.so libxonlydev.so

# the product's objects come from the product's Makefile, which runs once per invocation of this one and always (see Makefile: product)
.PHONY: product
product:
	$(MAKE) -s -C $(CSRC)

$(LIBBUILD)/device/kernels.o: | product ;

libnostrtest.so: nostr_shim.cpp $(HOST) $(HDRS)
	$(CXX) $(CXXFLAGS) -shared -o $@.tmp nostr_shim.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

FAKE_FLAGS := -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -Wno-unused-parameter -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include

libvgen_fake_nostr.so: nostr_rt.cpp fake_rt.cpp $(CSRC)/scanner.cpp $(CSRC)/cabi.cpp $(HOST) $(HDRS) $(CSRC)/runtime.h
	$(CXX) $(FAKE_FLAGS) -shared -o $@.tmp nostr_rt.cpp $(CSRC)/scanner.cpp $(CSRC)/cabi.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

$(HOOKBUILD)/xonly_dev.o: xonly_dev.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# (linked beside its name and renamed into place: a test of another pytest worker may load the library while this rule runs)
libxonlydev.so: $(HOOKBUILD)/xonly_dev.o $(LIBBUILD)/device/kernels.o
	$(HIPCC) --offload-arch=gfx950 -shared -o $@.tmp $^ -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined
	mv -f $@.tmp $@

clean:
	rm -f libnostrtest.so libvgen_fake_nostr.so libxonlydev.so $(HOOKBUILD)/xonly_dev.o
