# Test-only libraries of ed_keys_kernel (format 12, Solana), beside solana.mk; same flags.
#   libedkeysdev.so   driver of vg::launch_ed_keys over the product's own build/lib/device/kernels.o (the shipped code objects of
#                     ed_keys_kernel in both forms and of the compaction behind it, not a second compilation), on the table, the seeds,
#                     the counts and the ring the test chooses, with the product's host sources for the real table and the filter
#                     compiler (ed_keys_dev.hip; tests/test_gpu_ed_keys_kernel.py)
#   libedkeystest.so  host build (g++) of one lane's arithmetic on a caller's table (ed_keys_shim.cpp; tests/test_ed_keys_vectors.py)
# usage: make -C tests/native -f ed_keys.mk
CXX ?= g++
CXXFLAGS ?= -O2 -g -fPIC -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -I../../include
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../vgen_amd/csrc
HDRS := $(wildcard $(CSRC)/core/*.h $(CSRC)/host/*.h $(CSRC)/device/*.h)
HOST := $(CSRC)/host/host_ec.cpp $(CSRC)/host/encode.cpp $(CSRC)/host/regex_dfa.cpp $(CSRC)/host/filter.cpp $(CSRC)/host/pattern_info.cpp $(CSRC)/host/provider.cpp
LIBBUILD := ../../build/lib
HOOKBUILD := ../../build/hooks
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas -I../../include -Wno-pass-failed

all: libedkeystest.so libedkeysdev.so

libedkeystest.so: ed_keys_shim.cpp $(HOST) $(HDRS)
	$(CXX) $(CXXFLAGS) -shared -o $@.tmp ed_keys_shim.cpp $(HOST) -lpthread
	mv -f $@.tmp $@

# the product's objects come from the product's Makefile, which runs once per invocation of this one and always (see Makefile: product)
.PHONY: product
product:
	$(MAKE) -s -C $(CSRC)

$(LIBBUILD)/device/kernels.o: | product ;

$(HOOKBUILD)/ed_keys_dev.o: ed_keys_dev.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# (linked beside its name and renamed into place: a test of another pytest worker may load the library while this rule runs)
libedkeysdev.so: $(HOOKBUILD)/ed_keys_dev.o $(LIBBUILD)/device/kernels.o $(HOST)
	$(HIPCC) --offload-arch=gfx950 -O2 -std=c++17 -fPIC -I../../include -shared -o $@.tmp $^ -lpthread -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined
	mv -f $@.tmp $@

clean:
	rm -f libedkeystest.so libedkeysdev.so $(HOOKBUILD)/ed_keys_dev.o
