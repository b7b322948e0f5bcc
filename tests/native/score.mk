# Test-only driver of vg::launch_payload_score over the product's own build/lib/device/kernels.o (the shipped code objects of the score
# kernel and the compaction behind it, not a second compilation), on payloads the test crafts: tests/test_gpu_score_kernels.py.
# A makefile of its own beside the Makefile of the older test libraries; same flags.  usage: make -C tests/native -f score.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../vgen_amd/csrc
HDRS := $(wildcard $(CSRC)/core/*.h $(CSRC)/host/*.h $(CSRC)/device/*.h)
LIBBUILD := ../../build/lib
HOOKBUILD := ../../build/hooks
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas -I../../include -Wno-pass-failed

all: libscoredev.so

# the product's objects come from the product's Makefile, which runs once per invocation of this one and always (see Makefile: product)
.PHONY: product
product:
	$(MAKE) -s -C $(CSRC)

$(LIBBUILD)/device/kernels.o: | product ;

$(HOOKBUILD)/score_dev.o: score_dev.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# (linked beside its name and renamed into place: a test of another pytest worker may load the library while this rule runs)
libscoredev.so: $(HOOKBUILD)/score_dev.o $(LIBBUILD)/device/kernels.o
	$(HIPCC) --offload-arch=gfx950 -shared -o $@.tmp $^ -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined
	mv -f $@.tmp $@

clean:
	rm -f libscoredev.so $(HOOKBUILD)/score_dev.o
