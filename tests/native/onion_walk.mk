# Test-only driver of vg::launch_onion_points / vg::launch_onion over the product's own build/lib/device/kernels.o (the shipped code
# objects of the onion walk's kernels and the compaction behind them, not a second compilation), on lane counts, lane tables, shared
# points and a zero slot the test chooses: tests/test_gpu_onion_kernels.py.
# A makefile of its own beside onion.mk, as score.mk is beside the Makefile; same flags.  usage: make -C tests/native -f onion_walk.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../vgen_amd/csrc
HDRS := $(wildcard $(CSRC)/core/*.h $(CSRC)/host/*.h $(CSRC)/device/*.h)
LIBBUILD := ../../build/lib
HOOKBUILD := ../../build/hooks
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas -I../../include -Wno-pass-failed

all: libonionwalkdev.so

# the product's objects come from the product's Makefile, which runs once per invocation of this one and always (see Makefile: product)
.PHONY: product
product:
	$(MAKE) -s -C $(CSRC)

$(LIBBUILD)/device/kernels.o: | product ;

$(HOOKBUILD)/onion_walk_dev.o: onion_walk_dev.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# (linked beside its name and renamed into place: a test of another pytest worker may load the library while this rule runs)
libonionwalkdev.so: $(HOOKBUILD)/onion_walk_dev.o $(LIBBUILD)/device/kernels.o
	$(HIPCC) --offload-arch=gfx950 -shared -o $@.tmp $^ -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined
	mv -f $@.tmp $@

clean:
	rm -f libonionwalkdev.so $(HOOKBUILD)/onion_walk_dev.o
