# The body of a companion library's Makefile (../framing, ../multi): libsnappy_mi355x_$(LIB).so
# (gfx950 only) next to the package, linking libsnappy_mi355x.so by name (found beside it through
# $ORIGIN; ../Makefile builds it first).  The including Makefile sets LIB, PFX (the sources' and
# the ABI's prefix), VERSION_MACRO, SRCS, HOSTSRCS and its own HDRS; optionally LINK, the further
# companions it links by name (../blocks: multi), which their own Makefiles build first, and
# CHECK_EXTRA, other libraries' host-only files that its own host-only file calls into (../kafka).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
MK = ../common/companion.mk
HDRS += ../common/smc_layout.h ../common/smc_slots.h ../common/smc_device.h ../common/smc_hip_host.h ../common/smc_staging.h \
        ../../../include/snappy_mi355x.h
# the version: a hash of the sources, headers, Makefiles, target and compiler (as ../Makefile)
VERSION ?= src-$(shell (cat $(SRCS) $(HOSTSRCS) $(HDRS) Makefile $(MK); echo '$(EXTRA) $(ARCH)'; $(HIPCC) --version) 2>/dev/null | sha1sum | cut -c1-10)
EXTRA ?=
BASE = --offload-arch=$(ARCH) -O3 -std=c++17 -fno-strict-aliasing -fPIC -Wall $(EXTRA)
MAIN = ../../libsnappy_mi355x.so
LINK ?=
CHECK_EXTRA ?=
OUT ?= ../../libsnappy_mi355x_$(LIB).so
OBJ ?= build
OBJS = $(patsubst %.hip,$(OBJ)/%.o,$(SRCS)) $(patsubst %.cpp,$(OBJ)/%.o,$(HOSTSRCS))
CHECK = $(PFX)_host_check

all: $(OUT)

# the version string lives in $(PFX)_api.o only (a stamp that changes with the source hash rebuilds it)
$(OBJ)/version.stamp: FORCE
	@mkdir -p $(OBJ)
	@echo '$(VERSION)' | cmp -s - $@ || echo '$(VERSION)' > $@

$(OBJ)/$(PFX)_api.o: $(PFX)_api.hip $(HDRS) Makefile $(MK) $(OBJ)/version.stamp
	@mkdir -p $(OBJ)
	$(HIPCC) $(BASE) -D$(VERSION_MACRO)='"$(VERSION)"' -c -o $@ $<

$(OBJ)/%.o: %.hip $(HDRS) Makefile $(MK)
	@mkdir -p $(OBJ)
	$(HIPCC) $(BASE) -c -o $@ $<

# host only: no HIP in it (it also builds alone, see host_check)
$(OBJ)/%.o: %.cpp $(HDRS) Makefile $(MK)
	@mkdir -p $(OBJ)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -c -o $@ $<

$(OUT): $(OBJS) $(MAIN) $(LINK:%=../../libsnappy_mi355x_%.so)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJS) -L../.. $(LINK:%=-l:libsnappy_mi355x_%.so) -l:libsnappy_mi355x.so -Wl,-rpath,'$$ORIGIN'

# The host-only file and its stand-alone driver under AddressSanitizer and UBSan (CPU only;
# nothing here touches a device).
host_check: $(OBJ)/$(CHECK)
	$(OBJ)/$(CHECK)

$(OBJ)/$(CHECK): $(CHECK).cpp $(HOSTSRCS) $(CHECK_EXTRA) $(HDRS) Makefile $(MK)
	@mkdir -p $(OBJ)
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(CHECK).cpp $(HOSTSRCS) $(CHECK_EXTRA)

clean:
	rm -rf $(OUT) $(OBJ)

.PHONY: all clean host_check FORCE
FORCE:
