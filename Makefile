# Builds libtmr.so (gfx950) in-tree.  `python __graft_entry__.py build` drives this too.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
BUILD := build
LIB := tmrnet_amd/libtmr.so
SRC := $(wildcard tmrnet_amd/csrc/*.hip) tmrnet_amd/csrc/api.cpp tmrnet_amd/csrc/jpeg_host.cpp
OBJ := $(patsubst tmrnet_amd/csrc/%,$(BUILD)/%.o,$(SRC))
CFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Iinclude -Itmrnet_amd/csrc -munsafe-fp-atomics \
          $(EXTRA)

$(LIB): $(OBJ)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJ)

# header dependencies from the compiler (-MMD: build/*.d); an edit of the LDS-DMA engine
# (gemm16_kernel.h) rebuilds only the gemm16_<view>_<prec>.hip units
$(BUILD)/%.hip.o: tmrnet_amd/csrc/%.hip
	@mkdir -p $(BUILD)
	$(HIPCC) $(CFLAGS) -MMD -MP -c $< -o $@

$(BUILD)/%.cpp.o: tmrnet_amd/csrc/%.cpp
	@mkdir -p $(BUILD)
	$(HIPCC) $(CFLAGS) -MMD -MP -c $< -o $@

# the JPEG entropy decoder is host code only: plain C++, no device pass
$(BUILD)/jpeg_host.cpp.o: tmrnet_amd/csrc/jpeg_host.cpp
	@mkdir -p $(BUILD)
	$(HIPCC) -x c++ -O3 -std=c++17 -fPIC -Iinclude -MMD -MP -c $< -o $@

-include $(OBJ:.o=.d)

clean:
	rm -rf build tmrnet_amd/libtmr.so
.PHONY: clean
