# Builds the MI355X engine (narwhal_amd/libnarwhal_amd.so, gfx950 only), the CPU oracle
# (test infrastructure) and the host check libraries of the kernels' arithmetic, of the wire
# decoder, of the message jobs' staging layout and of a verify_batch call, and the gfx950 harness of the arithmetic on
# raw limbs (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Iinclude -Inarwhal_amd/csrc -Wall -Wno-unused-function
CSRC := narwhal_amd/csrc
HDRS := $(wildcard $(CSRC)/*.hpp) $(CSRC)/nw_kernels.h $(CSRC)/nw_runtime.h $(CSRC)/nw_host.h include/narwhal_amd.h
LIB := narwhal_amd/libnarwhal_amd.so
BUILD := build

all: $(LIB) oracle hostcheck lpcheck wirecheck stagecheck batchcheck loadgen

$(BUILD)/nw_kernels.o: $(CSRC)/nw_kernels.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/nw_batch.o: $(CSRC)/nw_batch.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/nw_cert.o: $(CSRC)/nw_cert.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/nw_small.o: $(CSRC)/nw_small.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/nw_wiredev.o: $(CSRC)/nw_wire.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/nw_jobs.o: $(CSRC)/nw_jobs.cpp $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(BUILD)/nw_wire.o: $(CSRC)/nw_wire.cpp $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(BUILD)/nw_service.o: $(CSRC)/nw_service.cpp $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(BUILD)/nw_host.o: $(CSRC)/nw_host.cpp $(CSRC)/nw_host.h $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(BUILD)/nw_api.o: $(CSRC)/nw_api.cpp $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(LIB): $(BUILD)/nw_kernels.o $(BUILD)/nw_batch.o $(BUILD)/nw_cert.o $(BUILD)/nw_small.o $(BUILD)/nw_wiredev.o $(BUILD)/nw_api.o $(BUILD)/nw_jobs.o $(BUILD)/nw_wire.o $(BUILD)/nw_service.o $(BUILD)/nw_host.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

oracle:
	$(MAKE) -s -C oracle

hostcheck: tools/libnw_hostcheck.so
tools/libnw_hostcheck.so: tools/hostcheck.hip tools/limb_ops.hpp tools/sc_ops.hpp $(HDRS)
	$(HIPCC) --cuda-host-only -O2 -std=c++17 -fPIC -shared -Iinclude $< -o $@

# the per-lane field / point routines and the limb-parallel ones (nw_lp.hpp) as gfx950 kernels
# over raw limbs (tests/test_gpu_field_limbs.py); a library of its own, not linked into $(LIB)
lpcheck: tools/libnw_lpcheck.so
tools/libnw_lpcheck.so: tools/lpcheck.hip tools/limb_ops.hpp tools/sc_ops.hpp $(HDRS)
	$(HIPCC) -O3 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -Iinclude -Wall -Wno-unused-function $< -o $@

# the device wire decoder (nw_wiredec.hpp) and the host placement (nw_wireplace.hpp) compiled for
# the CPU (tests/test_wire_device_cpu.py, test_wire_canon_cpu.py, test_wire_place_cpu.py)
wirecheck: tools/libnw_wirecheck.so
tools/libnw_wirecheck.so: tools/wirecheck.hip tools/wire_single.hpp $(CSRC)/nw_wiredec.hpp $(CSRC)/nw_wireplace.hpp
	$(HIPCC) --cuda-host-only -O2 -std=c++17 -fPIC -shared -Iinclude $< -o $@

# the same decoder text under AddressSanitizer / UBSan over generated and mutated frames, as a
# stand-alone CPU program (not part of `all`): make wiresan && tools/wire_canon_san
wiresan: tools/wire_canon_san
tools/wire_canon_san: tools/wire_canon_san.cpp tools/wire_single.hpp $(CSRC)/nw_wiredec.hpp
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# the message jobs' staging layout (nw_stage.hpp) over malloc'ed buffers (tests/test_stage_cpu.py)
stagecheck: tools/libnw_stagecheck.so
tools/libnw_stagecheck.so: tools/stagecheck.hip $(CSRC)/nw_stage.hpp include/narwhal_amd.h
	$(HIPCC) --cuda-host-only -O2 -std=c++17 -fPIC -shared -Iinclude $< -o $@

# the same file with its main under AddressSanitizer / UBSan, as a stand-alone CPU program (not
# part of `all`): make stagesan && tools/stage_san
stagesan: tools/stage_san
tools/stage_san: tools/stagecheck.hip $(CSRC)/nw_stage.hpp include/narwhal_amd.h
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DSTAGECHECK_MAIN -Iinclude -x c++ $< -o $@

# a verify_batch call's refusal rules (nw_batch_call.hpp), the batch job's section plan and the
# packing of per-item messages (nw_stage.hpp) for the CPU (tests/test_batch_call_cpu.py), and the
# same file with its main under AddressSanitizer / UBSan (not part of `all`):
# make batchsan && tools/batch_san
batchcheck: tools/libnw_batchcheck.so
BATCHCHECK_DEPS := tools/batchcheck.hip $(CSRC)/nw_batch_call.hpp $(CSRC)/nw_stage.hpp include/narwhal_amd.h
tools/libnw_batchcheck.so: $(BATCHCHECK_DEPS)
	$(HIPCC) --cuda-host-only -O2 -std=c++17 -fPIC -shared -Iinclude $< -o $@
batchsan: tools/batch_san
tools/batch_san: $(BATCHCHECK_DEPS)
	$(HIPCC) --cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DBATCHCHECK_MAIN -Iinclude $< -o $@

# the key set's sizing, region planning and probe / build / triage / ladder sequence, and the
# registered signers' hash table and one slice through it (nw_kernels.h, nw_strict.hpp;
# tools/hostcheck.hip's main) under AddressSanitizer / UBSan, as a stand-alone CPU program
# (not part of `all`; the instrumented field arithmetic takes about ten minutes to compile):
# make keysetsan && tools/keyset_san
keysetsan: tools/keyset_san
tools/keyset_san: tools/hostcheck.hip $(HDRS)
	$(HIPCC) --cuda-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DKEYSET_SAN_MAIN -Iinclude $< -o $@

# the lane function that hashes R || A || M for the strict launch over messages of any length
# (nw_sha512.hpp sha512_hram_lane) compiled for the CPU under AddressSanitizer / UBSan, as a
# stand-alone program (not part of `all`; tests/test_sha512_hram_cpu.py builds and runs it)
CLANGXX ?= /opt/rocm/llvm/bin/clang++
hramsan: tools/hram_lane_san
tools/hram_lane_san: tools/hram_lane_san.cpp tools/hram_san/hip/hip_runtime.h $(CSRC)/nw_sha512.hpp $(CSRC)/nw_field.hpp
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/hram_san -I$(CSRC) $< -o $@

# the same routine's 32-byte-prefix instance (sha512_prefix_lane<8>: prefix || M, the hash behind
# r of signing over messages of any length), built the same way (not part of `all`;
# tests/test_sha512_prefix_cpu.py builds and runs it)
prefixsan: tools/prefix_lane_san
tools/prefix_lane_san: tools/prefix_lane_san.cpp tools/hram_san/hip/hip_runtime.h $(CSRC)/nw_sha512.hpp $(CSRC)/nw_field.hpp
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/hram_san -I$(CSRC) $< -o $@

loadgen: tools/libnw_loadgen.so
tools/libnw_loadgen.so: tools/nw_loadgen.cpp include/narwhal_amd.h $(LIB)
	g++ -O2 -std=c++17 -fPIC -shared -Iinclude $< -o $@ -Lnarwhal_amd -lnarwhal_amd -Wl,-rpath,'$$ORIGIN/../narwhal_amd' -pthread

# CPU harness of the service's host logic over test doubles of the device entry points
# (tests/test_service_stress.py); _tsan: the same under ThreadSanitizer
STRESS_FLAGS := -std=c++17 -pthread -D__HIP_PLATFORM_AMD__ -Iinclude -I$(CSRC) -I/opt/rocm/include
stress: tools/service_stress tools/service_stress_tsan
tools/service_stress: tools/service_stress.cpp $(CSRC)/nw_service.cpp $(HDRS)
	g++ -O2 $(STRESS_FLAGS) tools/service_stress.cpp $(CSRC)/nw_service.cpp -o $@
tools/service_stress_tsan: tools/service_stress.cpp $(CSRC)/nw_service.cpp $(HDRS)
	g++ -O1 -g -fsanitize=thread -DNW_SERVICE_SYSTEM_CLOCK_WAIT $(STRESS_FLAGS) tools/service_stress.cpp $(CSRC)/nw_service.cpp -o $@

ubench: tools/ubench_valu
tools/ubench_valu: tools/ubench_valu.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 $< -o $@

clean:
	rm -rf $(BUILD) $(LIB) tools/libnw_hostcheck.so tools/libnw_lpcheck.so tools/libnw_wirecheck.so tools/libnw_stagecheck.so tools/libnw_batchcheck.so tools/libnw_loadgen.so tools/service_stress tools/service_stress_tsan tools/wire_canon_san tools/stage_san tools/batch_san tools/keyset_san tools/hram_lane_san tools/prefix_lane_san
	$(MAKE) -s -C oracle clean

.PHONY: all oracle hostcheck lpcheck wirecheck stagecheck batchcheck batchsan wiresan stagesan keysetsan hramsan prefixsan loadgen stress ubench clean
