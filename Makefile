# Build of liblpcnet_mi355x.so (gfx950) and the CPU checker under oracle/.
#
#   make            -> lpcnet_amd/liblpcnet_mi355x.so + oracle/ libraries
#   make lib        -> the product library only
#   make check      -> builds and runs tools/model_host_check,
#                      tools/pool_combiner_check, tools/conceal_plan_check,
#                      tools/device_mem_check and tools/feat_host_check
#                      (CPU only)
#
# Every translation unit is compiled with -ffp-contract=off: the engine is
# bit-exact with the reference x86 build only without FMA contraction.

HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
JOBS ?= 4
BUILD := build
LIB := lpcnet_amd/liblpcnet_mi355x.so
CSRC := lpcnet_amd/csrc
HDRS := include/lpcnet.h include/lpcnet_mi355x.h $(CSRC)/lpcnet_engine.h $(CSRC)/side_kernels.h $(CSRC)/device_math.h $(CSRC)/sampler.h $(CSRC)/lds_flags.h $(CSRC)/mf_common.h $(CSRC)/gru_tile.h $(CSRC)/l2_warm.h $(CSRC)/pow10_dd.h $(CSRC)/lpc_stages.h $(CSRC)/rcp_table_x86.inc $(CSRC)/mf_plan.h $(CSRC)/model_host.h $(CSRC)/side_tables.h $(CSRC)/device_mem.h $(CSRC)/batch.h $(CSRC)/pool_combiner.h $(CSRC)/kernel_choice.h $(CSRC)/conceal_plan.h
EXTRA ?=
COMMON := $(EXTRA) -O3 -fPIC -ffp-contract=off -fno-fast-math -std=c++17 -Iinclude -I$(CSRC) -fvisibility=hidden -Wall -Wno-unused-function
OBJS := $(BUILD)/kernels.o $(BUILD)/mf_kernel.o $(BUILD)/mf2_kernel.o $(BUILD)/fp_kernel.o $(BUILD)/selftest.o $(BUILD)/frame_kernel.o $(BUILD)/engine.o $(BUILD)/device_mem.o $(BUILD)/synth_steps.o $(BUILD)/lpc_kernel.o $(BUILD)/chunk_kernel.o $(BUILD)/model_gen.o $(BUILD)/host_rcpps.o $(BUILD)/decode_kernel.o $(BUILD)/mfw_kernel.o $(BUILD)/plc_kernel.o $(BUILD)/rdovae_kernel.o $(BUILD)/feat_kernel.o $(BUILD)/burg_kernel.o $(BUILD)/enc_kernel.o $(BUILD)/mf_plan.o $(BUILD)/model_host.o $(BUILD)/dropin.o $(BUILD)/pool_combiner.o $(BUILD)/kernel_choice.o $(BUILD)/side_tables.o $(BUILD)/side_calls.o $(BUILD)/conceal_kernel.o $(BUILD)/conceal_calls.o $(BUILD)/conceal_plan.o

SYNTH := tools/lpcnet_synth
DROPIN := tools/dropin_bench

all: lib synth dropin hostcheck oracle

lib: $(LIB)

# file-driven C caller of include/lpcnet.h (lpcnet_demo -synthesis equivalent):
# plain C99 against the public header only, linked to the in-tree library
synth: $(SYNTH)

$(SYNTH): tools/lpcnet_synth.c include/lpcnet.h $(LIB)
	$(CC) -std=c99 -O2 -Wall -Wextra -pedantic -Werror -Iinclude -o $@ $< -Llpcnet_amd -llpcnet_mi355x -Wl,-rpath,'$$ORIGIN/../lpcnet_amd'

# pthread C driver of the drop-in API (many handles at once) against the batch API
dropin: $(DROPIN)

$(DROPIN): tools/dropin_bench.c include/lpcnet.h include/lpcnet_mi355x.h $(LIB)
	$(CC) -std=c99 -O2 -Wall -Wextra -Werror -Iinclude -o $@ $< -Llpcnet_amd -llpcnet_mi355x -lpthread -Wl,-rpath,'$$ORIGIN/../lpcnet_amd'

$(BUILD):
	mkdir -p $(BUILD)

# The objects hipcc compiles, all with one command line: the kernels (.hip),
# the batch (engine.cpp), the HIP backend of its memory owners
# (device_mem.cpp), its synthesis and decode calls and their launches
# (synth_steps.cpp), the drop-in single-stream API over them (dropin.cpp), the
# PLC, feature, Burg, encoder and LPC calls beside synthesis (side_calls.cpp),
# the concealment machine (conceal_calls.cpp) and the host-only GRU_A planner,
# blob -> HostModel ingest and side tables (mf_plan, model_host, side_tables).
# feat_kernel, burg_kernel and enc_kernel share lpc_kernel's stages
# (lpc_stages.h) and so its flags: one contracted a*b+c in the Burg recursion
# changes the output.
# XFLAGS: what single objects add, below.
HIPCC_O = $(HIPCC) -x hip --offload-arch=$(ARCH) $(COMMON) $(XFLAGS) -c $< -o $@

$(BUILD)/%.o: $(CSRC)/%.hip $(HDRS) | $(BUILD)
	$(HIPCC_O)

$(BUILD)/%.o: $(CSRC)/%.cpp $(HDRS) | $(BUILD)
	$(HIPCC_O)

# no SLP vectorisation: packed f32 ops cost the shared SIMDs more than scalar pairs
$(BUILD)/mf_kernel.o $(BUILD)/mf2_kernel.o $(BUILD)/mfw_kernel.o: XFLAGS := -fno-slp-vectorize

# the fp32 chains schedule better under the max-ILP machine scheduler (batch-1 fp32 +0.6 %)
$(BUILD)/fp_kernel.o: XFLAGS := -mllvm -amdgpu-sched-strategy=max-ilp

# host-only: the CPU's own rcpps (x86 SSE), system compiler
$(BUILD)/host_rcpps.o: $(CSRC)/host_rcpps.cpp include/lpcnet_mi355x.h | $(BUILD)
	$(CXX) -O2 -fPIC -msse2 -ffp-contract=off -std=c++17 -Iinclude -fvisibility=hidden -Wall -c $< -o $@

# host-only: the drop-in pools' flat combiner (futex hand-offs, no device
# call), system compiler
$(BUILD)/pool_combiner.o: $(CSRC)/pool_combiner.cpp $(CSRC)/pool_combiner.h | $(BUILD)
	$(CXX) -O2 -fPIC -ffp-contract=off -std=c++17 -Iinclude -fvisibility=hidden -Wall -c $< -o $@

# host-only: which sample kernel and frame path a batch, launch or call takes
# (no device call, no HIP include), system compiler
$(BUILD)/kernel_choice.o: $(CSRC)/kernel_choice.cpp $(CSRC)/kernel_choice.h | $(BUILD)
	$(CXX) -O2 -fPIC -ffp-contract=off -std=c++17 -Iinclude -fvisibility=hidden -Wall -c $< -o $@

# host-only: the concealment machine's planner (no device call, no HIP
# include), system compiler
$(BUILD)/conceal_plan.o: $(CSRC)/conceal_plan.cpp $(CSRC)/conceal_plan.h | $(BUILD)
	$(CXX) -O2 -fPIC -ffp-contract=off -std=c++17 -Iinclude -fvisibility=hidden -Wall -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -lpthread

# stand-alone CPU check of the model tables over the host-only objects
# (tools/model_host_check.cpp gives the sanitizer recipe)
HOSTCHECK := tools/model_host_check

$(BUILD)/model_host_check.o: tools/model_host_check.cpp $(HDRS) | $(BUILD)
	$(HIPCC_O)

$(HOSTCHECK): $(BUILD)/model_host_check.o $(BUILD)/model_host.o $(BUILD)/side_tables.o $(BUILD)/mf_plan.o $(BUILD)/model_gen.o $(BUILD)/host_rcpps.o
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^

# stand-alone CPU check of the flat combiner with a fake launch
# (tools/pool_combiner_check.cpp gives the sanitizer recipes)
POOLCHECK := tools/pool_combiner_check

$(POOLCHECK): tools/pool_combiner_check.cpp $(BUILD)/pool_combiner.o $(CSRC)/pool_combiner.h
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $< $(BUILD)/pool_combiner.o -lpthread

# stand-alone CPU check of the concealment planner over every loss pattern of
# ten ticks (tools/conceal_plan_check.cpp gives the sanitizer recipe)
PLANCHECK := tools/conceal_plan_check

$(PLANCHECK): tools/conceal_plan_check.cpp $(BUILD)/conceal_plan.o $(CSRC)/conceal_plan.h
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $< $(BUILD)/conceal_plan.o

# stand-alone CPU check of the memory owners, the table uploads and the state
# rows over a fake backend (tools/device_mem_check.cpp gives the sanitizer
# recipe)
MEMCHECK := tools/device_mem_check

$(MEMCHECK): tools/device_mem_check.cpp $(CSRC)/device_mem.h
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ $<

# stand-alone check of what the side calls answer without a device, plain C
# against the public header and the in-tree library
# (tools/feat_host_check.c gives the sanitizer recipe)
FEATCHECK := tools/feat_host_check

$(FEATCHECK): tools/feat_host_check.c include/lpcnet_mi355x.h $(LIB)
	$(CC) -std=c99 -O2 -Wall -Wextra -Werror -Iinclude -o $@ $< -Llpcnet_amd -llpcnet_mi355x -Wl,-rpath,'$$ORIGIN/../lpcnet_amd'

hostcheck: $(HOSTCHECK) $(POOLCHECK) $(PLANCHECK) $(MEMCHECK) $(FEATCHECK)

check: hostcheck
	$(HOSTCHECK)
	$(POOLCHECK)
	$(PLANCHECK)
	$(MEMCHECK)
	$(FEATCHECK)

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(BUILD) $(LIB) $(SYNTH) $(DROPIN) $(HOSTCHECK) $(POOLCHECK) $(PLANCHECK) $(MEMCHECK) $(FEATCHECK)
	$(MAKE) -C oracle clean

.PHONY: all lib synth dropin hostcheck oracle clean check
