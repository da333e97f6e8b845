# Build of the MI355X-native drprg predict hot path.
#   make            -> drprg_amd/lib/libdrprg_hip.so, drprg_amd/bin/pandora, oracle/liboracle.so
# hipcc cross-compiles gfx950 without a GPU present.
HIPCC    ?= /opt/rocm/bin/hipcc
CC       ?= gcc
ARCH     ?= gfx950
CXXFLAGS := -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Iinclude
HIPFLAGS := $(CXXFLAGS) --offload-arch=$(ARCH)

SRC  := drprg_amd/csrc
OBJD := build/obj
HOST_SRCS := prg.cpp kmergraph.cpp index.cpp fastx.cpp genotype.cpp params.cpp denovo.cpp mapper.cpp read_prep.cpp resident.cpp capi.cpp capi_map.cpp capi_prep.cpp capi_reduce.cpp capi_genotype.cpp capi_tools.cpp vcfio.cpp bcfout.cpp annotate.cpp report_json.cpp qc_json.cpp ingest.cpp pgunzip.cpp rccl_dyn.cpp pack.cpp switches.cpp bam.cpp
HIP_SRCS := read_stats.hip sketch_probe.hip sketch_wave.hip sketch_filter.hip candidates.hip read_cluster.hip cluster.hip anchor_scan.hip packed.hip covg_cut.hip bam_pack.hip subsample.hip read_qual.hip dedup.hip read_trim.hip adapter_trim.hip adapter_edit.hip decoy_screen.hip base_mask.hip poly_tail.hip read_complexity.hip pair_overlap.hip pair_merge.hip pair_dedup.hip
LIB  := drprg_amd/lib/libdrprg_hip.so
OBJS := $(addprefix $(OBJD)/,$(HOST_SRCS:.cpp=.o)) $(addprefix $(OBJD)/,$(HIP_SRCS:.hip=.o))
BIN  := drprg_amd/bin/pandora
ORACLE := oracle/liboracle.so

DRPRG := drprg_amd/bin/drprg

all: $(LIB) $(BIN) $(DRPRG) $(ORACLE)

$(DRPRG): $(SRC)/drprg_main.cpp $(SRC)/adapter_args.h $(SRC)/decoy_args.h $(SRC)/mask_args.h $(SRC)/poly_args.h $(SRC)/pair_args.h $(SRC)/qc_args.h $(SRC)/read_stats_host.h $(SRC)/read_stats_words.h include/drprg_hip.h $(LIB)
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) -x c++ $< -o $@ -Ldrprg_amd/lib -ldrprg_hip -Wl,-rpath,'$$ORIGIN/../lib'

$(OBJD)/%.o: $(SRC)/%.cpp $(wildcard $(SRC)/*.h) include/drprg_hip.h
	@mkdir -p $(OBJD)
	$(HIPCC) $(CXXFLAGS) -x hip --offload-arch=$(ARCH) -c $< -o $@

$(OBJD)/%.o: $(SRC)/%.hip $(wildcard $(SRC)/*.h) include/drprg_hip.h
	@mkdir -p $(OBJD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p $(dir $@)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS) -lz -ldl

$(BIN): $(SRC)/pandora_main.cpp $(SRC)/adapter_args.h $(SRC)/decoy_args.h $(SRC)/mask_args.h $(SRC)/poly_args.h $(SRC)/pair_args.h $(SRC)/qc_args.h $(SRC)/read_stats_host.h $(SRC)/read_stats_words.h include/drprg_hip.h $(LIB)
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) -x c++ $< -o $@ -Ldrprg_amd/lib -ldrprg_hip -Wl,-rpath,'$$ORIGIN/../lib'

$(ORACLE): oracle/oracle.c oracle/oracle_index.c oracle/oracle_params.c oracle/oracle_vcf.c oracle/oracle_index.h
	$(CC) -O2 -fPIC -shared -Wall -o $@ oracle/oracle.c oracle/oracle_index.c oracle/oracle_params.c oracle/oracle_vcf.c -lm

clean:
	rm -rf build $(LIB) $(BIN) $(ORACLE)


.PHONY: all clean

# host code under AddressSanitizer + UBSan (CPU build only: GPU sanitizers are not available on the pool):
#   make asan && LD_PRELOAD=$(ls /opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so) \
#     ASAN_OPTIONS=detect_leaks=0 DRPRG_HIP_LIB=build/asan/libdrprg_hip.so python -m pytest tests -m "not gpu" -s
ASAN_FLAGS := -O1 -g -std=c++17 -fPIC -Iinclude -fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer
asan:
	@mkdir -p build/asan
	for f in $(HOST_SRCS:.cpp=); do $(HIPCC) $(ASAN_FLAGS) -x hip --offload-arch=$(ARCH) -c $(SRC)/$$f.cpp -o build/asan/$$f.o || exit 1; done
	for f in $(HIP_SRCS:.hip=); do $(HIPCC) $(ASAN_FLAGS) --offload-arch=$(ARCH) -c $(SRC)/$$f.hip -o build/asan/$$f.o || exit 1; done
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -fsanitize=address,undefined -fno-gpu-sanitize -o build/asan/libdrprg_hip.so build/asan/*.o -lz -ldl

.PHONY: asan
