# Top-level build: libgs4d.so (the product, hipcc for gfx950) and the CPU checker under oracle/.
PKG   := 4dgaussiansplatrendering_amd
CSRC  := $(PKG)/csrc
HOST  := $(PKG)/host
HIPCC ?= hipcc
ROCM ?= /opt/rocm
ARCH  ?= gfx950
LIB   := $(PKG)/libgs4d.so

HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function
# make TUNING=1: ablation knobs and per-tile stamps compiled into the kernels (experiments only; never the shipped build)
ifdef TUNING
HIPFLAGS += -DGS4D_TUNING
endif
# keygen/sort and preprocess must round exactly like the CPU expressions they are checked against
STRICT   := -ffp-contract=off

# the build mode is a prerequisite of every object: switching between `make lib`, `make lib TUNING=1`, `make lib COUNT_IDS_PLAIN=1`, `make lib BUILD_PLAIN=1`, `make lib TRANSFORM_STAGED_LOAD=1`, `make lib XFSEL_PLAIN=1`, `make lib POSE_GLOBAL_TABLE=1`, `make lib POSE_WALK=4`, `make lib WARP_LDS_NODES=512`, `make lib WARP_GLOBAL_LATTICE=1`, `make lib ROWS_MASS_RECOMPUTE=1`, `make lib ROWS_CHUNK=16`, `make lib PROJ_PLAIN_STORE=1` and `make lib PROJ_PITCH=4` rebuilds all of them
FLAGSTAMP := $(CSRC)/.flags.$(if $(TUNING),tuning,release)$(if $(COUNT_IDS_PLAIN),-plain)$(if $(BUILD_PLAIN),-buildplain)$(if $(TRANSFORM_STAGED_LOAD),-transformstagedload)$(if $(XFSEL_PLAIN),-xfselplain)$(if $(POSE_GLOBAL_TABLE),-poseglobaltable)$(if $(POSE_WALK),-posewalk$(POSE_WALK))$(if $(WARP_LDS_NODES),-warpldsnodes$(WARP_LDS_NODES))$(if $(WARP_GLOBAL_LATTICE),-warpgloballattice)$(if $(ROWS_MASS_RECOMPUTE),-rowsmassrecompute)$(if $(ROWS_CHUNK),-rowschunk$(ROWS_CHUNK))$(if $(PROJ_PLAIN_STORE),-projplainstore)$(if $(PROJ_PITCH),-projpitch$(PROJ_PITCH))
$(FLAGSTAMP):
	rm -f $(CSRC)/.flags.*
	touch $@

OBJS := $(CSRC)/gs4d_api.o $(CSRC)/sort.o $(CSRC)/preprocess.o $(CSRC)/binning.o $(CSRC)/composite.o $(CSRC)/tilelist.o $(CSRC)/composite2.o $(CSRC)/lines.o $(CSRC)/compact.o $(CSRC)/reorder.o $(CSRC)/cut.o $(CSRC)/select.o $(CSRC)/shade.o $(CSRC)/shade_time.o $(CSRC)/edit.o $(CSRC)/build.o $(CSRC)/decompose.o $(CSRC)/transform.o $(CSRC)/transform_selected.o $(CSRC)/pose.o $(CSRC)/sh_rotate.o $(CSRC)/warp.o $(CSRC)/slice.o $(CSRC)/centres.o $(CSRC)/measure.o $(CSRC)/merge.o $(CSRC)/merge_rows.o $(CSRC)/lod.o $(CSRC)/neighbours.o $(CSRC)/components.o $(CSRC)/nearest.o $(HOST)/gs4d_host.o

.PHONY: all lib oracle ref refscene refdraw refgl clean demo sweep
all: lib oracle demo sweep
DEMO := $(HOST)/scene_replay
SWEEP := $(HOST)/gs4d_sweep
demo: $(DEMO)
# the multi-GPU sweep (BASELINE.json configs[3]) driven from C++: the C ABI + HIP + RCCL, one process per GPU
sweep: $(SWEEP)
$(SWEEP): $(HOST)/gs4d_sweep.cpp include/gs4d.h $(LIB)
	g++ -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include $(HOST)/gs4d_sweep.cpp -o $@ -L$(PKG) -lgs4d -L$(ROCM)/lib -lrccl -lamdhip64 -ldl -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,$(ROCM)/lib
$(DEMO): $(HOST)/scene_replay.cpp $(HOST)/gs4d_compat.h include/gs4d.h $(LIB)
	g++ -O2 -std=c++17 -Wall -o $@ $(HOST)/scene_replay.cpp -L$(PKG) -lgs4d -Wl,-rpath,'$$ORIGIN/..'
lib: $(LIB)

# hd.h holds GS4D_HD / GS4D_UNROLL for every header that a CPU compiler compiles too
HD := $(CSRC)/hd.h
# depth_key.h is the one text of the two depth-key expressions: k_keygen (sort.hip) and blend_key_4d (preprocess.hip) compile it
$(CSRC)/sort.o: $(CSRC)/sort.hip $(CSRC)/depth_key.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# footprint_rect.h is the one text of the pixel rectangle (tests/footprint_rect_check.cpp compiles it too)
# proj_tile.h is the one text of a wave's stage of projected records — the put, the whole-line store, the slots (tests/proj_tile_check.cpp compiles its plain part too)
# make PROJ_PLAIN_STORE=1: k_project_count with every thread storing its own projected record, whatever the source; make PROJ_PITCH=4: the records of a wave's stage back to back instead of five pieces apart (the measurements of DESIGN.md §9 round 16; never the shipped build)
$(CSRC)/preprocess.o: $(CSRC)/preprocess.hip $(CSRC)/proj_tile.h $(CSRC)/footprint_rect.h $(CSRC)/depth_key.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(PROJ_PLAIN_STORE),-DGS4D_PROJ_PLAIN_STORE) $(if $(PROJ_PITCH),-DGS4D_PROJ_PITCH=$(PROJ_PITCH)) -c $< -o $@
$(CSRC)/lines.o: $(CSRC)/lines.hip $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
$(CSRC)/compact.o: $(CSRC)/compact.hip $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
$(CSRC)/reorder.o: $(CSRC)/reorder.hip $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
$(CSRC)/cut.o: $(CSRC)/cut.hip $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
$(CSRC)/shade.o: $(CSRC)/shade.hip $(CSRC)/record_tile.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# sh_time_record.h is the one text of gs4d_shade_sh_t's and gs4d_collapse_sh's definition — the weights of the time blocks, the effective row, gs4d_shade_sh's colour from a row: the kernels and the host library compile it (tests/sh_time_check.cpp compiles it too; gs4d_api.o takes the two calls' scalar checks from it); shade_time.o is built with the flags of shade.o
$(CSRC)/shade_time.o: $(CSRC)/shade_time.hip $(CSRC)/record_tile.h $(CSRC)/sh_time_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
$(CSRC)/edit.o: $(CSRC)/edit.hip $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# centre_query.h is the one text of gs4d_count_centres' definition: the kernel and the host library compile it
$(CSRC)/centres.o: $(CSRC)/centres.hip $(HD) $(CSRC)/centre_query.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# measure_record.h is the one text of what a record adds to gs4d_measure_records' measurement (it takes the centre and the skips from centre_query.h)
$(CSRC)/measure.o: $(CSRC)/measure.hip $(HD) $(CSRC)/measure_record.h $(CSRC)/centre_query.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# merge_record.h is the one text of gs4d_cell_labels' and gs4d_merge_records' definitions: the kernels and the host library compile it (tests/merge_record_check.cpp compiles it too; gs4d_api.o takes the grid check from it)
$(CSRC)/merge.o: $(CSRC)/merge.hip $(CSRC)/record_tile.h $(HD) $(CSRC)/merge_record.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# merge_rows_record.h is the one text of gs4d_merge_rows' definition, on top of merge_record.h: the kernels and the host library compile it (tests/merge_rows_check.cpp compiles it too; gs4d_api.o takes the two row calls' checks and operand lists from rows_operands.h)
# make ROWS_MASS_RECOMPUTE=1: the row reduction computes every member's mass again from its record instead of reading the word the key kernel left in scratch; make ROWS_CHUNK=16 (or 4, or 32): the words of a row one sub-group reduces, instead of 8 (the measurements of DESIGN.md §4; never the shipped build)
$(CSRC)/merge_rows.o: $(CSRC)/merge_rows.hip $(CSRC)/record_tile.h $(HD) $(CSRC)/merge_rows_record.h $(CSRC)/merge_record.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(ROWS_MASS_RECOMPUTE),-DGS4D_ROWS_MASS_RECOMPUTE) $(if $(ROWS_CHUNK),-DGS4D_ROWS_CHUNK=$(ROWS_CHUNK)) -c $< -o $@
# lod_query.h is the one text of gs4d_lod_cut's predicates (it takes the centre from centre_query.h): the kernel and the host library compile it (tests/lod_query_check.cpp compiles it too; gs4d_api.o takes the query check from it, and the two calls' operand lists from lod_operands.h); lod.o is built with the flags of shade.o and centres.o
$(CSRC)/lod.o: $(CSRC)/lod.hip $(CSRC)/record_tile.h $(HD) $(CSRC)/lod_query.h $(CSRC)/centre_query.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# neighbour_query.h is the one text of gs4d_count_neighbours' definition and of its cell function (it takes the centre and the skips from centre_query.h); neighbour_grid.h is the one text of the device's sorted-slot fetch and cell walk, which components.hip and nearest.hip compile too
$(CSRC)/neighbours.o: $(CSRC)/neighbours.hip $(HD) $(CSRC)/neighbour_grid.h $(CSRC)/neighbour_query.h $(CSRC)/centre_query.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# gs4d_label_components walks the grid of neighbours.hip with the same `near`; component_union.h is the one text of its union-find (the host library and tests/component_union_stress.cpp compile it too)
$(CSRC)/components.o: $(CSRC)/components.hip $(HD) $(CSRC)/neighbour_grid.h $(CSRC)/component_union.h $(CSRC)/neighbour_query.h $(CSRC)/centre_query.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# gs4d_nearest_neighbours walks the grid of neighbours.hip too; nearest_query.h is the one text of its order key, its dist2 and its sorted insertion (the host library compiles it too)
$(CSRC)/nearest.o: $(CSRC)/nearest.hip $(HD) $(CSRC)/neighbour_grid.h $(CSRC)/nearest_query.h $(CSRC)/neighbour_query.h $(CSRC)/centre_query.h $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# record_tile.h is the one text of a tile of 96-byte records — the record load, the put, the staged store and load in LDS, f32x4 — and of the host loop that launches the kernels in runs of workgroups (tests/record_tile_check.cpp compiles its plain part too)
# build_record.h is the one text of the record builders: the kernel and the host library compile it (tests/build_record_check.cpp compiles it too)
# make BUILD_PLAIN=1: gs4d_build_records with every thread storing its own record, without the LDS staging (the measurement of DESIGN.md §4; never the shipped build)
$(CSRC)/build.o: $(CSRC)/build.hip $(CSRC)/record_tile.h $(CSRC)/build_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(BUILD_PLAIN),-DGS4D_BUILD_PLAIN) -c $< -o $@
# decompose_record.h is the one text of gs4d_decompose_records' definition, on top of build_record.h: the kernel and the host library compile it (tests/decompose_record_check.cpp compiles it too); decompose.o is built with the flags of build.o
$(CSRC)/decompose.o: $(CSRC)/decompose.hip $(CSRC)/record_tile.h $(CSRC)/decompose_record.h $(CSRC)/build_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# transform_record.h is the one text of the record transforms and of the centre of a measurement: both transform kernels and the host library compile it (tests/transform_record_check.cpp and tests/transform_selected_check.cpp compile it too)
# make TRANSFORM_STAGED_LOAD=1: gs4d_transform_records with the input staged in LDS like the output, instead of every thread loading its own record (the measurement of DESIGN.md §4; never the shipped build)
$(CSRC)/transform.o: $(CSRC)/transform.hip $(CSRC)/record_tile.h $(CSRC)/transform_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(TRANSFORM_STAGED_LOAD),-DGS4D_TRANSFORM_STAGED_LOAD) -c $< -o $@
# make XFSEL_PLAIN=1: gs4d_transform_selected with every selected thread storing its own record, without the LDS staging and the wave masks (the measurement of DESIGN.md §4; never the shipped build)
$(CSRC)/transform_selected.o: $(CSRC)/transform_selected.hip $(CSRC)/record_tile.h $(CSRC)/transform_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(XFSEL_PLAIN),-DGS4D_XFSEL_PLAIN) -c $< -o $@
# pose_record.h is the one text of gs4d_pose_records' definition, on top of transform_record.h: the kernel and the host library compile it (tests/pose_record_check.cpp compiles it too)
# make POSE_GLOBAL_TABLE=1: gs4d_pose_records with every thread loading its table rows from global memory for every m, without the workgroup's copy of a small table in LDS; make POSE_WALK=4: a workgroup with the table in LDS takes 4 tiles instead of one (the measurements of DESIGN.md §4; never the shipped build)
$(CSRC)/pose.o: $(CSRC)/pose.hip $(CSRC)/record_tile.h $(CSRC)/pose_record.h $(CSRC)/transform_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(POSE_GLOBAL_TABLE),-DGS4D_POSE_GLOBAL_TABLE) $(if $(POSE_WALK),-DGS4D_POSE_WALK=$(POSE_WALK)) -c $< -o $@
# sh_rotate_record.h is the one text of gs4d_rotate_sh's definition — the frame of a map, the band matrices, a row under them — on top of pose_record.h: the kernel and the host library compile it (tests/sh_rotate_check.cpp compiles it too; gs4d_api.o and the host library take the call's checks and operand list from sh_rotate_operands.h); sh_rotate.o is built with the flags of pose.o
$(CSRC)/sh_rotate.o: $(CSRC)/sh_rotate.hip $(CSRC)/record_tile.h $(CSRC)/sh_rotate_record.h $(CSRC)/pose_record.h $(CSRC)/transform_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# warp_record.h is the one text of gs4d_warp_records' definition, on top of pose_record.h and transform_record.h: the kernel and the host library compile it (tests/warp_record_check.cpp compiles it too; gs4d_api.o takes the lattice check from it); warp.o is built with the flags of pose.o
# make WARP_LDS_NODES=512: gs4d_warp_records with the workgroup's copy in LDS of a lattice of at most 512 nodes, instead of every thread loading its nodes from global memory for every lattice; make WARP_GLOBAL_LATTICE=1 takes that copy out of such a build again (the measurements of DESIGN.md §4; the LDS copy is never the shipped build)
$(CSRC)/warp.o: $(CSRC)/warp.hip $(CSRC)/record_tile.h $(CSRC)/warp_record.h $(CSRC)/pose_record.h $(CSRC)/transform_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(WARP_LDS_NODES),-DGS4D_WARP_LDS_NODES=$(WARP_LDS_NODES)) $(if $(WARP_GLOBAL_LATTICE),-DGS4D_WARP_GLOBAL_LATTICE) -c $< -o $@
# slice_record.h is the one text of gs4d_slice_records' definition: the kernel and the host library compile it; slice.o is built with the flags of preprocess.o, so its expf is the draw's
$(CSRC)/slice.o: $(CSRC)/slice.hip $(CSRC)/record_tile.h $(CSRC)/slice_record.h $(HD) $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) -c $< -o $@
# make COUNT_IDS_PLAIN=1: gs4d_count_ids without its in-wave aggregation (the measurement of DESIGN.md §4; never the shipped build)
$(CSRC)/select.o: $(CSRC)/select.hip $(CSRC)/gs4d_internal.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) $(STRICT) $(if $(COUNT_IDS_PLAIN),-DGS4D_COUNT_IDS_PLAIN) -c $< -o $@
# operands.h is the one text of the record-set calls' buffer-argument check (tests/operand_check.cpp compiles it too)
$(CSRC)/gs4d_api.o: $(CSRC)/operands.h $(CSRC)/merge_record.h $(CSRC)/warp_record.h $(CSRC)/pose_record.h $(CSRC)/transform_record.h $(CSRC)/lod_operands.h $(CSRC)/rows_operands.h $(CSRC)/sh_rotate_operands.h $(CSRC)/sh_time_record.h $(CSRC)/lod_query.h $(CSRC)/centre_query.h $(HD)
$(CSRC)/%.o: $(CSRC)/%.hip $(CSRC)/gs4d_internal.h $(CSRC)/composite_common.h include/gs4d.h Makefile $(FLAGSTAMP)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(HOST)/gs4d_host.o: $(HOST)/gs4d_host.cpp $(CSRC)/build_record.h $(CSRC)/decompose_record.h $(CSRC)/transform_record.h $(CSRC)/pose_record.h $(CSRC)/sh_rotate_record.h $(CSRC)/sh_rotate_operands.h $(CSRC)/sh_time_record.h $(CSRC)/operands.h $(CSRC)/warp_record.h $(CSRC)/slice_record.h $(HD) $(CSRC)/centre_query.h $(CSRC)/measure_record.h $(CSRC)/merge_record.h $(CSRC)/merge_rows_record.h $(CSRC)/lod_query.h $(CSRC)/neighbour_query.h $(CSRC)/component_union.h $(CSRC)/nearest_query.h include/gs4d.h
	$(HIPCC) -O2 -std=c++17 -fPIC -fvisibility=hidden $(STRICT) -x c++ -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle oracle
ref:
	$(MAKE) -C oracle ref
refscene: lib
	$(MAKE) -C oracle refscene
refdraw: lib
	$(MAKE) -C oracle refdraw
refgl:
	$(MAKE) -C oracle refgl

clean:
	rm -f $(OBJS) $(LIB) $(DEMO) $(SWEEP)
	$(MAKE) -C oracle clean
