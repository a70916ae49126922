# TEST INFRASTRUCTURE ONLY: compiles the reference's sources where they lie under $(REF) (nothing is copied) over the stand-in libff / libfqfft of
# tests/harness/shim and writes everything into oracle/_ref/ (git-ignored).  Needs libsodium and GMP (here: /opt/conda).
# build() runs `make -f oracle/reference.mk` (target `all`): every program the CPU suite runs and the HIP-linked one the GPU suite runs.
REF      ?= /root/reference
CONDA    ?= /opt/conda
REPO     := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))..)
H        := $(REPO)/tests/harness
OUT      := $(REPO)/oracle/_ref
B        := $(OUT)/build
HIPD     := $(OUT)/hip
CXX      := g++
CXXFLAGS := -std=c++17 -O2 -g0 -w -include stddef.h
PLAIN_INC  := -I$(H)/shim -I$(REPO)/libiop_amd/csrc -I$(REF) -I$(CONDA)/include
SHIM_HDRS  := $(wildcard $(H)/shim/libff/*/*.hpp $(H)/shim/libff/*/*/*.hpp $(H)/shim/libff/*/*/*/*.hpp $(H)/shim/libfqfft/*/*.hpp $(H)/shim/libfqfft/*/*/*.hpp)
LIBSRC   := common/common.cpp bcs/hashing/blake2b.cpp protocols/ldt/ldt_reducer.cpp protocols/ldt/fri/fri_ldt.cpp protocols/ldt/fri/fri_aux.cpp \
            relations/sparse_matrix.cpp iop/utilities/batching.cpp algebra/utils.cpp
LIBOBJ   := $(patsubst %.cpp,$(B)/ref/%.o,$(LIBSRC))
# conda's lib directory also holds an older libstdc++: link through a directory with only the two libraries.  Every library is linked by name (-l: the
# ones built here have no soname, and a path on the command line would be recorded as the library's name) and found through a search path relative
# to the program ($ORIGIN), so that oracle/_ref/ keeps working when the tree is built in one place and run in another.
LDLIBS   := -L$(B)/lib -lsodium -lgmp
RPATH_TOP     := -Wl,-rpath,'$$ORIGIN/lib:$$ORIGIN/emu'
RPATH_REFTEST := -Wl,-rpath,'$$ORIGIN/../../../lib:$$ORIGIN/../../../emu'
EMU_LIB  = -L$(EMU) -liopx_emu
HIP_LIB  := -L$(REPO)/libiop_amd/lib -liop_amd

# the same program with the stubs of INTEGRATION.md compiled in, forwarding to a CPU build of the kernel sources (the recipe of tests/emu) through the C ABI
STUB_INC := -I$(B) -I$(B)/shadow $(PLAIN_INC) -I$(REPO)
STUBOBJ  := $(patsubst %.cpp,$(B)/ref_stubbed/%.o,$(LIBSRC))
EMU      := $(B)/emu

# libiop's own test files the CPU suite runs by default (tests/harness/harness.py REFTESTS_DEFAULT)
REFTESTS_DEFAULT := protocols/test_fri_aux protocols/test_aurora_protocol protocols/test_direct_ldt

all: $(B)/stubs.inc $(B)/reference_plain $(B)/reference_stubbed $(B)/reference_vectors $(addprefix $(B)/reftests/stubbed/,$(REFTESTS_DEFAULT)) hip

# ---- the CPU build of the kernel sources the stubbed programs link (tests/emu/Makefile's flags; built here so that nothing is written under tests/)
EMU_SRCS := $(wildcard $(REPO)/libiop_amd/csrc/*.hip)
EMU_HDRS := $(wildcard $(REPO)/libiop_amd/csrc/*.h) $(wildcard $(REPO)/libiop_amd/cpp/*.hpp) $(REPO)/tests/emu/fakehip/hip/hip_runtime.h \
            $(REPO)/tests/emu/fakehip/iopx/gfx950_comb.h $(REPO)/include/libiop_amd.h
EMU_OBJS := $(patsubst $(REPO)/libiop_amd/csrc/%.hip,$(EMU)/obj/%.o,$(EMU_SRCS)) $(EMU)/obj/emu_runtime.o
EMU_FLAGS := -O2 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas -fno-extern-tls-init -I$(REPO)/tests/emu/fakehip

$(EMU)/libiopx_emu.so: $(EMU_OBJS)
	$(CXX) -shared -o $@ $^

$(EMU)/obj/%.o: $(REPO)/libiop_amd/csrc/%.hip $(EMU_HDRS)
	@mkdir -p $(dir $@)
	$(CXX) $(EMU_FLAGS) -c -x c++ $< -o $@

$(EMU)/obj/emu_runtime.o: $(REPO)/tests/emu/emu_runtime.cpp $(EMU_HDRS)
	@mkdir -p $(dir $@)
	$(CXX) $(EMU_FLAGS) -c $< -o $@

$(B)/stubs.inc: $(REPO)/INTEGRATION.md $(H)/make_shadow.py
	mkdir -p $(B)
	rm -rf $(B)/shadow
	python3 $(H)/make_shadow.py $(REPO)/INTEGRATION.md $(B) libff/algebra/fields/binary/gf192.hpp libff/algebra/curves/edwards/edwards_pp.hpp

$(B)/ref_stubbed/%.o: $(REF)/libiop/%.cpp $(B)/stubs.inc
	mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) $(STUB_INC) -c $< -o $@

$(B)/run_stubbed.o: $(H)/run_reference.cpp $(B)/stubs.inc $(REPO)/libiop_amd/cpp/reference_binding.hpp
	$(CXX) $(CXXFLAGS) -DHARNESS_STUBS $(STUB_INC) -c $< -o $@

$(B)/reference_stubbed: $(B)/run_stubbed.o $(B)/shim_defs.o $(STUBOBJ) $(B)/lib/.stamp $(EMU)/libiopx_emu.so
	$(CXX) -o $@ $(B)/run_stubbed.o $(B)/shim_defs.o $(STUBOBJ) $(LDLIBS) $(EMU_LIB) $(RPATH_TOP)

# ---- the reference's OWN TEST FILES (libiop/tests/*/test_*.cpp, googletest replaced by shim/gtest/gtest.h), unmodified, as programs: plain and with the
# stubs compiled in (tests_prelude.hpp is force-included ahead of the test's text: libiop's headers, then the stub definitions of INTEGRATION.md)
# Left out: test_bcs_transformation (never sets bcs_transformation_parameters::pow_params_: the grind runs on indeterminate parameters), test_serialization (the
# reference's transcript serialisation does not carry proof_of_work_, so its own verifier says "Invalid pow" after the round trip), test_fractal_indexer,
# test_bivariate_embedding, test_lagrange_polynomial, test_successor_ordering (gf32 / gf128 / gf256, for which no stand-in is written), test_fri_optimizer, test_linking.
REFTESTS := algebra/test_fft algebra/test_exponentiation algebra/test_linearized_polynomial algebra/test_vanishing_polynomial algebra/test_lagrange \
            algebra/test_algebra_utils bcs/test_merkle_tree iop/test_iop iop/test_iop_query_position \
            protocols/test_fri protocols/test_fri_aux protocols/test_ldt_reducer protocols/test_direct_ldt protocols/test_aurora_protocol \
            protocols/test_fractal_protocol protocols/test_basic_lincheck protocols/test_holographic_lincheck \
            protocols/test_sumcheck protocols/test_rational_sumcheck protocols/test_rational_linear_combination protocols/test_rowcheck \
            protocols/test_boundary_constraint protocols/test_r1cs_to_lincheck_reduction protocols/test_ligero_protocol \
            protocols/test_ligero_interleaved_lincheck_et protocols/test_ligero_interleaved_lincheck_ot protocols/test_ligero_interleaved_rowcheck \
            relations/test_r1cs relations/test_identity_matrices snark/test_aurora_snark snark/test_fractal_snark snark/test_ligero_snark \
            snark/test_poseidon snark/test_pow
TEST_INC := -I$(REF)/libiop/tests -I$(REF)/libiop

$(B)/gtest_main_plain.o: $(H)/gtest_main.cpp $(H)/shim/gtest/gtest.h
	mkdir -p $(B)
	$(CXX) $(CXXFLAGS) $(PLAIN_INC) -c $< -o $@
$(B)/gtest_main_stubbed.o: $(H)/gtest_main.cpp $(H)/shim/gtest/gtest.h
	mkdir -p $(B)
	$(CXX) $(CXXFLAGS) -DHARNESS_STUBS $(STUB_INC) -c $< -o $@
$(B)/reftests/plain/%: $(REF)/libiop/tests/%.cpp $(B)/gtest_main_plain.o $(B)/shim_defs.o $(LIBOBJ) $(B)/lib/.stamp
	mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) $(PLAIN_INC) $(TEST_INC) -o $@ $< $(B)/gtest_main_plain.o $(B)/shim_defs.o $(LIBOBJ) $(LDLIBS) $(RPATH_REFTEST) -Wl,--allow-multiple-definition

$(B)/reftests/stubbed/%: $(REF)/libiop/tests/%.cpp $(H)/tests_prelude.hpp $(B)/stubs.inc $(B)/gtest_main_stubbed.o $(B)/shim_defs.o $(STUBOBJ) $(B)/lib/.stamp \
                         $(EMU)/libiopx_emu.so
	mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -DHARNESS_STUBS $(STUB_INC) $(TEST_INC) -include $(H)/tests_prelude.hpp -o $@ $< $(B)/gtest_main_stubbed.o $(B)/shim_defs.o \
	    $(STUBOBJ) $(LDLIBS) $(EMU_LIB) $(RPATH_REFTEST) -Wl,--allow-multiple-definition

reftests_plain: $(addprefix $(B)/reftests/plain/,$(REFTESTS))
reftests_stubbed: $(addprefix $(B)/reftests/stubbed/,$(REFTESTS))

$(B)/lib/.stamp:
	mkdir -p $(B)/lib
	ln -sf $(CONDA)/lib/libsodium.so.23 $(B)/lib/libsodium.so.23 && ln -sf libsodium.so.23 $(B)/lib/libsodium.so
	ln -sf $(CONDA)/lib/libgmp.so.10 $(B)/lib/libgmp.so.10 && ln -sf libgmp.so.10 $(B)/lib/libgmp.so
	touch $@

$(B)/ref/%.o: $(REF)/libiop/%.cpp
	mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) $(PLAIN_INC) -c $< -o $@

$(B)/run_plain.o: $(H)/run_reference.cpp $(SHIM_HDRS)
	mkdir -p $(B)
	$(CXX) $(CXXFLAGS) $(PLAIN_INC) -c $< -o $@

$(B)/vectors.o: $(H)/reference_vectors.cpp $(SHIM_HDRS)
	mkdir -p $(B)
	$(CXX) $(CXXFLAGS) $(PLAIN_INC) -c $< -o $@

$(B)/shim_defs.o: $(H)/shim_defs.cpp $(SHIM_HDRS)
	mkdir -p $(B)
	$(CXX) $(CXXFLAGS) $(PLAIN_INC) -c $< -o $@

$(B)/reference_vectors: $(B)/vectors.o $(B)/shim_defs.o $(LIBOBJ) $(B)/lib/.stamp
	$(CXX) -o $@ $(B)/vectors.o $(B)/shim_defs.o $(LIBOBJ) $(LDLIBS) $(RPATH_TOP) -Wl,--allow-multiple-definition

$(B)/reference_plain: $(B)/run_plain.o $(B)/shim_defs.o $(LIBOBJ) $(B)/lib/.stamp
	$(CXX) -o $@ $(B)/run_plain.o $(B)/shim_defs.o $(LIBOBJ) $(LDLIBS) $(RPATH_TOP) -Wl,--allow-multiple-definition

# the stubbed program against the HIP build of the library, for the GPU suite (tests/test_gpu_reference_prover.py): the reference's prover on the MI355X
# through the stubs.  oracle/_ref/ travels with the tree; libsodium / GMP are copied next to the program (the GPU machine has no reference tree).
hip: $(HIPD)/reference_stubbed_hip

$(HIPD)/reference_stubbed_hip: $(B)/run_stubbed.o $(B)/shim_defs.o $(STUBOBJ) $(REPO)/libiop_amd/lib/libiop_amd.so
	mkdir -p $(HIPD)/lib
	cp -L $(CONDA)/lib/libsodium.so.23 $(CONDA)/lib/libgmp.so.10 $(HIPD)/lib/
	$(CXX) -o $@ $(B)/run_stubbed.o $(B)/shim_defs.o $(STUBOBJ) $(HIPD)/lib/libsodium.so.23 $(HIPD)/lib/libgmp.so.10 -Wl,-rpath,'$$ORIGIN/lib' \
	    $(HIP_LIB) -Wl,-rpath,'$$ORIGIN/../../../libiop_amd/lib'

# libiop's own test files against the HIP build of the library (manual / -m gpu runs on the GPU machine; same recipe as reftests/stubbed)
$(HIPD)/reftests/%: $(REF)/libiop/tests/%.cpp $(H)/tests_prelude.hpp $(B)/stubs.inc $(B)/gtest_main_stubbed.o $(B)/shim_defs.o $(STUBOBJ)
	mkdir -p $(dir $@) $(HIPD)/lib
	cp -L $(CONDA)/lib/libsodium.so.23 $(CONDA)/lib/libgmp.so.10 $(HIPD)/lib/
	$(CXX) $(CXXFLAGS) -DHARNESS_STUBS $(STUB_INC) $(TEST_INC) -include $(H)/tests_prelude.hpp -o $@ $< $(B)/gtest_main_stubbed.o $(B)/shim_defs.o $(STUBOBJ) \
	    $(HIPD)/lib/libsodium.so.23 $(HIPD)/lib/libgmp.so.10 $(HIP_LIB) -Wl,-rpath,'$$ORIGIN/../../lib:$$ORIGIN/../../../../../libiop_amd/lib' \
	    -Wl,--allow-multiple-definition

reftests_hip: $(addprefix $(HIPD)/reftests/,$(REFTESTS))

clean:
	rm -rf $(OUT)

.PHONY: all hip reftests_plain reftests_stubbed reftests_hip clean
