# TEST INFRASTRUCTURE ONLY: the entries of gfx_ops.h over the wider fields (gf128_ops.hip, gf256_ops.hip; gf64_edges_selfcheck has gf64's) with each vector in turn off the 16-byte boundary, and the
# domain-shaped ones on a domain of one element, under AddressSanitizer and UBSan in a stand-alone program (gfx_ops_edges_selfcheck.cpp), over the
# sanitizer objects and flags of the Makefile beside this file.
#   make -f gfx_ops_edges_selfcheck.mk gfx_ops_edges_selfcheck_san && ./gfx_ops_edges_selfcheck_san
include Makefile

gfx_ops_edges_selfcheck_san: $(SAN_LIB_OBJS) obj_san/gfx_ops_edges_selfcheck.o
	$(CXX) -fsanitize=address,undefined -o $@ $^

# What the Makefile beside this file does not know, for a build through this file: the objects also depend on the second public header, and
# `make -f gfx_ops_edges_selfcheck.mk clean` removes this program too.  (A plain `make` rebuilds the emulation after an edit of libiop_amd.h, not of
# libiop_amd_gfx.h: run it through this file, or `make clean` first.)
$(OBJS) obj/emu_runtime.o obj/toy_kernels.o $(SAN_LIB_OBJS) obj_san/gfx_ops_edges_selfcheck.o: ../../include/libiop_amd_gfx.h

clean: clean_gfx_ops_edges_selfcheck
clean_gfx_ops_edges_selfcheck:
	rm -f gfx_ops_edges_selfcheck_san
.PHONY: clean_gfx_ops_edges_selfcheck
