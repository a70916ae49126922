# TEST INFRASTRUCTURE ONLY: the nine entries of include/libiop_amd_head.h with each vector in turn off the 16-byte boundary, at m = 0, sub_dim = 0 and
# sub_dim = m, under AddressSanitizer and UBSan in a stand-alone program (gfx_head_selfcheck.cpp), over the sanitizer objects and flags of the
# Makefile beside this file.  Built and run by hand on a CPU; nothing is loaded into Python.
#   make -f gfx_head_selfcheck.mk gfx_head_selfcheck_san && ASAN_OPTIONS=detect_leaks=0 ./gfx_head_selfcheck_san
# detect_leaks=0: the inverse tables at sub_dim = 0 are larger than one kernel argument block, so their upload takes a pinned staging chunk of the
# runtime (runtime.hip), which the library keeps for the life of the process with its event; without the option LeakSanitizer lists those events (one per
# field) at exit and nothing else.  Address and undefined-behaviour checks are not affected by it.
include gfx_head.mk

gfx_head_selfcheck_san: $(SAN_LIB_OBJS) obj_san/gfx_head_selfcheck.o
	$(CXX) -fsanitize=address,undefined -o $@ $^

obj_san/gfx_head_selfcheck.o: ../../include/libiop_amd_head.h

clean: clean_gfx_head_selfcheck
clean_gfx_head_selfcheck:
	rm -f gfx_head_selfcheck_san
.PHONY: clean_gfx_head_selfcheck
