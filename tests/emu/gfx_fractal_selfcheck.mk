# TEST INFRASTRUCTURE ONLY: the fifteen entries of include/libiop_amd_fractal.h with each vector in turn off the 16-byte boundary, at m = 0, k = 0 and
# k = m, and the batch division with its root inverted either way, under AddressSanitizer and UBSan in a stand-alone program
# (gfx_fractal_selfcheck.cpp), over the sanitizer objects and flags of the Makefile beside this file.  Built and run by hand on a CPU; nothing is
# loaded into Python.
#   make -f gfx_fractal_selfcheck.mk gfx_fractal_selfcheck_san && ASAN_OPTIONS=detect_leaks=0 ./gfx_fractal_selfcheck_san
# detect_leaks=0: as for gfx_head_selfcheck.mk (the runtime keeps its pinned staging chunks and their events for the life of the process).
include gfx_head.mk

$(OBJS) obj/emu_runtime.o obj/toy_kernels.o $(SAN_LIB_OBJS): ../../include/libiop_amd_fractal.h

gfx_fractal_selfcheck_san: $(SAN_LIB_OBJS) obj_san/gfx_fractal_selfcheck.o
	$(CXX) -fsanitize=address,undefined -o $@ $^

obj_san/gfx_fractal_selfcheck.o: ../../include/libiop_amd_fractal.h

clean: clean_gfx_fractal_selfcheck
clean_gfx_fractal_selfcheck:
	rm -f gfx_fractal_selfcheck_san
.PHONY: clean_gfx_fractal_selfcheck
