# TEST INFRASTRUCTURE ONLY: what the Makefile beside this file does not know about the fourth public header.  The objects of the emulation (and of the
# sanitizer builds) also depend on include/libiop_amd_head.h, which libiop_amd.h includes: a plain `make` rebuilds them after an edit of libiop_amd.h,
# not of this header.  Build through this file after editing it, or `make clean` first:
#   make -f gfx_head.mk
include gfx_batch.mk

.DEFAULT_GOAL := libiopx_emu.so

$(OBJS) obj/emu_runtime.o obj/toy_kernels.o $(SAN_LIB_OBJS): ../../include/libiop_amd_head.h
