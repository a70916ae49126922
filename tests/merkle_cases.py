"""Merkle leaf-kernel dispatch by alignment, shared by the CPU-emulation and GPU suites: k_merkle_leaves_sub24 (16-byte vector loads and
stores) is taken only when every additive oracle pointer and the node array are 16-byte aligned (merkle_blake2b.hip); sub-buffers 8 bytes
past an aligned base must go to the general kernel and give the oracle's tree."""
import numpy as np

import oracle
from helpers import rand_elems

# (number of oracles, coset size, leaves): shapes the fixed kernel takes when the pointers are aligned
ALIGN = [(1, 2, 64), (2, 4, 32), (4, 4, 128)]


def check_misaligned(lib, r, cs, L, misalign_oracles, misalign_nodes, additive=True):
    n = L * cs
    oracles = [rand_elems(800 + k, n, 3) for k in range(r)]
    bases = [lib.malloc(o.nbytes + 16) for o in oracles]
    nodes_base = lib.malloc((2 * L - 1) * 32 + 16)
    try:
        ptrs = []
        for k, (b, o) in enumerate(zip(bases, oracles)):
            p = b + (8 if misalign_oracles and k == r - 1 else 0)       # the last oracle alone, so the guard has to look at every pointer
            lib.h2d(p, o)
            ptrs.append(p)
        d_nodes = nodes_base + (8 if misalign_nodes else 0)
        lib.merkle_tree_dev(ptrs, 24, n, cs, d_nodes, 0 if additive else 1)
        got = np.empty((2 * L - 1, 32), dtype=np.uint8)
        lib.d2h(got, d_nodes)
        assert np.array_equal(got, oracle.merkle_build(oracles, cs, additive)), (r, cs, L, misalign_oracles, misalign_nodes, additive)
    finally:
        for b in bases:
            lib.free(b)
        lib.free(nodes_base)


def check_alignments(lib, r, cs, L):
    for mo, mn in ((False, False), (True, False), (False, True), (True, True)):
        check_misaligned(lib, r, cs, L, mo, mn)
    check_misaligned(lib, r, cs, L, False, True, additive=False)
