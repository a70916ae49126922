"""The product kernels that have a barrier or a rule of which wavefront owns which LDS rows, on the CPU emulation's threaded mode: every
workgroup runs with the block size of its launch, one fiber per thread, each alone up to its next __syncthreads(), in ascending, descending
and one seeded order of thread index, and with workgroups in descending order too wherever a pass works in place.  A value that crosses
threads inside one barrier interval is read stale under one of the first two orders (tests/test_thread_orders_selfcheck_emu.py shows that
with toy kernels), and every launch must keep barrier discipline.  The cases and their expectations are the existing case modules';
with one thread per workgroup, the suite's default, they run in the files named next to each.

Kernels a run-to-barrier fiber cannot model, and so kept on the default order (a dependence between lanes of ONE wavefront, which execute in
lockstep on the GPU):
  * k_gf192_mul_halves (fft_add.hip, `const unsigned long long live = __ballot(1)`): the ballot must see all lanes of the wavefront at once;
    its tests stay in tests/test_kernel_logic_emu.py (and tests/halves_cases.py) on order 0.
No kernel that was run here needed an exemption.

Not run here, and why:
  * k_poseidon_level (no barrier, one node per thread) takes levels of more than 2^14 nodes only, a tree of 2^16 leaves: minutes of the oracle.
  * k_poseidon_top is launched by nothing in the library (iopx_merkle_poseidon_bn128_dev takes k_poseidon_top_par for every tree).
"""
import os
import subprocess
import sys

import pytest
import torch

import aurora_cases as ac
import bn128_cases as bc
import fractal_cases as fc
import gf64_cases as g64
import golden_cases_edwards as ge
import ldt_cases as lc
import libiop_amd
import oracle
import poseidon_cases as pc
import test_kernel_logic_emu as kernel_logic
import thread_order_cases as tc
import upper_tile_cases as uc
from emu_lib import emu

HERE = os.path.dirname(os.path.abspath(__file__))
CPU = torch.device("cpu")
GD = tc.GROUPS_DESCENDING

# thread orders for passes that write where no other workgroup reads, and for passes in place (the butterfly passes: src == dst)
ORDERS = {"ascending": tc.ASCENDING, "descending": tc.DESCENDING, "seeded": tc.SEEDED}
IN_PLACE_ORDERS = dict(ORDERS, **{"ascending-groups-descending": tc.ASCENDING | GD, "descending-groups-descending": tc.DESCENDING | GD})
# the largest shapes leave the seeded permutation out (the suite's time; ascending and descending are never left out)
LARGE_ORDERS = {k: v for k, v in IN_PLACE_ORDERS.items() if not k.startswith("seeded")}


def orders_for(d):
    return sorted(LARGE_ORDERS if d >= 15 else IN_PLACE_ORDERS)


def under(order_name):
    """every launch inside runs under the order and must keep barrier discipline; order 0 comes back whatever happens"""
    return tc.thread_order(emu(), IN_PLACE_ORDERS[order_name])


# ---- additive FFT over gf192: k_phase1, k_bfly_upper_comb, k_bfly_edge, k_bfly_edge_multi, k_bfly_edge_fwd_batch ----------------------------------
GF192_DIMS = (11, 12, 13, 14, 15)


# (d = 17, three tiles of 5 + 5 + 1 levels: ascending, and descending threads with descending workgroups)
@pytest.mark.parametrize("d,order", [(d, o) for d in GF192_DIMS for o in orders_for(d)] + [(17, "ascending"), (17, "descending-groups-descending")])
def test_gf192_forward_and_inverse(d, order):
    with under(order):
        uc.check_fft_ifft(emu(), d, "standard" if d & 1 else "random")


@pytest.mark.parametrize("d,order", [(d, o) for d in GF192_DIMS for o in orders_for(d)])
def test_gf192_coset_lde(d, order):
    with under(order):
        uc.check_lde(emu(), False, d, "random" if d & 1 else "standard", 1, 3)


@pytest.mark.parametrize("d,order", [(d, o) for d in GF192_DIMS for o in orders_for(d)])
def test_gf192_reextension_batch(d, order):
    uc.reextend_refs(d, 3)
    with under(order):
        uc.check_reextend(emu(), False, d=d)


GENERAL_PRODUCT = r"""
import sys
import thread_order_cases as tc
import upper_tile_cases as uc
from emu_lib import emu
options = dict(uc.SCHEDULE_OPTIONS, IOPX_COMB=0)
for d in (11, 12, 13):
    for order in (tc.ASCENDING, tc.DESCENDING, tc.ASCENDING | tc.GROUPS_DESCENDING, tc.DESCENDING | tc.GROUPS_DESCENDING):
        with tc.thread_order(emu(), order):
            uc.check_fft_ifft(emu(), d, "random", options=options)
            uc.check_lde(emu(), False, d, "standard", 1, 3, options=options)
print("ok")
"""


def test_gf192_general_product_upper_pass():
    """IOPX_COMB=0 (read once per process, so a child): the upper passes are k_bfly_upper's, a barrier per level on 1024 threads"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE]), IOPX_COMB="0")
    out = subprocess.run([sys.executable, "-c", GENERAL_PRODUCT], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout[-2000:], out.stderr[-4000:])


# ---- gf64: k64_phase1, k64_bfly_upper, k64_bfly_edge and the folds (tests/test_gf64_emu.py) ------------------------------------------------------
@pytest.mark.parametrize("order", sorted(IN_PLACE_ORDERS))
@pytest.mark.parametrize("check", [g64.check_schedules, g64.check_fold, g64.check_ldt, g64.check_lde_ranges], ids=lambda f: f.__name__)
def test_gf64(check, order):
    with under(order):
        check(emu())


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_gf64_fft(order):
    with under(order):
        g64.check_fft(emu(), max_m=12)


# ---- multiplicative cosets: k_bn_mfft_pass (tests/test_bn128_emu.py), k_mfft_pass (tests/test_golden_edwards_tiny.py) and their folds ---------------
@pytest.mark.parametrize("order", sorted(IN_PLACE_ORDERS))
def test_bn128_tiny_cases(order):
    want = bc.load_json("bn128_tiny.json")["cases"]
    with under(order):
        got = bc.run_tiny(emu())
    for kind in want:
        bad = sorted(k for k in want[kind] if got[kind].get(k) != want[kind][k])
        assert not bad, "%s: %s" % (kind, bad)


@pytest.mark.parametrize("order", sorted(IN_PLACE_ORDERS))
def test_edwards_integer_vectors(order):
    lib = emu()
    with under(order):
        ge.check(lib.multiplicative_FFT, lib.multiplicative_IFFT, lib.multiplicative_IFFT_of_known_degree, lib.multiplicative_evaluate_next_f_i,
                 lambda o, cs: lib.merkle_tree(o, cs, domain_type=libiop_amd.DOMAIN_MULTIPLICATIVE))


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("logn", [6, 9, 12])
def test_edwards_transforms(logn, order):
    """(tests/test_kernel_logic_emu.py: one pass, and at 2^12 more than one pass and more than one tile per pass)"""
    with under(order):
        kernel_logic.test_mult_fft(logn)
        kernel_logic.test_mult_ifft(logn)


# ---- k_div_gf192 / k_div_fp3: the product tree of a workgroup (tests/test_fractal_emu.py) ----------------------------------------------------------
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("n", [1, 7, 300, 2500])
@pytest.mark.parametrize("field_name", ["gf192", "edwards_Fr"])
def test_div_kernel(field_name, n, order):
    with under(order):
        fc.check_div_kernel(emu(), torch, CPU, field_name, n)


# ---- k_merkle_top: the levels of the tree's top exchanged through global memory by one workgroup (tests/test_kernel_logic_emu.py) -----------------
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("additive,r,cs,L", [(True, 1, 1, 2), (True, 1, 2, 16), (False, 4, 2, 64), (True, 2, 2, 128), (False, 3, 2, 4096)])
def test_merkle_top(additive, r, cs, L, order):
    with under(order):
        kernel_logic.test_merkle(additive, r, cs, L)


# ---- Poseidon trees: k_poseidon_level_par and k_poseidon_top_par, state elements crossing lanes through LDS (tests/test_poseidon_emu.py) ------------
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name,r,cs,L,additive,zk", [
    ("test_params", 1, 1, 2, False, False), ("starkware_alpha5_t3", 2, 4, 4, False, False), ("high_alpha17_t4", 2, 3, 4, False, True),
    ("test_params", 1, 1, 1024, False, False),
])
def test_poseidon_merkle(name, r, cs, L, additive, zk, order):
    with under(order):
        pc.check_merkle(emu(), name, r, cs, L, additive, zk)


# ---- k_sumcheck_g_add: the per-lane prefix array in block-scope __shared__ memory (tests/test_ldt_emu.py) -------------------------------------------
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("m,sdim,seed,kind", [(5, 2, 1, "aurora"), (9, 4, 2, "general"), (12, 6, 4, "aurora")])
def test_sumcheck_g_additive(m, sdim, seed, kind, order):
    with under(order):
        lc.check_sumcheck_g_additive(emu(), m, sdim, seed, kind)


# ---- one whole proof ----------------------------------------------------------------------------------------------------------------------------
def test_aurora_proof_under_descending_order():
    lib = emu()
    inst = lib.aurora_example_instance(0, 1 << 10, 15, (1 << 10) - 1, 0x2204)
    try:
        ref = oracle.aurora_prove(ac.FIELDS["gf192"][0], 10, 15, 0x2204)
        with under("descending-groups-descending"):
            assert lib.aurora_prove(inst) == ref
    finally:
        lib.aurora_instance_free(inst)
