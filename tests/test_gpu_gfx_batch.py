"""The batched transforms and the fused re-extension over gf64, gf128 and gf256 on the MI355X: tests/gfx_batch_cases.py (the CPU leg is
tests/test_gfx_batch_emu.py)."""
import pytest

import gfx_batch_cases as B

pytestmark = pytest.mark.gpu

W = pytest.mark.parametrize("words", B.WORDS, ids=lambda w: B.NAME[w])
TILES = pytest.mark.parametrize("tiles", [None, B.SMALLEST_TILES], ids=["default-tiles", "smallest-tiles"])


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


class on_torch_stream:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        import torch
        self.lib.set_stream(torch.cuda.current_stream().cuda_stream)
        return torch, torch.device("cuda:0")

    def __exit__(self, *exc):
        self.lib.use_own_stream()


@W
@TILES
def test_reextend_grid(lib, words, tiles):
    B.check_reextend_grid(lib, words, tiles)


@W
@TILES
def test_lde_grid(lib, words, tiles):
    B.check_lde_grid(lib, words, tiles)


@W
@TILES
def test_ifft_grid(lib, words, tiles):
    B.check_ifft_grid(lib, words, tiles)


@W
@TILES
def test_reextend_lde_grid(lib, words, tiles):
    B.check_reextend_lde_grid(lib, words, tiles)


@W
def test_coset_windows_and_staging_rounds(lib, words):
    B.check_coset_windows(lib, words)


@W
def test_default_tiles_past_one_tile(lib, words):
    B.check_default_tiles(lib, words)


@W
def test_shifts(lib, words):
    B.check_shifts(lib, words)


@W
def test_alignment_selects_the_instantiation(lib, words):
    B.check_alignment(lib, words)


@W
def test_output_over_the_input(lib, words):
    B.check_aliased_output(lib, words)


@W
def test_refusals(lib, words):
    B.check_refusals(lib, words)


@W
def test_fused_reextension_launches_no_phase1(lib, words):
    B.check_structure(lib, words)


@W
def test_against_the_oracle(lib, words):
    B.check_against_the_oracle(lib, words)


@W
def test_native_proof_runs_the_batched_kernels(lib, words):
    B.check_native_proof_profile(lib, words)


@W
def test_python_proof_runs_the_batched_kernels(lib, words):
    with on_torch_stream(lib) as (torch, device):
        B.check_python_proof_profile(lib, torch, device, words)


def test_native_gf64_fri_snark_unchanged(lib):
    import gf64_aurora_cases as G
    G.check_native_fri_snark(lib)


@W
def test_native_prover_transcripts_unchanged(lib, words):
    """the existing comparisons of gf64_aurora_cases.py / gfx_aurora_cases.py at their first tuple, now through the fused route"""
    if words == 1:
        import gf64_aurora_cases as G
        G.check_native_prover(lib, G.NATIVE_TUPLES[0])
    else:
        import gfx_aurora_cases as C
        with on_torch_stream(lib) as (torch, device):
            C.check_native_prover(lib, torch, device, words, C.NATIVE_TUPLES[0])
