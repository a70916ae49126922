"""The batched transforms and the fused re-extension over gf64, gf128 and gf256 on the CPU build of the kernels: tests/gfx_batch_cases.py (the GPU
leg is tests/test_gpu_gfx_batch.py)."""
import pytest

import gfx_batch_cases as B
from emu_lib import emu

W = pytest.mark.parametrize("words", B.WORDS, ids=lambda w: B.NAME[w])
TILES = pytest.mark.parametrize("tiles", [None, B.SMALLEST_TILES], ids=["default-tiles", "smallest-tiles"])


def _torch():
    import torch
    return torch, torch.device("cpu")


@W
@TILES
def test_reextend_grid(words, tiles):
    B.check_reextend_grid(emu(), words, tiles)


@W
@TILES
def test_lde_grid(words, tiles):
    B.check_lde_grid(emu(), words, tiles)


@W
@TILES
def test_ifft_grid(words, tiles):
    B.check_ifft_grid(emu(), words, tiles)


@W
@TILES
def test_reextend_lde_grid(words, tiles):
    B.check_reextend_lde_grid(emu(), words, tiles)


@W
def test_coset_windows_and_staging_rounds(words):
    B.check_coset_windows(emu(), words)


@W
def test_default_tiles_past_one_tile(words):
    B.check_default_tiles(emu(), words)


@W
def test_shifts(words):
    B.check_shifts(emu(), words)


@W
def test_alignment_selects_the_instantiation(words):
    B.check_alignment(emu(), words)


@W
def test_output_over_the_input(words):
    B.check_aliased_output(emu(), words)


@W
def test_refusals(words):
    B.check_refusals(emu(), words)


@W
def test_fused_reextension_launches_no_phase1(words):
    B.check_structure(emu(), words)


@W
def test_against_the_oracle(words):
    B.check_against_the_oracle(emu(), words)


@W
def test_native_proof_runs_the_batched_kernels(words):
    B.check_native_proof_profile(emu(), words)


@W
def test_python_proof_runs_the_batched_kernels(words):
    B.check_python_proof_profile(emu(), *_torch(), words)


def test_native_gf64_fri_snark_unchanged():
    import gf64_aurora_cases as G
    G.check_native_fri_snark(emu())


@W
def test_native_prover_transcripts_unchanged(words):
    """the existing comparisons of gf64_aurora_cases.py / gfx_aurora_cases.py at their first tuple, now through the fused route"""
    if words == 1:
        import gf64_aurora_cases as G
        G.check_native_prover(emu(), G.NATIVE_TUPLES[0])
    else:
        import gfx_aurora_cases as C
        C.check_native_prover(emu(), *_torch(), words, C.NATIVE_TUPLES[0])
