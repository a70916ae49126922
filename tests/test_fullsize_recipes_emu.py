"""The recipes of tests/fullsize_cases.py at the fixture's small sizes through the CPU build of the kernels: the same inputs, call sequences
and digest function as the GPU tests' full-size pins, against the same generator's oracle digests.  A digest that differs on the GPU at
2^22 is then the kernels', not the recipe's.  Also: every entry the GPU tests read is in the fixture."""
import pytest
import torch

import fullsize_cases as fc
from emu_lib import emu

CPU = torch.device("cpu")
SMALL = [(m, k) for m in fc.SMALL_MS for k in fc.keys(m) if not k.startswith("fri_snark")]


def _small(m, key):
    return fc.load()["small"]["sizes"][str(m)][key]


@pytest.mark.parametrize("m,key", [c for c in SMALL if not c[1].startswith("fold_chain")])
def test_transform_recipe(m, key):
    err = fc.mismatch(fc.device_transform(emu(), key, m), _small(m, key), fc.SMALL_LOG_CHUNK)
    assert err is None, err


@pytest.mark.parametrize("m,key", [c for c in SMALL if c[1].startswith("fold_chain")])
def test_fold_chain_recipe(m, key):
    from libiop_amd import domains
    ops = domains.DeviceOps(emu(), torch, CPU, domains.GF192())
    want = _small(m, key)
    steps = [want] + want["folds"]
    seen = []

    def check(i, d_word):
        err = fc.mismatch(ops.download(d_word), steps[i], fc.SMALL_LOG_CHUNK)
        assert err is None, "step %d: %s" % (i, err)
        seen.append(i)

    fc.device_fold_chain(ops, key, m, check)
    assert seen == list(range(len(steps)))


@pytest.mark.parametrize("key", [k.format(m=fc.SMALL_DIM) for k in fc.SNARKS])
def test_fri_snark_recipe(key):
    mine, native = fc.device_snarks(emu(), torch, CPU, key)
    want = _small(fc.SMALL_DIM, key)
    err = fc.snark_mismatch(mine, want)
    assert err is None, "Python prover: " + err
    err = fc.snark_mismatch(native, want)
    assert err is None, "native prover: " + err


def test_fixture_has_every_entry_the_tests_read():
    doc = fc.load()
    assert doc["large"]["m"] == fc.LARGE_M and doc["large"]["log_chunk"] == fc.LARGE_LOG_CHUNK and doc["small"]["log_chunk"] == fc.SMALL_LOG_CHUNK
    sections = [(fc.LARGE_M, doc["large"]["entries"], fc.LARGE_LOG_CHUNK, True)]
    sections += [(m, doc["small"]["sizes"][str(m)], fc.SMALL_LOG_CHUNK, m == fc.SMALL_DIM) for m in fc.SMALL_MS]
    for m, entries, log_chunk, with_snarks in sections:
        for key in fc.keys(m):
            if key.startswith("fri_snark"):
                if with_snarks:
                    e = entries[key]
                    assert len(e["transcript_blake2b"]) == 64 and e["argument_bytes"] > 0, key
                continue
            e = entries[key]
            steps = [e] + e.get("folds", [])
            if key.startswith("fold_chain"):
                _, _, _, loc, _ = fc.fold_chain_input(key, m)
                assert [s["n"] for s in steps] == [1 << (m - sum(loc[:i])) for i in range(len(loc) + 1)], key
            else:
                assert e["n"] == 1 << m, key
            for s in steps:
                assert len(s["digest"]) == 64 and len(s["chunks"]) == max(1, s["n"] >> log_chunk), key


def test_chunk_digests_locate_a_difference():
    import numpy as np
    a = np.arange(3 << 8, dtype=np.uint64).reshape(-1, 3)
    entry = fc.record(a, 4)
    assert fc.mismatch(a, entry, 4) is None
    b = a.copy(); b[5 * 16 + 3, 2] ^= np.uint64(1)
    assert "first [5]" in fc.mismatch(b, entry, 4)
