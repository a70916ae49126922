"""The alt_bn128 Fr protocol-layer kernels on the MI355X, through the HIP library, against Python-integer values
(tests/bn128_protocol_cases.py): the tiny fixture, the 2^22 digests, raw data words, and 2^25-element runs checked at sampled
positions (grid-stride and index arithmetic past 2^24 elements x 32 bytes = 2^29 bytes, up to 2^30 bytes)."""
import numpy as np
import pytest

import bn128_protocol_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lb = libiop_amd.lib()
    lb.init(0)
    return lb


def test_tiny_cases(lib):
    want = C.load_json("bn128_protocol_tiny.json")["cases"]
    got = C.run_tiny(lib)
    bad = sorted(k for k in want if got.get(k) != want[k])
    assert not bad, bad


def test_digests_2p22(lib):
    want = C.load_json("bn128_protocol_digests_large.json")["cases"]
    report = []
    for name, out in C.run_large(lib, 22):
        if C.digest(out) != want[name]["digest"]:
            chunks = C.chunk_digests(out)
            report.append((name, [i for i, (g, w) in enumerate(zip(chunks, want[name]["chunks"])) if g != w][:16]))
    assert not report, "differing 2^16-element chunks: %s" % report


def test_raw_data_words(lib):
    C.check_raw_words(lib)


def sample_positions(n, tag):
    rng = np.random.default_rng(int.from_bytes(tag.encode()[:8].ljust(8, b"\0"), "little"))
    fixed = [0, 1, n - 1, n - 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, n // 2 + 255]
    return sorted({j for j in fixed if 0 <= j < n} | {int(v) for v in rng.integers(0, n, size=12)})


@pytest.mark.parametrize("op", ["rowcheck", "lincomb", "rational_sumcheck_constraint"])
def test_2p25_sampled(lib, op):
    """one entry per group (Aurora virtual oracles, Aurora vector steps, Fractal vector steps) at 2^25 elements"""
    F, m = C.BN, 25
    case = [c for c in C.large_cases(F, m) if c["op"] == op][0]
    if op == "lincomb":
        case = dict(case, num=2, coeffs=case["coeffs"][:2])
    inp = C.inputs(F, case)
    outs = C.run_case(lib, F, case, inp)
    idxs = sample_positions(1 << m, op)
    want = C.model_words(F, case, inp, idxs)
    for g, w in zip(outs, want):
        assert np.array_equal(g[idxs], w), op
