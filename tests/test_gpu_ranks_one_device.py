"""The 2-, 4- and 8-rank native paths on ONE MI355X.  `python -m torch.distributed.run` starts N ranks that all open GPU 0 (tests/gpu_ranks_worker.py);
they exchange through a gloo group and the staged callback communicator (comm_create_torch_callbacks(staged=True): a test vehicle, every buffer
crosses the host), so the world > 1 branches of libiop_amd/cpp/dist.hpp and cpp/iop.hpp, fft_add_dist.hip's layout kernels and rank-bit network,
comm.hip's k_interleave / k_gather_rows and run_phase1's split run as gfx950 code and their bytes are compared with the CPU oracle.  The cases are
those of tests/test_distributed_gloo.py (tests/sharded_native_cases.py holds both files' bodies); the oracle runs here, in the parent, once per case.

One child group per world size, one after another: 8 ranks and this process are the most that hold the GPU at once.  No retry anywhere: a group that
fails fails its tests."""
import json
import os
import socket
import subprocess
import sys
import time

import pytest

import sharded_native_cases as sn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_ranks_worker.py")
WORLDS = (2, 4, 8)
GROUP_TIMEOUT = {2: 300, 4: 300, 8: 420}          # seconds per child group (start-up of N interpreters included); a gloo collective waits 60 s for a dead peer


def _prove(protocol, field_code, log_n, num_inputs, seed, rs_extra):
    return {"case": "prove", "protocol": protocol, "field_code": field_code, "log_n": log_n, "num_inputs": num_inputs, "seed": seed, "rs_extra": rs_extra}


# (world, case) in tests/test_distributed_gloo.py's own shapes: the smallest that give every rank a non-empty chunk
# The 8-rank PROVER cases of the gloo file — Aurora (8, 7, 5), Aurora over the prime field (8, 9), Fractal (8, 181-bit field, 8) — are not run here: with
# eight processes on the one device they passed, but took 0.1 s to 119 s each from one run to the next (this file 240 s alone, 49 s inside the whole
# suite), and the file must stay under a quarter of the suite's time.  The 8-rank group keeps the distributed transform and the phase-1 split.
AURORA_GF192 = [(2, 7, 5), (4, 8, 5), (2, 7, 8)]                              # (world, log_n, rs_extra); rs_extra 8: the last FRI domain stays distributed
AURORA_PRIME = [(2, 9), (4, 10)]                                              # residue classes: leaf digests by all-to-all + interleave
FRACTAL = [(2, 0, 6, 15), (4, 0, 7, 15), (2, 1, 7, 0)]                        # (world, field_code, log_n, num_inputs)
FRI = [(2, 0, 10), (2, 1, 12)]                                                # (world, field_code, codeword domain dimension)
BAD_WITNESS = [(2, 0, 8)]


def _phase1_small(world):
    m = sn.phase1_min_m(world)
    return {"case": "phase1", "min_d": m - 2, "shapes": [[m, "general"]], "against_unbound": False}


PHASE1_DEFAULT = {"case": "phase1", "min_d": None, "shapes": [[16, "std"]], "against_unbound": True}     # the default threshold: nothing set


def cases_of(world):
    out = [{"case": "fft"}]
    out += [_prove("aurora", 0, log_n, 15, 0x2204, rs) for w, log_n, rs in AURORA_GF192 if w == world]
    out += [_prove("aurora", 1, log_n, 15, 0x2204, 5) for w, log_n in AURORA_PRIME if w == world]
    out += [_prove("fractal", fc, log_n, k, 0x2205, 3) for w, fc, log_n, k in FRACTAL if w == world]
    out += [_prove("fri", fc, dim, 8, 5, 2) for w, fc, dim in FRI if w == world]
    out += [{"case": "bad_witness", "field_code": fc, "log_n": log_n} for w, fc, log_n in BAD_WITNESS if w == world]
    return out + [_phase1_small(world), PHASE1_DEFAULT]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{world: {"cases": [...], "ranks": [every rank's output], "wall": seconds}} — the groups run one after another."""
    out_dir = tmp_path_factory.mktemp("ranks")
    by_world = {}
    for world in WORLDS:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        out = os.path.join(str(out_dir), "w%d" % world)
        cases = cases_of(world)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port", str(port),
               WORKER, "--cases", json.dumps(cases), "--out", out]
        env = dict(os.environ, GLOO_SOCKET_IFNAME="lo")
        t = time.time()
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=GROUP_TIMEOUT[world])
        wall = time.time() - t
        ranks = []
        for q in range(world):
            path = "%s.rank%d.json" % (out, q)
            if os.path.exists(path):
                with open(path) as f:
                    ranks.append(json.load(f))
        errors = [x["error"] for x in ranks if "error" in x]
        assert r.returncode == 0, (cmd, errors, r.stdout[-2000:], r.stderr[-6000:])
        assert len(ranks) == world and not errors and all(len(x["results"]) == len(cases) for x in ranks)
        by_world[world] = {"cases": cases, "ranks": ranks, "wall": wall}
        startup = max(x["startup_seconds"] for x in ranks)
        per_case = [max(x["seconds"][i] for x in ranks) for i in range(len(cases))]
        print("\n[ranks on one device] world %d: group wall %.1f s; start-up to the first case (torch import, gloo group, device) %.1f s; cases %.1f s: %s"
              % (world, wall, startup, sum(per_case), ", ".join("%s %.2f" % (c.get("protocol", c["case"]), s) for c, s in zip(cases, per_case))))
    return by_world


def _results(runs, world, case):
    """Every rank's result of `case` in the group of `world` ranks."""
    i = runs[world]["cases"].index(case)
    return [x["results"][i] for x in sorted(runs[world]["ranks"], key=lambda x: x["rank"])]


@pytest.mark.parametrize("world", WORLDS)
def test_native_distributed_full_size_fft(runs, world):
    """iopx_add_fft_gf192_dist_dev / _ifft_ at m = 6 (standard basis, zero shift), 8 (random basis and shift) and 11 (standard basis, shift 1 << m):
    forward, inverse of its own output and inverse of independent evaluations equal the oracle's slices bit for bit on every rank; for 4 and 8
    ranks the entry refuses m = 2 log2(world) - 1 without issuing a collective."""
    for rank, res in enumerate(_results(runs, world, {"case": "fft"})):
        res = dict(res, digests=[[bytes.fromhex(d) for d in one] for one in res["digests"]])
        assert sn.native_fft_verdicts(res, rank, world) == [True] * (9 if world == 2 else 12), (rank, res)
        assert res["collectives"] > 0


def _check_prover(runs, world, case):
    ref, ref_roots = sn.prove_expected(case["protocol"], case["field_code"], case["log_n"], case["num_inputs"], case["seed"], case["rs_extra"])
    for rank, res in enumerate(_results(runs, world, case)):
        assert bytes.fromhex(res["transcript"]) == ref, "rank %d: transcript differs from the oracle prover's" % rank
        assert [bytes.fromhex(r) for r in res["roots"]] == ref_roots, "rank %d index roots" % rank
        assert res["ranks_agree"], rank
        assert res["stats"][0] > 0, "no collective was issued"


@pytest.mark.parametrize("world,log_n,rs_extra", AURORA_GF192)
def test_native_sharded_aurora_prover_equals_oracle(runs, world, log_n, rs_extra):
    _check_prover(runs, world, _prove("aurora", 0, log_n, 15, 0x2204, rs_extra))


@pytest.mark.parametrize("world,log_n", AURORA_PRIME)
def test_native_sharded_aurora_prover_over_the_prime_field_equals_oracle(runs, world, log_n):
    _check_prover(runs, world, _prove("aurora", 1, log_n, 15, 0x2204, 5))


@pytest.mark.parametrize("world,field_code,log_n,num_inputs", FRACTAL)
def test_native_sharded_fractal_prover_equals_oracle(runs, world, field_code, log_n, num_inputs):
    _check_prover(runs, world, _prove("fractal", field_code, log_n, num_inputs, 0x2205, 3))


@pytest.mark.parametrize("world,field_code,dim", FRI)
def test_native_sharded_fri_snark_equals_oracle(runs, world, field_code, dim):
    _check_prover(runs, world, _prove("fri", field_code, dim, 8, 5, 2))


@pytest.mark.parametrize("world,field_code,log_n", BAD_WITNESS)
def test_native_sharded_unsatisfied_witness_takes_the_reference_schedule_on_every_rank(runs, world, field_code, log_n, monkeypatch):
    """The all-reduced mismatch count makes EVERY rank fall back: the bytes of the single-process prover run with IOPX_HEAD_EVAL=0."""
    import torch
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    expected = sn.bad_witness_expected(lib, field_code, log_n, monkeypatch.setenv, monkeypatch.delenv, torch.device("cuda:0"))
    res = _results(runs, world, {"case": "bad_witness", "field_code": field_code, "log_n": log_n})
    for rank, one in enumerate(res):
        assert bytes.fromhex(one["transcript"]) == expected, "rank %d" % rank
        assert one["ranks_agree"]
    combines = [one["ldt_combines"] for one in res]
    assert all(c >= 1 for c in combines) and sum(combines) == world + 2, combines


@pytest.mark.parametrize("world", WORLDS)
def test_phase1_split_over_the_ranks(runs, world):
    """run_phase1's split with the default tile geometry and only IOPX_P1_SHARD_MIN_D lowered, at the smallest m at which the forward transform,
    the inverse and the short-input extension all split (sharded_native_cases.phase1_min_m): the oracle's results, and collectives from each."""
    case = _phase1_small(world)
    (m, kind), = case["shapes"]
    for rank, (one,) in enumerate(_results(runs, world, case)):
        assert [bytes.fromhex(d) for d in one["digests"]] == sn.phase1_expected(m, kind), (rank, m)
        assert all(c > 0 for c in one["collectives"]), "a transform did not split: %r" % (one["collectives"],)


@pytest.mark.parametrize("world", WORLDS)
def test_phase1_split_at_the_default_threshold(runs, world):
    """m = 16 with nothing set: the bound transforms equal the same library's unbound ones (pinned by tests/test_gpu_fullsize.py), and the forward
    and inverse transforms (d = 16) issued collectives; the extension's phase 1 (d = 14) is below the threshold and stays whole."""
    for rank, (one,) in enumerate(_results(runs, world, PHASE1_DEFAULT)):
        assert one["digests"] == one["unbound"], rank
        assert one["collectives"][0] > 0 and one["collectives"][1] > 0 and one["collectives"][2] == 0, one["collectives"]
