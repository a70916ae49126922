"""Worker of tests/test_gpu_ranks_one_device.py: one rank of a `python -m torch.distributed.run` job whose ranks ALL open GPU 0.  The process
group is gloo (host tensors); the library's collectives reach it through comm_create_torch_callbacks(staged=True), which reads every send buffer
back from the device and writes every receive buffer to it on the library's stream.  So the world > 1 branches of libiop_amd/cpp/dist.hpp,
fft_add_dist.hip and run_phase1 run as gfx950 code with real peers, on a box with one GPU.

Runs every case of --cases (a JSON list, tests/test_gpu_ranks_one_device.py builds it) in order through tests/sharded_native_cases.py and writes
this rank's results (hex strings, counts, seconds) to <out>.rank<r>.json.  A rank that hits an exception writes what it has, with the error,
and exits non-zero at once — its peers are already inside the next collective, and the launcher tears the group down."""
import argparse
import hashlib
import json
import os
import sys
import time
from datetime import timedelta

T0 = time.time()
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _agree(dist, torch, world, payload):
    """True when every rank holds the same bytes: digests compared over the group."""
    h = torch.tensor(list(hashlib.blake2b(payload, digest_size=32).digest()), dtype=torch.uint8)
    hs = [torch.empty_like(h) for _ in range(world)]
    dist.all_gather(hs, h)
    return all(bool(torch.equal(x, h)) for x in hs)


def run_case(c, lib, comm, torch, dist, rank, world):
    import sharded_native_cases as sn
    kind = c["case"]
    if kind == "fft":
        res = sn.native_fft(lib, comm, rank, world)
        return {"digests": [[d.hex() for d in one] for one in res["digests"]], "collectives": res["collectives"], "refused": res["refused"]}
    if kind == "prove":
        t, roots, stats = sn.native_prove(lib, comm, c["protocol"], c["field_code"], c["log_n"], c["num_inputs"], c["seed"], c["rs_extra"])
        return {"transcript": t.hex(), "roots": [r.hex() for r in roots], "stats": list(stats), "ranks_agree": _agree(dist, torch, world, t + b"".join(roots))}
    if kind == "bad_witness":
        t, combines = sn.bad_witness_prove(lib, comm, c["field_code"], c["log_n"], torch.device("cuda:0"))
        return {"transcript": t.hex(), "ldt_combines": combines, "ranks_agree": _agree(dist, torch, world, t)}
    if kind == "phase1":
        if c["min_d"] is not None:
            lib.set_option("IOPX_P1_SHARD_MIN_D", c["min_d"])
        try:
            res = sn.phase1_split(lib, comm, [tuple(s) for s in c["shapes"]], against_unbound=c["against_unbound"])
        finally:
            if c["min_d"] is not None:
                lib.clear_option("IOPX_P1_SHARD_MIN_D")
        return [{k: ([d.hex() for d in v] if k != "collectives" else v) for k, v in one.items()} for one in res]
    raise ValueError("unknown case %r" % kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--group-timeout", type=float, default=60.0, help="seconds a gloo collective waits for its peers before it raises")
    args = ap.parse_args()
    cases = json.loads(args.cases)

    import torch
    import torch.distributed as dist
    import libiop_amd

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group(backend="gloo", timeout=timedelta(seconds=args.group_timeout))
    lib = libiop_amd.lib()                  # raises if the HIP library is missing: no fallback
    lib.init(0)                             # every rank on the one device
    torch.cuda.set_device(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)      # the unsatisfied-witness case builds its instance with torch tensors
    comm = lib.comm_create_torch_callbacks(dist, rank, world, staged=True)
    out = {"rank": rank, "world": world, "startup_seconds": time.time() - T0, "results": [], "seconds": []}
    code = 0
    try:
        for c in cases:
            t = time.time()
            out["results"].append(run_case(c, lib, comm, torch, dist, rank, world))
            out["seconds"].append(time.time() - t)
    except Exception as e:                  # noqa: BLE001 — no later case: the peers are inside its collectives
        import traceback
        traceback.print_exc()
        out["error"] = "case %d: %s: %s" % (len(out["results"]), type(e).__name__, e)
        code = 1
    with open("%s.rank%d.json" % (args.out, rank), "w") as f:
        json.dump(out, f)
    if code:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(code)                      # no teardown that would wait for the peers
    lib.comm_destroy(comm)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
