#!/usr/bin/env python3
"""Launch statistics of the upper butterfly kernels by tile height, from rocprofv3 --kernel-trace databases (rocpd sqlite) of the bench command.

Usage: upper_rates.py <label>=<results.db> [...] --out profiles/r07_upper_rates.json
A launch's tile height follows from its LDS request (24 bytes per element, 64 columns: 2^(6 + A) elements), its butterflies from the workgroup
count: cycles per wave-butterfly per SIMD = time x 2.4 GHz x 1024 SIMDs / (butterflies / 64), as tools/edge_rates.py counts them."""
import argparse
import collections
import json
import sqlite3

CLOCK, SIMDS = 2.4e9, 1024


def launches(path):
    c = sqlite3.connect(path)
    tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
    suf = [t for t in tabs if t.startswith("rocpd_metadata")][0][len("rocpd_metadata"):]
    q = ("select s.kernel_name, d.group_segment_size, d.grid_size_x, d.workgroup_size_x, d.end - d.start from rocpd_kernel_dispatch%s d "
         "join rocpd_info_kernel_symbol%s s on d.kernel_id = s.id where s.kernel_name like '%%k_bfly_upper%%'" % (suf, suf))
    return c.execute(q).fetchall()


def summarise(path):
    acc = collections.defaultdict(lambda: [0, 0.0, 0.0, collections.Counter()])
    for name, lds, grid, wg, ns in launches(path):
        elems = lds // 24
        levels = elems.bit_length() - 1 - 6                     # a one-level tile requests LDS it does not use
        inverse = "ILb1" in name.split("k_bfly_upper")[1][:12]  # first template argument: INV
        bfl = (grid // wg) * elems / 2 * levels
        for key in (("inv" if inverse else "fwd", levels), ("inv" if inverse else "fwd", "all")):
            a = acc[key]
            a[0] += 1; a[1] += ns * 1e-6; a[2] += bfl; a[3][wg] += 1
    out = {}
    for (d, lv), (calls, ms, bfl, wgs) in sorted(acc.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
        out["k_bfly_upper_%s levels=%s" % (d, lv)] = {
            "launches": calls, "ms": round(ms, 3), "avg_us": round(1e3 * ms / calls, 2), "butterflies": bfl, "threads_per_workgroup": sorted(wgs),
            "cycles_per_wave_butterfly_per_simd": round(ms * 1e-3 * CLOCK * SIMDS / (bfl / 64), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dbs", nargs="+", metavar="label=results.db")
    ap.add_argument("--out", required=True)
    ap.add_argument("--what", default="k_bfly_upper launches of `python bench.py --gpus 1 --steps 20 --warmup 5` under rocprofv3 --kernel-trace "
                                      "(27 proofs, trees on the main stream), the builds traced one after the other on one MI355X")
    a = ap.parse_args()
    out = {"source": "tools/upper_rates.py", "what": a.what, "builds": {}}
    for item in a.dbs:
        label, path = item.split("=", 1)
        out["builds"][label] = summarise(path)
    json.dump(out, open(a.out, "w"), indent=1)
    for label, b in out["builds"].items():
        for k, v in b.items():
            print(label, k, v["launches"], v["ms"], v["avg_us"], v["cycles_per_wave_butterfly_per_simd"])


if __name__ == "__main__":
    main()
