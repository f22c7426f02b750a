#!/usr/bin/env python3
"""green_bonds() on the README's 64x64 model at 13 energies (profiles/green_bonds.json):

  (a) green_bonds() on all 4096 sites: wall time, recurrence launches and their HIP-event time, the contractions' time;
  (b) green_map() on all sites with the same moments: the local blocks only, contracted on the host;
  (c) a 64-site line cut: a loop of green(site, energies, targets=site + neighbours) against green_bonds(sites=cut).

Medians of `--repeats` calls after a warm-up.  Needs a GPU.

    python3 tools/green_bonds_benchmark.py [--out FILE] [--repeats 5] [--size 64]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bodge_amd as ba

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--size", type=int, default=64)
args = ap.parse_args()


def gapped_swave(L):
    lattice = ba.CubicLattice((L, L, 1))
    system = ba.Hamiltonian(lattice)
    with system as (H, D):
        H.set_sites(-0.5 * ba.σ0)
        D.set_sites(1.0 * ba.jσ2)
        H.set_bonds(-1.0 * ba.σ0)
    return system


def median(values):
    return float(np.median(values))


def records(info):
    """The perf records of a call (one per host group) summed where they add up."""
    groups = info["perf"] if isinstance(info["perf"], list) else [info["perf"]]
    total = dict(groups[0])
    for key in ("launches", "vector_steps", "kernel_ms", "window_ms", "bytes_moved"):
        total[key] = sum(g[key] for g in groups)
    total["host_groups"] = len(groups)
    return total


L = args.size
system = gapped_swave(L)
energies = np.linspace(0.0, 1.2, 13)
cut = [(x, L // 2, 0) for x in range(L)]
neighbours = {site: [site] + [(site[0] + dx, site[1] + dy, 0) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))
                              if 0 <= site[0] + dx < L and 0 <= site[1] + dy < L] for site in cut}
system.green_bonds(energies[:3], cut[:4])  # warm-up (tables, buffers, kernel load)
system.green_map(energies[:3], cut[:4])
system.green(cut[0], energies[:3], targets=neighbours[cut[0]])

walls = {"bonds": [], "map": [], "bonds_cut": [], "loop": []}
perf = {"bonds": [], "map": []}
for _ in range(args.repeats):
    t0 = time.time()
    bonds = system.green_bonds(energies)
    walls["bonds"].append(time.time() - t0)
    perf["bonds"].append(records(bonds.info))
    t0 = time.time()
    mapped = system.green_map(energies, moments=bonds.info["moments"])
    walls["map"].append(time.time() - t0)
    perf["map"].append(records(mapped.info))
    t0 = time.time()
    line = system.green_bonds(energies, cut)
    walls["bonds_cut"].append(time.time() - t0)
    t0 = time.time()
    single = [system.green(site, energies, targets=neighbours[site]) for site in cut]
    walls["loop"].append(time.time() - t0)

difference_loop = max(float(np.abs(line.block(target, site) - g.blocks[t]).max())
                      for site, g in zip(cut, single) for t, target in enumerate(neighbours[site]))
difference_map = float(np.abs(bonds.local().blocks - mapped.blocks).max())
b, m = perf["bonds"][-1], perf["map"][-1]
kernel = {name: median([p["kernel_ms"] for p in perf[name]]) for name in perf}
window = {name: median([p["window_ms"] for p in perf[name]]) for name in perf}
rec = {
    "lattice": f"{L}x{L}", "energies": int(energies.size), "moments": bonds.info["moments"], "columns": bonds.info["columns"],
    "blocks": int(bonds.blocks.shape[0]),
    "a_green_bonds_all_sites": {
        "wall_s": median(walls["bonds"]), "launches": b["launches"], "recurrence_ms": kernel["bonds"], "window_ms": window["bonds"],
        "contraction_ms": window["bonds"] - kernel["bonds"], "us_per_launch": 1e3 * kernel["bonds"] / b["launches"],
        "bytes_per_launch": b["bytes_per_launch"], "ranges": b["green_ranges"], "host_groups": b["host_groups"],
        "lanes_per_row": b["lanes_per_row"], "vectors_per_launch": b["vectors_per_launch"], "green_bonds": b["green_bonds"],
        "result_bytes": int(bonds.blocks.nbytes)},
    "b_green_map_all_sites": {
        "wall_s": median(walls["map"]), "launches": m["launches"], "recurrence_ms": kernel["map"], "window_ms": window["map"],
        "us_per_launch": 1e3 * kernel["map"] / m["launches"], "bytes_per_launch": m["bytes_per_launch"],
        "host_groups": m["host_groups"], "lanes_per_row": m["lanes_per_row"], "vectors_per_launch": m["vectors_per_launch"],
        "moment_table_bytes": int(bonds.info["moments"] * mapped.blocks.shape[0] * 4 * mapped.info["columns"] * 16)},
    "c_line_cut_64_sites": {
        "green_bonds_wall_s": median(walls["bonds_cut"]), "loop_of_green_wall_s": median(walls["loop"]),
        "launches": line.info["perf"]["launches"], "blocks": int(line.blocks.shape[0]),
        "max_difference_bonds_vs_loop": difference_loop},
    "max_difference_local_vs_green_map": difference_map,
}
rec["recurrence_ms_a_over_b"] = kernel["bonds"] / kernel["map"]
rec["window_ms_a_over_b"] = window["bonds"] / window["map"]
rec["wall_a_over_b"] = rec["a_green_bonds_all_sites"]["wall_s"] / rec["b_green_map_all_sites"]["wall_s"]
rec["line_cut_speedup_over_loop"] = rec["c_line_cut_64_sites"]["loop_of_green_wall_s"] / rec["c_line_cut_64_sites"]["green_bonds_wall_s"]
print(json.dumps(rec), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
