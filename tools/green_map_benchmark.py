#!/usr/bin/env python3
"""Rates of the full-width picked recurrence behind green_map() on gapped s-wave lattices against the one-step
recurrence with dot products at the same width and lanes per row, and the wall time of green_map() on 64x64 (a line
cut of 64 sites, all 4096 sites, 13 energies) next to a loop of green() over the same sites
(profiles/green_map.json).  Medians of `--repeats` calls after a warm-up.  Needs a GPU.

    python3 tools/green_map_benchmark.py [--out FILE] [--sizes 256,1000] [--repeats 5] [--moments 512]
                                         [--loop-baseline FILE]

`--loop-baseline` merges a record {"loop_64_sites_wall_s": ...} of the same loop of green() measured with another
build of the library (the commit before green_map) in the same session.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bodge_amd as ba
from bodge_amd import backend
from bodge_amd.observables import _scale_of

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--sizes", default="256,1000")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--moments", type=int, default=512, help="moments per timed call of the per-launch part")
ap.add_argument("--loop-baseline")
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


out = {}
# ---------------------------------------------------------------- per launch: one full batch against the one-step recurrence
for L in (int(v) for v in args.sizes.split(",")):
    system = gapped_swave(L)
    solver = system._solver()
    scale = _scale_of(system)
    moments = args.moments
    solver.green_local_moments(scale, 8, np.arange(64, dtype=np.int32), 2)  # (finds the width of a batch on this lattice)
    width = solver.perf()["vectors_per_launch"]
    first = system.lattice[(L // 2, L // 2 - width // 4, 0)]
    sites = (first + np.arange(width // 2)).astype(np.int32)  # one full batch: width / 2 sites of a lattice row, 2 columns each
    solver.green_local_moments(scale, 32, sites, 2)  # warm-up (tables, buffers, kernel load)
    rates, windows = [], []
    for _ in range(args.repeats):
        solver.green_local_moments(scale, moments, sites, 2)
        p = solver.perf()
        rates.append(p["vector_steps"] / (p["window_ms"] / 1e3))
        windows.append(p["window_ms"])
    rec = {"moments": moments, "scale": scale, "sites_per_batch": int(sites.size)}
    rec["green_local"] = {
        "vector_steps_per_s": median(rates), "window_ms": median(windows), "launches": p["launches"],
        "bytes_per_launch": p["bytes_per_launch"], "lanes_per_row": p["lanes_per_row"],
        "vectors_per_launch": p["vectors_per_launch"], "green_local": p["green_local"], "ranges": p["green_ranges"],
        "real": p["real_arithmetic"], "ph": p["ph_packed"], "grid": p["grid"],
        "us_per_launch": 1e3 * median(windows) / p["launches"],
        "GBps": p["bytes_per_launch"] * p["launches"] / (median(windows) / 1e3) / 1e9}
    # the one-step recurrence with dot products on the same matrix: the same unit start vectors, the same lanes per
    # row, multi-step kernels and the band of a unit start switched off
    rows = (4 * sites.astype(np.int64)[:, None] + np.arange(2)[None, :]).reshape(-1)
    with backend.options(BODGE_AMD_SWEEP="0", BODGE_AMD_NO_BAND="1"):
        solver.set_lanes_per_row(p["lanes_per_row"])
        solver.dots_unit(scale, 16, rows)
        rates, windows = [], []
        for _ in range(args.repeats):
            solver.dots_unit(scale, moments - 1, rows)
            q = solver.perf()
            rates.append(q["vector_steps"] / (q["window_ms"] / 1e3))
            windows.append(q["window_ms"])
        solver.set_lanes_per_row(0)
    rec["one_step"] = {"vector_steps_per_s": median(rates), "window_ms": median(windows), "launches": q["launches"],
                       "steps_per_launch": q["steps_per_launch"], "dict_blocks": q["dict_blocks"], "pipelined": q["pipelined"],
                       "lanes_per_row": q["lanes_per_row"], "vectors_per_launch": q["vectors_per_launch"],
                       "us_per_launch": 1e3 * median(windows) / max(1, q["launches"])}
    rec["green_local"]["over_one_step"] = rec["green_local"]["vector_steps_per_s"] / rec["one_step"]["vector_steps_per_s"]
    out[f"{L}x{L}"] = rec
    print(json.dumps({f"{L}x{L}": rec}), flush=True)

# ---------------------------------------------------------------- end to end on 64x64: 13 energies, the default broadening
system = gapped_swave(64)
energies = np.linspace(0.0, 1.2, 13)
cut = [(x, 32, 0) for x in range(64)]
system.green_map(energies[:3], cut[:4])
system.green(cut[0], energies[:3])
walls = {"cut": [], "loop": [], "full": []}
for _ in range(args.repeats):
    t0 = time.time()
    line = system.green_map(energies, cut)
    walls["cut"].append(time.time() - t0)
    t0 = time.time()
    single = [system.green(site, energies) for site in cut]
    walls["loop"].append(time.time() - t0)
    t0 = time.time()
    full = system.green_map(energies)
    walls["full"].append(time.time() - t0)
difference = max(float(np.abs(line.blocks[s] - g.blocks[0]).max()) for s, g in enumerate(single))
groups = full.info["perf"] if isinstance(full.info["perf"], list) else [full.info["perf"]]  # (one record per host group)
perf = dict(groups[0], launches=sum(g["launches"] for g in groups), window_ms=sum(g["window_ms"] for g in groups))
rec = {"moments": line.info["moments"], "energies": int(energies.size),
       "line_cut_64_sites_wall_s": median(walls["cut"]), "all_4096_sites_wall_s": median(walls["full"]),
       "loop_64_sites_wall_s": median(walls["loop"]),
       "loop_4096_sites_wall_s_scaled": 64 * median(walls["loop"]),  # (64 sites timed, times 64)
       "line_cut_launches": line.info["perf"]["launches"], "full_launches": perf["launches"],
       "full_window_ms": perf["window_ms"], "full_us_per_launch": 1e3 * perf["window_ms"] / perf["launches"],
       "host_groups": len(groups), "vectors_per_launch": perf["vectors_per_launch"], "lanes_per_row": perf["lanes_per_row"],
       "max_difference_map_vs_loop": difference}
if args.loop_baseline:
    with open(args.loop_baseline) as fh:
        before = json.load(fh)
    rec["loop_64_sites_wall_s_previous_library"] = before["loop_64_sites_wall_s"]
    rec["loop_4096_sites_wall_s_previous_library_scaled"] = 64 * before["loop_64_sites_wall_s"]
    loop = before["loop_64_sites_wall_s"]
else:
    loop = rec["loop_64_sites_wall_s"]
rec["line_cut_speedup_over_loop"] = loop / rec["line_cut_64_sites_wall_s"]
rec["full_map_speedup_over_loop"] = 64 * loop / rec["all_4096_sites_wall_s"]
out["64x64_map_vs_loop"] = rec
print(json.dumps({"64x64_map_vs_loop": rec}), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
