#!/usr/bin/env python3
"""Rates of the picked recurrence behind green() on gapped s-wave lattices (Γ = 0.05, 4 source rows, 1 and 16
targets) against the one-step recurrence on the same matrix at the same lanes per row, and the wall time of
green() next to ldos() on 64x64 (profiles/green.json).  Medians of `--repeats` runs.  Needs a GPU.

    python3 tools/green_benchmark.py [--out FILE] [--sizes 256,1000] [--repeats 5] [--moments 1024]
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
from bodge_amd import chebyshev as cheb
from bodge_amd.observables import _scale_of

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--sizes", default="256,1000")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--moments", type=int, default=0, help="moments per timed call (default: the rule for Γ = 0.05)")
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
for L in (int(v) for v in args.sizes.split(",")):
    system = gapped_swave(L)
    solver = system._solver()
    scale = _scale_of(system)
    moments = args.moments or cheb.moments_for_resolvent(scale, 0.05, 12.0)
    site = system.lattice[(L // 2, L // 2, 0)]
    rows = 4 * site + np.arange(4, dtype=np.int64)
    rec = {"moments": moments, "scale": scale}
    for n_targets in (1, 16):
        targets = (site + np.arange(n_targets)).astype(np.int32)
        solver.green_moments(scale, 32, rows, targets)  # warm-up (tables, buffers, kernel load)
        rates, windows = [], []
        for _ in range(args.repeats):
            solver.green_moments(scale, moments, rows, targets)
            p = solver.perf()
            rates.append(p["vector_steps"] / (p["window_ms"] / 1e3))
            windows.append(p["window_ms"])
        rec[f"targets_{n_targets}"] = {
            "vector_steps_per_s": median(rates), "window_ms": median(windows), "launches": p["launches"],
            "bytes_per_launch": p["bytes_per_launch"], "lanes_per_row": p["lanes_per_row"],
            "vectors_per_launch": p["vectors_per_launch"], "green": p["green"], "ranges": p["green_ranges"],
            "real": p["real_arithmetic"], "ph": p["ph_packed"], "grid": p["grid"],
            "us_per_launch": 1e3 * median(windows) / p["launches"],
            "GBps": p["bytes_per_launch"] * p["launches"] / (median(windows) / 1e3) / 1e9}
    # the one-step recurrence with dot products on the same matrix: 4 unit start vectors, same lanes per row,
    # multi-step kernels switched off
    lanes = rec["targets_1"]["lanes_per_row"]
    with backend.options(BODGE_AMD_SWEEP="0", BODGE_AMD_NO_BAND="1"):
        solver.set_lanes_per_row(lanes)
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
    for n_targets in (1, 16):
        rec[f"targets_{n_targets}"]["over_one_step"] = (rec[f"targets_{n_targets}"]["vector_steps_per_s"] /
                                                        rec["one_step"]["vector_steps_per_s"])
    out[f"{L}x{L}"] = rec
    print(json.dumps({f"{L}x{L}": rec}), flush=True)

# green() next to ldos() on 64x64: 13 energies, the default broadening
system = gapped_swave(64)
site = (32, 32, 0)
energies = np.linspace(0.0, 1.2, 13)
system.green(site, energies[:3])
system.ldos(site, energies[:3])
walls = {"green": [], "ldos": []}
for _ in range(args.repeats):
    t0 = time.time()
    g = system.green(site, energies)
    walls["green"].append(time.time() - t0)
    t0 = time.time()
    rho = system.ldos(site, energies)
    walls["ldos"].append(time.time() - t0)
rec = {"moments": g.info["moments"], "green_wall_s": median(walls["green"]), "ldos_wall_s": median(walls["ldos"]),
       "green_over_ldos": median(walls["green"]) / median(walls["ldos"]),
       "max_relative_difference": float(np.abs(g.ldos() / np.asarray(rho) - 1).max())}
out["64x64_green_vs_ldos"] = rec
print(json.dumps({"64x64_green_vs_ldos": rec}), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
