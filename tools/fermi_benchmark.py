#!/usr/bin/env python3
"""fermi_matrix rates on gapped s-wave lattices (T = 0.05, distance 16) against the one-step recurrence at the
same lanes per row and width (profiles/fermi_matrix.json).  Needs a GPU.

    python3 tools/fermi_benchmark.py [--out FILE] [--sizes 256,1000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bodge_amd as ba
from bodge_amd.observables import _scale_of

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--sizes", default="256,1000")
args = ap.parse_args()
out = {}
for L in (int(v) for v in args.sizes.split(",")):
    lattice = ba.CubicLattice((L, L, 1))
    system = ba.Hamiltonian(lattice)
    with system as (H, D):
        H.set_sites(-0.5 * ba.σ0)
        D.set_sites(1.0 * ba.jσ2)
        H.set_bonds(-1.0 * ba.σ0)
    system.fermi_matrix(0.5, method="chebyshev", distance=16)  # warm-up (tables, buffers, kernel load)
    t0 = time.time()
    fm = system.fermi_matrix(0.05, method="chebyshev", distance=16)
    wall = time.time() - t0
    p = fm.info["perf"]
    rec = {"wall_s": wall, "moments": fm.info["moments"], "colours": fm.info["colours"], "components": fm.info["components"],
           "vector_steps": p["vector_steps"], "window_ms": p["window_ms"], "kernel_ms": p["kernel_ms"],
           "bytes_moved": p["bytes_moved"], "launches": p["launches"], "lanes_per_row": p["lanes_per_row"],
           "vectors_per_launch": p["vectors_per_launch"], "clenshaw": p["clenshaw"], "streams": p["streams"],
           "real": p["real_arithmetic"], "ph": p["ph_packed"], "grid": p["grid"],
           "vector_steps_per_s": p["vector_steps"] / (p["window_ms"] / 1e3),
           "GBps": p["bytes_moved"] / (p["window_ms"] / 1e3) / 1e9,
           "density_mean": float(fm.density().mean()), "pair_mean": float(fm.pair_amplitude().real.mean())}
    solver = system._solver()
    solver.set_lanes_per_row(p["lanes_per_row"])
    width = p["vectors_per_launch"]
    scale = _scale_of(system)
    solver.dots_random(scale, 16, width)
    solver.dots_random(scale, 512, width)
    q = solver.perf()
    solver.set_lanes_per_row(0)
    rec["one_step"] = {"vector_steps_per_s": q["vector_steps"] / (q["window_ms"] / 1e3), "window_ms": q["window_ms"],
                       "bytes_moved": q["bytes_moved"], "launches": q["launches"], "dict_blocks": q["dict_blocks"],
                       "lanes_per_row": q["lanes_per_row"], "vectors_per_launch": q["vectors_per_launch"], "streams": q["streams"],
                       "GBps": q["bytes_moved"] / (q["window_ms"] / 1e3) / 1e9}
    rec["clenshaw_over_one_step"] = rec["vector_steps_per_s"] / rec["one_step"]["vector_steps_per_s"]
    out[f"{L}x{L}"] = rec
    print(json.dumps({f"{L}x{L}": rec}), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
