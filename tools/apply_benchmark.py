#!/usr/bin/env python3
"""Rate of the stored-source Clenshaw step of apply() / evolve() on gapped s-wave lattices against the one-step
recurrence with dot products at the same lanes per row (profiles/apply.json).  Needs a GPU.

    python3 tools/apply_benchmark.py [--out FILE] [--sizes 256,1000] [--moments 512]

Per size: one full batch of columns (the width rule's), M coefficients, median of five calls after a warm-up,
HIP-event window of the call; the baseline is bdg_cheb_dots_unit on the same matrix, lanes and number of launches
with the stencil kernels and the growing band switched off.  Rates are algorithmic bytes per second of window: a
stored-source step counts four vector passes (read b_{k+1}, b_{k+2} and x, write b_k), a one-step launch three.
Also the wall time of evolve() on 64x64 for 16 times up to a·t = 200.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bodge_amd as ba
from bodge_amd import backend
from bodge_amd.observables import _scale_of


def gapped_swave(L):
    system = ba.Hamiltonian(ba.CubicLattice((L, L, 1)))
    with system as (H, D):
        H.set_sites(-0.5 * ba.σ0)
        D.set_sites(1.0 * ba.jσ2)
        H.set_bonds(-1.0 * ba.σ0)
    return system


def rate(perf):
    return perf["bytes_moved"] / (perf["window_ms"] / 1e3) / 1e9


ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--sizes", default="256,1000")
ap.add_argument("--moments", type=int, default=512)
args = ap.parse_args()
out = {}
rng = np.random.default_rng(0)
for L in (int(v) for v in args.sizes.split(",")):
    system = gapped_swave(L)
    solver = system._solver()
    scale = _scale_of(system)
    coef = (rng.standard_normal((args.moments, 1)) + 1j * rng.standard_normal((args.moments, 1))) / (1 + np.arange(args.moments))[:, None]
    solver.apply_series(scale, coef[:2], np.ones((1, solver.dim)))  # warm-up (tables, buffers, kernel load)
    # a full batch by the width rule: one vector buffer (64 B per site and column) within 96 MB, 64 columns at most, 32 real
    columns = 32 if solver.perf()["real_arithmetic"] else 64
    while columns > 4 and columns * 64.0 * system.lattice.size > 96.0 * 1024 * 1024:
        columns //= 2
    x = rng.standard_normal((columns, solver.dim)) + 1j * rng.standard_normal((columns, solver.dim))
    runs = []
    for _ in range(6):
        t0 = time.time()
        solver.apply_series(scale, coef, x)
        p = solver.perf()
        runs.append({"wall_s": time.time() - t0, "window_ms": p["window_ms"], "GBps": rate(p)})
    runs = runs[1:]
    rec = {"columns": columns, "moments": args.moments, "launches": p["launches"], "lanes_per_row": p["lanes_per_row"],
           "vectors_per_launch": p["vectors_per_launch"], "apply": p["apply"], "dict_blocks": p["dict_blocks"],
           "real": p["real_arithmetic"], "ph": p["ph_packed"], "streams": p["streams"], "grid": p["grid"],
           "bytes_per_launch": p["bytes_per_launch"], "bytes_moved": p["bytes_moved"],
           "window_ms": [r["window_ms"] for r in runs], "wall_s": [r["wall_s"] for r in runs],
           "window_ms_median": statistics.median(r["window_ms"] for r in runs),
           "GBps": statistics.median(r["GBps"] for r in runs)}
    # the one-step recurrence with dot products: same matrix, same lanes, as many launches, no stencil kernels, no band
    rows = np.arange(p["vectors_per_launch"], dtype=np.int64) * 4 * (system.lattice.size // p["vectors_per_launch"])
    solver.set_lanes_per_row(p["lanes_per_row"])
    base = []
    with backend.options(BODGE_AMD_SWEEP="0", BODGE_AMD_NO_BAND="1"):
        for _ in range(6):
            solver.dots_unit(scale, args.moments, rows)
            q = solver.perf()
            base.append({"window_ms": q["window_ms"], "GBps": rate(q)})
    solver.set_lanes_per_row(0)
    base = base[1:]
    rec["one_step"] = {"launches": q["launches"], "lanes_per_row": q["lanes_per_row"], "vectors_per_launch": q["vectors_per_launch"],
                       "steps_per_launch": q["steps_per_launch"], "dict_blocks": q["dict_blocks"], "real": q["real_arithmetic"],
                       "streams": q["streams"], "bytes_per_launch": q["bytes_per_launch"], "bytes_moved": q["bytes_moved"],
                       "window_ms": [r["window_ms"] for r in base],
                       "window_ms_median": statistics.median(r["window_ms"] for r in base),
                       "GBps": statistics.median(r["GBps"] for r in base)}
    rec["apply_over_one_step_GBps"] = rec["GBps"] / rec["one_step"]["GBps"]
    out[f"{L}x{L}"] = rec
    print(json.dumps({f"{L}x{L}": rec}), flush=True)
    del x, solver, system

system = gapped_swave(64)
scale = _scale_of(system)
times = np.linspace(0.0, 200.0 / scale, 16)
psi = np.zeros((system.lattice.size, 4), dtype=np.complex128)
psi[system.lattice[(32, 30, 0)], 0] = 1.0
system.evolve(psi, times[:2])  # warm-up
walls = []
for _ in range(5):
    t0 = time.time()
    moved = system.evolve(psi, times)
    walls.append(time.time() - t0)
p = system._solver().perf()
out["evolve_64x64_16_times"] = {"wall_s": walls, "wall_s_median": statistics.median(walls), "launches": p["launches"],
                                "window_ms": p["window_ms"], "lanes_per_row": p["lanes_per_row"], "apply": p["apply"],
                                "norm_drift": float(np.abs(np.linalg.norm(moved.reshape(16, -1), axis=1) - 1).max())}
print(json.dumps({"evolve_64x64_16_times": out["evolve_64x64_16_times"]}), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
