#!/usr/bin/env python3
"""Rates of the projected recurrence behind green_states() / spectral_function() on gapped s-wave lattices against the
one-step recurrence with dot products at the same lanes per row, and the wall time of spectral_function() on 64x64 for
a k-path of 64 points at 13 energies (profiles/green_states.json).  Medians of `--repeats` calls after
a warm-up, HIP-event windows.  Needs a GPU.

    python3 tools/green_states_benchmark.py [--out FILE] [--sizes 256,1000] [--repeats 5] [--moments 512]

A lane payload of the projected recurrence is one complex column in every mode; in real arithmetic the one-step
recurrence carries two real vectors in the same payload.  At equal lanes per row the two launches move the same vector
bytes, so the ratio that compares them is that of the payload-steps per second (`over_one_step`), which is the inverse
ratio of the times per launch.
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
    lattice = system.lattice
    solver = system._solver()
    scale = _scale_of(system)
    moments = args.moments
    probe = lattice.plane_waves(np.array([[0.1 * (q + 1), 0.07 * (q + 1), 0.0] for q in range(16)]))
    probe = np.concatenate([probe, probe.conj()])
    solver.green_state_moments(scale, 4, probe, 2)  # (finds the lanes of a batch on this lattice)
    lanes = solver.perf()["lanes_per_row"]
    states = probe[np.r_[0 : lanes // 4, 16 : 16 + lanes // 4]]  # one full batch: lanes / 2 states (k and -k), 2 columns each
    solver.green_state_moments(scale, 32, states, 2)  # warm-up (tables, buffers, kernel load)
    rates, windows = [], []
    for _ in range(args.repeats):
        solver.green_state_moments(scale, moments, states, 2)
        p = solver.perf()
        rates.append(p["vector_steps"] / (p["window_ms"] / 1e3))
        windows.append(p["window_ms"])
    rec = {"moments": moments, "scale": scale, "states_per_batch": int(states.shape[0])}
    rec["green_states"] = {
        "column_steps_per_s": median(rates), "window_ms": median(windows), "launches": p["launches"],
        "bytes_per_launch": p["bytes_per_launch"], "lanes_per_row": p["lanes_per_row"],
        "vectors_per_launch": p["vectors_per_launch"], "green_states": p["green_states"], "ranges": p["green_ranges"],
        "real": p["real_arithmetic"], "ph": p["ph_packed"], "grid": p["grid"], "lds_bytes": p["lds_bytes"],
        "us_per_launch": 1e3 * median(windows) / p["launches"],
        "GBps": p["bytes_per_launch"] * p["launches"] / (median(windows) / 1e3) / 1e9}
    # the one-step recurrence with dot products on the same matrix at the same lanes per row (unit start vectors in the
    # middle of the lattice), multi-step kernels and the band of a unit start switched off
    n_vectors = p["vectors_per_launch"]
    first = lattice[(L // 2, L // 2 - n_vectors // 4, 0)]
    rows = (4 * (first + np.arange(n_vectors // 2)).astype(np.int64)[:, None] + np.arange(2)[None, :]).reshape(-1)
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
                       "bytes_per_launch": q["bytes_per_launch"],
                       "us_per_launch": 1e3 * median(windows) / max(1, q["launches"]),
                       "GBps": q["bytes_per_launch"] * q["launches"] / (median(windows) / 1e3) / 1e9}
    rec["green_states"]["over_one_step"] = rec["one_step"]["us_per_launch"] / rec["green_states"]["us_per_launch"]
    rec["green_states"]["GBps_over_one_step"] = rec["green_states"]["GBps"] / rec["one_step"]["GBps"]
    out[f"{L}x{L}"] = rec
    print(json.dumps({f"{L}x{L}": rec}), flush=True)
    del solver, system

# ---------------------------------------------------------------- end to end on 64x64: a k-path of 64 points, 13 energies
system = gapped_swave(64)
energies = np.linspace(0.0, 1.2, 13)
corners = np.array([[0.0, 0.0, 0.0], [np.pi, 0.0, 0.0], [np.pi, np.pi, 0.0], [0.0, 0.0, 0.0]])  # Γ - X - M - Γ
path = np.concatenate([corners[i] + (corners[i + 1] - corners[i]) * np.linspace(0, 1, 22, endpoint=False)[:, None]
                       for i in range(3)])[:64]
system.spectral_function(path[:2], energies[:3])
walls = []
for _ in range(args.repeats):
    t0 = time.time()
    a = system.spectral_function(path, energies)
    walls.append(time.time() - t0)
groups = a.info["perf"] if isinstance(a.info["perf"], list) else [a.info["perf"]]
launches = sum(g["launches"] for g in groups)
window = sum(g["window_ms"] for g in groups)
rec = {"moments": a.info["moments"], "energies": int(energies.size), "momenta": int(path.shape[0]),
       "columns": a.info["columns"], "wall_s": median(walls), "launches": launches, "window_ms": window,
       "us_per_launch": 1e3 * window / launches, "lanes_per_row": groups[0]["lanes_per_row"],
       "green_states": groups[0]["green_states"], "ranges": groups[0]["green_ranges"],
       "peak_of_A_at_gamma": float(a.spectral()[0].max())}
out["64x64_k_path"] = rec
print(json.dumps({"64x64_k_path": rec}), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
