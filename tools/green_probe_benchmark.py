#!/usr/bin/env python3
"""green_map() and green_bonds() with distance= (probing) against the unprobed calls (profiles/green_probe.json,
DESIGN.md §22), on the README's gapped s-wave model at 13 energies:

  (a) 64 x 64, all sites: green_map(E) against green_map(E, distance=16) - wall time, launches, us per launch, bytes
      leaving the device, and the largest deviation of the probed LDOS from the exact one relative to the largest LDOS,
      inside and outside the gap, for signs +1 and for the mean of four ±1 samples;
  (b) the same for green_bonds() (deviation of all blocks, relative to the largest entry);
  (c) 256 x 256 and 1000 x 1000 with a position-dependent on-site block: green_map(E, distance=16) with samples 1 and 4 -
      wall time, kernel_ms, window_ms.  The unprobed call is not run at these sizes; its launch count is reported.

Medians of `--repeats` calls after a warm-up (`--large-repeats` for 1000 x 1000).  Every probed call is held to
launches = samples x ceil(colours·C / width) x (M - 1).  Needs a GPU.

    python3 tools/green_probe_benchmark.py [--out FILE] [--repeats 3] [--large-repeats 1] [--sizes 256,1000]
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
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--large-repeats", type=int, default=1)
ap.add_argument("--sizes", default="256,1000")
ap.add_argument("--distance", type=int, default=16)
args = ap.parse_args()
GAP = 1.0


def gapped_swave(L, disorder=0.0, seed=5):
    lattice = ba.CubicLattice((L, L, 1))
    system = ba.Hamiltonian(lattice)
    with system as (H, D):
        if disorder:
            potential = -0.5 + np.random.default_rng(seed).uniform(-disorder, disorder, L * L)
            H.set_sites(potential[:, None, None] * ba.σ0)
        else:
            H.set_sites(-0.5 * ba.σ0)
        D.set_sites(GAP * ba.jσ2)
        H.set_bonds(-1.0 * ba.σ0)
    return system


def median(values):
    return float(np.median(values))


def records(info):
    """The perf records of a call (one per host group) summed where they add up; a probed call's launch count checked."""
    groups = info["perf"] if isinstance(info["perf"], list) else [info["perf"]]
    if "distance" in info:
        steps, c, samples = info["moments"] - 1, info["columns"], info["samples"]
        for g in groups:
            colours = g["vector_steps"] // (samples * c * steps)
            batch = max(1, min(64, g["vectors_per_launch"], colours * c) // c)  # whole colours of a batch
            assert g["launches"] == samples * -(-colours // batch) * steps, (g["launches"], colours, batch)
    total = dict(groups[0])
    for key in ("launches", "vector_steps", "kernel_ms", "window_ms", "bytes_moved"):
        total[key] = sum(g[key] for g in groups)
    total["host_groups"] = len(groups)
    return total


def timed(call, repeats):
    walls, perf, result = [], [], None
    for _ in range(repeats):
        t0 = time.time()
        result = call()
        walls.append(time.time() - t0)
        perf.append(records(result.info))
    last = perf[-1]
    kernel, window = median([p["kernel_ms"] for p in perf]), median([p["window_ms"] for p in perf])
    out = {"wall_s": median(walls), "launches": last["launches"], "kernel_ms": kernel, "window_ms": window,
           "us_per_launch": 1e3 * kernel / last["launches"], "bytes_per_launch": last["bytes_per_launch"],
           "host_groups": last["host_groups"], "lanes_per_row": last["lanes_per_row"],
           "vectors_per_launch": last["vectors_per_launch"], "ranges": last["green_ranges"]}
    for key in ("colours", "periods", "samples"):
        if key in result.info:
            out[key] = result.info[key]
    return result, out


def deviation(probed, exact, inside):
    """max |probed - exact| over the energies `inside` and outside, relative to the largest |exact|."""
    difference = np.abs(probed - exact)
    top = float(np.abs(exact).max())
    return {"in_gap": float(difference[:, inside].max()) / top, "in_band": float(difference[:, ~inside].max()) / top}


energies = np.linspace(0.0, 1.2, 13)
inside = np.abs(energies) < GAP
d = args.distance
rec = {"energies": int(energies.size), "distance": d, "gap": GAP, "repeats": args.repeats}

# ---------------------------------------------------------------- (a), (b): 64 x 64, probed against unprobed
system = gapped_swave(64)
system.green_map(energies[:3], [(0, 0, 0), (5, 5, 0)])  # warm-up (tables, buffers, kernel load)
system.green_bonds(energies[:3], [(0, 0, 0), (5, 5, 0)])
system.green_map(energies[:3], distance=d, moments=32)
for name, call in (("a_green_map", system.green_map), ("b_green_bonds", system.green_bonds)):
    exact, plain = timed(lambda: call(energies), args.repeats)
    moments, columns = exact.info["moments"], exact.info["columns"]
    if name == "a_green_map":
        plain["bytes_leaving_device"] = int(moments * exact.blocks.shape[0] * 4 * columns * 16)  # the moment table
    else:
        plain["bytes_leaving_device"] = int(exact.blocks.nbytes)
    probed, one = timed(lambda: call(energies, distance=d), args.repeats)
    one["bytes_leaving_device"] = int(probed.blocks.nbytes)
    noisy, four = timed(lambda: call(energies, distance=d, samples=4), args.repeats)
    four["bytes_leaving_device"] = int(noisy.blocks.nbytes + noisy.stderr.nbytes)
    if name == "a_green_map":
        one["ldos_deviation"] = deviation(probed.ldos(), exact.ldos(), inside)
        four["ldos_deviation"] = deviation(noisy.ldos(), exact.ldos(), inside)
        four["largest_stderr_over_largest_block_entry"] = float(np.abs(noisy.stderr).max() / np.abs(exact.blocks).max())
    else:
        flat = lambda g: g.blocks.transpose(0, 2, 3, 1).reshape(-1, energies.size)
        one["block_deviation"] = deviation(flat(probed), flat(exact), inside)
        four["block_deviation"] = deviation(flat(noisy), flat(exact), inside)
    rec[name] = {"lattice": "64x64", "moments": moments, "columns": columns, "blocks": int(exact.blocks.shape[0]),
                 "unprobed": plain, "distance_signs_plus": one, "distance_z2_4_samples": four,
                 "wall_unprobed_over_probed": plain["wall_s"] / one["wall_s"],
                 "launches_unprobed_over_probed": plain["launches"] / one["launches"]}
    print(json.dumps({name: rec[name]}), flush=True)

# ---------------------------------------------------------------- (c): large lattices, probed only
for L in [int(s) for s in args.sizes.split(",") if s]:
    system = gapped_swave(L, disorder=0.2)
    repeats = args.repeats if L < 512 else args.large_repeats
    system.green_map(energies[:2], distance=d, moments=16)  # warm-up
    entry = {"lattice": f"{L}x{L}", "onsite": "-0.5 + U(-0.2, 0.2), a block of its own on every site", "repeats": repeats}
    for samples in (1, 4):
        result, figures = timed(lambda: system.green_map(energies, distance=d, samples=samples), repeats)
        figures["bytes_leaving_device"] = int(result.blocks.nbytes * (2 if samples > 1 else 1))
        figures["largest_ldos"] = float(result.ldos().max())
        if samples > 1:
            figures["largest_stderr"] = float(np.abs(result.stderr).max())
        entry[f"samples_{samples}"] = figures
        moments, columns = result.info["moments"], result.info["columns"]
        del result
    entry["moments"], entry["columns"] = moments, columns
    # the unprobed call runs under the same width rule (green_unit_width): this record's vectors per launch
    width = min(64, entry["samples_1"]["vectors_per_launch"])
    entry["batches"] = entry["samples_1"]["launches"] // (moments - 1)
    entry["unprobed_batches_not_run"] = -(-L * L // (width // columns))
    entry["unprobed_launches_not_run"] = entry["unprobed_batches_not_run"] * (moments - 1)
    rec[f"c_green_map_{L}x{L}"] = entry
    print(json.dumps({f"c_{L}": entry}), flush=True)

print(json.dumps(rec), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
