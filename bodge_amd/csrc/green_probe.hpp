// green_probe.hpp - the Green's function blocks G_ji(eps) on a pattern of block pairs by probing: one start vector per
// colour of sites and Nambu column instead of one per site and column (bdg_green_probe_blocks).  Part of the single
// translation unit bodge_hip.hip (included after green_bonds.hpp): the two kernels live in namespace bdg beside those
// of green_bonds(), the driver in the unnamed namespace.
//
// The pattern recurrence of green_bonds.hpp with other start vectors.  The caller colours the sites;
// vector v = C * c + b of a batch of whole colours starts at r_{c b} = sum_{i: colour(i) = c} xi_i e_{4i + b} with
// xi_i = +-1 (green_probe_start).  The tail, the pick of moment 0 and the contraction are those of green_bonds.hpp
// unchanged: store_bonds compares entry.x with slot_base + slot, and with entry.x = the colour of the block's column
// site and slot_base = the batch's first colour the vectors of colour c store into every pattern block (j, i) with
// colour(i) = c.  A pattern row holds a colour at most once (checked on the host), so an entry keeps its one writer.
// After the last contraction of a sample, green_probe_accumulate multiplies block (j, i) by xi_i and folds the sample
// into the running mean and sum of squared deviations (Welford), one thread per entry; only the mean and the standard
// error leave the device.
#pragma once

namespace bdg {

// cur = the probe vectors of the colours colour_base .. colour_base + n_slots - 1 (the buffer is zero before): thread
// (block row i, column b) writes xi_i (signs == nullptr: 1) into row 4i + b of vector ((colour[i] - colour_base) <<
// comp_shift) + b.  PER_LANE = 2: real payloads, vector v is component v & 1 of payload v >> 1.
template <int PER_LANE>
__global__ void green_probe_start(double2* __restrict__ vec, int64_t nb, int rl, const int* __restrict__ colour,
                                  const signed char* __restrict__ signs, int colour_base, int n_slots, int comp_shift) {
    const int64_t total = nb << comp_shift;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(idx & ((1 << comp_shift) - 1));
        const int64_t i = idx >> comp_shift;
        const int slot = colour[i] - colour_base;
        if (colour[i] < 0 || slot < 0 || slot >= n_slots) continue;
        const int v = (slot << comp_shift) + b;
        const double xi = signs ? (double)signs[i] : 1.0;
        const size_t at = vslot(b, (size_t)i, v / PER_LANE, (size_t)nb, rl);
        if (PER_LANE == 2)
            reinterpret_cast<double*>(vec)[2 * at + (v & 1)] = xi;
        else
            vec[at] = make_double2(xi, 0.0);
    }
}

// Sample s (1-based) of n_samples into the statistics: entry idx of [e][k][a][b] belongs to pattern block k with
// column site pat_col[k]; x = xi * sample (an exact sign flip), then, Re and Im apart and in this order,
//   delta = x - mean;  mean += delta / s;  m2 = fma(delta, x - mean, m2).
// The first sample starts from zeros without reading them (mean = x bit for bit); the last one leaves the standard
// error sqrt(m2 / (S (S - 1))) in m2.  One writer per entry.  A call of one sample keeps no statistics: mean is the
// sample buffer itself (the sign flip in place) and m2 is nullptr.
__global__ __launch_bounds__(256) void green_probe_accumulate(const double2* sample, int64_t total, int64_t n_pattern,
                                                              const int* __restrict__ pat_col,
                                                              const signed char* __restrict__ signs, int s,
                                                              int n_samples, double2* mean, double2* m2) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = (idx >> 4) % n_pattern;
        const double xi = signs ? (double)signs[pat_col[k]] : 1.0;
        double2 x = sample[idx];
        x.x *= xi;
        x.y *= xi;
        double2 m = make_double2(0.0, 0.0), q = m;
        if (s > 1) {
            m = mean[idx];
            q = m2[idx];
        }
        const double dx = x.x - m.x, dy = x.y - m.y;
        m.x += dx / (double)s;
        m.y += dy / (double)s;
        q.x = fma(dx, x.x - m.x, q.x);
        q.y = fma(dy, x.y - m.y, q.y);
        if (s == n_samples) {
            const double norm = n_samples > 1 ? (double)n_samples * (double)(n_samples - 1) : 1.0;
            q.x = n_samples > 1 ? sqrt(q.x / norm) : 0.0;
            q.y = n_samples > 1 ? sqrt(q.y / norm) : 0.0;
        }
        mean[idx] = m;
        if (m2) m2[idx] = q;
    }
}

}  // namespace bdg

namespace {

// The argument checks of bdg_green_probe_blocks that need the number of block rows and nothing else of the handle
// (bdg_host_probe_check), in the order of the header.
int green_probe_check(int64_t nb, int n_colours, const int32_t* site_colour, int n_samples, const int8_t* signs,
                      const int32_t* pat_indptr, const int32_t* pat_indices, int n_components) {
    if (pat_indptr[0] != 0) return fail(BDG_EINVAL, "pattern indptr must start at 0");
    for (int64_t j = 0; j < nb; ++j)
        if (pat_indptr[j + 1] < pat_indptr[j]) return fail(BDG_EINVAL, "pattern indptr is not monotone");
    if (pat_indptr[nb] < 1) return fail(BDG_EINVAL, "the pattern has no block");
    for (int64_t j = 0; j < nb; ++j)
        for (int64_t k = pat_indptr[j]; k < pat_indptr[j + 1]; ++k) {
            if (pat_indices[k] < 0 || pat_indices[k] >= nb)
                return fail(BDG_EINVAL, "pattern column %d out of range", pat_indices[k]);
            if (k > pat_indptr[j] && pat_indices[k] <= pat_indices[k - 1])
                return fail(BDG_EINVAL, "pattern row %lld is not in canonical order (sorted, no duplicates)", (long long)j);
        }
    if (n_components != 2 && n_components != 4) return fail(BDG_EINVAL, "n_components must be 2 or 4");
    for (int64_t i = 0; i < nb; ++i)
        if (site_colour[i] >= n_colours)
            return fail(BDG_EINVAL, "site %lld has colour %d of %d colours", (long long)i, site_colour[i], n_colours);
    if (signs)
        for (int64_t t = 0; t < (int64_t)n_samples * nb; ++t)
            if (signs[t] != 1 && signs[t] != -1)
                return fail(BDG_EINVAL, "sign %d of site %lld in sample %lld is not +1 or -1", (int)signs[t],
                            (long long)(t % nb), (long long)(t / nb));
    // two column sites of one colour in a row would be two writers of one table entry
    std::vector<int64_t> seen((size_t)n_colours, -1);
    for (int64_t j = 0; j < nb; ++j)
        for (int64_t k = pat_indptr[j]; k < pat_indptr[j + 1]; ++k) {
            const int c = site_colour[pat_indices[k]];
            if (c < 0) continue;
            if (seen[(size_t)c] == j)
                return fail(BDG_EINVAL, "pattern row %lld holds two column sites of colour %d", (long long)j, c);
            seen[(size_t)c] = j;
        }
    return BDG_OK;
}

int green_probe_counts(double scale, int n_moments, int n_weights, const double* weights, int n_colours,
                       const int32_t* site_colour, int n_samples, const int8_t* signs, const int32_t* pat_indptr,
                       const int32_t* pat_indices, const double* mean_out) {
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_weights < 1) return fail(BDG_EINVAL, "n_weights must be >= 1");
    if (n_weights > 65535 * bdg::kBondEnergies)
        return fail(BDG_EINVAL, "n_weights = %d: at most %d weight rows per call", n_weights, 65535 * bdg::kBondEnergies);
    if (n_colours < 1) return fail(BDG_EINVAL, "n_colours must be >= 1");
    if (n_samples < 1) return fail(BDG_EINVAL, "n_samples must be >= 1");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (!weights || !site_colour || !pat_indptr || !pat_indices || !mean_out) return fail(BDG_EINVAL, "null argument");
    if (!signs && n_samples > 1) return fail(BDG_EINVAL, "signs must be given for more than one sample");
    return BDG_OK;
}

// bdg_green_probe_blocks on the range loop of green_driver.hpp: GreenBonds with colours where it has source sites.  A
// batch is `batch_sites` whole colours, and the loop's batches are samples x colour batches: batch B is colour batch
// B % n_colour_batches of sample B / n_colour_batches.  d_out holds one sample; its last contraction is followed by
// the fold into d_mean / d_m2.
struct GreenProbe : GreenBonds {
    static constexpr int32_t bdg_perf::*kFlag = &bdg_perf::green_probe;
    int n_colour_batches, n_samples;
    const int32_t* site_colour;
    const int32_t* pat_indices;
    const int8_t* signs;
    double* stderr_out;
    DeviceBuffer<int> d_colour, d_col;
    DeviceBuffer<signed char> d_signs;
    DeviceBuffer<double2> d_mean, d_m2;
    int sample = 0, colour_batch = 0;

    const signed char* signs_of_sample() const { return signs ? d_signs.ptr + (size_t)sample * (size_t)sys->nb : nullptr; }
    int upload(hipStream_t st) {
        if (int rc = GreenBonds::upload(st)) return rc;
        const size_t nb = (size_t)sys->nb, n_pat = entry.size();
        if (int rc = d_colour.reserve(nb)) return rc;
        if (int rc = d_col.reserve(n_pat)) return rc;
        if (n_samples > 1) {  // (one sample keeps no statistics: d_out is the result)
            if (int rc = d_mean.reserve(out_count())) return rc;
            if (int rc = d_m2.reserve(out_count())) return rc;
        }
        HIP_TRY(hipMemcpyAsync(d_colour.ptr, site_colour, sizeof(int) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_col.ptr, pat_indices, sizeof(int) * n_pat, hipMemcpyHostToDevice, st));
        if (signs) {
            if (int rc = d_signs.reserve((size_t)n_samples * nb)) return rc;
            HIP_TRY(hipMemcpyAsync(d_signs.ptr, signs, (size_t)n_samples * nb, hipMemcpyHostToDevice, st));
        }
        return BDG_OK;
    }
    int start_batch(int b, double2* cur, double2* prev, Args* ga, hipStream_t st) {
        sample = b / n_colour_batches;
        colour_batch = b % n_colour_batches;
        s0 = colour_batch * batch_sites;
        n_slots = std::min(batch_sites, n_sites - s0);
        n_blocks = (int)(batch_ptr[(size_t)colour_batch + 1] - batch_ptr[(size_t)colour_batch]);
        blocks_of_batch = d_batch_blocks.ptr + batch_ptr[(size_t)colour_batch];
        ga->pat_indptr = d_indptr.ptr;
        ga->pat_entry = d_entry.ptr;
        ga->slot_base = s0;
        ga->n_slots = n_slots;
        ga->comp_shift = comp_shift();
        const int fill_grid = (int)std::min<size_t>(4096, (gs.vec_count + 255) / 256);
        bdg::fill_zero<<<fill_grid, 256, 0, st>>>(cur, (int64_t)gs.vec_count);
        bdg::fill_zero<<<fill_grid, 256, 0, st>>>(prev, (int64_t)gs.vec_count);
        const int grid = (int)std::min<size_t>(4096, (((size_t)sys->nb << comp_shift()) + 255) / 256);
        if (gs.mode.real)
            bdg::green_probe_start<2><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, d_colour.ptr, signs_of_sample(), s0, n_slots,
                                                            comp_shift());
        else
            bdg::green_probe_start<1><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, d_colour.ptr, signs_of_sample(), s0, n_slots,
                                                            comp_shift());
        return n_slots * n_components;
    }
    void moment0(const double2* cur, hipStream_t st) {
        if (n_blocks > 0) GreenBonds::moment0(cur, st);
    }
    int end_range(int n0, int n1, hipStream_t st) {
        if (n_blocks > 0) GreenBonds::end_range(n0, n1, st);  // (a batch of colours without a block contracts nothing)
        if (n1 == n_moments && colour_batch == n_colour_batches - 1) {
            const int grid = (int)std::min<size_t>(8192, (out_count() + 255) / 256);
            bdg::green_probe_accumulate<<<grid, 256, 0, st>>>(d_out.ptr, (int64_t)out_count(), (int64_t)entry.size(), d_col.ptr,
                                                              signs_of_sample(), sample + 1, n_samples,
                                                              n_samples > 1 ? d_mean.ptr : d_out.ptr,
                                                              n_samples > 1 ? d_m2.ptr : nullptr);
            if (sample + 1 < n_samples)  // the next sample's sums start from zero (upload zeroed the first one's)
                HIP_TRY(hipMemsetAsync(d_out.ptr, 0, sizeof(double2) * out_count(), st));
        }
        return BDG_OK;
    }
    int finish(hipStream_t st) {
        const double2* mean = n_samples > 1 ? d_mean.ptr : d_out.ptr;
        HIP_TRY(hipMemcpyAsync(out, mean, sizeof(double2) * out_count(), hipMemcpyDeviceToHost, st));
        if (stderr_out && n_samples > 1)
            HIP_TRY(hipMemcpyAsync(stderr_out, d_m2.ptr, sizeof(double2) * out_count(), hipMemcpyDeviceToHost, st));
        else if (stderr_out)
            std::memset(stderr_out, 0, sizeof(double2) * out_count());  // (one sample has no spread)
        return BDG_OK;
    }
    void release() {
        GreenBonds::release();
        d_colour.release();
        d_col.release();
        d_signs.release();
        d_mean.release();
        d_m2.release();
    }
};

int run_green_probe_blocks(bdg_system* sys, double scale, int n_moments, int n_weights, const double* weights,
                           int n_colours, const int32_t* site_colour, int n_samples, const int8_t* signs,
                           const int32_t* pat_indptr, const int32_t* pat_indices, int n_components, double* mean_out,
                           double* stderr_out) {
    // (argument errors first, in the order of the header; none of them needs a GPU)
    if (int rc = green_probe_counts(scale, n_moments, n_weights, weights, n_colours, site_colour, n_samples, signs,
                                    pat_indptr, pat_indices, mean_out))
        return rc;
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    const int64_t nb = sys->nb;
    if (int rc = green_probe_check(nb, n_colours, site_colour, n_samples, signs, pat_indptr, pat_indices, n_components))
        return rc;
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_green_probe_blocks needs a whole (square) matrix: slabs are not supported");
    const int64_t n_pat = pat_indptr[nb];

    // Arithmetic and storage mode as for a recurrence with unit start vectors; a batch holds whole colours.  The
    // pattern's blocks by batch as in run_green_bond_blocks, the colour of the column site in the place of its position
    // in a site list; a block whose column site has no colour belongs to no batch and stays zero.
    const ModeInfo mode = family_mode(sys);
    const GreenWidth lanes = green_unit_width(sys, mode, (int)std::min<int64_t>(64, (int64_t)n_colours * n_components));
    const int batch_colours = lanes.width / n_components;
    const int n_colour_batches = (n_colours + batch_colours - 1) / batch_colours;
    std::vector<int2> entry((size_t)n_pat);
    std::vector<int32_t> block_row((size_t)n_pat), batch_blocks((size_t)n_pat);
    std::vector<int64_t> batch_ptr((size_t)n_colour_batches + 1, 0);
    for (int64_t k = 0; k < n_pat; ++k) {
        const int c = site_colour[pat_indices[k]];
        if (c >= 0) ++batch_ptr[(size_t)(c / batch_colours) + 1];
    }
    for (int b = 0; b < n_colour_batches; ++b) batch_ptr[(size_t)b + 1] += batch_ptr[(size_t)b];
    {
        std::vector<int64_t> filled((size_t)n_colour_batches, 0);
        for (int64_t j = 0; j < nb; ++j)
            for (int64_t k = pat_indptr[j]; k < pat_indptr[j + 1]; ++k) {
                const int c = site_colour[pat_indices[k]];
                block_row[(size_t)k] = (int32_t)j;
                if (c < 0) {
                    entry[(size_t)k] = make_int2(-1, -1);
                    continue;
                }
                const int b = c / batch_colours;
                const int64_t local = filled[(size_t)b]++;
                entry[(size_t)k] = make_int2(c, (int)local);
                batch_blocks[(size_t)(batch_ptr[(size_t)b] + local)] = (int32_t)k;
            }
    }
    int64_t max_blocks = 1;
    for (int b = 0; b < n_colour_batches; ++b)
        max_blocks = std::max(max_blocks, batch_ptr[(size_t)b + 1] - batch_ptr[(size_t)b]);
    // the table and the contraction index a batch's entries (blocks x 16 at most) with int
    if (max_blocks >= ((int64_t)1 << 31) / 16)
        return fail(BDG_EINVAL, "a batch of %lld blocks: at most %lld per batch (32-bit table indices)", (long long)max_blocks,
                    (long long)(((int64_t)1 << 31) / 16 - 1));

    lanczos_free(sys);
    subspace_free(sys);
    HIP_TRY(hipSetDevice(sys->device));
    GreenSetup<GreenBondKernels> gs;
    if (int rc = family_setup(sys, mode, lanes.rl, 0, &gs)) return rc;
    const size_t moment_bytes = (size_t)max_blocks * 4 * n_components * sizeof(double2);  // one moment of the largest batch
    green_cut_ranges(n_moments, moment_bytes, &gs);
    const std::vector<int64_t> no_rows(1, 0);  // (the unit rows of GreenBonds: not used here)
    GreenProbe feature{{{}, sys, gs, batch_colours, n_colours, n_components, n_moments, n_weights, weights, pat_indptr, entry,
                        block_row, batch_blocks, batch_ptr, no_rows, max_blocks, mean_out,
                        4.0 * (double)(nb + 1) + (double)max_blocks * sizeof(int2) + (double)moment_bytes},
                       n_colour_batches, n_samples, site_colour, pat_indices, signs, stderr_out};
    return run_green_ranges(sys, gs, scale, n_moments, n_samples * n_colour_batches, feature);
}

}  // namespace
