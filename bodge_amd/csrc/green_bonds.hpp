// green_bonds.hpp - the Green's function blocks G_ji(eps) on a pattern of block pairs (j, i), every column site i a
// source (bdg_green_bond_blocks).  Part of the single translation unit bodge_hip.hip (included after green_map.hpp):
// the kernels live in namespace bdg beside those of green_map(), the driver in the unnamed namespace.
//
// The full-width picked recurrence of green_map.hpp with a pattern walk for a tail.  A batch carries
// the unit start vectors of up to 64 / C column sites (C = 2 or 4 Nambu columns per site): vector v = C * s + b starts
// at e_{4 i_s + b}.  After the store of t_{n+1} on block row j the lanes walk row j of the call's pattern; for every
// block k = (j, i) whose column site i is the site a lane's vectors started on, those vectors store their four entries
// on the rows of j: table [n - n0][k_local][a][b], 64 B each.  One writer per entry, no atomics.  The table never
// leaves the device: when a range of moments is full, green_bond_contract adds sum_n w[e][n] mu_n[k][a][b] to the
// result G[e][k][a][b] in ascending n, one thread per entry, and only G is copied out.
#pragma once

namespace bdg {

// What a launch reads besides a recurrence step's arguments.  pat_indptr and pat_entry describe the CALL's pattern
// (one upload per call): entry k of block row j is .x = the position of the block's column site in the call's site
// list (-1: none), .y = the block's index in the table of the batch that owns that site.  The batch owns the positions
// slot_base .. slot_base + n_slots - 1; table is the slice of this launch's moment, double2 [blocks][4][1 << comp_shift].
struct GreenBondArgs {
    StepArgs s;             // matrix, vector buffers, tiles; partial / discard / col_* are not read
    const int* pat_indptr;  // [nb + 1]
    const int2* pat_entry;  // [pat_indptr[nb]]
    double2* table;
    int slot_base;
    int n_slots;
    int comp_shift;         // log2 of the columns per site: 1 or 2
};

// Block row i, vectors of lane payload r: the payload's vectors (PER_LANE = 2: .x / .y are the real entries of vectors
// 2r, 2r+1, unpacked into (value, 0)) started on one site, position slot_base + (PER_LANE * r >> comp_shift) of the
// site list; a pattern row holds that site at most once (canonical order), and into that block they store.  The row's
// entries are fetched kBondChunk at a time, all loads of a chunk in flight together: the walk hangs on the end of a
// launch that is a chain of latencies on small lattices (64 x 64, 32 lanes: 7.29 us per launch with one entry per
// round trip, 6.96 with a chunk in flight, 6.43 for the local kernel).  A row without blocks costs the
// two loads of its bounds.
constexpr int kBondChunk = 8;

template <int PER_LANE>
__device__ inline void store_bonds(const GreenBondArgs& g, int i, int r, const double2 nx[4]) {
    const int k0 = g.pat_indptr[i], k1 = g.pat_indptr[i + 1];
    const int slot = (PER_LANE * r) >> g.comp_shift;
    const int position = slot < g.n_slots ? g.slot_base + slot : -2;  // (-2: a padding lane, no site)
    int local = -1;
    for (int c0 = k0; c0 < k1; c0 += kBondChunk) {
        int2 entry[kBondChunk];
#pragma unroll
        for (int u = 0; u < kBondChunk; ++u) entry[u] = g.pat_entry[min(c0 + u, k1 - 1)];
#pragma unroll
        for (int u = 0; u < kBondChunk; ++u)
            if (c0 + u < k1 && entry[u].x == position) local = entry[u].y;
    }
    if (local < 0) return;
    double2* block = g.table + ((local * 4) << g.comp_shift);
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
        const int b = (PER_LANE * r + q) & ((1 << g.comp_shift) - 1);  // column of vector PER_LANE * r + q on its site
#pragma unroll
        for (int al = 0; al < 4; ++al) {
            const double2 value = PER_LANE == 2 ? make_double2(q == 0 ? nx[al].x : nx[al].y, 0.0) : nx[al];
            block[(al << g.comp_shift) + b] = value;
        }
    }
}

// The tail of the pattern step on the shared tile loops (family.hpp): after the store of t_{n+1}, the walk of the
// pattern row.  Everything it needs is read there and nowhere earlier.
struct GreenBondTail : FamilyTail {
    using Args = GreenBondArgs;
    static constexpr const char* kFamily = "pattern recurrence";
    template <typename Mode, int RL>
    __device__ static void after(const GreenBondArgs& ga, NoValue, NoValue, int i, int r, const double2 nx[4]) {
        store_bonds<Mode::kVec>(ga, i, r, nx);
    }
};

// Moment 0 from the start vectors themselves: for the batch's block `local` = pattern block k = batch_blocks[local] on
// block row block_row[k], table[local][al][b] = t_0[al][block_row[k]][(slot << comp_shift) + b] with the slot of the
// block's column site.  One thread per entry.  PER_LANE = 2: real payloads, vector v in component v & 1 of payload v >> 1.
template <int PER_LANE>
__global__ void green_bond_pick(const double2* __restrict__ vec, int64_t nb, int rl, const int* __restrict__ batch_blocks,
                                const int* __restrict__ block_row, const int2* __restrict__ pat_entry, int n_blocks,
                                int slot_base, int comp_shift, double2* __restrict__ table) {
    const int64_t total = ((int64_t)n_blocks * 4) << comp_shift;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(idx & ((1 << comp_shift) - 1));
        const int al = (int)((idx >> comp_shift) & 3);
        const int k = batch_blocks[idx >> (comp_shift + 2)];
        const int v = ((pat_entry[k].x - slot_base) << comp_shift) + b;
        const double2 pair = vec[vslot(al, (size_t)block_row[k], v / PER_LANE, (size_t)nb, rl)];
        table[idx] = PER_LANE == 2 ? make_double2((v & 1) ? pair.y : pair.x, 0.0) : pair;
    }
}

// Moments to energies.  table holds the moments n0 .. n1 - 1 of a batch's blocks, [n - n0][entries] with
// entries = blocks x 4 x C; thread (x, energy tile y) owns entry x for kBondEnergies weight rows and continues their
// sums where the range before left them: acc <- acc + w[e][n] mu_n in ascending n, one chain of FMAs per output, so
// the bits do not depend on how the moments are cut into ranges.  C = 2: the entry (a, b) also feeds the hole column
// entry (a ^ 2, b ^ 2) of the same block with (-1)^n conj(mu_n[a][b]) (the rule of green.hole_columns).  The result
// has four columns: out[e][k][a][b], k = batch_blocks[entry's block].  Every output entry has one writer.
constexpr int kBondEnergies = 4;

template <int C>
__global__ __launch_bounds__(256) void green_bond_contract(const double2* __restrict__ table, int n0, int n1,
                                                           int entries, const double2* __restrict__ weights,
                                                           int n_moments, int n_weights,
                                                           const int* __restrict__ batch_blocks, int64_t n_pattern,
                                                           double2* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= entries) return;
    const int e0 = blockIdx.y * kBondEnergies;
    const int b = x % C, al = (x / C) & 3;
    const int64_t k = batch_blocks[x / (4 * C)];
    double2 acc[kBondEnergies], hole[kBondEnergies];
    size_t at[kBondEnergies];
#pragma unroll
    for (int u = 0; u < kBondEnergies; ++u) {
        const int e = min(e0 + u, n_weights - 1);  // (rows past the end repeat the last one and are not stored)
        at[u] = (((size_t)e * (size_t)n_pattern + (size_t)k) * 4) * 4;
        acc[u] = out[at[u] + al * 4 + b];
        if constexpr (C == 2) hole[u] = out[at[u] + (al ^ 2) * 4 + (b ^ 2)];
    }
    for (int n = n0; n < n1; ++n) {
        const double2 mu = table[(size_t)(n - n0) * entries + x];
        const double sign = (n & 1) ? -1.0 : 1.0;
#pragma unroll
        for (int u = 0; u < kBondEnergies; ++u) {
            const double2 w = weights[(size_t)min(e0 + u, n_weights - 1) * n_moments + n];
            acc[u].x = fma(w.x, mu.x, acc[u].x);
            acc[u].x = fma(-w.y, mu.y, acc[u].x);
            acc[u].y = fma(w.x, mu.y, acc[u].y);
            acc[u].y = fma(w.y, mu.x, acc[u].y);
            if constexpr (C == 2) {
                const double hx = sign * mu.x, hy = -sign * mu.y;  // (-1)^n conj(mu)
                hole[u].x = fma(w.x, hx, hole[u].x);
                hole[u].x = fma(-w.y, hy, hole[u].x);
                hole[u].y = fma(w.x, hy, hole[u].y);
                hole[u].y = fma(w.y, hx, hole[u].y);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kBondEnergies; ++u) {
        if (e0 + u >= n_weights) continue;
        out[at[u] + al * 4 + b] = acc[u];
        if constexpr (C == 2) out[at[u] + (al ^ 2) * 4 + (b ^ 2)] = hole[u];
    }
}

}  // namespace bdg

namespace {

using GreenBondKernels = FamilyKernels<bdg::GreenBondTail>;

// bdg_green_bond_blocks on the range loop of green_driver.hpp.  A batch is `batch_sites` whole column sites; the device
// table is [moment of the range][block of the batch][component][column], contracted into the result on the device
// when it is full.  The third event of a range closes its contraction: window_ms - kernel_ms is the contractions' time.
struct GreenBonds : GreenFeature {
    using Args = bdg::GreenBondArgs;
    static constexpr int32_t bdg_perf::*kFlag = &bdg_perf::green_bonds;
    static constexpr int kEvents = 3;
    bdg_system* sys;
    const GreenSetup<GreenBondKernels>& gs;
    int batch_sites, n_sites, n_components, n_moments, n_weights;
    const double* weights;
    const int32_t* pat_indptr;
    const std::vector<int2>& entry;
    const std::vector<int32_t>& block_row;
    const std::vector<int32_t>& batch_blocks;
    const std::vector<int64_t>& batch_ptr;
    const std::vector<int64_t>& start_rows;
    int64_t max_blocks;
    double* out;
    double launch_bytes;
    DeviceBuffer<int> d_indptr, d_block_row, d_batch_blocks;
    DeviceBuffer<int2> d_entry;
    DeviceBuffer<int64_t> d_rows;
    DeviceBuffer<double2> d_table, d_weights, d_out;
    int s0 = 0, n_slots = 0, n_blocks = 0;  // the batch in flight: its first site, its sites, its blocks
    const int* blocks_of_batch = nullptr;

    int comp_shift() const { return n_components == 2 ? 1 : 2; }
    size_t per_block() const { return (size_t)4 * n_components; }  // double2 entries of one block and moment
    size_t per_moment() const { return (size_t)n_blocks * per_block(); }
    size_t out_count() const { return (size_t)n_weights * entry.size() * 16; }
    int upload(hipStream_t st) {
        const size_t nb = (size_t)sys->nb, n_pat = entry.size();
        if (int rc = d_indptr.reserve(nb + 1)) return rc;
        if (int rc = d_block_row.reserve(n_pat)) return rc;
        if (int rc = d_batch_blocks.reserve(n_pat)) return rc;
        if (int rc = d_entry.reserve(n_pat)) return rc;
        if (int rc = d_rows.reserve(start_rows.size())) return rc;
        if (int rc = d_table.reserve((size_t)gs.range * max_blocks * per_block())) return rc;
        if (int rc = d_weights.reserve((size_t)n_weights * n_moments)) return rc;
        if (int rc = d_out.reserve(out_count())) return rc;
        HIP_TRY(hipMemcpyAsync(d_indptr.ptr, pat_indptr, sizeof(int) * (nb + 1), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_block_row.ptr, block_row.data(), sizeof(int) * n_pat, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_batch_blocks.ptr, batch_blocks.data(), sizeof(int) * n_pat, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_entry.ptr, entry.data(), sizeof(int2) * n_pat, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rows.ptr, start_rows.data(), sizeof(int64_t) * start_rows.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_weights.ptr, weights, sizeof(double2) * (size_t)n_weights * n_moments, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_out.ptr, 0, sizeof(double2) * out_count(), st));
        return BDG_OK;
    }
    int start_batch(int b, double2* cur, double2* prev, Args* ga, hipStream_t st) {
        s0 = b * batch_sites;
        n_slots = std::min(batch_sites, n_sites - s0);
        n_blocks = (int)(batch_ptr[(size_t)b + 1] - batch_ptr[(size_t)b]);
        blocks_of_batch = d_batch_blocks.ptr + batch_ptr[(size_t)b];
        ga->pat_indptr = d_indptr.ptr;
        ga->pat_entry = d_entry.ptr;
        ga->slot_base = s0;
        ga->n_slots = n_slots;
        ga->comp_shift = comp_shift();
        green_unit_start(sys, gs, cur, prev, d_rows.ptr + (size_t)s0 * n_components, n_slots * n_components, st);
        return n_slots * n_components;
    }
    void moment0(const double2* cur, hipStream_t st) {
        const int grid = (int)std::min<size_t>(1024, (per_moment() + 255) / 256);
        if (gs.mode.real)
            bdg::green_bond_pick<2><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, blocks_of_batch, d_block_row.ptr, d_entry.ptr,
                                                          n_blocks, s0, comp_shift(), d_table.ptr);
        else
            bdg::green_bond_pick<1><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, blocks_of_batch, d_block_row.ptr, d_entry.ptr,
                                                          n_blocks, s0, comp_shift(), d_table.ptr);
    }
    void point(Args* ga, int m) { ga->table = d_table.ptr + (size_t)m * per_moment(); }
    int end_range(int n0, int n1, hipStream_t st) {
        // the range's moments into the result: the sums go on where the range before left them
        const dim3 grid((unsigned)((per_moment() + 255) / 256), (unsigned)((n_weights + bdg::kBondEnergies - 1) / bdg::kBondEnergies));
        if (n_components == 2)
            bdg::green_bond_contract<2><<<grid, 256, 0, st>>>(d_table.ptr, n0, n1, (int)per_moment(), d_weights.ptr, n_moments,
                                                             n_weights, blocks_of_batch, (int64_t)entry.size(), d_out.ptr);
        else
            bdg::green_bond_contract<4><<<grid, 256, 0, st>>>(d_table.ptr, n0, n1, (int)per_moment(), d_weights.ptr, n_moments,
                                                             n_weights, blocks_of_batch, (int64_t)entry.size(), d_out.ptr);
        return BDG_OK;
    }
    int finish(hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(out, d_out.ptr, sizeof(double2) * out_count(), hipMemcpyDeviceToHost, st));
        return BDG_OK;
    }
    void release() {
        d_indptr.release();
        d_block_row.release();
        d_batch_blocks.release();
        d_entry.release();
        d_rows.release();
        d_table.release();
        d_weights.release();
        d_out.release();
    }
};

int run_green_bond_blocks(bdg_system* sys, double scale, int n_moments, int n_weights, const double* weights,
                          const int32_t* pat_indptr, const int32_t* pat_indices, int n_components, double* out) {
    // (argument errors first, in the order of the header; none of them needs a GPU)
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_weights < 1) return fail(BDG_EINVAL, "n_weights must be >= 1");
    if (n_weights > 65535 * bdg::kBondEnergies)  // (the contraction's grid: one y block per kBondEnergies weight rows)
        return fail(BDG_EINVAL, "n_weights = %d: at most %d weight rows per call", n_weights, 65535 * bdg::kBondEnergies);
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (!weights || !pat_indptr || !pat_indices || !out) return fail(BDG_EINVAL, "null argument");
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    const int64_t nb = sys->nb;
    if (pat_indptr[0] != 0) return fail(BDG_EINVAL, "pattern indptr must start at 0");
    for (int64_t j = 0; j < nb; ++j)
        if (pat_indptr[j + 1] < pat_indptr[j]) return fail(BDG_EINVAL, "pattern indptr is not monotone");
    const int64_t n_pat = pat_indptr[nb];
    if (n_pat < 1) return fail(BDG_EINVAL, "the pattern has no block");
    for (int64_t j = 0; j < nb; ++j)
        for (int64_t k = pat_indptr[j]; k < pat_indptr[j + 1]; ++k) {
            if (pat_indices[k] < 0 || pat_indices[k] >= nb)
                return fail(BDG_EINVAL, "pattern column %d out of range", pat_indices[k]);
            if (k > pat_indptr[j] && pat_indices[k] <= pat_indices[k - 1])
                return fail(BDG_EINVAL, "pattern row %lld is not in canonical order (sorted, no duplicates)", (long long)j);
        }
    if (n_components != 2 && n_components != 4) return fail(BDG_EINVAL, "n_components must be 2 or 4");
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_green_bond_blocks needs a whole (square) matrix: slabs are not supported");
    lanczos_free(sys);
    subspace_free(sys);  // (this driver alone of the four ends a subspace block as well: kept as it was)
    HIP_TRY(hipSetDevice(sys->device));

    // The column sites of the call: the distinct columns of the pattern, ascending.
    std::vector<int32_t> position((size_t)nb, -1);
    for (int64_t k = 0; k < n_pat; ++k) position[(size_t)pat_indices[k]] = 0;
    std::vector<int32_t> sites;
    for (int64_t i = 0; i < nb; ++i)
        if (position[(size_t)i] == 0) {
            position[(size_t)i] = (int32_t)sites.size();
            sites.push_back((int32_t)i);
        }
    const int n_sites = (int)sites.size();
    std::vector<int64_t> start_rows((size_t)n_sites * n_components);
    for (int s = 0; s < n_sites; ++s)
        for (int b = 0; b < n_components; ++b) start_rows[(size_t)s * n_components + b] = 4 * (int64_t)sites[(size_t)s] + b;

    // Arithmetic and storage mode as for a recurrence with unit start vectors; a batch holds whole sites.
    const ModeInfo mode = family_mode(sys);
    const GreenWidth lanes = green_unit_width(sys, mode, n_sites * n_components);
    const int batch_sites = lanes.width / n_components;
    const int n_batches = (n_sites + batch_sites - 1) / batch_sites;
    GreenSetup<GreenBondKernels> gs;
    if (int rc = family_setup(sys, mode, lanes.rl, 0, &gs)) return rc;

    // The pattern's blocks by batch: a block belongs to the batch of its column site and has an index in that batch's
    // table; batch_blocks lists the blocks of batch b (pattern order) from batch_ptr[b] on.
    std::vector<int2> entry((size_t)n_pat);
    std::vector<int32_t> block_row((size_t)n_pat), batch_blocks((size_t)n_pat);
    std::vector<int64_t> batch_ptr((size_t)n_batches + 1, 0);
    for (int64_t k = 0; k < n_pat; ++k) ++batch_ptr[(size_t)(position[(size_t)pat_indices[k]] / batch_sites) + 1];
    for (int b = 0; b < n_batches; ++b) batch_ptr[(size_t)b + 1] += batch_ptr[(size_t)b];
    {
        std::vector<int64_t> filled((size_t)n_batches, 0);
        for (int64_t j = 0; j < nb; ++j)
            for (int64_t k = pat_indptr[j]; k < pat_indptr[j + 1]; ++k) {
                const int pos = position[(size_t)pat_indices[k]];
                const int b = pos / batch_sites;
                const int64_t local = filled[(size_t)b]++;
                entry[(size_t)k] = make_int2(pos, (int)local);
                block_row[(size_t)k] = (int32_t)j;
                batch_blocks[(size_t)(batch_ptr[(size_t)b] + local)] = (int32_t)k;
            }
    }
    int64_t max_blocks = 0;
    for (int b = 0; b < n_batches; ++b) max_blocks = std::max(max_blocks, batch_ptr[(size_t)b + 1] - batch_ptr[(size_t)b]);

    const size_t moment_bytes = (size_t)max_blocks * 4 * n_components * sizeof(double2);  // one moment of the largest batch
    green_cut_ranges(n_moments, moment_bytes, &gs);
    GreenBonds feature{{}, sys, gs, batch_sites, n_sites, n_components, n_moments, n_weights, weights, pat_indptr, entry,
                       block_row, batch_blocks, batch_ptr, start_rows, max_blocks, out,
                       4.0 * (double)(nb + 1) + (double)max_blocks * sizeof(int2) + (double)moment_bytes};
    return run_green_ranges(sys, gs, scale, n_moments, n_batches, feature);
}

}  // namespace
