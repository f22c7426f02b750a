// green_map.hpp - local Chebyshev moments <e_{4j+a}|T_n(H~)|e_{4j+b}> at many sites j per batch, for the local
// Green's function blocks G_jj (bdg_green_local_moments).  Part of the single translation unit bodge_hip.hip
// (included after green.hpp): the kernels live in namespace bdg beside the picked kernels of green(), the
// driver in the unnamed namespace.
//
// Full-width picked recurrence.  A batch carries the unit start vectors of up to 64 / C sites
// (C = 2 or 4 Nambu columns per site): vector v = C * s + b starts at e_{4 j_s + b}.  Every vector runs the
// recurrence of green.hpp on its own; of t_n only the four entries on the rows of the vector's OWN site are
// moments that anybody wants.  So on the block row of slot s only the C vectors that belong to s store, 64 B
// each: table [n - n0][s][a][b].  One writer per entry, no atomics, no reduction, and the table grows with
// the number of sites, not with its square as the S x 2S product of bdg_green_moments would.
#pragma once

namespace bdg {

// What a launch reads besides a recurrence step's arguments.  table is the slice of this launch's moment:
// double2 (re, im) [n_slots][4][1 << comp_shift].  site_slot holds the position of a block row in the CALL's
// site list (one upload per call); the batch owns the positions slot_base .. slot_base + n_slots - 1.
struct GreenLocalArgs {
    StepArgs s;             // matrix, vector buffers, tiles; partial / discard / col_* are not read
    const int* site_slot;   // [nb] position of the block row in the site list, -1 = not a mapped site
    double2* table;
    int slot_base;
    int n_slots;
    int comp_shift;         // log2 of the columns per site: 1 or 2
};

// The four rows of a mapped site, vectors of lane payload r: stored only by the vectors that start on this
// site (v - (slot << comp_shift) is a column).  PER_LANE as in store_picked: 2 = .x / .y are the real entries of vectors
// 2r, 2r+1, unpacked into (value, 0).
template <int PER_LANE>
__device__ inline void store_local(const GreenLocalArgs& g, int position, int r, const double2 nx[4]) {
    const int slot = position - g.slot_base;  // (position -1: negative as well)
    if (slot < 0 || slot >= g.n_slots) return;
    // (everything below hangs on the slot just loaded: nothing of it can be kept in registers across the tile loop)
    double2* site = g.table + ((slot * 4) << g.comp_shift);
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
        const int b = PER_LANE * r + q - (slot << g.comp_shift);  // column of vector v = PER_LANE * r + q on this site
        if (b >= 0 && b < (1 << g.comp_shift)) {
#pragma unroll
            for (int al = 0; al < 4; ++al) {
                const double2 value = PER_LANE == 2 ? make_double2(q == 0 ? nx[al].x : nx[al].y, 0.0) : nx[al];
                site[(al << g.comp_shift) + b] = value;
            }
        }
    }
}

// The tail of the full-width picked step on the shared tile loops (family.hpp): after the store of t_{n+1}, the
// store of the vectors' own rows.  The site slot is read there and nowhere earlier.
struct GreenLocalTail : FamilyTail {
    using Args = GreenLocalArgs;
    static constexpr const char* kFamily = "picked recurrence";
    template <typename Mode, int RL>
    __device__ static void after(const GreenLocalArgs& ga, NoValue, NoValue, int i, int r, const double2 nx[4]) {
        store_local<Mode::kVec>(ga, ga.site_slot[i], r, nx);
    }
};

// Moment 0 from the start vectors themselves: table[s][al][b] = t_0[al][rows[s]][(s << comp_shift) + b], with
// the vector index counted inside the batch.  One thread per entry.  PER_LANE = 2: real payloads, vector v in
// component v & 1 of payload v >> 1.
template <int PER_LANE>
__global__ void green_local_pick(const double2* __restrict__ vec, int64_t nb, int rl, const int* __restrict__ rows,
                                 int n_slots, int comp_shift, double2* __restrict__ table) {
    const int64_t total = ((int64_t)n_slots * 4) << comp_shift;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(idx & ((1 << comp_shift) - 1));
        const int al = (int)((idx >> comp_shift) & 3);
        const int64_t slot = idx >> (comp_shift + 2);
        const int v = (int)(slot << comp_shift) + b;
        const double2 pair = vec[vslot(al, (size_t)rows[slot], v / PER_LANE, (size_t)nb, rl)];
        table[idx] = PER_LANE == 2 ? make_double2((v & 1) ? pair.y : pair.x, 0.0) : pair;
    }
}

}  // namespace bdg

namespace {

using GreenLocalKernels = FamilyKernels<bdg::GreenLocalTail>;

// bdg_green_local_moments on the range loop of green_driver.hpp.  A batch is `batch_sites` whole sites; the device
// table is [moment of the range][site of the batch][component][column], copied into the caller's table when it is full.
struct GreenLocal : GreenFeature {
    using Args = bdg::GreenLocalArgs;
    static constexpr int32_t bdg_perf::*kFlag = &bdg_perf::green_local;
    bdg_system* sys;
    const GreenSetup<GreenLocalKernels>& gs;
    int batch_sites, n_sites, n_components;
    const int32_t* block_rows;
    const std::vector<int32_t>& position;
    const std::vector<int64_t>& start_rows;
    double2* out;
    double launch_bytes;
    DeviceBuffer<int> d_position, d_sites;
    DeviceBuffer<int64_t> d_rows;
    DeviceBuffer<double2> d_table;
    int s0 = 0, n_slots = 0;  // the batch in flight: its first site, its sites

    int comp_shift() const { return n_components == 2 ? 1 : 2; }
    size_t per_site() const { return (size_t)4 * n_components; }  // double2 entries of one site and moment
    size_t per_moment() const { return (size_t)n_slots * per_site(); }
    int upload(hipStream_t st) {
        const int64_t nb = sys->nb;
        if (int rc = d_position.reserve((size_t)std::max<int64_t>(1, nb))) return rc;
        if (int rc = d_sites.reserve((size_t)n_sites)) return rc;
        if (int rc = d_rows.reserve(start_rows.size())) return rc;
        if (int rc = d_table.reserve((size_t)gs.range * batch_sites * per_site())) return rc;
        HIP_TRY(hipMemcpyAsync(d_position.ptr, position.data(), sizeof(int) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_sites.ptr, block_rows, sizeof(int) * n_sites, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rows.ptr, start_rows.data(), sizeof(int64_t) * start_rows.size(), hipMemcpyHostToDevice, st));
        return BDG_OK;
    }
    int start_batch(int b, double2* cur, double2* prev, Args* ga, hipStream_t st) {
        s0 = b * batch_sites;
        n_slots = std::min(batch_sites, n_sites - s0);
        ga->site_slot = d_position.ptr;
        ga->slot_base = s0;
        ga->n_slots = n_slots;
        ga->comp_shift = comp_shift();
        green_unit_start(sys, gs, cur, prev, d_rows.ptr + (size_t)s0 * n_components, n_slots * n_components, st);
        return n_slots * n_components;
    }
    void moment0(const double2* cur, hipStream_t st) {
        const int grid = (int)std::min<size_t>(1024, (per_moment() + 255) / 256);
        if (gs.mode.real)
            bdg::green_local_pick<2><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, d_sites.ptr + s0, n_slots, comp_shift(), d_table.ptr);
        else
            bdg::green_local_pick<1><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, d_sites.ptr + s0, n_slots, comp_shift(), d_table.ptr);
    }
    void point(Args* ga, int m) { ga->table = d_table.ptr + (size_t)m * per_moment(); }
    int end_range(int n0, int n1, hipStream_t st) {
        // rows (moment) of the batch's n_slots sites into the caller's rows of n_sites sites
        return green_copy_out(out + ((size_t)n0 * n_sites + s0) * per_site(), (size_t)n_sites * per_site(), d_table.ptr,
                              per_moment(), (size_t)(n1 - n0), st);
    }
    void release() {
        d_position.release();
        d_sites.release();
        d_rows.release();
        d_table.release();
    }
};

int run_green_local_moments(bdg_system* sys, double scale, int n_moments, int n_sites, const int32_t* block_rows,
                            int n_components, double* out) {
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    if (!block_rows || !out) return fail(BDG_EINVAL, "null argument");
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_green_local_moments needs a whole (square) matrix: slabs are not supported");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_sites < 1) return fail(BDG_EINVAL, "n_sites must be >= 1");
    if (n_components != 2 && n_components != 4) return fail(BDG_EINVAL, "n_components must be 2 or 4");
    const int64_t nb = sys->nb;
    // position of every block row in the site list; a block row is listed once (one writer per table entry)
    std::vector<int32_t> position((size_t)nb, -1);
    std::vector<int64_t> start_rows((size_t)n_sites * n_components);
    for (int s = 0; s < n_sites; ++s) {
        const int32_t j = block_rows[s];
        if (j < 0 || j >= nb) return fail(BDG_EINVAL, "block row %d out of range", j);
        if (position[(size_t)j] >= 0) return fail(BDG_EINVAL, "block row %d is listed twice", j);
        position[(size_t)j] = s;
        for (int b = 0; b < n_components; ++b) start_rows[(size_t)s * n_components + b] = 4 * (int64_t)j + b;
    }
    lanczos_free(sys);  // (no subspace_free here, unlike run_green_bond_blocks: kept as it was)
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic and storage mode as for a recurrence with unit start vectors; a batch holds whole sites.
    const ModeInfo mode = family_mode(sys);
    const GreenWidth lanes = green_unit_width(sys, mode, n_sites * n_components);
    const int batch_sites = lanes.width / n_components;
    GreenSetup<GreenLocalKernels> gs;
    if (int rc = family_setup(sys, mode, lanes.rl, 0, &gs)) return rc;
    const size_t moment_bytes = (size_t)batch_sites * 4 * n_components * sizeof(double2);  // one moment of a full batch
    green_cut_ranges(n_moments, moment_bytes, &gs);
    GreenLocal feature{{}, sys, gs, batch_sites, n_sites, n_components, block_rows, position, start_rows,
                       reinterpret_cast<double2*>(out), 4.0 * (double)nb + (double)moment_bytes};
    return run_green_ranges(sys, gs, scale, n_moments, (n_sites + batch_sites - 1) / batch_sites, feature);
}

}  // namespace
