// green.hpp - off-diagonal Chebyshev moments <e_{4j+a}|T_n(H~)|e_{4i+b}> for the Green's function blocks G_ji
// (bdg_green_moments).  Part of the single translation unit bodge_hip.hip (included after fermi.hpp): the
// kernels live in namespace bdg beside the Clenshaw kernels, the driver in the unnamed namespace.
//
// Picked recurrence.  A unit start vector e_{4i+b} run through t_{n+1} = 2 H~ t_n - t_{n-1}
// (H~ = H / scale) holds T_n(H~) e_{4i+b}; the four entries of t_n on the rows of a target site j are the
// moments mu_n[ja, ib].  A picked step moves what a recurrence step moves plus one int32 per block row (the
// target slot, -1 on all rows but the targets'), forms no dot product, and on a target row stores the four
// components of every active vector into the moment table.  Every table entry has one writer.
#pragma once

namespace bdg {

// What a picked launch reads besides a recurrence step's arguments.  table is the slice of this launch's
// moment: double2 (re, im) [n_targets][4][n_active]; vectors from n_active on are padding and stay zero.
struct GreenArgs {
    StepArgs s;               // matrix, vector buffers, tiles; partial / discard / col_* are not read
    const int* target_slot;   // [nb] slot of the block row in the table, -1 = not a target
    double2* table;
    int n_active;
};

// The four rows of block row `slot`'s site, vectors of lane payload r.  PER_LANE = 1: nx[al] is the complex
// entry of vector r; 2: .x / .y are the real entries of vectors 2r, 2r+1, unpacked into (value, 0).
template <int PER_LANE>
__device__ inline void store_picked(const GreenArgs& g, int slot, int r, const double2 nx[4]) {
    if (slot < 0) return;
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
        const int v = PER_LANE * r + q;
        if (v < g.n_active) {
#pragma unroll
            for (int al = 0; al < 4; ++al) {
                const double2 value = PER_LANE == 2 ? make_double2(q == 0 ? nx[al].x : nx[al].y, 0.0) : nx[al];
                g.table[((size_t)slot * 4 + al) * g.n_active + v] = value;
            }
        }
    }
}

// The tail of the picked step t_{n+1} = coef * (H t_n) - t_{n-1} on the shared tile loops (family.hpp): the target
// slot of the block row, and after the store of t_{n+1} the store of the target rows into the moment table.
struct GreenTail : FamilyTail {
    using Args = GreenArgs;
    static constexpr const char* kFamily = "picked recurrence";
    template <typename Mode, int RL>
    __device__ static int row(const GreenArgs& ga, NoValue, int i) {
        return ga.target_slot[i];
    }
    template <typename Mode, int RL>
    __device__ static void after(const GreenArgs& ga, NoValue, int target, int, int r, const double2 nx[4]) {
        store_picked<Mode::kVec>(ga, target, r, nx);
    }
};

// Moment 0 from the start vectors themselves: table[slot][al][v] = t_0[al][target_rows[slot]][v].  One thread
// per entry.  PER_LANE = 2: real payloads, vector v in component v & 1 of payload v >> 1.
template <int PER_LANE>
__global__ void green_pick(const double2* __restrict__ vec, int64_t nb, int rl, const int* __restrict__ target_rows,
                           int n_targets, int n_active, double2* __restrict__ table) {
    const int64_t total = (int64_t)n_targets * 4 * n_active;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int v = (int)(idx % n_active);
        const int al = (int)((idx / n_active) & 3);
        const int64_t slot = idx / (4 * (int64_t)n_active);
        const double2 pair = vec[vslot(al, (size_t)target_rows[slot], v / PER_LANE, (size_t)nb, rl)];
        table[idx] = PER_LANE == 2 ? make_double2((v & 1) ? pair.y : pair.x, 0.0) : pair;
    }
}

}  // namespace bdg

namespace {

using GreenKernels = FamilyKernels<bdg::GreenTail>;

// bdg_green_moments on the range loop of green_driver.hpp.  A batch is `width` source rows; the device table is
// [moment of the range][target][component][vector of the batch], copied into the caller's table when it is full.
struct GreenPicked : GreenFeature {
    using Args = bdg::GreenArgs;
    static constexpr int32_t bdg_perf::*kFlag = &bdg_perf::green;
    bdg_system* sys;
    const GreenSetup<GreenKernels>& gs;
    int width, n_sources, n_targets;
    const int64_t* source_rows;
    const int32_t* target_block_rows;
    const std::vector<int32_t>& slot_of;
    double2* out;
    double launch_bytes;
    DeviceBuffer<int> d_slot, d_targets;
    DeviceBuffer<int64_t> d_rows;
    DeviceBuffer<double2> d_table;
    int v0 = 0, n_active = 0;  // the batch in flight: its first source, its sources

    size_t per_moment() const { return (size_t)n_targets * 4 * (size_t)n_active; }
    int upload(hipStream_t st) {
        const int64_t nb = sys->nb;
        if (int rc = d_slot.reserve((size_t)std::max<int64_t>(1, nb))) return rc;
        if (int rc = d_targets.reserve((size_t)n_targets)) return rc;
        if (int rc = d_rows.reserve((size_t)n_sources)) return rc;
        if (int rc = d_table.reserve((size_t)gs.range * n_targets * 4 * (size_t)width)) return rc;
        HIP_TRY(hipMemcpyAsync(d_slot.ptr, slot_of.data(), sizeof(int) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_targets.ptr, target_block_rows, sizeof(int) * n_targets, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rows.ptr, source_rows, sizeof(int64_t) * n_sources, hipMemcpyHostToDevice, st));
        return BDG_OK;
    }
    int start_batch(int b, double2* cur, double2* prev, Args* ga, hipStream_t st) {
        v0 = b * width;
        n_active = std::min(width, n_sources - v0);
        ga->target_slot = d_slot.ptr;
        ga->n_active = n_active;
        green_unit_start(sys, gs, cur, prev, d_rows.ptr + v0, n_active, st);
        return n_active;
    }
    void moment0(const double2* cur, hipStream_t st) {
        const int grid = (int)std::min<size_t>(1024, (per_moment() + 255) / 256);
        if (gs.mode.real)
            bdg::green_pick<2><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, d_targets.ptr, n_targets, n_active, d_table.ptr);
        else
            bdg::green_pick<1><<<grid, 256, 0, st>>>(cur, sys->nb, gs.rl, d_targets.ptr, n_targets, n_active, d_table.ptr);
    }
    void point(Args* ga, int m) { ga->table = d_table.ptr + (size_t)m * per_moment(); }
    int end_range(int n0, int n1, hipStream_t st) {
        // rows (moment, target, component) of n_active entries into the caller's rows of n_sources
        return green_copy_out(out + (size_t)n0 * n_targets * 4 * (size_t)n_sources + v0, (size_t)n_sources, d_table.ptr,
                              (size_t)n_active, (size_t)(n1 - n0) * n_targets * 4, st);
    }
    void release() {
        d_slot.release();
        d_targets.release();
        d_rows.release();
        d_table.release();
    }
};

int run_green_moments(bdg_system* sys, double scale, int n_moments, int n_sources, const int64_t* source_rows,
                      int n_targets, const int32_t* target_block_rows, double* out) {
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    if (!source_rows || !target_block_rows || !out) return fail(BDG_EINVAL, "null argument");
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_green_moments needs a whole (square) matrix: slabs are not supported");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_sources < 1) return fail(BDG_EINVAL, "n_sources must be >= 1");
    if (n_targets < 1) return fail(BDG_EINVAL, "n_targets must be >= 1");
    const int64_t nb = sys->nb;
    for (int v = 0; v < n_sources; ++v)
        if (source_rows[v] < 0 || source_rows[v] >= 4 * nb)
            return fail(BDG_EINVAL, "source row %lld out of range", (long long)source_rows[v]);
    // slot of every block row in the table; a block row is listed once (one writer per table entry)
    std::vector<int32_t> slot_of((size_t)nb, -1);
    for (int t = 0; t < n_targets; ++t) {
        const int32_t j = target_block_rows[t];
        if (j < 0 || j >= nb) return fail(BDG_EINVAL, "target block row %d out of range", j);
        if (slot_of[(size_t)j] >= 0) return fail(BDG_EINVAL, "target block row %d is listed twice", j);
        slot_of[(size_t)j] = t;
    }
    lanczos_free(sys);  // (no subspace_free here, unlike run_green_bond_blocks: kept as it was)
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic and storage mode as for a recurrence with unit start vectors; a batch is `width` source rows.
    const ModeInfo mode = family_mode(sys);
    const GreenWidth lanes = green_unit_width(sys, mode, n_sources);
    GreenSetup<GreenKernels> gs;
    if (int rc = family_setup(sys, mode, lanes.rl, 0, &gs)) return rc;
    const size_t moment_bytes = (size_t)n_targets * 4 * (size_t)lanes.width * sizeof(double2);  // one moment of a full batch
    green_cut_ranges(n_moments, moment_bytes, &gs);
    GreenPicked feature{{}, sys, gs, lanes.width, n_sources, n_targets, source_rows, target_block_rows, slot_of,
                        reinterpret_cast<double2*>(out), 4.0 * (double)nb + (double)moment_bytes};
    return run_green_ranges(sys, gs, scale, n_moments, (n_sources + lanes.width - 1) / lanes.width, feature);
}

}  // namespace
