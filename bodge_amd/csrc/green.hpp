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

constexpr size_t kGreenTableBytes = (size_t)256 << 20;  // device moment table: a range of moments at a time

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
    lanczos_free(sys);
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic and storage mode as for a recurrence with unit start vectors.
    const ModeInfo mode = family_mode(sys);
    const bool real = mode.real;
    const int per_lane = mode.per_lane;
    // Source rows per batch: the widest power of two up to 64 whose vector buffer stays within 96 MB
    // (batch_width's rule for the one-step kernels); set_lanes_per_row fixes the lanes instead.
    const double per_vector = (double)nb * 4 * (real ? 8.0 : 16.0);
    int width = 64;
    while (width > 8 && width * per_vector > 96.0 * 1024 * 1024) width >>= 1;
    if (sys->lanes_override >= 4) width = std::min(64, sys->lanes_override * per_lane);
    width = std::min(width, n_sources);
    int rl = std::max(4, next_pow2((width + per_lane - 1) / per_lane));
    if (sys->lanes_override >= 4 && sys->lanes_override * per_lane >= width) rl = sys->lanes_override;
    const int rv = rl * per_lane;
    FamilyPlan<GreenKernels::Kernel> gplan;
    if (int rc = make_family_plan<GreenKernels>(sys, rl, mode, 0, &gplan)) return rc;
    const StepPlan& plan = gplan.step;
    bdg::StepArgs base{};
    if (int rc = matrix_args(sys, plan, &base)) return rc;
    int strip_rows = 0;
    if (int rc = prepare_tile_order(sys, plan.rows_per_tile, plan.n_tiles, (real ? 32.0 : 64.0) * rv, &base.tile_order,
                                    &strip_rows))
        return rc;
    const size_t vec_count = (size_t)4 * nb * rl;
    const VectorHints hints = family_vector_hints(vec_count);
    base.stream_vectors = hints.stream_vectors;
    const bool alternate = hints.alternate;
    const int n_batches = (n_sources + width - 1) / width;

    // Device table: [moment of the range][target][component][vector of the batch]; a range of moments whose
    // entries fit the limit, copied into the caller's table when it is full.
    size_t limit = kGreenTableBytes;
    if (const char* env = knob::raw("BODGE_AMD_GREEN_TABLE_BYTES")) limit = (size_t)std::max(1LL, atoll(env));
    const size_t per_moment_max = (size_t)n_targets * 4 * (size_t)width;  // double2 entries of one moment
    const int range = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_moments, limit / (per_moment_max * sizeof(double2))));
    const int n_ranges = (n_moments + range - 1) / range;

    if (int rc = sys->vec_a.reserve(vec_count)) return rc;
    if (int rc = sys->vec_b.reserve(vec_count)) return rc;
    DeviceBuffer<int> d_slot, d_targets;
    DeviceBuffer<int64_t> d_rows;
    DeviceBuffer<double2> d_table;
    std::vector<hipEvent_t> events;
    auto body = [&]() -> int {
        if (int rc = d_slot.reserve((size_t)std::max<int64_t>(1, nb))) return rc;
        if (int rc = d_targets.reserve((size_t)n_targets)) return rc;
        if (int rc = d_rows.reserve((size_t)n_sources)) return rc;
        if (int rc = d_table.reserve((size_t)range * per_moment_max)) return rc;
        hipStream_t st = sys->stream;
        HIP_TRY(hipMemcpyAsync(d_slot.ptr, slot_of.data(), sizeof(int) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_targets.ptr, target_block_rows, sizeof(int) * n_targets, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rows.ptr, source_rows, sizeof(int64_t) * n_sources, hipMemcpyHostToDevice, st));
        events.assign((size_t)2 * n_batches * n_ranges, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        const int fill_grid = (int)std::min<size_t>(4096, (vec_count + 255) / 256);
        bdg_perf perf{};
        for (int b = 0; b < n_batches; ++b) {
            const int v0 = b * width;
            const int n_active = std::min(width, n_sources - v0);
            const size_t per_moment = (size_t)n_targets * 4 * (size_t)n_active;
            bdg::GreenArgs ga{};
            ga.s = base;
            ga.target_slot = d_slot.ptr;
            ga.n_active = n_active;
            double2* cur = sys->vec_a.ptr;
            double2* prev = sys->vec_b.ptr;
            bdg::fill_zero<<<fill_grid, 256, 0, st>>>(cur, (int64_t)vec_count);
            bdg::fill_zero<<<fill_grid, 256, 0, st>>>(prev, (int64_t)vec_count);
            if (real)
                bdg::set_unit_real<<<1, 64, 0, st>>>(reinterpret_cast<double*>(cur), nb, nb, rv, n_active,
                                                     d_rows.ptr + v0, (int64_t)0);
            else
                bdg::set_unit<<<1, 64, 0, st>>>(cur, nb, nb, rv, n_active, d_rows.ptr + v0, (int64_t)0);
            for (int g = 0; g < n_ranges; ++g) {
                const int n0 = g * range, n1 = std::min(n_moments, n0 + range);
                const size_t ev = (size_t)2 * (b * n_ranges + g);
                HIP_TRY(hipEventRecord(events[ev], st));
                for (int n = n0; n < n1; ++n) {
                    double2* slice = d_table.ptr + (size_t)(n - n0) * per_moment;
                    if (n == 0) {
                        // mu_0 from t_0 itself
                        const int grid = (int)std::min<size_t>(1024, (per_moment + 255) / 256);
                        if (real)
                            bdg::green_pick<2><<<grid, 256, 0, st>>>(cur, nb, rl, d_targets.ptr, n_targets, n_active, slice);
                        else
                            bdg::green_pick<1><<<grid, 256, 0, st>>>(cur, nb, rl, d_targets.ptr, n_targets, n_active, slice);
                        continue;
                    }
                    // t_1 = H~ t_0 (t_{-1} = 0), then t_{n+1} = 2 H~ t_n - t_{n-1}: the new vector replaces prev
                    ga.s.cur = cur;
                    ga.s.prev = prev;
                    ga.s.coef = (n == 1 ? 1.0 : 2.0) / scale;
                    ga.s.reverse = alternate ? (n & 1) : 0;
                    ga.table = slice;
                    gplan.kernel<<<plan.grid, bdg::kBlockThreads, plan.lds_bytes, st>>>(ga);
                    std::swap(cur, prev);
                }
                HIP_TRY(hipEventRecord(events[ev + 1], st));
                HIP_TRY(hipGetLastError());
                // rows (moment, target, component) of n_active entries into the caller's rows of n_sources
                double2* dst = reinterpret_cast<double2*>(out) + (size_t)n0 * n_targets * 4 * (size_t)n_sources + v0;
                if (n_active == n_sources)
                    HIP_TRY(hipMemcpyAsync(dst, d_table.ptr, sizeof(double2) * (size_t)(n1 - n0) * per_moment,
                                           hipMemcpyDeviceToHost, st));
                else
                    HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double2) * (size_t)n_sources, d_table.ptr,
                                             sizeof(double2) * (size_t)n_active, sizeof(double2) * (size_t)n_active,
                                             (size_t)(n1 - n0) * n_targets * 4, hipMemcpyDeviceToHost, st));
            }
            perf.vector_steps += (int64_t)(n_moments - 1) * n_active;
        }
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t e = 0; e < events.size(); e += 2) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, events[e], events[e + 1]));
            perf.kernel_ms += t;
        }
        float window = 0.f;
        HIP_TRY(hipEventElapsedTime(&window, events.front(), events.back()));
        perf.window_ms = window;
        perf.launches = (int64_t)n_batches * (n_moments - 1);
        perf.bytes_per_launch = algorithmic_bytes(sys, rv, mode, plan.dictionary) + 4.0 * (double)nb +
                                (double)(per_moment_max * sizeof(double2));
        perf.bytes_moved = perf.bytes_per_launch * (double)perf.launches;
        family_perf(sys, plan, rv, strip_rows, 1, &perf);
        perf.green = plan.dictionary ? 2 : 1;
        perf.green_ranges = n_ranges;
        sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(sys->stream);
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    d_slot.release();
    d_targets.release();
    d_rows.release();
    d_table.release();
    return rc;
}

}  // namespace
