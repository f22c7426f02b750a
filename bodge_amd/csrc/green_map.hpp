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
    const int comp_shift = n_components == 2 ? 1 : 2;
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
    lanczos_free(sys);
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic and storage mode as for a recurrence with unit start vectors.
    const ModeInfo mode = family_mode(sys);
    const bool real = mode.real;
    const int per_lane = mode.per_lane;
    // Vectors per batch: the widest power of two up to 64 whose vector buffer stays within 96 MB (batch_width's
    // rule for the one-step kernels); set_lanes_per_row fixes the lanes instead.  A batch holds whole sites.
    const double per_vector = (double)nb * 4 * (real ? 8.0 : 16.0);
    int width = 64;
    while (width > 8 && width * per_vector > 96.0 * 1024 * 1024) width >>= 1;
    if (sys->lanes_override >= 4) width = std::min(64, sys->lanes_override * per_lane);
    width = std::min(width, n_sites * n_components);
    int rl = std::max(4, next_pow2((width + per_lane - 1) / per_lane));
    if (sys->lanes_override >= 4 && sys->lanes_override * per_lane >= width) rl = sys->lanes_override;
    const int rv = rl * per_lane;
    const int batch_sites = width / n_components;
    FamilyPlan<GreenLocalKernels::Kernel> gplan;
    if (int rc = make_family_plan<GreenLocalKernels>(sys, rl, mode, 0, &gplan)) return rc;
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
    const int n_batches = (n_sites + batch_sites - 1) / batch_sites;

    // Device table: [moment of the range][site of the batch][component][column]; a range of moments whose
    // entries fit the limit, copied into the caller's table when it is full.
    size_t limit = kGreenTableBytes;
    if (const char* env = knob::raw("BODGE_AMD_GREEN_TABLE_BYTES")) limit = (size_t)std::max(1LL, atoll(env));
    const size_t per_site = (size_t)4 * n_components;                   // double2 entries of one site and moment
    const size_t per_moment_max = (size_t)batch_sites * per_site;
    const int range = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_moments, limit / (per_moment_max * sizeof(double2))));
    const int n_ranges = (n_moments + range - 1) / range;

    if (int rc = sys->vec_a.reserve(vec_count)) return rc;
    if (int rc = sys->vec_b.reserve(vec_count)) return rc;
    DeviceBuffer<int> d_position, d_sites;
    DeviceBuffer<int64_t> d_rows;
    DeviceBuffer<double2> d_table;
    std::vector<hipEvent_t> events;
    auto body = [&]() -> int {
        if (int rc = d_position.reserve((size_t)std::max<int64_t>(1, nb))) return rc;
        if (int rc = d_sites.reserve((size_t)n_sites)) return rc;
        if (int rc = d_rows.reserve(start_rows.size())) return rc;
        if (int rc = d_table.reserve((size_t)range * per_moment_max)) return rc;
        hipStream_t st = sys->stream;
        HIP_TRY(hipMemcpyAsync(d_position.ptr, position.data(), sizeof(int) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_sites.ptr, block_rows, sizeof(int) * n_sites, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rows.ptr, start_rows.data(), sizeof(int64_t) * start_rows.size(), hipMemcpyHostToDevice, st));
        events.assign((size_t)2 * n_batches * n_ranges, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        const int fill_grid = (int)std::min<size_t>(4096, (vec_count + 255) / 256);
        bdg_perf perf{};
        for (int b = 0; b < n_batches; ++b) {
            const int s0 = b * batch_sites;
            const int n_slots = std::min(batch_sites, n_sites - s0);
            const int n_active = n_slots * n_components;
            const size_t per_moment = (size_t)n_slots * per_site;
            bdg::GreenLocalArgs ga{};
            ga.s = base;
            ga.site_slot = d_position.ptr;
            ga.slot_base = s0;
            ga.n_slots = n_slots;
            ga.comp_shift = comp_shift;
            double2* cur = sys->vec_a.ptr;
            double2* prev = sys->vec_b.ptr;
            bdg::fill_zero<<<fill_grid, 256, 0, st>>>(cur, (int64_t)vec_count);
            bdg::fill_zero<<<fill_grid, 256, 0, st>>>(prev, (int64_t)vec_count);
            const int64_t* rows = d_rows.ptr + (size_t)s0 * n_components;
            if (real)
                bdg::set_unit_real<<<1, 64, 0, st>>>(reinterpret_cast<double*>(cur), nb, nb, rv, n_active, rows, (int64_t)0);
            else
                bdg::set_unit<<<1, 64, 0, st>>>(cur, nb, nb, rv, n_active, rows, (int64_t)0);
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
                            bdg::green_local_pick<2><<<grid, 256, 0, st>>>(cur, nb, rl, d_sites.ptr + s0, n_slots, comp_shift, slice);
                        else
                            bdg::green_local_pick<1><<<grid, 256, 0, st>>>(cur, nb, rl, d_sites.ptr + s0, n_slots, comp_shift, slice);
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
                // rows (moment) of the batch's n_slots sites into the caller's rows of n_sites sites
                double2* dst = reinterpret_cast<double2*>(out) + ((size_t)n0 * n_sites + s0) * per_site;
                if (n_slots == n_sites)
                    HIP_TRY(hipMemcpyAsync(dst, d_table.ptr, sizeof(double2) * (size_t)(n1 - n0) * per_moment,
                                           hipMemcpyDeviceToHost, st));
                else
                    HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double2) * (size_t)n_sites * per_site, d_table.ptr,
                                             sizeof(double2) * per_moment, sizeof(double2) * per_moment,
                                             (size_t)(n1 - n0), hipMemcpyDeviceToHost, st));
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
        perf.green_ranges = n_ranges;
        perf.green_local = plan.dictionary ? 2 : 1;
        sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(sys->stream);
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    d_position.release();
    d_sites.release();
    d_rows.release();
    d_table.release();
    return rc;
}

}  // namespace
