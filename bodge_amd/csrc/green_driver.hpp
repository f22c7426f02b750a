// green_driver.hpp - the host side that the four Green moment-table drivers share: bdg_green_moments (green.hpp),
// bdg_green_local_moments (green_map.hpp), bdg_green_bond_blocks (green_bonds.hpp) and bdg_green_state_moments
// (green_states.hpp).  Part of the single translation unit bodge_hip.hip (included before green.hpp); everything
// lives in its unnamed namespace.
//
// All four walk batches of start vectors x ranges of moments x moments on the handle's stream: a
// batch's vectors run t_{n+1} = 2 H~ t_n - t_{n-1}, every launch leaves its moment in a slice of a device table, and
// when a range of moments is full the feature hands the table on.  GreenSetup is what such a call decides before its
// first launch (the family's set-up of family.hpp plus the ranges), run_green_ranges the loop; a driver keeps its argument checks, its host-side index tables and a
// feature type whose hooks the loop calls (resolved at compile time: a launch of a small lattice is 6 - 7 us, and host
// time per launch shows).
#pragma once

namespace {

constexpr size_t kGreenTableBytes = (size_t)256 << 20;  // device moment table: a range of moments at a time

// Vectors per batch and lanes per row of a call with unit start vectors: the unit rule of family.hpp, at most the
// `n_vectors` the call has.
struct GreenWidth {
    int width, rl;
};
GreenWidth green_unit_width(const bdg_system* sys, const ModeInfo& mode, int n_vectors) {
    const int width = std::min(family_unit_width(sys, mode), n_vectors);
    return {width, family_unit_lanes(sys, mode, width)};
}

// What a call has decided before its first launch: the family's set-up (family_setup fills it) and the ranges, which
// need the bytes of one moment's table - and those follow from the lanes and, for the partials of green_states.hpp,
// from the grid: green_cut_ranges.
template <typename Kernels>
struct GreenSetup : FamilySetup<Kernels> {
    int range = 0, n_ranges = 0;  // moments per fill of the device table, fills per batch
};

// A range of moments whose tables (`moment_bytes` each, the widest batch's) fit BODGE_AMD_GREEN_TABLE_BYTES.
template <typename Kernels>
void green_cut_ranges(int n_moments, size_t moment_bytes, GreenSetup<Kernels>* gs) {
    size_t limit = kGreenTableBytes;
    if (const char* env = knob::raw("BODGE_AMD_GREEN_TABLE_BYTES")) limit = (size_t)std::max(1LL, atoll(env));
    gs->range = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_moments, limit / moment_bytes));
    gs->n_ranges = (n_moments + gs->range - 1) / gs->range;
}

// Start of a batch of unit vectors: cur = e_{rows[v]} in vector v < n_active, zero elsewhere; prev = 0.
template <typename Kernels>
void green_unit_start(const bdg_system* sys, const GreenSetup<Kernels>& gs, double2* cur, double2* prev,
                      const int64_t* rows, int n_active, hipStream_t st) {
    const int fill_grid = (int)std::min<size_t>(4096, (gs.vec_count + 255) / 256);
    bdg::fill_zero<<<fill_grid, 256, 0, st>>>(cur, (int64_t)gs.vec_count);
    bdg::fill_zero<<<fill_grid, 256, 0, st>>>(prev, (int64_t)gs.vec_count);
    if (gs.mode.real)
        bdg::set_unit_real<<<1, 64, 0, st>>>(reinterpret_cast<double*>(cur), sys->nb, sys->nb, gs.rv, n_active, rows, (int64_t)0);
    else
        bdg::set_unit<<<1, 64, 0, st>>>(cur, sys->nb, sys->nb, gs.rv, n_active, rows, (int64_t)0);
}

// A full range leaves the device: `rows` rows of `row` entries of the table into the caller's rows of `pitch` entries
// from dst on - one plain copy where the batch fills the caller's rows.
int green_copy_out(double2* dst, size_t pitch, const double2* table, size_t row, size_t rows, hipStream_t st) {
    if (row == pitch)
        HIP_TRY(hipMemcpyAsync(dst, table, sizeof(double2) * rows * row, hipMemcpyDeviceToHost, st));
    else
        HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double2) * pitch, table, sizeof(double2) * row, sizeof(double2) * row, rows,
                                 hipMemcpyDeviceToHost, st));
    return BDG_OK;
}

// What a feature need not say.  A feature type has
//   Args, kFlag            the kernel's argument struct; the bdg_perf flag of the call (1 streamed-block, 2 dictionary)
//   launch_bytes           what a launch moves besides algorithmic_bytes (bdg_perf::bytes_per_launch)
//   upload(st)             reserve its device buffers, upload its tables
//   start_batch(b, cur, prev, &args, st)   the start vectors into cur, zero into prev, the batch's fields into args;
//                          returns the vectors of the batch
//   moment0(cur, st)       mu_0 from t_0 itself, into the first slice
//   point(&args, m)        the slice of the range's m-th moment into args
//   close_range(n0, n1, st)   launches that belong to the range's kernel time
//   end_range(n0, n1, st)  the full table handed on, after the closing event
//   finish(st)             after the last batch, before the stream is awaited
//   release()              its device buffers given back; called once, on every way out
// and, with kEvents = 3, a third event per range after end_range: the timing window then ends there.
struct GreenFeature {
    static constexpr int kEvents = 2;
    void close_range(int, int, hipStream_t) {}
    int finish(hipStream_t) { return BDG_OK; }
};

template <typename Kernels, typename Feature>
int run_green_ranges(bdg_system* sys, const GreenSetup<Kernels>& gs, double scale, int n_moments, int n_batches, Feature& f) {
    if (int rc = sys->vec_a.reserve(gs.vec_count)) return rc;
    if (int rc = sys->vec_b.reserve(gs.vec_count)) return rc;
    const StepPlan& plan = gs.plan.step;
    std::vector<hipEvent_t> events;
    auto body = [&]() -> int {
        hipStream_t st = sys->stream;
        if (int rc = f.upload(st)) return rc;
        events.assign((size_t)Feature::kEvents * n_batches * gs.n_ranges, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        bdg_perf perf{};
        for (int b = 0; b < n_batches; ++b) {
            typename Feature::Args ga{};
            ga.s = gs.base;
            double2* cur = sys->vec_a.ptr;
            double2* prev = sys->vec_b.ptr;
            const int n_active = f.start_batch(b, cur, prev, &ga, st);
            for (int g = 0; g < gs.n_ranges; ++g) {
                const int n0 = g * gs.range, n1 = std::min(n_moments, n0 + gs.range);
                const size_t ev = (size_t)Feature::kEvents * (b * gs.n_ranges + g);
                HIP_TRY(hipEventRecord(events[ev], st));
                for (int n = n0; n < n1; ++n) {
                    if (n == 0) {
                        f.moment0(cur, st);
                        continue;
                    }
                    // t_1 = H~ t_0 (t_{-1} = 0), then t_{n+1} = 2 H~ t_n - t_{n-1}: the new vector replaces prev
                    ga.s.cur = cur;
                    ga.s.prev = prev;
                    ga.s.coef = (n == 1 ? 1.0 : 2.0) / scale;
                    ga.s.reverse = gs.alternate ? (n & 1) : 0;
                    f.point(&ga, n - n0);
                    gs.plan.kernel<<<plan.grid, bdg::kBlockThreads, plan.lds_bytes, st>>>(ga);
                    std::swap(cur, prev);
                }
                f.close_range(n0, n1, st);
                HIP_TRY(hipEventRecord(events[ev + 1], st));
                HIP_TRY(hipGetLastError());
                if (int rc = f.end_range(n0, n1, st)) return rc;
                if constexpr (Feature::kEvents == 3) {
                    HIP_TRY(hipEventRecord(events[ev + 2], st));
                    HIP_TRY(hipGetLastError());
                }
            }
            perf.vector_steps += (int64_t)(n_moments - 1) * n_active;
        }
        if (int rc = f.finish(st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        // kernel time: first to second event of every range; the window: first event to the last one of all
        for (size_t e = 0; e < events.size(); e += Feature::kEvents) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, events[e], events[e + 1]));
            perf.kernel_ms += t;
        }
        float window = 0.f;
        HIP_TRY(hipEventElapsedTime(&window, events.front(), events.back()));
        perf.window_ms = window;
        perf.launches = (int64_t)n_batches * (n_moments - 1);
        perf.bytes_per_launch = algorithmic_bytes(sys, gs.rv, gs.mode, plan.dictionary) + f.launch_bytes;
        perf.bytes_moved = perf.bytes_per_launch * (double)perf.launches;
        family_perf(sys, plan, gs.rv, gs.strip_rows, 1, &perf);
        perf.green_ranges = gs.n_ranges;
        perf.*Feature::kFlag = plan.dictionary ? 2 : 1;
        sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(sys->stream);
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    f.release();
    return rc;
}

}  // namespace
