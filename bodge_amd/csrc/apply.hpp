// apply.hpp - a Chebyshev series of H on caller-supplied vectors, y = Σ_k c_k T_k(H~) x (bdg_apply_series)
// Part of the single translation unit bodge_hip.hip (included after fermi.hpp): the kernels live in
// namespace bdg beside the Clenshaw kernels of fermi.hpp, the driver in the unnamed namespace beside
// run_fermi_blocks.
//
// Clenshaw with a stored source.  Every batch column is a pair (vector v, function f):
//     b_{M} = b_{M+1} = 0,   b_k = 2 H~ b_{k+1} - b_{k+2} + c_k[f] x_v   (k = M-1 .. 1),
//     y = H~ b_1 - b_2 + c_0[f] x_v
// (H~ = H / scale).  x is a third vector buffer in the batch layout and c_k a complex coefficient per
// column, read from a device table; no colour array is read and no dot product is formed.  A launch moves
// what a Clenshaw step of fermi.hpp moves plus one read of x: four vector passes instead of three.
//
// A lane payload (double2) is ONE complex column in every mode.  In the real modes (Mode::kVec == 2) the
// matrix arithmetic treats .x and .y as two real vectors; H is real there, so it acts on the real and the
// imaginary part of a complex column alike and the two slots carry Re and Im.  Only the source term couples
// them: one complex multiply-add per payload, the same code in all four modes.
#pragma once

namespace bdg {

// What a stored-source Clenshaw launch reads besides a recurrence step's arguments.  Column r of the batch is
// the pair (vector, function) number col_base + r of the call, function (col_base + r) % n_functions; columns
// from n_active on are padding (x is zero there, and so is their coefficient).
struct ApplyArgs {
    StepArgs s;              // matrix, vector buffers, tiles; partial / discard / col_* are not read
    const double2* x;        // the source vectors, planar [4][nb][RL] like cur / prev
    const double2* coef_row; // c_k[f], f < n_functions: row k of the device table [n_moments][n_functions]
    int n_functions;
    int col_base;
    int n_active;
};

// Function of lane payload r's column (-1 on the padding columns), and c_k of that function (0 on padding)
__device__ inline int apply_function(const ApplyArgs& a, int r) {
    return r < a.n_active ? (a.col_base + r) % a.n_functions : -1;
}
__device__ inline double2 apply_coefficient(const ApplyArgs& a, int f) {
    return f >= 0 ? a.coef_row[f] : make_double2(0.0, 0.0);
}

// v += c * x as complex numbers
__device__ inline void add_stored_source(double2& v, double2 c, double2 x) {
    v.x = fma(c.x, x.x, v.x);
    v.x = fma(-c.y, x.y, v.x);
    v.y = fma(c.x, x.y, v.y);
    v.y = fma(c.y, x.x, v.y);
}

// The tail of the stored-source Clenshaw step b_k = coef * (H b_{k+1}) - b_{k+2} + c_k x on the shared tile loops
// (family.hpp): the column's coefficient, and before the store one more vector load (x, into the tile loop's dead
// registers) and the complex multiply-add.  The two forms carry the coefficient differently, each as its registers
// allow: the dictionary form reads it once per kernel; the streamed-block form keeps only the function index.
template <bool DICTIONARY>
struct ApplyTail : FamilyTail {
    using Args = ApplyArgs;
    static constexpr const char* kFamily = "stored-source Clenshaw";
    using Column = std::conditional_t<DICTIONARY, double2, int>;
    template <typename Mode, int RL>
    __device__ static Column begin(const ApplyArgs& ca, int r, double2*) {
        if constexpr (DICTIONARY) return apply_coefficient(ca, apply_function(ca, r));
        else return apply_function(ca, r);
    }
    template <typename Mode, int RL>
    __device__ static double2 row(const ApplyArgs& ca, Column column, int) {
        if constexpr (DICTIONARY) {
            return column;
        } else {
            // Read here and not before the tile loop, and from an index the compiler cannot see through: the kernel
            // is at its 128 registers across that loop, and a coefficient (or its address) kept there spills
            // (ComplexPHMode, 12 - 20 bytes per lane with hipcc of ROCm 7.2.0, AMD clang 22.0.0git: checked on that
            // compiler only - tests/test_apply_host.py pins scratch = 0 for every instance, so another compiler that
            // sees through the empty asm, or needs no such help, shows up there).
            int f = column;
            asm volatile("" : "+v"(f));
            return apply_coefficient(ca, f);
        }
    }
    template <typename Mode, int RL>
    __device__ static void amend(const ApplyArgs& ca, double2 ck, int i, int r, double2 nx[4], double2 x[4]) {
        const StepArgs& a = ca.s;
#pragma unroll
        for (int al = 0; al < 4; ++al) {
            const size_t own = vslot(al, (size_t)i, r, a.ncols, RL);
            x[al] = (a.stream_vectors & 1) ? load_stream(ca.x + own) : ca.x[own];
        }
#pragma unroll
        for (int al = 0; al < 4; ++al) add_stored_source(nx[al], ck, x[al]);
    }
};

// Host vectors (site-major complex, `n_stage` of them one after the other, the first being vector `vec_base`
// of the call) into the batch layout: column r takes vector (col_base + r) / n_functions, padding columns 0.
__global__ void apply_scatter(const double2* __restrict__ stage, double2* __restrict__ planar, int64_t nb, int rl,
                              int n_active, int col_base, int n_functions, int vec_base) {
    const int64_t total = 4 * nb * rl;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx % rl);
        const int64_t e = idx / rl;  // 4 * site + component
        double2 v = make_double2(0.0, 0.0);
        if (r < n_active) v = stage[(size_t)((col_base + r) / n_functions - vec_base) * 4 * nb + e];
        planar[vslot((int)(e & 3), (size_t)(e >> 2), r, (size_t)nb, rl)] = v;
    }
}

// The first n_active columns of a batch back to site-major order, column r at out + r * 4 * nb.
__global__ void apply_gather(const double2* __restrict__ planar, double2* __restrict__ out, int64_t nb, int rl,
                             int n_active) {
    const int64_t total = 4 * nb * n_active;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx % n_active);
        const int64_t e = idx / n_active;
        out[(size_t)r * 4 * nb + e] = planar[vslot((int)(e & 3), (size_t)(e >> 2), r, (size_t)nb, rl)];
    }
}

}  // namespace bdg

namespace {

using ApplyKernels = FamilyKernels<bdg::ApplyTail<false>, SharedDictKernels<bdg::ApplyTail<true>>>;

// HBM bytes of one stored-source launch: a recurrence launch's matrix stream, and FOUR vector passes where it has
// three (read b_{k+1}, b_{k+2} and x, write b_k), plus the launch's row of the coefficient table.
double apply_bytes(const bdg_system* sys, int vectors, const ModeInfo& mode, bool dictionary, int n_functions) {
    return algorithmic_bytes(sys, vectors, mode, dictionary) +
           mode.entry_bytes / 3.0 * (double)vectors * (double)sys->nb + 16.0 * n_functions;
}

// The batch loop of a stored-source series: the columns (vector, function) of the call in batches of the one-step
// width, every batch staged site-major in vec_d on the way in and on the way out.  `x` and `y_out` are host arrays
// (bdg_apply_series) or, with `on_device`, device arrays in the same vector-major order (the block of subspace.hpp:
// the staging buffer is then filled from and emptied to the block; x == y_out is allowed when n_functions == 1, a
// batch reads and writes its own columns only).  `coef` is on the host in both cases.  `record` = leave the call's
// figures in sys->perf.
int apply_series_batches(bdg_system* sys, double scale, int n_moments, int n_functions, const double* coef, int n_vectors,
                         const double* x, double* y_out, bool on_device, bool record) {
    const int64_t n_columns = (int64_t)n_vectors * n_functions;
    const int64_t nb = sys->nb;
    const hipMemcpyKind kind_in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind kind_out = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;

    // Real arithmetic whenever the matrix is real: the columns may be complex all the same (Re and Im in the two
    // slots of a payload).  In every mode a payload is one column, so `rl` lanes carry rl columns.
    const ModeInfo mode = family_mode(sys);
    const bool real = mode.real;
    const int per_lane = mode.per_lane;
    // Columns per batch by the one-step width rule: the widest power of two whose vector buffer (16 B per entry
    // and column) stays within 96 MB, at most 64 columns - 32 in real arithmetic, whose kernels count a column as
    // two of their 64 vectors; set_lanes_per_row fixes the lanes instead.
    const double per_column = (double)nb * 4 * 16.0;
    int width = real ? 32 : 64;
    while (width > 4 && width * per_column > 96.0 * 1024 * 1024) width >>= 1;
    int rl = std::max(4, next_pow2((int)std::min<int64_t>(n_columns, width)));
    if (sys->lanes_override >= 4) rl = sys->lanes_override;
    FamilyPlan<ApplyKernels::Kernel> aplan;
    if (int rc = make_family_plan<ApplyKernels>(sys, rl, mode, 0, &aplan)) return rc;
    const StepPlan& plan = aplan.step;
    const int rv = rl * per_lane;
    bdg::StepArgs base{};
    if (int rc = matrix_args(sys, plan, &base)) return rc;
    int strip_rows = 0;
    if (int rc = prepare_tile_order(sys, plan.rows_per_tile, plan.n_tiles, 64.0 * rl, &base.tile_order, &strip_rows))
        return rc;
    const size_t vec_count = (size_t)4 * nb * rl;
    const VectorHints hints = family_vector_hints(vec_count);
    base.stream_vectors = hints.stream_vectors;
    const bool alternate = hints.alternate;
    const int n_batches = (int)((n_columns + rl - 1) / rl);

    // Side by side on two of the handle's stream sets while one launch leaves the GPU part empty (the rule of
    // run_recurrence for the one-step kernels); BODGE_AMD_STREAMS overrides.
    int n_streams = (double)nb * rv <= kSideBySideOneStepLimit ? 2 : 1;
    if (const char* env = knob::raw("BODGE_AMD_STREAMS")) n_streams = std::clamp(atoi(env), 1, 4);
    n_streams = std::max(1, std::min(n_streams, n_batches));
    while ((int)sys->side_sets.size() < n_streams - 1) {
        auto side = std::make_unique<StreamSet>();
        if (int rc = pooled_stream(sys->device, (int)sys->side_sets.size(), &side->stream)) return fail(rc, "stream creation failed");
        sys->side_sets.push_back(std::move(side));
    }
    std::vector<StreamSet*> sets{sys};
    for (int s = 1; s < n_streams; ++s) sets.push_back(sys->side_sets[(size_t)s - 1].get());
    // per set: b_{k+1} / b_{k+2} (vec_a, vec_b), the source x (vec_c) and the site-major staging of the batch's
    // vectors on the way in and of its columns on the way out (vec_d)
    for (StreamSet* set : sets) {
        if (int rc = set->vec_a.reserve(vec_count)) return rc;
        if (int rc = set->vec_b.reserve(vec_count)) return rc;
        if (int rc = set->vec_c.reserve(vec_count)) return rc;
        if (int rc = set->vec_d.reserve(vec_count)) return rc;
    }

    DeviceBuffer<double2> d_coef;
    std::vector<hipEvent_t> events;
    const size_t vec_len = (size_t)4 * nb;  // complex entries of one host vector
    auto body = [&]() -> int {
        if (int rc = d_coef.reserve((size_t)n_moments * n_functions)) return rc;
        hipStream_t st = sys->stream;
        HIP_TRY(hipMemcpyAsync(d_coef.ptr, coef, sizeof(double2) * (size_t)n_moments * n_functions, hipMemcpyHostToDevice, st));
        // (tables, packed blocks and the upload above are on the handle's stream: the side streams wait for them)
        if (!sys->ev_side) HIP_TRY(hipEventCreateWithFlags(&sys->ev_side, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(sys->ev_side, st));
        for (int s = 1; s < n_streams; ++s) HIP_TRY(hipStreamWaitEvent(sets[(size_t)s]->stream, sys->ev_side, 0));
        events.assign((size_t)2 * n_batches, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        const int fill_grid = (int)std::min<size_t>(4096, (vec_count + 255) / 256);
        bdg_perf perf{};
        for (int first = 0; first < n_batches; first += n_streams) {
            const int last = std::min(n_batches, first + n_streams);
            std::vector<bdg::ApplyArgs> args((size_t)(last - first));
            std::vector<double2*> cur((size_t)(last - first)), prev((size_t)(last - first));
            for (int b = first; b < last; ++b) {
                const size_t q = (size_t)(b - first);
                StreamSet* set = sets[q];
                bdg::ApplyArgs& ca = args[q];
                ca.s = base;
                ca.x = set->vec_c.ptr;
                ca.n_functions = n_functions;
                ca.col_base = b * rl;
                ca.n_active = (int)std::min<int64_t>(rl, n_columns - (int64_t)ca.col_base);
                cur[q] = set->vec_a.ptr;
                prev[q] = set->vec_b.ptr;
                // the vectors this batch's columns belong to: at most rl of them, so they fit the staging buffer
                const int v_lo = ca.col_base / n_functions;
                const int v_hi = (ca.col_base + ca.n_active - 1) / n_functions;
                HIP_TRY(hipMemcpyAsync(set->vec_d.ptr, x + (size_t)2 * vec_len * v_lo,
                                       sizeof(double2) * vec_len * (size_t)(v_hi - v_lo + 1), kind_in, set->stream));
                bdg::apply_scatter<<<fill_grid, 256, 0, set->stream>>>(set->vec_d.ptr, set->vec_c.ptr, nb, rl, ca.n_active,
                                                                        ca.col_base, n_functions, v_lo);
                bdg::fill_zero<<<fill_grid, 256, 0, set->stream>>>(set->vec_a.ptr, (int64_t)vec_count);
                bdg::fill_zero<<<fill_grid, 256, 0, set->stream>>>(set->vec_b.ptr, (int64_t)vec_count);
                HIP_TRY(hipEventRecord(events[(size_t)2 * b], set->stream));
            }
            // b_k for k = M-1 .. 1, then y: one launch per coefficient, the batches of the round in turn
            for (int n = 0; n < n_moments; ++n) {
                const int k = n_moments - 1 - n;
                for (int b = first; b < last; ++b) {
                    const size_t q = (size_t)(b - first);
                    bdg::ApplyArgs& ca = args[q];
                    ca.s.cur = cur[q];
                    ca.s.prev = prev[q];
                    ca.s.coef = (k == 0 ? 1.0 : 2.0) / scale;
                    ca.s.reverse = alternate ? (n & 1) : 0;
                    ca.coef_row = d_coef.ptr + (size_t)k * n_functions;
                    aplan.kernel<<<plan.grid, bdg::kBlockThreads, plan.lds_bytes, sets[q]->stream>>>(ca);
                    std::swap(cur[q], prev[q]);
                }
            }
            for (int b = first; b < last; ++b) {
                const size_t q = (size_t)(b - first);
                HIP_TRY(hipEventRecord(events[(size_t)2 * b + 1], sets[q]->stream));
                const int64_t total = (int64_t)vec_len * args[q].n_active;
                const int grid = (int)std::min<int64_t>(4096, (total + 255) / 256);
                bdg::apply_gather<<<grid, 256, 0, sets[q]->stream>>>(cur[q], sets[q]->vec_d.ptr, nb, rl, args[q].n_active);
                perf.vector_steps += (int64_t)n_moments * args[q].n_active;
            }
            HIP_TRY(hipGetLastError());
            for (int b = first; b < last; ++b) {
                const size_t q = (size_t)(b - first);
                HIP_TRY(hipMemcpyAsync(y_out + (size_t)2 * vec_len * args[q].col_base, sets[q]->vec_d.ptr,
                                       sizeof(double2) * vec_len * (size_t)args[q].n_active, kind_out, sets[q]->stream));
            }
        }
        for (int s = 1; s < n_streams; ++s) HIP_TRY(hipStreamSynchronize(sets[(size_t)s]->stream));
        HIP_TRY(hipStreamSynchronize(st));
        float window = 0.f;
        for (int b = 0; b < n_batches; ++b) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, events[(size_t)2 * b], events[(size_t)2 * b + 1]));
            perf.kernel_ms += t;
            HIP_TRY(hipEventElapsedTime(&t, events[0], events[(size_t)2 * b + 1]));
            window = std::max(window, t);
        }
        perf.window_ms = window;
        perf.launches = (int64_t)n_batches * n_moments;
        perf.bytes_per_launch = apply_bytes(sys, rv, mode, plan.dictionary, n_functions);
        perf.bytes_moved = perf.bytes_per_launch * (double)perf.launches;
        family_perf(sys, plan, rv, strip_rows, n_streams, &perf);
        perf.apply = plan.dictionary ? 2 : 1;
        if (record) sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) {
        (void)hipStreamSynchronize(sys->stream);
        for (auto& side : sys->side_sets) (void)hipStreamSynchronize(side->stream);
    }
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    d_coef.release();
    return rc;
}

int run_apply_series(bdg_system* sys, double scale, int n_moments, int n_functions, const double* coef, int n_vectors,
                     const double* x, double* y_out) {
    // (argument errors first, the scalar ones before the handle is looked at: none of them needs a GPU)
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_functions < 1) return fail(BDG_EINVAL, "n_functions must be >= 1");
    if (n_vectors < 1) return fail(BDG_EINVAL, "n_vectors must be >= 1");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (!coef || !x || !y_out) return fail(BDG_EINVAL, "null argument");
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_apply_series needs a whole (square) matrix: slabs are not supported");
    if ((int64_t)n_vectors * n_functions > INT32_MAX) return fail(BDG_EINVAL, "n_vectors x n_functions exceeds 2^31 - 1 columns");
    lanczos_free(sys);
    HIP_TRY(hipSetDevice(sys->device));
    return apply_series_batches(sys, scale, n_moments, n_functions, coef, n_vectors, x, y_out, false, true);
}

}  // namespace
