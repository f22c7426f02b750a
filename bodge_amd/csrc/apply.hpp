// apply.hpp - a Chebyshev series of H on caller-supplied vectors, y = Σ_k c_k T_k(H~) x (bdg_apply_series)
// Part of the single translation unit bodge_hip.hip (included after fermi.hpp): the kernels live in
// namespace bdg beside the Clenshaw kernels of fermi.hpp, the driver in the unnamed namespace: the feature
// ApplySeries on the rounds loop of family.hpp (run_family_rounds), which run_fermi_blocks runs too.
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

// A stored-source series on the rounds loop of family.hpp.  A batch is rl columns (vector, function) of the call; per
// stream set the loop's b_{k+1} / b_{k+2} (vec_a, vec_b), the source x (vec_c) and the site-major staging of the batch's
// vectors on the way in and of its columns on the way out (vec_d).
struct ApplySeries : FamilyFeature {
    using Args = bdg::ApplyArgs;
    static constexpr int32_t bdg_perf::*kFlag = &bdg_perf::apply;
    static constexpr int kVectors = 4;
    bdg_system* sys;
    const FamilySetup<ApplyKernels>& fs;
    int n_moments, n_functions;
    int64_t n_columns;
    const double* coef;
    const double* x;
    double* y_out;
    hipMemcpyKind kind_in, kind_out;
    bool kRecord;  // not a constant here, though it hides FamilyFeature's: the caller decides (false for bdg_subspace_project)
    double launch_bytes;
    DeviceBuffer<double2> d_coef;

    size_t vec_len() const { return (size_t)4 * sys->nb; }  // complex entries of one host vector
    int upload(hipStream_t st) {
        if (int rc = d_coef.reserve((size_t)n_moments * n_functions)) return rc;
        HIP_TRY(hipMemcpyAsync(d_coef.ptr, coef, sizeof(double2) * (size_t)n_moments * n_functions, hipMemcpyHostToDevice, st));
        return BDG_OK;
    }
    int start_batch(int b, StreamSet* set, Args* ca) {
        ca->x = set->vec_c.ptr;
        ca->n_functions = n_functions;
        ca->col_base = b * fs.rl;
        ca->n_active = (int)std::min<int64_t>(fs.rl, n_columns - (int64_t)ca->col_base);
        // the vectors this batch's columns belong to: at most rl of them, so they fit the staging buffer
        const int v_lo = ca->col_base / n_functions;
        const int v_hi = (ca->col_base + ca->n_active - 1) / n_functions;
        HIP_TRY(hipMemcpyAsync(set->vec_d.ptr, x + (size_t)2 * vec_len() * v_lo, sizeof(double2) * vec_len() * (size_t)(v_hi - v_lo + 1),
                               kind_in, set->stream));
        const int fill_grid = (int)std::min<size_t>(4096, (fs.vec_count + 255) / 256);
        bdg::apply_scatter<<<fill_grid, 256, 0, set->stream>>>(set->vec_d.ptr, set->vec_c.ptr, sys->nb, fs.rl, ca->n_active,
                                                                ca->col_base, n_functions, v_lo);
        return ca->n_active;
    }
    void point(Args* ca, int k) { ca->coef_row = d_coef.ptr + (size_t)k * n_functions; }
    void end_batch(int, StreamSet* set, const double2* y, const Args& ca) {
        const int64_t total = (int64_t)vec_len() * ca.n_active;
        const int grid = (int)std::min<int64_t>(4096, (total + 255) / 256);
        bdg::apply_gather<<<grid, 256, 0, set->stream>>>(y, set->vec_d.ptr, sys->nb, fs.rl, ca.n_active);
    }
    int drain_batch(int, StreamSet* set, const Args& ca) {
        HIP_TRY(hipMemcpyAsync(y_out + (size_t)2 * vec_len() * ca.col_base, set->vec_d.ptr, sizeof(double2) * vec_len() * (size_t)ca.n_active,
                               kind_out, set->stream));
        return BDG_OK;
    }
    // every stream has carried its own columns to y_out
    int finish(const std::vector<StreamSet*>& sets, hipStream_t) {
        for (size_t s = 1; s < sets.size(); ++s) HIP_TRY(hipStreamSynchronize(sets[s]->stream));
        return BDG_OK;
    }
    void release() { d_coef.release(); }
};

// The columns (vector, function) of the call in batches of the column rule's width (family.hpp).  `x` and `y_out` are
// host arrays (bdg_apply_series) or, with `on_device`, device arrays in the same vector-major order (the block of
// subspace.hpp: the staging buffer is then filled from and emptied to the block; x == y_out is allowed when
// n_functions == 1, a batch reads and writes its own columns only).  `coef` is on the host in both cases.  `record` =
// leave the call's figures in sys->perf.
int apply_series_batches(bdg_system* sys, double scale, int n_moments, int n_functions, const double* coef, int n_vectors,
                         const double* x, double* y_out, bool on_device, bool record) {
    const int64_t n_columns = (int64_t)n_vectors * n_functions;
    // Real arithmetic whenever the matrix is real: the columns may be complex all the same (Re and Im in the two
    // slots of a payload).  In every mode a payload is one column, so `rl` lanes carry rl columns.
    const ModeInfo mode = family_mode(sys);
    FamilySetup<ApplyKernels> fs;
    if (int rc = family_setup(sys, mode, family_column_lanes(sys, mode, n_columns), 0, &fs)) return rc;
    ApplySeries feature{{}, sys, fs, n_moments, n_functions, n_columns, coef, x, y_out,
                        on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                        on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, record,
                        apply_bytes(sys, fs.rv, mode, fs.plan.step.dictionary, n_functions)};
    return run_family_rounds(sys, fs, scale, n_moments, (int)((n_columns + fs.rl - 1) / fs.rl), feature);
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
