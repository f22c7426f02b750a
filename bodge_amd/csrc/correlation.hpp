// correlation.hpp - double Chebyshev moments mu[n, m] = sum_v <v|T_n(H~) A T_m(H~) B|v> (bdg_moment_matrix)
// Part of the single translation unit bodge_hip.hip (included after apply.hpp): the kernels live in namespace
// bdg, the driver in the unnamed namespace beside run_apply_series;
// set-up and lanes by family_setup and the column rule of family.hpp.
//
// Two recurrences and a Gram product.  For a batch of start columns |r> in the planar batch
// layout of apply.hpp (double2[4][nb][rl], one payload = one complex column in every arithmetic mode):
//     X_n = T_n(H~) |r>,   Y_m = A T_m(H~) B |r>,   mu[n, m] += <X_n|Y_m>      (n, m < M,  H~ = H / scale)
// X and Y advance through the stored-source Clenshaw kernels of apply.hpp with a zero coefficient (a plain step
// 2 H~ t_n - t_{n-1}); every t_n is copied out into a row of a panel (X: device-to-device copy, Y: corr_operator
// applies A on the way).  A panel row holds K = 4 nb rl complex entries.  The hot path is the tall-skinny complex
// Gram product of the two panels, O(M^2 K), against O(M) sparse products: corr_gram, fp64 MFMA.
//
// Summation order of one mu entry: slices of K of fixed length (BODGE_AMD_CORRELATION_SLICE) summed by one
// workgroup each in ascending k, then the slices in ascending order (corr_reduce), then the batches in order.
// It depends on K alone - not on M, not on how the moments are blocked - and no atomic is used.
#pragma once

namespace bdg {

// y = Op t on the planar batch layout: Op a BSR matrix with its own pattern and full 4x4 complex blocks
// (scipy order), complex arithmetic on the payload, out of place.  One thread per (block row, column).
__global__ void corr_operator(const int* __restrict__ indptr, const int* __restrict__ indices,
                              const double2* __restrict__ blocks, const double2* __restrict__ t,
                              double2* __restrict__ y, int64_t nb, int rl) {
    const int64_t total = nb * rl;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx % rl);
        const int64_t i = idx / rl;
        double2 acc[4];
#pragma unroll
        for (int al = 0; al < 4; ++al) acc[al] = make_double2(0.0, 0.0);
        for (int k = indptr[i]; k < indptr[i + 1]; ++k) {
            const size_t j = (size_t)indices[k];
            const double2* blk = blocks + (size_t)16 * k;
            double2 x[4];
#pragma unroll
            for (int be = 0; be < 4; ++be) x[be] = t[vslot(be, j, r, (size_t)nb, rl)];
#pragma unroll
            for (int al = 0; al < 4; ++al)
#pragma unroll
                for (int be = 0; be < 4; ++be) {
                    const double2 h = blk[4 * al + be];
                    acc[al].x = fma(h.x, x[be].x, acc[al].x);
                    acc[al].x = fma(-h.y, x[be].y, acc[al].x);
                    acc[al].y = fma(h.x, x[be].y, acc[al].y);
                    acc[al].y = fma(h.y, x[be].x, acc[al].y);
                }
        }
#pragma unroll
        for (int al = 0; al < 4; ++al) y[vslot(al, (size_t)i, r, (size_t)nb, rl)] = acc[al];
    }
}

// P[s][n][m] = sum_{k in slice s} conj(X[n][k]) Y[m][k]: rows of K contiguous complex entries, row stride K.
// Grid (ceil(rows_x / 64), ceil(rows_y / 64), slices); 256 threads per 64 x 64 tile of mu, one wave per 32 x 32
// sub-tile as 2 x 2 tiles of v_mfma_f64_16x16x4_f64.  conj(x) y = (xr yr + xi yi) + i (xr yi - xi yr): four real
// products into two accumulators per tile.  Lane l (i = l & 15, kk = l >> 4) supplies A[row i][k = kk] and
// B[k = kk][col i]; it receives D[row kk + 4 reg][col i], reg < 4 (the f64 map: not that of the other MFMAs).
// Operands are staged through LDS in steps of 16 k: a [k][row] image with rows of 65 entries (a 16-lane group of a
// 16-byte read then covers 16 different slots), the next step's entries fetched into registers meanwhile.
// Rows beyond the panel heights and k beyond the end of the slice are never read: they enter as zero.
constexpr int kCorrTile = 64;   // rows of X and of Y per workgroup
constexpr int kCorrStepK = 16;  // k per LDS stage
constexpr int kCorrLd = kCorrTile + 1;

__device__ __forceinline__ void corr_fetch(const double2* __restrict__ panel, int rows, int row0, int64_t ld,
                                           int64_t k, int64_t k_hi, int r, double2 (&v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int row = row0 + r + 16 * u;
        v[u] = make_double2(0.0, 0.0);
        if (row < rows && k < k_hi) v[u] = panel[(size_t)row * ld + k];
    }
}

__global__ __launch_bounds__(256, 2) void corr_gram(const double2* __restrict__ xp, const double2* __restrict__ yp,
                                                    int rows_x, int rows_y, int64_t K, int slice,
                                                    double2* __restrict__ part) {
    __shared__ double2 xs[kCorrStepK * kCorrLd];
    __shared__ double2 ys[kCorrStepK * kCorrLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kk = lane >> 4;
    const int n0 = blockIdx.x * kCorrTile, m0 = blockIdx.y * kCorrTile;
    const int wn = (wave >> 1) * 32, wm = (wave & 1) * 32;
    const int64_t k_lo = (int64_t)blockIdx.z * slice;
    const int64_t k_hi = min(K, k_lo + (int64_t)slice);
    const int kq = threadIdx.x & 15, r = threadIdx.x >> 4;  // staging: this thread's k and its first row

    v4f64 pr[2][2], pi[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            pr[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
            pi[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
        }

    double2 gx[4], gy[4];
    corr_fetch(xp, rows_x, n0, K, k_lo + kq, k_hi, r, gx);
    corr_fetch(yp, rows_y, m0, K, k_lo + kq, k_hi, r, gy);
    for (int64_t k0 = k_lo; k0 < k_hi; k0 += kCorrStepK) {
        __syncthreads();  // (the stage before has been read)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            xs[kq * kCorrLd + r + 16 * u] = gx[u];
            ys[kq * kCorrLd + r + 16 * u] = gy[u];
        }
        __syncthreads();
        if (k0 + kCorrStepK < k_hi) {
            corr_fetch(xp, rows_x, n0, K, k0 + kCorrStepK + kq, k_hi, r, gx);
            corr_fetch(yp, rows_y, m0, K, k0 + kCorrStepK + kq, k_hi, r, gy);
        }
#pragma unroll
        for (int ks = 0; ks < kCorrStepK; ks += 4) {
            double2 xa[2], yb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                xa[a] = xs[(ks + kk) * kCorrLd + wn + 16 * a + i];
                yb[a] = ys[(ks + kk) * kCorrLd + wm + 16 * a + i];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    pr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[a].x, yb[b].x, pr[a][b], 0, 0, 0);
                    pr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[a].y, yb[b].y, pr[a][b], 0, 0, 0);
                    pi[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[a].x, yb[b].y, pi[a][b], 0, 0, 0);
                    pi[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[a].y, yb[b].x, pi[a][b], 0, 0, 0);
                }
        }
    }

    double2* out = part + (size_t)blockIdx.z * rows_x * rows_y;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int n = n0 + wn + 16 * a + kk + 4 * reg;
                const int m = m0 + wm + 16 * b + i;
                if (n < rows_x && m < rows_y) out[(size_t)n * rows_y + m] = make_double2(pr[a][b][reg], pi[a][b][reg]);
            }
}

// mu[n0 + n][m0 + m] += sum_s P[s][n][m], s ascending: one thread per entry, no atomics.
__global__ void corr_reduce(const double2* __restrict__ part, int slices, int rows_x, int rows_y, double2* __restrict__ mu,
                            int n_moments, int n0, int m0) {
    const int64_t count = (int64_t)rows_x * rows_y;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        double re = 0.0, im = 0.0;
        for (int s = 0; s < slices; ++s) {
            const double2 p = part[(size_t)s * count + e];
            re += p.x;
            im += p.y;
        }
        const int n = (int)(e / rows_y), m = (int)(e % rows_y);
        double2& dst = mu[(size_t)(n0 + n) * n_moments + m0 + m];
        dst.x += re;
        dst.y += im;
    }
}

}  // namespace bdg

namespace {

constexpr size_t kCorrelationBytes = (size_t)4 << 30;  // both panels together
constexpr int kCorrelationSlice = 4096;                // complex entries of a panel row per workgroup of corr_gram

// The checks of an operator that need no matrix size, and those that do.
int check_operator_shape(const bdg_operator* op, const char* name) {
    if (op->nnzb < 0) return fail(BDG_EINVAL, "operator %s: negative block count", name);
    if (!op->indptr || (op->nnzb > 0 && (!op->indices || !op->data)))
        return fail(BDG_EINVAL, "operator %s: null array", name);
    return BDG_OK;
}
int check_operator(const bdg_operator* op, const char* name, int64_t nb) {
    if (op->indptr[0] != 0 || op->indptr[nb] != op->nnzb)
        return fail(BDG_EINVAL, "operator %s: indptr[nb] = %d does not match its %d blocks", name, op->indptr[nb], op->nnzb);
    for (int64_t i = 0; i < nb; ++i)
        if (op->indptr[i + 1] < op->indptr[i] || op->indptr[i + 1] > op->nnzb)
            return fail(BDG_EINVAL, "operator %s: indptr is not monotone within [0, nnzb] at row %lld", name, (long long)i);
    for (int32_t k = 0; k < op->nnzb; ++k)
        if (op->indices[k] < 0 || op->indices[k] >= nb)
            return fail(BDG_EINVAL, "operator %s: column index %d out of range", name, op->indices[k]);
    return BDG_OK;
}

struct DeviceOperator {
    DeviceBuffer<int> indptr, indices;
    DeviceBuffer<double2> blocks;
    int upload(const bdg_operator* op, int64_t nb, hipStream_t st) {
        if (int rc = indptr.reserve((size_t)nb + 1)) return rc;
        if (int rc = indices.reserve((size_t)std::max(1, op->nnzb))) return rc;
        if (int rc = blocks.reserve((size_t)std::max(1, op->nnzb) * 16)) return rc;
        HIP_TRY(hipMemcpyAsync(indptr.ptr, op->indptr, sizeof(int) * (size_t)(nb + 1), hipMemcpyHostToDevice, st));
        if (op->nnzb > 0) {
            HIP_TRY(hipMemcpyAsync(indices.ptr, op->indices, sizeof(int) * (size_t)op->nnzb, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(blocks.ptr, op->data, sizeof(double2) * 16 * (size_t)op->nnzb, hipMemcpyHostToDevice, st));
        }
        return BDG_OK;
    }
    void release() {
        indptr.release();
        indices.release();
        blocks.release();
    }
};

int run_moment_matrix(bdg_system* sys, double scale, int n_moments, const bdg_operator* a, const bdg_operator* b,
                      int n_vectors, const int64_t* rows, const double* x, double* mu_out) {
    // (argument errors first, in the order of the header; none of them needs a GPU)
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_vectors < 1) return fail(BDG_EINVAL, "n_vectors must be >= 1");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (!a || !b || !mu_out) return fail(BDG_EINVAL, "null argument");
    if ((rows != nullptr) == (x != nullptr))
        return fail(BDG_EINVAL, "give exactly one of rows (unit start vectors) and x (caller vectors)");
    if (int rc = check_operator_shape(a, "A")) return rc;
    if (int rc = check_operator_shape(b, "B")) return rc;
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    // (what of an operator can only be checked against the matrix size comes here, before anything else of the handle)
    const int64_t nb = sys->nb;
    if (int rc = check_operator(a, "A", nb)) return rc;
    if (int rc = check_operator(b, "B", nb)) return rc;
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_moment_matrix needs a whole (square) matrix: slabs are not supported");
    if (rows)
        for (int v = 0; v < n_vectors; ++v)
            if (rows[v] < 0 || rows[v] >= 4 * nb) return fail(BDG_EINVAL, "start row %lld out of range", (long long)rows[v]);
    lanczos_free(sys);
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic mode of the family, columns per batch by its column rule (family.hpp).
    const ModeInfo mode = family_mode(sys);
    int rl = family_column_lanes(sys, mode, n_vectors);

    // Panels: Mb rows each, the largest multiple of 64 (or M itself) for which both stay within the budget.  A batch
    // that is too wide even for 64 rows is narrowed (down to 4 lanes) unless the lanes are fixed.
    size_t budget = kCorrelationBytes;
    if (const char* env = knob::raw("BODGE_AMD_CORRELATION_BYTES")) budget = (size_t)std::max(1LL, atoll(env));
    int slice = kCorrelationSlice;
    if (const char* env = knob::raw("BODGE_AMD_CORRELATION_SLICE")) slice = atoi(env);
    if (slice < 4 || (slice & 3)) return fail(BDG_EINVAL, "BODGE_AMD_CORRELATION_SLICE must be a positive multiple of 4");
    auto panel_rows = [&](int lanes) -> int {
        const size_t row_bytes = (size_t)4 * nb * lanes * sizeof(double2);
        if ((size_t)2 * n_moments * row_bytes <= budget) return n_moments;
        const size_t fit = budget / (2 * row_bytes) / 64 * 64;
        return fit >= (size_t)n_moments ? 0 : (int)fit;  // (fewer than 64 rows fit, and M itself does not: 0)
    };
    int mb = panel_rows(rl);
    while (mb == 0 && rl > 4 && sys->lanes_override < 4) mb = panel_rows(rl >>= 1);
    if (mb == 0)
        return fail(BDG_EINVAL,
                    "bdg_moment_matrix: two panels of %d rows at %d lanes need %zu bytes, BODGE_AMD_CORRELATION_BYTES allows %zu",
                    std::min(n_moments, 64), rl, (size_t)2 * std::min(n_moments, 64) * 4 * nb * rl * sizeof(double2), budget);
    const int n_chunks = (n_moments + mb - 1) / mb;
    const int64_t K = (int64_t)4 * nb * rl;
    const int64_t n_slices = (K + slice - 1) / slice;
    if (n_slices > 65535) return fail(BDG_EINVAL, "BODGE_AMD_CORRELATION_SLICE = %d cuts a panel row into more than 65535 slices", slice);

    // (the lanes are final only here, after the panels may have narrowed them)
    FamilySetup<ApplyKernels> fs;
    if (int rc = family_setup(sys, mode, rl, 0, &fs)) return rc;
    const StepPlan& plan = fs.plan.step;
    const size_t vec_count = fs.vec_count;  // = K
    const int n_batches = (n_vectors + rl - 1) / rl;

    // start batch (kept: the X recurrence restarts from it), the two vector pairs, the caller's vectors of a batch
    DeviceBuffer<double2> d_start, d_xa, d_xb, d_ya, d_yb, d_stage, d_xpanel, d_ypanel, d_part, d_mu, d_coef;
    DeviceBuffer<int64_t> d_rows;
    DeviceOperator op_a, op_b;
    std::vector<hipEvent_t> events;  // (start, stop) per Gram + reduce, then the window's two
    auto body = [&]() -> int {
        hipStream_t st = sys->stream;
        for (DeviceBuffer<double2>* buf : {&d_start, &d_xa, &d_xb, &d_ya, &d_yb})
            if (int rc = buf->reserve(vec_count)) return rc;
        if (x) {
            if (int rc = d_stage.reserve(vec_count)) return rc;
        } else {
            if (int rc = d_rows.reserve((size_t)n_vectors)) return rc;
            HIP_TRY(hipMemcpyAsync(d_rows.ptr, rows, sizeof(int64_t) * (size_t)n_vectors, hipMemcpyHostToDevice, st));
        }
        if (int rc = d_xpanel.reserve((size_t)mb * vec_count)) return rc;
        if (int rc = d_ypanel.reserve((size_t)mb * vec_count)) return rc;
        if (int rc = d_part.reserve((size_t)n_slices * mb * mb)) return rc;
        if (int rc = d_mu.reserve((size_t)n_moments * n_moments)) return rc;
        if (int rc = d_coef.reserve(2)) return rc;
        if (int rc = op_a.upload(a, nb, st)) return rc;
        if (int rc = op_b.upload(b, nb, st)) return rc;
        // coefficient rows of the stored-source kernel: 0 = a plain step, 1 = the source itself (the restart of X)
        const double coef_rows[4] = {0.0, 0.0, 1.0, 0.0};
        HIP_TRY(hipMemcpyAsync(d_coef.ptr, coef_rows, sizeof coef_rows, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_mu.ptr, 0, sizeof(double2) * (size_t)n_moments * n_moments, st));
        events.assign((size_t)2 * n_batches * n_chunks * n_chunks + 2, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        const int fill_grid = (int)std::min<size_t>(4096, (vec_count + 255) / 256);
        const int op_grid = (int)std::min<int64_t>(4096, (nb * rl + 255) / 256);
        const size_t vec_len = (size_t)4 * nb;  // complex entries of one host vector
        bdg_perf perf{};
        size_t ev = 0;
        HIP_TRY(hipEventRecord(events[events.size() - 2], st));
        for (int bt = 0; bt < n_batches; ++bt) {
            const int col_base = bt * rl;
            const int n_active = std::min(rl, n_vectors - col_base);
            bdg::ApplyArgs ca{};
            ca.s = fs.base;
            ca.x = d_start.ptr;
            ca.n_functions = 1;
            ca.col_base = 0;
            ca.n_active = n_active;
            int64_t launches = 0;
            // one launch of the recurrence kernel: prev <- coef H cur - prev + c x, c = 0 (plain step) or 1
            auto step = [&](double2*& cur, double2*& prev, double coef, int parity, int coef_row) {
                ca.s.cur = cur;
                ca.s.prev = prev;
                ca.s.coef = coef;
                ca.s.reverse = fs.alternate ? (parity & 1) : 0;
                ca.coef_row = d_coef.ptr + coef_row;
                fs.plan.kernel<<<plan.grid, bdg::kBlockThreads, plan.lds_bytes, st>>>(ca);
                std::swap(cur, prev);
                ++launches;
            };
            if (x) {
                HIP_TRY(hipMemcpyAsync(d_stage.ptr, x + (size_t)2 * vec_len * col_base, sizeof(double2) * vec_len * (size_t)n_active,
                                       hipMemcpyHostToDevice, st));
                bdg::apply_scatter<<<fill_grid, 256, 0, st>>>(d_stage.ptr, d_start.ptr, nb, rl, n_active, col_base, 1, col_base);
            } else {
                bdg::fill_zero<<<fill_grid, 256, 0, st>>>(d_start.ptr, (int64_t)vec_count);
                bdg::set_unit<<<1, 64, 0, st>>>(d_start.ptr, nb, nb, rl, n_active, d_rows.ptr + col_base, (int64_t)0);
            }
            // Y: t_0 = B |r>
            double2* ycur = d_ya.ptr;
            double2* yprev = d_yb.ptr;
            bdg::corr_operator<<<op_grid, 256, 0, st>>>(op_b.indptr.ptr, op_b.indices.ptr, op_b.blocks.ptr, d_start.ptr, ycur, nb, rl);
            bdg::fill_zero<<<fill_grid, 256, 0, st>>>(yprev, (int64_t)vec_count);
            for (int yc = 0; yc < n_chunks; ++yc) {
                const int m0 = yc * mb, m1 = std::min(n_moments, m0 + mb);
                for (int m = m0; m < m1; ++m) {
                    if (m > 0) step(ycur, yprev, (m == 1 ? 1.0 : 2.0) / scale, m, 0);
                    bdg::corr_operator<<<op_grid, 256, 0, st>>>(op_a.indptr.ptr, op_a.indices.ptr, op_a.blocks.ptr, ycur,
                                                                d_ypanel.ptr + (size_t)(m - m0) * vec_count, nb, rl);
                }
                // X from the kept start batch: the source enters zeroed buffers with coefficient 1
                double2* xcur = d_xa.ptr;
                double2* xprev = d_xb.ptr;
                bdg::fill_zero<<<fill_grid, 256, 0, st>>>(xcur, (int64_t)vec_count);
                bdg::fill_zero<<<fill_grid, 256, 0, st>>>(xprev, (int64_t)vec_count);
                step(xcur, xprev, 1.0 / scale, 0, 1);
                for (int xc = 0; xc < n_chunks; ++xc) {
                    const int n0 = xc * mb, n1 = std::min(n_moments, n0 + mb);
                    for (int n = n0; n < n1; ++n) {
                        if (n > 0) step(xcur, xprev, (n == 1 ? 1.0 : 2.0) / scale, n, 0);
                        HIP_TRY(hipMemcpyAsync(d_xpanel.ptr + (size_t)(n - n0) * vec_count, xcur, sizeof(double2) * vec_count,
                                               hipMemcpyDeviceToDevice, st));
                    }
                    const int rows_x = n1 - n0, rows_y = m1 - m0;
                    HIP_TRY(hipEventRecord(events[ev], st));
                    const dim3 grid((unsigned)((rows_x + bdg::kCorrTile - 1) / bdg::kCorrTile),
                                    (unsigned)((rows_y + bdg::kCorrTile - 1) / bdg::kCorrTile), (unsigned)n_slices);
                    bdg::corr_gram<<<grid, 256, 0, st>>>(d_xpanel.ptr, d_ypanel.ptr, rows_x, rows_y, K, slice, d_part.ptr);
                    const int red_grid = (int)std::min<int64_t>(4096, ((int64_t)rows_x * rows_y + 255) / 256);
                    bdg::corr_reduce<<<red_grid, 256, 0, st>>>(d_part.ptr, (int)n_slices, rows_x, rows_y, d_mu.ptr, n_moments, n0, m0);
                    HIP_TRY(hipEventRecord(events[ev + 1], st));
                    ev += 2;
                    perf.gram_flops += 8.0 * rows_x * rows_y * (double)K;
                }
            }
            HIP_TRY(hipGetLastError());
            perf.launches += launches;
            perf.vector_steps += launches * n_active;
        }
        HIP_TRY(hipEventRecord(events[events.size() - 1], st));
        HIP_TRY(hipMemcpyAsync(mu_out, d_mu.ptr, sizeof(double2) * (size_t)n_moments * n_moments, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t e = 0; e + 2 < events.size(); e += 2) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, events[e], events[e + 1]));
            perf.gram_ms += t;
        }
        float window = 0.f;
        HIP_TRY(hipEventElapsedTime(&window, events[events.size() - 2], events[events.size() - 1]));
        perf.window_ms = window;
        perf.kernel_ms = window;
        perf.bytes_per_launch = apply_bytes(sys, fs.rv, mode, plan.dictionary, 1);
        perf.bytes_moved = perf.bytes_per_launch * (double)perf.launches;
        family_perf(sys, plan, fs.rv, fs.strip_rows, 1, &perf);
        perf.correlation = 1;
        sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(sys->stream);
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    for (DeviceBuffer<double2>* buf : {&d_start, &d_xa, &d_xb, &d_ya, &d_yb, &d_stage, &d_xpanel, &d_ypanel, &d_part, &d_mu, &d_coef})
        buf->release();
    d_rows.release();
    op_a.release();
    op_b.release();
    return rc;
}

}  // namespace
