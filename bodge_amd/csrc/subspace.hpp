// subspace.hpp - a block of vectors that stays on the device: filter, Gram projection, rotation, residuals
// (bdg_subspace_*).  Part of the single translation unit bodge_hip.hip (included after lanczos.hpp): the kernels
// live in namespace bdg, the drivers in the unnamed namespace.
//
// Filtered subspace iteration.  The block is two arrays X and HX of B columns, vector-major: column
// c is K = 4 nb contiguous complex entries in the order of bdg_spmv (entry 4 * site + component).  That is the
// [row][K] panel corr_gram reads and the site-major staging layout apply_scatter / apply_gather move, so
//     filter    X <- sum_k c_k T_k(H~) X      the batch loop of bdg_apply_series, staged from and to the block
//     project   HX <- H X, S = X^† X, G = X^† HX    one more series (c = {0, 1}, scale 1), corr_gram + corr_reduce
//     rotate    X <- X Q, HX <- HX Q, r_j = |HX_j - theta_j X_j|    the kernels below
// need no change of layout between them.  A third array of the same size takes the out-of-place rotations.
// Nothing here uses an atomic: S, G and the residuals have the same bits from run to run.
#pragma once

namespace bdg {

// x[(first + c) K + e] = entry e of the start vector (seed, first_id + c), Rademacher: what bdg_random_vector returns.
__global__ void subspace_fill(double2* __restrict__ x, int64_t K, int count, uint64_t seed, uint64_t first_id) {
    const int64_t total = K * count;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = idx / K, e = idx % K;
        x[idx] = start_entry(vector_key(seed, first_id + (uint64_t)c), (uint64_t)e, 0);
    }
}

// out[j][k] = sum_b Q[b][j] X[b][k], j < n_out, k < K: X and out are rows of K contiguous complex entries (the block's
// columns), Q is n_in x n_out, row-major.  A tall, skinny complex product on v_mfma_f64_16x16x4_f64 with the operand
// map corr_gram documents: the matrix rows are the output columns j (A[row j][b] = Q[b][j]), the matrix columns are
// k (B[b][col k] = X[b][k]), the sum runs over b.  Lane l (i = l & 15, kk = l >> 4) supplies A[row i][b = kk] and
// B[b = kk][col i] and receives D[row kk + 4 reg][col i].  (q x) = (qr xr - qi xi) + i (qr xi + qi xr): four real
// products into two accumulators per tile.
// Grid (ceil(K / 64), ceil(n_out / 64)), 256 threads: a workgroup owns 64 output columns and 64 k, a wave 16 of
// those k and all 64 columns (4 tiles).  Q enters through LDS, kRotChunk rows of the workgroup's 64 columns at a time,
// staged once per workgroup ([b][j] image with rows of 65 entries, as in corr_gram); X is read straight from memory,
// 16 lanes on 16 consecutive k of one column (256 contiguous bytes), once per workgroup; the store is the same shape.
// Rows b >= n_in, columns j >= n_out and k >= K are never read or written: they enter as zero.
constexpr int kRotTile = 64;   // output columns, and k, per workgroup
constexpr int kRotChunk = 32;  // rows of Q per LDS stage
constexpr int kRotLd = kRotTile + 1;

__global__ __launch_bounds__(256) void subspace_rotate(const double2* __restrict__ x, const double2* __restrict__ q,
                                                       double2* __restrict__ out, int n_in, int n_out, int64_t K) {
    __shared__ double2 qs[kRotChunk * kRotLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kk = lane >> 4;
    const int j0 = blockIdx.y * kRotTile;
    const int64_t k = (int64_t)blockIdx.x * kRotTile + wave * 16 + i;
    const bool k_valid = k < K;
    const int sj = threadIdx.x & 63, sb = threadIdx.x >> 6;  // staging: this thread's column and its first row

    v4f64 pr[4], pi[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        pr[a] = v4f64{0.0, 0.0, 0.0, 0.0};
        pi[a] = v4f64{0.0, 0.0, 0.0, 0.0};
    }

    for (int b0 = 0; b0 < n_in; b0 += kRotChunk) {
        // this chunk's entries of X first: they are in flight while Q is staged
        double2 xv[kRotChunk / 4];
#pragma unroll
        for (int u = 0; u < kRotChunk / 4; ++u) {
            const int b = b0 + 4 * u + kk;
            xv[u] = make_double2(0.0, 0.0);
            if (b < n_in && k_valid) xv[u] = x[(size_t)b * K + k];
        }
        __syncthreads();  // (the stage before has been read)
#pragma unroll
        for (int u = 0; u < kRotChunk / 4; ++u) {
            const int bb = sb + 4 * u;
            double2 v = make_double2(0.0, 0.0);
            if (b0 + bb < n_in && j0 + sj < n_out) v = q[(size_t)(b0 + bb) * n_out + j0 + sj];
            qs[bb * kRotLd + sj] = v;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kRotChunk / 4; ++u) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const double2 qa = qs[(4 * u + kk) * kRotLd + 16 * a + i];
                pr[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, xv[u].x, pr[a], 0, 0, 0);
                pr[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(-qa.y, xv[u].y, pr[a], 0, 0, 0);
                pi[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, xv[u].y, pi[a], 0, 0, 0);
                pi[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.y, xv[u].x, pi[a], 0, 0, 0);
            }
        }
    }

    if (!k_valid) return;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int j = j0 + 16 * a + kk + 4 * reg;
            if (j < n_out) out[(size_t)j * K + k] = make_double2(pr[a][reg], pi[a][reg]);
        }
}

// part[w][j] = sum over the k of workgroup w of |HX[j][k] - theta[j] X[j][k]|^2.  Grid (kResidualGrid, n_out), 256
// threads: workgroup w takes the k-range [w, w + 1) * ceil(K / grid) of column j, a thread every 256th entry of it in
// ascending order, and the 256 sums meet in a fixed tree.
constexpr int kResidualGrid = 64;

__global__ __launch_bounds__(256) void subspace_residual(const double2* __restrict__ x, const double2* __restrict__ hx,
                                                         const double* __restrict__ theta, int64_t K,
                                                         double* __restrict__ part) {
    __shared__ double sums[256];
    const int j = blockIdx.y;
    const int64_t span = (K + gridDim.x - 1) / gridDim.x;
    const int64_t k_lo = (int64_t)blockIdx.x * span, k_hi = min(K, k_lo + span);
    const double th = theta[j];
    const double2* xj = x + (size_t)j * K;
    const double2* hj = hx + (size_t)j * K;
    double acc = 0.0;
    for (int64_t k = k_lo + threadIdx.x; k < k_hi; k += 256) {
        const double2 a = xj[k], h = hj[k];
        const double re = fma(-th, a.x, h.x), im = fma(-th, a.y, h.y);
        acc = fma(re, re, acc);
        acc = fma(im, im, acc);
    }
    sums[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) sums[threadIdx.x] += sums[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * gridDim.y + j] = sums[0];
}

// res[j] = sqrt(sum_w part[w][j]), w ascending: one thread per column.
__global__ void subspace_residual_reduce(const double* __restrict__ part, int n_parts, int n_out, double* __restrict__ res) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    double total = 0.0;
    for (int w = 0; w < n_parts; ++w) total += part[(size_t)w * n_out + j];
    res[j] = sqrt(total);
}

}  // namespace bdg

namespace {

constexpr int kSubspaceMaxColumns = 4096;

struct SubspaceState {
    int cols = 0;
    DeviceBuffer<double2> array[3];  // X, HX and the target of a rotation, in the roles below
    double2 *x = nullptr, *hx = nullptr, *spare = nullptr;
    DeviceBuffer<double2> part, gram, q;
    DeviceBuffer<double> theta, res_part, res;
};

void subspace_free(bdg_system* sys) {
    SubspaceState* sp = static_cast<SubspaceState*>(sys->subspace);
    if (!sp) return;
    if (sys->stream) (void)hipStreamSynchronize(sys->stream);
    for (auto& side : sys->side_sets)
        if (side->stream) (void)hipStreamSynchronize(side->stream);
    for (auto& buf : sp->array) buf.release();
    sp->part.release();
    sp->gram.release();
    sp->q.release();
    sp->theta.release();
    sp->res_part.release();
    sp->res.release();
    delete sp;
    sys->subspace = nullptr;
}

// The handle's block, or nullptr with the error set
SubspaceState* subspace_of(bdg_system* sys, const char* call) {
    if (!sys) {
        fail(BDG_EINVAL, "null system handle");
        return nullptr;
    }
    SubspaceState* sp = static_cast<SubspaceState*>(sys->subspace);
    if (!sp)
        fail(BDG_EINVAL, "%s: no subspace block on this handle (bdg_subspace_begin has not been called, or a dense solve or "
             "a Lanczos run has ended it)", call);
    return sp;
}

int subspace_check_columns(const SubspaceState* sp, const char* call, int first, int count) {
    if (first < 0 || count < 1 || (int64_t)first + count > sp->cols)
        return fail(BDG_EINVAL, "%s: columns [%d, %d) are not within the block's %d", call, first, first + count, sp->cols);
    return BDG_OK;
}

int subspace_begin(bdg_system* sys, int n_columns, uint64_t seed, uint64_t first_vec_id) {
    if (n_columns < 1 || n_columns > kSubspaceMaxColumns)
        return fail(BDG_EINVAL, "bdg_subspace_begin: n_columns must lie in [1, %d]", kSubspaceMaxColumns);
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_subspace_begin needs a whole (square) matrix: slabs are not supported");
    HIP_TRY(hipSetDevice(sys->device));
    lanczos_free(sys);
    subspace_free(sys);
    const int64_t K = 4 * sys->nb;
    const int64_t n_slices = (K + kCorrelationSlice - 1) / kCorrelationSlice;
    if (n_slices > 65535) return fail(BDG_EINVAL, "bdg_subspace_begin: the matrix is too large for the Gram product's slices");
    SubspaceState* sp = new SubspaceState();
    sp->cols = n_columns;
    sys->subspace = sp;  // (subspace_free gives back whatever the steps below obtained)
    const size_t count = (size_t)K * n_columns;
    auto body = [&]() -> int {
        for (auto& buf : sp->array)
            if (int rc = buf.reserve(count)) return rc;
        if (int rc = sp->part.reserve((size_t)n_slices * n_columns * n_columns)) return rc;
        if (int rc = sp->gram.reserve((size_t)2 * n_columns * n_columns)) return rc;
        if (int rc = sp->q.reserve((size_t)n_columns * n_columns)) return rc;
        if (int rc = sp->theta.reserve((size_t)n_columns)) return rc;
        if (int rc = sp->res_part.reserve((size_t)bdg::kResidualGrid * n_columns)) return rc;
        if (int rc = sp->res.reserve((size_t)n_columns)) return rc;
        sp->x = sp->array[0].ptr;
        sp->hx = sp->array[1].ptr;
        sp->spare = sp->array[2].ptr;
        const int grid = (int)std::min<size_t>(4096, (count + 255) / 256);
        bdg::subspace_fill<<<grid, 256, 0, sys->stream>>>(sp->x, K, n_columns, seed, first_vec_id);
        bdg::fill_zero<<<grid, 256, 0, sys->stream>>>(sp->hx, (int64_t)count);
        bdg::fill_zero<<<grid, 256, 0, sys->stream>>>(sp->spare, (int64_t)count);  // (dead columns stay finite)
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(sys->stream));
        return BDG_OK;
    };
    const int rc = body();
    if (rc) {
        const std::string message = g_error;
        subspace_free(sys);
        g_error = message;
    }
    return rc;
}

int subspace_refill(bdg_system* sys, int first_column, int count, uint64_t seed, uint64_t first_vec_id) {
    SubspaceState* sp = subspace_of(sys, "bdg_subspace_refill");
    if (!sp) return BDG_EINVAL;
    if (int rc = subspace_check_columns(sp, "bdg_subspace_refill", first_column, count)) return rc;
    HIP_TRY(hipSetDevice(sys->device));
    const int64_t K = 4 * sys->nb;
    const size_t total = (size_t)K * count;
    const int grid = (int)std::min<size_t>(4096, (total + 255) / 256);
    bdg::subspace_fill<<<grid, 256, 0, sys->stream>>>(sp->x + (size_t)K * first_column, K, count, seed, first_vec_id);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sys->stream));
    return BDG_OK;
}

// Columns of X to the host (`out`) or from it (`in`): exactly one of the two is given
int subspace_copy(bdg_system* sys, int first_column, int count, const double* in, double* out) {
    const char* call = in ? "bdg_subspace_write" : "bdg_subspace_read";
    if (!in && !out) return fail(BDG_EINVAL, "null argument");
    SubspaceState* sp = subspace_of(sys, call);
    if (!sp) return BDG_EINVAL;
    if (int rc = subspace_check_columns(sp, call, first_column, count)) return rc;
    HIP_TRY(hipSetDevice(sys->device));
    const size_t K = (size_t)4 * sys->nb;
    double2* at = sp->x + K * first_column;
    const size_t bytes = sizeof(double2) * K * (size_t)count;
    if (in) HIP_TRY(hipMemcpyAsync(at, in, bytes, hipMemcpyHostToDevice, sys->stream));
    else HIP_TRY(hipMemcpyAsync(out, at, bytes, hipMemcpyDeviceToHost, sys->stream));
    HIP_TRY(hipStreamSynchronize(sys->stream));
    return BDG_OK;
}

int subspace_filter(bdg_system* sys, double scale, int n_moments, const double* coef) {
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (!coef) return fail(BDG_EINVAL, "null argument");
    SubspaceState* sp = subspace_of(sys, "bdg_subspace_filter");
    if (!sp) return BDG_EINVAL;
    HIP_TRY(hipSetDevice(sys->device));
    std::vector<double> complex_coef((size_t)2 * n_moments, 0.0);
    for (int k = 0; k < n_moments; ++k) complex_coef[(size_t)2 * k] = coef[k];
    double* block = reinterpret_cast<double*>(sp->x);
    return apply_series_batches(sys, scale, n_moments, 1, complex_coef.data(), sp->cols, block, block, true, true);
}

int subspace_project(bdg_system* sys, double* s_out, double* g_out) {
    if (!s_out || !g_out) return fail(BDG_EINVAL, "null argument");
    SubspaceState* sp = subspace_of(sys, "bdg_subspace_project");
    if (!sp) return BDG_EINVAL;
    HIP_TRY(hipSetDevice(sys->device));
    // HX = H X: the series 0 T_0 + 1 T_1 at scale 1 - the source enters zeroed buffers, then one step of H
    const double h_coef[4] = {0.0, 0.0, 1.0, 0.0};
    if (int rc = apply_series_batches(sys, 1.0, 2, 1, h_coef, sp->cols, reinterpret_cast<const double*>(sp->x),
                                      reinterpret_cast<double*>(sp->hx), true, false))
        return rc;
    const int B = sp->cols;
    const int64_t K = 4 * sys->nb;
    const int64_t n_slices = (K + kCorrelationSlice - 1) / kCorrelationSlice;
    const size_t entries = (size_t)B * B;
    hipStream_t st = sys->stream;
    HIP_TRY(hipMemsetAsync(sp->gram.ptr, 0, sizeof(double2) * 2 * entries, st));
    const unsigned tiles = (unsigned)((B + bdg::kCorrTile - 1) / bdg::kCorrTile);
    const dim3 grid(tiles, tiles, (unsigned)n_slices);
    const int red_grid = (int)std::min<size_t>(4096, (entries + 255) / 256);
    const double2* right[2] = {sp->x, sp->hx};
    for (int m = 0; m < 2; ++m) {  // S = X^† X, then G = X^† HX (the partials are reused: same stream)
        bdg::corr_gram<<<grid, 256, 0, st>>>(sp->x, right[m], B, B, K, kCorrelationSlice, sp->part.ptr);
        bdg::corr_reduce<<<red_grid, 256, 0, st>>>(sp->part.ptr, (int)n_slices, B, B, sp->gram.ptr + (size_t)m * entries, B, 0, 0);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s_out, sp->gram.ptr, sizeof(double2) * entries, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g_out, sp->gram.ptr + entries, sizeof(double2) * entries, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BDG_OK;
}

int subspace_rotate_block(bdg_system* sys, int n_out, const double* q, const double* theta, double* residual_out) {
    if (!q || !theta || !residual_out) return fail(BDG_EINVAL, "null argument");
    SubspaceState* sp = subspace_of(sys, "bdg_subspace_rotate");
    if (!sp) return BDG_EINVAL;
    if (n_out < 1 || n_out > sp->cols)
        return fail(BDG_EINVAL, "bdg_subspace_rotate: n_out must lie in [1, %d], the block's columns", sp->cols);
    HIP_TRY(hipSetDevice(sys->device));
    const int B = sp->cols;
    const int64_t K = 4 * sys->nb;
    hipStream_t st = sys->stream;
    HIP_TRY(hipMemcpyAsync(sp->q.ptr, q, sizeof(double2) * (size_t)B * n_out, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sp->theta.ptr, theta, sizeof(double) * (size_t)n_out, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((K + bdg::kRotTile - 1) / bdg::kRotTile), (unsigned)((n_out + bdg::kRotTile - 1) / bdg::kRotTile));
    bdg::subspace_rotate<<<grid, 256, 0, st>>>(sp->x, sp->q.ptr, sp->spare, B, n_out, K);
    std::swap(sp->x, sp->spare);
    bdg::subspace_rotate<<<grid, 256, 0, st>>>(sp->hx, sp->q.ptr, sp->spare, B, n_out, K);
    std::swap(sp->hx, sp->spare);
    const dim3 res_grid((unsigned)bdg::kResidualGrid, (unsigned)n_out);
    bdg::subspace_residual<<<res_grid, 256, 0, st>>>(sp->x, sp->hx, sp->theta.ptr, K, sp->res_part.ptr);
    bdg::subspace_residual_reduce<<<(n_out + 255) / 256, 256, 0, st>>>(sp->res_part.ptr, bdg::kResidualGrid, n_out, sp->res.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(residual_out, sp->res.ptr, sizeof(double) * (size_t)n_out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BDG_OK;
}

}  // namespace
