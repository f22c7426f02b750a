// response_map.hpp - one operator's response at every site: the 4x4 blocks
//     K_{q,j}[g, d] = sum_nm c_q[n][m] sum_ab A[a, b] conj(X_m[(j, g), b]) X_n[(j, d), a],   X_n = T_n(H~) E
// for the unit columns E on the support of A (bdg_response_map).  Part of the single translation unit bodge_hip.hip
// (included after correlation.hpp): the kernels live in namespace bdg, the driver in the unnamed namespace beside
// run_moment_matrix (correlation.hpp).
//
// One recurrence of S <= 32 columns, one dense product, one contraction.  The columns advance through
// the stored-source Clenshaw kernels of apply.hpp with a zero coefficient (a plain step 2 H~ t_n - t_{n-1}), as in
// run_moment_matrix; after every step resp_pick gathers the rows of a chunk of target sites from t_n into row n of
// the X panel, site-major: entry ((s 4 + component) Sp + column) of a row of K = 4 Sp sites complex entries, Sp the
// columns padded to whole batches.  The hot path is Z_q = c_q^T X, (M x M) (M x K), on the fp64 matrix cores
// (resp_gemm); resp_contract then sums a site's 16 entries over m and the columns.
//
// Summation order of one entry of K: n ascending inside Z (four n per MFMA, the MFMAs in order), then m ascending,
// and inside one m the columns b ascending with a ascending inside.  It depends on M and S alone - not on the chunk
// of sites an entry falls into, not on its place in the chunk - and no atomic is used.
#pragma once

namespace bdg {

// X[n][((s 4 + component) Sp + col0 + r)] = t_n[component][site_s][r] for the sites s of a chunk, r < rl: one thread
// per entry.  Columns beyond the active ones of a batch are zero in t_n (they started as zero columns).
__global__ void resp_pick(const double2* __restrict__ t, const int* __restrict__ sites, int n_chunk, int64_t nb, int rl,
                          int Sp, int col0, double2* __restrict__ row) {
    const int64_t total = (int64_t)n_chunk * 4 * rl;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx % rl);
        const int64_t pair = idx / rl;  // s 4 + component
        row[pair * Sp + col0 + r] = t[vslot((int)(pair & 3), (size_t)sites[pair >> 2], r, (size_t)nb, rl)];
    }
}

// Z[m][k] = sum_n c[n][m] X[n][k], m < M, k < K: c is M x M row-major, X and Z are rows of K contiguous complex
// entries.  On v_mfma_f64_16x16x4_f64 with the operand map corr_gram documents: the matrix rows are m
// (A[row m][n] = c[n][m]), the matrix columns are k (B[n][col k] = X[n][k]), the sum runs over n.  Lane l (i = l & 15,
// kk = l >> 4) supplies A[row i][n = kk] and B[n = kk][col i] and receives D[row kk + 4 reg][col i], reg < 4.
// (c x) = (cr xr - ci xi) + i (cr xi + ci xr): four real products into two accumulators per tile.
// Grid (ceil(K / 64), ceil(M / 64)); 256 threads per 64 x 64 tile of Z, one wave per 32 x 32 sub-tile as 2 x 2 MFMA
// tiles.  Both operands are staged through LDS in steps of 16 n: [n][m] and [n][k] images with rows of 65 entries (a
// 16-lane group of a 16-byte read covers 16 consecutive slots), written as they lie in memory (64 consecutive m or k
// of one n per wave), the next step's entries fetched into registers meanwhile.  n >= M, m >= M and k >= K are never
// read or written: they enter as zero.  n ascends.
constexpr int kRespTile = 64;   // m, and k, per workgroup
constexpr int kRespStepN = 16;  // n per LDS stage
constexpr int kRespLd = kRespTile + 1;

__device__ __forceinline__ void resp_fetch(const double2* __restrict__ src, int rows, int64_t ld, int n, int64_t col,
                                           double2 (&v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int row = n + 4 * u;
        v[u] = make_double2(0.0, 0.0);
        if (row < rows && col < ld) v[u] = src[(size_t)row * ld + col];
    }
}

__global__ __launch_bounds__(256, 2) void resp_gemm(const double2* __restrict__ c, const double2* __restrict__ xp, int M,
                                                    int64_t K, double2* __restrict__ zp) {
    __shared__ double2 cs[kRespStepN * kRespLd];
    __shared__ double2 xs[kRespStepN * kRespLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kk = lane >> 4;
    const int m0 = blockIdx.y * kRespTile;
    const int64_t k0 = (int64_t)blockIdx.x * kRespTile;
    const int wm = (wave >> 1) * 32, wk = (wave & 1) * 32;
    const int sc = threadIdx.x & 63, sn = threadIdx.x >> 6;  // staging: this thread's m or k and its first n

    v4f64 pr[2][2], pi[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            pr[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
            pi[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
        }

    double2 gc[4], gx[4];
    resp_fetch(c, M, M, sn, m0 + sc, gc);
    resp_fetch(xp, M, K, sn, k0 + sc, gx);
    for (int n0 = 0; n0 < M; n0 += kRespStepN) {
        __syncthreads();  // (the stage before has been read)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cs[(sn + 4 * u) * kRespLd + sc] = gc[u];
            xs[(sn + 4 * u) * kRespLd + sc] = gx[u];
        }
        __syncthreads();
        if (n0 + kRespStepN < M) {
            resp_fetch(c, M, M, n0 + kRespStepN + sn, m0 + sc, gc);
            resp_fetch(xp, M, K, n0 + kRespStepN + sn, k0 + sc, gx);
        }
#pragma unroll
        for (int ns = 0; ns < kRespStepN; ns += 4) {
            double2 ca[2], xb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                ca[a] = cs[(ns + kk) * kRespLd + wm + 16 * a + i];
                xb[a] = xs[(ns + kk) * kRespLd + wk + 16 * a + i];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    pr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[a].x, xb[b].x, pr[a][b], 0, 0, 0);
                    pr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ca[a].y, xb[b].y, pr[a][b], 0, 0, 0);
                    pi[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[a].x, xb[b].y, pi[a][b], 0, 0, 0);
                    pi[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[a].y, xb[b].x, pi[a][b], 0, 0, 0);
                }
        }
    }

#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int m = m0 + wm + 16 * a + kk + 4 * reg;
                const int64_t k = k0 + wk + 16 * b + i;
                if (m < M && k < K) zp[(size_t)m * K + k] = make_double2(pr[a][b][reg], pi[a][b][reg]);
            }
}

// out[(s 4 + g) 4 + d] = sum_m sum_b conj(X[m][(s, g), b]) (sum_a Z[m][(s, d), a] A[a][b]), a, b < S: one thread per
// entry, m ascending, b ascending, a ascending inside; A is S x S row-major.  No atomics, one writer per entry.
__global__ void resp_contract(const double2* __restrict__ xp, const double2* __restrict__ zp, const double2* __restrict__ amat,
                              int M, int64_t K, int Sp, int S, int n_chunk, double2* __restrict__ out) {
    const int64_t total = (int64_t)n_chunk * 16;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = idx >> 4;
        const int g = (int)(idx >> 2) & 3, d = (int)idx & 3;
        const double2* xr = xp + (s * 4 + g) * Sp;
        const double2* zr = zp + (s * 4 + d) * Sp;
        double re = 0.0, im = 0.0;
        for (int m = 0; m < M; ++m, xr += K, zr += K)
            for (int b = 0; b < S; ++b) {
                double wr = 0.0, wi = 0.0;
                for (int a = 0; a < S; ++a) {
                    const double2 z = zr[a], h = amat[a * S + b];
                    wr = fma(z.x, h.x, wr);
                    wr = fma(-z.y, h.y, wr);
                    wi = fma(z.x, h.y, wi);
                    wi = fma(z.y, h.x, wi);
                }
                const double2 x = xr[b];  // conj(x) w = (xr wr + xi wi) + i (xr wi - xi wr)
                re = fma(x.x, wr, re);
                re = fma(x.y, wi, re);
                im = fma(x.x, wi, im);
                im = fma(-x.y, wr, im);
            }
        out[idx] = make_double2(re, im);
    }
}

}  // namespace bdg

namespace {

constexpr int kResponseMaxRows = 32;    // scalar rows on the support of A
constexpr int kResponseSiteStep = 16;   // a chunk of target sites is a multiple of this (or all of them)

int run_response_map(bdg_system* sys, double scale, int n_moments, int n_source_rows, const int64_t* source_rows,
                     const double* a, int n_kernels, const double* coef, int n_sites, const int32_t* block_rows,
                     double* out) {
    // (argument errors first, in the order of the header; none of them needs a GPU)
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_source_rows < 1) return fail(BDG_EINVAL, "n_source_rows must be >= 1");
    if (n_kernels < 1) return fail(BDG_EINVAL, "n_kernels must be >= 1");
    if (n_sites < 1) return fail(BDG_EINVAL, "n_sites must be >= 1");
    if (n_source_rows > kResponseMaxRows)
        return fail(BDG_EINVAL, "n_source_rows = %d: the support of A is limited to %d scalar rows", n_source_rows, kResponseMaxRows);
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (!source_rows || !a || !coef || !block_rows || !out) return fail(BDG_EINVAL, "null argument");
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    const int64_t nb = sys->nb;
    for (int v = 0; v < n_source_rows; ++v) {
        if (source_rows[v] < 0 || source_rows[v] >= 4 * nb)
            return fail(BDG_EINVAL, "source row %lld out of range", (long long)source_rows[v]);
        for (int u = 0; u < v; ++u)
            if (source_rows[u] == source_rows[v]) return fail(BDG_EINVAL, "source row %lld listed twice", (long long)source_rows[v]);
    }
    {
        std::vector<uint8_t> seen((size_t)std::max<int64_t>(nb, 0), 0);
        for (int s = 0; s < n_sites; ++s) {
            if (block_rows[s] < 0 || block_rows[s] >= nb) return fail(BDG_EINVAL, "block row %d out of range", block_rows[s]);
            if (seen[(size_t)block_rows[s]]++) return fail(BDG_EINVAL, "block row %d listed twice", block_rows[s]);
        }
    }
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_response_map needs a whole (square) matrix: slabs are not supported");
    lanczos_free(sys);
    subspace_free(sys);
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic mode of the family, lanes by its column rule (family.hpp); the S columns fill whole batches of rl lanes.
    const ModeInfo mode = family_mode(sys);
    const int rl = family_column_lanes(sys, mode, n_source_rows);
    const int n_batches = (n_source_rows + rl - 1) / rl;
    const int Sp = n_batches * rl;  // padded columns of a site's entries in a panel row
    const int M = n_moments;

    // Chunks of target sites: all of them, or the largest multiple of 16 for which X and Z stay within the budget.
    size_t budget = kCorrelationBytes;
    if (const char* env = knob::raw("BODGE_AMD_CORRELATION_BYTES")) budget = (size_t)std::max(1LL, atoll(env));
    const size_t site_bytes = (size_t)2 * M * 4 * Sp * sizeof(double2);  // one site in both panels
    int chunk = n_sites;
    if ((size_t)n_sites * site_bytes > budget) {
        const size_t fit = budget / site_bytes / kResponseSiteStep * kResponseSiteStep;
        if (fit == 0)
            return fail(BDG_EINVAL,
                        "bdg_response_map: two panels of %d rows for %d sites at %d columns need %zu bytes, "
                        "BODGE_AMD_CORRELATION_BYTES allows %zu",
                        M, std::min(n_sites, kResponseSiteStep), Sp, (size_t)std::min(n_sites, kResponseSiteStep) * site_bytes, budget);
        chunk = (int)std::min<size_t>(fit, (size_t)n_sites);
    }
    const int n_chunks = (n_sites + chunk - 1) / chunk;
    const int64_t K_max = (int64_t)chunk * 4 * Sp;
    if ((K_max + bdg::kRespTile - 1) / bdg::kRespTile > 0x7fffffffLL)
        return fail(BDG_EINVAL, "bdg_response_map: a chunk of %d sites is too wide for one launch", chunk);

    FamilySetup<ApplyKernels> fs;
    if (int rc = family_setup(sys, mode, rl, 0, &fs)) return rc;
    const StepPlan& plan = fs.plan.step;
    const size_t vec_count = fs.vec_count;

    DeviceBuffer<double2> d_start, d_xa, d_xb, d_xpanel, d_zpanel, d_coef, d_a, d_out, d_zero;
    DeviceBuffer<int64_t> d_rows;
    DeviceBuffer<int> d_sites;
    std::vector<hipEvent_t> events;  // (start, stop) per product, then the window's two
    auto body = [&]() -> int {
        hipStream_t st = sys->stream;
        for (DeviceBuffer<double2>* buf : {&d_start, &d_xa, &d_xb})
            if (int rc = buf->reserve(vec_count)) return rc;
        if (int rc = d_xpanel.reserve((size_t)M * K_max)) return rc;
        if (int rc = d_zpanel.reserve((size_t)M * K_max)) return rc;
        if (int rc = d_coef.reserve((size_t)n_kernels * M * M)) return rc;
        if (int rc = d_a.reserve((size_t)n_source_rows * n_source_rows)) return rc;
        if (int rc = d_out.reserve((size_t)n_kernels * n_sites * 16)) return rc;
        if (int rc = d_zero.reserve(1)) return rc;
        if (int rc = d_rows.reserve((size_t)n_source_rows)) return rc;
        if (int rc = d_sites.reserve((size_t)n_sites)) return rc;
        HIP_TRY(hipMemcpyAsync(d_rows.ptr, source_rows, sizeof(int64_t) * (size_t)n_source_rows, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_sites.ptr, block_rows, sizeof(int) * (size_t)n_sites, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_coef.ptr, coef, sizeof(double2) * (size_t)n_kernels * M * M, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_a.ptr, a, sizeof(double2) * (size_t)n_source_rows * n_source_rows, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_zero.ptr, 0, sizeof(double2), st));  // the coefficient of the source: a plain step
        events.assign((size_t)2 * n_chunks * n_kernels + 2, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        const int fill_grid = (int)std::min<size_t>(4096, (vec_count + 255) / 256);
        bdg_perf perf{};
        size_t ev = 0;
        HIP_TRY(hipEventRecord(events[events.size() - 2], st));
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int s0 = ch * chunk, cs = std::min(chunk, n_sites - s0);
            const int64_t K = (int64_t)cs * 4 * Sp;
            const int pick_grid = (int)std::min<int64_t>(4096, ((int64_t)cs * 4 * rl + 255) / 256);
            // every chunk reruns the recurrence from the start columns, batch after batch
            for (int bt = 0; bt < n_batches; ++bt) {
                const int col_base = bt * rl;
                const int n_active = std::min(rl, n_source_rows - col_base);
                bdg::fill_zero<<<fill_grid, 256, 0, st>>>(d_start.ptr, (int64_t)vec_count);
                bdg::set_unit<<<1, 64, 0, st>>>(d_start.ptr, nb, nb, rl, n_active, d_rows.ptr + col_base, (int64_t)0);
                double2* cur = d_xa.ptr;
                double2* prev = d_xb.ptr;
                HIP_TRY(hipMemcpyAsync(cur, d_start.ptr, sizeof(double2) * vec_count, hipMemcpyDeviceToDevice, st));
                bdg::fill_zero<<<fill_grid, 256, 0, st>>>(prev, (int64_t)vec_count);
                bdg::ApplyArgs ca{};
                ca.s = fs.base;
                ca.x = d_start.ptr;
                ca.n_functions = 1;
                ca.col_base = 0;
                ca.n_active = n_active;
                ca.coef_row = d_zero.ptr;
                int64_t launches = 0;
                for (int n = 0; n < M; ++n) {
                    if (n > 0) {  // prev <- coef H cur - prev + 0 x
                        ca.s.cur = cur;
                        ca.s.prev = prev;
                        ca.s.coef = (n == 1 ? 1.0 : 2.0) / scale;
                        ca.s.reverse = fs.alternate ? (n & 1) : 0;
                        fs.plan.kernel<<<plan.grid, bdg::kBlockThreads, plan.lds_bytes, st>>>(ca);
                        std::swap(cur, prev);
                        ++launches;
                    }
                    bdg::resp_pick<<<pick_grid, 256, 0, st>>>(cur, d_sites.ptr + s0, cs, nb, rl, Sp, col_base,
                                                              d_xpanel.ptr + (size_t)n * K);
                }
                HIP_TRY(hipGetLastError());
                perf.launches += launches;
                perf.vector_steps += launches * n_active;
            }
            const dim3 grid((unsigned)((K + bdg::kRespTile - 1) / bdg::kRespTile), (unsigned)((M + bdg::kRespTile - 1) / bdg::kRespTile));
            const int con_grid = (int)std::min<int64_t>(4096, ((int64_t)cs * 16 + 255) / 256);
            for (int q = 0; q < n_kernels; ++q) {
                HIP_TRY(hipEventRecord(events[ev], st));
                bdg::resp_gemm<<<grid, 256, 0, st>>>(d_coef.ptr + (size_t)q * M * M, d_xpanel.ptr, M, K, d_zpanel.ptr);
                HIP_TRY(hipEventRecord(events[ev + 1], st));
                ev += 2;
                bdg::resp_contract<<<con_grid, 256, 0, st>>>(d_xpanel.ptr, d_zpanel.ptr, d_a.ptr, M, K, Sp, n_source_rows, cs,
                                                             d_out.ptr + ((size_t)q * n_sites + s0) * 16);
                perf.gemm_flops += 8.0 * M * M * (double)K;
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(events[events.size() - 1], st));
        HIP_TRY(hipMemcpyAsync(out, d_out.ptr, sizeof(double2) * (size_t)n_kernels * n_sites * 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t e = 0; e + 2 < events.size(); e += 2) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, events[e], events[e + 1]));
            perf.gemm_ms += t;
        }
        float window = 0.f;
        HIP_TRY(hipEventElapsedTime(&window, events[events.size() - 2], events[events.size() - 1]));
        perf.window_ms = window;
        perf.kernel_ms = window;
        perf.bytes_per_launch = apply_bytes(sys, fs.rv, mode, plan.dictionary, 1);
        perf.bytes_moved = perf.bytes_per_launch * (double)perf.launches;
        family_perf(sys, plan, fs.rv, fs.strip_rows, 1, &perf);
        perf.response_map = 1;
        sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(sys->stream);
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    for (DeviceBuffer<double2>* buf : {&d_start, &d_xa, &d_xb, &d_xpanel, &d_zpanel, &d_coef, &d_a, &d_out, &d_zero})
        buf->release();
    d_rows.release();
    d_sites.release();
    return rc;
}

}  // namespace
