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

// Generic form: cheb_clenshaw's tile loop (LDS staging of the streamed blocks, gathers of t_n) with the
// epilogue t_{n+1} = coef * (H t_n) - t_{n-1} and the store of the target rows.
template <typename Mode, int RL>
__global__ __launch_bounds__(kBlockThreads, 4) void cheb_green(GreenArgs ga) {
    extern __shared__ double2 lds[];
    const StepArgs& a = ga.s;
    constexpr int RW = kWave / RL;
    constexpr int SPB = Mode::kSlotsPerBlock;
    constexpr int STRIDE = Mode::kBlockStride;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int s = lane / RL;
    const int r = lane % RL;
    const int region = a.stage_blocks * STRIDE;
    double2* stage = lds + wave * region;
    const double2* all_blocks = static_cast<const double2*>(a.blocks);

    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int slots = gridDim.x >> 3;
    const int t_lo = (int)(((int64_t)a.n_tiles * xcd) >> 3);
    const int t_hi = (int)(((int64_t)a.n_tiles * (xcd + 1)) >> 3);

    for (int t = t_lo + slot; t < t_hi; t += slots) {
        const int tt = a.reverse ? t_lo + t_hi - 1 - t : t;
        const int tile = a.tile_order ? a.tile_order[tt] : tt + a.tile_base;
        const int row0 = (tile * kWavesPerBlock + wave) * RW;
        if (row0 >= a.nb) continue;
        const int row_end = min(row0 + RW, a.nb);
        const int kb0 = a.indptr[row0];
        const int kb1 = a.indptr[row_end];

        const int i = row0 + s;
        const bool valid = i < a.nb;
        int kbeg = 0, kend = 0;
        if (valid) {
            kbeg = a.indptr[i];
            kend = a.indptr[i + 1];
        }
        double2 acc[4];
#pragma unroll
        for (int al = 0; al < 4; ++al) acc[al] = make_double2(0.0, 0.0);

        for (int c0 = kb0; c0 < kb1; c0 += a.stage_blocks) {
            const int c1 = min(c0 + a.stage_blocks, kb1);
            const int n_el = (c1 - c0) * SPB;
            const double2* src = all_blocks + (size_t)c0 * SPB;
            for (int e0 = 0; e0 < n_el; e0 += 4 * kWave) {
                double2 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kWave + lane;
                    if (e < n_el) v[u] = load_stream(src + e);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kWave + lane;
                    if (e < n_el) stage[(e / SPB) * STRIDE + (e % SPB)] = v[u];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

            const int k0 = max(kbeg, c0), k1 = min(kend, c1);
            double2 x[4], xn[4];
            if (k0 < k1) {
                const size_t j = (size_t)a.indices[k0];
#pragma unroll
                for (int be = 0; be < 4; ++be) xn[be] = a.cur[vslot(be, j, r, a.ncols, RL)];
            }
            for (int k = k0; k < k1; ++k) {
#pragma unroll
                for (int be = 0; be < 4; ++be) x[be] = xn[be];
                if (k + 1 < k1) {
                    const size_t j = (size_t)a.indices[k + 1];
#pragma unroll
                    for (int be = 0; be < 4; ++be) xn[be] = a.cur[vslot(be, j, r, a.ncols, RL)];
                }
                Mode::mac_row(acc, stage + (k - c0) * STRIDE, x);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }

        if (valid) {
            // (read here, not before the tile loop: one live register less across it keeps ComplexPHMode out of scratch)
            const int target = ga.target_slot[i];
            double2 nx[4];
#pragma unroll
            for (int al = 0; al < 4; ++al) {
                const size_t own = vslot(al, (size_t)i, r, a.ncols, RL);
                const double2 p = (a.stream_vectors & 1) ? load_stream(a.prev + own) : a.prev[own];
                nx[al].x = fma(a.coef, acc[al].x, -p.x);
                nx[al].y = fma(a.coef, acc[al].y, -p.y);
            }
#pragma unroll
            for (int al = 0; al < 4; ++al) {
                const size_t own = vslot(al, (size_t)i, r, a.ncols, RL);
                if (a.stream_vectors & 2) store_stream(a.prev + own, nx[al]);
                else a.prev[own] = nx[al];
            }
            store_picked<Mode::kVec>(ga, target, r, nx);
        }
    }
}

// Dictionary form: cheb_clenshaw_dict's tile loop (block table in LDS, fixed-width row words, own and
// neighbouring rows of t_n shared through LDS) with the same epilogue.
template <typename Mode, int RL, int MAXB>
__global__ __launch_bounds__(kBlockThreads, 4) void cheb_green_dict(GreenArgs ga) {
    extern __shared__ double2 lds[];
    const StepArgs& a = ga.s;
    constexpr int RW = kWave / RL;
    constexpr int SPB = Mode::kSlotsPerBlock;
    constexpr int STRIDE = Mode::kBlockStride;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int s = lane / RL;
    const int r = lane % RL;

    const double2* table = static_cast<const double2*>(a.dict_table);
    for (int e = threadIdx.x; e < a.n_unique * SPB; e += kBlockThreads)
        lds[(e / SPB) * STRIDE + (e % SPB)] = table[e];
    double2* share = lds + a.n_unique * STRIDE + wave * (kWave * 4);
    __syncthreads();

    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int slots = gridDim.x >> 3;
    const int t_lo = (int)(((int64_t)a.n_tiles * xcd) >> 3);
    const int t_hi = (int)(((int64_t)a.n_tiles * (xcd + 1)) >> 3);
    auto first_row = [&](int t) {
        if (t >= t_hi) return a.nb;
        const int tt = a.reverse ? t_lo + t_hi - 1 - t : t;
        const int tile = a.tile_order ? a.tile_order[tt] : tt + a.tile_base;
        return (tile * kWavesPerBlock + wave) * RW;
    };
    struct RowMeta {
        int len;
        unsigned word[MAXB];
    };
    auto col_of = [](unsigned w) { return (size_t)(w & 0xFFFFFFu); };
    auto id_of = [](unsigned w) { return (int)(w >> 24); };
    constexpr int ELLW = MAXB <= 3 ? 4 : 8;
    auto load_meta = [&](int row0, RowMeta& m) {
        const int i = row0 + s;
        const uint4* src = reinterpret_cast<const uint4*>(a.dict_ell) + (size_t)min(i, a.nb - 1) * (ELLW / 4);
        unsigned words[8];
        const uint4 lo = src[0];
        words[0] = lo.x, words[1] = lo.y, words[2] = lo.z, words[3] = lo.w;
        if constexpr (ELLW == 8) {
            const uint4 hi = src[1];
            words[4] = hi.x, words[5] = hi.y, words[6] = hi.z, words[7] = hi.w;
        } else {
            words[4] = words[5] = words[6] = words[7] = 0xFFFFFFFFu;
        }
        m.len = 0;
#pragma unroll
        for (int q = 0; q < MAXB; ++q) {
            const bool there = i < a.nb && words[q] != 0xFFFFFFFFu;
            m.len += there ? 1 : 0;
            m.word[q] = there ? words[q] : 0u;
        }
    };

    int pos = t_lo + slot;
    int row0 = first_row(pos);
    RowMeta meta;
    load_meta(row0, meta);
    for (; pos < t_hi; pos += slots) {
        const int row0_n = first_row(pos + slots);
        RowMeta meta_n;
        load_meta(row0_n, meta_n);

        const int i = row0 + s;
        const bool valid = i < a.nb;
        {
            double2 own[4];
#pragma unroll
            for (int be = 0; be < 4; ++be)
                own[be] = valid ? a.cur[vslot(be, (size_t)i, r, a.ncols, RL)] : make_double2(0.0, 0.0);
#pragma unroll
            for (int be = 0; be < 4; ++be) share[SHARE_SLOT(lane, be)] = own[be];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        if (valid) {
            auto source = [&](unsigned w) {
                const long d = (long)col_of(w) - (long)i;
                const long ss = (long)s + d;
                return (ss >= 0 && ss < RW && (long)i + d < a.nb) ? (int)d : (int)kWave;
            };
            const int target = ga.target_slot[i];
            double2 acc[4], x[4], xn[4];
#pragma unroll
            for (int al = 0; al < 4; ++al) acc[al] = make_double2(0.0, 0.0);
            if (meta.len > 0 && source(meta.word[0]) == kWave) {
#pragma unroll
                for (int be = 0; be < 4; ++be)
                    xn[be] = a.cur[vslot(be, col_of(meta.word[0]), r, a.ncols, RL)];
            }
#pragma unroll
            for (int q = 0; q < MAXB; ++q) {
                if (q < meta.len) {
                    const int src = source(meta.word[q]);
                    if (src == kWave) {
#pragma unroll
                        for (int be = 0; be < 4; ++be) x[be] = xn[be];
                    } else {
#pragma unroll
                        for (int be = 0; be < 4; ++be) x[be] = share[SHARE_SLOT(lane + src * RL, be)];
                    }
                    if (q + 1 < MAXB && q + 1 < meta.len && source(meta.word[q + 1 < MAXB ? q + 1 : 0]) == kWave) {
#pragma unroll
                        for (int be = 0; be < 4; ++be)
                            xn[be] = a.cur[vslot(be, col_of(meta.word[q + 1 < MAXB ? q + 1 : 0]), r, a.ncols, RL)];
                    }
                    Mode::mac_row(acc, lds + id_of(meta.word[q]) * STRIDE, x);
                }
            }
            double2 p[4];
            if (a.stream_vectors & 1) {
#pragma unroll
                for (int al = 0; al < 4; ++al) p[al] = load_stream(a.prev + vslot(al, (size_t)i, r, a.ncols, RL));
            } else {
#pragma unroll
                for (int al = 0; al < 4; ++al) p[al] = a.prev[vslot(al, (size_t)i, r, a.ncols, RL)];
            }
#pragma unroll
            for (int al = 0; al < 4; ++al) {
                p[al].x = fma(a.coef, acc[al].x, -p[al].x);
                p[al].y = fma(a.coef, acc[al].y, -p[al].y);
            }
            if (a.stream_vectors & 2) {
#pragma unroll
                for (int al = 0; al < 4; ++al) store_stream(a.prev + vslot(al, (size_t)i, r, a.ncols, RL), p[al]);
            } else {
#pragma unroll
                for (int al = 0; al < 4; ++al) a.prev[vslot(al, (size_t)i, r, a.ncols, RL)] = p[al];
            }
            store_picked<Mode::kVec>(ga, target, r, p);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        row0 = row0_n;
        meta = meta_n;
    }
}

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

using GreenKernel = void (*)(bdg::GreenArgs);

template <typename Mode>
GreenKernel green_generic_for(int rl) {
    switch (rl) {
        case 4: return bdg::cheb_green<Mode, 4>;
        case 8: return bdg::cheb_green<Mode, 8>;
        case 16: return bdg::cheb_green<Mode, 16>;
        case 32: return bdg::cheb_green<Mode, 32>;
        case 64: return bdg::cheb_green<Mode, 64>;
    }
    return nullptr;
}

template <typename Mode, int MAXB>
GreenKernel green_dict_for(int rl) {
    switch (rl) {
        case 4: return bdg::cheb_green_dict<Mode, 4, MAXB>;
        case 8: return bdg::cheb_green_dict<Mode, 8, MAXB>;
        case 16: return bdg::cheb_green_dict<Mode, 16, MAXB>;
        case 32: return bdg::cheb_green_dict<Mode, 32, MAXB>;
    }
    // (64 lanes: complex modes only, as for the Clenshaw dictionary kernel)
    if constexpr (Mode::kVec == 1)
        if (rl == 64) return bdg::cheb_green_dict<Mode, 64, MAXB>;
    return nullptr;
}

template <typename Mode>
GreenKernel green_kernel_for(bool dictionary, int max_row_blocks, int rl) {
    if (!dictionary) return green_generic_for<Mode>(rl);
    if (max_row_blocks <= 3) return green_dict_for<Mode, 3>(rl);
    if (max_row_blocks <= 5) return green_dict_for<Mode, 5>(rl);
    return green_dict_for<Mode, 7>(rl);
}

GreenKernel green_kernel(const ModeInfo& mode, bool dictionary, int max_row_blocks, int rl) {
    switch (mode.id) {
        case 1: return green_kernel_for<RealMode>(dictionary, max_row_blocks, rl);
        case 2: return green_kernel_for<ComplexPHMode>(dictionary, max_row_blocks, rl);
        case 3: return green_kernel_for<RealPHMode>(dictionary, max_row_blocks, rl);
    }
    return green_kernel_for<ComplexMode>(dictionary, max_row_blocks, rl);
}

// Launch plan of the picked step: that of the Clenshaw kernels (make_clenshaw_plan) for its own kernels.
struct GreenPlan {
    StepPlan step;  // tiles, grid, LDS, mode, dictionary flag (step.kernel unused)
    GreenKernel kernel = nullptr;
};

int make_green_plan(bdg_system* sys, int rl, const ModeInfo& mode, GreenPlan* out) {
    StepPlan& plan = out->step;
    plan = StepPlan{};
    plan.rl = rl;
    plan.mode = mode;
    const int rows_per_wave = bdg::kWave / rl;
    plan.rows_per_tile = rows_per_wave * bdg::kWavesPerBlock;
    plan.n_tiles = (int)((sys->nb + plan.rows_per_tile - 1) / plan.rows_per_tile);
    plan.dictionary = dict_kernel(sys, mode, rl) != nullptr;
    out->kernel = green_kernel(mode, plan.dictionary, sys->max_row_blocks, rl);
    if (!out->kernel) return fail(BDG_EINVAL, "unsupported lanes-per-row %d for the picked recurrence kernels", rl);
    if (plan.dictionary) {
        plan.lds_bytes = plan.lds_footprint = (size_t)sys->n_unique * mode.stride * sizeof(double2) +
                                              (size_t)bdg::kBlockThreads * 4 * sizeof(double2);
    } else {
        const int tile_blocks = rows_per_wave * std::max(1, sys->max_row_blocks);
        const int cap = (int)((160 * 1024 / bdg::kWavesPerBlock) / (mode.stride * sizeof(double2)));
        plan.stage_blocks = std::max(1, std::min(tile_blocks, cap));
        plan.lds_bytes = plan.lds_footprint =
            (size_t)bdg::kWavesPerBlock * plan.stage_blocks * mode.stride * sizeof(double2);
        if (plan.lds_bytes > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(out->kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
    }
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(out->kernel),
                                                         bdg::kBlockThreads, plan.lds_bytes));
    per_cu = std::max(1, std::min(per_cu, 8));
    if (const char* cap = knob::raw("BODGE_AMD_BLOCKS_PER_CU")) per_cu = std::max(1, atoi(cap));
    const int grid = std::min(plan.n_tiles, per_cu * sys->num_cus);
    plan.grid = std::max(8, (grid + 7) / 8 * 8);
    return BDG_OK;
}

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
    const char* real_env = knob::raw("BODGE_AMD_REAL");
    const bool real = sys->is_real && !(real_env && real_env[0] == '0');
    const char* ph_env = knob::raw("BODGE_AMD_PH");
    const ModeInfo mode = mode_info(real, sys->is_ph && !(ph_env && ph_env[0] == '0'));
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
    GreenPlan gplan;
    if (int rc = make_green_plan(sys, rl, mode, &gplan)) return rc;
    const StepPlan& plan = gplan.step;
    bdg::StepArgs base{};
    if (int rc = matrix_args(sys, plan, &base)) return rc;
    int strip_rows = 0;
    if (int rc = prepare_tile_order(sys, plan.rows_per_tile, plan.n_tiles, (real ? 32.0 : 64.0) * rv, &base.tile_order,
                                    &strip_rows))
        return rc;
    const size_t vec_count = (size_t)4 * nb * rl;
    base.stream_vectors = 2 * vec_count * sizeof(double2) > kStreamVectorBytes ? 3 : 0;
    if (const char* env = knob::raw("BODGE_AMD_STREAM_VECTORS")) base.stream_vectors = std::atoi(env);
    bool alternate = true;
    if (const char* env = knob::raw("BODGE_AMD_ALTERNATE")) alternate = std::atoi(env) != 0;
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
        perf.lanes_per_row = rl;
        perf.vectors_per_launch = rv;
        perf.grid = plan.grid;
        perf.lds_bytes = (int32_t)plan.lds_footprint;
        perf.pipelined = 0;
        perf.real_arithmetic = real ? 1 : 0;
        perf.strip_rows = strip_rows;
        perf.ph_packed = mode.ph ? 1 : 0;
        perf.dict_blocks = plan.dictionary ? sys->n_unique : 0;
        perf.steps_per_launch = 1;
        perf.dict_skipped = sys->dict_skipped;
        perf.streams = 1;
        perf.groups_per_launch = 1;
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
