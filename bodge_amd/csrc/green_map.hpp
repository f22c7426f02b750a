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

// Generic form: the twin of cheb_green (LDS staging of the streamed blocks, gathers of t_n, epilogue
// t_{n+1} = coef * (H t_n) - t_{n-1}) with the store of the vectors' own rows.
template <typename Mode, int RL>
__global__ __launch_bounds__(kBlockThreads, 4) void cheb_green_local(GreenLocalArgs ga) {
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
            // (the position is read here, after the tile loop and the vector stores: nothing of it is live before)
            store_local<Mode::kVec>(ga, ga.site_slot[i], r, nx);
        }
    }
}

// Dictionary form: the twin of cheb_green_dict (block table in LDS, fixed-width row words, own and
// neighbouring rows of t_n shared through LDS) with the same epilogue.
template <typename Mode, int RL, int MAXB>
__global__ __launch_bounds__(kBlockThreads, 4) void cheb_green_local_dict(GreenLocalArgs ga) {
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
            // (the position is read in the epilogue, not before the tile's products: one live register less across them)
            store_local<Mode::kVec>(ga, ga.site_slot[i], r, p);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        row0 = row0_n;
        meta = meta_n;
    }
}

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

using GreenLocalKernel = void (*)(bdg::GreenLocalArgs);

template <typename Mode>
GreenLocalKernel green_local_generic_for(int rl) {
    switch (rl) {
        case 4: return bdg::cheb_green_local<Mode, 4>;
        case 8: return bdg::cheb_green_local<Mode, 8>;
        case 16: return bdg::cheb_green_local<Mode, 16>;
        case 32: return bdg::cheb_green_local<Mode, 32>;
        case 64: return bdg::cheb_green_local<Mode, 64>;
    }
    return nullptr;
}

template <typename Mode, int MAXB>
GreenLocalKernel green_local_dict_for(int rl) {
    switch (rl) {
        case 4: return bdg::cheb_green_local_dict<Mode, 4, MAXB>;
        case 8: return bdg::cheb_green_local_dict<Mode, 8, MAXB>;
        case 16: return bdg::cheb_green_local_dict<Mode, 16, MAXB>;
        case 32: return bdg::cheb_green_local_dict<Mode, 32, MAXB>;
    }
    // (64 lanes: complex modes only, as for the Clenshaw dictionary kernel)
    if constexpr (Mode::kVec == 1)
        if (rl == 64) return bdg::cheb_green_local_dict<Mode, 64, MAXB>;
    return nullptr;
}

template <typename Mode>
GreenLocalKernel green_local_kernel_for(bool dictionary, int max_row_blocks, int rl) {
    if (!dictionary) return green_local_generic_for<Mode>(rl);
    if (max_row_blocks <= 3) return green_local_dict_for<Mode, 3>(rl);
    if (max_row_blocks <= 5) return green_local_dict_for<Mode, 5>(rl);
    return green_local_dict_for<Mode, 7>(rl);
}

GreenLocalKernel green_local_kernel(const ModeInfo& mode, bool dictionary, int max_row_blocks, int rl) {
    switch (mode.id) {
        case 1: return green_local_kernel_for<RealMode>(dictionary, max_row_blocks, rl);
        case 2: return green_local_kernel_for<ComplexPHMode>(dictionary, max_row_blocks, rl);
        case 3: return green_local_kernel_for<RealPHMode>(dictionary, max_row_blocks, rl);
    }
    return green_local_kernel_for<ComplexMode>(dictionary, max_row_blocks, rl);
}

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
    const char* real_env = knob::raw("BODGE_AMD_REAL");
    const bool real = sys->is_real && !(real_env && real_env[0] == '0');
    const char* ph_env = knob::raw("BODGE_AMD_PH");
    const ModeInfo mode = mode_info(real, sys->is_ph && !(ph_env && ph_env[0] == '0'));
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
    PickedPlan<GreenLocalKernel> gplan;
    if (int rc = make_picked_plan(sys, rl, mode, green_local_kernel, &gplan)) return rc;
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
