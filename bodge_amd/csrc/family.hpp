// family.hpp - what the Clenshaw-family kernels and drivers share (fermi.hpp, apply.hpp, correlation.hpp,
// response_map.hpp, green.hpp, green_map.hpp, green_bonds.hpp, green_states.hpp).  Part of the single translation unit bodge_hip.hip (included after
// recurrence.hpp, before fermi.hpp): the kernels live in namespace bdg, the host helpers in the unnamed namespace.
//
// Every kernel of the family is one recurrence step  nx = coef * (H cur) - prev  written over prev, plus a few lines
// that are the feature's own: its TAIL.  The tile loop exists twice, once per form of the matrix:
//   cheb_family       streamed blocks: cheb_step's tile loop (LDS staging of the blocks, one-ahead gathers of cur)
//   cheb_family_dict  dictionary: cheb_step_dict's tile loop (block table in LDS, fixed-width row words, own and
//                     neighbouring rows of cur shared through LDS)
// and a tail is a type with static hooks, a template parameter of the kernel (no run-time "which caller"):
//   Args, kFamily                      the kernel's argument struct (Args::s is the StepArgs of the step); the
//                                      family's name in error messages
//   begin(args, r, behind)  -> Column  once per kernel, before the tile loop.  `behind` is the LDS behind what the
//                                      tile loop uses (plan: extra_lds bytes)
//   row(args, column, i)    -> Row     per block row i, read for the epilogue
//   amend(args, row, i, r, nx, spare)  between update and store: may change nx; spare[4] are dead registers
//   after(args, column, row, i, r, nx) after the store: reads nx only
//   finish(args, column, lds, lane, wave)  after the tile loop
// FamilyTail holds the empty hooks: a tail derives from it and names only the hooks it uses.  The hooks and the common
// epilogue are inline device functions; the two tile loops themselves stay in the __global__ functions (moved into a
// shared device function they cost 2 - 4 VGPRs and ComplexPHMode spilled: DESIGN.md §16).
//
// On the host: the dispatch and the launch plan of a family kernel, the two width rules
// (family_column_lanes; family_unit_width / family_unit_lanes), FamilySetup / family_setup - what every one of the
// eight drivers decides before its first launch - and run_family_rounds, the loop of fermi.hpp and apply.hpp, whose
// batches run side by side on the handle's stream sets.  The Green drivers' loop is in green_driver.hpp.
#pragma once

namespace bdg {

struct NoValue {};

struct FamilyTail {
    template <typename Mode, int RL, typename Args>
    __device__ static NoValue begin(const Args&, int, double2*) { return {}; }
    template <typename Mode, int RL, typename Args, typename Column>
    __device__ static NoValue row(const Args&, const Column&, int) { return {}; }
    template <typename Mode, int RL, typename Args, typename Row>
    __device__ static void amend(const Args&, const Row&, int, int, double2[4], double2[4]) {}
    template <typename Mode, int RL, typename Args, typename Column, typename Row>
    __device__ static void after(const Args&, const Column&, const Row&, int, int, const double2[4]) {}
    template <typename Mode, int RL, typename Args, typename Column>
    __device__ static void finish(const Args&, const Column&, double2*, int, int) {}
};

// The common epilogue: p = prev of block row i, nx = coef * acc - p; then the store of nx over prev.  Bit 0 of
// stream_vectors asks for the non-temporal load, bit 1 for the non-temporal store.  GROUPED: one branch on the hint
// around the four accesses (the dictionary loop: chosen per access it was 2 - 3 % slower there); otherwise the hint
// is chosen per access (the streamed-block loop: grouped, some of its instances need 2 VGPRs more).
template <int RL, bool GROUPED>
__device__ inline void family_update(const StepArgs& a, int i, int r, const double2 acc[4], double2 nx[4]) {
    if constexpr (GROUPED) {
        if (a.stream_vectors & 1) {
#pragma unroll
            for (int al = 0; al < 4; ++al) nx[al] = load_stream(a.prev + vslot(al, (size_t)i, r, a.ncols, RL));
        } else {
#pragma unroll
            for (int al = 0; al < 4; ++al) nx[al] = a.prev[vslot(al, (size_t)i, r, a.ncols, RL)];
        }
    } else {
#pragma unroll
        for (int al = 0; al < 4; ++al) {
            const size_t own = vslot(al, (size_t)i, r, a.ncols, RL);
            nx[al] = (a.stream_vectors & 1) ? load_stream(a.prev + own) : a.prev[own];
        }
    }
#pragma unroll
    for (int al = 0; al < 4; ++al) {
        nx[al].x = fma(a.coef, acc[al].x, -nx[al].x);
        nx[al].y = fma(a.coef, acc[al].y, -nx[al].y);
    }
}

template <int RL, bool GROUPED>
__device__ inline void family_store(const StepArgs& a, int i, int r, const double2 nx[4]) {
    if constexpr (GROUPED) {
        if (a.stream_vectors & 2) {
#pragma unroll
            for (int al = 0; al < 4; ++al) store_stream(a.prev + vslot(al, (size_t)i, r, a.ncols, RL), nx[al]);
        } else {
#pragma unroll
            for (int al = 0; al < 4; ++al) a.prev[vslot(al, (size_t)i, r, a.ncols, RL)] = nx[al];
        }
    } else {
#pragma unroll
        for (int al = 0; al < 4; ++al) {
            const size_t own = vslot(al, (size_t)i, r, a.ncols, RL);
            if (a.stream_vectors & 2) store_stream(a.prev + own, nx[al]);
            else a.prev[own] = nx[al];
        }
    }
}

// The XCD split of the tiles: workgroup b works for XCD b & 7 on that eighth of the tiles, every gridDim.x / 8-th one.
struct TileSplit {
    int t_lo, t_hi, first, step;
};
__device__ inline TileSplit tile_split(const StepArgs& a) {
    const int xcd = blockIdx.x & 7;
    TileSplit ts;
    ts.t_lo = (int)(((int64_t)a.n_tiles * xcd) >> 3);
    ts.t_hi = (int)(((int64_t)a.n_tiles * (xcd + 1)) >> 3);
    ts.first = ts.t_lo + (int)(blockIdx.x >> 3);
    ts.step = gridDim.x >> 3;
    return ts;
}
// Tile at position t of the split (launch direction, strip order)
__device__ inline int tile_at(const StepArgs& a, const TileSplit& ts, int t) {
    const int tt = a.reverse ? ts.t_lo + ts.t_hi - 1 - t : t;
    return a.tile_order ? a.tile_order[tt] : tt + a.tile_base;
}

template <typename Mode, int RL, typename Tail>
__global__ __launch_bounds__(kBlockThreads, 4) void cheb_family(typename Tail::Args ga) {
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
    const auto column = Tail::template begin<Mode, RL>(ga, r, lds + kWavesPerBlock * region);

    const TileSplit ts = tile_split(a);
    for (int t = ts.first; t < ts.t_hi; t += ts.step) {
        const int row0 = (tile_at(a, ts, t) * kWavesPerBlock + wave) * RW;
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
            // (the row's value is read here, not before the tile loop: the kernels sit at their 128 registers across
            // it, and one more live value there puts ComplexPHMode into scratch)
            const auto row = Tail::template row<Mode, RL>(ga, column, i);
            // The epilogue's addresses are formed here, from indices the compiler cannot see through.  With the
            // epilogue in functions of its own, hipcc of ROCm 7.2.0 (AMD clang 22.0.0git) otherwise forms their
            // lane-dependent parts (prev + 16 r, ...) before the tile loop and keeps them across it: 2 - 4 VGPRs more
            // in every mode and 12 - 36 bytes of scratch in ComplexPHMode.  Checked on that compiler only, and the
            // resource tests (scratch = 0, the VGPR limits) are the only guard: another compiler that sees through the
            // empty asm, or needs no such help, shows up there.
            int re = r, ie = i;
            asm volatile("" : "+v"(re), "+v"(ie));
            double2 nx[4];
            family_update<RL, false>(a, ie, re, acc, nx);
            Tail::template amend<Mode, RL>(ga, row, ie, re, nx, acc);
            family_store<RL, false>(a, ie, re, nx);
            Tail::template after<Mode, RL>(ga, column, row, i, re, nx);
        }
    }
    Tail::template finish<Mode, RL>(ga, column, lds, lane, wave);
}

// A block row of the dictionary form: its blocks as fixed-width row words (column in the low 24 bits, id of the
// block in the table in the high 8), absent ones as 0 behind `len`.
template <int MAXB>
struct RowMeta {
    int len;
    unsigned word[MAXB];
};
__device__ inline size_t word_column(unsigned w) { return (size_t)(w & 0xFFFFFFu); }
__device__ inline int word_block(unsigned w) { return (int)(w >> 24); }

// Row words of block row i (rows of 4 or 8 words: 16-byte loads); a row past the end reads the last one and keeps nothing
template <int MAXB>
__device__ inline void load_meta(const StepArgs& a, int i, RowMeta<MAXB>& m) {
    constexpr int ELLW = MAXB <= 3 ? 4 : 8;
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
}

// First block row of this wave in the tile at position t of the split; nb past the split's end
template <int RW>
__device__ inline int first_row(const StepArgs& a, const TileSplit& ts, int t, int wave) {
    if (t >= ts.t_hi) return a.nb;
    return (tile_at(a, ts, t) * kWavesPerBlock + wave) * RW;
}

// Where lane (s, r) of block row i finds the column of word w: the distance in rows to a lane of its own wave
// that shares that row through LDS, or kWave = gather it from memory
template <int RW>
__device__ inline int source(const StepArgs& a, unsigned w, int i, int s) {
    const long d = (long)word_column(w) - (long)i;
    const long ss = (long)s + d;
    return (ss >= 0 && ss < RW && (long)i + d < a.nb) ? (int)d : (int)kWave;
}

template <typename Mode, int RL, int MAXB, typename Tail>
__global__ __launch_bounds__(kBlockThreads, 4) void cheb_family_dict(typename Tail::Args ga) {
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
    const auto column = Tail::template begin<Mode, RL>(ga, r, lds + a.n_unique * STRIDE + kWavesPerBlock * (kWave * 4));
    __syncthreads();

    const TileSplit ts = tile_split(a);
    int pos = ts.first;
    int row0 = first_row<RW>(a, ts, pos, wave);
    RowMeta<MAXB> meta;
    load_meta(a, row0 + s, meta);
    for (; pos < ts.t_hi; pos += ts.step) {
        const int row0_n = first_row<RW>(a, ts, pos + ts.step, wave);
        RowMeta<MAXB> meta_n;
        load_meta(a, row0_n + s, meta_n);

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
            const auto row = Tail::template row<Mode, RL>(ga, column, i);
            double2 acc[4], x[4], xn[4];
#pragma unroll
            for (int al = 0; al < 4; ++al) acc[al] = make_double2(0.0, 0.0);
            if (meta.len > 0 && source<RW>(a, meta.word[0], i, s) == kWave) {
#pragma unroll
                for (int be = 0; be < 4; ++be)
                    xn[be] = a.cur[vslot(be, word_column(meta.word[0]), r, a.ncols, RL)];
            }
#pragma unroll
            for (int q = 0; q < MAXB; ++q) {
                if (q < meta.len) {
                    const int src = source<RW>(a, meta.word[q], i, s);
                    if (src == kWave) {
#pragma unroll
                        for (int be = 0; be < 4; ++be) x[be] = xn[be];
                    } else {
#pragma unroll
                        for (int be = 0; be < 4; ++be) x[be] = share[SHARE_SLOT(lane + src * RL, be)];
                    }
                    if (q + 1 < MAXB && q + 1 < meta.len &&
                        source<RW>(a, meta.word[q + 1 < MAXB ? q + 1 : 0], i, s) == kWave) {
#pragma unroll
                        for (int be = 0; be < 4; ++be)
                            xn[be] = a.cur[vslot(be, word_column(meta.word[q + 1 < MAXB ? q + 1 : 0]), r, a.ncols, RL)];
                    }
                    Mode::mac_row(acc, lds + word_block(meta.word[q]) * STRIDE, x);
                }
            }
            // (x[] is free from here on: it is the tail's spare; the opaque indices as in cheb_family)
            int re = r, ie = i;
            asm volatile("" : "+v"(re), "+v"(ie));
            double2 p[4];
            family_update<RL, true>(a, ie, re, acc, p);
            Tail::template amend<Mode, RL>(ga, row, ie, re, p, x);
            family_store<RL, true>(a, ie, re, p);
            Tail::template after<Mode, RL>(ga, column, row, i, re, p);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        row0 = row0_n;
        meta = meta_n;
    }
    Tail::template finish<Mode, RL>(ga, column, lds, lane, wave);
}

}  // namespace bdg

namespace {

// The dictionary kernels of a family: the shared loop with a tail, or (fermi.hpp) a loop of the family's own.
template <typename DictTail>
struct SharedDictKernels {
    template <typename Mode, int RL, int MAXB>
    static constexpr void (*kernel)(typename DictTail::Args) = bdg::cheb_family_dict<Mode, RL, MAXB, DictTail>;
};

// The kernel of a family for (mode, form, blocks per row, lanes per row): the tail of the streamed-block form and the
// dictionary kernels (the shared loop with the same tail unless the family says otherwise).  Lanes 4 .. 64; the
// 64-lane dictionary form exists in the complex modes only, as for the one-step dictionary kernel.  nullptr: no such
// instance.
template <typename Tail, typename Dict = SharedDictKernels<Tail>>
struct FamilyKernels {
    using Kernel = void (*)(typename Tail::Args);
    static constexpr const char* kFamily = Tail::kFamily;  // as the error messages name it

    template <typename Mode>
    static Kernel streamed(int rl) {
        switch (rl) {
            case 4: return bdg::cheb_family<Mode, 4, Tail>;
            case 8: return bdg::cheb_family<Mode, 8, Tail>;
            case 16: return bdg::cheb_family<Mode, 16, Tail>;
            case 32: return bdg::cheb_family<Mode, 32, Tail>;
            case 64: return bdg::cheb_family<Mode, 64, Tail>;
        }
        return nullptr;
    }
    template <typename Mode, int MAXB>
    static Kernel dictionary(int rl) {
        switch (rl) {
            case 4: return Dict::template kernel<Mode, 4, MAXB>;
            case 8: return Dict::template kernel<Mode, 8, MAXB>;
            case 16: return Dict::template kernel<Mode, 16, MAXB>;
            case 32: return Dict::template kernel<Mode, 32, MAXB>;
        }
        if constexpr (Mode::kVec == 1)
            if (rl == 64) return Dict::template kernel<Mode, 64, MAXB>;
        return nullptr;
    }
    template <typename Mode>
    static Kernel for_mode(bool dict, int max_row_blocks, int rl) {
        if (!dict) return streamed<Mode>(rl);
        if (max_row_blocks <= 3) return dictionary<Mode, 3>(rl);
        if (max_row_blocks <= 5) return dictionary<Mode, 5>(rl);
        return dictionary<Mode, 7>(rl);
    }
    static Kernel select(const ModeInfo& mode, bool dict, int max_row_blocks, int rl) {
        switch (mode.id) {
            case 1: return for_mode<RealMode>(dict, max_row_blocks, rl);
            case 2: return for_mode<ComplexPHMode>(dict, max_row_blocks, rl);
            case 3: return for_mode<RealPHMode>(dict, max_row_blocks, rl);
        }
        return for_mode<ComplexMode>(dict, max_row_blocks, rl);
    }
};

// Launch plan of a family kernel: the one-step recurrence's choice between the dictionary and the streamed-block
// form (dict_kernel decides, as in make_plan), its tiles and its LDS without the space of the dot reduction, plus
// `extra_lds` bytes behind it for the tail.  The pipelined one-step form has no twin in the family: a matrix that
// would take it runs the streamed-block form.
template <typename Kernel>
struct FamilyPlan {
    StepPlan step;  // tiles, grid, LDS, mode, dictionary flag (step.kernel unused)
    Kernel kernel = nullptr;
};

template <typename Kernels>
int make_family_plan(bdg_system* sys, int rl, const ModeInfo& mode, size_t extra_lds,
                     FamilyPlan<typename Kernels::Kernel>* out) {
    StepPlan& plan = out->step;
    plan = StepPlan{};
    plan.rl = rl;
    plan.mode = mode;
    const int rows_per_wave = bdg::kWave / rl;
    plan.rows_per_tile = rows_per_wave * bdg::kWavesPerBlock;
    plan.n_tiles = (int)((sys->nb + plan.rows_per_tile - 1) / plan.rows_per_tile);
    plan.dictionary = dict_kernel(sys, mode, rl) != nullptr;
    out->kernel = Kernels::select(mode, plan.dictionary, sys->max_row_blocks, rl);
    if (!out->kernel) return fail(BDG_EINVAL, "unsupported lanes-per-row %d for the %s kernels", rl, Kernels::kFamily);
    const void* kernel = reinterpret_cast<const void*>(out->kernel);
    if (plan.dictionary) {
        plan.lds_bytes = (size_t)sys->n_unique * mode.stride * sizeof(double2) +
                         (size_t)bdg::kBlockThreads * 4 * sizeof(double2);
    } else {
        const int tile_blocks = rows_per_wave * std::max(1, sys->max_row_blocks);
        const int cap = (int)(((160 * 1024 - extra_lds) / bdg::kWavesPerBlock) / (mode.stride * sizeof(double2)));
        plan.stage_blocks = std::max(1, std::min(tile_blocks, cap));
        plan.lds_bytes = (size_t)bdg::kWavesPerBlock * plan.stage_blocks * mode.stride * sizeof(double2);
    }
    plan.lds_bytes = plan.lds_footprint = plan.lds_bytes + extra_lds;
    if (plan.lds_bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, bdg::kBlockThreads, plan.lds_bytes));
    per_cu = std::max(1, std::min(per_cu, 8));
    if (const char* cap = knob::raw("BODGE_AMD_BLOCKS_PER_CU")) per_cu = std::max(1, atoi(cap));
    const int grid = std::min(plan.n_tiles, per_cu * sys->num_cus);
    plan.grid = std::max(8, (grid + 7) / 8 * 8);
    return BDG_OK;
}

// Arithmetic and storage mode of a family call: real whenever the matrix is real, particle-hole packed whenever it
// is particle-hole symmetric (the start vectors of the family never stand in the way); BODGE_AMD_REAL=0 and
// BODGE_AMD_PH=0 switch either off.
ModeInfo family_mode(const bdg_system* sys) {
    const char* real_env = knob::raw("BODGE_AMD_REAL");
    const bool real = sys->is_real && !(real_env && real_env[0] == '0');
    const char* ph_env = knob::raw("BODGE_AMD_PH");
    return mode_info(real, sys->is_ph && !(ph_env && ph_env[0] == '0'));
}

// Vector hints and launch direction of a family call: non-temporal loads and stores of prev once the two vector
// buffers (vec_count payloads each) outgrow kStreamVectorBytes, the direction of the tiles alternating from launch
// to launch; BODGE_AMD_STREAM_VECTORS and BODGE_AMD_ALTERNATE override.
struct VectorHints {
    int stream_vectors;
    bool alternate;
};
VectorHints family_vector_hints(size_t vec_count) {
    VectorHints hints{2 * vec_count * sizeof(double2) > kStreamVectorBytes ? 3 : 0, true};
    if (const char* env = knob::raw("BODGE_AMD_STREAM_VECTORS")) hints.stream_vectors = std::atoi(env);
    if (const char* env = knob::raw("BODGE_AMD_ALTERNATE")) hints.alternate = std::atoi(env) != 0;
    return hints;
}

// The bdg_perf fields that follow from the plan in every family driver; the driver adds its own (its flag, launches,
// bytes, timings, ...).
void family_perf(const bdg_system* sys, const StepPlan& plan, int rv, int strip_rows, int streams, bdg_perf* perf) {
    perf->lanes_per_row = plan.rl;
    perf->vectors_per_launch = rv;
    perf->grid = plan.grid;
    perf->lds_bytes = (int32_t)plan.lds_footprint;
    perf->pipelined = 0;
    perf->real_arithmetic = plan.mode.real ? 1 : 0;
    perf->strip_rows = strip_rows;
    perf->ph_packed = plan.mode.ph ? 1 : 0;
    perf->dict_blocks = plan.dictionary ? sys->n_unique : 0;
    perf->steps_per_launch = 1;
    perf->dict_skipped = sys->dict_skipped;
    perf->streams = streams;
    perf->groups_per_launch = 1;
}

// The width rules.  One vector buffer of a batch stays within 96 MB (batch_width's rule for the one-step kernels);
// set_lanes_per_row fixes the lanes instead.
constexpr double kFamilyBufferBytes = 96.0 * 1024 * 1024;

// Lanes per row of a call whose columns are complex (apply, correlation, response_map, green_states):
// a payload is one column, 16 B per entry.  The widest power of two within the 96 MB, at most 64 columns - 32 in real
// arithmetic, whose kernels count a column as two of their 64 vectors - and no wider than the call's columns need.
int family_column_lanes(const bdg_system* sys, const ModeInfo& mode, int64_t n_columns) {
    const double per_column = (double)sys->nb * 4 * 16.0;
    int width = mode.real ? 32 : 64;
    while (width > 4 && width * per_column > kFamilyBufferBytes) width >>= 1;
    const int rl = std::max(4, next_pow2((int)std::min<int64_t>(n_columns, width)));
    return sys->lanes_override >= 4 ? sys->lanes_override : rl;
}

// A call with unit start vectors (fermi, the Green tables): the widest batch in vectors - a power of two up to 64, a
// real vector being half a payload - and the lanes per row of a batch of at most `n_active_max` of them.
int family_unit_width(const bdg_system* sys, const ModeInfo& mode) {
    const double per_vector = (double)sys->nb * 4 * (mode.real ? 8.0 : 16.0);
    int width = 64;
    while (width > 8 && width * per_vector > kFamilyBufferBytes) width >>= 1;
    if (sys->lanes_override >= 4) width = std::min(64, sys->lanes_override * mode.per_lane);
    return width;
}
int family_unit_lanes(const bdg_system* sys, const ModeInfo& mode, int n_active_max) {
    const int rl = std::max(4, next_pow2((n_active_max + mode.per_lane - 1) / mode.per_lane));
    return sys->lanes_override >= 4 && sys->lanes_override * mode.per_lane >= n_active_max ? sys->lanes_override : rl;
}

// What a family call has decided before its first launch, given its mode and lanes per row.
template <typename Kernels>
struct FamilySetup {
    FamilyPlan<typename Kernels::Kernel> plan;
    ModeInfo mode{};
    int rl = 0, rv = 0;        // lanes per row, vectors per launch
    bdg::StepArgs base{};      // the matrix side of every launch's arguments
    int strip_rows = 0;
    size_t vec_count = 0;      // payloads of one vector buffer
    bool alternate = false;    // the tiles' direction alternates from launch to launch
};

template <typename Kernels>
int family_setup(bdg_system* sys, const ModeInfo& mode, int rl, size_t extra_lds, FamilySetup<Kernels>* fs) {
    fs->mode = mode;
    fs->rl = rl;
    fs->rv = rl * mode.per_lane;
    if (int rc = make_family_plan<Kernels>(sys, rl, mode, extra_lds, &fs->plan)) return rc;
    const StepPlan& plan = fs->plan.step;
    if (int rc = matrix_args(sys, plan, &fs->base)) return rc;
    // A row of t_n is one 16-byte payload per lane and component, 64 rl bytes, in every mode: per vector that is
    // (real ? 32 : 64) bytes, and rv = (real ? 2 : 1) rl vectors share the row.
    if (int rc = prepare_tile_order(sys, plan.rows_per_tile, plan.n_tiles, 64.0 * rl, &fs->base.tile_order, &fs->strip_rows))
        return rc;
    fs->vec_count = (size_t)4 * sys->nb * rl;
    const VectorHints hints = family_vector_hints(fs->vec_count);
    fs->base.stream_vectors = hints.stream_vectors;
    fs->alternate = hints.alternate;
    return BDG_OK;
}

// Streams of a call whose batches run side by side (fermi, apply): two of the handle's stream sets while one launch
// leaves the GPU part empty (the rule of run_recurrence for the one-step kernels), never more than it has batches;
// BODGE_AMD_STREAMS overrides.
int family_streams(const bdg_system* sys, int rv, int n_batches) {
    int n_streams = (double)sys->nb * rv <= kSideBySideOneStepLimit ? 2 : 1;
    if (const char* env = knob::raw("BODGE_AMD_STREAMS")) n_streams = std::clamp(atoi(env), 1, 4);
    return std::max(1, std::min(n_streams, n_batches));
}

// What a feature of the rounds loop need not say.  A feature type has
//   Args, kFlag, launch_bytes   the kernel's arguments (with n_active), the call's bdg_perf flag, its bytes_per_launch
//   kVectors, kRecord      vector buffers of a stream set in use, 2 (vec_a, vec_b) .. 4; whether sys->perf takes the record
//   upload(st)             reserve its device buffers, upload its tables
//   start_batch(b, set, &args)   the batch's fields into args, its start kernels onto the set's stream; returns the
//                          active columns, or an error (< 0)
//   point(&args, k)        the source coefficient of T_k into args
//   end_batch(b, set, y, args), drain_batch(b, set, args)   after the stop event; after the round's hipGetLastError
//   finish(sets, st)       after the last round: joins the side streams before the handle's stream is awaited
//   release()              its device buffers given back; called once, on every way out
struct FamilyFeature {
    static constexpr bool kRecord = true;  // (a feature whose caller decides hides it with a member: ApplySeries)
    template <typename Args>
    int drain_batch(int, StreamSet*, const Args&) { return BDG_OK; }
};

// The Clenshaw loop of fermi.hpp and apply.hpp: batches in rounds of one per stream; per batch b_M = b_{M+1} = 0, then
// one launch per coefficient (k = M-1 .. 0), the batches of a round in turn so that their launches fill each other's gaps.
template <typename Kernels, typename Feature>
int run_family_rounds(bdg_system* sys, const FamilySetup<Kernels>& fs, double scale, int n_moments, int n_batches, Feature& f) {
    const int n_streams = family_streams(sys, fs.rv, n_batches);
    std::vector<StreamSet*> sets;
    if (int rc = side_stream_sets(sys, n_streams, &sets)) return rc;
    for (StreamSet* set : sets) {
        DeviceBuffer<double2>* const vectors[4] = {&set->vec_a, &set->vec_b, &set->vec_c, &set->vec_d};
        for (int v = 0; v < Feature::kVectors; ++v)
            if (int rc = vectors[v]->reserve(fs.vec_count)) return rc;
    }
    const StepPlan& plan = fs.plan.step;
    std::vector<hipEvent_t> events;
    auto body = [&]() -> int {
        hipStream_t st = sys->stream;
        if (int rc = f.upload(st)) return rc;
        // (tables, packed blocks and the feature's uploads are on the handle's stream: the side streams wait for them)
        if (!sys->ev_side) HIP_TRY(hipEventCreateWithFlags(&sys->ev_side, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(sys->ev_side, st));
        for (int s = 1; s < n_streams; ++s) HIP_TRY(hipStreamWaitEvent(sets[(size_t)s]->stream, sys->ev_side, 0));
        events.assign((size_t)2 * n_batches, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        const int fill_grid = (int)std::min<size_t>(4096, (fs.vec_count + 255) / 256);
        bdg_perf perf{};
        std::vector<typename Feature::Args> args((size_t)n_streams);
        std::vector<double2*> cur((size_t)n_streams), prev((size_t)n_streams);
        for (int first = 0; first < n_batches; first += n_streams) {
            const int last = std::min(n_batches, first + n_streams);
            for (int b = first; b < last; ++b) {
                const size_t q = (size_t)(b - first);
                StreamSet* set = sets[q];
                args[q] = typename Feature::Args{};
                args[q].s = fs.base;
                cur[q] = set->vec_a.ptr;
                prev[q] = set->vec_b.ptr;
                if (int rc = f.start_batch(b, set, &args[q]); rc < 0) return rc;
                bdg::fill_zero<<<fill_grid, 256, 0, set->stream>>>(set->vec_a.ptr, (int64_t)fs.vec_count);
                bdg::fill_zero<<<fill_grid, 256, 0, set->stream>>>(set->vec_b.ptr, (int64_t)fs.vec_count);
                HIP_TRY(hipEventRecord(events[(size_t)2 * b], set->stream));
            }
            for (int n = 0; n < n_moments; ++n) {
                const int k = n_moments - 1 - n;
                for (int b = first; b < last; ++b) {
                    const size_t q = (size_t)(b - first);
                    typename Feature::Args& ca = args[q];
                    ca.s.cur = cur[q];
                    ca.s.prev = prev[q];
                    ca.s.coef = (k == 0 ? 1.0 : 2.0) / scale;
                    ca.s.reverse = fs.alternate ? (n & 1) : 0;
                    f.point(&ca, k);
                    fs.plan.kernel<<<plan.grid, bdg::kBlockThreads, plan.lds_bytes, sets[q]->stream>>>(ca);
                    std::swap(cur[q], prev[q]);
                }
            }
            for (int b = first; b < last; ++b) {
                const size_t q = (size_t)(b - first);
                HIP_TRY(hipEventRecord(events[(size_t)2 * b + 1], sets[q]->stream));
                f.end_batch(b, sets[q], cur[q], args[q]);
                perf.vector_steps += (int64_t)n_moments * args[q].n_active;
            }
            HIP_TRY(hipGetLastError());
            for (int b = first; b < last; ++b)
                if (int rc = f.drain_batch(b, sets[(size_t)(b - first)], args[(size_t)(b - first)])) return rc;
        }
        if (int rc = f.finish(sets, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        // kernel time: start to stop event of every batch; the window: the first start to the latest stop
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
        perf.bytes_per_launch = f.launch_bytes;
        perf.bytes_moved = perf.bytes_per_launch * (double)perf.launches;
        family_perf(sys, plan, fs.rv, fs.strip_rows, n_streams, &perf);
        perf.*Feature::kFlag = plan.dictionary ? 2 : 1;
        if (f.kRecord) sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) {  // (an error leaves nothing in flight: later calls reuse the streams' buffers)
        (void)hipStreamSynchronize(sys->stream);
        for (auto& side : sys->side_sets) (void)hipStreamSynchronize(side->stream);
    }
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    f.release();
    return rc;
}

}  // namespace
