// fermi.hpp - the local one-body density matrix f(H) on the Hamiltonian's block pattern (bdg_fermi_blocks)
// Part of the single translation unit bodge_hip.hip (included after recurrence.hpp): the kernels live in
// namespace bdg beside the recurrence kernels, the driver in the unnamed namespace: its argument checks, its
// colour tables and the feature FermiBlocks on the rounds loop of family.hpp (run_family_rounds).
//
// Probing + Clenshaw.  The sites are coloured so that two sites of one colour are far apart
// in the graph of H; for colour c and Nambu component β the probe vector is r = Σ_{i ∈ c} e_{4i+β}, and
//     b_{M} = b_{M+1} = 0,   b_k = 2 H~ b_{k+1} - b_{k+2} + c_k r   (k = M-1 .. 1),   y = H~ b_1 - b_2 + c_0 r
// (H~ = H / scale) gives y = Σ_k c_k T_k(H~) r = f(H) r, whose rows 4j..4j+3 are column β of the block
// F_ji for every pattern block (j, i) with i of colour c.  A Clenshaw step moves what a recurrence step moves
// (read b_{k+1} around the row, read b_{k+2}, write b_k in place of it) plus one int32 colour per block row;
// the source term c_k r is made in registers from that colour, and no dot product is formed.
#pragma once

namespace bdg {

// What a Clenshaw launch reads besides a recurrence step's arguments.  Vector v of a batch is probe
// (colour colour_base + (v >> comp_shift), Nambu component v & ((1 << comp_shift) - 1)); vectors from
// n_active on are padding and stay zero.
struct ClenshawArgs {
    StepArgs s;               // matrix, vector buffers, tiles; partial / discard / col_* are not read
    const int* site_colour;   // [nb] colour of every block row
    double source;            // c_k: the coefficient this launch adds on the probe entries
    int colour_base;
    int comp_shift;           // 1: components 0, 1 (electron columns), 2: all four
    int n_active;
};

// nx[al] += c_k on the entries where the probe vectors of lane payload r are 1: row `colour` matches the
// vector's colour and al its component.  PER_LANE = 1: .x is the real part of vector r; 2: .x / .y are
// vectors 2r, 2r+1.  Compares instead of indexing keep nx in registers.
template <int PER_LANE>
__device__ inline void add_source(double2 nx[4], const ClenshawArgs& a, int colour, int r) {
    const int mask = (1 << a.comp_shift) - 1;
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
        const int v = PER_LANE * r + q;
        const bool hit = v < a.n_active && colour == a.colour_base + (v >> a.comp_shift);
        const int comp = v & mask;
#pragma unroll
        for (int al = 0; al < 4; ++al) {
            const double add = hit && comp == al ? a.source : 0.0;
            if (q == 0) nx[al].x += add;
            else nx[al].y += add;
        }
    }
}

// The tail of the probing Clenshaw step b_k = coef * (H b_{k+1}) - b_{k+2} + c_k r on the shared streamed-block tile
// loop (family.hpp): the colour of the block row, and the source term before the store.
struct FermiTail : FamilyTail {
    using Args = ClenshawArgs;
    static constexpr const char* kFamily = "Clenshaw";
    template <typename Mode, int RL>
    __device__ static int row(const ClenshawArgs& ca, NoValue, int i) {
        return ca.site_colour[i];
    }
    template <typename Mode, int RL>
    __device__ static void amend(const ClenshawArgs& ca, int colour, int, int r, double2 nx[4], double2[4]) {
        add_source<Mode::kVec>(nx, ca, colour, r);
    }
};

// Dictionary form: a tile loop of its own, the one the shared cheb_family_dict was lifted from (block table in LDS,
// fixed-width row words, own and neighbouring rows of b_{k+1} shared through LDS) with the Clenshaw epilogue.  With
// FermiTail on the shared loop this form was 4.5 % slower per launch on a cache-resident 256 x 256 lattice and 1.6 % on
// a 1000 x 1000 one (profiles/family_tile_loop_ab.json), so it stays; the streamed-block form, within
// the spread of the measurement on the shared loop, runs that.
template <typename Mode, int RL, int MAXB>
__global__ __launch_bounds__(kBlockThreads, 4) void cheb_clenshaw_dict(ClenshawArgs ca) {
    extern __shared__ double2 lds[];
    const StepArgs& a = ca.s;
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
            const int colour = ca.site_colour[i];
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
            add_source<Mode::kVec>(p, ca, colour, r);
            if (a.stream_vectors & 2) {
#pragma unroll
                for (int al = 0; al < 4; ++al) store_stream(a.prev + vslot(al, (size_t)i, r, a.ncols, RL), p[al]);
            } else {
#pragma unroll
                for (int al = 0; al < 4; ++al) a.prev[vslot(al, (size_t)i, r, a.ncols, RL)] = p[al];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        row0 = row0_n;
        meta = meta_n;
    }
}

// Columns of the pattern blocks whose column site has a colour of the batch, from the batch's final y:
//   out[k][al][b] = y[al][j][v],   v = (colour - colour_base) << comp_shift | b
// for entry e = (block k, block row j, colour) of the per-colour list and b < 1 << comp_shift.  One thread
// per (entry, al, b); the entries of one batch are a contiguous range of the list.  PER_LANE = 2: real
// payloads, vector v in component v & 1 of payload v >> 1.
template <int PER_LANE>
__global__ void fermi_extract(const double2* __restrict__ y, int64_t nb, int rl, const int* __restrict__ ent_block,
                              const int* __restrict__ ent_row, const int* __restrict__ ent_colour, int64_t n_ent,
                              int colour_base, int comp_shift, double2* __restrict__ out) {
    const int64_t per_entry = (int64_t)4 << comp_shift;
    const int64_t total = n_ent * per_entry;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = idx / per_entry;
        const int rest = (int)(idx - e * per_entry);
        const int al = rest >> comp_shift;
        const int b = rest & ((1 << comp_shift) - 1);
        const int v = ((ent_colour[e] - colour_base) << comp_shift) | b;
        const size_t at = vslot(al, (size_t)ent_row[e], v / PER_LANE, (size_t)nb, rl);
        double2 value;
        if (PER_LANE == 2) {
            const double2 pair = y[at];
            value = make_double2((v & 1) ? pair.y : pair.x, 0.0);
        } else {
            value = y[at];
        }
        out[(size_t)ent_block[e] * 16 + al * 4 + b] = value;
    }
}

}  // namespace bdg

namespace {

struct FermiDictKernels {
    template <typename Mode, int RL, int MAXB>
    static constexpr void (*kernel)(bdg::ClenshawArgs) = bdg::cheb_clenshaw_dict<Mode, RL, MAXB>;
};
using FermiKernels = FamilyKernels<bdg::FermiTail, FermiDictKernels>;

// HBM bytes of one Clenshaw launch: a recurrence launch's (same matrix stream, same three vector passes)
// plus the int32 colour of every block row.
double clenshaw_bytes(const bdg_system* sys, int vectors, const ModeInfo& mode, bool dictionary) {
    return algorithmic_bytes(sys, vectors, mode, dictionary) + 4.0 * (double)sys->nb;
}

// bdg_fermi_blocks on the rounds loop of family.hpp.  A batch is `colours_per_batch` whole colours; every batch
// leaves its columns of the pattern blocks in d_out, which goes to the caller after the last one.
struct FermiBlocks : FamilyFeature {
    using Args = bdg::ClenshawArgs;
    static constexpr int32_t bdg_perf::*kFlag = &bdg_perf::clenshaw;
    static constexpr int kVectors = 2;
    bdg_system* sys;
    const FamilySetup<FermiKernels>& fs;
    int n_colours, n_components, colours_per_batch;
    const double* coef;
    const int32_t* site_colour;
    const std::vector<int64_t>& colour_ptr;  // per colour: its range of the entry list
    const std::vector<int32_t>&ent_block, &ent_row, &ent_colour;
    int64_t n_pat;
    double* blocks_out;
    double launch_bytes;
    DeviceBuffer<int> d_colour, d_block, d_row, d_ent_colour;
    DeviceBuffer<double2> d_out;

    int upload(hipStream_t st) {
        const int64_t nb = sys->nb;
        if (int rc = d_colour.reserve((size_t)std::max<int64_t>(1, nb))) return rc;
        if (int rc = d_block.reserve(ent_block.size())) return rc;
        if (int rc = d_row.reserve(ent_block.size())) return rc;
        if (int rc = d_ent_colour.reserve(ent_block.size())) return rc;
        if (int rc = d_out.reserve((size_t)std::max<int64_t>(1, n_pat) * 16)) return rc;
        HIP_TRY(hipMemcpyAsync(d_colour.ptr, site_colour, sizeof(int) * nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_block.ptr, ent_block.data(), sizeof(int) * ent_block.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_row.ptr, ent_row.data(), sizeof(int) * ent_block.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_ent_colour.ptr, ent_colour.data(), sizeof(int) * ent_block.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_out.ptr, 0, sizeof(double2) * 16 * (size_t)n_pat, st));
        return BDG_OK;
    }
    int start_batch(int b, StreamSet*, Args* ca) {
        ca->site_colour = d_colour.ptr;
        ca->colour_base = b * colours_per_batch;
        ca->comp_shift = n_components == 4 ? 2 : 1;
        ca->n_active = std::min(colours_per_batch, n_colours - ca->colour_base) * n_components;
        return ca->n_active;
    }
    void point(Args* ca, int k) { ca->source = coef[k]; }
    void end_batch(int, StreamSet* set, const double2* y, const Args& ca) {
        const int c0 = ca.colour_base, c1 = c0 + ca.n_active / n_components;
        const int64_t e0 = colour_ptr[(size_t)c0], count = colour_ptr[(size_t)c1] - e0;
        if (count > 0) {
            const int64_t total = count * 4 * n_components;
            const int grid = (int)std::min<int64_t>(8192, (total + 255) / 256);
            const auto extract = fs.mode.real ? bdg::fermi_extract<2> : bdg::fermi_extract<1>;
            extract<<<grid, 256, 0, set->stream>>>(y, sys->nb, fs.rl, d_block.ptr + e0, d_row.ptr + e0, d_ent_colour.ptr + e0, count,
                                                   c0, ca.comp_shift, d_out.ptr);
        }
    }
    // the side streams join the handle's, which then carries d_out to the caller
    int finish(const std::vector<StreamSet*>& sets, hipStream_t st) {
        for (size_t s = 1; s < sets.size(); ++s) {
            HIP_TRY(hipEventRecord(sys->ev_side, sets[s]->stream));
            HIP_TRY(hipStreamWaitEvent(st, sys->ev_side, 0));
        }
        HIP_TRY(hipMemcpyAsync(blocks_out, d_out.ptr, sizeof(double2) * 16 * (size_t)n_pat, hipMemcpyDeviceToHost, st));
        return BDG_OK;
    }
    void release() {
        for (DeviceBuffer<int>* buf : {&d_colour, &d_block, &d_row, &d_ent_colour}) buf->release();
        d_out.release();
    }
};

int run_fermi_blocks(bdg_system* sys, double scale, int n_moments, const double* coef, int n_colours,
                     const int32_t* site_colour, int n_components, const int32_t* pat_indptr,
                     const int32_t* pat_indices, double* blocks_out) {
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    if (!coef || !site_colour || !pat_indptr || !pat_indices || !blocks_out) return fail(BDG_EINVAL, "null argument");
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_fermi_blocks needs a whole (square) matrix: slabs are not supported");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_colours < 1) return fail(BDG_EINVAL, "n_colours must be >= 1");
    if (n_components != 2 && n_components != 4) return fail(BDG_EINVAL, "n_components must be 2 or 4");
    const int64_t nb = sys->nb;
    if (pat_indptr[0] != 0) return fail(BDG_EINVAL, "pattern indptr must start at 0");
    for (int64_t i = 0; i < nb; ++i)
        if (pat_indptr[i + 1] < pat_indptr[i]) return fail(BDG_EINVAL, "pattern indptr is not monotone");
    const int64_t n_pat = pat_indptr[nb];
    for (int64_t k = 0; k < n_pat; ++k)
        if (pat_indices[k] < 0 || pat_indices[k] >= nb) return fail(BDG_EINVAL, "pattern column %d out of range", pat_indices[k]);
    for (int64_t i = 0; i < nb; ++i)
        if (site_colour[i] >= n_colours) return fail(BDG_EINVAL, "site colour %d out of range", site_colour[i]);
    lanczos_free(sys);
    HIP_TRY(hipSetDevice(sys->device));

    // Per-colour list of the pattern blocks (k, row j) whose column site i has that colour (counting sort);
    // a site with a negative colour is not probed by this call (the caller shares the colours out).
    std::vector<int64_t> colour_ptr((size_t)n_colours + 1, 0);
    for (int64_t k = 0; k < n_pat; ++k)
        if (site_colour[pat_indices[k]] >= 0) ++colour_ptr[(size_t)site_colour[pat_indices[k]] + 1];
    for (int c = 0; c < n_colours; ++c) colour_ptr[(size_t)c + 1] += colour_ptr[(size_t)c];
    const int64_t n_ent = colour_ptr[(size_t)n_colours];
    std::vector<int32_t> ent_block((size_t)std::max<int64_t>(1, n_ent)), ent_row(ent_block.size()), ent_colour(ent_block.size());
    {
        std::vector<int64_t> fill(colour_ptr.begin(), colour_ptr.end() - 1);
        for (int64_t j = 0; j < nb; ++j)
            for (int64_t k = pat_indptr[j]; k < pat_indptr[j + 1]; ++k) {
                const int c = site_colour[pat_indices[k]];
                if (c < 0) continue;
                const int64_t at = fill[(size_t)c]++;
                ent_block[(size_t)at] = (int32_t)k;
                ent_row[(size_t)at] = (int32_t)j;
                ent_colour[(size_t)at] = c;
            }
    }

    // Arithmetic and storage mode as for a recurrence with real start vectors (the probes are 0 / 1).  Vectors per
    // batch: whole colours, by the unit rule of family.hpp.
    const ModeInfo mode = family_mode(sys);
    const int colours_per_batch = std::max(1, std::min(n_colours, family_unit_width(sys, mode) / n_components));
    FamilySetup<FermiKernels> fs;
    if (int rc = family_setup(sys, mode, family_unit_lanes(sys, mode, colours_per_batch * n_components), 0, &fs)) return rc;
    FermiBlocks feature{{}, sys, fs, n_colours, n_components, colours_per_batch, coef, site_colour, colour_ptr, ent_block, ent_row,
                        ent_colour, n_pat, blocks_out, clenshaw_bytes(sys, fs.rv, mode, fs.plan.step.dictionary)};
    return run_family_rounds(sys, fs, scale, n_moments, (n_colours + colours_per_batch - 1) / colours_per_batch, feature);
}

}  // namespace
