// green_states.hpp - Chebyshev moments of the resolvent between extended states,
//     mu_n[q][a][b] = <w_q a|T_n(H~)|w_q b>,   |w b> = sum_j w[j] e_{4j+b}
// (bdg_green_state_moments), for G(eps) in plane waves, wave packets, orbitals: the momentum-resolved spectral
// function and its Nambu partners.  Part of the single translation unit bodge_hip.hip (included after
// green_map.hpp): the kernels live in namespace bdg beside the picked kernels, the driver in the unnamed namespace.
//
// Projected recurrence.  A lane payload (double2) is ONE complex column in every mode, as in
// apply.hpp: in the real modes .x / .y carry Re and Im of the column and the real H acts on both alike.  Column
// c = C * q + b of a batch is state q of the batch started on Nambu component b (C = 2 or 4 columns per state).
// Every step is the step of green_map.hpp with another epilogue: after the store of t_{n+1}, lane (s, r) adds
// conj(w_q(r)[i]) * t_{n+1}[4i + al][r] for al = 0..3 to eight accumulators it keeps over all its tiles.  After
// the tile loop they are summed over the site lanes (xor shuffles), over the four waves (LDS, fixed order) and
// stored as one partial per workgroup; green_state_reduce adds the workgroups' partials in index order.  No
// atomics: one writer per partial and per table entry, every sum has a shape fixed by (grid, lanes) alone.
#pragma once

namespace bdg {

// What a launch reads besides a recurrence step's arguments.
struct GreenStateArgs {
    StepArgs s;                 // matrix, vector buffers, tiles; partial / discard / col_* are not read
    const double2* amplitudes;  // [states of the batch][nb]: w_q[i] of the batch's first state onwards
    double* partial;            // this launch's moment: [gridDim.x][RL][4][re, im]
    int n_active;               // columns of the batch that carry a state (the others are zero padding)
    int comp_shift;             // log2 of the columns per state: 1 or 2
};

// w of lane payload r on block row i (0 on the padding columns)
__device__ inline double2 state_amplitude(const GreenStateArgs& g, int r, int i) {
    return r < g.n_active ? g.amplitudes[(size_t)(r >> g.comp_shift) * g.s.nb + i] : make_double2(0.0, 0.0);
}

// proj[al] += conj(w) * nx[al], al = 0..3, (re, im) interleaved.  With w = 1 the products are exact and with
// w = 0 they add zeros: a unit amplitude reproduces the picked entries of green_map.hpp bit for bit.
__device__ inline void project_state(double proj[8], const double2 w, const double2 nx[4]) {
#pragma unroll
    for (int al = 0; al < 4; ++al) {
        proj[2 * al] = fma(w.x, nx[al].x, proj[2 * al]);
        proj[2 * al] = fma(w.y, nx[al].y, proj[2 * al]);
        proj[2 * al + 1] = fma(w.x, nx[al].y, proj[2 * al + 1]);
        proj[2 * al + 1] = fma(-w.y, nx[al].x, proj[2 * al + 1]);
    }
}

// The same on accumulators that live in LDS: `rows` holds a row of 4 * kWave slots per wave, slot (al, lane) laid out
// component-major like SHARE_SLOT (the 64 lanes of one 16-byte access touch consecutive slots).  A lane reads and
// writes its own four slots only, so nothing is to be ordered between lanes.  Held in registers across the tile loop
// the eight doubles made the streamed-block form spill in every mode (20 - 68 bytes per lane) and the dictionary form
// in ComplexPHMode; in LDS they cost eight 16-byte LDS accesses per tile and no register.
// The lane's slot is worked out where it is used, from an index the compiler cannot see through: kept across the
// tile loop it was the one register too many of the streamed-block form in ComplexPHMode (12 bytes of scratch per lane with
// hipcc of ROCm 7.2.0, AMD clang 22.0.0git; tests/test_green_states_host.py pins scratch = 0 for every instance).
__device__ inline double2* projection_slot(double2* rows) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    return rows + (tid / kWave) * (kWave * 4) + (tid & (kWave - 1));
}
__device__ inline void project_state_lds(double2* rows, const double2 w, const double2 nx[4]) {
    double2* accum = projection_slot(rows);
#pragma unroll
    for (int al = 0; al < 4; ++al) {
        double2 v = accum[al * kWave];
        v.x = fma(w.x, nx[al].x, v.x);
        v.x = fma(w.y, nx[al].y, v.x);
        v.y = fma(w.x, nx[al].y, v.y);
        v.y = fma(-w.y, nx[al].x, v.y);
        accum[al * kWave] = v;
    }
}
__device__ inline void clear_projection(double2* rows) {
    double2* accum = projection_slot(rows);
#pragma unroll
    for (int al = 0; al < 4; ++al) accum[al * kWave] = make_double2(0.0, 0.0);
}
__device__ inline void load_projection(double2* rows, double proj[8]) {
    const double2* accum = projection_slot(rows);
#pragma unroll
    for (int al = 0; al < 4; ++al) {
        const double2 v = accum[al * kWave];
        proj[2 * al] = v.x;
        proj[2 * al + 1] = v.y;
    }
}

// reduce_dots with W = 8 doubles per lane: over the site lanes by xor shuffles, over the four waves through
// `red` (kWavesPerBlock * RL * 8 doubles) in wave order, one partial per workgroup: partial[block][r][al][re, im].
template <int RL>
__device__ inline void reduce_projection(double proj[8], double* red, double* partial, int lane, int wave) {
    constexpr int W = 8;
#pragma unroll
    for (int off = kWave / 2; off >= RL; off >>= 1)
#pragma unroll
        for (int c = 0; c < W; ++c) proj[c] += __shfl_xor(proj[c], off);
    if (lane < RL)
#pragma unroll
        for (int c = 0; c < W; ++c) red[(wave * RL + lane) * W + c] = proj[c];
    __syncthreads();
    for (int e = threadIdx.x; e < W * RL; e += kBlockThreads) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) tot += red[w * RL * W + e];
        partial[(size_t)blockIdx.x * RL * W + e] = tot;
    }
}

// The tail of the projected step on the shared tile loops (family.hpp): the accumulators of the projection lie in
// the LDS behind what the tile loop uses (the staging regions in the streamed-block form, the shared rows in the
// dictionary form), a row per wave; after the store of t_{n+1} the lane adds its products, and after the tile loop
// the workgroup reduces them.
struct GreenStateTail : FamilyTail {
    using Args = GreenStateArgs;
    static constexpr const char* kFamily = "projected recurrence";
    // the accumulators: four 16-byte slots per lane (16 KB).  The reduction of the eight doubles per lane
    // (kWavesPerBlock * RL * 8 doubles <= 16 KB) reuses the front of the LDS.
    static constexpr size_t kExtraLds = (size_t)kBlockThreads * 4 * sizeof(double2);
    template <typename Mode, int RL>
    __device__ static double2* begin(const GreenStateArgs&, int, double2* behind) {
        clear_projection(behind);
        return behind;
    }
    template <typename Mode, int RL>
    __device__ static void after(const GreenStateArgs& ga, double2* accum, NoValue, int i, int r, const double2 nx[4]) {
        // (the amplitude is read here, after the tile's products and the vector stores: nothing of it is live before)
        project_state_lds(accum, state_amplitude(ga, r, i), nx);
    }
    template <typename Mode, int RL>
    __device__ static void finish(const GreenStateArgs& ga, double2* accum, double2* lds, int lane, int wave) {
        double proj[8];
        load_projection(accum, proj);
        __syncthreads();  // every wave is done with the tile loop's LDS and its accumulators: the reduction reuses the front
        reduce_projection<RL>(proj, reinterpret_cast<double*>(lds), ga.partial, lane, wave);
    }
};

// t_0 of a batch from the amplitude table: t_0[4i + a][C q + b] = w_q[i] * delta_ab; the components a >= C and the
// padding columns are zero.  Writes every payload of the buffer (no zero fill before it).
__global__ void green_state_start(double2* __restrict__ vec, int64_t nb, int rl, int n_active, int comp_shift,
                                  const double2* __restrict__ amplitudes) {
    const int64_t total = 4 * nb * rl;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx % rl);
        const int64_t e = idx / rl;  // 4 * site + component
        const int al = (int)(e & 3);
        const int64_t site = e >> 2;
        double2 v = make_double2(0.0, 0.0);
        if (r < n_active && (r & ((1 << comp_shift) - 1)) == al) v = amplitudes[(size_t)(r >> comp_shift) * nb + site];
        vec[vslot(al, (size_t)site, r, (size_t)nb, rl)] = v;
    }
}

// Moment 0: the projection of the step kernels applied to t_0 itself, in their lane layout (lane (s, r): block
// rows s, s + 64 / RL, ... of the wave's share) and with their reduction: partial[block][r][al][re, im].
template <int RL>
__global__ __launch_bounds__(kBlockThreads) void green_state_project(const double2* __restrict__ vec, int nb, int n_active,
                                                                      int comp_shift, const double2* __restrict__ amplitudes,
                                                                      double* __restrict__ partial) {
    __shared__ double red[kWavesPerBlock * RL * 8];
    constexpr int RW = kWave / RL;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int s = lane / RL;
    const int r = lane % RL;
    double proj[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t row0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * RW; row0 < nb;
         row0 += (int64_t)gridDim.x * kWavesPerBlock * RW) {
        const int i = (int)row0 + s;
        if (i < nb && r < n_active) {
            double2 x[4];
#pragma unroll
            for (int al = 0; al < 4; ++al) x[al] = vec[vslot(al, (size_t)i, r, (size_t)nb, RL)];
            project_state(proj, amplitudes[(size_t)(r >> comp_shift) * nb + i], x);
        }
    }
    reduce_projection<RL>(proj, red, partial, lane, wave);
}

// Second stage: table[m][q][a][b] = sum over the workgroups g, in index order, of partial[m][g][C q + b][a], for the
// moments m of a range.  One workgroup per (moment, 64 entries): thread t adds the workgroups t / 64, t / 64 + 4, ...
// of entry t % 64, then the four sums of an entry are added in ascending order.  The tree is fixed by `groups` alone.
__global__ __launch_bounds__(256) void green_state_reduce(const double2* __restrict__ partial, double2* __restrict__ table,
                                                           int groups, int rl, int n_active, int comp_shift) {
    __shared__ double2 part[256];
    const int entries = rl * 4;                 // complex entries of one workgroup's partial: [r][al]
    const int chunks = (entries + 63) / 64;
    const int m = blockIdx.x / chunks;
    const int e = (blockIdx.x % chunks) * 64 + (threadIdx.x & 63);
    const int first = threadIdx.x >> 6;
    double2 tot = make_double2(0.0, 0.0);
    if (e < entries) {
        const double2* p = partial + (size_t)m * groups * entries + e;
        for (int g = first; g < groups; g += 4) {
            const double2 v = p[(size_t)g * entries];
            tot.x += v.x;
            tot.y += v.y;
        }
    }
    part[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x < 64 && e < entries) {
        double2 sum = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sum.x += part[k * 64 + threadIdx.x].x;
            sum.y += part[k * 64 + threadIdx.x].y;
        }
        const int r = e >> 2, al = e & 3;
        if (r < n_active) {
            const int q = r >> comp_shift, b = r & ((1 << comp_shift) - 1);
            table[(size_t)m * n_active * 4 + ((((size_t)q * 4 + al) << comp_shift) + b)] = sum;
        }
    }
}

}  // namespace bdg

namespace {

using GreenStateKernels = FamilyKernels<bdg::GreenStateTail>;

using GreenProjectKernel = void (*)(const double2*, int, int, int, const double2*, double*);

GreenProjectKernel green_state_project_for(int rl) {
    switch (rl) {
        case 4: return bdg::green_state_project<4>;
        case 8: return bdg::green_state_project<8>;
        case 16: return bdg::green_state_project<16>;
        case 32: return bdg::green_state_project<32>;
        case 64: return bdg::green_state_project<64>;
    }
    return nullptr;
}

// bdg_green_state_moments on the range loop of green_driver.hpp.  A batch is `batch_states` whole states.  Device
// tables of a range of moments: the workgroups' partials [moment][workgroup][column][component], which the launches
// fill, and the reduced table [moment][state of the batch][component][column], copied into the caller's when the range
// is full.
struct GreenStates : GreenFeature {
    using Args = bdg::GreenStateArgs;
    static constexpr int32_t bdg_perf::*kFlag = &bdg_perf::green_states;
    bdg_system* sys;
    const GreenSetup<GreenStateKernels>& gs;
    GreenProjectKernel project;
    int batch_states, n_states, n_components;
    const double* amplitudes;
    double2* out;
    double launch_bytes;
    DeviceBuffer<double2> d_amplitudes, d_partial, d_table;
    int q0 = 0, n_slots = 0;  // the batch in flight: its first state, its states

    int comp_shift() const { return n_components == 2 ? 1 : 2; }
    size_t per_state() const { return (size_t)4 * n_components; }  // double2 entries of one state and moment
    size_t per_moment() const { return (size_t)n_slots * per_state(); }
    size_t partial_entries() const { return (size_t)gs.plan.step.grid * gs.rl * 4; }  // double2 entries of one moment's partials
    const double2* batch_amplitudes() const { return d_amplitudes.ptr + (size_t)q0 * sys->nb; }
    int upload(hipStream_t st) {
        if (int rc = d_amplitudes.reserve((size_t)n_states * sys->nb)) return rc;
        if (int rc = d_partial.reserve((size_t)gs.range * partial_entries())) return rc;
        if (int rc = d_table.reserve((size_t)gs.range * batch_states * per_state())) return rc;
        HIP_TRY(hipMemcpyAsync(d_amplitudes.ptr, amplitudes, sizeof(double2) * (size_t)n_states * sys->nb, hipMemcpyHostToDevice, st));
        return BDG_OK;
    }
    int start_batch(int b, double2* cur, double2* prev, Args* ga, hipStream_t st) {
        q0 = b * batch_states;
        n_slots = std::min(batch_states, n_states - q0);
        ga->amplitudes = batch_amplitudes();
        ga->n_active = n_slots * n_components;
        ga->comp_shift = comp_shift();
        const int fill_grid = (int)std::min<size_t>(4096, (gs.vec_count + 255) / 256);
        bdg::green_state_start<<<fill_grid, 256, 0, st>>>(cur, sys->nb, gs.rl, ga->n_active, comp_shift(), ga->amplitudes);
        bdg::fill_zero<<<fill_grid, 256, 0, st>>>(prev, (int64_t)gs.vec_count);
        return ga->n_active;
    }
    void moment0(const double2* cur, hipStream_t st) {
        project<<<gs.plan.step.grid, bdg::kBlockThreads, 0, st>>>(cur, (int)sys->nb, n_slots * n_components, comp_shift(),
                                                                  batch_amplitudes(), reinterpret_cast<double*>(d_partial.ptr));
    }
    void point(Args* ga, int m) { ga->partial = reinterpret_cast<double*>(d_partial.ptr + (size_t)m * partial_entries()); }
    void close_range(int n0, int n1, hipStream_t st) {
        // one launch sums the partials of the whole range
        const int reduce_chunks = (gs.rl * 4 + 63) / 64;
        bdg::green_state_reduce<<<(n1 - n0) * reduce_chunks, 256, 0, st>>>(d_partial.ptr, d_table.ptr, gs.plan.step.grid, gs.rl,
                                                                            n_slots * n_components, comp_shift());
    }
    int end_range(int n0, int n1, hipStream_t st) {
        // rows (moment) of the batch's n_slots states into the caller's rows of n_states states
        return green_copy_out(out + ((size_t)n0 * n_states + q0) * per_state(), (size_t)n_states * per_state(), d_table.ptr,
                              per_moment(), (size_t)(n1 - n0), st);
    }
    void release() {
        d_amplitudes.release();
        d_partial.release();
        d_table.release();
    }
};

int run_green_state_moments(bdg_system* sys, double scale, int n_moments, int n_states, const double* amplitudes,
                            int n_components, double* out) {
    if (!sys) return fail(BDG_EINVAL, "null system handle");
    if (!amplitudes || !out) return fail(BDG_EINVAL, "null argument");
    if (sys->ncols != sys->nb || sys->row_offset != 0)
        return fail(BDG_EINVAL, "bdg_green_state_moments needs a whole (square) matrix: slabs are not supported");
    if (!(scale > 0.0)) return fail(BDG_EINVAL, "scale must be positive");
    if (n_moments < 1) return fail(BDG_EINVAL, "n_moments must be >= 1");
    if (n_states < 1) return fail(BDG_EINVAL, "n_states must be >= 1");
    if (n_components != 2 && n_components != 4) return fail(BDG_EINVAL, "n_components must be 2 or 4");
    const int64_t nb = sys->nb;
    lanczos_free(sys);  // (no subspace_free here, unlike run_green_bond_blocks: kept as it was)
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic as for apply(): real whenever the matrix is real, the columns complex all the same (Re and Im in
    // the two slots of a payload).  In every mode a payload is one column, so `rl` lanes carry rl columns.
    const ModeInfo mode = family_mode(sys);
    // Columns per batch by the column rule of family.hpp.  A batch holds whole states.
    const int rl = family_column_lanes(sys, mode, (int64_t)n_states * n_components);
    const int batch_states = rl / n_components;
    GreenSetup<GreenStateKernels> gs;
    if (int rc = family_setup(sys, mode, rl, bdg::GreenStateTail::kExtraLds, &gs)) return rc;
    const GreenProjectKernel project = green_state_project_for(rl);
    if (!project) return fail(BDG_EINVAL, "unsupported lanes-per-row %d for the projected recurrence kernels", rl);

    // partials and reduced table both count towards the limit of a range
    const size_t partial_bytes = (size_t)gs.plan.step.grid * rl * 4 * sizeof(double2);
    green_cut_ranges(n_moments, (size_t)batch_states * 4 * n_components * sizeof(double2) + partial_bytes, &gs);
    GreenStates feature{{}, sys, gs, project, batch_states, n_states, n_components, amplitudes, reinterpret_cast<double2*>(out),
                        16.0 * (double)nb * batch_states + (double)partial_bytes};
    return run_green_ranges(sys, gs, scale, n_moments, (n_states + batch_states - 1) / batch_states, feature);
}

}  // namespace
