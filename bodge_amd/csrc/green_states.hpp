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
    const int comp_shift = n_components == 2 ? 1 : 2;
    lanczos_free(sys);
    HIP_TRY(hipSetDevice(sys->device));

    // Arithmetic as for apply(): real whenever the matrix is real, the columns complex all the same (Re and Im in
    // the two slots of a payload).  In every mode a payload is one column, so `rl` lanes carry rl columns.
    const ModeInfo mode = family_mode(sys);
    const bool real = mode.real;
    const int per_lane = mode.per_lane;
    // Columns per batch by the width rule of run_apply_series: the widest power of two whose vector buffer stays
    // within 96 MB, at most 64 columns - 32 in real arithmetic; set_lanes_per_row fixes the lanes instead.  A batch
    // holds whole states.
    const double per_column = (double)nb * 4 * 16.0;
    int width = real ? 32 : 64;
    while (width > 4 && width * per_column > 96.0 * 1024 * 1024) width >>= 1;
    int rl = std::max(4, next_pow2((int)std::min<int64_t>((int64_t)n_states * n_components, width)));
    if (sys->lanes_override >= 4) rl = sys->lanes_override;
    const int rv = rl * per_lane;
    const int batch_states = rl / n_components;
    FamilyPlan<GreenStateKernels::Kernel> gplan;
    if (int rc = make_family_plan<GreenStateKernels>(sys, rl, mode, bdg::GreenStateTail::kExtraLds, &gplan)) return rc;
    const GreenProjectKernel project = green_state_project_for(rl);
    if (!project) return fail(BDG_EINVAL, "unsupported lanes-per-row %d for the projected recurrence kernels", rl);
    const StepPlan& plan = gplan.step;
    bdg::StepArgs base{};
    if (int rc = matrix_args(sys, plan, &base)) return rc;
    int strip_rows = 0;
    if (int rc = prepare_tile_order(sys, plan.rows_per_tile, plan.n_tiles, 64.0 * rl, &base.tile_order, &strip_rows))
        return rc;
    const size_t vec_count = (size_t)4 * nb * rl;
    const VectorHints hints = family_vector_hints(vec_count);
    base.stream_vectors = hints.stream_vectors;
    const bool alternate = hints.alternate;
    const int n_batches = (n_states + batch_states - 1) / batch_states;

    // Device tables of a range of moments: the workgroups' partials [moment][workgroup][column][component] and the
    // reduced table [moment][state of the batch][component][column]; both count towards the limit, and the reduced
    // table is copied into the caller's when the range is full.
    size_t limit = kGreenTableBytes;
    if (const char* env = knob::raw("BODGE_AMD_GREEN_TABLE_BYTES")) limit = (size_t)std::max(1LL, atoll(env));
    const size_t per_state = (size_t)4 * n_components;            // double2 entries of one state and moment
    const size_t per_moment_max = (size_t)batch_states * per_state;
    const size_t partial_entries = (size_t)plan.grid * rl * 4;     // double2 entries of one moment's partials
    const int range = (int)std::max<size_t>(
        1, std::min<size_t>((size_t)n_moments, limit / ((per_moment_max + partial_entries) * sizeof(double2))));
    const int n_ranges = (n_moments + range - 1) / range;

    if (int rc = sys->vec_a.reserve(vec_count)) return rc;
    if (int rc = sys->vec_b.reserve(vec_count)) return rc;
    DeviceBuffer<double2> d_amplitudes, d_partial, d_table;
    std::vector<hipEvent_t> events;
    auto body = [&]() -> int {
        if (int rc = d_amplitudes.reserve((size_t)n_states * nb)) return rc;
        if (int rc = d_partial.reserve((size_t)range * partial_entries)) return rc;
        if (int rc = d_table.reserve((size_t)range * per_moment_max)) return rc;
        hipStream_t st = sys->stream;
        HIP_TRY(hipMemcpyAsync(d_amplitudes.ptr, amplitudes, sizeof(double2) * (size_t)n_states * nb, hipMemcpyHostToDevice, st));
        events.assign((size_t)2 * n_batches * n_ranges, nullptr);
        for (auto& ev : events) HIP_TRY(hipEventCreate(&ev));

        const int fill_grid = (int)std::min<size_t>(4096, (vec_count + 255) / 256);
        const int reduce_chunks = (rl * 4 + 63) / 64;
        bdg_perf perf{};
        for (int b = 0; b < n_batches; ++b) {
            const int q0 = b * batch_states;
            const int n_slots = std::min(batch_states, n_states - q0);
            const int n_active = n_slots * n_components;
            const size_t per_moment = (size_t)n_slots * per_state;
            bdg::GreenStateArgs ga{};
            ga.s = base;
            ga.amplitudes = d_amplitudes.ptr + (size_t)q0 * nb;
            ga.n_active = n_active;
            ga.comp_shift = comp_shift;
            double2* cur = sys->vec_a.ptr;
            double2* prev = sys->vec_b.ptr;
            bdg::green_state_start<<<fill_grid, 256, 0, st>>>(cur, nb, rl, n_active, comp_shift, ga.amplitudes);
            bdg::fill_zero<<<fill_grid, 256, 0, st>>>(prev, (int64_t)vec_count);
            for (int g = 0; g < n_ranges; ++g) {
                const int n0 = g * range, n1 = std::min(n_moments, n0 + range);
                const size_t ev = (size_t)2 * (b * n_ranges + g);
                HIP_TRY(hipEventRecord(events[ev], st));
                for (int n = n0; n < n1; ++n) {
                    double* partial = reinterpret_cast<double*>(d_partial.ptr + (size_t)(n - n0) * partial_entries);
                    if (n == 0) {
                        // mu_0 from t_0 itself
                        project<<<plan.grid, bdg::kBlockThreads, 0, st>>>(cur, (int)nb, n_active, comp_shift, ga.amplitudes, partial);
                        continue;
                    }
                    // t_1 = H~ t_0 (t_{-1} = 0), then t_{n+1} = 2 H~ t_n - t_{n-1}: the new vector replaces prev
                    ga.s.cur = cur;
                    ga.s.prev = prev;
                    ga.s.coef = (n == 1 ? 1.0 : 2.0) / scale;
                    ga.s.reverse = alternate ? (n & 1) : 0;
                    ga.partial = partial;
                    gplan.kernel<<<plan.grid, bdg::kBlockThreads, plan.lds_bytes, st>>>(ga);
                    std::swap(cur, prev);
                }
                // one launch sums the partials of the whole range
                bdg::green_state_reduce<<<(n1 - n0) * reduce_chunks, 256, 0, st>>>(d_partial.ptr, d_table.ptr, plan.grid, rl,
                                                                                    n_active, comp_shift);
                HIP_TRY(hipEventRecord(events[ev + 1], st));
                HIP_TRY(hipGetLastError());
                // rows (moment) of the batch's n_slots states into the caller's rows of n_states states
                double2* dst = reinterpret_cast<double2*>(out) + ((size_t)n0 * n_states + q0) * per_state;
                if (n_slots == n_states)
                    HIP_TRY(hipMemcpyAsync(dst, d_table.ptr, sizeof(double2) * (size_t)(n1 - n0) * per_moment,
                                           hipMemcpyDeviceToHost, st));
                else
                    HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double2) * (size_t)n_states * per_state, d_table.ptr,
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
        perf.bytes_per_launch = algorithmic_bytes(sys, rv, mode, plan.dictionary) + 16.0 * (double)nb * batch_states +
                                (double)(partial_entries * sizeof(double2));
        perf.bytes_moved = perf.bytes_per_launch * (double)perf.launches;
        family_perf(sys, plan, rv, strip_rows, 1, &perf);
        perf.green_ranges = n_ranges;
        perf.green_states = plan.dictionary ? 2 : 1;
        sys->perf = perf;
        return BDG_OK;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(sys->stream);
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    d_amplitudes.release();
    d_partial.release();
    d_table.release();
    return rc;
}

}  // namespace
