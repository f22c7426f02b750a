/*
 * bodge_hip.h - C ABI of the MI355X (gfx950) BdG solver library `libbodge_hip.so`.
 *
 * The reference package is pure Python and has no FFI layer; its accelerator
 * seam is the `cuda: bool` switch inside three Hamiltonian methods, each of
 * which hands ONE matrix to a GPU library call and takes arrays back:
 *
 *   free_energy()  bodge/hamiltonian.py:282-302  (dense eigvalsh; CuPy at :291-295)
 *   diagonalize()  bodge/hamiltonian.py:203-232  (dense eigh;     CuPy at :210-221)
 *   ldos()         bodge/hamiltonian.py:342-382  (sparse LU resolvent per energy)
 *
 * and the matrix they consume is the BSR triple built at :37-67 / :102-118
 * (4x4 complex128 blocks, int32 indices/indptr).  The entry points below are
 * what a ctypes binding placed at those call sites would bind: upload the BSR
 * triple once, then ask for Chebyshev dot products / moments (free energy,
 * LDOS) or for a dense Hermitian eigensolve (diagonalize, small free_energy).
 *
 * Conventions: every pointer is a caller-owned host buffer unless stated; the
 * library copies to and from HBM.  Complex numbers are interleaved (re, im)
 * doubles, i.e. numpy complex128.  Every function returns 0 on success or a
 * negative BDG_E* code; `bdg_last_error()` then describes the failure (thread
 * local).  No callbacks, no exceptions, one host thread per handle.  The handles
 * of one device share that device's HIP streams (round 4): calls on two handles
 * from two host threads are correct but ordered on the GPU, not concurrent.
 */
#ifndef BODGE_HIP_H
#define BODGE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDG_OK 0
#define BDG_EINVAL (-1)   /* bad argument (shape, range, null pointer)      */
#define BDG_EDEVICE (-2)  /* HIP runtime error / no usable GPU              */
#define BDG_ENOMEM (-3)   /* device allocation failed                       */
#define BDG_ELIBRARY (-4) /* rocSOLVER / RCCL could not be loaded or failed */

/* start-vector kinds for the stochastic trace (counter-based) */
#define BDG_VEC_RADEMACHER 0 /* entries +1 / -1                  */
#define BDG_VEC_Z4 1         /* entries in {1, i, -1, -i}        */

typedef struct bdg_system bdg_system; /* one uploaded Hamiltonian on one GPU */
typedef struct bdg_comm bdg_comm;     /* one RCCL communicator rank          */
typedef struct bdg_group bdg_group;   /* several slabs driven by one process */

/* Performance record of the most recent Chebyshev call on a handle. */
typedef struct bdg_perf {
    double kernel_ms;      /* HIP-event time around the recurrence launches, summed over the streams */
    int64_t launches;      /* number of recurrence-kernel launches in that window    */
    int64_t vector_steps;  /* launches x vectors advanced per launch                 */
    double bytes_per_launch; /* algorithmic HBM bytes of one launch      */
    int32_t lanes_per_row; /* kernel configuration actually used                     */
    int32_t vectors_per_launch;
    int32_t grid;          /* workgroups per launch                                  */
    int32_t lds_bytes;     /* LDS one workgroup occupies                             */
    int32_t pipelined;     /* 1 = register-prefetch kernel, 0 = generic kernel       */
    int32_t real_arithmetic; /* 1 = real-valued specialisation (imag(H)=0, real vectors) */
    int32_t strip_rows;    /* strip width of the tile order in block rows, 0 = natural order */
    int32_t ph_packed;     /* 1 = particle-hole packed blocks (12 of 16 entries stored)      */
    int32_t dict_blocks;   /* >0 = dictionary form: number of distinct blocks in the table   */
    int32_t steps_per_launch; /* recurrence steps one launch makes: 3 or 2 = multi-step sweeps of a 2-D lattice
                                 stencil (cheb_sweep3 / cheb_sweep), else 1 */
    int32_t rolling;       /* 1 = 3-D stencil kernel with the x-neighbours in registers (cheb_roll3) */
    int32_t dict_skipped;  /* why the matrix has no block dictionary: 0 = it has one, 1 = more than 256
                              distinct blocks, 2 = more than 2^24 block columns, 3 = BODGE_AMD_DICT=0 */
    int32_t onsite_streamed; /* 1 = position-dependent on-site blocks: the diagonal block of every site is
                                streamed from HBM once per launch, only the bond blocks sit in the table
                                (dict_blocks then counts the distinct bond blocks); 2 = the bond blocks are
                                streamed as well (real matrices with spin-diagonal hopping: no table)      */
    int32_t streams;       /* HIP streams the batches of the call ran on side by side (1 = back to back) */
    double bytes_moved;    /* algorithmic HBM bytes of all `launches` together.  Less than launches x
                              bytes_per_launch: the first sweep of a run reads no t_{-1} (and no t_0 when it
                              makes the random start block itself), and the last launch of a run stores no
                              vectors - nothing reads them, the call returns dot products (BODGE_AMD_KEEP_LAST=1
                              stores them all the same).  Divide by window_ms for the achieved rate. */
    double window_ms;      /* HIP-event time from the first launch of the call to the end of its last one.  A call
                              with several batches of vectors runs them on `streams` streams side by side (the
                              idle start and end of one launch fill with another batch's work): kernel_ms then
                              sums the streams' own times (kernel_ms / launches = duration of one launch, what a
                              profiler reports) and window_ms is the elapsed time they share.  One stream:
                              window_ms = kernel_ms. */
    int64_t sweeps;        /* multi-step sweeps made, summed over the lane groups (= launches with one launch per sweep) */
    int32_t persistent;    /* 1 = cheb_march3: every launch makes all the sweeps of a reduction chunk (up to 21 = 63
                              steps) of `groups_per_launch` lane groups; its waves claim (sweep, group, unit) tasks and
                              start one as soon as the neighbouring units have published the sweep before */
    int32_t groups_per_launch; /* lane groups (batches of the call) advanced by one persistent launch, else 1 */
    int32_t clenshaw;      /* bdg_fermi_blocks: 1 = its Clenshaw steps ran the streamed-block kernel (cheb_clenshaw),
                              2 = the dictionary kernel (cheb_clenshaw_dict); 0 = the call was another one */
    int32_t green;         /* bdg_green_moments: 1 = its picked steps ran the streamed-block kernel (cheb_green),
                              2 = the dictionary kernel (cheb_green_dict); 0 = the call was another one */
    int32_t green_ranges;  /* bdg_green_moments, bdg_green_local_moments, bdg_green_state_moments: ranges of moments the
                              device table was filled and copied out in (bdg_green_bond_blocks: filled and contracted in) */
    int32_t green_local;   /* bdg_green_local_moments: 1 = its steps ran the streamed-block kernel (cheb_green_local),
                              2 = the dictionary kernel (cheb_green_local_dict); 0 = the call was another one */
    int32_t apply;         /* bdg_apply_series: 1 = its stored-source Clenshaw steps ran the streamed-block kernel
                              (cheb_clenshaw_vec), 2 = the dictionary kernel (cheb_clenshaw_vec_dict); 0 = the call was
                              another one */
    int32_t green_states;  /* bdg_green_state_moments: 1 = its steps ran the streamed-block kernel (cheb_green_state),
                              2 = the dictionary kernel (cheb_green_state_dict); 0 = the call was another one */
    int32_t green_bonds;   /* bdg_green_bond_blocks: 1 = its steps ran the streamed-block kernel, 2 = the dictionary kernel
                              (cheb_family / cheb_family_dict with GreenBondTail); 0 = the call was another one */
    int32_t roll_chunk;    /* cheb_roll3: plane-steps per unit (RollArgs.chunk) of the last rolling launch of the batch the
                              record describes; 0 = whole-column segments, and 0 when the call did not roll */
    int32_t composed;      /* 1 = the three-step sweeps of the call were composed ones (cheb_sweep3_composed: every launch steps
                              by T_3(H/scale), three array passes per three steps, updating t_{3(k-1)} to t_{3(k+1)} in place;
                              steps_per_launch stays 3 and bytes_per_launch is the three-pass launch); 0 = classic sweeps, or
                              the call was another one.  (response_map moved into what was padding before gemm_ms: the
                              record keeps its size and no other field moved.) */
    int32_t response_map;  /* bdg_response_map: 1 = the call was this one, 0 = another one */
    double gemm_ms;        /* bdg_response_map: HIP-event time of its product launches (resp_gemm) */
    double gemm_flops;     /* bdg_response_map: 8 x n_moments^2 x K summed over the chunks of sites and the kernels, K = 4 x
                              padded columns x sites of the chunk complex entries per panel row */
    int32_t green_probe;   /* bdg_green_probe_blocks: 1 = its steps ran the streamed-block kernel, 2 = the dictionary kernel
                              (cheb_family / cheb_family_dict with GreenBondTail); 0 = the call was another one.  (The newest
                              field: with `correlation` it fills the eight bytes before gram_ms, four of which were padding -
                              the record keeps its size, `correlation` moved by four bytes and no other field moved.) */
    int32_t correlation;   /* bdg_moment_matrix: 1 = the call was this one, 0 = another one */
    double gram_ms;        /* bdg_moment_matrix: HIP-event time of its Gram + reduce launches (corr_gram, corr_reduce) */
    double gram_flops;     /* bdg_moment_matrix: 8 x rows of X x rows of Y x K summed over the Gram launches, K = 4 nb x
                              lanes_per_row complex entries per panel row */
} bdg_perf;

const char* bdg_last_error(void);
const char* bdg_version(void);

/* Number of visible HIP devices (0 is a valid answer and not an error). */
int bdg_device_count(int* count);

/*
 * Upload a BSR matrix with 4x4 complex128 blocks (replaces the host->device
 * copy `cp.asarray(H)` of hamiltonian.py:214 / :295, but for the sparse form).
 *   nb      number of block rows (lattice sites)
 *   nnzb    number of stored blocks
 *   indptr  int32[nb+1], indices int32[nnzb] (column block per stored block)
 *   data    double[nnzb*32]: blocks in C order data[k][row][col] (re, im)
 * The triple must be canonical (sorted, no duplicates); validated on the host.
 */
int bdg_create(int device, int64_t nb, int64_t nnzb, const int32_t* indptr,
               const int32_t* indices, const double* data, bdg_system** out);
int bdg_destroy(bdg_system* sys);

/*
 * Row-slab variant (domain decomposition over lattice planes, one slab per GPU): the
 * handle owns block rows [row_offset, row_offset + nb) of the global matrix.  Column ids
 * are LOCAL: 0..nb-1 are the owned rows, nb..ncols-1 are halo rows whose t_n entries are
 * refreshed from other slabs before every recurrence launch.  Start vectors are indexed
 * globally, so the result does not depend on how the rows are cut.  bodge_amd/slab.py
 * derives these arrays from the global BSR triple.
 */
int bdg_create_slab(int device, int64_t nb, int64_t ncols, int64_t nnzb, const int32_t* indptr,
                    const int32_t* indices, const double* data, int64_t row_offset,
                    bdg_system** out);
/*
 * Exchange lists of a slab.  For peer p: send_count[p] owned rows (local ids, concatenated
 * in send_rows) go to it and recv_count[p] rows arrive from it into local columns
 * recv_col[p] .. recv_col[p]+recv_count[p]-1.  peer_rank[p] is an RCCL rank when `comm` is
 * given (one process per GPU: grouped ncclSend/ncclRecv per launch), or a member index of a
 * bdg_group when comm is NULL (one process driving several slabs: device-to-device copies).
 */
int bdg_slab_set_exchange(bdg_system* sys, bdg_comm* comm, int32_t n_peers, const int32_t* peer_rank,
                          const int64_t* send_count, const int64_t* send_rows,
                          const int64_t* recv_col, const int64_t* recv_count);
/* Same-process group of slabs: the dot products returned are summed over the members. */
int bdg_group_create(bdg_system** members, int32_t n_members, bdg_group** out);
int bdg_group_destroy(bdg_group* group);
int bdg_group_dots_random(bdg_group* group, double scale, int32_t n_steps, int32_t n_vectors,
                          uint64_t seed, uint64_t first_vec_id, int32_t vec_kind,
                          double* d_out, double* e_out);
int bdg_group_dots_unit(bdg_group* group, double scale, int32_t n_steps, int32_t n_vectors,
                        const int64_t* rows, double* d_out, double* e_out);

/* y = H x for one host vector of 4*nb complex entries (site-major, the order
 * of `H @ x` on the reference's matrix).  For parity tests. */
int bdg_spmv(bdg_system* sys, const double* x, double* y);

/*
 * Chebyshev recurrence on `n_vectors` start vectors advanced together:
 *   t_0 = v,  t_1 = H t_0 / scale,  t_{n+1} = 2 H t_n / scale - t_{n-1}
 *   d[n*n_vectors + r] = <t_n|t_n>,  e[n*n_vectors + r] = Re <t_{n+1}|t_n>,  n < n_steps
 * `scale` must bound the spectrum of H.  Random start vectors are generated on
 * the device from (seed, first_vec_id + r, element index); unit start vectors
 * are e_{rows[r]} (rows index the 4*nb scalar rows).
 */
int bdg_cheb_dots_random(bdg_system* sys, double scale, int32_t n_steps, int32_t n_vectors,
                         uint64_t seed, uint64_t first_vec_id, int32_t vec_kind,
                         double* d_out, double* e_out);
int bdg_cheb_dots_unit(bdg_system* sys, double scale, int32_t n_steps, int32_t n_vectors,
                       const int64_t* rows, double* d_out, double* e_out);

/*
 * Moments mu_m = sum_r <v_r|T_m(H/scale)|v_r>, m < n_moments (even), from the
 * dots above via mu_2n = 2 d_n - mu_0, mu_2n+1 = 2 e_n - mu_1.  If `comm` is
 * non-null the moment vector is summed over all ranks with one RCCL
 * all-reduce before it is returned (each rank passes its own first_vec_id).
 */
int bdg_cheb_moments(bdg_system* sys, bdg_comm* comm, double scale, int32_t n_moments,
                     int32_t n_vectors, uint64_t seed, uint64_t first_vec_id, int32_t vec_kind,
                     double* mu_out);
/*
 * Blocks of the density matrix F = f(H) = sum_k coef[k] T_k(H/scale) on a block pattern, by probing
 * (DESIGN.md §10).  site_colour[i] in [0, n_colours) colours the nb block rows (a negative colour leaves
 * the site out of this call); the probe vector of colour c and Nambu component b is the sum of the unit
 * vectors e_{4i+b} over the sites i of colour c, and f(H) applied to it (Clenshaw's recurrence, one launch
 * per coefficient) gives column b of every pattern block whose column site has colour c:
 *   blocks_out[((k*4 + a)*4 + b)*2 + {0, 1}] = (re, im) of [f(H) r_{c b}][4j + a]
 * for block k = (block row j, column pat_indices[k]) of the pattern (pat_indptr[nb + 1], canonical order,
 * any subset of block pairs).  Exact when two sites of one colour are farther apart in the graph of H
 * than the expansion reaches; otherwise the blocks carry the contributions of the other sites of the
 * colour.  n_components = 4 computes all columns, 2 the electron columns b = 0, 1 only (the caller
 * derives the others from particle-hole symmetry; columns 2, 3 are then returned as 0).  Colours are
 * batched (whole colours, up to 64 probe vectors per launch) on the handle's stream sets; bdg_perf_query
 * reports the call (`clenshaw` says which kernel form ran).  Whole matrices only (not slabs).
 */
int bdg_fermi_blocks(bdg_system* sys, double scale, int32_t n_moments, const double* coef, int32_t n_colours,
                     const int32_t* site_colour, int32_t n_components, const int32_t* pat_indptr,
                     const int32_t* pat_indices, double* blocks_out);

/*
 * A Chebyshev series of H applied to caller-supplied vectors:
 *   y[v, f] = sum_k coef[k, f] T_k(H/scale) x_v,   k < n_moments, f < n_functions, v < n_vectors
 * coef[(k*n_functions + f)*2 + {0, 1}] = (re, im) of the complex coefficient c_k of function f (c_0 as it enters
 * the sum, not doubled); x holds n_vectors vectors of 4*nb complex entries one after the other (site-major, the
 * order of bdg_spmv); y_out + (v*n_functions + f)*8*nb receives the 4*nb complex entries of y[v, f].  The pairs
 * (v, f) are the columns of Clenshaw's recurrence with a stored source, b_k = 2 H b_{k+1}/scale - b_{k+2} +
 * c_k[f] x_v, one launch per coefficient (kernels cheb_clenshaw_vec / cheb_clenshaw_vec_dict, no dot products).
 * A real matrix runs in real arithmetic with complex vectors and coefficients all the same: the two slots of a
 * real kernel's lane payload carry Re and Im of one column.  Columns are batched by the width rule of the
 * one-step kernels (one vector buffer within 96 MB, at most 64 columns, 32 in real arithmetic;
 * bdg_set_lanes_per_row fixes the lanes = columns per batch) on the handle's stream sets.  bdg_perf_query
 * reports the call: `apply` says which kernel form ran, vectors_per_launch counts a column of real arithmetic
 * as two vectors (as bytes_per_launch does), vector_steps counts columns, and window_ms spans the batches'
 * transfers between rounds when there are more batches than streams.  Whole matrices only (not slabs).
 */
int bdg_apply_series(bdg_system* sys, double scale, int32_t n_moments, int32_t n_functions, const double* coef,
                     int32_t n_vectors, const double* x, double* y_out);

/* A BSR operator with its own pattern on the block rows of a system: indptr int32[nb + 1], indices int32[nnzb],
 * data double[nnzb*32]: nnzb blocks of 4x4 complex128 in C order data[k][row][col] (re, im), scipy BSR order. */
typedef struct bdg_operator {
    int32_t nnzb;
    const int32_t* indptr;
    const int32_t* indices;
    const double* data;
} bdg_operator;

/*
 * Double Chebyshev moments of two operators:
 *   mu_out[(n*n_moments + m)*2 + {0, 1}] = (re, im) of sum_v <v|T_n(H/scale) A T_m(H/scale) B|v>,   n, m < n_moments
 * over n_vectors start vectors: the unit vectors e_{rows[v]} (rows index the 4*nb scalar rows), or the caller's
 * vectors x (n_vectors vectors of 4*nb complex entries one after the other, site-major, the order of bdg_spmv);
 * exactly one of rows / x is given, the other is NULL.  The start vectors are the columns of batches of the width
 * rule of bdg_apply_series (bdg_set_lanes_per_row fixes the lanes = columns per batch).  Per batch two recurrences
 * run on the handle's stream through the stored-source kernels of bdg_apply_series with a zero coefficient,
 * X_n = T_n |r> and Y_m = A T_m B |r> (corr_operator applies A and B), into two panels of rows of
 * K = 4*nb*lanes complex entries, and corr_gram (fp64 MFMA) forms P[s][n][m] = sum_{k in slice s} conj(X_n[k]) Y_m[k]
 * on slices of BODGE_AMD_CORRELATION_SLICE entries (default 4096, a multiple of 4), which corr_reduce sums into mu in
 * ascending order: no atomics, the same bits from run to run.  The panels hold Mb <= n_moments rows each, the
 * largest multiple of 64 (or n_moments itself) for which both stay within BODGE_AMD_CORRELATION_BYTES (default
 * 4 GiB); with Mb < n_moments the moments are blocked (Y once, chunk after chunk; X again for every chunk of Y), and
 * a batch too wide for Mb = 64 is narrowed down to 4 lanes before the call gives up with BDG_EINVAL and the bytes
 * needed.  Argument errors come before any device call, in this order: counts < 1, scale <= 0, null pointers, both
 * or neither of rows / x, an operator with a negative count or null arrays, null handle, an operator whose
 * indptr[nb] disagrees with its block count or whose indices leave [0, nb) (the matrix size comes from the
 * handle), slab.  bdg_perf_query reports the call: correlation = 1, launches = recurrence launches (per batch and
 * pass M - 1 steps of Y, and M of X: its restart from the kept start batch is one), vector_steps = columns x
 * launches, gram_ms and gram_flops.  Whole matrices only (not slabs).
 */
int bdg_moment_matrix(bdg_system* sys, double scale, int32_t n_moments, const bdg_operator* a, const bdg_operator* b,
                      int32_t n_vectors, const int64_t* rows, const double* x, double* mu_out);

/*
 * One operator's response at every site.  For A with support on the S = n_source_rows distinct scalar
 * rows `source_rows` (1 <= S <= 32; a[(al*S + be)*2 + {0, 1}] = (re, im) of A between rows source_rows[al] and
 * source_rows[be], no symmetry assumed) and n_kernels coefficient matrices coef[((q*n_moments + n)*n_moments + m)*2 +
 * {0, 1}] = (re, im) of c_q[n][m] (as chebyshev_coefficients_2d returns them), with X_n = T_n(H/scale) E on the unit
 * columns E of the source rows:
 *   out[(((q*n_sites + s)*4 + g)*4 + d)*2 + {0, 1}] = (re, im) of
 *       K_{q,j_s}[g][d] = sum_nm c_q[n][m] sum_{al,be} A[al][be] conj(X_m[4 j_s + g][be]) X_n[4 j_s + d][al]
 * for the distinct block rows j_s = block_rows[s] in any order (the source may be among them), so that
 * sum_{g,d} B[g][d] K[g][d] = sum_ab A_ab (B_j)_ba F_q(E_a, E_b) for any 4x4 operator B on site j: a plain trace, no
 * factor 1/2.  The columns run through the stored-source kernels of bdg_apply_series with a zero coefficient, padded
 * with zero columns to whole batches of the width rule (bdg_set_lanes_per_row fixes the lanes); after every step
 * resp_pick gathers the rows of a chunk of sites into row n of a panel X (site-major), resp_gemm (fp64 MFMA) forms
 * Z_q = c_q^T X and resp_contract sums a site's 16 entries over m and the columns: n ascending, then m ascending, no
 * atomics - the same bits from run to run and however the sites are chunked.  X and Z hold n_moments rows each; a
 * chunk is all sites, or the largest multiple of 16 sites for which both stay within BODGE_AMD_CORRELATION_BYTES
 * (default 4 GiB), and every chunk reruns the recurrence; if 16 sites do not fit the call returns BDG_EINVAL with the
 * bytes needed.  Argument errors come before any device call, in this order: counts < 1, S > 32, scale <= 0, null
 * pointers, null handle, source rows or block rows out of range or repeated, slab.  bdg_perf_query reports the call:
 * response_map = 1, launches = chunks x batches x (n_moments - 1), vector_steps = columns x launches, gemm_ms and
 * gemm_flops.  Ends a Lanczos run or a subspace block on the handle.  Whole matrices only (not slabs).
 */
int bdg_response_map(bdg_system* sys, double scale, int32_t n_moments, int32_t n_source_rows, const int64_t* source_rows,
                     const double* a, int32_t n_kernels, const double* coef, int32_t n_sites, const int32_t* block_rows,
                     double* out);

/*
 * Off-diagonal Chebyshev moments for the Green's function blocks G_ji:
 *   out[(((n*n_targets + t)*4 + a)*n_sources + v)*2 + {0, 1}] = (re, im) of <e_{4j_t + a}|T_n(H/scale)|e_{source_rows[v]}>
 * for n < n_moments, j_t = target_block_rows[t] (distinct block rows), a < 4.  Every source row is a unit
 * start vector of the recurrence t_{n+1} = 2 H t_n / scale - t_{n-1}; one launch per moment advances the
 * vectors and stores the rows of the target sites (kernels cheb_green / cheb_green_dict, no dot products).
 * The source rows are batched by the width rule of the one-step kernels and run on the handle's stream.  On
 * the device the table covers a range of moments of at most 256 MB (BODGE_AMD_GREEN_TABLE_BYTES) that is
 * copied into `out` when it is full, so device memory does not grow with n_moments.  bdg_perf_query reports
 * the call (`green` says which kernel form ran).  Whole matrices only (not slabs).
 */
int bdg_green_moments(bdg_system* sys, double scale, int32_t n_moments, int32_t n_sources, const int64_t* source_rows,
                      int32_t n_targets, const int32_t* target_block_rows, double* out);

/*
 * Local Chebyshev moments at many sites per batch, for maps of the local Green's function blocks G_jj
 * (DESIGN.md §12):
 *   out[(((n*n_sites + s)*4 + a)*n_components + b)*2 + {0, 1}] = (re, im) of <e_{4j_s + a}|T_n(H/scale)|e_{4j_s + b}>
 * for n < n_moments, j_s = block_rows[s] (distinct block rows), a < 4, b < n_components (2: the electron
 * columns, 4: all).  The unit vectors of up to 64 / n_components sites share one batch of the one-step width
 * rule (bdg_set_lanes_per_row fixes the lanes); one launch per moment advances all of them, and on the rows
 * of a site only the vectors that started there store (kernels cheb_green_local / cheb_green_local_dict: one
 * writer per entry, no dot products).  The device table covers a range of moments of at most 256 MB
 * (BODGE_AMD_GREEN_TABLE_BYTES), copied into `out` when it is full.  bdg_perf_query reports the call
 * (`green_local` says which kernel form ran).  Whole matrices only (not slabs).
 */
int bdg_green_local_moments(bdg_system* sys, double scale, int32_t n_moments, int32_t n_sites,
                            const int32_t* block_rows, int32_t n_components, double* out);

/*
 * Green's function blocks on a pattern of block pairs, every column site a source:
 *   out[(((e*nnz + k)*4 + a)*4 + b)*2 + {0, 1}] = (re, im) of sum_n w[e][n] <e_{4j + a}|T_n(H/scale)|e_{4i + b}>
 * for e < n_weights, the pattern block k = (block row j, column pat_indices[k]) with i = pat_indices[k], nnz =
 * pat_indptr[nb], a, b < 4, and the weights weights[(e*n_moments + n)*2 + {0, 1}] = (re, im) of w[e][n] (for G(z_e):
 * the series weights of the resolvent).  The pattern is a BSR skeleton as in bdg_fermi_blocks, any subset of block
 * pairs in canonical order (columns ascending within a row, no duplicates); the column sites of the call are the
 * distinct entries of pat_indices.  The unit vectors of up to 64 / n_components column sites share one batch of the
 * one-step width rule (bdg_set_lanes_per_row fixes the lanes), n_components = 2 (the electron columns; the hole
 * columns follow from mu_n[a][b] = (-1)^n conj mu_n[a^2][b^2] on the same block, right for a particle-hole symmetric
 * matrix only) or 4.  One launch per moment advances all vectors, and on block row j the vectors of site i store
 * their entries of every pattern block (j, i) (kernels cheb_family / cheb_family_dict with GreenBondTail: one writer
 * per entry).  The moments stay on the device: the table covers a range of moments of at most 256 MB
 * (BODGE_AMD_GREEN_TABLE_BYTES), and when it is full green_bond_contract adds the range to the result in ascending n,
 * one chain of FMAs per entry, no atomics - the same bits from run to run and however the moments are cut into
 * ranges.  Only `out` leaves the device.  Argument errors come before any device call, in this order: counts < 1
 * (n_moments, n_weights; n_weights above 262140), scale <= 0, null pointers, null handle, a pattern whose indptr does
 * not start at 0 or is not monotone, that has no block, whose indices leave [0, nb) or are not in canonical order,
 * n_components not 2 or 4, slab.  bdg_perf_query reports the call: green_bonds says which kernel form ran, launches =
 * batches x (n_moments - 1), kernel_ms the recurrence launches, window_ms the whole of recurrence and contractions
 * (window_ms - kernel_ms = the contractions' time).  Ends a Lanczos run or a subspace block on the handle.  Whole
 * matrices only (not slabs).
 */
int bdg_green_bond_blocks(bdg_system* sys, double scale, int32_t n_moments, int32_t n_weights, const double* weights,
                          const int32_t* pat_indptr, const int32_t* pat_indices, int32_t n_components, double* out);

/*
 * Green's function blocks on a pattern of block pairs by probing: one start vector per colour of sites
 * and Nambu column where bdg_green_bond_blocks has one per column site and Nambu column.  site_colour[i] < n_colours is
 * the caller's colour of block row i (negative: the site is no source), signs[s*nb + i] = xi_i = +1 or -1 the sign of
 * site i in sample s < n_samples (NULL: all +1, n_samples must be 1).  Per sample, for the pattern block k = (j, i)
 * with c = site_colour[i] >= 0,
 *   x_s[e][k][a][b] = xi_i * sum_n w[e][n] [T_n(H/scale) r_{c b}][4j + a],   r_{c b} = sum_{i': colour(i') = c} xi_i' e_{4i' + b}
 * - the block G_ji plus xi_i xi_i' G_ji' of the other sites i' of the colour; a block whose column site has a negative
 * colour is returned as 0.  mean_out, in the layout of bdg_green_bond_blocks' out, is the mean of x_s over the samples;
 * stderr_out (NULL allowed, same layout) holds sqrt(sum_s (x_s - mean)^2 / (S (S - 1))) of the real parts in its real
 * part and of the imaginary parts in its imaginary part, zeros for one sample.  Weights, pattern and n_components as
 * for bdg_green_bond_blocks; the hole-column rule holds term by term because the signs are real.  A batch of the
 * one-step width rule holds the vectors of 64 / n_components whole colours or a power of two less (bdg_set_lanes_per_row
 * fixes the lanes); green_probe_start writes the start vectors, the launches, the pick of moment 0 and the contraction
 * are those of bdg_green_bond_blocks with the colour of a block's column site where that call has the site's position
 * (kernels cheb_family / cheb_family_dict with GreenBondTail: one writer per entry, because a pattern row may hold a
 * colour only once).  After a sample's last contraction green_probe_accumulate folds it into mean and squared deviations
 * on the device (Welford: delta = x - mean, mean += delta / s, M2 += delta (x - mean); one thread per entry, no atomics;
 * one sample returns x bit for bit).  The device table covers a range of moments of at most 256 MB
 * (BODGE_AMD_GREEN_TABLE_BYTES).  Argument errors come before any device call, in this order: counts (n_moments,
 * n_weights < 1; n_weights above 262140; n_colours < 1; n_samples < 1), scale <= 0, null pointers (signs == NULL with
 * n_samples > 1 after the others), null handle, a pattern whose indptr does not start at 0 or is not monotone, that has
 * no block, whose indices leave [0, nb) or are not in canonical order, n_components not 2 or 4, a colour >= n_colours, a
 * sign that is not +1 or -1, a pattern row that holds two column sites of one colour (the message names the row), slab,
 * a batch of 2^31 / 16 blocks or more (the table is indexed with 32 bits).  bdg_perf_query reports the call: green_probe
 * says which kernel form ran, launches = n_samples x colour batches x (n_moments - 1), kernel_ms the recurrence launches,
 * window_ms the whole.  Ends a Lanczos run or a subspace block on the handle.  Whole matrices only (not slabs).
 */
int bdg_green_probe_blocks(bdg_system* sys, double scale, int32_t n_moments, int32_t n_weights, const double* weights,
                           int32_t n_colours, const int32_t* site_colour, int32_t n_samples, const int8_t* signs,
                           const int32_t* pat_indptr, const int32_t* pat_indices, int32_t n_components, double* mean_out,
                           double* stderr_out);

/*
 * The argument checks of bdg_green_probe_blocks from "a pattern whose indptr ..." to "two column sites of one colour",
 * in that order, for a matrix of nb block rows: on the host, without a handle or a device (after nb, n_colours,
 * n_samples < 1, null pointers and signs == NULL with n_samples > 1).  0 or BDG_EINVAL with the same messages.  For
 * tests and for callers that want to validate colours and signs before they create a handle; the Python package itself
 * does not call it, and bdg_green_probe_blocks runs the same function.
 */
int bdg_host_probe_check(int64_t nb, int32_t n_colours, const int32_t* site_colour, int32_t n_samples, const int8_t* signs,
                         const int32_t* pat_indptr, const int32_t* pat_indices, int32_t n_components);

/*
 * Chebyshev moments of the resolvent between extended states, for G(eps) in plane waves, wave packets or orbitals
 * (DESIGN.md §16).  A state q is one complex amplitude per site, amplitudes[(q*nb + j)*2 + {0, 1}] = (re, im) of
 * w_q[j] in site-index order; its Nambu vectors are |w_q b> = sum_j w_q[j] e_{4j + b}.
 *   out[((((n*n_states + q)*4 + a)*n_components + b)*2 + {0, 1}] = (re, im) of <w_q a|T_n(H/scale)|w_q b>
 * for n < n_moments, a < 4, b < n_components (2: the electron columns, 4: all).  A lane payload is one complex
 * column in every arithmetic mode (as for bdg_apply_series): a batch holds the columns of up to 64 / n_components
 * states (32 / n_components in real arithmetic) by the one-step width rule (bdg_set_lanes_per_row fixes the lanes).
 * One launch per moment advances all of them and projects t_{n+1} on the states (kernels cheb_green_state /
 * cheb_green_state_dict: one partial per workgroup, no atomics); green_state_reduce sums the partials of a range of
 * moments in a fixed order.  Partials and table of a range take at most 256 MB (BODGE_AMD_GREEN_TABLE_BYTES); the
 * table is copied into `out` when the range is full.  bdg_perf_query reports the call (`green_states` says which
 * kernel form ran).  Whole matrices only (not slabs).
 */
int bdg_green_state_moments(bdg_system* sys, double scale, int32_t n_moments, int32_t n_states,
                            const double* amplitudes, int32_t n_components, double* out);

/* Per-start-vector moments for unit vectors: mu_out[m*n_vectors + r]. */
int bdg_cheb_diag_moments(bdg_system* sys, double scale, int32_t n_moments, int32_t n_vectors,
                          const int64_t* rows, double* mu_out);

/*
 * Lanczos process on H^2 (eigenvalues of H closest to zero, i.e. the excitation gap, for
 * matrices beyond dense reach).  `begin` prepares n_vectors (<= 64) independent processes from
 * counter-based start vectors; `advance` runs n_iter more iterations and returns, per
 * iteration j and vector r, alpha[j*n_vectors + r] = <v_j|H^2|v_j> and
 * beta[j*n_vectors + r] = beta_{j+1} (the tridiagonal matrix of H^2 in the Lanczos basis;
 * its lowest eigenvalues converge to the squares of the smallest |eigenvalues| of H).
 * At most max_iter iterations in total.  Whole matrices only (not slabs).
 */
int bdg_lanczos_begin(bdg_system* sys, int32_t n_vectors, uint64_t seed, uint64_t first_vec_id,
                      int32_t vec_kind, int32_t max_iter);
int bdg_lanczos_advance(bdg_system* sys, int32_t n_iter, double* alpha_out, double* beta_out);
/*
 * Ritz vectors by a second pass: on a freshly begun process (same arguments as the first pass:
 * the Lanczos vectors v_j are reproduced bit for bit) run n_iter iterations and accumulate
 *   y[l][r] = sum_j coef[(j*n_levels + l)*n_vectors + r] * v_j^{(r)},   l < n_levels,
 * the eigenvector estimates of H^2 whose coordinates in the Lanczos basis the caller computed
 * from alpha/beta.  y_out[(l*n_vectors + r)*8*nb ...] receives 4*nb complex entries (site-major)
 * per (level, start vector).  With eigenvalue eps, (H + eps) y is an eigenvector of H.
 */
int bdg_lanczos_ritz_vectors(bdg_system* sys, int32_t n_iter, int32_t n_levels, const double* coef,
                             double* y_out);

/*
 * Eigenpairs from the same second pass without the Ritz block leaving the device (Rayleigh-Ritz with H
 * on the GPU; what a caller of diagonalize() wants from a lattice too large to diagonalise: reference
 * tests/test_physics.py:105, `eigvals, eigvecs = system.diagonalize()`).  Arguments as for
 * bdg_lanczos_ritz_vectors, plus eps[l] = the level's eigenvalue estimate (square root of the converged
 * Ritz value of H^2).  Per level the candidates (H + eps_l) y span the +eps_l eigenspace; the rank of
 * their Gram matrix (eigenvalues above rank_tol x the largest) is the multiplicity; H is diagonalised
 * inside that span.  n_out receives the number of states found over all levels; the max_out lowest are
 * returned: values_out[k] ascending, vectors_out + 8*nb*k = 4*nb complex entries (site-major) of state k.
 * At most 16 columns (16 real-arithmetic or 16 complex start vectors).  Ends the Lanczos run.
 */
int bdg_lanczos_ritz_pairs(bdg_system* sys, int32_t n_iter, int32_t n_levels, const double* coef,
                           const double* eps, double rank_tol, int32_t max_out, int32_t* n_out,
                           double* values_out, double* vectors_out);

/*
 * A block of vectors that stays on the device (filtered subspace iteration).  The block is two arrays
 * X and HX of n_columns columns, vector-major: column c is 4*nb contiguous complex entries in the order of bdg_spmv.
 * A third array of the same size takes the out-of-place rotations.  The block hangs off the handle; a dense solve
 * (bdg_eigh_dense, bdg_eigh_dense_above) or bdg_lanczos_begin on the handle ends it (they need the memory), and
 * every later bdg_subspace_* call but `begin` and `end` then returns BDG_EINVAL with a message, as it does when
 * `begin` was never called.  A failed allocation is reported (BDG_ENOMEM) and not retried: the handle is left
 * without a block.  Whole matrices only: slabs return BDG_EINVAL.
 *
 *   begin    allocate for n_columns <= 4096 columns; X[c] = the Rademacher start vector (seed, first_vec_id + c) of
 *            bdg_random_vector, HX = 0.  Replaces a block the handle already has.
 *   end      free the block (no error if there is none).
 *   filter   X <- sum_k coef[k] T_k(H/scale) X, k < n_moments, real coefficients, c_0 as it enters the sum: the
 *            stored-source Clenshaw kernels and the batching of bdg_apply_series, a batch's staging buffer filled
 *            from and emptied to the block instead of the host.  bdg_perf_query reports it like bdg_apply_series.
 *   project  HX <- H X (one step of the same kernels), then s_out = X^† X and g_out = X^† HX, n_columns x n_columns
 *            complex each, row-major (entry [n][m] = sum_k conj(X[n][k]) Y[m][k]): corr_gram on slices of 4096
 *            entries, corr_reduce over the slices in ascending order, no atomics.
 *   rotate   X <- X Q and HX <- HX Q for q = Q, n_columns x n_out complex, row-major (out[j][k] = sum_b Q[b][j]
 *            X[b][k]; kernel subspace_rotate, fp64 MFMA), then residual_out[j] = |HX_j - theta[j] X_j|_2, j < n_out
 *            (subspace_residual: one partial per workgroup and column; subspace_residual_reduce: their sum in
 *            ascending order).  Columns >= n_out are dead afterwards (finite, but unspecified) until refilled.
 *   refill   X[first_column + c] = start vector (seed, first_vec_id + c), c < count.  HX is not touched.
 *   read     `count` columns of X from first_column on to out (count * 4*nb complex entries).
 *   write    the same columns from x.
 */
int bdg_subspace_begin(bdg_system* sys, int32_t n_columns, uint64_t seed, uint64_t first_vec_id);
int bdg_subspace_end(bdg_system* sys);
int bdg_subspace_filter(bdg_system* sys, double scale, int32_t n_moments, const double* coef);
int bdg_subspace_project(bdg_system* sys, double* s_out, double* g_out);
int bdg_subspace_rotate(bdg_system* sys, int32_t n_out, const double* q, const double* theta, double* residual_out);
int bdg_subspace_refill(bdg_system* sys, int32_t first_column, int32_t count, uint64_t seed, uint64_t first_vec_id);
int bdg_subspace_read(bdg_system* sys, int32_t first_column, int32_t count, double* out);
int bdg_subspace_write(bdg_system* sys, int32_t first_column, int32_t count, const double* x);

/* Write the counter-based start vector (4*nb complex entries) to a host buffer. */
int bdg_random_vector(bdg_system* sys, uint64_t seed, uint64_t vec_id, int32_t vec_kind,
                      double* v_out);

/*
 * Dense Hermitian eigensolve of the uploaded matrix on the GPU (replaces
 * cupy.linalg.eigvalsh / eigh at hamiltonian.py:295 / :215): all 4*nb
 * eigenvalues ascending in w_out; if z_out is non-null it receives the
 * eigenvectors in column-major (Fortran) order: eigenvector n occupies the
 * 4nb complex entries starting at z_out[2*n*4nb].
 * Drivers.  Eigenvalues only (z_out NULL, what free_energy needs): own Householder
 * tridiagonalisation + bisection from 4*nb > 512 on (no library; real arithmetic when imag(H) = 0),
 * own Jacobi kernels below.  With eigenvectors: own one-sided Jacobi kernels for 4*nb <= 2048 (and
 * up to 4096 for as long as the rocSOLVER object is still being read from cold storage, see
 * bdg_dense_prefetch); above, rocSOLVER dsyevd when imag(H) = 0 (real eigenvectors, widened to
 * complex in z_out) and zheevd otherwise; limit 4*nb <= 46000.  Results are scanned for non-finite
 * values on the device.
 */
int bdg_eigh_dense(bdg_system* sys, double* w_out, double* z_out);

/*
 * What diagonalize() keeps (hamiltonian.py:235-238: the eigenpairs with eigenvalue > 0): all 4*nb
 * eigenvalues ascending in w_out, and the eigenvectors of those above `lower_bound` only - vector m of
 * them (ascending) in the 4*nb complex entries from z_out + 8*nb*m; *n_vectors = their number.  If it
 * exceeds `capacity` (vectors z_out has room for) BDG_EINVAL is returned with *n_vectors set and z_out
 * untouched.  Route from 4*nb > 512 on, no library involved: Householder tridiagonalisation, bisection,
 * inverse iteration on the tridiagonal matrix (close eigenvalues orthogonalised against each other) and
 * back-transformation by the stored reflectors - half the vectors of the full solve for a BdG matrix.
 * Below, and when BODGE_AMD_EIGH names another driver, bdg_eigh_dense runs and its result is cut.
 */
int bdg_eigh_dense_above(bdg_system* sys, double lower_bound, int64_t capacity, double* w_out,
                         int64_t* n_vectors, double* z_out);

/*
 * max |H - H^†| over the stored entries of the uploaded matrix, computed on the device: the
 * Hermiticity test the reference makes on the host when a `with` block closes
 * (hamiltonian.py:121-122, `abs(M - M.getH()).max() > 1e-6` -> RuntimeError).  Whole matrices only.
 */
int bdg_hermiticity_defect(bdg_system* sys, double* defect_out);

/*
 * Host-side assembly helpers: CPU threads only, no device call, usable without a GPU.  They make
 * the passes over the BSR blocks that precede bdg_create with every core instead of one.
 *
 * bdg_host_fill_terms: scatter `count` 2x2 complex spin matrices (`values`: 8 doubles each if
 *   per_term, else one matrix used for every term) into blocks `ids[n]` of `data` (nnzb x 4 x 4
 *   complex128), in term order.  kind 0: hopping H_ij -> blk[0:2,0:2] = v, blk[2:4,2:4] = -conj(v)
 *   (hamiltonian.py:106-108); kind 1: pairing Δ_ij -> blk[0:2,2:4] = v (:112-113); kind 2: the
 *   transposed block of a pairing term, blk[2:4,0:2] = v^† (:115-116).  `touched` (nnzb bytes or
 *   NULL) gets 1 at every block written.
 * bdg_host_scan_blocks: one read of every block.  nonzero[k] = block k has a non-zero entry (the
 *   blocks `matrix("bsr")` keeps, :142-143); ph_defect = max |blk[2:4,2:4] + conj(blk[0:2,0:2])|,
 *   |blk[2:4,0:2] + conj(blk[0:2,2:4])| (0 = spectrum symmetric about zero); row_sum_max = max
 *   over scalar rows of Σ|H_rc| (Gershgorin bound); all_real = imag(data) == 0.  Any output may
 *   be NULL.  A NaN entry makes both floating-point results NaN.
 * bdg_host_compact_blocks: the BSR triple without the blocks whose keep[k] is 0; outputs are
 *   caller-allocated (indptr_out nb+1, the others n_nonzero long).
 */
int bdg_host_fill_terms(double* data, int64_t nnzb, const int64_t* ids, int64_t count, const double* values,
                        int per_term, int kind, uint8_t* touched);
int bdg_host_scan_blocks(const double* data, const int32_t* indptr, int64_t nb, uint8_t* nonzero, int64_t* n_nonzero,
                         double* ph_defect, double* row_sum_max, int32_t* all_real);
int bdg_host_compact_blocks(const double* data, const int32_t* indices, const int32_t* indptr, int64_t nb,
                            const uint8_t* keep, double* data_out, int32_t* indices_out, int32_t* indptr_out);

/*
 * Host arithmetic of the composed three-step sweep (bdg_perf.composed; CPU only, no device call, usable without a
 * GPU).  Such a run steps by T_3(H/scale): sweep k starts from u = t_{3k} and makes w_j = T_j(H/scale) u =
 * (t_{3k+j} + t_{3k-j}) / 2, and row n = 3k + j of its dot table holds <w_j|w_j>, Re <w_{j+1}|w_j> instead of d_n, e_n.
 * This function turns such a table back:  raw[n * raw_stride + 2 * r + {0, 1}] are the two products of row n < n_steps
 * and vector r < n_vectors (raw_stride >= 2 * n_vectors doubles per row); d_out / e_out [n * ld + r] receive
 * <t_n|t_n> and Re <t_{n+1}|t_n> (ld >= n_vectors).  Every new moment is a measured product minus older moments, so
 * rounding errors add and are not amplified; d_{3k} is handed through bit for bit.  Any n_steps >= 1.
 */
int bdg_host_composed_dots(int32_t n_steps, int32_t n_vectors, const double* raw, int64_t raw_stride, double* d_out,
                           double* e_out, int64_t ld);

/*
 * Optional: start reading the rocSOLVER / rocBLAS shared objects into the page cache on a
 * background thread (file I/O only; returns at once, idempotent).  The first dense eigensolve
 * above 4*nb = 2048 loads a 931 MB library, which takes minutes from cold storage; a caller who
 * knows it will diagonalize (the reference's diagonalize() / free_energy() call sites,
 * hamiltonian.py:203-232, :282-302) calls this when the Hamiltonian is created so that the read
 * overlaps with assembly and upload.  bdg_eigh_dense waits for it.
 */
int bdg_dense_prefetch(void);
/* Wait up to timeout_seconds (negative: until done) for that read; *ready = 1 once it has finished. */
int bdg_dense_prefetch_wait(double timeout_seconds, int32_t* ready);
/* The same for the RCCL shared object (573 MB), which the first bdg_comm_* call loads.  If the
 * dense-solver read has been started too, this one follows it (one stream at a time). */
int bdg_rccl_prefetch(void);
int bdg_rccl_prefetch_wait(double timeout_seconds, int32_t* ready);

int bdg_perf_query(bdg_system* sys, bdg_perf* out);

/*
 * Optional geometry hint: block row i is site (x, y, z) of an lx x ly x lz cubic
 * lattice with i = z + lz*(y + ly*x) (reference lattice.py:108).  Lets the library
 * order its row tiles strip-major so that neighbour re-reads stay in L2.  Pure
 * performance hint: results do not depend on it.  (0,0,0) clears it.
 */
int bdg_set_lattice_shape(bdg_system* sys, int32_t lx, int32_t ly, int32_t lz);

/* Tuning override for experiments: lanes per block row (0 = automatic). */
int bdg_set_lanes_per_row(bdg_system* sys, int32_t lanes);

/*
 * Process-wide override of one of the library's run-time switches (the BODGE_AMD_* names listed
 * in csrc/knobs.hpp and DESIGN.md's appendix): `value` replaces what the environment variable of
 * that name says, value = NULL removes the override.  Thread safe, unlike setenv() next to the
 * getenv() of a running call; tests and bench.py select kernel forms this way.  The defaults
 * are the product: nothing needs to be set in normal use.
 */
int bdg_set_option(const char* name, const char* value);

/*
 * RCCL communicator, one rank per process/GPU.  Rank 0 calls
 * bdg_comm_unique_id and distributes the 128 bytes out of band; every rank
 * then calls bdg_comm_init with the same bytes.
 */
int bdg_comm_unique_id(uint8_t id_out[128]);
int bdg_comm_init(int device, const uint8_t id[128], int32_t n_ranks, int32_t rank,
                  bdg_comm** out);
/* What the communicator really spans: ncclCommCount, this rank, its device ordinal and that
 * device's PCI bus id (e.g. "0000:75:00.0") - for records that must show N distinct GPUs. */
int bdg_comm_info(bdg_comm* comm, int32_t* n_ranks, int32_t* rank, int32_t* device, char pci_bus_id[32]);
int bdg_comm_allreduce_sum(bdg_comm* comm, double* buf, int64_t count);
int bdg_comm_allreduce_max(bdg_comm* comm, double* buf, int64_t count);
int bdg_comm_destroy(bdg_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* BODGE_HIP_H */
