// K3 on the slab twins: sparse x dense sandwich  out = A^T diag(d) B  of an unrestricted product (reference:
// ext/sparse.pyx:211-260 csr_dense_sandwich -> ext/sparse_helpers-tmpl.cpp:23-146).  Three kernels that keep the
// accumulators of a wave's sparse columns in static registers and gather the rows of a dense slab out of LDS:
//   csr_dense_gather_kernel  (slab)  runs of (slab, column) entries, B C- or F-ordered, any alignment
//   csr_dense_ell_kernel     (ell)   interleaved-ELL twin, static iterations with skip masks, 64 dense columns
//   csr_dense_ellw_kernel    (ellw)  the same with lane <-> two dense columns, 128 dense columns per part
// The lane-group and entry-list members of the family are sparse_lg.hip and sparse_ent.hip; the launchers of all five
// share slab_launch.hpp.
#include "common.hpp"
#include "reduce.hpp"
#include "slab_launch.hpp"

namespace tmh {

// =======================================================================================
// K3 (v2)  sparse x dense cross sandwich as a slab-blocked GATHER with static register
// accumulators ("segmented wavefront reduction over column nonzeros").
//
// Format (built once per sparse block, see tabmat_amd/ext/_types.py SlabCsc): rows are cut
// into slabs of SLAB_R rows; inside a slab the nonzeros are ordered by (column, row), so the
// entries of one (slab, column) pair are one contiguous run:
//     vals[e]  value A[k, i]
//     koff[e]  (k - slab*SLAB_R) * 64 * sizeof(F)   -- byte offset of row k in the LDS slab
//     cnt [slab][column]   run length (uint16), columns padded to a multiple of 64
//     gptr[slab][group]    start of the run of column-group `group` (64 columns) in that slab
//
// Kernel: a workgroup of 8 waves owns a range of slabs and a 64-column part of the dense
// operand.  Per slab it stages  dB[k, j] = d[k] * B[k, j0 + j]  (SLAB_R x 64) into LDS with
// coalesced 16-byte loads (double-buffered, one barrier per slab).  Wave w owns sparse
// columns [64 w, 64 w + 64): lane <-> dense column j, and the 64 accumulators
// out[64 w + c, j0 + lane], c = 0..63, are STATIC registers (the column loop is fully
// unrolled), kept for the whole slab range.  Each nonzero costs one ds_read_b64 of the LDS slab
// row and one v_fma_f64; the (value, offset) stream is fetched 64 entries at a time with one
// coalesced vector load and broadcast with v_readlane.  No atomics, no LDS writes in the
// inner loop; partial results are reduced by reduce_partials_kernel.
// =======================================================================================
constexpr int SLAB_R = 128;

constexpr int GATHER_CPW = 32;                      // sparse columns (static accumulators) per wave
constexpr int GATHER_NW = 16;                       // waves per workgroup -> 512 sparse columns
constexpr int GATHER_THREADS = GATHER_NW * 64;

// Stream entries are broadcast to the 64 lanes in two ways: the VALUE through a small per-wave LDS
// ring of 64 doubles (uniform-address ds_read_b64), the ROW OFFSET with v_readlane from the register
// that holds the current 64-entry chunk (lane <-> entry), so that the slab read does not wait for
// an LDS round trip and the LDS sees 4 instead of 6 cycles per nonzero.  The ring / register are
// rewritten in place when their 64 entries are consumed.
#define TM_GATHER_STEP(A, X, LIDX)                                                        \
    const F A = ring[(LIDX)];                                                             \
    const F X = *reinterpret_cast<const F *>(                                             \
        slab + (unsigned)__builtin_amdgcn_readlane((int)kcur, (LIDX)) + lane_off);

// SCALE: the dense slab in LDS holds B unscaled (async global->LDS copy); d is folded into the
// stream value when an entry enters the ring, and entries of rows with d == 0 are redirected to
// an all-zero LDS row so that excluded rows contribute exactly nothing.
// CM: column-major LDS slab (F-ordered B): the stream's row offset row * 64 * sizeof(F) becomes
// row * sizeof(F).
template <typename F, bool SCALE, bool CM>
__device__ __forceinline__ void make_entry(F a, unsigned ko, const F *__restrict__ dl,
                                           unsigned zero_off, F &a_out, unsigned &ko_out) {
    if (SCALE) {
        const F dk = dl[ko / (64u * (unsigned)sizeof(F))];
        a_out = a * dk;
        ko_out = dk != F(0) ? ko : zero_off;
    } else {
        a_out = a;
        ko_out = CM ? ko >> 6 : ko;
    }
}

template <typename F, bool SCALE, bool CM, int C>
struct ColLoop {
    // processes static column C of the wave's group, then recurses to C + 1
    static __device__ __forceinline__ void run(F (&acc)[GATHER_CPW],
                                               const unsigned char *__restrict__ slab,
                                               F *__restrict__ ring, unsigned &kcur,
                                               const F *__restrict__ dl, unsigned zero_off,
                                               int cntv, int &pos, F &na, unsigned &nk,
                                               const F *__restrict__ vals,
                                               const unsigned *__restrict__ koff, int64_t base,
                                               int total, int lane, int lane_off) {
        int nc = __builtin_amdgcn_readlane(cntv, C);
        while (nc > 0) {
            // stay inside the current 64-entry chunk: no rotation test in the hot loop
            const int l0 = pos & 63;
            const int m = min(nc, 64 - l0);
            int t = l0;
            const int tend = l0 + m;
            for (; t + 4 <= tend; t += 4) {   // 8 independent LDS reads in flight
                TM_GATHER_STEP(a0, x0, t)
                TM_GATHER_STEP(a1, x1, t + 1)
                TM_GATHER_STEP(a2, x2, t + 2)
                TM_GATHER_STEP(a3, x3, t + 3)
                acc[C] = fma(a0, x0, acc[C]);
                acc[C] = fma(a1, x1, acc[C]);
                acc[C] = fma(a2, x2, acc[C]);
                acc[C] = fma(a3, x3, acc[C]);
            }
            for (; t < tend; ++t) {
                TM_GATHER_STEP(a0, x0, t)
                acc[C] = fma(a0, x0, acc[C]);
            }
            pos += m;
            nc -= m;
            if ((pos & 63) == 0) {
                // chunk exhausted: the prefetched chunk replaces it, next prefetch is issued
                F a_new;
                make_entry<F, SCALE, CM>(na, nk, dl, zero_off, a_new, kcur);
                __builtin_amdgcn_wave_barrier();
                ring[lane] = a_new;
                __builtin_amdgcn_wave_barrier();
                const int nxt = pos + 64 + lane;
                if (nxt < total) {
                    na = vals[base + nxt];
                    nk = koff[base + nxt];
                }
            }
        }
        if constexpr (C + 1 < GATHER_CPW)
            ColLoop<F, SCALE, CM, C + 1>::run(acc, slab, ring, kcur, dl, zero_off, cntv, pos, na, nk,
                                          vals, koff, base, total, lane, lane_off);
    }
};

// ORDER_F: the slab is kept COLUMN-major in LDS ([64 columns][SLAB_R + 1 rows], rows fastest,
// odd column stride): the vectors of an F-ordered B (consecutive rows of one column) are stored
// contiguously, and the gather's read  lane <-> column, uniform row  hits 64 distinct addresses
// (lane * (SLAB_R + 1) + row) without bank conflicts.  Row offsets of the stream (row * ROWB for the
// row-major slab) are divided by 64 when a chunk enters the ring.
template <typename F, bool ORDER_F>
struct GatherLds {
    static constexpr int ROWB = 64 * (int)sizeof(F);             // bytes per LDS slab row (row-major)
    static constexpr int COLB = (SLAB_R + 1) * (int)sizeof(F);   // bytes per LDS slab column (column-major)
    static constexpr int SLABB = ORDER_F ? ((64 * COLB + 15) / 16) * 16 : SLAB_R * ROWB;  // per buffer
    static constexpr int ZERO_OFF = 2 * SLABB;                   // all-zero row
    static constexpr int DL_OFF = ZERO_OFF + ROWB;               // d of the slab rows, 2 buffers
    static constexpr int RING_OFF = DL_OFF + 2 * SLAB_R * (int)sizeof(F);
    static constexpr int TOTAL = RING_OFF + GATHER_NW * 64 * (int)sizeof(F);
};

template <typename F, bool ORDER_F, bool VEC_OK>
__global__ __launch_bounds__(GATHER_THREADS) void csr_dense_gather_kernel(
    const F *__restrict__ vals, const unsigned *__restrict__ koff,
    const unsigned short *__restrict__ cnt, const int64_t *__restrict__ gptr, int n_groups,
    int64_t n_slabs, int64_t slabs_per_block, const F *__restrict__ B, int64_t n, int64_t r,
    int nB, const F *__restrict__ d, F *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using L = GatherLds<F, ORDER_F>;
    constexpr bool ASYNC = !ORDER_F && VEC_OK;   // global_load_lds staging, d folded into the stream
    constexpr int VEC = 16 / (int)sizeof(F);
    constexpr int ROWB = L::ROWB;
    constexpr int SLABB = L::SLABB;
    constexpr int NV = SLAB_R * 64 / VEC / GATHER_THREADS;  // 16-byte vectors staged per thread
    static_assert(NV >= 1 && (64 / VEC) % NV == 0, "staging: NV vectors of one row per thread");
    typedef F vec_t __attribute__((ext_vector_type(VEC)));

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> SGPRs / s_load
    const int group = blockIdx.z * GATHER_NW + wave;
    const bool active = group < n_groups;
    const int j0 = blockIdx.y * 64;
    const int64_t s0 = (int64_t)blockIdx.x * slabs_per_block;
    const int64_t s1 = min(s0 + slabs_per_block, n_slabs);
    const int lane_off = ORDER_F ? lane * L::COLB : lane * (int)sizeof(F);
    F *dl_all = reinterpret_cast<F *>(smem_raw + L::DL_OFF);
    F *ring = reinterpret_cast<F *>(smem_raw + L::RING_OFF) + wave * 64;

    F acc[GATHER_CPW];
#pragma unroll
    for (int c = 0; c < GATHER_CPW; ++c) acc[c] = F(0);
    for (int i = tid; i < ROWB / (int)sizeof(F); i += GATHER_THREADS)
        reinterpret_cast<F *>(smem_raw + L::ZERO_OFF)[i] = F(0);

    // ---------------- staging of the dense slab ----------------
    vec_t stage[ASYNC ? 1 : NV];
    vec_t dstage[1];   // ORDER_F: d of the thread's row vector (the same rows for all of its NV vectors)
    F dsc = F(0);
    // ASYNC: every wave copies NV KiB-sized pieces (64 lanes x 16 B) of the slab straight into
    // LDS with global_load_lds (no VGPRs, no ds_write pass); d of the slab rows goes to LDS (dl).
    // Otherwise (F-ordered or unaligned B): loads into registers, scaled by d when written to LDS.
    auto issue_slab = [&](int64_t s, int buf) {
        if (ASYNC) {
            constexpr int RPP = 1024 / ROWB;             // slab rows per 1 KiB piece
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int piece = wave * NV + i;
                const int row = piece * RPP + (lane * 16) / ROWB;
                const int c = ((lane * 16) % ROWB) / (int)sizeof(F);
                const int64_t k = min(s * SLAB_R + row, n - 1);
                const int cc = min(j0 + c, nB - VEC);
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(B + k * r + cc),
                    (__attribute__((address_space(3))) void *)(smem_raw + buf * SLABB + piece * 1024),
                    16, 0, 0);
            }
            if (tid < SLAB_R) dsc = d[min(s * SLAB_R + tid, n - 1)];
        } else if (!ORDER_F) {
            constexpr int VPR = 64 / VEC;        // vectors per slab row
            constexpr int TPR = VPR / NV;        // threads per slab row (NV consecutive vectors each)
            const int row = tid / TPR;
            const int c0 = (tid % TPR) * NV * VEC;
            const int64_t k = min(s * SLAB_R + row, n - 1);
            dsc = d[k];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    stage[ASYNC ? 0 : i][e] = B[k * r + min(j0 + c0 + i * VEC + e, nB - 1)];
            }
        } else {
            constexpr int RPC = SLAB_R / VEC;  // row-vectors per column
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int q = tid + i * GATHER_THREADS;
                const int c = min(j0 + q / RPC, nB - 1);
                const int row = (q % RPC) * VEC;
                const int64_t k = s * SLAB_R + row;
                if (VEC_OK) {
                    const int64_t kk = min(k, n - VEC);
                    stage[ASYNC ? 0 : i] = *reinterpret_cast<const vec_t *>(B + (int64_t)c * n + kk);
                    if (i == 0) dstage[0] = *reinterpret_cast<const vec_t *>(d + kk);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int64_t kk = min(k + e, n - 1);
                        stage[ASYNC ? 0 : i][e] = B[(int64_t)c * n + kk];
                        if (i == 0) dstage[0][e] = d[kk];
                    }
                }
            }
        }
    };
    auto finish_slab = [&](int64_t s, int buf) {
        unsigned char *dst = smem_raw + buf * SLABB;
        if (ASYNC) {
            if (tid < SLAB_R) dl_all[buf * SLAB_R + tid] = (s * SLAB_R + tid < n) ? dsc : F(0);
        } else if (!ORDER_F) {
            constexpr int VPR = 64 / VEC;
            constexpr int TPR = VPR / NV;
            const int row = tid / TPR;
            const int c0 = (tid % TPR) * NV * VEC;
            const bool rok = (s * SLAB_R + row < n) && dsc != F(0);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = c0 + i * VEC;
                vec_t v;
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    v[e] = (rok && j0 + c + e < nB) ? dsc * stage[ASYNC ? 0 : i][e] : F(0);
                *reinterpret_cast<vec_t *>(dst + row * ROWB + c * (int)sizeof(F)) = v;
            }
        } else {
            constexpr int RPC = SLAB_R / VEC;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int q = tid + i * GATHER_THREADS;
                const int c = q / RPC;
                const int row = (q % RPC) * VEC;
                const bool cok = j0 + c < nB;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const F dv = dstage[0][e];
                    const bool ok = cok && (s * SLAB_R + row + e < n) && dv != F(0);
                    *reinterpret_cast<F *>(dst + c * L::COLB + (row + e) * (int)sizeof(F)) =
                        ok ? dv * stage[ASYNC ? 0 : i][e] : F(0);
                }
            }
        }
    };

    // Two-deep software pipeline over the slabs so that no load of an iteration depends on
    // another load issued in the same iteration (each would cost a full HBM round trip):
    //   iteration s issues   meta(s + 2)  = run lengths + stream base/total      (stage M)
    //                        head(s + 1)  = first two 64-entry chunks, from meta(s + 1) (stage H)
    //                        slab(s + 1)  = dense rows of the next slab           (stage S)
    //   then computes slab s out of LDS, completes slab(s + 1) in the other LDS buffer, barrier.
    int m_cnt = 0, m_total = 0;          // meta of slab s + 2 (after stage M)
    int64_t m_base = 0;
    int h_cnt = 0, h_total = 0;          // head of slab s + 1 (after stage H)
    int64_t h_base = 0;
    F h_va = F(0), h_na = F(0);
    unsigned h_vk = 0, h_nk = 0;
    auto load_meta = [&](int64_t s) {
        m_cnt = 0; m_total = 0; m_base = 0;
        if (!active || s >= s1) return;
        m_cnt = lane < GATHER_CPW ? (int)cnt[(s * n_groups + group) * GATHER_CPW + lane] : 0;
        m_base = gptr[s * n_groups + group];
        m_total = (int)(gptr[s * n_groups + group + 1] - m_base);
    };
    auto load_head = [&]() {             // consumes meta, issues the chunk loads
        h_cnt = m_cnt; h_total = m_total; h_base = m_base;
        h_va = F(0); h_na = F(0); h_vk = 0; h_nk = 0;
        if (lane < h_total) {
            h_va = vals[h_base + lane];
            h_vk = koff[h_base + lane];
        }
        if (64 + lane < h_total) {
            h_na = vals[h_base + 64 + lane];
            h_nk = koff[h_base + 64 + lane];
        }
    };

    if (s0 < s1) {
        load_meta(s0);
        load_head();                      // head(s0)
        load_meta(s0 + 1);                // meta(s0 + 1)
        issue_slab(s0, 0);
        finish_slab(s0, 0);
    }
    __syncthreads();
    for (int64_t s = s0; s < s1; ++s) {
        const int buf = (int)((s - s0) & 1);
        // take over the prefetched head of this slab
        const int cntv = h_cnt, total = h_total;
        const int64_t base = h_base;
        F va = h_va, na = h_na;
        unsigned vk = h_vk, nk = h_nk;
        if (s + 1 < s1) {
            load_head();                  // head(s + 1) from meta(s + 1), loaded last iteration
            issue_slab(s + 1, buf ^ 1);
        }
        load_meta(s + 2);
        if (active && total > 0) {
            int pos = 0;
            const F *dl = dl_all + buf * SLAB_R;
            const unsigned zero_off = (unsigned)(L::ZERO_OFF - buf * SLABB);
            F a_cur;
            unsigned kcur;
            make_entry<F, ASYNC, ORDER_F>(va, vk, dl, zero_off, a_cur, kcur);
            __builtin_amdgcn_wave_barrier();
            ring[lane] = a_cur;
            __builtin_amdgcn_wave_barrier();
            ColLoop<F, ASYNC, ORDER_F, 0>::run(acc, smem_raw + buf * SLABB, ring, kcur, dl, zero_off, cntv, pos,
                                      na, nk, vals, koff, base, total, lane, lane_off);
        }
        if (s + 1 < s1) finish_slab(s + 1, buf ^ 1);
        __syncthreads();
    }
    if (active) {
        // ws layout: [part = blockIdx.y][blockIdx.x][n_groups * CPW cols][64]
        F *dst = ws + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * n_groups + group) *
                          (GATHER_CPW * 64);
#pragma unroll
        for (int c = 0; c < GATHER_CPW; ++c) dst[c * 64 + lane] = acc[c];
    }
}

// =======================================================================================
// K3 (ELL)  sparse x dense on an interleaved-ELL twin: static iterations with skip masks.
//
// The run loop of the kernel above spends ~10 cycles per nonzero and CU on a 5 % dense block (its
// dynamic control flow, not the LDS or the FMAs: scripts/ubench/gather_dyn.hip reproduces the rate
// without any staging).  Here a (slab, 32-column group) block is I ITERATIONS of 64 slots,
// slot it*64 + 2c + u = the (2 it + u)-th nonzero (rows ascending) of column c, padded to the
// longest run of the group (I = ceil(longest / 2)).  An iteration is one coalesced 64-lane load
// {value, row offset}; its code is straight-line with STATIC accumulators and constant lanes:
// per slot v_readlane (row offset -> SGPR), v_add, ds_read_b64 of the slab row, half a uniform
// 16-byte ring read (two values), v_fma_f64.  The padding (x1.9 at 5 % density) is not executed:
// a ballot of the real slots gives a 64-bit mask, and every batch of 4 slots (2 columns) whose
// mask bits are all clear is skipped with one scalar test -- 6.9 cycles per real nonzero and CU in
// isolation (scripts/ubench/gather_ellmask.hip) against 10.0 for the run loop.
// Staging, d folding and the zero row are those of csr_dense_gather_kernel's asynchronous path.
// =======================================================================================
constexpr unsigned ELL_PADKEY = 0xFFFFFFFFu;

template <typename F>
__global__ __launch_bounds__(GATHER_THREADS) void csr_dense_ell_kernel(
    const F *__restrict__ vals, const unsigned *__restrict__ koff, const int64_t *__restrict__ gptr,
    int n_groups, int64_t n_slabs, int64_t slabs_per_block, const F *__restrict__ B, int64_t n,
    int64_t r, int nB, const F *__restrict__ d, F *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using L = GatherLds<F, false>;
    constexpr int VEC = 16 / (int)sizeof(F);
    constexpr int ROWB = L::ROWB;
    constexpr int SLABB = L::SLABB;
    constexpr int NV = SLAB_R * 64 / VEC / GATHER_THREADS;
    constexpr int RPP = 1024 / ROWB;
    constexpr int NA = 16 / (int)sizeof(F);          // values per 16-byte ring read
    typedef F avec_t __attribute__((ext_vector_type(NA)));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int group = blockIdx.z * GATHER_NW + wave;
    const bool active = group < n_groups;
    const int j0 = blockIdx.y * 64;
    const int64_t s0 = (int64_t)blockIdx.x * slabs_per_block;
    const int64_t s1 = min(s0 + slabs_per_block, n_slabs);
    const unsigned lane_off = lane * (unsigned)sizeof(F);
    F *dl_all = reinterpret_cast<F *>(smem_raw + L::DL_OFF);
    F *ring = reinterpret_cast<F *>(smem_raw + L::RING_OFF) + wave * 64;

    F acc[GATHER_CPW];
#pragma unroll
    for (int c = 0; c < GATHER_CPW; ++c) acc[c] = F(0);
    for (int i = tid; i < ROWB / (int)sizeof(F); i += GATHER_THREADS)
        reinterpret_cast<F *>(smem_raw + L::ZERO_OFF)[i] = F(0);

    F dsc = F(0);
    auto issue_slab = [&](int64_t s, int buf) {       // async copy of B[slab rows, j0 .. j0 + 64)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int piece = wave * NV + i;
            const int row = piece * RPP + (lane * 16) / ROWB;
            const int c = ((lane * 16) % ROWB) / (int)sizeof(F);
            const int64_t k = min(s * SLAB_R + row, n - 1);
            const int cc = min(j0 + c, nB - VEC);
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)(B + k * r + cc),
                (__attribute__((address_space(3))) void *)(smem_raw + buf * SLABB + piece * 1024), 16, 0,
                0);
        }
        if (tid < SLAB_R) dsc = d[min(s * SLAB_R + tid, n - 1)];
    };
    auto finish_slab = [&](int64_t s, int buf) {
        if (tid < SLAB_R) dl_all[buf * SLAB_R + tid] = (s * SLAB_R + tid < n) ? dsc : F(0);
    };
    // value scaled by d, row offset redirected to the zero row for padding and d == 0 rows
    auto enter = [&](F a, unsigned ko, const F *dl, unsigned zero_off, F &a_out, unsigned &k_out) {
        const bool real = ko != ELL_PADKEY;
        const F dk = real ? dl[ko / (unsigned)ROWB] : F(0);
        a_out = real ? a * dk : F(0);
        k_out = dk != F(0) ? ko : zero_off;
        return dk != F(0);
    };

    // meta(s + 2) / head(s + 1) pipeline as in csr_dense_gather_kernel
    int h_iters = 0;
    int64_t h_base = 0;
    int64_t mv_base = 0, mv_end = 0;    // meta of slab s + 2 as loaded (per-lane copies)
    bool m_valid = false;
    int vzero = 0;
    asm volatile("" : "+v"(vzero));     // a zero the compiler cannot see through (kept in a VGPR)
    F h_va = F(0), h_na = F(0);
    unsigned h_vk = ELL_PADKEY, h_nk = ELL_PADKEY;
    auto load_meta = [&](int64_t s) {
        m_valid = false;
        if (!active || s >= s1) return;
        // VECTOR loads on purpose (lane-dependent zero offset): a scalar load would share lgkmcnt
        // with the LDS reads, and since scalar loads return out of order the compiler waits for
        // it (one memory round trip per slab) before the next LDS access
        // (kept in VGPRs until load_head turns them into wave-uniform values one slab later)
        const int64_t *gp = gptr + s * n_groups + group + vzero;
        mv_base = gp[0];
        mv_end = gp[1];
        m_valid = true;
    };
    auto load_head = [&]() {
        h_base = m_valid ? readfirstlane_i64(mv_base) : 0;
        h_iters = m_valid ? (int)((readfirstlane_i64(mv_end) - h_base) >> 6) : 0;
        if (h_iters > 0) {
            h_va = vals[h_base + lane];
            h_vk = koff[h_base + lane];
            const int64_t q = h_base + (h_iters > 1 ? 64 : 0) + lane;
            h_na = vals[q];
            h_nk = koff[q];
        }
    };

    if (s0 < s1) {
        load_meta(s0);
        load_head();
        load_meta(s0 + 1);
        issue_slab(s0, 0);
        finish_slab(s0, 0);
    }
    __syncthreads();
    for (int64_t s = s0; s < s1; ++s) {
        const int buf = (int)((s - s0) & 1);
        const int iters = h_iters;
        const int64_t base = h_base;
        F va = h_va, na = h_na;
        unsigned vk = h_vk, nk = h_nk;
        if (s + 1 < s1) {
            load_head();
            issue_slab(s + 1, buf ^ 1);
        }
        load_meta(s + 2);
        if (active && iters > 0) {
            const F *dl = dl_all + buf * SLAB_R;
            const unsigned zero_off = (unsigned)(L::ZERO_OFF - buf * SLABB);
            const unsigned char *slab = smem_raw + buf * SLABB;
            F a_cur;
            unsigned k_cur;
            unsigned long long live = __builtin_amdgcn_ballot_w64(enter(va, vk, dl, zero_off, a_cur, k_cur));
            __builtin_amdgcn_wave_barrier();
            ring[lane] = a_cur;
            __builtin_amdgcn_wave_barrier();
            for (int it = 0; it < iters; ++it) {
#pragma unroll
                for (int g0 = 0; g0 < 64; g0 += 4) {
                    if (((live >> g0) & 0xFull) == 0) continue;      // 2 columns of padding / d == 0
                    F x[4], a[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        x[e] = *reinterpret_cast<const F *>(
                            slab + (unsigned)__builtin_amdgcn_readlane((int)k_cur, g0 + e) + lane_off);
#pragma unroll
                    for (int e = 0; e < 4; e += NA) {
                        const avec_t av = *reinterpret_cast<const avec_t *>(ring + g0 + e);
#pragma unroll
                        for (int q = 0; q < NA; ++q) a[e + q] = av[q];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        acc[(g0 + e) / 2] = fma(a[e], x[e], acc[(g0 + e) / 2]);
                    // pin the FMAs here (else the selector sinks them behind all loads)
                    asm volatile("" : "+v"(acc[g0 / 2]));
                    asm volatile("" : "+v"(acc[g0 / 2 + 1]));
                }
                if (it + 1 < iters) {
                    // the prefetched chunk replaces the consumed one, the next prefetch is issued
                    // (unconditional clamped loads: nothing waits for them before the next turn)
                    live = __builtin_amdgcn_ballot_w64(enter(na, nk, dl, zero_off, a_cur, k_cur));
                    __builtin_amdgcn_wave_barrier();
                    ring[lane] = a_cur;
                    __builtin_amdgcn_wave_barrier();
                    const int64_t q = base + (int64_t)min(it + 2, iters - 1) * 64 + lane;
                    na = vals[q];
                    nk = koff[q];
                }
            }
        }
        if (s + 1 < s1) finish_slab(s + 1, buf ^ 1);
        __syncthreads();
    }
    if (active) {
        F *dst = ws + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * n_groups + group) *
                          (GATHER_CPW * 64);
#pragma unroll
        for (int c = 0; c < GATHER_CPW; ++c) dst[c * 64 + lane] = acc[c];
    }
}

// =======================================================================================
// K3 (wide ELL)  the same static-iteration gather with lane <-> TWO dense columns: the LDS slab
// holds ELLW_R = 64 rows x 128 dense columns, a nonzero costs one 16-byte LDS read + two FMAs and
// its {value, row offset} is streamed and broadcast ONCE for 128 dense columns instead of once per
// 64-column part (the 64-column kernel spends 2 x 6.9 cycles per nonzero and CU on 128 columns,
// this geometry 11.0: scripts/ubench/gather_ellwide.hip; the floor is the LDS read bandwidth,
// 8 cycles per KiB row).  A wave owns ELLW_C = 16 sparse columns (32 accumulators), an iteration
// is 16 columns x 4 slots, slot it*64 + 4c + u = the (4 it + u)-th nonzero of column c; padding
// is skipped two slots at a time.  A workgroup covers 256 sparse columns; wider blocks use
// blockIdx.z, whose workgroups read the same slabs at the same time on the same XCD (L2 hits).
// =======================================================================================
constexpr int ELLW_R = 64;
constexpr int ELLW_C = 16;
constexpr int ELLW_NW = 256 / ELLW_C;               // waves per workgroup: 256 sparse columns
constexpr int ELLW_THREADS = ELLW_NW * 64;
constexpr int ELLW_U = 64 / ELLW_C;                  // slots per column and iteration
constexpr int ELLW_W = 128;                          // dense columns per part
constexpr int ELLW_HC = 3;                           // chunks of a block prefetched one slab ahead
constexpr int ELLW_SK = 2;                           // slots per skip batch

template <typename F>
struct EllwLds {
    static constexpr int ROWB = ELLW_W * (int)sizeof(F);
    static constexpr int SLABB = ELLW_R * ROWB;
    static constexpr int ZERO_OFF = 2 * SLABB;
    static constexpr int DL_OFF = ZERO_OFF + ROWB;
    static constexpr int RING_OFF = DL_OFF + 2 * ELLW_R * (int)sizeof(F);
    static constexpr int TOTAL = RING_OFF + ELLW_NW * 64 * (int)sizeof(F);
};

template <typename F>
__global__ __launch_bounds__(ELLW_THREADS) void csr_dense_ellw_kernel(
    const F *__restrict__ vals, const unsigned *__restrict__ koff, const int64_t *__restrict__ gptr,
    int n_groups, int64_t n_slabs, int64_t slabs_per_block, const F *__restrict__ B, int64_t n,
    int64_t r, int nB, const F *__restrict__ d, F *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using L = EllwLds<F>;
    constexpr int VEC = 16 / (int)sizeof(F);
    constexpr int ROWB = L::ROWB;
    constexpr int SLABB = L::SLABB;
    constexpr int NV = SLABB / 16 / ELLW_THREADS;      // 16-byte pieces staged per thread
    constexpr int RPP = 1024 / ROWB;                     // slab rows per 1 KiB wave piece (1 or 2)
    typedef F pair_t __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int group = blockIdx.z * ELLW_NW + wave;
    const bool active = group < n_groups;
    const int j0 = blockIdx.y * ELLW_W;
    const int64_t s0 = (int64_t)blockIdx.x * slabs_per_block;
    const int64_t s1 = min(s0 + slabs_per_block, n_slabs);
    const unsigned lane_off = lane * 2u * (unsigned)sizeof(F);
    F *dl_all = reinterpret_cast<F *>(smem_raw + L::DL_OFF);
    F *ring = reinterpret_cast<F *>(smem_raw + L::RING_OFF) + wave * 64;

    pair_t acc[ELLW_C];
#pragma unroll
    for (int c = 0; c < ELLW_C; ++c) acc[c] = pair_t{F(0), F(0)};
    for (int i = tid; i < ROWB / (int)sizeof(F); i += ELLW_THREADS)
        reinterpret_cast<F *>(smem_raw + L::ZERO_OFF)[i] = F(0);

    F dsc = F(0);
    auto issue_slab = [&](int64_t s, int buf) {       // async copy of B[slab rows, j0 .. j0 + 128)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int piece = wave * NV + i;
            const int row = piece * RPP + (lane * 16) / ROWB;
            const int c = ((lane * 16) % ROWB) / (int)sizeof(F);
            const int64_t k = min(s * ELLW_R + row, n - 1);
            const int cc = min(j0 + c, nB - VEC);
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)(B + k * r + cc),
                (__attribute__((address_space(3))) void *)(smem_raw + buf * SLABB + piece * 1024), 16, 0,
                0);
        }
        if (tid < ELLW_R) dsc = d[min(s * ELLW_R + tid, n - 1)];
    };
    auto finish_slab = [&](int64_t s, int buf) {
        if (tid < ELLW_R) dl_all[buf * ELLW_R + tid] = (s * ELLW_R + tid < n) ? dsc : F(0);
    };
    auto enter = [&](F a, unsigned ko, const F *dl, unsigned zero_off, F &a_out, unsigned &k_out) {
        const bool real = ko != ELL_PADKEY;
        const F dk = real ? dl[ko / (unsigned)ROWB] : F(0);
        a_out = real ? a * dk : F(0);
        k_out = dk != F(0) ? ko : zero_off;
        return dk != F(0);
    };

    // Pipeline over the slabs: meta(s + 2) = block start / length, head(s + 1) = the first
    // ELLW_HC chunks of the block (from meta(s + 1)), slab(s + 1) = async copy of the dense rows.
    // The head holds ALL chunks of a typical block (~2 iterations at 5 % density): vector loads
    // complete in order, so a chunk requested inside the slab loop would sit behind the 64 KB slab
    // copy issued at the top of the iteration and the wave would wait for that round trip after
    // its first chunk (measured: 6.4 ms with 2 head chunks + in-loop prefetch).
    int h_iters = 0;
    int64_t h_base = 0;
    int64_t mv_base = 0, mv_end = 0;    // meta of slab s + 2 as loaded (per-lane copies)
    bool m_valid = false;
    int vzero = 0;
    asm volatile("" : "+v"(vzero));     // a zero the compiler cannot see through (kept in a VGPR)
    F h_v[ELLW_HC];
    unsigned h_k[ELLW_HC];
#pragma unroll
    for (int c = 0; c < ELLW_HC; ++c) { h_v[c] = F(0); h_k[c] = ELL_PADKEY; }
    auto load_meta = [&](int64_t s) {
        m_valid = false;
        if (!active || s >= s1) return;
        // VECTOR loads on purpose (lane-dependent zero offset): a scalar load would share lgkmcnt
        // with the LDS reads, and since scalar loads return out of order the compiler waits for
        // it (one memory round trip per slab) before the next LDS access
        // (kept in VGPRs until load_head turns them into wave-uniform values one slab later)
        const int64_t *gp = gptr + s * n_groups + group + vzero;
        mv_base = gp[0];
        mv_end = gp[1];
        m_valid = true;
    };
    auto load_head = [&]() {
        h_base = m_valid ? readfirstlane_i64(mv_base) : 0;
        h_iters = m_valid ? (int)((readfirstlane_i64(mv_end) - h_base) >> 6) : 0;
        if (h_iters > 0) {
#pragma unroll
            for (int c = 0; c < ELLW_HC; ++c) {
                const int64_t q = h_base + (int64_t)min(c, h_iters - 1) * 64 + lane;
                h_v[c] = vals[q];
                h_k[c] = koff[q];
            }
        }
    };

    if (s0 < s1) {
        load_meta(s0);
        load_head();
        load_meta(s0 + 1);
        issue_slab(s0, 0);
        finish_slab(s0, 0);
    }
    __syncthreads();
    for (int64_t s = s0; s < s1; ++s) {
        const int buf = (int)((s - s0) & 1);
        const int iters = h_iters;
        const int64_t base = h_base;
        F cv[ELLW_HC];
        unsigned ck[ELLW_HC];
#pragma unroll
        for (int c = 0; c < ELLW_HC; ++c) { cv[c] = h_v[c]; ck[c] = h_k[c]; }
        if (s + 1 < s1) {
            load_head();
            issue_slab(s + 1, buf ^ 1);
        }
        load_meta(s + 2);
        if (active && iters > 0) {
            const F *dl = dl_all + buf * ELLW_R;
            const unsigned zero_off = (unsigned)(L::ZERO_OFF - buf * SLABB);
            const unsigned char *slab = smem_raw + buf * SLABB;
            auto do_chunk = [&](F va, unsigned vk) {
                F a_cur;
                unsigned k_cur;
                const unsigned long long live =
                    __builtin_amdgcn_ballot_w64(enter(va, vk, dl, zero_off, a_cur, k_cur));
                __builtin_amdgcn_wave_barrier();
                ring[lane] = a_cur;
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int g8 = 0; g8 < 64; g8 += 8) {
                if (((live >> g8) & 0xFFull) == 0) continue;       // two whole columns dead
#pragma unroll
                for (int g0 = g8; g0 < g8 + 8; g0 += ELLW_SK) {
                    if (((live >> g0) & ((1ull << ELLW_SK) - 1)) == 0) continue;   // padding / d == 0 slots
                    pair_t x[ELLW_SK];
                    F a[ELLW_SK];
#pragma unroll
                    for (int e = 0; e < ELLW_SK; ++e)
                        x[e] = *reinterpret_cast<const pair_t *>(
                            slab + (unsigned)__builtin_amdgcn_readlane((int)k_cur, g0 + e) + lane_off);
#pragma unroll
                    for (int e = 0; e < ELLW_SK; e += 2) {
                        const pair_t av = *reinterpret_cast<const pair_t *>(ring + g0 + e);
                        a[e] = av[0];
                        a[e + 1] = av[1];
                    }
                    pair_t &A = acc[g0 / ELLW_U];
#pragma unroll
                    for (int e = 0; e < ELLW_SK; ++e) {
                        A[0] = fma(a[e], x[e][0], A[0]);
                        A[1] = fma(a[e], x[e][1], A[1]);
                    }
                    asm volatile("" : "+v"(A));      // pin the FMAs here
                }
                }
                __builtin_amdgcn_wave_barrier();     // ring is rewritten by the next chunk
            };
#pragma unroll
            for (int c = 0; c < ELLW_HC; ++c)
                if (c < iters) do_chunk(cv[c], ck[c]);
            for (int it = ELLW_HC; it < iters; ++it) {      // long blocks: the rest synchronously
                const int64_t q = base + (int64_t)it * 64 + lane;
                do_chunk(vals[q], koff[q]);
            }
        }
        if (s + 1 < s1) finish_slab(s + 1, buf ^ 1);
        __syncthreads();
    }
    if (active) {
        // ws layout: [part][block][n_groups * ELLW_C columns][128]
        F *dst = ws + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * n_groups + group) *
                          (ELLW_C * ELLW_W);
#pragma unroll
        for (int c = 0; c < ELLW_C; ++c)
            *reinterpret_cast<pair_t *>(dst + c * ELLW_W + lane * 2) = acc[c];
    }
}

constexpr SlabGeom GATHER_GEOM{SLAB_R, GATHER_CPW, GATHER_NW, 64, true};
constexpr SlabGeom ELLW_GEOM{ELLW_R, ELLW_C, ELLW_NW, ELLW_W, false};

template <typename F>
static int run_csr_dense_gather(const F *vals, const unsigned *koff, const unsigned short *cnt,
                                const int64_t *gptr, int64_t n, int64_t m, const F *B, int64_t r,
                                int order_f, const F *d, F *out, hipStream_t st) {
    const int64_t nB = r;
    if (m * nB == 0) return TM_OK;
    const SlabPlan p = slab_plan(n, m, nB, GATHER_GEOM);
    if (p.n_slabs == 0) return slab_zero_fill<F>(out, m, nB, nullptr, st);
    SlabWs<F> w;
    int rc = slab_workspace(p, 0, 0, st, &w);
    if (rc) return rc;
    const size_t lds = order_f ? (size_t)GatherLds<F, true>::TOTAL : (size_t)GatherLds<F, false>::TOTAL;
    // 16-byte vector loads need aligned bases and row/column strides that keep every vector
    // 16-byte aligned and entirely inside the matrix
    constexpr int VEC = 16 / (int)sizeof(F);
    const bool base_ok = (reinterpret_cast<uintptr_t>(B) & 15) == 0 && n >= VEC && nB >= VEC;
    const bool vec_ok = order_f ? (base_ok && n % VEC == 0 && (reinterpret_cast<uintptr_t>(d) & 15) == 0)
                                : (base_ok && r % VEC == 0);
    auto kern = order_f ? (vec_ok ? &csr_dense_gather_kernel<F, true, true>
                                  : &csr_dense_gather_kernel<F, true, false>)
                        : (vec_ok ? &csr_dense_gather_kernel<F, false, true>
                                  : &csr_dense_gather_kernel<F, false, false>);
    return slab_launch_and_finish<F>(kern, p, lds, w, m, nB, out, nullptr, st, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(kern, grid, block, lds, st, vals, koff, cnt, gptr, p.n_groups, p.n_slabs, p.spb, B, n, r,
                           (int)nB, d, w.part);
    });
}

// ell and ellw: one argument list, one launch
template <typename F, typename Kern>
static int run_csr_dense_ell_form(const char *entry, Kern kern, const SlabGeom &geom, size_t lds, const F *vals,
                                  const unsigned *koff, const int64_t *gptr, int64_t n, int64_t m, const F *B,
                                  int64_t r, const F *d, F *out, hipStream_t st) {
    const int64_t nB = r;
    if (m * nB == 0) return TM_OK;
    int rc = slab_check_b(entry, B, r);
    if (!rc && !geom.pad_m) rc = slab_check_m(entry, m, geom.cpw);
    if (rc) return rc;
    const SlabPlan p = slab_plan(n, m, nB, geom);
    if (p.n_slabs == 0) return slab_zero_fill<F>(out, m, nB, nullptr, st);
    SlabWs<F> w;
    rc = slab_workspace(p, 0, 0, st, &w);
    if (rc) return rc;
    return slab_launch_and_finish<F>(kern, p, lds, w, m, nB, out, nullptr, st, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(kern, grid, block, lds, st, vals, koff, gptr, p.n_groups, p.n_slabs, p.spb, B, n, r,
                           (int)nB, d, w.part);
    });
}

}  // namespace tmh

extern "C" {

int tm_slab_rows(void) { return tmh::SLAB_R; }
int tm_slab_group_cols(void) { return tmh::GATHER_CPW; }
int tm_ellw_rows(void) { return tmh::ELLW_R; }
int tm_ellw_group_cols(void) { return tmh::ELLW_C; }

int tm_csr_dense_sandwich_slab_f32(const float *vals, const uint32_t *koff, const uint16_t *cnt,
                                   const int64_t *gptr, int64_t n, int64_t m, const float *B,
                                   int64_t r, int order_f, const float *d, float *out, void *stream) {
    return tmh::run_csr_dense_gather<float>(vals, koff, cnt, gptr, n, m, B, r, order_f, d, out,
                                            tmh::as_stream(stream));
}
int tm_csr_dense_sandwich_slab_f64(const double *vals, const uint32_t *koff, const uint16_t *cnt,
                                   const int64_t *gptr, int64_t n, int64_t m, const double *B,
                                   int64_t r, int order_f, const double *d, double *out, void *stream) {
    return tmh::run_csr_dense_gather<double>(vals, koff, cnt, gptr, n, m, B, r, order_f, d, out,
                                             tmh::as_stream(stream));
}

int tm_csr_dense_sandwich_ell_f32(const float *vals, const uint32_t *koff, const int64_t *gptr,
                                  int64_t n, int64_t m, const float *B, int64_t r, const float *d,
                                  float *out, void *stream) {
    return tmh::run_csr_dense_ell_form<float>("tm_csr_dense_sandwich_ell", &tmh::csr_dense_ell_kernel<float>,
                                              tmh::GATHER_GEOM, tmh::GatherLds<float, false>::TOTAL, vals, koff, gptr,
                                              n, m, B, r, d, out, tmh::as_stream(stream));
}
int tm_csr_dense_sandwich_ell_f64(const double *vals, const uint32_t *koff, const int64_t *gptr,
                                  int64_t n, int64_t m, const double *B, int64_t r, const double *d,
                                  double *out, void *stream) {
    return tmh::run_csr_dense_ell_form<double>("tm_csr_dense_sandwich_ell", &tmh::csr_dense_ell_kernel<double>,
                                               tmh::GATHER_GEOM, tmh::GatherLds<double, false>::TOTAL, vals, koff, gptr,
                                               n, m, B, r, d, out, tmh::as_stream(stream));
}
int tm_csr_dense_sandwich_ellw_f32(const float *vals, const uint32_t *koff, const int64_t *gptr,
                                   int64_t n, int64_t m, const float *B, int64_t r, const float *d,
                                   float *out, void *stream) {
    return tmh::run_csr_dense_ell_form<float>("tm_csr_dense_sandwich_ellw", &tmh::csr_dense_ellw_kernel<float>,
                                              tmh::ELLW_GEOM, tmh::EllwLds<float>::TOTAL, vals, koff, gptr, n, m, B, r,
                                              d, out, tmh::as_stream(stream));
}
int tm_csr_dense_sandwich_ellw_f64(const double *vals, const uint32_t *koff, const int64_t *gptr,
                                   int64_t n, int64_t m, const double *B, int64_t r, const double *d,
                                   double *out, void *stream) {
    return tmh::run_csr_dense_ell_form<double>("tm_csr_dense_sandwich_ellw", &tmh::csr_dense_ellw_kernel<double>,
                                               tmh::ELLW_GEOM, tmh::EllwLds<double>::TOTAL, vals, koff, gptr, n, m, B,
                                               r, d, out, tmh::as_stream(stream));
}

}  // extern "C"
