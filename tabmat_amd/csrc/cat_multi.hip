// The FUSED cross terms of ALL categorical blocks of a SplitMatrix with its dense / sparse block (the multi_cat_*
// family); the single-categorical kernels are in cat.hip.
//
// Every kernel here is a TILE kernel: a workgroup zeroes a tile of doubles [stacked levels][columns of its part] at
// the start of its LDS, adds into it with LDS atomics over its range of rows or slabs, and stores it as its slice of
// the partials ws[part][workgroup][levels x columns].  The pieces around the loops -- tile, slice, store, scratch
// behind the tile, level of a row, packed code word -- and the host path from the partials to `out` exist once, below.
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "reduce.hpp"

namespace tmh {

// ---------------------------------------------------------------------------------------
// FUSED cross terms of ALL categorical blocks of a SplitMatrix with its dense / sparse block.
// One pass over the wide operand serves every categorical: the LDS tile holds the stacked
// outputs [sum_c ncol_c][TJ] of a TJ-column slice of the wide operand (parts = column slices),
// so the dense block is read from HBM exactly once for all categoricals together (instead of
// once per categorical) and the 4-byte codes are re-read once per part.
// ---------------------------------------------------------------------------------------
constexpr int MAX_CATS = 16;
struct CatSet {
    const int32_t *codes[MAX_CATS];
    int ncol[MAX_CATS];
    int drop[MAX_CATS];
    int off[MAX_CATS];   // row offset of categorical c in the stacked output
    int n_cats;
    int total;           // sum of ncol
};

// ---------------------------------------------------------------------------------------
// device pieces the tile kernels share
// ---------------------------------------------------------------------------------------
// bytes of a tile of `nel` doubles, rounded to the 16-byte alignment of what follows it in LDS (host and device)
__host__ __device__ constexpr size_t tile_lds_bytes(size_t nel) { return ((nel * sizeof(lds_acc_t) + 15) / 16) * 16; }

// (no barrier: the kernels carve their scratch first and synchronise once)
__device__ __forceinline__ void zero_tile(lds_acc_t *tile, int nel) {
    for (int b = threadIdx.x; b < nel; b += blockDim.x) tile[b] = 0.0;
}

// the per-wave scratch of a kernel starts behind its tile
__device__ __forceinline__ unsigned char *scratch_behind_tile(unsigned char *smem, int nel) {
    return smem + tile_lds_bytes((size_t)nel);
}

// this workgroup's slice of the partials ws[part = blockIdx.y][workgroup = blockIdx.x][stride]
template <typename F>
__device__ __forceinline__ F *workgroup_slice(F *ws, int64_t stride) {
    return ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * stride;
}

// tile [rows][tstr] -> dst [rows][cols]: tstr == cols for the dense kernels' tiles, cols + 1 for the padded tiles of
// the sparse ones
template <typename F>
__device__ __forceinline__ void store_tile(const lds_acc_t *tile, int rows, int tstr, int cols, F *__restrict__ dst) {
    if (tstr == cols) {                  // (known at compile time at every call)
        for (int b = threadIdx.x; b < rows * cols; b += blockDim.x) dst[b] = (F)tile[b];
    } else {
        for (int b = threadIdx.x; b < rows * cols; b += blockDim.x) dst[b] = (F)tile[(b / cols) * tstr + (b % cols)];
    }
}

// column of `row` in categorical c: its level, counted from the first kept one (< 0: missing code or dropped level).
// Called as level_of(cs.codes[c], cs.drop[c], row): with the whole CatSet behind a reference the narrow dense kernels
// compile differently (they no longer unroll over the categoricals; 60 instantiations changed registers).
__device__ __forceinline__ int level_of(const int32_t *codes, int drop, int64_t row) { return codes[row] - drop; }

// packed code word of a row (tm_multi_cat_pack_codes, at most 3 categoricals): field c = the tile row of the row's
// level in categorical c (cs.off[c] + level), 10 bits each; PACKED_NONE: missing code or dropped level
constexpr int PACKED_BITS = 10;
constexpr int PACKED_NONE = (1 << PACKED_BITS) - 1;
__device__ __forceinline__ int packed_field(unsigned pk, int c) { return (int)((pk >> (PACKED_BITS * c)) & (unsigned)PACKED_NONE); }

// C-ordered dense: TJ lanes per row (64 / TJ rows per wave step), lane <-> dense column.
// NC = number of categoricals when <= 4 (codes of UNR rows x NC categoricals are loaded up
// front so that ~UNR * (2 + NC) independent loads are in flight per lane), 0 = generic loop.
template <typename F, int TJ, int NC>
__global__ __launch_bounds__(1024) void multi_cat_dense_c_kernel(
    CatSet cs, const F *__restrict__ d, const F *__restrict__ M, int64_t n, int64_t m,
    int64_t rows_per_block, F *__restrict__ ws, int64_t stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);  // [total][TJ]
    const int nel = cs.total * TJ;
    zero_tile(tile, nel);
    __syncthreads();
    constexpr int RPW = 64 / TJ;
    constexpr int UNR = 4;
    constexpr int NCC = NC > 0 ? NC : 1;
    const int lane = threadIdx.x & 63;
    const int sub = lane / TJ, jl = lane % TJ;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int64_t j = (int64_t)blockIdx.y * TJ + jl;
    const bool jok = j < m;
    const int64_t t0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t t1 = min(t0 + rows_per_block, n);
    const int64_t step = (int64_t)nwave * RPW;
    for (int64_t k0 = t0 + (int64_t)wave * RPW + sub; k0 < t1; k0 += UNR * step) {
        F x[UNR];
        int cc[UNR][NCC];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t k = k0 + u * step;
            const bool ok = k < t1;
            x[u] = (ok && jok) ? d[k] * M[k * m + j] : F(0);
            if (NC > 0) {
#pragma unroll
                for (int c = 0; c < NCC; ++c) cc[u][c] = ok ? level_of(cs.codes[c], cs.drop[c], k) : -1;
            }
        }
        if (NC > 0) {
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int c = 0; c < NCC; ++c)
                    if (jok && cc[u][c] >= 0)
                        atomic_add(&tile[(cs.off[c] + cc[u][c]) * TJ + jl], (lds_acc_t)x[u]);
        } else {
#pragma unroll 1
            for (int c = 0; c < cs.n_cats; ++c) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int64_t k = k0 + u * step;
                    const int c1 = k < t1 ? level_of(cs.codes[c], cs.drop[c], k) : -1;
                    if (jok && c1 >= 0) atomic_add(&tile[(cs.off[c] + c1) * TJ + jl], (lds_acc_t)x[u]);
                }
            }
        }
    }
    __syncthreads();
    store_tile(tile, cs.total, TJ, TJ, workgroup_slice(ws, stride));
}

// C-ordered dense, wide loads (the fast path for aligned operands and <= 8 categoricals):
// a wave step covers MCW_RS = 32 rows x TJ = 16 * VEC columns (VEC = columns per 16-byte load):
// 8 global_load_dwordx4 per lane bring the 32 rows in (16 lanes per row, 4 rows per instruction),
// d and the codes arrive lane <-> row with one coalesced load each and are parked in a per-wave
// LDS scratch as {d, byte offset of the level's tile row}, read back per 4-row group (4 distinct
// addresses per read).  The loads of step t + 1 are in flight while step t issues its atomics
// (two register sets, the loop is unrolled by two: no copies of in-flight loads).
// Tile layout [level][TJ] with the columns of a lane de-interleaved: column c sits at
// (c / VEC) + 16 * (c % VEC), so one ds_add covers 16 consecutive elements per row.
// The narrow kernel above spends one 8-byte load instruction per lane and element and reloads the
// codes in every lane: ~20 vector-memory instructions per 2 KB of the dense operand.
constexpr int MCW_RS = 32;
constexpr int MCW_VEC = 2;

template <typename F, int NC>
__global__ __launch_bounds__(1024) void multi_cat_dense_wide_kernel(
    CatSet cs, const F *__restrict__ d, const F *__restrict__ M, int64_t n, int64_t m,
    int64_t rows_per_block, F *__restrict__ ws, int64_t stride, const int32_t *__restrict__ rows,
    WgLogBuf *__restrict__ wglog) {
    const unsigned long long t_begin = wg_log_begin(wglog);
    // rows != NULL: `n` is the length of the row list and every position is mapped through it
    // (cost proportional to the list; the reference's `for k in rows`, ext/split.pyx:32-80)
    // VEC = 2 columns per lane for both types (16-byte loads for f64, 8-byte loads for f32): the
    // tile is made of doubles, and 32 columns per part is what fits LDS at a few hundred levels
    constexpr int VEC = MCW_VEC;
    constexpr int TJ = 16 * VEC;
    constexpr int NI = MCW_RS / 4;               // load instructions per step
    typedef F vec_t __attribute__((ext_vector_type(VEC)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);  // [total][TJ], lane-column de-interleaved
    const int nel = cs.total * TJ;
    zero_tile(tile, nel);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    // per-wave scratch: d[MCW_RS] then NC x int[MCW_RS] tile-row byte offsets (-1: no level)
    unsigned char *scr = scratch_behind_tile(smem_raw, nel) + (size_t)wave * MCW_RS * (sizeof(F) + NC * sizeof(int));
    F *sd = reinterpret_cast<F *>(scr);
    int *sc = reinterpret_cast<int *>(scr + MCW_RS * sizeof(F));
    __syncthreads();
    const int q = lane >> 4, jl = lane & 15;
    const int64_t j = (int64_t)blockIdx.y * TJ + jl * VEC;
    const int64_t jc = min(j, m - VEC);          // clamped (a part past the last column adds nothing)
    const bool jok = j < m;
    const int64_t t0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t t1 = min(t0 + rows_per_block, n);
    const int64_t step = (int64_t)nwave * MCW_RS;
    const int lr = lane & (MCW_RS - 1);          // row of the step this lane loads d / codes for

    struct Regs { vec_t x[NI]; F dk; int code[NC]; };
    auto load = [&](int64_t k0, Regs &R) {
        // (row list: all row ids first, then the row loads -- a row id fetched inside the loop was
        // waited for before the next one went out)
        int64_t kr[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) kr[i] = min(k0 + 4 * i + q, n - 1);
        if (rows) {
#pragma unroll
            for (int i = 0; i < NI; ++i) kr[i] = (int64_t)rows[kr[i]];
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            // (streamed once: nontemporal loads keep the dense block out of the L2 -- 2.01 -> 1.71 ms at cfg4)
            R.x[i] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(M + kr[i] * m + jc));
        }
        const int64_t k = k0 + lr;
        const int64_t kp = min(k, n - 1);
        const int64_t kc = rows ? (int64_t)rows[kp] : kp;
        R.dk = d[kc];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = level_of(cs.codes[c], cs.drop[c], kc);
            R.code[c] = (k < t1 && col >= 0) ? (cs.off[c] + col) * TJ * (int)sizeof(lds_acc_t) : -1;
        }
    };
    auto process = [&](const Regs &R) {
        __builtin_amdgcn_wave_barrier();
        if (lane < MCW_RS) {
            sd[lr] = R.dk;
#pragma unroll
            for (int c = 0; c < NC; ++c)     // rows with d == 0 contribute exactly nothing
                sc[c * MCW_RS + lr] = R.dk != F(0) ? R.code[c] : -1;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int row = 4 * i + q;
            const F dk = sd[row];
            int off[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) off[c] = sc[c * MCW_RS + row];
            vec_t x = R.x[i];
#pragma unroll
            for (int v = 0; v < VEC; ++v) x[v] *= dk;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (jok && off[c] >= 0) {
                    lds_acc_t *dst = reinterpret_cast<lds_acc_t *>(smem_raw + off[c]) + jl;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) atomic_add(dst + 16 * v, (lds_acc_t)x[v]);
                }
            }
        }
    };
    Regs ra, rb;
    int64_t k0 = t0 + (int64_t)wave * MCW_RS;
    if (k0 < t1) load(k0, ra);
    for (; k0 < t1; k0 += 2 * step) {
        const bool more = k0 + step < t1;
        if (more) load(k0 + step, rb);
        process(ra);
        if (more) {
            if (k0 + 2 * step < t1) load(k0 + 2 * step, ra);
            process(rb);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) wg_log_end(wglog, t_begin, WG_CAT_DENSE);
    F *dst = workgroup_slice(ws, stride);              // (the de-interleave is this kernel's own: not store_tile)
    for (int b = threadIdx.x; b < nel; b += blockDim.x) {
        const int c = b % TJ;
        dst[b] = (F)tile[(b / TJ) * TJ + (c / VEC) + 16 * (c % VEC)];
    }
}

// F-ordered dense: lane <-> row, loop over the TJ columns of the part.
template <typename F, int TJ>
__global__ __launch_bounds__(1024) void multi_cat_dense_f_kernel(
    CatSet cs, const F *__restrict__ d, const F *__restrict__ M, int64_t n, int64_t m,
    int64_t rows_per_block, F *__restrict__ ws, int64_t stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);
    const int nel = cs.total * TJ;
    zero_tile(tile, nel);
    __syncthreads();
    const int64_t j0 = (int64_t)blockIdx.y * TJ;
    const int64_t t0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t t1 = min(t0 + rows_per_block, n);
    for (int64_t k = t0 + threadIdx.x; k < t1; k += blockDim.x) {
        const F dk = d[k];
        int col[MAX_CATS];
#pragma unroll
        for (int c = 0; c < MAX_CATS; ++c)
            col[c] = c < cs.n_cats ? level_of(cs.codes[c], cs.drop[c], k) : -1;
        for (int jl = 0; jl < TJ && j0 + jl < m; ++jl) {
            const F x = dk * M[(j0 + jl) * n + k];
#pragma unroll
            for (int c = 0; c < MAX_CATS; ++c)
                if (col[c] >= 0) atomic_add(&tile[(cs.off[c] + col[c]) * TJ + jl], (lds_acc_t)x);
        }
    }
    __syncthreads();
    store_tile(tile, cs.total, TJ, TJ, workgroup_slice(ws, stride));
}

// tmp [part][total][TJ] -> out[total][m]
template <typename F>
__global__ void multi_cat_untile_kernel(const F *__restrict__ tmp, int64_t total, int64_t m,
                                        int TJ, F *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total * m) return;
    const int64_t a = e / m, j = e % m;
    out[e] = tmp[((j / TJ) * total + a) * TJ + (j % TJ)];
}

// Sparse operand in slab-blocked column-major form (sparse_slab.hip): part = one 32-column group,
// lane <-> nonzero of the (slab, group) stream.  The LDS tile has a row stride of
// group_cols + 1: consecutive stream entries belong to the same column (runs of ~6 rows), with an
// unpadded stride they would all fall on one bank pair.  STAGE: every wave first copies the
// codes and d of its 128-row slab into its own LDS scratch (coalesced loads), the per-nonzero
// lookups are then LDS reads instead of 64-lane global gathers.
template <typename F, bool STAGE>
__global__ __launch_bounds__(1024) void multi_cat_sparse_kernel(
    CatSet cs, const F *__restrict__ d, const F *__restrict__ vals,
    const unsigned *__restrict__ koff, const unsigned char *__restrict__ ecol,
    const int64_t *__restrict__ gptr, int n_groups, int64_t n_slabs, int64_t slabs_per_block,
    int slab_rows, int group_cols, int64_t n, F *__restrict__ ws, int64_t stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);  // [total][group_cols + 1]
    const int tstr = group_cols + 1;
    const int nel = cs.total * tstr;
    zero_tile(tile, nel);
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    // per-wave scratch (STAGE): d of the slab rows, then the codes of every categorical
    unsigned char *scratch = scratch_behind_tile(smem_raw, nel);
    F *sd = reinterpret_cast<F *>(scratch) + (size_t)wave * slab_rows;
    int32_t *sc = reinterpret_cast<int32_t *>(reinterpret_cast<F *>(scratch) + (size_t)nwave * slab_rows) +
                  (size_t)wave * cs.n_cats * slab_rows;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * slabs_per_block;
    const int64_t s1 = min(s0 + slabs_per_block, n_slabs);
    const unsigned rowb = 64u * (unsigned)sizeof(F);
    // every wave walks its own slabs (s0 + wave, + nwave, ...): 16 independent streams per
    // workgroup; the pointers of the next slab are requested before the current one is used
    int64_t nb = 0, ne = 0;
    if (s0 + wave < s1) {
        nb = gptr[(s0 + wave) * n_groups + g];
        ne = gptr[(s0 + wave) * n_groups + g + 1];
    }
    for (int64_t s = s0 + wave; s < s1; s += nwave) {
        const int64_t base = nb, end = ne;
        if (s + nwave < s1) {
            nb = gptr[(s + nwave) * n_groups + g];
            ne = gptr[(s + nwave) * n_groups + g + 1];
        }
        if (STAGE) {
            __builtin_amdgcn_wave_barrier();
            for (int r = lane; r < slab_rows; r += 64) {
                const int64_t k = min(s * slab_rows + r, n - 1);
                sd[r] = d[k];
                for (int c = 0; c < cs.n_cats; ++c) sc[c * slab_rows + r] = level_of(cs.codes[c], cs.drop[c], k);
            }
            __builtin_amdgcn_wave_barrier();
        }
        for (int64_t e0 = base + lane; e0 < end; e0 += 128) {
            const int64_t e1 = e0 + 64;
            const bool ok1 = e1 < end;
            const unsigned ko0 = koff[e0];
            const unsigned ko1 = ok1 ? koff[e1] : 0u;
            const F v0 = vals[e0];
            const F v1 = ok1 ? vals[e1] : F(0);
            const int ec0 = ecol[e0];
            const int ec1 = ok1 ? ecol[e1] : 0;
            const int r0 = (int)(ko0 / rowb), r1 = (int)(ko1 / rowb);
            const int64_t k0 = s * slab_rows + r0;
            const int64_t k1 = s * slab_rows + r1;
            const F d0 = STAGE ? sd[r0] : d[k0];
            const F d1 = ok1 ? (STAGE ? sd[r1] : d[k1]) : F(0);
            const F x0 = d0 != F(0) ? d0 * v0 : F(0);   // rows masked out by d == 0 contribute
            const F x1 = d1 != F(0) ? d1 * v1 : F(0);   // exactly nothing, whatever they hold
#pragma unroll 1
            for (int c = 0; c < cs.n_cats; ++c) {
                const int c0 = STAGE ? sc[c * slab_rows + r0] : level_of(cs.codes[c], cs.drop[c], k0);
                const int c1 = ok1 ? (STAGE ? sc[c * slab_rows + r1] : level_of(cs.codes[c], cs.drop[c], k1)) : -1;
                if (c0 >= 0) atomic_add(&tile[(cs.off[c] + c0) * tstr + ec0], (lds_acc_t)x0);
                if (c1 >= 0) atomic_add(&tile[(cs.off[c] + c1) * tstr + ec1], (lds_acc_t)x1);
            }
        }
    }
    __syncthreads();
    store_tile(tile, cs.total, tstr, group_cols, workgroup_slice(ws, stride));
}

// Fast variant for 1..4 categoricals: one (slab, group) block per wave step.  While a block is
// processed, the first 256 stream entries of the wave's NEXT block and the d / codes of that
// slab's 128 rows are already in flight into registers (one memory round trip per block, hidden
// behind the previous block's atomics); d and codes are then parked in per-wave LDS scratch so the
// per-nonzero lookups are LDS reads.
template <typename F, int NC>
__global__ __launch_bounds__(1024) void multi_cat_sparse_pf_kernel(
    CatSet cs, const F *__restrict__ d, const F *__restrict__ vals,
    const unsigned *__restrict__ koff, const unsigned char *__restrict__ ecol,
    const int64_t *__restrict__ gptr, int n_groups, int64_t n_slabs, int64_t slabs_per_block,
    int group_cols, int64_t n, F *__restrict__ ws, int64_t stride, WgLogBuf *__restrict__ wglog) {
    const unsigned long long t_begin = wg_log_begin(wglog);
    constexpr int SR = 128;              // slab rows (tm_slab_rows)
    constexpr int NQ = 4;                // prefetched 64-entry chunks per block
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);  // [total][group_cols + 1]
    const int tstr = group_cols + 1;
    const int nel = cs.total * tstr;
    zero_tile(tile, nel);
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    unsigned char *scratch = scratch_behind_tile(smem_raw, nel);
    F *sd = reinterpret_cast<F *>(scratch) + (size_t)wave * SR;
    int32_t *sc = reinterpret_cast<int32_t *>(reinterpret_cast<F *>(scratch) + (size_t)nwave * SR) +
                  (size_t)wave * NC * SR;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * slabs_per_block;
    const int64_t s1 = min(s0 + slabs_per_block, n_slabs);
    const unsigned rowb = 64u * (unsigned)sizeof(F);

    // pointers two blocks ahead, stream + row data one block ahead
    int64_t q_base = 0, q_end = 0;
    int64_t p_base = 0, p_end = 0;
    unsigned p_ko[NQ];
    F p_v[NQ];
    int p_ec[NQ];
    F p_d[2];
    int p_c[NC][2];
    auto load_ptrs = [&](int64_t s) {
        q_base = q_end = 0;
        if (s < s1) {
            q_base = gptr[s * n_groups + g];
            q_end = gptr[s * n_groups + g + 1];
        }
    };
    auto load_block = [&](int64_t s) {     // consumes the pointers, issues the loads of block s
        p_base = q_base;
        p_end = q_end;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int64_t e = p_base + q * 64 + lane;
            const int64_t ec = min(e, max(p_end - 1, p_base));     // clamped: branch-free issue
            const bool ok = e < p_end;
            p_ko[q] = ok ? koff[ec] : 0u;
            p_v[q] = ok ? vals[ec] : F(0);
            p_ec[q] = ok ? (int)ecol[ec] : 0;
        }
        if (s < s1) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t k = min(s * SR + lane + 64 * h, n - 1);
                p_d[h] = d[k];
#pragma unroll
                for (int c = 0; c < NC; ++c) p_c[c][h] = level_of(cs.codes[c], cs.drop[c], k);
            }
        }
    };
    const int64_t sw = s0 + wave;
    load_ptrs(sw);
    load_block(sw);
    load_ptrs(sw + nwave);
    for (int64_t s = sw; s < s1; s += nwave) {
        // take over the prefetched block
        const int64_t base = p_base, end = p_end;
        unsigned ko[NQ];
        F v[NQ];
        int ec[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { ko[q] = p_ko[q]; v[q] = p_v[q]; ec[q] = p_ec[q]; }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            sd[lane + 64 * h] = p_d[h];
#pragma unroll
            for (int c = 0; c < NC; ++c) sc[c * SR + lane + 64 * h] = p_c[c][h];
        }
        __builtin_amdgcn_wave_barrier();
        load_block(s + nwave);
        load_ptrs(s + 2 * nwave);
        auto scatter = [&](unsigned kk, F vv, int ee) {
            const int r = (int)(kk / rowb);
            const F dk = sd[r];
            const F x = dk != F(0) ? dk * vv : F(0);   // rows masked out by d == 0 contribute nothing
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int cc = sc[c * SR + r];
                if (cc >= 0) atomic_add(&tile[(cs.off[c] + cc) * tstr + ee], (lds_acc_t)x);
            }
        };
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (base + q * 64 + lane < end) scatter(ko[q], v[q], ec[q]);
        // blocks longer than the prefetch window (dense columns): the rest straight from memory
        for (int64_t e = base + NQ * 64 + lane; e < end; e += 64) scatter(koff[e], vals[e], (int)ecol[e]);
    }
    __syncthreads();
    if (threadIdx.x == 0) wg_log_end(wglog, t_begin, WG_CAT_SPARSE);
    store_tile(tile, cs.total, tstr, group_cols, workgroup_slice(ws, stride));
}

// The same fused categorical x sparse cross terms on the ENTRY twin of the sparse block (round 4: the stream K3
// walks, csrc/sparse_ent.hip / tabmat_amd/ext/_types.py::SlabEnt -- {value, row << 4 | column in group} in batches
// of 16 slots, blocks of a 16-column group slab after slab), so that a design whose sparse x dense term runs on the
// entry kernel needs no slab-form twin (3.4 GB at BASELINE configs[3]) for this term.  A workgroup owns TWO column
// groups (32 kernel columns: tile [total levels][33] of doubles, as the slab kernel) over a range of slabs; its
// waves alternate between the two groups and cut the range among themselves; lane <-> slot, 64 slots per step.
// The d and the codes of a slot's row are gathered from global memory (rows of a (group, slab) block lie within
// 64 rows: the lines stay in the L1 / L2); the stream of the step after next and the gathers of the next step are
// in flight while the current one is scattered (the slab kernel's lesson: it was latency-bound, not atomic-bound).
#ifndef EN_CS_U
#define EN_CS_U 4
#endif
template <typename F, int NC>
__global__ __launch_bounds__(1024) void multi_cat_sparse_ent_kernel(
    CatSet cs, const F *__restrict__ d, const F *__restrict__ vals, const unsigned short *__restrict__ meta,
    const unsigned *__restrict__ bstart, int n_groups, int64_t n, int64_t n_slabs, int64_t slabs_per_block,
    F *__restrict__ ws, int64_t stride, const unsigned *__restrict__ packed) {
    // packed (round 5, may be NULL; NC <= 3): packed[row] = the tile rows of the row's levels, 10 bits each (1023 =
    // none: missing / dropped level), built once per matrix by tm_multi_cat_pack_codes -- ONE gather per slot
    // instead of NC (the kernel is bound by its dependent loads: no gathers at all 0.60 ms against 1.02,
    // profiles/r4_catsparse.txt)
    constexpr int GC = 32, TSTR = GC + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);  // [total][33]
    const int nel = cs.total * TSTR;
    zero_tile(tile, nel);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int h = wave & 1;                               // which of the pair's two groups
    const int g = 2 * blockIdx.y + h;
    const int nwh = (nwave + 1 - h) / 2;                  // waves on this group
    const int wi = wave >> 1;
    const int64_t s0 = (int64_t)blockIdx.x * slabs_per_block;
    const int64_t s1 = min(s0 + slabs_per_block, n_slabs);
    if (g < n_groups && s1 > s0) {
        const int64_t spw = (s1 - s0 + nwh - 1) / nwh;
        const int64_t sa = min(s0 + (int64_t)wi * spw, s1), sb = min(sa + spw, s1);
        const unsigned *brow = bstart + (int64_t)g * (n_slabs + 1);
        const int64_t e0 = (int64_t)brow[sa] * 16, e1 = (int64_t)brow[sb] * 16;     // slots of the wave
        // U x 64 slots per step and lane: the kernel is bound by the memory round trips of its two dependent
        // loads (stream -> d / codes of the row), not by the atomics -- more of them in flight per wave
        constexpr int U = EN_CS_U;
        struct Step { F v[U]; unsigned m[U]; F dk[U]; int c[U][NC]; };
        auto load_stream = [&](int64_t e, Step &t) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = e + 64 * u + lane < e1;
                const int64_t i = ok ? e + 64 * u + lane : (e1 > e0 ? e1 - 1 : 0);
                t.v[u] = ok ? vals[i] : F(0);
                t.m[u] = meta[i];
            }
        };
        // (round 6: 16-bit meta words {slab & 63, row in slab, column}: the slab of a slot from the tag and a running
        // slab, in stream order -- load_rows is called step after step; rows of slots behind the wave's stream clamped.
        // All 64 lanes of a sub-step use ONE running slab, replaced by lane 63's slab afterwards: right because the
        // builder keeps any five consecutive batches of a group, and the first four at or after any slab sa, within 63
        // slabs -- SlabEnt.CONT_PERIOD, tests/test_ent_stream_ranges.py)
        unsigned cur_slab = (unsigned)sa;
        const unsigned row_max = (unsigned)(n - 1);
        auto load_rows = [&](Step &t) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned slab = cur_slab + (((t.m[u] >> 10) - cur_slab) & 63u);
                cur_slab = (unsigned)__builtin_amdgcn_readlane((int)slab, 63);
                const unsigned row = min((slab << 6) | ((t.m[u] >> 4) & 63u), row_max);
                t.dk[u] = d[row];
                if (NC <= 3 && packed != nullptr) {
                    const unsigned pk = packed[row];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const int f = packed_field(pk, c);
                        t.c[u][c] = f == PACKED_NONE ? -1 : f - cs.off[c];
                    }
                    continue;
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) t.c[u][c] = level_of(cs.codes[c], cs.drop[c], row);
            }
        };
        if (e1 > e0) {
            Step cur, nxt, nx2;
            load_stream(e0, cur);
            load_stream(e0 + 64 * U, nxt);
            load_rows(cur);
            for (int64_t e = e0; e < e1; e += 64 * U) {
                load_stream(e + 128 * U, nx2);
                load_rows(nxt);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    // rows masked out by d == 0 (and padding slots: value 0) contribute exactly nothing
                    const F x = (cur.dk[u] != F(0) && cur.v[u] != F(0)) ? cur.dk[u] * cur.v[u] : F(0);
                    const int col = 16 * h + (int)(cur.m[u] & 15u);
                    if (x != F(0)) {
#pragma unroll
                        for (int c = 0; c < NC; ++c)
                            if (cur.c[u][c] >= 0)
                                atomic_add(&tile[(cs.off[c] + cur.c[u][c]) * TSTR + col], (lds_acc_t)x);
                    }
                }
                cur = nxt;
                nxt = nx2;
            }
        }
    }
    __syncthreads();
    store_tile(tile, cs.total, TSTR, GC, workgroup_slice(ws, stride));
}

// The same on the entry twin with the per-row operands STAGED (round 6).  The kernel above is bound
// by its dependent loads: stream -> {d, codes} of the slot's row (no gathers at all 0.60 ms against 1.02,
// profiles/r4_catsparse.txt).  A (group, slab) block only names rows of ITS 64-row slab, and a wave walks the slabs of
// its range in order, so what a slot needs of its row is known without looking at the stream: the wave loads d and the
// code word(s) of the slab's 64 rows lane <-> row (two coalesced loads), EN_CS_D slabs ahead together with the block's
// stream, parks them in 768 bytes of per-wave LDS when the slab's turn comes, and every slot reads its row's pair from
// there -- no load depends on another load.  One step of 64 slots per block (a block of more than 64 slots: further
// steps straight from memory; 3 % of the blocks at BASELINE configs[3]).  PK: the packed code word of
// tm_multi_cat_pack_codes (NC <= 3), else NC code words per row.
#ifndef EN_CS_D
#define EN_CS_D 4
#endif
#ifndef EN_CS_BOTH
#define EN_CS_BOTH 1
#endif
template <typename F, int NC, bool PK>
__global__ __launch_bounds__(1024) void multi_cat_sparse_ent_staged_kernel(
    CatSet cs, const F *__restrict__ d, const F *__restrict__ vals, const unsigned short *__restrict__ meta,
    const unsigned *__restrict__ bstart, int n_groups, int64_t n, int64_t n_slabs, int64_t slabs_per_block,
    F *__restrict__ ws, int64_t stride, const unsigned *__restrict__ packed, int tile_bytes) {
    constexpr int GC = 32, TSTR = GC + 1;
    constexpr int NCW = PK ? 1 : NC;                      // staged code words per row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);  // [total][33]
    const int nel = cs.total * TSTR;
    zero_tile(tile, nel);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwave = blockDim.x >> 6;
    F *sd = reinterpret_cast<F *>(smem_raw + tile_bytes) + wave * 64;                                      // d of the slab's rows
    int *sc = reinterpret_cast<int *>(smem_raw + tile_bytes + (size_t)nwave * 64 * sizeof(F)) + wave * 64 * NCW;
    // EN_CS_BOTH: a wave walks BOTH groups of the pair over its slabs (the rows' operands are fetched and parked once per
    // slab for two blocks: 10 instead of 12 loads and 2 instead of 4 staging writes per slab and pair); else the waves
    // alternate between the two groups.
    constexpr int NG = EN_CS_BOTH ? 2 : 1;
    const int h0 = EN_CS_BOTH ? 0 : (wave & 1);
    const int g0 = 2 * blockIdx.y + h0;
    const int nwh = EN_CS_BOTH ? nwave : (nwave + 1 - h0) / 2;     // waves that share this group's slabs
    const int wi = EN_CS_BOTH ? wave : (wave >> 1);
    const int64_t s0 = (int64_t)blockIdx.x * slabs_per_block;
    const int64_t s1 = min(s0 + slabs_per_block, n_slabs);
    if (g0 < n_groups && s1 > s0) {
        const int64_t spw = (s1 - s0 + nwh - 1) / nwh;
        const int64_t sa = min(s0 + (int64_t)wi * spw, s1), sb = min(sa + spw, s1);
        // (an odd number of groups: the last pair's second group does not exist -- its bounds are read from the first
        // group's row and its blocks count as empty)
        const bool has[2] = {true, g0 + 1 < n_groups};
        const unsigned *brow[2] = {bstart + (int64_t)g0 * (n_slabs + 1),
                                   bstart + (int64_t)(has[1] ? g0 + 1 : g0) * (n_slabs + 1)};
        // Every load of the walk is UNCONDITIONAL (clamped addresses, results masked afterwards): the compiler can only
        // count its waits (s_waitcnt vmcnt(N) for the requests of EN_CS_D slabs ago, the newer ones stay in flight)
        // over loads it knows were issued -- a first version with the loads behind `if (slot < slots of the block)`
        // waited with vmcnt(0) in front of every slab, one memory round trip per slab: 1.27 ms against 0.94 for the
        // gather kernel.  Three stages, EN_CS_D slabs apart: block bounds (two broadcast loads) -> stream + the rows'
        // operands -> scatter.
        struct Bnd { unsigned b0[NG], b1[NG]; };
        struct Pre { F v[NG]; unsigned m[NG]; F dd; int c[NCW]; unsigned b0[NG]; int nsl[NG]; };
        // (the bounds through VECTOR loads at a lane-invariant address the compiler cannot see through: scalar loads
        // share their counter with the LDS atomics, every use would wait for those too)
        int vz = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
#endif
        auto request_bounds = [&](int64_t s, Bnd &q) {
            const int64_t sc_ = min(s, sb - 1) + vz;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                q.b0[k] = brow[k][sc_];
                q.b1[k] = brow[k][sc_ + 1];
            }
        };
        auto request = [&](int64_t s, const Bnd &q, Pre &p) {
            const bool live = s < sb;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const unsigned qb0 = (unsigned)__builtin_amdgcn_readfirstlane((int)q.b0[k]);
                const unsigned qb1 = (unsigned)__builtin_amdgcn_readfirstlane((int)q.b1[k]);
                p.b0[k] = qb0;
                p.nsl[k] = (live && has[k]) ? (int)(qb1 - qb0) * 16 : 0;
                const bool ok = lane < p.nsl[k];
                const int64_t e = (int64_t)qb0 * 16 + (ok ? lane : 0);        // (slot b0 * 16 exists: slack behind the stream)
                const F v = __builtin_nontemporal_load(vals + e);
                p.m[k] = __builtin_nontemporal_load(meta + e);
                p.v[k] = ok ? v : F(0);
            }
            const int64_t row_ = min(s, sb - 1) * 64 + lane;
            const int64_t row = min(row_, n - 1);              // (ragged last slab: no slot names a row beyond n - 1)
            p.dd = d[row];
            if constexpr (PK) {
                p.c[0] = (int)packed[row];
            } else {
#pragma unroll
                for (int c = 0; c < NC; ++c) p.c[c] = level_of(cs.codes[c], cs.drop[c], row);
            }
        };
        auto process = [&](Pre &p) {
            int any = 0;
#pragma unroll
            for (int k = 0; k < NG; ++k) any |= p.nsl[k];
            if (any == 0) return;
            sd[lane] = p.dd;
#pragma unroll
            for (int c = 0; c < NCW; ++c) sc[c * 64 + lane] = p.c[c];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                F v = p.v[k];
                unsigned m = p.m[k];
                const int cbase = 16 * (h0 + k);
                for (int off = 0; off < p.nsl[k]; off += 64) {
                    if (off > 0) {                 // a block of more than 64 slots: the rest straight from memory
                        const bool ok = off + lane < p.nsl[k];
                        const int64_t e = (int64_t)p.b0[k] * 16 + off + (ok ? lane : 0);
                        v = ok ? vals[e] : F(0);
                        m = meta[e];
                    }
                    const int r6 = (int)((m >> 4) & 63u);
                    const int col = cbase + (int)(m & 15u);
                    const F dk = sd[r6];
                    // rows masked out by d == 0 (and padding slots: value 0) contribute exactly nothing
                    const F x = (dk != F(0) && v != F(0)) ? dk * v : F(0);
                    if (x != F(0)) {
                        if constexpr (PK) {
                            const unsigned pk = (unsigned)sc[r6];
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                const int f = packed_field(pk, c);
                                if (f != PACKED_NONE) atomic_add(&tile[f * TSTR + col], (lds_acc_t)x);
                            }
                        } else {
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                const int cc = sc[c * 64 + r6];
                                if (cc >= 0) atomic_add(&tile[(cs.off[c] + cc) * TSTR + col], (lds_acc_t)x);
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        };
        constexpr int DEPTH = EN_CS_D;             // slabs in flight per wave and stage
        Pre p[DEPTH];
        Bnd q[DEPTH];
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) request_bounds(sa + j, q[j]);
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            request(sa + j, q[j], p[j]);
            request_bounds(sa + DEPTH + j, q[j]);
        }
        for (int64_t s = sa; s < sb; s += DEPTH) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                process(p[j]);
                request(s + DEPTH + j, q[j], p[j]);
                request_bounds(s + 2 * DEPTH + j, q[j]);
            }
        }
    }
    __syncthreads();
    store_tile(tile, cs.total, TSTR, GC, workgroup_slice(ws, stride));
}

// Row-list form of the fused categorical x sparse cross terms (the reference's cost for `rows=` is
// proportional to len(rows): categorical_matrix.py:825-838 works on self[rows]): the selected rows'
// entry lists come from the chunk-major twin through a {start, end} table [chunk][selected row]
// (the table the row-list K2 uses), part = one 32-column group of a 128-column chunk, tile
// [total levels][33] of doubles in LDS.  8 lanes per selected row walk its list in the group's
// chunk and keep the entries of the group; codes and d are read once per row.
// (IX = uint8_t: the columns as bytes inside their 128-column chunk, round 6)
template <typename F, typename IX>
__global__ __launch_bounds__(1024) void multi_cat_sparse_rows_kernel(
    CatSet cs, const F *__restrict__ cm_data, const IX *__restrict__ cm_ind,
    const int32_t *__restrict__ ranges, const int32_t *__restrict__ rows, const F *__restrict__ d_sel,
    int64_t n_sel, int64_t rows_per_block, F *__restrict__ ws, int64_t stride) {
    constexpr int GC = 32;                       // columns per group
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_acc_t *tile = reinterpret_cast<lds_acc_t *>(smem_raw);  // [total][GC + 1]
    constexpr int tstr = GC + 1;
    const int nel = cs.total * tstr;
    zero_tile(tile, nel);
    __syncthreads();
    // (the u8 column twin counts from its chunk's first column: `g >> 2` and `g & 3` below are group / chunk and
    // group % chunk only while a chunk holds exactly four groups)
    static_assert(SPARSE_CHUNK_COLS == 4 * GC, "the chunk of the chunk-major twin must hold four 32-column groups");
    const int g = blockIdx.y;                    // 32-column group; chunk = g / 4
    const int ch = g >> 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int lr = lane >> 3, lt = lane & 7;
    const int64_t t0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t t1 = min(t0 + rows_per_block, n_sel);
    const int32_t *rg = ranges + (int64_t)ch * n_sel * 2;
    for (int64_t k0 = t0 + wave * 8; k0 < t1; k0 += (int64_t)nwave * 8) {
        const int64_t k = k0 + lr;
        if (k >= t1) continue;
        const F dk = d_sel[k];
        if (dk == F(0)) continue;                // rows with d == 0 contribute exactly nothing
        const int e0 = rg[2 * k], e1 = rg[2 * k + 1];
        if (e0 >= e1) continue;
        const int64_t row = rows[k];
        int off[MAX_CATS];
#pragma unroll
        for (int c = 0; c < MAX_CATS; ++c) {
            off[c] = -1;
            if (c < cs.n_cats) {
                const int col = level_of(cs.codes[c], cs.drop[c], row);
                off[c] = col >= 0 ? (cs.off[c] + col) * tstr : -1;
            }
        }
        for (int e = e0 + lt; e < e1; e += 8) {
            const int col = (int)cm_ind[e] - (sizeof(IX) == 1 ? (g & 3) : g) * GC;
            if (col < 0 || col >= GC) continue;
            const lds_acc_t x = (lds_acc_t)(dk * cm_data[e]);
#pragma unroll
            for (int c = 0; c < MAX_CATS; ++c)
                if (off[c] >= 0) atomic_add(&tile[off[c] + col], x);
        }
    }
    __syncthreads();
    store_tile(tile, cs.total, tstr, GC, workgroup_slice(ws, stride));
}

// packed[row] = sum_c field_c << (PACKED_BITS c), field_c = tile row of the row's level in categorical c (cs.off[c] +
// code - drop) or PACKED_NONE when the row has none there (missing code, dropped first level)
__global__ __launch_bounds__(256) void multi_cat_pack_codes_kernel(CatSet cs, int64_t n, unsigned *__restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        unsigned pk = 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned f = (unsigned)PACKED_NONE;
            if (c < cs.n_cats) {
                const int col = level_of(cs.codes[c], cs.drop[c], r);
                if (col >= 0 && col < cs.ncol[c]) f = (unsigned)(cs.off[c] + col);
            }
            pk |= f << (PACKED_BITS * c);
        }
        out[r] = pk;
    }
}

// ---------------------------------------------------------------------------------------
// host: the one path from a tile kernel's partials to `out`
// ---------------------------------------------------------------------------------------
// LDS a workgroup may ask for (the CU has LDS_BYTES = 160 KB).  A tile alone: HIST_LDS_MAX, 128 KB (common.hpp).
// Tile plus the per-wave scratch of the wide dense and the slab kernels (d and codes of a wave step / a slab):
constexpr size_t TILE_SCRATCH_LDS_MAX = 150 * 1024;
// ... and tile plus the staged entry kernel's 768 bytes per wave (d and code words of a 64-row slab):
constexpr size_t ENT_STAGED_LDS_MAX = 156 * 1024;

static int make_catset(const void *const *h_codes, const int64_t *h_ncols, const int32_t *h_drop,
                       int n_cats, CatSet *cs) {
    if (n_cats < 1 || n_cats > MAX_CATS) {
        set_error("multi-cat call supports 1..%d categoricals, got %d", MAX_CATS, n_cats);
        return TM_EINVAL;
    }
    int off = 0;
    for (int c = 0; c < MAX_CATS; ++c) {
        cs->codes[c] = c < n_cats ? reinterpret_cast<const int32_t *>(h_codes[c]) : nullptr;
        cs->ncol[c] = c < n_cats ? (int)h_ncols[c] : 0;
        cs->drop[c] = c < n_cats ? h_drop[c] : 0;
        cs->off[c] = off;
        off += cs->ncol[c];
    }
    cs->n_cats = n_cats;
    cs->total = off;
    return TM_OK;
}

// Prologue of every launcher: the CatSet, and the two answers that need no kernel -- an empty result, and no rows
// (`units` rows or selected rows: out = 0; otherwise the untile kernel writes every element).  *done: nothing to launch.
template <typename F>
static int fused_begin(const void *const *h_codes, const int64_t *h_ncols, const int32_t *h_drop, int n_cats,
                       int64_t units, int64_t m, F *out, hipStream_t st, CatSet *cs, bool *done) {
    *done = true;
    int rc = make_catset(h_codes, h_ncols, h_drop, n_cats, cs);
    if (rc) return rc;
    const int64_t total = (int64_t)cs->total * m;
    if (total == 0) return TM_OK;
    if (units == 0) {
        TM_HIP(hipMemsetAsync(out, 0, sizeof(F) * (size_t)total, st));
        return TM_OK;
    }
    *done = false;
    return TM_OK;
}

// ... and its last check: the tile [stacked levels][columns of a part] must fit the LDS
static int tile_fits(const char *what, const CatSet &cs, size_t tile_bytes) {
    if (tile_bytes <= HIST_LDS_MAX) return TM_OK;
    set_error("%s: %d stacked categories exceed the LDS tile", what, cs.total);
    return TM_EUNSUPPORTED;
}

// `units` (rows, selected rows or slabs) cut into contiguous workgroup ranges for a grid of `parts` column parts:
// `rounds_knob` (1 without a knob) rounds of workgroups over the chip, no range shorter than `min_units`, ranges a
// multiple of `align`.
struct RangeCut {
    int64_t nblk, per;     // workgroups per part, units per workgroup
};
static RangeCut cut_ranges(int64_t units, int64_t parts, const char *rounds_knob, int64_t min_units, int64_t align) {
    const int64_t rounds = rounds_knob ? tune(rounds_knob, 1) : 1;
    int64_t nblk = std::max<int64_t>(1, rounds * NUM_CU / parts);
    nblk = std::min<int64_t>(nblk, std::max<int64_t>(1, ceil_div(units, min_units)));
    const int64_t per = ceil_div(ceil_div(units, nblk), align) * align;
    return {ceil_div(units, per), per};
}

// How a tile kernel's partials become `out` [cs.total][m] (part_cols: TJ of the dense kernels, group_cols of the slab
// kernels, 32 = a pair of 16-column groups of the entry kernels).  The workspace holds tmp [parts][cs.total][part_cols] and the
// partials ws [parts][nblk][cs.total * part_cols]; `launch(grid, block, ws, stride)` launches `kern` (timed as the
// op's main kernel), whose workgroups each leave one slice of ws; the slices are summed in a fixed order into tmp
// (reduce.hpp) and tmp is untiled into out.
template <typename F, typename Kern, typename Launch>
static int launch_and_finish(Kern kern, int64_t nblk, int64_t parts, int threads, size_t lds, const CatSet &cs,
                             int part_cols, int64_t m, F *out, hipStream_t st, Launch &&launch) {
    const int64_t stride = (int64_t)cs.total * part_cols;
    const size_t tmp_bytes = ((sizeof(F) * (size_t)(parts * stride) + 255) / 256) * 256;
    void *wsv = nullptr;
    int rc = get_workspace(tmp_bytes + sizeof(F) * (size_t)(parts * nblk * stride) + 256, &wsv, st);
    if (rc) return rc;
    F *tmp = reinterpret_cast<F *>(wsv);
    F *ws = reinterpret_cast<F *>(reinterpret_cast<char *>(wsv) + tmp_bytes);
    if (lds > 48 * 1024)
        TM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    prof_begin(st);
    launch(dim3((unsigned)nblk, (unsigned)parts), dim3((unsigned)threads), ws, stride);
    prof_end(st);
    TM_LAUNCH_CHECK();
    rc = launch_reduce_partials<F>(ws, stride, (int)nblk, (int)parts, tmp, parts * stride, false, st);
    if (rc) return rc;
    hipLaunchKernelGGL((multi_cat_untile_kernel<F>), dim3((unsigned)ceil_div((int64_t)cs.total * m, 256)), dim3(256), 0,
                       st, tmp, (int64_t)cs.total, m, part_cols, out);
    TM_LAUNCH_CHECK();
    return TM_OK;
}

// f(integral_constant<int, NC>) with NC = n_cats for 1 .. MAX_NC categoricals and NC = OVER above (0: a kernel's
// generic rung; MAX_NC itself where the caller has refused more) -- the kernels' NC template parameter
template <int MAX_NC, int OVER = MAX_NC, int NC = 1, typename Fn>
static int dispatch_nc(int n_cats, Fn &&f) {
    if constexpr (NC > MAX_NC) return f(std::integral_constant<int, OVER>{});
    else return n_cats == NC ? f(std::integral_constant<int, NC>{}) : dispatch_nc<MAX_NC, OVER, NC + 1>(n_cats, f);
}

// f(integral_constant<int, TJ>) for TJ = 64, 32 .. 1: the narrow dense kernels' columns per part
template <int TJ = 64, typename Fn>
static int dispatch_tj(int tj, Fn &&f) {
    if (tj == TJ) return f(std::integral_constant<int, TJ>{});
    if constexpr (TJ > 1) return dispatch_tj<TJ / 2>(tj, f);
    return TM_EINVAL;
}

// waves per workgroup of the kernels that size their scratch by it: 16 own a CU; 12 leave registers (and LDS) for the
// co-resident syrk (syrk_co.hip)
static int waves_knob(const char *knob, int dflt) {
    return (int)std::min<int64_t>(16, std::max<int64_t>(4, tune(knob, dflt)));
}

template <typename F>
static int run_multi_cat_dense(const void *const *h_codes, const int64_t *h_ncols,
                               const int32_t *h_drop, int n_cats, int64_t n, const F *d, const F *M,
                               int64_t m, int order_f, F *out, hipStream_t st,
                               const int32_t *rows = nullptr, int64_t n_rows = 0) {
    if (rows != nullptr) n = n_rows;          // positions of the row list from here on
    CatSet cs;
    bool done;
    int rc = fused_begin(h_codes, h_ncols, h_drop, n_cats, n, m, out, st, &cs, &done);
    if (rc || done) return rc;
    // wide-load path: C-ordered, 16-byte aligned rows, <= 8 categoricals, tile + scratch in LDS
    constexpr int TJW = 16 * MCW_VEC;
    const size_t tile_b = tile_lds_bytes((size_t)cs.total * TJW);
    const size_t lds_w = tile_b + (size_t)16 * MCW_RS * (sizeof(F) + (size_t)n_cats * sizeof(int));
    if (!order_f && n_cats <= 8 && m >= MCW_VEC && m % MCW_VEC == 0 &&
        (reinterpret_cast<uintptr_t>(M) & 15) == 0 && lds_w <= TILE_SCRATCH_LDS_MAX &&
        (int64_t)cs.total * TJW * (int64_t)sizeof(lds_acc_t) < (1ll << 30)) {
        const int64_t n_parts = ceil_div(m, TJW);
        const RangeCut cut = cut_ranges(n, n_parts, "catdense_rounds", 4096, MCW_RS);
        // With a large f64 tile (cfg4: 384 levels x 32 columns = 96 KB) EIGHT waves are faster -- 1.63 against
        // 1.82 ms alone, 14.6 against 15.0 ms for the whole cfg4 step (fewer waves queue on the LDS
        // atomic pipe; 6, 10 and 12 waves gain nothing); small tiles and f32 stay at 16
        const int nw = waves_knob("catdense_waves", (sizeof(F) == 8 && tile_b > 64 * 1024) ? 8 : 16);
        return dispatch_nc<8>(n_cats, [&](auto nc) {
            auto kern = &multi_cat_dense_wide_kernel<F, decltype(nc)::value>;
            auto launch = [&](dim3 grid, dim3 block, F *ws, int64_t stride) {
                hipLaunchKernelGGL(kern, grid, block, lds_w, st, cs, d, M, n, m, cut.per, ws, stride, rows, wg_log_ptr());
            };
            return launch_and_finish<F>(kern, cut.nblk, n_parts, nw * 64, lds_w, cs, TJW, m, out, st, launch);
        });
    }
    if (rows != nullptr) {
        set_error("multi_cat_dense: the row-list form needs the wide-load path");
        return TM_EUNSUPPORTED;
    }
    int TJ = 64;
    while (TJ > 1 && sizeof(lds_acc_t) * (size_t)cs.total * TJ > HIST_LDS_MAX) TJ >>= 1;
    while (TJ > 1 && TJ / 2 >= m) TJ >>= 1;
    const size_t lds = sizeof(lds_acc_t) * (size_t)cs.total * TJ;
    rc = tile_fits("multi_cat_dense", cs, lds);
    if (rc) return rc;
    const int64_t n_parts = ceil_div(m, TJ);
    const RangeCut cut = cut_ranges(n, n_parts, nullptr, 4096, 1);
    return dispatch_tj(TJ, [&](auto tj) {
        auto go = [&](auto kern) {
            auto launch = [&](dim3 grid, dim3 block, F *ws, int64_t stride) {
                hipLaunchKernelGGL(kern, grid, block, lds, st, cs, d, M, n, m, cut.per, ws, stride);
            };
            return launch_and_finish<F>(kern, cut.nblk, n_parts, 1024, lds, cs, TJ, m, out, st, launch);
        };
        constexpr int V = decltype(tj)::value;
        if (order_f) return go(&multi_cat_dense_f_kernel<F, V>);
        return dispatch_nc<4, 0>(n_cats, [&](auto nc) { return go(&multi_cat_dense_c_kernel<F, V, decltype(nc)::value>); });
    });
}

template <typename F>
static int run_multi_cat_sparse(const void *const *h_codes, const int64_t *h_ncols,
                                const int32_t *h_drop, int n_cats, int64_t n, const F *d,
                                const F *vals, const unsigned *koff, const unsigned char *ecol,
                                const int64_t *gptr, int64_t m, int slab_rows, int group_cols,
                                F *out, hipStream_t st) {
    CatSet cs;
    bool done;
    int rc = fused_begin(h_codes, h_ncols, h_drop, n_cats, n, m, out, st, &cs, &done);
    if (rc || done) return rc;
    const size_t tile_bytes = tile_lds_bytes((size_t)cs.total * (group_cols + 1));
    rc = tile_fits("multi_cat_sparse", cs, tile_bytes);
    if (rc) return rc;
    // per-wave staging of the slab's d and codes when it fits next to the tile
    const int nw = waves_knob("catsparse_waves", 16);
    const size_t stage_bytes = (size_t)nw * slab_rows * (sizeof(F) + sizeof(int32_t) * (size_t)n_cats);
    const bool stage = tile_bytes + stage_bytes <= TILE_SCRATCH_LDS_MAX;
    const size_t lds = tile_bytes + (stage ? stage_bytes : 0);
    const int n_groups = (int)ceil_div(m, group_cols);
    const int64_t n_slabs = ceil_div(n, slab_rows);
    const RangeCut cut = cut_ranges(n_slabs, n_groups, "catsparse_rounds", 1, 1);
    if (stage && n_cats <= 8 && slab_rows == 128)
        return dispatch_nc<8>(n_cats, [&](auto nc) {
            auto kern = &multi_cat_sparse_pf_kernel<F, decltype(nc)::value>;
            auto launch = [&](dim3 grid, dim3 block, F *ws, int64_t stride) {
                hipLaunchKernelGGL(kern, grid, block, lds, st, cs, d, vals, koff, ecol, gptr, n_groups, n_slabs, cut.per,
                                   group_cols, n, ws, stride, wg_log_ptr());
            };
            return launch_and_finish<F>(kern, cut.nblk, n_groups, nw * 64, lds, cs, group_cols, m, out, st, launch);
        });
    auto kern = stage ? &multi_cat_sparse_kernel<F, true> : &multi_cat_sparse_kernel<F, false>;
    auto launch = [&](dim3 grid, dim3 block, F *ws, int64_t stride) {
        hipLaunchKernelGGL(kern, grid, block, lds, st, cs, d, vals, koff, ecol, gptr, n_groups, n_slabs, cut.per,
                           slab_rows, group_cols, n, ws, stride);
    };
    return launch_and_finish<F>(kern, cut.nblk, n_groups, nw * 64, lds, cs, group_cols, m, out, st, launch);
}

// entry-twin form (see multi_cat_sparse_ent_kernel): out [total levels][mk], mk = 16 * groups kernel columns
template <typename F>
static int run_multi_cat_sparse_ent(const void *const *h_codes, const int64_t *h_ncols, const int32_t *h_drop,
                                    int n_cats, int64_t n, const F *d, const F *vals, const unsigned short *meta,
                                    const unsigned *bstart, int64_t mk, F *out, hipStream_t st,
                                    const unsigned *packed = nullptr, int64_t n_slots = 0) {
    CatSet cs;
    bool done;
    int rc = fused_begin(h_codes, h_ncols, h_drop, n_cats, n, mk, out, st, &cs, &done);
    if (rc || done) return rc;
    TM_REQUIRE(mk % 16 == 0 && n_cats >= 1 && n_cats <= 8, "kernel columns in groups of 16, 1 .. 8 categoricals");
    TM_REQUIRE(n < (1ll << 28), "at most 2^28 - 1 rows per block");
    constexpr int GC = 32;
    const size_t lds = tile_lds_bytes((size_t)cs.total * (GC + 1));
    rc = tile_fits("multi_cat_sparse_ent", cs, lds);
    if (rc) return rc;
    TM_REQUIRE(packed == nullptr || (n_cats <= 3 && cs.total < PACKED_NONE), "packed codes: at most 3 categoricals, 1022 levels");
    const int nw = waves_knob("catsparse_waves", 16);
    const int n_groups = (int)(mk / 16);
    const int n_pairs = (n_groups + 1) / 2;
    const int64_t n_slabs = ceil_div(n, 64);
    const RangeCut cut = cut_ranges(n_slabs, n_pairs, "catsparse_rounds", 1, 1);
    auto finish = [&](auto kern, size_t lds_k, auto &&launch) {
        return launch_and_finish<F>(kern, cut.nblk, n_pairs, nw * 64, lds_k, cs, GC, mk, out, st, launch);
    };
    // staged form (round 6): d and the code word(s) of a slab's rows parked in per-wave LDS next to the tile
    const int ncw = packed != nullptr ? 1 : n_cats;
    const size_t lds_staged = lds + (size_t)nw * 64 * (sizeof(F) + 4 * (size_t)ncw);
    // ... where a (group, slab) block fills a good part of a 64-lane step: the staged walk takes one step (and one
    // fetch of the rows' operands) per BLOCK, the gather kernel 256 slots per step whatever the blocks hold -- 512
    // columns @ 5 %: 59 slots per block, staged -16 %; 512 @ 4 % (48): -7 %; 512 @ 3 % (38): +10 %; 2048 @ 1.25 % (18):
    // +85 % -- the staged walk costs per block, the gather walk per slot; crossover ~44 (profiles/r6_catsparse.txt).  n_slots = slots of the whole stream (0: unknown -> gather kernel).
    const double fill = (double)n_slots / ((double)std::max(n_groups, 1) * (double)n_slabs);
    if (tune("catsparse_staged", 1) != 0 && lds_staged <= ENT_STAGED_LDS_MAX &&
        fill >= (double)tune("catsparse_staged_fill", 44)) {
        auto staged = [&](auto kern) {
            return finish(kern, lds_staged, [&](dim3 grid, dim3 block, F *ws, int64_t stride) {
                hipLaunchKernelGGL(kern, grid, block, lds_staged, st, cs, d, vals, meta, bstart, n_groups, n, n_slabs,
                                   cut.per, ws, stride, packed, (int)lds);
            });
        };
        if (packed != nullptr)
            return dispatch_nc<3>(n_cats, [&](auto nc) {
                return staged(&multi_cat_sparse_ent_staged_kernel<F, decltype(nc)::value, true>);
            });
        return dispatch_nc<8>(n_cats, [&](auto nc) {
            return staged(&multi_cat_sparse_ent_staged_kernel<F, decltype(nc)::value, false>);
        });
    }
    return dispatch_nc<8>(n_cats, [&](auto nc) {
        auto kern = &multi_cat_sparse_ent_kernel<F, decltype(nc)::value>;
        return finish(kern, lds, [&](dim3 grid, dim3 block, F *ws, int64_t stride) {
            hipLaunchKernelGGL(kern, grid, block, lds, st, cs, d, vals, meta, bstart, n_groups, n, n_slabs, cut.per, ws,
                               stride, packed);
        });
    });
}

// row-list form (see multi_cat_sparse_rows_kernel)
template <typename F, typename IX>
static int run_multi_cat_sparse_rows(const void *const *h_codes, const int64_t *h_ncols,
                                     const int32_t *h_drop, int n_cats, const F *cm_data,
                                     const IX *cm_ind, const int32_t *ranges, const int32_t *rows,
                                     int64_t n_sel, int64_t m, const F *d_sel, F *out, hipStream_t st) {
    CatSet cs;
    bool done;
    int rc = fused_begin(h_codes, h_ncols, h_drop, n_cats, n_sel, m, out, st, &cs, &done);
    if (rc || done) return rc;
    constexpr int GC = 32;
    const size_t lds = tile_lds_bytes((size_t)cs.total * (GC + 1));
    rc = tile_fits("multi_cat_sparse_rows", cs, lds);
    if (rc) return rc;
    const int n_groups = (int)ceil_div(m, GC);
    const RangeCut cut = cut_ranges(n_sel, n_groups, "catsparse_rounds", 2048, 1);
    auto kern = &multi_cat_sparse_rows_kernel<F, IX>;
    auto launch = [&](dim3 grid, dim3 block, F *ws, int64_t stride) {
        hipLaunchKernelGGL(kern, grid, block, lds, st, cs, cm_data, cm_ind, ranges, rows, d_sel, n_sel, cut.per, ws, stride);
    };
    return launch_and_finish<F>(kern, cut.nblk, n_groups, 1024, lds, cs, GC, m, out, st, launch);
}

}  // namespace tmh

using namespace tmh;


extern "C" {

int tm_multi_cat_dense_sandwich_f32(const void *const *h_codes, const int64_t *h_ncols,
                                    const int32_t *h_drop_first, int n_cats, int64_t n,
                                    const float *d, const float *M, int64_t M_ncol, int order_f,
                                    float *out, void *stream) {
    return run_multi_cat_dense<float>(h_codes, h_ncols, h_drop_first, n_cats, n, d, M, M_ncol,
                                      order_f, out, as_stream(stream));
}
int tm_multi_cat_dense_sandwich_f64(const void *const *h_codes, const int64_t *h_ncols,
                                    const int32_t *h_drop_first, int n_cats, int64_t n,
                                    const double *d, const double *M, int64_t M_ncol, int order_f,
                                    double *out, void *stream) {
    return run_multi_cat_dense<double>(h_codes, h_ncols, h_drop_first, n_cats, n, d, M, M_ncol,
                                       order_f, out, as_stream(stream));
}
int tm_multi_cat_dense_sandwich_rows_f32(const void *const *h_codes, const int64_t *h_ncols,
                                         const int32_t *h_drop_first, int n_cats, int64_t n,
                                         const float *d, const float *M, int64_t M_ncol,
                                         const int32_t *rows, int64_t n_rows, float *out,
                                         void *stream) {
    return run_multi_cat_dense<float>(h_codes, h_ncols, h_drop_first, n_cats, n, d, M, M_ncol, 0, out,
                                      as_stream(stream), rows, n_rows);
}
int tm_multi_cat_dense_sandwich_rows_f64(const void *const *h_codes, const int64_t *h_ncols,
                                         const int32_t *h_drop_first, int n_cats, int64_t n,
                                         const double *d, const double *M, int64_t M_ncol,
                                         const int32_t *rows, int64_t n_rows, double *out,
                                         void *stream) {
    return run_multi_cat_dense<double>(h_codes, h_ncols, h_drop_first, n_cats, n, d, M, M_ncol, 0, out,
                                       as_stream(stream), rows, n_rows);
}
int tm_multi_cat_sparse_sandwich_ent_f32(const void *const *h_codes, const int64_t *h_ncols,
                                         const int32_t *h_drop_first, int n_cats, int64_t n, const float *d,
                                         const float *vals, const uint16_t *meta, const uint32_t *bstart,
                                         int64_t n_slots, int64_t mk, float *out, void *stream) {
    return run_multi_cat_sparse_ent<float>(h_codes, h_ncols, h_drop_first, n_cats, n, d, vals, meta, bstart, mk,
                                           out, as_stream(stream), nullptr, n_slots);
}
int tm_multi_cat_sparse_sandwich_ent_f64(const void *const *h_codes, const int64_t *h_ncols,
                                         const int32_t *h_drop_first, int n_cats, int64_t n, const double *d,
                                         const double *vals, const uint16_t *meta, const uint32_t *bstart,
                                         int64_t n_slots, int64_t mk, double *out, void *stream) {
    return run_multi_cat_sparse_ent<double>(h_codes, h_ncols, h_drop_first, n_cats, n, d, vals, meta, bstart, mk,
                                            out, as_stream(stream), nullptr, n_slots);
}
int tm_multi_cat_pack_codes(const void *const *h_codes, const int64_t *h_ncols, const int32_t *h_drop_first, int n_cats,
                            int64_t n, uint32_t *packed, void *stream) {
    CatSet cs;
    int rc = make_catset(h_codes, h_ncols, h_drop_first, n_cats, &cs);
    if (rc) return rc;
    TM_REQUIRE(n_cats <= 3 && cs.total < PACKED_NONE, "packed codes: at most 3 categoricals, 1022 stacked levels");
    if (n == 0) return TM_OK;
    hipLaunchKernelGGL(multi_cat_pack_codes_kernel, dim3((unsigned)std::min<int64_t>(4 * NUM_CU, ceil_div(n, 256))),
                       dim3(256), 0, as_stream(stream), cs, n, packed);
    TM_LAUNCH_CHECK();
    return TM_OK;
}
int tm_multi_cat_sparse_sandwich_entp_f32(const void *const *h_codes, const int64_t *h_ncols,
                                          const int32_t *h_drop_first, int n_cats, int64_t n, const float *d,
                                          const float *vals, const uint16_t *meta, const uint32_t *bstart,
                                          int64_t n_slots, int64_t mk, const uint32_t *packed, float *out, void *stream) {
    return run_multi_cat_sparse_ent<float>(h_codes, h_ncols, h_drop_first, n_cats, n, d, vals, meta, bstart, mk, out,
                                           as_stream(stream), packed, n_slots);
}
int tm_multi_cat_sparse_sandwich_entp_f64(const void *const *h_codes, const int64_t *h_ncols,
                                          const int32_t *h_drop_first, int n_cats, int64_t n, const double *d,
                                          const double *vals, const uint16_t *meta, const uint32_t *bstart,
                                          int64_t n_slots, int64_t mk, const uint32_t *packed, double *out, void *stream) {
    return run_multi_cat_sparse_ent<double>(h_codes, h_ncols, h_drop_first, n_cats, n, d, vals, meta, bstart, mk,
                                            out, as_stream(stream), packed, n_slots);
}
int tm_multi_cat_sparse_sandwich_slab_f32(const void *const *h_codes, const int64_t *h_ncols,
                                          const int32_t *h_drop_first, int n_cats, int64_t n,
                                          const float *d, const float *vals, const uint32_t *koff,
                                          const uint8_t *ecol, const int64_t *gptr, int64_t m,
                                          float *out, void *stream) {
    return run_multi_cat_sparse<float>(h_codes, h_ncols, h_drop_first, n_cats, n, d, vals, koff,
                                       ecol, gptr, m, tm_slab_rows(), tm_slab_group_cols(), out,
                                       as_stream(stream));
}
int tm_multi_cat_sparse_sandwich_slab_f64(const void *const *h_codes, const int64_t *h_ncols,
                                          const int32_t *h_drop_first, int n_cats, int64_t n,
                                          const double *d, const double *vals, const uint32_t *koff,
                                          const uint8_t *ecol, const int64_t *gptr, int64_t m,
                                          double *out, void *stream) {
    return run_multi_cat_sparse<double>(h_codes, h_ncols, h_drop_first, n_cats, n, d, vals, koff,
                                        ecol, gptr, m, tm_slab_rows(), tm_slab_group_cols(), out,
                                        as_stream(stream));
}
int tm_multi_cat_sparse_sandwich_rows_f32(const void *const *h_codes, const int64_t *h_ncols,
                                          const int32_t *h_drop_first, int n_cats,
                                          const float *cm_data, const int32_t *cm_indices,
                                          const int32_t *row_ranges, const int32_t *rows,
                                          int64_t n_sel, int64_t m, const float *d_sel, float *out,
                                          void *stream) {
    return run_multi_cat_sparse_rows<float, int32_t>(h_codes, h_ncols, h_drop_first, n_cats, cm_data,
                                                 cm_indices, row_ranges, rows, n_sel, m, d_sel, out,
                                                 as_stream(stream));
}
int tm_multi_cat_sparse_sandwich_rows_f64(const void *const *h_codes, const int64_t *h_ncols,
                                          const int32_t *h_drop_first, int n_cats,
                                          const double *cm_data, const int32_t *cm_indices,
                                          const int32_t *row_ranges, const int32_t *rows,
                                          int64_t n_sel, int64_t m, const double *d_sel, double *out,
                                          void *stream) {
    return run_multi_cat_sparse_rows<double, int32_t>(h_codes, h_ncols, h_drop_first, n_cats, cm_data,
                                                  cm_indices, row_ranges, rows, n_sel, m, d_sel, out,
                                                  as_stream(stream));
}
int tm_multi_cat_sparse_sandwich_rows_u8_f32(const void *const *h_codes, const int64_t *h_ncols,
                                             const int32_t *h_drop_first, int n_cats,
                                             const float *cm_data, const uint8_t *cm_col8,
                                             const int32_t *row_ranges, const int32_t *rows,
                                             int64_t n_sel, int64_t m, const float *d_sel, float *out,
                                             void *stream) {
    return run_multi_cat_sparse_rows<float, uint8_t>(h_codes, h_ncols, h_drop_first, n_cats, cm_data,
                                                          cm_col8, row_ranges, rows, n_sel, m, d_sel, out,
                                                          as_stream(stream));
}
int tm_multi_cat_sparse_sandwich_rows_u8_f64(const void *const *h_codes, const int64_t *h_ncols,
                                             const int32_t *h_drop_first, int n_cats,
                                             const double *cm_data, const uint8_t *cm_col8,
                                             const int32_t *row_ranges, const int32_t *rows,
                                             int64_t n_sel, int64_t m, const double *d_sel, double *out,
                                             void *stream) {
    return run_multi_cat_sparse_rows<double, uint8_t>(h_codes, h_ncols, h_drop_first, n_cats, cm_data,
                                                           cm_col8, row_ranges, rows, n_sel, m, d_sel, out,
                                                           as_stream(stream));
}
}  // extern "C"
