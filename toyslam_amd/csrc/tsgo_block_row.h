// tsgo_block_row.h — the ONE walk of a block row: out_i = sum over the blocks (i, c) of the row of B_ic x_c, B 3x3 row-major, x three entries.
// What the cycle kernels of tsgo_amg_kernels.h have in common — k_bcsr_residual, k_bcsr_apply, k_restrict, k_prolong_add, k_tail_up and
// both halves of k_coarse_tail — with the small 3x3 helpers and the cycle format the walk reads.  Device only.  Who does NOT use it: the
// file table of tsgo_hip.hip.
//
// A kernel is: where its lane stands (block_row), what it asks for before the walk, ONE call of row_dot, group_sum, its epilogue.
//   - block_row<LPR>(n, xcd8, st, ptr): LPR lanes share row g = (workgroup of lpr_block(xcd8), thread) / LPR, lane `sub` of them; the row
//     is CLAMPED to n - 1, so the surplus workgroups of a grid rounded up for the XCD map walk the last row again and write nothing:
//     `head` (g < n && sub == 0) is the one lane that writes.  ROW64 and LPR == 64: the row is wave-uniform and its bounds come through
//     the scalar cache, one dependent round trip shorter (k_bcsr_residual alone asks for it).
//   - The early exit (row_bounds; block_row calls it): every cycle kernel reads st->done.  The flag is REQUESTED first and TESTED only
//     after the loads that depend on the kernel arguments alone (the row bounds) have been issued and held (issue_before_exit): tested at
//     the very top it put one more scalar round trip (st -> done) in front of the first vector load of kernels whose whole life is four
//     such trips.  The kernel tests `.done` right behind the call and requests what its epilogue needs (r_i, z_i, Dinv_i, omega) BEFORE
//     the walk: it arrives while the blocks are walked instead of adding a dependent trip at the end.
//   - row_dot<STRIDE>(bounds, sub, col, blocks, x, s0, s1, s2): lane `sub` takes the blocks p0 + sub, p0 + sub + STRIDE, ...  Per block the
//     loads are issued in the order column index, block words, gathered entries, and all before the arithmetic.  ONE block per trip: two
//     per trip, every load of the pair issued before either is used, was measured in round 3 — 78 instead of 62 VGPRs, six resident waves
//     per SIMD instead of eight, and the sweeps of levels 1-2 got slower, 7.7 -> 8.4 us and 7.9 -> 8.7 us.  The sums are in the type of s.
//     blocks: CyBlocks<PK> (the cycle format, below) or IdxBlocks<H> (36 contiguous bytes per block, addressed by block index);
//     x: VecAt (x_c = z[c * stride ..], global or LDS; under SUB the difference of two vectors, never materialised).
// The multiply-adds keep the shape s += b0 v0 + b1 v1 + b2 v2 (m3_row): every kernel's sums round as they did when each spelt it out.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "tsgo_kernels.h"

namespace tsgo {

// ---- 3x3 blocks, row-major ---------------------------------------------------------------------------------------------------------
template <typename T, typename A, typename B> __device__ __forceinline__ void m3_mul_acc(const A* a, const B* b, T* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] += T(a[3 * i]) * T(b[j]) + T(a[3 * i + 1]) * T(b[3 + j]) + T(a[3 * i + 2]) * T(b[6 + j]);
}
template <typename T, typename A, typename B> __device__ __forceinline__ void m3_tmul_acc(const A* a, const B* b, T* c) {   // c += a^T b
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] += T(a[i]) * T(b[j]) + T(a[3 + i]) * T(b[3 + j]) + T(a[6 + i]) * T(b[6 + j]);
}
template <typename T> __device__ __forceinline__ void m3_inv(const T* m, T* o) {
    const T c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const T det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (!(fabs(det) > T(0))) { for (int k = 0; k < 9; ++k) o[k] = T(0); return; }
    const T r = T(1) / det;
    o[0] = c00 * r; o[1] = (m[2] * m[7] - m[1] * m[8]) * r; o[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    o[3] = c01 * r; o[4] = (m[0] * m[8] - m[2] * m[6]) * r; o[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    o[6] = c02 * r; o[7] = (m[1] * m[6] - m[0] * m[7]) * r; o[8] = (m[0] * m[4] - m[1] * m[3]) * r;
}
// dst = src (nine values, converted to the destination's type), dst = src^T
template <typename S, typename D> __device__ __forceinline__ void m3_copy(const S* src, D* dst) {
#pragma unroll
    for (int m = 0; m < 9; ++m) dst[m] = src[m];
}
template <typename S, typename D> __device__ __forceinline__ void m3_transpose(const S* src, D* dst) {
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) dst[3 * x + y] = src[3 * y + x];
}
// row i of B v, and s += B v: the one place the block-row sums are spelt out
template <typename B, typename V> __device__ __forceinline__ auto m3_row(const B* b, int i, V v0, V v1, V v2) { return b[3 * i] * v0 + b[3 * i + 1] * v1 + b[3 * i + 2] * v2; }
template <typename B, typename V, typename S> __device__ __forceinline__ void m3_mulv_acc(const B* b, V v0, V v1, V v2, S& s0, S& s1, S& s2) {
    s0 += m3_row(b, 0, v0, v1, v2); s1 += m3_row(b, 1, v0, v1, v2); s2 += m3_row(b, 2, v0, v1, v2);
}

// ---- cycle format ------------------------------------------------------------------------------------------------------------------
// The setup kernels address 3x3 blocks by block index (36 contiguous bytes, "AoS").  Read that way by the cycle kernels —
// a lane per block, nine loads — every load instruction of a wavefront touches 36-byte-strided words: 18+ cache lines
// for 256 useful bytes, and the texture addressers, not the memory system, set the pace (profiles/r01e: L1 tag pipes at
// 40 %).  The cycle therefore reads a COPY in which the blocks of one row are stored plane-major: word m of the j-th
// block of row i lives at W * ptr[i] + m * len_i + j, so that lanes j, j+1, ... load consecutive words.  One or two lines per
// load instruction.  The copy is written once per hierarchy build by the kernels that PRODUCE the blocks (k_prolongator: P and R = P^T;
// k_mirror_pack: the Galerkin matrix of the next level); k_to_planes writes it for the explicit level 0 alone.  Two encodings:
//   PK = 0: W = 9 words, the block's nine f32 values.
//   PK = 1 (tsgo_config.cycle_storage = 16, default): W = 5 words = nine IEEE half floats + a power-of-two exponent (int16) common
//           to the block: value_k = half_k * 2^e, e chosen so that the block's largest entry sits in [2^14, 2^15) — eleven
//           significant bits relative to the block's own maximum whatever its magnitude (gauge blocks of 1e6 next to 1e-3).
//           20 bytes per block instead of 36 and five loads instead of nine: the sweeps of the big levels are byte-bound at
//           1 M poses and half byte-, half latency-bound at 100 k.  A block and its mirror (A_ij, A_ji^T) have the same maximum,
//           hence the same exponent and element-wise the same rounding: the rounded matrix is still symmetric, and because
//           every use inside the cycle (pre-sweeps, residual, post-sweeps; restriction and prolongation through R = P^T copies of
//           the same rounded blocks) reads THIS copy, the V-cycle stays a symmetric operator.  The setup (Galerkin products,
//           diagonal inverses) keeps the f32 blocks.
constexpr int kCyWordsF32 = 9, kCyWordsF16 = 5;
template <int PK> __host__ __device__ constexpr int cy_words() { return PK ? kCyWordsF16 : kCyWordsF32; }
// the nine values of one block into its cycle-format words (the j-th block of a row of `len` blocks whose words start at `o` = base + j)
template <int PK> __device__ __forceinline__ void cy_store(const float* v, uint32_t* __restrict__ o, size_t len) {
    if (PK) {
        float mx = 0;
#pragma unroll
        for (int m = 0; m < 9; ++m) mx = fmaxf(mx, fabsf(v[m]));
        int e = 0;
        if (mx > 0.f && mx < 3.0e38f) {
            e = ilogbf(mx) - 14;                                  // largest entry -> [2^14, 2^15)
            e = e < -126 ? -126 : (e > 112 ? 112 : e);            // 2^e and 2^-e stay normal floats
        }
        const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
        unsigned short h[9];
#pragma unroll
        for (int m = 0; m < 9; ++m) h[m] = __half_as_ushort(__float2half_rn(v[m] * inv));
#pragma unroll
        for (int m = 0; m < 4; ++m) o[(size_t)m * len] = (uint32_t)h[2 * m] | ((uint32_t)h[2 * m + 1] << 16);
        o[(size_t)4 * len] = (uint32_t)h[8] | ((uint32_t)(unsigned short)(short)e << 16);
    } else {
#pragma unroll
        for (int m = 0; m < 9; ++m) o[(size_t)m * len] = __float_as_uint(v[m]);
    }
}
// the j-th block of a row whose cycle-format words start at `base` (row length len): its words as stored (cy_fetch: loads only, so
// that several blocks' words can be requested before any is used), and the words as nine values of type T (cy_decode)
template <int PK> __device__ __forceinline__ void cy_fetch(const uint32_t* __restrict__ base, size_t len, size_t j, uint32_t* w) {
    const uint32_t* q = base + j;
#pragma unroll
    for (int m = 0; m < cy_words<PK>(); ++m) w[m] = q[(size_t)m * len];
}
template <typename T, int PK> __device__ __forceinline__ void cy_decode(const uint32_t* w, T* b) {
    if (PK) {
        const int e = (int)(short)(w[4] >> 16);
        const float sc = __uint_as_float((uint32_t)(e + 127) << 23);          // 2^e, e in [-126, 127] by construction
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            b[2 * m] = T(__half2float(__ushort_as_half((unsigned short)(w[m] & 0xffffu))) * sc);
            b[2 * m + 1] = T(__half2float(__ushort_as_half((unsigned short)(w[m] >> 16))) * sc);
        }
        b[8] = T(__half2float(__ushort_as_half((unsigned short)(w[4] & 0xffffu))) * sc);
    } else {
#pragma unroll
        for (int m = 0; m < 9; ++m) b[m] = T(__uint_as_float(w[m]));
    }
}
template <typename T, int PK> __device__ __forceinline__ void cy_load(const uint32_t* __restrict__ base, size_t len, size_t j, T* b) {
    uint32_t w[cy_words<PK>()];
    cy_fetch<PK>(base, len, j, w);
    cy_decode<T, PK>(w, b);
}

// ---- where a lane stands, and the early exit -----------------------------------------------------------------------------------------
// The coarse levels hold little work (12.5k / 1.5k / 196 block rows at 100k poses): what matters is the length of the dependent-load
// chain, so LPR lanes share one block row (one 3x3 block per lane per trip) and finish with an LPR-lane xor-shuffle sum (group_sum).
// The block-row kernels' arguments begin with a plain head (tsgo_kernels.h, "Argument heads"): n, xcd8, st, the row pointer, the column
// and matrix words and the gathered vector — what is needed until the first dependent vector load is out — and the epilogue's operands behind.
// Block-row kernels of the big levels take the XCD-aware workgroup map of the table kernels (xcd_block(), tsgo_kernels.h): an XCD walks a
// contiguous eighth of the rows, so the vector entries a row gathers (its neighbours': nearby rows) are fetched into ONE L2 instead of all
// eight (PMC, round 3: k_restrict from level 0 fetched 1.74x its algorithmic bytes, k_prolong_add 1.48x).  xcd8 = 0: round-robin, as before.
__device__ __forceinline__ int lpr_block(int xcd8) { return xcd8 ? xcd_block(xcd8) : (int)blockIdx.x; }      // xcd8: 0, or gridDim.x / 8

struct RowBounds { int p0, p1, done; };
struct BlockRow : RowBounds { int row, sub; bool head; };
// FLAG = false: a kernel outside a solve (the power iteration) neither reads nor tests the flag
template <bool FLAG = true, typename T> __device__ __forceinline__ RowBounds row_bounds(const CgState<T>* __restrict__ st, const int* __restrict__ ptr, int row) {
    const int done = FLAG ? st->done : 0;
    int p0 = ptr[row];
    const int p1 = ptr[row + 1];
    issue_before_exit(p0);
    return {p0, p1, done};
}
template <int LPR, bool FLAG = true, bool ROW64 = false, typename T>
__device__ __forceinline__ BlockRow block_row(int n, int xcd8, const CgState<T>* __restrict__ st, const int* __restrict__ ptr) {
    const int g = (lpr_block(xcd8) * kBlock + threadIdx.x) / LPR, sub = threadIdx.x % LPR;
    const int row = ROW64 && LPR == 64 ? __builtin_amdgcn_readfirstlane(g < n ? g : n - 1) : (g < n ? g : n - 1);
    return {row_bounds<FLAG>(st, ptr, row), row, sub, g < n && sub == 0};
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------------
template <int PK> struct CyBlocks {      // the row's blocks in the cycle format: words = the matrix's copy, the row's start at W * p0
    const uint32_t* base; size_t len; int p0;
    __device__ __forceinline__ CyBlocks(const void* words, const RowBounds& r) : base((const uint32_t*)words + (size_t)r.p0 * cy_words<PK>()), len((size_t)(r.p1 - r.p0)), p0(r.p0) {}
    template <typename A> __device__ __forceinline__ void load(int a, A* b) const { cy_load<A, PK>(base, len, (size_t)(a - p0), b); }
};
template <typename H> struct IdxBlocks {      // block a of the block-indexed array
    const H* blk;
    __device__ __forceinline__ IdxBlocks(const void* blocks, const RowBounds&) : blk((const H*)blocks) {}
    template <typename A> __device__ __forceinline__ void load(int a, A* b) const { m3_copy(blk + (size_t)a * 9, b); }
};
template <typename V, bool SUB = false> struct VecAt {      // x_c = z[c * zs ..], global or LDS; SUB: less m[c * zs ..]
    const V* z; int zs; const V* m;
    template <typename A> __device__ __forceinline__ void get(int c, A& x0, A& x1, A& x2) const {
        const size_t i = (size_t)c * zs;
        x0 = z[i]; x1 = z[i + 1]; x2 = z[i + 2];
        if (SUB) { x0 -= m[i]; x1 -= m[i + 1]; x2 -= m[i + 2]; }
    }
};
template <int STRIDE, typename Blocks, typename X, typename A>
__device__ __forceinline__ void row_dot(const RowBounds& r, int sub, const int* __restrict__ col, const Blocks& blocks, const X& x, A& s0, A& s1, A& s2) {
    for (int a = r.p0 + sub; a < r.p1; a += STRIDE) {
        const int c = col[a];
        A b[9], x0, x1, x2;
        blocks.load(a, b);
        x.get(c, x0, x1, x2);
        m3_mulv_acc(b, x0, x1, x2, s0, s1, s2);
    }
}

}  // namespace tsgo
