// tsgo_marginal_kernels.h — the batched solve behind tsgo_marginals: NV right-hand sides of the reduced pose system S X = B at once.
//
// Batch vectors are [rows][NV][3] (landmark vectors [L][NV][2]): the NV columns of one row are contiguous.  The two Schur passes keep
// the SELL shape of tsgo_kernels.h (one wavefront per slice, G lanes per vertex) and carry all NV columns in registers, so every slot
// plane, index and gathered pose state is read ONCE per batch product.  Block-row kernels (the hierarchy's levels, the vector steps)
// take one thread per (row, column): the NV threads of a row read the same 3x3 block (one broadcast) and contiguous vector entries.
// Every reduction is a per-workgroup partial followed by one fixed-order fold (k_mb_fold): no atomics, the same call gives the same
// bits.  Only T = double is instantiated (tsgo_marginals refuses f32 handles).
#pragma once
#include <hip/hip_runtime.h>

#include "host/batch_plan.h"
#include "tsgo_amg_kernels.h"
#include "tsgo_kernels.h"

namespace tsgo {

constexpr int kMbMaxWidth = 16;      // the widest batch instantiated (tsgo_hip.hip: marginal_width)

// Per-column CG state, and the batch's "all columns finished" word every iteration kernel looks at first.
template <typename T> struct MbCol { T gamma, bdb; int iters, done, fail, pad; };
template <typename T> struct MbState { int all_done, pad[3]; MbCol<T> col[kMbMaxWidth]; };

// t = W_il^T v for one landmark slot (2 x 3 map of the (a0, a1, ppx, ppy) algebra): what k_schur_lm sums
template <typename T> __device__ __forceinline__ void wt_apply(T a0, T a1, T ppx, T ppy, T c, T s, T v0, T v1, T v2, T& o0, T& o1) {
    const T vt0 = c * v0 + s * v1, vt1 = c * v1 - s * v0;
    const T m0 = a0 * (ppy * v2 - vt0), m1 = a1 * (-vt1 - ppx * v2);
    o0 = c * m0 - s * m1; o1 = s * m0 + c * m1;
}

// Per-column sums over a workgroup: v[c] of every thread -> out[c] (fixed order: wave sums, then the waves in order).
template <typename T, int NV> __device__ __forceinline__ void block_cols(const T* v, T* red, T* out) {
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const T s = wave_sum(v[c]);
        if ((threadIdx.x & 63) == 0) red[w * NV + c] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        T s = 0;
        for (int k = 0; k < kWavesPerBlock; ++k) s += red[k * NV + threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// ---- the two Schur passes, NV columns ------------------------------------------------------------------------------------------
// t[l][c] = Dl^-1 W_l^T v[.][c]
template <typename T, int G, int NV>
__global__ __launch_bounds__(kBlock) void k_mb_schur_lm(Table<T> tb, const T* __restrict__ v, const T* __restrict__ ps, const T* __restrict__ ninv,
                                                        T* __restrict__ t, const int* __restrict__ stop) {
    if (*stop) return;
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    if (!wk.live) return;
    const int slice = wk.slice, lane = wk.lane, l = wk.vertex;
    T acc[NV][2];
#pragma unroll
    for (int c = 0; c < NV; ++c) { acc[c][0] = 0; acc[c][1] = 0; }
    for (uint32_t row = tb.row_off[slice]; row < tb.row_off[slice + 1]; ++row) {
        const size_t k = (size_t)row * 64 + lane;
        const uint32_t i = tb.idx[k];
        const LmSlot<T> d = lm_slot<T>(tb, k);
        const auto cs = ld2<T>(ps + (size_t)i * 4 + 2);
        const T* vi = v + (size_t)i * NV * 3;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            T o0, o1;
            wt_apply<T>(d.a0, d.a1, d.ppx, d.ppy, cs.x, cs.y, vi[3 * c], vi[3 * c + 1], vi[3 * c + 2], o0, o1);
            acc[c][0] += o0; acc[c][1] += o1;
        }
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) { acc[c][0] = group_sum<T, G>(acc[c][0]); acc[c][1] = group_sum<T, G>(acc[c][1]); }
    if (l < tb.n_vertices && wk.head) {
        const T ixx = ninv[(size_t)l * kNinvRec], ixy = ninv[(size_t)l * kNinvRec + 1], iyy = ninv[(size_t)l * kNinvRec + 2];
        T* tl = t + (size_t)l * NV * 2;
#pragma unroll
        for (int c = 0; c < NV; ++c) { tl[2 * c] = ixx * acc[c][0] + ixy * acc[c][1]; tl[2 * c + 1] = ixy * acc[c][0] + iyy * acc[c][1]; }
    }
}

// out = S v (MODE 0, with per-workgroup partials of v^T S v per column in dot_part[block][NV]), or out = rvec - S v (MODE 1).
// S v = Hpp v - W t: the pose's own block (dp), its landmark slots (t from k_mb_schur_lm) and its pose-pose slots (three planes, or the
// general eight-plane form OJ = 1: analytic odometry Jacobians, virtual landmarks).
template <typename T, int G, int OJ, int NV, int MODE>
__global__ __launch_bounds__(kBlock) void k_mb_schur_pose(Table<T> tb, Table<T> od, const T* __restrict__ v, const T* __restrict__ t,
                                                          const T* __restrict__ ps, const T* __restrict__ dp, T* __restrict__ out,
                                                          const T* __restrict__ rvec, T* __restrict__ dot_part, const int* __restrict__ stop) {
    __shared__ T red[kWavesPerBlock * NV];
    if (*stop) return;      // workgroup-uniform
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const int slice = wk.slice, lane = wk.lane, i = wk.vertex;
    T o[NV][3];
#pragma unroll
    for (int c = 0; c < NV; ++c) { o[c][0] = 0; o[c][1] = 0; o[c][2] = 0; }
    T dot[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) dot[c] = 0;
    if (wk.live) {
        const bool valid = i < tb.n_vertices;
        const int ic = valid ? i : tb.n_vertices - 1;
        const auto cs = ld2<T>(ps + (size_t)ic * 4 + 2);
        const T c0 = cs.x, s0 = cs.y;
        {
            for (uint32_t row = tb.row_off[slice]; row < tb.row_off[slice + 1]; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t l = tb.idx[k];
                const LmSlot<T> d = lm_slot<T>(tb, k);
                const T* tl = t + (size_t)l * NV * 2;
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    const T tx = tl[2 * c], ty = tl[2 * c + 1];
                    const T t0 = d.a0 * (c0 * tx + s0 * ty), t1 = d.a1 * (c0 * ty - s0 * tx);
                    o[c][0] += c0 * t0 - s0 * t1; o[c][1] += s0 * t0 + c0 * t1; o[c][2] -= t0 * d.ppy - t1 * d.ppx;
                }
            }
        }
        {
            const size_t S = od.slots;
            for (uint32_t row = od.row_off[slice]; row < od.row_off[slice + 1]; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t j = od.idx[k] & kPoseIdxMask;
                const T* vj = v + (size_t)j * NV * 3;
                if (OJ) {
                    const PairSlot<T> h = pair_slot<T>(od.dyn, S, k);
#pragma unroll
                    for (int c = 0; c < NV; ++c) pair_apply<T>(h.v, vj[3 * c], vj[3 * c + 1], vj[3 * c + 2], o[c][0], o[c][1], o[c][2]);
                } else {
                    const T h0 = od.dyn[k], h1 = od.dyn[S + k], h2 = od.dyn[2 * S + k];
#pragma unroll
                    for (int c = 0; c < NV; ++c) { o[c][0] -= h0 * vj[3 * c]; o[c][1] -= h1 * vj[3 * c + 1]; o[c][2] -= h2 * vj[3 * c + 2]; }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NV; ++c) { o[c][0] = group_sum<T, G>(o[c][0]); o[c][1] = group_sum<T, G>(o[c][1]); o[c][2] = group_sum<T, G>(o[c][2]); }
        if (valid && wk.head) {
            T d[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) d[m] = dp[(size_t)i * 6 + m];
            const T* vi = v + (size_t)i * NV * 3;
            T* oi = out + (size_t)i * NV * 3;
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                T d0, d1, d2;
                const T v0 = vi[3 * c], v1 = vi[3 * c + 1], v2 = vi[3 * c + 2];
                sym3_mul<T>(d, v0, v1, v2, d0, d1, d2);
                const T s0v = o[c][0] + d0, s1v = o[c][1] + d1, s2v = o[c][2] + d2;
                if (MODE == 1) {
                    const T* ri = rvec + (size_t)i * NV * 3;
                    oi[3 * c] = ri[3 * c] - s0v; oi[3 * c + 1] = ri[3 * c + 1] - s1v; oi[3 * c + 2] = ri[3 * c + 2] - s2v;
                } else {
                    oi[3 * c] = s0v; oi[3 * c + 1] = s1v; oi[3 * c + 2] = s2v;
                    dot[c] = s0v * v0 + s1v * v1 + s2v * v2;
                }
            }
        }
    }
    if (MODE == 0) block_cols<T, NV>(dot, red, dot_part + (size_t)blockIdx.x * NV);
}

// ---- reductions and the vector steps of PCG (one thread per (row, column)) ------------------------------------------------------
// out[w] = sum over k of part[k][w], w < W, in a fixed order (one workgroup; W divides kBlock)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mb_fold(int n_part, int W, const T* __restrict__ part, T* __restrict__ out, const int* __restrict__ stop) {
    __shared__ T red[kBlock];
    if (*stop) return;
    const int c = threadIdx.x % W, g = threadIdx.x / W, ng = kBlock / W;
    T s = 0;
    for (int k = g; k < n_part; k += ng) s += part[(size_t)k * W + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < W) {
        T a = 0;
        for (int q = 0; q < ng; ++q) a += red[q * W + threadIdx.x];
        out[threadIdx.x] = a;
    }
}

// Per-workgroup partials of (r, z) and (r, Minv r) for every column: part[block][2 NV] = (gamma[NV] | rdr[NV]).  Z_BJ: write z = Minv r
// first (the block-Jacobi preconditioner).
template <typename T, int NV, int Z_BJ>
__global__ __launch_bounds__(kBlock) void k_mb_dots(int P, const T* __restrict__ r, T* __restrict__ z, const T* __restrict__ minv,
                                                    T* __restrict__ part, const int* __restrict__ stop) {
    __shared__ T red[2 * kBlock];
    if (*stop) return;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    T g = 0, d = 0;
    if (e < P * NV) {
        const int i = e / NV;
        const T r0 = r[(size_t)e * 3], r1 = r[(size_t)e * 3 + 1], r2 = r[(size_t)e * 3 + 2];
        T m0, m1, m2;
        sym3_mul<T>(minv + (size_t)i * 6, r0, r1, r2, m0, m1, m2);
        d = r0 * m0 + r1 * m1 + r2 * m2;
        if (Z_BJ) { z[(size_t)e * 3] = m0; z[(size_t)e * 3 + 1] = m1; z[(size_t)e * 3 + 2] = m2; g = d; }
        else g = r0 * z[(size_t)e * 3] + r1 * z[(size_t)e * 3 + 1] + r2 * z[(size_t)e * 3 + 2];
    }
    red[threadIdx.x] = g; red[kBlock + threadIdx.x] = d;
    __syncthreads();
    if (threadIdx.x < 2 * NV) {      // kBlock is a multiple of NV: the column of thread k is k % NV in every workgroup
        const int c = threadIdx.x % NV, h = threadIdx.x / NV;
        T a = 0;
        for (int k = c; k < kBlock; k += NV) a += red[h * kBlock + k];
        part[(size_t)blockIdx.x * 2 * NV + threadIdx.x] = a;
    }
}

// First step of a batch: gamma = (r, z), bdb = (b, Minv b) from the folded dots; p = z.  A zero column (padding of a part-filled batch) is
// done at once with x = 0; a negative (r, z) is a breakdown of the preconditioner.
template <typename T, int NV>
__global__ __launch_bounds__(kBlock) void k_mb_start(int P, const T* __restrict__ fg, const T* __restrict__ z, T* __restrict__ p, MbState<T>* __restrict__ st) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < P * NV) { p[(size_t)e * 3] = z[(size_t)e * 3]; p[(size_t)e * 3 + 1] = z[(size_t)e * 3 + 1]; p[(size_t)e * 3 + 2] = z[(size_t)e * 3 + 2]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int all = 1;
        for (int c = 0; c < kMbMaxWidth; ++c) {
            MbCol<T> s{}; s.iters = 0; s.done = 1; s.fail = 0;
            if (c < NV) {
                s.gamma = fg[c]; s.bdb = fg[NV + c];
                s.done = !(s.bdb > T(0)) ? 1 : 0;
                if (!s.done && !(s.gamma > T(0))) { s.done = 1; s.fail = 1; }
            }
            st->col[c] = s;
            all &= s.done;
        }
        st->all_done = all;
    }
}

// x += alpha p, r -= alpha q for the columns still running (alpha = gamma / (p, S p) from the folded dots)
template <typename T, int NV>
__global__ __launch_bounds__(kBlock) void k_mb_alpha(int P, const T* __restrict__ fd, const MbState<T>* __restrict__ st, const T* __restrict__ p,
                                                     const T* __restrict__ q, T* __restrict__ x, T* __restrict__ r) {
    if (st->all_done) return;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= P * NV) return;
    const int c = e % NV;
    const MbCol<T> s = st->col[c];
    if (s.done) return;
    const T delta = fd[c];
    if (!(delta > T(0))) return;      // breakdown: k_mb_beta reports it, x and r stay as they are
    const T a = s.gamma / delta;
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[(size_t)e * 3 + k] += a * p[(size_t)e * 3 + k]; r[(size_t)e * 3 + k] -= a * q[(size_t)e * 3 + k]; }
}

// The verdict of every column (the stopping rule of tsgo_config.pcg_rel_tol: r^T D^-1 r <= tol^2 b^T D^-1 b) and p = z + beta p for
// the columns that go on.  Reads state slot st_in, workgroup 0 writes st_out (a ring of two, as the single-vector solve's).
template <typename T, int NV>
__global__ __launch_bounds__(kBlock) void k_mb_beta(int P, const T* __restrict__ fd, const T* __restrict__ fg, const MbState<T>* __restrict__ st_in,
                                                    MbState<T>* __restrict__ st_out, const T* __restrict__ z, T* __restrict__ p, T tol2, int max_iters) {
    if (st_in->all_done) {      // a finished batch: the state is carried over whole, so that either slot holds the final verdicts
        if (blockIdx.x == 0 && threadIdx.x < kMbMaxWidth) st_out->col[threadIdx.x] = st_in->col[threadIdx.x];
        if (blockIdx.x == 0 && threadIdx.x == 0) st_out->all_done = 1;
        return;
    }
    auto verdict = [&](int c, MbCol<T>& s, T& beta) {
        s = st_in->col[c]; beta = 0;
        if (s.done) return;
        const T delta = fd[c], gnew = fg[c], rdr = fg[NV + c];
        s.iters += 1;
        if (!(delta > T(0)) || !(gnew >= T(0)) || rdr != rdr) { s.done = 1; s.fail = 1; return; }      // (p, S p) <= 0 or (r, M^-1 r) < 0: breakdown
        if (!(rdr > tol2 * s.bdb)) { s.done = 1; s.gamma = gnew; return; }
        if (s.iters >= max_iters) { s.done = 1; s.fail = 2; s.gamma = gnew; return; }
        beta = gnew / s.gamma; s.gamma = gnew;
    };
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < P * NV) {
        const int c = e % NV;
        MbCol<T> s; T beta;
        verdict(c, s, beta);
        if (!s.done) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[(size_t)e * 3 + k] = z[(size_t)e * 3 + k] + beta * p[(size_t)e * 3 + k];
        }
    }
    if (blockIdx.x == 0) {
        __shared__ int dn[kMbMaxWidth];
        if (threadIdx.x < kMbMaxWidth) {
            MbCol<T> s; T beta;
            if (threadIdx.x < NV) verdict(threadIdx.x, s, beta); else s = st_in->col[threadIdx.x];
            st_out->col[threadIdx.x] = s;
            dn[threadIdx.x] = s.done;
        }
        __syncthreads();
        if (threadIdx.x == 0) { int all = 1; for (int c = 0; c < kMbMaxWidth; ++c) all &= dn[c]; st_out->all_done = all; }
    }
}

// ---- the V-cycle, NV columns (T vectors on every level) ----------------------------------------------------------------------
// level 0 smoothing with the Schur diagonal's inverse blocks: MODE 0 z = w Minv r, MODE 1 z += w Minv (r - s)
template <typename T, int NV, int MODE>
__global__ __launch_bounds__(kBlock) void k_mb_smooth0(int P, const T* __restrict__ minv, const T* __restrict__ omega, const T* __restrict__ r,
                                                       const T* __restrict__ s, T* __restrict__ z, const int* __restrict__ stop) {
    if (*stop) return;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= P * NV) return;
    const int i = e / NV;
    T e0 = r[(size_t)e * 3], e1 = r[(size_t)e * 3 + 1], e2 = r[(size_t)e * 3 + 2];
    if (MODE == 1) { e0 -= s[(size_t)e * 3]; e1 -= s[(size_t)e * 3 + 1]; e2 -= s[(size_t)e * 3 + 2]; }
    T z0, z1, z2;
    sym3_mul<T>(minv + (size_t)i * 6, e0, e1, e2, z0, z1, z2);
    const T w = *omega;
    if (MODE == 0) { z[(size_t)e * 3] = w * z0; z[(size_t)e * 3 + 1] = w * z1; z[(size_t)e * 3 + 2] = w * z2; }
    else { z[(size_t)e * 3] += w * z0; z[(size_t)e * 3 + 1] += w * z1; z[(size_t)e * 3 + 2] += w * z2; }
}

// Block-row products over a block-indexed matrix of the hierarchy (3x3 blocks, row-major, HT<T>):
//   MODE 0: out = b - M x          (residual)
//   MODE 1: out = x + w Dinv (b - M x), x == nullptr: out = w Dinv b     (a block-Jacobi sweep)
//   MODE 2: out = M x              (restriction, M = R)
//   MODE 3: out += M x             (prolongation, M = P; out's rows are not x's)
template <typename T, int NV, int MODE>
__global__ __launch_bounds__(kBlock) void k_mb_bsr(int n, const int* __restrict__ ptr, const int* __restrict__ col, const HT<T>* __restrict__ M,
                                                   const T* __restrict__ x, const T* __restrict__ b, const HT<T>* __restrict__ dinv,
                                                   const T* __restrict__ omega, T* __restrict__ out, const int* __restrict__ stop) {
    if (*stop) return;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n * NV) return;
    const int i = e / NV, c = e % NV;
    T a0 = 0, a1 = 0, a2 = 0;
    if (x) {
        for (int q = ptr[i]; q < ptr[i + 1]; ++q) {
            const HT<T>* m = M + (size_t)q * 9;
            const T* xj = x + ((size_t)col[q] * NV + c) * 3;
            const T x0 = xj[0], x1 = xj[1], x2 = xj[2];
            a0 += (T)m[0] * x0 + (T)m[1] * x1 + (T)m[2] * x2;
            a1 += (T)m[3] * x0 + (T)m[4] * x1 + (T)m[5] * x2;
            a2 += (T)m[6] * x0 + (T)m[7] * x1 + (T)m[8] * x2;
        }
    }
    T* o = out + (size_t)e * 3;
    if (MODE == 2) { o[0] = a0; o[1] = a1; o[2] = a2; return; }
    if (MODE == 3) { o[0] += a0; o[1] += a1; o[2] += a2; return; }
    const T r0 = b[(size_t)e * 3] - a0, r1 = b[(size_t)e * 3 + 1] - a1, r2 = b[(size_t)e * 3 + 2] - a2;
    if (MODE == 0) { o[0] = r0; o[1] = r1; o[2] = r2; return; }
    const HT<T>* d = dinv + (size_t)i * 9;
    const T w = *omega;
    const T d0 = (T)d[0] * r0 + (T)d[1] * r1 + (T)d[2] * r2, d1 = (T)d[3] * r0 + (T)d[4] * r1 + (T)d[5] * r2, d2 = (T)d[6] * r0 + (T)d[7] * r1 + (T)d[8] * r2;
    if (x) { const T* xi = x + (size_t)e * 3; o[0] = xi[0] + w * d0; o[1] = xi[1] + w * d1; o[2] = xi[2] + w * d2; }
    else { o[0] = w * d0; o[1] = w * d1; o[2] = w * d2; }
}

// the coarsest level: z = inv b, inv dense (n3 x n3, row-major), one thread per (block row, column)
template <typename T, int NV>
__global__ __launch_bounds__(kBlock) void k_mb_dense(int nb, const T* __restrict__ inv, const T* __restrict__ b, T* __restrict__ z, const int* __restrict__ stop) {
    if (*stop) return;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= nb * NV) return;
    const int i = e / NV, c = e % NV, n3 = nb * 3;
    T a[3] = {0, 0, 0};
    for (int j = 0; j < nb; ++j) {
        const T* bj = b + ((size_t)j * NV + c) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T* row = inv + (size_t)(3 * i + k) * n3 + 3 * j;
            a[k] += row[0] * bj[0] + row[1] * bj[1] + row[2] * bj[2];
        }
    }
    T* o = z + (size_t)e * 3;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
}

// ---- right-hand sides and read-out -------------------------------------------------------------------------------------------
// (one query column, MbColumn: host/batch_plan.h)

// One slot k of a landmark in the landmark-major table: its pose and Y_il = W_il Dl^-1 (3 x 2).  Padding slots have zero weights and
// give Y = 0.
template <typename T>
__device__ __forceinline__ void lm_y_block(const Table<T>& tb, const T* __restrict__ ps, size_t k, const T* dinv3, uint32_t& pose, T y[3][2]) {
    pose = tb.idx[k];
    const LmSlot<T> d = lm_slot<T>(tb, k);
    const auto cs = ld2<T>(ps + (size_t)pose * 4 + 2);
    const T ixx = dinv3[0], ixy = dinv3[1], iyy = dinv3[2];
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {       // column kk of W_il^T (2 x 3) = W_il^T e_kk; Y_il row kk = (Dl^-1 W_il^T e_kk)^T
        T m0, m1;
        wt_apply<T>(d.a0, d.a1, d.ppx, d.ppy, cs.x, cs.y, T(kk == 0), T(kk == 1), T(kk == 2), m0, m1);
        y[kk][0] = ixx * m0 + ixy * m1; y[kk][1] = ixy * m0 + iyy * m1;
    }
}

// b[.][c] for every column c of the batch (b zeroed before).  A landmark column accumulates over its slots (a pose may observe it twice).
template <typename T, int NV>
__global__ __launch_bounds__(64) void k_mb_rhs(Table<T> tb, int G, const T* __restrict__ ps, const T* __restrict__ lmrec, const MbColumn* __restrict__ cols,
                                               T* __restrict__ b) {
    const int c = threadIdx.x;
    if (c >= NV) return;
    const MbColumn q = cols[c];
    if (q.kind == 0) { b[((size_t)q.idx * NV + c) * 3 + q.comp] = T(1); return; }
    if (q.kind != 1) return;
    const int l = q.idx, vps = 64 / G, slice = l / vps;
    const T* dv = lmrec + (size_t)l * kLmRec + 2;
    for (uint32_t row = tb.row_off[slice]; row < tb.row_off[slice + 1]; ++row)
        for (int g = 0; g < G; ++g) {
            const size_t k = (size_t)row * 64 + (size_t)((l % vps) * G + g);
            uint32_t i; T y[3][2];
            lm_y_block<T>(tb, ps, k, dv, i, y);
            T* bi = b + ((size_t)i * NV + c) * 3;
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) bi[kk] += y[kk][q.comp];
        }
}

// The 3 x 3 (pose) or 2 x 2 (landmark: Dl^-1 + Y_l^T X over the observing poses only) marginal of every query of the batch.
// items[q] = (kind, idx, first column); out[q] = 9 doubles, row-major, unsymmetrised (the host symmetrises).
template <typename T, int NV>
__global__ __launch_bounds__(64) void k_mb_extract(Table<T> tb, int G, int n_items, const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                   const MbColumn* __restrict__ items, const T* __restrict__ x, double* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= n_items) return;
    const MbColumn it = items[q];
    double* o = out + (size_t)q * 9;
    for (int k = 0; k < 9; ++k) o[k] = 0;
    if (it.kind == 0) {
        const T* xi = x + (size_t)it.idx * NV * 3;
        for (int a = 0; a < 3; ++a)
            for (int bb = 0; bb < 3; ++bb) o[3 * a + bb] = (double)xi[(it.comp + bb) * 3 + a];
        return;
    }
    const int l = it.idx, vps = 64 / G, slice = l / vps;
    const T* dv = lmrec + (size_t)l * kLmRec + 2;
    T s00 = 0, s01 = 0, s10 = 0, s11 = 0;
    for (uint32_t row = tb.row_off[slice]; row < tb.row_off[slice + 1]; ++row)
        for (int g = 0; g < G; ++g) {
            const size_t k = (size_t)row * 64 + (size_t)((l % vps) * G + g);
            uint32_t i; T y[3][2];
            lm_y_block<T>(tb, ps, k, dv, i, y);
            const T* x0 = x + ((size_t)i * NV + it.comp) * 3;
            const T* x1 = x0 + 3;
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) { s00 += y[kk][0] * x0[kk]; s01 += y[kk][0] * x1[kk]; s10 += y[kk][1] * x0[kk]; s11 += y[kk][1] * x1[kk]; }
        }
    o[0] = (double)(dv[0] + s00); o[1] = (double)(dv[1] + s01); o[3] = (double)(dv[1] + s10); o[4] = (double)(dv[2] + s11);
}

// Sign of a pose-landmark cross block (tsgo_joint_marginals).  H^-1 = [[S^-1, -S^-1 Y], [-Y^T S^-1, D^-1 + Y^T S^-1 Y]] with
// Y = W D^-1; lm_y_block builds Y_l = W_{:,l} Dl^-1 with the W of H itself, so a pose row against a landmark column, and a landmark
// row against a pose column, take -1 (checked against the dense inverse of the oracle's H: tests/test_gpu_joint_marginals.py).
constexpr int kMbCrossSign = -1;

// The joint marginal's rows against the NV columns of one batch: out[r][c] = Sigma[r][column c of the batch] (f64, unsymmetrised) for
// every row r of the query list.  items[q] = (kind, idx, first row of query q).  One wavefront per query:
//   pose i:      rows = X[i][c] (a gather; lane = (row, column));
//   landmark l:  rows = Y_l^T X[.][c] over the landmark's slots in the landmark-major table, plus Dl^-1 on the columns of l itself.
//                Lane = (part, row, column): part p takes every (64 / 2 NV)-th slot row from the p-th, and the parts are folded in
//                order through LDS.
// No atomics: a repeated call gives the same bits.  Padding columns (kind -1) give 0.
template <typename T, int NV>
__global__ __launch_bounds__(64) void k_mb_joint(Table<T> tb, int G, const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                 const MbColumn* __restrict__ items, const MbColumn* __restrict__ cols, const T* __restrict__ x,
                                                 double* __restrict__ out) {
    constexpr int kPairs = 2 * NV, kParts = 64 / kPairs;      // NV in {1, 8, 16}: kPairs divides 64
    __shared__ T red[64];
    const MbColumn it = items[blockIdx.x];
    const int lane = threadIdx.x;
    double* o = out + (size_t)it.comp * NV;
    if (it.kind == 0) {      // workgroup-uniform
        if (lane < 3 * NV) {
            const int a = lane / NV, c = lane % NV;
            const int kind = cols[c].kind;
            const T v = x[((size_t)it.idx * NV + c) * 3 + a];
            o[(size_t)a * NV + c] = kind < 0 ? 0.0 : (double)(kind == 1 ? T(kMbCrossSign) * v : v);
        }
        return;
    }
    const int pair = lane % kPairs, part = lane / kPairs, a = pair / NV, c = pair % NV;
    const int l = it.idx, vps = 64 / G, slice = l / vps;
    const T* dv = lmrec + (size_t)l * kLmRec + 2;
    T s = 0;
    for (uint32_t row = tb.row_off[slice] + part; row < tb.row_off[slice + 1]; row += kParts)
        for (int g = 0; g < G; ++g) {
            const size_t k = (size_t)row * 64 + (size_t)((l % vps) * G + g);
            uint32_t i; T y[3][2];
            lm_y_block<T>(tb, ps, k, dv, i, y);
            const T* xi = x + ((size_t)i * NV + c) * 3;
            const T y0 = a ? y[0][1] : y[0][0], y1 = a ? y[1][1] : y[1][0], y2 = a ? y[2][1] : y[2][0];
            s += y0 * xi[0] + y1 * xi[1] + y2 * xi[2];
        }
    red[lane] = s;
    __syncthreads();
    if (part != 0) return;
    T acc = 0;
    for (int q = 0; q < kParts; ++q) acc += red[q * kPairs + pair];
    const MbColumn q = cols[c];
    double v = 0;
    if (q.kind == 0) v = (double)(T(kMbCrossSign) * acc);
    else if (q.kind == 1) v = (double)(q.idx == l ? acc + dv[a == q.comp ? 2 * a : 1] : acc);      // Dl^-1 = (ixx ixy; ixy iyy)
    o[(size_t)a * NV + c] = v;
}

}  // namespace tsgo
