// tsgo_kernels.h — the hand-written gfx950 kernels of the Gauss-Newton hot path.
//
// Execution shape shared by every "table" kernel: one 64-lane wavefront per SELL slice, G lanes
// (1, 2, 4 or 8) cooperating on one vertex, a workgroup of 256 threads = 4 slices.  A lane walks the
// rows of its slice; every per-slot plane load is a fully coalesced 64-lane row (512 B in f64), the
// only irregular access is ONE small gathered record per slot (a 64-B pose record or a 16-B
// landmark vector).  Sums over a vertex's edges stay in registers and finish with G-lane xor
// shuffles: no atomics anywhere, results are bitwise reproducible.  MFMA is not used: there is no
// dense contraction on this path (blocks are 3x3 / 3x2 and the arithmetic intensity is < 1 flop/B).
//
// What each kernel replaces in the reference's CUDA pipeline (function, not code):
//   lin_lm / lin_pose   ProcessSe2Point2s + ProcessSe2s  (remote/cuda/optimizer/kernels/
//                       KernelSe2Point2.cu:46-155, KernelSe2.cu:37-112): residual, Jacobian, Huber,
//                       J^T W J / J^T W r — but into block-sparse storage by segmented register sums
//                       instead of 25-36 atomicAdds per edge into a dense n x n H
//   pose_finalize       FixVertices + Negativate (KernelCommon.cu:6-25,62-71) + preconditioner
//   schur_lm/schur_pose + cg_update   the linear solve (cuSOLVER geqrf/ormqr + cuBLAS trsm,
//                       remote/cuda/solver/SolverCudaQr.h:51-79) as implicit-Schur PCG
//   pose_update / schur_lm<BACKSUB>   Update (KernelCommon.cu:27-60)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/problem.h"      // record layouts of the prior CSR (PRI_*, PRL_*)
#include "tsgo_math.h"

namespace tsgo {

constexpr int kBlock = 256;             // threads per workgroup = 4 wavefronts
constexpr int kWavesPerBlock = kBlock / 64;
constexpr uint32_t kDirMask = 0x80000000u;      // odom slot: the row's pose is the edge's second vertex
constexpr uint32_t kVlmMask = 0x40000000u;      // odom slot: a virtual landmark measurement (edge type 2), general-pairs kernels only
constexpr uint32_t kPoseIdxMask = 0x3FFFFFFFu;  // odom slot: the neighbour's internal pose number

// record layouts (in units of T)
constexpr int kPoseRec = 8;   // zc: v0 v1 v2 c s . . .      (the vector CG multiplies + the pose's cos/sin)
constexpr int kNinvRec = 4;   // ninv: ixx ixy iyy .          (Dl^-1 alone, what k_schur_lm's product mode reads)
constexpr int kLmRec = 8;     // lmrec: lx ly ixx ixy iyy ux uy .   (landmark, Dl^-1, u = Dl^-1 g_l)

// 16-byte (f64) / 8-byte (f32) pair loads for the gathered records: one gathered 64-B pose record costs
// three load instructions instead of five (each wave-instruction of a gather touches 64 lines).
template <typename T> struct Pair;
template <> struct Pair<double> { using type = double2; };
template <> struct Pair<float> { using type = float2; };
template <typename T> __device__ __forceinline__ typename Pair<T>::type ld2(const T* p) {
    return *reinterpret_cast<const typename Pair<T>::type*>(p);
}

template <typename T> __device__ __forceinline__ void st2(T* p, T a, T b) {
    typename Pair<T>::type v; v.x = a; v.y = b;
    *reinterpret_cast<typename Pair<T>::type*>(p) = v;
}

// Keeps the compiler from sinking a load below an early exit: the value must exist when this statement is reached, so the load
// that produces it is issued (and waited for) before the test that follows — beside the flag's own load instead of behind it.
template <typename V> __device__ __forceinline__ void issue_before_exit(V& v) { asm volatile("" : "+v"(v)); }

template <typename T> struct CgState { T gamma_old, alpha_old, gamma0, pad; int iters, done, fail, pad2; };

// LM tables keep their per-slot values as 16-byte PAIRS, pair-plane-major: st = [(zx,zy) | (w0,w1)],
// dyn = [(a0,a1) | (ppx,ppy)], element k of pair-plane q at (q*slots + k)*2: one dwordx4 per lane and
// plane instead of two dwordx2 (8-byte lanes stream at 0.54-0.70x the 16-byte rate, MI355X_MICROARCH.md).
// The ODOM table keeps single-value planes.  dyn32 = the same four numbers of every LM slot as ONE float4: the two
// Schur products INSIDE the multigrid cycle read it instead (a preconditioner tolerates f32 operands; the
// product PCG itself takes stays f64).
template <typename T> struct Table {       // one SELL table on the device
    const uint32_t* row_off; const uint32_t* idx; const T* st; T* dyn; float4* dyn32; size_t slots; int n_slices; int n_vertices; int xcd;
};

// XCD-aware workgroup -> slice-group map (guide T1).  Workgroups are dealt round-robin over the 8 XCDs,
// each with a private L2; giving XCD x the x-th contiguous eighth of the slices makes every gathered
// record (pose records, landmark vectors) live in ONE L2 instead of being pulled into all eight
// (profiles/r01a: 1.7x over-fetch on k_schur_lm).  Grids are rounded up to a multiple of 8; only speed
// depends on the placement guess, never correctness.
// xcd_block(eighth): for the kernels whose argument head carries the grid's eighth (xcd8 = gridDim.x / 8 under the map, 0 for
// round-robin): gridDim.x itself is a hidden kernel argument that would be fetched from memory.
__device__ __forceinline__ int xcd_block(int eighth) { return (int)((blockIdx.x % 8u) * (unsigned)eighth + blockIdx.x / 8u); }
__device__ __forceinline__ int xcd_block() { return xcd_block((int)(gridDim.x / 8u)); }

// ---- accessors of the table kernels: values in, values out -------------------------------------------------------------------------
// Where a thread stands: its slice (through the XCD map when the table asks for it), its lane, the vertex its group of G lanes works on,
// whether the slice exists, and whether the lane is the group's head (the one that writes the vertex's result and folds its priors).
struct Walk { int slice, lane, vertex, live, head; };
template <int G> __device__ __forceinline__ Walk walk_of(int n_slices, int xcd8) {      // xcd8: 0, or gridDim.x / 8 under the XCD map
    Walk w;
    w.slice = (xcd8 ? xcd_block(xcd8) : (int)blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    w.live = w.slice < n_slices;
    w.lane = threadIdx.x & 63;
    w.vertex = w.slice * (64 / G) + w.lane / G;
    w.head = (w.lane % G) == 0;
    return w;
}
// (a table kernel without an argument head hands over its Table's: table_xcd8)
template <typename T> __device__ __forceinline__ int table_xcd8(const Table<T>& tb) { return tb.xcd ? (int)(gridDim.x / 8u) : 0; }

// Argument heads.  The command processor of gfx950 delivers the first 14 dwords of a kernel's arguments in SGPRs before the wave starts
// (kernarg preload, the build's -amdgpu-kernarg-preload-count), but only the leading run of PLAIN arguments: it stops at the first
// by-value aggregate.  The kernels launched per PCG iteration or per Gauss-Newton step therefore begin with what they need before their
// first vector load is issued, as pointers and ints (a pointer is 2 dwords and 8-byte aligned); the aggregates come behind.  The table
// kernels of that set start with the walked table's (row_off, n_slices, n_vertices, xcd8) — xcd8: the grid's eighth under the XCD map,
// else 0; Engine::launch_table lists them — and read those four from the head alone: the copies inside their Table argument are not
// used.  tools/kernarg_heads.py checks the assembly.

// LM slot k: what was measured (static planes), what the linearisation left (dyn, or dyn32 under LOW), and the store of both copies.
template <typename T> struct LmMeas { T zx, zy, w0, w1; };
template <typename T> __device__ __forceinline__ LmMeas<T> lm_meas(const Table<T>& tb, size_t k) {
    const auto zz = ld2<T>(tb.st + 2 * k), ww = ld2<T>(tb.st + 2 * (tb.slots + k));
    return {zz.x, zz.y, ww.x, ww.y};
}
template <typename T> struct LmSlot { T a0, a1, ppx, ppy; };
template <typename T, int LOW = 0> __device__ __forceinline__ LmSlot<T> lm_slot(const Table<T>& tb, size_t k) {
    if (LOW) { const float4 f = tb.dyn32[k]; return {f.x, f.y, f.z, f.w}; }
    const auto aa = ld2<T>(tb.dyn + 2 * k), pp = ld2<T>(tb.dyn + 2 * (tb.slots + k));
    return {aa.x, aa.y, pp.x, pp.y};
}
template <typename T> __device__ __forceinline__ void lm_slot_store(const Table<T>& tb, size_t k, const LmLin<T>& o) {
    st2<T>(tb.dyn + 2 * k, o.a0, o.a1); st2<T>(tb.dyn + 2 * (tb.slots + k), o.ppx, o.ppy);
    tb.dyn32[k] = make_float4((float)o.a0, (float)o.a1, (float)o.ppx, (float)o.ppy);
}

// Pose-pose slot k: the nine static planes (mi, w; a virtual landmark slot keeps its two points and two weights there) and the
// PP_PLANES dynamic planes of the general form (tsgo_math.h).
template <typename T> struct OdomMeas { T mi[6], w[3]; };
template <typename T> __device__ __forceinline__ OdomMeas<T> odom_meas(const Table<T>& od, size_t k) {
    OdomMeas<T> o;
#pragma unroll
    for (int m = 0; m < 6; ++m) o.mi[m] = od.st[(size_t)m * od.slots + k];
#pragma unroll
    for (int m = 0; m < 3; ++m) o.w[m] = od.st[(size_t)(6 + m) * od.slots + k];
    return o;
}
template <typename T> __device__ __forceinline__ PairSlot<T> pair_slot(const T* dyn, size_t S, size_t k) {
    PairSlot<T> h;
#pragma unroll
    for (int m = 0; m < PP_PLANES; ++m) h.v[m] = dyn[(size_t)m * S + k];
    return h;
}

// Pose record i of zc (or of its f32 copy zc32 under LOW: 32 B instead of 64 gathered through L2): the vector and the pose's cos / sin.
template <typename T> struct PoseVec { T v0, v1, v2, c, s; };
template <typename T, int LOW> __device__ __forceinline__ PoseVec<T> pose_vec(const T* zc, const float* zc32, size_t i) {
    if (LOW) { const float* zr = zc32 + i * kPoseRec; const float4 q = *reinterpret_cast<const float4*>(zr); return {q.x, q.y, q.z, q.w, zr[4]}; }
    const T* zr = zc + i * kPoseRec;
    const auto z01 = ld2<T>(zr), z23 = ld2<T>(zr + 2);
    return {z01.x, z01.y, z23.x, z23.y, zr[4]};
}

// lane_xor<M>(v): the value lane (i ^ M) holds, M one of 1, 2, 4, 8, 16, 32 — the exchange every lane sum below is made of.  __shfl_xor
// is a ds_bpermute_b32 per dword: a trip through the LDS crossbar (its latency that of an LDS read) in each of the up to six DEPENDENT
// rounds of a sum, at the tail of every kernel's longest wave.  The same exchange without leaving the VALU:
//   M = 1, 2   DPP quad_perm [1,0,3,2] / [2,3,0,1]                 (the compiler folds the move into the add that follows)
//   M = 4      two DPP moves inside the row of 16: lanes of banks 0 and 2 read four lanes up (row_shl:4, bank mask 0x5), banks 1 and 3
//              four lanes down (row_shr:4, bank mask 0xa)
//   M = 8      DPP row_ror:8
//   M = 16, 32 v_permlane16_swap / v_permlane32_swap of the value with itself: result 0 holds the partner's value in the odd rows
//              (upper half), result 1 in the even rows (lower half)
// 8-byte values move as two dwords.  A true xor exchange: every lane adds the same two operands as under __shfl_xor, the sums keep their
// bits.  What differs between the forms is what a lane reads from a partner the EXEC mask has switched off, so the sums are called where
// the wave's control flow has converged: every call site (this file, tsgo_amg_kernels.h, tsgo_block_row.h's users, the marginal, sample,
// init, lm and dogleg kernels) is reached either by whole waves — wk.live, st->done, row bounds and kernel arguments are wave-uniform; the
// clamp path of block_row keeps every lane of a surplus workgroup walking the last row — or BEHIND the lane-divergent walk (row_dot's
// strided loop, the tables' padding `continue`, k_pair_gemm_wave's `if (live)` loop), never inside it: none had to be made uniform.
// Blocks are one-dimensional and a multiple of 64 threads: threadIdx.x & 63 is the lane.  (The struct reductions of the edge-report and GNC
// kernels and the integer sums of the pattern builders are not these sums and keep __shfl_xor.)
// TSGO_SHUFFLE_SUMS (build.py: the plain library) keeps the __shfl_xor forms, and the two-sums-one-after-the-other shape of
// block_sum2 and k_cg_step's prologue: the B side of the bitwise comparison.
#ifndef TSGO_SHUFFLE_SUMS
template <int M> __device__ __forceinline__ uint32_t lane_xor_dword(uint32_t u) {
    static_assert(M == 1 || M == 2 || M == 4 || M == 8 || M == 16 || M == 32, "lane_xor: one bit of the lane number");
    const int v = (int)u;
    // __builtin_amdgcn_mov_dpp(src, dpp_ctrl, row_mask, bank_mask, bound_ctrl), __builtin_amdgcn_update_dpp(old, src, ...)
    // (M = 1, 2, 8 read a lane of the row whatever the lane: no `old` value, bound_ctrl — the form the compiler folds into an f32 add)
    if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);                 // quad_perm:[1,0,3,2]
    else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);            // quad_perm:[2,3,0,1]
    else if constexpr (M == 4) {
        const int up = __builtin_amdgcn_update_dpp(v, v, 0x104, 0xf, 0x5, false);                             // row_shl:4: lane i reads i + 4
        return (uint32_t)__builtin_amdgcn_update_dpp(up, v, 0x114, 0xf, 0xa, false);                          // row_shr:4: lane i reads i - 4
    }
    else if constexpr (M == 8) return (uint32_t)__builtin_amdgcn_mov_dpp(v, 0x128, 0xf, 0xf, true);           // row_ror:8
    else if constexpr (M == 16) { const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false); return (threadIdx.x & 16u) ? r[0] : r[1]; }
    else { const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false); return (threadIdx.x & 32u) ? r[0] : r[1]; }
}
template <int M, typename T> __device__ __forceinline__ T lane_xor(T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "lane_xor: one or two dwords");
    if constexpr (sizeof(T) == 4) {
        uint32_t u;
        __builtin_memcpy(&u, &v, 4);
        u = lane_xor_dword<M>(u);
        __builtin_memcpy(&v, &u, 4);
    } else {
        uint32_t u[2];
        __builtin_memcpy(u, &v, 8);
        u[0] = lane_xor_dword<M>(u[0]); u[1] = lane_xor_dword<M>(u[1]);
        __builtin_memcpy(&v, u, 8);
    }
    return v;
}
#else
template <int M, typename T> __device__ __forceinline__ T lane_xor(T v) { return __shfl_xor(v, M); }
#endif

// Sum over the G lanes of a group (masks ascending) and over the wave (masks descending): every lane gets the result.
template <typename T, int G, int M = 1> __device__ __forceinline__ T group_sum(T v) {
    if constexpr (M < G) { v += lane_xor<M>(v); return group_sum<T, G, 2 * M>(v); }
    else return v;
}

template <typename T, int M = 32> __device__ __forceinline__ T wave_sum(T v) {
    v += lane_xor<M>(v);
    if constexpr (M > 1) return wave_sum<T, M / 2>(v);
    else return v;
}

// Sum over the workgroup; every thread gets the result.  `red` = kWavesPerBlock T's of LDS.
template <typename T> __device__ __forceinline__ T block_sum(T v, T* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    T s = red[0];
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) s += red[k];
    return s;
}

// Two workgroup sums through the same rounds: the lane exchanges of a and b interleave (two independent chains instead of one after the
// other), ONE barrier pair, two rows of LDS.  Per value the order of the additions is block_sum's.  `red` = 2 * kWavesPerBlock T's.
template <typename T> __device__ __forceinline__ void block_sum2(T& a, T& b, T* red) {
#ifdef TSGO_SHUFFLE_SUMS
    a = block_sum<T>(a, red); b = block_sum<T>(b, red);
#else
    a = wave_sum(a); b = wave_sum(b);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[kWavesPerBlock + w] = b; }
    __syncthreads();
    a = red[0]; b = red[kWavesPerBlock];
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) { a += red[k]; b += red[kWavesPerBlock + k]; }
#endif
}

// Fixed-order sum of n partials by a whole workgroup (n is a few hundred).
template <typename T> __device__ __forceinline__ T block_sum_array(const T* a, int n, T* red) {
    T v = 0;
    for (int k = threadIdx.x; k < n; k += kBlock) v += a[k];
    return block_sum(v, red);
}

// The stopping rule of the multigrid-preconditioned PCG, evaluated by ONE workgroup at the start of an iteration (tsgo_amg_kernels.h:
// k_iter_gate, or workgroup 0 of the iteration's first product kernel): sums the partials of r^T D^-1 r (left by k_cg_step) and of
// b^T D^-1 b, sets st->done when the residual meets the tolerance, and — eager launches — tells the host thread in ONE aligned 8-byte
// store that the seq-th launched iteration has started and what it saw (seq | done | fail | iterations completed; Engine::do_solve_paced).
template <typename T> struct GateArgs { CgState<T>* st; const T* rdr_part; const T* bpart; int n; T tol2; int* host_flag; int seq; };
template <typename T> __device__ __forceinline__ int iter_gate_body(const GateArgs<T> g, T* red) {      // thread 0 returns the verdict (done); red: 2 * kWavesPerBlock
    const int done = g.st->done, iters = g.st->iters, fail0 = g.st->fail;
    T a = 0, b = 0;                                  // the partials are on their way while the state is looked at
    for (int k = threadIdx.x; k < g.n; k += kBlock) { a += g.rdr_part[k]; b += g.bpart[k]; }
    issue_before_exit(a);
    int done_now = done, fail_now = fail0;
    if (!(done || iters == 0)) {                     // iteration 0: no step has been taken yet (a warm start is judged by k_warm_scale)
        block_sum2<T>(a, b, red);
        const T rdr = a, bdb = b;
        if (threadIdx.x == 0 && !(rdr > g.tol2 * bdb)) { fail_now = (rdr != rdr) ? 1 : 0; done_now = 1; g.st->done = 1; g.st->fail = fail_now; }      // NaN: breakdown
    }
    if (g.host_flag && threadIdx.x == 0)      // ONE aligned 8-byte store: the host never sees the fields of two gates mixed
        *reinterpret_cast<volatile unsigned long long*>(g.host_flag) =
            ((unsigned long long)(unsigned)g.seq << 32) | ((unsigned long long)(done_now ? 1u : 0u) << 31) | ((unsigned long long)((unsigned)fail_now & 7u) << 28) | (unsigned long long)((unsigned)iters & 0x0fffffffu);
    return done_now;
}

// Unary priors (edge types 3 and 4, include/tsgo.h), folded in by the lane that writes a vertex's result, in input order, in the world
// frame; records behind a CSR of offsets per internal vertex (host/problem.h: PRI_*, PRL_*).  lm_chi / n_lm_chi: the per-workgroup chi^2
// partials of the landmark priors (k_lin_lm<.., 1>), which workgroup 0 of k_lin_pose<.., .., 1> adds to its own partial in a fixed order.
template <typename T> struct PriorArgs { const uint32_t* off; const T* rec; T* lm_chi; int n_lm_chi; };

// Robust kernels per edge class (tsgo_set_robust; tsgo_math.h: robust_eval), the compile-time axis RK of the kernels that robustify:
// RK = 0 is the compile-time Huber (delta 1.5) — what a handle with the default setting launches, the same instructions as before the
// setting existed; RK = 1 reads kind and width of the class whose table is being walked from this by-value kernel argument (kernarg
// memory, scalar loads).  The class is known where the edge function is called (the LM rows, ODOM against virtual landmark by kVlmMask,
// the prior records) and the kind is the same for every lane: the selection in robust_eval is a scalar branch.
//
// RK = 2: robust kernels per EDGE (tsgo_set_edge_robust, include/tsgo.h; engine/engine_edge_robust.inc).  An edge carries one byte: 0 leaves
// it to its class (kind and width from this argument, as under RK = 1, so a later tsgo_set_robust applies), k >= 1 gives it entry k - 1 of
// the handle's palette, a device table of at most kEdgeRobustMax (width, kind) records of 16 B in f64 — one pair load, and the whole
// table sits in a handful of cache lines.  The kernels that walk a table read the byte of the SLOT (one array per table, in slot order:
// contiguous in lane order like the slot's own planes, 0 on padding) or of the prior RECORD; the visitors of the once-per-edge walk and
// the sampling kernels, which hold the input edge index anyway, read the byte of the EDGE.  The kernel object is then per lane and
// robust_eval a per-lane switch: divergent only in rows that mix kernels.  f64 only.  The pointers sit behind the class fields and are
// null (never read) under RK = 0 and 1.
constexpr int kEdgeRobustMax = 15;
template <typename T> struct RobustEntry { T delta; int kind; int pad; };
template <typename T> struct RobustArgs {
    int kind[kEdgeClasses]; int pad; T delta[kEdgeClasses];
    const RobustEntry<T>* pal;                                  // RK = 2 from here on: the palette
    const uint8_t *by_lm, *by_pose, *odom;                      // ... a byte per slot of the lm-major LM, pose-major LM and pose-pose tables
    const uint8_t *pose_prior, *lm_prior;                       // ... a byte per prior record
    const uint8_t* edge;                                        // ... a byte per input edge
};
template <int RK, typename T> __device__ __forceinline__ auto robust_class(const RobustArgs<T>& ra, int cls) {
    if constexpr (RK == 0) return HuberDefault{};
    else return Robust<T>{ra.kind[cls], ra.delta[cls]};
}
// The kernel of ONE slot, record or edge: the class's (cls_kernel = robust_class<RK>) unless RK = 2 and bytes[k] names a palette entry.
template <int RK, typename T, typename K> __device__ __forceinline__ K robust_at(const RobustArgs<T>& ra, const K& cls_kernel, const uint8_t* __restrict__ bytes, size_t k) {
    if constexpr (RK == 2) {
        const uint32_t b = bytes[k];
        if (b != 0u) { const RobustEntry<T> e = ra.pal[b - 1u]; return Robust<T>{e.kind, e.delta}; }
    }
    return cls_kernel;
}

// Pose prior (type 3): e_t = R_m^T (t - t_m), e_th = wrap(th - m_th); J = blockdiag(R_m^T, 1).  With a = robust weight * (w0, w1, w2):
// H_pp += [[R_m diag(a0, a1) R_m^T, 0], [0, a2]] (h00 h01 h11 h22), b_p -= J^T diag(a) e (b0 b1 b2); returns rho.  rk: the class's robust kernel.
template <typename T, typename K> __device__ __forceinline__ T pose_prior_fold(const T* q, T x, T y, T c, T s, T& h00, T& h01, T& h11, T& h22, T& b0, T& b1, T& b2, const K& rk) {
    const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C), w01 = ld2<T>(q + PRI_W0);
    const T cm = cs.x, sm = cs.y;
    const PosePriorLin<T> o = pose_prior_linearize<T>(m01.x, m01.y, cm, sm, w01.x, w01.y, q[PRI_W2], x, y, c, s, rk);
    h00 += o.a0 * cm * cm + o.a1 * sm * sm; h01 += (o.a0 - o.a1) * cm * sm; h11 += o.a0 * sm * sm + o.a1 * cm * cm; h22 += o.a2;
    const T f0 = o.a0 * o.e0, f1 = o.a1 * o.e1;
    b0 -= cm * f0 - sm * f1; b1 -= sm * f0 + cm * f1; b2 -= o.a2 * o.et;
    return o.rho;
}

// ------------------------------------------------------------------------------------------------
// K1 lin_lm: per landmark — landmark-side linearisation of its LM edges.
//   reads : slot planes zx zy w0 w1 + pose index (coalesced), pose state ps[i] = (x,y,c,s) (gather)
//   writes: slot planes a0 a1 ppx ppy (lm-major copy), lmrec[l][2..6] = Dl^-1, u
// PRI = 1: the landmark priors (type 4: D_l += Omega_w, b_l -= Omega_w (l - m)) before the inverse, and one chi^2 partial of them per
// workgroup into pa.lm_chi (every wave reaches the workgroup sum: none leaves early)
// RK = 1: the robust kernels of classes LM and landmark prior from ra (RobustArgs above); RK = 2: per slot / per record (ra.by_lm, ra.lm_prior)
template <typename T, int G, int PRI = 0, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_lin_lm(const uint32_t* __restrict__ row_off, int n_slices, int n_vertices, int xcd8, int zero_fixed,
                                                   T* __restrict__ lmrec, const T* __restrict__ ps, const T* __restrict__ gauge_l,
                                                   T* __restrict__ ninv, Table<T> tb, T lambda,
                                                   const PriorArgs<T> pa = PriorArgs<T>{nullptr, nullptr, nullptr, 0},
                                                   const RobustArgs<T> ra = RobustArgs<T>{}) {
    const Walk wk = walk_of<G>(n_slices, xcd8);
    const int slice = wk.slice, lane = wk.lane, l = wk.vertex, live = wk.live;
    if (!PRI && !live) return;
    const auto rk_lm = robust_class<RK>(ra, kClassLm);
    const bool valid = l < n_vertices;      // (false on every lane of a wave past the last slice)
    const int lc = valid ? l : n_vertices - 1;
    const T lx = lmrec[(size_t)lc * kLmRec], ly = lmrec[(size_t)lc * kLmRec + 1];
    T dxx = 0, dxy = 0, dyy = 0, g0 = 0, g1 = 0;
    T chi = 0;
    const uint32_t r0 = live ? row_off[slice] : 0u, r1 = live ? row_off[slice + 1] : 0u;
    for (uint32_t row = r0; row < r1; ++row) {
        const size_t k = (size_t)row * 64 + lane;
        const uint32_t i = tb.idx[k];
        const LmMeas<T> z = lm_meas<T>(tb, k);
        const T* q = ps + (size_t)i * 4;
        const auto q01 = ld2<T>(q), q23 = ld2<T>(q + 2);
        const T x = q01.x, y = q01.y, c = q23.x, s = q23.y;
        const LmLin<T> o = lm_linearize<T>(x, y, c, s, lx, ly, z.zx, z.zy, z.w0, z.w1, robust_at<RK>(ra, rk_lm, ra.by_lm, k));
        lm_slot_store<T>(tb, k, o);
        dxx += o.a0 * c * c + o.a1 * s * s; dxy += (o.a0 - o.a1) * c * s; dyy += o.a0 * s * s + o.a1 * c * c;
        const T f0 = o.a0 * o.e0, f1 = o.a1 * o.e1;
        g0 -= c * f0 - s * f1; g1 -= s * f0 + c * f1;
    }
    dxx = group_sum<T, G>(dxx); dxy = group_sum<T, G>(dxy); dyy = group_sum<T, G>(dyy);
    g0 = group_sum<T, G>(g0); g1 = group_sum<T, G>(g1);
    if (valid && wk.head) {
        // lambda: the LM-style damping of the reference's Python optimizer (H + lambda I, graph_optimizer.py:42), 0 under the
        // cpu/eigen rules; zero_fixed: that optimizer also zeroes b at fixed vertices (:150), OptimizerCpu.h does not
        if constexpr (PRI != 0) {
            for (uint32_t k = pa.off[l]; k < pa.off[l + 1]; ++k) {
                const T* q = pa.rec + (size_t)k * PRI_LM_REC;
                const auto m = ld2<T>(q + PRL_MX), w = ld2<T>(q + PRL_W0);
                const LmPriorLin<T> o = lm_prior_linearize<T>(m.x, m.y, w.x, w.y, lx, ly, robust_at<RK>(ra, robust_class<RK>(ra, kClassLmPrior), ra.lm_prior, k));
                dxx += o.a0; dyy += o.a1; g0 -= o.a0 * o.e0; g1 -= o.a1 * o.e1;
                chi += o.rho;
            }
        }
        const T ga = gauge_l[l];
        if (zero_fixed && ga > T(0)) { g0 = 0; g1 = 0; }
        T ixx, ixy, iyy;
        inv_sym2<T>(dxx + ga + lambda, dxy, dyy + ga + lambda, ixx, ixy, iyy);
        T* o = lmrec + (size_t)l * kLmRec;
        o[2] = ixx; o[3] = ixy; o[4] = iyy; o[5] = ixx * g0 + ixy * g1; o[6] = ixy * g0 + iyy * g1;
        // compact copy of Dl^-1 for the Schur product's epilogue: 32 B per landmark instead of a 64-B record
        T* nq = ninv + (size_t)l * kNinvRec;
        nq[0] = ixx; nq[1] = ixy; nq[2] = iyy;
    }
    if constexpr (PRI != 0) {
        __shared__ T red[kWavesPerBlock];
        const T total = block_sum<T>(chi, red);
        if (threadIdx.x == 0) pa.lm_chi[blockIdx.x] = total;
    }
}

// ------------------------------------------------------------------------------------------------
// K2 lin_pose: per pose — pose-side linearisation of its LM edges + its ODOM rows.
//   writes: slot planes (pose-major copy), ODOM weights, part[i][18] = Dp(6) g(3) Sd(6) Wu(3) in the
//           world frame, one chi^2 partial per workgroup
// OJ = 1: pose-pose slots in GENERAL form (tsgo_math.h: eight dynamic planes per slot, the slot's own row block of the Hessian) — what
// analytic ODOM Jacobians (odom_analytic, tsgo_config.odom_jacobian) and virtual landmark measurements (edge type 2, kVlmMask) need;
// ODOM edges under the reference's constant Jacobians are written in that form too when the graph holds the other kind.
// PRI = 1: the pose priors (type 3, pose_prior_fold) of the pose in the epilogue, before a fixed pose's gradient is zeroed, and the landmark
// priors' chi^2 partials (pa.lm_chi, left by k_lin_lm<.., 1>) in workgroup 0's partial.  The host lists only the priors of owned poses.
// RK = 1: the robust kernels of classes LM, ODOM, virtual landmark and pose prior from ra (RobustArgs above); RK = 2: per slot / per record
// (ra.by_pose, ra.odom — both slots of a pose-pose edge carry its byte — and ra.pose_prior)
template <typename T, int G, int OJ = 0, int PRI = 0, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_lin_pose(const uint32_t* __restrict__ row_off, int n_slices, int n_vertices, int xcd8, int zero_fixed,
                                                     const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                     const uint32_t* __restrict__ od_row_off, const T* __restrict__ gauge_p,
                                                     Table<T> tb, Table<T> od, int pose_first, int pose_last, T* __restrict__ part,
                                                     T* __restrict__ chi_part, T lambda, int odom_analytic = 0,
                                                     const PriorArgs<T> pa = PriorArgs<T>{nullptr, nullptr, nullptr, 0},
                                                     const RobustArgs<T> ra = RobustArgs<T>{}) {
    __shared__ T red[kWavesPerBlock];
    const Walk wk = walk_of<G>(n_slices, xcd8);
    const int slice = wk.slice, lane = wk.lane, i = wk.vertex;
    const bool live = wk.live, valid = live && i < n_vertices;
    const auto rk_lm = robust_class<RK>(ra, kClassLm), rk_odom = robust_class<RK>(ra, kClassOdom);
    T chi = 0;
    if (live) {
        const int ic = valid ? i : n_vertices - 1;
        const T x0 = ps[(size_t)ic * 4], y0 = ps[(size_t)ic * 4 + 1], c = ps[(size_t)ic * 4 + 2], s = ps[(size_t)ic * 4 + 3];
        T sA0 = 0, sA1 = 0, sAv0 = 0, sAv1 = 0, sVV = 0, ge0 = 0, ge1 = 0, get = 0;
        T K00 = 0, K01 = 0, K11 = 0, Kv0 = 0, Kv1 = 0, vKv = 0, wu0 = 0, wu1 = 0, wut = 0;
        {
            const uint32_t r0 = row_off[slice], r1 = row_off[slice + 1];
            for (uint32_t row = r0; row < r1; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t l = tb.idx[k];
                const LmMeas<T> z = lm_meas<T>(tb, k);
                const T* lr = lmrec + (size_t)l * kLmRec;
                const auto l01 = ld2<T>(lr), l23 = ld2<T>(lr + 2), l45 = ld2<T>(lr + 4);
                const T lx = l01.x, ly = l01.y, nxx = l23.x, nxy = l23.y, nyy = l45.x, ux = l45.y, uy = lr[6];
                const LmLin<T> o = lm_linearize<T>(x0, y0, c, s, lx, ly, z.zx, z.zy, z.w0, z.w1, robust_at<RK>(ra, rk_lm, ra.by_pose, k));
                lm_slot_store<T>(tb, k, o);
                chi += o.rho;
                const T v0 = o.ppy, v1 = -o.ppx;
                sA0 += o.a0; sA1 += o.a1; sAv0 += o.a0 * v0; sAv1 += o.a1 * v1; sVV += o.a0 * v0 * v0 + o.a1 * v1 * v1;
                ge0 += o.a0 * o.e0; ge1 += o.a1 * o.e1; get += o.a0 * o.e0 * v0 + o.a1 * o.e1 * v1;
                const T n00 = c * c * nxx + 2 * c * s * nxy + s * s * nyy;
                const T n01 = c * s * (nyy - nxx) + (c * c - s * s) * nxy;
                const T n11 = s * s * nxx - 2 * c * s * nxy + c * c * nyy;
                const T k00 = o.a0 * n00 * o.a0, k01 = o.a0 * n01 * o.a1, k11 = o.a1 * n11 * o.a1;
                K00 += k00; K01 += k01; K11 += k11;
                const T kv0 = k00 * v0 + k01 * v1, kv1 = k01 * v0 + k11 * v1;
                Kv0 += kv0; Kv1 += kv1; vKv += v0 * kv0 + v1 * kv1;
                const T t0 = c * ux + s * uy, t1 = c * uy - s * ux;
                wu0 += o.a0 * t0; wu1 += o.a1 * t1; wut += o.a0 * t0 * v0 + o.a1 * t1 * v1;
            }
        }
        // ODOM rows (listed at both endpoints; chi^2 counted at id1)
        T od0 = 0, od1 = 0, od2 = 0, og0 = 0, og1 = 0, og2 = 0;
        T od01 = 0, od02 = 0, od12 = 0;        // off-diagonal entries of the pose's ODOM diagonal block: analytic Jacobians only
        {
            const size_t S = od.slots;
            const uint32_t r0 = od_row_off[slice], r1 = od_row_off[slice + 1];
            for (uint32_t row = r0; row < r1; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t raw = od.idx[k];
                const bool second = (raw & kDirMask) != 0;
                const uint32_t j = raw & kPoseIdxMask;
                const OdomMeas<T> z = odom_meas<T>(od, k);
                const T* oq = ps + (size_t)j * 4;
                const T xj = oq[0], yj = oq[1], cj = oq[2], sj = oq[3];
                if (OJ && (raw & kVlmMask)) {      // virtual landmark measurement: mi = (pox, poy, pnx, pny, ., .), w = (w0, w1, .)
                    const VlmLin<T> v = vlm_linearize<T>(x0, y0, c, s, xj, yj, cj, sj, z.mi[0], z.mi[1], z.mi[2], z.mi[3], z.w[0], z.w[1],
                                                               robust_at<RK>(ra, robust_class<RK>(ra, kClassVlm), ra.odom, k));
                    T h[PP_PLANES];
                    vlm_slot<T>(v, h);
#pragma unroll
                    for (int m = 0; m < PP_PLANES; ++m) od.dyn[(size_t)m * S + k] = h[m];
                    od0 += v.om0; od1 += v.om1; od02 += v.om0 * v.u0; od12 += v.om1 * v.u1; od2 += v.om0 * v.u0 * v.u0 + v.om1 * v.u1 * v.u1;
                    og0 -= v.om0 * v.d0; og1 -= v.om1 * v.d1; og2 -= v.om0 * v.u0 * v.d0 + v.om1 * v.u1 * v.d1;
                    if (!second) chi += v.rho;
                    continue;
                }
                const auto rk_slot = robust_at<RK>(ra, rk_odom, ra.odom, k);
                const OdomLin<T> o = second ? odom_linearize<T>(xj, yj, cj, sj, x0, y0, c, s, z.mi, z.w, rk_slot)
                                            : odom_linearize<T>(x0, y0, c, s, xj, yj, cj, sj, z.mi, z.w, rk_slot);
                if (OJ && odom_analytic) {
                    const OdomBlocks<T> ob = second ? odom_blocks<T>(o, xj, yj, cj, sj, x0, y0, c, s, z.mi) : odom_blocks<T>(o, x0, y0, c, s, xj, yj, cj, sj, z.mi);
                    // H_12 = [[-K, 0], [g^T, -w]] at the first endpoint, its transpose at the second
                    od.dyn[(size_t)PP_K00 * S + k] = ob.k00; od.dyn[(size_t)PP_K01 * S + k] = ob.k01; od.dyn[(size_t)PP_K11 * S + k] = ob.k11;
                    od.dyn[(size_t)PP_C0 * S + k] = second ? ob.g0 : T(0); od.dyn[(size_t)PP_C1 * S + k] = second ? ob.g1 : T(0);
                    od.dyn[(size_t)PP_R0 * S + k] = second ? T(0) : ob.g0; od.dyn[(size_t)PP_R1 * S + k] = second ? T(0) : ob.g1;
                    od.dyn[(size_t)PP_KAPPA * S + k] = ob.w;
                    od0 += ob.k00; od01 += ob.k01; od1 += ob.k11;
                    if (!second) { od02 -= ob.g0; od12 -= ob.g1; od2 += ob.s + ob.w; og0 += ob.h0; og1 += ob.h1; og2 += ob.kt - ob.ht; }
                    else { od2 += ob.w; og0 -= ob.h0; og1 -= ob.h1; og2 -= ob.kt; }
                } else {
                    if (OJ) {      // the reference's constants in the general form: K = diag(a0, a1), c = r = 0, kappa = a2
                        od.dyn[(size_t)PP_K00 * S + k] = o.a[0]; od.dyn[(size_t)PP_K01 * S + k] = T(0); od.dyn[(size_t)PP_K11 * S + k] = o.a[1];
                        od.dyn[(size_t)PP_C0 * S + k] = T(0); od.dyn[(size_t)PP_C1 * S + k] = T(0); od.dyn[(size_t)PP_R0 * S + k] = T(0); od.dyn[(size_t)PP_R1 * S + k] = T(0);
                        od.dyn[(size_t)PP_KAPPA * S + k] = o.a[2];
                    } else { od.dyn[k] = o.a[0]; od.dyn[S + k] = o.a[1]; od.dyn[2 * S + k] = o.a[2]; }
                    od0 += o.a[0]; od1 += o.a[1]; od2 += o.a[2];
                    const T sg = second ? T(-1) : T(1);
                    og0 += sg * o.a[0] * o.e[0]; og1 += sg * o.a[1] * o.e[1]; og2 += sg * o.a[2] * o.e[2];
                }
                // a padding slot has w = 0: rho = 0 there
                if (!second) chi += o.rho;
            }
        }
#define GS(v) v = group_sum<T, G>(v)
        GS(sA0); GS(sA1); GS(sAv0); GS(sAv1); GS(sVV); GS(ge0); GS(ge1); GS(get);
        GS(K00); GS(K01); GS(K11); GS(Kv0); GS(Kv1); GS(vKv); GS(wu0); GS(wu1); GS(wut);
        GS(od0); GS(od1); GS(od2); GS(og0); GS(og1); GS(og2);
        if (OJ) { GS(od01); GS(od02); GS(od12); }
#undef GS
        if (valid && wk.head) {
            // gauge and damping enter once: through the shard that owns the pose
            const bool own = i >= pose_first && i < pose_last;
            const T ga = own ? gauge_p[i] + lambda : T(0);
            const bool fixed_here = zero_fixed && gauge_p[i] > T(0);      // gauge_p holds the owned poses' terms; others see 0 and the owner's partial decides
            T* o = part + (size_t)i * 18;
            o[0] = c * c * sA0 + s * s * sA1 + od0 + ga; o[1] = c * s * (sA0 - sA1) + od01; o[3] = s * s * sA0 + c * c * sA1 + od1 + ga;
            o[2] = -(c * sAv0 - s * sAv1) + od02; o[4] = -(s * sAv0 + c * sAv1) + od12; o[5] = sVV + od2 + ga;
            o[6] = c * ge0 - s * ge1 + og0; o[7] = s * ge0 + c * ge1 + og1; o[8] = -get + og2;
            if constexpr (PRI != 0) {
                T h00 = 0, h01 = 0, h11 = 0, h22 = 0, b0 = 0, b1 = 0, b2 = 0;
                for (uint32_t k = pa.off[i]; k < pa.off[i + 1]; ++k)
                    chi += pose_prior_fold<T>(pa.rec + (size_t)k * PRI_POSE_REC, x0, y0, c, s, h00, h01, h11, h22, b0, b1, b2,
                                                  robust_at<RK>(ra, robust_class<RK>(ra, kClassPosePrior), ra.pose_prior, k));
                o[0] += h00; o[1] += h01; o[3] += h11; o[5] += h22; o[6] += b0; o[7] += b1; o[8] += b2;
            }
            if (fixed_here) { o[6] = 0; o[7] = 0; o[8] = 0; }
            o[9] = c * c * K00 - 2 * c * s * K01 + s * s * K11;
            o[10] = c * s * (K00 - K11) + (c * c - s * s) * K01;
            o[12] = s * s * K00 + 2 * c * s * K01 + c * c * K11;
            o[11] = -(c * Kv0 - s * Kv1); o[13] = -(s * Kv0 + c * Kv1); o[14] = vKv;
            o[15] = -(c * wu0 - s * wu1); o[16] = -(s * wu0 + c * wu1); o[17] = wut;
        }
    }
    if constexpr (PRI != 0) {
        if (blockIdx.x == 0) for (int k = threadIdx.x; k < pa.n_lm_chi; k += kBlock) chi += pa.lm_chi[k];
    }
    const T total = block_sum<T>(chi, red);
    if (threadIdx.x == 0) chi_part[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------
// K3 pose_finalize: per pose (thread = pose) — M = Dp - Sd (gauge already inside Dp), M^-1, reduced
// right-hand side, CG start (x = p = q = 0, r = b~, z = M^-1 r) and gamma_0 partials.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pose_finalize(int P, const T* __restrict__ part, const T* __restrict__ ps,
                                                          T* __restrict__ dp, T* __restrict__ minv, T* __restrict__ r,
                                                          T* __restrict__ p, T* __restrict__ q, T* __restrict__ x,
                                                          T* __restrict__ zc, T* __restrict__ gpart,
                                                          CgState<T>* __restrict__ st0, const T* __restrict__ omega_ptr,
                                                          T* __restrict__ gamma0_scale, float* __restrict__ zc32) {
    __shared__ T red[kWavesPerBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T g = 0;
    if (i < P) {
        const T* o = part + (size_t)i * 18;
        T m[6], mi[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { dp[(size_t)i * 6 + k] = o[k]; m[k] = o[k] - o[9 + k]; }
        inv_sym3<T>(m, mi);
#pragma unroll
        for (int k = 0; k < 6; ++k) minv[(size_t)i * 6 + k] = mi[k];
        const T r0 = o[6] - o[15], r1 = o[7] - o[16], r2 = o[8] - o[17];
        T z0, z1, z2;
        sym3_mul<T>(mi, r0, r1, r2, z0, z1, z2);
        r[(size_t)i * 3] = r0; r[(size_t)i * 3 + 1] = r1; r[(size_t)i * 3 + 2] = r2;
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[(size_t)i * 3 + k] = 0; q[(size_t)i * 3 + k] = 0; x[(size_t)i * 3 + k] = 0; }
        T* zr = zc + (size_t)i * kPoseRec;
        const T w = *omega_ptr;    // 1 for block-Jacobi PCG; the level-0 smoother damping under the multigrid cycle
        zr[0] = w * z0; zr[1] = w * z1; zr[2] = w * z2; zr[3] = ps[(size_t)i * 4 + 2]; zr[4] = ps[(size_t)i * 4 + 3];
        if (zc32) {     // f32 copy of the record for the products inside the multigrid cycle (k_schur_lm / k_schur_pose, LOW)
            float* zq = zc32 + (size_t)i * kPoseRec;
            *reinterpret_cast<float4*>(zq) = make_float4((float)(w * z0), (float)(w * z1), (float)(w * z2), (float)zr[3]);
            zq[4] = (float)zr[4];
        }
        g = r0 * z0 + r1 * z1 + r2 * z2;
    }
    const T total = block_sum<T>(g, red);
    if (threadIdx.x == 0) gpart[blockIdx.x] = total;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        CgState<T> s; s.gamma_old = 0; s.alpha_old = 0; s.gamma0 = 0; s.pad = 0; s.iters = 0; s.done = 0; s.fail = 0; s.pad2 = 0;
        *st0 = s;
        *gamma0_scale = 1;       // cold start; the warm-start kernels overwrite it
    }
}

// ------------------------------------------------------------------------------------------------
// KA schur_lm: per landmark — t = Dl^-1 W^T v, v being the vector held in zc[.][0..2].
//   MODE 0: write t.   MODE 1 (back-substitution): dl = u - t, landmark += step * dl, |dl|^2 partial.
//   MODE 2 (the back-substitution of a rules = 2 trial): MODE 1, and the landmarks' share of the predicted decrease, g_l^T dl + lambda |dl|^2
//   with g_l = D_l u recovered from the inverse block already in registers, one partial per workgroup into pred_part.
// HOT KERNEL 1 of the PCG iteration.
template <typename T, int G, int MODE, int LOW = 0>
__global__ __launch_bounds__(kBlock) void k_schur_lm(const uint32_t* __restrict__ row_off, int n_slices, int n_vertices, int xcd8, int gate_n,
                                                     CgState<T>* st, const T* __restrict__ ninv, const T* __restrict__ gate_rdr,
                                                     const T* __restrict__ gate_b, Table<T> tb, const T* __restrict__ zc,
                                                     T* __restrict__ lmrec, T* __restrict__ t, T step, T* __restrict__ dl_out, T* __restrict__ norm_part,
                                                     const float* __restrict__ zc32 = nullptr, float* __restrict__ t32 = nullptr,
                                                     const GateArgs<T> gate = GateArgs<T>{nullptr, nullptr, nullptr, 0, T(0), nullptr, 0},
                                                     T lambda = T(0), T* __restrict__ pred_part = nullptr) {
    __shared__ T red[2 * kWavesPerBlock];
    __shared__ int verdict;
    // The iteration's stopping rule rides in workgroup 0 of its first product (gate_n > 0; the state it judges and sets is st, its
    // partials gate_rdr / gate_b, the rest of GateArgs in `gate`): one launch fewer per iteration.  st is neither const nor __restrict__:
    // workgroup 0 writes st->done in the very launch whose other workgroups read it.  Workgroup 0 hands the verdict to all of its waves
    // through LDS: in the launch that finds the solve converged, ALL of workgroup 0 now leaves early (before, its waves read the flag each
    // for itself and most computed their slices for nothing).  The other workgroups do not wait for the verdict: they read the flag with a
    // relaxed atomic load and may see the value of before or after the gate; both are tolerated: a solve that has just converged runs this
    // one pass for nothing (its output is scratch: nothing reads t once st->done is set) or skips it, and every later kernel of the
    // iteration sees st->done.
    // the flag of a finished solve is requested here and tested after the loads that depend on the arguments alone (row bounds,
    // the vertex's inverse block) are on their way: tested first, it adds a scalar round trip in front of the first vector load
    int done = 0;
    if (MODE == 0 && gate_n > 0 && blockIdx.x == 0) {
        const int d = iter_gate_body<T>(GateArgs<T>{st, gate_rdr, gate_b, gate_n, gate.tol2, gate.host_flag, gate.seq}, red);
        if (threadIdx.x == 0) verdict = d;
        __syncthreads();
        done = __builtin_amdgcn_readfirstlane(verdict);
    } else if (MODE == 0) done = __hip_atomic_load(&st->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const Walk wk = walk_of<G>(n_slices, xcd8);
    const int slice = wk.slice, lane = wk.lane, l = wk.vertex;
    T nrm = 0, prd = 0;
    if (wk.live) {
        T acc0 = 0, acc1 = 0;
        uint32_t r0 = row_off[slice];
        const uint32_t r1 = row_off[slice + 1];
        // the inverse block this vertex needs at the very end is requested first: its latency hides behind the rows
        const int lq = (l < n_vertices) ? l : n_vertices - 1;
        const auto n01 = ld2<T>(ninv + (size_t)lq * kNinvRec);
        T n2 = ninv[(size_t)lq * kNinvRec + 2];
        issue_before_exit(r0);      // (the row bounds too: with the flag's request at the very top, the compiler otherwise sinks them below the test)
        issue_before_exit(n2);
        if (done) return;
        // UB rows are walked at a time with every load of the batch issued before any use: a wave's time is
        // the depth of its dependent-load chain (row -> index -> gathered pose record), so memory-level
        // parallelism is what buys time.  Rows past the end are clamped (in bounds) and masked out of the sums.
        constexpr int UB = (G >= 4) ? 2 : 4;
        for (uint32_t base = r0; base < r1; base += UB) {
            uint32_t i[UB]; LmSlot<T> d[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const uint32_t row = min(base + u, r1 - 1);
                const size_t k = (size_t)row * 64 + lane;
                i[u] = tb.idx[k];
                d[u] = lm_slot<T, LOW>(tb, k);
            }
            PoseVec<T> z[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) z[u] = pose_vec<T, LOW>(zc, zc32, i[u]);
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                if (base + u < r1) {
                    const T c = z[u].c, s = z[u].s;
                    const T vt0 = c * z[u].v0 + s * z[u].v1, vt1 = c * z[u].v1 - s * z[u].v0;
                    const T m0 = d[u].a0 * (d[u].ppy * z[u].v2 - vt0), m1 = d[u].a1 * (-vt1 - d[u].ppx * z[u].v2);
                    acc0 += c * m0 - s * m1; acc1 += s * m0 + c * m1;
                }
            }
        }
        acc0 = group_sum<T, G>(acc0); acc1 = group_sum<T, G>(acc1);
        if (l < n_vertices && wk.head) {
            T* lr = lmrec + (size_t)l * kLmRec;
            const T ixx = n01.x, ixy = n01.y, iyy = n2;
            const T t0 = ixx * acc0 + ixy * acc1, t1 = ixy * acc0 + iyy * acc1;
            if (MODE == 0) {
                if (LOW) *reinterpret_cast<float2*>(t32 + (size_t)l * 2) = make_float2((float)t0, (float)t1);
                else { t[(size_t)l * 2] = t0; t[(size_t)l * 2 + 1] = t1; }
            }
            else {
                const T u0 = lr[5], u1 = lr[6];
                const T d0 = u0 - t0, d1 = u1 - t1;
                dl_out[(size_t)l * 2] = d0; dl_out[(size_t)l * 2 + 1] = d1;
                lr[0] += step * d0; lr[1] += step * d1;
                nrm = d0 * d0 + d1 * d1;
                if (MODE == 2) {
                    T dxx, dxy, dyy;
                    inv_sym2<T>(ixx, ixy, iyy, dxx, dxy, dyy);      // D_l (damping and gauge inside); a landmark without edges has 0 and d = 0
                    const T g0 = dxx * u0 + dxy * u1, g1 = dxy * u0 + dyy * u1;
                    prd = g0 * d0 + g1 * d1 + lambda * nrm;
                }
            }
        }
    }
    else if (done) return;
    if (MODE != 0) {
        const T total = block_sum<T>(nrm, red);
        if (threadIdx.x == 0) norm_part[blockIdx.x] = total;
    }
    if (MODE == 2) {
        const T total = block_sum<T>(prd, red);
        if (threadIdx.x == 0) pred_part[blockIdx.x] = total;
    }
}

// ------------------------------------------------------------------------------------------------
// KB schur_pose: per pose — out = Hpp v - W t (this shard's share), partial dot (out, v).
// HOT KERNEL 2 of the PCG iteration.
template <typename T, int G, int LOW = 0, int OJ = 0>
__global__ __launch_bounds__(kBlock) void k_schur_pose(const uint32_t* __restrict__ row_off, int n_slices, int n_vertices, int xcd8,
                                                       const CgState<T>* __restrict__ st, const T* __restrict__ zc,
                                                       const float* __restrict__ zc32, const uint32_t* __restrict__ od_row_off,
                                                       Table<T> tb, Table<T> od, const T* __restrict__ t, const T* __restrict__ dp,
                                                       int pose_first, int pose_last, T* __restrict__ out,
                                                       T* __restrict__ dot_part, const T* __restrict__ rvec, T* __restrict__ rz_part,
                                                       const float* __restrict__ t32 = nullptr,
                                                       const T* __restrict__ post_minv = nullptr, const T* __restrict__ post_r = nullptr,
                                                       const T* __restrict__ post_omega = nullptr, T* __restrict__ zc_post = nullptr) {
    __shared__ T red[2 * kWavesPerBlock];
    // post_minv (the SECOND product inside a multigrid cycle, one shard, f32-copy operands): the level-0 post-smoothing
    // zc_i += omega Minv_i (r_i - (S z)_i) in this kernel's epilogue instead of a launch of its own (k_smooth0<1>).  The pass gathers
    // its operands from the f32 copies (zc32), so writing the f64 records it does not read is no race; the f32 copies are rewritten by
    // k_cg_step before anything reads them again.
    const int done = st->done;      // requested now, tested after the first argument-only loads are in flight (see k_schur_lm)
    const Walk wk = walk_of<G>(n_slices, xcd8);
    const int slice = wk.slice, lane = wk.lane, i = wk.vertex, live = wk.live;
    T dot = 0, rz = 0;
    if (!live && done) return;      // workgroup-uniform: done is, and the other waves of the group leave below
    if (live) {
        const bool valid = i < n_vertices;
        const int ic = valid ? i : n_vertices - 1;
        const PoseVec<T> zi = pose_vec<T, LOW>(zc, zc32, ic);
        T v0 = zi.v0, v1 = zi.v1, v2 = zi.v2, c = zi.c, s = zi.s;
        uint32_t lm_r0 = row_off[slice];
        const uint32_t lm_r1 = row_off[slice + 1];
        issue_before_exit(lm_r0);      // (the row bounds too, as in k_schur_lm)
        issue_before_exit(v0);
        if (done) return;
        // the pose's own diagonal block and residual entry are used at the very end: asked for first
        const bool head = valid && wk.head;
        const bool own = head && i >= pose_first && i < pose_last;
        T dpi[6] = {0, 0, 0, 0, 0, 0}, rv0 = 0, rv1 = 0, rv2 = 0;
        if (own) {
#pragma unroll
            for (int m = 0; m < 6; ++m) dpi[m] = dp[(size_t)i * 6 + m];
        }
        if (head && rvec) { rv0 = rvec[(size_t)i * 3]; rv1 = rvec[(size_t)i * 3 + 1]; rv2 = rvec[(size_t)i * 3 + 2]; }
        T pm[6] = {0, 0, 0, 0, 0, 0}, pr0 = 0, pr1 = 0, pr2 = 0, pz0 = 0, pz1 = 0, pz2 = 0, pw = 0;      // post-smoothing operands: asked for before the rows are walked
        if (LOW && post_r && head) {      // post_r alone (the FIRST product of a cycle): `out` receives the residual r - S z the restriction wants
            pr0 = post_r[(size_t)i * 3]; pr1 = post_r[(size_t)i * 3 + 1]; pr2 = post_r[(size_t)i * 3 + 2];
            if (post_minv) {
#pragma unroll
                for (int m = 0; m < 6; ++m) pm[m] = post_minv[(size_t)i * 6 + m];
                const T* zr = zc_post + (size_t)i * kPoseRec;
                pz0 = zr[0]; pz1 = zr[1]; pz2 = zr[2]; pw = *post_omega;
            }
        }
        T acc0 = 0, acc1 = 0, acc2 = 0;
        {
            const uint32_t r0 = lm_r0, r1 = lm_r1;
#pragma unroll 2
            for (uint32_t row = r0; row < r1; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t l = tb.idx[k];
                const LmSlot<T> d = lm_slot<T, LOW>(tb, k);
                T tx, ty;
                if (LOW) { const float2 txy = *reinterpret_cast<const float2*>(t32 + (size_t)l * 2); tx = txy.x; ty = txy.y; }
                else { const auto txy = ld2<T>(t + (size_t)l * 2); tx = txy.x; ty = txy.y; }
                const T t0 = d.a0 * (c * tx + s * ty), t1 = d.a1 * (c * ty - s * tx);
                acc0 += t0; acc1 += t1; acc2 += t0 * d.ppy - t1 * d.ppx;
            }
        }
        T o0 = 0, o1 = 0, o2 = 0;
        {
            const size_t S = od.slots;
            const uint32_t r0 = od_row_off[slice], r1 = od_row_off[slice + 1];
            for (uint32_t row = r0; row < r1; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t raw = od.idx[k];
                const uint32_t j = raw & kPoseIdxMask;
                T zj[3];
                if (LOW) { const float* q = zc32 + (size_t)j * kPoseRec; zj[0] = q[0]; zj[1] = q[1]; zj[2] = q[2]; }
                else { const T* q = zc + (size_t)j * kPoseRec; zj[0] = q[0]; zj[1] = q[1]; zj[2] = q[2]; }
                if (OJ) {           // the slot's own row block H_pn = [[-K, c], [r^T, -kappa]] (tsgo_math.h), whatever edge it came from
                    const PairSlot<T> h = pair_slot<T>(od.dyn, S, k);
                    pair_apply<T>(h.v, zj[0], zj[1], zj[2], o0, o1, o2);
                } else { o0 -= od.dyn[k] * zj[0]; o1 -= od.dyn[S + k] * zj[1]; o2 -= od.dyn[2 * S + k] * zj[2]; }
            }
        }
        acc0 = group_sum<T, G>(acc0); acc1 = group_sum<T, G>(acc1); acc2 = group_sum<T, G>(acc2);
        o0 = group_sum<T, G>(o0); o1 = group_sum<T, G>(o1); o2 = group_sum<T, G>(o2);
        if (head) {
            o0 += c * acc0 - s * acc1; o1 += s * acc0 + c * acc1; o2 -= acc2;
            if (own) {
                T d0, d1, d2;
                sym3_mul<T>(dpi, v0, v1, v2, d0, d1, d2);
                o0 += d0; o1 += d1; o2 += d2;
            }
            if (LOW && post_r && !post_minv) { out[(size_t)i * 3] = pr0 - o0; out[(size_t)i * 3 + 1] = pr1 - o1; out[(size_t)i * 3 + 2] = pr2 - o2; }
            else { out[(size_t)i * 3] = o0; out[(size_t)i * 3 + 1] = o1; out[(size_t)i * 3 + 2] = o2; }
            dot = o0 * v0 + o1 * v1 + o2 * v2;
            if (rvec) rz = rv0 * v0 + rv1 * v1 + rv2 * v2;
            if (LOW && post_minv) {      // k_smooth0<1>: zc += omega Minv (r - S zc)
                T z0, z1, z2;
                sym3_mul<T>(pm, pr0 - o0, pr1 - o1, pr2 - o2, z0, z1, z2);
                T* zr = zc_post + (size_t)i * kPoseRec;
                zr[0] = pz0 + pw * z0; zr[1] = pz1 + pw * z1; zr[2] = pz2 + pw * z2;
            }
        }
    }
    if (rvec) {        // wave-uniform: a kernel argument.  The PCG product: (S z, z) and (r, z) in one reduction
        block_sum2<T>(dot, rz, red);
        if (threadIdx.x == 0) { dot_part[blockIdx.x] = dot; rz_part[blockIdx.x] = rz; }
    } else {
        const T total = block_sum<T>(dot, red);
        if (threadIdx.x == 0) dot_part[blockIdx.x] = total;
    }
}

// ------------------------------------------------------------------------------------------------
// KC cg_update: per pose — the vector half of a Chronopoulos-Gear PCG iteration (one global
// reduction point per iteration instead of two).  Every workgroup first sums the partials of
// delta = (S z, z) (from KB) and gamma = (r, z) (from the previous KC / pose_finalize) in a fixed
// order, then:  beta = gamma/gamma_old, alpha = gamma/(delta - beta*gamma/alpha_old),
//   p = z + beta p,  q = S z + beta q,  x += alpha p,  r -= alpha q,  z = M^-1 r.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_cg_update(int P, int n_dot, const CgState<T>* __restrict__ st_in, const T* __restrict__ dot_part,
                                                      const T* __restrict__ gpart_in, int n_g, const T* __restrict__ sz,
                                                      T* __restrict__ gpart_out, CgState<T>* __restrict__ st_out, const T* __restrict__ minv,
                                                      T* __restrict__ r, T* __restrict__ p, T* __restrict__ q,
                                                      T* __restrict__ x, T* __restrict__ zc, T tol2, int max_iters,
                                                      const T* __restrict__ gamma0_scale) {
    __shared__ T red[kWavesPerBlock];
    const CgState<T> s = *st_in;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (s.done) { if (writer) *st_out = s; return; }
    const T delta = block_sum_array<T>(dot_part, n_dot, red);
    const T gamma = block_sum_array<T>(gpart_in, n_g, red);
    // warm-started solves measure convergence against the right-hand side, not against the (already small) first residual
    const T gamma0 = s.iters == 0 ? gamma * (*gamma0_scale) : s.gamma0;
    CgState<T> n = s; n.gamma0 = gamma0;
    if (!(gamma > tol2 * gamma0) || s.iters >= max_iters) {      // converged (or cap, or NaN): x is final
        n.done = 1; n.fail = (gamma != gamma) ? 1 : ((gamma > tol2 * gamma0) ? 2 : 0);
        if (writer) *st_out = n;
        return;
    }
    T beta, alpha;
    if (s.iters == 0) { beta = 0; alpha = gamma / delta; }
    else { beta = gamma / s.gamma_old; alpha = gamma / (delta - beta * gamma / s.alpha_old); }
    if (!(alpha > 0) || !(alpha < T(1e300))) {                    // breakdown: keep x, flag it
        n.done = 1; n.fail = 1;
        if (writer) *st_out = n;
        return;
    }
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T g = 0;
    if (i < P) {
        T rr[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t j = (size_t)i * 3 + k;
            const T zk = zc[(size_t)i * kPoseRec + k];
            const T pk = zk + beta * p[j];
            const T qk = sz[j] + beta * q[j];
            p[j] = pk; q[j] = qk;
            x[j] += alpha * pk;
            rr[k] = r[j] - alpha * qk;
            r[j] = rr[k];
        }
        T z0, z1, z2;
        sym3_mul<T>(minv + (size_t)i * 6, rr[0], rr[1], rr[2], z0, z1, z2);
        T* zr = zc + (size_t)i * kPoseRec;
        zr[0] = z0; zr[1] = z1; zr[2] = z2;
        g = rr[0] * z0 + rr[1] * z1 + rr[2] * z2;
    }
    const T total = block_sum<T>(g, red);
    if (threadIdx.x == 0) gpart_out[blockIdx.x] = total;
    if (writer) { n.gamma_old = gamma; n.alpha_old = alpha; n.iters = s.iters + 1; *st_out = n; }
}

// Warm start, first half.  d_k / a^k (a = 1 - step: what a damped step leaves of its delta) is smooth in k, so the next delta is
// predicted by continuing the polynomial of degree m - 1 through the last m deltas: x0 = sum_j c[m-1][j] v[j],
// c[m-1][j] = (-1)^j C(m, j+1) a^(j+1).  Which order m: the one that would have predicted the LAST delta best from the
// deltas before it — k_save_x leaves ||d - prediction_m||^2 for every order it could test in errpart[m-1][block].
constexpr int kMaxWarm = 6;      // deltas of earlier Gauss-Newton iterations the warm start can combine
constexpr int kWarmMargin = 4;   // a higher order is taken when its squared prediction error is this many times smaller: its coefficients
                                 // (order 4 at step 0.2: 3.2, -3.8, 2.0, -0.4) amplify whatever in the deltas is not a smooth trend
template <typename T> struct WarmTerms {
    const T* v[kMaxWarm];          // deltas, newest first
    T c[kMaxWarm][kMaxWarm];       // row m-1: the coefficients of order m
    int n_max;                     // highest order allowed (0: no warm start — plain copy)
    int n_tested;                  // orders 1..n_tested have an error in errpart
    const T* errpart; int nb_err;  // [kMaxWarm][nb_err]
};

// x -> zc[.][0..2] (the landmark pass reads its vector from zc).  w.n_max = 0: plain copy of x into zc.  Otherwise x = the
// prediction of the order with the smallest tested error (order 1 when nothing has been tested yet) first.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pack_x(int P, int n_max, int n_tested, int nb_err, const T* __restrict__ errpart, T* __restrict__ x,
                                                   T* __restrict__ zc, int* __restrict__ order_out, const WarmTerms<T> w) {
    // (n_max, n_tested, nb_err, errpart: w's, in the plain head; read from there alone)
    __shared__ T red[kWavesPerBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int m = n_max > 0 ? 1 : 0;
    if (n_max > 0 && n_tested > 0) {          // every workgroup sums the same partials in the same order: one choice
        T best = block_sum_array<T>(errpart, nb_err, red);
        for (int j = 1; j < n_tested && j < n_max; ++j) {
            const T e = block_sum_array<T>(errpart + (size_t)j * nb_err, nb_err, red);
            if (e * kWarmMargin < best) { best = e; m = j + 1; }
        }
    }
    if (order_out && blockIdx.x == 0 && threadIdx.x == 0) *order_out = m;
    if (i >= P) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T v = x[(size_t)i * 3 + k];
        if (m > 0) {
            v = w.c[m - 1][0] * w.v[0][(size_t)i * 3 + k];
            for (int j = 1; j < m; ++j) v += w.c[m - 1][j] * w.v[j][(size_t)i * 3 + k];
            x[(size_t)i * 3 + k] = v;
        }
        zc[(size_t)i * kPoseRec + k] = v;
    }
}

// The solved delta x -> zc[.][0..2] and -> xsave (the newest entry of the warm start's history), and what every order would
// have made of predicting it from the deltas before it (w.v, newest first; orders 1..w.n_max): errpart[m-1][block].
template <typename T>
__device__ __forceinline__ void save_x_body(int P, int n_max, const T* __restrict__ x, T* __restrict__ zc, T* __restrict__ xsave, T* __restrict__ errpart, const WarmTerms<T>& w, T* red) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T err[kMaxWarm];
#pragma unroll
    for (int m = 0; m < kMaxWarm; ++m) err[m] = 0;
    if (i < P) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T v = x[(size_t)i * 3 + k];
            zc[(size_t)i * kPoseRec + k] = v;
            xsave[(size_t)i * 3 + k] = v;
            T u[kMaxWarm];
#pragma unroll
            for (int j = 0; j < kMaxWarm; ++j) u[j] = j < n_max ? w.v[j][(size_t)i * 3 + k] : T(0);
#pragma unroll
            for (int m = 0; m < kMaxWarm; ++m) {
                if (m < n_max) {
                    T p = 0;
#pragma unroll
                    for (int j = 0; j <= m; ++j) p += w.c[m][j] * u[j];
                    err[m] += (v - p) * (v - p);
                }
            }
        }
    }
    for (int m = 0; m < n_max; ++m) {
        const T total = block_sum<T>(err[m], red);
        if (threadIdx.x == 0) errpart[(size_t)m * gridDim.x + blockIdx.x] = total;
    }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_save_x(int P, int n_max, const T* __restrict__ x, T* __restrict__ zc, T* __restrict__ xsave, T* __restrict__ errpart, const WarmTerms<T> w) {      // (n_max: w's, in the plain head; read from there alone)
    __shared__ T red[kWavesPerBlock];
    save_x_body<T>(P, n_max, x, zc, xsave, errpart, w, red);
}

// History across requests (tsgo_config.warm_requests): a delta of the previous graph, in ITS pose numbering, into this graph's —
// src[i] = the old index of pose i, or -1 for a pose the old graph did not hold.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_gather_hist(int P, const int* __restrict__ src, const T* __restrict__ old, T* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    const int j = src[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = j >= 0 ? old[(size_t)j * 3 + k] : T(0);
}

// Warm start, second half: r = b~ - S x0 (S x0 in sx), zc = omega Minv r, partials of r^T Minv r.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_warm_residual(int P, const T* __restrict__ sx, const T* __restrict__ minv, T* __restrict__ r,
                                                          T* __restrict__ zc, const T* __restrict__ omega_ptr, T* __restrict__ part, float* __restrict__ zc32) {
    __shared__ T red[kWavesPerBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T g = 0;
    if (i < P) {
        const T r0 = r[(size_t)i * 3] - sx[(size_t)i * 3], r1 = r[(size_t)i * 3 + 1] - sx[(size_t)i * 3 + 1], r2 = r[(size_t)i * 3 + 2] - sx[(size_t)i * 3 + 2];
        r[(size_t)i * 3] = r0; r[(size_t)i * 3 + 1] = r1; r[(size_t)i * 3 + 2] = r2;
        T z0, z1, z2;
        sym3_mul<T>(minv + (size_t)i * 6, r0, r1, r2, z0, z1, z2);
        const T w = *omega_ptr;
        T* zr = zc + (size_t)i * kPoseRec;
        zr[0] = w * z0; zr[1] = w * z1; zr[2] = w * z2;
        if (zc32) { float* zq = zc32 + (size_t)i * kPoseRec; zq[0] = (float)(w * z0); zq[1] = (float)(w * z1); zq[2] = (float)(w * z2); }
        g = r0 * z0 + r1 * z1 + r2 * z2;
    }
    const T total = block_sum<T>(g, red);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// scale = max(1, (b^T D^-1 b) / (r0^T D^-1 r0)) from the two partial arrays; one workgroup.
// st0 (multigrid PCG, whose stopping rule is r^T D^-1 r <= tol^2 b^T D^-1 b, k_cg_step): a warm start that already meets the
// rule ends the solve before its first iteration.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_warm_scale(int n, const T* b_part, const T* __restrict__ r_part, T* gpart_out, T* __restrict__ scale,
                                                       CgState<T>* __restrict__ st0, T tol2) {
    __shared__ T red[kWavesPerBlock];
    const T nb = block_sum_array<T>(b_part, n, red);
    const T nr = block_sum_array<T>(r_part, n, red);
    // block-Jacobi PCG reads gamma = r^T Minv r from gpart: hand it the warm-started value
    if (gpart_out) for (int k = threadIdx.x; k < n; k += kBlock) gpart_out[k] = r_part[k];
    if (threadIdx.x == 0) {
        *scale = (nr > T(0) && nb > nr) ? nb / nr : T(1);
        if (st0 && !(nr > tol2 * nb)) st0->done = 1;
    }
}

// pose (+)= step * delta: VertexSe2::Update (remote/graph/vertex/VertexSe2.h:16-27) with the 0.2 of
// OptimizerCpu.h:164 — theta = atan2(sin, cos) + step*dth, translation added in the world frame.
template <typename T>
__device__ __forceinline__ void pose_update_body(int P, const T* __restrict__ x, T* __restrict__ ps, T* __restrict__ theta, T step, T* __restrict__ norm_part, T* red) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T nrm = 0;
    if (i < P) {
        const T d0 = x[(size_t)i * 3], d1 = x[(size_t)i * 3 + 1], d2 = x[(size_t)i * 3 + 2];
        nrm = d0 * d0 + d1 * d1 + d2 * d2;
        if (step != T(0)) {
            T* q = ps + (size_t)i * 4;
            const T th = atan2(q[3], q[2]) + step * d2;
            q[0] += step * d0; q[1] += step * d1; q[2] = cos(th); q[3] = sin(th);
            theta[i] = th;
        }
    }
    const T total = block_sum<T>(nrm, red);
    if (threadIdx.x == 0) norm_part[blockIdx.x] = total;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pose_update(int P, const T* __restrict__ x, T* __restrict__ ps,
                                                        T* __restrict__ theta, T step, T* __restrict__ norm_part) {
    __shared__ T red[kWavesPerBlock];
    pose_update_body<T>(P, x, ps, theta, step, norm_part, red);
}

// k_save_x and k_pose_update in one launch (one-shard handles, a step that is taken): both are thread = pose over the same grid and read the
// same x, and the landmark back-substitution that used to run between them reads zc and lmrec, neither ps nor theta.  The two bodies are
// the two kernels' own, one after the other: every partial keeps its slot and its bits.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_save_update(int P, int n_max, const T* __restrict__ x, T* __restrict__ zc, T* __restrict__ xsave, T* __restrict__ errpart,
                                                        T* __restrict__ ps, T* __restrict__ theta, T step, T* __restrict__ norm_part, const WarmTerms<T> w) {
    __shared__ T red[kWavesPerBlock];
    save_x_body<T>(P, n_max, x, zc, xsave, errpart, w, red);
    pose_update_body<T>(P, x, ps, theta, step, norm_part, red);
}

// Step report (Engine::launch_report / wait_report; not the per-edge report, whose launcher is launch_edge_report): ONE workgroup
// copies n partials into pinned host memory with plain coalesced stores, fences at system scope, and one lane then publishes the report's 64-bit sequence number with a system-scope release store,
// the form in which iter_gate_body publishes a gate.  The host thread polls the word and then sums the partials in the order it
// always did.  The kernel waits for nothing.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_report(int n, const T* __restrict__ src, T* __restrict__ host_dst, unsigned long long* host_word, unsigned long long seq) {
    for (int k = threadIdx.x; k < n; k += kBlock) host_dst[k] = src[k];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(host_word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace tsgo
