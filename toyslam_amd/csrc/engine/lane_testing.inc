// engine/lane_testing.inc — TSGO_TESTING builds only, included by tsgo_hip.hip at FILE scope (no engine, no graph):
// tsgo_testing_lane_sums (include/tsgo_testing.h) runs the lane sums of tsgo_kernels.h — group_sum<T, G> for every G, wave_sum<T>,
// block_sum2<T> — in ONE workgroup of kBlock threads on caller-given values and hands back what every thread got.
// tests/test_gpu_lane_sums.py compares that, bit for bit, with the xor butterfly written out in numpy: it is the test that settles which
// half of a permlane swap a lane takes and which way row_shl / row_shr move (lane_xor).
namespace {

constexpr int kLaneSumRows = 10;      // group_sum G = 1, 2, 4, 8, 16, 32, 64; wave_sum; block_sum2's two results

template <typename T>
__global__ __launch_bounds__(kBlock) void k_testing_lane_sums(const T* __restrict__ in, T* __restrict__ out) {
    __shared__ T red[2 * kWavesPerBlock];
    const T v = in[threadIdx.x];
    T* o = out + threadIdx.x;
    o[0 * kBlock] = group_sum<T, 1>(v); o[1 * kBlock] = group_sum<T, 2>(v); o[2 * kBlock] = group_sum<T, 4>(v); o[3 * kBlock] = group_sum<T, 8>(v);
    o[4 * kBlock] = group_sum<T, 16>(v); o[5 * kBlock] = group_sum<T, 32>(v); o[6 * kBlock] = group_sum<T, 64>(v);
    o[7 * kBlock] = wave_sum<T>(v);
    T a = v, b = in[kBlock - 1 - threadIdx.x];      // the second value: the same numbers, thread order reversed
    block_sum2<T>(a, b, red);
    o[8 * kBlock] = a; o[9 * kBlock] = b;
}

template <typename T> int lane_sums_run(const T* in, T* out) {
    SymScratch S;
    T *d_in, *d_out;
    if (int rc = S.up(&d_in, in, (size_t)kBlock)) return rc;
    if (int rc = S.get(&d_out, (size_t)kLaneSumRows * kBlock)) return rc;
    hipLaunchKernelGGL((k_testing_lane_sums<T>), dim3(1), dim3(kBlock), 0, nullptr, (const T*)d_in, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(nullptr));
    return sym_down(out, (const T*)d_out, (size_t)kLaneSumRows * kBlock);
}

}  // namespace
