// Offset pairs of the decoder's training forward (reference decoder.py:62-83) without the (B, M, N) distance matrix:
// every (batch, src, dst) with dist2(src, dst) <= eps^2 between unpadded tokens, listed as torch.nonzero lists them
// ((batch, src, dst) lexicographic), the feature rows of the listed pairs, and the sum of gradient rows back per token.
//   op_count_kernel    one thread per a row walks the b points through LDS: the row's number of pairs
//   op_scan_kernel     exclusive scan of the counts (one workgroup, each thread a contiguous chunk), total last
//   op_fill_kernel     the same walk again, writing (batch, a, b) from the row's offset on: ascending b inside a row
//   op_gather_kernel   out[k] = x[batch_k * rows + index_k]
//   op_segment_sum_kernel  out[r] = sum of g[perm[k]] for k in [offsets[r], offsets[r + 1]), in that order: one workgroup per
//                      token row, one thread per column -- many pairs share a token, and the order of their sum is fixed
//                      (the src side: consecutive pairs; the dst side: the pairs stably sorted by dst row), no float atomics
// dist2 = (dx dx + dy dy) + dz dz in fp32, one rounding per operation (the library is compiled with -ffp-contract=off), the
// arithmetic of reg_loss.hip's rl_pairs_kernel and of torch.sum(torch.square(a - b), dim=-1) on three elements.
#include "dpm_common.h"

namespace {

constexpr int OP_T = 256;

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// FILL = false: counts[b, r]; FILL = true: triples from offsets[b, r] on.  Padded rows list nothing, padded b points are skipped.
template <bool FILL>
__global__ __launch_bounds__(OP_T) void op_walk_kernel(const float *__restrict__ xa, const float *__restrict__ xb,
                                                       const uint8_t *__restrict__ pad_a, const uint8_t *__restrict__ pad_b, int M,
                                                       int N, float eps2, int32_t *__restrict__ counts,
                                                       const int32_t *__restrict__ offsets, int32_t *__restrict__ triples) {
    __shared__ float cb[3][OP_T];
    __shared__ uint8_t cp[OP_T];
    const int b = blockIdx.y, r = blockIdx.x * OP_T + threadIdx.x, rr = min(r, M - 1);
    const float *pa = xa + (size_t)b * 3 * M, *pb = xb + (size_t)b * 3 * N;
    const float ax = pa[rr], ay = pa[M + rr], az = pa[2 * M + rr];
    const bool row = r < M && !pad_a[(size_t)b * M + rr];
    int n = 0;
    int32_t *dst = nullptr;
    if (FILL && row) dst = triples + 3 * (size_t)offsets[(size_t)b * M + r];
    for (int c0 = 0; c0 < N; c0 += OP_T) {
        __syncthreads();
        const int c = c0 + threadIdx.x;
        if (c < N) {
            cb[0][threadIdx.x] = pb[c], cb[1][threadIdx.x] = pb[N + c], cb[2][threadIdx.x] = pb[2 * N + c];
            cp[threadIdx.x] = pad_b[(size_t)b * N + c];
        }
        __syncthreads();
        if (!row) continue;
        const int lim = min(OP_T, N - c0);
        for (int k = 0; k < lim; ++k) {
            if (cp[k] || !(dist2(ax, ay, az, cb[0][k], cb[1][k], cb[2][k]) <= eps2)) continue;
            if (FILL) dst[3 * n] = b, dst[3 * n + 1] = r, dst[3 * n + 2] = c0 + k;
            ++n;
        }
    }
    if (!FILL && r < M) counts[(size_t)b * M + r] = n;
}

// offsets[0..R]: exclusive scan of counts[0..R), offsets[R] = the total, or -1 where it does not fit an int32
__global__ __launch_bounds__(OP_T) void op_scan_kernel(const int32_t *__restrict__ counts, long long R, int32_t *__restrict__ offsets) {
    __shared__ long long part[OP_T];
    const int t = threadIdx.x;
    const long long chunk = (R + OP_T - 1) / OP_T, r0 = min(R, t * chunk), r1 = min(R, r0 + chunk);
    long long s = 0;
    for (long long r = r0; r < r1; ++r) s += counts[r];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int k = 0; k < OP_T; ++k) {
            const long long v = part[k];
            part[k] = run;
            run += v;
        }
        offsets[R] = run > 0x7fffffffLL ? -1 : (int32_t)run;
    }
    __syncthreads();
    long long run = part[t];
    for (long long r = r0; r < r1; ++r) {
        offsets[r] = (int32_t)min(run, 0x7fffffffLL);
        run += counts[r];
    }
}

__global__ __launch_bounds__(OP_T) void op_gather_kernel(const float *__restrict__ x, int ldx, const int32_t *__restrict__ triples,
                                                         int col, int rows, long long K, int E4, float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * OP_T + threadIdx.x;
    if (e >= K * E4) return;
    const long long k = e / E4;
    const int c = (int)(e - k * E4);
    const size_t r = (size_t)triples[3 * k] * rows + triples[3 * k + col];
    reinterpret_cast<float4 *>(out)[e] = *reinterpret_cast<const float4 *>(x + r * ldx + 4 * c);
}

__global__ __launch_bounds__(OP_T) void op_segment_sum_kernel(const float *__restrict__ g, int ldg, const int32_t *__restrict__ offsets,
                                                              const int32_t *__restrict__ perm, int E, float *__restrict__ out) {
    const size_t r = blockIdx.x;
    const int k0 = offsets[r], k1 = offsets[r + 1];
    for (int c = threadIdx.x; c < E; c += OP_T) {
        float acc = 0.f;
        for (int k = k0; k < k1; ++k) acc += g[(size_t)(perm ? perm[k] : k) * ldg + c];
        out[r * E + c] = acc;
    }
}

bool shape_ok(int B, int M, int N) { return B >= 1 && M >= 1 && N >= 1 && B <= 65535 && (long long)B * M < 0x7fffffffLL; }

}  // namespace

extern "C" int dpm_offset_pairs_count(const float *xyz_a, const float *xyz_b, const uint8_t *pad_a, const uint8_t *pad_b, int B,
                                      int M, int N, double eps, int32_t *counts, int32_t *offsets, dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz_a && xyz_b && pad_a && pad_b && counts && offsets && shape_ok(B, M, N) && eps >= 0.0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(op_walk_kernel<false>, dim3(dpm_cdiv(M, OP_T), B), dim3(OP_T), 0, st, xyz_a, xyz_b, pad_a, pad_b, M, N,
                       (float)(eps * eps), counts, (const int32_t *)nullptr, (int32_t *)nullptr);
    hipLaunchKernelGGL(op_scan_kernel, dim3(1), dim3(OP_T), 0, st, counts, (long long)B * M, offsets);
    return dpm_launch_status();
}

extern "C" int dpm_offset_pairs_fill(const float *xyz_a, const float *xyz_b, const uint8_t *pad_a, const uint8_t *pad_b, int B,
                                     int M, int N, double eps, const int32_t *offsets, int32_t *triples, dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz_a && xyz_b && pad_a && pad_b && offsets && triples && shape_ok(B, M, N) && eps >= 0.0);
    hipLaunchKernelGGL(op_walk_kernel<true>, dim3(dpm_cdiv(M, OP_T), B), dim3(OP_T), 0, (hipStream_t)stream, xyz_a, xyz_b, pad_a,
                       pad_b, M, N, (float)(eps * eps), (int32_t *)nullptr, offsets, triples);
    return dpm_launch_status();
}

extern "C" int dpm_offset_pairs_gather(const float *x, int ldx, const int32_t *triples, int side, int rows, long long K, int E,
                                       float *out, dpm_stream_t stream) {
    DPM_CHECK_ARG(K >= 0 && rows >= 1 && E >= 4 && E % 4 == 0 && ldx >= E && ldx % 4 == 0 && (side == 0 || side == 1));
    if (K == 0) return DPM_OK;
    DPM_CHECK_ARG(x && triples && out && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 && K * (E / 4) < (1LL << 39));
    hipLaunchKernelGGL(op_gather_kernel, dim3(dpm_cdiv(K * (E / 4), OP_T)), dim3(OP_T), 0, (hipStream_t)stream, x, ldx, triples,
                       1 + side, rows, K, E / 4, out);
    return dpm_launch_status();
}

extern "C" int dpm_offset_pairs_segment_sum(const float *g, int ldg, const int32_t *offsets, const int32_t *perm, long long R, int E,
                                            float *out, dpm_stream_t stream) {
    DPM_CHECK_ARG(offsets && out && R >= 1 && R < 0x7fffffffLL && E >= 1 && ldg >= E);   // g may be NULL when no pair exists
    hipLaunchKernelGGL(op_segment_sum_kernel, dim3((unsigned)R), dim3(OP_T), 0, (hipStream_t)stream, g, ldg, offsets, perm, E, out);
    return dpm_launch_status();
}
