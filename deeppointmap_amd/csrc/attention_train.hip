// Scaled-dot-product attention for training (descriptor_attention.py:14-15, 33-44; head_dim 32, dropout 0,
// key_padding_mask, M != N): a forward that keeps the log-sum-exp of every score row, and a backward that recomputes
// strips of the score matrix from Q, K and that log-sum-exp.  No tensor of M x N elements exists in either direction.
//   at_forward_kernel   one workgroup per (64 queries, head, sequence), 16 queries per wave; key tiles of 64 through LDS;
//                       online softmax; out and lse = m + log(sum)
//   at_delta_kernel     delta[b,h,m] = sum_c dOut[m, h*32 + c] * out[m, h*32 + c]
//   at_dq_kernel        one workgroup per query block, walks the key blocks:   dQ = dS K
//   at_dkv_kernel       one workgroup per key block, walks the query blocks:   dV = P^T dOut, dK = dS^T Q
//                       with P = exp(S - lse), dP = dOut V^T, dS = P (dP - delta) / sqrt(d)
// Two passes, each workgroup the only writer of its rows and each sum in one order: no floating-point atomics, two runs
// give identical bytes.  The score strip is paid twice.
//
// Every product is v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), as in reg_loss.hip: the gradients are
// compared with fp64 at the reference's own fp32 error, and the backward has five products per strip whose operands (P, dS)
// are made in registers -- the bf16x3 form of gemm_b3.hip would split each of them three ways per strip (six term products
// each) on the vector pipe, which is what these kernels are bound by already.
//
// Operand layouts (lane = 16 g + i): A operand A[i][k = g], B operand B[k = g][i], result D[4 g + q][i].  A strip product
// S^T = K Q^T leaves lane (g, i) with query i and keys 16 j + 4 g + q (j = 0..3, q = 0..3): the row statistics of a query
// are two shuffles away, and the SAME registers are the B operand of the next product (P^T against V^T) when its k index
// runs over the keys 16 j + 4 g + q for fixed (j, q) -- P and dS never pass through LDS.
//
// LDS images (ds_read_b32: banks mod 32 per 32-lane half): a tile read as A[row i][k g] has rows 34 floats apart (bank
// 2 i + g: conflict-free), a tile read as A[row 4 g + q][column i] has rows 36 apart (bank 16 g + i: conflict-free); a tile
// read both ways is kept in both images (at most 4 x 64 rows: 35 KB).
#include "dpm_common.h"
#include "workspace.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int AT_T = 256, AT_R = 64, AT_D = 32, AT_LA = 34, AT_LB = 36;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows [0, 64) x 32 floats of src (row stride ld; rows >= valid read as zero) -> the images asked for
__device__ __forceinline__ void stage_tile(const float *__restrict__ src, int ld, int valid, float *imgA, float *imgB) {
    const int t = threadIdx.x, c = (t & 7) * 4;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = p * 32 + (t >> 3);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < valid) v = *reinterpret_cast<const float4 *>(src + (size_t)r * ld + c);
        if (imgA) {
            float2 *d = reinterpret_cast<float2 *>(imgA + r * AT_LA + c);
            d[0] = make_float2(v.x, v.y), d[1] = make_float2(v.z, v.w);
        }
        if (imgB) *reinterpret_cast<float4 *>(imgB + r * AT_LB + c) = v;
    }
}

// the wave's 16 rows as B-operand fragments: f[kk] = row (i)[4 kk + g]
__device__ __forceinline__ void row_fragments(const float *__restrict__ row, float (&f)[8]) {
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) f[kk] = row[kk * 4 + g];
}

// acc[j] = (tile rows 16 j .. 16 j + 15) x fragments: lane (g, i) gets rows 16 j + 4 g + q of column i
__device__ __forceinline__ void strip_product(const float *imgA, const float (&f)[8], f32x4 (&acc)[4]) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) acc[j] = mfma4(imgA[(j * 16 + i) * AT_LA + kk * 4 + g], f[kk], acc[j]);
    }
}

// o[cb] += sum over the tile rows r = 16 j + 4 g + q of imgB[r][16 cb + .] * w[j][q]: lane (g, i) gets columns
// 16 cb + 4 g + q' of the wave's row i
__device__ __forceinline__ void weighted_rows(const float *imgB, const f32x4 (&w)[4], f32x4 (&o)[2]) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float *r = imgB + (j * 16 + g * 4 + q) * AT_LB + i;
            o[0] = mfma4(r[0], w[j][q], o[0]);
            o[1] = mfma4(r[16], w[j][q], o[1]);
        }
}

struct Rows {
    const float *p;
    int ld;
    long long s;
};

__global__ __launch_bounds__(AT_T) void at_forward_kernel(Rows Q, Rows K, Rows V, float *__restrict__ out, int ldo, long long so,
                                                          float *__restrict__ lse, const uint8_t *__restrict__ mask, int M, int N,
                                                          int heads, float scale) {
    __shared__ __attribute__((aligned(16))) float Ka[AT_R * AT_LA], Vb[AT_R * AT_LB];
    __shared__ float kbias[AT_R];
    const int b = blockIdx.z, h = blockIdx.y, row0 = blockIdx.x * AT_R;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
    const float NEG = -__builtin_inff();
    const int qr = row0 + w * 16 + i;
    float qf[8];
    row_fragments(Q.p + (size_t)b * Q.s + (size_t)min(qr, M - 1) * Q.ld + h * AT_D, qf);
    const float *Kh = K.p + (size_t)b * K.s + h * AT_D, *Vh = V.p + (size_t)b * V.s + h * AT_D;
    float m = NEG, s = 0.f;
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 0; k0 < N; k0 += AT_R) {
        __syncthreads();   // the previous tile's readers are done
        stage_tile(Kh + (size_t)k0 * K.ld, K.ld, N - k0, Ka, nullptr);
        stage_tile(Vh + (size_t)k0 * V.ld, V.ld, N - k0, nullptr, Vb);
        if (t < AT_R) kbias[t] = (k0 + t < N && !(mask && mask[(size_t)b * N + k0 + t])) ? 0.f : NEG;
        __syncthreads();
        f32x4 z[4];
        strip_product(Ka, qf, z);
        float tm = NEG;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                z[j][q] = z[j][q] * scale + kbias[j * 16 + g * 4 + q];
                tm = fmaxf(tm, z[j][q]);
            }
        tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        // every key so far padding (mn = -inf): all p are exp(-inf - 0) = 0 and the state stays empty; no branch, the matrix
        // instructions below need the whole wave
        const float mn = fmaxf(m, tm), mref = mn == NEG ? 0.f : mn;
        const float alpha = m == NEG ? 0.f : expf(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                z[j][q] = expf(z[j][q] - mref);
                ps += z[j][q];
            }
        s = s * alpha + ps, m = mn;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) o[c][q] *= alpha;
        weighted_rows(Vb, z, o);
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (qr < M) {
        const float inv = 1.f / s;   // no unmasked key: 0 / 0 = NaN, as the reference
        float *dst = out + (size_t)b * so + (size_t)qr * ldo + h * AT_D + g * 4;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            *reinterpret_cast<float4 *>(dst + c * 16) = make_float4(o[c][0] * inv, o[c][1] * inv, o[c][2] * inv, o[c][3] * inv);
        if (g == 0) lse[((size_t)b * heads + h) * M + qr] = m + logf(s);
    }
}

// one thread per (sequence, head, query): 32 products in channel order
__global__ __launch_bounds__(AT_T) void at_delta_kernel(const float *__restrict__ out, int ldo, long long so,
                                                        const float *__restrict__ dout, int ldd, long long sd, int M, int heads,
                                                        float *__restrict__ delta) {
    const int b = blockIdx.z, h = blockIdx.y, r = blockIdx.x * AT_T + threadIdx.x;
    if (r >= M) return;
    const float4 *a = reinterpret_cast<const float4 *>(out + (size_t)b * so + (size_t)r * ldo + h * AT_D);
    const float4 *d = reinterpret_cast<const float4 *>(dout + (size_t)b * sd + (size_t)r * ldd + h * AT_D);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < AT_D / 4; ++c) {
        const float4 x = a[c], y = d[c];
        acc += x.x * y.x, acc += x.y * y.y, acc += x.z * y.z, acc += x.w * y.w;
    }
    delta[((size_t)b * heads + h) * M + r] = acc;
}

__global__ __launch_bounds__(AT_T) void at_dq_kernel(Rows Q, Rows K, Rows V, Rows dO, const float *__restrict__ lse,
                                                     const float *__restrict__ delta, const uint8_t *__restrict__ mask,
                                                     float *__restrict__ dQ, int M, int N, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) float Ka[AT_R * AT_LA], Kb[AT_R * AT_LB], Va[AT_R * AT_LA];
    __shared__ float kbias[AT_R];
    const int b = blockIdx.z, h = blockIdx.y, row0 = blockIdx.x * AT_R;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
    const float NEG = -__builtin_inff();
    const int qr = row0 + w * 16 + i, qc = min(qr, M - 1);
    float qf[8], df[8];
    row_fragments(Q.p + (size_t)b * Q.s + (size_t)qc * Q.ld + h * AT_D, qf);
    row_fragments(dO.p + (size_t)b * dO.s + (size_t)qc * dO.ld + h * AT_D, df);
    const float l = lse[((size_t)b * heads + h) * M + qc], dl = delta[((size_t)b * heads + h) * M + qc];
    const float *Kh = K.p + (size_t)b * K.s + h * AT_D, *Vh = V.p + (size_t)b * V.s + h * AT_D;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 0; k0 < N; k0 += AT_R) {
        __syncthreads();
        stage_tile(Kh + (size_t)k0 * K.ld, K.ld, N - k0, Ka, Kb);
        stage_tile(Vh + (size_t)k0 * V.ld, V.ld, N - k0, Va, nullptr);
        if (t < AT_R) kbias[t] = (k0 + t < N && !(mask && mask[(size_t)b * N + k0 + t])) ? 0.f : NEG;
        __syncthreads();
        f32x4 z[4], dp[4];
        strip_product(Ka, qf, z);
        strip_product(Va, df, dp);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float p = expf(z[j][q] * scale + kbias[j * 16 + g * 4 + q] - l);   // padding: exp(-inf) = 0
                z[j][q] = p * (dp[j][q] - dl) * scale;
            }
        weighted_rows(Kb, z, acc);
    }
    if (qr < M) {
        float *dst = dQ + ((size_t)b * M + qr) * (heads * AT_D) + h * AT_D + g * 4;
#pragma unroll
        for (int c = 0; c < 2; ++c) *reinterpret_cast<float4 *>(dst + c * 16) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    }
}

__global__ __launch_bounds__(AT_T) void at_dkv_kernel(Rows Q, Rows K, Rows V, Rows dO, const float *__restrict__ lse,
                                                      const float *__restrict__ delta, const uint8_t *__restrict__ mask,
                                                      float *__restrict__ dK, float *__restrict__ dV, int M, int N, int heads,
                                                      float scale) {
    __shared__ __attribute__((aligned(16))) float Qa[AT_R * AT_LA], Qb[AT_R * AT_LB], Da[AT_R * AT_LA], Db[AT_R * AT_LB];
    __shared__ float rl[AT_R], rd[AT_R];
    const int b = blockIdx.z, h = blockIdx.y, key0 = blockIdx.x * AT_R;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
    const int kr = key0 + w * 16 + i, kc = min(kr, N - 1);
    float kf[8], vf[8];
    row_fragments(K.p + (size_t)b * K.s + (size_t)kc * K.ld + h * AT_D, kf);
    row_fragments(V.p + (size_t)b * V.s + (size_t)kc * V.ld + h * AT_D, vf);
    const bool live = kr < N && !(mask && mask[(size_t)b * N + kc]);
    const float *Qh = Q.p + (size_t)b * Q.s + h * AT_D, *Dh = dO.p + (size_t)b * dO.s + h * AT_D;
    const float *lh = lse + ((size_t)b * heads + h) * M, *dh = delta + ((size_t)b * heads + h) * M;
    f32x4 ak[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, av[2] = {ak[0], ak[0]};
    for (int q0 = 0; q0 < M; q0 += AT_R) {
        __syncthreads();
        stage_tile(Qh + (size_t)q0 * Q.ld, Q.ld, M - q0, Qa, Qb);
        stage_tile(Dh + (size_t)q0 * dO.ld, dO.ld, M - q0, Da, Db);
        if (t < AT_R) {
            const bool in = q0 + t < M;
            rl[t] = in ? lh[q0 + t] : __builtin_inff();   // rows beyond M: exp(-inf) = 0
            rd[t] = in ? dh[q0 + t] : 0.f;
        }
        __syncthreads();
        f32x4 z[4], dp[4];
        strip_product(Qa, kf, z);     // lane (g, i): key i of the wave, queries 16 j + 4 g + q
        strip_product(Da, vf, dp);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = j * 16 + g * 4 + q;
                const float p = live ? expf(z[j][q] * scale - rl[r]) : 0.f;
                dp[j][q] = p * (dp[j][q] - rd[r]) * scale;
                z[j][q] = p;
            }
        weighted_rows(Db, z, av);
        weighted_rows(Qb, dp, ak);
    }
    if (kr < N) {
        const size_t off = ((size_t)b * N + kr) * (heads * AT_D) + h * AT_D + g * 4;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            // padding keys: exactly zero (their P is 0 above; written as +0, not as a sum of signed zeros)
            const float4 k4 = live ? make_float4(ak[c][0], ak[c][1], ak[c][2], ak[c][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 v4 = live ? make_float4(av[c][0], av[c][1], av[c][2], av[c][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(dK + off + c * 16) = k4;
            *reinterpret_cast<float4 *>(dV + off + c * 16) = v4;
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

bool rows_ok(const float *p, int ld, long long s) { return p && aligned16(p) && ld >= AT_D && ld % 4 == 0 && s % 4 == 0; }

bool shape_ok(int B, int M, int N, int heads) { return B >= 1 && M >= 1 && N >= 1 && heads >= 1 && B <= 65535 && heads <= 65535; }

float *layout(WsCursor &c, int B, int M, int heads) { return c.take256<float>((size_t)B * heads * M); }   // delta: one float per query row

}  // namespace

extern "C" size_t dpm_attention_train_workspace_bytes(int B, int M, int N, int heads) {
    if (!shape_ok(B, M, N, heads)) return 0;
    WsCursor c(nullptr);
    layout(c, B, M, heads);
    return c.bytes();
}

extern "C" int dpm_attention_train_forward(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk,
                                           const float *V, int ldv, long long sv, float *out, int ldo, long long so, float *lse,
                                           int B, int M, int N, int heads, int head_dim, const uint8_t *key_mask,
                                           dpm_stream_t stream) {
    DPM_CHECK_ARG(lse && shape_ok(B, M, N, heads) && head_dim >= 1);
    if (head_dim != AT_D) return DPM_EUNSUPPORTED;
    DPM_CHECK_ARG(rows_ok(Q, ldq, sq) && rows_ok(K, ldk, sk) && rows_ok(V, ldv, sv) && rows_ok(out, ldo, so));
    hipLaunchKernelGGL(at_forward_kernel, dim3(dpm_cdiv(M, AT_R), heads, B), dim3(AT_T), 0, (hipStream_t)stream, Rows{Q, ldq, sq},
                       Rows{K, ldk, sk}, Rows{V, ldv, sv}, out, ldo, so, lse, key_mask, M, N, heads, 1.0f / sqrtf((float)head_dim));
    return dpm_launch_status();
}

extern "C" int dpm_attention_train_backward(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk,
                                            const float *V, int ldv, long long sv, const float *out, int ldo, long long so,
                                            const float *lse, const float *dout, int ldd, long long sd, const uint8_t *key_mask,
                                            float *dQ, float *dK, float *dV, int B, int M, int N, int heads, int head_dim,
                                            void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(lse && workspace && shape_ok(B, M, N, heads) && head_dim >= 1);
    if (head_dim != AT_D) return DPM_EUNSUPPORTED;
    DPM_CHECK_ARG(rows_ok(Q, ldq, sq) && rows_ok(K, ldk, sk) && rows_ok(V, ldv, sv) && rows_ok(out, ldo, so) &&
                  rows_ok(dout, ldd, sd));
    DPM_CHECK_ARG(dQ && dK && dV && aligned16(dQ) && aligned16(dK) && aligned16(dV));
    hipStream_t st = (hipStream_t)stream;
    WsCursor c(workspace);
    float *delta = layout(c, B, M, heads);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const Rows q{Q, ldq, sq}, k{K, ldk, sk}, v{V, ldv, sv}, d{dout, ldd, sd};
    hipLaunchKernelGGL(at_delta_kernel, dim3(dpm_cdiv(M, AT_T), heads, B), dim3(AT_T), 0, st, out, ldo, so, dout, ldd, sd, M, heads,
                       delta);
    hipLaunchKernelGGL(at_dkv_kernel, dim3(dpm_cdiv(N, AT_R), heads, B), dim3(AT_T), 0, st, q, k, v, d, lse, delta, key_mask, dK, dV,
                       M, N, heads, scale);
    hipLaunchKernelGGL(at_dq_kernel, dim3(dpm_cdiv(M, AT_R), heads, B), dim3(AT_T), 0, st, q, k, v, d, lse, delta, key_mask, dQ, M, N,
                       heads, scale);
    return dpm_launch_status();
}
