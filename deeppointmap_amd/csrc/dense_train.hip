// The dense layers for training: the reference's build_mlp (network/encoder/utils.py:358-413: Conv -> LayerNorm -> ReLU), the
// projections, LayerNorms and MLP of DescriptorAttentionLayer (network/decoder/descriptor_attention.py:16-48) and the heads
// (network/decoder/heads.py), forward and backward, as ONE primitive in two forms
//   plain:   out = act(x W^T + bias + residual)
//   normed:  h = x W^T + bias + residual;  out = act(LN(h) * gamma + beta + post)          (eps 1e-5, biased variance)
// x (R, Cin) rows ldx apart, W (Cout, Cin) rows ldw apart, residual / post / out / h (R, Cout) contiguous, act none or ReLU.
//   dt_gemm_kernel<NJ, LN, BKN>   one workgroup per (64 rows, 16 NJ columns): the product on the matrix cores and the epilogue.
//                          LN (16 NJ = Cout in {32, 64, 128, 256}: the workgroup owns whole rows): h, (mean, rstd) per row and
//                          the normalised output from the accumulators.  BKN: the second operand is read as [k][n]
//                          (dX = dh W, W untransposed).
//   dt_ln_rows_kernel      the other widths: LayerNorm of the h rows the plain kernel wrote, one wave per row
//   dt_bwd_rows_kernel     one wave per row: g = dy . [out > 0] (= d post), dn = gamma g,
//                          dh = rstd (dn - mean(dn) - xhat mean(dn xhat)), xhat = (h - mean) rstd   (= d residual)
//   dt_colsum_kernel       d gamma = sum_rows g xhat, d beta = sum_rows g: one workgroup per (64 columns, row slice s of S <= 256),
//                          one partial per workgroup -> workspace[s][2 Cout]
//   dt_dw_kernel           dW = dh^T x with the rows as the reduction dimension: one workgroup per (64 Cin columns, 64 Cout
//                          rows, row slice s of S <= 32) over its 64-row tiles s, s + S, ... -> workspace[s][Cout Cin + Cout]
//                          (dW, then the column sums of dh = d bias); the scheme of lp_backward_kernel (loop_head_train.hip)
//   dt_reduce_kernel       sum over the slices, in slice order
// The backward keeps x, h, (mean, rstd) and out (the ReLU mask is out > 0) and nothing else.  No floating-point atomics; every
// sum has one order that depends on the shapes alone: two runs give identical bytes.
//
// Every product is v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), as in reg_loss.hip, attention_train.hip and
// loop_head_train.hip; operand layouts as there (lane = 16 g + i: A[i][k = g], B[k = g][i], D[4 g + q][i]).  Every element of
// x W^T is ONE accumulator chain over k in ascending order from zero (k beyond Cin contributes exact zeros), then + bias, then
// + residual, whatever the tiling: the plain and the normed form agree on h bit for bit.
//
// LDS images (ds_read_b32: banks mod 32 per 32-lane half): a tile read as [row i][k g] has rows 34 floats apart (bank 2 i + g:
// conflict-free), a tile read as [row g][column i] has rows 80 apart (bank 16 g + i: conflict-free).  Operand rows that are not
// 16-byte aligned (ld % 4 != 0 or a misaligned base: W[:, :Cin] of a (Cout, Cin + 3) weight) are staged with scalar loads, as
// the VEC switch of gemm.hip does.
#include "dpm_common.h"
#include "workspace.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int DT_T = 256, DT_R = 64, DT_KC = 32, DT_LA = 34, DT_LB = 80, DT_SPLITS = 32, DT_CSPLITS = 256;
constexpr float DT_EPS = 1e-5f;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ float4 load4(const float *__restrict__ s, int left, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec && left >= 4) return *reinterpret_cast<const float4 *>(s);
    if (left > 0) v.x = s[0];
    if (left > 1) v.y = s[1];
    if (left > 2) v.z = s[2];
    if (left > 3) v.w = s[3];
    return v;
}

// `rows` x 32 floats of src (row stride ld; rows >= vr and columns >= vc read as zero) -> an image with rows DT_LA apart
__device__ __forceinline__ void stage_rk(const float *__restrict__ src, long long ld, int rows, int vr, int vc, bool vec, float *img) {
    for (int p = threadIdx.x; p < rows * (DT_KC / 4); p += DT_T) {
        const int r = p >> 3, c = (p & 7) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < vr) v = load4(src + (long long)r * ld + c, vc - c, vec);
        float2 *d = reinterpret_cast<float2 *>(img + r * DT_LA + c);
        d[0] = make_float2(v.x, v.y), d[1] = make_float2(v.z, v.w);
    }
}

// `rows` x 64 floats of src (rows >= vr and columns >= vc read as zero) -> an image with rows DT_LB apart
__device__ __forceinline__ void stage_rc(const float *__restrict__ src, long long ld, int rows, int vr, int vc, bool vec, float *img) {
    for (int p = threadIdx.x; p < rows * 16; p += DT_T) {
        const int r = p >> 4, c = (p & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < vr) v = load4(src + (long long)r * ld + c, vc - c, vec);
        *reinterpret_cast<float4 *>(img + r * DT_LB + c) = v;
    }
}

// acc[j][q] = sum_k A[row 16 w + 4 g + q][k] B(k, column 16 j + i) for 64 rows at A and 16 NJ columns.  !BKN: B(k, n) =
// Bm[n * ldb + k] (a weight, rows = output channels); BKN: B(k, n) = Bm[k * ldb + n] (NJ = 4).
template <int NJ, bool BKN>
__device__ __forceinline__ void gemm_strip(const float *__restrict__ A, long long lda, int vr, bool vecA, const float *__restrict__ Bm,
                                           long long ldb, int vn, bool vecB, int K, float *As, float *Bs, f32x4 (&acc)[NJ]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += DT_KC) {
        const int vk = min(DT_KC, K - k0);
        __syncthreads();   // the previous readers of both images are done
        stage_rk(A + k0, lda, DT_R, vr, vk, vecA, As);
        if (BKN) stage_rc(Bm + (long long)k0 * ldb, ldb, DT_KC, vk, vn, vecB, Bs);
        else stage_rk(Bm + k0, ldb, 16 * NJ, vn, vk, vecB, Bs);
        __syncthreads();
        const float *ar = As + (16 * w + i) * DT_LA + g;
        const float *br = BKN ? Bs + g * DT_LB + i : Bs + i * DT_LA + g;
#pragma unroll
        for (int kk = 0; kk < DT_KC / 4; ++kk) {
            const float a = ar[4 * kk];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = mfma4(a, BKN ? br[4 * kk * DT_LB + 16 * j] : br[16 * j * DT_LA + 4 * kk], acc[j]);
        }
    }
}

// sum over the 16 lanes that hold one output row (lanes 16 g .. 16 g + 15), the same value in each of them
__device__ __forceinline__ float row16_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}

template <int NJ, bool LN, bool BKN>
__global__ __launch_bounds__(DT_T) void dt_gemm_kernel(const float *__restrict__ x, long long ldx, const float *__restrict__ W, long long ldw,
                                                       const float *__restrict__ bias, const float *__restrict__ residual,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ post, long long R, int K, int Cout, int act, int vecx,
                                                       int vecw, float *__restrict__ out, float *__restrict__ h, float *__restrict__ stats) {
    __shared__ __attribute__((aligned(16))) float As[DT_R * DT_LA], Bs[BKN ? DT_KC * DT_LB : 16 * NJ * DT_LA];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * DT_R;
    const int c0 = blockIdx.y * 16 * NJ, vr = (int)min((long long)DT_R, R - row0), vn = min(16 * NJ, Cout - c0);
    f32x4 acc[NJ];
    gemm_strip<NJ, BKN>(x + row0 * ldx, ldx, vr, vecx != 0, BKN ? W + c0 : W + (long long)c0 * ldw, ldw, vn, vecw != 0, K, As, Bs, acc);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = c0 + 16 * j + i;
        if (c >= Cout) continue;
        if (bias) {
            const float b = bias[c];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[j][q] += b;
        }
        if (residual) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * w + 4 * g + q;
                if (r < vr) acc[j][q] += residual[(row0 + r) * Cout + c];
            }
        }
    }
    if (!LN) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = c0 + 16 * j + i;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * w + 4 * g + q;
                const float v = acc[j][q];
                if (c < Cout && r < vr) out[(row0 + r) * Cout + c] = (act == DPM_ACT_RELU && !(v > 0.f)) ? 0.f : v;
            }
        }
        return;
    }
    // LayerNorm: 16 NJ == Cout, row 16 w + 4 g + q of the tile lives in acc[.][q] of the 16 lanes of group g
    const float fC = (float)Cout;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 16 * w + 4 * g + q;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) s += acc[j][q];
        const float mean = row16_sum(s) / fC;
        float s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float d = acc[j][q] - mean;
            s2 += d * d;
        }
        const float rstd = 1.f / sqrtf(row16_sum(s2) / fC + DT_EPS);
        if (r >= vr) continue;
        const long long row = row0 + r;
        if (i == 0) stats[2 * row] = mean, stats[2 * row + 1] = rstd;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = 16 * j + i;
            const float hv = acc[j][q];
            h[row * Cout + c] = hv;
            float v = (hv - mean) * rstd * gamma[c] + beta[c];
            if (post) v += post[row * Cout + c];
            out[row * Cout + c] = (act == DPM_ACT_RELU && !(v > 0.f)) ? 0.f : v;
        }
    }
}

// LayerNorm of one h row per wave (the widths the GEMM kernel's epilogue does not cover)
__global__ __launch_bounds__(DT_T) void dt_ln_rows_kernel(const float *__restrict__ h, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, const float *__restrict__ post, long long R,
                                                          int Cout, int act, float *__restrict__ out, float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float *hr = h + row * Cout;
    const float fC = (float)Cout;
    float s = 0.f;
    for (int c = lane; c < Cout; c += 64) s += hr[c];
    const float mean = wave_sum(s) / fC;
    float s2 = 0.f;
    for (int c = lane; c < Cout; c += 64) {
        const float d = hr[c] - mean;
        s2 += d * d;
    }
    const float rstd = 1.f / sqrtf(wave_sum(s2) / fC + DT_EPS);
    if (lane == 0) stats[2 * row] = mean, stats[2 * row + 1] = rstd;
    for (int c = lane; c < Cout; c += 64) {
        float v = (hr[c] - mean) * rstd * gamma[c] + beta[c];
        if (post) v += post[row * Cout + c];
        out[row * Cout + c] = (act == DPM_ACT_RELU && !(v > 0.f)) ? 0.f : v;
    }
}

// one wave per row.  plain (gamma == NULL): g = dy . [out > 0].  normed: g likewise (written if asked for), dh as above.
__global__ __launch_bounds__(DT_T) void dt_bwd_rows_kernel(const float *__restrict__ dy, const float *__restrict__ out,
                                                           const float *__restrict__ h, const float *__restrict__ stats,
                                                           const float *__restrict__ gamma, long long R, int Cout, int act,
                                                           float *__restrict__ gout, float *__restrict__ dh) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float *dyr = dy + row * Cout, *outr = out + row * Cout;
    const bool relu = act == DPM_ACT_RELU;
    if (!gamma) {
        for (int c = lane; c < Cout; c += 64) gout[row * Cout + c] = (relu && !(outr[c] > 0.f)) ? 0.f : dyr[c];
        return;
    }
    const float *hr = h + row * Cout;
    const float mean = stats[2 * row], rstd = stats[2 * row + 1], fC = (float)Cout;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < Cout; c += 64) {
        const float gv = (relu && !(outr[c] > 0.f)) ? 0.f : dyr[c];
        const float dn = gamma[c] * gv, xh = (hr[c] - mean) * rstd;
        s1 += dn;
        s2 += dn * xh;
    }
    const float m1 = wave_sum(s1) / fC, m2 = wave_sum(s2) / fC;
    for (int c = lane; c < Cout; c += 64) {
        const float gv = (relu && !(outr[c] > 0.f)) ? 0.f : dyr[c];
        const float dn = gamma[c] * gv, xh = (hr[c] - mean) * rstd;
        dh[row * Cout + c] = rstd * ((dn - m1) - xh * m2);
        if (gout) gout[row * Cout + c] = gv;
    }
}

// ws[s][0][c] = sum over the rows of slice s of g xhat, ws[s][1][c] = ... of g.  Thread (sub, column): rows sub, sub + 4, ...
// of every tile of the slice in ascending order, then the four subs in order.
__global__ __launch_bounds__(DT_T) void dt_colsum_kernel(const float *__restrict__ dy, const float *__restrict__ out,
                                                         const float *__restrict__ h, const float *__restrict__ stats, long long R,
                                                         int Cout, int act, int ntiles, int S, float *__restrict__ ws) {
    __shared__ float part[2][4][64];
    const int t = threadIdx.x, col = t & 63, sub = t >> 6, c = blockIdx.x * 64 + col, s = blockIdx.y;
    const bool relu = act == DPM_ACT_RELU;
    float sg = 0.f, sb = 0.f;
    if (c < Cout) {
        for (int tile = s; tile < ntiles; tile += S) {
            const long long row0 = (long long)tile * DT_R;
            const int vr = (int)min((long long)DT_R, R - row0);
            for (int r = sub; r < vr; r += 4) {
                const long long o = (row0 + r) * Cout + c;
                const float gv = (relu && !(out[o] > 0.f)) ? 0.f : dy[o];
                const float xh = (h[o] - stats[2 * (row0 + r)]) * stats[2 * (row0 + r) + 1];
                sg += gv * xh;
                sb += gv;
            }
        }
    }
    part[0][sub][col] = sg, part[1][sub][col] = sb;
    __syncthreads();
    if (t < 128) {
        const int k = t >> 6;
        const float v = ((part[k][0][col] + part[k][1][col]) + part[k][2][col]) + part[k][3][col];
        if (c < Cout) ws[((size_t)s * 2 + k) * Cout + c] = v;
    }
}

// workspace[s][c][k] (c < Cout, k < Cin), then workspace[s][Cout Cin + c]: the partial dW and column sums of dh of slice s
__global__ __launch_bounds__(DT_T) void dt_dw_kernel(const float *__restrict__ dh, int vecd, const float *__restrict__ x, long long ldx,
                                                     int vecx, long long R, int Cin, int Cout, int ntiles, int S, int want_db,
                                                     float *__restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float Gs[DT_R * DT_LB], Xs[DT_R * DT_LB];
    const int k0 = blockIdx.x * 64, c0 = blockIdx.y * 64, s = blockIdx.z;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
    const int vc = min(64, Cout - c0), vk = min(64, Cin - k0);
    const bool sums = want_db && blockIdx.x == 0;
    f32x4 dw[4];
    float db = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) dw[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tile = s; tile < ntiles; tile += S) {
        const long long row0 = (long long)tile * DT_R;
        const int vr = (int)min((long long)DT_R, R - row0);
        __syncthreads();   // the previous tile's readers are done
        stage_rc(dh + row0 * Cout + c0, Cout, DT_R, vr, vc, vecd != 0, Gs);
        stage_rc(x + row0 * ldx + k0, ldx, DT_R, vr, vk, vecx != 0, Xs);
        __syncthreads();
        if (sums && t < 64) {
            float a = 0.f;
            for (int r = 0; r < DT_R; ++r) a += Gs[r * DT_LB + t];
            db += a;
        }
        const float *gr = Gs + g * DT_LB + 16 * w + i, *xr = Xs + g * DT_LB + i;
#pragma unroll
        for (int kk = 0; kk < DT_R / 4; ++kk) {
            const float a = gr[4 * kk * DT_LB];
#pragma unroll
            for (int u = 0; u < 4; ++u) dw[u] = mfma4(a, xr[4 * kk * DT_LB + 16 * u], dw[u]);
        }
    }
    float *o = ws + (size_t)s * ((size_t)Cout * Cin + Cout);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + 16 * w + 4 * g + q, k = k0 + 16 * u + i;
            if (c < Cout && k < Cin) o[(size_t)c * Cin + k] = dw[u][q];
        }
    if (sums && t < 64 && c0 + t < Cout) o[(size_t)Cout * Cin + c0 + t] = db;
}

// a[idx] (idx < na) or b[idx - na] = sum over the S slices of ws[s][idx], in slice order; a NULL target is skipped
__global__ __launch_bounds__(DT_T) void dt_reduce_kernel(const float *__restrict__ ws, int S, size_t n, size_t na, float *__restrict__ a,
                                                         float *__restrict__ b) {
    const size_t idx = (size_t)blockIdx.x * DT_T + threadIdx.x;
    if (idx >= n) return;
    float *dst = idx < na ? (a ? a + idx : nullptr) : (b ? b + (idx - na) : nullptr);
    if (!dst) return;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += ws[(size_t)s * n + idx];
    *dst = acc;
}

bool vec_ok(const void *p, long long ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

// the row tiles go to blockIdx.x (< 2^31), weights stay below 2^31 elements
bool shape_ok(long long R, int Cin, int Cout) {
    return R >= 0 && R < (1LL << 36) && Cin >= 1 && Cout >= 1 && (long long)Cin * Cout < (1LL << 30) && Cout <= (1 << 20) && Cin <= (1 << 20);
}

int row_tiles(long long R) { return (int)((R + DT_R - 1) / DT_R); }

int slices(long long R, int most = DT_SPLITS) {
    const int nt = row_tiles(R);
    return nt < most ? nt : most;
}

// one slice both backward calls start at: the dW partials, and room for the row kernel's column partials: all DT_CSPLITS of
// them as soon as the rows exceed DT_SPLITS tiles, so that the size is constant from there on
float *layout(WsCursor &c, long long R, int Cin, int Cout) {
    const size_t S = (size_t)slices(R), S2 = row_tiles(R) > DT_SPLITS ? (size_t)DT_CSPLITS : S;
    return c.take256<float>(S * ((size_t)Cout * Cin + Cout) + S2 * 2 * (size_t)Cout);
}

int zero_async(float *p, size_t n, hipStream_t st) {
    const hipError_t e = p ? hipMemsetAsync(p, 0, 4 * n, st) : hipSuccess;
    return e == hipSuccess ? DPM_OK : (int)e;
}

bool fused_width(int Cout) { return Cout == 32 || Cout == 64 || Cout == 128 || Cout == 256; }

template <int NJ>
void launch_ln(hipStream_t st, unsigned tiles, const float *x, int ldx, const float *W, int ldw, const float *bias, const float *residual,
               const float *gamma, const float *beta, const float *post, long long R, int Cin, int Cout, int act, float *out, float *h,
               float *stats) {
    hipLaunchKernelGGL((dt_gemm_kernel<NJ, true, false>), dim3(tiles, 1), dim3(DT_T), 0, st, x, (long long)ldx, W, (long long)ldw, bias,
                       residual, gamma, beta, post, R, Cin, Cout, act, (int)vec_ok(x, ldx), (int)vec_ok(W, ldw), out, h, stats);
}

}  // namespace

extern "C" size_t dpm_dense_train_workspace_bytes(long long R, int Cin, int Cout) {
    if (!shape_ok(R, Cin, Cout)) return 0;
    WsCursor c(nullptr);
    layout(c, R, Cin, Cout);
    return c.bytes();
}

extern "C" int dpm_dense_train_forward(const float *x, int ldx, const float *W, int ldw, const float *bias, const float *residual,
                                       const float *gamma, const float *beta, const float *post, long long R, int Cin, int Cout, int act,
                                       float *out, float *h, float *stats, dpm_stream_t stream) {
    DPM_CHECK_ARG(shape_ok(R, Cin, Cout) && W && ldx >= Cin && ldw >= Cin && (act == DPM_ACT_NONE || act == DPM_ACT_RELU));
    const bool normed = gamma != nullptr;
    DPM_CHECK_ARG(normed ? beta != nullptr : (!beta && !post && !h && !stats));
    if (R == 0) return DPM_OK;   // empty operands may be null pointers
    DPM_CHECK_ARG(x && out && (!normed || (h && stats)));
    hipStream_t st = (hipStream_t)stream;
    const unsigned tiles = (unsigned)row_tiles(R);
    if (normed && fused_width(Cout)) {
        switch (Cout) {
        case 32: launch_ln<2>(st, tiles, x, ldx, W, ldw, bias, residual, gamma, beta, post, R, Cin, Cout, act, out, h, stats); break;
        case 64: launch_ln<4>(st, tiles, x, ldx, W, ldw, bias, residual, gamma, beta, post, R, Cin, Cout, act, out, h, stats); break;
        case 128: launch_ln<8>(st, tiles, x, ldx, W, ldw, bias, residual, gamma, beta, post, R, Cin, Cout, act, out, h, stats); break;
        default: launch_ln<16>(st, tiles, x, ldx, W, ldw, bias, residual, gamma, beta, post, R, Cin, Cout, act, out, h, stats); break;
        }
        return dpm_launch_status();
    }
    hipLaunchKernelGGL((dt_gemm_kernel<4, false, false>), dim3(tiles, dpm_cdiv(Cout, 64)), dim3(DT_T), 0, st, x, (long long)ldx, W,
                       (long long)ldw, bias, residual, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, R, Cin, Cout,
                       normed ? DPM_ACT_NONE : act, (int)vec_ok(x, ldx), (int)vec_ok(W, ldw), normed ? h : out, (float *)nullptr,
                       (float *)nullptr);
    if (normed)
        hipLaunchKernelGGL(dt_ln_rows_kernel, dim3(dpm_cdiv(R, 4)), dim3(DT_T), 0, st, h, gamma, beta, post, R, Cout, act, out, stats);
    return dpm_launch_status();
}

extern "C" int dpm_dense_train_backward_rows(const float *dy, const float *out, const float *h, const float *stats, const float *gamma,
                                             long long R, int Cout, int act, float *g, float *dh, float *dgamma, float *dbeta,
                                             void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(shape_ok(R, 1, Cout) && (act == DPM_ACT_NONE || act == DPM_ACT_RELU));
    const bool normed = gamma != nullptr;
    DPM_CHECK_ARG(normed ? ((!dgamma == !dbeta) && (!dgamma || workspace)) : (!h && !stats && !dh && !dgamma && !dbeta));
    hipStream_t st = (hipStream_t)stream;
    if (R == 0) {
        const int e = zero_async(dgamma, (size_t)Cout, st);
        return e != DPM_OK ? e : zero_async(dbeta, (size_t)Cout, st);
    }
    DPM_CHECK_ARG(dy && (out || act == DPM_ACT_NONE) && (normed ? (h && stats && dh) : g != nullptr));
    if (!out) out = dy;   // never read for ACT_NONE
    hipLaunchKernelGGL(dt_bwd_rows_kernel, dim3(dpm_cdiv(R, 4)), dim3(DT_T), 0, st, dy, out, h, stats, gamma, R, Cout, act, g, dh);
    if (dgamma) {
        WsCursor c(workspace);
        float *ws = layout(c, R, 1, Cout);
        const int nt = row_tiles(R), S = slices(R, DT_CSPLITS);
        hipLaunchKernelGGL(dt_colsum_kernel, dim3(dpm_cdiv(Cout, 64), S), dim3(DT_T), 0, st, dy, out, h, stats, R, Cout, act, nt, S, ws);
        hipLaunchKernelGGL(dt_reduce_kernel, dim3(dpm_cdiv(2 * (long long)Cout, DT_T)), dim3(DT_T), 0, st, ws, S, 2 * (size_t)Cout,
                           (size_t)Cout, dgamma, dbeta);
    }
    return dpm_launch_status();
}

extern "C" int dpm_dense_train_backward_gemm(const float *dh, const float *x, int ldx, const float *W, int ldw, long long R, int Cin,
                                             int Cout, float *dx, float *dW, float *dbias, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(shape_ok(R, Cin, Cout) && ldx >= Cin && ldw >= Cin && (!dbias || dW) && (!dW || workspace) && (!dx || W));
    hipStream_t st = (hipStream_t)stream;
    if (R == 0) {
        const int e = zero_async(dW, (size_t)Cout * Cin, st);
        return e != DPM_OK ? e : zero_async(dbias, (size_t)Cout, st);
    }
    DPM_CHECK_ARG(dh && (!dW || x));
    const int nt = row_tiles(R);
    if (dx)   // dX = dh W: the reduction runs over Cout, W is read as [k = channel][n = input column]
        hipLaunchKernelGGL((dt_gemm_kernel<4, false, true>), dim3(nt, dpm_cdiv(Cin, 64)), dim3(DT_T), 0, st, dh, (long long)Cout, W,
                           (long long)ldw, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr,
                           (const float *)nullptr, R, Cout, Cin, DPM_ACT_NONE, (int)vec_ok(dh, Cout), (int)vec_ok(W, ldw), dx,
                           (float *)nullptr, (float *)nullptr);
    if (dW) {
        WsCursor c(workspace);
        float *ws = layout(c, R, Cin, Cout);
        const int S = slices(R);
        const size_t n = (size_t)Cout * Cin + Cout;
        hipLaunchKernelGGL(dt_dw_kernel, dim3(dpm_cdiv(Cin, 64), dpm_cdiv(Cout, 64), S), dim3(DT_T), 0, st, dh, (int)vec_ok(dh, Cout), x,
                           (long long)ldx, (int)vec_ok(x, ldx), R, Cin, Cout, nt, S, dbias ? 1 : 0, ws);
        hipLaunchKernelGGL(dt_reduce_kernel, dim3(dpm_cdiv((long long)n, DT_T)), dim3(DT_T), 0, st, ws, S, n, (size_t)Cout * Cin, dW, dbias);
    }
    return dpm_launch_status();
}
