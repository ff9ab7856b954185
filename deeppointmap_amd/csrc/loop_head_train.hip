// The loop head for training (heads.py:45-69 OverlapHead, model_pipeline.py:156-181): stage two of the reference's schedule
// trains nothing but this head, on top of a frozen encoder and attention trunk.
//   head(x, y) = projection(cat(mean_l mlp(x), mean_l mlp(y))),  mlp = Conv1d -> ReLU -> Conv1d (kernel size 1)
// The mean over the tokens commutes with the second (affine) convolution, so the only token-sized work is
//   m[b, c] = (1 / L) sum_l relu(x[b, l, :] . W1[c, :] + b1[c])                                   ("loop_pool")
// and, in the backward, the weight gradient of that one layer.  The rest of the head acts on (B, 2 E) rows and stays torch.
//   lp_forward_kernel    one workgroup per (64 channels, 64 tokens, sequence): pre strip on the matrix cores, ReLU, column
//                        sums of the strip -> workspace[b][tile][c]
//   lp_mean_kernel       m[b, c] = (sum over the tiles, in tile order) / L
//   lp_backward_kernel   one workgroup per (64 channels, row split s of S): for each of its 64-row tiles the pre strip again
//                        (pre_strip below: the forward's instruction sequence, hence the forward's bits and its ReLU mask),
//                        G = [pre > 0] g[b, c] / L into LDS, dW1 += G^T x on the matrix cores with the rows as the
//                        reduction dimension -> workspace[s][E E + E] (dW1 then db1 partials)
//   lp_reduce_kernel     dW1, db1 = sum over the splits, in split order
//   lb_kernel            binary cross-entropy of (B,) probabilities, the reference's counts and the gradient seed: one
//                        workgroup, one order
// pre and relu(pre) never reach global memory; x gets no gradient (everything upstream is frozen in this stage).  No
// floating-point atomics and every sum in one order: two runs give identical bytes.
//
// Every product is v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), as in reg_loss.hip and
// attention_train.hip; operand layouts as described there (lane = 16 g + i: A[i][k = g], B[k = g][i], D[4 g + q][i]).  Each
// wave keeps four (pre strip) or sixteen (dW1) independent accumulators.  Every pre element is ONE accumulator chain over
// k = 0 .. 255 in ascending order from zero, plus the bias: its bits do not depend on the tiling.
//
// LDS images (ds_read_b32: banks mod 32 per 32-lane half): a tile read as [row i][k g] has rows 66 floats apart (bank
// 2 i + g: conflict-free), a tile read as [row g][column i] has rows 80 apart (bank 16 g + i: conflict-free).  W1 is 256 KiB:
// it passes through LDS in tiles of 64 channels x 64 k.
#include "dpm_common.h"
#include "workspace.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int LP_T = 256, LP_E = 256, LP_R = 64, LP_C = 64, LP_K = 64, LP_LA = 66, LP_LB = 80, LP_SPLITS = 32;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows [0, 64) x 64 floats of src (row stride ld; rows >= valid read as zero) -> an image with rows LD floats apart
template <int LD>
__device__ __forceinline__ void stage_chunk(const float *__restrict__ src, long long ld, int valid, float *img) {
    const int t = threadIdx.x, c = (t & 15) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int r = p * 16 + (t >> 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < valid) v = *reinterpret_cast<const float4 *>(src + (long long)r * ld + c);
        float2 *d = reinterpret_cast<float2 *>(img + r * LD + c);
        d[0] = make_float2(v.x, v.y), d[1] = make_float2(v.z, v.w);
    }
}

// acc[j][q] = x[row 16 w + 4 g + q] . W1c[16 j + i] + b1c[16 j + i] for the 64 rows at x and the 64 channels at W1c.  The
// forward and the backward both call THIS: the mask of the backward is the forward's comparison on the forward's bits.
__device__ __forceinline__ void pre_strip(const float *__restrict__ x, long long ldx, int valid, const float *__restrict__ W1c,
                                          const float *__restrict__ b1c, float *Xs, float *Wa, f32x4 (&acc)[4]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < LP_E; k0 += LP_K) {
        __syncthreads();   // the previous readers of both images are done
        stage_chunk<LP_LA>(x + k0, ldx, valid, Xs);
        stage_chunk<LP_LA>(W1c + k0, LP_E, LP_C, Wa);
        __syncthreads();
        const float *xr = Xs + (16 * w + i) * LP_LA + g, *wr = Wa + i * LP_LA + g;
#pragma unroll
        for (int kk = 0; kk < LP_K / 4; ++kk) {
            const float a = xr[4 * kk];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma4(a, wr[16 * j * LP_LA + 4 * kk], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float bias = b1c[16 * j + i];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][q] += bias;
    }
}

__global__ __launch_bounds__(LP_T) void lp_forward_kernel(const float *__restrict__ x, long long ldx, const float *__restrict__ W1,
                                                          const float *__restrict__ b1, int L, int tiles, float *__restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float Xs[LP_R * LP_LA], Wa[LP_C * LP_LA];
    __shared__ float part[4][LP_C];
    const int c0 = blockIdx.x * LP_C, tile = blockIdx.y, b = blockIdx.z, row0 = tile * LP_R, valid = min(LP_R, L - row0);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
    f32x4 acc[4];
    pre_strip(x + ((long long)b * L + row0) * ldx, ldx, valid, W1 + (size_t)c0 * LP_E, b1 + c0, Xs, Wa, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) s += (16 * w + 4 * g + q < valid && acc[j][q] > 0.f) ? acc[j][q] : 0.f;
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (g == 0) part[w][16 * j + i] = s;
    }
    __syncthreads();
    if (t < LP_C) ws[((size_t)b * tiles + tile) * LP_E + c0 + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
}

__global__ __launch_bounds__(LP_T) void lp_mean_kernel(const float *__restrict__ ws, int tiles, int L, int n, float *__restrict__ m) {
    const int idx = blockIdx.x * LP_T + threadIdx.x;
    if (idx >= n) return;
    const int b = idx / LP_E, c = idx % LP_E;
    float s = 0.f;
    for (int tile = 0; tile < tiles; ++tile) s += ws[((size_t)b * tiles + tile) * LP_E + c];
    m[idx] = s / (float)L;
}

__global__ __launch_bounds__(LP_T) void lp_backward_kernel(const float *__restrict__ x, long long ldx, const float *__restrict__ W1,
                                                           const float *__restrict__ b1, const float *__restrict__ gm, int L,
                                                           long long R, int ntiles, int S, float *__restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float Xs[LP_R * LP_LB], Wa[LP_C * LP_LA], Gs[LP_R * LP_LB];
    __shared__ float part[4][LP_C];
    const int c0 = blockIdx.x * LP_C, s = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = lane & 15, g = lane >> 4;
    const float fL = (float)L;
    f32x4 dw[4][4];
    float db[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc)
#pragma unroll
        for (int u = 0; u < 4; ++u) dw[kc][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tile = s; tile < ntiles; tile += S) {
        const long long row0 = (long long)tile * LP_R;
        const int valid = (int)min((long long)LP_R, R - row0);
        const float *xt = x + row0 * ldx;
        f32x4 acc[4];
        pre_strip(xt, ldx, valid, W1 + (size_t)c0 * LP_E, b1 + c0, Xs, Wa, acc);
        // G[row][c] = [pre > 0] g[sequence of the row][c] / L; a wave writes its own 16 rows
        float ds[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * w + 4 * g + q;
            const bool live = r < valid;
            const long long bq = live ? (row0 + r) / L : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = (live && acc[j][q] > 0.f) ? gm[bq * LP_E + c0 + 16 * j + i] / fL : 0.f;
                Gs[r * LP_LB + 16 * j + i] = v;
                ds[j] += v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ds[j] += __shfl_xor(ds[j], 16, 64);
            ds[j] += __shfl_xor(ds[j], 32, 64);
            db[j] += ds[j];
        }
        // dW1[c0 + 16 w + .][64 kc + 16 u + .] += sum over the rows of G[row][16 w + .] x[row][64 kc + 16 u + .]
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            __syncthreads();   // G is complete (kc = 0); the previous chunk's readers are done
            stage_chunk<LP_LB>(xt + kc * LP_K, ldx, valid, Xs);
            __syncthreads();
            const float *gr = Gs + g * LP_LB + 16 * w + i, *xr = Xs + g * LP_LB + i;
#pragma unroll
            for (int kk = 0; kk < LP_R / 4; ++kk) {
                const float a = gr[4 * kk * LP_LB];
#pragma unroll
                for (int u = 0; u < 4; ++u) dw[kc][u] = mfma4(a, xr[4 * kk * LP_LB + 16 * u], dw[kc][u]);
            }
        }
    }
    float *o = ws + (size_t)s * (LP_E * LP_E + LP_E);
#pragma unroll
    for (int kc = 0; kc < 4; ++kc)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) o[(size_t)(c0 + 16 * w + 4 * g + q) * LP_E + LP_K * kc + 16 * u + i] = dw[kc][u][q];
    __syncthreads();
    if (g == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) part[w][16 * j + i] = db[j];
    }
    __syncthreads();
    if (t < LP_C) o[LP_E * LP_E + c0 + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
}

__global__ __launch_bounds__(LP_T) void lp_reduce_kernel(const float *__restrict__ ws, int S, float *__restrict__ dW1,
                                                         float *__restrict__ db1) {
    constexpr int n = LP_E * LP_E + LP_E;
    const int idx = blockIdx.x * LP_T + threadIdx.x;
    if (idx >= n) return;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += ws[(size_t)s * n + idx];
    if (idx < LP_E * LP_E) dW1[idx] = acc;
    else db1[idx - LP_E * LP_E] = acc;
}

// torch's binary_cross_entropy (both logarithms clamped at -100) and its backward formula; the reference's counts
__global__ __launch_bounds__(LP_T) void lb_kernel(const float *__restrict__ pred, const float *__restrict__ target, int B,
                                                  float *__restrict__ loss, float *__restrict__ stats, float *__restrict__ dunit) {
    __shared__ float red[6][LP_T];
    const int t = threadIdx.x;
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = t; k < B; k += LP_T) {
        const float p = pred[k], y = target[k];
        const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
        v[0] += -(y * lp + (1.f - y) * lq);
        const bool gt = y != 0.f, pr = p > 0.5f;
        v[1] += gt ? 1.f : 0.f;
        v[2] += gt ? 0.f : 1.f;
        v[3] += pr == gt ? 1.f : 0.f;
        v[4] += (pr && gt) ? 1.f : 0.f;
        v[5] += (pr && !gt) ? 1.f : 0.f;
        dunit[k] = (p - y) / fmaxf(p * (1.f - p), 1e-12f) / (float)B;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k][t] = v[k];
    __syncthreads();
    for (int half = LP_T / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int k = 0; k < 6; ++k) red[k][t] += red[k][t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float l = red[0][0] / (float)B;
        *loss = l;
        stats[0] = l;
    } else if (t < 6) {
        stats[t] = red[t][0];
    } else if (t < 8) {
        stats[t] = 0.f;
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// grid limits, and B L / 64 row tiles must fit an int
bool shape_ok(int B, int L) { return B >= 1 && L >= 1 && B <= 65535 && dpm_cdiv(L, LP_R) <= 65535 && (long long)B * L < (1LL << 36); }

int row_tiles(int B, int L) { return (int)(((long long)B * L + LP_R - 1) / LP_R); }

// one slice for either call: the forward's per-tile column sums or the backward's partial dW1, whichever is larger
float *layout(WsCursor &c, int B, int L) {
    const size_t fwd = (size_t)B * dpm_cdiv(L, LP_R) * LP_E;
    const int nt = row_tiles(B, L);
    const size_t bwd = (size_t)(nt < LP_SPLITS ? nt : LP_SPLITS) * (LP_E * LP_E + LP_E);
    return c.take256<float>(fwd > bwd ? fwd : bwd);
}

}  // namespace

extern "C" size_t dpm_loop_pool_workspace_bytes(int B, int L, int E) {
    if (!shape_ok(B, L) || E != LP_E) return 0;
    WsCursor c(nullptr);
    layout(c, B, L);
    return c.bytes();
}

extern "C" int dpm_loop_pool_forward(const float *x, int ldx, const float *W1, const float *b1, int B, int L, int E, float *m,
                                     void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(x && W1 && b1 && m && workspace && shape_ok(B, L) && E >= 1);
    if (E != LP_E) return DPM_EUNSUPPORTED;
    DPM_CHECK_ARG(aligned16(x) && aligned16(W1) && ldx >= LP_E && ldx % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    WsCursor c(workspace);
    float *ws = layout(c, B, L);
    const int tiles = (int)dpm_cdiv(L, LP_R);
    hipLaunchKernelGGL(lp_forward_kernel, dim3(LP_E / LP_C, tiles, B), dim3(LP_T), 0, st, x, (long long)ldx, W1, b1, L, tiles, ws);
    hipLaunchKernelGGL(lp_mean_kernel, dim3(dpm_cdiv((long long)B * LP_E, LP_T)), dim3(LP_T), 0, st, ws, tiles, L, B * LP_E, m);
    return dpm_launch_status();
}

extern "C" int dpm_loop_pool_backward(const float *x, int ldx, const float *W1, const float *b1, const float *g, int B, int L,
                                      int E, float *dW1, float *db1, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(x && W1 && b1 && g && dW1 && db1 && workspace && shape_ok(B, L) && E >= 1);
    if (E != LP_E) return DPM_EUNSUPPORTED;
    DPM_CHECK_ARG(aligned16(x) && aligned16(W1) && ldx >= LP_E && ldx % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    WsCursor c(workspace);
    float *ws = layout(c, B, L);
    const int ntiles = row_tiles(B, L), S = ntiles < LP_SPLITS ? ntiles : LP_SPLITS;
    hipLaunchKernelGGL(lp_backward_kernel, dim3(LP_E / LP_C, S), dim3(LP_T), 0, st, x, (long long)ldx, W1, b1, g, L,
                       (long long)B * L, ntiles, S, ws);
    hipLaunchKernelGGL(lp_reduce_kernel, dim3(dpm_cdiv(LP_E * LP_E + LP_E, LP_T)), dim3(LP_T), 0, st, ws, S, dW1, db1);
    return dpm_launch_status();
}

extern "C" int dpm_loop_bce_forward(const float *pred, const float *target, int B, float *loss, float *stats, float *dpred_unit,
                                    dpm_stream_t stream) {
    DPM_CHECK_ARG(pred && target && loss && stats && dpred_unit && B >= 1);
    hipLaunchKernelGGL(lb_kernel, dim3(1), dim3(LP_T), 0, (hipStream_t)stream, pred, target, B, loss, stats, dpred_unit);
    return dpm_launch_status();
}
