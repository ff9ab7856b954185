// RegistrationLoss (reference network/loss.py) for training: the InfoNCE pairing terms and their analytic backward without
// any (B, S, D) tensor.  One call handles one feature pair (fine or coarse) in both directions; "a" is the side whose rows
// a sweep walks, "b" the other side, and the dst -> src direction is the same kernel with the sides swapped.
//   rl_pairs_kernel     nearest neighbour of every a point among the b points, dist2 = (dx dx + dy dy) + dz dz in fp32
//                       (the library is compiled with -ffp-contract=off: this is torch's CPU sum bit for bit), first index
//                       on ties, -1 unless min dist2 <= eps^2; per-row count of the neutral entries (make_pairs)
//   rl_prep_kernel      x (B,C,N) -> norm (B,N), x / max(norm, 1e-12) transposed to (B,N,C) (F.normalize)
//   rl_forward_kernel   strips of 64 rows x tiles of 256 columns of z = a^ b^T / tau on fp32 MFMA (the instruction and k
//                       order of match.hip), an online log-sum-exp per row (coarse: entries with dist2 <= eps^2 other than
//                       the row's own neighbour are left out), the label logit, the fine row argmax (eval_pairing_acc)
//   rl_partial_kernel   per-row terms -> per-chunk sums in double, then rl_reduce_kernel -> the two direction means and
//                       counts: two levels, each in one fixed order (no float atomics)
//   rl_backward_kernel  the same strips again: dZ = w_r (p_r - onehot) + w_c (p_c - onehot) through LDS into a second MFMA
//                       product dZ b^, then the normalisation backward straight into the (B,C,M) gradient.  Run once per
//                       side (row sweep, then the column sweep with the sides swapped), deterministic.
// The dst -> src statistics come from a second sweep, not from partial column statistics per strip as in match.hip: those
// would be (B, S / 64, D) pairs of floats of workspace (128 MiB per feature pair at B = 2, S = D = 16384) against twice the
// MFMA work.  The partial-statistics variant was not built or measured.
#include "dpm_common.h"
#include "workspace.h"

#include <type_traits>

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int RL_ROWS = 64, RL_COLS = 256, RL_KT = 32, RL_LD = RL_KT + 2, RL_T = 256;
constexpr int RL_SMEM = (RL_ROWS + RL_COLS) * RL_LD;   // floats: operand tiles of the strip product
constexpr int RL_DLD = RL_COLS + 4;                    // row stride of the dZ tile (rows 4 banks apart: conflict-free reads)
constexpr int RL_SMEM_B = RL_ROWS * RL_DLD;            // the backward's dZ tile over the dead operand tiles
static_assert(RL_SMEM_B >= RL_SMEM, "the dZ tile reuses the operand tiles");
constexpr float RL_NORM_EPS = 1e-12f;
constexpr int RL_COUNTED = 1, RL_HIT = 2;

// 64 x 256 tile of A B^T, the product of match.hip's match_strip_gemm: wave w owns columns 64 w .. 64 w + 63 as 4 x 4 blocks
// of 16 x 16; lane layout of block (i, j): row i*16 + (lane & 15), columns j*16 + (lane >> 4)*4 + 0..3.  Rows / columns
// beyond rows_a / N read the last valid one (masked by the callers).  C % 32 == 0.
__device__ __forceinline__ void rl_strip_gemm(const float *__restrict__ A, int rows_a, const float *__restrict__ B, int N, int C,
                                              float *smem, f32x4 (&acc)[4][4]) {
    float (*As)[RL_LD] = reinterpret_cast<float (*)[RL_LD]>(smem);
    float (*Bs)[RL_LD] = reinterpret_cast<float (*)[RL_LD]>(smem + RL_ROWS * RL_LD);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int sr = t >> 3, sk = (t & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 ar[2], br[8];
    auto request = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            ar[p] = *reinterpret_cast<const float4 *>(A + (size_t)min(p * 32 + sr, rows_a - 1) * C + k0 + sk);
#pragma unroll
        for (int p = 0; p < 8; ++p)
            br[p] = *reinterpret_cast<const float4 *>(B + (size_t)min(p * 32 + sr, N - 1) * C + k0 + sk);
    };
    request(0);
    for (int k0 = 0; k0 < C; k0 += RL_KT) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float2 *d = reinterpret_cast<float2 *>(&As[p * 32 + sr][sk]);
            d[0] = make_float2(ar[p].x, ar[p].y), d[1] = make_float2(ar[p].z, ar[p].w);
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            float2 *d = reinterpret_cast<float2 *>(&Bs[p * 32 + sr][sk]);
            d[0] = make_float2(br[p].x, br[p].y), d[1] = make_float2(br[p].z, br[p].w);
        }
        __syncthreads();
        if (k0 + RL_KT < C) request(k0 + RL_KT);
#pragma unroll
        for (int kk = 0; kk < RL_KT; kk += 4) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[i * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[w * 64 + j * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], a[i], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;   // no contraction (-ffp-contract=off): torch's CPU sum over the last dimension
}

// (m, s) of two partial log-sum-exps over disjoint sets; m = -inf means the empty set (s = 0)
__device__ __forceinline__ void lse_merge(float &m, float &s, float mo, float so) {
    const float mn = fmaxf(m, mo);
    if (mn == -__builtin_inff()) return;
    s = (m == mn ? s : s * expf(m - mn)) + (mo == mn ? so : so * expf(mo - mn));
    m = mn;
}

// larger value wins, the smaller index on ties (torch.max)
__device__ __forceinline__ void argmax_merge(float &v, int &i, float vo, int io) {
    if (vo > v || (vo == v && io < i)) v = vo, i = io;
}

__global__ __launch_bounds__(RL_T) void rl_pairs_kernel(const float *__restrict__ xa, const float *__restrict__ xb, int M, int N,
                                                        float eps2, int *__restrict__ nn, int *__restrict__ neutral) {
    __shared__ float cb[3][RL_T];
    const int b = blockIdx.y, r = blockIdx.x * RL_T + threadIdx.x;
    const float *pa = xa + (size_t)b * 3 * M, *pb = xb + (size_t)b * 3 * N;
    const int rr = min(r, M - 1);
    const float ax = pa[rr], ay = pa[M + rr], az = pa[2 * M + rr];
    float best = __builtin_inff();
    int bi = 0, within = 0;
    for (int c0 = 0; c0 < N; c0 += RL_T) {
        __syncthreads();
        const int c = c0 + threadIdx.x;
        if (c < N) cb[0][threadIdx.x] = pb[c], cb[1][threadIdx.x] = pb[N + c], cb[2][threadIdx.x] = pb[2 * N + c];
        __syncthreads();
        const int n = min(RL_T, N - c0);
        for (int k = 0; k < n; ++k) {
            const float d = dist2(ax, ay, az, cb[0][k], cb[1][k], cb[2][k]);
            if (d < best) best = d, bi = c0 + k;   // strict: the first index on ties (torch.min)
            within += d <= eps2;
        }
    }
    if (r < M) {
        const bool corr = best <= eps2;
        nn[(size_t)b * M + r] = corr ? bi : -1;
        if (neutral) neutral[(size_t)b * M + r] = within - (corr ? 1 : 0);   // the neighbour itself is not neutral
    }
}

// 64 points x 64 channels per pass through LDS: coalesced reads along the points, coalesced writes along the channels
__global__ __launch_bounds__(RL_T) void rl_prep_kernel(const float *__restrict__ x, int N, int C, float *__restrict__ xhat,
                                                       float *__restrict__ norm) {
    __shared__ float tile[64][65];
    __shared__ float part[4][64];
    const int b = blockIdx.y, p0 = blockIdx.x * 64, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float *xb = x + (size_t)b * C * N;
    const int p = p0 + lane;
    float ss = 0.f;
    if (p < N)
        for (int c = w; c < C; c += 4) {
            const float v = xb[(size_t)c * N + p];
            ss += v * v;
        }
    part[w][lane] = ss;
    __syncthreads();
    if (t < 64) {
        const float n = sqrtf((part[0][t] + part[1][t]) + (part[2][t] + part[3][t]));
        part[0][t] = fmaxf(n, RL_NORM_EPS);
        if (p0 + t < N) norm[(size_t)b * N + p0 + t] = n;
    }
    __syncthreads();
    for (int c0 = 0; c0 < C; c0 += 64) {
        for (int e = t; e < 64 * 64; e += RL_T) {
            const int cc = e >> 6, pp = e & 63;
            tile[cc][pp] = p0 + pp < N ? xb[(size_t)(c0 + cc) * N + p0 + pp] : 0.f;
        }
        __syncthreads();
        for (int e = t; e < 64 * 64; e += RL_T) {
            const int pp = e >> 6, cc = e & 63;
            if (p0 + pp < N) xhat[((size_t)b * N + p0 + pp) * C + c0 + cc] = tile[cc][pp] / part[0][pp];
        }
        __syncthreads();
    }
}

struct RowOut {
    float *lse, *term;
    int *flags, *argmax;
};

template <bool NEUTRAL>
__global__ __launch_bounds__(RL_T) void rl_forward_kernel(const float *__restrict__ Ah, const float *__restrict__ Bh,
                                                          const float *__restrict__ xa, const float *__restrict__ xb,
                                                          const uint8_t *__restrict__ pad_a, const int *__restrict__ nn_a, int M,
                                                          int N, int C, float itau, float eps2, RowOut out) {
    __shared__ __attribute__((aligned(16))) float smem[RL_SMEM];
    __shared__ float cx[3][RL_COLS];
    __shared__ float rm[4][RL_ROWS], rs[4][RL_ROWS], rv[4][RL_ROWS], lab[RL_ROWS];
    __shared__ int ri[4][RL_ROWS];
    const int b = blockIdx.y, row0 = blockIdx.x * RL_ROWS, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float NEG = -__builtin_inff();
    int nn[4];
    float px[4], py[4], pz[4], m[4], s[4], bv[4];
    int bi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + i * 16 + (lane & 15), rc = min(r, M - 1);
        nn[i] = r < M ? nn_a[(size_t)b * M + r] : -1;
        if (NEUTRAL) {
            const float *p = xa + (size_t)b * 3 * M;
            px[i] = p[rc], py[i] = p[M + rc], pz[i] = p[2 * M + rc];
        }
        m[i] = NEG, s[i] = 0.f, bv[i] = NEG, bi[i] = 0x7fffffff;
    }
    const float *A = Ah + ((size_t)b * M + row0) * C;
    for (int col0 = 0; col0 < N; col0 += RL_COLS) {
        if (NEUTRAL) {
            __syncthreads();   // the previous tile's readers of cx are done
            const int c = col0 + t;
            if (c < N) {
                const float *p = xb + (size_t)b * 3 * N;
                cx[0][t] = p[c], cx[1][t] = p[N + c], cx[2][t] = p[2 * N + c];
            }
        }
        f32x4 acc[4][4];
        rl_strip_gemm(A, M - row0, Bh + ((size_t)b * N + col0) * C, N - col0, C, smem, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float z[16];
            float tm = NEG;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cl = w * 64 + j * 16 + (lane >> 4) * 4 + q, c = col0 + cl;
                    const float raw = acc[i][j][q];
                    bool in = c < N;
                    if (!NEUTRAL && in && raw > bv[i]) bv[i] = raw, bi[i] = c;   // columns in increasing order: first on ties
                    const float v = raw * itau;
                    if (c == nn[i]) lab[i * 16 + (lane & 15)] = v;
                    if (NEUTRAL && in && c != nn[i] && dist2(px[i], py[i], pz[i], cx[0][cl], cx[1][cl], cx[2][cl]) <= eps2) in = false;
                    z[j * 4 + q] = in ? v : NEG;
                    tm = fmaxf(tm, z[j * 4 + q]);
                }
            const float mn = fmaxf(m[i], tm);
            if (mn != NEG) {
                float acc_s = m[i] == mn ? s[i] : s[i] * expf(m[i] - mn);
#pragma unroll
                for (int e = 0; e < 16; ++e) acc_s += expf(z[e] - mn);
                s[i] = acc_s, m[i] = mn;
            }
        }
    }
    // the four lanes of a row (equal lane & 15) in this wave, then the four waves in order
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int x = 16; x <= 32; x <<= 1) {
            const float mo = __shfl_xor(m[i], x, 64), so = __shfl_xor(s[i], x, 64);
            lse_merge(m[i], s[i], mo, so);
            if (!NEUTRAL) {
                const float vo = __shfl_xor(bv[i], x, 64);
                const int io = __shfl_xor(bi[i], x, 64);
                argmax_merge(bv[i], bi[i], vo, io);
            }
        }
        if (lane < 16) {
            const int r = i * 16 + lane;
            rm[w][r] = m[i], rs[w][r] = s[i], rv[w][r] = bv[i], ri[w][r] = bi[i];
        }
    }
    __syncthreads();
    if (t < RL_ROWS && row0 + t < M) {
        float mm = rm[0][t], ss = rs[0][t], vv = rv[0][t];
        int ii = ri[0][t];
        for (int k = 1; k < 4; ++k) {
            lse_merge(mm, ss, rm[k][t], rs[k][t]);
            argmax_merge(vv, ii, rv[k][t], ri[k][t]);
        }
        const size_t r = (size_t)b * M + row0 + t;
        const int n = nn_a[r];
        const float lse = mm + logf(ss);
        const bool counted = n >= 0 && !pad_a[r];
        out.lse[r] = lse;
        out.term[r] = counted ? lse - lab[t] : 0.f;
        out.flags[r] = (counted ? RL_COUNTED : 0) | (!NEUTRAL && counted && ii == n ? RL_HIT : 0);
        if (!NEUTRAL && out.argmax) out.argmax[r] = ii;
    }
}

// Two fixed-order levels (no float atomics): rl_partial_kernel sums the per-row terms of chunk blockIdx.x of direction
// blockIdx.y (rows [x * chunk, (x + 1) * chunk), chunk = ceil(R / RL_PARTS): the partition depends on R alone) in double;
// rl_reduce_kernel folds the RL_PARTS partials of each direction in one tree.
constexpr int RL_PARTS = RL_T;

struct Partials {
    double *v;           // (2, RL_PARTS)
    long long *n, *h;    // counted rows, hits
};

__device__ __forceinline__ void block_sum3(double &v, long long &n, long long &h) {
    __shared__ double sv[RL_T];
    __shared__ long long sn[RL_T], sh[RL_T];
    const int t = threadIdx.x;
    sv[t] = v, sn[t] = n, sh[t] = h;
    __syncthreads();
    for (int off = RL_T / 2; off > 0; off >>= 1) {
        if (t < off) sv[t] += sv[t + off], sn[t] += sn[t + off], sh[t] += sh[t + off];
        __syncthreads();
    }
    v = sv[0], n = sn[0], h = sh[0];
    __syncthreads();
}

__global__ __launch_bounds__(RL_T) void rl_partial_kernel(const float *__restrict__ term_a, const int *__restrict__ flags_a,
                                                          long long Ra, const float *__restrict__ term_b,
                                                          const int *__restrict__ flags_b, long long Rb, Partials p) {
    const int d = blockIdx.y, part = blockIdx.x;
    const float *term = d ? term_b : term_a;
    const int *flags = d ? flags_b : flags_a;
    const long long R = d ? Rb : Ra, chunk = (R + RL_PARTS - 1) / RL_PARTS;
    const long long r0 = part * chunk, r1 = min(R, r0 + chunk);
    double v = 0.0;
    long long c = 0, hh = 0;
    for (long long r = r0 + threadIdx.x; r < r1; r += RL_T) {
        const int f = flags[r];
        if (f & RL_COUNTED) v += (double)term[r], ++c;
        hh += (f & RL_HIT) != 0;
    }
    block_sum3(v, c, hh);
    if (threadIdx.x == 0) p.v[d * RL_PARTS + part] = v, p.n[d * RL_PARTS + part] = c, p.h[d * RL_PARTS + part] = hh;
}

// stats: [0] (l_a + l_b) / 2, [1] l_a, [2] l_b, [3] n_a, [4] n_b, [5] hits_a, [6] hits_b; l = sum / n, 0 without rows
__global__ __launch_bounds__(RL_T) void rl_reduce_kernel(Partials p, float *__restrict__ loss, float *__restrict__ stats) {
    const int t = threadIdx.x;
    double l[2];
    long long n[2], h[2];
    for (int d = 0; d < 2; ++d) {
        double v = p.v[d * RL_PARTS + t];
        long long c = p.n[d * RL_PARTS + t], hh = p.h[d * RL_PARTS + t];
        block_sum3(v, c, hh);
        l[d] = c > 0 ? v / (double)c : 0.0;
        n[d] = c, h[d] = hh;
    }
    if (t == 0) {
        const float la = (float)l[0], lb = (float)l[1];
        *loss = (la + lb) / 2.f;
        stats[0] = *loss, stats[1] = la, stats[2] = lb;
        stats[3] = (float)n[0], stats[4] = (float)n[1], stats[5] = (float)h[0], stats[6] = (float)h[1], stats[7] = 0.f;
    }
}

struct SideIn {
    const float *hat, *xyz, *norm, *lse;
    const int *nn, *flags;
};

// Gradient of the pair's loss with respect to the a features: rows of a, every column of b.  dir_a: index of a's direction
// in stats (0 src, 1 dst).  NJ = C / 64 output channel blocks of 16 per wave.
template <bool NEUTRAL, int NJ>
__global__ __launch_bounds__(RL_T) void rl_backward_kernel(SideIn a, SideIn bs, int M, int N, float itau, float eps2,
                                                           const float *__restrict__ gloss, const float *__restrict__ stats,
                                                           int dir_a, float *__restrict__ grad) {
    constexpr int C = 64 * NJ;
    __shared__ __attribute__((aligned(16))) float smem[RL_SMEM_B];
    __shared__ float cx[3][RL_COLS], clse[RL_COLS], red[4][RL_ROWS];
    __shared__ int cnn[RL_COLS];
    const int b = blockIdx.y, row0 = blockIdx.x * RL_ROWS, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float g = *gloss, na = stats[3 + dir_a], nb = stats[4 - dir_a];
    const float wr = na > 0.f ? g / (2.f * na) : 0.f, wc = nb > 0.f ? g / (2.f * nb) : 0.f;
    int rn[4];   // the row's neighbour where the row counts, else -1
    float rl[4], px[4], py[4], pz[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + i * 16 + (lane & 15), rc = min(r, M - 1);
        const size_t ix = (size_t)b * M + rc;
        rn[i] = r < M && (a.flags[ix] & RL_COUNTED) ? a.nn[ix] : -1;
        rl[i] = a.lse[ix];
        if (NEUTRAL) {
            const float *p = a.xyz + (size_t)b * 3 * M;
            px[i] = p[rc], py[i] = p[M + rc], pz[i] = p[2 * M + rc];
        }
    }
    f32x4 dacc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) dacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *A = a.hat + ((size_t)b * M + row0) * C, *Bb = bs.hat + (size_t)b * N * C;
    float (*dz)[RL_DLD] = reinterpret_cast<float (*)[RL_DLD]>(smem);
    for (int col0 = 0; col0 < N; col0 += RL_COLS) {
        __syncthreads();   // the previous tile's dZ product and column readers are done
        {
            const int c = col0 + t;
            if (c < N) {
                const size_t ix = (size_t)b * N + c;
                cnn[t] = bs.flags[ix] & RL_COUNTED ? bs.nn[ix] : -1;
                clse[t] = bs.lse[ix];
                if (NEUTRAL) {
                    const float *p = bs.xyz + (size_t)b * 3 * N;
                    cx[0][t] = p[c], cx[1][t] = p[N + c], cx[2][t] = p[2 * N + c];
                }
            }
        }
        f32x4 acc[4][4];
        rl_strip_gemm(A, M - row0, Bb + (size_t)col0 * C, N - col0, C, smem, acc);   // ends with a barrier
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row0 + i * 16 + (lane & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float d4[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cl = w * 64 + j * 16 + (lane >> 4) * 4 + q, c = col0 + cl;
                    float d = 0.f;
                    if (c < N && r < M) {
                        const float z = acc[i][j][q] * itau;
                        const bool near = NEUTRAL && dist2(px[i], py[i], pz[i], cx[0][cl], cx[1][cl], cx[2][cl]) <= eps2;
                        if (rn[i] >= 0) {
                            const bool lbl = c == rn[i];
                            const float p = near && !lbl ? 0.f : expf(z - rl[i]);
                            d += wr * (p - (lbl ? 1.f : 0.f));
                        }
                        const int cn = cnn[cl];
                        if (cn >= 0) {
                            const bool lbl = r == cn;
                            const float p = near && !lbl ? 0.f : expf(z - clse[cl]);
                            d += wc * (p - (lbl ? 1.f : 0.f));
                        }
                    }
                    d4[q] = d;
                }
                *reinterpret_cast<float4 *>(&dz[i * 16 + (lane & 15)][w * 64 + j * 16 + (lane >> 4) * 4]) =
                    make_float4(d4[0], d4[1], d4[2], d4[3]);
            }
        }
        __syncthreads();
        // dA[r][ch] += sum_k dZ[r][k] b^[k][ch]: wave w owns channels w*16*NJ .. + 16*NJ
        const int kn = min(RL_COLS, N - col0);
        for (int kk = 0; kk < kn; kk += 4) {
            const int k = min(col0 + kk + (lane >> 4), N - 1);   // dZ is 0 beyond N: any finite row will do
            float bo[NJ], ao[4];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bo[j] = Bb[(size_t)k * C + w * 16 * NJ + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 4; ++i) ao[i] = dz[i * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) dacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bo[j], ao[i], dacc[i][j], 0, 0, 0);
        }
    }
    // normalisation backward: dx = (dx^ - x^ (x^ . dx^)) / norm, or dx^ / eps where the norm was clamped
    float xh[4][NJ][4], dot[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rc = min(row0 + i * 16 + (lane & 15), M - 1);
        float sdot = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float4 v = *reinterpret_cast<const float4 *>(a.hat + ((size_t)b * M + rc) * C + w * 16 * NJ + j * 16 + (lane >> 4) * 4);
            xh[i][j][0] = v.x, xh[i][j][1] = v.y, xh[i][j][2] = v.z, xh[i][j][3] = v.w;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dacc[i][j][q] *= itau;
                sdot += xh[i][j][q] * dacc[i][j][q];
            }
        }
        sdot += __shfl_xor(sdot, 16, 64);
        sdot += __shfl_xor(sdot, 32, 64);
        if (lane < 16) red[w][i * 16 + lane] = sdot;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rr = i * 16 + (lane & 15);
        dot[i] = (red[0][rr] + red[1][rr]) + (red[2][rr] + red[3][rr]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + i * 16 + (lane & 15);
        if (r >= M) continue;
        const float n = a.norm[(size_t)b * M + r];
        const bool clamped = !(n >= RL_NORM_EPS);
        const float inv = 1.f / (clamped ? RL_NORM_EPS : n);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ch = w * 16 * NJ + j * 16 + (lane >> 4) * 4 + q;
                const float dx = clamped ? dacc[i][j][q] : dacc[i][j][q] - xh[i][j][q] * dot[i];
                grad[((size_t)b * C + ch) * M + r] = dx * inv;
            }
    }
}

struct Ws {
    float *hat_a, *hat_b, *norm_a, *norm_b, *lse_a, *lse_b, *term_a, *term_b;
    int *flags_a, *flags_b;
    Partials part;
};

Ws layout(WsCursor &c, int B, int M, int N, int C) {
    const size_t ra = (size_t)B * M, rb = (size_t)B * N;
    Ws w;
    w.hat_a = c.take256<float>(ra * C), w.hat_b = c.take256<float>(rb * C);
    w.norm_a = c.take256<float>(ra), w.norm_b = c.take256<float>(rb);
    w.lse_a = c.take256<float>(ra), w.lse_b = c.take256<float>(rb);
    w.term_a = c.take256<float>(ra), w.term_b = c.take256<float>(rb);
    w.flags_a = c.take256<int>(ra), w.flags_b = c.take256<int>(rb);
    w.part.v = c.take256<double>(2 * RL_PARTS), w.part.n = c.take256<long long>(2 * RL_PARTS);
    w.part.h = c.take256<long long>(2 * RL_PARTS);
    return w;
}
bool shape_ok(int B, int M, int N, int C) { return B >= 1 && M >= 1 && N >= 1 && C >= 1 && B <= 65535; }

float threshold(double eps) { return (float)(eps * eps); }   // torch compares an fp32 tensor with the scalar rounded to fp32

}  // namespace

extern "C" int dpm_reg_loss_pairs(const float *xyz_a, const float *xyz_b, int B, int M, int N, double eps, int32_t *nn_a,
                                  int32_t *nn_b, int32_t *neutral_a, int32_t *neutral_b, dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz_a && xyz_b && nn_a && nn_b && shape_ok(B, M, N, 1) && eps >= 0.0);
    hipStream_t st = (hipStream_t)stream;
    const float e2 = threshold(eps);
    hipLaunchKernelGGL(rl_pairs_kernel, dim3(dpm_cdiv(M, RL_T), B), dim3(RL_T), 0, st, xyz_a, xyz_b, M, N, e2, nn_a, neutral_a);
    hipLaunchKernelGGL(rl_pairs_kernel, dim3(dpm_cdiv(N, RL_T), B), dim3(RL_T), 0, st, xyz_b, xyz_a, N, M, e2, nn_b, neutral_b);
    return dpm_launch_status();
}

extern "C" size_t dpm_reg_loss_workspace_bytes(int B, int M, int N, int C) {
    if (!shape_ok(B, M, N, C)) return 0;
    WsCursor c(nullptr);
    layout(c, B, M, N, C);
    return c.bytes();
}

static bool reg_loss_channels(int C) { return C == 64 || C == 128 || C == 192 || C == 256; }

extern "C" int dpm_reg_loss_forward(const float *fea_a, const float *fea_b, const float *xyz_a, const float *xyz_b,
                                    const uint8_t *pad_a, const uint8_t *pad_b, const int32_t *nn_a, const int32_t *nn_b, int B,
                                    int M, int N, int C, double tau, double eps, int neutral, int32_t *argmax_a,
                                    int32_t *argmax_b, float *loss, float *stats, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(fea_a && fea_b && pad_a && pad_b && nn_a && nn_b && loss && stats && workspace && shape_ok(B, M, N, C));
    DPM_CHECK_ARG(tau > 0.0 && eps >= 0.0 && (!neutral || (xyz_a && xyz_b)));
    if (!reg_loss_channels(C)) return DPM_EUNSUPPORTED;
    WsCursor c(workspace);
    const Ws ws = layout(c, B, M, N, C);
    hipStream_t st = (hipStream_t)stream;
    const float itau = 1.0f / (float)tau, e2 = threshold(eps);
    hipLaunchKernelGGL(rl_prep_kernel, dim3(dpm_cdiv(M, 64), B), dim3(RL_T), 0, st, fea_a, M, C, ws.hat_a, ws.norm_a);
    hipLaunchKernelGGL(rl_prep_kernel, dim3(dpm_cdiv(N, 64), B), dim3(RL_T), 0, st, fea_b, N, C, ws.hat_b, ws.norm_b);
    const RowOut oa{ws.lse_a, ws.term_a, ws.flags_a, argmax_a}, ob{ws.lse_b, ws.term_b, ws.flags_b, argmax_b};
    if (neutral) {
        hipLaunchKernelGGL(rl_forward_kernel<true>, dim3(dpm_cdiv(M, RL_ROWS), B), dim3(RL_T), 0, st, ws.hat_a, ws.hat_b, xyz_a,
                           xyz_b, pad_a, nn_a, M, N, C, itau, e2, oa);
        hipLaunchKernelGGL(rl_forward_kernel<true>, dim3(dpm_cdiv(N, RL_ROWS), B), dim3(RL_T), 0, st, ws.hat_b, ws.hat_a, xyz_b,
                           xyz_a, pad_b, nn_b, N, M, C, itau, e2, ob);
    } else {
        hipLaunchKernelGGL(rl_forward_kernel<false>, dim3(dpm_cdiv(M, RL_ROWS), B), dim3(RL_T), 0, st, ws.hat_a, ws.hat_b, xyz_a,
                           xyz_b, pad_a, nn_a, M, N, C, itau, e2, oa);
        hipLaunchKernelGGL(rl_forward_kernel<false>, dim3(dpm_cdiv(N, RL_ROWS), B), dim3(RL_T), 0, st, ws.hat_b, ws.hat_a, xyz_b,
                           xyz_a, pad_b, nn_b, N, M, C, itau, e2, ob);
    }
    hipLaunchKernelGGL(rl_partial_kernel, dim3(RL_PARTS, 2), dim3(RL_T), 0, st, ws.term_a, ws.flags_a, (long long)B * M,
                       ws.term_b, ws.flags_b, (long long)B * N, ws.part);
    hipLaunchKernelGGL(rl_reduce_kernel, dim3(1), dim3(RL_T), 0, st, ws.part, loss, stats);
    return dpm_launch_status();
}

template <int NJ>
static void launch_backward(bool neutral, const SideIn &a, const SideIn &b, int B, int M, int N, float itau, float e2,
                            const float *g, const float *stats, int dir_a, float *grad, hipStream_t st) {
    if (neutral)
        hipLaunchKernelGGL((rl_backward_kernel<true, NJ>), dim3(dpm_cdiv(M, RL_ROWS), B), dim3(RL_T), 0, st, a, b, M, N, itau, e2,
                           g, stats, dir_a, grad);
    else
        hipLaunchKernelGGL((rl_backward_kernel<false, NJ>), dim3(dpm_cdiv(M, RL_ROWS), B), dim3(RL_T), 0, st, a, b, M, N, itau,
                           e2, g, stats, dir_a, grad);
}

extern "C" int dpm_reg_loss_backward(const float *xyz_a, const float *xyz_b, const int32_t *nn_a, const int32_t *nn_b, int B,
                                     int M, int N, int C, double tau, double eps, int neutral, const float *grad_loss,
                                     const float *stats, const void *workspace, float *grad_a, float *grad_b,
                                     dpm_stream_t stream) {
    DPM_CHECK_ARG(nn_a && nn_b && grad_loss && stats && workspace && grad_a && grad_b && shape_ok(B, M, N, C));
    DPM_CHECK_ARG(tau > 0.0 && eps >= 0.0 && (!neutral || (xyz_a && xyz_b)));
    if (!reg_loss_channels(C)) return DPM_EUNSUPPORTED;
    WsCursor c(const_cast<void *>(workspace));
    const Ws ws = layout(c, B, M, N, C);
    hipStream_t st = (hipStream_t)stream;
    const float itau = 1.0f / (float)tau, e2 = threshold(eps);
    const SideIn sa{ws.hat_a, xyz_a, ws.norm_a, ws.lse_a, nn_a, ws.flags_a}, sb{ws.hat_b, xyz_b, ws.norm_b, ws.lse_b, nn_b, ws.flags_b};
    auto run = [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        launch_backward<NJ>(neutral, sa, sb, B, M, N, itau, e2, grad_loss, stats, 0, grad_a, st);   // row sweep
        launch_backward<NJ>(neutral, sb, sa, B, N, M, itau, e2, grad_loss, stats, 1, grad_b, st);   // column sweep
    };
    switch (C) {
    case 64: run(std::integral_constant<int, 1>{}); break;
    case 128: run(std::integral_constant<int, 2>{}); break;
    case 192: run(std::integral_constant<int, 3>{}); break;
    default: run(std::integral_constant<int, 4>{}); break;
    }
    return dpm_launch_status();
}
