// The grouping layer of the encoder for TRAINING (pointnext.py:52-61, 97-107 and what autograd does with them):
//   out[b,s,c] = max_k relu(LN_c(P[b, idx[b,s,k], :] + W_rel (xyz[idx] - centre) / radius)),   P = fea W_f^T + b by the caller,
// forward with the winning slot per (b,s,c), and a backward that produces dP, dW_rel, dgamma, dbeta without a (B,S,K,Cout)
// tensor and without floating-point atomics.
//
// Lane layout (both directions, as csrc/group_mlp.hip): G = Cout / (4 V) lanes share a row of Cout channels, a float4 (V = 1) or
// two (Cout = 512) per lane; a wave holds RPW = 64 / G rows at a time; LayerNorm's sums are butterflies inside the lane group.
//
// Backward.  A channel routes its gradient to the winning (s,k) row only, but LayerNorm couples the channels of a row: dh of a row
// with at least one winner is dense.  Rows are regrouped by the POINT they gathered -- the inverse of idx, built per call:
//   mask[s]      = the set of k that win some channel of centre s                     (row_mask_kernel)
//   count[j]     = number of winning rows (s,k) with idx[s,k] = j                      (count_kernel, integer atomics)
//   offsets      = exclusive scan of count                                            (scan_kernel)
//   lists        = the rows of each point, filled in arrival order                     (fill_kernel, integer atomics)
//   entries      = each list sorted by s * K + k (rank = number of smaller keys)       (rank_kernel): the order is a function of
//                  idx and the slots alone, whatever order the atomics ran in
// and ONE kernel walks every point's list in that order: it recomputes the pre-norm row and its statistics from P[j] (loaded once
// per point), forms dh, accumulates dP[j] in registers (one writer per row: points nobody gathered and padding points get exact
// zeros) and keeps per-lane partial sums of dgamma, dbeta and dW_rel.  Those leave the kernel as one partial per wave, and
// reduce_kernel adds the partials in wave order.  Which points a wave owns depends on the shapes only, so two runs give identical
// bytes.
//
// idx entries outside [0, N) are read as clamped, min(max(idx, 0), N - 1), in every kernel that reads idx, as the inference
// kernels do.  Rows of P and xyz that idx never names are loaded by the backward (every point's row is) but enter no result: they
// may hold anything, NaN included.
#include "dpm_common.h"
#include "workspace.h"

namespace {

template <int COUT>
struct Lay {
    static constexpr int V = COUT == 512 ? 2 : 1;    // float4 per lane
    static constexpr int G = COUT / (4 * V);         // lanes per row
    static constexpr int RPW = 64 / G;               // rows per wave
};

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);   // a + b == b + a bit for bit: every lane of the group ends equal
    return v;
}

// pre-norm row -> normalised row n = (h - mean) * rs and rs = 1 / sqrt(var + eps); wr carries 1 / radius
template <int COUT>
__device__ __forceinline__ void norm_row(const float4 (&p)[Lay<COUT>::V], const float (&wr)[Lay<COUT>::V][4][3], float rx, float ry,
                                         float rz, float (&n)[Lay<COUT>::V][4], float &rs) {
    constexpr int V = Lay<COUT>::V, G = Lay<COUT>::G;
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        n[v][0] = fmaf(wr[v][0][2], rz, fmaf(wr[v][0][1], ry, fmaf(wr[v][0][0], rx, p[v].x)));
        n[v][1] = fmaf(wr[v][1][2], rz, fmaf(wr[v][1][1], ry, fmaf(wr[v][1][0], rx, p[v].y)));
        n[v][2] = fmaf(wr[v][2][2], rz, fmaf(wr[v][2][1], ry, fmaf(wr[v][2][0], rx, p[v].z)));
        n[v][3] = fmaf(wr[v][3][2], rz, fmaf(wr[v][3][1], ry, fmaf(wr[v][3][0], rx, p[v].w)));
        sum += (n[v][0] + n[v][1]) + (n[v][2] + n[v][3]);
    }
    const float mean = group_sum<G>(sum) * (1.0f / (float)COUT);
    float sq = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            n[v][e] -= mean;
            sq = fmaf(n[v][e], n[v][e], sq);
        }
    rs = __builtin_amdgcn_rsqf(group_sum<G>(sq) * (1.0f / (float)COUT) + 1e-5f);   // var + eps >= 1e-5: a normal number
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) n[v][e] *= rs;
}

template <int COUT>
__device__ __forceinline__ void load_rel_weights(const float *__restrict__ Wr, int ldwr, float inv_r, int gl,
                                                 float (&wr)[Lay<COUT>::V][4][3]) {
#pragma unroll
    for (int v = 0; v < Lay<COUT>::V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int d = 0; d < 3; ++d) wr[v][e][d] = Wr[(size_t)(4 * (gl + Lay<COUT>::G * v) + e) * ldwr + d] * inv_r;
}

// ---- forward: one wave per centre; out and the winning slot (255: no neighbour above the ReLU floor) -----------------------------
template <int COUT>
__global__ __launch_bounds__(256) void group_train_fwd_kernel(
    const float *__restrict__ P_all, const float *__restrict__ xyz_all, const float *__restrict__ ctr_all,
    const int32_t *__restrict__ idx_all, const float *__restrict__ Wr, int ldwr, const float *__restrict__ gamma,
    const float *__restrict__ beta, int N, int S, int K, long long total, float inv_r, float *__restrict__ out_all,
    uint8_t *__restrict__ slot_all) {
    constexpr int V = Lay<COUT>::V, G = Lay<COUT>::G, RPW = Lay<COUT>::RPW;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gl = lane % G, gr = lane / G;
    const long long cc = (long long)blockIdx.x * 4 + w;
    if (cc >= total) return;   // whole waves leave: no block barrier below
    float wr[V][4][3], gm[V][4], bt[V][4];
    load_rel_weights<COUT>(Wr, ldwr, inv_r, gl, wr);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) gm[v][e] = gamma[4 * (gl + G * v) + e], bt[v][e] = beta[4 * (gl + G * v) + e];
    const int b = (int)(cc / S);
    const float *P = P_all + (size_t)b * N * COUT, *xyz = xyz_all + (size_t)b * N * 3;
    const int32_t *idx = idx_all + (size_t)cc * K;
    const float cx = ctr_all[(size_t)cc * 3], cy = ctr_all[(size_t)cc * 3 + 1], cz = ctr_all[(size_t)cc * 3 + 2];
    float mx[V][4];
    int sl[V][4];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) mx[v][e] = 0.f, sl[v][e] = 255;   // the ReLU floor wins until a row exceeds it
    for (int r0 = 0; r0 < K; r0 += RPW) {   // K is a multiple of RPW (host check)
        const int k = r0 + gr;
        const int j = min(max(idx[k], 0), N - 1);
        const float rx = xyz[(size_t)j * 3] - cx, ry = xyz[(size_t)j * 3 + 1] - cy, rz = xyz[(size_t)j * 3 + 2] - cz;
        float4 p[V];
#pragma unroll
        for (int v = 0; v < V; ++v) p[v] = *reinterpret_cast<const float4 *>(P + (size_t)j * COUT + 4 * (gl + G * v));
        float n[V][4], rs;
        norm_row<COUT>(p, wr, rx, ry, rz, n, rs);
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = fmaf(n[v][e], gm[v][e], bt[v][e]);
                if (y > mx[v][e]) mx[v][e] = y, sl[v][e] = k;   // strict: the earliest slot keeps a tie
            }
    }
    // the row groups of the wave (equal gl): larger value, then smaller slot -- symmetric, so all of them end equal
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int off = G; off < 64; off <<= 1) {
                const float om = __shfl_xor(mx[v][e], off, 64);
                const int os = __shfl_xor(sl[v][e], off, 64);
                if (om > mx[v][e] || (om == mx[v][e] && os < sl[v][e])) mx[v][e] = om, sl[v][e] = os;
            }
    if (gr == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const size_t o = (size_t)cc * COUT + 4 * (gl + G * v);
            *reinterpret_cast<float4 *>(out_all + o) = make_float4(mx[v][0], mx[v][1], mx[v][2], mx[v][3]);
            *reinterpret_cast<uint32_t *>(slot_all + o) =
                (uint32_t)sl[v][0] | ((uint32_t)sl[v][1] << 8) | ((uint32_t)sl[v][2] << 16) | ((uint32_t)sl[v][3] << 24);
        }
    }
}

// ---- the inverse of idx over the rows that hold a winner ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_mask_kernel(const uint8_t *__restrict__ slot_all, long long total, int words,
                                                       uint32_t *__restrict__ mask) {
    const long long cc = (long long)blockIdx.x * 256 + threadIdx.x;
    if (cc >= total) return;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(slot_all) + (size_t)cc * words;
    uint32_t m = 0;
    for (int i = 0; i < words; ++i) {
        const uint32_t q = sw[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t s = (q >> (8 * e)) & 255u;
            if (s < 32u) m |= 1u << s;
        }
    }
    mask[cc] = m;
}

// FILL = false: count[point] += 1 per winning row; FILL = true: the row's key s * K + k goes to the point's list
template <bool FILL>
__global__ __launch_bounds__(256) void invert_kernel(const int32_t *__restrict__ idx_all, const uint32_t *__restrict__ mask, int N,
                                                     int S, int kshift, long long rows, int32_t *__restrict__ cursor,
                                                     int32_t *__restrict__ lists) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;   // r = (b * S + s) * K + k
    if (r >= rows) return;
    const long long cc = r >> kshift;
    const int k = (int)(r & ((1 << kshift) - 1));
    if (!((mask[cc] >> k) & 1u)) return;
    const int b = (int)(cc / S), s = (int)(cc - (long long)b * S);
    const int j = min(max(idx_all[r], 0), N - 1);
    const int pos = atomicAdd(cursor + (size_t)b * N + j, 1);
    if (FILL) lists[pos] = (s << kshift) | k;
}

// exclusive scan of count[0..n) -> offsets[0..n] and a copy in cursor[0..n) (the fill's running positions); one block
__global__ __launch_bounds__(1024) void scan_kernel(int32_t *__restrict__ cursor, int32_t *__restrict__ offsets, long long n) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const long long chunk = (n + 1023) / 1024, lo = min((long long)t * chunk, n), hi = min(lo + chunk, n);
    int sum = 0;
    for (long long i = lo; i < hi; ++i) sum += cursor[i];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // inclusive scan of the per-thread totals
        const int add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (long long i = lo; i < hi; ++i) {
        const int c = cursor[i];
        offsets[i] = run, cursor[i] = run;
        run += c;
    }
    if (t == 1023) offsets[n] = part[1023];
}

// stable order inside every list: an entry's place is the number of smaller keys of its list (keys are distinct)
__global__ __launch_bounds__(256) void rank_kernel(const int32_t *__restrict__ idx_all, const uint32_t *__restrict__ mask, int N,
                                                   int S, int kshift, long long rows, const int32_t *__restrict__ offsets,
                                                   const int32_t *__restrict__ lists, int32_t *__restrict__ entries) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const long long cc = r >> kshift;
    const int k = (int)(r & ((1 << kshift) - 1));
    if (!((mask[cc] >> k) & 1u)) return;
    const int b = (int)(cc / S), s = (int)(cc - (long long)b * S);
    const int j = min(max(idx_all[r], 0), N - 1);
    const int beg = offsets[(size_t)b * N + j], end = offsets[(size_t)b * N + j + 1], key = (s << kshift) | k;
    int rank = 0;
    for (int i = beg; i < end; ++i) rank += lists[i] < key;
    entries[beg + rank] = key;
}

// ---- backward: point-major ---------------------------------------------------------------------------------------------------------
// partial: (waves, 5, COUT) = per wave [dgamma ; dbeta ; sum dh rel_x ; sum dh rel_y ; sum dh rel_z] (rel without 1 / radius)
template <int COUT>
__global__ __launch_bounds__(256) void group_train_bwd_kernel(
    const float *__restrict__ P_all, const float *__restrict__ xyz_all, const float *__restrict__ ctr_all,
    const float *__restrict__ Wr, int ldwr, const float *__restrict__ gamma, int N, int S, int kshift, float inv_r,
    const float *__restrict__ dout_all, const uint8_t *__restrict__ slot_all, const int32_t *__restrict__ offsets,
    const int32_t *__restrict__ entries, long long points, int ppw, int waves, float *__restrict__ dP_all,
    float *__restrict__ partial) {
    constexpr int V = Lay<COUT>::V, G = Lay<COUT>::G, RPW = Lay<COUT>::RPW;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gl = lane % G, gr = lane / G;
    const int gw = blockIdx.x * 4 + w;
    if (gw >= waves) return;   // whole waves leave: no block barrier below
    float wr[V][4][3], gm[V][4];
    load_rel_weights<COUT>(Wr, ldwr, inv_r, gl, wr);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) gm[v][e] = gamma[4 * (gl + G * v) + e];
    float dg[V][4], db[V][4], dw[V][4][3];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) dg[v][e] = db[v][e] = dw[v][e][0] = dw[v][e][1] = dw[v][e][2] = 0.f;
    const int kmask = (1 << kshift) - 1;
    for (int t = 0; t < ppw; ++t) {
        const long long pt = ((long long)gw * ppw + t) * RPW + gr;   // this lane group's point (b * N + j)
        const bool live = pt < points;
        const long long pc = live ? pt : points - 1;
        const int b = (int)(pc / N);
        const int beg = live ? offsets[pc] : 0, len = live ? offsets[pc + 1] - beg : 0;
        const int maxlen = wave_reduce(len, [](int a, int b) { return max(a, b); });
        float4 p[V];
#pragma unroll
        for (int v = 0; v < V; ++v) p[v] = *reinterpret_cast<const float4 *>(P_all + (size_t)pc * COUT + 4 * (gl + G * v));
        const float px = xyz_all[(size_t)pc * 3], py = xyz_all[(size_t)pc * 3 + 1], pz = xyz_all[(size_t)pc * 3 + 2];
        float dp[V][4];
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) dp[v][e] = 0.f;
        for (int i = 0; i < maxlen; ++i) {   // wave-uniform trip count: the butterflies below run with every lane present
            const bool act = i < len;
            const int key = act ? entries[beg + i] : 0;
            const int s = key >> kshift, k = key & kmask;
            const size_t cs = (size_t)b * S + s;
            const float rx = px - ctr_all[cs * 3], ry = py - ctr_all[cs * 3 + 1], rz = pz - ctr_all[cs * 3 + 2];
            float n[V][4], rs;
            norm_row<COUT>(p, wr, rx, ry, rz, n, rs);
            float dy[V][4], dn[V][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const size_t o = cs * COUT + 4 * (gl + G * v);
                const uint32_t q = *reinterpret_cast<const uint32_t *>(slot_all + o);
                const float4 d4 = *reinterpret_cast<const float4 *>(dout_all + o);
                const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dy[v][e] = (act && (int)((q >> (8 * e)) & 255u) == k) ? d[e] : 0.f;
                    dn[v][e] = dy[v][e] * gm[v][e];
                    s1 += dn[v][e];
                    s2 = fmaf(dn[v][e], n[v][e], s2);
                }
            }
            const float m1 = group_sum<G>(s1) * (1.0f / (float)COUT), m2 = group_sum<G>(s2) * (1.0f / (float)COUT);
            if (act) {
#pragma unroll
                for (int v = 0; v < V; ++v)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float dh = rs * ((dn[v][e] - m1) - n[v][e] * m2);
                        dp[v][e] += dh;
                        dg[v][e] = fmaf(dy[v][e], n[v][e], dg[v][e]);
                        db[v][e] += dy[v][e];
                        dw[v][e][0] = fmaf(dh, rx, dw[v][e][0]);
                        dw[v][e][1] = fmaf(dh, ry, dw[v][e][1]);
                        dw[v][e][2] = fmaf(dh, rz, dw[v][e][2]);
                    }
            }
        }
        if (live) {
#pragma unroll
            for (int v = 0; v < V; ++v)
                *reinterpret_cast<float4 *>(dP_all + (size_t)pt * COUT + 4 * (gl + G * v)) =
                    make_float4(dp[v][0], dp[v][1], dp[v][2], dp[v][3]);
        }
    }
    // the wave's partial: the lane groups added in butterfly order, written by the first
    float *out = partial + (size_t)gw * 5 * COUT;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float q[5] = {dg[v][e], db[v][e], dw[v][e][0], dw[v][e][1], dw[v][e][2]};
#pragma unroll
            for (int i = 0; i < 5; ++i) {
#pragma unroll
                for (int off = G; off < 64; off <<= 1) q[i] += __shfl_xor(q[i], off, 64);
                if (gr == 0) out[i * COUT + 4 * (gl + G * v) + e] = q[i];
            }
        }
}

// partials added in wave order: thread (i, c) of 5 x Cout
__global__ __launch_bounds__(256) void group_train_reduce_kernel(const float *__restrict__ partial, int waves, int Cout, float inv_r,
                                                                 float *__restrict__ dWr, float *__restrict__ dgamma,
                                                                 float *__restrict__ dbeta) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 5 * Cout) return;
    float acc = 0.f;
    for (int g = 0; g < waves; ++g) acc += partial[(size_t)g * 5 * Cout + t];
    const int i = t / Cout, c = t - i * Cout;
    if (i == 0) dgamma[c] = acc;
    else if (i == 1) dbeta[c] = acc;
    else dWr[c * 3 + (i - 2)] = acc * inv_r;
}

struct Plan {
    int rpw, ppw, waves;
    uint32_t *mask;
    int32_t *cursor, *offsets, *lists, *entries;
    float *partial;
};

// the launch plan and, through the cursor, the workspace layout (the base is taken as given: the caller's 16-byte alignment)
bool make_plan(WsCursor &c, int B, int N, int S, int K, int Cout, Plan &p) {
    if (!(Cout == 32 || Cout == 64 || Cout == 128 || Cout == 256 || Cout == 512) || !(K == 16 || K == 32)) return false;
    const long long points = (long long)B * N, rows = (long long)B * S * K;
    if (B < 1 || N < 1 || S < 1 || points >= (1LL << 30) || rows >= (1LL << 31) || (long long)S * K >= (1LL << 31)) return false;
    const int V = Cout == 512 ? 2 : 1;
    p.rpw = 64 / (Cout / (4 * V));
    const long long groups = (points + p.rpw - 1) / p.rpw;
    const long long cap = 131072 / Cout > 256 ? 131072 / Cout : 256;   // the partials stay at 2.5 MiB whatever the width
    p.ppw = (int)((groups + cap - 1) / cap);
    p.waves = (int)((groups + p.ppw - 1) / p.ppw);
    p.mask = c.take256<uint32_t>((size_t)B * S);
    p.cursor = c.take256<int32_t>((size_t)points);
    p.offsets = c.take256<int32_t>((size_t)points + 1);
    p.lists = c.take256<int32_t>((size_t)rows);
    p.entries = c.take256<int32_t>((size_t)rows);
    p.partial = c.take256<float>((size_t)p.waves * 5 * Cout);
    return true;
}

}  // namespace

extern "C" int dpm_group_train_forward(const float *P, const float *xyz, const float *centers, const int32_t *idx,
                                       const float *W_rel, int ldw_rel, const float *gamma, const float *beta, int B, int N,
                                       int S, int K, int Cout, double radius, float *out, uint8_t *slots, dpm_stream_t stream) {
    DPM_CHECK_ARG(P && xyz && centers && idx && W_rel && gamma && beta && out && slots);
    DPM_CHECK_ARG(B >= 1 && N >= 1 && S >= 1 && K >= 1 && ldw_rel >= 3 && radius > 0.0);
    DPM_CHECK_ARG(((uintptr_t)P & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)slots & 3) == 0);
    Plan pl;
    WsCursor none(nullptr, false);   // the forward has no workspace: the plan only says whether the shape is supported
    if (!make_plan(none, B, N, S, K, Cout, pl)) return DPM_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * S;
    const float inv_r = 1.0f / (float)radius;
#define DPM_GT(C)                                                                                                               \
    hipLaunchKernelGGL((group_train_fwd_kernel<C>), dim3(dpm_cdiv(total, 4)), dim3(256), 0, st, P, xyz, centers, idx, W_rel,   \
                       ldw_rel, gamma, beta, N, S, K, total, inv_r, out, slots);                                                \
    break
    switch (Cout) {
        case 32: DPM_GT(32);
        case 64: DPM_GT(64);
        case 128: DPM_GT(128);
        case 256: DPM_GT(256);
        default: DPM_GT(512);
    }
#undef DPM_GT
    return dpm_launch_status();
}

extern "C" size_t dpm_group_train_workspace_bytes(int B, int N, int S, int K, int Cout) {
    Plan pl;
    WsCursor c(nullptr, false);
    return make_plan(c, B, N, S, K, Cout, pl) ? c.bytes() : 0;
}

extern "C" int dpm_group_train_backward(const float *P, const float *xyz, const float *centers, const int32_t *idx,
                                        const float *W_rel, int ldw_rel, const float *gamma, int B, int N, int S, int K, int Cout,
                                        double radius, const float *dout, const uint8_t *slots, float *dP, float *dW_rel,
                                        float *dgamma, float *dbeta, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(P && xyz && centers && idx && W_rel && gamma && dout && slots && dP && dW_rel && dgamma && dbeta && workspace);
    DPM_CHECK_ARG(B >= 1 && N >= 1 && S >= 1 && K >= 1 && ldw_rel >= 3 && radius > 0.0);
    DPM_CHECK_ARG(((uintptr_t)P & 15) == 0 && ((uintptr_t)dout & 15) == 0 && ((uintptr_t)dP & 15) == 0 &&
                  ((uintptr_t)slots & 3) == 0 && ((uintptr_t)workspace & 15) == 0);
    Plan pl;
    WsCursor c(workspace, false);
    if (!make_plan(c, B, N, S, K, Cout, pl)) return DPM_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *mask = pl.mask;
    int32_t *cursor = pl.cursor, *offsets = pl.offsets, *lists = pl.lists, *entries = pl.entries;
    float *partial = pl.partial;
    const long long total = (long long)B * S, points = (long long)B * N, rows = total * K;
    const int kshift = K == 16 ? 4 : 5;
    const float inv_r = 1.0f / (float)radius;
    if (hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)points, st) != hipSuccess) return dpm_launch_status();
    hipLaunchKernelGGL(row_mask_kernel, dim3(dpm_cdiv(total, 256)), dim3(256), 0, st, slots, total, Cout / 4, mask);
    hipLaunchKernelGGL(invert_kernel<false>, dim3(dpm_cdiv(rows, 256)), dim3(256), 0, st, idx, mask, N, S, kshift, rows, cursor,
                       lists);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, cursor, offsets, points);
    hipLaunchKernelGGL(invert_kernel<true>, dim3(dpm_cdiv(rows, 256)), dim3(256), 0, st, idx, mask, N, S, kshift, rows, cursor,
                       lists);
    hipLaunchKernelGGL(rank_kernel, dim3(dpm_cdiv(rows, 256)), dim3(256), 0, st, idx, mask, N, S, kshift, rows, offsets, lists,
                       entries);
#define DPM_GT(C)                                                                                                                \
    hipLaunchKernelGGL((group_train_bwd_kernel<C>), dim3(dpm_cdiv(pl.waves, 4)), dim3(256), 0, st, P, xyz, centers, W_rel, ldw_rel, \
                       gamma, N, S, kshift, inv_r, dout, slots, offsets, entries, points, pl.ppw, pl.waves, dP, partial);         \
    break
    switch (Cout) {
        case 32: DPM_GT(32);
        case 64: DPM_GT(64);
        case 128: DPM_GT(128);
        case 256: DPM_GT(256);
        default: DPM_GT(512);
    }
#undef DPM_GT
    hipLaunchKernelGGL(group_train_reduce_kernel, dim3(dpm_cdiv(5 * Cout, 256)), dim3(256), 0, st, partial, pl.waves, Cout, inv_r,
                       dW_rel, dgamma, dbeta);
    return dpm_launch_status();
}
