// The optimiser step of a whole parameter group in one launch (AdamW, Adam, SGD; torch.optim's single-tensor update rules,
// torch/optim/adam.py `_single_tensor_adam`, torch/optim/sgd.py `_single_tensor_sgd`).  The reference trains 192 tensors
// (110 encoder + 82 decoder) with torch.optim.AdamW (pipeline/modules/utils.py:86-100), which walks them one by one or in
// foreach lists; here two tables in device memory describe the group and one grid covers all of it:
//   tensors (T,5) int64   [param, grad, state0, state1, numel]: addresses of fp32 arrays (state0 = exp_avg / momentum_buffer,
//                         state1 = exp_avg_sq; 0 where the algorithm has none)
//   chunks  (K,2) int32   [tensor, chunk]: block k updates elements [chunk * CHUNK, min(numel, (chunk + 1) * CHUNK)) of its tensor
// The tables change only when an address does; the step's scalars (lr from param_groups, bias corrections) are kernel arguments
// computed in double on the host, as torch computes them, and rounded to fp32 once.
//
// The update is element-wise: no element depends on how the group is cut into tensors or chunks.  A tensor whose four
// addresses are all 16-byte aligned moves as float4 (chunks start at multiples of CHUNK, so every chunk of it is aligned too);
// any other tensor -- a view at an odd offset -- takes the scalar path.  Both paths run the same expression per element.
//
// Rounding order per element (-ffp-contract=off; every fusion is written out):
//   AdamW   p = p * (float)(1 - lr wd)                                   torch: param.mul_(1 - lr * weight_decay)
//   Adam    g = fmaf(wd, p, g)                                           torch: grad.add(param, alpha=weight_decay)
//   both    m = fmaf(g - m, (float)(1 - beta1), m)                       torch: exp_avg.lerp_(grad, 1 - beta1)
//           v = fmaf((float)(1 - beta2) * g, g, v * beta2)               torch: exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
//           p = fmaf(-(float)(lr / (1 - beta1^t)), m / (sqrtf(v) / (float)sqrt(1 - beta2^t) + eps), p)       torch: addcdiv_
//   SGD     g = fmaf(wd, p, g);  buf = first ? g : fmaf(g, (float)(1 - dampening), buf * momentum)
//           g = nesterov ? fmaf(momentum, buf, g) : buf;  p = fmaf(-lr, g, p)
// Division and square root are IEEE-rounded.
//
// Data-parallel training (deeppointmap_amd/data_parallel.py; the reference wraps its model in DistributedDataParallel,
// pipeline/modules/trainer.py:239-243) adds two kernels over the same two-table scheme:
//   flat_copy_kernel           every gradient of a stage into ONE flat fp32 buffer (pack), or the buffer back into the tensors
//                              (unpack, the initial broadcast of parameters); table (T,3) int64 [address, offset, numel]
//   optim_step_synced_kernel   the update above with g read from `n_slices` copies of that buffer (one per rank, `slice_stride`
//                              elements apart) instead of a gradient tensor: g = slice_0[i]; g = g + slice_r[i] for r = 1 ..
//                              n_slices - 1, in that order; g = g / divisor (a true division: W = 3, 5, 6, 7 are defined like
//                              the powers of two) -- and then the very same Rule functor, so every rule is stated once.
// The synced kernel streams n_slices + 3 reads and 3 writes per element (AdamW).  A thread issues the float4 loads of up to
// SLICE_BATCH = 8 slices back to back before the first add -- 8 KiB per wave in flight, at 7 waves per SIMD far above the ~32 KiB
// per CU at which the HBM streams at its rate -- while the sum itself stays sequential in rank order.
#include "dpm_common.h"

namespace {

constexpr int CHUNK = 4096;   // elements per block: 256 threads x 4 float4

struct AdamArgs {
    float decay;       // AdamW: 1 - lr wd (1 = none); Adam: wd
    float w1, beta2, w2, neg_step_size, bc2_sqrt, eps;
};
struct SgdArgs {
    float wd, momentum, w_damp, neg_lr;
    int has_buf, first, nesterov;
};

template <bool DECOUPLED>
struct AdamRule {
    AdamArgs a;
    __device__ __forceinline__ void operator()(float &p, float g, float &m, float &v) const {
        if (DECOUPLED) {
            if (a.decay != 1.f) p = p * a.decay;
        } else if (a.decay != 0.f) {
            g = fmaf(a.decay, p, g);
        }
        m = fmaf(g - m, a.w1, m);
        v = fmaf(a.w2 * g, g, v * a.beta2);
        p = fmaf(a.neg_step_size, m / (sqrtf(v) / a.bc2_sqrt + a.eps), p);
    }
    static constexpr int STATES = 2;
};

struct SgdRule {
    SgdArgs a;
    __device__ __forceinline__ void operator()(float &p, float g, float &buf, float &) const {
        if (a.wd != 0.f) g = fmaf(a.wd, p, g);
        if (a.has_buf) {
            buf = a.first ? g : fmaf(g, a.w_damp, buf * a.momentum);
            g = a.nesterov ? fmaf(a.momentum, buf, g) : buf;
        }
        p = fmaf(a.neg_lr, g, p);
    }
    static constexpr int STATES = 1;   // read and written only with has_buf
};

template <class Rule>
__global__ __launch_bounds__(256) void optim_step_kernel(const long long *__restrict__ tensors, const int32_t *__restrict__ chunks,
                                                         const Rule rule, const bool use_s0) {
    const int t = chunks[2 * blockIdx.x];
    const long long *row = tensors + 5 * (size_t)t;
    float *p = reinterpret_cast<float *>(row[0]);
    const float *g = reinterpret_cast<const float *>(row[1]);
    float *s0 = reinterpret_cast<float *>(row[2]), *s1 = reinterpret_cast<float *>(row[3]);
    const long long n = row[4], e0 = (long long)chunks[2 * blockIdx.x + 1] * CHUNK;
    const int len = (int)min((long long)CHUNK, n - e0);
    if (len <= 0) return;
    p += e0, g += e0;
    if (use_s0) s0 += e0;
    if (Rule::STATES == 2) s1 += e0;
    const bool vec = ((row[0] | row[1] | (use_s0 ? row[2] : 0) | (Rule::STATES == 2 ? row[3] : 0)) & 15) == 0;
    const int body = vec ? (len & ~3) : 0;
    for (int i = threadIdx.x * 4; i < body; i += 1024) {
        float4 P = *reinterpret_cast<float4 *>(p + i);
        const float4 G = *reinterpret_cast<const float4 *>(g + i);
        float4 A = use_s0 ? *reinterpret_cast<float4 *>(s0 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 Bv = Rule::STATES == 2 ? *reinterpret_cast<float4 *>(s1 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        rule(P.x, G.x, A.x, Bv.x), rule(P.y, G.y, A.y, Bv.y), rule(P.z, G.z, A.z, Bv.z), rule(P.w, G.w, A.w, Bv.w);
        *reinterpret_cast<float4 *>(p + i) = P;
        if (use_s0) *reinterpret_cast<float4 *>(s0 + i) = A;
        if (Rule::STATES == 2) *reinterpret_cast<float4 *>(s1 + i) = Bv;
    }
    for (int i = body + threadIdx.x; i < len; i += 256) {
        float P = p[i], A = use_s0 ? s0[i] : 0.f, Bv = Rule::STATES == 2 ? s1[i] : 0.f;
        rule(P, g[i], A, Bv);
        p[i] = P;
        if (use_s0) s0[i] = A;
        if (Rule::STATES == 2) s1[i] = Bv;
    }
}

constexpr int SLICE_BATCH = 8;   // slices whose loads are issued before the first add

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float add4(const float a, const float b) { return a + b; }
__device__ __forceinline__ float4 div4(const float4 a, const float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }
__device__ __forceinline__ float div4(const float a, const float d) { return a / d; }

// acc (+)= slice_0 + ... + slice_{N-1} at g, left to right: the N loads are independent and issued together, the adds are not
template <class V, int N>
__device__ __forceinline__ V add_slices(V acc, const bool first, const float *g, const long long stride) {
    V part[N];
#pragma unroll
    for (int k = 0; k < N; ++k) part[k] = *reinterpret_cast<const V *>(g + k * stride);
#pragma unroll
    for (int k = 0; k < N; ++k) acc = first && k == 0 ? part[0] : add4(acc, part[k]);
    return acc;
}

// ((slice_0 + slice_1) + slice_2 ...) / divisor at g (V = float4 or float), SLICE_BATCH slices at a time
template <class V>
__device__ __forceinline__ V ordered_mean(const float *g, const int n_slices, const long long stride, const float divisor) {
    V acc{};
    int r = 0;
    for (; r + SLICE_BATCH <= n_slices; r += SLICE_BATCH) acc = add_slices<V, SLICE_BATCH>(acc, r == 0, g + r * stride, stride);
    const float *rest = g + r * stride;
    switch (n_slices - r) {   // uniform: one scalar branch
    case 7: acc = add_slices<V, 7>(acc, r == 0, rest, stride); break;
    case 6: acc = add_slices<V, 6>(acc, r == 0, rest, stride); break;
    case 5: acc = add_slices<V, 5>(acc, r == 0, rest, stride); break;
    case 4: acc = add_slices<V, 4>(acc, r == 0, rest, stride); break;
    case 3: acc = add_slices<V, 3>(acc, r == 0, rest, stride); break;
    case 2: acc = add_slices<V, 2>(acc, r == 0, rest, stride); break;
    case 1: acc = add_slices<V, 1>(acc, r == 0, rest, stride); break;
    default: break;
    }
    return div4(acc, divisor);
}

// tensors (T,5): [param, element offset into a slice, state0, state1, numel]
template <class Rule>
__global__ __launch_bounds__(256) void optim_step_synced_kernel(const long long *__restrict__ tensors, const int32_t *__restrict__ chunks,
                                                                const float *__restrict__ slices, const int n_slices,
                                                                const long long slice_stride, const float divisor, const Rule rule,
                                                                const bool use_s0) {
    const int t = chunks[2 * blockIdx.x];
    const long long *row = tensors + 5 * (size_t)t;
    float *p = reinterpret_cast<float *>(row[0]);
    float *s0 = reinterpret_cast<float *>(row[2]), *s1 = reinterpret_cast<float *>(row[3]);
    const long long off = row[1], n = row[4], e0 = (long long)chunks[2 * blockIdx.x + 1] * CHUNK;
    const int len = (int)min((long long)CHUNK, n - e0);
    if (len <= 0 || off < 0 || off + n > slice_stride) return;   // a row that does not fit a slice updates nothing
    const float *g = slices + off + e0;
    p += e0;
    if (use_s0) s0 += e0;
    if (Rule::STATES == 2) s1 += e0;
    const bool vec = ((row[0] | (use_s0 ? row[2] : 0) | (Rule::STATES == 2 ? row[3] : 0) | (long long)(slices + off)) & 15) == 0;
    const int body = vec ? (len & ~3) : 0;   // slice_stride % 4 == 0 (checked by the entry point): every slice is aligned alike
    for (int i = threadIdx.x * 4; i < body; i += 1024) {
        float4 P = *reinterpret_cast<float4 *>(p + i);
        float4 A = use_s0 ? *reinterpret_cast<float4 *>(s0 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 Bv = Rule::STATES == 2 ? *reinterpret_cast<float4 *>(s1 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 G = ordered_mean<float4>(g + i, n_slices, slice_stride, divisor);
        rule(P.x, G.x, A.x, Bv.x), rule(P.y, G.y, A.y, Bv.y), rule(P.z, G.z, A.z, Bv.z), rule(P.w, G.w, A.w, Bv.w);
        *reinterpret_cast<float4 *>(p + i) = P;
        if (use_s0) *reinterpret_cast<float4 *>(s0 + i) = A;
        if (Rule::STATES == 2) *reinterpret_cast<float4 *>(s1 + i) = Bv;
    }
    for (int i = body + threadIdx.x; i < len; i += 256) {
        float P = p[i], A = use_s0 ? s0[i] : 0.f, Bv = Rule::STATES == 2 ? s1[i] : 0.f;
        rule(P, ordered_mean<float>(g + i, n_slices, slice_stride, divisor), A, Bv);
        p[i] = P;
        if (use_s0) s0[i] = A;
        if (Rule::STATES == 2) s1[i] = Bv;
    }
}

// table (T,3): [address of an fp32 tensor, element offset into flat, numel].  Pack: flat[offset + i] = tensor[i], zeros for
// address 0 (a gradient that is None); unpack: tensor[i] = flat[offset + i], address 0 skipped.  Nothing else of flat is touched.
template <bool UNPACK>
__global__ __launch_bounds__(256) void flat_copy_kernel(const long long *__restrict__ table, const int32_t *__restrict__ chunks,
                                                        float *flat, const long long flat_len) {
    const int t = chunks[2 * blockIdx.x];
    const long long *row = table + 3 * (size_t)t;
    const long long off = row[1], n = row[2], e0 = (long long)chunks[2 * blockIdx.x + 1] * CHUNK;
    const int len = (int)min((long long)CHUNK, n - e0);
    if (len <= 0 || off < 0 || off + n > flat_len) return;   // a row that does not fit the buffer moves nothing
    float *x = reinterpret_cast<float *>(row[0]);
    if (UNPACK && !x) return;
    float *f = flat + off + e0;
    const bool zeros = !x;
    if (x) x += e0;
    const bool vec = ((row[0] | (long long)(flat + off)) & 15) == 0;
    const int body = vec ? (len & ~3) : 0;
    for (int i = threadIdx.x * 4; i < body; i += 1024) {
        if (UNPACK) *reinterpret_cast<float4 *>(x + i) = *reinterpret_cast<const float4 *>(f + i);
        else *reinterpret_cast<float4 *>(f + i) = zeros ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4 *>(x + i);
    }
    for (int i = body + threadIdx.x; i < len; i += 256) {
        if (UNPACK) x[i] = f[i];
        else f[i] = zeros ? 0.f : x[i];
    }
}

// the step's scalars in double on the host, rounded to fp32 once, then launch(rule, use_s0): one place for both entry points
template <class Launch>
int optim_dispatch(int algo, double lr, double beta1, double beta2, double eps, double weight_decay, double step, double momentum,
                   double dampening, int nesterov, int first, Launch launch) {
    if (algo == DPM_OPTIM_SGD) {
        const SgdArgs a{(float)weight_decay, (float)momentum, (float)(1.0 - dampening), (float)(-lr), momentum != 0.0, first, nesterov};
        launch(SgdRule{a}, momentum != 0.0);
        return dpm_launch_status();
    }
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    AdamArgs a;
    a.decay = algo == DPM_OPTIM_ADAMW ? (float)(1.0 - lr * weight_decay) : (float)weight_decay;
    a.w1 = (float)(1.0 - beta1), a.beta2 = (float)beta2, a.w2 = (float)(1.0 - beta2);
    a.neg_step_size = (float)(-(lr / bc1)), a.bc2_sqrt = (float)sqrt(bc2), a.eps = (float)eps;
    if (algo == DPM_OPTIM_ADAMW) launch(AdamRule<true>{a}, true);
    else launch(AdamRule<false>{a}, true);
    return dpm_launch_status();
}

}  // namespace

extern "C" int dpm_optim_chunk(void) { return CHUNK; }

extern "C" int dpm_optim_step(int algo, const long long *tensors, const int32_t *chunks, int n_chunks, double lr, double beta1,
                              double beta2, double eps, double weight_decay, double step, double momentum, double dampening,
                              int nesterov, int first, dpm_stream_t stream) {
    DPM_CHECK_ARG(n_chunks >= 0 && (algo == DPM_OPTIM_ADAMW || algo == DPM_OPTIM_ADAM || algo == DPM_OPTIM_SGD));
    if (n_chunks == 0) return DPM_OK;
    DPM_CHECK_ARG(tensors && chunks);
    DPM_CHECK_ARG(algo == DPM_OPTIM_SGD || step >= 1.0);
    hipStream_t s = (hipStream_t)stream;
    return optim_dispatch(algo, lr, beta1, beta2, eps, weight_decay, step, momentum, dampening, nesterov, first,
                          [&](auto rule, bool use_s0) { optim_step_kernel<<<n_chunks, 256, 0, s>>>(tensors, chunks, rule, use_s0); });
}

extern "C" int dpm_optim_step_synced(int algo, const long long *tensors, const int32_t *chunks, int n_chunks, double lr, double beta1,
                                     double beta2, double eps, double weight_decay, double step, double momentum, double dampening,
                                     int nesterov, int first, const float *slices, int n_slices, long long slice_stride,
                                     double divisor, dpm_stream_t stream) {
    DPM_CHECK_ARG(n_chunks >= 0 && (algo == DPM_OPTIM_ADAMW || algo == DPM_OPTIM_ADAM || algo == DPM_OPTIM_SGD));
    DPM_CHECK_ARG(n_slices >= 1 && slice_stride >= 0 && slice_stride % 4 == 0 && divisor >= 1.0);
    if (n_chunks == 0) return DPM_OK;
    DPM_CHECK_ARG(tensors && chunks && slices);
    DPM_CHECK_ARG(algo == DPM_OPTIM_SGD || step >= 1.0);
    hipStream_t s = (hipStream_t)stream;
    const float d = (float)divisor;
    return optim_dispatch(algo, lr, beta1, beta2, eps, weight_decay, step, momentum, dampening, nesterov, first,
                          [&](auto rule, bool use_s0) {
                              optim_step_synced_kernel<<<n_chunks, 256, 0, s>>>(tensors, chunks, slices, n_slices, slice_stride, d,
                                                                                rule, use_s0);
                          });
}

extern "C" int dpm_flat_pack(const long long *table, const int32_t *chunks, int n_chunks, float *flat, long long flat_len,
                             dpm_stream_t stream) {
    DPM_CHECK_ARG(n_chunks >= 0 && flat_len >= 0 && flat_len % 4 == 0);
    if (n_chunks == 0) return DPM_OK;
    DPM_CHECK_ARG(table && chunks && flat);
    flat_copy_kernel<false><<<n_chunks, 256, 0, (hipStream_t)stream>>>(table, chunks, flat, flat_len);
    return dpm_launch_status();
}

extern "C" int dpm_flat_unpack(const long long *table, const int32_t *chunks, int n_chunks, const float *flat, long long flat_len,
                               dpm_stream_t stream) {
    DPM_CHECK_ARG(n_chunks >= 0 && flat_len >= 0 && flat_len % 4 == 0);
    if (n_chunks == 0) return DPM_OK;
    DPM_CHECK_ARG(table && chunks && flat);
    flat_copy_kernel<true><<<n_chunks, 256, 0, (hipStream_t)stream>>>(table, chunks, const_cast<float *>(flat), flat_len);
    return dpm_launch_status();
}
