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

}  // namespace

extern "C" int dpm_optim_chunk(void) { return CHUNK; }

extern "C" int dpm_optim_step(int algo, const long long *tensors, const int32_t *chunks, int n_chunks, double lr, double beta1,
                              double beta2, double eps, double weight_decay, double step, double momentum, double dampening,
                              int nesterov, int first, dpm_stream_t stream) {
    DPM_CHECK_ARG(n_chunks >= 0 && (algo == DPM_OPTIM_ADAMW || algo == DPM_OPTIM_ADAM || algo == DPM_OPTIM_SGD));
    if (n_chunks == 0) return DPM_OK;
    DPM_CHECK_ARG(tensors && chunks);
    hipStream_t s = (hipStream_t)stream;
    if (algo == DPM_OPTIM_SGD) {
        const SgdArgs a{(float)weight_decay, (float)momentum, (float)(1.0 - dampening), (float)(-lr), momentum != 0.0, first, nesterov};
        optim_step_kernel<<<n_chunks, 256, 0, s>>>(tensors, chunks, SgdRule{a}, momentum != 0.0);
        return dpm_launch_status();
    }
    DPM_CHECK_ARG(step >= 1.0);
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    AdamArgs a;
    a.decay = algo == DPM_OPTIM_ADAMW ? (float)(1.0 - lr * weight_decay) : (float)weight_decay;
    a.w1 = (float)(1.0 - beta1), a.beta2 = (float)beta2, a.w2 = (float)(1.0 - beta2);
    a.neg_step_size = (float)(-(lr / bc1)), a.bc2_sqrt = (float)sqrt(bc2), a.eps = (float)eps;
    if (algo == DPM_OPTIM_ADAMW) optim_step_kernel<<<n_chunks, 256, 0, s>>>(tensors, chunks, AdamRule<true>{a}, true);
    else optim_step_kernel<<<n_chunks, 256, 0, s>>>(tensors, chunks, AdamRule<false>{a}, true);
    return dpm_launch_status();
}
