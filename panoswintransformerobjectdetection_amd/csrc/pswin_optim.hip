// AdamW over the ONE flat fp32 parameter buffer of a model (dp.GradReducer.flatten_parameters), gfx950.
//
// A training step of the hot path ends in the optimizer update (bench.py's step = fwd + bwd + AdamW, as the reference's
// configs/swin/*.py run it, mmdet/apis/train.py:91-112) and begins with the bf16 copies of the Linear weights that the bf16 kernels
// read.  Over one flat buffer both are a single streaming pass: p, g, m, v in; p, m, v and bf16(p) out -- 30 bytes per parameter,
// one launch, instead of the framework's two multi-tensor launches (28 B) plus a cast pass (6 B) at the start of the next step.
// Arithmetic = torch.optim.AdamW (decoupled weight decay, bias-corrected moments), f32, in this order:
//   p -= lr * wd * p;   m += (1 - b1) * (g - m);   v = b2 * v + (1 - b2) * g * g;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The step number t lives in device memory (a captured hipGraph replays the launch with the same arguments).
#include "pswin_common.hpp"

using namespace pswin;

namespace {

constexpr int MAX_GROUPS = PSWIN_ADAMW_MAX_GROUPS;
struct GroupMults {
    float lr[MAX_GROUPS], decay[MAX_GROUPS];       // per parameter group: multipliers of the base lr / weight decay
};

// GROUPS: group_of[i] names the parameter group of elements 4 i .. 4 i + 3 (one byte per 16-byte granule: 0.8 % more traffic);
// the reference's paramwise_cfg (decay_mult = 0 for norm layers / position tables) is two groups
template <bool GROUPS>
__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, unsigned short* __restrict__ lowp, long long n4, double lr,
                                                         double b1d, double b2d, float eps, double wd, const float* __restrict__ step,
                                                         const unsigned char* __restrict__ group_of, const GroupMults gm) {
    // the hyper-parameters arrive as doubles (as torch hands them to its kernel) and every derived constant is formed in double
    // before it is rounded to f32: 1 - 0.999f is 1.3e-5 away from 1 - 0.999
    const double t = (double)*step;
    const double bc1 = 1.0 - pow(b1d, t), bc2 = 1.0 - pow(b2d, t);
    const float bc2s = (float)sqrt(bc2), w1 = (float)(1.0 - b1d), w2 = (float)(1.0 - b2d), b2 = (float)b2d;
    float step_size = (float)(lr / bc1), decay = (float)(lr * wd);
    [[maybe_unused]] float step_g[MAX_GROUPS], decay_g[MAX_GROUPS];
    if constexpr (GROUPS) {
#pragma unroll
        for (int k = 0; k < MAX_GROUPS; ++k) {        // per group exactly what torch computes for a group with lr * lr_mult, wd * decay_mult
            const double lrk = lr * (double)gm.lr[k];
            step_g[k] = (float)(lrk / bc1);
            decay_g[k] = (float)(lrk * (wd * (double)gm.decay[k]));
        }
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mv = reinterpret_cast<const f32x4*>(m)[i], vv = reinterpret_cast<const f32x4*>(v)[i];
        if constexpr (GROUPS) {
            const int k = group_of[i];
            step_size = step_g[0];
            decay = decay_g[0];
#pragma unroll
            for (int q = 1; q < MAX_GROUPS; ++q) {    // select, not index: keeps the tables in registers
                step_size = k == q ? step_g[q] : step_size;
                decay = k == q ? decay_g[q] : decay;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pv[e];
            pe -= decay * pe;
            const float me = mv[e] + w1 * (gv[e] - mv[e]);
            const float ve = b2 * vv[e] + w2 * gv[e] * gv[e];
            const float denom = sqrtf(ve) / bc2s + eps;
            pe -= step_size * me / denom;
            pv[e] = pe;
            mv[e] = me;
            vv[e] = ve;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if (lowp) {
            u32x2 o = {pack2_bf16(pv[0], pv[1]), pack2_bf16(pv[2], pv[3])};
            reinterpret_cast<u32x2*>(lowp)[i] = o;
        }
    }
}

}  // namespace

extern "C" int pswin_adamw_flat_groups(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const unsigned char* group_of,
                                       int n_groups, const float* lr_mult, const float* decay_mult, double lr, double beta1, double beta2,
                                       double eps, double weight_decay, const float* step, void* stream) {
    PSWIN_CHECK_ARG(p && g && m && v && step && n > 0 && n % 4 == 0);
    PSWIN_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (reinterpret_cast<uintptr_t>(p_bf16) & 7) == 0);
    PSWIN_CHECK_ARG(lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.);
    PSWIN_CHECK_ARG(group_of ? (n_groups >= 1 && n_groups <= MAX_GROUPS && lr_mult && decay_mult) : n_groups == 0);
    const long long n4 = n / 4;
    long long blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;             // 16 workgroups of 4 waves per CU, grid-stride over the rest
    GroupMults gm;
    for (int k = 0; k < MAX_GROUPS; ++k) {
        gm.lr[k] = (group_of && k < n_groups) ? lr_mult[k] : 1.f;
        gm.decay[k] = (group_of && k < n_groups) ? decay_mult[k] : 1.f;
        PSWIN_CHECK_ARG(gm.lr[k] >= 0.f && gm.decay[k] >= 0.f);
    }
    if (group_of)
        hipLaunchKernelGGL(adamw_flat_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                           reinterpret_cast<unsigned short*>(p_bf16), n4, lr, beta1, beta2, (float)eps, weight_decay, step, group_of, gm);
    else
        hipLaunchKernelGGL(adamw_flat_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                           reinterpret_cast<unsigned short*>(p_bf16), n4, lr, beta1, beta2, (float)eps, weight_decay, step, group_of, gm);
    PSWIN_LAUNCH_RET();
}

extern "C" int pswin_adamw_flat(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2,
                                double eps, double weight_decay, const float* step, void* stream) {
    return pswin_adamw_flat_groups(p, g, m, v, p_bf16, n, nullptr, 0, nullptr, nullptr, lr, beta1, beta2, eps, weight_decay, step, stream);
}

// ---- the training recipe on the device (lr schedule, gradient-norm clipping, non-finite guard) ------------------------------------
// A captured step replays its launches with the arguments of the capture, so everything that changes from step to step -- the
// scheduled lr, the clip coefficient, whether the step is applied at all -- is computed by a kernel into a small device record that
// the update reads.  The three launches of a step (include/pswin.h): sum of squares -> record (one workgroup) -> update.

namespace {

constexpr int SQ_PARTIALS = PSWIN_GRADSQ_PARTIALS;
constexpr int SQ_THREADS = 256;
static_assert(sizeof(pswin_step_record) == 96 && sizeof(pswin_lr_schedule) == 88, "layouts of include/pswin.h (mirrored in _lib.py)");

// fixed-shape tree over SQ_THREADS doubles in LDS: the same additions in the same order on every run
__device__ inline double block_sum_fixed(double s, double* red) {
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = SQ_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

__device__ inline double sumsq4(const f32x4 v) {
    const double a = v[0], b = v[1], c = v[2], d = v[3];
    return ((a * a + b * b) + c * c) + d * d;
}

// block b sums granules [b * chunk, min((b + 1) * chunk, n4)); the grid is SQ_PARTIALS blocks whatever the device, so every partial
// covers the same range on every run and every rank.  Four loads in flight per thread; f64 accumulation.
__global__ __launch_bounds__(SQ_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, long long n4, long long chunk,
                                                                double* __restrict__ partials) {
    __shared__ double red[SQ_THREADS];
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n4 ? lo + chunk : n4;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    double s = 0.0;
    long long i = lo + threadIdx.x;
    for (; i + 3 * SQ_THREADS < hi; i += 4 * SQ_THREADS) {
        const f32x4 a = g4[i], b = g4[i + SQ_THREADS], c = g4[i + 2 * SQ_THREADS], d = g4[i + 3 * SQ_THREADS];
        s += sumsq4(a);
        s += sumsq4(b);
        s += sumsq4(c);
        s += sumsq4(d);
    }
    for (; i < hi; i += SQ_THREADS) s += sumsq4(g4[i]);
    const double total = block_sum_fixed(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

struct RecordArgs {
    pswin_lr_schedule s;
    double base[MAX_GROUPS];                        // lr * lr_mult[k]
    double max_norm;                                // <= 0: no clipping
    int skip_nonfinite;
};

// mmcv's StepLrUpdaterHook.get_lr / FixedLrUpdaterHook and LrUpdaterHook.get_warmup_lr for iteration i, in double
__device__ inline double scheduled_lr(const pswin_lr_schedule& s, double base, int i) {
    double lr = base;
    if (s.policy == PSWIN_LR_STEP) {
        const int progress = s.by_epoch ? i / s.iters_per_epoch : i;
        int e = 0;
        if (s.n_milestones > 0) {
            for (int q = 0; q < s.n_milestones; ++q) e += progress >= s.milestones[q] ? 1 : 0;
        } else if (s.step_every > 0) {
            e = progress / s.step_every;
        }
        lr = base * pow(s.gamma, (double)e);
        if (s.has_min_lr) lr = lr > s.min_lr ? lr : s.min_lr;
    }
    if (s.warmup != PSWIN_WARMUP_NONE && i < s.warmup_iters) {
        const double frac = (double)i / (double)s.warmup_iters;
        if (s.warmup == PSWIN_WARMUP_CONSTANT) lr = lr * s.warmup_ratio;
        else if (s.warmup == PSWIN_WARMUP_LINEAR) lr = lr * (1.0 - (1.0 - frac) * (1.0 - s.warmup_ratio));
        else lr = lr * pow(s.warmup_ratio, 1.0 - frac);
    }
    return lr;
}

__global__ __launch_bounds__(SQ_THREADS) void adamw_record_kernel(const double* __restrict__ partials, const RecordArgs a,
                                                                  float* __restrict__ step, float* __restrict__ iteration,
                                                                  float* __restrict__ skipped, pswin_step_record* __restrict__ rec) {
    __shared__ double red[SQ_THREADS];
    double s = 0.0;
    if (partials) {
        constexpr int PER = SQ_PARTIALS / SQ_THREADS;
#pragma unroll
        for (int j = 0; j < PER; ++j) s += partials[threadIdx.x * PER + j];
    }
    const double sumsq = block_sum_fixed(s, red);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(sumsq);
    const bool finite = isfinite(norm);
    double coef = 1.0;
    if (a.max_norm > 0.0) {
        const double c = a.max_norm / (norm + 1e-6);
        coef = c > 1.0 ? 1.0 : c;                   // (a NaN norm gives a NaN coefficient, as torch's clamp does)
    }
    const int i = (int)*iteration;
    const bool applied = !a.skip_nonfinite || finite;
    *iteration = (float)(i + 1);
    float t = *step;
    if (applied) {
        t += 1.0f;
        *step = t;
    } else {
        *skipped = *skipped + 1.0f;
    }
    for (int k = 0; k < MAX_GROUPS; ++k) rec->lr[k] = scheduled_lr(a.s, a.base[k], i);
    rec->norm = norm;
    rec->lr_base = (float)rec->lr[0];
    rec->norm_f = (float)norm;
    rec->coef = (float)coef;
    rec->t = t;
    rec->applied = applied ? 1 : 0;
    rec->iteration = i;
}

// adamw_flat_kernel<GROUPS> with lr per group, t and the clip coefficient from the record; g * coef is the gradient (f32)
template <bool GROUPS>
__global__ __launch_bounds__(256) void adamw_flat_sched_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, unsigned short* __restrict__ lowp, long long n4,
                                                               double b1d, double b2d, float eps, double wd,
                                                               const pswin_step_record* __restrict__ rec,
                                                               const unsigned char* __restrict__ group_of, const GroupMults gm) {
    if (!rec->applied) return;
    const double t = (double)rec->t;
    const float coef = rec->coef;
    const double bc1 = 1.0 - pow(b1d, t), bc2 = 1.0 - pow(b2d, t);
    const float bc2s = (float)sqrt(bc2), w1 = (float)(1.0 - b1d), w2 = (float)(1.0 - b2d), b2 = (float)b2d;
    const double lr = rec->lr[0];
    float step_size = (float)(lr / bc1), decay = (float)(lr * wd);
    [[maybe_unused]] float step_g[MAX_GROUPS], decay_g[MAX_GROUPS];
    if constexpr (GROUPS) {
#pragma unroll
        for (int k = 0; k < MAX_GROUPS; ++k) {
            const double lrk = rec->lr[k];
            step_g[k] = (float)(lrk / bc1);
            decay_g[k] = (float)(lrk * (wd * (double)gm.decay[k]));
        }
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i] * coef;
        f32x4 mv = reinterpret_cast<const f32x4*>(m)[i], vv = reinterpret_cast<const f32x4*>(v)[i];
        if constexpr (GROUPS) {
            const int k = group_of[i];
            step_size = step_g[0];
            decay = decay_g[0];
#pragma unroll
            for (int q = 1; q < MAX_GROUPS; ++q) {
                step_size = k == q ? step_g[q] : step_size;
                decay = k == q ? decay_g[q] : decay;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pv[e];
            pe -= decay * pe;
            const float me = mv[e] + w1 * (gv[e] - mv[e]);
            const float ve = b2 * vv[e] + w2 * gv[e] * gv[e];
            const float denom = sqrtf(ve) / bc2s + eps;
            pe -= step_size * me / denom;
            pv[e] = pe;
            mv[e] = me;
            vv[e] = ve;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if (lowp) {
            u32x2 o = {pack2_bf16(pv[0], pv[1]), pack2_bf16(pv[2], pv[3])};
            reinterpret_cast<u32x2*>(lowp)[i] = o;
        }
    }
}

bool valid_schedule(const pswin_lr_schedule& s) {
    if (s.policy != PSWIN_LR_FIXED && s.policy != PSWIN_LR_STEP) return false;
    if (s.warmup < PSWIN_WARMUP_NONE || s.warmup > PSWIN_WARMUP_EXP) return false;
    if (s.warmup != PSWIN_WARMUP_NONE && !(s.warmup_iters >= 1 && s.warmup_ratio >= 0. && s.warmup_ratio <= 1.)) return false;
    if (s.by_epoch && s.iters_per_epoch < 1) return false;
    if (s.n_milestones < 0 || s.n_milestones > PSWIN_LR_MAX_MILESTONES || s.step_every < 0) return false;
    for (int q = 0; q < s.n_milestones; ++q)
        if (s.milestones[q] < 0 || (q > 0 && s.milestones[q] < s.milestones[q - 1])) return false;
    if (!(s.gamma >= 0. && s.gamma <= 1e300)) return false;
    if (s.has_min_lr && !(s.min_lr >= 0.)) return false;
    return true;
}

}  // namespace

extern "C" int pswin_grad_sumsq(const float* g, long long n, double* partials, void* stream) {
    PSWIN_CHECK_ARG(g && partials && n > 0 && n % 4 == 0 && aligned16(g) && (reinterpret_cast<uintptr_t>(partials) & 7) == 0);
    const long long n4 = n / 4;
    const long long chunk = (n4 + SQ_PARTIALS - 1) / SQ_PARTIALS;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(SQ_PARTIALS), dim3(SQ_THREADS), 0, (hipStream_t)stream, g, n4, chunk, partials);
    PSWIN_LAUNCH_RET();
}

extern "C" int pswin_adamw_record(const double* partials, const pswin_lr_schedule* sched, double lr, int n_groups, const float* lr_mult,
                                  double max_norm, int skip_nonfinite, float* step, float* iteration, float* skipped,
                                  pswin_step_record* record, void* stream) {
    PSWIN_CHECK_ARG(sched && step && iteration && skipped && record && (reinterpret_cast<uintptr_t>(record) & 7) == 0);
    PSWIN_CHECK_ARG(lr >= 0. && valid_schedule(*sched));
    PSWIN_CHECK_ARG(lr_mult ? (n_groups >= 1 && n_groups <= MAX_GROUPS) : (n_groups == 0 || n_groups == 1));
    PSWIN_CHECK_ARG(partials ? (reinterpret_cast<uintptr_t>(partials) & 7) == 0 : (!(max_norm > 0.) && !skip_nonfinite));
    PSWIN_CHECK_ARG(!(max_norm != max_norm));
    RecordArgs a;
    a.s = *sched;
    for (int k = 0; k < MAX_GROUPS; ++k) {
        const float mult = (lr_mult && k < n_groups) ? lr_mult[k] : 1.f;
        PSWIN_CHECK_ARG(mult >= 0.f);
        a.base[k] = lr * (double)mult;
    }
    a.max_norm = max_norm;
    a.skip_nonfinite = skip_nonfinite ? 1 : 0;
    hipLaunchKernelGGL(adamw_record_kernel, dim3(1), dim3(SQ_THREADS), 0, (hipStream_t)stream, partials, a, step, iteration, skipped, record);
    PSWIN_LAUNCH_RET();
}

extern "C" int pswin_adamw_flat_sched(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const unsigned char* group_of,
                                      int n_groups, const float* decay_mult, double beta1, double beta2, double eps, double weight_decay,
                                      const pswin_step_record* record, void* stream) {
    PSWIN_CHECK_ARG(p && g && m && v && record && n > 0 && n % 4 == 0);
    PSWIN_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (reinterpret_cast<uintptr_t>(p_bf16) & 7) == 0);
    PSWIN_CHECK_ARG((reinterpret_cast<uintptr_t>(record) & 7) == 0);
    PSWIN_CHECK_ARG(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.);
    PSWIN_CHECK_ARG(group_of ? (n_groups >= 1 && n_groups <= MAX_GROUPS && decay_mult) : n_groups == 0);
    const long long n4 = n / 4;
    long long blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    GroupMults gm;
    for (int k = 0; k < MAX_GROUPS; ++k) {
        gm.lr[k] = 1.f;                                   // (the record's lr already carries lr_mult)
        gm.decay[k] = (group_of && k < n_groups) ? decay_mult[k] : 1.f;
        PSWIN_CHECK_ARG(gm.decay[k] >= 0.f);
    }
    if (group_of)
        hipLaunchKernelGGL(adamw_flat_sched_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                           reinterpret_cast<unsigned short*>(p_bf16), n4, beta1, beta2, (float)eps, weight_decay, record, group_of, gm);
    else
        hipLaunchKernelGGL(adamw_flat_sched_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                           reinterpret_cast<unsigned short*>(p_bf16), n4, beta1, beta2, (float)eps, weight_decay, record, group_of, gm);
    PSWIN_LAUNCH_RET();
}
