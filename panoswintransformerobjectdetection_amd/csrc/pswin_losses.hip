// The detector's training losses between "targets built" and "backward through the heads" (losses.ce_rows / l1_rows / mask_bce_rows /
// rpn_losses: the five losses of MiniMaskRCNN and the class and mask losses of MiniCascadeRCNN's stages) -- gfx950 only.
//
// The conventions of pswin_cascade.hip: the heads' outputs are read from device memory in place as f32 or bf16, nothing is read back and
// no buffer has to be cleared between calls: every element of every output is written by plain vector stores, so a captured step replays
// on the same buffers.  No atomics, no workspace, no state.
//
// ARITHMETIC.  Every value is evaluated in double from the float inputs and rounded once (exp / log / log1p included): the rows are short,
// the kernels are bound by latency or by the gradient's stores either way, and the result is then within half a float32 ulp of the float64
// definition.  Every sum is taken in a FIXED order (a lane's elements in ascending order, then a tree over the lanes whose shape depends
// on nothing but the sizes), so a call returns the same bits every time.
//
// CE ROWS: LOSS_ROWS rows per workgroup, four lanes per row.  Lane q takes classes q, q + 4, ... for the row's maximum and then for the sum
// of exp(x - max); the four partial results are merged by two exchanges.  The backward leaves (log-sum-exp, label, upstream) of its rows in
// LDS, then all threads walk the rows' (C + 1) columns in memory order.
// L1 ROWS: one row per lane; the backward as giou_rows_bwd_kernel: the first LOSS_ROWS lanes leave the four values and the class of a row in
// LDS, then all threads write the rows' 4 C columns class by class.
// MASK BCE ROWS: one workgroup per RoI sums the S x S map of the label's channel through the logits' strides and, if asked, leaves that
// channel as f32 [M][S][S] (`picked`): all the backward needs of the logits, so that the caller does not have to keep the C-channel tensor
// alive between the passes.  The backward walks the gradient in MEMORY order (NCHW or channels-last, the layout of the logits), 16 bytes
// per lane where a RoI's C S S elements allow it.
// RPN LOSSES: one workgroup per image sums its S slots.  The backward gives every workgroup RPN_CHUNK anchors of one image: it marks in LDS
// which slot (if any) names each of its anchors -- the valid slots of an image hold distinct anchors, so no two writers meet -- and then
// streams the chunk out: the slot's two gradients where there is one, zeros elsewhere.
#include "pswin_common.hpp"

namespace {
using namespace pswin;

constexpr int LOSS_ROWS = 64;
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_CMAX = 128;
constexpr int MASK_SMAX = 56;
constexpr int MASK_GROUPS_PER_THREAD = 4;       // backward: 16-byte groups one thread writes
constexpr int RPN_CHUNK = 4096;                 // anchors one workgroup of the backward owns

template <int DT>
__device__ inline float load1(const void* base, size_t o) {
    if constexpr (DT == PSWIN_F32) return reinterpret_cast<const float*>(base)[o];
    else return bf16_bits_to_f32(reinterpret_cast<const unsigned short*>(base)[o]);
}

template <int DT>
__device__ inline void store1(void* base, size_t o, float v) {
    if constexpr (DT == PSWIN_F32) reinterpret_cast<float*>(base)[o] = v;
    else reinterpret_cast<unsigned short*>(base)[o] = f32_to_bf16_bits(v);
}

__device__ inline int clamp_label(long long v, int C) { return v < 0 ? 0 : (v > C - 1 ? C - 1 : (int)v); }

// sum of v over the LOSS_THREADS threads of a workgroup, the same bits in every thread: a tree whose shape is fixed
__device__ inline double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                                                           // red may still be read from the sum before
    red[t] = v;
    __syncthreads();
    for (int s = LOSS_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// BCE-with-logits of one element and its derivative: max(x, 0) - x t + log1p(exp(-|x|));  sigmoid(x) - t
__device__ inline double bce_logits(double x, double t) { return fmax(x, 0.0) - x * t + log1p(exp(-fabs(x))); }
__device__ inline double sigmoid_d(double x) {
    const double e = exp(-fabs(x));
    return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// ---- ce_rows ---------------------------------------------------------------------------------------------------------------------------
// The four lanes of row `row` (lab inside [0, C1)): the row's maximum and log(sum exp(x - max)), the same bits in all four
template <int DT>
__device__ inline void ce_row_stats(const void* cls, size_t row, int C1, int q, double& mx, double& logsum) {
    double m = -INFINITY;
    for (int c = q; c < C1; c += 4) m = fmax(m, (double)load1<DT>(cls, row * (size_t)C1 + c));
    m = fmax(m, __shfl_xor(m, 1, 64));
    m = fmax(m, __shfl_xor(m, 2, 64));
    double s = 0.0;
    for (int c = q; c < C1; c += 4) s += exp((double)load1<DT>(cls, row * (size_t)C1 + c) - m);
    s += __shfl_xor(s, 1, 64);                                                 // (s0 + s1) and (s2 + s3), then their sum: the same in every lane
    s += __shfl_xor(s, 2, 64);
    mx = m;
    logsum = log(s);
}

// grid ceil(N / LOSS_ROWS)
template <int DT>
__global__ __launch_bounds__(LOSS_THREADS) void ce_rows_fwd_kernel(const void* __restrict__ cls, const long long* __restrict__ labels, int N,
                                                                  int C1, float* __restrict__ out) {
    const int q = threadIdx.x & 3;
    const int r = blockIdx.x * LOSS_ROWS + (threadIdx.x >> 2);
    const bool live = r < N;
    const size_t row = live ? r : N - 1;                                      // a dead lane reads the last row and writes nothing
    const long long lab = labels[row];
    float v = 0.f;
    if (lab >= 0 && lab < C1) {                                               // uniform over the four lanes of a row
        double m, ls;
        ce_row_stats<DT>(cls, row, C1, q, m, ls);
        v = (float)((m - (double)load1<DT>(cls, row * (size_t)C1 + (size_t)lab)) + ls);
    }
    if (live && q == 0) out[r] = v;
}

template <int DT>
__global__ __launch_bounds__(LOSS_THREADS) void ce_rows_bwd_kernel(const void* __restrict__ cls, const long long* __restrict__ labels,
                                                                  const float* __restrict__ grad_rows, int N, int C1, void* __restrict__ grad) {
    __shared__ double s_lse[LOSS_ROWS];
    __shared__ float s_up[LOSS_ROWS];
    __shared__ int s_label[LOSS_ROWS];                                        // -1: the whole row is zeros
    const int t = threadIdx.x, q = t & 3, lr = t >> 2;
    const int row0 = blockIdx.x * LOSS_ROWS;
    const bool live = row0 + lr < N;
    const size_t row = live ? row0 + lr : N - 1;
    const long long lab = labels[row];
    const bool on = lab >= 0 && lab < C1;
    double m = 0.0, ls = 0.0;
    if (on) ce_row_stats<DT>(cls, row, C1, q, m, ls);
    if (q == 0) {
        s_lse[lr] = m + ls;
        s_up[lr] = grad_rows[row];
        s_label[lr] = on ? (int)lab : -1;
    }
    __syncthreads();
    const int rows = N - row0 < LOSS_ROWS ? N - row0 : LOSS_ROWS;
    const size_t base = (size_t)row0 * C1;
    for (int i = t; i < rows * C1; i += LOSS_THREADS) {
        const int r = i / C1, c = i - r * C1;
        float v = 0.f;
        if (s_label[r] >= 0) {
            const double p = exp((double)load1<DT>(cls, base + i) - s_lse[r]);
            v = (float)((p - (c == s_label[r] ? 1.0 : 0.0)) * (double)s_up[r]);
        }
        store1<DT>(grad, base + i, v);
    }
}

// ---- l1_rows ---------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(LOSS_ROWS) void l1_rows_fwd_kernel(const void* __restrict__ reg, const long long* __restrict__ labels,
                                                               const float* __restrict__ weight, const float* __restrict__ target, int N, int C,
                                                               float* __restrict__ out) {
    const int n = blockIdx.x * LOSS_ROWS + threadIdx.x;
    if (n >= N) return;
    const float w = weight[n];
    float v = 0.f;
    if (w != 0.f) {                                                           // a weight-0 row reads nothing else
        const f32x4 d = load4<DT>(reg, (size_t)n * (4 * C) + 4 * (size_t)clamp_label(labels[n], C));
        const f32x4 tg = reinterpret_cast<const f32x4*>(target)[n];
        const double s = ((fabs((double)d[0] - (double)tg[0]) + fabs((double)d[1] - (double)tg[1])) + fabs((double)d[2] - (double)tg[2])) +
                         fabs((double)d[3] - (double)tg[3]);
        v = (float)((double)w * s);
    }
    out[n] = v;
}

__device__ inline float signed_by(float d, float g) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); }      // sign(0) = 0, as abs's gradient

template <int DT>
__global__ __launch_bounds__(LOSS_THREADS) void l1_rows_bwd_kernel(const void* __restrict__ reg, const long long* __restrict__ labels,
                                                                  const float* __restrict__ weight, const float* __restrict__ target,
                                                                  const float* __restrict__ grad_rows, int N, int C, void* __restrict__ grad) {
    __shared__ f32x4 s_grad[LOSS_ROWS];
    __shared__ int s_class[LOSS_ROWS];                                        // -1: the whole row is zeros
    const int t = threadIdx.x;
    const int row0 = blockIdx.x * LOSS_ROWS;
    if (t < LOSS_ROWS) {
        const int n = row0 + t;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        int cls = -1;
        if (n < N) {
            const float w = weight[n];
            if (w != 0.f) {
                cls = clamp_label(labels[n], C);
                const f32x4 d = load4<DT>(reg, (size_t)n * (4 * C) + 4 * (size_t)cls);
                const f32x4 tg = reinterpret_cast<const f32x4*>(target)[n];
                const float up = w * grad_rows[n];                            // fl(weight * upstream): what abs's gradient is multiplied by
                g = f32x4{signed_by(d[0] - tg[0], up), signed_by(d[1] - tg[1], up), signed_by(d[2] - tg[2], up), signed_by(d[3] - tg[3], up)};
            }
        }
        s_grad[t] = g;
        s_class[t] = cls;
    }
    __syncthreads();
    const int rows = N - row0 < LOSS_ROWS ? N - row0 : LOSS_ROWS;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = t; i < rows * C; i += LOSS_THREADS) {
        const int r = i / C, c = i - r * C;
        store4<DT>(grad, (size_t)(row0 + r) * (4 * C) + 4 * (size_t)c, c == s_class[r] ? s_grad[r] : zero);
    }
}

// ---- mask_bce_rows ---------------------------------------------------------------------------------------------------------------------
// grid M
template <int DT>
__global__ __launch_bounds__(LOSS_THREADS) void mask_bce_fwd_kernel(const void* __restrict__ logits, long long sn, long long sc, long long sy,
                                                                   long long sx, const long long* __restrict__ labels,
                                                                   const float* __restrict__ target, const float* __restrict__ weight, int C, int S,
                                                                   float* __restrict__ out, float* __restrict__ picked) {
    __shared__ double red[LOSS_THREADS];
    const int m = blockIdx.x;
    const float w = weight[m];
    if (w == 0.f) {                                                           // uniform over the workgroup; a weight-0 row reads nothing else
        if (threadIdx.x == 0) out[m] = 0.f;
        if (picked)
            for (int i = threadIdx.x; i < S * S; i += LOSS_THREADS) picked[(size_t)m * S * S + i] = 0.f;
        return;
    }
    const size_t base = (size_t)m * sn + (size_t)clamp_label(labels[m], C) * sc;
    const float* tg = target + (size_t)m * S * S;
    double s = 0.0;
    for (int i = threadIdx.x; i < S * S; i += LOSS_THREADS) {
        const int y = i / S, x = i - y * S;
        const float v = load1<DT>(logits, base + (size_t)y * sy + (size_t)x * sx);
        if (picked) picked[(size_t)m * S * S + i] = v;
        s += bce_logits((double)v, (double)tg[i]);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[m] = (float)((double)w * (s / (double)(S * S)));
}

// The gradient of element f of RoI m in MEMORY order: f = (y S + x) C + c for channels-last logits, f = c S S + (y S + x) otherwise
__device__ inline float mask_grad_elem(const float* picked, const float* tg, int f, int C, int SS, bool channels_last, int lab, double scale) {
    int c, px;
    if (channels_last) {
        px = f / C;
        c = f - px * C;
    } else {
        c = f / SS;
        px = f - c * SS;
    }
    if (c != lab) return 0.f;
    return (float)((sigmoid_d((double)picked[px]) - (double)tg[px]) * scale);
}

// grid M * blocks_per_roi.  VEC: a RoI's C S S elements are a multiple of the 16-byte group and the buffers are 16-byte aligned
template <int DT, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void mask_bce_bwd_kernel(const float* __restrict__ picked, int channels_last,
                                                                   const long long* __restrict__ labels, const float* __restrict__ target,
                                                                   const float* __restrict__ weight, const float* __restrict__ grad_rows, int C,
                                                                   int S, int blocks_per_roi, void* __restrict__ grad) {
    constexpr int VE = VEC ? Vec<DT>::VE : 1;
    const int m = blockIdx.x / blocks_per_roi, blk = blockIdx.x - m * blocks_per_roi;
    const int SS = S * S, per_roi = C * SS;
    const float w = weight[m];
    const int lab = w != 0.f ? clamp_label(labels[m], C) : -1;                // -1: no channel is selected, the RoI's `picked` is not read
    const double scale = (double)w * (double)grad_rows[m] / (double)SS;
    const size_t roi_base = (size_t)m * per_roi;
    const float* tg = target + (size_t)m * SS;
    picked += (size_t)m * SS;
    const int g0 = blk * (LOSS_THREADS * MASK_GROUPS_PER_THREAD);
#pragma unroll
    for (int k = 0; k < MASK_GROUPS_PER_THREAD; ++k) {
        const int f0 = (g0 + k * LOSS_THREADS + (int)threadIdx.x) * VE;
        if (f0 >= per_roi) break;
        if constexpr (VEC) {
            float v[VE];
#pragma unroll
            for (int e = 0; e < VE; ++e) v[e] = mask_grad_elem(picked, tg, f0 + e, C, SS, channels_last != 0, lab, scale);
            store_vec<DT>(grad, roi_base + f0, v);
        } else {
            store1<DT>(grad, roi_base + f0, mask_grad_elem(picked, tg, f0, C, SS, channels_last != 0, lab, scale));
        }
    }
}

// ---- rpn_losses ------------------------------------------------------------------------------------------------------------------------
// does slot s of image b count for the class loss / the box loss?  An index outside [0, A) makes the slot invalid for both.
__device__ inline bool cls_slot(const long long* idx, const float* valid, int s, int A) {
    const long long a = idx[s];
    return valid[s] != 0.f && a >= 0 && a < A;
}
__device__ inline bool reg_slot(const long long* idx, const unsigned char* pos_valid, int s, int P, int A) {
    if (s >= P || !pos_valid[s]) return false;
    const long long a = idx[s];
    return a >= 0 && a < A;
}
// max(sum of the counted slots' valid, 1)
__device__ inline double rpn_avg(const long long* idx, const float* valid, int S, int A, double* red) {
    double n = 0.0;
    for (int s = threadIdx.x; s < S; s += LOSS_THREADS)
        if (cls_slot(idx, valid, s, A)) n += (double)valid[s];
    return fmax(block_sum(n, red), 1.0);
}

// grid B
__global__ __launch_bounds__(LOSS_THREADS) void rpn_losses_fwd_kernel(const float* __restrict__ cls_all, const float* __restrict__ reg_all,
                                                                     const long long* __restrict__ idx, const float* __restrict__ valid,
                                                                     const unsigned char* __restrict__ pos_valid, const float* __restrict__ reg_t,
                                                                     int A, int S, int P, float* __restrict__ out) {
    __shared__ double red[LOSS_THREADS];
    const int b = blockIdx.x;
    idx += (size_t)b * S;
    valid += (size_t)b * S;
    pos_valid += (size_t)b * P;
    const double avg = rpn_avg(idx, valid, S, A, red);
    double lc = 0.0, lr = 0.0;
    for (int s = threadIdx.x; s < S; s += LOSS_THREADS) {
        if (cls_slot(idx, valid, s, A)) lc += (double)valid[s] * bce_logits((double)cls_all[(size_t)b * A + (size_t)idx[s]], s < P ? 1.0 : 0.0);
        if (reg_slot(idx, pos_valid, s, P, A)) {
            const f32x4 d = reinterpret_cast<const f32x4*>(reg_all)[(size_t)b * A + (size_t)idx[s]];
            const f32x4 tg = reinterpret_cast<const f32x4*>(reg_t)[(size_t)b * P + s];
            lr += ((fabs((double)d[0] - (double)tg[0]) + fabs((double)d[1] - (double)tg[1])) + fabs((double)d[2] - (double)tg[2])) +
                  fabs((double)d[3] - (double)tg[3]);
        }
    }
    lc = block_sum(lc, red);
    lr = block_sum(lr, red);
    if (threadIdx.x == 0) {
        out[2 * b] = (float)(lc / avg);
        out[2 * b + 1] = (float)(lr / avg);
    }
}

// grid (ceil(A / RPN_CHUNK), B)
__global__ __launch_bounds__(LOSS_THREADS) void rpn_losses_bwd_kernel(const float* __restrict__ cls_all, const float* __restrict__ reg_all,
                                                                     const long long* __restrict__ idx, const float* __restrict__ valid,
                                                                     const unsigned char* __restrict__ pos_valid, const float* __restrict__ reg_t,
                                                                     const float* __restrict__ grad_out, int A, int S, int P,
                                                                     float* __restrict__ grad_cls, float* __restrict__ grad_reg) {
    __shared__ double red[LOSS_THREADS];
    __shared__ int s_slot[RPN_CHUNK];                                         // the slot that names the anchor, or -1
    const int b = blockIdx.y, a0 = blockIdx.x * RPN_CHUNK;
    const int n = A - a0 < RPN_CHUNK ? A - a0 : RPN_CHUNK;
    idx += (size_t)b * S;
    valid += (size_t)b * S;
    pos_valid += (size_t)b * P;
    for (int i = threadIdx.x; i < n; i += LOSS_THREADS) s_slot[i] = -1;
    const double avg = rpn_avg(idx, valid, S, A, red);                        // (its barriers also order the fill before the marks)
    for (int s = threadIdx.x; s < S; s += LOSS_THREADS) {
        // an invalid slot is skipped: it may name the anchor of a valid one.  The counted slots of an image name distinct anchors.
        if (!cls_slot(idx, valid, s, A) && !reg_slot(idx, pos_valid, s, P, A)) continue;
        const long long a = idx[s];
        if (a >= a0 && a < a0 + n) s_slot[(int)(a - a0)] = s;
    }
    __syncthreads();
    const double gc = (double)grad_out[2 * b] / avg, gr = (double)grad_out[2 * b + 1] / avg;
    const float up_reg = (float)gr;
    for (int i = threadIdx.x; i < n; i += LOSS_THREADS) {
        const int s = s_slot[i];
        const size_t a = (size_t)b * A + a0 + i;
        float dc = 0.f;
        f32x4 dr = {0.f, 0.f, 0.f, 0.f};
        if (s >= 0) {
            if (cls_slot(idx, valid, s, A)) dc = (float)((double)valid[s] * (sigmoid_d((double)cls_all[a]) - (s < P ? 1.0 : 0.0)) * gc);
            if (reg_slot(idx, pos_valid, s, P, A)) {
                const f32x4 d = reinterpret_cast<const f32x4*>(reg_all)[a];
                const f32x4 tg = reinterpret_cast<const f32x4*>(reg_t)[(size_t)b * P + s];
                dr = f32x4{signed_by(d[0] - tg[0], up_reg), signed_by(d[1] - tg[1], up_reg), signed_by(d[2] - tg[2], up_reg),
                           signed_by(d[3] - tg[3], up_reg)};
            }
        }
        grad_cls[a] = dc;
        reinterpret_cast<f32x4*>(grad_reg)[a] = dr;
    }
}

// ---- argument checks -------------------------------------------------------------------------------------------------------------------
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool aligned_elem(const void* p, int dt) { return dt == PSWIN_F32 ? aligned4(p) : (reinterpret_cast<uintptr_t>(p) & 1) == 0; }
// rows of 4 C elements read and written four at a time: 16-byte groups in f32, 8-byte groups in bf16
inline bool aligned_quad(const void* p, int dt) { return dt == PSWIN_F32 ? aligned16(p) : aligned8(p); }

bool ce_args_ok(const void* cls, int dt, const long long* labels, int N, int C) {
    if (!cls || !labels || !valid_dtype(dt) || N < 1 || C < 1 || C > LOSS_CMAX || (long long)N * (C + 1) > 0x7fffffffLL) return false;
    return aligned_elem(cls, dt) && aligned8(labels);
}

bool l1_args_ok(const void* reg, int dt, const long long* labels, const float* weight, const float* target, int N, int C) {
    if (!reg || !labels || !weight || !target || !valid_dtype(dt) || N < 1 || C < 1 || C > LOSS_CMAX || (long long)N * 4 * C > 0x7fffffffLL)
        return false;
    return aligned_quad(reg, dt) && aligned8(labels) && aligned4(weight) && aligned16(target);
}

// tensor: the [M][C][S][S] tensor of the call (the logits of the forward, the gradient of the backward)
bool mask_args_ok(const void* tensor, int dt, const long long* labels, const float* target, const float* weight, int M, int C, int S) {
    if (!tensor || !labels || !target || !weight || !valid_dtype(dt) || M < 1 || C < 1 || C > LOSS_CMAX || S < 1 || S > MASK_SMAX) return false;
    if ((long long)M * C * S * S > 0x7fffffffLL) return false;
    return aligned_elem(tensor, dt) && aligned8(labels) && aligned4(target) && aligned4(weight);
}

// the two dense layouts of [M][C][S][S] logits: 0 = NCHW, 1 = channels-last, -1 = neither
int mask_layout(long long sn, long long sc, long long sy, long long sx, int C, int S) {
    if (sn != (long long)C * S * S) return -1;
    if (sc == (long long)S * S && sy == S && sx == 1) return 0;
    if (sc == 1 && sy == (long long)S * C && sx == C) return 1;
    return -1;
}

bool rpn_args_ok(const float* cls_all, const float* reg_all, const long long* idx, const float* valid, const unsigned char* pos_valid,
                 const float* reg_t, int B, int A, int S, int P) {
    if (!cls_all || !reg_all || !idx || !valid || !pos_valid || !reg_t) return false;
    if (B < 1 || B > 65535 || A < 1 || S < 1 || P < 1 || P > S || (long long)B * A * 4 > 0x7fffffffLL || (long long)B * S > 0x7fffffffLL) return false;
    return aligned4(cls_all) && aligned16(reg_all) && aligned8(idx) && aligned4(valid) && aligned16(reg_t);
}

}  // namespace

extern "C" {

int pswin_losses_rows_per_workgroup(void) { return LOSS_ROWS; }
int pswin_rpn_losses_chunk(void) { return RPN_CHUNK; }

int pswin_ce_rows_fwd(const void* cls, int dtype, const long long* labels, int N, int C, float* out, void* stream) {
    PSWIN_CHECK_ARG(out && aligned4(out) && ce_args_ok(cls, dtype, labels, N, C));
    const dim3 grid((N + LOSS_ROWS - 1) / LOSS_ROWS);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(ce_rows_fwd_kernel<PSWIN_F32>, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, cls, labels, N, C + 1, out);
    else
        hipLaunchKernelGGL(ce_rows_fwd_kernel<PSWIN_BF16>, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, cls, labels, N, C + 1, out);
    PSWIN_LAUNCH_RET();
}

int pswin_ce_rows_bwd(const void* cls, int dtype, const long long* labels, const float* grad_rows, int N, int C, void* grad, void* stream) {
    PSWIN_CHECK_ARG(grad_rows && grad && aligned4(grad_rows) && ce_args_ok(cls, dtype, labels, N, C) && aligned_elem(grad, dtype));
    const dim3 grid((N + LOSS_ROWS - 1) / LOSS_ROWS);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(ce_rows_bwd_kernel<PSWIN_F32>, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, cls, labels, grad_rows, N, C + 1, grad);
    else
        hipLaunchKernelGGL(ce_rows_bwd_kernel<PSWIN_BF16>, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, cls, labels, grad_rows, N, C + 1, grad);
    PSWIN_LAUNCH_RET();
}

int pswin_l1_rows_fwd(const void* reg, int dtype, const long long* labels, const float* weight, const float* target, int N, int C, float* out,
                      void* stream) {
    PSWIN_CHECK_ARG(out && aligned4(out) && l1_args_ok(reg, dtype, labels, weight, target, N, C));
    const dim3 grid((N + LOSS_ROWS - 1) / LOSS_ROWS);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(l1_rows_fwd_kernel<PSWIN_F32>, grid, dim3(LOSS_ROWS), 0, (hipStream_t)stream, reg, labels, weight, target, N, C, out);
    else
        hipLaunchKernelGGL(l1_rows_fwd_kernel<PSWIN_BF16>, grid, dim3(LOSS_ROWS), 0, (hipStream_t)stream, reg, labels, weight, target, N, C, out);
    PSWIN_LAUNCH_RET();
}

int pswin_l1_rows_bwd(const void* reg, int dtype, const long long* labels, const float* weight, const float* target, const float* grad_rows, int N,
                      int C, void* grad, void* stream) {
    PSWIN_CHECK_ARG(grad_rows && grad && aligned4(grad_rows) && l1_args_ok(reg, dtype, labels, weight, target, N, C) && aligned_quad(grad, dtype));
    const dim3 grid((N + LOSS_ROWS - 1) / LOSS_ROWS);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(l1_rows_bwd_kernel<PSWIN_F32>, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, reg, labels, weight, target, grad_rows, N,
                           C, grad);
    else
        hipLaunchKernelGGL(l1_rows_bwd_kernel<PSWIN_BF16>, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, reg, labels, weight, target, grad_rows, N,
                           C, grad);
    PSWIN_LAUNCH_RET();
}

int pswin_mask_bce_rows_fwd(const void* logits, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                            const long long* labels, const float* target, const float* weight, int M, int C, int S, float* out, float* picked,
                            void* stream) {
    PSWIN_CHECK_ARG(out && aligned4(out) && aligned4(picked) && mask_args_ok(logits, dtype, labels, target, weight, M, C, S));
    PSWIN_CHECK_ARG(stride_n >= 1 && stride_c >= 1 && stride_y >= 1 && stride_x >= 1);
    PSWIN_CHECK_ARG((M - 1) * stride_n + (C - 1) * stride_c + (S - 1) * (stride_y + stride_x) <= 0x7fffffffLL);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(mask_bce_fwd_kernel<PSWIN_F32>, dim3(M), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, stride_n, stride_c, stride_y,
                           stride_x, labels, target, weight, C, S, out, picked);
    else
        hipLaunchKernelGGL(mask_bce_fwd_kernel<PSWIN_BF16>, dim3(M), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, stride_n, stride_c, stride_y,
                           stride_x, labels, target, weight, C, S, out, picked);
    PSWIN_LAUNCH_RET();
}

int pswin_mask_bce_rows_bwd(const float* picked, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                            const long long* labels, const float* target, const float* weight, const float* grad_rows, int M, int C, int S,
                            void* grad, void* stream) {
    PSWIN_CHECK_ARG(picked && grad_rows && aligned4(picked) && aligned4(grad_rows) && mask_args_ok(grad, dtype, labels, target, weight, M, C, S));
    const int layout = mask_layout(stride_n, stride_c, stride_y, stride_x, C, S);
    PSWIN_CHECK_ARG(layout >= 0);
    const int per_roi = C * S * S;
    const int ve = dtype == PSWIN_F32 ? 4 : 8;
    const bool vec = per_roi % ve == 0 && aligned16(grad);
    const int groups = vec ? per_roi / ve : per_roi;
    const int per_block = LOSS_THREADS * MASK_GROUPS_PER_THREAD;
    const int bpr = (groups + per_block - 1) / per_block;
    PSWIN_CHECK_ARG((long long)M * bpr <= 0x7fffffffLL);
    const dim3 grid((unsigned)(M * bpr));
#define PSWIN_MASK_BWD(DT, VEC)                                                                                                          \
    hipLaunchKernelGGL((mask_bce_bwd_kernel<DT, VEC>), grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, picked, layout, labels, target, weight, \
                       grad_rows, C, S, bpr, grad)
    if (dtype == PSWIN_F32) {
        if (vec) PSWIN_MASK_BWD(PSWIN_F32, true);
        else PSWIN_MASK_BWD(PSWIN_F32, false);
    } else {
        if (vec) PSWIN_MASK_BWD(PSWIN_BF16, true);
        else PSWIN_MASK_BWD(PSWIN_BF16, false);
    }
#undef PSWIN_MASK_BWD
    PSWIN_LAUNCH_RET();
}

int pswin_rpn_losses_fwd(const float* cls_all, const float* reg_all, const long long* idx, const float* valid, const unsigned char* pos_valid,
                         const float* reg_t, int B, int A, int S, int P, float* out, void* stream) {
    PSWIN_CHECK_ARG(out && aligned4(out) && rpn_args_ok(cls_all, reg_all, idx, valid, pos_valid, reg_t, B, A, S, P));
    hipLaunchKernelGGL(rpn_losses_fwd_kernel, dim3(B), dim3(LOSS_THREADS), 0, (hipStream_t)stream, cls_all, reg_all, idx, valid, pos_valid, reg_t, A,
                       S, P, out);
    PSWIN_LAUNCH_RET();
}

int pswin_rpn_losses_bwd(const float* cls_all, const float* reg_all, const long long* idx, const float* valid, const unsigned char* pos_valid,
                         const float* reg_t, const float* grad_out, int B, int A, int S, int P, float* grad_cls, float* grad_reg, void* stream) {
    PSWIN_CHECK_ARG(grad_out && grad_cls && grad_reg && aligned4(grad_out) && aligned4(grad_cls) && aligned16(grad_reg));
    PSWIN_CHECK_ARG(rpn_args_ok(cls_all, reg_all, idx, valid, pos_valid, reg_t, B, A, S, P));
    const dim3 grid((A + RPN_CHUNK - 1) / RPN_CHUNK, B);
    hipLaunchKernelGGL(rpn_losses_bwd_kernel, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, cls_all, reg_all, idx, valid, pos_valid, reg_t,
                       grad_out, A, S, P, grad_cls, grad_reg);
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
