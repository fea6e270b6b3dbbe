// Cascade R-CNN's two device-side pieces for a padded batch (cascade.refine_rois / cascade.giou_rows: what MiniCascadeRCNN does between
// a stage's box head and the next stage's assigner, and its box loss on decoded boxes) -- gfx950 only.
//
// Everything is read from device memory in place (the box head's logits and deltas as f32 or bf16), nothing is read back and no buffer
// has to be cleared between calls: every element of every output is written by plain vector stores, so a captured step replays on the
// same buffers.  No atomics, no workspace, no state.
//
// ARITHMETIC.  The decoder and the GIoU are evaluated in double from the float inputs and rounded once, as pswin_detect.hip does for its
// decoder: a row is a few dozen operations, the kernels are latency-bound either way, and the result is then within half a float32 ulp
// (plus exp's error) of the float64 definition whatever cancellation the boxes hold.
//
// REFINE (cascade_refine_kernel): CASCADE_ROWS rows per workgroup, four lanes per row.  Lane q scans classes q, q + 4, ... for the first
// maximum of ITS classes (strict >), the four candidates are merged by (value, then lower index): torch.argmax's answer on the same values,
// ties included (bf16 logits tie often).  Lane 0 of the row gathers the four deltas of the class, decodes, clips and stores.
//
// GIOU ROWS (giou_rows_fwd_kernel): one row per lane.  (giou_rows_bwd_kernel): a workgroup of 256 threads takes CASCADE_ROWS rows; the
// first CASCADE_ROWS lanes recompute the forward of one row each and leave its four delta gradients and its label in LDS, then all
// threads write the rows' 4 C gradient columns class by class -- the four values in the label's class of a weighted row, zeros elsewhere.
#include "pswin_common.hpp"

namespace {
using namespace pswin;

constexpr int CASCADE_ROWS = 64;
constexpr int CASCADE_THREADS = 256;            // refine: 4 lanes per row; backward: all threads store
constexpr int CASCADE_CMAX = 128;
constexpr double WH_CLIP = 4.135166556742356;   // |log(16 / 1000)|

template <int DT>
__device__ inline float load1(const void* base, size_t o) {
    if constexpr (DT == PSWIN_F32) return reinterpret_cast<const float*>(base)[o];
    else return bf16_bits_to_f32(reinterpret_cast<const unsigned short*>(base)[o]);
}

struct Box {
    double x1, y1, x2, y2;
};

// detector.decode_deltas without the clip to an image; d: the four raw deltas, s: the stds
__device__ inline Box decode_box(f32x4 roi, f32x4 d, f32x4 s, double& gw, double& gh) {
    const double dx = (double)d[0] * (double)s[0], dy = (double)d[1] * (double)s[1];
    const double dw = fmin(fmax((double)d[2] * (double)s[2], -WH_CLIP), WH_CLIP), dh = fmin(fmax((double)d[3] * (double)s[3], -WH_CLIP), WH_CLIP);
    const double pw = (double)roi[2] - (double)roi[0], ph = (double)roi[3] - (double)roi[1];
    const double px = ((double)roi[0] + (double)roi[2]) * 0.5, py = ((double)roi[1] + (double)roi[3]) * 0.5;
    gw = pw * exp(dw);
    gh = ph * exp(dh);
    const double gx = px + pw * dx, gy = py + ph * dy;
    return Box{gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5};
}

__device__ inline int clamp_label(long long v, int C) { return v < 0 ? 0 : (v > C - 1 ? C - 1 : (int)v); }

// grid (ceil(R / CASCADE_ROWS), B)
template <int CDT, int DDT>
__global__ __launch_bounds__(CASCADE_THREADS) void cascade_refine_kernel(const float* __restrict__ rois, const void* __restrict__ cls,
                                                                        const void* __restrict__ deltas, const long long* __restrict__ labels,
                                                                        int R, int C, f32x4 stds, float img_h, float img_w,
                                                                        float* __restrict__ new_rois, long long* __restrict__ used) {
    const int q = threadIdx.x & 3;
    const int r = blockIdx.x * CASCADE_ROWS + (threadIdx.x >> 2);
    const bool live = r < R;
    const size_t row = (size_t)blockIdx.y * R + (live ? r : R - 1);           // a dead lane reads the last row and writes nothing
    const long long lab = labels ? labels[row] : (long long)C;
    int best_i = C;
    float best_v = 0.f;
    if (lab >= C) {                                                           // uniform over the four lanes of a row
        for (int c = q; c < C; c += 4) {
            const float v = load1<CDT>(cls, row * (size_t)(C + 1) + c);
            // first maximum; a NaN counts as the maximum, as torch.argmax has it
            if (best_i == C || v > best_v || (v != v && best_v == best_v)) {
                best_v = v;
                best_i = c;
            }
        }
#pragma unroll
        for (int s = 1; s <= 2; s <<= 1) {
            const float ov = __shfl_xor(best_v, s, 64);
            const int oi = __shfl_xor(best_i, s, 64);
            const bool mine_nan = best_v != best_v, other_nan = ov != ov;
            const bool take = oi < C && (best_i == C || (other_nan && !mine_nan) || (!mine_nan && !other_nan && ov > best_v) ||
                                         ((ov == best_v || (mine_nan && other_nan)) && oi < best_i));
            if (take) {
                best_v = ov;
                best_i = oi;
            }
        }
    }
    if (!live || q != 0) return;
    const int u = lab >= C ? best_i : clamp_label(lab, C);
    const f32x4 roi = reinterpret_cast<const f32x4*>(rois)[row];
    const f32x4 d = load4<DDT>(deltas, row * (size_t)(4 * C) + 4 * (size_t)u);
    double gw, gh;
    const Box b = decode_box(roi, d, stds, gw, gh);
    const double W = img_w, H = img_h;
    reinterpret_cast<f32x4*>(new_rois)[row] = f32x4{(float)fmin(fmax(b.x1, 0.0), W), (float)fmin(fmax(b.y1, 0.0), H),
                                                    (float)fmin(fmax(b.x2, 0.0), W), (float)fmin(fmax(b.y2, 0.0), H)};
    used[row] = u;
}

// torch's rule for the gradient of max(a, b) / min(a, b) towards a: all of it where a wins, half on a tie, nothing where it loses
__device__ inline double share_max(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ inline double share_min(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }

// One row of cascade.giou_rows: the value 1 - GIoU(decoded box, target) (mmdet bbox_overlaps(mode='giou', is_aligned=True), operation by
// operation) and, if GRAD, its gradient with respect to the four raw deltas.
template <bool GRAD>
__device__ inline double giou_row(f32x4 roi, f32x4 d, f32x4 s, f32x4 tgt, double eps, double (&dd)[4]) {
    double gw, gh;
    const Box p = decode_box(roi, d, s, gw, gh);
    const double t0 = tgt[0], t1 = tgt[1], t2 = tgt[2], t3 = tgt[3];
    const double area1 = (p.x2 - p.x1) * (p.y2 - p.y1), area2 = (t2 - t0) * (t3 - t1);
    const double ltx = fmax(p.x1, t0), lty = fmax(p.y1, t1), rbx = fmin(p.x2, t2), rby = fmin(p.y2, t3);
    const double w0 = fmax(rbx - ltx, 0.0), w1 = fmax(rby - lty, 0.0);
    const double overlap = w0 * w1;
    const double union_raw = area1 + area2 - overlap;
    const double uni = fmax(union_raw, eps);
    const double iou = overlap / uni;
    const double ex0 = fmin(p.x1, t0), ey0 = fmin(p.y1, t1), ex1 = fmax(p.x2, t2), ey1 = fmax(p.y2, t3);
    const double e0 = fmax(ex1 - ex0, 0.0), e1 = fmax(ey1 - ey0, 0.0);
    const double ea_raw = e0 * e1;
    const double ea = fmax(ea_raw, eps);
    const double giou = iou - (ea - uni) / ea;
    if constexpr (GRAD) {
        // d(1 - giou): giou = overlap / uni - 1 + uni / ea
        const double g_uni = -(1.0 / ea - overlap / (uni * uni)) * share_max(union_raw, eps);
        const double g_ea = (uni / (ea * ea)) * share_max(ea_raw, eps);
        const double g_ov = -(1.0 / uni) - g_uni;
        const double g_w0 = (rbx - ltx >= 0.0) ? g_ov * w1 : 0.0, g_w1 = (rby - lty >= 0.0) ? g_ov * w0 : 0.0;
        const double g_e0 = (ex1 - ex0 >= 0.0) ? g_ea * e1 : 0.0, g_e1 = (ey1 - ey0 >= 0.0) ? g_ea * e0 : 0.0;
        const double pw = p.x2 - p.x1, ph = p.y2 - p.y1;
        const double g_x1 = -g_w0 * share_max(p.x1, t0) - g_e0 * share_min(p.x1, t0) - g_uni * ph;
        const double g_y1 = -g_w1 * share_max(p.y1, t1) - g_e1 * share_min(p.y1, t1) - g_uni * pw;
        const double g_x2 = g_w0 * share_min(p.x2, t2) + g_e0 * share_max(p.x2, t2) + g_uni * ph;
        const double g_y2 = g_w1 * share_min(p.y2, t3) + g_e1 * share_max(p.y2, t3) + g_uni * pw;
        const double rw = (double)roi[2] - (double)roi[0], rh = (double)roi[3] - (double)roi[1];
        const double s2 = (double)d[2] * (double)s[2], s3 = (double)d[3] * (double)s[3];
        dd[0] = (g_x1 + g_x2) * rw * (double)s[0];
        dd[1] = (g_y1 + g_y2) * rh * (double)s[1];
        dd[2] = (s2 >= -WH_CLIP && s2 <= WH_CLIP) ? (g_x2 - g_x1) * 0.5 * gw * (double)s[2] : 0.0;     // torch's clamp: passed on the bounds
        dd[3] = (s3 >= -WH_CLIP && s3 <= WH_CLIP) ? (g_y2 - g_y1) * 0.5 * gh * (double)s[3] : 0.0;
    }
    return 1.0 - giou;
}

template <int DDT>
__global__ __launch_bounds__(CASCADE_ROWS) void giou_rows_fwd_kernel(const float* __restrict__ rois, const void* __restrict__ deltas,
                                                                    const long long* __restrict__ labels, const float* __restrict__ weight,
                                                                    const float* __restrict__ target, int N, int C, f32x4 stds, double eps,
                                                                    float* __restrict__ out) {
    const int n = blockIdx.x * CASCADE_ROWS + threadIdx.x;
    if (n >= N) return;
    const float w = weight[n];
    float v = 0.f;
    if (w != 0.f) {                                                           // a weight-0 row reads nothing else
        const int c = clamp_label(labels[n], C);
        double dd[4];
        const double l = giou_row<false>(reinterpret_cast<const f32x4*>(rois)[n], load4<DDT>(deltas, (size_t)n * (4 * C) + 4 * (size_t)c), stds,
                                         reinterpret_cast<const f32x4*>(target)[n], eps, dd);
        v = (float)((double)w * l);
    }
    out[n] = v;
}

template <int DDT>
__global__ __launch_bounds__(CASCADE_THREADS) void giou_rows_bwd_kernel(const float* __restrict__ rois, const void* __restrict__ deltas,
                                                                       const long long* __restrict__ labels, const float* __restrict__ weight,
                                                                       const float* __restrict__ target, const float* __restrict__ grad_rows,
                                                                       int N, int C, f32x4 stds, double eps, void* __restrict__ grad_deltas) {
    __shared__ f32x4 s_grad[CASCADE_ROWS];
    __shared__ int s_class[CASCADE_ROWS];                                     // -1: the whole row is zeros
    const int t = threadIdx.x;
    const int row0 = blockIdx.x * CASCADE_ROWS;
    if (t < CASCADE_ROWS) {
        const int n = row0 + t;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        int cls = -1;
        if (n < N) {
            const float w = weight[n];
            if (w != 0.f) {
                cls = clamp_label(labels[n], C);
                double dd[4];
                giou_row<true>(reinterpret_cast<const f32x4*>(rois)[n], load4<DDT>(deltas, (size_t)n * (4 * C) + 4 * (size_t)cls), stds,
                               reinterpret_cast<const f32x4*>(target)[n], eps, dd);
                const double up = (double)grad_rows[n] * (double)w;
                g = f32x4{(float)(up * dd[0]), (float)(up * dd[1]), (float)(up * dd[2]), (float)(up * dd[3])};
            }
        }
        s_grad[t] = g;
        s_class[t] = cls;
    }
    __syncthreads();
    const int rows = N - row0 < CASCADE_ROWS ? N - row0 : CASCADE_ROWS;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = t; i < rows * C; i += CASCADE_THREADS) {
        const int r = i / C, c = i - r * C;
        store4<DDT>(grad_deltas, (size_t)(row0 + r) * (4 * C) + 4 * (size_t)c, c == s_class[r] ? s_grad[r] : zero);
    }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool stds_ok(const float* s) { return s && s[0] > 0.f && s[1] > 0.f && s[2] > 0.f && s[3] > 0.f; }

// rows of 4 C elements read and written four at a time: 16-byte groups in f32, 8-byte groups in bf16
inline bool deltas_aligned(const void* p, int dt) { return dt == PSWIN_F32 ? aligned16(p) : aligned8(p); }

bool giou_args_ok(const float* rois, const void* deltas, int dt, const long long* labels, const float* weight, const float* target, int N, int C,
                  const float* stds, double eps) {
    if (!rois || !deltas || !labels || !weight || !target || !valid_dtype(dt) || !stds_ok(stds)) return false;
    if (N < 1 || C < 1 || C > CASCADE_CMAX || (long long)N * 4 * C > 0x7fffffffLL || !(eps > 0.0)) return false;
    return aligned16(rois) && aligned16(target) && deltas_aligned(deltas, dt) && aligned8(labels) && aligned4(weight);
}

}  // namespace

extern "C" {

int pswin_cascade_rows_per_workgroup(void) { return CASCADE_ROWS; }

int pswin_cascade_refine(const float* rois, const void* cls, int cls_dtype, const void* deltas, int deltas_dtype, const long long* labels, int B,
                         int R, int C, const float* stds, int img_h, int img_w, float* new_rois, long long* used, void* stream) {
    PSWIN_CHECK_ARG(rois && cls && deltas && new_rois && used && valid_dtype(cls_dtype) && valid_dtype(deltas_dtype) && stds_ok(stds));
    PSWIN_CHECK_ARG(B >= 1 && B <= 65535 && R >= 1 && C >= 1 && C <= CASCADE_CMAX && img_h >= 1 && img_w >= 1);
    PSWIN_CHECK_ARG((long long)B * R * 4 * C <= 0x7fffffffLL);
    PSWIN_CHECK_ARG(aligned16(rois) && aligned16(new_rois) && deltas_aligned(deltas, deltas_dtype) && aligned8(used) && aligned8(labels));
    PSWIN_CHECK_ARG(cls_dtype == PSWIN_F32 ? aligned4(cls) : (reinterpret_cast<uintptr_t>(cls) & 1) == 0);
    const f32x4 s = {stds[0], stds[1], stds[2], stds[3]};
    const dim3 grid((R + CASCADE_ROWS - 1) / CASCADE_ROWS, B);
    return dispatch2(cls_dtype, deltas_dtype, [&](auto cdt, auto ddt) {
        hipLaunchKernelGGL((cascade_refine_kernel<decltype(cdt)::value, decltype(ddt)::value>), grid, dim3(CASCADE_THREADS), 0, (hipStream_t)stream,
                           rois, cls, deltas, labels, R, C, s, (float)img_h, (float)img_w, new_rois, used);
        PSWIN_LAUNCH_RET();
    });
}

int pswin_giou_rows_fwd(const float* rois, const void* deltas, int deltas_dtype, const long long* labels, const float* weight, const float* target,
                        int N, int C, const float* stds, double eps, float* out, void* stream) {
    PSWIN_CHECK_ARG(out && aligned4(out) && giou_args_ok(rois, deltas, deltas_dtype, labels, weight, target, N, C, stds, eps));
    const f32x4 s = {stds[0], stds[1], stds[2], stds[3]};
    const dim3 grid((N + CASCADE_ROWS - 1) / CASCADE_ROWS);
    if (deltas_dtype == PSWIN_F32)
        hipLaunchKernelGGL(giou_rows_fwd_kernel<PSWIN_F32>, grid, dim3(CASCADE_ROWS), 0, (hipStream_t)stream, rois, deltas, labels, weight, target, N,
                           C, s, eps, out);
    else
        hipLaunchKernelGGL(giou_rows_fwd_kernel<PSWIN_BF16>, grid, dim3(CASCADE_ROWS), 0, (hipStream_t)stream, rois, deltas, labels, weight, target, N,
                           C, s, eps, out);
    PSWIN_LAUNCH_RET();
}

int pswin_giou_rows_bwd(const float* rois, const void* deltas, int deltas_dtype, const long long* labels, const float* weight, const float* target,
                        const float* grad_rows, int N, int C, const float* stds, double eps, void* grad_deltas, void* stream) {
    PSWIN_CHECK_ARG(grad_rows && grad_deltas && aligned4(grad_rows) && valid_dtype(deltas_dtype) && deltas_aligned(grad_deltas, deltas_dtype));
    PSWIN_CHECK_ARG(giou_args_ok(rois, deltas, deltas_dtype, labels, weight, target, N, C, stds, eps));
    const f32x4 s = {stds[0], stds[1], stds[2], stds[3]};
    const dim3 grid((N + CASCADE_ROWS - 1) / CASCADE_ROWS);
    if (deltas_dtype == PSWIN_F32)
        hipLaunchKernelGGL(giou_rows_bwd_kernel<PSWIN_F32>, grid, dim3(CASCADE_THREADS), 0, (hipStream_t)stream, rois, deltas, labels, weight, target,
                           grad_rows, N, C, s, eps, grad_deltas);
    else
        hipLaunchKernelGGL(giou_rows_bwd_kernel<PSWIN_BF16>, grid, dim3(CASCADE_THREADS), 0, (hipStream_t)stream, rois, deltas, labels, weight,
                           target, grad_rows, N, C, s, eps, grad_deltas);
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
