// Detector inference behind the heads, for a whole batch with fixed shapes (the test-time counterpart of pswin_assign.hip) -- gfx950 only.
//
//   class-wise NMS (BBoxHead.get_bboxes -> multiclass_nms, mmdet/models/roi_heads/bbox_heads/bbox_head.py:270-371,
//   mmdet/core/post_processing/bbox_nms.py:7-93): detector.multiclass_nms for every image of a batch, the proposal count of each image
//   read from device memory.  Five small launches around the existing pswin_nms_groups, with two stable sorts of the caller between them:
//     (1) pswin_multiclass_nms_scores: softmax over the C + 1 logits of a proposal, threshold; key[b][c][r] = score or -1
//         -- the caller sorts every (image, class) list, descending and stable: equal scores stay in ascending proposal order --
//     (2) pswin_multiclass_nms: decode the candidates of every list in sorted order and count them; the 64-row bit-mask / single-wave
//         scan of pswin_nms_groups with (image, class) as the group, in slices of DET_NMS_SLICE groups that share one mask workspace;
//         then final[b][r * C + c] = score of a survivor or -1 (every entry is written: the lists' orders are permutations)
//         -- the caller sorts every image's final row, descending and stable: equal scores stay in ascending r * C + c --
//     (3) pswin_multiclass_nms_select: the first K of that order -> boxes, scores, labels, source, count; rows past the count are zeros.
//   Worst case (every proposal of every class above the threshold and nothing suppressed): B * C groups of R rows, R^2 / 2 IoUs and a
//   walk over R rows each -- nothing depends on how many candidates there are except the work the NMS skips.
//   Softmax and the delta decoder are evaluated in double and rounded once (a proposal row is 129 logits at most; the decode runs per
//   candidate): the same formulas as F.softmax and detector.decode_deltas, so the float64 definition is met to half an ulp.
//
//   mask paste (FCNMaskHead.get_seg_masks / _do_paste_mask(skip_empty=False), mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:169-377):
//   pswin_paste_masks, one launch.  A workgroup stages sigmoid(logits) of its detection's class channel in LDS (f32, with a zero border:
//   grid_sample's zero padding without a bounds test), then samples it bilinearly for PASTE_ROWS image rows with grid_sample's
//   align_corners=False geometry and stores (value >= thr) as bytes, 16 pixels per lane and store where the row's address allows.
//   Neither the float image nor the sampling grid exists in memory; rows of detections past the image's count are written as zeros.
#include "pswin_detect_post.hpp"

namespace {
using namespace pswin;

struct DetDecode {
    float std[4];
    float img_h, img_w;
    const float* scale;                                 // f32 [B][4] (w, h, w, h) or NULL
    const float* rois;                                  // f32 [B][R][4]
    const void* deltas;                                 // [B][R][4 C]
    int deltas_dt, R, C;
    __device__ inline f32x4 operator()(int b, int r, int c) const;   // det_box: what the chain's kernels call (pswin_detect_post.hpp)
};

// detector.decode_deltas for class c of proposal r of image b (means 0, the width / height deltas clamped at |log(16 / 1000)|, the box
// clipped to the image), then divided by the image's scale factor: in double, rounded once
__device__ inline f32x4 det_box(const DetDecode& p, int b, int r, int c) {
    const f32x4 s = reinterpret_cast<const f32x4*>(p.rois)[(size_t)b * p.R + r];
    const size_t o = ((size_t)b * p.R + r) * (size_t)(4 * p.C) + 4 * c;
    const double clip = 4.135166556742356;              // |log(16 / 1000)|
    const double dx = (double)det_load(p.deltas, p.deltas_dt, o) * (double)p.std[0];
    const double dy = (double)det_load(p.deltas, p.deltas_dt, o + 1) * (double)p.std[1];
    const double dw = fmin(fmax((double)det_load(p.deltas, p.deltas_dt, o + 2) * (double)p.std[2], -clip), clip);
    const double dh = fmin(fmax((double)det_load(p.deltas, p.deltas_dt, o + 3) * (double)p.std[3], -clip), clip);
    const double sw = (double)s[2] - (double)s[0], sh = (double)s[3] - (double)s[1];
    const double sx = ((double)s[0] + (double)s[2]) * 0.5, sy = ((double)s[1] + (double)s[3]) * 0.5;
    const double w = sw * exp(dw), h = sh * exp(dh), x = sx + sw * dx, y = sy + sh * dy;
    const double W = p.img_w, H = p.img_h;
    double x1 = fmin(fmax(x - w * 0.5, 0.0), W), y1 = fmin(fmax(y - h * 0.5, 0.0), H);
    double x2 = fmin(fmax(x + w * 0.5, 0.0), W), y2 = fmin(fmax(y + h * 0.5, 0.0), H);
    if (p.scale) {
        const f32x4 f = reinterpret_cast<const f32x4*>(p.scale)[b];
        x1 /= (double)f[0];
        y1 /= (double)f[1];
        x2 /= (double)f[2];
        y2 /= (double)f[3];
    }
    return f32x4{(float)x1, (float)y1, (float)x2, (float)y2};
}

__device__ inline f32x4 DetDecode::operator()(int b, int r, int c) const { return det_box(*this, b, r, c); }

// (1) one thread per proposal: key[b][c][r] = softmax(logits[b][r])[c] if it is above the threshold and r < roi_count[b], else -1
__global__ __launch_bounds__(DET_THREADS) void det_scores_kernel(const void* __restrict__ cls, int cls_dt, const int* __restrict__ roi_count, int R,
                                                                 int C, float score_thr, float* __restrict__ keys) {
    const int b = blockIdx.y, r = blockIdx.x * DET_THREADS + threadIdx.x;
    if (r >= R) return;
    const int n = det_clamp(roi_count[b], R);
    float* kp = keys + (size_t)b * C * R + r;
    if (r >= n) {
        for (int c = 0; c < C; ++c) kp[(size_t)c * R] = -1.f;
        return;
    }
    const size_t row = ((size_t)b * R + r) * (size_t)(C + 1);
    float m = det_load(cls, cls_dt, row);
    for (int c = 1; c <= C; ++c) m = fmaxf(m, det_load(cls, cls_dt, row + c));
    double sum = 0.0;
    for (int c = 0; c <= C; ++c) sum += exp((double)det_load(cls, cls_dt, row + c) - (double)m);
    for (int c = 0; c < C; ++c) {
        const float p = (float)(exp((double)det_load(cls, cls_dt, row + c) - (double)m) / sum);
        kp[(size_t)c * R] = p > score_thr ? p : -1.f;
    }
}

DetDecode det_decode_args(const float* rois, const void* deltas, int deltas_dtype, const float* stds, int img_h, int img_w, const float* scale, int R,
                          int C) {
    DetDecode p;
    for (int i = 0; i < 4; ++i) p.std[i] = stds[i];
    p.img_h = (float)img_h;
    p.img_w = (float)img_w;
    p.scale = scale;
    p.rois = rois;
    p.deltas = deltas;
    p.deltas_dt = deltas_dtype;
    p.R = R;
    p.C = C;
    return p;
}

// ---- mask paste: the staging of one source; the sampling and the stores are paste_rows (pswin_detect_post.hpp) --------------------------------
template <int DT>
__global__ __launch_bounds__(PASTE_THREADS) void paste_kernel(const void* __restrict__ logits, long long sn, long long sc, long long sy,
                                                              long long sx, const long long* __restrict__ labels, const float* __restrict__ boxes,
                                                              const int* __restrict__ count, int K, int C, int H, int W, float thr,
                                                              unsigned char* __restrict__ out) {
    __shared__ float prob[PASTE_LD * PASTE_LD];
    const int b = blockIdx.z, k = blockIdx.y, ybase = blockIdx.x * PASTE_ROWS;
    const size_t det = (size_t)b * K + k;
    const bool live = k < det_clamp(count[b], K);       // the same for the whole workgroup
    f32x4 box = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        box = reinterpret_cast<const f32x4*>(boxes)[det];
        paste_stage<DT>(prob, logits, sn, sc, sy, sx, det, paste_channel(labels[det], C));
    }
    paste_rows(prob, live, box, det, ybase, H, W, thr, out);
}

}  // namespace

extern "C" {

int pswin_multiclass_nms_workspace(int B, int R, int C) {
    if (!det_shape_ok(B, R, C)) return PSWIN_ERR_ARG;
    const DetWorkspace w = det_workspace(B, R, C);
    return w.total <= 0x7fffffffull ? (int)w.total : PSWIN_ERR_ARG;
}

int pswin_multiclass_nms_scores(const void* cls, int cls_dtype, const int32_t* roi_count, int B, int R, int C, float score_thr, float* keys,
                                void* stream) {
    PSWIN_CHECK_ARG(cls && roi_count && keys && valid_dtype(cls_dtype) && det_shape_ok(B, R, C) && score_thr >= 0.f);
    PSWIN_CHECK_ARG((reinterpret_cast<uintptr_t>(cls) & 3) == 0 && (reinterpret_cast<uintptr_t>(keys) & 3) == 0);
    hipLaunchKernelGGL(det_scores_kernel, dim3((R + DET_THREADS - 1) / DET_THREADS, B), dim3(DET_THREADS), 0, (hipStream_t)stream, cls, cls_dtype,
                       roi_count, R, C, score_thr, keys);
    PSWIN_LAUNCH_RET();
}

int pswin_multiclass_nms(const float* sorted_keys, const long long* sorted_index, const float* rois, const void* deltas, int deltas_dtype,
                         const float* stds, int img_h, int img_w, const float* scale, int B, int R, int C, float iou_thr, float* final_keys,
                         void* workspace, void* stream) {
    PSWIN_CHECK_ARG(sorted_keys && sorted_index && rois && deltas && stds && final_keys && workspace && valid_dtype(deltas_dtype));
    PSWIN_CHECK_ARG(det_shape_ok(B, R, C) && img_h >= 1 && img_w >= 1 && iou_thr >= 0.f);
    PSWIN_CHECK_ARG(aligned16(rois) && aligned16(workspace) && (!scale || aligned16(scale)) && (reinterpret_cast<uintptr_t>(sorted_index) & 7) == 0);
    PSWIN_CHECK_ARG((reinterpret_cast<uintptr_t>(deltas) & 7) == 0 && (reinterpret_cast<uintptr_t>(sorted_keys) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(final_keys) & 3) == 0);
    return det_nms_lists(sorted_keys, sorted_index, det_decode_args(rois, deltas, deltas_dtype, stds, img_h, img_w, scale, R, C), B, iou_thr,
                         final_keys, workspace, stream);
}

int pswin_multiclass_nms_select(const float* top_keys, const long long* top_index, long long row_stride, int n_sorted, const float* rois,
                                const void* deltas, int deltas_dtype, const float* stds, int img_h, int img_w, const float* scale, int B, int R,
                                int C, int K, float* boxes, float* scores, long long* labels, int32_t* source, int32_t* count, void* stream) {
    PSWIN_CHECK_ARG(top_keys && top_index && rois && deltas && stds && boxes && scores && labels && source && count && valid_dtype(deltas_dtype));
    PSWIN_CHECK_ARG(det_shape_ok(B, R, C) && K >= 1 && K <= DET_KMAX && img_h >= 1 && img_w >= 1);
    PSWIN_CHECK_ARG(n_sorted >= 1 && n_sorted <= R * C && row_stride >= n_sorted);
    PSWIN_CHECK_ARG(aligned16(rois) && aligned16(boxes) && (!scale || aligned16(scale)) && (reinterpret_cast<uintptr_t>(deltas) & 7) == 0);
    PSWIN_CHECK_ARG((reinterpret_cast<uintptr_t>(top_index) & 7) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(top_keys) & 3) == 0 && (reinterpret_cast<uintptr_t>(scores) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(source) & 3) == 0 && (reinterpret_cast<uintptr_t>(count) & 3) == 0);
    return det_select(top_keys, top_index, row_stride, n_sorted, det_decode_args(rois, deltas, deltas_dtype, stds, img_h, img_w, scale, R, C), B, K,
                      boxes, scores, labels, source, count, stream);
}

int pswin_paste_masks(const void* logits, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                      const long long* labels, const float* boxes, const int32_t* count, int B, int K, int C, int H, int W, float thr,
                      unsigned char* out, void* stream) {
    PSWIN_CHECK_ARG(logits && labels && boxes && count && out && valid_dtype(dtype));
    PSWIN_CHECK_ARG(B >= 1 && B <= 65535 && K >= 1 && K <= DET_KMAX && C >= 1 && C <= DET_CMAX && H >= 1 && W >= 1 && H <= 65536 && W <= 65536);
    PSWIN_CHECK_ARG(stride_n >= 1 && stride_c >= 1 && stride_y >= 1 && stride_x >= 1);
    PSWIN_CHECK_ARG(aligned16(out) && aligned16(boxes) && (reinterpret_cast<uintptr_t>(labels) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(logits) & (dtype == PSWIN_F32 ? 3 : 1)) == 0);
    const dim3 grid((H + PASTE_ROWS - 1) / PASTE_ROWS, K, B);
    PSWIN_CHECK_ARG(grid.x <= 65535u);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(paste_kernel<PSWIN_F32>, grid, dim3(PASTE_THREADS), 0, (hipStream_t)stream, logits, stride_n, stride_c, stride_y, stride_x,
                           labels, boxes, count, K, C, H, W, thr, out);
    else
        hipLaunchKernelGGL(paste_kernel<PSWIN_BF16>, grid, dim3(PASTE_THREADS), 0, (hipStream_t)stream, logits, stride_n, stride_c, stride_y, stride_x,
                           labels, boxes, count, K, C, H, W, thr, out);
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
