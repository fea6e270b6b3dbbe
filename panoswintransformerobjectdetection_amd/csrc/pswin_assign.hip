// MaxIoUAssigner.assign for a whole padded batch (mmdet/core/bbox/assigners/max_iou_assigner.py:85-212; the RPN's and the RoI head's
// target assignment of the detector step) -- gfx950 only.
//
// The per-image box count is read from device memory, so a captured step takes the next batch's annotations by copying them into the
// same buffers.  Two launches, no atomics and nothing that has to be cleared between launches:
//   (1) every workgroup covers ASSIGN_ROWS candidates of one image and writes, for each of the image's gt boxes, the largest IoU among
//       its candidates into its own row of the workspace (plain stores; rows of gt slots past the image's count are never written and
//       never read);
//   (2) every workgroup folds the image's partial rows in index order, then recomputes the IoUs of its candidates with the same device
//       function -- so "this candidate reaches the gt's maximum" is an exact == -- and writes gt_inds / max_iou.
// A maximum of finite floats does not depend on the order it is taken in, so the result is bit-identical from run to run.
// IoU is detector.box_iou's, operation by operation (the library is built with -ffp-contract=off and IEEE division).
#include "pswin_common.hpp"

namespace {
using namespace pswin;

constexpr int ASSIGN_THREADS = 256, ASSIGN_PER_THREAD = 4, ASSIGN_ROWS = ASSIGN_THREADS * ASSIGN_PER_THREAD;
constexpr int ASSIGN_GMAX = 256;                        // one thread of a workgroup per gt slot

__device__ inline float box_area(f32x4 b) { return fmaxf(b[2] - b[0], 0.f) * fmaxf(b[3] - b[1], 0.f); }

// detector.box_iou(gt, cand): clamped widths, union (area_gt + area_cand) - inter floored at 1e-6
__device__ inline float assign_iou(f32x4 g, float ga, f32x4 c, float ca) {
    const float iw = fmaxf(fminf(g[2], c[2]) - fmaxf(g[0], c[0]), 0.f), ih = fmaxf(fminf(g[3], c[3]) - fmaxf(g[1], c[1]), 0.f);
    const float inter = iw * ih;
    return inter / fmaxf((ga + ca) - inter, 1e-6f);
}

__device__ inline int assign_count(const int* __restrict__ gt_count, int b, int Gmax) {
    const int g = gt_count[b];
    return g < 0 ? 0 : (g > Gmax ? Gmax : g);
}

// a candidate in front of lead_gt is the image's own gt row of that index: past the count it is padding
__device__ inline bool assign_is_padding(int i, int lead_gt, int G) { return i < lead_gt && i >= G; }

struct AssignCands {
    f32x4 box[ASSIGN_PER_THREAD];
    float area[ASSIGN_PER_THREAD];
    int idx[ASSIGN_PER_THREAD];
};

// candidate k of thread t: row blockIdx.x * ASSIGN_ROWS + k * ASSIGN_THREADS + t (a wave reads 1 KiB of consecutive boxes)
__device__ inline void assign_load(AssignCands& c, const float* __restrict__ cand, long long cand_stride, int b, int N) {
    const f32x4* src = reinterpret_cast<const f32x4*>(cand) + (size_t)b * (size_t)cand_stride;
#pragma unroll
    for (int k = 0; k < ASSIGN_PER_THREAD; ++k) {
        const int i = blockIdx.x * ASSIGN_ROWS + k * ASSIGN_THREADS + threadIdx.x;
        c.idx[k] = i;
        c.box[k] = i < N ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        c.area[k] = box_area(c.box[k]);
    }
}

__global__ __launch_bounds__(ASSIGN_THREADS) void assign_gt_max_kernel(const float* __restrict__ cand, long long cand_stride,
                                                                      const float* __restrict__ gt, const int* __restrict__ gt_count, int N,
                                                                      int Gmax, int lead_gt, float* __restrict__ partial) {
    __shared__ f32x4 gb[ASSIGN_GMAX];
    __shared__ float ga[ASSIGN_GMAX];
    __shared__ float wm[ASSIGN_THREADS / 64][ASSIGN_GMAX];
    const int b = blockIdx.y, t = threadIdx.x;
    const int G = assign_count(gt_count, b, Gmax);
    if (G == 0) return;                                 // the whole workgroup: nothing of this image's rows is read in launch 2
    if (t < G) {
        const f32x4 g = reinterpret_cast<const f32x4*>(gt)[(size_t)b * Gmax + t];
        gb[t] = g;
        ga[t] = box_area(g);
    }
    AssignCands c;
    assign_load(c, cand, cand_stride, b, N);
    bool on[ASSIGN_PER_THREAD];
#pragma unroll
    for (int k = 0; k < ASSIGN_PER_THREAD; ++k) on[k] = c.idx[k] < N && !assign_is_padding(c.idx[k], lead_gt, G);
    __syncthreads();
    for (int g = 0; g < G; ++g) {
        const f32x4 gbox = gb[g];                       // the same address in every lane: an LDS broadcast
        const float garea = ga[g];
        float m = -1.f;                                 // below every IoU
#pragma unroll
        for (int k = 0; k < ASSIGN_PER_THREAD; ++k) {
            const float v = assign_iou(gbox, garea, c.box[k], c.area[k]);
            m = on[k] ? fmaxf(m, v) : m;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
        if ((t & 63) == 0) wm[t >> 6][g] = m;
    }
    __syncthreads();
    if (t < G) {
        float m = wm[0][t];
#pragma unroll
        for (int w = 1; w < ASSIGN_THREADS / 64; ++w) m = fmaxf(m, wm[w][t]);
        partial[((size_t)b * gridDim.x + blockIdx.x) * Gmax + t] = m;
    }
}

__global__ __launch_bounds__(ASSIGN_THREADS) void assign_write_kernel(const float* __restrict__ cand, long long cand_stride,
                                                                     const float* __restrict__ gt, const int* __restrict__ gt_count, int N,
                                                                     int Gmax, int lead_gt, float pos_thr, float neg_thr, float min_pos,
                                                                     int match_low_quality, const float* __restrict__ partial,
                                                                     long long* __restrict__ gt_inds, float* __restrict__ max_iou) {
    __shared__ f32x4 gb[ASSIGN_GMAX];
    __shared__ float ga[ASSIGN_GMAX];
    __shared__ float gm[ASSIGN_GMAX];                   // the gt's largest IoU over the image's valid candidates
    __shared__ int low[ASSIGN_GMAX];                    // the gt takes part in the low-quality match
    const int b = blockIdx.y, t = threadIdx.x;
    const int G = assign_count(gt_count, b, Gmax);
    if (t < G) {
        const f32x4 g = reinterpret_cast<const f32x4*>(gt)[(size_t)b * Gmax + t];
        gb[t] = g;
        ga[t] = box_area(g);
        const float* p = partial + (size_t)b * gridDim.x * Gmax + t;
        float m = -1.f;
        for (unsigned r = 0; r < gridDim.x; ++r) m = fmaxf(m, p[(size_t)r * Gmax]);
        gm[t] = m;
        low[t] = match_low_quality && m >= min_pos;
    }
    AssignCands c;
    assign_load(c, cand, cand_stride, b, N);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ASSIGN_PER_THREAD; ++k) {
        const int i = c.idx[k];
        if (i >= N) continue;
        long long ind;
        float best;
        if (assign_is_padding(i, lead_gt, G)) {
            ind = -1;
            best = -1.f;
        } else if (G == 0) {                            // max_iou_assigner.py:147-153
            ind = 0;
            best = 0.f;
        } else {
            best = -1.f;
            int arg = 0, last = 0;
            for (int g = 0; g < G; ++g) {
                const float v = assign_iou(gb[g], ga[g], c.box[k], c.area[k]);
                if (v > best) {                         // the lowest g among equals
                    best = v;
                    arg = g;
                }
                if (low[g] && v == gm[g]) last = g + 1;     // the reference's sequential loop: a later gt overwrites an earlier one
            }
            ind = -1;
            if (best >= 0.f && best < neg_thr) ind = 0;
            if (best >= pos_thr) ind = arg + 1;
            if (last > 0) ind = last;
        }
        const size_t o = (size_t)b * N + i;
        gt_inds[o] = ind;
        if (max_iou) max_iou[o] = best;
    }
}

bool assign_shape_ok(int B, int N, int Gmax) {
    if (B < 1 || B > 65535 || N < 1 || Gmax < 1 || Gmax > ASSIGN_GMAX) return false;
    const long long blocks = ((long long)N + ASSIGN_ROWS - 1) / ASSIGN_ROWS;
    return (long long)B * N <= 0x7fffffffLL && (long long)B * blocks * Gmax * 4 <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int pswin_max_iou_assign_rows_per_workgroup(void) { return ASSIGN_ROWS; }

int pswin_max_iou_assign_workspace(int B, int N, int Gmax) {
    if (!assign_shape_ok(B, N, Gmax)) return PSWIN_ERR_ARG;
    return (int)((long long)B * ((N + ASSIGN_ROWS - 1) / ASSIGN_ROWS) * Gmax * 4);
}

int pswin_max_iou_assign(const float* cand, int cand_per_image, const float* gt, const int32_t* gt_count, int B, int N, int Gmax, int lead_gt,
                         float pos_iou_thr, float neg_iou_thr, float min_pos_iou, int match_low_quality, long long* gt_inds, float* max_iou,
                         void* workspace, void* stream) {
    PSWIN_CHECK_ARG(cand && gt && gt_count && gt_inds && workspace && assign_shape_ok(B, N, Gmax));
    PSWIN_CHECK_ARG(lead_gt >= 0 && lead_gt <= N && (cand_per_image == 0 || cand_per_image == 1));
    PSWIN_CHECK_ARG(aligned16(cand) && aligned16(gt) && aligned16(workspace));
    PSWIN_CHECK_ARG((reinterpret_cast<uintptr_t>(gt_inds) & 7) == 0 && (reinterpret_cast<uintptr_t>(max_iou) & 3) == 0);
    const dim3 grid((N + ASSIGN_ROWS - 1) / ASSIGN_ROWS, B);
    const long long stride = cand_per_image ? N : 0;
    float* partial = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(assign_gt_max_kernel, grid, dim3(ASSIGN_THREADS), 0, (hipStream_t)stream, cand, stride, gt, gt_count, N, Gmax, lead_gt,
                       partial);
    hipLaunchKernelGGL(assign_write_kernel, grid, dim3(ASSIGN_THREADS), 0, (hipStream_t)stream, cand, stride, gt, gt_count, N, Gmax, lead_gt,
                       pos_iou_thr, neg_iou_thr, min_pos_iou, match_low_quality, partial, gt_inds, max_iou);
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
