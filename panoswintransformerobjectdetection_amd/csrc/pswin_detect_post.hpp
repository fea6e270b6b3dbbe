// What the two class-wise NMS chains and the two mask pastes have in common (csrc/pswin_detect.hip: logits and deltas of ONE view;
// csrc/pswin_augtest.hip: boxes and probabilities merged over test views) -- gfx950 only.
//
// The chain's kernels take the box of (image b, proposal r, class c) from a BoxOf: `f32x4 operator()(int b, int r, int c) const` and the
// members R and C.  The paste's kernels stage their 28 x 28 probability tile in LDS themselves and share the sampling and the stores.
#pragma once
#include "pswin_common.hpp"

namespace pswin {

constexpr int DET_RMAX = 1024, DET_CMAX = 128, DET_KMAX = 1024, DET_THREADS = 256;
constexpr int DET_NMS_SLICE = 256;                      // (image, class) groups per pswin_nms_groups call: 64 MiB of masks at 1024 rows
constexpr int PASTE_M = 28, PASTE_LD = PASTE_M + 2, PASTE_THREADS = 256, PASTE_ROWS = 32;

__device__ inline float det_load(const void* p, int dt, size_t i) {
    return dt == PSWIN_F32 ? reinterpret_cast<const float*>(p)[i] : bf16_bits_to_f32(reinterpret_cast<const unsigned short*>(p)[i]);
}

__host__ __device__ inline int det_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// (2a) one thread per (image, class, sorted position): the candidate's box into the NMS input, and the list's candidate count (written by
// the one thread that sees the last candidate, or by thread 0 of a list without any)
template <class BoxOf>
__global__ __launch_bounds__(DET_THREADS) void det_gather_kernel(const float* __restrict__ skeys, const long long* __restrict__ sidx, BoxOf p,
                                                                 int Rp, float* __restrict__ sboxes, int* __restrict__ counts) {
    const int b = blockIdx.z, c = blockIdx.y, j = blockIdx.x * DET_THREADS + threadIdx.x;
    if (j >= p.R) return;
    const size_t g = (size_t)b * p.C + c;
    const bool valid = skeys[g * p.R + j] > 0.f;
    if (valid) {
        const int r = det_clamp((int)sidx[g * p.R + j], p.R - 1);
        reinterpret_cast<f32x4*>(sboxes)[g * Rp + j] = p(b, r, c);
        if (j + 1 >= p.R || !(skeys[g * p.R + j + 1] > 0.f)) counts[g] = j + 1;
    } else if (j == 0) {
        counts[g] = 0;
    }
}

// (2b) final[b][r * C + c] = the score of a candidate the NMS kept, else -1
__global__ static __launch_bounds__(DET_THREADS) void det_scatter_kernel(const float* __restrict__ skeys, const long long* __restrict__ sidx,
                                                                         const unsigned char* __restrict__ keep, int R, int Rp, int C,
                                                                         float* __restrict__ final_keys) {
    const int b = blockIdx.z, c = blockIdx.y, j = blockIdx.x * DET_THREADS + threadIdx.x;
    if (j >= R) return;
    const size_t g = (size_t)b * C + c;
    const float key = skeys[g * R + j];
    const int r = det_clamp((int)sidx[g * R + j], R - 1);
    const bool kept = key > 0.f && keep[g * Rp + j] != 0;
    final_keys[((size_t)b * R + r) * C + c] = kept ? key : -1.f;
}

// (3) one thread per (image, output row)
template <class BoxOf>
__global__ __launch_bounds__(DET_THREADS) void det_select_kernel(const float* __restrict__ tvals, const long long* __restrict__ tidx, long long ld,
                                                                 int n_sorted, BoxOf p, int K, float* __restrict__ boxes,
                                                                 float* __restrict__ scores, long long* __restrict__ labels,
                                                                 int* __restrict__ source, int* __restrict__ count) {
    const int b = blockIdx.y, k = blockIdx.x * DET_THREADS + threadIdx.x;
    if (k >= K) return;
    const size_t row = (size_t)b * (size_t)ld;
    const float v = k < n_sorted ? tvals[row + k] : -1.f;
    const size_t o = (size_t)b * K + k;
    f32x4 box = {0.f, 0.f, 0.f, 0.f};
    float sc = 0.f;
    long long lab = 0;
    int src = 0;
    if (v > 0.f) {
        long long flat = tidx[row + k];
        const long long last = (long long)p.R * p.C - 1;
        flat = flat < 0 ? 0 : (flat > last ? last : flat);
        const int r = (int)(flat / p.C), c = (int)(flat % p.C);
        box = p(b, r, c);
        sc = v;
        lab = c;
        src = (int)flat;
        const bool more = k + 1 < K && k + 1 < n_sorted && tvals[row + k + 1] > 0.f;
        if (!more) count[b] = k + 1;
    } else if (k == 0) {
        count[b] = 0;
    }
    reinterpret_cast<f32x4*>(boxes)[o] = box;
    scores[o] = sc;
    labels[o] = lab;
    source[o] = src;
}

inline bool det_shape_ok(int B, int R, int C) { return B >= 1 && B <= 65535 && R >= 1 && R <= DET_RMAX && C >= 1 && C <= DET_CMAX; }

struct DetWorkspace {
    size_t boxes, counts, keep, masks, total;
    int Rp, slice;
};

inline DetWorkspace det_workspace(int B, int R, int C) {
    DetWorkspace w;
    const size_t G = (size_t)B * C;
    w.Rp = ceil_to(R, 64);
    w.slice = G < (size_t)DET_NMS_SLICE ? (int)G : DET_NMS_SLICE;
    w.boxes = 0;
    w.counts = w.boxes + G * w.Rp * 16;
    w.keep = w.counts + (G * 4 + 15) / 16 * 16;
    w.masks = w.keep + (G * w.Rp + 15) / 16 * 16;
    w.total = w.masks + (size_t)w.slice * w.Rp * 32 * 8;   // pswin_nms_workspace(slice, Rp)
    return w;
}

// stage (2) of a chain on checked arguments: gather, the greedy rule on every (image, class) list, scatter
template <class BoxOf>
inline int det_nms_lists(const float* sorted_keys, const long long* sorted_index, const BoxOf& p, int B, float iou_thr, float* final_keys,
                         void* workspace, void* stream) {
    const int R = p.R, C = p.C;
    const DetWorkspace w = det_workspace(B, R, C);
    PSWIN_CHECK_ARG(w.total <= 0x7fffffffull);
    char* ws = reinterpret_cast<char*>(workspace);
    float* sboxes = reinterpret_cast<float*>(ws + w.boxes);
    int* counts = reinterpret_cast<int*>(ws + w.counts);
    unsigned char* keep = reinterpret_cast<unsigned char*>(ws + w.keep);
    const dim3 grid((R + DET_THREADS - 1) / DET_THREADS, C, B);
    hipLaunchKernelGGL(det_gather_kernel<BoxOf>, grid, dim3(DET_THREADS), 0, (hipStream_t)stream, sorted_keys, sorted_index, p, w.Rp, sboxes, counts);
    const int G = B * C;
    for (int g0 = 0; g0 < G; g0 += w.slice) {           // the slices run one after the other on the stream and share the mask words
        const int n = G - g0 < w.slice ? G - g0 : w.slice;
        const int rc = pswin_nms_groups(sboxes + (size_t)g0 * w.Rp * 4, counts + g0, n, w.Rp, iou_thr, keep + (size_t)g0 * w.Rp, ws + w.masks, stream);
        if (rc != PSWIN_OK) return rc;
    }
    hipLaunchKernelGGL(det_scatter_kernel, grid, dim3(DET_THREADS), 0, (hipStream_t)stream, sorted_keys, sorted_index, keep, R, w.Rp, C, final_keys);
    PSWIN_LAUNCH_RET();
}

// stage (3) of a chain on checked arguments
template <class BoxOf>
inline int det_select(const float* top_keys, const long long* top_index, long long row_stride, int n_sorted, const BoxOf& p, int B, int K,
                      float* boxes, float* scores, long long* labels, int32_t* source, int32_t* count, void* stream) {
    hipLaunchKernelGGL(det_select_kernel<BoxOf>, dim3((K + DET_THREADS - 1) / DET_THREADS, B), dim3(DET_THREADS), 0, (hipStream_t)stream, top_keys,
                       top_index, row_stride, n_sorted, p, K, boxes, scores, labels, source, count);
    PSWIN_LAUNCH_RET();
}

// ---- mask paste ----------------------------------------------------------------------------------------------------------------------------
// grid_sample's source coordinate of an image pixel centre `pc` (x + 0.5 or y + 0.5) for a box side [lo, hi]: the normalised coordinate
// (pc - lo) / (hi - lo) * 2 - 1 with an infinite value set to 0 (_do_paste_mask), then ((g + 1) * 28 - 1) / 2 (align_corners=False).
// A NaN (0 / 0: the centre lies on a box side of zero length) comes back as NaN: the pixel samples nothing.
__device__ inline float paste_coord(float pc, float lo, float hi) {
    float g = (pc - lo) / (hi - lo) * 2.f - 1.f;
    if (__builtin_isinf(g)) g = 0.f;
    return ((g + 1.f) * (float)PASTE_M - 1.f) / 2.f;
}

// One axis of the bilinear sample at source coordinate i (paste_coord): whether it lies in (-1, 28) -- outside, and for a NaN, the pixel
// samples nothing -- and, inside, the lower cell f = floor(i) in [-1, 27] with the weights of cells f and f + 1
struct PasteAxis {
    bool in;
    int f;
    float w0, w1;
};
__device__ inline PasteAxis paste_axis(float i) {
    PasteAxis a = {i > -1.f && i < (float)PASTE_M, 0, 0.f, 0.f};
    if (a.in) {
        const float ff = floorf(i);
        a.f = (int)ff;
        a.w1 = i - ff;
        a.w0 = (ff + 1.f) - i;
    }
    return a;
}
// The sampled probability of a pixel whose two axes are inside: `prob` is the staged tile (paste_stage).  THE per-pixel value of every
// paste: the bitmap kernels (paste_rows) and the run-length kernel (csrc/pswin_rle.hip) compare it with thr.
__device__ inline float paste_value(const float* prob, const PasteAxis& ax, const PasteAxis& ay) {
    const float* q = prob + (ay.f + 1) * PASTE_LD + 1 + ax.f;
    return q[0] * (ax.w0 * ay.w0) + q[1] * (ax.w1 * ay.w0) + q[PASTE_LD] * (ax.w0 * ay.w1) + q[PASTE_LD + 1] * (ax.w1 * ay.w1);
}

// The staging of one source: prob (PASTE_LD x PASTE_LD f32 in LDS) = sigmoid(logits[det][c]) inside a zero border, by all PASTE_THREADS
// threads of the workgroup, NOT synchronised
template <int DT>
__device__ inline void paste_stage(float* prob, const void* __restrict__ logits, long long sn, long long sc, long long sy, long long sx,
                                   size_t det, long long c) {
    for (int i = threadIdx.x; i < PASTE_LD * PASTE_LD; i += PASTE_THREADS) {
        const int yy = i / PASTE_LD - 1, xx = i % PASTE_LD - 1;
        float v = 0.f;
        if (yy >= 0 && yy < PASTE_M && xx >= 0 && xx < PASTE_M) {
            const float l = det_load(logits, DT, (size_t)((long long)det * sn + c * sc + yy * sy + xx * sx));
            v = 1.f / (1.f + expf(-l));
        }
        prob[i] = v;
    }
}
__device__ inline long long paste_channel(long long lab, int C) { return lab < 0 ? 0 : (lab > C - 1 ? C - 1 : lab); }

// The rows ybase .. ybase + PASTE_ROWS - 1 of detection `det`: prob is the workgroup's staged tile (PASTE_LD x PASTE_LD f32, zero border),
// written by all threads and NOT yet synchronised; a detection that is not live writes zeros
__device__ inline void paste_rows(const float* prob, bool live, f32x4 box, size_t det, int ybase, int H, int W, float thr,
                                  unsigned char* __restrict__ out) {
    const int t = threadIdx.x;
    __syncthreads();
    const unsigned zero_bit = 0.f >= thr ? 1u : 0u;     // what a pixel that samples nothing compares to
    const bool whole = (W & 15) == 0;                   // every row starts on a 16-byte boundary: vector stores only
    const int SL = whole ? W >> 4 : (W >> 4) + 2;       // work items per row: the 16-pixel groups, then the row's unaligned head and tail
    const int rows = H - ybase < PASTE_ROWS ? H - ybase : PASTE_ROWS;
    for (int it = t; it < rows * SL; it += PASTE_THREADS) {
        const int y = ybase + it / SL, s = it % SL;
        const size_t rowoff = (det * H + y) * (size_t)W;
        int head = whole ? 0 : (int)((16 - (rowoff & 15)) & 15);
        head = head > W ? W : head;
        const int nvec = (W - head) >> 4;
        int xs, n;
        if (s < nvec) {
            xs = head + 16 * s;
            n = 16;
        } else if (s == nvec) {
            xs = 0;
            n = head;
        } else if (s == nvec + 1) {
            xs = head + 16 * nvec;
            n = W - xs;
        } else {
            continue;
        }
        unsigned bits = 0u;                             // bit p: pixel xs + p
        if (live) {
            const PasteAxis ay = paste_axis(paste_coord((float)y + 0.5f, box[1], box[3]));
            if (ay.in) {
#pragma unroll
                for (int p = 0; p < 16; ++p) {
                    const PasteAxis ax = paste_axis(paste_coord((float)(xs + p) + 0.5f, box[0], box[2]));
                    const float val = ax.in ? paste_value(prob, ax, ay) : 0.f;
                    bits |= (val >= thr ? 1u : 0u) << p;
                }
            } else {
                bits = zero_bit ? 0xffffu : 0u;
            }
        }
        unsigned char* dst = out + rowoff + xs;
        if (n == 16) {
            u32x4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned nib = (bits >> (4 * q)) & 15u;
                v[q] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
            }
            *reinterpret_cast<u32x4*>(dst) = v;         // xs + 16 <= W and (rowoff + xs) % 16 == 0
        } else {
            for (int p = 0; p < n; ++p) dst[p] = (unsigned char)((bits >> p) & 1u);
        }
    }
}

}  // namespace pswin
