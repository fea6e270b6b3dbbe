// RandomSampler, box targets and mask targets of a padded detector batch (detector.sample_ranks / rpn_targets / roi_targets /
// mask_targets: what MiniMaskRCNN.heads_loss does between "assigned" and "loss") -- gfx950 only.
//
// Everything is read from device memory, nothing is read back and no buffer has to be cleared between calls, so a captured step takes the
// next batch's annotations, assignment and keys by replaying on the same buffers.
//
// SELECTION (pswin_sample_ranks): the first k of N candidates of two lists (positives, negatives) per image by the 64-bit composite
// (bits of the float32 composed key) << 32 | index.  The composed key is >= 0, so its bit pattern orders as the float does; the composite
// is unique per candidate, so "the k smallest, ascending" is ONE answer whatever order the work is done in: ties of the composed key come
// out in ascending index, as a stable sort leaves them.  A reduction tree of one kernel: a workgroup loads a chunk of SAMPLE_ROWS
// composites into LDS, sorts them bitonically and writes the chunk's first min(k, SAMPLE_ROWS) to the workspace (plain stores, every
// entry the next level reads is written by this call); the next level runs the same kernel on those until one chunk is left, whose
// first n_pos / n_neg indices are the result.  k <= SAMPLE_ROWS / 2, so every level shrinks its input at least by half.
//
// EPILOGUES (pswin_rpn_targets, pswin_roi_targets): one workgroup per image gathers what the ranks select and encodes the box deltas as
// detector.encode_deltas does, operation by operation (the library is built with -ffp-contract=off and IEEE division; only logf may
// differ from the host).  The number of valid positives is an integer count: no order to depend on.
//
// MASK TARGETS (pswin_mask_targets): one workgroup per (image, RoI); a thread per sample point reads the up to four uint8 taps of the
// ONE assigned bitmap and writes 0.f or 1.f.
#include "pswin_common.hpp"

namespace {
using namespace pswin;

typedef unsigned long long u64;

constexpr int SAMPLE_THREADS = 256, SAMPLE_ROWS = 2048;         // 2048 composites of 8 bytes: 16 KB of LDS
constexpr int SAMPLE_KMAX = SAMPLE_ROWS / 2;
constexpr u64 SAMPLE_PAD = ~0ull;                               // behind every candidate: its index half is no index
constexpr int TARGET_THREADS = 256;
constexpr int TARGET_GMAX = 256;
constexpr int MASK_THREADS = 256, MASK_SIZE_MAX = 64;

__host__ __device__ inline int sample_kept(int k) { return k < SAMPLE_ROWS ? k : SAMPLE_ROWS; }
__host__ __device__ inline long long sample_chunks(long long m) { return (m + SAMPLE_ROWS - 1) / SAMPLE_ROWS; }

// The composite of candidate i in list `list` (0: positives are the members, 1: negatives): detector.sample_ranks' composed key
__device__ inline u64 sample_composite(long long ind, float key, int list, unsigned i) {
    const bool member = list == 0 ? ind > 0 : ind == 0;
    const float behind = ind < 0 ? key + 4.f : key + 2.f;
    const float c = member ? key : behind;
    return ((u64)__builtin_bit_cast(unsigned, c) << 32) | (u64)i;
}

// grid (chunks, 2 lists, B).  First level (in == nullptr): chunk c covers candidates [c * SAMPLE_ROWS, ...) of gt_inds / key [B][N].
// Later levels: `in` holds M composites per (image, list).  Last level (one chunk; rank_pos != nullptr): the first n_pos / n_neg indices
// go to rank_pos / rank_neg as int64, clamped to [0, N); otherwise the chunk's first `kept` composites go to out[(b, list)][chunk].
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_level_kernel(const long long* __restrict__ gt_inds, const float* __restrict__ key,
                                                                     const u64* __restrict__ in, int M, int N, int kept, u64* __restrict__ out,
                                                                     long long* __restrict__ rank_pos, long long* __restrict__ rank_neg,
                                                                     int n_pos, int n_neg) {
    __shared__ u64 s[SAMPLE_ROWS];
    const int chunk = blockIdx.x, list = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const size_t bl = (size_t)b * 2 + list;
    for (int r = t; r < SAMPLE_ROWS; r += SAMPLE_THREADS) {
        const long long i = (long long)chunk * SAMPLE_ROWS + r;
        u64 v = SAMPLE_PAD;
        if (i < M) v = in ? in[bl * (size_t)M + i] : sample_composite(gt_inds[(size_t)b * N + i], key[(size_t)b * N + i], list, (unsigned)i);
        s[r] = v;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= SAMPLE_ROWS; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int p = t; p < SAMPLE_ROWS / 2; p += SAMPLE_THREADS) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
                const u64 a = s[lo], c = s[hi];
                if ((a > c) == ((lo & k2) == 0)) {
                    s[lo] = c;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    if (rank_pos) {
        long long* dst = list == 0 ? rank_pos + (size_t)b * n_pos : rank_neg + (size_t)b * n_neg;
        const int n = list == 0 ? n_pos : n_neg;
        for (int r = t; r < n; r += SAMPLE_THREADS) {
            const unsigned i = (unsigned)(s[r] & 0xffffffffull);
            dst[r] = i < (unsigned)N ? (long long)i : (long long)(N - 1);      // a pad only with keys outside the contract: stay in range
        }
    } else {
        u64* dst = out + (bl * gridDim.x + chunk) * (size_t)kept;
        for (int r = t; r < kept; r += SAMPLE_THREADS) dst[r] = s[r];
    }
}

bool sample_shape_ok(int B, int N, int k) {
    if (B < 1 || B > 65535 || N < 1 || k < 1 || k > N || k > SAMPLE_KMAX) return false;
    return (long long)B * N <= 0x7fffffffLL;
}

// composites the first and the second level write, per (image, list)
void sample_level_sizes(int N, int k, long long& first, long long& second) {
    const int kept = sample_kept(k);
    const long long c0 = sample_chunks(N);
    first = c0 > 1 ? c0 * kept : 0;
    const long long c1 = sample_chunks(first);
    second = c1 > 1 ? c1 * kept : 0;
}

// detector.encode_deltas (means 0), operation by operation
__device__ inline f32x4 encode_box(f32x4 src, f32x4 dst, f32x4 stds) {
    const float sw = fmaxf(src[2] - src[0], 1e-3f), sh = fmaxf(src[3] - src[1], 1e-3f);
    const float dw = fmaxf(dst[2] - dst[0], 1e-3f), dh = fmaxf(dst[3] - dst[1], 1e-3f);
    const float sx = (src[0] + src[2]) * 0.5f, sy = (src[1] + src[3]) * 0.5f;
    const float dx = (dst[0] + dst[2]) * 0.5f, dy = (dst[1] + dst[3]) * 0.5f;
    return f32x4{((dx - sx) / sw) / stds[0], ((dy - sy) / sh) / stds[1], logf(dw / sw) / stds[2], logf(dh / sh) / stds[3]};
}

__device__ inline int clamp_index(long long v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : (int)v); }

// the number of set flags of the workgroup (an integer: the order of the additions does not matter); every thread gets it
__device__ inline int block_count(int mine, int* red) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mine += __shfl_xor(mine, s, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int w = 0; w < TARGET_THREADS / 64; ++w) n += red[w];
    return n;
}

// valid positives of image b among pos_rank[b][0 .. n_pos_max)
__device__ inline int count_valid_positives(const long long* __restrict__ gt_inds, const long long* __restrict__ pos_rank, int b, int N,
                                            int n_pos_max, int* red) {
    int mine = 0;
    for (int r = threadIdx.x; r < n_pos_max; r += TARGET_THREADS)
        mine += gt_inds[(size_t)b * N + clamp_index(pos_rank[(size_t)b * n_pos_max + r], N)] > 0 ? 1 : 0;
    return block_count(mine, red);
}

__global__ __launch_bounds__(TARGET_THREADS) void rpn_targets_kernel(const long long* __restrict__ gt_inds, const long long* __restrict__ pos_rank,
                                                                    const long long* __restrict__ neg_rank, const float* __restrict__ anchors,
                                                                    const float* __restrict__ gt, int N, int Gmax, int n_pos_max, int n_tot,
                                                                    long long* __restrict__ idx, float* __restrict__ valid,
                                                                    unsigned char* __restrict__ pos_valid, float* __restrict__ reg_t) {
    __shared__ int red[TARGET_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n_pos = count_valid_positives(gt_inds, pos_rank, b, N, n_pos_max, red);
    const long long* ind = gt_inds + (size_t)b * N;
    const size_t row = (size_t)b * (n_pos_max + n_tot);
    const f32x4 one = {1.f, 1.f, 1.f, 1.f};
    for (int r = t; r < n_pos_max + n_tot; r += TARGET_THREADS) {
        if (r < n_pos_max) {
            const int i = clamp_index(pos_rank[(size_t)b * n_pos_max + r], N);
            const long long g = ind[i];
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (g > 0)
                d = encode_box(reinterpret_cast<const f32x4*>(anchors)[i],
                               reinterpret_cast<const f32x4*>(gt)[(size_t)b * Gmax + clamp_index(g - 1, Gmax)], one);
            idx[row + r] = i;
            valid[row + r] = g > 0 ? 1.f : 0.f;
            pos_valid[(size_t)b * n_pos_max + r] = g > 0 ? 1 : 0;
            reinterpret_cast<f32x4*>(reg_t)[(size_t)b * n_pos_max + r] = d;
        } else {
            const int j = r - n_pos_max;
            const int i = clamp_index(neg_rank[(size_t)b * n_tot + j], N);
            idx[row + r] = i;
            valid[row + r] = (ind[i] == 0 && j < n_tot - n_pos) ? 1.f : 0.f;
        }
    }
}

__global__ __launch_bounds__(TARGET_THREADS) void roi_targets_kernel(const long long* __restrict__ gt_inds, const long long* __restrict__ pos_rank,
                                                                    const long long* __restrict__ neg_order, const float* __restrict__ cand,
                                                                    const float* __restrict__ gt, const long long* __restrict__ gt_labels, int N,
                                                                    int Gmax, int n_pos_max, int n_tot, long long background, f32x4 stds,
                                                                    float* __restrict__ rois, long long* __restrict__ labels,
                                                                    float* __restrict__ reg_t, unsigned char* __restrict__ pos_valid,
                                                                    long long* __restrict__ gt_idx) {
    __shared__ int red[TARGET_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const int filler = n_pos_max - count_valid_positives(gt_inds, pos_rank, b, N, n_pos_max, red);
    const long long* ind = gt_inds + (size_t)b * N;
    const f32x4* boxes = reinterpret_cast<const f32x4*>(cand) + (size_t)b * N;
    for (int r = t; r < n_tot; r += TARGET_THREADS) {
        const size_t o = (size_t)b * n_tot + r;
        if (r < n_pos_max) {
            const size_t p = (size_t)b * n_pos_max + r;
            const int i = clamp_index(pos_rank[p], N);
            const long long g = ind[i];
            const int a = clamp_index(g - 1, Gmax);                 // (gt_inds - 1).clamp(min=0); never past the padded rows
            const f32x4 box = boxes[i];
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (g > 0) d = encode_box(box, reinterpret_cast<const f32x4*>(gt)[(size_t)b * Gmax + a], stds);
            reinterpret_cast<f32x4*>(rois)[o] = box;
            labels[o] = g > 0 ? gt_labels[(size_t)b * Gmax + a] : background;
            reinterpret_cast<f32x4*>(reg_t)[p] = d;
            pos_valid[p] = g > 0 ? 1 : 0;
            gt_idx[p] = a;
        } else {
            int take = r - n_pos_max + filler;                      // < n_tot: inside neg_order
            take = take > N - 1 ? N - 1 : take;
            reinterpret_cast<f32x4*>(rois)[o] = boxes[clamp_index(neg_order[(size_t)b * n_tot + take], N)];
            labels[o] = background;
        }
    }
}

// grid (P, B).  grid_sample(bilinear, zeros, align_corners=False) of ONE uint8 plane at the RoI's size x size points, >= 0.5.
__global__ __launch_bounds__(MASK_THREADS) void mask_targets_kernel(const unsigned char* __restrict__ masks, const float* __restrict__ rois,
                                                                   const long long* __restrict__ gt_idx, const unsigned char* __restrict__ pos_valid,
                                                                   int P, int Gmax, int H, int W, int size, float* __restrict__ out) {
    const int p = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const size_t roi = (size_t)b * P + p;
    float* dst = out + roi * (size_t)(size * size);
    if (!pos_valid[roi]) {                                          // the whole workgroup: nothing is read
        for (int q = t; q < size * size; q += MASK_THREADS) dst[q] = 0.f;
        return;
    }
    const f32x4 r = reinterpret_cast<const f32x4*>(rois)[roi];
    const unsigned char* plane = masks + ((size_t)b * Gmax + clamp_index(gt_idx[roi], Gmax)) * ((size_t)H * W);
    const float fW = (float)W, fH = (float)H;
    for (int q = t; q < size * size; q += MASK_THREADS) {
        const int i = q / size, j = q % size;
        const float tx = ((float)j + 0.5f) / (float)size, ty = ((float)i + 0.5f) / (float)size;
        const float gx = (r[0] + (r[2] - r[0]) * tx) / fW * 2.f - 1.f, gy = (r[1] + (r[3] - r[1]) * ty) / fH * 2.f - 1.f;
        const float x = ((gx + 1.f) * fW - 1.f) / 2.f, y = ((gy + 1.f) * fH - 1.f) / 2.f;      // align_corners=False
        const float xw = floorf(x), yn = floorf(y);
        const float w = x - xw, e = 1.f - w, n = y - yn, s = 1.f - n;
        // a tap outside the plane (or a coordinate that is no number) contributes 0; the tests are made on the floats, so that no
        // out-of-range value is ever converted to an index
        const bool x0 = xw > -1.f && xw < fW, x1 = xw + 1.f > -1.f && xw + 1.f < fW;
        const bool y0 = yn > -1.f && yn < fH, y1 = yn + 1.f > -1.f && yn + 1.f < fH;
        const int xi = (x0 || x1) ? (int)xw : 0, yi = (y0 || y1) ? (int)yn : 0;
        const unsigned char* q0 = plane + (long long)yi * W + xi;
        const float nw = (x0 && y0) ? (float)q0[0] : 0.f, ne = (x1 && y0) ? (float)q0[1] : 0.f;
        const float sw = (x0 && y1) ? (float)q0[W] : 0.f, se = (x1 && y1) ? (float)q0[W + 1] : 0.f;
        const float v = ((nw * (s * e) + ne * (s * w)) + sw * (n * e)) + se * (n * w);
        dst[q] = v >= 0.5f ? 1.f : 0.f;
    }
}

bool targets_shape_ok(int B, int N, int Gmax, int n_pos_max, int n_tot) {
    if (B < 1 || B > 65535 || N < 1 || Gmax < 1 || Gmax > TARGET_GMAX) return false;
    if (n_pos_max < 1 || n_tot < n_pos_max || n_tot > N || n_tot > SAMPLE_KMAX) return false;
    return (long long)B * N <= 0x7fffffffLL;
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" {

int pswin_sample_rows_per_workgroup(void) { return SAMPLE_ROWS; }

int pswin_sample_workspace(int B, int N, int k) {
    if (!sample_shape_ok(B, N, k)) return PSWIN_ERR_ARG;
    long long first, second;
    sample_level_sizes(N, k, first, second);
    const long long n = (long long)B * 2 * (first + second) * 8;        // two buffers that the levels write in turn
    return n > 0x7fffffffLL ? PSWIN_ERR_ARG : (n > 16 ? (int)n : 16);  // a single chunk needs none: never 0 bytes
}

int pswin_sample_ranks(const long long* gt_inds, const float* key, int B, int N, int n_pos, int n_neg, long long* pos_rank, long long* neg_rank,
                       void* workspace, void* stream) {
    PSWIN_CHECK_ARG(gt_inds && key && pos_rank && neg_rank && workspace && n_pos >= 1 && n_neg >= 1);
    const int k = n_pos > n_neg ? n_pos : n_neg;
    PSWIN_CHECK_ARG(sample_shape_ok(B, N, k) && pswin_sample_workspace(B, N, k) > 0);
    PSWIN_CHECK_ARG(aligned8(gt_inds) && aligned4(key) && aligned8(pos_rank) && aligned8(neg_rank) && aligned16(workspace));
    long long first, second;
    sample_level_sizes(N, k, first, second);
    const int kept = sample_kept(k);
    u64* buf[2] = {reinterpret_cast<u64*>(workspace), reinterpret_cast<u64*>(workspace) + (size_t)B * 2 * first};
    const u64* in = nullptr;
    long long M = N;
    for (int level = 0;; ++level) {
        const long long chunks = sample_chunks(M);
        const bool last = chunks == 1;
        hipLaunchKernelGGL(sample_level_kernel, dim3((unsigned)chunks, 2, B), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, gt_inds, key, in,
                           (int)M, N, kept, last ? nullptr : buf[level & 1], last ? pos_rank : nullptr, last ? neg_rank : nullptr, n_pos, n_neg);
        if (last) break;
        in = buf[level & 1];
        M = chunks * kept;
    }
    PSWIN_LAUNCH_RET();
}

int pswin_rpn_targets(const long long* gt_inds, const long long* pos_rank, const long long* neg_rank, const float* anchors, const float* gt, int B,
                      int N, int Gmax, int n_pos_max, int n_tot, long long* idx, float* valid, unsigned char* pos_valid, float* reg_t,
                      void* stream) {
    PSWIN_CHECK_ARG(gt_inds && pos_rank && neg_rank && anchors && gt && idx && valid && pos_valid && reg_t);
    PSWIN_CHECK_ARG(targets_shape_ok(B, N, Gmax, n_pos_max, n_tot));
    PSWIN_CHECK_ARG(aligned8(gt_inds) && aligned8(pos_rank) && aligned8(neg_rank) && aligned8(idx) && aligned4(valid));
    PSWIN_CHECK_ARG(aligned16(anchors) && aligned16(gt) && aligned16(reg_t));
    hipLaunchKernelGGL(rpn_targets_kernel, dim3(B), dim3(TARGET_THREADS), 0, (hipStream_t)stream, gt_inds, pos_rank, neg_rank, anchors, gt, N, Gmax,
                       n_pos_max, n_tot, idx, valid, pos_valid, reg_t);
    PSWIN_LAUNCH_RET();
}

int pswin_roi_targets(const long long* gt_inds, const long long* pos_rank, const long long* neg_order, const float* cand, const float* gt,
                      const long long* gt_labels, int B, int N, int Gmax, int n_pos_max, int n_tot, int num_classes, const float* stds,
                      float* rois, long long* labels, float* reg_t, unsigned char* pos_valid, long long* gt_idx, void* stream) {
    PSWIN_CHECK_ARG(gt_inds && pos_rank && neg_order && cand && gt && gt_labels && stds && rois && labels && reg_t && pos_valid && gt_idx);
    PSWIN_CHECK_ARG(targets_shape_ok(B, N, Gmax, n_pos_max, n_tot) && num_classes >= 1);
    PSWIN_CHECK_ARG(aligned8(gt_inds) && aligned8(pos_rank) && aligned8(neg_order) && aligned8(gt_labels) && aligned8(labels) && aligned8(gt_idx));
    PSWIN_CHECK_ARG(aligned16(cand) && aligned16(gt) && aligned16(rois) && aligned16(reg_t));
    PSWIN_CHECK_ARG(stds[0] > 0.f && stds[1] > 0.f && stds[2] > 0.f && stds[3] > 0.f);
    const f32x4 s = {stds[0], stds[1], stds[2], stds[3]};
    hipLaunchKernelGGL(roi_targets_kernel, dim3(B), dim3(TARGET_THREADS), 0, (hipStream_t)stream, gt_inds, pos_rank, neg_order, cand, gt, gt_labels, N,
                       Gmax, n_pos_max, n_tot, (long long)num_classes, s, rois, labels, reg_t, pos_valid, gt_idx);
    PSWIN_LAUNCH_RET();
}

int pswin_mask_targets(const unsigned char* masks, const float* rois, const long long* gt_idx, const unsigned char* pos_valid, int B, int P,
                       int Gmax, int H, int W, int size, float* out, void* stream) {
    PSWIN_CHECK_ARG(masks && rois && gt_idx && pos_valid && out);
    PSWIN_CHECK_ARG(B >= 1 && B <= 65535 && P >= 1 && Gmax >= 1 && Gmax <= TARGET_GMAX && H >= 1 && W >= 1 && size >= 1 && size <= MASK_SIZE_MAX);
    PSWIN_CHECK_ARG((long long)H * W <= 0x7fffffffLL && (long long)B * P <= 0x7fffffffLL);
    PSWIN_CHECK_ARG(aligned16(rois) && aligned8(gt_idx) && aligned4(out));
    hipLaunchKernelGGL(mask_targets_kernel, dim3(P, B), dim3(MASK_THREADS), 0, (hipStream_t)stream, masks, rois, gt_idx, pos_valid, P, Gmax, H, W,
                       size, out);
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
