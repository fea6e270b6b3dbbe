// The RPN's proposals of a whole batch (detector.proposals_batch: MiniMaskRCNN._proposals image by image, stacked) -- gfx950 only.
//
// Everything is read from device memory, nothing is read back, no buffer has to be cleared between calls and there are no atomics, so a
// captured step takes the next batch's logits and deltas by replaying on the same buffers.  The number of launches depends on the level
// sizes, nms_pre and P only, never on B.
//
// (1) SELECTION, per (image, level): the first k_l = min(nms_pre, n_l) candidates in descending score, equal scores in ascending anchor
//     index (detector._topk_stable).  The order is that of the composite (descending_key(score) << 32 | index within the level), unique per
//     candidate, taken through a reduction tree of LDS chunk sorts (pswin_chunk_sort.hpp) over grid (chunks, L, B): pass 0 reads the scores,
//     every chunk keeps its first k_l composites, the next pass sorts those, until a level is down to one chunk.  k_l <= PROP_ROWS / 4, so
//     every pass shrinks a level's chunks at least fourfold; a level that is finished takes no part in the later passes.
//     The pass that finishes a level gathers anchor and delta of its k_l candidates, decodes them as detector.decode_deltas does in
//     float32, operation by operation (the library is built with -ffp-contract=off; only expf may differ from the host), and writes boxes
//     and sorted scores straight into the layout of pswin_nms_groups, [B L][nmax][4], with the list's count.
// (2) NMS: pswin_nms_groups on all B L lists at once.
// (3) FINAL ORDER, per image: the candidates of all levels concatenated level-major in rank order, a suppressed candidate's score -1e4;
//     the first P in descending score, equal scores in ascending concatenated position -- the same tree with the composite
//     (descending_key(score) << 32 | position).  Its last pass writes rois, scores and count.
//
// Every index taken from a composite is clamped into range before it is used: scores outside the contract (NaN) leave the order
// unspecified, but nothing is gathered out of bounds.
#include "pswin_chunk_sort.hpp"

#include <math.h>

namespace {
using namespace pswin;

constexpr int PROP_THREADS = 1024, PROP_ROWS = 8192;            // 8192 composites of 8 bytes: the 64 KB of LDS one workgroup may declare
constexpr int PROP_KMAX = PROP_ROWS / 4;                        // nms_pre and P: also the row limit of pswin_nms_groups
constexpr int PROP_LMAX = 8;
constexpr int PROP_GROUPS_MAX = 2048;                           // B L: the group limit of pswin_nms_groups
constexpr int PROP_PASSES_MAX = 16;
constexpr float PROP_SUPPRESSED = -1e4f;

// the lists of one tree: the pyramid levels of an image (selection) or the image itself (final order)
struct Lists {
    int n[PROP_LMAX];           // candidates of a list
    int k[PROP_LMAX];           // composites a chunk keeps
    int first[PROP_LMAX + 1];   // selection: the level's first anchor; final order: the level's first concatenated position
    int count;
};

// one pass of a tree
struct Pass {
    int M[PROP_LMAX];               // composites of a list this pass reads (pass 0: its candidates); 0: the list takes no part
    int last[PROP_LMAX];            // one chunk is left: the pass writes the list's result
    long long in_off[PROP_LMAX], out_off[PROP_LMAX];      // the list's place in an image's region of the buffer read / written, composites
    long long in_stride, out_stride;                    // composites per image in those buffers
    int chunks;                     // the most chunks any list has: grid.x
    int in_buf, out_buf;            // 0 / 1; -1: none (pass 0 reads the scores, a pass in which every list is finished writes no composites)
};

struct Plan {
    Pass pass[PROP_PASSES_MAX];
    int passes;
    long long total[2];             // composites per image of the two buffers the passes write in turn
};

inline long long chunks_of(long long m) { return (m + PROP_ROWS - 1) / PROP_ROWS; }

// The passes of a tree over lists of n[l] candidates that keeps k[l] <= PROP_KMAX per chunk.  Pass p writes buffer p & 1; a list lies at the
// same offset in every pass of one parity (its later outputs are shorter than its first).
bool plan_tree(const Lists& ls, Plan& pl) {
    long long M[PROP_LMAX], cap[2][PROP_LMAX] = {};
    for (int half = 0; half < 2; ++half) {                     // first the sizes of passes 0 and 1, then the passes themselves
        bool done[PROP_LMAX] = {};
        long long off[2][PROP_LMAX];
        for (int q = 0; q < 2; ++q) {
            long long at = 0;
            for (int l = 0; l < ls.count; ++l) {
                off[q][l] = at;
                at += cap[q][l];
            }
            pl.total[q] = at;
        }
        for (int l = 0; l < ls.count; ++l) M[l] = ls.n[l];
        for (int p = 0;; ++p) {
            if (p == PROP_PASSES_MAX) return false;
            Pass& ps = pl.pass[p];
            const int q = p & 1;
            bool any = false, writes = false;
            ps.chunks = 0;
            for (int l = 0; l < ls.count; ++l) {
                ps.M[l] = 0;
                ps.last[l] = 0;
                ps.in_off[l] = p ? off[q ^ 1][l] : 0;
                ps.out_off[l] = off[q][l];
                if (done[l]) continue;
                const long long c = chunks_of(M[l]);
                ps.M[l] = (int)M[l];
                ps.chunks = c > ps.chunks ? (int)c : ps.chunks;
                if (c == 1) {
                    ps.last[l] = 1;
                    done[l] = true;
                } else {
                    M[l] = c * ls.k[l];
                    if (p < 2) cap[q][l] = M[l];
                    any = writes = true;
                }
            }
            ps.in_stride = p ? pl.total[q ^ 1] : 0;
            ps.out_stride = pl.total[q];
            ps.in_buf = p ? (q ^ 1) : -1;
            ps.out_buf = writes ? q : -1;
            if (!any) {
                pl.passes = p + 1;
                break;
            }
        }
    }
    return true;
}

// detector.decode_deltas(anchor, delta, stds = 1, (H, W)), operation by operation in float32 (a product with the std 1 is the factor itself)
__device__ inline f32x4 decode_box(f32x4 a, f32x4 d, float clip, float fH, float fW) {
    const float sw = a[2] - a[0], sh = a[3] - a[1];
    const float sx = (a[0] + a[2]) * 0.5f, sy = (a[1] + a[3]) * 0.5f;
    const float w = sw * expf(fminf(fmaxf(d[2], -clip), clip)), h = sh * expf(fminf(fmaxf(d[3], -clip), clip));
    const float x = sx + sw * d[0], y = sy + sh * d[1];
    const float hw = w * 0.5f, hh = h * 0.5f;
    return f32x4{fminf(fmaxf(x - hw, 0.f), fW), fminf(fmaxf(y - hh, 0.f), fH), fminf(fmaxf(x + hw, 0.f), fW), fminf(fmaxf(y + hh, 0.f), fH)};
}

// the chunk of composites a later pass reads, or pads behind the list's end
__device__ inline void load_composites(chunk_u64* s, const chunk_u64* __restrict__ src, int chunk, int M) {
    for (int r = threadIdx.x; r < PROP_ROWS; r += PROP_THREADS) {
        const long long i = (long long)chunk * PROP_ROWS + r;
        s[r] = i < M ? src[i] : CHUNK_PAD;
    }
}

__device__ inline void store_kept(const chunk_u64* s, chunk_u64* __restrict__ dst, int kept) {
    for (int r = threadIdx.x; r < kept; r += PROP_THREADS) dst[r] = s[r];
}

// grid (chunks, L, B).  scores f32 [B][A], deltas f32 [B][A][4], anchors f32 [A][4].  The pass that finishes level l of image b writes
// boxes[b L + l][r], sorted[b L + l][r] for r < k_l and counts[b L + l] = k_l.
__global__ __launch_bounds__(PROP_THREADS) void proposals_select_kernel(const float* __restrict__ scores, const float* __restrict__ deltas,
                                                                       const float* __restrict__ anchors, Lists lv, Pass ps, int A,
                                                                       const chunk_u64* __restrict__ in, chunk_u64* __restrict__ out, int nmax,
                                                                       float clip, float fH, float fW, float* __restrict__ boxes,
                                                                       float* __restrict__ sorted, int* __restrict__ counts) {
    __shared__ chunk_u64 s[PROP_ROWS];
    const int chunk = blockIdx.x, l = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const int M = ps.M[l];
    if ((long long)chunk * PROP_ROWS >= M) return;              // the whole workgroup: a finished level, or a level with fewer chunks
    const int n = lv.n[l], k = lv.k[l];
    const float* sc = scores + (size_t)b * A + lv.first[l];
    if (in) {
        load_composites(s, in + (size_t)b * ps.in_stride + ps.in_off[l], chunk, M);
    } else {
        for (int r = t; r < PROP_ROWS; r += PROP_THREADS) {
            const long long i = (long long)chunk * PROP_ROWS + r;
            s[r] = i < n ? descending_composite(sc[i], (unsigned)i) : CHUNK_PAD;
        }
    }
    chunk_sort_ascending<PROP_ROWS, PROP_THREADS>(s);
    if (!ps.last[l]) {
        store_kept(s, out + (size_t)b * ps.out_stride + ps.out_off[l] + (size_t)chunk * k, k);
        return;
    }
    const size_t g = (size_t)b * gridDim.y + l;
    const f32x4* an = reinterpret_cast<const f32x4*>(anchors) + lv.first[l];
    const f32x4* de = reinterpret_cast<const f32x4*>(deltas) + (size_t)b * A + lv.first[l];
    for (int r = t; r < k; r += PROP_THREADS) {
        unsigned i = (unsigned)(s[r] & 0xffffffffull);
        i = i < (unsigned)n ? i : (unsigned)(n - 1);            // a pad only with scores outside the contract: stay in range
        reinterpret_cast<f32x4*>(boxes)[g * nmax + r] = decode_box(an[i], de[i], clip, fH, fW);
        sorted[g * nmax + r] = sc[i];
    }
    if (t == 0) counts[g] = k;
}

// the level of concatenated position q and its rank there
__device__ inline int level_of(const Lists& lv, int q, int& rank) {
    int l = 0;
    while (l + 1 < lv.count && q >= lv.first[l + 1]) ++l;
    rank = q - lv.first[l];
    return l;
}

// grid (chunks, 1, B).  boxes / sorted / keep: what the selection and the NMS left, [B L][nmax]; lv.first: the levels' first concatenated
// positions, lv.first[L] = K.  The last pass writes rois f32 [B][P][4], out_scores f32 [B][P] and count int32 [B].
__global__ __launch_bounds__(PROP_THREADS) void proposals_order_kernel(const float* __restrict__ boxes, const float* __restrict__ sorted,
                                                                      const unsigned char* __restrict__ keep, Lists lv, Pass ps,
                                                                      const chunk_u64* __restrict__ in, chunk_u64* __restrict__ out, int nmax,
                                                                      int P, float* __restrict__ rois, float* __restrict__ out_scores,
                                                                      int* __restrict__ count) {
    __shared__ chunk_u64 s[PROP_ROWS];
    const int chunk = blockIdx.x, b = blockIdx.z, t = threadIdx.x;
    const int M = ps.M[0], K = lv.first[lv.count];
    if ((long long)chunk * PROP_ROWS >= M) return;
    const size_t g0 = (size_t)b * lv.count;
    auto score_at = [&](int q, size_t& row) {
        int rank;
        const int l = level_of(lv, q, rank);
        row = (g0 + l) * nmax + rank;
        return keep[row] ? sorted[row] : PROP_SUPPRESSED;
    };
    if (in) {
        load_composites(s, in + (size_t)b * ps.in_stride + ps.in_off[0], chunk, M);
    } else {
        for (int r = t; r < PROP_ROWS; r += PROP_THREADS) {
            const long long q = (long long)chunk * PROP_ROWS + r;
            size_t row;
            s[r] = q < K ? descending_composite(score_at((int)q, row), (unsigned)q) : CHUNK_PAD;
        }
    }
    chunk_sort_ascending<PROP_ROWS, PROP_THREADS>(s);
    if (!ps.last[0]) {
        store_kept(s, out + (size_t)b * ps.out_stride + ps.out_off[0] + (size_t)chunk * P, P);
        return;
    }
    int mine = 0;
    for (int r = t; r < P; r += PROP_THREADS) {
        unsigned q = (unsigned)(s[r] & 0xffffffffull);
        q = q < (unsigned)K ? q : (unsigned)(K - 1);
        size_t row;
        const float v = score_at((int)q, row);
        reinterpret_cast<f32x4*>(rois)[(size_t)b * P + r] = reinterpret_cast<const f32x4*>(boxes)[row];
        out_scores[(size_t)b * P + r] = v;
        mine += v > PROP_SUPPRESSED ? 1 : 0;
    }
    // the survivors of the image: an integer sum, whatever the order (the sorted chunk is no longer needed: its LDS holds the partial sums)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    __syncthreads();
    int* red = reinterpret_cast<int*>(s);
    if ((t & 63) == 0) red[t >> 6] = mine;
    __syncthreads();
    if (t == 0) {
        int total = 0;
        for (int w = 0; w < PROP_THREADS / 64; ++w) total += red[w];
        count[b] = total;
    }
}

// what a call works on: the lists of both trees, their plans and the places of everything in the workspace (bytes)
struct Layout {
    Lists levels, image;
    Plan select, order;
    int A, K, P, nmax, groups;
    long long sel[2], ord[2], boxes, sorted, counts, keep, masks, bytes;
};

inline long long align256(long long v) { return (v + 255) / 256 * 256; }

bool make_layout(const int* level_sizes, int L, int B, int nms_pre, int max_per_img, Layout& w) {
    if (!level_sizes || L < 1 || L > PROP_LMAX || B < 1 || nms_pre < 1 || nms_pre > PROP_KMAX || max_per_img < 1) return false;
    if ((long long)B * L > PROP_GROUPS_MAX) return false;
    long long A = 0, K = 0;
    int kmax = 0;
    w.levels.count = L;
    for (int l = 0; l < L; ++l) {
        const int n = level_sizes[l];
        if (n < 1) return false;
        const int k = n < nms_pre ? n : nms_pre;
        w.levels.n[l] = n;
        w.levels.k[l] = k;
        w.levels.first[l] = (int)A;
        w.image.first[l] = (int)K;
        A += n;
        K += k;
        kmax = k > kmax ? k : kmax;
        if (A * B > 0x7fffffffLL) return false;
    }
    w.levels.first[L] = (int)A;
    w.image.first[L] = (int)K;
    w.A = (int)A;
    w.K = (int)K;
    w.P = K < max_per_img ? (int)K : max_per_img;
    if (w.P > PROP_KMAX) return false;
    w.image.count = L;                        // level_of walks the levels; the tree has ONE list per image, list 0
    w.image.n[0] = w.K;
    w.image.k[0] = w.P;
    w.nmax = ceil_to(kmax, 64);
    w.groups = B * L;
    Lists one = w.image;
    one.count = 1;
    if (!plan_tree(w.levels, w.select) || !plan_tree(one, w.order)) return false;
    const int nms = pswin_nms_workspace(w.groups, w.nmax);
    if (nms <= 0) return false;
    long long at = 0;
    auto take = [&](long long bytes) {
        const long long here = at;
        at = align256(at + bytes);
        return here;
    };
    for (int q = 0; q < 2; ++q) w.sel[q] = take((long long)B * w.select.total[q] * 8);
    for (int q = 0; q < 2; ++q) w.ord[q] = take((long long)B * w.order.total[q] * 8);
    w.boxes = take((long long)w.groups * w.nmax * 16);
    w.sorted = take((long long)w.groups * w.nmax * 4);
    w.keep = take((long long)w.groups * w.nmax);
    w.counts = take((long long)w.groups * 4);
    w.masks = take(nms);
    w.bytes = at;
    return at <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int pswin_rpn_proposals_rows_per_workgroup(void) { return PROP_ROWS; }

int pswin_rpn_proposals_launches(const int* level_sizes, int L, int nms_pre, int max_per_img) {
    Layout w;
    if (!make_layout(level_sizes, L, 1, nms_pre, max_per_img, w)) return PSWIN_ERR_ARG;
    return w.select.passes + 2 + w.order.passes;
}

int pswin_rpn_proposals_workspace(const int* level_sizes, int L, int B, int nms_pre, int max_per_img) {
    Layout w;
    if (!make_layout(level_sizes, L, B, nms_pre, max_per_img, w)) return PSWIN_ERR_ARG;
    return (int)w.bytes;
}

int pswin_rpn_proposals(const float* scores, const float* deltas, const float* anchors, const int* level_sizes, int L, int B, int nms_pre,
                        float iou_thr, int max_per_img, int img_h, int img_w, float* rois, float* out_scores, int32_t* count, void* workspace,
                        void* stream) {
    PSWIN_CHECK_ARG(scores && deltas && anchors && rois && out_scores && count && workspace && img_h >= 1 && img_w >= 1 && iou_thr >= 0.f);
    PSWIN_CHECK_ARG(aligned16(deltas) && aligned16(anchors) && aligned16(rois) && aligned16(workspace));
    PSWIN_CHECK_ARG((reinterpret_cast<uintptr_t>(scores) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_scores) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(count) & 3) == 0);
    Layout w;
    PSWIN_CHECK_ARG(make_layout(level_sizes, L, B, nms_pre, max_per_img, w));
    char* ws = reinterpret_cast<char*>(workspace);
    chunk_u64* sel[2] = {reinterpret_cast<chunk_u64*>(ws + w.sel[0]), reinterpret_cast<chunk_u64*>(ws + w.sel[1])};
    chunk_u64* ord[2] = {reinterpret_cast<chunk_u64*>(ws + w.ord[0]), reinterpret_cast<chunk_u64*>(ws + w.ord[1])};
    float* boxes = reinterpret_cast<float*>(ws + w.boxes);
    float* sorted = reinterpret_cast<float*>(ws + w.sorted);
    unsigned char* keep = reinterpret_cast<unsigned char*>(ws + w.keep);
    int* counts = reinterpret_cast<int*>(ws + w.counts);
    const float clip = (float)fabs(log(16.0 / 1000.0));
    for (int p = 0; p < w.select.passes; ++p) {
        const Pass& ps = w.select.pass[p];
        hipLaunchKernelGGL(proposals_select_kernel, dim3(ps.chunks, L, B), dim3(PROP_THREADS), 0, (hipStream_t)stream, scores, deltas, anchors,
                           w.levels, ps, w.A, ps.in_buf < 0 ? nullptr : sel[ps.in_buf], ps.out_buf < 0 ? nullptr : sel[ps.out_buf], w.nmax, clip,
                           (float)img_h, (float)img_w, boxes, sorted, counts);
    }
    const int rc = pswin_nms_groups(boxes, counts, w.groups, w.nmax, iou_thr, keep, ws + w.masks, stream);
    if (rc != PSWIN_OK) return rc;
    for (int p = 0; p < w.order.passes; ++p) {
        const Pass& ps = w.order.pass[p];
        hipLaunchKernelGGL(proposals_order_kernel, dim3(ps.chunks, 1, B), dim3(PROP_THREADS), 0, (hipStream_t)stream, boxes, sorted, keep, w.image,
                           ps, ps.in_buf < 0 ? nullptr : ord[ps.in_buf], ps.out_buf < 0 ? nullptr : ord[ps.out_buf], w.nmax, w.P, rois,
                           out_scores, count);
    }
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
