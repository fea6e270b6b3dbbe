// Test-time augmentation behind the heads: the merges of multi-scale / flipped test views (tta.py; mmdet/core/post_processing/merge_augs.py,
// mmdet/core/bbox/transforms.py bbox_mapping / bbox_mapping_back) for a whole batch with fixed shapes -- gfx950 only.
//
// The views' geometry is HOST data (pswin_aug_view, V <= 8), copied into the kernels' arguments: fixed when a call is captured.  Everything
// else is read from device memory, nothing is read back, every output element is written by plain stores on every call (no memset, no
// atomics), and float32 arithmetic goes operation by operation (the library is built with -ffp-contract=off; only expf may differ from the
// host's), so tta.map_to_view, map_back and merge_aug_proposals are met bit for bit.
//
//   pswin_aug_merge_proposals  the first count[v][b] proposals of every view mapped back, concatenated view-major, greedy NMS in descending
//       score, the first max_per_img survivors.  Three launches whatever V, B and P: (1) one workgroup per image sorts the V P composites
//       (descending_key(score) << 32 | concatenated position) in LDS (pswin_chunk_sort.hpp; V P <= 8192 is one chunk) and writes the
//       mapped-back boxes in that order; (2) the suppression bit masks, one 64-thread workgroup per (64 rows, one 64-column word, image),
//       up to 128 words per row -- pswin_nms_groups stops at 32; (3) one wave per image walks the rows in order, lane w owning words w and
//       w + 64 of the removed set, the rows' words fetched one batch of 16 rows ahead, and writes a survivor straight to its output row (its
//       rank is a population count); it stops once max_per_img rows are out.
//   pswin_aug_map_rois         [B][N][4] -> [V][B][N][4], bbox_mapping of every view in one launch.
//   pswin_aug_merge_bboxes     per view softmax and decode_deltas clipped to the view, mapped back; summed in view order, divided by V.  One
//       wave per proposal: lane c (+ 64, + 128) owns class c; the softmax's maximum and sum are wave reductions.
//   pswin_multiclass_nms_*_boxes   the class-wise NMS chain of pswin_detect.hip on given boxes and probabilities (pswin_detect_post.hpp).
//   pswin_paste_masks_aug      the paste of pswin_detect.hip whose staged 28 x 28 tile is the mean over up to 24 sources of the sigmoid of
//       the label's channel, columns reversed for a flipped source; no merged probability is written to memory.
#include "pswin_chunk_sort.hpp"
#include "pswin_detect_post.hpp"

#include <math.h>

namespace {
using namespace pswin;

constexpr int AUG_VMAX = PSWIN_AUG_VIEWS_MAX, AUG_SRC_MAX = PSWIN_AUG_MASK_SOURCES_MAX;
constexpr int AUG_ROWS_MAX = 8192, AUG_SORT_THREADS = 1024, AUG_THREADS = 256;

struct AugViews {
    float h[AUG_VMAX], w[AUG_VMAX];
    float s[AUG_VMAX][4];
    int flip[AUG_VMAX];
    int V;
};

bool aug_views(const pswin_aug_view* views, int V, AugViews& a) {
    if (!views || V < 1 || V > AUG_VMAX) return false;
    a = AugViews{};
    a.V = V;
    for (int v = 0; v < V; ++v) {
        if (views[v].img_h < 1 || views[v].img_w < 1) return false;
        a.h[v] = (float)views[v].img_h;
        a.w[v] = (float)views[v].img_w;
        for (int k = 0; k < 4; ++k) {
            if (!(views[v].scale[k] > 0.f) || !(views[v].scale[k] < INFINITY)) return false;
            a.s[v][k] = views[v].scale[k];
        }
        a.flip[v] = views[v].flip != 0;
    }
    return true;
}

// tta.map_back (bbox_mapping_back): un-flip with the view's width, then divide by the scale factor
__device__ inline f32x4 aug_map_back(f32x4 b, const AugViews& vw, int v) {
    if (vw.flip[v]) {
        const float x0 = vw.w[v] - b[2], x2 = vw.w[v] - b[0];
        b[0] = x0;
        b[2] = x2;
    }
    return f32x4{b[0] / vw.s[v][0], b[1] / vw.s[v][1], b[2] / vw.s[v][2], b[3] / vw.s[v][3]};
}

// tta.map_to_view (bbox_mapping): multiply by the scale factor, then flip with the view's width
__device__ inline f32x4 aug_map_to(f32x4 b, const AugViews& vw, int v) {
    f32x4 o = {b[0] * vw.s[v][0], b[1] * vw.s[v][1], b[2] * vw.s[v][2], b[3] * vw.s[v][3]};
    if (vw.flip[v]) {
        const float x0 = vw.w[v] - o[2], x2 = vw.w[v] - o[0];
        o[0] = x0;
        o[2] = x2;
    }
    return o;
}

// ---- proposals -----------------------------------------------------------------------------------------------------------------------------
// (1) grid (B).  props f32 [V][B][P][4], scores f32 [V][B][P], count int32 [V][B] -> sboxes f32 [B][Np][4] and sscores f32 [B][Np] in the
// order of the composites (rows past the image's n candidates: zeros), n[b]
template <int ROWS>
__global__ __launch_bounds__(AUG_SORT_THREADS) void aug_sort_kernel(const float* __restrict__ props, const float* __restrict__ scores,
                                                                    const int* __restrict__ count, AugViews vw, int B, int P, int Np,
                                                                    float* __restrict__ sboxes, float* __restrict__ sscores,
                                                                    int* __restrict__ n_out) {
    __shared__ chunk_u64 s[ROWS];                               // all of the 64 KB a workgroup may declare at ROWS = 8192
    const int b = blockIdx.x, t = threadIdx.x, N = vw.V * P;
    for (int q = t; q < ROWS; q += AUG_SORT_THREADS) {
        chunk_u64 c = CHUNK_PAD;
        if (q < N) {
            const int v = q / P, r = q - v * P;
            if (r < det_clamp(count[v * B + b], P)) c = descending_composite(scores[((size_t)v * B + b) * P + r], (unsigned)q);
        }
        s[q] = c;
    }
    chunk_sort_ascending<ROWS, AUG_SORT_THREADS>(s);
    for (int j = t; j < Np; j += AUG_SORT_THREADS) {            // Np <= ROWS
        const chunk_u64 c = s[j];
        f32x4 box = {0.f, 0.f, 0.f, 0.f};
        float sc = 0.f;
        if (c != CHUNK_PAD) {
            unsigned q = (unsigned)(c & 0xffffffffull);
            q = q < (unsigned)N ? q : (unsigned)(N - 1);
            const int v = (int)q / P, r = (int)q - v * P;
            const size_t row = ((size_t)v * B + b) * P + r;
            box = aug_map_back(reinterpret_cast<const f32x4*>(props)[row], vw, v);
            sc = scores[row];
        }
        reinterpret_cast<f32x4*>(sboxes)[(size_t)b * Np + j] = box;
        sscores[(size_t)b * Np + j] = sc;
    }
    if (t == 0) {
        int n = 0;
        for (int v = 0; v < vw.V; ++v) n += det_clamp(count[v * B + b], P);
        n_out[b] = n;
    }
}

// (2) grid (NW, NW, B), NW = Np / 64.  mask[b][i][w] bit j: IoU(i, 64 w + j) > thr, columns right of the row only (detector.box_iou: clamped
// widths, union floored at 1e-6 -- the rule of pswin_nms_groups).  Written for the rows of every started 64-row chunk and the words that
// hold a column below n; nothing else is read by the walk.
__global__ __launch_bounds__(64) void aug_mask_kernel(const float* __restrict__ sboxes, const int* __restrict__ n_in, int Np, int NW, float thr,
                                                      unsigned long long* __restrict__ mask) {
    __shared__ f32x4 cb[64];
    __shared__ float ca[64];
    const int w = blockIdx.x, rc = blockIdx.y, b = blockIdx.z, r = threadIdx.x;
    if (w < rc) return;
    const int n = det_clamp(n_in[b], Np);
    if (64 * rc >= n || 64 * w >= n) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(sboxes) + (size_t)b * Np;
    const int j = 64 * w + r, i = 64 * rc + r;
    if (j < n) {
        const f32x4 bx = src[j];
        cb[r] = bx;
        ca[r] = fmaxf(bx[2] - bx[0], 0.f) * fmaxf(bx[3] - bx[1], 0.f);
    }
    __syncthreads();
    unsigned long long bits = 0ull;
    if (i < n) {
        const f32x4 a = src[i];
        const float aa = fmaxf(a[2] - a[0], 0.f) * fmaxf(a[3] - a[1], 0.f);
        const int jn = n - 64 * w < 64 ? n - 64 * w : 64;
        for (int jj = 0; jj < jn; ++jj) {
            const f32x4 bx = cb[jj];
            const float iw = fmaxf(fminf(a[2], bx[2]) - fmaxf(a[0], bx[0]), 0.f), ih = fmaxf(fminf(a[3], bx[3]) - fmaxf(a[1], bx[1]), 0.f);
            const float inter = iw * ih;
            const float iou = inter / fmaxf(aa + ca[jj] - inter, 1e-6f);
            if (64 * w + jj > i && iou > thr) bits |= 1ull << jj;
        }
    }
    mask[((size_t)b * Np + i) * NW + w] = bits;                 // i < Np: chunks are whole
}

// (3) grid (B), one wave.  The greedy rule in row order; a survivor of rank k < Pm goes to rois[b][k] / scores[b][k]; rows past the count
// are zeros.
__global__ __launch_bounds__(64) void aug_scan_kernel(const int* __restrict__ n_in, int Np, int NW, const unsigned long long* __restrict__ mask,
                                                      const float* __restrict__ sboxes, const float* __restrict__ sscores, int Pm,
                                                      float* __restrict__ rois, float* __restrict__ scores, int* __restrict__ count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = det_clamp(n_in[b], Np);
    const int words = (n + 63) >> 6;
    const unsigned long long* mg = mask + (size_t)b * Np * NW;
    unsigned long long remv0 = 0ull, remv1 = 0ull;              // lane w holds words w and w + 64 of the removed set
    const int batches = 4 * words;                              // batch t = rows 16 t .. 16 t + 15, chunk c = t >> 2
    auto fetch = [&](int t, unsigned long long (&m0)[16], unsigned long long (&m1)[16]) {
        const int c = t >> 2;
        const bool on0 = t < batches && lane >= c && lane < words, on1 = t < batches && lane + 64 >= c && lane + 64 < words;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const size_t row = (size_t)(16 * t + r) * NW;
            m0[r] = on0 ? mg[row + lane] : 0ull;
            m1[r] = on1 ? mg[row + 64 + lane] : 0ull;
        }
    };
    auto lane64 = [&](unsigned long long v, int l) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), l);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
        return ((unsigned long long)hi << 32) | lo;
    };
    unsigned long long cur = 0ull, kw = 0ull;                   // word c of the removed set as a scalar; the chunk's verdicts
    int kept = 0;                                               // survivors so far: wave-uniform
    auto walk = [&](int t, const unsigned long long (&m0)[16], const unsigned long long (&m1)[16]) {
        const int c = t >> 2;
        const bool low = c < 64;                                // wave-uniform
        if ((t & 3) == 0) {
            cur = lane64(low ? remv0 : remv1, c & 63);
            kw = 0ull;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = 16 * (t & 3) + r, i = 16 * t + r;
            if (i < n && !((cur >> rr) & 1ull)) {               // wave-uniform
                remv0 |= m0[r];
                remv1 |= m1[r];
                cur |= lane64(low ? m0[r] : m1[r], c & 63);
                kw |= 1ull << rr;
            }
        }
        if ((t & 3) == 3) {
            const bool mine = (kw >> lane) & 1ull;
            const int rank = kept + __builtin_popcountll(kw & ((1ull << lane) - 1ull));
            if (mine && rank < Pm) {
                const size_t src = (size_t)b * Np + 64 * c + lane, dst = (size_t)b * Pm + rank;
                reinterpret_cast<f32x4*>(rois)[dst] = reinterpret_cast<const f32x4*>(sboxes)[src];
                scores[dst] = sscores[src];
            }
            kept += __builtin_popcountll(kw);
        }
    };
    unsigned long long a0[16], a1[16], b0[16], b1[16];
    fetch(0, a0, a1);
    for (int t = 0; t < batches; t += 2) {
        if ((t & 3) == 0 && kept >= Pm) break;
        fetch(t + 1, b0, b1);
        walk(t, a0, a1);
        fetch(t + 2, a0, a1);
        walk(t + 1, b0, b1);
    }
    const int total = kept < Pm ? kept : Pm;
    for (int k = total + lane; k < Pm; k += 64) {
        reinterpret_cast<f32x4*>(rois)[(size_t)b * Pm + k] = f32x4{0.f, 0.f, 0.f, 0.f};
        scores[(size_t)b * Pm + k] = 0.f;
    }
    if (lane == 0) count[b] = total;
}

struct PropLayout {
    int N, Np, NW, Pm;
    long long boxes, scores, n, masks, bytes;
};

bool prop_layout(int V, int B, int P, int max_per_img, PropLayout& w) {
    if (V < 1 || V > AUG_VMAX || B < 1 || B > 65535 || P < 1 || max_per_img < 1 || (long long)V * P > AUG_ROWS_MAX) return false;
    w.N = V * P;
    w.Np = ceil_to(w.N, 64);
    w.NW = w.Np / 64;
    w.Pm = max_per_img < w.N ? max_per_img : w.N;
    auto up = [](long long v) { return (v + 255) / 256 * 256; };
    w.boxes = 0;
    w.scores = up(w.boxes + (long long)B * w.Np * 16);
    w.n = up(w.scores + (long long)B * w.Np * 4);
    w.masks = up(w.n + (long long)B * 4);
    w.bytes = w.masks + (long long)B * w.Np * w.NW * 8;
    return w.bytes <= 0x7fffffffLL;
}

// ---- map_rois --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_map_rois_kernel(const float* __restrict__ boxes, AugViews vw, int BN, float* __restrict__ out) {
    const int i = blockIdx.x * AUG_THREADS + threadIdx.x, v = blockIdx.y;
    if (i >= BN) return;
    reinterpret_cast<f32x4*>(out)[(size_t)v * BN + i] = aug_map_to(reinterpret_cast<const f32x4*>(boxes)[i], vw, v);
}

// ---- merge_bboxes ----------------------------------------------------------------------------------------------------------------------------
struct AugHeads {
    const float* rois[AUG_VMAX];                                // f32 [B][R][4] of each view
    const void* cls[AUG_VMAX];                                  // [B][R][C + 1]
    const void* deltas[AUG_VMAX];                               // [B][R][4 C]
};

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

constexpr int AUG_SLOTS = (DET_CMAX + 1 + 63) / 64;             // classes (and the background column) a lane owns: c = lane + 64 j

// grid (ceil(R / 4), B), one wave per proposal.  boxes f32 [B][R][4 C], scores f32 [B][R][C + 1]
template <int CDT, int DDT>
__global__ __launch_bounds__(AUG_THREADS) void aug_merge_bboxes_kernel(AugHeads hp, AugViews vw, f32x4 stds, float clip, int R, int C,
                                                                       float* __restrict__ boxes, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (AUG_THREADS / 64) + (threadIdx.x >> 6), b = blockIdx.y;
    if (r >= R) return;                                         // a whole wave
    const size_t row = (size_t)b * R + r;
    float accs[AUG_SLOTS];
    f32x4 accb[AUG_SLOTS];
#pragma unroll
    for (int j = 0; j < AUG_SLOTS; ++j) {
        accs[j] = 0.f;
        accb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int v = 0; v < vw.V; ++v) {
        const f32x4 s = reinterpret_cast<const f32x4*>(hp.rois[v])[row];
        float l[AUG_SLOTS], e[AUG_SLOTS];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < AUG_SLOTS; ++j) {
            const int c = lane + 64 * j;
            l[j] = c <= C ? det_load(hp.cls[v], CDT, row * (size_t)(C + 1) + c) : -INFINITY;
            m = fmaxf(m, l[j]);
        }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < AUG_SLOTS; ++j) {
            e[j] = lane + 64 * j <= C ? expf(l[j] - m) : 0.f;
            sum += e[j];
        }
        sum = wave_sum(sum);
        const float sw = s[2] - s[0], sh = s[3] - s[1];
        const float sx = (s[0] + s[2]) * 0.5f, sy = (s[1] + s[3]) * 0.5f;
        const float fW = vw.w[v], fH = vw.h[v];
#pragma unroll
        for (int j = 0; j < AUG_SLOTS; ++j) {
            const int c = lane + 64 * j;
            accs[j] += e[j] / sum;
            if (c < C) {                                        // detector.decode_deltas, operation by operation
                const f32x4 d = load4<DDT>(hp.deltas[v], row * (size_t)(4 * C) + 4 * c) * stds;
                const float w = sw * expf(fminf(fmaxf(d[2], -clip), clip)), h = sh * expf(fminf(fmaxf(d[3], -clip), clip));
                const float x = sx + sw * d[0], y = sy + sh * d[1];
                const float hw = w * 0.5f, hh = h * 0.5f;
                const f32x4 bx = {fminf(fmaxf(x - hw, 0.f), fW), fminf(fmaxf(y - hh, 0.f), fH), fminf(fmaxf(x + hw, 0.f), fW),
                                  fminf(fmaxf(y + hh, 0.f), fH)};
                accb[j] += aug_map_back(bx, vw, v);
            }
        }
    }
    const float fV = (float)vw.V;
#pragma unroll
    for (int j = 0; j < AUG_SLOTS; ++j) {
        const int c = lane + 64 * j;
        if (c <= C) scores[row * (size_t)(C + 1) + c] = accs[j] / fV;
        if (c < C) reinterpret_cast<f32x4*>(boxes)[row * (size_t)C + c] = accb[j] / fV;
    }
}

// ---- class-wise NMS on given boxes and probabilities ---------------------------------------------------------------------------------------
struct MergedBoxes {
    const float* boxes;                                         // f32 [B][R][4 C]
    int R, C;
    __device__ inline f32x4 operator()(int b, int r, int c) const { return reinterpret_cast<const f32x4*>(boxes)[((size_t)b * R + r) * C + c]; }
};

// one thread per proposal: key[b][c][r] = scores[b][r][c] if it is above the threshold and r < roi_count[b], else -1
__global__ __launch_bounds__(DET_THREADS) void aug_scores_kernel(const float* __restrict__ scores, const int* __restrict__ roi_count, int R, int C,
                                                                 float score_thr, float* __restrict__ keys) {
    const int b = blockIdx.y, r = blockIdx.x * DET_THREADS + threadIdx.x;
    if (r >= R) return;
    const bool on = r < det_clamp(roi_count[b], R);
    float* kp = keys + (size_t)b * C * R + r;
    const float* sp = scores + ((size_t)b * R + r) * (size_t)(C + 1);
    for (int c = 0; c < C; ++c) {
        const float p = on ? sp[c] : -1.f;
        kp[(size_t)c * R] = p > score_thr ? p : -1.f;
    }
}

// ---- mask paste over several sources ---------------------------------------------------------------------------------------------------------
struct AugMaskSources {
    const void* p[AUG_SRC_MAX];
    long long sn[AUG_SRC_MAX], sc[AUG_SRC_MAX], sy[AUG_SRC_MAX], sx[AUG_SRC_MAX];
    int flip[AUG_SRC_MAX];
    int n;
};

template <int DT>
__global__ __launch_bounds__(PASTE_THREADS) void paste_aug_kernel(AugMaskSources src, const long long* __restrict__ labels,
                                                                  const float* __restrict__ boxes, const int* __restrict__ count, int K, int C,
                                                                  int H, int W, float thr, unsigned char* __restrict__ out) {
    __shared__ float prob[PASTE_LD * PASTE_LD];
    const int b = blockIdx.z, k = blockIdx.y, ybase = blockIdx.x * PASTE_ROWS, t = threadIdx.x;
    const size_t det = (size_t)b * K + k;
    const bool live = k < det_clamp(count[b], K);               // the same for the whole workgroup
    f32x4 box = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        box = reinterpret_cast<const f32x4*>(boxes)[det];
        const long long lab = labels[det];
        const long long c = lab < 0 ? 0 : (lab > C - 1 ? C - 1 : lab);
        const float fN = (float)src.n;
        for (int i = t; i < PASTE_LD * PASTE_LD; i += PASTE_THREADS) {
            const int yy = i / PASTE_LD - 1, xx = i % PASTE_LD - 1;
            float v = 0.f;
            if (yy >= 0 && yy < PASTE_M && xx >= 0 && xx < PASTE_M) {
                float sum = 0.f;                                // tta.merge_aug_masks: in source order, then one division
                for (int s = 0; s < src.n; ++s) {
                    const int xs = src.flip[s] ? PASTE_M - 1 - xx : xx;
                    const float l = det_load(src.p[s], DT, (size_t)((long long)det * src.sn[s] + c * src.sc[s] + yy * src.sy[s] + xs * src.sx[s]));
                    sum += 1.f / (1.f + expf(-l));
                }
                v = sum / fN;
            }
            prob[i] = v;
        }
    }
    paste_rows(prob, live, box, det, ybase, H, W, thr, out);
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int pswin_aug_merge_proposals_launches(int V, int P, int max_per_img) {
    PropLayout w;
    return prop_layout(V, 1, P, max_per_img, w) ? 3 : PSWIN_ERR_ARG;
}

int pswin_aug_merge_proposals_workspace(int V, int B, int P, int max_per_img) {
    PropLayout w;
    return prop_layout(V, B, P, max_per_img, w) ? (int)w.bytes : PSWIN_ERR_ARG;
}

int pswin_aug_merge_proposals(const float* props, const float* scores, const int32_t* count, const pswin_aug_view* views, int V, int B, int P,
                              float iou_thr, int max_per_img, float* rois, float* out_scores, int32_t* out_count, void* workspace, void* stream) {
    PSWIN_CHECK_ARG(props && scores && count && rois && out_scores && out_count && workspace && iou_thr >= 0.f);
    PSWIN_CHECK_ARG(aligned16(props) && aligned16(rois) && aligned16(workspace) && aligned_to(scores, 4) && aligned_to(out_scores, 4) &&
                    aligned_to(count, 4) && aligned_to(out_count, 4));
    AugViews vw;
    PropLayout w;
    PSWIN_CHECK_ARG(aug_views(views, V, vw) && prop_layout(V, B, P, max_per_img, w));
    char* ws = reinterpret_cast<char*>(workspace);
    float* sboxes = reinterpret_cast<float*>(ws + w.boxes);
    float* sscores = reinterpret_cast<float*>(ws + w.scores);
    int* n = reinterpret_cast<int*>(ws + w.n);
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(ws + w.masks);
    if (w.N <= 2048)
        hipLaunchKernelGGL(aug_sort_kernel<2048>, dim3(B), dim3(AUG_SORT_THREADS), 0, (hipStream_t)stream, props, scores, count, vw, B, P, w.Np, sboxes,
                           sscores, n);
    else
        hipLaunchKernelGGL(aug_sort_kernel<AUG_ROWS_MAX>, dim3(B), dim3(AUG_SORT_THREADS), 0, (hipStream_t)stream, props, scores, count, vw, B, P, w.Np,
                           sboxes, sscores, n);
    hipLaunchKernelGGL(aug_mask_kernel, dim3(w.NW, w.NW, B), dim3(64), 0, (hipStream_t)stream, sboxes, n, w.Np, w.NW, iou_thr, masks);
    hipLaunchKernelGGL(aug_scan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, n, w.Np, w.NW, masks, sboxes, sscores, w.Pm, rois, out_scores,
                       out_count);
    PSWIN_LAUNCH_RET();
}

int pswin_aug_map_rois(const float* boxes, const pswin_aug_view* views, int V, int B, int N, float* out, void* stream) {
    PSWIN_CHECK_ARG(boxes && out && aligned16(boxes) && aligned16(out) && B >= 1 && N >= 1 && (long long)B * N <= 0x7fffffffLL / 64);
    AugViews vw;
    PSWIN_CHECK_ARG(aug_views(views, V, vw));
    hipLaunchKernelGGL(aug_map_rois_kernel, dim3((B * N + AUG_THREADS - 1) / AUG_THREADS, V), dim3(AUG_THREADS), 0, (hipStream_t)stream, boxes, vw,
                       B * N, out);
    PSWIN_LAUNCH_RET();
}

int pswin_aug_merge_bboxes(const float* const* rois, const void* const* cls, const void* const* deltas, int cls_dtype, int deltas_dtype,
                           const float* stds, const pswin_aug_view* views, int V, int B, int R, int C, float* boxes, float* scores, void* stream) {
    PSWIN_CHECK_ARG(rois && cls && deltas && stds && boxes && scores && valid_dtype(cls_dtype) && valid_dtype(deltas_dtype) && det_shape_ok(B, R, C));
    PSWIN_CHECK_ARG(aligned16(boxes) && aligned_to(scores, 4));
    AugViews vw;
    PSWIN_CHECK_ARG(aug_views(views, V, vw));
    AugHeads hp = {};
    for (int v = 0; v < V; ++v) {
        PSWIN_CHECK_ARG(rois[v] && cls[v] && deltas[v] && aligned16(rois[v]) && aligned_to(cls[v], cls_dtype == PSWIN_F32 ? 4 : 2) &&
                        aligned_to(deltas[v], deltas_dtype == PSWIN_F32 ? 16 : 8));
        hp.rois[v] = rois[v];
        hp.cls[v] = cls[v];
        hp.deltas[v] = deltas[v];
    }
    const f32x4 s4 = {stds[0], stds[1], stds[2], stds[3]};
    const float clip = (float)fabs(log(16.0 / 1000.0));
    const dim3 grid((R + AUG_THREADS / 64 - 1) / (AUG_THREADS / 64), B);
    return dispatch2(cls_dtype, deltas_dtype, [&](auto cdt, auto ddt) {
        hipLaunchKernelGGL((aug_merge_bboxes_kernel<decltype(cdt)::value, decltype(ddt)::value>), grid, dim3(AUG_THREADS), 0, (hipStream_t)stream, hp,
                           vw, s4, clip, R, C, boxes, scores);
        PSWIN_LAUNCH_RET();
    });
}

int pswin_multiclass_nms_scores_boxes(const float* scores, const int32_t* roi_count, int B, int R, int C, float score_thr, float* keys,
                                      void* stream) {
    PSWIN_CHECK_ARG(scores && roi_count && keys && det_shape_ok(B, R, C) && score_thr >= 0.f && aligned_to(scores, 4) && aligned_to(keys, 4));
    hipLaunchKernelGGL(aug_scores_kernel, dim3((R + DET_THREADS - 1) / DET_THREADS, B), dim3(DET_THREADS), 0, (hipStream_t)stream, scores, roi_count,
                       R, C, score_thr, keys);
    PSWIN_LAUNCH_RET();
}

int pswin_multiclass_nms_boxes(const float* sorted_keys, const long long* sorted_index, const float* merged_boxes, int B, int R, int C,
                               float iou_thr, float* final_keys, void* workspace, void* stream) {
    PSWIN_CHECK_ARG(sorted_keys && sorted_index && merged_boxes && final_keys && workspace && det_shape_ok(B, R, C) && iou_thr >= 0.f);
    PSWIN_CHECK_ARG(aligned16(merged_boxes) && aligned16(workspace) && aligned_to(sorted_index, 8) && aligned_to(sorted_keys, 4) &&
                    aligned_to(final_keys, 4));
    return det_nms_lists(sorted_keys, sorted_index, MergedBoxes{merged_boxes, R, C}, B, iou_thr, final_keys, workspace, stream);
}

int pswin_multiclass_nms_select_boxes(const float* top_keys, const long long* top_index, long long row_stride, int n_sorted,
                                      const float* merged_boxes, int B, int R, int C, int K, float* boxes, float* scores, long long* labels,
                                      int32_t* source, int32_t* count, void* stream) {
    PSWIN_CHECK_ARG(top_keys && top_index && merged_boxes && boxes && scores && labels && source && count);
    PSWIN_CHECK_ARG(det_shape_ok(B, R, C) && K >= 1 && K <= DET_KMAX && n_sorted >= 1 && n_sorted <= R * C && row_stride >= n_sorted);
    PSWIN_CHECK_ARG(aligned16(merged_boxes) && aligned16(boxes) && aligned_to(top_index, 8) && aligned_to(labels, 8) && aligned_to(top_keys, 4) &&
                    aligned_to(scores, 4) && aligned_to(source, 4) && aligned_to(count, 4));
    return det_select(top_keys, top_index, row_stride, n_sorted, MergedBoxes{merged_boxes, R, C}, B, K, boxes, scores, labels, source, count, stream);
}

int pswin_paste_masks_aug(const pswin_aug_mask_sources* sources, int dtype, const long long* labels, const float* boxes, const int32_t* count,
                          int B, int K, int C, int H, int W, float thr, unsigned char* out, void* stream) {
    PSWIN_CHECK_ARG(sources && labels && boxes && count && out && valid_dtype(dtype) && sources->count >= 1 && sources->count <= AUG_SRC_MAX);
    PSWIN_CHECK_ARG(B >= 1 && B <= 65535 && K >= 1 && K <= DET_KMAX && C >= 1 && C <= DET_CMAX && H >= 1 && W >= 1 && H <= 65536 && W <= 65536);
    PSWIN_CHECK_ARG(aligned16(out) && aligned16(boxes) && aligned_to(labels, 8));
    AugMaskSources s = {};
    s.n = sources->count;
    for (int i = 0; i < s.n; ++i) {
        PSWIN_CHECK_ARG(sources->logits[i] && aligned_to(sources->logits[i], dtype == PSWIN_F32 ? 4 : 2));
        PSWIN_CHECK_ARG(sources->stride_n[i] >= 1 && sources->stride_c[i] >= 1 && sources->stride_y[i] >= 1 && sources->stride_x[i] >= 1);
        s.p[i] = sources->logits[i];
        s.sn[i] = sources->stride_n[i];
        s.sc[i] = sources->stride_c[i];
        s.sy[i] = sources->stride_y[i];
        s.sx[i] = sources->stride_x[i];
        s.flip[i] = sources->flip[i] != 0;
    }
    const dim3 grid((H + PASTE_ROWS - 1) / PASTE_ROWS, K, B);
    PSWIN_CHECK_ARG(grid.x <= 65535u);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(paste_aug_kernel<PSWIN_F32>, grid, dim3(PASTE_THREADS), 0, (hipStream_t)stream, s, labels, boxes, count, K, C, H, W, thr, out);
    else
        hipLaunchKernelGGL(paste_aug_kernel<PSWIN_BF16>, grid, dim3(PASTE_THREADS), 0, (hipStream_t)stream, s, labels, boxes, count, K, C, H, W, thr, out);
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
