// COCO run-length encoding of instance masks on the device (panoswintransformerobjectdetection_amd/rle.py states the format) -- gfx950 only.
//
// One bit-level formulation, two producers of column bits, four launches whatever N, B, K or the data are:
//   (1) a producer writes the masks as BIT-PLANES into the workspace: word (n, w, x) holds the pixels y = 64 w .. 64 w + 63 of column x of
//       mask n, bit y & 63, zero past H.  rle_planes_kernel reads the bytes of [N][H][W] bitmaps (a lane owns a column, or 16 adjacent ones
//       with 16-byte loads: the reads of a wavefront are row segments, no transpose); rle_paste_planes_kernel evaluates the mask paste's
//       own sample (paste_stage / paste_axis / paste_value of pswin_detect_post.hpp: the x terms stay in the lane, the y terms belong to
//       the row) and never forms the bitmap.  Planes are an eighth of the bitmap's bytes, and every later pass reads only them.
//   (2) rle_scan_kernel, one workgroup per mask: per column the number of run boundaries -- popcount of w ^ ((w << 1) | carry), carry = the
//       previous word's top bit, for the column's first word the last pixel of column x - 1, 0 at x = 0 -- then over the columns an
//       exclusive sum (the column's first slot in its mask) and an exclusive maximum of the position of the column's last boundary (the
//       position the column's first difference is taken from: positions grow with x, so the maximum is the latest, and 0 -- no boundary
//       yet -- is what the first difference is taken from).
//   (3) rle_offsets_kernel, one workgroup: offsets = the exclusive sum over the masks of (boundaries + 1), 0 for a row past count[b].
//   (4) rle_write_kernel, a lane per column: runs[offsets[n] + slot] = position - previous position for each of its boundaries, and the
//       lane of the last column adds the final run H W - previous.  Every store is guarded by index < capacity.
// The passes meet at kernel boundaries only; there are no atomics and no cursor: the contents are a function of the inputs alone.
#include "pswin_detect_post.hpp"

namespace pswin {
namespace {

constexpr int RLE_THREADS = 256, RLE_OFF_THREADS = 1024;
typedef unsigned long long u64;

struct RleWorkspace {
    size_t planes, colstart, lastpos, totals, total;
    int HW;                                             // 64-row words per column
};

inline RleWorkspace rle_layout(long long N, int H, int W) {
    RleWorkspace w;
    w.HW = (H + 63) / 64;
    const size_t cols = (size_t)N * (size_t)W;
    w.planes = 0;
    w.colstart = w.planes + cols * w.HW * 8;
    w.lastpos = w.colstart + (cols * 4 + 15) / 16 * 16;
    w.totals = w.lastpos + (cols * 4 + 15) / 16 * 16;
    w.total = w.totals + ((size_t)N * 8 + 15) / 16 * 16;
    return w;
}

// mask n is a detection row: rows past the clamped count own no runs and are never read
__device__ inline bool rle_live(const int* __restrict__ count, long long n, int K) {
    return !count || (int)(n % K) < det_clamp(count[n / K], K);
}

// (1a) bitmaps -> planes.  COLS adjacent columns per lane (16: W % 16 == 0 and a 16-byte aligned base; 1: any W); grid (n, column block, w).
// The 16-column form runs one wavefront per workgroup, 1024 columns: a wider block would leave whole wavefronts without a column.
template <int COLS>
constexpr int RLE_PLANES_THREADS = COLS == 16 ? 64 : RLE_THREADS;
template <int COLS>
__global__ __launch_bounds__(RLE_PLANES_THREADS<COLS>) void rle_planes_kernel(const unsigned char* __restrict__ masks, const int* __restrict__ count, int K,
                                                                 int H, int W, int HW, u64* __restrict__ planes) {
    const long long n = blockIdx.x;
    const int x0 = (blockIdx.y * RLE_PLANES_THREADS<COLS> + threadIdx.x) * COLS, w = blockIdx.z;
    if (x0 >= W || !rle_live(count, n, K)) return;
    const int y0 = 64 * w, rows = H - y0 < 64 ? H - y0 : 64;
    const unsigned char* src = masks + ((size_t)n * H + y0) * (size_t)W + x0;
    u64 bits[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) bits[c] = 0ull;
    for (int r = 0; r < rows; ++r) {
        if constexpr (COLS == 16) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(src + (size_t)r * W);
#pragma unroll
            for (int c = 0; c < 16; ++c) bits[c] |= (u64)(((v[c >> 2] >> (8 * (c & 3))) & 0xffu) != 0u) << r;
        } else {
            bits[0] |= (u64)(src[(size_t)r * W] != 0) << r;
        }
    }
    u64* dst = planes + ((size_t)n * HW + w) * (size_t)W + x0;
#pragma unroll
    for (int c = 0; c < COLS; ++c) dst[c] = bits[c];
}

// (1b) the paste's sample -> planes; grid (n = b K + k, column block, w), a lane per column
template <int DT>
__global__ __launch_bounds__(PASTE_THREADS) void rle_paste_planes_kernel(const void* __restrict__ logits, long long sn, long long sc, long long sy,
                                                                         long long sx, const long long* __restrict__ labels,
                                                                         const float* __restrict__ boxes, const int* __restrict__ count, int K,
                                                                         int C, int H, int W, int HW, float thr, u64* __restrict__ planes) {
    __shared__ float prob[PASTE_LD * PASTE_LD];
    const size_t det = blockIdx.x;
    if (!rle_live(count, (long long)det, K)) return;    // the same for the whole workgroup
    const int x = blockIdx.y * PASTE_THREADS + threadIdx.x, w = blockIdx.z;
    const f32x4 box = reinterpret_cast<const f32x4*>(boxes)[det];
    paste_stage<DT>(prob, logits, sn, sc, sy, sx, det, paste_channel(labels[det], C));
    __syncthreads();
    if (x >= W) return;
    const PasteAxis ax = paste_axis(paste_coord((float)x + 0.5f, box[0], box[2]));
    const int y0 = 64 * w, rows = H - y0 < 64 ? H - y0 : 64;
    u64 bits = 0ull;
    for (int r = 0; r < rows; ++r) {
        const PasteAxis ay = paste_axis(paste_coord((float)(y0 + r) + 0.5f, box[1], box[3]));
        const float val = ax.in && ay.in ? paste_value(prob, ax, ay) : 0.f;   // a pixel that samples nothing compares as 0
        bits |= (u64)(val >= thr) << r;
    }
    planes[(det * HW + w) * (size_t)W + x] = bits;
}

// the boundaries of one plane word: bit y set = pixel y differs from its predecessor in scan order
__device__ inline u64 rle_trans(u64 word, u64 carry, int valid) {
    const u64 t = word ^ ((word << 1) | carry);
    return valid >= 64 ? t : t & ((1ull << valid) - 1ull);
}
// the last pixel of column x - 1 (0 before the first column)
__device__ inline u64 rle_join(const u64* __restrict__ mask_planes, int x, int H, int W, int HW) {
    return x > 0 ? (mask_planes[(size_t)(HW - 1) * W + x - 1] >> ((H - 1) & 63)) & 1ull : 0ull;
}

// (2) one workgroup per mask; colstart / lastpos u32 [N][W], totals u64 [N] (boundaries + 1 passes 2^32 for a checkerboard of 2^32 - 1 pixels)
__global__ __launch_bounds__(RLE_THREADS) void rle_scan_kernel(const u64* __restrict__ planes, const int* __restrict__ count, int K, int H, int W,
                                                               int HW, unsigned* __restrict__ colstart, unsigned* __restrict__ lastpos,
                                                               u64* __restrict__ totals) {
    __shared__ unsigned s_sum[RLE_THREADS], s_max[RLE_THREADS];
    const long long n = blockIdx.x;
    const int t = threadIdx.x;
    if (!rle_live(count, n, K)) {
        if (t == 0) totals[n] = 0ull;
        return;
    }
    const u64* mp = planes + (size_t)n * HW * (size_t)W;
    unsigned run_sum = 0u, run_max = 0u;
    for (int base = 0; base < W; base += RLE_THREADS) {
        const int x = base + t;
        unsigned c = 0u, lp = 0u;
        if (x < W) {
            u64 carry = rle_join(mp, x, H, W, HW);
            for (int w = 0; w < HW; ++w) {
                const u64 word = mp[(size_t)w * W + x];
                const u64 tr = rle_trans(word, carry, H - 64 * w);
                carry = word >> 63;
                c += (unsigned)__builtin_popcountll(tr);
                if (tr) lp = (unsigned)x * (unsigned)H + 64u * w + (63u - (unsigned)__builtin_clzll(tr));
            }
        }
        s_sum[t] = c;
        s_max[t] = lp;
        __syncthreads();
        for (int d = 1; d < RLE_THREADS; d <<= 1) {     // inclusive scans of the block's 256 columns
            const unsigned a = t >= d ? s_sum[t - d] : 0u, m = t >= d ? s_max[t - d] : 0u;
            __syncthreads();
            s_sum[t] += a;
            s_max[t] = s_max[t] > m ? s_max[t] : m;
            __syncthreads();
        }
        if (x < W) {
            const unsigned em = t ? s_max[t - 1] : 0u;
            colstart[(size_t)n * W + x] = run_sum + (s_sum[t] - c);
            lastpos[(size_t)n * W + x] = run_max > em ? run_max : em;
        }
        const unsigned bs = s_sum[RLE_THREADS - 1], bm = s_max[RLE_THREADS - 1];
        run_sum += bs;
        run_max = run_max > bm ? run_max : bm;
        __syncthreads();
    }
    if (t == 0) totals[n] = (u64)run_sum + 1ull;              // the boundaries and the final run
}

// (3) offsets i64 [N + 1]: one workgroup walks the masks in chunks of its size
__global__ __launch_bounds__(RLE_OFF_THREADS) void rle_offsets_kernel(const u64* __restrict__ totals, long long N,
                                                                      long long* __restrict__ offsets) {
    __shared__ u64 s[RLE_OFF_THREADS];
    const int t = threadIdx.x;
    u64 run = 0ull;
    for (long long base = 0; base < N; base += RLE_OFF_THREADS) {
        const long long n = base + t;
        const u64 v = n < N ? totals[n] : 0ull;
        s[t] = v;
        __syncthreads();
        for (int d = 1; d < RLE_OFF_THREADS; d <<= 1) {
            const u64 a = t >= d ? s[t - d] : 0ull;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        if (n < N) offsets[n] = (long long)(run + s[t] - v);
        run += s[RLE_OFF_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) offsets[N] = (long long)run;
}

// (4) grid (n, column block), a lane per column
__global__ __launch_bounds__(RLE_THREADS) void rle_write_kernel(const u64* __restrict__ planes, const int* __restrict__ count, int K, int H, int W,
                                                                int HW, const unsigned* __restrict__ colstart,
                                                                const unsigned* __restrict__ lastpos, const long long* __restrict__ offsets,
                                                                unsigned* __restrict__ runs, long long capacity) {
    const long long n = blockIdx.x;
    const int x = blockIdx.y * RLE_THREADS + threadIdx.x;
    if (x >= W || !rle_live(count, n, K)) return;
    const u64* mp = planes + (size_t)n * HW * (size_t)W;
    long long slot = offsets[n] + (long long)colstart[(size_t)n * W + x];
    unsigned prev = lastpos[(size_t)n * W + x];
    u64 carry = rle_join(mp, x, H, W, HW);
    for (int w = 0; w < HW; ++w) {
        const u64 word = mp[(size_t)w * W + x];
        u64 tr = rle_trans(word, carry, H - 64 * w);
        carry = word >> 63;
        const unsigned p0 = (unsigned)x * (unsigned)H + 64u * w;
        while (tr) {
            const unsigned pos = p0 + (unsigned)__builtin_ctzll(tr);
            tr &= tr - 1ull;
            if (slot < capacity) runs[slot] = pos - prev;
            prev = pos;
            ++slot;
        }
    }
    if (x == W - 1 && slot < capacity) runs[slot] = (unsigned)H * (unsigned)W - prev;
}

inline bool rle_shape_ok(long long N, int H, int W) {
    return N >= 1 && N <= 0x7fffffffll && H >= 1 && W >= 1 && H <= 65536 && W <= 65536 && (unsigned long long)H * (unsigned long long)W < (1ull << 32);
}

// passes (2) - (4) over planes that a producer has queued on the stream
inline int rle_from_planes(const int32_t* count, long long N, int K, int H, int W, long long* offsets, uint32_t* runs, long long capacity,
                           void* workspace, hipStream_t st) {
    const RleWorkspace l = rle_layout(N, H, W);
    char* ws = reinterpret_cast<char*>(workspace);
    const u64* planes = reinterpret_cast<const u64*>(ws + l.planes);
    unsigned* colstart = reinterpret_cast<unsigned*>(ws + l.colstart);
    unsigned* lastpos = reinterpret_cast<unsigned*>(ws + l.lastpos);
    u64* totals = reinterpret_cast<u64*>(ws + l.totals);
    hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)N), dim3(RLE_THREADS), 0, st, planes, count, K, H, W, l.HW, colstart, lastpos, totals);
    hipLaunchKernelGGL(rle_offsets_kernel, dim3(1), dim3(RLE_OFF_THREADS), 0, st, totals, N, offsets);
    hipLaunchKernelGGL(rle_write_kernel, dim3((unsigned)N, (W + RLE_THREADS - 1) / RLE_THREADS), dim3(RLE_THREADS), 0, st, planes, count, K, H, W,
                       l.HW, colstart, lastpos, offsets, runs, capacity);
    PSWIN_LAUNCH_RET();
}

inline bool rle_outputs_ok(const long long* offsets, const uint32_t* runs, long long capacity, const void* workspace) {
    return offsets && runs && workspace && capacity >= 1 && (reinterpret_cast<uintptr_t>(offsets) & 7) == 0 &&
           (reinterpret_cast<uintptr_t>(runs) & 3) == 0 && aligned16(workspace);
}

}  // namespace
}  // namespace pswin

using namespace pswin;

extern "C" {

int pswin_rle_workspace(long long N, int H, int W, long long* bytes) {
    PSWIN_CHECK_ARG(bytes && rle_shape_ok(N, H, W));
    *bytes = (long long)rle_layout(N, H, W).total;
    return PSWIN_OK;
}

int pswin_rle_encode(const unsigned char* masks, const int32_t* count, long long N, int K, int H, int W, long long* offsets, uint32_t* runs,
                     long long capacity, void* workspace, void* stream) {
    PSWIN_CHECK_ARG(masks && rle_shape_ok(N, H, W) && rle_outputs_ok(offsets, runs, capacity, workspace));
    PSWIN_CHECK_ARG(!count || (K >= 1 && N % K == 0 && (reinterpret_cast<uintptr_t>(count) & 3) == 0));
    const RleWorkspace l = rle_layout(N, H, W);
    u64* planes = reinterpret_cast<u64*>(reinterpret_cast<char*>(workspace) + l.planes);
    const int Kc = count ? K : 1;
    if ((W & 15) == 0 && aligned16(masks))
        hipLaunchKernelGGL(rle_planes_kernel<16>, dim3((unsigned)N, (W / 16 + 63) / 64, l.HW), dim3(RLE_PLANES_THREADS<16>), 0,
                           (hipStream_t)stream, masks, count, Kc, H, W, l.HW, planes);
    else
        hipLaunchKernelGGL(rle_planes_kernel<1>, dim3((unsigned)N, (W + RLE_THREADS - 1) / RLE_THREADS, l.HW), dim3(RLE_THREADS), 0,
                           (hipStream_t)stream, masks, count, Kc, H, W, l.HW, planes);
    return rle_from_planes(count, N, Kc, H, W, offsets, runs, capacity, workspace, (hipStream_t)stream);
}

int pswin_paste_masks_rle(const void* logits, int dtype, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                          const long long* labels, const float* boxes, const int32_t* count, int B, int K, int C, int H, int W, float thr,
                          long long* offsets, uint32_t* runs, long long capacity, void* workspace, void* stream) {
    PSWIN_CHECK_ARG(logits && labels && boxes && count && valid_dtype(dtype));
    PSWIN_CHECK_ARG(B >= 1 && B <= 65535 && K >= 1 && K <= DET_KMAX && C >= 1 && C <= DET_CMAX);
    const long long N = (long long)B * K;
    PSWIN_CHECK_ARG(rle_shape_ok(N, H, W) && rle_outputs_ok(offsets, runs, capacity, workspace));
    PSWIN_CHECK_ARG(stride_n >= 1 && stride_c >= 1 && stride_y >= 1 && stride_x >= 1);
    PSWIN_CHECK_ARG(aligned16(boxes) && (reinterpret_cast<uintptr_t>(labels) & 7) == 0 && (reinterpret_cast<uintptr_t>(count) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(logits) & (dtype == PSWIN_F32 ? 3 : 1)) == 0);
    const RleWorkspace l = rle_layout(N, H, W);
    u64* planes = reinterpret_cast<u64*>(reinterpret_cast<char*>(workspace) + l.planes);
    const dim3 grid((unsigned)N, (W + PASTE_THREADS - 1) / PASTE_THREADS, l.HW);
    if (dtype == PSWIN_F32)
        hipLaunchKernelGGL(rle_paste_planes_kernel<PSWIN_F32>, grid, dim3(PASTE_THREADS), 0, (hipStream_t)stream, logits, stride_n, stride_c,
                           stride_y, stride_x, labels, boxes, count, K, C, H, W, l.HW, thr, planes);
    else
        hipLaunchKernelGGL(rle_paste_planes_kernel<PSWIN_BF16>, grid, dim3(PASTE_THREADS), 0, (hipStream_t)stream, logits, stride_n, stride_c,
                           stride_y, stride_x, labels, boxes, count, K, C, H, W, l.HW, thr, planes);
    return rle_from_planes(count, N, K, H, W, offsets, runs, capacity, workspace, (hipStream_t)stream);
}

}  // extern "C"
