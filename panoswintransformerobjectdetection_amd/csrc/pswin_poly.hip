// COCO polygon annotations to masks on the device (panoswintransformerobjectdetection_amd/polygons.py states the rule, pycocotools'
// rleFrPoly) -- gfx950 only.  Built into its own library, libpswin_poly_hip.so (include/pswin_poly.h): libpswin_hip.so is not touched.
// Two launches: polygons -> BIT-PLANES in the workspace (word (n, w, x) holds the pixels y = 64 w .. 64 w + 63 of column x of object n,
// bit y & 63, zero past H: the layout of csrc/pswin_rle.hip), then planes -> bytes.  The runs come from pswin_rle_encode on those bytes.
#include "pswin_poly.h"
#include "pswin_detect_post.hpp"

namespace pswin {
namespace {

typedef unsigned long long u64;
constexpr int POLY_EXPAND_THREADS = 256;
template <int COLS>
constexpr int RLE_PLANES_THREADS = COLS == 16 ? 64 : POLY_EXPAND_THREADS;

// object n is read only inside its image's clamped count
__device__ inline bool rle_live(const int* __restrict__ count, long long n, int K) { return (int)(n % K) < det_clamp(count[n / K], K); }

// polygons -> planes (polygons.py states why every
// column holds an even number of events: a column's bits are the prefix XOR, from 0, of that column's events alone).  Grid (object
// n = b K + k, tile of 64 columns), one wavefront; a lane owns column c.  Per part the lanes stage the integer vertices in LDS, a chunk of
// POLY_CHUNK edges at a time, and every lane walks the edges: an edge has an event in column c exactly when min(xs, xe) <= 5 c + 2 and
// 5 c + 3 <= max(xs, xe); the lane toggles the event's row in its own LDS words (a plain XOR: no lane touches another's), fills the column
// by a prefix XOR down the words and ORs the part into the object's plane words, which it alone owns.  The work per edge is a comparison
// for most lanes and at most 24 bisection steps for the others, whatever the coordinates are; offsets are clamped to the buffers, so a
// stale buffer is read inside its bounds and costs no more than its size.
constexpr int POLY_LANES = 64, POLY_CHUNK = 256, POLY_STAGE = 260, POLY_MAX_SIDE = 4096;   // POLY_STAGE ints: >= POLY_CHUNK + 1, 16-byte rows
typedef __attribute__((ext_vector_type(2))) double f64x2;

// int(5 x + 0.5), truncating; |x| <= 2^20 on every checked path, and any other bit pattern (NaN too) lands inside +-2^23
__device__ inline int poly_vertex(double x) {
    double v = 5.0 * x + 0.5;
    if (!(v >= -8388608.0)) v = -8388608.0;
    if (v > 8388608.0) v = 8388608.0;
    return (int)v;
}

// the row yd in [0, H] of the event an edge has between u = u0 and u0 + 1 (the caller has checked that it has one, so dx >= 1)
__device__ inline int poly_event_row(int xs, int ys, int xe, int ye, int u0, int H) {
    const int dx = xe > xs ? xe - xs : xs - xe, dy = ye > ys ? ye - ys : ys - ye;
    int m;                                              // the smaller v of the two points
    if (dx >= dy) {
        if (xs > xe) {
            int t = xs; xs = xe; xe = t;
            t = ys; ys = ye; ye = t;
        }
        const double s = (double)(ye - ys) / (double)dx;
        const int t = u0 - xs;                          // u = xs + t: the points t and t + 1
        const int va = (int)((double)ys + s * (double)t + 0.5), vb = (int)((double)ys + s * (double)(t + 1) + 0.5);
        m = va < vb ? va : vb;
    } else {
        if (ys > ye) {
            int t = xs; xs = xe; xe = t;
            t = ys; ys = ye; ye = t;
        }
        const double s = (double)(xe - xs) / (double)dy;
        const bool up = xe > xs;
        int lo = 0, hi = dy;                            // u(t) = int(xs + s t + 0.5) is monotone: the first t past the boundary, by bisection
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            const int u = (int)((double)xs + s * (double)mid + 0.5);
            if (up ? u > u0 : u <= u0) hi = mid; else lo = mid;
        }
        m = ys + hi - 1;                                // v = ys + t: the points hi - 1 and hi
    }
    double yd = ((double)m + 0.5) / 5.0 - 0.5;
    yd = yd < 0.0 ? 0.0 : (yd > (double)H ? (double)H : yd);
    return (int)ceil(yd);
}

__device__ inline int poly_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(POLY_LANES) void poly_planes_kernel(const double* __restrict__ xy, const int* __restrict__ part_offsets,
                                                                 const int* __restrict__ obj_offsets, const int* __restrict__ count,
                                                                 int max_parts, int max_vertices, int K, int H, int W, int HW,
                                                                 u64* __restrict__ planes) {
    extern __shared__ __attribute__((aligned(16))) char poly_smem[];
    u64* tog = reinterpret_cast<u64*>(poly_smem);                                    // [HW][64]: word w of the lane's column
    int* sX = reinterpret_cast<int*>(poly_smem + (size_t)HW * POLY_LANES * 8);
    int* sY = sX + POLY_STAGE;
    const long long n = blockIdx.x;
    if (!rle_live(count, n, K)) return;                 // the same for the whole workgroup
    const int lane = threadIdx.x, c = blockIdx.y * POLY_LANES + lane, u0 = 5 * c + 2;
    const bool mine = c < W;
    const f64x2* pts = reinterpret_cast<const f64x2*>(xy);
    u64* dst = planes + (size_t)n * HW * (size_t)W + c;
    const int p0 = poly_clamp(obj_offsets[n], 0, max_parts), p1 = poly_clamp(obj_offsets[n + 1], p0, max_parts);
    bool first = true;
    for (int p = p0; p < p1; ++p) {
        const int v0 = poly_clamp(part_offsets[p], 0, max_vertices), k = poly_clamp(part_offsets[p + 1], v0, max_vertices) - v0;
        if (k < 1) continue;
        for (int w = 0; w < HW; ++w) tog[w * POLY_LANES + lane] = 0ull;
        for (int base = 0; base < k; base += POLY_CHUNK) {
            const int ne = k - base < POLY_CHUNK ? k - base : POLY_CHUNK;
            __syncthreads();                            // the previous chunk has been read
            for (int i = lane; i <= ne; i += POLY_LANES) {
                const int idx = base + i == k ? 0 : base + i;                        // X[k] = X[0]
                const f64x2 pt = pts[v0 + idx];
                sX[i] = poly_vertex(pt[0]);
                sY[i] = poly_vertex(pt[1]);
            }
            __syncthreads();
            if (mine) {
                for (int e = 0; e < ne; ++e) {
                    const int xs = sX[e], xe = sX[e + 1];
                    if ((xs < xe ? xs : xe) <= u0 && u0 < (xs < xe ? xe : xs)) {
                        const int yd = poly_event_row(xs, sY[e], xe, sY[e + 1], u0, H);
                        if (yd < H) tog[(yd >> 6) * POLY_LANES + lane] ^= 1ull << (yd & 63);
                    }
                }
            }
        }
        if (mine) {
            u64 carry = 0ull;
            for (int w = 0; w < HW; ++w) {
                u64 x = tog[w * POLY_LANES + lane];
                x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
                if (carry) x = ~x;
                carry = x >> 63;
                const int valid = H - 64 * w;
                if (valid < 64) x &= (1ull << valid) - 1ull;
                dst[(size_t)w * W] = first ? x : (dst[(size_t)w * W] | x);
            }
        }
        first = false;
    }
    if (first && mine)
        for (int w = 0; w < HW; ++w) dst[(size_t)w * W] = 0ull;                      // an object without a part
}

// planes -> bytes: every byte of masks uint8 [N][H][W], zeros for the rows past the count (their planes are not read).  Grid and the two
// forms: 16 adjacent columns per lane with 16-byte stores (one wavefront per workgroup, 1024 columns), or one column per lane.
template <int COLS>
__global__ __launch_bounds__(RLE_PLANES_THREADS<COLS>) void poly_expand_kernel(const u64* __restrict__ planes, const int* __restrict__ count,
                                                                               int K, int H, int W, int HW, unsigned char* __restrict__ masks) {
    const long long n = blockIdx.x;
    const int x0 = (blockIdx.y * RLE_PLANES_THREADS<COLS> + threadIdx.x) * COLS, w = blockIdx.z;
    if (x0 >= W) return;
    const bool live = rle_live(count, n, K);
    const int y0 = 64 * w, rows = H - y0 < 64 ? H - y0 : 64;
    const u64* src = planes + ((size_t)n * HW + w) * (size_t)W + x0;
    u64 bits[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) bits[c] = live ? src[c] : 0ull;
    unsigned char* dst = masks + ((size_t)n * H + y0) * (size_t)W + x0;
    for (int r = 0; r < rows; ++r) {
        if constexpr (COLS == 16) {
            u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < 16; ++c) v[c >> 2] |= (unsigned)((bits[c] >> r) & 1ull) << (8 * (c & 3));
            *reinterpret_cast<u32x4*>(dst + (size_t)r * W) = v;
        } else {
            dst[(size_t)r * W] = (unsigned char)((bits[0] >> r) & 1ull);
        }
    }
}

inline bool poly_shape_ok(int B, int K, int H, int W) {
    return B >= 1 && K >= 1 && (long long)B * K <= 0x7fffffffll && H >= 1 && W >= 1 && H <= POLY_MAX_SIDE && W <= POLY_MAX_SIDE;
}

}  // namespace
}  // namespace pswin

using namespace pswin;

extern "C" {

int pswin_poly_version(void) { return PSWIN_POLY_ABI_VERSION; }

int pswin_poly_workspace(int B, int K, int H, int W, long long* bytes) {
    PSWIN_CHECK_ARG(bytes && poly_shape_ok(B, K, H, W));
    *bytes = (long long)B * K * ((H + 63) / 64) * W * 8;
    return PSWIN_OK;
}

int pswin_poly_masks(const double* xy, const int32_t* part_offsets, const int32_t* obj_offsets, const int32_t* count, int max_parts,
                     int max_vertices, int B, int K, int H, int W, unsigned char* masks, void* workspace, void* stream) {
    PSWIN_CHECK_ARG(xy && part_offsets && obj_offsets && count && masks && workspace && aligned16(xy) && aligned16(workspace));
    PSWIN_CHECK_ARG((reinterpret_cast<uintptr_t>(part_offsets) & 3) == 0 && (reinterpret_cast<uintptr_t>(obj_offsets) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(count) & 3) == 0 && max_parts >= 1 && max_vertices >= 1 && poly_shape_ok(B, K, H, W));
    const long long N = (long long)B * K;
    const int HW = (H + 63) / 64;
    u64* planes = reinterpret_cast<u64*>(workspace);
    const size_t lds = (size_t)HW * POLY_LANES * 8 + 2 * POLY_STAGE * sizeof(int);
    hipLaunchKernelGGL(poly_planes_kernel, dim3((unsigned)N, (W + POLY_LANES - 1) / POLY_LANES), dim3(POLY_LANES), lds, (hipStream_t)stream, xy,
                       part_offsets, obj_offsets, count, max_parts, max_vertices, K, H, W, HW, planes);
    if ((W & 15) == 0 && aligned16(masks))
        hipLaunchKernelGGL(poly_expand_kernel<16>, dim3((unsigned)N, (W / 16 + 63) / 64, HW), dim3(RLE_PLANES_THREADS<16>), 0,
                           (hipStream_t)stream, planes, count, K, H, W, HW, masks);
    else
        hipLaunchKernelGGL(poly_expand_kernel<1>, dim3((unsigned)N, (W + POLY_EXPAND_THREADS - 1) / POLY_EXPAND_THREADS, HW),
                           dim3(POLY_EXPAND_THREADS), 0, (hipStream_t)stream, planes, count, K, H, W, HW, masks);
    PSWIN_LAUNCH_RET();
}

}  // extern "C"
