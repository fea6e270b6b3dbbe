// LayerNorm fused with the PanoSwin row movers (gfx950).
//
// In the reference every block does  norm1 -> cat uv -> roll/flip/cat -> pad -> window_partition  (HOT:503-513,
// 64-75) and PatchMerging does  pad -> 4 strided slices -> cat -> norm  (HOT:563-574): a LayerNorm pass plus 4-7
// full-tensor copies.  Here the normalisation happens inside the indexed row copy: one read of the source rows,
// one write of the normalised rows in their destination layout (window slots / merged tokens), statistics kept
// per source token for the backward pass.  The same kernel with an identity map is the plain LayerNorm used for
// norm2 and the output norms, writing bf16 directly when the consumer is a bf16 GEMM.
// HOT = mmdet/models/backbones/simple_panoswin_transformer.py of the reference.
//
// Mapping: a row of C elements is L lanes x up to 4 chunks of 4 elements (L = 2..64, a power of two, chosen on
// the host so that L * 16 >= C); consecutive lanes read consecutive 16-byte chunks; row reductions are log2(L)
// __shfl_xor steps.  Statistics and all arithmetic are fp32 regardless of the I/O dtype.
// Pinned by tests/test_ln_edges_gpu.py: every output within a float64 bound counted from the roundings below (tests/_ln_cases.py);
// y from the stored statistics, every bf16 store (round to nearest even) and the sums of integer gradients bit for bit.
// Not pinned: the order of the additions inside a row sum, and rsqrtf beyond its documented accuracy.
#include "pswin_common.hpp"

using namespace pswin;

namespace {

constexpr int THREADS = 256;

// Sum over the L lanes of a row (every lane receives it).  Steps inside a 16-lane DPP row run on the VALU
// (v_add_f32 with a DPP modifier, ~5 cycles): __shfl_xor compiles to ds_bpermute_b32, an LDS-crossbar round trip of
// ~100+ cycles each, and the 2 x log2(L) dependent ones per row were a quarter of a LayerNorm backward iteration.
template <int L>
__device__ inline float row_sum(float v) {
    if constexpr (L >= 2) v = dpp_add<0xB1>(v);      // quad_perm [1,0,3,2]: lane ^ 1
    if constexpr (L >= 4) v = dpp_add<0x4E>(v);      // quad_perm [2,3,0,1]: lane ^ 2
    if constexpr (L >= 8) v = dpp_add<0x141>(v);     // row_half_mirror: the other quad of the 8 (quads are uniform by now)
    if constexpr (L >= 16) v = dpp_add<0x140>(v);    // row_mirror: the other half of the 16
    if constexpr (L >= 32) v += __shfl_xor(v, 16);
    if constexpr (L >= 64) v += __shfl_xor(v, 32);
    return v;
}

// ---------------------------------------------------------------------------------------------
// The row math, written once for the generic kernels (any C, up to NCH chunks per lane behind a `ch < nchunks` test) and the exact-row
// kernels below (EXACT: C == 4 * L * NCH, every chunk slot of every lane is in the row).
// ---------------------------------------------------------------------------------------------
template <int L, bool EXACT>
__device__ inline bool in_row(int lane, int k, int nchunks) {
    if constexpr (EXACT) return true;
    else return lane + k * L < nchunks;
}

// mean and 1 / sqrt(var + eps) of the row whose chunks this lane holds in v
template <int L, int NCH, bool EXACT>
__device__ inline void row_stats(const f32x4 (&v)[NCH], int lane, int nchunks, int C, float eps, float& mu, float& rs_) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
        if (in_row<L, EXACT>(lane, k, nchunks)) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    mu = row_sum<L>(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (in_row<L, EXACT>(lane, k, nchunks)) {
            const f32x4 d = v[k] - mu;
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    }
    rs_ = rsqrtf(row_sum<L>(q) / (float)C + eps);
}

__device__ inline f32x4 ln_affine(f32x4 v, float mu, float rs_, f32x4 g4, f32x4 b4) { return (v - mu) * rs_ * g4 + b4; }

// resid + scale_b * (win + bias), the operations and their order those of window_scatter_add_kernel; an absent bias / scale is skipped
// (a select on a uniform flag, not a branch: the operands are already in registers)
__device__ inline f32x4 branch_add(f32x4 w, f32x4 bias4, bool has_bias, float sc, bool has_scale, f32x4 resid4) {
    f32x4 val = has_bias ? w + bias4 : w;
    val = has_scale ? val * sc : val;
    return val + resid4;
}

// backward, one chunk: xhat and dy * gamma, the dgamma / dbeta sums and this lane's share of the two row sums
__device__ inline void bwd_chunk(f32x4 xv, f32x4 dyv, f32x4 g4, float mu, float rs_, f32x4& xh, f32x4& g, f32x4& dg, f32x4& db,
                                 float& s1, float& s2) {
    xh = (xv - mu) * rs_;
    g = dyv * g4;
    dg = dg + dyv * xh;
    db = db + dyv;
    s1 += (g[0] + g[1]) + (g[2] + g[3]);
    s2 += (g[0] * xh[0] + g[1] * xh[1]) + (g[2] * xh[2] + g[3] * xh[3]);
}
__device__ inline f32x4 bwd_dx(f32x4 g, f32x4 xh, float s1, float s2, float rs_) { return (g - s1 - xh * s2) * rs_; }

// ---------------------------------------------------------------------------------------------
// Buffer access of the exact-row kernels: wave-uniform resources, 32-bit byte offsets per lane.  A lane or row that must read zeros
// (pad slot, row past the end, merged quarter outside the image) gets the offset OOB, past every operand the host admits: the load
// returns zeros and a store is dropped, without a branch.  An absent optional operand is a resource of zero bytes.
// ---------------------------------------------------------------------------------------------
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr unsigned OOB = 0xFFFF0000u;              // OOB plus the chunk offsets of a row (< 64 KB) neither wraps nor comes back in range
constexpr unsigned long long MAX_OPERAND_BYTES = 0xFFFF0000ull;

__device__ inline rsrc_t uniform_rsrc(const void* base, unsigned bytes) {
    const unsigned long long v = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                             __builtin_amdgcn_readfirstlane((int)(base ? bytes : 0u)), 0x00020000);
}
template <int DT>
constexpr unsigned ES = (DT == PSWIN_F32) ? 4u : 2u;

// 4 consecutive elements as they lie in memory (what a software pipeline carries from the request to the use: expanding bf16 at the
// request would put the wait for the load right behind it) ...
template <int DT>
using raw4_t = std::conditional_t<DT == PSWIN_F32, f32x4, u32x2>;
// AUX: the cache policy bits of the buffer instruction (0 = default, NT = non-temporal: a stream the kernel reads once)
constexpr int NT = 2;
template <int DT, int AUX = 0>
__device__ inline raw4_t<DT> braw4(rsrc_t r, unsigned boff) {
    if constexpr (DT == PSWIN_F32) return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, boff, 0, AUX));
    else return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, boff, 0, AUX));
}
// ... and as f32 (the bf16 expansion is load4's)
template <int DT>
__device__ inline f32x4 expand4(raw4_t<DT> raw) {
    if constexpr (DT == PSWIN_F32) {
        return raw;
    } else {
        f32x4 v;
        v[0] = __builtin_bit_cast(float, raw[0] << 16);
        v[1] = __builtin_bit_cast(float, raw[0] & 0xffff0000u);
        v[2] = __builtin_bit_cast(float, raw[1] << 16);
        v[3] = __builtin_bit_cast(float, raw[1] & 0xffff0000u);
        return v;
    }
}
template <int DT, int AUX = 0>
__device__ inline f32x4 bload4(rsrc_t r, unsigned boff) { return expand4<DT>(braw4<DT, AUX>(r, boff)); }
template <int DT, int AUX = 0>
__device__ inline void bstore4(rsrc_t r, unsigned boff, f32x4 v) {
    if constexpr (DT == PSWIN_F32) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, boff, 0, AUX);
    } else {
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3])}, r, boff, 0, AUX);
    }
}
__device__ inline unsigned bload_u32(rsrc_t r, unsigned boff) { return __builtin_amdgcn_raw_buffer_load_b32(r, boff, 0, 0); }
__device__ inline float bload_f32(rsrc_t r, unsigned boff) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, boff, 0, 0)); }

// MODE 0: out row (b, slot) <- source token map[slot] (or slot when map == nullptr), -1 = zero row.
// MODE 1: PatchMerging: out row (b, i*W2 + j) <- concat of the 4 tokens (2i+dy, 2j+dx), zeros outside (H, W).
struct RowSrc {
    int mode;
    const int32_t* map;   // MODE 0
    int S, n_out;         // tokens per image, out rows per image
    int H, W, W2;         // MODE 1
};

// source element offset (in elements, within the image) of chunk `ch` of out row r; -1 = zero
template <int MODE>
__device__ inline long long src_offset(const RowSrc& rs, int r, int ch, int C, int mode0_src) {
    if constexpr (MODE == 0) {
        return mode0_src < 0 ? -1 : (long long)mode0_src * C + 4 * ch;
    } else {
        const int cq = C / 4;                 // C is the OUTPUT width (4 * input channels): chunks per quarter = cq / 4
        const int per_q = cq / 4;
        const int k = ch / per_q, within = ch - k * per_q;
        const int i = r / rs.W2, j = r - i * rs.W2;
        const int yy = 2 * i + (k & 1), xx = 2 * j + (k >> 1);
        if (yy >= rs.H || xx >= rs.W) return -1;
        return ((long long)yy * rs.W + xx) * (C / 4) + 4 * within;
    }
}

template <int MODE, int XDT, int YDT, int L, int NCH>
__global__ __launch_bounds__(THREADS) void ln_fwd_kernel(const void* __restrict__ x, RowSrc rs,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps,
                                                         void* __restrict__ y, float* __restrict__ mean,
                                                         float* __restrict__ rstd, long long rows, int C,
                                                         const float* __restrict__ add) {
    constexpr int RPB = THREADS / L;
    const int lane = threadIdx.x % L;
    const long long row = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (row >= rows) return;
    const int b = (int)(row / rs.n_out);
    const int r = (int)(row - (long long)b * rs.n_out);
    const int nchunks = C / 4;
    const size_t img_in = (size_t)b * rs.S * (MODE == 0 ? C : C / 4);
    int src0 = 0;
    if constexpr (MODE == 0) src0 = rs.map ? rs.map[r] : r;
    f32x4 v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ch < nchunks) {
            const long long off = src_offset<MODE>(rs, r, ch, C, src0);
            if (off >= 0) v[k] = load4<XDT>(x, img_in + (size_t)off);
        }
    }
    if (MODE == 0 && src0 < 0) {            // zero (padding) slot: stays zero, as F.pad after norm1 does (HOT:504-512)
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int ch = lane + k * L;
            if (ch < nchunks) store4<YDT>(y, (size_t)row * C + 4 * (size_t)ch, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    float mu, rs_;
    row_stats<L, NCH, false>(v, lane, nchunks, C, eps, mu, rs_);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        if (ch < nchunks) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + 4 * ch);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(beta + 4 * ch);
            f32x4 o = ln_affine(v[k], mu, rs_, g4, b4);
            // add: one more f32 row per output row of an image ([n_out, C]: the absolute position encoding, HOT:932-934, added to the
            // normalised patch embedding while it is in registers instead of by a pass over the residual stream)
            if (add) o = o + *reinterpret_cast<const f32x4*>(add + (size_t)r * C + 4 * (size_t)ch);
            store4<YDT>(y, (size_t)row * C + 4 * (size_t)ch, o);
        }
    }
    if (lane == 0) {
        // statistics live at the SOURCE token for MODE 0 (the backward pass walks tokens), at the out row for MODE 1
        const size_t at = (MODE == 0) ? (size_t)b * rs.S + src0 : (size_t)row;
        mean[at] = mu;
        rstd[at] = rs_;
    }
}

// The exact-row form of ln_fwd_kernel (C == 12 * L, rows and operands within 32-bit offsets): the source index, gamma, beta and the
// added row are requested first, then the three chunks of the source row; a zero slot (MODE 0) or a quarter outside the image (MODE 1)
// reads zeros through the offset OOB instead of branching round the load.  MODE 1 needs L % 4 == 0 (whole chunks per quarter).
template <int MODE, int XDT, int YDT, int L>
__global__ __launch_bounds__(THREADS) void ln_fwd_rows_kernel(const void* __restrict__ x, RowSrc rs, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, void* __restrict__ y,
                                                              float* __restrict__ mean, float* __restrict__ rstd, unsigned rows,
                                                              unsigned B, const float* __restrict__ add) {
    constexpr int NCH = 3, C = 4 * L * NCH, RPB = THREADS / L;
    constexpr unsigned CIN = (MODE == 0) ? C : C / 4;            // width of a source token
    const unsigned lane = threadIdx.x % L;
    const unsigned row = blockIdx.x * RPB + threadIdx.x / L;
    if (row >= rows) return;
    const unsigned n_out = (unsigned)rs.n_out, S = (unsigned)rs.S;
    const unsigned b = row / n_out, r = row - b * n_out;
    const bool has_map = rs.map != nullptr, has_add = add != nullptr;
    int src0 = 0;
    if constexpr (MODE == 0) src0 = (int)bload_u32(uniform_rsrc(rs.map, n_out * 4u), r * 4u);
    const rsrc_t gr = uniform_rsrc(gamma, C * 4u), br = uniform_rsrc(beta, C * 4u), ar = uniform_rsrc(add, n_out * (C * 4u));
    const rsrc_t xr = uniform_rsrc(x, B * S * (CIN * ES<XDT>)), yr = uniform_rsrc(y, rows * (C * ES<YDT>));
    f32x4 g4[NCH], b4[NCH], a4[NCH], v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const unsigned cb = (lane + k * L) * 16u;
        g4[k] = bload4<PSWIN_F32>(gr, cb);
        b4[k] = bload4<PSWIN_F32>(br, cb);
        a4[k] = bload4<PSWIN_F32>(ar, r * (C * 4u) + cb);
    }
    if constexpr (MODE == 0) {
        if (!has_map) src0 = (int)r;
#pragma unroll
        for (int k = 0; k < NCH; ++k)
            v[k] = bload4<XDT>(xr, src0 < 0 ? OOB : (b * S + (unsigned)src0) * (C * ES<XDT>) + (lane + k * L) * (4 * ES<XDT>));
    } else {
        constexpr unsigned PER_Q = 3 * L / 4;                    // chunks per quarter
        const unsigned W2 = (unsigned)rs.W2, i = r / W2, j = r - i * W2;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const unsigned ch = lane + k * L, kq = ch / PER_Q, within = ch - kq * PER_Q;
            const unsigned yy = 2 * i + (kq & 1), xx = 2 * j + (kq >> 1);
            const bool inside = (yy < (unsigned)rs.H) & (xx < (unsigned)rs.W);
            v[k] = bload4<XDT>(xr, inside ? ((b * S + yy * (unsigned)rs.W + xx) * CIN + 4 * within) * ES<XDT> : OOB);
        }
    }
    const bool zero_row = MODE == 0 && src0 < 0;                 // padding slot: stays zero, as F.pad after norm1 does (HOT:504-512)
    float mu, rs_;
    row_stats<L, NCH, true>(v, lane, NCH * L, C, eps, mu, rs_);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        f32x4 o = ln_affine(v[k], mu, rs_, g4[k], b4[k]);
        o = has_add ? o + a4[k] : o;
        o = zero_row ? f32x4{0.f, 0.f, 0.f, 0.f} : o;
        bstore4<YDT>(yr, row * (C * ES<YDT>) + (lane + k * L) * (4 * ES<YDT>), o);
    }
    if (lane == 0 && !zero_row) {
        const unsigned at = (MODE == 0) ? b * S + (unsigned)src0 : row;
        mean[at] = mu;
        rstd[at] = rs_;
    }
}

// optional destination map of ln_add_fwd_kernel's normalised rows: token t of image b -> y row b * n_out + map[t]; pads = the slots of an
// image no token maps to (zero rows).  map == nullptr: token order (row = b * S + t).
struct OutMap {
    const int32_t* map;
    const int32_t* pads;
    int n_out, n_pads, B;
};
// optional second output of ln_bwd_kernel (MODE 0): ex[b][map ? map[t] : t] = bf16(scale[b] * dx[b][t]), zero rows at the pad slots --
// the window gather (or plain cast) that turns the residual-stream gradient into the branch gradient the next backward kernel reads
// (window_scatter_add's backward), written while dx is in registers instead of by a pass of its own
struct BwdExtra {
    void* ex;
    const int32_t* map;
    const float* scale;
    const int32_t* pads;
    int n_rows, n_pads, B;
};

// window_scatter_add + LayerNorm in token order, one pass (the attention half of a block ends with
// x1 = x + DropPath(window_reverse(proj(.)) + b) and norm2(x1) follows at once, HOT:516-536):
//   x1[b][t] = resid[b][t] + scale[b] * (win[b][inv[t]] + bias);   y[b][t] = LN(x1[b][t]) * gamma + beta
// x1 is written for the shortcut and the backward pass, but not read back by a separate LayerNorm kernel.  The
// arithmetic (and its order) is that of window_scatter_add_kernel followed by ln_fwd_kernel: bitwise the same result.
template <int WDT, int YDT, int L, int NCH>
__global__ __launch_bounds__(THREADS) void ln_add_fwd_kernel(const void* __restrict__ win, const int32_t* __restrict__ inv,
                                                             const float* __restrict__ resid, const float* __restrict__ scale,
                                                             const float* __restrict__ bias, float* __restrict__ x1,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float eps, void* __restrict__ y, float* __restrict__ mean,
                                                             float* __restrict__ rstd, long long rows, int S, int n_slots,
                                                             int C, OutMap om) {
    constexpr int RPB = THREADS / L;
    const int lane = threadIdx.x % L;
    const long long row = (long long)blockIdx.x * RPB + threadIdx.x / L;
    const int nchunks = C / 4;
    if (row >= rows) {
        // round 4: y may be written through a token -> slot map (the norm1 + shift + pad + partition of the NEXT block fused into the
        // residual add that ends this one); the slots no token maps to are zero rows, written by the row groups behind the last token
        const long long p = row - rows;
        if (om.map && p < (long long)om.n_pads * om.B) {
            const int b = (int)(p / om.n_pads);
            const size_t yrow = (size_t)b * om.n_out + om.pads[p - (long long)b * om.n_pads];
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const int ch = lane + k * L;
                if (ch < nchunks) store4<YDT>(y, yrow * C + 4 * (size_t)ch, f32x4{0.f, 0.f, 0.f, 0.f});
            }
        }
        return;
    }
    const int b = (int)(row / S);
    const int t = (int)(row - (long long)b * S);
    const size_t yrow = om.map ? (size_t)b * om.n_out + om.map[t] : (size_t)row;
    const size_t wrow = ((size_t)b * n_slots + (inv ? inv[t] : t)) * C;
    const float sc = scale ? scale[b] : 1.0f;
    f32x4 v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ch < nchunks) {
            const f32x4 w = load4<WDT>(win, wrow + 4 * (size_t)ch);
            f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
            if (bias) b4 = *reinterpret_cast<const f32x4*>(bias + 4 * (size_t)ch);
            v[k] = branch_add(w, b4, bias != nullptr, sc, scale != nullptr,
                              *reinterpret_cast<const f32x4*>(resid + (size_t)row * C + 4 * (size_t)ch));
            *reinterpret_cast<f32x4*>(x1 + (size_t)row * C + 4 * (size_t)ch) = v[k];
        }
    }
    float mu, rs_;
    row_stats<L, NCH, false>(v, lane, nchunks, C, eps, mu, rs_);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        if (ch < nchunks) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + 4 * ch);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(beta + 4 * ch);
            store4<YDT>(y, yrow * C + 4 * (size_t)ch, ln_affine(v[k], mu, rs_, g4, b4));
        }
    }
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs_;
    }
}

// The exact-row form of ln_add_fwd_kernel (C == 12 * L: the model's widths 96, 192, 384, 768): no chunk test, no branch around a load.
// A thread asks for its indices and the operands that do not depend on them (gamma, beta, bias, the shortcut row) in one burst, then for
// the window row the index names, and consumes nothing before the last request is out.  Same arithmetic (row_stats, ln_affine,
// branch_add) on the same lane <-> chunk mapping: bitwise the results of the generic kernel.
template <int WDT, int YDT, int L>
__global__ __launch_bounds__(THREADS) void ln_add_fwd_rows_kernel(const void* __restrict__ win, const int32_t* __restrict__ inv,
                                                                  const float* __restrict__ resid, const float* __restrict__ scale,
                                                                  const float* __restrict__ bias, float* __restrict__ x1,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  float eps, void* __restrict__ y, float* __restrict__ mean,
                                                                  float* __restrict__ rstd, unsigned rows, unsigned S, unsigned n_slots,
                                                                  OutMap om) {
    constexpr int NCH = 3, C = 4 * L * NCH, RPB = THREADS / L;
    const unsigned lane = threadIdx.x % L;
    const unsigned row = blockIdx.x * RPB + threadIdx.x / L;
    const unsigned B = (unsigned)om.B;
    const rsrc_t yr = uniform_rsrc(y, B * (unsigned)om.n_out * (C * ES<YDT>));
    if (row >= rows) {                       // the zero slots of the output map (see ln_add_fwd_kernel)
        const unsigned p = row - rows, np = (unsigned)om.n_pads;
        if (om.map && p < np * B) {
            const unsigned b = p / np;
            const unsigned yrow = b * (unsigned)om.n_out + (unsigned)om.pads[p - b * np];
#pragma unroll
            for (int k = 0; k < NCH; ++k) bstore4<YDT>(yr, yrow * (C * ES<YDT>) + (lane + k * L) * (4 * ES<YDT>), f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    const unsigned b = row / S, t = row - b * S;
    const bool has_map = om.map != nullptr, has_inv = inv != nullptr, has_scale = scale != nullptr, has_bias = bias != nullptr;
    // request burst 1: the indices, then what needs no index
    const unsigned mt = bload_u32(uniform_rsrc(om.map, S * 4u), t * 4u);
    const unsigned it = bload_u32(uniform_rsrc(inv, S * 4u), t * 4u);
    const float scv = bload_f32(uniform_rsrc(scale, B * 4u), b * 4u);
    const rsrc_t gr = uniform_rsrc(gamma, C * 4u), br = uniform_rsrc(beta, C * 4u), bir = uniform_rsrc(bias, C * 4u);
    const rsrc_t rr = uniform_rsrc(resid, rows * (C * 4u)), x1r = uniform_rsrc(x1, rows * (C * 4u));
    const rsrc_t wr = uniform_rsrc(win, B * n_slots * (C * ES<WDT>));
    f32x4 g4[NCH], b4[NCH], bi[NCH], rv[NCH], w[NCH], v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const unsigned cb = (lane + k * L) * 16u;
        g4[k] = bload4<PSWIN_F32>(gr, cb);
        b4[k] = bload4<PSWIN_F32>(br, cb);
        bi[k] = bload4<PSWIN_F32>(bir, cb);
        rv[k] = bload4<PSWIN_F32>(rr, row * (C * 4u) + cb);
    }
    // burst 2: the window row
    const unsigned wrow = (b * n_slots + (has_inv ? it : t)) * (C * ES<WDT>);
#pragma unroll
    for (int k = 0; k < NCH; ++k) w[k] = bload4<WDT>(wr, wrow + (lane + k * L) * (4 * ES<WDT>));
    const float sc = has_scale ? scv : 1.0f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) v[k] = branch_add(w[k], bi[k], has_bias, sc, has_scale, rv[k]);
#pragma unroll
    for (int k = 0; k < NCH; ++k) bstore4<PSWIN_F32>(x1r, row * (C * 4u) + (lane + k * L) * 16u, v[k]);
    float mu, rs_;
    row_stats<L, NCH, true>(v, lane, NCH * L, C, eps, mu, rs_);
    const unsigned yrow = has_map ? b * (unsigned)om.n_out + mt : row;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
        bstore4<YDT>(yr, yrow * (C * ES<YDT>) + (lane + k * L) * (4 * ES<YDT>), ln_affine(v[k], mu, rs_, g4[k], b4[k]));
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs_;
    }
}

// the ends of the backward kernels (defined behind ln_bwd_kernel)
template <int L, int NCH>
__device__ inline void bwd_zero_pads(const BwdExtra& ex, int lane, int rsub, int nchunks, int C);
template <int L, int NCH, bool RSUM>
__device__ inline void bwd_partials(float (&red)[2][THREADS * 4], const f32x4 (&dg)[NCH], const f32x4 (&db)[NCH],
                                    const f32x4 (&dr)[RSUM ? NCH : 1], float* __restrict__ part, int lane, int rsub, int nchunks, int C);

// Backward.  MODE 0 walks source tokens (b, t): dy row = dy[b][inv ? inv[t] : t].  MODE 1 walks merged rows and
// scatters the 4 quarters of dx back to their tokens.  dgamma / dbeta: per-block partial sums, fixed order.
// RSUM: also accumulate sum_rows res_scale[b] * dres[row] (the bias gradient of the Linear whose output, plus bias, was
// added onto the residual stream through the shortcut this LayerNorm's input came along): third partial segment.
template <int MODE, int DYDT, int XDT, int L, int NCH, bool RSUM, bool EX = false>
__global__ __launch_bounds__(THREADS, (EX && NCH == 3) ? 4 : 1) void ln_bwd_kernel(const void* __restrict__ dy, const int32_t* __restrict__ inv,
                                                         const void* __restrict__ x, RowSrc rs,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, void* __restrict__ dx,
                                                         const float* __restrict__ dres,
                                                         const float* __restrict__ res_scale, float* __restrict__ part,
                                                         long long rows, int C, BwdExtra ex = BwdExtra{}) {
    constexpr int RPB = THREADS / L;
    __shared__ alignas(16) float red[2][THREADS * 4];      // [row group][lane][4 elements] of one chunk column at a time
    const int lane = threadIdx.x % L;
    const int rsub = threadIdx.x / L;
    const int nchunks = C / 4;
    const int n_in = (MODE == 0) ? rs.S : rs.n_out;        // rows walked per image
    f32x4 dg[NCH], db[NCH], dr[RSUM ? NCH : 1];
#pragma unroll
    for (int k = 0; k < NCH; ++k) dg[k] = db[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < (RSUM ? NCH : 1); ++k) dr[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long row = (long long)blockIdx.x * RPB + rsub; row < rows; row += (long long)gridDim.x * RPB) {
        const int b = (int)(row / n_in);
        const int r = (int)(row - (long long)b * n_in);
        size_t dy_row;
        if constexpr (MODE == 0) dy_row = (size_t)b * rs.n_out + (inv ? inv[r] : r);
        else dy_row = (size_t)row;
        const size_t img_in = (size_t)b * rs.S * (MODE == 0 ? C : C / 4);
        const float mu = mean[row], rs_ = rstd[row];
        const float rsc = (RSUM && res_scale) ? res_scale[b] : 1.0f;
        [[maybe_unused]] unsigned ex_row = 0;                    // element offset of the extra output's row (the launcher checks < 2^31 elements)
        [[maybe_unused]] float ex_sc = 1.0f;
        if constexpr (EX) {
            ex_row = ((unsigned)b * (unsigned)ex.n_rows + (unsigned)(ex.map ? ex.map[r] : r)) * (unsigned)C;
            ex_sc = ex.scale ? ex.scale[b] : 1.0f;
        }
        f32x4 xh[NCH], g[NCH], rv[NCH];
        long long offs[NCH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int ch = lane + k * L;
            xh[k] = g[k] = rv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            offs[k] = -1;
            if (ch < nchunks) {
                offs[k] = src_offset<MODE>(rs, r, ch, C, r);
                f32x4 xv = {0.f, 0.f, 0.f, 0.f};
                if (offs[k] >= 0) {
                    xv = load4<XDT>(x, img_in + (size_t)offs[k]);
                    // the shortcut gradient is requested together with the other two streams (it is only needed
                    // after the row reductions; loading it there exposed its latency)
                    if (dres) rv[k] = *reinterpret_cast<const f32x4*>(dres + img_in + (size_t)offs[k]);
                }
                const f32x4 dyv = load4<DYDT>(dy, dy_row * C + 4 * (size_t)ch);
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + 4 * ch);
                bwd_chunk(xv, dyv, g4, mu, rs_, xh[k], g[k], dg[k], db[k], s1, s2);
            }
        }
        s1 = row_sum<L>(s1) / (float)C;
        s2 = row_sum<L>(s2) / (float)C;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int ch = lane + k * L;
            if (ch < nchunks && offs[k] >= 0) {
                f32x4 v = bwd_dx(g[k], xh[k], s1, s2, rs_);
                // the gradient that reaches x along the residual shortcut, added here instead of in a separate pass
                if (dres) {
                    v = v + rv[k];
                    if constexpr (RSUM) dr[k] = dr[k] + rv[k] * rsc;
                }
                store4<XDT>(dx, img_in + (size_t)offs[k], v);
                if constexpr (EX) store4<PSWIN_BF16>(ex.ex, ex_row + 4u * (unsigned)ch, v * ex_sc);
            }
        }
    }
    if constexpr (EX) bwd_zero_pads<L, NCH>(ex, lane, rsub, nchunks, C);
    bwd_partials<L, NCH, RSUM>(red, dg, db, dr, part, lane, rsub, nchunks, C);
}

// the slots of the extra output no token maps to: zero rows (what the separate window gather writes there)
template <int L, int NCH>
__device__ inline void bwd_zero_pads(const BwdExtra& ex, int lane, int rsub, int nchunks, int C) {
    constexpr int RPB = THREADS / L;
    const long long npad = (long long)ex.n_pads * ex.B;
    for (long long p = (long long)blockIdx.x * RPB + rsub; p < npad; p += (long long)gridDim.x * RPB) {
        const int b = (int)(p / ex.n_pads);
        const size_t er = (size_t)b * ex.n_rows + ex.pads[p - (long long)b * ex.n_pads];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int ch = lane + k * L;
            if (ch < nchunks) store4<PSWIN_BF16>(ex.ex, er * C + 4 * (size_t)ch, f32x4{0.f, 0.f, 0.f, 0.f});
        }
    }
}

// block reduction of dgamma / dbeta (and the shortcut sums) over the RPB row groups (fixed order), then one partial row per block
template <int L, int NCH, bool RSUM>
__device__ inline void bwd_partials(float (&red)[2][THREADS * 4], const f32x4 (&dg)[NCH], const f32x4 (&db)[NCH],
                                    const f32x4 (&dr)[RSUM ? NCH : 1], float* __restrict__ part, int lane, int rsub, int nchunks, int C) {
    constexpr int RPB = THREADS / L;
    constexpr int NSEG = RSUM ? 3 : 2;
    float* outp = part + (size_t)blockIdx.x * NSEG * C;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        __syncthreads();
        if (ch < nchunks) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                red[0][(rsub * L + lane) * 4 + e] = dg[k][e];
                red[1][(rsub * L + lane) * 4 + e] = db[k][e];
            }
        }
        __syncthreads();
        if (rsub == 0 && ch < nchunks) {            // the four elements of a chunk side by side (one 16-byte LDS read each), every sum in row-group order
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int q = 0; q < RPB; ++q) {
                a = a + *reinterpret_cast<const f32x4*>(&red[0][(q * L + lane) * 4]);
                c = c + *reinterpret_cast<const f32x4*>(&red[1][(q * L + lane) * 4]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                outp[4 * ch + e] = a[e];
                outp[C + 4 * ch + e] = c[e];
            }
        }
        if constexpr (RSUM) {
            __syncthreads();
            if (ch < nchunks) {
#pragma unroll
                for (int e = 0; e < 4; ++e) red[0][(rsub * L + lane) * 4 + e] = dr[k][e];
            }
            __syncthreads();
            if (rsub == 0 && ch < nchunks) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int q = 0; q < RPB; ++q) a = a + *reinterpret_cast<const f32x4*>(&red[0][(q * L + lane) * 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) outp[2 * C + 4 * ch + e] = a[e];
            }
        }
    }
}

// The exact-row form of ln_bwd_kernel, MODE 0, fp32 x (C == 12 * L): the same persistent grid, partial rows and arithmetic, as a
// software pipeline one row deep.  When dx of row i is in registers, the operands of row i + 1 (x, dres, dy, mean, rstd, the scales)
// are requested -- before row i's stores, which the single in-order counter would otherwise put in front of them -- and inv[] of row
// i + 2 behind them.  A prefetch past the last row reads zeros through OOB.  x, dres and dy are read once and carry the non-temporal
// policy; dx and the extra output are read by the next kernel and keep the default one.
struct BwdRow {               // what a row needs besides its chunks: requested with them
    unsigned em;                // ex.map[r]
    float mu, rs_, rsc, exsc;
};
template <int DYDT, int L, bool RSUM, bool EX>
__global__ __launch_bounds__(THREADS, 4) void ln_bwd_rows_kernel(const void* __restrict__ dy, const int32_t* __restrict__ inv,
                                                                 const float* __restrict__ x, RowSrc rs, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 float* __restrict__ dx, const float* __restrict__ dres,
                                                                 const float* __restrict__ res_scale, float* __restrict__ part,
                                                                 unsigned rows, unsigned B, BwdExtra ex) {
    constexpr int NCH = 3, C = 4 * L * NCH, RPB = THREADS / L;
    __shared__ alignas(16) float red[2][THREADS * 4];
    const unsigned lane = threadIdx.x % L, rsub = threadIdx.x / L;
    const unsigned S = (unsigned)rs.S, n_out = (unsigned)rs.n_out, n_ex = (unsigned)ex.n_rows;
    const bool has_inv = inv != nullptr, has_dres = dres != nullptr, has_rsc = RSUM && res_scale != nullptr;
    const bool has_em = EX && ex.map != nullptr, has_exsc = EX && ex.scale != nullptr;
    const rsrc_t invr = uniform_rsrc(inv, S * 4u), emr = uniform_rsrc(EX ? ex.map : nullptr, S * 4u);
    const rsrc_t meanr = uniform_rsrc(mean, rows * 4u), rstdr = uniform_rsrc(rstd, rows * 4u);
    const rsrc_t rscr = uniform_rsrc(RSUM ? res_scale : nullptr, B * 4u), exscr = uniform_rsrc(EX ? ex.scale : nullptr, B * 4u);
    const rsrc_t xr = uniform_rsrc(x, rows * (C * 4u)), drr = uniform_rsrc(dres, rows * (C * 4u)), dxr = uniform_rsrc(dx, rows * (C * 4u));
    const rsrc_t dyr = uniform_rsrc(dy, B * n_out * (C * ES<DYDT>));
    const rsrc_t exr = uniform_rsrc(EX ? ex.ex : nullptr, B * n_ex * (C * 2u));
    // gamma: fetched once per block into LDS and read from there for every row -- 12 registers that the request for the next row needs
    __shared__ f32x4 gam[NCH * L];
    if (threadIdx.x < NCH * L) gam[threadIdx.x] = bload4<PSWIN_F32>(uniform_rsrc(gamma, C * 4u), threadIdx.x * 16u);
    __syncthreads();
    f32x4 dg[NCH], db[NCH], dr[RSUM ? NCH : 1];
#pragma unroll
    for (int k = 0; k < NCH; ++k) dg[k] = db[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < (RSUM ? NCH : 1); ++k) dr[k] = f32x4{0.f, 0.f, 0.f, 0.f};

    // The loop is uniform over the block: trip j covers the rows j0 .. j0 + RPB - 1, image and token of j0 come from one scalar
    // division, and a row past the end takes part with zeros for operands (OOB) and dropped stores -- it adds nothing to the sums.
    // S >= RPB (host), so a block's rows lie in at most two images.
    struct Pos {
        unsigned row, b, r;
        bool ok;
    };
    const unsigned step = gridDim.x * RPB;
    auto pos_of = [&](unsigned row0) {
        const unsigned b0 = row0 / S, r0 = row0 - b0 * S + rsub;
        const bool wrap = r0 >= S;
        return Pos{row0 + rsub, wrap ? b0 + 1 : b0, wrap ? r0 - S : r0, row0 + rsub < rows};
    };
    // inv[r], the one index an address of the chunk requests depends on: asked for two trips ahead
    auto fetch_idx = [&](const Pos& p) { return bload_u32(invr, p.ok ? p.r * 4u : OOB); };
    auto fetch_row = [&](const Pos& p, unsigned iv, BwdRow& i, f32x4 (&xv)[NCH], f32x4 (&rv)[NCH], raw4_t<DYDT> (&dyv)[NCH]) {
        const unsigned ro = p.ok ? p.r * 4u : OOB, bo = p.ok ? p.b * 4u : OOB, wo = p.ok ? p.row * 4u : OOB;
        i.em = bload_u32(emr, ro);
        i.mu = bload_f32(meanr, wo);
        i.rs_ = bload_f32(rstdr, wo);
        i.rsc = bload_f32(rscr, bo);
        i.exsc = bload_f32(exscr, bo);
        const unsigned xo = p.ok ? p.row * (C * 4u) + lane * 16u : OOB;
        const unsigned dyo = p.ok ? (p.b * n_out + (has_inv ? iv : p.r)) * (C * ES<DYDT>) + lane * (4 * ES<DYDT>) : OOB;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {             // OOB + the chunk offsets stays past every operand
            xv[k] = bload4<PSWIN_F32, NT>(xr, xo + k * L * 16u);
            rv[k] = bload4<PSWIN_F32, NT>(drr, xo + k * L * 16u);
            dyv[k] = braw4<DYDT, NT>(dyr, dyo + k * L * (4 * ES<DYDT>));
        }
    };

    unsigned row0 = blockIdx.x * RPB;
    Pos pc = pos_of(row0), pn = pos_of(row0 + step);
    BwdRow cur;
    f32x4 xv[NCH], rv[NCH];
    raw4_t<DYDT> dyv[NCH];
    const unsigned iv_first = fetch_idx(pc);
    __builtin_amdgcn_sched_barrier(0);
    fetch_row(pc, iv_first, cur, xv, rv, dyv);
    unsigned iv_next = fetch_idx(pn);
    __builtin_amdgcn_sched_barrier(0);
    // one trip: the math of the row in registers, the request for the next one, the stores
    auto trip = [&](unsigned row0) {
        const float mu = cur.mu, rs_ = cur.rs_;
        f32x4 xh[NCH], g[NCH], rc[NCH];
        float s1 = 0.f, s2 = 0.f;
        unsigned gl = lane;
        asm volatile("" : "+v"(gl));                // read per row: hoisted out of the loop the values would live in registers again
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            bwd_chunk(xv[k], expand4<DYDT>(dyv[k]), gam[gl + k * L], mu, rs_, xh[k], g[k], dg[k], db[k], s1, s2);
            rc[k] = rv[k];
        }
        s1 = row_sum<L>(s1) / (float)C;
        s2 = row_sum<L>(s2) / (float)C;
        const float rsc = has_rsc ? cur.rsc : 1.0f;
        const unsigned dx_off = pc.ok ? pc.row * (C * 4u) + lane * 16u : OOB;
        [[maybe_unused]] const unsigned ex_off = pc.ok ? (pc.b * n_ex + (has_em ? cur.em : pc.r)) * (C * 2u) + lane * 8u : OOB;
        [[maybe_unused]] const float ex_sc = has_exsc ? cur.exsc : 1.0f;
        f32x4 v[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            v[k] = bwd_dx(g[k], xh[k], s1, s2, rs_);
            v[k] = has_dres ? v[k] + rc[k] : v[k];
            if constexpr (RSUM) dr[k] = has_dres ? dr[k] + rc[k] * rsc : dr[k];
        }
        // the next trip's operands and the index of the one after it, ahead of this trip's stores (only dx is live here: the request
        // for a whole row fits in the registers the row's operands have just left)
        __builtin_amdgcn_sched_barrier(0);          // not earlier: hoisted above the row math, the request no longer fits in 128 VGPRs
        fetch_row(pn, iv_next, cur, xv, rv, dyv);
        pc = pn;
        pn = pos_of(row0 + 2 * step);
        iv_next = fetch_idx(pn);
        __builtin_amdgcn_sched_barrier(0);          // and not later: behind the stores it would wait for them
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            bstore4<PSWIN_F32>(dxr, dx_off + k * L * 16u, v[k]);
            if constexpr (EX) bstore4<PSWIN_BF16>(exr, ex_off + k * L * 8u, v[k] * ex_sc);
        }
    };
    // Dropped stores (OOB), as many as a trip makes, and a loop that is entered without a test (a workgroup owns at least one trip): both
    // edges then reach the loop header with the same requests outstanding -- the next row, the index behind it, a row's stores -- and
    // the first waits of a trip are counted ones that leave the previous row's stores in flight.  With a test in front of the loop the
    // compiler moves the first request behind it and behind these stores, and the header wait drains everything again.
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        bstore4<PSWIN_F32>(dxr, OOB + k * L * 16u, f32x4{0.f, 0.f, 0.f, 0.f});
        if constexpr (EX) bstore4<PSWIN_BF16>(exr, OOB + k * L * 8u, f32x4{0.f, 0.f, 0.f, 0.f});
    }
    __builtin_amdgcn_sched_barrier(0);
    do {
        trip(row0);
        row0 += step;
    } while (row0 < rows);
    unsigned le = lane, re = rsub;
    asm volatile("" : "+v"(le), "+v"(re));          // the addresses of the ends are worked out here, not carried through the loop
    if constexpr (EX) bwd_zero_pads<L, NCH>(ex, (int)le, (int)re, NCH * L, C);
    bwd_partials<L, NCH, RSUM>(red, dg, db, dr, part, (int)le, (int)re, NCH * L, C);
}

// ---------------------------------------------------------------------------------------------
// Output norms (HOT:975-977: norm{i}(x_out) -> view(B, H, W, C) -> permute(0, 3, 1, 2).contiguous()):
// LayerNorm written directly in NCHW.  A block normalises RPB = THREADS / L consecutive tokens, parks the result in an
// LDS tile and writes it out channel-major, RPB * 4 bytes contiguous per channel, instead of a token-major store plus a
// separate strided transpose pass over the (largest) output tensor; the backward kernel reads the NCHW gradient the
// same way.  fp32 in, fp32 out; S % RPB == 0 (the host falls back to LN + copy otherwise).
// ---------------------------------------------------------------------------------------------
template <int L, int NCH>
__global__ __launch_bounds__(THREADS) void ln_nchw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps,
                                                              float* __restrict__ y, float* __restrict__ mean,
                                                              float* __restrict__ rstd, int S, int C,
                                                              const unsigned short* __restrict__ win, const float* __restrict__ scale,
                                                              const float* __restrict__ bias, float* __restrict__ x1) {
    constexpr int RPB = THREADS / L;
    extern __shared__ float tile[];                 // [C][RPB + 1]
    const int lane = threadIdx.x % L, rsub = threadIdx.x / L;
    const long long row = (long long)blockIdx.x * RPB + rsub;       // grid covers B * S exactly
    const int nchunks = C / 4;
    // win != nullptr (round 4): the rows are x1 = x + scale_b * (win + bias) -- the residual add that closes a stage (x: the shortcut,
    // win: the bf16 MLP branch in token order) -- written to x1 and normalised in the same pass; the arithmetic and its order are those
    // of window_scatter_add_kernel (as in ln_add_fwd_kernel): bitwise the same x1
    const float sc = (win && scale) ? scale[(long long)blockIdx.x * RPB / S] : 1.0f;
    f32x4 v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ch < nchunks) {
            if (win) {
                const f32x4 w = load4<PSWIN_BF16>(win, (size_t)row * C + 4 * (size_t)ch);
                f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
                if (bias) b4 = *reinterpret_cast<const f32x4*>(bias + 4 * (size_t)ch);
                v[k] = branch_add(w, b4, bias != nullptr, sc, scale != nullptr, *reinterpret_cast<const f32x4*>(x + (size_t)row * C + 4 * ch));
                *reinterpret_cast<f32x4*>(x1 + (size_t)row * C + 4 * (size_t)ch) = v[k];
            } else {
                v[k] = *reinterpret_cast<const f32x4*>(x + (size_t)row * C + 4 * ch);
            }
        }
    }
    float mu, rs_;
    row_stats<L, NCH, false>(v, lane, nchunks, C, eps, mu, rs_);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        if (ch < nchunks) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + 4 * ch);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(beta + 4 * ch);
            const f32x4 o = ln_affine(v[k], mu, rs_, g4, b4);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[(4 * ch + e) * (RPB + 1) + rsub] = o[e];
        }
    }
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs_;
    }
    __syncthreads();
    const long long row0 = (long long)blockIdx.x * RPB;
    const int b = (int)(row0 / S);
    const int t0 = (int)(row0 - (long long)b * S);
    float* yb = y + (size_t)b * C * S + t0;
    constexpr int Q = RPB / 4;                       // 16-byte groups per channel
    for (int i = threadIdx.x; i < C * Q; i += THREADS) {
        const int c = i / Q, r4 = i - c * Q;
        const float* tp = tile + c * (RPB + 1) + 4 * r4;
        *reinterpret_cast<f32x4*>(yb + (size_t)c * S + 4 * r4) = f32x4{tp[0], tp[1], tp[2], tp[3]};
    }
}

template <int L, int NCH>
__global__ __launch_bounds__(THREADS) void ln_nchw_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ dres,
                                                              float* __restrict__ dx, float* __restrict__ part,
                                                              long long rows, int S, int C, void* __restrict__ ex,
                                                              const float* __restrict__ ex_scale) {
    constexpr int RPB = THREADS / L;
    constexpr int Q = RPB / 4;
    extern __shared__ float tile[];                 // [RPB][C + 4] then the partial-sum staging
    __shared__ alignas(16) float red[2][THREADS * 4];
    const int lane = threadIdx.x % L, rsub = threadIdx.x / L;
    const int nchunks = C / 4, LD = C + 4;
    f32x4 dg[NCH], db[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) dg[k] = db[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long row0 = (long long)blockIdx.x * RPB; row0 < rows; row0 += (long long)gridDim.x * RPB) {
        const int b = (int)(row0 / S);
        const int t0 = (int)(row0 - (long long)b * S);
        const float* dyb = dy + (size_t)b * C * S + t0;
        __syncthreads();
        for (int i = threadIdx.x; i < C * Q; i += THREADS) {
            const int c = i / Q, r4 = i - c * Q;
            const f32x4 t = *reinterpret_cast<const f32x4*>(dyb + (size_t)c * S + 4 * r4);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[(4 * r4 + e) * LD + c] = t[e];
        }
        __syncthreads();
        const long long row = row0 + rsub;
        const float mu = mean[row], rs_ = rstd[row];
        f32x4 xh[NCH], g[NCH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int ch = lane + k * L;
            xh[k] = g[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ch < nchunks) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)row * C + 4 * ch);
                const f32x4 dyv = *reinterpret_cast<const f32x4*>(tile + rsub * LD + 4 * ch);
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + 4 * ch);
                bwd_chunk(xv, dyv, g4, mu, rs_, xh[k], g[k], dg[k], db[k], s1, s2);
            }
        }
        s1 = row_sum<L>(s1) / (float)C;
        s2 = row_sum<L>(s2) / (float)C;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int ch = lane + k * L;
            if (ch < nchunks) {
                f32x4 v = bwd_dx(g[k], xh[k], s1, s2, rs_);
                if (dres) v = v + *reinterpret_cast<const f32x4*>(dres + (size_t)row * C + 4 * ch);
                *reinterpret_cast<f32x4*>(dx + (size_t)row * C + 4 * ch) = v;
                // ex (round 4): bf16(scale[b] * dx) in token order -- the gradient of the stage's closing MLP branch (the backward of
                // window_scatter_add's cast), written while dx is in registers instead of by a pswin_window_gather pass
                if (ex) store4<PSWIN_BF16>(ex, (size_t)row * C + 4 * (size_t)ch, ex_scale ? v * ex_scale[b] : v);
            }
        }
    }
    const f32x4 no_dr[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    bwd_partials<L, NCH, false>(red, dg, db, no_dr, part, lane, rsub, nchunks, C);
}

// The exact-row forms of the two NCHW kernels (C == 12 * L).  Forward: nothing depends on an index, so scale[b], gamma, beta, bias and
// the chunks of both streams leave in one burst; an absent branch (win == nullptr) is a zero-byte resource and a select.
template <int L>
__global__ __launch_bounds__(THREADS, 8) void ln_nchw_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                                   float* __restrict__ mean, float* __restrict__ rstd, unsigned S,
                                                                   unsigned rows, unsigned B, const unsigned short* __restrict__ win,
                                                                   const float* __restrict__ scale, const float* __restrict__ bias,
                                                                   float* __restrict__ x1) {
    constexpr int NCH = 3, C = 4 * L * NCH, RPB = THREADS / L;
    extern __shared__ float tile[];                 // [C][RPB + 1]
    const unsigned lane = threadIdx.x % L, rsub = threadIdx.x / L;
    const unsigned row0 = blockIdx.x * RPB, row = row0 + rsub;      // grid covers B * S exactly
    const unsigned b = row0 / S, t0 = row0 - b * S;
    const bool has_win = win != nullptr, has_scale = has_win && scale != nullptr, has_bias = has_win && bias != nullptr;
    const float scv = bload_f32(uniform_rsrc(has_win ? scale : nullptr, B * 4u), b * 4u);
    const rsrc_t gr = uniform_rsrc(gamma, C * 4u), br = uniform_rsrc(beta, C * 4u), bir = uniform_rsrc(has_win ? bias : nullptr, C * 4u);
    const rsrc_t xr = uniform_rsrc(x, rows * (C * 4u)), wr = uniform_rsrc(win, rows * (C * 2u));
    const rsrc_t x1r = uniform_rsrc(has_win ? x1 : nullptr, rows * (C * 4u));
    f32x4 g4[NCH], b4[NCH], bi[NCH], xv[NCH], w[NCH], v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const unsigned cb = (lane + k * L) * 16u;
        g4[k] = bload4<PSWIN_F32>(gr, cb);
        b4[k] = bload4<PSWIN_F32>(br, cb);
        bi[k] = bload4<PSWIN_F32>(bir, cb);
        xv[k] = bload4<PSWIN_F32>(xr, row * (C * 4u) + cb);
        w[k] = bload4<PSWIN_BF16>(wr, row * (C * 2u) + (lane + k * L) * 8u);
    }
    const float sc = has_scale ? scv : 1.0f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        v[k] = has_win ? branch_add(w[k], bi[k], has_bias, sc, has_scale, xv[k]) : xv[k];
        bstore4<PSWIN_F32>(x1r, row * (C * 4u) + (lane + k * L) * 16u, v[k]);        // no branch written: dropped (zero-byte resource)
    }
    float mu, rs_;
    row_stats<L, NCH, true>(v, lane, NCH * L, C, eps, mu, rs_);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int ch = lane + k * L;
        const f32x4 o = ln_affine(v[k], mu, rs_, g4[k], b4[k]);
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(4 * ch + e) * (RPB + 1) + rsub] = o[e];
    }
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs_;
    }
    __syncthreads();
    float* yb = y + (size_t)b * C * S + t0;
    constexpr int Q = RPB / 4;                       // 16-byte groups per channel
    for (int i = threadIdx.x; i < C * Q; i += THREADS) {
        const int c = i / Q, r4 = i - c * Q;
        const float* tp = tile + c * (RPB + 1) + 4 * r4;
        *reinterpret_cast<f32x4*>(yb + (size_t)c * S + 4 * r4) = f32x4{tp[0], tp[1], tp[2], tp[3]};
    }
}

// Backward: a software pipeline one trip deep.  The next trip's dy tile (registers), x, dres, mean, rstd and ex_scale[b] are requested
// before this trip's stores; a trip's operands are therefore on their way before the barrier that publishes its transposed dy tile.
// The prefetch behind the last trip reads zeros through OOB.
template <int L>
__global__ __launch_bounds__(THREADS, 4) void ln_nchw_bwd_rows_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                      const float* __restrict__ gamma, const float* __restrict__ dres,
                                                                      float* __restrict__ dx, float* __restrict__ part, unsigned rows,
                                                                      unsigned S, unsigned B, void* __restrict__ ex,
                                                                      const float* __restrict__ ex_scale) {
    constexpr int NCH = 3, C = 4 * L * NCH, RPB = THREADS / L, Q = RPB / 4, LD = C + 4;
    constexpr int TIT = C * Q / THREADS;            // 16-byte requests per thread for a dy tile (= 3)
    static_assert(C * Q % THREADS == 0, "the dy tile is a whole number of requests per thread");
    extern __shared__ float tile[];                 // [RPB][C + 4]
    __shared__ alignas(16) float red[2][THREADS * 4];
    const unsigned lane = threadIdx.x % L, rsub = threadIdx.x / L;
    const bool has_dres = dres != nullptr, has_exs = ex != nullptr && ex_scale != nullptr;
    const rsrc_t dyr = uniform_rsrc(dy, rows * (C * 4u)), xr = uniform_rsrc(x, rows * (C * 4u)), drr = uniform_rsrc(dres, rows * (C * 4u));
    const rsrc_t meanr = uniform_rsrc(mean, rows * 4u), rstdr = uniform_rsrc(rstd, rows * 4u);
    const rsrc_t exsr = uniform_rsrc(ex ? ex_scale : nullptr, B * 4u), gr = uniform_rsrc(gamma, C * 4u);
    const rsrc_t dxr = uniform_rsrc(dx, rows * (C * 4u)), exr = uniform_rsrc(ex, rows * (C * 2u));
    f32x4 g4[NCH], dg[NCH], db[NCH];
    const f32x4 no_dr[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        g4[k] = bload4<PSWIN_F32>(gr, (lane + k * L) * 16u);
        dg[k] = db[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 tq[TIT], xv[NCH], rv[NCH];
    float mu, rs_, exs;
    const unsigned step = gridDim.x * RPB;
    auto fetch = [&](unsigned row0) {
        const bool ok = row0 < rows;                // block-uniform (S % RPB == 0)
        const unsigned b = row0 / S, t0 = row0 - b * S, row = row0 + rsub;
#pragma unroll
        for (int it = 0; it < TIT; ++it) {
            const unsigned i = threadIdx.x + it * THREADS, c = i / Q, r4 = i - c * Q;
            tq[it] = bload4<PSWIN_F32, NT>(dyr, ok ? ((b * C + c) * S + t0 + 4 * r4) * 4u : OOB);
        }
        mu = bload_f32(meanr, ok ? row * 4u : OOB);
        rs_ = bload_f32(rstdr, ok ? row * 4u : OOB);
        exs = bload_f32(exsr, ok ? b * 4u : OOB);
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            xv[k] = bload4<PSWIN_F32, NT>(xr, ok ? row * (C * 4u) + (lane + k * L) * 16u : OOB);
            rv[k] = bload4<PSWIN_F32, NT>(drr, ok ? row * (C * 4u) + (lane + k * L) * 16u : OOB);
        }
    };
    unsigned row0 = blockIdx.x * RPB;
    __builtin_amdgcn_sched_barrier(0);
    fetch(row0);
    __builtin_amdgcn_sched_barrier(0);
    auto trip = [&](unsigned row0) {
        const unsigned row = row0 + rsub;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < TIT; ++it) {
            const unsigned i = threadIdx.x + it * THREADS, c = i / Q, r4 = i - c * Q;
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[(4 * r4 + e) * LD + c] = tq[it][e];
        }
        __syncthreads();
        // a value of its own, not the register the next trip's ex_scale[b] is loaded into: a copy of that one at the end of the trip
        // would wait for the request just made
        const float mu_ = mu, rs0 = rs_, es = has_exs ? exs : 1.0f;
        f32x4 xh[NCH], g[NCH], v[NCH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const f32x4 dyv = *reinterpret_cast<const f32x4*>(tile + rsub * LD + 4 * (lane + k * L));
            bwd_chunk(xv[k], dyv, g4[k], mu_, rs0, xh[k], g[k], dg[k], db[k], s1, s2);
        }
        s1 = row_sum<L>(s1) / (float)C;
        s2 = row_sum<L>(s2) / (float)C;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            v[k] = bwd_dx(g[k], xh[k], s1, s2, rs0);
            v[k] = has_dres ? v[k] + rv[k] : v[k];
        }
        __builtin_amdgcn_sched_barrier(0);          // the request stays between the row math and the stores (see ln_bwd_rows_kernel)
        fetch(row0 + step);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            bstore4<PSWIN_F32>(dxr, row * (C * 4u) + (lane + k * L) * 16u, v[k]);
            // ex: bf16(scale[b] * dx) in token order (see ln_nchw_bwd_kernel); ex == nullptr: a zero-byte resource drops the store
            bstore4<PSWIN_BF16>(exr, row * (C * 2u) + (lane + k * L) * 8u, v[k] * es);
        }
    };
    // dropped stores and a loop entered without a test: the loop header sees the same requests on both edges (see ln_bwd_rows_kernel)
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        bstore4<PSWIN_F32>(dxr, OOB + k * L * 16u, f32x4{0.f, 0.f, 0.f, 0.f});
        bstore4<PSWIN_BF16>(exr, OOB + k * L * 8u, f32x4{0.f, 0.f, 0.f, 0.f});
    }
    __builtin_amdgcn_sched_barrier(0);
    do {
        trip(row0);
        row0 += step;
    } while (row0 < rows);
    bwd_partials<L, NCH, false>(red, dg, db, no_dr, part, (int)lane, (int)rsub, NCH * L, C);
}

// out_k[c] = sum_r part[r][k * C + c] for the nseg (2 or 3) segments of rows of nseg * C floats; 16 columns x 64 row lanes
__global__ void colsum_seg_kernel(const float* __restrict__ part, int R, int C, int nseg, float* __restrict__ out_a,
                                  float* __restrict__ out_b, float* __restrict__ out_c) {
    __shared__ float red[64][16];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const int N = nseg * C;
    float s0 = 0.f, s1 = 0.f;
    if (c < N) {
        int r = rl;
        for (; r + 64 < R; r += 128) {
            s0 += part[(size_t)r * N + c];
            s1 += part[(size_t)(r + 64) * N + c];
        }
        for (; r < R; r += 64) s0 += part[(size_t)r * N + c];
    }
    red[rl][cl] = s0 + s1;
    __syncthreads();
    if (rl < 16) red[rl][cl] = (red[rl][cl] + red[rl + 16][cl]) + (red[rl + 32][cl] + red[rl + 48][cl]);
    __syncthreads();
    if (rl == 0 && c < N) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[k][cl];
        if (c < C) out_a[c] = s;
        else if (c < 2 * C) out_b[c - C] = s;
        else out_c[c - 2 * C] = s;
    }
}

inline void launch_colsum_seg(const float* part, int R, int C, int nseg, float* out_a, float* out_b, float* out_c,
                              hipStream_t st) {
    hipLaunchKernelGGL(colsum_seg_kernel, dim3((nseg * C + 15) / 16), dim3(1024), 0, st, part, R, C, nseg, out_a, out_b, out_c);
}

// up to 4 chunks of 4 elements per lane (8 for rows wider than 1024 elements: PatchMerging of C >= 384)
inline int pick_lanes(int C) {
    int L = 2;
    while (L * 16 < C && L < 64) L *= 2;
    return L;
}
inline bool wide_row(int C) { return C > 1024; }
constexpr int MAX_C = 2048;

// Persistent grid of the backward kernels: exactly the resident capacity (256 CUs x 4 blocks of 4 waves at ~125 VGPRs).
// 1536 blocks ran as 1.5 rounds (the last half round leaves half of the chip idle: -1.2 % end to end), 512 leave two
// of the four wave slots per SIMD empty (3.4 TB/s).  The partial rows are summed by the grouped end-of-pass reduction.
constexpr int BWD_MAX_BLOCKS = 1024;

inline int bwd_blocks(long long rows, int L) {
    const int rpb = THREADS / L;
    long long nb = (rows + rpb - 1) / rpb;
    return (int)(nb < BWD_MAX_BLOCKS ? nb : BWD_MAX_BLOCKS);
}

// f(std::integral_constant<int, LL>()) for the lane counts pick_lanes() returns
template <typename F>
inline int with_lanes(int L, F&& f) {
    switch (L) {
        case 2: return f(std::integral_constant<int, 2>());
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        case 64: return f(std::integral_constant<int, 64>());
        default: return PSWIN_ERR_ARG;
    }
}

// pswin_ln_rows_tune: 0 = the exact-row kernels where they apply, 1 = always the generic kernels
int g_rows_mode = 0;

// the exact-row kernels: C == 12 * L with L = 8 .. 64 (96, 192, 384, 768), rows and every operand within 32-bit byte offsets
inline bool exact_rows(int L, int C, long long rows) {
    return g_rows_mode == 0 && L >= 8 && C == 12 * L && rows < 0x7fffffffll;
}
inline bool fits32(long long elems, int elem_bytes) { return (unsigned long long)elems * (unsigned)elem_bytes < MAX_OPERAND_BYTES; }

template <typename F>
inline int with_row_lanes(int L, F&& f) {
    switch (L) {
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        case 64: return f(std::integral_constant<int, 64>());
        default: return PSWIN_ERR_ARG;
    }
}

template <int MODE, int XDT, int YDT>
int launch_fwd(int L, const void* x, const RowSrc& rs, const float* gamma, const float* beta, float eps, void* y,
               float* mean, float* rstd, long long rows, int C, hipStream_t st, const float* add = nullptr) {
    const long long B = rows / rs.n_out;
    if (exact_rows(L, C, rows) && fits32(B * rs.S * (MODE == 0 ? C : C / 4), XDT == PSWIN_F32 ? 4 : 2) &&
        fits32(rows * C, YDT == PSWIN_F32 ? 4 : 2) && fits32((long long)rs.n_out * C, 4)) {
        return with_row_lanes(L, [&](auto ll) {
            constexpr int LL = decltype(ll)::value;
            const int rpb = THREADS / LL;
            hipLaunchKernelGGL((ln_fwd_rows_kernel<MODE, XDT, YDT, LL>), dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(THREADS), 0, st,
                               x, rs, gamma, beta, eps, y, mean, rstd, (unsigned)rows, (unsigned)B, add);
            PSWIN_LAUNCH_RET();
        });
    }
    if (wide_row(C)) {
        hipLaunchKernelGGL((ln_fwd_kernel<MODE, XDT, YDT, 64, 8>), dim3((unsigned)((rows + 3) / 4)), dim3(THREADS), 0,
                           st, x, rs, gamma, beta, eps, y, mean, rstd, rows, C, add);
        PSWIN_LAUNCH_RET();
    }
    return with_lanes(L, [&](auto ll) {
        constexpr int LL = decltype(ll)::value;
        const int rpb = THREADS / LL;
        hipLaunchKernelGGL((ln_fwd_kernel<MODE, XDT, YDT, LL, 4>), dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(THREADS), 0,
                           st, x, rs, gamma, beta, eps, y, mean, rstd, rows, C, add);
        PSWIN_LAUNCH_RET();
    });
}

template <int MODE, int DYDT, int XDT, bool RSUM>
int launch_bwd(int L, const void* dy, const int32_t* inv, const void* x, const RowSrc& rs, const float* mean,
               const float* rstd, const float* gamma, void* dx, const float* dres, const float* res_scale, float* part,
               long long rows, int C, int blocks, hipStream_t st, BwdExtra ex = BwdExtra{}) {
    constexpr bool CAN_EX = MODE == 0 && XDT == PSWIN_F32;
    if constexpr (MODE == 0 && XDT == PSWIN_F32) {
        const long long B = rows / rs.S;
        if (exact_rows(L, C, rows) && rs.S >= THREADS / L && fits32(rows * C, 4) && fits32(B * rs.n_out * C, DYDT == PSWIN_F32 ? 4 : 2) &&
            (!ex.ex || fits32(B * ex.n_rows * C, 2))) {
            return with_row_lanes(L, [&](auto ll) {
                constexpr int LL = decltype(ll)::value;
                if (ex.ex)
                    hipLaunchKernelGGL((ln_bwd_rows_kernel<DYDT, LL, RSUM, true>), dim3(blocks), dim3(THREADS), 0, st, dy, inv,
                                       (const float*)x, rs, mean, rstd, gamma, (float*)dx, dres, res_scale, part, (unsigned)rows, (unsigned)B, ex);
                else
                    hipLaunchKernelGGL((ln_bwd_rows_kernel<DYDT, LL, RSUM, false>), dim3(blocks), dim3(THREADS), 0, st, dy, inv,
                                       (const float*)x, rs, mean, rstd, gamma, (float*)dx, dres, res_scale, part, (unsigned)rows, (unsigned)B, BwdExtra{});
                PSWIN_LAUNCH_RET();
            });
        }
    }
    if (wide_row(C)) {
        if (ex.ex) return PSWIN_ERR_UNSUPPORTED;
        hipLaunchKernelGGL((ln_bwd_kernel<MODE, DYDT, XDT, 64, 8, RSUM>), dim3(blocks), dim3(THREADS), 0, st, dy, inv, x, rs,
                           mean, rstd, gamma, dx, dres, res_scale, part, rows, C, BwdExtra{});
        PSWIN_LAUNCH_RET();
    }
    if (ex.ex && !CAN_EX) return PSWIN_ERR_UNSUPPORTED;
    return with_lanes(L, [&](auto ll) {
        constexpr int LL = decltype(ll)::value;
        if constexpr (CAN_EX) {
            if (ex.ex) {
                if (C / 4 <= 3 * LL)
                    hipLaunchKernelGGL((ln_bwd_kernel<MODE, DYDT, XDT, LL, 3, RSUM, true>), dim3(blocks), dim3(THREADS), 0, st, dy, inv,
                                       x, rs, mean, rstd, gamma, dx, dres, res_scale, part, rows, C, ex);
                else
                    hipLaunchKernelGGL((ln_bwd_kernel<MODE, DYDT, XDT, LL, 4, RSUM, true>), dim3(blocks), dim3(THREADS), 0, st, dy, inv,
                                       x, rs, mean, rstd, gamma, dx, dres, res_scale, part, rows, C, ex);
                PSWIN_LAUNCH_RET();
            }
        }
        if (C / 4 <= 3 * LL)      // 3 chunks per lane (C = 96, 192, 384, 768): 20 registers less, 4 waves per SIMD
            hipLaunchKernelGGL((ln_bwd_kernel<MODE, DYDT, XDT, LL, 3, RSUM>), dim3(blocks), dim3(THREADS), 0, st, dy, inv,
                               x, rs, mean, rstd, gamma, dx, dres, res_scale, part, rows, C, BwdExtra{});
        else
            hipLaunchKernelGGL((ln_bwd_kernel<MODE, DYDT, XDT, LL, 4, RSUM>), dim3(blocks), dim3(THREADS), 0, st, dy, inv,
                               x, rs, mean, rstd, gamma, dx, dres, res_scale, part, rows, C, BwdExtra{});
        PSWIN_LAUNCH_RET();
    });
}

}  // namespace

extern "C" int pswin_ln_workspace(long long rows, int C) {
    if (rows <= 0 || C <= 0 || C % 8) return PSWIN_ERR_ARG;
    return bwd_blocks(rows, pick_lanes(C)) * 3 * C;
}

/* tuning hook: 0 = the exact-row LayerNorm kernels where they apply (default), 1 = always the generic kernels */
extern "C" int pswin_ln_rows_tune(int mode) {
    if (mode != 0 && mode != 1) return PSWIN_ERR_ARG;
    g_rows_mode = mode;
    return PSWIN_OK;
}

extern "C" int pswin_ln_partial_rows(long long rows, int C) {
    if (rows <= 0 || C <= 0 || C % 8) return PSWIN_ERR_ARG;
    return bwd_blocks(rows, pick_lanes(C));
}

extern "C" int pswin_ln_gather_fwd_add(const void* x, int x_dtype, const int32_t* map, const float* gamma,
                                       const float* beta, float eps, const float* add_rows, void* y, int y_dtype, float* mean,
                                       float* rstd, int B, int S, int n_out, int C, void* stream) {
    PSWIN_CHECK_ARG(x && gamma && beta && y && mean && rstd && B > 0 && S > 0 && n_out > 0);
    PSWIN_CHECK_ARG(valid_dtype(x_dtype) && valid_dtype(y_dtype));
    PSWIN_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= MAX_C && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta));
    PSWIN_CHECK_ARG(map || n_out == S);
    PSWIN_CHECK_ARG(!add_rows || (!map && aligned16(add_rows)));      // the added rows follow the token order of an image
    RowSrc rs = {0, map, S, n_out, 0, 0, 0};
    const long long rows = (long long)B * n_out;
    const int L = pick_lanes(C);
    return dispatch2(x_dtype, y_dtype, [&](auto xd, auto yd) {
        return launch_fwd<0, decltype(xd)::value, decltype(yd)::value>(L, x, rs, gamma, beta, eps, y, mean, rstd, rows,
                                                                       C, (hipStream_t)stream, add_rows);
    });
}

extern "C" int pswin_ln_gather_fwd(const void* x, int x_dtype, const int32_t* map, const float* gamma,
                                   const float* beta, float eps, void* y, int y_dtype, float* mean, float* rstd, int B,
                                   int S, int n_out, int C, void* stream) {
    return pswin_ln_gather_fwd_add(x, x_dtype, map, gamma, beta, eps, nullptr, y, y_dtype, mean, rstd, B, S, n_out, C, stream);
}

extern "C" int pswin_scatter_add_ln_fwd_map(const void* win, int win_dtype, const int32_t* inv, const float* resid,
                                            const float* scale, const float* bias, float* x1, const float* gamma,
                                            const float* beta, float eps, void* y, int y_dtype, float* mean, float* rstd, int B,
                                            int S, int n_slots, int C, const int32_t* out_map, int n_out, const int32_t* out_pads,
                                            int n_out_pads, void* stream) {
    PSWIN_CHECK_ARG(win && resid && x1 && gamma && beta && y && mean && rstd && B > 0 && S > 0 && n_slots > 0);
    PSWIN_CHECK_ARG(valid_dtype(win_dtype) && valid_dtype(y_dtype) && (inv || n_slots == S));
    PSWIN_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= 1024 && aligned16(win) && aligned16(resid) && aligned16(x1) && aligned16(y));
    PSWIN_CHECK_ARG(aligned16(gamma) && aligned16(beta) && aligned16(bias));
    PSWIN_CHECK_ARG(out_map ? (n_out >= S && n_out_pads == n_out - S && (out_pads || n_out_pads == 0)) : (n_out == S && n_out_pads == 0));
    const OutMap om = {out_map, out_pads, n_out, n_out_pads, B};
    const long long rows = (long long)B * S;
    const long long groups = rows + (out_map ? (long long)B * n_out_pads : 0);     // row groups: tokens, then the zero slots
    const int L = pick_lanes(C);
    hipStream_t st = (hipStream_t)stream;
    const bool rows32 = exact_rows(L, C, groups) && fits32(rows * C, 4) && fits32((long long)B * n_slots * C, win_dtype == PSWIN_F32 ? 4 : 2) &&
                        fits32((long long)B * n_out * C, y_dtype == PSWIN_F32 ? 4 : 2);
    return dispatch2(win_dtype, y_dtype, [&](auto wd, auto yd) {
        if (rows32) {
            return with_row_lanes(L, [&](auto ll) {
                constexpr int LL = decltype(ll)::value;
                const int rpb = THREADS / LL;
                hipLaunchKernelGGL((ln_add_fwd_rows_kernel<decltype(wd)::value, decltype(yd)::value, LL>),
                                   dim3((unsigned)((groups + rpb - 1) / rpb)), dim3(THREADS), 0, st, win, inv, resid, scale, bias, x1,
                                   gamma, beta, eps, y, mean, rstd, (unsigned)rows, (unsigned)S, (unsigned)n_slots, om);
                PSWIN_LAUNCH_RET();
            });
        }
        return with_lanes(L, [&](auto ll) {
            constexpr int LL = decltype(ll)::value;
            const int rpb = THREADS / LL;
            hipLaunchKernelGGL((ln_add_fwd_kernel<decltype(wd)::value, decltype(yd)::value, LL, 4>),
                               dim3((unsigned)((groups + rpb - 1) / rpb)), dim3(THREADS), 0, st, win, inv, resid, scale, bias, x1,
                               gamma, beta, eps, y, mean, rstd, rows, S, n_slots, C, om);
            PSWIN_LAUNCH_RET();
        });
    });
}

extern "C" int pswin_scatter_add_ln_fwd(const void* win, int win_dtype, const int32_t* inv, const float* resid,
                                        const float* scale, const float* bias, float* x1, const float* gamma,
                                        const float* beta, float eps, void* y, int y_dtype, float* mean, float* rstd, int B,
                                        int S, int n_slots, int C, void* stream) {
    return pswin_scatter_add_ln_fwd_map(win, win_dtype, inv, resid, scale, bias, x1, gamma, beta, eps, y, y_dtype, mean, rstd, B, S, n_slots, C,
                                        nullptr, S, nullptr, 0, stream);
}

extern "C" int pswin_ln_gather_bwd_ex(const void* dy, int dy_dtype, const int32_t* inv, const void* x, int x_dtype,
                                      const float* mean, const float* rstd, const float* gamma, const float* dres,
                                      const float* res_scale, float* dres_sum, void* dx, float* dgamma, float* dbeta,
                                      float* workspace, int B, int S, int n_out, int C, void* ex, const int32_t* ex_map, int ex_rows,
                                      const float* ex_scale, const int32_t* ex_pads, int n_ex_pads, void* stream) {
    PSWIN_CHECK_ARG(dy && x && mean && rstd && gamma && dx && workspace && B > 0 && S > 0 && n_out > 0);
    PSWIN_CHECK_ARG((dgamma && dbeta) || (!dgamma && !dbeta));
    PSWIN_CHECK_ARG(valid_dtype(x_dtype) && valid_dtype(dy_dtype));
    PSWIN_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= MAX_C && aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(gamma));
    PSWIN_CHECK_ARG(inv || n_out == S);
    PSWIN_CHECK_ARG(!dres || (x_dtype == PSWIN_F32 && aligned16(dres)));
    PSWIN_CHECK_ARG(!dres_sum || dres);
    if (ex) {
        PSWIN_CHECK_ARG(x_dtype == PSWIN_F32 && aligned16(ex) && !wide_row(C) && (long long)B * ex_rows * C < 0x7fffffffll);
        PSWIN_CHECK_ARG(ex_map ? (ex_rows >= S && n_ex_pads == ex_rows - S && (ex_pads || n_ex_pads == 0)) : (ex_rows == S && n_ex_pads == 0));
    }
    const BwdExtra be = {ex, ex_map, ex_scale, ex_pads, ex_rows, ex ? n_ex_pads : 0, B};
    RowSrc rs = {0, nullptr, S, n_out, 0, 0, 0};
    const long long rows = (long long)B * S;
    const int L = pick_lanes(C);
    const int blocks = bwd_blocks(rows, L);
    int rc;
    if (dres_sum) {
        rc = dispatch2(dy_dtype, PSWIN_F32, [&](auto dd, auto xd) {
            return launch_bwd<0, decltype(dd)::value, PSWIN_F32, true>(L, dy, inv, x, rs, mean, rstd, gamma, dx, dres, res_scale,
                                                                       workspace, rows, C, blocks, (hipStream_t)stream, be);
        });
    } else {
        rc = dispatch2(dy_dtype, x_dtype, [&](auto dd, auto xd) {
            return launch_bwd<0, decltype(dd)::value, decltype(xd)::value, false>(L, dy, inv, x, rs, mean, rstd, gamma, dx, dres,
                                                                                  nullptr, workspace, rows, C, blocks,
                                                                                  (hipStream_t)stream, be);
        });
    }
    if (rc) return rc;
    // partial rows are [dgamma(C) | dbeta(C) | dres_sum(C)]; the outputs may live in different buffers.
    // dgamma == dbeta == NULL: the caller sums the partial rows itself (pswin_reduce_jobs); dres_sum then only selects
    // the 3-segment row layout and is not written.
    if (dgamma) launch_colsum_seg(workspace, blocks, C, dres_sum ? 3 : 2, dgamma, dbeta, dres_sum, (hipStream_t)stream);
    PSWIN_LAUNCH_RET();
}

extern "C" int pswin_ln_gather_bwd(const void* dy, int dy_dtype, const int32_t* inv, const void* x, int x_dtype,
                                   const float* mean, const float* rstd, const float* gamma, const float* dres,
                                   const float* res_scale, float* dres_sum, void* dx, float* dgamma, float* dbeta,
                                   float* workspace, int B, int S, int n_out, int C, void* stream) {
    return pswin_ln_gather_bwd_ex(dy, dy_dtype, inv, x, x_dtype, mean, rstd, gamma, dres, res_scale, dres_sum, dx, dgamma, dbeta, workspace, B, S,
                                  n_out, C, nullptr, nullptr, S, nullptr, nullptr, 0, stream);
}

extern "C" int pswin_ln_patch_merge_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, float eps,
                                        void* y, int y_dtype, float* mean, float* rstd, int B, int H, int W, int C,
                                        void* stream) {
    PSWIN_CHECK_ARG(x && gamma && beta && y && mean && rstd && B > 0 && H > 0 && W > 0);
    PSWIN_CHECK_ARG(valid_dtype(x_dtype) && valid_dtype(y_dtype));
    const int C4 = 4 * C;
    PSWIN_CHECK_ARG(C >= 16 && C % 16 == 0 && C4 <= MAX_C && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta));
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    RowSrc rs = {1, nullptr, H * W, H2 * W2, H, W, W2};
    const long long rows = (long long)B * H2 * W2;
    const int L = pick_lanes(C4);
    return dispatch2(x_dtype, y_dtype, [&](auto xd, auto yd) {
        return launch_fwd<1, decltype(xd)::value, decltype(yd)::value>(L, x, rs, gamma, beta, eps, y, mean, rstd, rows,
                                                                       C4, (hipStream_t)stream);
    });
}

extern "C" int pswin_ln_patch_merge_bwd(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean,
                                        const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta,
                                        float* workspace, int B, int H, int W, int C, void* stream) {
    PSWIN_CHECK_ARG(dy && x && mean && rstd && gamma && dx && workspace && B > 0 && H > 0 && W > 0);
    PSWIN_CHECK_ARG((dgamma && dbeta) || (!dgamma && !dbeta));
    PSWIN_CHECK_ARG(valid_dtype(x_dtype) && valid_dtype(dy_dtype));
    const int C4 = 4 * C;
    PSWIN_CHECK_ARG(C >= 16 && C % 16 == 0 && C4 <= MAX_C && aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(gamma));
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    RowSrc rs = {1, nullptr, H * W, H2 * W2, H, W, W2};
    const long long rows = (long long)B * H2 * W2;
    const int L = pick_lanes(C4);
    const int blocks = bwd_blocks(rows, L);
    int rc = dispatch2(dy_dtype, x_dtype, [&](auto dd, auto xd) {
        return launch_bwd<1, decltype(dd)::value, decltype(xd)::value, false>(L, dy, nullptr, x, rs, mean, rstd, gamma, dx,
                                                                              nullptr, nullptr, workspace, rows, C4, blocks,
                                                                              (hipStream_t)stream);
    });
    if (rc) return rc;
    if (dgamma) launch_colsum_seg(workspace, blocks, C4, 2, dgamma, dbeta, nullptr, (hipStream_t)stream);
    PSWIN_LAUNCH_RET();
}

extern "C" int pswin_ln_nchw_supported(int S, int C) {
    if (S <= 0 || C < 8 || C % 8 || C > 1024) return 0;
    const int L = pick_lanes(C);
    const int rpb = THREADS / L;
    return (rpb >= 4 && S % rpb == 0) ? 1 : 0;
}

extern "C" int pswin_scatter_add_ln_nchw_fwd(const void* win_bf16, const float* x, const float* scale, const float* bias, float* x1,
                                             const float* gamma, const float* beta, float eps, float* y, float* mean, float* rstd,
                                             int B, int S, int C, void* stream) {
    const void* win = win_bf16;
    PSWIN_CHECK_ARG(x && gamma && beta && y && mean && rstd && B > 0 && pswin_ln_nchw_supported(S, C));
    PSWIN_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta));
    PSWIN_CHECK_ARG(win ? (x1 && aligned16(win) && aligned16(x1) && aligned16(bias)) : (!x1 && !scale && !bias));
    const int L = pick_lanes(C), rpb = THREADS / L;
    const long long rows = (long long)B * S;
    const unsigned grid = (unsigned)(rows / rpb);
    const size_t lds = (size_t)C * (rpb + 1) * sizeof(float);
    if (exact_rows(L, C, rows) && fits32(rows * C, 4)) {
        return with_row_lanes(L, [&](auto ll) {
            hipLaunchKernelGGL((ln_nchw_fwd_rows_kernel<decltype(ll)::value>), dim3(grid), dim3(THREADS), lds, (hipStream_t)stream, x, gamma,
                               beta, eps, y, mean, rstd, (unsigned)S, (unsigned)rows, (unsigned)B,
                               reinterpret_cast<const unsigned short*>(win), scale, bias, x1);
            PSWIN_LAUNCH_RET();
        });
    }
    return with_lanes(L, [&](auto ll) {
        hipLaunchKernelGGL((ln_nchw_fwd_kernel<decltype(ll)::value, 4>), dim3(grid), dim3(THREADS), lds, (hipStream_t)stream, x, gamma,
                           beta, eps, y, mean, rstd, S, C, reinterpret_cast<const unsigned short*>(win), scale, bias, x1);
        PSWIN_LAUNCH_RET();
    });
}

extern "C" int pswin_ln_nchw_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, float* mean,
                                 float* rstd, int B, int S, int C, void* stream) {
    return pswin_scatter_add_ln_nchw_fwd(nullptr, x, nullptr, nullptr, nullptr, gamma, beta, eps, y, mean, rstd, B, S, C, stream);
}

extern "C" int pswin_ln_nchw_bwd_ex(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                    const float* dres, float* dx, float* dgamma, float* dbeta, float* workspace, void* ex_bf16,
                                    const float* ex_scale, int B, int S, int C, void* stream) {
    PSWIN_CHECK_ARG(dy && x && mean && rstd && gamma && dx && workspace && B > 0 && pswin_ln_nchw_supported(S, C));
    PSWIN_CHECK_ARG((dgamma && dbeta) || (!dgamma && !dbeta));
    PSWIN_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(dx) && aligned16(gamma) && aligned16(dres) && aligned16(ex_bf16));
    const int L = pick_lanes(C), rpb = THREADS / L;
    const long long rows = (long long)B * S;
    const int blocks = bwd_blocks(rows, L);
    const size_t lds = (size_t)rpb * (C + 4) * sizeof(float);
    const bool rows32 = exact_rows(L, C, rows) && fits32(rows * C, 4);
    const int rc = rows32 ? with_row_lanes(L, [&](auto ll) {
        hipLaunchKernelGGL((ln_nchw_bwd_rows_kernel<decltype(ll)::value>), dim3(blocks), dim3(THREADS), lds, (hipStream_t)stream, dy, x,
                           mean, rstd, gamma, dres, dx, workspace, (unsigned)rows, (unsigned)S, (unsigned)B, ex_bf16, ex_scale);
        return PSWIN_OK;
    }) : with_lanes(L, [&](auto ll) {
        hipLaunchKernelGGL((ln_nchw_bwd_kernel<decltype(ll)::value, 4>), dim3(blocks), dim3(THREADS), lds, (hipStream_t)stream, dy, x,
                           mean, rstd, gamma, dres, dx, workspace, rows, S, C, ex_bf16, ex_scale);
        return PSWIN_OK;
    });
    if (rc) return rc;
    if (dgamma) launch_colsum_seg(workspace, blocks, C, 2, dgamma, dbeta, nullptr, (hipStream_t)stream);
    PSWIN_LAUNCH_RET();
}

extern "C" int pswin_ln_nchw_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                 const float* dres, float* dx, float* dgamma, float* dbeta, float* workspace, int B, int S,
                                 int C, void* stream) {
    return pswin_ln_nchw_bwd_ex(dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, workspace, nullptr, nullptr, B, S, C, stream);
}
