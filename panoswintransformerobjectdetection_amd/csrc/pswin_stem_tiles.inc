// Tile-geometry dependent part of pswin_stem.hip: included once per tile height STEM_TH inside its own namespace.
constexpr int TH = STEM_TH;                  // output tile rows of the 3x3 kernels; a wave owns two tile rows
constexpr int NW = TH / 2;
constexpr int WG = 64 * NW;
constexpr int XR = TH + 4, XC = TW + 4;      // input tile with a halo of 2
constexpr int AR = TH + 2, AC = TW + 2;      // a1 / dy2 tile with a halo of 1
constexpr int A_PIX = AR * AC;
constexpr int A_GROUPS = (A_PIX + 15) / 16;  // groups of 16 pixels
// row pitch (pixels) of the a1 LDS image.  8-row geometry (conv2 weight gradient): 40 = 0 mod 8, so the off64 swizzle of pixel
// (row, x) depends on x only and a fragment address is (row term) + (a lane constant per tap column): the kernel's inner loop then needs
// no address arithmetic (it was ~50 VALU instructions per tile row next to 36 MFMAs).  16-row geometry: dense (AC), addresses are
// tile-invariant there and hoisted by the compiler.
constexpr int ACP = STEM_TH == 8 ? 40 : AC;
constexpr int XS_BYTES = XR * XC * 8;
constexpr int ZSLOT = XS_BYTES;              // 16 zero bytes behind the input tile
constexpr int XS_TOTAL = XS_BYTES + 16;

struct Tile {
    int b, y0, x0;
};
__device__ inline Tile tile_of(int t, int nty, int ntx) {
    Tile r;
    r.b = t / (nty * ntx);
    const int rem = t - r.b * nty * ntx;
    const int ty = rem / ntx;
    r.y0 = ty * TH;
    r.x0 = (rem - ty * ntx) * TW;
    return r;
}

// input tile with halo 2 -> LDS (8 bytes per pixel, zero outside the image), plus the zero slot.
// Round 4: every request of the tile is issued before the first is consumed.  The round-1 form -- `if (inside) v = x4[...]` in a loop --
// compiled to a branch around each load with `s_waitcnt vmcnt(0)` behind it (hipcc's "register or load" select: cdna_hip_programming.md,
// projection-GEMM trap 4c): one memory round trip per loop trip, 2 per tile here and 8-10 for the dy2 tiles below, which was most of a
// tile's time (conv2 weight gradient: 10.6 us per tile for 1.1 us of MFMA work).  Now a buffer load per element with an out-of-range
// offset for pixels outside the image (the hardware returns zeros, no branch), all trips unrolled, loads first, LDS stores after.
// a buffer resource the compiler can SEE is wave-uniform (its inputs through readfirstlane): without it every buffer load below sat in a
// waterfall loop (cdna_hip_programming.md T20), which serialises consecutive loads just like the branches did
__device__ inline rsrc_t uniform_rsrc(const void* base, size_t bytes) {
    const unsigned long long v = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                             __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

constexpr int XS_IT = (XR * XC + WG - 1) / WG;
struct XsRegs {
    u32x2 v[XS_IT];
};
// request a tile's input pixels (registers only) ...
__device__ inline void issue_xs(const u64* __restrict__ x4, const Tile& t, int H, int W, XsRegs& r) {
    const rsrc_t xr = uniform_rsrc(x4 + (size_t)t.b * H * W, (size_t)H * W * 8);
#pragma unroll
    for (int it = 0; it < XS_IT; ++it) {
        const int i = threadIdx.x + it * WG;
        const int rr = i / XC, cc = i - rr * XC;
        const int gy = t.y0 - 2 + rr, gx = t.x0 - 2 + cc;
        const bool in = (i < XR * XC) & (gy >= 0) & (gy < H) & (gx >= 0) & (gx < W);       // (bitwise: no short-circuit branches in the request burst)
        r.v[it] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(xr, in ? (unsigned)(gy * W + gx) * 8u : 0xFFFFFF00u, 0, 0));
    }
}
// ... and put them into the LDS tile (the two halves let a kernel keep the NEXT tile's request in flight under this tile's work)
__device__ inline void store_xs(const XsRegs& r, char* xs) {
#pragma unroll
    for (int it = 0; it < XS_IT; ++it) {
        const int i = threadIdx.x + it * WG;
        if (i < XR * XC) reinterpret_cast<u32x2*>(xs)[i] = r.v[it];
    }
    if (threadIdx.x < 2) reinterpret_cast<u64*>(xs + ZSLOT)[threadIdx.x] = 0;
}
__device__ inline void load_xs(const u64* __restrict__ x4, const Tile& t, int H, int W, char* xs) {
    XsRegs r;
    issue_xs(x4, t, H, W, r);
    store_xs(r, xs);
}

// a [rows][row_px] block of 128-byte pixels of image b (dy2 / y2 layout) -> LDS image off128(pixel, chunk), zeros outside the image: the same
// all-requests-first form.  (py0, px0): image coordinates of the block's first pixel; n_pix pixels, row_px per row.
template <int N_PIX, int BATCH = 16>
__device__ inline void load_pix128(const void* __restrict__ src, int b, int H, int W, int py0, int px0, int row_px, char* dst) {
    constexpr int IT = (N_PIX * 8 + WG - 1) / WG;
    constexpr int NB = IT < BATCH ? IT : BATCH;          // requests in flight per thread (4 registers each): BATCH bounds the register cost
    const rsrc_t sr = uniform_rsrc(reinterpret_cast<const char*>(src) + (size_t)b * H * W * 128, (size_t)H * W * 128);
#pragma unroll
    for (int it0 = 0; it0 < IT; it0 += NB) {
        u32x4 v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = threadIdx.x + (it0 + k) * WG;
            const int P = i >> 3, ch = i & 7;
            const int py = P / row_px, px = P - py * row_px;
            const int gy = py0 + py, gx = px0 + px;
            const bool in = (it0 + k < IT) & (i < N_PIX * 8) & (gy >= 0) & (gy < H) & (gx >= 0) & (gx < W);
            v[k] = __builtin_amdgcn_raw_buffer_load_b128(sr, in ? (unsigned)(gy * W + gx) * 128u + 16u * ch : 0xFFFFFF00u, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = threadIdx.x + (it0 + k) * WG;
            if (it0 + k < IT && i < N_PIX * 8) *reinterpret_cast<u32x4*>(dst + off128(i >> 3, i & 7)) = v[k];
        }
    }
}

// The same block by LDS-DMA (buffer_load ... lds: no staging registers, no ds_write): every request of the tile is in flight at once --
// load_pix128 needs four registers per request, which held the conv2 data-gradient kernel (256 registers) to two bursts of five, i.e.
// two memory round trips per tile.  A wave instruction moves 8 pixels x 128 B and writes lane-linear (lane i -> byte 16 i of its 1 KB), so
// the off128 swizzle is applied on the SOURCE side: lane i fetches chunk (i & 7) ^ (i >> 3) of pixel 8 it + (i >> 3), whose low three
// bits are i >> 3.  Pixels outside the image or past n_valid: out-of-range offset, zeros land in LDS.  N_PIX: a multiple of 8.
typedef __attribute__((address_space(3))) void stem_lds_void;
template <int N_PIX>
__device__ inline void dma_pix128(const void* __restrict__ src, int b, int H, int W, int py0, int px0, int row_px, int n_valid, char* dst,
                                  int wave, int lane) {
    static_assert(N_PIX % 8 == 0, "whole wave instructions");
    const rsrc_t sr = uniform_rsrc(reinterpret_cast<const char*>(src) + (size_t)b * H * W * 128, (size_t)H * W * 128);
    const int pl = lane >> 3, ch = (lane & 7) ^ pl;
#pragma unroll
    for (int k = 0; k < (N_PIX / 8 + NW - 1) / NW; ++k) {
        const int it = wave + k * NW;                  // wave-uniform
        if (it < N_PIX / 8) {
            const int P = 8 * it + pl;
            const int py = P / row_px, px = P - py * row_px;
            const int gy = py0 + py, gx = px0 + px;
            const bool in = (P < n_valid) & (gy >= 0) & (gy < H) & (gx >= 0) & (gx < W);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(sr, (stem_lds_void*)(dst + it * 1024), 16, in ? (unsigned)(gy * W + gx) * 128u + 16u * ch : 0xFFFFFF00u,
                                                     0, 0, 0);
        }
    }
}

// conv1 weights as MFMA A operands: rows = output channel 16 nt + c, k = the 4 channel slots of tap 4 s + g
struct W1Frags {
    s16x4 a[2][3];
};
__device__ inline W1Frags load_w1(const void* w1p, int c, int g) {
    W1Frags f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int s = 0; s < 3; ++s)
            f.a[nt][s] = *reinterpret_cast<const s16x4*>(reinterpret_cast<const char*>(w1p) + ((16 * nt + c) * 12 + 4 * s + g) * 8);
    return f;
}

// conv1 for the 16 pixels (py, px0 + c) of a region whose pixel (0, 0) sits at xs[oy][ox] minus one row/column of taps:
// acc[nt][e] = y1[channel 16 nt + 4 g + e][pixel c]
__device__ inline void conv1_group(const char* xs, const W1Frags& w, int py, int px, int oy, int ox, int g, f32x4 (&acc)[2]) {
    acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        int tap = 4 * s + g;
        tap = tap < 9 ? tap : 0;                  // slots 9..11: zero weights, any finite operand
        const int ty = tap / 3, tx = tap - 3 * ty;
        const s16x4 b = *reinterpret_cast<const s16x4*>(xs + ((py + ty + oy) * XC + px + tx + ox) * 8);
        acc[0] = mfma16(w.a[0][s], b, acc[0]);
        acc[1] = mfma16(w.a[1][s], b, acc[1]);
    }
}

// a1 = relu(bn1(conv1 x)) on the tile with halo 1 -> LDS image [612 (+pad) pixels][32 ch] (off64), zero outside the image
__device__ inline void build_a1(const char* xs, const W1Frags& w, const float (&sc)[2][4], const float (&sh)[2][4],
                                const Tile& t, int H, int W, int wave, int c, int g, char* a1s) {
    for (int grp = wave; grp < A_GROUPS; grp += NW) {
        const int P = 16 * grp + c;
        const int Pc = P < A_PIX ? P : A_PIX - 1;
        const int py = Pc / AC, px = Pc - py * AC;
        f32x4 acc[2];
        conv1_group(xs, w, py, px, 0, 0, g, acc);
        const int gy = t.y0 - 1 + py, gx = t.x0 - 1 + px;
        const bool in = (P < A_PIX) && gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float z = fmaxf(__builtin_fmaf(acc[nt][e], sc[nt][e], sh[nt][e]), 0.f);
                v[e] = in ? z : 0.f;
            }
            u32x2 pk = {pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3])};
            const int Pl = ACP == AC ? P : (P / AC) * ACP + (P - (P / AC) * AC);       // pixel index in the image's row pitch
            *reinterpret_cast<u32x2*>(a1s + off64(Pl, 2 * nt + (g >> 1)) + (g & 1) * 8) = pk;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// F1: statistics of y1 = conv1(x) (never stored) and the input autocorrelation XX
// ---------------------------------------------------------------------------------------------
constexpr int PART1 = 2 * C1 + 48 * 48;   // per-wave partial row: sum y1 [32], sum y1^2 [32], XX [48][48]

#if STEM_TH == 8    // dispatched with the 8-row geometry only (pswin_stem_conv1_stats)
__global__ __launch_bounds__(WG, 2) void stem_stats1_kernel(const u64* __restrict__ x4, const void* __restrict__ w1p, int H,
                                                         int W, int nty, int ntx, int ntiles, int want_xx,
                                                         float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) char xs[XS_TOTAL];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const W1Frags w = load_w1(w1p, c, g);
    float s1[2][4], q1[2][4];
    f32x4 xx[3][3];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) s1[nt][e] = q1[nt][e] = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) xx[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const Tile t = tile_of(tile, nty, ntx);
        __syncthreads();
        load_xs(x4, t, H, W, xs);
        __syncthreads();
        // y1 on the tile pixels: group = half a tile row
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int grp = wave * 4 + k;
            const int py = grp >> 1, px = 16 * (grp & 1) + c;
            f32x4 acc[2];
            conv1_group(xs, w, py, px, 1, 1, g, acc);
            const bool in = (t.y0 + py < H) && (t.x0 + px < W);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = in ? acc[nt][e] : 0.f;
                    s1[nt][e] += v;
                    q1[nt][e] = __builtin_fmaf(v, v, q1[nt][e]);
                }
        }
        if (want_xx) {
            // XX += xp^T xp over the valid pixels of tile rows 2 wave, 2 wave + 1 (one 32-pixel contraction step each)
            const int q = c >> 2, p = c & 3;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int y = 2 * wave + k;
                const bool rowin = t.y0 + y < H;
                bf16x8 f[3];
#pragma unroll
                for (int nb = 0; nb < 3; ++nb) {
                    const int tap = 4 * nb + p;
                    const int ty = tap / 3, tx = tap - 3 * ty;
                    const char* lo = tap < 9 ? xs + ((y + ty + 1) * XC + 4 * g + q + tx + 1) * 8 : xs + ZSLOT;
                    const char* hi = tap < 9 ? lo + 16 * 8 : lo;
                    u32x4 raw = __builtin_bit_cast(u32x4, tr_pair(lo, hi));
                    // element r of the lo (hi) half belongs to pixel column 4 g + r (16 + 4 g + r)
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int col = (d >> 1) * 16 + 4 * g + 2 * (d & 1);
                        const bool in0 = rowin && (t.x0 + col < W), in1 = rowin && (t.x0 + col + 1 < W);
                        raw[d] &= (in0 ? 0x0000ffffu : 0u) | (in1 ? 0xffff0000u : 0u);
                    }
                    f[nb] = __builtin_bit_cast(bf16x8, raw);
                }
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) xx[a][b] = mfma32(f[a], f[b], xx[a][b]);
            }
        }
    }
    float* out = partial + ((size_t)blockIdx.x * NW + wave) * PART1;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = row16_sum(s1[nt][e]), b = row16_sum(q1[nt][e]);
            if (c == 0) {
                out[16 * nt + 4 * g + e] = a;
                out[C1 + 16 * nt + 4 * g + e] = b;
            }
        }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) out[2 * C1 + (16 * a + 4 * g + e) * 48 + 16 * b + c] = xx[a][b][e];
}
#endif

// ---------------------------------------------------------------------------------------------
// F2: y2 = conv2(relu(bn1(conv1 x))) + per-channel sum / sum of squares of y2
// ---------------------------------------------------------------------------------------------
constexpr int A1S_BYTES = STEM_TH == 8 ? (AR + 1) * ACP * 64 : A_GROUPS * 16 * 64;     // 39936 (16 rows) / 28160 (8 rows: pitch 40, one spare row for the last group's padding lanes)
constexpr int W2S_BYTES = 9 * C2 * 64;            // 36864
constexpr int PART2 = 2 * C2;

#if STEM_TH == 16   // dispatched with the 16-row geometry only (pswin_stem_conv2_fwd).  Round 4 A/B: the 8-row geometry -- two 4-wave workgroups per CU (63 KB of LDS
                    // each) whose tile phases overlap -- measured 250.3 against 249.1 us: the kernel is bound by its steady state (LDS reads + MFMA issue), not by phases
__global__ __launch_bounds__(WG, 2) void stem_conv2_fwd_kernel(const u64* __restrict__ x4, const void* __restrict__ w1p,
                                                            const float* __restrict__ scale1, const float* __restrict__ shift1,
                                                            const void* __restrict__ w2p, int H, int W, int nty, int ntx,
                                                            int ntiles, void* __restrict__ y2, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) char smem[XS_TOTAL + A1S_BYTES + W2S_BYTES];
    char* xs = smem;
    char* a1s = smem + XS_TOTAL;
    char* w2s = a1s + A1S_BYTES;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const W1Frags w = load_w1(w1p, c, g);
    float sc[2][4], sh[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sc[nt][e] = scale1[16 * nt + 4 * g + e];
            sh[nt][e] = shift1[16 * nt + 4 * g + e];
        }
    // conv2 weights [9][64 out][32 in] -> LDS rows of 64 bytes (row = tap * 64 + out)
    for (int i = threadIdx.x; i < 9 * C2 * 4; i += WG) {
        const int row = i >> 2, ch = i & 3;
        *reinterpret_cast<u32x4*>(w2s + off64(row, ch)) = reinterpret_cast<const u32x4*>(w2p)[i];
    }
    float s2[4][4], q2[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) s2[mt][e] = q2[mt][e] = 0.f;

    // The input pixels of the NEXT tile are requested once conv1 has consumed this tile's (the input tile is dead from there on), fly
    // under the conv2 MFMAs and are written to LDS behind them: with one workgroup per CU the request's round trip (~2 us of a ~7 us
    // tile) was otherwise fully exposed.  (Writing them at the loop top instead made the wait drain the epilogue's stores as well:
    // loop-edge merging of the in-order counter.)
    if ((int)blockIdx.x < ntiles) load_xs(x4, tile_of(blockIdx.x, nty, ntx), H, W, xs);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const Tile t = tile_of(tile, nty, ntx);
        __syncthreads();                       // this tile's input pixels are in LDS; the previous tile's a1 readers are done
        build_a1(xs, w, sc, sh, t, H, W, wave, c, g, a1s);
        __syncthreads();
        XsRegs xnext;
        {
            const int tn = tile + (int)gridDim.x;
            issue_xs(x4, tile_of(tn < ntiles ? tn : tile, nty, ntx), H, W, xnext);       // (past the end: re-request this tile, unused)
        }
        // wave: tile rows 2 wave, 2 wave + 1, both 16-pixel halves; acc[pt][mt][e] = y2[channel 16 mt + 4 g + e][pixel c]
        f32x4 acc[4][4];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[pt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // operand fragments of tap t + 1 are read from LDS under the MFMAs of tap t (explicit double buffer; the
        // scheduling barrier keeps the compiler from serialising read -> wait -> 16 MFMAs per tap)
        bf16x8 fa[2][4], fb[2][4];
        auto read_tap = [&](int tap, bf16x8 (&a)[4], bf16x8 (&b)[4]) {
            const int ty = tap / 3, tx = tap - 3 * ty;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = *reinterpret_cast<const bf16x8*>(w2s + off64(tap * C2 + 16 * mt + c, g));
#pragma unroll
            for (int pt = 0; pt < 4; ++pt) {
                const int r = 2 * wave + (pt >> 1), col = 16 * (pt & 1) + c;
                b[pt] = *reinterpret_cast<const bf16x8*>(a1s + off64((r + ty) * AC + col + tx, g));
            }
        };
        read_tap(0, fa[0], fb[0]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap + 1 < 9) read_tap(tap + 1, fa[(tap + 1) & 1], fb[(tap + 1) & 1]);
#pragma unroll
            for (int pt = 0; pt < 4; ++pt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[pt][mt] = mfma32(fa[tap & 1][mt], fb[tap & 1][pt], acc[pt][mt]);
            __builtin_amdgcn_sched_barrier(0);
        }
        store_xs(xnext, xs);                   // the next tile's input pixels (requested above)
        // epilogue: statistics + bf16 store (8 consecutive channels per lane after the group exchange)
        const rsrc_t ys = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(y2) + (size_t)t.b * H * W * 128, 0,
                                                            (int)((size_t)H * W * 128), 0x00020000);
        // tiles that lie inside the image (all of them when H, W are multiples of the tile) take the statistics as packed f32 pairs
        // (v_pk_add_f32 / v_pk_fma_f32: 64 instructions per wave and tile instead of 192 with the per-value select)
        const bool full = (t.y0 + TH <= H) & (t.x0 + TW <= W);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const int gy = t.y0 + 2 * wave + (pt >> 1), gx = t.x0 + 16 * (pt & 1) + c;
            const bool in = gy < H && gx < W;
            if (full) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    typedef __attribute__((ext_vector_type(2))) float f2;
                    const f2 a0 = {acc[pt][mt][0], acc[pt][mt][1]}, a1 = {acc[pt][mt][2], acc[pt][mt][3]};
                    f2 s0 = {s2[mt][0], s2[mt][1]}, s1 = {s2[mt][2], s2[mt][3]}, q0 = {q2[mt][0], q2[mt][1]}, q1 = {q2[mt][2], q2[mt][3]};
                    s0 = s0 + a0;
                    s1 = s1 + a1;
                    q0 = __builtin_elementwise_fma(a0, a0, q0);
                    q1 = __builtin_elementwise_fma(a1, a1, q1);
                    s2[mt][0] = s0[0]; s2[mt][1] = s0[1]; s2[mt][2] = s1[0]; s2[mt][3] = s1[1];
                    q2[mt][0] = q0[0]; q2[mt][1] = q0[1]; q2[mt][2] = q1[0]; q2[mt][3] = q1[1];
                }
            } else {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = in ? acc[pt][mt][e] : 0.f;
                        s2[mt][e] += v;
                        q2[mt][e] = __builtin_fmaf(v, v, q2[mt][e]);
                    }
            }
            const unsigned poff = in ? (unsigned)(gy * W + gx) * 128u + (unsigned)row8_d0(g) * 2u : 0xFFFFFF00u;
            __builtin_amdgcn_raw_buffer_store_b128(pack_row8(acc[pt][0], acc[pt][1]), ys, poff, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(pack_row8(acc[pt][2], acc[pt][3]), ys, poff + 64u, 0, 0);
        }
    }
    if (partial) {
        float* out = partial + ((size_t)blockIdx.x * NW + wave) * PART2;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = row16_sum(s2[mt][e]), b = row16_sum(q2[mt][e]);
                if (c == 0) {
                    out[16 * mt + 4 * g + e] = a;
                    out[C2 + 16 * mt + 4 * g + e] = b;
                }
            }
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// B4: conv2 weight gradient  dW2[out][tap][in] = sum_p dy2[p][out] * a1[p + tap][in], a1 recomputed from the input.
// wave = (output-channel half mh, 4 tile rows kq); one tile row (32 pixels) per contraction step.
// ---------------------------------------------------------------------------------------------
constexpr int DYS_BYTES = TH * TW * 128;             // 65536
constexpr int WG2_TILES = 2 * 9 * 2;                 // accumulator tiles per wave
constexpr int WG2_OUT = 2 * WG2_TILES * 256;

#if STEM_TH == 8    // dispatched with the 8-row geometry only (pswin_stem_conv2_wgrad); the 16-row instantiation spilled 172 VGPRs and was never launched
// Round 4 (second half): wave = (input-channel tile nt, 4 tile rows kq).  The 18 (tap, input-channel tile) products of a tile row are
// split between the two waves of a row group by input-channel tile, and each wave carries all four output-channel tiles: a transposed a1
// fragment feeds FOUR MFMAs instead of two, and a tile row costs 26 transposed reads instead of 40 for the same 36 MFMAs.  Measured: no
// change (275 us against 272-293 us box to box) -- the per-step LDS latency this removes was not the bound.  The SQ counters
// (profiles/r04_stem_sq_counters.txt) say what is: ~855 VALU instructions per tile and wave (address arithmetic of the tile loads and of
// the swizzled fragment reads, BatchNorm + ReLU + packing in build_a1) = 46 % of the SIMD's issue time next to 38 % for the MFMAs, and
// the waves wait 44 % of their time; with 255 registers nothing tile-invariant can be kept across tiles.
__device__ inline void wgrad_rows(const char* dys, const char* a1s, int nt, int kq, int g, int q, int p, f32x4 (&acc)[4][9]) {
    static_assert(ACP % 8 == 0, "the column-only swizzle needs a row pitch that is a multiple of 8 pixels");
    int xoff[3];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) xoff[tx] = off64(4 * g + q + tx, 2 * nt + (p >> 1)) + (p & 1) * 8;
#pragma unroll 1
    for (int yy = 0; yy < 4; ++yy) {
        const int y = 4 * kq + yy;
        bf16x8 a[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const char* lo = dys + off128(y * TW + 4 * g + q, 2 * mt + (p >> 1)) + (p & 1) * 8;
            a[mt] = tr_pair(lo, lo + 16 * 128);
        }
        // 9 taps: the next tap's transposed a1 fragment is read under this tap's MFMAs.  Address = row term + xoff[tx] (pitch 40: the
        // swizzle depends on the column only)
        auto read_b = [&](int tap) {
            const int ty = tap / 3, tx = tap - 3 * ty;
            const char* lo = a1s + (y + ty) * (ACP * 64) + xoff[tx];
            return tr_pair(lo, lo + 16 * 64);
        };
        bf16x8 bcur = read_b(0);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            bf16x8 bnext = bcur;
            if (tap + 1 < 9) bnext = read_b(tap + 1);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][tap] = mfma32(a[mt], bcur, acc[mt][tap]);
            __builtin_amdgcn_sched_barrier(0);
            bcur = bnext;
        }
    }
}

__global__ __launch_bounds__(WG, 2) void stem_conv2_wgrad_kernel(const u64* __restrict__ x4, const void* __restrict__ w1p,
                                                              const float* __restrict__ scale1, const float* __restrict__ shift1,
                                                              const void* __restrict__ dy2, int H, int W, int nty, int ntx,
                                                              int ntiles, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) char smem[XS_TOTAL + A1S_BYTES + DYS_BYTES];
    char* xs = smem;
    char* a1s = smem + XS_TOTAL;
    char* dys = a1s + A1S_BYTES;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4, q = c >> 2, p = c & 3;
    const int wnt = wave & 1, kq = wave >> 1;
    const W1Frags w = load_w1(w1p, c, g);
    float sc[2][4], sh[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sc[nt][e] = scale1[16 * nt + 4 * g + e];
            sh[nt][e] = shift1[16 * nt + 4 * g + e];
        }
    f32x4 acc[4][9];                                   // [output-channel tile mt][tap], input-channel tile wnt
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const Tile t = tile_of(tile, nty, ntx);
        __syncthreads();
        dma_pix128<TH * TW>(dy2, t.b, H, W, t.y0, t.x0, TW, TH * TW, dys, wave, lane);      // LDS-DMA: no staging registers
        load_xs(x4, t, H, W, xs);
        __syncthreads();
        build_a1(xs, w, sc, sh, t, H, W, wave, c, g, a1s);
        __syncthreads();
        wgrad_rows(dys, a1s, wnt, kq, g, q, p, acc);
    }
    // sum the NW / 2 row-group waves of each input-channel tile through LDS in a fixed order; the last one writes.  Output layout (unchanged):
    // [mh = mt >> 1][mi = mt & 1][tap][nt][e][lane]
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    float* out = partial + (size_t)blockIdx.x * WG2_OUT;
    constexpr int KQ = NW / 2;
    static_assert(WG2_TILES * 256 * 4 <= XS_TOTAL + A1S_BYTES + DYS_BYTES, "reduction buffer must fit the tile buffers");
    for (int half = 0; half < 2; ++half)
        for (int r = 0; r < KQ; ++r) {
            if (wnt == half && kq == r) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        const int obase = (mt >> 1) * WG2_TILES * 256 + ((((mt & 1) * 9 + j) * 2 + half) * 4) * 64 + lane;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int idx = ((mt * 9 + j) * 4 + e) * 64 + lane;
                            float v = acc[mt][j][e];
                            if (r > 0) v += red[idx];
                            if (r < KQ - 1) red[idx] = v; else out[obase + e * 64] = v;
                        }
                    }
            }
            __syncthreads();
        }
}
#endif

#if STEM_TH == 16   // the data-gradient kernel needs 122 KB of LDS: only the 16-row geometry is instantiated
// ---------------------------------------------------------------------------------------------
// B5: conv2 data gradient da1, BN1 backward sums and the conv1 weight-gradient correlation G, g1 never stored:
//   da1[p][in] = sum_tap dy2[p - tap][out] W2[tap][out][in];  g1 = da1 [relu(bn1 y1) > 0] (y1 recomputed);
//   out: sum g1 [32], sum g1 * yhat1 [32], G[32][48] = sum_p g1[p][ch] * xp[p][slot].
// prm: f32 [4][32] = scale1, shift1, a = rstd1, b = -mean1 rstd1.
// ---------------------------------------------------------------------------------------------
constexpr int DYH_BYTES = A_GROUPS * 16 * 128;       // 79872: dy2 tile with halo 1
constexpr int W2T_BYTES = 9 * C1 * 128;              // 36864
constexpr int PART5 = 2 * C1 + C1 * 48;              // 1600

__global__ __launch_bounds__(WG, 2) void stem_conv2_bwd_kernel(const u64* __restrict__ x4, const void* __restrict__ w1p,
                                                            const float* __restrict__ prm, const void* __restrict__ dy2,
                                                            const void* __restrict__ w2t, int H, int W, int nty, int ntx,
                                                            int ntiles, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) char smem[XS_TOTAL + DYH_BYTES + W2T_BYTES + 4 * C1 * 4];
    char* xs = smem;
    char* dyh = smem + XS_TOTAL;
    char* g1s = dyh;                                  // aliases the dy2 tile once the data gradient is done
    char* w2s = dyh + DYH_BYTES;
    float* prs = reinterpret_cast<float*>(w2s + W2T_BYTES);      // scale1, shift1, a, b: read per use (round 4: the 32 registers they held
                                                                 // per lane are what the all-requests-first tile load needs; no spills)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4, q = c >> 2, p = c & 3;
    const W1Frags w = load_w1(w1p, c, g);
    if (threadIdx.x < 4 * C1) prs[threadIdx.x] = prm[threadIdx.x];
    for (int i = threadIdx.x; i < 9 * C1 * 8; i += WG) {       // [9][32 in][64 out] -> rows of 128 bytes
        const int row = i >> 3, ch = i & 7;
        *reinterpret_cast<u32x4*>(w2s + off128(row, ch)) = reinterpret_cast<const u32x4*>(w2t)[i];
    }
    float sg[2][4], sgy[2][4];
    f32x4 gacc[2][3];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sg[nt][e] = sgy[nt][e] = 0.f;
#pragma unroll
        for (int nb = 0; nb < 3; ++nb) gacc[nt][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const Tile t = tile_of(tile, nty, ntx);
        __syncthreads();
        dma_pix128<A_GROUPS * 16>(dy2, t.b, H, W, t.y0 - 1, t.x0 - 1, AC, A_PIX, dyh, wave, lane);   // the whole dy2 tile in flight at once (LDS-DMA)
        load_xs(x4, t, H, W, xs);
        __syncthreads();
        f32x4 acc[4][2];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[pt][0] = acc[pt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        // (tap, k-step) operand fragments double buffered in registers: the next step's LDS reads run under this step's MFMAs
        bf16x8 fa[2][2], fb[2][4];
        auto read_step = [&](int st, bf16x8 (&a)[2], bf16x8 (&bb)[4]) {
            const int tap = st >> 1, s_ = st & 1;
            const int ty = tap / 3, tx = tap - 3 * ty;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const bf16x8*>(w2s + off128(tap * C1 + 16 * mt + c, 4 * s_ + g));
#pragma unroll
            for (int pt = 0; pt < 4; ++pt) {
                const int r = 2 * wave + (pt >> 1), col = 16 * (pt & 1) + c;
                bb[pt] = *reinterpret_cast<const bf16x8*>(dyh + off128((r - ty + 2) * AC + col - tx + 2, 4 * s_ + g));
            }
        };
        read_step(0, fa[0], fb[0]);
#pragma unroll
        for (int st = 0; st < 18; ++st) {
            if (st + 1 < 18) read_step(st + 1, fa[(st + 1) & 1], fb[(st + 1) & 1]);
#pragma unroll
            for (int pt = 0; pt < 4; ++pt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc[pt][mt] = mfma32(fa[st & 1][mt], fb[st & 1][pt], acc[pt][mt]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // mask by the ReLU of the recomputed a1, BN1 backward sums
        u32x2 gp[4][2];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const int r = 2 * wave + (pt >> 1), col = 16 * (pt & 1) + c;
            f32x4 y1[2];
            conv1_group(xs, w, r, col, 1, 1, g, y1);
            const bool in = (t.y0 + r < H) && (t.x0 + col < W);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int ch0 = 16 * nt + 4 * g;
                const f32x4 sc4 = *reinterpret_cast<const f32x4*>(prs + ch0), sh4 = *reinterpret_cast<const f32x4*>(prs + C1 + ch0);
                const f32x4 pa4 = *reinterpret_cast<const f32x4*>(prs + 2 * C1 + ch0), pb4 = *reinterpret_cast<const f32x4*>(prs + 3 * C1 + ch0);
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool on = in && (__builtin_fmaf(y1[nt][e], sc4[e], sh4[e]) > 0.f);
                    const float gg = on ? acc[pt][nt][e] : 0.f;
                    const float yh = __builtin_fmaf(y1[nt][e], pa4[e], pb4[e]);
                    sg[nt][e] += gg;
                    sgy[nt][e] = __builtin_fmaf(gg, yh, sgy[nt][e]);
                    v[e] = gg;
                }
                gp[pt][nt] = u32x2{pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3])};
            }
        }
        __syncthreads();                               // every wave is done with the dy2 tile
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const int pix = (2 * wave + (pt >> 1)) * TW + 16 * (pt & 1) + c;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) *reinterpret_cast<u32x2*>(g1s + off64(pix, 2 * nt + (g >> 1)) + (g & 1) * 8) = gp[pt][nt];
        }
        __builtin_amdgcn_wave_barrier();               // a wave reads back only the two tile rows it wrote
        // G += g1^T xp over tile rows 2 wave, 2 wave + 1
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int y = 2 * wave + k;
            bf16x8 a[2], b[3];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const char* lo = g1s + off64(y * TW + 4 * g + q, 2 * mt + (p >> 1)) + (p & 1) * 8;
                a[mt] = tr_pair(lo, lo + 16 * 64);
            }
#pragma unroll
            for (int nb = 0; nb < 3; ++nb) {
                const int tap = 4 * nb + p;
                const int ty = tap / 3, tx = tap - 3 * ty;
                const char* lo = tap < 9 ? xs + ((y + ty + 1) * XC + 4 * g + q + tx + 1) * 8 : xs + ZSLOT;
                b[nb] = tr_pair(lo, tap < 9 ? lo + 16 * 8 : lo);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nb = 0; nb < 3; ++nb) gacc[mt][nb] = mfma32(a[mt], b[nb], gacc[mt][nb]);
        }
    }
    float* out = partial + ((size_t)blockIdx.x * NW + wave) * PART5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = row16_sum(sg[nt][e]), b = row16_sum(sgy[nt][e]);
            if (c == 0) {
                out[16 * nt + 4 * g + e] = a;
                out[C1 + 16 * nt + 4 * g + e] = b;
            }
        }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nb = 0; nb < 3; ++nb)
#pragma unroll
            for (int e = 0; e < 4; ++e) out[2 * C1 + (16 * mt + 4 * g + e) * 48 + 16 * nb + c] = gacc[mt][nb][e];
}
#endif  // STEM_TH == 16
