// Shared device/host helpers for libpswin_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "pswin.h"

#define PSWIN_CHECK_ARG(cond) \
    do {                      \
        if (!(cond)) return PSWIN_ERR_ARG; \
    } while (0)

#define PSWIN_LAUNCH_RET()                              \
    do {                                                \
        hipError_t e__ = hipGetLastError();             \
        return e__ == hipSuccess ? PSWIN_OK : (int)e__; \
    } while (0)

namespace pswin {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

__host__ __device__ inline int ceil_to(int v, int m) { return (v + m - 1) / m * m; }

__device__ inline float bf16_bits_to_f32(unsigned short b) {
    return __builtin_bit_cast(float, (unsigned int)b << 16);
}
// round-to-nearest-even f32 -> bf16 (hipcc lowers the cast to v_cvt_pk_bf16_f32 on gfx950, NaN-preserving)
__device__ inline unsigned short f32_to_bf16_bits(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(unsigned short, b);
}
// two f32 -> one dword of two bf16 (lo in bits 0-15) with ONE v_cvt_pk_bf16_f32: `f32_to_bf16_bits(lo) | f32_to_bf16_bits(hi) << 16`
// compiles to two conversions, a shift and an or (seen in the ISA of every kernel that packed its outputs that way)
typedef __attribute__((ext_vector_type(2))) float pswin_f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 pswin_bf16x2_t;
__device__ inline unsigned int pack2_bf16(float lo, float hi) {
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(pswin_f32x2_t{lo, hi}, pswin_bf16x2_t));
}

// 4 consecutive elements of a row, as f32, from an f32 or bf16 buffer
template <int DT>
__device__ inline f32x4 load4(const void* base, size_t elem_off) {
    if constexpr (DT == PSWIN_F32) {
        return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + elem_off);
    } else {
        u32x2 raw = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(base) + elem_off);
        f32x4 r;
        r[0] = __builtin_bit_cast(float, raw[0] << 16);
        r[1] = __builtin_bit_cast(float, raw[0] & 0xffff0000u);
        r[2] = __builtin_bit_cast(float, raw[1] << 16);
        r[3] = __builtin_bit_cast(float, raw[1] & 0xffff0000u);
        return r;
    }
}

template <int DT>
__device__ inline void store4(void* base, size_t elem_off, f32x4 v) {
    if constexpr (DT == PSWIN_F32) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(base) + elem_off) = v;
    } else {
        u32x2 raw;
        raw[0] = pack2_bf16(v[0], v[1]);
        raw[1] = pack2_bf16(v[2], v[3]);
        *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(base) + elem_off) = raw;
    }
}

// One 16-byte channel group of a row as f32: 8 bf16 or 4 f32 elements
template <int DT>
struct Vec {
    static constexpr int VE = (DT == PSWIN_BF16) ? 8 : 4;
};

template <int DT>
__device__ inline void load_vec(const void* base, size_t elem_off, float (&v)[Vec<DT>::VE]) {
    if constexpr (DT == PSWIN_BF16) {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(base) + elem_off);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] = __builtin_bit_cast(float, raw[e] << 16);
            v[2 * e + 1] = __builtin_bit_cast(float, raw[e] & 0xffff0000u);
        }
    } else {
        const f32x4 r = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + elem_off);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e];
    }
}

template <int DT>
__device__ inline void store_vec(void* base, size_t elem_off, const float (&v)[Vec<DT>::VE]) {
    if constexpr (DT == PSWIN_BF16) {
        u32x4 raw;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            raw[e] = pack2_bf16(v[2 * e], v[2 * e + 1]);
        *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(base) + elem_off) = raw;
    } else {
        f32x4 r = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(base) + elem_off) = r;
    }
}

// v_mfma_f32_16x16x32_bf16 on 8-element bf16 operand fragments (or their 4 packed dwords)
__device__ inline f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ inline f32x4 mfma32(u32x4 a, u32x4 b, f32x4 c) {
    return mfma32(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c);
}

// v plus the value of the lane that DPP control CTRL selects within its 16-lane row: one v_add_f32 with a DPP modifier
template <int CTRL>
__device__ inline float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ inline float row16_sum(float v) {   // across the 16 lanes of a group (every lane gets the sum)
    v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);   // row_half_mirror: the other quad of the 8 (all 4 lanes of a quad agree by now)
    return dpp_add<0x140>(v);   // row_mirror: the other half of the 16
}

// v_permlane16_swap: exchanges the odd 16-lane rows of a with the even rows of b.  The builtin (not inline asm) so that
// the compiler's hazard recognizer sees the instruction: its operands often come straight from MFMA accumulators, and
// the MFMA-write -> VALU-read wait states are software managed (an asm version with a fixed s_nop read stale values).
__device__ inline void swap16_u32(unsigned& a, unsigned& b) {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}

// Rows of two 16-wide MFMA tiles.  Lane (c, g) holds, for one row, the accumulator quads q0 = col[4g..4g+3] and
// q1 = col[16+4g..16+4g+3] of a 32-column group.  Exchanging q1 of the even groups with q0 of the odd ones (lanes 16 apart)
// leaves every lane with 8 CONTIGUOUS columns starting at row8_d0(g): one 16-byte row store instead of two 8-byte ones.
__device__ inline int row8_d0(int g) { return 8 * (g >> 1) + 16 * (g & 1); }
// the two quads as the 8-element operand fragment {q0[0..3], q1[0..3]} of bf16 pairs
__device__ inline u32x4 pack8(f32x4 q0, f32x4 q1) {
    return u32x4{pack2_bf16(q0[0], q0[1]), pack2_bf16(q0[2], q0[3]), pack2_bf16(q1[0], q1[1]), pack2_bf16(q1[2], q1[3])};
}
// a packed fragment -> this lane's 8 contiguous columns
__device__ inline u32x4 row8(u32x4 f) {
    const auto r0 = __builtin_amdgcn_permlane16_swap(f[0], f[2], false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(f[1], f[3], false, false);
    return u32x4{r0[0], r1[0], r0[1], r1[1]};
}
__device__ inline u32x4 pack_row8(f32x4 q0, f32x4 q1) { return row8(pack8(q0, q1)); }
// the same exchange on f32 quads.  Whole-vector bit casts only: hipcc (ROCm 7.2) folds __builtin_bit_cast(T, vec[e])
// inside an unrolled loop to element 0.
__device__ inline void exchange_row8(f32x4& q0, f32x4& q1) {
    const u32x4 a = __builtin_bit_cast(u32x4, q0), b = __builtin_bit_cast(u32x4, q1);
    const auto r0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
    const auto r2 = __builtin_amdgcn_permlane16_swap(a[2], b[2], false, false);
    const auto r3 = __builtin_amdgcn_permlane16_swap(a[3], b[3], false, false);
    q0 = __builtin_bit_cast(f32x4, u32x4{r0[0], r1[0], r2[0], r3[0]});
    q1 = __builtin_bit_cast(f32x4, u32x4{r0[1], r1[1], r2[1], r3[1]});
}

// Sample liveness (per-sample DropPath): a block branch's factor vector `sample_scale` (f32 [B], B <= 64) with rows_per_sample rows per
// sample, sample-major.  Sample b is DEAD iff sample_scale[b] == 0.0f: its branch output is multiplied by zero and every gradient
// that flows into the branch for it is an exact zero, so kernels may leave its rows out.  Everything below is wave-uniform (one lane
// per sample, one ballot): bit b of the mask = sample b is live.
constexpr int LIVE_SAMPLES_MAX = 64;
__device__ inline unsigned long long live_sample_mask(const float* __restrict__ sample_scale, int B) {
    const int lane = threadIdx.x & 63;
    const float s = lane < B ? sample_scale[lane] : 0.f;
    return __ballot(s != 0.0f);
}
__device__ inline unsigned long long dead_sample_mask(unsigned long long live, int B) {
    return ~live & (B >= 64 ? ~0ull : (1ull << B) - 1ull);
}
__device__ inline int sample_count(unsigned long long mask) { return __builtin_popcountll(mask); }
// the k-th (from 0) sample of `mask` in ascending order; k < sample_count(mask)
__device__ inline int kth_sample(unsigned long long mask, int k) {
    const int lane = threadIdx.x & 63;
    const bool hit = ((mask >> lane) & 1ull) && __builtin_popcountll(mask & ((1ull << lane) - 1ull)) == k;
    return __builtin_ctzll(__ballot(hit));
}

// out[c] = sum_r part[r][c] (r in fixed order: bitwise reproducible).  16 columns x 64 row lanes per block, so that
// even 512 partial rows are only 8 (independent) loads deep per thread: this stage is pure latency.
__global__ static void colsum_kernel(const float* __restrict__ part, int R, int N, float* __restrict__ out) {
    __shared__ float red[64][16];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < N) {
        int r = rl;
        for (; r + 192 < R; r += 256) {
            s0 += part[(size_t)r * N + c];
            s1 += part[(size_t)(r + 64) * N + c];
            s2 += part[(size_t)(r + 128) * N + c];
            s3 += part[(size_t)(r + 192) * N + c];
        }
        for (; r < R; r += 64) s0 += part[(size_t)r * N + c];
    }
    red[rl][cl] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (rl < 16) {      // 16 x 16 threads finish: thread (rl, cl) sums rows rl, rl+16, rl+32, rl+48, then a 16-lane tree
        float s = (red[rl][cl] + red[rl + 16][cl]) + (red[rl + 32][cl] + red[rl + 48][cl]);
        red[rl][cl] = s;
    }
    __syncthreads();
    if (rl == 0 && c < N) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[k][cl];
        out[c] = s;
    }
}

inline void launch_colsum(const float* part, int R, int N, float* out, hipStream_t st) {
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 15) / 16), dim3(1024), 0, st, part, R, N, out);
}

// Opt a kernel in to `bytes` of dynamic LDS (> 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize) on the CURRENT device.
// The attribute is per device, so the "already done" memo is a bit per device ordinal (lock-free; setting it twice is harmless);
// a failure is returned to the caller instead of surfacing later as an unexplained launch error.
inline int ensure_dynamic_lds(const void* kernel, size_t bytes, std::atomic<unsigned long long>& done) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    const bool memo = dev >= 0 && dev < 64;
    const unsigned long long bit = memo ? 1ull << dev : 0ull;
    if (memo && (done.load(std::memory_order_acquire) & bit)) return PSWIN_OK;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    if (memo) done.fetch_or(bit, std::memory_order_release);
    return PSWIN_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool valid_dtype(int dt) { return dt == PSWIN_F32 || dt == PSWIN_BF16; }

// f(std::integral_constant a, std::integral_constant b) for two dtypes that passed valid_dtype
template <typename F>
inline int dispatch2(int a, int b, F&& f) {
    if (a == PSWIN_F32 && b == PSWIN_F32) return f(std::integral_constant<int, PSWIN_F32>(), std::integral_constant<int, PSWIN_F32>());
    if (a == PSWIN_F32 && b == PSWIN_BF16) return f(std::integral_constant<int, PSWIN_F32>(), std::integral_constant<int, PSWIN_BF16>());
    if (a == PSWIN_BF16 && b == PSWIN_F32) return f(std::integral_constant<int, PSWIN_BF16>(), std::integral_constant<int, PSWIN_F32>());
    return f(std::integral_constant<int, PSWIN_BF16>(), std::integral_constant<int, PSWIN_BF16>());
}

}  // namespace pswin
