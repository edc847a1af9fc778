// fid.hip — the device side of the Frechet Inception Distance (stylex/fid.py, stylex/fid_inception.py; reference
// stylex/stylex_train.py:1577-1622 goes through image files and the pytorch_fid package instead).
//
//   fid_prep_kernel          image batch -> Inception input: the byte an image file would hold, ToTensor's q / 255, the bilinear
//                            resize to 299 x 299 (index rule of resize_norm_fwd_kernel, frozen_ew.hip) and 2 v - 1, one pass
//   fid_prep_u8_kernel       the same from bytes (the output of the JPEG round trip, jpeg_rt.hip)
//   affine_act_slice_kernel  the eval BatchNorm + ReLU tail of frozen_ew.hip with an output batch stride: the last layer of
//                            an Inception branch writes its channel slice of the block's concatenated output (no torch.cat)
//   fid_pool_kernel          f[b][d] = mean over the final map's pixels, fp32, index order (compensated sum)
//   fid_gram_kernel          sum[d] += sum_b f, gram[i][j] += sum_b f_i f_j (i <= j) in fp64 on v_mfma_f64_16x16x4_f64; one wave
//                            owns a 16 x 16 tile: it reads, accumulates and writes it, b ascending — no atomics, same bits
//                            for the same inputs
// This translation unit is built without the SLP vectoriser (Makefile: CXXFLAGS_fid), the rule of torgb.hip: the two rows
// of the bilinear blend are the pattern it pairs into packed fp32 instructions with a crossed operand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

inline unsigned grid_for(unsigned long n) {
    unsigned long b = (n + 255) / 256;
    return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

// ---- image -> Inception input --------------------------------------------------------------------------------------------
struct RsIdx { int i0, i1; float l0, l1; };
// ATen's area_pixel_compute_source_index (align_corners = false), as frozen_ew.hip's rs_index
__device__ __forceinline__ RsIdx rs_index(int dst, float ratio, int in) {
    float src = ratio * (dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    RsIdx r;
    r.i0 = (int)src;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = src - r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

template <bool BF16>
__device__ __forceinline__ float load_px(const void* x, long off) {
    if (BF16) return __uint_as_float((unsigned)static_cast<const unsigned short*>(x)[off] << 16);
    return static_cast<const float*>(x)[off];
}

// save_image's byte and ToTensor's q / 255: stylex_image_quantise (stylex_internal.h, shared with image_metrics.hip)
__device__ __forceinline__ float quantise(float v) { return stylex_image_quantise(v); }

template <bool BF16>
__global__ __launch_bounds__(256) void fid_prep_kernel(const void* __restrict__ x, float* __restrict__ y, int Hi, int Wi, int Ho,
                                                       int Wo, long sb, long sc, long sh, long sw, unsigned total) {
    const float rh = (float)Hi / Ho, rw = (float)Wi / Wo;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int ox = i % Wo, oy = (i / Wo) % Ho, c = (i / (Wo * Ho)) % 3, b = i / (Wo * Ho * 3);
        const RsIdx h = rs_index(oy, rh, Hi), w = rs_index(ox, rw, Wi);
        const long base = b * sb + c * sc;
        const float p00 = quantise(load_px<BF16>(x, base + h.i0 * sh + w.i0 * sw));
        const float p01 = quantise(load_px<BF16>(x, base + h.i0 * sh + w.i1 * sw));
        const float p10 = quantise(load_px<BF16>(x, base + h.i1 * sh + w.i0 * sw));
        const float p11 = quantise(load_px<BF16>(x, base + h.i1 * sh + w.i1 * sw));
        const float r0 = w.l0 * p00 + w.l1 * p01;
        const float r1 = w.l0 * p10 + w.l1 * p11;
        const float v = h.l0 * r0 + h.l1 * r1;
        y[i] = 2.f * v - 1.f;
    }
}

// fid_prep_kernel reading bytes (dense [B][3][Hi][Wi], e.g. a decoded JPEG round trip, jpeg_rt.hip): q / 255 as the same
// true division, the same blend with the same roundings — bit for bit fid_prep_kernel of the fp32 image q / 255
__global__ __launch_bounds__(256) void fid_prep_u8_kernel(const unsigned char* __restrict__ x, float* __restrict__ y, int Hi, int Wi,
                                                          int Ho, int Wo, unsigned total) {
    const float rh = (float)Hi / Ho, rw = (float)Wi / Wo;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int ox = i % Wo, oy = (i / Wo) % Ho, bc = i / (Wo * Ho);
        const RsIdx h = rs_index(oy, rh, Hi), w = rs_index(ox, rw, Wi);
        const unsigned char* p = x + (size_t)bc * Hi * Wi;
        const float p00 = __fdiv_rn((float)p[h.i0 * Wi + w.i0], 255.f);
        const float p01 = __fdiv_rn((float)p[h.i0 * Wi + w.i1], 255.f);
        const float p10 = __fdiv_rn((float)p[h.i1 * Wi + w.i0], 255.f);
        const float p11 = __fdiv_rn((float)p[h.i1 * Wi + w.i1], 255.f);
        // the blend as the compiler contracts fid_prep_kernel's (one fma per sum, the second product rounded on its own),
        // spelled out so that the two kernels cannot drift apart: tests/test_jpeg_gpu.py compares them bit for bit
        {
#pragma clang fp contract(off)
            const float r0 = fmaf(w.l0, p00, w.l1 * p01);
            const float r1 = fmaf(w.l0, p10, w.l1 * p11);
            const float v = fmaf(h.l0, r0, h.l1 * r1);
            y[i] = fmaf(v, 2.f, -1.f);
        }
    }
}

// ---- BatchNorm + ReLU tail into a channel slice ---------------------------------------------------------------------------
// y[b * ybs + j] = act(x[b][j] * s[c] + t[c] (+ r[b][j])), j = c * HW + p: affine_act_fwd_kernel (frozen_ew.hip) with the
// output batch stride `ybs` (elements) in place of C * HW; the same operations in the same order on every element
template <int V>
__global__ __launch_bounds__(256) void affine_act_slice_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                               const float* __restrict__ t, const float* __restrict__ r,
                                                               float* __restrict__ y, unsigned total_v, unsigned HW, unsigned C,
                                                               unsigned CHW, unsigned ybs, int relu) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total_v; i += gridDim.x * 256u) {
        const unsigned e = i * V;
        const unsigned b = e / CHW, j = e - b * CHW;
        const unsigned c = j / HW;
        const float sc = s[c], sh = t[c];
        float v[V], rr[V];
        if (V == 4) {
            *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(x + e);
            if (r) *reinterpret_cast<float4*>(rr) = *reinterpret_cast<const float4*>(r + e);
        } else {
            v[0] = x[e];
            if (r) rr[0] = r[e];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float o = fmaf(v[k], sc, sh);
            if (r) o += rr[k];
            v[k] = relu ? fmaxf(o, 0.f) : o;
        }
        float* yo = y + (size_t)b * ybs + j;
        if (V == 4) *reinterpret_cast<float4*>(yo) = *reinterpret_cast<float4*>(v);
        else yo[0] = v[0];
    }
}

// ---- pooled features and their fp64 moments --------------------------------------------------------------------------------
// f[r] = (x[r][0] + x[r][1] + ... + x[r][HW - 1]) / HW, r = b * D + d; one row per thread, added in index order with a
// compensation term (Kahan): a plain fp32 running sum of a 36 x 36 map of same-signed values was 1.7e-6 off per feature,
// 13 x the error of the network in front of it; compensated, the sum is good to an ulp or two whatever HW is.  (No
// fast-math in this build: the compiler keeps the four operations as written.)
__device__ __forceinline__ void kahan_add(float v, float& acc, float& comp) {
    const float y = v - comp;
    const float t = acc + y;
    comp = (t - acc) - y;
    acc = t;
}

__global__ __launch_bounds__(256) void fid_pool_kernel(const float* __restrict__ x, float* __restrict__ f, unsigned rows, unsigned HW) {
    for (unsigned r = blockIdx.x * 256u + threadIdx.x; r < rows; r += gridDim.x * 256u) {
        const float* p = x + (size_t)r * HW;
        float acc = 0.f, comp = 0.f;
        if (HW % 4 == 0) {
            for (unsigned k = 0; k < HW; k += 4) {
                const float4 q = *reinterpret_cast<const float4*>(p + k);
                kahan_add(q.x, acc, comp);
                kahan_add(q.y, acc, comp);
                kahan_add(q.z, acc, comp);
                kahan_add(q.w, acc, comp);
            }
        } else {
            for (unsigned k = 0; k < HW; ++k) kahan_add(p[k], acc, comp);
        }
        f[r] = acc / (float)HW;
    }
}

typedef double double4_t __attribute__((ext_vector_type(4)));

// Tile t of the upper triangle (row-major over 16 x 16 tiles, T tiles per side) -> (ti, tj), ti <= tj
__device__ __forceinline__ void tile_of(unsigned t, unsigned T, unsigned* ti, unsigned* tj) {
    unsigned row = 0, len = T;
    while (t >= len) {
        t -= len;
        --len;
        ++row;
    }
    *ti = row;
    *tj = row + t;
}

// One wave per tile.  v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one f64
// each; result register g of lane l is C[row (l >> 4) + 4 g][col l & 15].  Here A[i][k] = f[b0 + k][i0 + i] and
// B[k][j] = f[b0 + k][j0 + j], rows past B are zero.  A diagonal tile keeps its elements below the diagonal to itself
// (neither read nor written) and also owns sum[i0 .. i0 + 15]: every lane adds the features it loads for A (b = k mod 4),
// the four partial sums are combined in the order ((k0 + k1) + (k2 + k3)).
__global__ __launch_bounds__(256) void fid_gram_kernel(const float* __restrict__ f, double* __restrict__ sum,
                                                       double* __restrict__ gram, unsigned B, unsigned D, unsigned tiles) {
    const unsigned t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= tiles) return;  // whole waves leave: every MFMA below runs with all 64 lanes
    const unsigned lane = threadIdx.x & 63u, col = lane & 15u, k = lane >> 4;
    unsigned ti, tj;
    tile_of(t, D / 16u, &ti, &tj);
    const unsigned i0 = ti * 16u, j0 = tj * 16u;
    const bool diag = ti == tj;
    double4_t acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const unsigned row = k + 4u * g;
        acc[g] = (!diag || row <= col) ? gram[(size_t)(i0 + row) * D + j0 + col] : 0.0;
    }
    double part = 0.0;
    for (unsigned b0 = 0; b0 < B; b0 += 4u) {
        const unsigned b = b0 + k;
        double a = 0.0, bb = 0.0;
        if (b < B) {
            a = (double)f[(size_t)b * D + i0 + col];
            bb = (double)f[(size_t)b * D + j0 + col];
        }
        part += a;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const unsigned row = k + 4u * g;
        if (!diag || row <= col) gram[(size_t)(i0 + row) * D + j0 + col] = acc[g];
    }
    if (diag) {
        const double p0 = __shfl(part, (int)col, 64), p1 = __shfl(part, (int)col + 16, 64);
        const double p2 = __shfl(part, (int)col + 32, 64), p3 = __shfl(part, (int)col + 48, 64);
        if (lane < 16u) sum[i0 + col] += (p0 + p1) + (p2 + p3);
    }
}

inline bool misaligned16(const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) != 0;
}

}  // namespace

extern "C" {

int stylex_fid_prep(const void* x, float* y, const int64_t* sh, const int64_t* strides, int x_is_bf16, void* stream) {
    // sh = {B, Hi, Wi, Ho, Wo}; strides = element strides of x (b, c, h, w), channels 0..2 are read; y dense [B][3][Ho][Wo]
    if (!x || !y || !sh || !strides) return STYLEX_EINVAL;
    for (int k = 0; k < 5; ++k)
        if (sh[k] < 1 || sh[k] > 0x7fffffffLL) return STYLEX_EINVAL;
    int64_t last = 0;  // the largest element offset that is read
    const int64_t ext[4] = {sh[0], 3, sh[1], sh[2]};
    for (int k = 0; k < 4; ++k) {
        if (strides[k] < 0 || strides[k] > 0x7fffffffLL) return STYLEX_EINVAL;
        last += (ext[k] - 1) * strides[k];
    }
    const int64_t total = sh[0] * 3 * sh[3] * sh[4];
    if (total > 0x7fffffffLL || last > 0x7fffffffLL) return STYLEX_EINVAL;
    if (x_is_bf16)
        hipLaunchKernelGGL(fid_prep_kernel<true>, dim3(grid_for((unsigned long)total)), dim3(256), 0, (hipStream_t)stream, x, y,
                           (int)sh[1], (int)sh[2], (int)sh[3], (int)sh[4], (long)strides[0], (long)strides[1], (long)strides[2],
                           (long)strides[3], (unsigned)total);
    else
        hipLaunchKernelGGL(fid_prep_kernel<false>, dim3(grid_for((unsigned long)total)), dim3(256), 0, (hipStream_t)stream, x, y,
                           (int)sh[1], (int)sh[2], (int)sh[3], (int)sh[4], (long)strides[0], (long)strides[1], (long)strides[2],
                           (long)strides[3], (unsigned)total);
    return (int)hipGetLastError();
}

int stylex_fid_prep_u8(const unsigned char* x_u8, float* y, const int64_t* sh, void* stream) {
    // sh = {B, Hi, Wi, Ho, Wo}; x_u8 dense [B][3][Hi][Wi]; y dense [B][3][Ho][Wo]
    if (!x_u8 || !y || !sh) return STYLEX_EINVAL;
    for (int k = 0; k < 5; ++k)
        if (sh[k] < 1 || sh[k] > 0x7fffffffLL) return STYLEX_EINVAL;
    const int64_t total = sh[0] * 3 * sh[3] * sh[4];
    if (total > 0x7fffffffLL || sh[0] * 3 * sh[1] * sh[2] > 0x7fffffffLL) return STYLEX_EINVAL;
    hipLaunchKernelGGL(fid_prep_u8_kernel, dim3(grid_for((unsigned long)total)), dim3(256), 0, (hipStream_t)stream, x_u8, y, (int)sh[1],
                       (int)sh[2], (int)sh[3], (int)sh[4], (unsigned)total);
    return (int)hipGetLastError();
}

int stylex_affine_act_nchw_slice_fwd(const float* x, const float* scale, const float* shift, const float* residual, float* y,
                                     int64_t B, int64_t C, int64_t HW, int64_t y_batch_stride, int relu, void* stream) {
    if (!x || !scale || !shift || !y || B < 1 || C < 1 || HW < 1 || B * C * HW > 0x7fffffffLL) return STYLEX_EINVAL;
    if (y_batch_stride < C * HW || B * y_batch_stride > 0x7fffffffLL) return STYLEX_EINVAL;
    const unsigned long total = (unsigned long)(B * C * HW);
    const bool v4 = HW % 4 == 0 && y_batch_stride % 4 == 0 && !misaligned16(x, y, residual);
    if (v4)
        hipLaunchKernelGGL(affine_act_slice_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, x, scale, shift,
                           residual, y, (unsigned)(total / 4), (unsigned)HW, (unsigned)C, (unsigned)(C * HW),
                           (unsigned)y_batch_stride, relu);
    else
        hipLaunchKernelGGL(affine_act_slice_kernel<1>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, scale, shift,
                           residual, y, (unsigned)total, (unsigned)HW, (unsigned)C, (unsigned)(C * HW), (unsigned)y_batch_stride,
                           relu);
    return (int)hipGetLastError();
}

int stylex_fid_moments_acc(const float* x, float* feat, double* sum, double* gram, int64_t B, int64_t D, int64_t HW, void* stream) {
    if (!x || !sum || !gram || B < 1 || D < 16 || D % 16 || HW < 1 || B * D * HW > 0x7fffffffLL || D > 32768) return STYLEX_EINVAL;
    if (!feat && HW != 1) return STYLEX_EINVAL;  // the pooled features need a home; a [B][D] map is its own
    if ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(gram)) & 7) return STYLEX_EINVAL;
    if (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15)) return STYLEX_EINVAL;
    const float* f = x;
    if (feat) {
        hipLaunchKernelGGL(fid_pool_kernel, dim3(grid_for((unsigned long)(B * D))), dim3(256), 0, (hipStream_t)stream, x, feat,
                           (unsigned)(B * D), (unsigned)HW);
        f = feat;
    }
    const int64_t T = D / 16, tiles = T * (T + 1) / 2;
    hipLaunchKernelGGL(fid_gram_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, f, sum, gram,
                       (unsigned)B, (unsigned)D, (unsigned)tiles);
    return (int)hipGetLastError();
}

}  // extern "C"
