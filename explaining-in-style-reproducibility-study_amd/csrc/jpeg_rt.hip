// jpeg_rt.hip — the lossy part of a baseline JPEG round trip on the device: the bytes libjpeg-turbo decodes
// from the file it wrote of an image batch at quality q (4:2:0, standard tables, JDCT_ISLOW, fancy upsampling), without
// the entropy coder, which is lossless.  The reference saves every generated image of calculate_fid as such a file
// (stylex_train.py:1578-1622, image_extension = jpg) and pytorch_fid decodes it.  Integer arithmetic throughout, 32 bits.
//
//   jpeg_codec_kernel      one wave per 16 x 16 MCU: reads the pixels once (clamped at the ragged edges: the encoder's edge
//                          replication), save_image's byte, RGB -> YCbCr, 2 x 2 chroma downsampling, then for the MCU's six
//                          8 x 8 blocks (one lane per 8-point line, 48 of 64 lanes) jfdctint rows | columns, quantisation,
//                          dequantisation, jidctint columns (these four in registers of the lane that owns the column) |
//                          rows.  Writes the decoded Y plane and the two decoded chroma planes, padded to whole MCUs, to
//                          the workspace
//   jpeg_upsample_rgb_kernel  h2v2 fancy upsampling (one chroma sample of halo across MCUs: hence the second launch) and
//                          YCbCr -> RGB; four pixels of a row per thread
// No atomics, no scratch, no data-dependent order: the same input gives the same bytes.  Built without the SLP vectoriser
// (Makefile: CXXFLAGS_jpeg_rt) like fid.hip: the byte of step 1 is two fp32 roundings per channel, three channels in a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

constexpr int FIX16(double v) { return (int)(v * 65536.0 + 0.5); }

// jfdctint.c / jidctint.c, CONST_BITS = 13, PASS1_BITS = 2
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

template <int N>
__device__ __forceinline__ int descale(int x) {
    return (x + (1 << (N - 1))) >> N;
}

// one 8-point forward transform; FIRST: the row pass (results scaled up by 4), else the column pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int N = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale<2>(t10 + t11);
    d[4] = FIRST ? (t10 - t11) * 4 : descale<2>(t10 - t11);
    const int z1 = (t12 + t13) * F_0_541;
    d[2] = descale<N>(z1 + t13 * F_0_765);
    d[6] = descale<N>(z1 - t12 * F_1_847);
    const int z5 = (t4 + t6 + t5 + t7) * F_1_175;
    const int y1 = -(t4 + t7) * F_0_899, y2 = -(t5 + t6) * F_2_562;
    const int y3 = -(t4 + t6) * F_1_961 + z5, y4 = -(t5 + t7) * F_0_390 + z5;
    d[7] = descale<N>(t4 * F_0_298 + y1 + y3);
    d[5] = descale<N>(t5 * F_2_053 + y2 + y4);
    d[3] = descale<N>(t6 * F_3_072 + y2 + y3);
    d[1] = descale<N>(t7 * F_1_501 + y1 + y4);
}

// one 8-point inverse transform, results descaled by N bits (11: the column pass, 18: the row pass)
template <int N>
__device__ __forceinline__ void idct8(int (&c)[8]) {
    const int z1 = (c[2] + c[6]) * F_0_541;
    const int e2 = z1 - c[6] * F_1_847, e3 = z1 + c[2] * F_0_765;
    const int e0 = (c[0] + c[4]) * 8192, e1 = (c[0] - c[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    const int o0 = c[7], o1 = c[5], o2 = c[3], o3 = c[1];
    const int z5 = (o0 + o2 + o1 + o3) * F_1_175;
    const int y1 = -(o0 + o3) * F_0_899, y2 = -(o1 + o2) * F_2_562;
    const int y3 = -(o0 + o2) * F_1_961 + z5, y4 = -(o1 + o3) * F_0_390 + z5;
    const int t0 = o0 * F_0_298 + y1 + y3, t1 = o1 * F_2_053 + y2 + y4;
    const int t2 = o2 * F_3_072 + y2 + y3, t3 = o3 * F_1_501 + y1 + y4;
    c[0] = descale<N>(t10 + t3);
    c[7] = descale<N>(t10 - t3);
    c[1] = descale<N>(t11 + t2);
    c[6] = descale<N>(t11 - t2);
    c[2] = descale<N>(t12 + t1);
    c[5] = descale<N>(t12 - t1);
    c[3] = descale<N>(t13 + t0);
    c[4] = descale<N>(t13 - t0);
}

// The quantisation tables of one quality (natural order; [0] luminance, [1] chrominance) and, per entry, the reciprocal
// m = floor(2^27 / d) + 1 of the divisor d = 8 q: for 0 <= n < 2^16 and d <= 2040, floor(n / d) = (n m) >> 27 exactly,
// because the excess e = m d - 2^27 <= d satisfies e n < 2^27 (make_tables checks it per entry).
struct JpegTables {
    unsigned short q[2][64];
    unsigned rcp[2][64];
};

template <bool BF16>
__device__ __forceinline__ float load_px(const void* x, long off) {
    if (BF16) return __uint_as_float((unsigned)static_cast<const unsigned short*>(x)[off] << 16);
    return static_cast<const float*>(x)[off];
}

// save_image's byte: x * 255 + 0.5 clamped to [0, 255], truncated.  Two roundings, as torch's mul(255).add_(0.5): contraction
// is switched off for these two operations (__fadd_rn(__fmul_rn(v, 255), 0.5) is fused into one fma like any a * b + c)
__device__ __forceinline__ int to_byte(float v) {
#pragma clang fp contract(off)
    const float p = v * 255.f;
    const float t = p + 0.5f;
    return (int)floorf(fminf(fmaxf(t, 0.f), 255.f));
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

constexpr int ROW = 9;         // LDS row stride of an 8 x 8 block in ints: rows and columns both spread over the banks
constexpr int BLK = 8 * ROW;   // block stride

// Workspace of one image: the decoded Y plane [Hm][Wm], then Cb and Cr [Hm / 2][Wm / 2], bytes (Hm, Wm: H, W rounded up
// to whole MCUs, so every 8-byte row of a block lies inside it and is 8-byte aligned)
template <bool BF16>
__global__ __launch_bounds__(64) void jpeg_codec_kernel(const void* __restrict__ x, unsigned char* __restrict__ ws, int H, int W,
                                                        int mcu_rows, int mcu_cols, long sb, long sc, long sh, long sw,
                                                        JpegTables tab) {
    __shared__ int blk[6 * BLK];          // Y00 Y01 Y10 Y11 Cb Cr, samples - 128, then the transform workspace
    __shared__ int full[2][16][17];       // Cb, Cr at full resolution
    const int lane = threadIdx.x;
    const int mx = blockIdx.x % mcu_cols, my = (blockIdx.x / mcu_cols) % mcu_rows, b = blockIdx.x / (mcu_cols * mcu_rows);
    const int x0 = mx * 16, y0 = my * 16;

    // steps 1-3: bytes, colour conversion; a pixel past the right or bottom edge is the edge pixel (edge replication)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = (lane >> 4) + 4 * k, col = lane & 15;
        const int gy = min(y0 + row, H - 1), gx = min(x0 + col, W - 1);
        const long off = b * sb + gy * sh + gx * sw;
        const int r = to_byte(load_px<BF16>(x, off)), g = to_byte(load_px<BF16>(x, off + sc)),
                  bl = to_byte(load_px<BF16>(x, off + 2 * sc));
        const int yy = (FIX16(.299) * r + FIX16(.587) * g + FIX16(.114) * bl + 32768) >> 16;
        const int cb = (-FIX16(.16874) * r - FIX16(.33126) * g + FIX16(.5) * bl + (128 << 16) + 32767) >> 16;
        const int cr = (FIX16(.5) * r - FIX16(.41869) * g - FIX16(.08131) * bl + (128 << 16) + 32767) >> 16;
        blk[((row >> 3) * 2 + (col >> 3)) * BLK + (row & 7) * ROW + (col & 7)] = yy - 128;
        full[0][row][col] = cb;
        full[1][row][col] = cr;
    }
    __syncthreads();
    // step 4: 2 x 2 downsampling.  Input rows are replicated to an even height only (the clamp above does that), and the
    // last DOWNSAMPLED row fills the rest of the MCU: rows past the chroma plane's last row repeat that row.
    {
        const int last = ((H + 1) >> 1) - 1 - my * 8;  // the plane's last row, MCU-local (>= 0: the MCU holds image rows)
        const int lr = lane >> 3, lc = lane & 7, sr = 2 * min(lr, last);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int s = full[c][sr][2 * lc] + full[c][sr][2 * lc + 1] + full[c][sr + 1][2 * lc] + full[c][sr + 1][2 * lc + 1];
            blk[(4 + c) * BLK + lr * ROW + lc] = ((s + 1 + (lc & 1)) >> 2) - 128;
        }
    }
    __syncthreads();
    const int bi = lane >> 3, li = lane & 7;  // this lane's block and line (lanes 48..63 have none)
    int d[8];
    // step 5, rows
    if (lane < 48) {
        int* p = blk + bi * BLK + li * ROW;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        fdct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = d[k];
    }
    __syncthreads();
    // step 5 columns, steps 6 and 7 columns: the lane keeps its column
    if (lane < 48) {
        int* p = blk + bi * BLK + li;
        const int comp = bi >> 2;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k * ROW];
        fdct8<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = tab.q[comp][k * 8 + li];
            const unsigned m = tab.rcp[comp][k * 8 + li];
            const unsigned n = (unsigned)(d[k] < 0 ? -d[k] : d[k]) + 4u * q;  // |c| + (d >> 1), d = 8 q
            const int lvl = (int)__umulhi(n << 5, m);                        // (n m) >> 27 = floor(n / (8 q))
            d[k] = (d[k] < 0 ? -lvl : lvl) * q;
        }
        idct8<11>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k * ROW] = d[k];
    }
    __syncthreads();
    // step 7 rows, + 128, clamp; one 8-byte store per line
    if (lane < 48) {
        const int* p = blk + bi * BLK + li * ROW;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        idct8<18>(d);
        uint2 o;
        o.x = clamp255(d[0] + 128) | clamp255(d[1] + 128) << 8 | clamp255(d[2] + 128) << 16 | clamp255(d[3] + 128) << 24;
        o.y = clamp255(d[4] + 128) | clamp255(d[5] + 128) << 8 | clamp255(d[6] + 128) << 16 | clamp255(d[7] + 128) << 24;
        const size_t Wm = (size_t)mcu_cols * 16, Hm = (size_t)mcu_rows * 16;
        unsigned char* img = ws + (size_t)b * (Hm * Wm + Hm * Wm / 2);
        unsigned char* dst;
        if (bi < 4) dst = img + ((size_t)y0 + (bi >> 1) * 8 + li) * Wm + x0 + (bi & 1) * 8;
        else dst = img + Hm * Wm + (bi - 4) * (Hm * Wm / 4) + ((size_t)my * 8 + li) * (Wm / 2) + mx * 8;
        *reinterpret_cast<uint2*>(dst) = o;
    }
}

// steps 8 and 9.  Thread i: pixels x = 4 xq .. 4 xq + 3 of row y of image b; the chroma columns it needs are
// 2 xq - 1 .. 2 xq + 2, rows y >> 1 and the one above (even y) or below (odd y), all clamped to the ceil(H / 2) x ceil(W / 2)
// plane.  VEC4: W % 4 == 0 and an aligned output, one 4-byte store per channel; else byte stores guarded by x < W.
template <bool VEC4>
__global__ __launch_bounds__(256) void jpeg_upsample_rgb_kernel(const unsigned char* __restrict__ ws, unsigned char* __restrict__ y,
                                                                int H, int W, int mcu_rows, int mcu_cols, unsigned total) {
    const int Wq = (W + 3) >> 2, CH = (H + 1) >> 1, CW = (W + 1) >> 1;
    const size_t Wm = (size_t)mcu_cols * 16, Hm = (size_t)mcu_rows * 16;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int xq = i % Wq, yy = (i / Wq) % H, b = i / ((unsigned)Wq * H);
        const unsigned char* img = ws + (size_t)b * (Hm * Wm + Hm * Wm / 2);
        const int cy = yy >> 1, fy = (yy & 1) ? min(cy + 1, CH - 1) : max(cy - 1, 0);
        int cx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cx[j] = min(max(2 * xq - 1 + j, 0), CW - 1);
        int px[2][4];  // Cb, Cr - 128 of the four pixels
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const unsigned char* pl = img + Hm * Wm + c * (Hm * Wm / 4);
            const unsigned char* nr = pl + (size_t)cy * (Wm / 2);
            const unsigned char* fr = pl + (size_t)fy * (Wm / 2);
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = 3 * nr[cx[j]] + fr[cx[j]];
            px[c][0] = ((3 * v[1] + v[0] + 8) >> 4) - 128;
            px[c][1] = ((3 * v[1] + v[2] + 7) >> 4) - 128;
            px[c][2] = ((3 * v[2] + v[1] + 8) >> 4) - 128;
            px[c][3] = ((3 * v[2] + v[3] + 7) >> 4) - 128;
        }
        const unsigned lum = *reinterpret_cast<const unsigned*>(img + (size_t)yy * Wm + 4 * xq);  // inside the padded plane
        unsigned out[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = (lum >> (8 * j)) & 255, cb = px[0][j], cr = px[1][j];
            const int r = clamp255(l + ((FIX16(1.402) * cr + 32768) >> 16));
            const int g = clamp255(l + ((-FIX16(.34414) * cb + 32768 - FIX16(.71414) * cr) >> 16));
            const int bl = clamp255(l + ((FIX16(1.772) * cb + 32768) >> 16));
            out[0] |= (unsigned)r << (8 * j);
            out[1] |= (unsigned)g << (8 * j);
            out[2] |= (unsigned)bl << (8 * j);
        }
        unsigned char* dst = y + ((size_t)b * 3 * H + yy) * W + 4 * xq;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned char* o = dst + (size_t)c * H * W;
            if (VEC4) {
                *reinterpret_cast<unsigned*>(o) = out[c];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * xq + j < W) o[j] = (unsigned char)(out[c] >> (8 * j));
            }
        }
    }
}

const unsigned char kLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                 14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                 18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char kChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                   99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// jpeg_set_quality(quality, force_baseline = TRUE) and the reciprocals; false if a reciprocal fails its exactness condition
bool make_tables(int quality, JpegTables* t) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            int q = ((c ? kChroma[k] : kLuma[k]) * s + 50) / 100;
            q = q < 1 ? 1 : (q > 255 ? 255 : q);
            const uint64_t d = 8u * (unsigned)q, m = (1ull << 27) / d + 1;
            if ((m * d - (1ull << 27)) * 65535ull >= (1ull << 27) || m > 0xffffffffull) return false;
            t->q[c][k] = (unsigned short)q;
            t->rcp[c][k] = (unsigned)m;
        }
    return true;
}

inline bool bad_dims(int64_t B, int64_t H, int64_t W) {
    return B < 1 || H < 8 || W < 8 || B > 0x7fffffffLL || H > 0x7fffffffLL || W > 0x7fffffffLL;
}

}  // namespace

extern "C" {

int64_t stylex_jpeg_roundtrip_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    if (bad_dims(B, H, W)) return -1;
    const int64_t Hm = (H + 15) / 16 * 16, Wm = (W + 15) / 16 * 16;
    if (Hm * Wm > 0x7fffffffLL || B * (Hm * Wm / 2 * 3) > (1LL << 40)) return -1;
    return B * (Hm * Wm / 2 * 3);
}

int stylex_jpeg_roundtrip(const void* x, unsigned char* y_u8, const int64_t* sh, const int64_t* strides, int x_is_bf16, int quality,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    // sh = {B, H, W}; strides = element strides of x (b, c, h, w), channels 0..2 are read; y_u8 dense [B][3][H][W]
    if (!x || !y_u8 || !sh || !strides || !workspace) return STYLEX_EINVAL;
    if (quality < 1 || quality > 100 || bad_dims(sh[0], sh[1], sh[2])) return STYLEX_EINVAL;
    const int64_t B = sh[0], H = sh[1], W = sh[2];
    const int64_t need = stylex_jpeg_roundtrip_workspace_bytes(B, H, W);
    if (need < 0 || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return STYLEX_EINVAL;
    int64_t last = 0;  // the largest element offset that is read
    const int64_t ext[4] = {B, 3, H, W};
    for (int k = 0; k < 4; ++k) {
        if (strides[k] < 0 || strides[k] > 0x7fffffffLL) return STYLEX_EINVAL;
        last += (ext[k] - 1) * strides[k];
    }
    const int64_t mr = (H + 15) / 16, mc = (W + 15) / 16, quads = B * H * ((W + 3) / 4);
    if (last > 0x7fffffffLL || B * 3 * H * W > 0x7fffffffLL || B * mr * mc > 0x7fffffffLL || quads > 0x7fffffffLL)
        return STYLEX_EINVAL;
    JpegTables tab;
    if (!make_tables(quality, &tab)) return STYLEX_EINVAL;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const dim3 ga((unsigned)(B * mr * mc)), ba(64);
    if (x_is_bf16)
        hipLaunchKernelGGL(jpeg_codec_kernel<true>, ga, ba, 0, (hipStream_t)stream, x, ws, (int)H, (int)W, (int)mr, (int)mc,
                           (long)strides[0], (long)strides[1], (long)strides[2], (long)strides[3], tab);
    else
        hipLaunchKernelGGL(jpeg_codec_kernel<false>, ga, ba, 0, (hipStream_t)stream, x, ws, (int)H, (int)W, (int)mr, (int)mc,
                           (long)strides[0], (long)strides[1], (long)strides[2], (long)strides[3], tab);
    const int e = (int)hipGetLastError();
    if (e) return e;
    const unsigned long nb = ((unsigned long)quads + 255) / 256;
    const dim3 gb((unsigned)(nb > 65536 ? 65536 : nb)), bb(256);
    if (W % 4 == 0 && (reinterpret_cast<uintptr_t>(y_u8) & 3) == 0)
        hipLaunchKernelGGL(jpeg_upsample_rgb_kernel<true>, gb, bb, 0, (hipStream_t)stream, ws, y_u8, (int)H, (int)W, (int)mr, (int)mc,
                           (unsigned)quads);
    else
        hipLaunchKernelGGL(jpeg_upsample_rgb_kernel<false>, gb, bb, 0, (hipStream_t)stream, ws, y_u8, (int)H, (int)W, (int)mr, (int)mc,
                           (unsigned)quads);
    return (int)hipGetLastError();
}

}  // extern "C"
