// resample_u8.hip — the device input pipeline's byte arithmetic (stylex/input_pipeline.py): PIL's 8-bit bilinear resize
// (Image.resize(size, BILINEAR): fixed-point coefficients with 22 fraction bits, a horizontal pass and a vertical pass that
// each round to bytes), the RGBA premultiplied round trip around it, crop, and the final byte -> value/255 table lookup
// into planar fp32.  One launch serves every image of a ragged batch: block (x, j) works on job j of a job table in device
// memory, blocks past a job's last pixel leave at once.  Coefficients and tap bounds are computed on the host in float64 and
// travel in the same int32 table; the kernels do integer arithmetic only (no float touches a pixel value; the result is
// lut[byte]), no atomics, one thread per output pixel with all its channels.
//
// The entry points check every job against the HOST copy of the table before anything is launched: channel counts, windows
// inside their images, every tap range the launch will read inside its source, every store inside its destination.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

constexpr int NT = 256;
constexpr int PRECISION_BITS = 22;
constexpr int FLAG_PREMUL = 1, FLAG_UNPREMUL = 2, FLAG_LUT = 4;
enum { KIND_ROWS = 0, KIND_COLS = 1, KIND_CROP = 2 };

// One job = one pass over one image (20 int32, input_pipeline.JOB_INTS).  "o" runs along the resampled axis in OUTPUT
// indices (columns for the row pass, rows for the column pass), "p" along the other axis in source indices.
struct RsJob {
    int src_off;     // byte offset of the source image in the source buffer
    int src_h, src_w, src_bpp;  // source extent in pixels, bytes per pixel (3: packed RGB; 4: RGBA or PIL's padded RGB)
    int C;           // channels computed (3 or 4)
    int in0;         // source index that tap position 0 of the coefficient table refers to (origin of the resized box)
    int o0, o1;      // output range of the pass (crop: source rows)
    int p0, p1;      // range along the other axis (crop: source columns)
    int bounds_off;  // int32 offset in the table of {first tap, tap count} per output index
    int coef_off;    // int32 offset of the coefficients, ksize per output index
    int ksize;
    int dst_off, dst_stride, dst_plane;  // in destination elements (4-byte pixels, or floats for FLAG_LUT)
    int flags;
    int pad[3];
};
static_assert(sizeof(RsJob) == 80, "RsJob mirrors input_pipeline.JOB_INTS");

__device__ __forceinline__ int muldiv255(int c, int a) {
    const int t = c * a + 128;
    return ((t >> 8) + t) >> 8;
}

// acc + byte * coefficient as one full-rate v_mad_u32_u24: bilinear coefficients lie in [0, 1 << 22] (checked on the host),
// so the 24-bit multiply is exact and the sums never go negative.
__device__ __forceinline__ int tap(int acc, unsigned byte, int k) { return acc + (int)__umul24(byte, (unsigned)k); }

// PIL's clip8 of a non-negative sum.  Written on unsigned values on purpose: from the signed form (arithmetic shift +
// clamp to [0, 255]) hipcc packs two channels with gfx950's v_ashr_pk_u8_i32 and ORs the other two on top assuming bits
// 31:16 of its result are zero; on the MI355X they were not (the third channel and the pad byte of every pixel came out
// with bits of the second channel's accumulator in them).
__device__ __forceinline__ unsigned clip8(int acc) {
    const unsigned v = (unsigned)acc >> PRECISION_BITS;
    return v > 255u ? 255u : v;
}

// colours of a premultiplied pixel divided by alpha, as PIL's rgba2rgbA
__device__ __forceinline__ int unpremul(int c, int a) {
    if (a == 0 || a == 255) return c;
    const int q = (255 * c) / a;
    return q > 255 ? 255 : q;
}

__device__ __forceinline__ void store_pixel(const RsJob& j, int r, int x, int c0, int c1, int c2, int c3, uint32_t* dst,
                                            const float* __restrict__ lut, float* __restrict__ out) {
    if (j.flags & FLAG_UNPREMUL) {
        c0 = unpremul(c0, c3);
        c1 = unpremul(c1, c3);
        c2 = unpremul(c2, c3);
    }
    if (j.flags & FLAG_LUT) {
        float* o = out + j.dst_off + (long)r * j.dst_stride + x;
        o[0] = lut[c0];
        o[j.dst_plane] = lut[c1];
        o[2L * j.dst_plane] = lut[c2];
        if (j.C == 4) o[3L * j.dst_plane] = lut[c3];
    } else {
        dst[j.dst_off + (long)r * j.dst_stride + x] = (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16) | ((uint32_t)c3 << 24);
    }
}

// Horizontal pass: uint8 HWC source (3 or 4 bytes per pixel) -> 4-byte pixels, only the rows [p0, p1) and the output
// columns [o0, o1) the column pass will read.
__global__ __launch_bounds__(NT) void resample_rows_u8_kernel(const int* __restrict__ table, int first_job,
                                                              const uint8_t* __restrict__ src, uint32_t* __restrict__ dst) {
    const RsJob& j = reinterpret_cast<const RsJob*>(table)[first_job + blockIdx.y];
    const int ncols = j.o1 - j.o0;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= ncols * (j.p1 - j.p0)) return;
    const int r = i / ncols, x = i - r * ncols;
    const int xx = j.o0 + x;
    const int xmin = table[j.bounds_off + 2 * xx], cnt = table[j.bounds_off + 2 * xx + 1];
    const int* __restrict__ k = table + j.coef_off + (long)xx * j.ksize;
    const uint8_t* px = src + j.src_off + ((long)(j.p0 + r) * j.src_w + j.in0 + xmin) * j.src_bpp;
    const bool premul = (j.flags & FLAG_PREMUL) != 0;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    if (j.src_bpp == 4) {
        const uint32_t* p4 = reinterpret_cast<const uint32_t*>(px);
        for (int t = 0; t < cnt; ++t) {
            const uint32_t v = p4[t];
            const int kk = k[t];
            int c0 = v & 255, c1 = (v >> 8) & 255, c2 = (v >> 16) & 255;
            const int c3 = v >> 24;
            if (premul) {
                c0 = muldiv255(c0, c3);
                c1 = muldiv255(c1, c3);
                c2 = muldiv255(c2, c3);
            }
            a0 = tap(a0, c0, kk);
            a1 = tap(a1, c1, kk);
            a2 = tap(a2, c2, kk);
            a3 = tap(a3, c3, kk);
        }
    } else {
        for (int t = 0; t < cnt; ++t) {
            const int kk = k[t];
            a0 = tap(a0, px[3 * t], kk);
            a1 = tap(a1, px[3 * t + 1], kk);
            a2 = tap(a2, px[3 * t + 2], kk);
        }
    }
    const uint32_t c3 = j.C == 4 ? clip8(a3) : 0u;
    dst[j.dst_off + (long)r * j.dst_stride + x] = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (c3 << 24);
}

// Vertical pass over the 4-byte intermediate, dword loads along x.  Writes 4-byte pixels (the stage-1 image an augmented
// item's second resize reads) or, with FLAG_LUT, the final planar fp32 values lut[byte].
__global__ __launch_bounds__(NT) void resample_cols_u8_kernel(const int* __restrict__ table, int first_job,
                                                              const uint8_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                              const float* __restrict__ lut, float* __restrict__ out) {
    const RsJob& j = reinterpret_cast<const RsJob*>(table)[first_job + blockIdx.y];
    const int ncols = j.p1 - j.p0;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= ncols * (j.o1 - j.o0)) return;
    const int r = i / ncols, x = i - r * ncols;
    const int yy = j.o0 + r;
    const int ymin = table[j.bounds_off + 2 * yy], cnt = table[j.bounds_off + 2 * yy + 1];
    const int* __restrict__ k = table + j.coef_off + (long)yy * j.ksize;
    const uint32_t* col = reinterpret_cast<const uint32_t*>(src + j.src_off) + (long)(j.in0 + ymin) * j.src_w + j.p0 + x;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int t = 0; t < cnt; ++t) {
        const uint32_t v = col[(long)t * j.src_w];
        const int kk = k[t];
        a0 = tap(a0, v & 255, kk);
        a1 = tap(a1, (v >> 8) & 255, kk);
        a2 = tap(a2, (v >> 16) & 255, kk);
        a3 = tap(a3, v >> 24, kk);
    }
    store_pixel(j, r, x, clip8(a0), clip8(a1), clip8(a2), j.C == 4 ? clip8(a3) : 0, dst, lut, out);
}

// Images already at their final scale: crop window -> planar fp32 lut[byte].
__global__ __launch_bounds__(NT) void crop_lut_u8_kernel(const int* __restrict__ table, int first_job,
                                                         const uint8_t* __restrict__ src, const float* __restrict__ lut,
                                                         float* __restrict__ out) {
    const RsJob& j = reinterpret_cast<const RsJob*>(table)[first_job + blockIdx.y];
    const int ncols = j.p1 - j.p0;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= ncols * (j.o1 - j.o0)) return;
    const int r = i / ncols, x = i - r * ncols;
    const uint8_t* px = src + j.src_off + ((long)(j.o0 + r) * j.src_w + j.p0 + x) * j.src_bpp;
    store_pixel(j, r, x, px[0], px[1], px[2], j.C == 4 ? px[3] : 0, nullptr, lut, out);
}

// ---- host: every job checked against the host copy of the table -------------------------------------------------------

struct RsCheck {
    const int32_t* table;
    int64_t table_ints, src_bytes, dst_pixels, out_floats;
    bool have_dst, have_out;
};

bool job_ok(int kind, const RsJob& j, const RsCheck& c, int64_t* npix) {
    if (j.C != 3 && j.C != 4) return false;
    if ((j.src_bpp != 3 && j.src_bpp != 4) || j.src_bpp < j.C) return false;
    if (kind == KIND_COLS && j.src_bpp != 4) return false;
    if (j.src_h < 1 || j.src_w < 1 || j.src_off < 0) return false;
    if (j.src_bpp == 4 && (j.src_off & 3)) return false;
    if ((int64_t)j.src_off + (int64_t)j.src_h * j.src_w * j.src_bpp > c.src_bytes) return false;
    if (j.o0 < 0 || j.o1 <= j.o0 || j.p0 < 0 || j.p1 <= j.p0) return false;  // empty window
    // extent of the source along the pass axis / the other axis
    const int along = kind == KIND_ROWS ? j.src_w : j.src_h, across = kind == KIND_ROWS ? j.src_h : j.src_w;
    if (j.p1 > across) return false;
    int64_t nrows, ncols;
    if (kind == KIND_ROWS) {
        nrows = j.p1 - j.p0;
        ncols = j.o1 - j.o0;
    } else {
        nrows = j.o1 - j.o0;
        ncols = j.p1 - j.p0;
    }
    if (nrows * ncols > 0x7fffffff) return false;
    *npix = nrows * ncols;
    if (kind == KIND_CROP) {
        if (j.o1 > along || !(j.flags & FLAG_LUT) || (j.flags & (FLAG_PREMUL | FLAG_UNPREMUL))) return false;
    } else {
        if (j.ksize < 1 || j.bounds_off < 0 || j.coef_off < 0) return false;
        if ((int64_t)j.bounds_off + 2 * (int64_t)j.o1 > c.table_ints) return false;
        if ((int64_t)j.coef_off + (int64_t)j.o1 * j.ksize > c.table_ints) return false;
        for (int o = j.o0; o < j.o1; ++o) {  // every tap the launch reads lies inside the source
            const int64_t first = (int64_t)j.in0 + c.table[j.bounds_off + 2 * o];
            const int cnt = c.table[j.bounds_off + 2 * o + 1];
            if (cnt < 0 || cnt > j.ksize || first < 0 || first + cnt > along) return false;
            for (int t = 0; t < cnt; ++t) {  // what tap() and clip8() rely on
                const int32_t k = c.table[j.coef_off + (int64_t)o * j.ksize + t];
                if (k < 0 || k > (1 << PRECISION_BITS)) return false;
            }
        }
        if ((j.flags & (FLAG_PREMUL | FLAG_UNPREMUL)) && j.C != 4) return false;
        if (kind == KIND_ROWS && (j.flags & ~FLAG_PREMUL)) return false;
        if (kind == KIND_COLS && (j.flags & FLAG_PREMUL)) return false;
    }
    if (j.dst_off < 0 || j.dst_stride < ncols) return false;
    const int64_t last = (int64_t)j.dst_off + (nrows - 1) * j.dst_stride + ncols;
    if (j.flags & FLAG_LUT) {
        if (!c.have_out || j.dst_plane < 0 || last + (int64_t)(j.C - 1) * j.dst_plane > c.out_floats) return false;
    } else {
        if (!c.have_dst || last > c.dst_pixels) return false;
    }
    return true;
}

// returns the launch's grid x (blocks of the largest job), or STYLEX_EINVAL
int64_t check_jobs(int kind, const RsCheck& c, int64_t first_job, int64_t njobs) {
    if (!c.table || c.table_ints < 0 || first_job < 0 || njobs < 1 || njobs > 65535) return STYLEX_EINVAL;
    if ((first_job + njobs) * (int64_t)(sizeof(RsJob) / 4) > c.table_ints) return STYLEX_EINVAL;
    const RsJob* jobs = reinterpret_cast<const RsJob*>(c.table) + first_job;
    int64_t most = 0;
    for (int64_t n = 0; n < njobs; ++n) {
        int64_t npix = 0;
        if (!job_ok(kind, jobs[n], c, &npix)) return STYLEX_EINVAL;
        most = npix > most ? npix : most;
    }
    return (most + NT - 1) / NT;
}

}  // namespace

extern "C" {

int stylex_resample_rows_u8(const int32_t* table_host, const int32_t* table_dev, int64_t table_ints, int64_t first_job,
                            int64_t njobs, const void* src, int64_t src_bytes, void* dst, int64_t dst_pixels, void* stream) {
    if (!table_host || !table_dev || !src || !dst || src_bytes < 1 || dst_pixels < 1) return STYLEX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(table_dev)) & 3)
        return STYLEX_EINVAL;
    const RsCheck c = {table_host, table_ints, src_bytes, dst_pixels, 0, true, false};
    const int64_t blocks = check_jobs(KIND_ROWS, c, first_job, njobs);
    if (blocks < 1) return STYLEX_EINVAL;
    StylexTimedCall tm(STYLEX_TIMING_INPUT, (double)src_bytes + 4.0 * dst_pixels, (hipStream_t)stream);
    stylex_note_kernel("resample_rows_u8_kernel");
    hipLaunchKernelGGL(resample_rows_u8_kernel, dim3((unsigned)blocks, (unsigned)njobs), dim3(NT), 0, (hipStream_t)stream,
                       table_dev, (int)first_job, (const uint8_t*)src, (uint32_t*)dst);
    return (int)hipGetLastError();
}

int stylex_resample_cols_u8(const int32_t* table_host, const int32_t* table_dev, int64_t table_ints, int64_t first_job,
                            int64_t njobs, const void* src, int64_t src_bytes, void* dst, int64_t dst_pixels, const float* lut,
                            float* out, int64_t out_floats, void* stream) {
    if (!table_host || !table_dev || !src || src_bytes < 1 || (!dst && !out) || (out && !lut)) return STYLEX_EINVAL;
    if ((dst && dst_pixels < 1) || (out && out_floats < 1)) return STYLEX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(table_dev) |
         reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(lut)) & 3)
        return STYLEX_EINVAL;
    const RsCheck c = {table_host, table_ints, src_bytes, dst_pixels, out_floats, dst != nullptr, out != nullptr};
    const int64_t blocks = check_jobs(KIND_COLS, c, first_job, njobs);
    if (blocks < 1) return STYLEX_EINVAL;
    StylexTimedCall tm(STYLEX_TIMING_INPUT, (double)src_bytes + 4.0 * (dst ? dst_pixels : 0) + 4.0 * (out ? out_floats : 0),
                       (hipStream_t)stream);
    stylex_note_kernel("resample_cols_u8_kernel");
    hipLaunchKernelGGL(resample_cols_u8_kernel, dim3((unsigned)blocks, (unsigned)njobs), dim3(NT), 0, (hipStream_t)stream,
                       table_dev, (int)first_job, (const uint8_t*)src, (uint32_t*)dst, lut, out);
    return (int)hipGetLastError();
}

int stylex_crop_lut_u8(const int32_t* table_host, const int32_t* table_dev, int64_t table_ints, int64_t first_job, int64_t njobs,
                       const void* src, int64_t src_bytes, const float* lut, float* out, int64_t out_floats, void* stream) {
    if (!table_host || !table_dev || !src || !lut || !out || src_bytes < 1 || out_floats < 1) return STYLEX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(table_dev) | reinterpret_cast<uintptr_t>(out) |
         reinterpret_cast<uintptr_t>(lut)) & 3)
        return STYLEX_EINVAL;
    const RsCheck c = {table_host, table_ints, src_bytes, 0, out_floats, false, true};
    const int64_t blocks = check_jobs(KIND_CROP, c, first_job, njobs);
    if (blocks < 1) return STYLEX_EINVAL;
    StylexTimedCall tm(STYLEX_TIMING_INPUT, (double)src_bytes + 4.0 * out_floats, (hipStream_t)stream);
    stylex_note_kernel("crop_lut_u8_kernel");
    hipLaunchKernelGGL(crop_lut_u8_kernel, dim3((unsigned)blocks, (unsigned)njobs), dim3(NT), 0, (hipStream_t)stream, table_dev,
                       (int)first_job, (const uint8_t*)src, lut, out);
    return (int)hipGetLastError();
}

}  // extern "C"
