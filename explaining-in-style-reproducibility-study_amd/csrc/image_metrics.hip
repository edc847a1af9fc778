// image_metrics.hip — image-pair statistics of a reconstruction against its original (stylex/recon_metrics.py):
// per image the sums of |d|, d^2 and of the per-position SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid
// positions, population moments, C1 = 0.01^2, C2 = 0.03^2, data range 1).
//
//   image_pair_stats_kernel   one block per (image, channel, T x T output tile).  Both (T + 10)^2 halo tiles are staged once
//                             into LDS as fp32 under the value rule (the byte of an image file / 255, or clamp(v, 0, 1));
//                             the thread that stages a pixel its tile owns adds |d| and d^2.  Horizontal pass of the five
//                             quantities x, y, x^2, y^2, xy into LDS, vertical pass and the SSIM quotient in registers, one
//                             position per thread.  fp64 from the thread outward: wave shuffles, the four waves in order,
//                             one partial [3] per block into the workspace.
//   image_pair_reduce_kernel  one wave per image adds that image's partials: lane l takes l, l + 64, ... ascending, then
//                             the shuffle tree.  No atomics anywhere: the same inputs give the same bits.
// Every fp32 operation is written as the instruction it is (fmaf or one rounded operation, contraction off), and the three
// centred moments take the same forms: for y = x the numerator and the denominator of the quotient are the same two
// floats, the quotient is exactly 1.0f, every partial is an integer and the sum is exact.
// Built without the SLP vectoriser (Makefile: CXXFLAGS_image_metrics), the rule of torgb.hip: the five products per tap are
// the rows of independent fp32 operations it pairs into packed instructions.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

constexpr int T = 16;               // output tile extent: 16 x 16 positions, one per thread
constexpr int WIN = 11;             // window extent
constexpr int HALO = T + WIN - 1;   // 26
constexpr int TS = 48;              // LDS row stride of a halo tile in floats: rows r and r + 1 of a half-wave's 16-column
                                    // reads land 16 banks apart
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

struct Window { float w[WIN]; };

struct Operand {
    const void* p;
    long sb, sc, sh, sw;
    int bf16;
};

__device__ __forceinline__ float load_px(const Operand& o, long off) {
    if (o.bf16) return __uint_as_float((unsigned)static_cast<const unsigned short*>(o.p)[off] << 16);
    return static_cast<const float*>(o.p)[off];
}

// The SSIM of one window position from its five weighted means.  mu mu, the centred moments and the two factors of the
// numerator and the denominator: for y = x, 2 mxy + C1 and (mxx + myy) + C1 are one rounding of the same real number
// (2 mxy and mxx + myy are exact), likewise the second factor.
__device__ __forceinline__ float ssim_quotient(float mx, float my, float exx, float eyy, float exy) {
#pragma clang fp contract(off)
    const float mxx = mx * mx, myy = my * my, mxy = mx * my;
    const float sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    const float a1 = fmaf(2.f, mxy, C1), a2 = fmaf(2.f, sxy, C2);
    const float b1 = (mxx + myy) + C1, b2 = (sxx + syy) + C2;
    return __fdiv_rn(a1 * a2, b1 * b2);
}

template <bool Q>
__global__ __launch_bounds__(256) void image_pair_stats_kernel(Operand x, Operand y, double* __restrict__ partial, Window win, int H,
                                                               int W, int C, int tiles_x, int tiles_y) {
    __shared__ float tx[HALO * TS], ty[HALO * TS];
    __shared__ float hq[5][HALO][T];
    __shared__ double red[4][3];
    const unsigned tid = threadIdx.x;
    const unsigned tiles = (unsigned)(tiles_x * tiles_y);
    const unsigned t = blockIdx.x % tiles, bc = blockIdx.x / tiles;
    const int c = (int)(bc % (unsigned)C), b = (int)(bc / (unsigned)C);
    const int tyi = (int)t / tiles_x, txi = (int)t % tiles_x;
    const int oy = tyi * T, ox = txi * T;
    // the pixels whose differences this tile adds: its T rows / columns; the last tile of a row / column takes the ten behind
    // them as well (they are inside its halo), so that every pixel of the plane has one owner
    const int own_y = tyi == tiles_y - 1 ? H : oy + T, own_x = txi == tiles_x - 1 ? W : ox + T;
    const long xbase = b * x.sb + c * x.sc, ybase = b * y.sb + c * y.sc;

    double s_abs = 0.0, s_sq = 0.0;
    for (unsigned e = tid; e < (unsigned)(HALO * HALO); e += 256u) {
#pragma clang fp contract(off)
        const int r = (int)e / HALO, cc = (int)e - r * HALO;
        const int gy = oy + r, gx = ox + cc;
        float vx = 0.f, vy = 0.f;  // outside the plane: read by masked positions only
        if (gy < H && gx < W) {
            const float rx = load_px(x, xbase + gy * x.sh + gx * x.sw), ry = load_px(y, ybase + gy * y.sh + gx * y.sw);
            float dx, dy;  // what the differences are taken of: bytes (exact integers) or clamped values
            if (Q) {
                dx = stylex_image_byte(rx);
                dy = stylex_image_byte(ry);
                vx = __fdiv_rn(dx, 255.f);
                vy = __fdiv_rn(dy, 255.f);
            } else {
                dx = vx = fminf(fmaxf(rx, 0.f), 1.f);
                dy = vy = fminf(fmaxf(ry, 0.f), 1.f);
            }
            if (gy < own_y && gx < own_x) {
                const float d = dx - dy;
                s_abs += (double)fabsf(d);
                s_sq += (double)(d * d);
            }
        }
        tx[r * TS + cc] = vx;
        ty[r * TS + cc] = vy;
    }
    __syncthreads();

    // horizontal pass: row r, output column j <- taps j .. j + 10 of the halo row
    for (unsigned e = tid; e < (unsigned)(HALO * T); e += 256u) {
#pragma clang fp contract(off)
        const int r = (int)e / T, j = (int)e % T;
        const float* px = tx + r * TS + j;
        const float* py = ty + r * TS + j;
        float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float a = px[k], bb = py[k], w = win.w[k];
            ax = fmaf(w, a, ax);
            ay = fmaf(w, bb, ay);
            axx = fmaf(w, a * a, axx);
            ayy = fmaf(w, bb * bb, ayy);
            axy = fmaf(w, a * bb, axy);
        }
        hq[0][r][j] = ax;
        hq[1][r][j] = ay;
        hq[2][r][j] = axx;
        hq[3][r][j] = ayy;
        hq[4][r][j] = axy;
    }
    __syncthreads();

    // vertical pass and quotient: position (i, j) of the tile
    const int i = (int)tid / T, j = (int)tid % T;
    float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
        const float w = win.w[k];
        mx = fmaf(w, hq[0][i + k][j], mx);
        my = fmaf(w, hq[1][i + k][j], my);
        exx = fmaf(w, hq[2][i + k][j], exx);
        eyy = fmaf(w, hq[3][i + k][j], eyy);
        exy = fmaf(w, hq[4][i + k][j], exy);
    }
    const float q = ssim_quotient(mx, my, exx, eyy, exy);
    const bool valid = oy + i < H - (WIN - 1) && ox + j < W - (WIN - 1);
    double v0 = s_abs, v1 = s_sq, v2 = valid ? (double)q : 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v0 += __shfl_down(v0, off, 64);
        v1 += __shfl_down(v1, off, 64);
        v2 += __shfl_down(v2, off, 64);
    }
    if ((tid & 63u) == 0u) {
        red[tid >> 6][0] = v0;
        red[tid >> 6][1] = v1;
        red[tid >> 6][2] = v2;
    }
    __syncthreads();
    if (tid < 3u) partial[(size_t)blockIdx.x * 3 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// out[b][k] = sum of partial[b * n + m][k], m < n: lane l adds m = l, l + 64, ... ascending, then the shuffle tree
__global__ __launch_bounds__(64) void image_pair_reduce_kernel(const double* __restrict__ partial, double* __restrict__ out, unsigned n) {
    const unsigned b = blockIdx.x, lane = threadIdx.x;
    const double* p = partial + (size_t)b * n * 3;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    for (unsigned m = lane; m < n; m += 64u) {
        v0 += p[(size_t)m * 3];
        v1 += p[(size_t)m * 3 + 1];
        v2 += p[(size_t)m * 3 + 2];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v0 += __shfl_down(v0, off, 64);
        v1 += __shfl_down(v1, off, 64);
        v2 += __shfl_down(v2, off, 64);
    }
    if (lane == 0u) {
        out[(size_t)b * 3] = v0;
        out[(size_t)b * 3 + 1] = v1;
        out[(size_t)b * 3 + 2] = v2;
    }
}

// exp(-(k - 5)^2 / (2 sigma^2)), sigma = 1.5, normalised to sum 1 in fp64, then rounded to fp32
Window gaussian_window() {
    double g[WIN], sum = 0.0;
    for (int k = 0; k < WIN; ++k) {
        const double d = k - WIN / 2;
        g[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    Window w;
    for (int k = 0; k < WIN; ++k) w.w[k] = (float)(g[k] / sum);
    return w;
}

// blocks of the first launch, or -1 for a shape the kernels do not take
int64_t plan_blocks(int64_t B, int64_t C, int64_t H, int64_t W, int64_t* tiles_x, int64_t* tiles_y) {
    if (B < 1 || C < 1 || C > 4 || H < WIN || W < WIN || H > 0x7fffffffLL || W > 0x7fffffffLL || B > 0x7fffffffLL) return -1;
    const int64_t ty = (H - (WIN - 1) + T - 1) / T, tx = (W - (WIN - 1) + T - 1) / T;
    if (ty * tx > 0x7fffffffLL) return -1;
    const int64_t per_image = C * ty * tx;
    if (per_image > 0x7fffffffLL || B * per_image > 0x7fffffffLL) return -1;
    if (tiles_x) *tiles_x = tx;
    if (tiles_y) *tiles_y = ty;
    return B * per_image;
}

bool make_operand(const void* p, const int64_t* st, int bf16, int64_t B, int64_t C, int64_t H, int64_t W, Operand* o) {
    const int64_t ext[4] = {B, C, H, W};
    int64_t last = 0;  // the largest element offset that is read
    for (int k = 0; k < 4; ++k) {
        if (st[k] < 0 || st[k] > 0x7fffffffLL) return false;
        last += (ext[k] - 1) * st[k];
    }
    if (last > 0x7fffffffLL) return false;
    *o = Operand{p, (long)st[0], (long)st[1], (long)st[2], (long)st[3], bf16 ? 1 : 0};
    return true;
}

}  // namespace

extern "C" {

int64_t stylex_image_pair_stats_tile(void) { return T; }

int64_t stylex_image_pair_stats_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
    const int64_t blocks = plan_blocks(B, C, H, W, nullptr, nullptr);
    return blocks < 0 ? -1 : blocks * 3 * (int64_t)sizeof(double);
}

int stylex_image_pair_stats(const void* x, const void* y, double* out, const int64_t* sh, const int64_t* x_strides,
                            const int64_t* y_strides, int x_is_bf16, int y_is_bf16, int quantise, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    if (!x || !y || !out || !sh || !x_strides || !y_strides || !workspace) return STYLEX_EINVAL;
    const int64_t B = sh[0], C = sh[1], H = sh[2], W = sh[3];
    int64_t tiles_x = 0, tiles_y = 0;
    const int64_t blocks = plan_blocks(B, C, H, W, &tiles_x, &tiles_y);
    if (blocks < 0) return STYLEX_EINVAL;
    if (workspace_bytes < blocks * 3 * (int64_t)sizeof(double)) return STYLEX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(out)) & 7) return STYLEX_EINVAL;
    Operand ox, oy;
    if (!make_operand(x, x_strides, x_is_bf16, B, C, H, W, &ox) || !make_operand(y, y_strides, y_is_bf16, B, C, H, W, &oy))
        return STYLEX_EINVAL;
    static const Window win = gaussian_window();
    double* partial = static_cast<double*>(workspace);
    if (quantise)
        hipLaunchKernelGGL(image_pair_stats_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ox, oy, partial,
                           win, (int)H, (int)W, (int)C, (int)tiles_x, (int)tiles_y);
    else
        hipLaunchKernelGGL(image_pair_stats_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ox, oy, partial,
                           win, (int)H, (int)W, (int)C, (int)tiles_x, (int)tiles_y);
    const int e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(image_pair_reduce_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, partial, out,
                       (unsigned)(blocks / B));
    return (int)hipGetLastError();
}

}  // extern "C"
