// fused_bwd.hip — backward-side elementwise + per-(image,channel) reduction kernels of the fused
// fast path (steps without gradient penalty / path-length regularisation need no double backward,
// so conv + bias/noise + LeakyReLU (+ demodulation / residual merge) run as ONE forward kernel and
// the gradient bookkeeping below replaces 5-8 separate full-tensor passes and reductions).
//
// Activation tensors NHWC fp32 or bf16 (act_dtype), sums in fp32.  One block = one image b x one contiguous pixel range; a thread owns VEC
// consecutive channels and walks pixels with stride rows-per-pass, accumulating up to 3 column sums
// in registers; the block combines them through LDS in fixed order and writes
// partial[b][chunk][k][C]; the (tiny) sum over chunks is done by the caller.  Deterministic.
//
// Reference ops covered (stylex/stylex_train.py): the backward of  x = lrelu(conv + bias) (:726-731),
// (x + res)/sqrt(2) (:743), x = lrelu(conv2dmod(x, style) + noise) (:700-714) and of the modulation
// / demodulation products inside Conv2DMod.forward (:650-656).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "stylex_internal.h"

namespace {

constexpr int NT = 256;

template <int K>
struct Acc {
    float4 v[K];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

// Block-level reduction over the pixel-row dimension and store of partial[b][chunk][k][c..c+3].
template <int K>
__device__ __forceinline__ void block_reduce_store(Acc<K>& a, float* smem, int cv, int prow, int CV, int rpp, int C,
                                                   float* partial_row /* [K][C] */, bool active) {
    // smem layout [K][rpp][CV] float4
    float4* s4 = reinterpret_cast<float4*>(smem);
    if (active) {
#pragma unroll
        for (int k = 0; k < K; ++k) s4[(k * rpp + prow) * CV + cv] = a.v[k];
    }
    __syncthreads();
    if (active && prow == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int r = 0; r < rpp; ++r) {
                float4 u = s4[(k * rpp + r) * CV + cv];
                t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
            }
            float* d = partial_row + (long)k * C + cv * 4;
            if (cv * 4 + 3 < C) {
                *reinterpret_cast<float4*>(d) = t;
            } else {
                float tt[4] = {t.x, t.y, t.z, t.w};
                for (int e = 0; e < 4 && cv * 4 + e < C; ++e) d[e] = tt[e];
            }
        }
    }
}

struct Geo {
    int b, cv, prow, CV, rpp;
    long p_begin, p_end;  // pixel range of this block within image b
    bool active;
};

__device__ __forceinline__ Geo make_geo(int HW, int C, int nchunks) {
    Geo g;
    g.CV = (C + 3) / 4;
    if (g.CV > NT) g.CV = NT;  // C <= 1024 asserted by the host
    g.rpp = NT / g.CV;
    g.cv = threadIdx.x % g.CV;
    g.prow = threadIdx.x / g.CV;
    g.active = g.prow < g.rpp;
    g.b = blockIdx.y;
    long per = ((long)HW + nchunks - 1) / nchunks;
    g.p_begin = (long)blockIdx.x * per;
    g.p_end = g.p_begin + per < HW ? g.p_begin + per : HW;
    return g;
}

// activation loads/stores (fp32 or bf16 by runtime flag); C % 4 == 0 is checked on the host
__device__ __forceinline__ float4 ld4(const void* p, long off, int bf) { return act_ld4(p, off, bf); }
__device__ __forceinline__ void st4(void* p, long off, float4 v, int bf) { act_st4(p, off, v, bf); }
__device__ __forceinline__ float4 ldp4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// (h, w) of a lane's pixel, advanced by a fixed pixel step without a division (the step is split once per block)
struct PixWalk {
    int h, w, dh, dw, W;
    __device__ __forceinline__ PixWalk(int p, int step, int W_) : W(W_) {
        h = p / W_;
        w = p - h * W_;
        dh = step / W_;
        dw = step - dh * W_;
    }
    __device__ __forceinline__ void advance() {
        w += dw;
        h += dh;
        if (w >= W) {
            w -= W;
            ++h;
        }
    }
};
// noise plane of image b: transposed (the reference's read, noise[b][w][h]) or natural order (nat[b][h][w])
__device__ __forceinline__ long noise_off(int b, int ns, int h, int w, int natural) {
    return natural ? ((long)b * ns + h) * ns + w : ((long)b * ns + w) * ns + h;
}

// dx = dy * scale * (lrelu ? (y > 0 ? 1 : 0.2) : 1);  partial[b][chunk][c] = sum_pixels dx
__global__ __launch_bounds__(NT) void act_bwd_reduce_kernel(const void* __restrict__ dy, const void* __restrict__ y,
                                                           void* __restrict__ dx, float* __restrict__ partial, int HW,
                                                           int C, int nchunks, int lrelu, float scale, int bf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    Geo g = make_geo(HW, C, nchunks);
    Acc<1> a;
    a.zero();
    const int c = g.cv * 4;
    if (g.active && c < C) {
        const long base = (long)g.b * HW;
        for (long p = g.p_begin + g.prow; p < g.p_end; p += g.rpp) {
            const long o = (base + p) * C + c;
            float4 gv = ld4(dy, o, bf);
            gv.x *= scale; gv.y *= scale; gv.z *= scale; gv.w *= scale;
            if (lrelu) {
                const float slope = lrelu == 2 ? 0.f : 0.2f;  // 2 = ReLU
                float4 yv = ld4(y, o, bf);
                gv.x = yv.x > 0.f ? gv.x : slope * gv.x;
                gv.y = yv.y > 0.f ? gv.y : slope * gv.y;
                gv.z = yv.z > 0.f ? gv.z : slope * gv.z;
                gv.w = yv.w > 0.f ? gv.w : slope * gv.w;
            }
            if (dx) st4(dx, o, gv, bf);
            a.v[0].x += gv.x; a.v[0].y += gv.y; a.v[0].z += gv.z; a.v[0].w += gv.w;
        }
    }
    block_reduce_store<1>(a, smem, g.cv, g.prow, g.CV, g.rpp, C, partial + ((long)g.b * nchunks + blockIdx.x) * C,
                          g.active && c < C);
}

// Backward prologue of  y = lrelu( d[b,c] * z + noise[b,w,h]*nw[c] + nb[c] ):
//   gz = gy * lrelu'(y)                       (written; the conv gradients apply d while staging)
//   S0[b,c] = sum gz * (d*z)   with d*z = lrelu^-1(y) - noise   => grad wrt d is S0 / d
//   S1[b,c] = sum gz * noise_plane[b,w,h]     => grad wrt noise weight (summed over b by the caller)
//   S2[b,c] = sum gz                          => grad wrt noise bias
__global__ __launch_bounds__(NT) void modconv_bwd_prep_kernel(const void* __restrict__ gy, const void* __restrict__ y,
                                                             const float* __restrict__ noise, int ns,
                                                             const float* __restrict__ nw, const float* __restrict__ nb,
                                                             void* __restrict__ gz, float* __restrict__ partial, int H,
                                                             int W, int C, int nchunks, int lrelu, int bf,
                                                             const float* __restrict__ gz_scale, int natural) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int HW = H * W;
    Geo g = make_geo(HW, C, nchunks);
    Acc<3> a;
    a.zero();
    const int c = g.cv * 4;
    if (g.active && c < C) {
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f), b4 = w4;
        if (noise) {
            w4 = ldp4(nw + c);
            b4 = ldp4(nb + c);
        }
        float4 d4 = make_float4(1.f, 1.f, 1.f, 1.f);
        if (gz_scale) d4 = ldp4(gz_scale + (long)g.b * C + c);
        const long base = (long)g.b * HW;
        PixWalk pw((int)(g.p_begin + g.prow), g.rpp, W);  // p < H*W fits 32 bits; one division per lane, none per pixel
        for (long p = g.p_begin + g.prow; p < g.p_end; p += g.rpp, pw.advance()) {
            const long o = (base + p) * C + c;
            float4 gv = ld4(gy, o, bf);
            float4 yv = ld4(y, o, bf);
            float nz = 0.f;
            if (noise) nz = noise[noise_off(g.b, ns, pw.h, pw.w, natural)];
            float4 t = yv;  // pre-activation
            if (lrelu) {
                gv.x = yv.x > 0.f ? gv.x : 0.2f * gv.x; t.x = yv.x > 0.f ? yv.x : 5.f * yv.x;
                gv.y = yv.y > 0.f ? gv.y : 0.2f * gv.y; t.y = yv.y > 0.f ? yv.y : 5.f * yv.y;
                gv.z = yv.z > 0.f ? gv.z : 0.2f * gv.z; t.z = yv.z > 0.f ? yv.z : 5.f * yv.z;
                gv.w = yv.w > 0.f ? gv.w : 0.2f * gv.w; t.w = yv.w > 0.f ? yv.w : 5.f * yv.w;
            }
            // the STORED gradient optionally carries the demodulation coefficient d[b][c] (both consumers — the data
            // gradient and the weight gradient — want gz * d; folding it here makes their operands scale-free, so the
            // data gradient can take the LDS-DMA kernel); the sums below use the unscaled value
            if (gz_scale) st4(gz, o, make_float4(gv.x * d4.x, gv.y * d4.y, gv.z * d4.z, gv.w * d4.w), bf);
            else st4(gz, o, gv, bf);
            a.v[0].x += gv.x * (t.x - (nz * w4.x + b4.x));
            a.v[0].y += gv.y * (t.y - (nz * w4.y + b4.y));
            a.v[0].z += gv.z * (t.z - (nz * w4.z + b4.z));
            a.v[0].w += gv.w * (t.w - (nz * w4.w + b4.w));
            a.v[1].x += gv.x * nz; a.v[1].y += gv.y * nz; a.v[1].z += gv.z * nz; a.v[1].w += gv.w * nz;
            a.v[2].x += gv.x; a.v[2].y += gv.y; a.v[2].z += gv.z; a.v[2].w += gv.w;
        }
    }
    block_reduce_store<3>(a, smem, g.cv, g.prow, g.CV, g.rpp, C, partial + ((long)g.b * nchunks + blockIdx.x) * 3 * C,
                          g.active && c < C);
}

// gx = t * s[b,c];  partial[b][chunk][c] = sum_pixels x * t     (grad wrt the modulation scale)
__global__ __launch_bounds__(NT) void scale_reduce_kernel(const void* __restrict__ x, const void* __restrict__ t,
                                                         const float* __restrict__ s, void* __restrict__ gx,
                                                         float* __restrict__ partial, int HW, int C, int nchunks, int bf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    Geo g = make_geo(HW, C, nchunks);
    Acc<1> a;
    a.zero();
    const int c = g.cv * 4;
    if (g.active && c < C) {
        float4 s4 = ldp4(s + (long)g.b * C + c);
        const long base = (long)g.b * HW;
        for (long p = g.p_begin + g.prow; p < g.p_end; p += g.rpp) {
            const long o = (base + p) * C + c;
            float4 tv = ld4(t, o, bf);
            float4 xv = ld4(x, o, bf);
            a.v[0].x += xv.x * tv.x; a.v[0].y += xv.y * tv.y; a.v[0].z += xv.z * tv.z; a.v[0].w += xv.w * tv.w;
            if (gx) {
                tv.x *= s4.x; tv.y *= s4.y; tv.z *= s4.z; tv.w *= s4.w;
                st4(gx, o, tv, bf);
            }
        }
    }
    block_reduce_store<1>(a, smem, g.cv, g.prow, g.CV, g.rpp, C, partial + ((long)g.b * nchunks + blockIdx.x) * C,
                          g.active && c < C);
}

// ---- 16-byte lanes (bf16, C % 8 == 0, 16-byte aligned pointers) ------------------------------------------------------
// modconv_bwd_prep and scale_reduce with 8 channels per lane — one 16-byte access per tensor and pixel, as the elementwise
// kernels that reach the HBM rate have — and two pixels per iteration, both pixels' loads issued before the first use.  The
// geometry is the 4-channel one with two neighbouring lanes merged: the same block ranges, the same pixel rows (rpp), so a
// block has at most NT8 = 128 active lanes, each adding, per channel, the same pixels in the same order as the 4-channel
// lane of that channel, and the LDS pass adds the same rows in the same order.  Outputs AND sums are the 4-channel kernels'
// bits (an untrained GAN amplifies a last-bit difference of a gradient sum within a few steps: a re-associated sum would
// change what a training run computes).  act_bwd_reduce keeps its 4-channel lanes: the same form of it was measured at
// par at >= 64 px (-2.5 ... +2 %) and 5 % faster only at 32 px, so it was not kept (kernel table).
constexpr int NT8 = NT / 2;
struct L8 {
    float e[8];
};
__device__ __forceinline__ uint4 ldraw8(const void* p, long off) {
    return *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(p) + off);
}
__device__ __forceinline__ L8 unpack8(const uint4& h) {
    L8 r;
    r.e[0] = act_lo(h.x); r.e[1] = act_hi(h.x); r.e[2] = act_lo(h.y); r.e[3] = act_hi(h.y);
    r.e[4] = act_lo(h.z); r.e[5] = act_hi(h.z); r.e[6] = act_lo(h.w); r.e[7] = act_hi(h.w);
    return r;
}
__device__ __forceinline__ L8 ld8(const void* p, long off) { return unpack8(ldraw8(p, off)); }
__device__ __forceinline__ void st8(void* p, long off, const L8& v) {
    *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(p) + off) =
        make_uint4(act_pack2(v.e[0], v.e[1]), act_pack2(v.e[2], v.e[3]), act_pack2(v.e[4], v.e[5]), act_pack2(v.e[6], v.e[7]));
}
__device__ __forceinline__ L8 ldp8(const float* p) {
    const float4 a = ldp4(p), b = ldp4(p + 4);
    return L8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}

struct Geo8 {
    int b, cv, prow, CV, rpp;
    int p_begin, p_end;
    bool active;
};
__device__ __forceinline__ Geo8 make_geo8(int HW, int C, int nchunks) {
    Geo8 g;
    g.CV = C >> 3;            // <= 128: C <= 1024
    g.rpp = NT / (C >> 2);    // the pixel rows of the 4-channel geometry: at most NT8 lanes are active
    g.cv = threadIdx.x % g.CV;
    g.prow = threadIdx.x / g.CV;
    g.active = g.prow < g.rpp;
    g.b = blockIdx.y;
    const long per = ((long)HW + nchunks - 1) / nchunks;  // the ranges of make_geo
    const long pb = (long)blockIdx.x * per;
    g.p_begin = (int)(pb < HW ? pb : HW);
    g.p_end = (int)(pb + per < HW ? pb + per : HW);
    return g;
}

// smem [K][rpp][CV] x 8 floats; partial[b][chunk][k][c .. c+7]
template <int K>
__device__ __forceinline__ void block_reduce_store8(const L8 (&a)[K], float* smem, const Geo8& g, int C, float* partial_row) {
    float4* s4 = reinterpret_cast<float4*>(smem);
    if (g.active) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int at = ((k * g.rpp + g.prow) * g.CV + g.cv) * 2;
            s4[at] = make_float4(a[k].e[0], a[k].e[1], a[k].e[2], a[k].e[3]);
            s4[at + 1] = make_float4(a[k].e[4], a[k].e[5], a[k].e[6], a[k].e[7]);
        }
    }
    __syncthreads();
    if (g.active && g.prow == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f), u = t;
            for (int r = 0; r < g.rpp; ++r) {
                const int at = ((k * g.rpp + r) * g.CV + g.cv) * 2;
                const float4 x = s4[at], y = s4[at + 1];
                t.x += x.x; t.y += x.y; t.z += x.z; t.w += x.w;
                u.x += y.x; u.y += y.y; u.z += y.z; u.w += y.w;
            }
            float4* d = reinterpret_cast<float4*>(partial_row + (long)k * C + g.cv * 8);
            d[0] = t;
            d[1] = u;
        }
    }
}

__global__ __launch_bounds__(NT8) void modconv_bwd_prep_wide_kernel(const void* __restrict__ gy, const void* __restrict__ y,
                                                                  const float* __restrict__ noise, int ns,
                                                                  const float* __restrict__ nw, const float* __restrict__ nb,
                                                                  void* __restrict__ gz, float* __restrict__ partial, int H,
                                                                  int W, int C, int nchunks, int lrelu,
                                                                  const float* __restrict__ gz_scale, int natural) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int HW = H * W;
    const Geo8 g = make_geo8(HW, C, nchunks);
    L8 a[3] = {};
    if (g.active) {
        const int c = g.cv * 8;
        L8 w8 = {}, b8 = {}, d8 = {};
        if (noise) {
            w8 = ldp8(nw + c);
            b8 = ldp8(nb + c);
        }
        if (gz_scale) d8 = ldp8(gz_scale + (long)g.b * C + c);
        const long step = (long)g.rpp * C;
        long o = ((long)g.b * HW + g.p_begin + g.prow) * C + c;
        PixWalk pw(g.p_begin + g.prow, g.rpp, W);
        for (int p = g.p_begin + g.prow; p < g.p_end; p += 2 * g.rpp, o += 2 * step, pw.advance()) {
            const bool two = p + g.rpp < g.p_end;
            const long o1 = two ? o + step : o;
            const int h0 = pw.h, w0 = pw.w;
            pw.advance();
            const int h1 = two ? pw.h : h0, w1 = two ? pw.w : w0;  // (never an index past the plane)
            const L8 g0 = ld8(gy, o), g1 = ld8(gy, o1), y0 = ld8(y, o), y1 = ld8(y, o1);
            float nz0 = 0.f, nz1 = 0.f;
            if (noise) {
                nz0 = noise[noise_off(g.b, ns, h0, w0, natural)];
                nz1 = noise[noise_off(g.b, ns, h1, w1, natural)];
            }
            L8 q0, q1, t0 = y0, t1 = y1, s0, s1;  // gradient, pre-activation, stored value
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                q0.e[e] = g0.e[e];
                q1.e[e] = g1.e[e];
                if (lrelu) {
                    q0.e[e] = y0.e[e] > 0.f ? g0.e[e] : 0.2f * g0.e[e];
                    t0.e[e] = y0.e[e] > 0.f ? y0.e[e] : 5.f * y0.e[e];
                    q1.e[e] = y1.e[e] > 0.f ? g1.e[e] : 0.2f * g1.e[e];
                    t1.e[e] = y1.e[e] > 0.f ? y1.e[e] : 5.f * y1.e[e];
                }
                s0.e[e] = gz_scale ? q0.e[e] * d8.e[e] : q0.e[e];
                s1.e[e] = gz_scale ? q1.e[e] * d8.e[e] : q1.e[e];
            }
            st8(gz, o, s0);
            if (two) st8(gz, o1, s1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a[0].e[e] += q0.e[e] * (t0.e[e] - (nz0 * w8.e[e] + b8.e[e]));
                a[1].e[e] += q0.e[e] * nz0;
                a[2].e[e] += q0.e[e];
            }
            if (two) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    a[0].e[e] += q1.e[e] * (t1.e[e] - (nz1 * w8.e[e] + b8.e[e]));
                    a[1].e[e] += q1.e[e] * nz1;
                    a[2].e[e] += q1.e[e];
                }
            }
        }
    }
    block_reduce_store8<3>(a, smem, g, C, partial + ((long)g.b * nchunks + blockIdx.x) * 3 * C);
}

__global__ __launch_bounds__(NT8) void scale_reduce_wide_kernel(const void* __restrict__ x, const void* __restrict__ t,
                                                              const float* __restrict__ s, void* __restrict__ gx,
                                                              float* __restrict__ partial, int HW, int C, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Geo8 g = make_geo8(HW, C, nchunks);
    L8 a[1] = {};
    if (g.active) {
        const int c = g.cv * 8;
        const L8 s8 = ldp8(s + (long)g.b * C + c);
        const long step = (long)g.rpp * C;
        long o = ((long)g.b * HW + g.p_begin + g.prow) * C + c;
        for (int p = g.p_begin + g.prow; p < g.p_end; p += 2 * g.rpp, o += 2 * step) {
            const bool two = p + g.rpp < g.p_end;
            const long o1 = two ? o + step : o;
            L8 t0 = ld8(t, o), t1 = ld8(t, o1);
            const L8 x0 = ld8(x, o), x1 = ld8(x, o1);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[0].e[e] += x0.e[e] * t0.e[e];
            if (two) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a[0].e[e] += x1.e[e] * t1.e[e];
            }
            if (gx) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    t0.e[e] *= s8.e[e];
                    t1.e[e] *= s8.e[e];
                }
                st8(gx, o, t0);
                if (two) st8(gx, o1, t1);
            }
        }
    }
    block_reduce_store8<1>(a, smem, g, C, partial + ((long)g.b * nchunks + blockIdx.x) * C);
}

inline size_t reduce_smem8(int C, int K) { return (size_t)K * (NT / (C >> 2)) * (C >> 3) * 32; }

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }  // true for NULL
// bf16 tensors whose every pixel is a whole number of 16-byte vectors; STYLEX_GLUE_WIDE=0 forces the 4-channel lanes
// (read per launch: A/B tests toggle it in-process)
inline bool glue_wide(int act_dtype, int C) {
    const char* env = getenv("STYLEX_GLUE_WIDE");
    return act_dtype == 1 && C % 8 == 0 && !(env && env[0] == '0');
}

inline size_t reduce_smem(int C, int K) {
    int CV = (C + 3) / 4;
    if (CV > NT) CV = NT;
    int rpp = NT / CV;
    return (size_t)K * rpp * CV * 16;
}

inline bool ok_shape(const int64_t* sh, int nchunks) {
    return sh[0] > 0 && sh[1] > 0 && sh[2] > 0 && sh[3] > 0 && sh[3] <= 1024 && (sh[3] % 4 == 0) && nchunks > 0 &&
           sh[0] <= 65535;
}

}  // namespace

extern "C" {

int stylex_reduce_chunks(const int64_t* sh) {
    // blocks ~ 2048 in total, at least 64 pixels per block
    long HW = (long)sh[1] * sh[2];
    long n = (2048 + sh[0] - 1) / sh[0];
    long maxc = (HW + 63) / 64;
    if (n > maxc) n = maxc;
    if (n < 1) n = 1;
    return (int)n;
}

int stylex_act_bwd_reduce(const void* dy, const void* y, void* dx, float* partial, const int64_t* sh, int nchunks,
                          int lrelu, float scale, int act_dtype, void* stream) {
    if (act_dtype != 0 && act_dtype != 1) return STYLEX_EINVAL;
    if (!dy || !partial || !ok_shape(sh, nchunks) || (lrelu && !y)) return STYLEX_EINVAL;
    int HW = (int)(sh[1] * sh[2]), C = (int)sh[3];
    hipLaunchKernelGGL(act_bwd_reduce_kernel, dim3(nchunks, (unsigned)sh[0]), dim3(NT), reduce_smem(C, 1),
                       (hipStream_t)stream, dy, y, dx, partial, HW, C, nchunks, lrelu, scale, act_dtype);
    return (int)hipGetLastError();
}

static int modconv_bwd_prep_impl(const void* gy, const void* y, const float* noise, int64_t noise_stride,
                                 const float* noise_w, const float* noise_b, void* gz, float* partial, const int64_t* sh,
                                 int nchunks, int lrelu, int act_dtype, const float* gz_scale, int natural, void* stream);

int stylex_modconv_bwd_prep(const void* gy, const void* y, const float* noise, int64_t noise_stride,
                            const float* noise_w, const float* noise_b, void* gz, float* partial, const int64_t* sh,
                            int nchunks, int lrelu, int act_dtype, void* stream) {
    return modconv_bwd_prep_impl(gy, y, noise, noise_stride, noise_w, noise_b, gz, partial, sh, nchunks, lrelu, act_dtype,
                                 nullptr, 0, stream);
}

int stylex_modconv_bwd_prep_scaled(const void* gy, const void* y, const float* noise, int64_t noise_stride,
                                   const float* noise_w, const float* noise_b, const float* gz_scale, void* gz,
                                   float* partial, const int64_t* sh, int nchunks, int lrelu, int act_dtype, void* stream) {
    if (!gz_scale || (reinterpret_cast<uintptr_t>(gz_scale) & 15)) return STYLEX_EINVAL;
    return modconv_bwd_prep_impl(gy, y, noise, noise_stride, noise_w, noise_b, gz, partial, sh, nchunks, lrelu, act_dtype,
                                 gz_scale, 0, stream);
}

// The same pass over the noise plane in NATURAL order, noise[b][h][w] (stride noise_stride in both directions): the
// plane the forward's epilogue read.  gz_scale may be NULL (unscaled gz).
int stylex_modconv_bwd_prep_nat(const void* gy, const void* y, const float* noise, int64_t noise_stride,
                                const float* noise_w, const float* noise_b, const float* gz_scale, void* gz, float* partial,
                                const int64_t* sh, int nchunks, int lrelu, int act_dtype, void* stream) {
    if (!noise || (reinterpret_cast<uintptr_t>(gz_scale) & 15)) return STYLEX_EINVAL;
    return modconv_bwd_prep_impl(gy, y, noise, noise_stride, noise_w, noise_b, gz, partial, sh, nchunks, lrelu, act_dtype,
                                 gz_scale, 1, stream);
}

static int modconv_bwd_prep_impl(const void* gy, const void* y, const float* noise, int64_t noise_stride,
                                 const float* noise_w, const float* noise_b, void* gz, float* partial, const int64_t* sh,
                                 int nchunks, int lrelu, int act_dtype, const float* gz_scale, int natural, void* stream) {
    if (act_dtype != 0 && act_dtype != 1) return STYLEX_EINVAL;
    // 0 = linear, 1 = LeakyReLU(0.2).  No ReLU mode: S0 needs the pre-activation, which y = 0 does not determine
    if (lrelu != 0 && lrelu != 1) return STYLEX_EINVAL;
    if (!gy || !y || !gz || !partial || !ok_shape(sh, nchunks)) return STYLEX_EINVAL;
    if (noise && (!noise_w || !noise_b || noise_stride < sh[1] || noise_stride < sh[2])) return STYLEX_EINVAL;
    int C = (int)sh[3];
    if (glue_wide(act_dtype, C) && al16(gy) && al16(y) && al16(gz) && al16(partial) && al16(noise_w) && al16(noise_b) &&
        al16(gz_scale)) {
        hipLaunchKernelGGL(modconv_bwd_prep_wide_kernel, dim3(nchunks, (unsigned)sh[0]), dim3(NT8), reduce_smem8(C, 3),
                           (hipStream_t)stream, gy, y, noise, (int)noise_stride, noise_w, noise_b, gz, partial, (int)sh[1],
                           (int)sh[2], C, nchunks, lrelu, gz_scale, natural);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(modconv_bwd_prep_kernel, dim3(nchunks, (unsigned)sh[0]), dim3(NT), reduce_smem(C, 3),
                       (hipStream_t)stream, gy, y, noise, (int)noise_stride, noise_w, noise_b, gz, partial, (int)sh[1],
                       (int)sh[2], C, nchunks, lrelu, act_dtype, gz_scale, natural);
    return (int)hipGetLastError();
}

int stylex_scale_reduce(const void* x, const void* t, const float* s, void* gx, float* partial, const int64_t* sh,
                        int nchunks, int act_dtype, void* stream) {
    if (act_dtype != 0 && act_dtype != 1) return STYLEX_EINVAL;
    if (!x || !t || !s || !partial || !ok_shape(sh, nchunks)) return STYLEX_EINVAL;
    int HW = (int)(sh[1] * sh[2]), C = (int)sh[3];
    if (glue_wide(act_dtype, C) && al16(x) && al16(t) && al16(s) && al16(gx) && al16(partial)) {
        hipLaunchKernelGGL(scale_reduce_wide_kernel, dim3(nchunks, (unsigned)sh[0]), dim3(NT8), reduce_smem8(C, 1),
                           (hipStream_t)stream, x, t, s, gx, partial, HW, C, nchunks);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(scale_reduce_kernel, dim3(nchunks, (unsigned)sh[0]), dim3(NT), reduce_smem(C, 1),
                       (hipStream_t)stream, x, t, s, gx, partial, HW, C, nchunks, act_dtype);
    return (int)hipGetLastError();
}

}  // extern "C"
