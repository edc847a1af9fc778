// linattn.hip — the linear-attention blocks of attn_layers (reference stylex/stylex_train.py:100-206) on NHWC
// activations, fp32 or bf16 in HBM, every sum and exponential in fp32.
//
//   attention core   per (sample, head), 64 channels per head, N = H*W pixels:
//                      K = softmax over the PIXELS of k (per channel d),  Q = softmax over the CHANNELS of q * 64^-0.5
//                      C[d,e] = sum_n K[n,d] v[n,e]      P[n,e] = sum_d Q[n,d] C[d,e]      y = gelu_erf(P)
//       forward  1  linattn_ctx_partial   reads k, v once: a block owns a pixel range, keeps the running column max / sum
//                                         (online soft-max) and its 64x64 partial of C
//                2  linattn_ctx_combine   rescales and adds the partials in chunk order -> C, lse[d] = max + log(sum)
//                3  linattn_out           reads q once: row soft-max, P = Q C, writes P (the backward's gelu') and y
//       backward 1  linattn_bwd_q         reads q, P, gy once: G = gy * gelu'(P),  dQ = G C^T -> dq through the row
//                                         soft-max;  its 64x64 partial of dC = Q^T G
//                2  linattn_dctx_combine  adds the partials in chunk order -> dC;  r[d] = sum_e dC[d,e] C[d,e], which is
//                                         the per-column term sum_n K[n,d] dK[n,d] of the column soft-max: no extra pass
//                3  linattn_bwd_kv        reads k, v once: K = exp(k - lse),  dv = K dC,  dk = K * (v dC^T - r)
//   ChanNorm         (x - mean) / (sqrt(biased var) + eps) * g + b over the channels of a pixel: C/4 lanes per pixel,
//                    wave-shuffle reductions; dg / db as per-block partials
//   depthwise 3x3    pad 1, no bias; its data gradient is the same kernel on the mirrored taps (the caller flips the
//                    nine weights); the weight gradient as per-block partials of the 9 per-channel sums
//
// Every reduction over pixels or batch has a fixed order: per-block partials (fixed shuffle / LDS order inside a block),
// then a second launch that adds the slices in index order.  No atomics.
//
// The 64-wide contractions run on the vector ALU from LDS tiles (a thread owns a 4x4 or 2x4 patch of the output, both
// operands are read K-major as 8/16-byte LDS loads), fp32 in both precision modes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

constexpr int NT = 256;
constexpr int HD = 64;        // channels per head
constexpr int TP = 32;        // pixels per tile
constexpr int LDT = TP + 2;   // row stride of a transposed tile [HD][TP]: 8-byte aligned rows, 4-way store conflicts at most
constexpr int MAXCHUNK = 64;  // pixel chunks per (sample, head)

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// acc[r][c] += sum_kk A[kk * lda + i0 + r] * B[kk * ldb + j0 + c]   (both operands K-major in LDS)
template <int MI>
__device__ __forceinline__ void mac_tile(float (&acc)[MI][4], const float* A, int lda, int i0, const float* B, int ldb, int j0,
                                         int K) {
#pragma unroll 4
    for (int kk = 0; kk < K; ++kk) {
        float a[MI];
        if (MI == 4) {
            const float4 t = *reinterpret_cast<const float4*>(A + kk * lda + i0);
            a[0] = t.x, a[1] = t.y, a[2] = t.z, a[3] = t.w;
        } else {
            const float2 t = *reinterpret_cast<const float2*>(A + kk * lda + i0);
            a[0] = t.x, a[1] = t.y;
        }
        const float4 b = *reinterpret_cast<const float4*>(B + kk * ldb + j0);
#pragma unroll
        for (int r = 0; r < MI; ++r) {
            acc[r][0] += a[r] * b.x;
            acc[r][1] += a[r] * b.y;
            acc[r][2] += a[r] * b.z;
            acc[r][3] += a[r] * b.w;
        }
    }
}

__device__ __forceinline__ float row16_max(float v) {
    for (int o = 8; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    for (int o = 8; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Q = softmax over the 64 channels of a head * scale, for the 4 channels a thread holds; the 16 lanes of a pixel are
// consecutive lanes of one wave
__device__ __forceinline__ float4 row_softmax_scaled(float4 q, float scale) {
    const float m = row16_max(fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
    float4 e = make_float4(expf(q.x - m), expf(q.y - m), expf(q.z - m), expf(q.w - m));
    const float s = scale / row16_sum(e.x + e.y + e.z + e.w);
    return make_float4(e.x * s, e.y * s, e.z * s, e.w * s);
}

struct Strides {
    long q_px, q_b, k_px, k_b, v_px, v_b;  // element strides between pixels / samples of q, k, v (channel stride 1)
};

// ------------------------------------------------------------------------------------------------------------------
// forward 1: partial context of a pixel chunk.  grid (chunks, heads, B)
template <bool BF>
__global__ __launch_bounds__(NT) void linattn_ctx_partial(const void* __restrict__ k, const void* __restrict__ v, Strides st,
                                                         int HW, int chunk, float* __restrict__ pctx,
                                                         float* __restrict__ pmax, float* __restrict__ psum) {
    __shared__ __align__(16) float ks[TP * HD];  // k, then exp(k - max): [n][d]
    __shared__ __align__(16) float vs[TP * HD];  // [n][e]
    __shared__ float redm[4][HD], reds[4][HD], alpha_s[HD];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y, nch = gridDim.x;
    const int p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, HW);
    const long kb = (long)b * st.k_b + h * HD, vb = (long)b * st.v_b + h * HD;
    const int d = tid & 63, part = tid >> 6;  // column soft-max: 4 row groups of 8 pixels per column
    const int ig = tid >> 4, jg = tid & 15;   // contraction: rows d = 4 ig .., columns e = 4 jg ..
    float m_run = -INFINITY, s_run = 0.f;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int t0 = p0; t0 < p1; t0 += TP) {
        for (int idx = tid; idx < TP * 16; idx += NT) {
            const int n = idx >> 4, c4 = idx & 15, p = t0 + n;
            float4 kq = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), vq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < p1) {
                kq = act_ld4<BF>(k, kb + (long)p * st.k_px + c4 * 4);
                vq = act_ld4<BF>(v, vb + (long)p * st.v_px + c4 * 4);
            }
            *reinterpret_cast<float4*>(&ks[n * HD + c4 * 4]) = kq;
            *reinterpret_cast<float4*>(&vs[n * HD + c4 * 4]) = vq;
        }
        __syncthreads();
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 8; ++r) mx = fmaxf(mx, ks[(part * 8 + r) * HD + d]);
        redm[part][d] = mx;
        __syncthreads();
        // the tile holds at least one pixel, so the new maximum is finite; exp(-inf - finite) = 0 on the first tile
        const float m_new = fmaxf(m_run, fmaxf(fmaxf(redm[0][d], redm[1][d]), fmaxf(redm[2][d], redm[3][d])));
        const float al = expf(m_run - m_new);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float e = expf(ks[(part * 8 + r) * HD + d] - m_new);
            ks[(part * 8 + r) * HD + d] = e;
            ps += e;
        }
        reds[part][d] = ps;
        if (part == 0) alpha_s[d] = al;
        m_run = m_new;
        __syncthreads();
        s_run = s_run * al + (((reds[0][d] + reds[1][d]) + reds[2][d]) + reds[3][d]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = alpha_s[ig * 4 + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] *= a;
        }
        mac_tile<4>(acc, ks, HD, ig * 4, vs, HD, jg * 4, TP);
        __syncthreads();
    }
    const long slot = ((long)b * heads + h) * nch + blockIdx.x;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4*>(pctx + slot * (HD * HD) + (ig * 4 + r) * HD + jg * 4) =
            make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    if (part == 0) {
        pmax[slot * HD + d] = m_run;
        psum[slot * HD + d] = s_run;
    }
}

// forward 2: grid (heads, B).  context[d][e] = sum_c pctx[c][d][e] exp(m_c[d] - M[d]) / S[d], chunks in index order
__global__ __launch_bounds__(NT) void linattn_ctx_combine(const float* __restrict__ pctx, const float* __restrict__ pmax,
                                                         const float* __restrict__ psum, int nch, float* __restrict__ context,
                                                         float* __restrict__ lse) {
    __shared__ float M_s[HD], invS_s[HD];
    const int tid = threadIdx.x;
    const long bh = (long)blockIdx.y * gridDim.x + blockIdx.x;
    const float* pm = pmax + bh * nch * HD;
    if (tid < HD) {
        float M = -INFINITY;
        for (int c = 0; c < nch; ++c) M = fmaxf(M, pm[c * HD + tid]);
        float S = 0.f;
        for (int c = 0; c < nch; ++c) S += psum[(bh * nch + c) * HD + tid] * expf(pm[c * HD + tid] - M);
        M_s[tid] = M;
        invS_s[tid] = 1.f / S;
        lse[bh * HD + tid] = M + logf(S);
    }
    __syncthreads();
    for (int i = tid; i < HD * HD; i += NT) {
        const int d = i >> 6;
        float a = 0.f;
        for (int c = 0; c < nch; ++c) a += pctx[(bh * nch + c) * (HD * HD) + i] * expf(pm[c * HD + d] - M_s[d]);
        context[bh * (HD * HD) + i] = a * invS_s[d];
    }
}

// forward 3: grid (chunks, heads, B).  pre[n][e] = sum_d Q[n][d] C[d][e];  y = gelu(pre).  pre / y: dense [B][HW][heads*64]
template <bool BF>
__global__ __launch_bounds__(NT) void linattn_out(const void* __restrict__ q, Strides st, const float* __restrict__ context,
                                                 int HW, int chunk, void* __restrict__ pre, void* __restrict__ y) {
    __shared__ __align__(16) float cs[HD * HD];   // [d][e]
    __shared__ __align__(16) float qT[HD * LDT];  // [d][n]
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    const int p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, HW);
    const long qb = (long)b * st.q_b + h * HD;
    const long inner = (long)heads * HD;
    const int ig = tid >> 4, jg = tid & 15;  // the thread loads AND produces pixels 2 ig, 2 ig + 1, channels 4 jg ..
    const float* cg = context + ((long)b * heads + h) * (HD * HD);
    for (int i = tid; i < HD * HD; i += NT) cs[i] = cg[i];
    for (int t0 = p0; t0 < p1; t0 += TP) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int n = ig * 2 + r, p = t0 + n;
            float4 qq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < p1) qq = act_ld4<BF>(q, qb + (long)p * st.q_px + jg * 4);
            qq = row_softmax_scaled(qq, 0.125f);
            qT[(jg * 4 + 0) * LDT + n] = qq.x;
            qT[(jg * 4 + 1) * LDT + n] = qq.y;
            qT[(jg * 4 + 2) * LDT + n] = qq.z;
            qT[(jg * 4 + 3) * LDT + n] = qq.w;
        }
        __syncthreads();
        float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        mac_tile<2>(acc, qT, LDT, ig * 2, cs, HD, jg * 4, HD);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int p = t0 + ig * 2 + r;
            if (p < p1) {
                const long off = ((long)b * HW + p) * inner + h * HD + jg * 4;
                act_st4<BF>(pre, off, make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]));
                act_st4<BF>(y, off, make_float4(gelu_erf(acc[r][0]), gelu_erf(acc[r][1]), gelu_erf(acc[r][2]), gelu_erf(acc[r][3])));
            }
        }
        __syncthreads();
    }
}

// backward 1: grid (chunks, heads, B).  dq dense [B][HW][heads*64]; pdc[b][h][chunk][d][e]
template <bool BF>
__global__ __launch_bounds__(NT) void linattn_bwd_q(const void* __restrict__ q, Strides st, const void* __restrict__ pre,
                                                   const void* __restrict__ gy, const float* __restrict__ context, int HW,
                                                   int chunk, void* __restrict__ dq, float* __restrict__ pdc) {
    __shared__ __align__(16) float cT[HD * HD];   // [e][d]
    __shared__ __align__(16) float Qn[TP * HD];   // [n][d]
    __shared__ __align__(16) float Gn[TP * HD];   // [n][e]
    __shared__ __align__(16) float GT[HD * LDT];  // [e][n]
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y, nch = gridDim.x;
    const int p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, HW);
    const long qb = (long)b * st.q_b + h * HD;
    const long inner = (long)heads * HD;
    const int ig = tid >> 4, jg = tid & 15;
    const float* cg = context + ((long)b * heads + h) * (HD * HD);
    for (int i = tid; i < HD * HD; i += NT) cT[i] = cg[(i & 63) * HD + (i >> 6)];  // i = e * 64 + d
    float dc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) dc[r][c] = 0.f;
    for (int t0 = p0; t0 < p1; t0 += TP) {
        float4 Q[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int n = ig * 2 + r, p = t0 + n;
            float4 qq = make_float4(0.f, 0.f, 0.f, 0.f), pp = qq, gg = qq;
            if (p < p1) {
                const long off = ((long)b * HW + p) * inner + h * HD + jg * 4;
                qq = act_ld4<BF>(q, qb + (long)p * st.q_px + jg * 4);
                pp = act_ld4<BF>(pre, off);
                gg = act_ld4<BF>(gy, off);
            }
            Q[r] = row_softmax_scaled(qq, 0.125f);
            const float4 G = make_float4(gg.x * gelu_erf_grad(pp.x), gg.y * gelu_erf_grad(pp.y), gg.z * gelu_erf_grad(pp.z),
                                         gg.w * gelu_erf_grad(pp.w));  // 0 for the pixels past the chunk's end
            *reinterpret_cast<float4*>(&Qn[n * HD + jg * 4]) = Q[r];
            *reinterpret_cast<float4*>(&Gn[n * HD + jg * 4]) = G;
            GT[(jg * 4 + 0) * LDT + n] = G.x;
            GT[(jg * 4 + 1) * LDT + n] = G.y;
            GT[(jg * 4 + 2) * LDT + n] = G.z;
            GT[(jg * 4 + 3) * LDT + n] = G.w;
        }
        __syncthreads();
        float a[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // dQ[n][d] = sum_e G[n][e] C[d][e]
        mac_tile<2>(a, GT, LDT, ig * 2, cT, HD, jg * 4, HD);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            // dq = Q * (dQ - sum_d' softmax[d'] dQ[d']),  Q = softmax * scale
            const float dot = row16_sum(Q[r].x * a[r][0] + Q[r].y * a[r][1] + Q[r].z * a[r][2] + Q[r].w * a[r][3]) * 8.f;
            const int p = t0 + ig * 2 + r;
            if (p < p1)
                act_st4<BF>(dq, ((long)b * HW + p) * inner + h * HD + jg * 4,
                            make_float4(Q[r].x * (a[r][0] - dot), Q[r].y * (a[r][1] - dot), Q[r].z * (a[r][2] - dot),
                                        Q[r].w * (a[r][3] - dot)));
        }
        mac_tile<4>(dc, Qn, HD, ig * 4, Gn, HD, jg * 4, TP);  // dC[d][e] += sum_n Q[n][d] G[n][e]
        __syncthreads();
    }
    const long slot = ((long)b * heads + h) * nch + blockIdx.x;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4*>(pdc + slot * (HD * HD) + (ig * 4 + r) * HD + jg * 4) = make_float4(dc[r][0], dc[r][1], dc[r][2], dc[r][3]);
}

// backward 2: grid (heads, B).  dC = sum of the chunk partials in index order;  r[d] = sum_e dC[d][e] C[d][e]
__global__ __launch_bounds__(NT) void linattn_dctx_combine(const float* __restrict__ pdc, const float* __restrict__ context,
                                                          int nch, float* __restrict__ dctx, float* __restrict__ rsum) {
    const int tid = threadIdx.x;
    const long bh = (long)blockIdx.y * gridDim.x + blockIdx.x;
    const int d = tid >> 2, e0 = (tid & 3) * 16;  // 4 consecutive lanes share a row
    float r = 0.f;
    for (int e = e0; e < e0 + 16; ++e) {
        const int i = d * HD + e;
        float a = 0.f;
        for (int c = 0; c < nch; ++c) a += pdc[(bh * nch + c) * (HD * HD) + i];
        dctx[bh * (HD * HD) + i] = a;
        r += a * context[bh * (HD * HD) + i];
    }
    r += __shfl_xor(r, 1);
    r += __shfl_xor(r, 2);
    if ((tid & 3) == 0) rsum[bh * HD + d] = r;
}

// backward 3: grid (chunks, heads, B).  dk, dv dense [B][HW][heads*64]
template <bool BF>
__global__ __launch_bounds__(NT) void linattn_bwd_kv(const void* __restrict__ k, const void* __restrict__ v, Strides st,
                                                    const float* __restrict__ lse, const float* __restrict__ dctx,
                                                    const float* __restrict__ rsum, int HW, int chunk, void* __restrict__ dk,
                                                    void* __restrict__ dv) {
    __shared__ __align__(16) float dCn[HD * HD];  // [d][e]
    __shared__ __align__(16) float dCT[HD * HD];  // [e][d]
    __shared__ __align__(16) float KT[HD * LDT];  // [d][n]
    __shared__ __align__(16) float VT[HD * LDT];  // [e][n]
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    const int p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, HW);
    const long bh = (long)b * heads + h;
    const long kb = (long)b * st.k_b + h * HD, vb = (long)b * st.v_b + h * HD;
    const long inner = (long)heads * HD;
    const int ig = tid >> 4, jg = tid & 15;
    const float* dg = dctx + bh * (HD * HD);
    for (int i = tid; i < HD * HD; i += NT) {
        dCn[i] = dg[i];
        dCT[i] = dg[(i & 63) * HD + (i >> 6)];
    }
    const float4 ls = *reinterpret_cast<const float4*>(lse + bh * HD + jg * 4);
    const float4 rs = *reinterpret_cast<const float4*>(rsum + bh * HD + jg * 4);
    for (int t0 = p0; t0 < p1; t0 += TP) {
        float4 K[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int n = ig * 2 + r, p = t0 + n;
            float4 vq = make_float4(0.f, 0.f, 0.f, 0.f);
            K[r] = vq;
            if (p < p1) {
                const float4 kq = act_ld4<BF>(k, kb + (long)p * st.k_px + jg * 4);
                vq = act_ld4<BF>(v, vb + (long)p * st.v_px + jg * 4);
                K[r] = make_float4(expf(kq.x - ls.x), expf(kq.y - ls.y), expf(kq.z - ls.z), expf(kq.w - ls.w));
            }
            KT[(jg * 4 + 0) * LDT + n] = K[r].x;
            KT[(jg * 4 + 1) * LDT + n] = K[r].y;
            KT[(jg * 4 + 2) * LDT + n] = K[r].z;
            KT[(jg * 4 + 3) * LDT + n] = K[r].w;
            VT[(jg * 4 + 0) * LDT + n] = vq.x;
            VT[(jg * 4 + 1) * LDT + n] = vq.y;
            VT[(jg * 4 + 2) * LDT + n] = vq.z;
            VT[(jg * 4 + 3) * LDT + n] = vq.w;
        }
        __syncthreads();
        float a[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // dv[n][e] = sum_d K[n][d] dC[d][e]
        mac_tile<2>(a, KT, LDT, ig * 2, dCn, HD, jg * 4, HD);
        float c[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // dK[n][d] = sum_e v[n][e] dC[d][e]
        mac_tile<2>(c, VT, LDT, ig * 2, dCT, HD, jg * 4, HD);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int p = t0 + ig * 2 + r;
            if (p < p1) {
                const long off = ((long)b * HW + p) * inner + h * HD + jg * 4;
                act_st4<BF>(dv, off, make_float4(a[r][0], a[r][1], a[r][2], a[r][3]));
                act_st4<BF>(dk, off, make_float4(K[r].x * (c[r][0] - rs.x), K[r].y * (c[r][1] - rs.y), K[r].z * (c[r][2] - rs.z),
                                                 K[r].w * (c[r][3] - rs.w)));
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------
// per-block reduction of NV per-thread sums over the threads that own the same channel group (tid % LP), in thread order
template <int NV>
__device__ __forceinline__ void block_reduce_by_group(const float (&acc)[NV], float* red /* [NT][NV + 1] */, int LP,
                                                      float* __restrict__ dst /* [LP * NV] */) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NV; ++i) red[tid * (NV + 1) + i] = acc[i];
    __syncthreads();
    for (int item = tid; item < LP * NV; item += NT) {
        const int grp = item / NV, val = item - grp * NV;
        float s = 0.f;
        for (int t = grp; t < NT; t += LP) s += red[t * (NV + 1) + val];
        dst[item] = s;
    }
}

// out[i] = (sum over the slices, in index order, of partial[s][i])
__global__ __launch_bounds__(NT) void reduce_slices_kernel(const float* __restrict__ partial, int slices, int n,
                                                          float* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < slices; ++k) s += partial[(long)k * n + i];
    out[i] = s;
}

// ChanNorm forward: C = 4 << lp_shift channels, LP = C / 4 lanes per pixel
template <bool BF>
__global__ __launch_bounds__(NT) void chan_norm_fwd_kernel(const void* __restrict__ x, const float* __restrict__ g,
                                                          const float* __restrict__ bias, void* __restrict__ y,
                                                          float* __restrict__ mean, float* __restrict__ stdv, long P, int lp_shift,
                                                          float eps) {
    const int LP = 1 << lp_shift, C = LP * 4, tid = threadIdx.x;
    const int cg = tid & (LP - 1), PPB = NT >> lp_shift;
    const float4 gg = *reinterpret_cast<const float4*>(g + cg * 4), bb = *reinterpret_cast<const float4*>(bias + cg * 4);
    const float inv_c = 1.f / (float)C;
    // the LP lanes of a pixel share p: they stay converged for the shuffles
    for (long p = (long)blockIdx.x * PPB + (tid >> lp_shift); p < P; p += (long)gridDim.x * PPB) {
        const float4 v = act_ld4<BF>(x, p * C + cg * 4);
        float s = (v.x + v.y) + (v.z + v.w);
        for (int o = LP >> 1; o; o >>= 1) s += __shfl_xor(s, o);
        const float mu = s * inv_c;
        const float4 d = make_float4(v.x - mu, v.y - mu, v.z - mu, v.w - mu);
        float q = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        for (int o = LP >> 1; o; o >>= 1) q += __shfl_xor(q, o);
        const float sd = sqrtf(q * inv_c), inv = 1.f / (sd + eps);
        act_st4<BF>(y, p * C + cg * 4,
                    make_float4(d.x * inv * gg.x + bb.x, d.y * inv * gg.y + bb.y, d.z * inv * gg.z + bb.z, d.w * inv * gg.w + bb.w));
        if (cg == 0) {
            mean[p] = mu;
            stdv[p] = sd;
        }
    }
}

// ChanNorm backward: one joint shuffle reduction (two sums) per pixel; partial[block][2][C] = (dg, db) of the block's pixels
template <bool BF>
__global__ __launch_bounds__(NT) void chan_norm_bwd_kernel(const void* __restrict__ x, const void* __restrict__ gy,
                                                          const float* __restrict__ g, const float* __restrict__ mean,
                                                          const float* __restrict__ stdv, void* __restrict__ gx,
                                                          float* __restrict__ partial, long P, int lp_shift, float eps,
                                                          long px_per_block) {
    __shared__ float red[NT * 9];
    const int LP = 1 << lp_shift, C = LP * 4, tid = threadIdx.x;
    const int cg = tid & (LP - 1), PPB = NT >> lp_shift;
    const float4 gg = *reinterpret_cast<const float4*>(g + cg * 4);
    const float inv_c = 1.f / (float)C;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const long p0 = (long)blockIdx.x * px_per_block, p1 = p0 + px_per_block < P ? p0 + px_per_block : P;
    for (long p = p0 + (tid >> lp_shift); p < p1; p += PPB) {
        const float4 v = act_ld4<BF>(x, p * C + cg * 4), go = act_ld4<BF>(gy, p * C + cg * 4);
        const float mu = mean[p], sd = stdv[p], inv = 1.f / (sd + eps);
        const float4 d = make_float4(v.x - mu, v.y - mu, v.z - mu, v.w - mu);
        const float4 gh = make_float4(go.x * gg.x, go.y * gg.y, go.z * gg.z, go.w * gg.w);
        float s1 = (gh.x + gh.y) + (gh.z + gh.w);
        float s2 = (gh.x * d.x + gh.y * d.y) + (gh.z * d.z + gh.w * d.w);
        for (int o = LP >> 1; o; o >>= 1) {
            s1 += __shfl_xor(s1, o);
            s2 += __shfl_xor(s2, o);
        }
        // y = d * inv * g + b, inv = 1 / (sd + eps):  dx = inv * (gh - mean(gh)) - inv^2 * sum(gh d) / (C sd) * d
        const float m1 = s1 * inv_c, coef = sd > 0.f ? inv * inv * s2 * inv_c / sd : 0.f;
        if (gx)
            act_st4<BF>(gx, p * C + cg * 4,
                        make_float4(inv * (gh.x - m1) - coef * d.x, inv * (gh.y - m1) - coef * d.y, inv * (gh.z - m1) - coef * d.z,
                                    inv * (gh.w - m1) - coef * d.w));
        acc[0] += go.x * d.x * inv, acc[1] += go.y * d.y * inv, acc[2] += go.z * d.z * inv, acc[3] += go.w * d.w * inv;
        acc[4] += go.x, acc[5] += go.y, acc[6] += go.z, acc[7] += go.w;
    }
    if (!partial) return;
    // group-major scratch row [cg][dg0..3, db0..3] -> partial[block][0][C] = dg, [1][C] = db
    float* row = partial + (long)blockIdx.x * 2 * C;
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) red[t * 9 + i] = acc[i];
    __syncthreads();
    for (int item = t; item < LP * 8; item += NT) {
        const int grp = item >> 3, val = item & 7;
        float s = 0.f;
        for (int u = grp; u < NT; u += LP) s += red[u * 9 + val];
        row[(val >> 2) * C + grp * 4 + (val & 3)] = s;
    }
}

// depthwise 3x3, pad 1: one thread per (pixel, 4 channels); w fp32 [C][9]
template <bool BF>
__global__ __launch_bounds__(NT) void dwconv3x3_kernel(const void* __restrict__ x, const float* __restrict__ w,
                                                      void* __restrict__ y, int B, int H, int W, int C) {
    const int C4 = C >> 2;
    const long idx = (long)blockIdx.x * NT + threadIdx.x, total = (long)B * H * W * C4;
    if (idx >= total) return;
    const int cg = (int)(idx % C4);
    const long pix = idx / C4;
    const int wq = (int)(pix % W), hq = (int)((pix / W) % H);
    const long b = pix / ((long)W * H);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* wc = w + (long)cg * 36;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = hq + kh - 1;
        if (ih < 0 || ih >= H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = wq + kw - 1;
            if (iw < 0 || iw >= W) continue;
            const float4 v = act_ld4<BF>(x, ((b * H + ih) * W + iw) * C + cg * 4);
            const int t = kh * 3 + kw;
            acc.x += v.x * wc[t];
            acc.y += v.y * wc[9 + t];
            acc.z += v.z * wc[18 + t];
            acc.w += v.w * wc[27 + t];
        }
    }
    act_st4<BF>(y, pix * C + cg * 4, acc);
}

// depthwise weight gradient: partial[block][C][9] = sum over the block's pixels of x[p + tap] * gy[p]
template <bool BF>
__global__ __launch_bounds__(NT) void dwconv3x3_wgrad_kernel(const void* __restrict__ x, const void* __restrict__ gy,
                                                            float* __restrict__ partial, int B, int H, int W, int lp_shift,
                                                            long px_per_block) {
    __shared__ float red[NT * 37];
    const int LP = 1 << lp_shift, C = LP * 4, tid = threadIdx.x;
    const int cg = tid & (LP - 1), PPB = NT >> lp_shift;
    const long P = (long)B * H * W;
    float acc[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) acc[i] = 0.f;
    const long p0 = (long)blockIdx.x * px_per_block, p1 = p0 + px_per_block < P ? p0 + px_per_block : P;
    for (long p = p0 + (tid >> lp_shift); p < p1; p += PPB) {
        const int wq = (int)(p % W), hq = (int)((p / W) % H);
        const float4 go = act_ld4<BF>(gy, p * C + cg * 4);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = hq + kh - 1;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iw = wq + kw - 1;
                if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
                const float4 v = act_ld4<BF>(x, (p + (long)(kh - 1) * W + (kw - 1)) * C + cg * 4);
                const int t = kh * 3 + kw;
                acc[t] += v.x * go.x;
                acc[9 + t] += v.y * go.y;
                acc[18 + t] += v.z * go.z;
                acc[27 + t] += v.w * go.w;
            }
        }
    }
    block_reduce_by_group<36>(acc, red, LP, partial + (long)blockIdx.x * C * 9);  // [cg][4][9] = [C][9]
}

inline int lp_shift_of(long C) {  // C = 4 << s, s in [0, 6]
    for (int s = 0; s <= 6; ++s)
        if (C == (4L << s)) return s;
    return -1;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline long stream_blocks(long P, int ppb_threads) {  // blocks of a pixel stream: >= 8 passes per block, <= 1024 blocks
    long n = (P + 8L * ppb_threads - 1) / (8L * ppb_threads);
    return n < 1 ? 1 : (n > 1024 ? 1024 : n);
}

struct AttnPlan {
    int B, HW, heads, nch, chunk;
};

inline bool attn_plan(const int64_t* sh, AttnPlan* pl) {
    if (sh[0] <= 0 || sh[0] > 65535 || sh[1] <= 0 || sh[1] > (1 << 30) || sh[2] <= 0 || sh[2] > 65535) return false;
    pl->B = (int)sh[0], pl->HW = (int)sh[1], pl->heads = (int)sh[2];
    // enough blocks to fill the chip (>= 2048 where the pixels allow it), whole tiles per chunk, <= MAXCHUNK chunks
    long want = (2048 + (long)pl->B * pl->heads - 1) / ((long)pl->B * pl->heads);
    const long tiles = (pl->HW + TP - 1) / TP;
    if (want > tiles) want = tiles;
    if (want > MAXCHUNK) want = MAXCHUNK;
    if (want < 1) want = 1;
    const long tiles_per = (tiles + want - 1) / want;
    pl->chunk = (int)(tiles_per * TP);
    pl->nch = (int)((pl->HW + pl->chunk - 1) / pl->chunk);
    return true;
}

inline bool strides_ok(const int64_t* s) {
    for (int i = 0; i < 6; ++i)
        if (s[i] <= 0 || (s[i] & 3)) return false;
    return true;
}

}  // namespace

extern "C" {

int stylex_linattn_chunks(const int64_t* sh) {
    AttnPlan pl;
    return attn_plan(sh, &pl) ? pl.nch : STYLEX_EINVAL;
}

int stylex_linattn_fwd(const void* q, const void* k, const void* v, const int64_t* strides, void* y, void* pre, float* context,
                       float* lse, float* workspace, const int64_t* sh, int act_dtype, void* stream) {
    AttnPlan pl;
    if (!q || !k || !v || !strides || !y || !pre || !context || !lse || !workspace || !sh || !attn_plan(sh, &pl) ||
        !strides_ok(strides))
        return STYLEX_EINVAL;
    const int esz = act_dtype ? 2 : 4;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
         reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(pre)) & (4 * esz - 1))
        return STYLEX_EINVAL;
    if (!aligned16(context) || !aligned16(workspace)) return STYLEX_EINVAL;
    const Strides st = {strides[0], strides[1], strides[2], strides[3], strides[4], strides[5]};
    const long slots = (long)pl.B * pl.heads * pl.nch;
    float *pctx = workspace, *pmax = pctx + slots * HD * HD, *psum = pmax + slots * HD;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(pl.nch, pl.heads, pl.B);
    if (act_dtype) {
        hipLaunchKernelGGL(linattn_ctx_partial<true>, grid, dim3(NT), 0, s, k, v, st, pl.HW, pl.chunk, pctx, pmax, psum);
    } else {
        hipLaunchKernelGGL(linattn_ctx_partial<false>, grid, dim3(NT), 0, s, k, v, st, pl.HW, pl.chunk, pctx, pmax, psum);
    }
    hipLaunchKernelGGL(linattn_ctx_combine, dim3(pl.heads, pl.B), dim3(NT), 0, s, pctx, pmax, psum, pl.nch, context, lse);
    stylex_note_kernel("linattn_out<%s>", act_dtype ? "true" : "false");
    if (act_dtype) {
        hipLaunchKernelGGL(linattn_out<true>, grid, dim3(NT), 0, s, q, st, context, pl.HW, pl.chunk, pre, y);
    } else {
        hipLaunchKernelGGL(linattn_out<false>, grid, dim3(NT), 0, s, q, st, context, pl.HW, pl.chunk, pre, y);
    }
    return (int)hipGetLastError();
}

int stylex_linattn_bwd(const void* q, const void* k, const void* v, const int64_t* strides, const void* pre, const void* gy,
                       const float* context, const float* lse, void* dq, void* dk, void* dv, float* workspace,
                       const int64_t* sh, int act_dtype, void* stream) {
    AttnPlan pl;
    if (!q || !k || !v || !strides || !pre || !gy || !context || !lse || !dq || !dk || !dv || !workspace || !sh ||
        !attn_plan(sh, &pl) || !strides_ok(strides))
        return STYLEX_EINVAL;
    const int esz = act_dtype ? 2 : 4;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
         reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(dq) |
         reinterpret_cast<uintptr_t>(dk) | reinterpret_cast<uintptr_t>(dv)) & (4 * esz - 1))
        return STYLEX_EINVAL;
    if (!aligned16(context) || !aligned16(lse) || !aligned16(workspace)) return STYLEX_EINVAL;
    const Strides st = {strides[0], strides[1], strides[2], strides[3], strides[4], strides[5]};
    const long slots = (long)pl.B * pl.heads * pl.nch, bh = (long)pl.B * pl.heads;
    float *pdc = workspace, *dctx = pdc + slots * HD * HD, *rsum = dctx + bh * HD * HD;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(pl.nch, pl.heads, pl.B);
    if (act_dtype) {
        hipLaunchKernelGGL(linattn_bwd_q<true>, grid, dim3(NT), 0, s, q, st, pre, gy, context, pl.HW, pl.chunk, dq, pdc);
    } else {
        hipLaunchKernelGGL(linattn_bwd_q<false>, grid, dim3(NT), 0, s, q, st, pre, gy, context, pl.HW, pl.chunk, dq, pdc);
    }
    hipLaunchKernelGGL(linattn_dctx_combine, dim3(pl.heads, pl.B), dim3(NT), 0, s, pdc, context, pl.nch, dctx, rsum);
    stylex_note_kernel("linattn_bwd_kv<%s>", act_dtype ? "true" : "false");
    if (act_dtype) {
        hipLaunchKernelGGL(linattn_bwd_kv<true>, grid, dim3(NT), 0, s, k, v, st, lse, dctx, rsum, pl.HW, pl.chunk, dk, dv);
    } else {
        hipLaunchKernelGGL(linattn_bwd_kv<false>, grid, dim3(NT), 0, s, k, v, st, lse, dctx, rsum, pl.HW, pl.chunk, dk, dv);
    }
    return (int)hipGetLastError();
}

int stylex_chan_norm_fwd(const void* x, const float* g, const float* b, void* y, float* mean, float* stdv, const int64_t* sh,
                         float eps, int act_dtype, void* stream) {
    if (!x || !g || !b || !y || !mean || !stdv || !sh || sh[0] <= 0 || !(eps >= 0.f)) return STYLEX_EINVAL;
    const int ls = lp_shift_of(sh[1]);
    if (ls < 0) return STYLEX_NOT_APPLICABLE;
    if (!aligned16(g) || !aligned16(b) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & (act_dtype ? 7 : 15)))
        return STYLEX_EINVAL;
    const long P = sh[0];
    const int PPB = NT >> ls;
    long blocks = (P + PPB - 1) / PPB;
    if (blocks > 4096) blocks = 4096;
    stylex_note_kernel("chan_norm_fwd_kernel<%s>", act_dtype ? "true" : "false");
    if (act_dtype) {
        hipLaunchKernelGGL(chan_norm_fwd_kernel<true>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, g, b, y, mean,
                           stdv, P, ls, eps);
    } else {
        hipLaunchKernelGGL(chan_norm_fwd_kernel<false>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, g, b, y,
                           mean, stdv, P, ls, eps);
    }
    return (int)hipGetLastError();
}

int stylex_chan_norm_bwd_blocks(const int64_t* sh) {
    const int ls = lp_shift_of(sh[1]);
    if (sh[0] <= 0 || ls < 0) return STYLEX_EINVAL;
    return (int)stream_blocks(sh[0], NT >> ls);
}

int stylex_chan_norm_bwd(const void* x, const void* gy, const float* g, const float* mean, const float* stdv, void* gx,
                         float* partial, float* dgb, const int64_t* sh, float eps, int act_dtype, void* stream) {
    if (!x || !gy || !g || !mean || !stdv || !sh || sh[0] <= 0 || (!gx && !partial) || (partial && !dgb) || !(eps >= 0.f))
        return STYLEX_EINVAL;
    const int ls = lp_shift_of(sh[1]);
    if (ls < 0) return STYLEX_NOT_APPLICABLE;
    if (!aligned16(g) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(gx)) &
                          (act_dtype ? 7 : 15)))
        return STYLEX_EINVAL;
    const long P = sh[0], blocks = stream_blocks(P, NT >> ls), ppb = (P + blocks - 1) / blocks;
    const int C = (int)sh[1];
    stylex_note_kernel("chan_norm_bwd_kernel<%s>", act_dtype ? "true" : "false");
    if (act_dtype) {
        hipLaunchKernelGGL(chan_norm_bwd_kernel<true>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, gy, g, mean,
                           stdv, gx, partial, P, ls, eps, ppb);
    } else {
        hipLaunchKernelGGL(chan_norm_bwd_kernel<false>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, gy, g, mean,
                           stdv, gx, partial, P, ls, eps, ppb);
    }
    if (partial)
        hipLaunchKernelGGL(reduce_slices_kernel, dim3((2 * C + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, partial, (int)blocks,
                           2 * C, dgb);
    return (int)hipGetLastError();
}

int stylex_dwconv3x3_fwd(const void* x, const float* w, void* y, const int64_t* sh, int act_dtype, void* stream) {
    if (!x || !w || !y || !sh || sh[0] <= 0 || sh[1] <= 0 || sh[2] <= 0 || sh[3] <= 0 || sh[1] > 65535 || sh[2] > 65535)
        return STYLEX_EINVAL;
    if (sh[3] & 3) return STYLEX_NOT_APPLICABLE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & (act_dtype ? 7 : 15)) return STYLEX_EINVAL;
    const long total = sh[0] * sh[1] * sh[2] * (sh[3] >> 2), blocks = (total + NT - 1) / NT;
    if (blocks > 0x7fffffffL) return STYLEX_EINVAL;
    stylex_note_kernel("dwconv3x3_kernel<%s>", act_dtype ? "true" : "false");
    if (act_dtype) {
        hipLaunchKernelGGL(dwconv3x3_kernel<true>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, w, y, (int)sh[0],
                           (int)sh[1], (int)sh[2], (int)sh[3]);
    } else {
        hipLaunchKernelGGL(dwconv3x3_kernel<false>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, w, y, (int)sh[0],
                           (int)sh[1], (int)sh[2], (int)sh[3]);
    }
    return (int)hipGetLastError();
}

int stylex_dwconv3x3_wgrad_blocks(const int64_t* sh) {
    const int ls = lp_shift_of(sh[3]);
    if (sh[0] <= 0 || sh[1] <= 0 || sh[2] <= 0 || ls < 0) return STYLEX_EINVAL;
    return (int)stream_blocks(sh[0] * sh[1] * sh[2], NT >> ls);
}

int stylex_dwconv3x3_bwd_weight(const void* x, const void* gy, float* partial, float* dw, const int64_t* sh, int act_dtype,
                                void* stream) {
    if (!x || !gy || !partial || !dw || !sh || sh[0] <= 0 || sh[1] <= 0 || sh[2] <= 0 || sh[1] > 65535 || sh[2] > 65535)
        return STYLEX_EINVAL;
    const int ls = lp_shift_of(sh[3]);
    if (ls < 0) return STYLEX_NOT_APPLICABLE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gy)) & (act_dtype ? 7 : 15)) return STYLEX_EINVAL;
    const long P = sh[0] * sh[1] * sh[2], blocks = stream_blocks(P, NT >> ls), ppb = (P + blocks - 1) / blocks;
    const int n = (int)sh[3] * 9;
    stylex_note_kernel("dwconv3x3_wgrad_kernel<%s>", act_dtype ? "true" : "false");
    if (act_dtype) {
        hipLaunchKernelGGL(dwconv3x3_wgrad_kernel<true>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, gy, partial,
                           (int)sh[0], (int)sh[1], (int)sh[2], ls, ppb);
    } else {
        hipLaunchKernelGGL(dwconv3x3_wgrad_kernel<false>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, gy, partial,
                           (int)sh[0], (int)sh[1], (int)sh[2], ls, ppb);
    }
    hipLaunchKernelGGL(reduce_slices_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, partial, (int)blocks, n, dw);
    return (int)hipGetLastError();
}

}  // extern "C"
