// bn_train.hip — training-mode BatchNorm2d with its activation / residual tail, and the softmax cross-entropy, for the
// classifier StylEx explains (reference stylex/train_mobilenet_classifier.py: MobileNetV2, 52 normalisations;
// classifier_training_celeba.ipynb: ResNet-18, 20).  The convolutions stay on the stock library (as in the frozen forward,
// frozen_ew.hip); what sits between them is HBM streams and per-channel reductions:
//
//   stats        x [B][C][HW] -> mean[c], biased var[c] over the n = B * HW elements of a channel, and the running-statistics
//                update of nn.BatchNorm2d.  Three launches: (1) per-block sums, (2) per-block sums of (x - mean)^2 — the
//                CENTRED second pass, never E[x^2] - mean^2 — (3) the combine.
//   fwd          y = act((x - mean) * rsqrt(var + eps) * gamma + beta (+ residual)), act in {none, ReLU, ReLU6}: one pass.
//   bwd_reduce   g = gy * gate(y);  dbeta[c] = sum g,  dgamma[c] = sum g * xhat: per-block sums + combine.
//   bwd_apply    gx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n),  gres = g: one pass.
//   softmax_ce   mean over rows of logsumexp - logit[target], the count of rows whose argmax is the target, and the gradient.
//
// Reductions: a channel's n elements are cut into S = ceil(n / BN_CHUNK) consecutive chunks (S <= BN_MAX_SPLIT, the chunk
// grows beyond that), one block per (chunk, channel).  Every sum is ACCUMULATED IN FP64: a lane adds its elements in index
// order, the 64 lanes of a wave are combined by xor shuffles (commutative: every lane holds the same bits), the 4 waves and
// then the S chunk partials in fixed order.  The fp64 sum of n fp32 values or products carries a relative error below
// n * 2^-53 of the sum of the absolute terms; the one rounding that matters is the final fp64 -> fp32 store.  No atomics:
// the same inputs give the same bits.  (fp64 adds run at a rate that leaves these kernels on the HBM roof: two converts and
// two to five fp64 operations per 4 to 12 bytes read.)
//
// invstd = 1 / sqrt(var + eps) everywhere: the sum var + eps in fp32 (ATen's arithmetic: var = 1 - eps gives exactly 1), the
// square root and the division in fp64.
//
// Access width: 16-byte lanes when HW % 4 == 0 and every tensor pointer is 16-byte aligned — a lane's four elements then lie
// in one (b, c) row; single elements otherwise (HW = 49 in MobileNetV2's last blocks).  No access can pass a row's end.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

constexpr unsigned BN_CHUNK = 8192;      // elements of one channel per first-stage block (a multiple of 4)
constexpr unsigned BN_MAX_SPLIT = 256;   // chunks per channel at most: the combine reads one partial per thread
constexpr unsigned EW_SPAN = 4096;       // elements per block of the streaming kernels
constexpr unsigned EW_ROWS = 256;        // (b, c) rows a streaming block may touch (its per-row constants live in LDS)
constexpr int CE_MAX_K = 1024;
constexpr int CE_PER_LANE = CE_MAX_K / 64;

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_RELU6 = 2 };

struct Split { unsigned n, S, chunk; };

inline Split bn_split(int64_t B, int64_t HW) {
    Split s;
    s.n = (unsigned)(B * HW);
    s.S = (s.n + BN_CHUNK - 1) / BN_CHUNK;
    s.chunk = BN_CHUNK;
    if (s.S > BN_MAX_SPLIT) {
        s.S = BN_MAX_SPLIT;
        s.chunk = (((s.n + s.S - 1) / s.S) + 3u) & ~3u;
        s.S = (s.n + s.chunk - 1) / s.chunk;
    }
    return s;
}

inline bool bn_shape_ok(int64_t B, int64_t C, int64_t HW) {
    return B >= 1 && C >= 1 && HW >= 1 && C <= 65535 && B * C * HW <= 0x7fffffffLL;
}

// Sum of v over the block's 256 threads in fixed order; every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double* buf) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // buf may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    return (buf[0] + buf[1]) + (buf[2] + buf[3]);
}

// Sum of the S chunk partials of channel c (S <= 256: one per thread), every thread of every block in the same order.
__device__ __forceinline__ double combine_partials(const double* __restrict__ part, unsigned c, unsigned S, double* buf) {
    return block_sum(threadIdx.x < S ? part[(size_t)c * S + threadIdx.x] : 0.0, buf);
}

__device__ __forceinline__ bool gate_open(float y, int act) {
    return act == ACT_NONE || (y > 0.f && (act == ACT_RELU || y < 6.f));
}

// Walks the elements j0 <= j < j1 of channel c (j = b * HW + p) V at a time and hands each to f(offset into the tensor).
template <int V, typename F>
__device__ __forceinline__ void for_channel_chunk(unsigned c, unsigned C, unsigned HW, unsigned j0, unsigned j1, F f) {
#pragma unroll 4
    for (unsigned j = j0 + threadIdx.x * V; j < j1; j += 256u * V) {
        const unsigned b = j / HW, p = j - b * HW;
        f((b * C + c) * HW + p);
    }
}

template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float* v) {
    if (V == 4) *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(p);
    else v[0] = p[0];
}
template <int V>
__device__ __forceinline__ void store_v(float* __restrict__ p, const float* v) {
    if (V == 4) *reinterpret_cast<float4*>(p) = *reinterpret_cast<const float4*>(v);
    else p[0] = v[0];
}

// (1) psum[c][s] = sum of x over chunk s of channel c
template <int V>
__global__ __launch_bounds__(256) void bn_sum_kernel(const float* __restrict__ x, double* __restrict__ psum, unsigned C, unsigned HW,
                                                     unsigned n, unsigned chunk) {
    __shared__ double buf[4];
    const unsigned c = blockIdx.y, S = gridDim.x, j0 = blockIdx.x * chunk, j1 = min(n, j0 + chunk);
    double acc = 0.0;
    for_channel_chunk<V>(c, C, HW, j0, j1, [&](unsigned e) {
        float v[V];
        load_v<V>(x + e, v);
#pragma unroll
        for (int k = 0; k < V; ++k) acc += (double)v[k];
    });
    acc = block_sum(acc, buf);
    if (threadIdx.x == 0) psum[(size_t)c * S + blockIdx.x] = acc;
}

// (2) pvar[c][s] = sum of (x - mean)^2 over chunk s, mean = (sum of psum[c][.]) / n in fp64
template <int V>
__global__ __launch_bounds__(256) void bn_centred_kernel(const float* __restrict__ x, const double* __restrict__ psum,
                                                         double* __restrict__ pvar, unsigned C, unsigned HW, unsigned n,
                                                         unsigned chunk) {
    __shared__ double buf[4];
    const unsigned c = blockIdx.y, S = gridDim.x, j0 = blockIdx.x * chunk, j1 = min(n, j0 + chunk);
    const double mean = combine_partials(psum, c, S, buf) / (double)n;
    double acc = 0.0;
    for_channel_chunk<V>(c, C, HW, j0, j1, [&](unsigned e) {
        float v[V];
        load_v<V>(x + e, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double d = (double)v[k] - mean;
            acc = fma(d, d, acc);
        }
    });
    acc = block_sum(acc, buf);
    if (threadIdx.x == 0) pvar[(size_t)c * S + blockIdx.x] = acc;
}

// (3) mean[c], var[c] (biased) and, when rm / rv are given, rm = (1 - m) rm + m mean, rv = (1 - m) rv + m var n / (n - 1)
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const double* __restrict__ psum, const double* __restrict__ pvar,
                                                             float* __restrict__ mean, float* __restrict__ var,
                                                             float* __restrict__ rm, float* __restrict__ rv, double momentum,
                                                             unsigned S, unsigned n) {
    __shared__ double buf[4];
    const unsigned c = blockIdx.x;
    const double m = combine_partials(psum, c, S, buf) / (double)n;
    const double v = combine_partials(pvar, c, S, buf) / (double)n;
    if (threadIdx.x == 0) {
        mean[c] = (float)m;
        var[c] = (float)v;
        if (rm) rm[c] = (float)((1.0 - momentum) * (double)rm[c] + momentum * m);
        if (rv) rv[c] = (float)((1.0 - momentum) * (double)rv[c] + momentum * (v * (double)n / (double)(n - 1)));
    }
}

// Per-row constants of a streaming block: the block covers the elements [i0, i1) of the flat tensor, i.e. the rows
// r0 = i0 / HW .. (i1 - 1) / HW (at most EW_ROWS of them); thread t prepares row r0 + t.
struct RowSpan { unsigned i0, i1, r0, rows; };
__device__ __forceinline__ RowSpan row_span(unsigned total, unsigned span, unsigned HW) {
    RowSpan r;
    r.i0 = blockIdx.x * span;
    r.i1 = min(total, r.i0 + span);
    r.r0 = r.i0 / HW;
    r.rows = (r.i1 - 1) / HW - r.r0 + 1;
    return r;
}

// y = act((x - mean[c]) * s[c] + beta[c] (+ r)),  s = gamma * rsqrt(var + eps) formed in fp64 and rounded once
template <int V>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ var, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ res,
                                                         float* __restrict__ y, double eps, unsigned total, unsigned span,
                                                         unsigned HW, unsigned C, int act) {
    __shared__ float k_mean[EW_ROWS], k_s[EW_ROWS], k_b[EW_ROWS];
    const RowSpan rs = row_span(total, span, HW);
    if (threadIdx.x < rs.rows) {
        const unsigned c = (rs.r0 + threadIdx.x) % C;
        k_mean[threadIdx.x] = mean[c];
        k_s[threadIdx.x] = (float)((double)gamma[c] / sqrt((double)(var[c] + (float)eps)));
        k_b[threadIdx.x] = beta[c];
    }
    __syncthreads();
    for (unsigned e = rs.i0 + threadIdx.x * V; e < rs.i1; e += 256u * V) {
        const unsigned r = e / HW - rs.r0;
        const float mu = k_mean[r], sc = k_s[r], sh = k_b[r];
        float v[V], rr[V];
        load_v<V>(x + e, v);
        if (res) load_v<V>(res + e, rr);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float o = fmaf(v[k] - mu, sc, sh);
            if (res) o += rr[k];
            if (act != ACT_NONE) o = fmaxf(o, 0.f);
            if (act == ACT_RELU6) o = fminf(o, 6.f);
            v[k] = o;
        }
        store_v<V>(y + e, v);
    }
}

// pdb[c][s] = sum g, pdg[c][s] = sum g * xhat over chunk s;  g = gy * gate(y),  xhat = (x - mean) * rsqrt(var + eps) in fp64
template <int V>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                            const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ var, double* __restrict__ pdb,
                                                            double* __restrict__ pdg, double eps, unsigned C, unsigned HW,
                                                            unsigned n, unsigned chunk, int act) {
    __shared__ double buf[4];
    const unsigned c = blockIdx.y, S = gridDim.x, j0 = blockIdx.x * chunk, j1 = min(n, j0 + chunk);
    const double mu = (double)mean[c], invstd = 1.0 / sqrt((double)(var[c] + (float)eps));
    double sg = 0.0, sgx = 0.0;
    for_channel_chunk<V>(c, C, HW, j0, j1, [&](unsigned e) {
        float g[V], xx[V], yy[V];
        load_v<V>(gy + e, g);
        load_v<V>(x + e, xx);
        if (act != ACT_NONE) load_v<V>(y + e, yy);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double gg = (act == ACT_NONE || gate_open(yy[k], act)) ? (double)g[k] : 0.0;
            sg += gg;
            sgx = fma(gg, ((double)xx[k] - mu) * invstd, sgx);
        }
    });
    sg = block_sum(sg, buf);
    sgx = block_sum(sgx, buf);
    if (threadIdx.x == 0) {
        pdb[(size_t)c * S + blockIdx.x] = sg;
        pdg[(size_t)c * S + blockIdx.x] = sgx;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const double* __restrict__ pdb, const double* __restrict__ pdg,
                                                           float* __restrict__ dbeta, float* __restrict__ dgamma, unsigned S) {
    __shared__ double buf[4];
    const unsigned c = blockIdx.x;
    const double b = combine_partials(pdb, c, S, buf);
    const double g = combine_partials(pdg, c, S, buf);
    if (threadIdx.x == 0) {
        dbeta[c] = (float)b;
        dgamma[c] = (float)g;
    }
}

// gx = s * (g - k1 - xhat * k2),  xhat = (x - mean) * invstd,  s = gamma * invstd,  k1 = dbeta / n,  k2 = dgamma / n;
// gres = g.  The per-row constants are formed in fp64 and rounded once.
template <int V>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                           const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ var, const float* __restrict__ gamma,
                                                           const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                           float* __restrict__ gx, float* __restrict__ gres, double eps,
                                                           unsigned total, unsigned span, unsigned HW, unsigned C, unsigned n,
                                                           int act) {
    __shared__ float k_mean[EW_ROWS], k_inv[EW_ROWS], k_s[EW_ROWS], k_1[EW_ROWS], k_2[EW_ROWS];
    const RowSpan rs = row_span(total, span, HW);
    if (threadIdx.x < rs.rows) {
        const unsigned c = (rs.r0 + threadIdx.x) % C;
        const double invstd = 1.0 / sqrt((double)(var[c] + (float)eps));
        k_mean[threadIdx.x] = mean[c];
        k_inv[threadIdx.x] = (float)invstd;
        k_s[threadIdx.x] = (float)((double)gamma[c] * invstd);
        k_1[threadIdx.x] = (float)((double)dbeta[c] / (double)n);
        k_2[threadIdx.x] = (float)((double)dgamma[c] / (double)n);
    }
    __syncthreads();
    for (unsigned e = rs.i0 + threadIdx.x * V; e < rs.i1; e += 256u * V) {
        const unsigned r = e / HW - rs.r0;
        const float mu = k_mean[r], inv = k_inv[r], sc = k_s[r], k1 = k_1[r], k2 = k_2[r];
        float g[V], xx[V], yy[V], o[V];
        load_v<V>(gy + e, g);
        if (gx) load_v<V>(x + e, xx);
        if (act != ACT_NONE) load_v<V>(y + e, yy);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (act != ACT_NONE && !gate_open(yy[k], act)) g[k] = 0.f;
            if (gx) o[k] = fmaf(-((xx[k] - mu) * inv), k2, g[k] - k1) * sc;
        }
        if (gx) store_v<V>(gx + e, o);
        if (gres) store_v<V>(gres + e, g);
    }
}

// ---- softmax cross-entropy: one wave per row, K <= 1024 (16 logits per lane in registers) ----------------------------------
struct CeRow { float mx, sum, xt; int arg; };

// max (first index on ties), sum of exp(x - max) and the target's logit of row `row`; the target is matched by comparing
// indices, never used as one.  Every lane returns the same values.
__device__ __forceinline__ CeRow ce_row(const float* __restrict__ row, int K, long long target, float* v) {
    const int lane = threadIdx.x & 63;
    float mx = -INFINITY, xt = 0.f;
    int arg = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < CE_PER_LANE; ++i) {
        const int k = lane + 64 * i;
        v[i] = k < K ? row[k] : -INFINITY;
        if (k < K && (v[i] > mx || arg == 0x7fffffff)) mx = v[i], arg = k;
        if (k < K && (long long)k == target) xt = v[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (om > mx || (om == mx && oa < arg)) mx = om, arg = oa;
        xt += __shfl_xor(xt, o, 64);  // one lane holds the target's logit, the others 0
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CE_PER_LANE; ++i) {
        v[i] = lane + 64 * i < K ? expf(v[i] - mx) : 0.f;
        sum += v[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    CeRow r;
    r.mx = mx, r.sum = sum, r.xt = xt, r.arg = arg;
    return r;
}

// row_loss[b] = log(sum exp(x - max)) + (max - x[target]) (NaN for a target outside [0, K)), row_ok[b] = argmax == target
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ targets,
                                                      float* __restrict__ row_loss, int* __restrict__ row_ok, int B, int K) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const long long t = targets[b];
    float v[CE_PER_LANE];
    const CeRow r = ce_row(logits + (size_t)b * K, K, t, v);
    if ((threadIdx.x & 63) == 0) {
        const bool valid = t >= 0 && t < (long long)K;
        row_loss[b] = valid ? logf(r.sum) + (r.mx - r.xt) : NAN;
        row_ok[b] = valid && (long long)r.arg == t ? 1 : 0;
    }
}

// loss = (sum_b row_loss[b]) / B in fp64, fixed order; n_correct = sum_b row_ok[b]
__global__ __launch_bounds__(256) void ce_final_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_ok,
                                                       float* __restrict__ loss, long long* __restrict__ n_correct, int B) {
    __shared__ double buf[4];
    double acc = 0.0, cnt = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        acc += (double)row_loss[b];
        cnt += (double)row_ok[b];
    }
    acc = block_sum(acc, buf);
    cnt = block_sum(cnt, buf);  // integers below 2^31: exact in fp64
    if (threadIdx.x == 0) {
        loss[0] = (float)(acc / (double)B);
        n_correct[0] = (long long)cnt;
    }
}

// glogits[b][k] = (softmax[b][k] - [k == target]) * gloss / B; a row whose target is outside [0, K) gets zeros
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ targets,
                                                     const float* __restrict__ gloss, float* __restrict__ glogits, int B, int K) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const long long t = targets[b];
    float v[CE_PER_LANE];
    const CeRow r = ce_row(logits + (size_t)b * K, K, t, v);
    const bool valid = t >= 0 && t < (long long)K;
    const float gs = gloss[0] / (float)B, inv = 1.f / r.sum;
    float* out = glogits + (size_t)b * K;
#pragma unroll
    for (int i = 0; i < CE_PER_LANE; ++i) {
        const int k = lane + 64 * i;
        if (k < K) out[k] = valid ? (v[i] * inv - ((long long)k == t ? 1.f : 0.f)) * gs : 0.f;
    }
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                      const void* e = nullptr) {
    return !((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
              reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(e)) & 15);
}

// elements per block of a streaming kernel: at most EW_SPAN, and few enough that the block touches <= EW_ROWS rows
inline unsigned ew_span(int64_t HW) {
    const int64_t by_rows = (int64_t)(EW_ROWS - 2) * HW;  // a multiple of 4 whenever HW is
    return (unsigned)(by_rows < (int64_t)EW_SPAN ? by_rows : (int64_t)EW_SPAN);
}

inline bool act_ok(int act) { return act == ACT_NONE || act == ACT_RELU || act == ACT_RELU6; }

}  // namespace

extern "C" {

int64_t stylex_bn_train_workspace_bytes(int64_t B, int64_t C, int64_t HW) {
    if (!bn_shape_ok(B, C, HW)) return -1;
    return (int64_t)2 * C * bn_split(B, HW).S * (int64_t)sizeof(double);
}

int stylex_bn_stats_nchw(const float* x, float* mean, float* var, float* running_mean, float* running_var, double momentum,
                         int64_t B, int64_t C, int64_t HW, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !mean || !var || !workspace || !bn_shape_ok(B, C, HW) || B * HW < 2 || (!running_mean) != (!running_var))
        return STYLEX_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return STYLEX_EINVAL;
    const Split sp = bn_split(B, HW);
    if (workspace_bytes < stylex_bn_train_workspace_bytes(B, C, HW)) return STYLEX_EWORKSPACE;
    double* psum = static_cast<double*>(workspace);
    double* pvar = psum + (size_t)C * sp.S;
    const dim3 grid(sp.S, (unsigned)C);
    hipStream_t s = (hipStream_t)stream;
    if (HW % 4 == 0 && aligned16(x)) {
        hipLaunchKernelGGL(bn_sum_kernel<4>, grid, dim3(256), 0, s, x, psum, (unsigned)C, (unsigned)HW, sp.n, sp.chunk);
        hipLaunchKernelGGL(bn_centred_kernel<4>, grid, dim3(256), 0, s, x, psum, pvar, (unsigned)C, (unsigned)HW, sp.n, sp.chunk);
    } else {
        hipLaunchKernelGGL(bn_sum_kernel<1>, grid, dim3(256), 0, s, x, psum, (unsigned)C, (unsigned)HW, sp.n, sp.chunk);
        hipLaunchKernelGGL(bn_centred_kernel<1>, grid, dim3(256), 0, s, x, psum, pvar, (unsigned)C, (unsigned)HW, sp.n, sp.chunk);
    }
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)C), dim3(256), 0, s, psum, pvar, mean, var, running_mean,
                       running_var, momentum, sp.S, sp.n);
    return (int)hipGetLastError();
}

int stylex_bn_act_nchw_fwd(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                           const float* residual, float* y, double eps, int64_t B, int64_t C, int64_t HW, int act, void* stream) {
    if (!x || !mean || !var || !gamma || !beta || !y || !bn_shape_ok(B, C, HW) || !act_ok(act)) return STYLEX_EINVAL;
    const unsigned total = (unsigned)(B * C * HW), span = ew_span(HW);
    const unsigned blocks = (total + span - 1) / span;
    hipStream_t s = (hipStream_t)stream;
    if (HW % 4 == 0 && aligned16(x, y, residual))
        hipLaunchKernelGGL(bn_act_fwd_kernel<4>, dim3(blocks), dim3(256), 0, s, x, mean, var, gamma, beta, residual, y, eps, total,
                           span, (unsigned)HW, (unsigned)C, act);
    else
        hipLaunchKernelGGL(bn_act_fwd_kernel<1>, dim3(blocks), dim3(256), 0, s, x, mean, var, gamma, beta, residual, y, eps, total,
                           span, (unsigned)HW, (unsigned)C, act);
    return (int)hipGetLastError();
}

int stylex_bn_act_nchw_bwd_reduce(const float* gy, const float* y, const float* x, const float* mean, const float* var,
                                  float* dgamma, float* dbeta, double eps, int64_t B, int64_t C, int64_t HW, int act,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (!gy || !x || !mean || !var || !dgamma || !dbeta || !workspace || !bn_shape_ok(B, C, HW) || B * HW < 2 || !act_ok(act) ||
        (act != ACT_NONE && !y))
        return STYLEX_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return STYLEX_EINVAL;
    const Split sp = bn_split(B, HW);
    if (workspace_bytes < stylex_bn_train_workspace_bytes(B, C, HW)) return STYLEX_EWORKSPACE;
    double* pdb = static_cast<double*>(workspace);
    double* pdg = pdb + (size_t)C * sp.S;
    const dim3 grid(sp.S, (unsigned)C);
    hipStream_t s = (hipStream_t)stream;
    if (HW % 4 == 0 && aligned16(gy, y, x))
        hipLaunchKernelGGL(bn_bwd_reduce_kernel<4>, grid, dim3(256), 0, s, gy, y, x, mean, var, pdb, pdg, eps, (unsigned)C,
                           (unsigned)HW, sp.n, sp.chunk, act);
    else
        hipLaunchKernelGGL(bn_bwd_reduce_kernel<1>, grid, dim3(256), 0, s, gy, y, x, mean, var, pdb, pdg, eps, (unsigned)C,
                           (unsigned)HW, sp.n, sp.chunk, act);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((unsigned)C), dim3(256), 0, s, pdb, pdg, dbeta, dgamma, sp.S);
    return (int)hipGetLastError();
}

int stylex_bn_act_nchw_bwd_apply(const float* gy, const float* y, const float* x, const float* mean, const float* var,
                                 const float* gamma, const float* dgamma, const float* dbeta, float* gx, float* gres, double eps,
                                 int64_t B, int64_t C, int64_t HW, int act, void* stream) {
    if (!gy || !mean || !var || !gamma || !dgamma || !dbeta || (!gx && !gres) || (gx && !x) || !bn_shape_ok(B, C, HW) ||
        B * HW < 2 || !act_ok(act) || (act != ACT_NONE && !y))
        return STYLEX_EINVAL;
    const unsigned total = (unsigned)(B * C * HW), span = ew_span(HW);
    const unsigned blocks = (total + span - 1) / span;
    hipStream_t s = (hipStream_t)stream;
    if (HW % 4 == 0 && aligned16(gy, y, x, gx, gres))
        hipLaunchKernelGGL(bn_bwd_apply_kernel<4>, dim3(blocks), dim3(256), 0, s, gy, y, x, mean, var, gamma, dgamma, dbeta, gx, gres,
                           eps, total, span, (unsigned)HW, (unsigned)C, (unsigned)(B * HW), act);
    else
        hipLaunchKernelGGL(bn_bwd_apply_kernel<1>, dim3(blocks), dim3(256), 0, s, gy, y, x, mean, var, gamma, dgamma, dbeta, gx, gres,
                           eps, total, span, (unsigned)HW, (unsigned)C, (unsigned)(B * HW), act);
    return (int)hipGetLastError();
}

int64_t stylex_softmax_ce_workspace_bytes(int64_t B, int64_t K) {
    if (B < 1 || K < 1 || K > CE_MAX_K || B * K > 0x7fffffffLL) return -1;
    return B * (int64_t)(sizeof(float) + sizeof(int));
}

int stylex_softmax_ce_fwd(const float* logits, const int64_t* targets, float* loss, int64_t* n_correct, int64_t B, int64_t K,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    if (!logits || !targets || !loss || !n_correct || !workspace || stylex_softmax_ce_workspace_bytes(B, K) < 0)
        return STYLEX_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return STYLEX_EINVAL;
    if (workspace_bytes < stylex_softmax_ce_workspace_bytes(B, K)) return STYLEX_EWORKSPACE;
    float* row_loss = static_cast<float*>(workspace);
    int* row_ok = reinterpret_cast<int*>(row_loss + B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits,
                       reinterpret_cast<const long long*>(targets), row_loss, row_ok, (int)B, (int)K);
    hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, s, row_loss, row_ok, loss, reinterpret_cast<long long*>(n_correct),
                       (int)B);
    return (int)hipGetLastError();
}

int stylex_softmax_ce_bwd(const float* logits, const int64_t* targets, const float* gloss, float* glogits, int64_t B, int64_t K,
                          void* stream) {
    if (!logits || !targets || !gloss || !glogits || stylex_softmax_ce_workspace_bytes(B, K) < 0) return STYLEX_EINVAL;
    hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits,
                       reinterpret_cast<const long long*>(targets), gloss, glogits, (int)B, (int)K);
    return (int)hipGetLastError();
}

}  // extern "C"
