// GroupNorm (+ activation, + a per-batch column vector) over channel-last activations, and the batched column concat of the U-Net's skip connections: shared by the
// operator-level entry points of csrc/cv1_ops.hip and the CosyVoice-300M estimator inside the flow handle (csrc/flow.hip, cfg.estimator == 2).
#pragma once
#include "common.h"

namespace cv {

// ---- GroupNorm (torch.nn.GroupNorm(G, C) on [B, C, T]; here channel-last x [B][T][C]) ----------------------------------------------------
// Every kernel below comes in two instantiations.  LEN = false: all B batch rows are T frames long, S time slices (a kernel argument), `part` pitch S.
// LEN = true, the rows of a PADDED pass: batch row b holds len[b] <= T valid frames (device int32 [B]) and is normalised over those alone; its slice count S and its
// slice bounds come from len[b] through the expressions the launcher applies to T, so the double-precision partial sums and the order they are added in are those of
// the row alone at its own length and its valid frames carry the same bits.  Frames t >= len[b] come out as exact zeros (after col_add): the next convolution must
// see what it sees behind the end of the row alone.  The launches are sized for T; a slice beyond a row's own S does nothing and pass 2 never reads it; the `part`
// pitch is kGroupSlices, the largest S.  With LEN = false none of this is compiled in.
constexpr int kGroupSlices = 32;
__host__ __device__ inline int group_slices_rows(int T, int R) { const int S = (T + 8 * R - 1) / (8 * R); return S < 1 ? 1 : (S > kGroupSlices ? kGroupSlices : S); }               // ~8 rows per lane
__host__ __device__ inline int group_slices_generic(int T, int cg) { const int S = (int)(((long long)T * cg + 8191) / 8192); return S < 1 ? 1 : (S > kGroupSlices ? kGroupSlices : S); }   // ~8 K elements per workgroup of pass 1

// Pass 1: partial sums per (batch, group, time slice) in double (a group of the regulator is the whole [80 x T] utterance: fp32 running sums would
// lose the digits torch's two-level Welford keeps).  part[((b * G + g) * pitch + s) * 2 + {0, 1}] = {sum, sum of squares}.
template <bool LEN>
static __global__ __launch_bounds__(256) void group_stats_kernel(const float* x, double* part, int T, int C, int G, int S, const int* len) {
    __shared__ double red[2][4];
    const int s = blockIdx.x, g = blockIdx.y, b = blockIdx.z, cg = C / G;
    int L = T, pitch = S;
    if constexpr (LEN) {
        L = len[b]; S = group_slices_generic(L, cg); pitch = kGroupSlices;
        if (s >= S) return;                               // (the whole workgroup: L and S are uniform)
    }
    const int t0 = (int)((long long)L * s / S), t1 = (int)((long long)L * (s + 1) / S);
    const float* xb = x + ((long long)b * T) * C + (long long)g * cg;
    const long long n = (long long)(t1 - t0) * cg;
    double a = 0.0, q = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const int t = t0 + (int)(i / cg), c = (int)(i % cg);
        const double v = (double)xb[(long long)t * C + c];
        a += v; q += v * v;
    }
    // fixed-order reduction: lanes of a wave through shuffles, then the four waves through LDS
    for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off); q += __shfl_xor(q, off); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[0][w] = a; red[1][w] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = part + (((long long)b * G + g) * pitch + s) * 2;
        o[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        o[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// Pass 2: y = act((x - mean_g) * rstd_g * gamma[c] + beta[c]) + col_add[b][c]
//   (Block1D: Conv1d -> GroupNorm -> Mish, matcha decoder.py; the ResnetBlock1D's time projection `h += mlp(t_emb)[:, :, None]` rides along as col_add)
template <bool LEN>
static __global__ __launch_bounds__(256) void group_apply_kernel(const float* x, float* y, const double* part, int T, int C, int G, int S,
                                                                  const float* gamma, const float* beta, float eps, int act,
                                                                  const float* col_add, long long col_add_batch, long long total, const int* len) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), cg = C / G, g = c / cg;
    const int b = (int)(i / ((long long)T * C));
    int L = T, pitch = S;
    if constexpr (LEN) {
        L = len[b];
        if ((int)((i / C) % T) >= L) { y[i] = 0.f; return; }
        S = group_slices_generic(L, cg); pitch = kGroupSlices;
    }
    const double* p = part + ((long long)b * G + g) * pitch * 2;
    double a = 0.0, q = 0.0;
    for (int s = 0; s < S; ++s) { a += p[2 * s]; q += p[2 * s + 1]; }
    const double n = (double)L * cg, mean = a / n;
    double var = q / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    float v = (x[i] - (float)mean) * rstd;
    if (gamma) v *= gamma[c];
    if (beta) v += beta[c];
    v = apply_act(act, v, 0.f);
    if (col_add) v += col_add[(long long)b * col_add_batch + c];
    y[i] = v;
}

// Pass 1 for the shapes of the U-Net estimator (C % 4 == 0, 256 % (C / 4) == 0, a group = a multiple of 4 channels): one workgroup per (time slice, batch) reads whole
// rows as float4 (a row of 256 channels = 1 KB, fully coalesced; the kernel above walks a 128-byte group column and measured 13.8 us per launch at [2][1000][256])
// and reduces ALL groups of its slice: lane (row r, float4 j) sums its four channels over rows r, r + R, ..., the lanes of a group are then added in a fixed order
// through LDS.  Same `part` layout as group_stats_kernel.
template <bool LEN>
static __global__ __launch_bounds__(256) void group_stats_rows_kernel(const float* x, double* part, int T, int C, int G, int S, const int* len) {
    __shared__ double red[2][256];
    const int s = blockIdx.x, b = blockIdx.y, q = C >> 2, R = 256 / q, cg4 = (C / G) >> 2;
    int L = T, pitch = S;
    if constexpr (LEN) {
        L = len[b]; S = group_slices_rows(L, R); pitch = kGroupSlices;
        if (s >= S) return;                               // (the whole workgroup)
    }
    const int j = threadIdx.x % q, r = threadIdx.x / q;
    const int t0 = (int)((long long)L * s / S), t1 = (int)((long long)L * (s + 1) / S);
    const float4* xb = reinterpret_cast<const float4*>(x + (long long)b * T * C);
    double a = 0.0, sq = 0.0;
    for (int t = t0 + r; t < t1; t += R) {
        const float4 v = xb[(long long)t * q + j];
        const double v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
        a += (v0 + v1) + (v2 + v3); sq += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
    }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = sq;
    __syncthreads();
    if ((int)threadIdx.x < G) {
        const int g = threadIdx.x;
        double sa = 0.0, ss = 0.0;
        for (int rr = 0; rr < R; ++rr)
            for (int jj = 0; jj < cg4; ++jj) { sa += red[0][rr * q + g * cg4 + jj]; ss += red[1][rr * q + g * cg4 + jj]; }
        double* o = part + (((long long)b * G + g) * pitch + s) * 2;
        o[0] = sa; o[1] = ss;
    }
}

// Pass 2 for the same shapes: lane (row r, float4 j) owns four channels of ONE group - it reduces the group's partial sums once and then walks its rows with float4
// loads / stores (the kernel above redoes the double-precision reduction per element: 7.3 us per launch at [2][1011][256] against 2 MB in + 2 MB out).  Same expressions
// per element as group_apply_kernel: the same bits.
template <bool LEN>
static __global__ __launch_bounds__(256) void group_apply_rows_kernel(const float* x, float* y, const double* part, int T, int C, int G, int S, int rows_per_wg,
                                                                       const float* gamma, const float* beta, float eps, int act,
                                                                       const float* col_add, long long col_add_batch, const int* len) {
    __shared__ double ps[2 * 8 * kGroupSlices];              // the batch row's partial sums [G][S][2] (G <= 8: see group_norm()), then the totals behind them
    __shared__ double tot[2 * 8];
    const int b = blockIdx.y, q = C >> 2, R = 256 / q, cg = C / G;
    const int j = threadIdx.x % q, r = threadIdx.x / q, c = 4 * j, g = c / cg;
    const int t0 = blockIdx.x * rows_per_wg, t1 = min(T, t0 + rows_per_wg);
    const float4* xb = reinterpret_cast<const float4*>(x + (long long)b * T * C);
    float4* yb = reinterpret_cast<float4*>(y + (long long)b * T * C);
    int L = T;
    if constexpr (LEN) {
        L = len[b]; S = group_slices_rows(L, R);
        if (t0 >= L) {                                    // a workgroup behind the row's end (uniform): zeros, no statistics
            for (int t = t0 + r; t < t1; t += R) yb[(long long)t * q + j] = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    // every lane needs ITS group's totals: S dependent loads per lane were what this launch took (11.5 us at S = 32).  The workgroup fetches the G * S pairs once, 2 G lanes
    // add them in slice order (the order of group_apply_kernel: the same bits), everybody reads the result.
    if constexpr (LEN) {
        const double* p = part + (long long)b * G * kGroupSlices * 2;
        for (int i = threadIdx.x; i < G * S * 2; i += 256) { const int gg = i / (2 * S), k = i % (2 * S); ps[i] = p[gg * kGroupSlices * 2 + k]; }
    } else {
        const double* p = part + (long long)b * G * S * 2;
        for (int i = threadIdx.x; i < G * S * 2; i += 256) ps[i] = p[i];
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * G) {
        const int gg = threadIdx.x >> 1, which = threadIdx.x & 1;
        double acc = 0.0;
        for (int s = 0; s < S; ++s) acc += ps[(gg * S + s) * 2 + which];
        tot[threadIdx.x] = acc;
    }
    __syncthreads();
    const double a = tot[2 * g], sq = tot[2 * g + 1];
    const double n = (double)L * cg, mean = a / n;
    double var = sq / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps)), fm = (float)mean;
    const float4 gm = gamma ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 bt = beta ? *reinterpret_cast<const float4*>(beta + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 ca = col_add ? *reinterpret_cast<const float4*>(col_add + (long long)b * col_add_batch + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = t0 + r; t < t1; t += R) {
        if constexpr (LEN) {
            if (t >= L) { yb[(long long)t * q + j] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
        }
        const float4 v = xb[(long long)t * q + j];
        float o[4] = {(v.x - fm) * rstd, (v.y - fm) * rstd, (v.z - fm) * rstd, (v.w - fm) * rstd};
        if (gamma) { o[0] *= gm.x; o[1] *= gm.y; o[2] *= gm.z; o[3] *= gm.w; }
        if (beta) { o[0] += bt.x; o[1] += bt.y; o[2] += bt.z; o[3] += bt.w; }
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = apply_act(act, o[k], 0.f);
        if (col_add) { o[0] += ca.x; o[1] += ca.y; o[2] += ca.z; o[3] += ca.w; }
        yb[(long long)t * q + j] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

template <bool LEN>
static inline void group_norm_launch(const float* x, float* y, int B, int T, int C, int G, const float* gamma, const float* beta, float eps, int act,
                                     const float* col_add, long long col_add_batch, double* workspace, hipStream_t s, const int* len) {
    const int q = C / 4;
    const bool al16 = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)col_add) & 15) == 0 && col_add_batch % 4 == 0;
    if (C % 4 == 0 && q <= 256 && 256 % q == 0 && (C / G) % 4 == 0 && G <= 8 && al16) {      // (nothing here depends on a length: a row alone takes the same form)
        const int R = 256 / q, S = group_slices_rows(T, R), rows = 4 * R;                     // pass 2: 4 rows per lane
        hipLaunchKernelGGL(group_stats_rows_kernel<LEN>, dim3(S, B), dim3(256), 0, s, x, workspace, T, C, G, S, len);
        hipLaunchKernelGGL(group_apply_rows_kernel<LEN>, dim3((unsigned)((T + rows - 1) / rows), B), dim3(256), 0, s, x, y, workspace, T, C, G, S, rows, gamma, beta, eps, act,
                           col_add, col_add_batch, len);
        return;
    }
    const int S = group_slices_generic(T, C / G);
    hipLaunchKernelGGL(group_stats_kernel<LEN>, dim3(S, G, B), dim3(256), 0, s, x, workspace, T, C, G, S, len);
    const long long total = (long long)B * T * C;
    hipLaunchKernelGGL(group_apply_kernel<LEN>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, y, workspace, T, C, G, S, gamma, beta, eps, act, col_add, col_add_batch, total, len);
}

// y = act(GroupNorm(x)) + col_add[b]; len: null, or the rows' lengths of a padded pass (device int32 [B], every entry 1..T).  workspace: B * G * 64 doubles
// (B * G * kGroupSlices pairs)
static inline void group_norm(const float* x, float* y, int B, int T, int C, int G, const float* gamma, const float* beta, float eps, int act,
                              const float* col_add, long long col_add_batch, double* workspace, hipStream_t s, const int* len = nullptr) {
    if (len) group_norm_launch<true>(x, y, B, T, C, G, gamma, beta, eps, act, col_add, col_add_batch, workspace, s, len);
    else group_norm_launch<false>(x, y, B, T, C, G, gamma, beta, eps, act, col_add, col_add_batch, workspace, s, len);
}

// x [B][T][C] (C % 4 == 0, 16-byte aligned): rows t >= len[b] <- 0.  The reference's `x * mask` wherever no GroupNorm follows (flow/decoder.py:210-291); the valid rows
// are not touched, so their bits are those of the row alone.
static __global__ __launch_bounds__(256) void zero_tail_rows_kernel(float* x, int B, int T, int C4, const int* len) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * T * C4) return;
    const int t = (int)((i / C4) % T), b = (int)(i / ((long long)C4 * T));
    if (t >= len[b]) reinterpret_cast<float4*>(x)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
static inline void zero_tail_rows(float* x, int B, int T, int C, const int* len, hipStream_t s) {
    hipLaunchKernelGGL(zero_tail_rows_kernel, dim3((unsigned)(((long long)B * T * (C / 4) + 255) / 256)), dim3(256), 0, s, x, B, T, C / 4, len);
}

// out[b][t][0:ca] = a[b][t], out[b][t][ca:ca+cb] = bb[b][t] for t < T; a / bb have their own per-batch pitches (rows per batch may exceed T:
// the up-sampled stream of the U-Net is cut to the skip connection's length, flow/decoder.py:275)
static __global__ __launch_bounds__(256) void concat_cols_batched_kernel(const float* a, int ca, long long a_batch, const float* bb, int cb, long long b_batch,
                                                                          float* out, int T, int B) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int w = ca + cb;
    if (i >= (long long)B * T * w) return;
    const int c = (int)(i % w), t = (int)((i / w) % T), b = (int)(i / ((long long)w * T));
    out[i] = c < ca ? a[(long long)b * a_batch + (long long)t * ca + c] : bb[(long long)b * b_batch + (long long)t * cb + (c - ca)];
}

}  // namespace cv
