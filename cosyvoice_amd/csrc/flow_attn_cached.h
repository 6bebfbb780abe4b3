// Attention of a few NEW queries against a long CACHED context: the transformer blocks of the flow estimator on the incremental streaming path (cv_flow_stream_chunk,
// flow.hip).  The chunk-causal estimator (matcha BasicTransformerBlock inside CausalConditionalDecoder, flow/decoder.py:405-494, with the chunk mask of
// add_optional_chunk_mask, utils/mask.py) lets a frame see every frame up to the end of its own chunk: the Tn frames of an arriving chunk are queries at the
// ABSOLUTE positions q0 .. q0 + Tn - 1, the keys and values are rows 0 .. q0 + Tn - 1 of a per-(Euler step, guidance row, block) cache that earlier calls filled.
//   query i sees the keys < min(klen[b], ((q0 + i) / chunk + 1) * chunk)
// cv_attention's / attn_flow32_kernel's MASK_CHUNK masks by the LOCAL query index and reads K / V of one [B][T] tensor: neither has the offset or a base per row.
//
// Shape of the work: Tn = 50 - 200 queries, 8 heads, 2 batch rows, 1000+ keys.  A query-tiled grid alone is 32 - 64 workgroups on 256 CUs, each walking the whole
// context; so the keys are PARTITIONED as well: grid = (64-query tiles x NS key slices, heads, batch rows).  Slice s of batch row b owns the 64-key tiles
// [s tps, (s + 1) tps), tps = ceil(ceil(kend_b / 64) / NS), kend_b = the key limit of the LAST query of the call - a fixed partition per (key count, NS), tiles at
// absolute multiples of 64, so a query's bits depend on (its position, klen, chunk, NS) alone: not on Tn, not on what shares the launch.  A slice leaves per query the
// flash-attention partial (running maximum m, denominator l, unnormalised accumulator o[64]); attn_cached_merge_kernel folds the NS partials in slice order.  A slice
// that holds no visible key of a query reports (m, l) = (-inf, 0) and a zero accumulator, and the merge skips it - no exp(-inf - -inf) anywhere.  NS = 1 writes the
// normalised rows itself (no second launch).
//
// Precision, template BF:
//   false  fp32 Q rows and fp32 cache rows, both products on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation in a fixed order) - attention_kernel's
//          arithmetic (attention.h);
//   true   bf16 Q rows, bf16 K and V cache rows, P rounded to bf16 for the second product, v_mfma_f32_16x16x32_bf16 with fp32 accumulation, fp32 softmax in log2
//          units, the denominator sums the UNROUNDED probabilities: the operand rounding points of attn_flow32_kernel (flow_attn32.h).
// Layout per wave (16 queries), as in attention.h: S^T = K.Q^T leaves lane (q = lane & 15, g = lane >> 4) with the keys 16 kt + 4 g + r of its query, which is the
// B-operand order of O^T += V^T.P^T; K tiles sit in LDS as [key][d] at a pitch of 8 (mod 16) dwords (conflict-free ds_read_b128 fragments), V as [key][d] (fp32) or
// transposed and key-permuted [d][key] (bf16).  Cache rows at or beyond klen[b] are never read.
#pragma once
#include "common.h"
#include "attention.h"

namespace cv {

constexpr int ATTN_CACHED_MAX_B = 8;

struct AttnCachedArgs {
    const void* q; int ldq;                          // new rows [B][Tn][ldq] (fp32 | bf16), head h at columns 64 h ..
    const void* k[ATTN_CACHED_MAX_B];                // per batch row: K cache rows [klen][ldc], head h at columns 64 h ..
    const void* v[ATTN_CACHED_MAX_B];                // ... V cache rows
    int klen[ATTN_CACHED_MAX_B];                     // ... rows the cache holds (q0 + Tn in the estimator)
    int ldc;
    void* o; int ldo;                                // result [B][Tn][ldo] (fp32 | bf16): written here when ns == 1, by the merge otherwise
    float* pm; float* pl; float* po;                 // partials [B][H][Tn][ns] (m, l) and [B][H][Tn][ns][64]
    int B, H, Tn, q0, chunk, ns;
    float scale;
};

// tiles per slice of batch row b (host and device agree through this one expression)
__host__ __device__ inline int attn_cached_kend(const AttnCachedArgs& p, int b, int q_last_abs) {
    return p.chunk > 0 ? min(p.klen[b], (q_last_abs / p.chunk + 1) * p.chunk) : p.klen[b];
}

template <bool BF>
__global__ __launch_bounds__(256) CV_WAVES_PER_EU(1, 2) void attn_cached_kernel(AttnCachedArgs p) {
    constexpr int BQ = 64, BKV = 64, LD = BF ? 36 : 68;                  // LDS row pitch in dwords
    __shared__ __attribute__((aligned(16))) float Ks[BKV * LD];
    __shared__ __attribute__((aligned(16))) float Vs[BKV * LD];
    unsigned* Ku = reinterpret_cast<unsigned*>(Ks); unsigned* Vt = reinterpret_cast<unsigned*>(Vs);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, lg = lane >> 4;
    const int sl = (int)blockIdx.x % p.ns, qb = (int)blockIdx.x / p.ns, h = blockIdx.y, b = blockIdx.z;
    const int qi = qb * BQ + wave * 16 + lq;                             // local row of this lane's query
    const bool qvalid = qi < p.Tn;
    const float NEG_INF = -__builtin_huge_valf();
    const float sc = BF ? p.scale * 1.4426950408889634f : p.scale;       // bf16 form: scores in log2 units (softmax on v_exp_f32)

    // the slice's share of the keys (fixed per key count), cut at what this workgroup's last query may see
    const int klen = p.klen[b];
    const int nt = (attn_cached_kend(p, b, p.q0 + p.Tn - 1) + BKV - 1) / BKV, tps = (nt + p.ns - 1) / p.ns;
    const int kbeg = sl * tps * BKV;
    const int kend = min((sl + 1) * tps * BKV, attn_cached_kend(p, b, p.q0 + min(p.Tn - 1, qb * BQ + BQ - 1)));
    int klim = qvalid ? attn_cached_kend(p, b, p.q0 + qi) : 0;           // per-query key limit (exclusive)

    const int esz = BF ? 2 : 4;
    const char* qp = static_cast<const char*>(p.q) + (((long long)b * p.Tn + (qvalid ? qi : 0)) * p.ldq + h * 64) * esz;
    const char* kb = static_cast<const char*>(p.k[b]) + (long long)h * 64 * esz;
    const char* vb = static_cast<const char*>(p.v[b]) + (long long)h * 64 * esz;
    const long long rowb = (long long)p.ldc * esz;

    float m_run = NEG_INF, l_run = 0.f;
    v4f acc[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[d] = (v4f){0.f, 0.f, 0.f, 0.f};

    if constexpr (!BF) {
        float4 qf[4];                                                     // qf[dg] = Q[qi][16 dg + 4 lg .. + 3]
#pragma unroll
        for (int dg = 0; dg < 4; ++dg) {
            float4 t = *reinterpret_cast<const float4*>(qp + (dg * 16 + lg * 4) * 4);
            if (!qvalid) t = make_float4(0.f, 0.f, 0.f, 0.f);
            qf[dg] = t;
        }
        float4 rk[4], rv[4];
        auto load_kv = [&](int kt0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int vv = tid + i * 256, row = vv >> 4, c4 = (vv & 15) * 4, key = kt0 + row;
                const bool ok = key < klen;                              // rows the cache does not hold are zeros (never dereferenced)
                const long long kr = ok ? key : 0;
                float4 kx = *reinterpret_cast<const float4*>(kb + kr * rowb + c4 * 4), vx = *reinterpret_cast<const float4*>(vb + kr * rowb + c4 * 4);
                if (!ok) { kx = make_float4(0.f, 0.f, 0.f, 0.f); vx = kx; }
                rk[i] = kx; rv[i] = vx;
            }
        };
        if (kbeg < kend) load_kv(kbeg);
        for (int kt0 = kbeg; kt0 < kend; kt0 += BKV) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int vv = tid + i * 256, row = vv >> 4, c4 = (vv & 15) * 4;
                *reinterpret_cast<float4*>(&Ks[row * LD + c4]) = rk[i];
                *reinterpret_cast<float4*>(&Vs[row * LD + c4]) = rv[i];
            }
            __syncthreads();
            if (kt0 + BKV < kend) load_kv(kt0 + BKV);
            v4f s[4];                                                     // s[kt][r] <-> key kt0 + 16 kt + 4 lg + r, query lq
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                v4f sa = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dg = 0; dg < 4; ++dg) {
                    const float4 kf = *reinterpret_cast<const float4*>(&Ks[(kt * 16 + lq) * LD + dg * 16 + lg * 4]);
                    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[dg].x, sa, 0, 0, 0);
                    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[dg].y, sa, 0, 0, 0);
                    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[dg].z, sa, 0, 0, 0);
                    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[dg].w, sa, 0, 0, 0);
                }
                s[kt] = sa;
            }
            float mt = NEG_INF;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt0 + kt * 16 + lg * 4 + r;
                    const float x = key < klim ? s[kt][r] * sc : NEG_INF;
                    s[kt][r] = x; mt = fmaxf(mt, x);
                }
            mt = fmaxf(mt, __shfl_xor(mt, 16)); mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);
            const float alpha = (m_run == NEG_INF) ? 0.f : expf(m_run - m_new);
            float rsum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = s[kt][r];
                    const float e = (x == NEG_INF) ? 0.f : expf(x - m_new);
                    s[kt][r] = e; rsum += e;
                }
            rsum += __shfl_xor(rsum, 16); rsum += __shfl_xor(rsum, 32);
            l_run = l_run * alpha + rsum; m_run = m_new;
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[d] = acc[d] * alpha;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)                               // O^T += V^T P^T: a = V[key][16 dt + lq], b = P[query lq][key slot]
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = s[kt][r];
                    const float* vrow = &Vs[(kt * 16 + lg * 4 + r) * LD + lq];
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[dt * 16], pv, acc[dt], 0, 0, 0);
                }
            __syncthreads();
        }
    } else {
        uint4 qf[2];                                                      // the B operand of S^T = K.Q^T: lane (q, g) supplies d = 32 dg + 8 g .. + 7
#pragma unroll
        for (int dg = 0; dg < 2; ++dg) {
            uint4 t = *reinterpret_cast<const uint4*>(qp + (dg * 32 + lg * 8) * 2);
            if (!qvalid) t = make_uint4(0u, 0u, 0u, 0u);
            qf[dg] = t;
        }
        // thread t stages the key PAIRS (2 j, 2 j + 1), j = (t >> 4) + 16 i, columns c4 .. c4 + 3: adjacent keys share a dword of V^T
        const int c4 = (tid & 15) * 4, j0 = tid >> 4;
        uint2 rk[2][2], rv[2][2];
        auto load_kv = [&](int kt0) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int par = 0; par < 2; ++par) {
                    const int key = kt0 + 2 * (j0 + 16 * i) + par;
                    const bool ok = key < klen;
                    const long long kr = ok ? key : 0;
                    uint2 kx = *reinterpret_cast<const uint2*>(kb + kr * rowb + c4 * 2), vx = *reinterpret_cast<const uint2*>(vb + kr * rowb + c4 * 2);
                    if (!ok) { kx = make_uint2(0u, 0u); vx = kx; }
                    rk[i][par] = kx; rv[i][par] = vx;
                }
        };
        if (kbeg < kend) load_kv(kbeg);
        for (int kt0 = kbeg; kt0 < kend; kt0 += BKV) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k0 = 2 * (j0 + 16 * i);                         // even key of the pair, 0 .. 62
                *reinterpret_cast<uint2*>(&Ku[k0 * LD + c4 / 2]) = rk[i][0];
                *reinterpret_cast<uint2*>(&Ku[(k0 + 1) * LD + c4 / 2]) = rk[i][1];
                // key k0 = 32 blk + 16 s + 4 g + r  ->  column 32 blk + 8 g + 4 s + r (r even: the pair shares a dword)
                const int col = (k0 & 32) + ((k0 >> 2) & 3) * 8 + ((k0 >> 4) & 1) * 4 + (k0 & 3);
                const uint2 a = rv[i][0], c = rv[i][1];
                Vt[(c4 + 0) * LD + col / 2] = (a.x & 0xffffu) | (c.x << 16);
                Vt[(c4 + 1) * LD + col / 2] = (a.x >> 16) | (c.x & 0xffff0000u);
                Vt[(c4 + 2) * LD + col / 2] = (a.y & 0xffffu) | (c.y << 16);
                Vt[(c4 + 3) * LD + col / 2] = (a.y >> 16) | (c.y & 0xffff0000u);
            }
            __syncthreads();
            if (kt0 + BKV < kend) load_kv(kt0 + BKV);
            v4f s[4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                v4f sa = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dg = 0; dg < 2; ++dg) {
                    const uint4 kf = *reinterpret_cast<const uint4*>(&Ku[(kt * 16 + lq) * LD + dg * 16 + lg * 4]);
                    sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, kf), __builtin_bit_cast(v8bf, qf[dg]), sa, 0, 0, 0);
                }
                s[kt] = sa;
            }
            float mt = NEG_INF;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt0 + kt * 16 + lg * 4 + r;
                    const float x = key < klim ? s[kt][r] * sc : NEG_INF;
                    s[kt][r] = x; mt = fmaxf(mt, x);
                }
            mt = fmaxf(mt, __shfl_xor(mt, 16)); mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);
            const float alpha = (m_run == NEG_INF) ? 0.f : exp2f(m_run - m_new);
            float rsum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = s[kt][r];
                    const float e = (x == NEG_INF) ? 0.f : exp2f(x - m_new);
                    s[kt][r] = e; rsum += e;                              // the denominator sums the UNROUNDED probabilities
                }
            rsum += __shfl_xor(rsum, 16); rsum += __shfl_xor(rsum, 32);
            l_run = l_run * alpha + rsum; m_run = m_new;
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[d] = acc[d] * alpha;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {                          // k-slot (g, 4 s + r) of 32-key block blk is key 32 blk + 16 s + 4 g + r on both operands
                const uint4 pb = make_uint4(pack_bf16x2(s[2 * blk][0], s[2 * blk][1]), pack_bf16x2(s[2 * blk][2], s[2 * blk][3]),
                                            pack_bf16x2(s[2 * blk + 1][0], s[2 * blk + 1][1]), pack_bf16x2(s[2 * blk + 1][2], s[2 * blk + 1][3]));
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const uint4 vf = *reinterpret_cast<const uint4*>(&Vt[(dt * 16 + lq) * LD + blk * 16 + lg * 4]);
                    acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, vf), __builtin_bit_cast(v8bf, pb), acc[dt], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }

    if (!qvalid) return;
    // lane (q, g) holds d = 16 dt + 4 g .. + 3 of its query
    if (p.ns == 1) {
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        if constexpr (BF) {
            bf16_t* op = static_cast<bf16_t*>(p.o) + ((long long)b * p.Tn + qi) * p.ldo + h * 64 + lg * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<uint2*>(op + dt * 16) = make_uint2(pack_bf16x2(acc[dt][0] * inv, acc[dt][1] * inv), pack_bf16x2(acc[dt][2] * inv, acc[dt][3] * inv));
        } else {
            float* op = static_cast<float*>(p.o) + ((long long)b * p.Tn + qi) * p.ldo + h * 64 + lg * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<float4*>(op + dt * 16) = make_float4(acc[dt][0] * inv, acc[dt][1] * inv, acc[dt][2] * inv, acc[dt][3] * inv);
        }
        return;
    }
    const long long pi = (((long long)b * p.H + h) * p.Tn + qi) * p.ns + sl;
    if (lg == 0) { p.pm[pi] = m_run; p.pl[pi] = l_run; }                 // an empty slice: (-inf, 0), accumulator 0
    float* pop = p.po + pi * 64 + lg * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<float4*>(pop + dt * 16) = make_float4(acc[dt][0], acc[dt][1], acc[dt][2], acc[dt][3]);
}

// o[q] = sum_s w_s o_s / sum_s w_s l_s, w_s = exp(m_s - max m), slices in order; a slice with m = -inf (no visible key) contributes nothing.
// One thread per (query, 4 output columns).
template <bool BF>
__global__ __launch_bounds__(256) void attn_cached_merge_kernel(AttnCachedArgs p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nq = (long long)p.B * p.H * p.Tn;
    if (i >= nq * 16) return;
    const long long qf = i >> 4; const int d4 = (int)(i & 15) * 4;
    const int qi = (int)(qf % p.Tn), h = (int)((qf / p.Tn) % p.H), b = (int)(qf / ((long long)p.Tn * p.H));
    const float NEG_INF = -__builtin_huge_valf();
    const float* pm = p.pm + qf * p.ns; const float* pl = p.pl + qf * p.ns; const float* po = p.po + qf * p.ns * 64 + d4;
    float M = NEG_INF;
    for (int s = 0; s < p.ns; ++s) M = fmaxf(M, pm[s]);
    float L = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int s = 0; s < p.ns; ++s) {
        const float ms = pm[s];
        if (ms == NEG_INF) continue;
        const float w = BF ? exp2f(ms - M) : expf(ms - M);
        const float4 o = *reinterpret_cast<const float4*>(po + (long long)s * 64);
        L += w * pl[s]; a0 += w * o.x; a1 += w * o.y; a2 += w * o.z; a3 += w * o.w;
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;
    const long long oi = ((long long)b * p.Tn + qi) * p.ldo + h * 64 + d4;
    if constexpr (BF) *reinterpret_cast<uint2*>(static_cast<bf16_t*>(p.o) + oi) = make_uint2(pack_bf16x2(a0 * inv, a1 * inv), pack_bf16x2(a2 * inv, a3 * inv));
    else *reinterpret_cast<float4*>(static_cast<float*>(p.o) + oi) = make_float4(a0 * inv, a1 * inv, a2 * inv, a3 * inv);
}

// K | V columns of the new QKV rows [nz][Tn][3 inner] -> rows t0 .. t0 + Tn of the K and V caches of batch rows 0 .. nz - 1 (E = float | bf16_t, 16 bytes per thread)
template <typename E>
__global__ __launch_bounds__(256) void kv_append_kernel(const E* qkv, AttnCachedArgs dst, int nz, int Tn, int t0, int inner) {
    constexpr int V = 16 / (int)sizeof(E);
    const int per = 2 * inner / V;                                        // 16-byte pieces per row
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nz * Tn * per) return;
    const int c = (int)(i % per) * V, t = (int)((i / per) % Tn), b = (int)(i / ((long long)per * Tn));
    const uint4 x = *reinterpret_cast<const uint4*>(qkv + ((long long)b * Tn + t) * 3 * inner + inner + c);
    E* row = const_cast<E*>(static_cast<const E*>(c < inner ? dst.k[b] : dst.v[b])) + (long long)(t0 + t) * dst.ldc + (c < inner ? c : c - inner);
    *reinterpret_cast<uint4*>(row) = x;
}

// Input of a kernel-3 causal convolution on the incremental path: stg [nz][Tn + 2][K] = the two rows in front of this call's rows (halo [nz][2][K], zeros on the first
// call: the causal padding) ++ x [nz][Tn][K]; the last two rows of x become the halo of the next call.  Tn >= 2.  The thread that reads a halo element rewrites it.
static __global__ __launch_bounds__(256) void halo_stage_kernel(const float* x, float* halo, float* stg, int nz, int Tn, int K) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)(Tn + 2) * K;
    if (i >= nz * per) return;
    const int b = (int)(i / per); const long long r = i % per; const int t = (int)(r / K), c = (int)(r % K);
    if (t < 2) {
        float* hp = halo + ((long long)b * 2 + t) * K + c;
        stg[i] = *hp;
        *hp = x[((long long)b * Tn + Tn - 2 + t) * K + c];
    } else stg[i] = x[((long long)b * Tn + t - 2) * K + c];
}

}  // namespace cv
