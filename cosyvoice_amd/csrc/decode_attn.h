// The arithmetic the Qwen2 LM's decode attention kernels share (llm_kernels.h, llm_batch_kernels.h): rotate-half RoPE of the new token in registers, the VALU
// online-softmax wave pass, and the flash-decoding merge of (numerators, max, denominator) partials.  Device helpers only, all forced inline: a kernel keeps
// its own loads, launch geometry and stores, and gets these expressions - which decide bits - from one place.
// Lane layout of the wave pass: a 16-lane group (grp = lane / 16) covers one key row, lane sub = lane % 16 holds dims d0 = 4 sub .. + 3; the 4 groups of a wave
// take 4 consecutive keys per slot.
#pragma once
#include "common.h"

namespace cv {

constexpr int ATTN_PART = 68;      // a partial row: 64 unnormalised numerators + running max + denominator (+2 pad: rows stay 16-byte aligned)
constexpr float ATTN_NEG = -__builtin_huge_valf();      // a masked score; the running max of a wave that has seen no key

// rotate-half RoPE of 4 dims: `partner` holds dims (d + 32) % 64, sg = -1 for d < 32
__device__ __forceinline__ float4 rope_half4(float4 a, float4 partner, float4 c4, float4 s4, float sg) {
    return make_float4(a.x * c4.x + sg * partner.x * s4.x, a.y * c4.y + sg * partner.y * s4.y, a.z * c4.z + sg * partner.z * s4.z, a.w * c4.w + sg * partner.w * s4.w);
}
// dims d0 .. d0 + 3 of the 64-float head row x (a q or k head of the qkv vector) at position pos; rope tables cos / sin [max_len][32]
__device__ __forceinline__ float4 rope_row4(const float* x, const float* rope_cos, const float* rope_sin, int pos, int d0) {
    const int dp = (d0 + 32) & 63;
    const float4 c4 = *reinterpret_cast<const float4*>(rope_cos + pos * 32 + (d0 & 31));
    const float4 s4 = *reinterpret_cast<const float4*>(rope_sin + pos * 32 + (d0 & 31));
    const float4 a = *reinterpret_cast<const float4*>(x + d0), b = *reinterpret_cast<const float4*>(x + dp);
    return rope_half4(a, b, c4, s4, d0 < 32 ? -1.f : 1.f);
}
// the new token of query head h (kv head g) for a lane's d0, from qkv = [q(heads * 64) | k(kv_heads * 64) | v(kv_heads * 64)]: RoPE'd q and k, raw v
struct NewToken { float4 q4, kn4, vn4; };
__device__ __forceinline__ NewToken load_new_token(const float* qkv, int h, int g, int heads, int kv_heads, const float* rope_cos, const float* rope_sin, int pos, int d0) {
    const float* qraw = qkv + h * 64;
    const float* kq = qkv + heads * 64 + g * 64;
    const float* vq = qkv + (heads + kv_heads) * 64 + g * 64;
    const int dp = (d0 + 32) & 63;
    const float4 c4 = *reinterpret_cast<const float4*>(rope_cos + pos * 32 + (d0 & 31));
    const float4 s4 = *reinterpret_cast<const float4*>(rope_sin + pos * 32 + (d0 & 31));
    const float4 qa = *reinterpret_cast<const float4*>(qraw + d0), qb = *reinterpret_cast<const float4*>(qraw + dp);
    const float4 ka = *reinterpret_cast<const float4*>(kq + d0), kp = *reinterpret_cast<const float4*>(kq + dp);
    NewToken n;
    n.vn4 = *reinterpret_cast<const float4*>(vq + d0);
    const float sg = d0 < 32 ? -1.f : 1.f;
    n.q4 = rope_half4(qa, qb, c4, s4, sg);
    n.kn4 = rope_half4(ka, kp, c4, s4, sg);
    return n;
}
// KV-cache append of the new token's row of kv head g (cache [kv_heads][max_len][64]); the caller picks the one 16-lane group that does it
__device__ __forceinline__ void append_kv(float* kcache, float* vcache, int g, int max_len, int pos, int d0, float4 kn4, float4 vn4) {
    *reinterpret_cast<float4*>(kcache + ((long long)g * max_len + pos) * 64 + d0) = kn4;
    *reinterpret_cast<float4*>(vcache + ((long long)g * max_len + pos) * 64 + d0) = vn4;
}

// Online softmax of one wave: running max, per-group denominator (identical on the 16 lanes of a group) and this lane's 4 numerators.
struct SoftmaxState { float m_run = ATTN_NEG, l_run = 0.f; float4 acc = make_float4(0.f, 0.f, 0.f, 0.f); };

// One pass: NS slots x 4 lane groups of keys, slot sl of lane group grp is key j0 + 4 sl + grp (keys >= limit are masked).  NEWTOK: key `pos` is the new token,
// not in the cache yet - its k / v come from registers.  SKIP_EMPTY: a wave that holds no key of the pass leaves its state alone (wave-uniform); without it
// the caller guarantees that every pass holds a key.
// The lane group is an argument of its own so that the key index keeps the kernels' association (j0 + 4 sl) + grp, and the float4 operands travel by value: either one
// written the other way costs attn_decode_kernel its second wave per SIMD (profiles/decode_attn_fold.txt).
template <int NS, bool NEWTOK, bool SKIP_EMPTY>
__device__ __forceinline__ void softmax_pass(SoftmaxState& s, float4 q4, const float4* k4, const float4* v4, int j0, int grp, int limit, int pos, float4 kn4, float4 vn4) {
    const float NEG = ATTN_NEG;
    float sc[NS];
    float mt = NEG;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
        const int j = j0 + sl * 4 + grp;
        const float4 kk = (NEWTOK && j == pos) ? kn4 : k4[sl];
        float a = q4.x * kk.x + q4.y * kk.y + q4.z * kk.z + q4.w * kk.w;
        a = group16_sum(a) * 0.125f;
        sc[sl] = j < limit ? a : NEG;
        mt = fmaxf(mt, sc[sl]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16)); mt = fmaxf(mt, __shfl_xor(mt, 32));
    if (SKIP_EMPTY && mt == NEG) return;
    const float m_new = fmaxf(s.m_run, mt);          // finite: the pass holds at least one key
    const float scale = (s.m_run == NEG) ? 0.f : expf(s.m_run - m_new);
    s.acc.x *= scale; s.acc.y *= scale; s.acc.z *= scale; s.acc.w *= scale;
    float lt = 0.f;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
        const int j = j0 + sl * 4 + grp;
        const float e = (sc[sl] == NEG) ? 0.f : expf(sc[sl] - m_new);
        const float4 vv = (NEWTOK && j == pos) ? vn4 : v4[sl];
        s.acc.x += e * vv.x; s.acc.y += e * vv.y; s.acc.z += e * vv.z; s.acc.w += e * vv.w;
        lt += e;
    }
    s.l_run = s.l_run * scale + lt;
    s.m_run = m_new;
}
// after the last pass: numerators and denominator summed over the 4 lane groups
__device__ __forceinline__ void wave_finish(SoftmaxState& s) {
    s.acc.x += __shfl_xor(s.acc.x, 16); s.acc.y += __shfl_xor(s.acc.y, 16); s.acc.z += __shfl_xor(s.acc.z, 16); s.acc.w += __shfl_xor(s.acc.w, 16);
    s.acc.x += __shfl_xor(s.acc.x, 32); s.acc.y += __shfl_xor(s.acc.y, 32); s.acc.z += __shfl_xor(s.acc.z, 32); s.acc.w += __shfl_xor(s.acc.w, 32);
    s.l_run += __shfl_xor(s.l_run, 16); s.l_run += __shfl_xor(s.l_run, 32);
}
// 4 numerators of a partial row; the lane with `first` also leaves (max, denominator) - an empty partial carries max 0, denominator 0
__device__ __forceinline__ void store_partial(float* row, int d0, float4 a, float m, float l, bool first) {
    *reinterpret_cast<float4*>(row + d0) = a;
    if (first) { row[64] = (l > 0.f) ? m : 0.f; row[65] = l; }
}

// Flash-decoding merge of partial rows, in index order: M = max over the non-empty ones, a = sum expf(m - M) * numerators, den = sum expf(m - M) * l.
struct Merged {
    float4 a; float den, M;
    __device__ __forceinline__ float4 normalised() const { const float inv = 1.f / den; return make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv); }
};
// this thread's operands of rows row0 + q * stride, q < N (rows >= count re-read row count - 1: unconditional, clamped loads): numerators d0 .. + 3 and (max, denominator)
template <int N>
__device__ __forceinline__ void load_partials(const float* row0, long long stride, int d0, int count, float2* ml, float4* pa) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float* ps = row0 + min(q, count - 1) * stride;
        pa[q] = *reinterpret_cast<const float4*>(ps + d0);
        ml[q] = *reinterpret_cast<const float2*>(ps + 64);
    }
}
// The operands come through ml(q) -> (max, denominator) and pa(q) -> this thread's 4 numerators, so that a caller decides where they live: registers requested
// ahead of time (load_partials) or LDS rows read where they are used (merge_rows).  Partials q >= count do not exist.
// m0 / max_over_empty are the o_proj prologue's rule (gemv_kernel<..., NSP>), which is NOT the others': its max starts from a partial (slice 0's, or the new
// token's score) and, without a new token, runs over the empty slices too - their stored max is 0, so M can be 0 where the plain rule gives a negative max.
// Kept bit for bit: it decides the headline's logits.
template <int N, class ML, class PA>
__device__ __forceinline__ Merged merge_partials(int count, ML ml, PA pa, float m0 = ATTN_NEG, bool max_over_empty = false) {
    Merged r;
    r.M = m0;
#pragma unroll
    for (int q = 0; q < N; ++q) if (q < count && (ml(q).y > 0.f || max_over_empty)) r.M = fmaxf(r.M, ml(q).x);
    r.den = 0.f; r.a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float wgt = (q < count && ml(q).y > 0.f) ? expf(ml(q).x - r.M) : 0.f;       // an empty partial carries l = 0
        const float4 t = pa(q);
        r.den += wgt * ml(q).y;
        r.a.x += wgt * t.x; r.a.y += wgt * t.y; r.a.z += wgt * t.z; r.a.w += wgt * t.w;
    }
    return r;
}
// the N rows row0 + q * stride a workgroup's waves left in LDS
template <int N>
__device__ __forceinline__ Merged merge_rows(const float* row0, int stride, int d0) {
    return merge_partials<N>(N, [&](int q) { return make_float2(row0[q * stride + 64], row0[q * stride + 65]); },
                             [&](int q) { return *reinterpret_cast<const float4*>(row0 + q * stride + d0); });
}

}  // namespace cv
