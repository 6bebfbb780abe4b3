// CosyVoice-300M TransformerLM decode step behind ONE C entry point (reference: cosyvoice/llm/llm.py:162-223 TransformerLM.inference ->
// cosyvoice/transformer/encoder.py:267-327 forward_chunk -> encoder_layer.py:60-119 -> attention.py:200-330 RelPositionMultiHeadedAttention with its key / value cache).
//
// The step is one output row through 14 pre-norm layers over fp32 weights: 734 MB of weights per token, nothing else of size.  Until round 4 the host side
// (cosyvoice1_hip.py) replayed it as 115 launches of the general operators (LayerNorm, tiled GEMM -> GEMV, the [H][1][n] matrix_bd GEMM, the MFMA attention
// with one useful query row); what bounded it was the NUMBER of dependent launches, not their bytes.  Here the step is 73 launches (optionally one hipGraph):
//     per layer   [LayerNorm + (q+u | q+v | k | v) GEMV -> the layer's cache row]  [one-query relative-position attention, keys split over 8 workgroups per head]
//                 [merge of the 8 partial softmaxes + output GEMV + residual]  [LayerNorm + w_1 GEMV + ReLU]  [w_2 GEMV + residual]
//     around it   [embed GEMV] [LayerNorm + ReLU, * sqrt(d)] ... [after_norm + decoder GEMV -> logits]
// The GEMV is gemm_conv.h's gemv_f32_kernel (same lane / wave / k order, same four-way combine) with its input vector staged in LDS by a prologue; the LayerNorm
// prologue repeats norm_rows_kernel's register path arithmetic, so every product of the step has the bits of the launch-per-operator path.  The attention is a
// new summation order (exact fp32 dot products per key instead of the MFMA chain): results agree to fp32 rounding.
// What changes from token to token - the position, i.e. the cache row written, the key count and the first row of the relative-position table - is read by
// the kernels from a device block (Lm1Dyn) that the step's FIRST kernel (launched outside the graph, it also takes the input row's address) updates; what
// changes from request to request - the cache and table buffers - is rebound there by cv_lm1_bind.  One captured graph therefore serves every step of every request
// (option "graph", off by default: on the MI355X the replay costs 0.607 ms per token against 0.591 ms for the same launches issued one by one).
#include "api_common.h"
#include "common.h"
#include "llm_kernels.h"
#include <climits>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace cv {

constexpr int LM1_MAX_LAYERS = 32;
constexpr int LM1_SPLITS = 8;                 // key ranges per head in the decode attention
constexpr int LM1_MAX_KEYS_PER_SPLIT = 4096;  // (a bound on the cache a handle binds: 32768 positions)
#define LM1_NEG_INF (-__builtin_huge_valf())
constexpr int LM1_MAX_K = 4096;               // longest GEMV input (the feed-forward width)

struct Lm1Dyn {
    int pos, n_tab, pad0, pad1;
    float* rows[LM1_MAX_LAYERS];              // per layer [cap][4 d]: (q + u | q + v | k | v) of every position so far
    const float* tabs[LM1_MAX_LAYERS];        // per layer [2 n_tab - 1][d]: linear_pos(pe), row m = relative position n_tab - 1 - m
};

enum { LM1_PRO_NONE = 0, LM1_PRO_LN = 1, LM1_PRO_MERGE = 2 };

constexpr int LM1_MAX_SLOTS = 8;               // sequences of the lock-step batched decode (cv_lm1_batch_*)
struct Lm1GemvArgs {
    const float* x;                            // [K] (NONE / LN) or the attention partials [heads][LM1_SPLITS][66] (MERGE)
    const float* g; const float* b; float eps; // LN prologue
    const float* W; long long ldw; const float* bias; const float* res; float* y;
    Lm1Dyn* dyn; int layer;                    // layer >= 0: y = dyn->rows[layer] + pos * N   (the cache row of this position)
    int set_pos;                               // >= 0: block 0 publishes the step's position (first kernel of a step); -2: the position of the device loop (st->pos)
    const DecodeState* st;                     // set_pos == -2 (cv_lm1_decode): the loop state the sampler and advance_pos_kernel keep on the device
    int N, K, Kp, act, pro;
    // the slots of the batched decode: x / res / y above are slot 0's, dyn / st are [nb] (Lm1Dyn::pad0 != 0: the slot takes part in the step); the matrix, bias, gamma / beta are shared
    long long sx, sres, sy;                    // floats between two slots' x / res / y
    int nb;                                    // 0: the single sequence
};

// The prologue of the decode GEMVs: the input vector into LDS (xs, zero beyond K up to steps * 64 floats), by one of three rules; `issue_weights()` requests the caller's
// first weight loads at the point where they hide the most (before everything - or, under the LayerNorm, right behind the row's own loads).
template <int NW, typename F>
static __device__ __forceinline__ void lm1_gemv_prologue(const Lm1GemvArgs& p, float* xs, float* mw, int steps, F&& issue_weights) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (every prologue requests its own small operands BEFORE the caller's weight rows: vmcnt retires in issue order, what the prologue waits for must not queue behind the weight stream)
    // ---- prologue: the input vector into LDS, zero beyond K up to the last 64-float step
    if (p.pro == LM1_PRO_LN) {
        // norm_rows_kernel's register path (C <= 1024, C % 4 == 0), every wave on the whole row; wave w parks chunk w
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane * 4 + k * 256;
            const float4 t = *reinterpret_cast<const float4*>(p.x + min(c, p.K - 4));        // unconditional (clamped) loads: all four in flight together
            const bool ok = c < p.K;
            v[k] = make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
        }
        const int cw = lane * 4 + wave * 256;                   // gamma / beta of the wave's chunk travel with the row, not after the statistics
        const float4 gw = *reinterpret_cast<const float4*>(p.g + min(cw, p.K - 4)), bw = *reinterpret_cast<const float4*>(p.b + min(cw, p.K - 4));
        issue_weights();
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane * 4 + k * 256 < p.K) s += v[k].x + v[k].y + v[k].z + v[k].w;
        s = wave_sum(s);
        const float mean = s / (float)p.K;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane * 4 + k * 256 < p.K) { const float a = v[k].x - mean, b = v[k].y - mean, cc = v[k].z - mean, d = v[k].w - mean; q += a * a + b * b + cc * cc + d * d; }
        q = wave_sum(q);
        const float rstd = rsqrtf(q / (float)p.K + p.eps);
        {
            // the chunk this wave parks (same expressions as norm_rows_kernel's epilogue)
            const float4 vw = make_float4(wave == 0 ? v[0].x : wave == 1 ? v[1].x : wave == 2 ? v[2].x : v[3].x, wave == 0 ? v[0].y : wave == 1 ? v[1].y : wave == 2 ? v[2].y : v[3].y,
                                          wave == 0 ? v[0].z : wave == 1 ? v[1].z : wave == 2 ? v[2].z : v[3].z, wave == 0 ? v[0].w : wave == 1 ? v[1].w : wave == 2 ? v[2].w : v[3].w);
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            if (cw < p.K) {
                o[0] = (vw.x - mean) * rstd; o[1] = (vw.y - mean) * rstd; o[2] = (vw.z - mean) * rstd; o[3] = (vw.w - mean) * rstd;
                o[0] *= gw.x; o[1] *= gw.y; o[2] *= gw.z; o[3] *= gw.w;
                o[0] += bw.x; o[1] += bw.y; o[2] += bw.z; o[3] += bw.w;
            }
            if (cw < steps * 64) *reinterpret_cast<float4*>(&xs[cw]) = make_float4(o[0], o[1], o[2], o[3]);
        }
    } else if (p.pro == LM1_PRO_MERGE) {
        // x[h * 64 + d] = sum_s acc_s[d] * (e^(m_s - M) / sum_s l_s e^(m_s - M)): the key ranges of one head's softmax, in range order.  The LM1_SPLITS weights of a
        // head are made ONCE per workgroup (one lane per (head, range), the head's lanes combine through shuffles) and read back from LDS - not once per element.
        // Round 6: a lane's partial accumulators (up to 4 elements x LM1_SPLITS ranges) are REQUESTED before the weights are made - they do not depend on them, and
        // behind the barrier they were a second global round trip on the critical path of the launch (5.5 us for a 2 - 4 MB matrix).  Same sums, same order.
        constexpr int EPT = 4;
        const int hs = min(tid, (p.K >> 6) * LM1_SPLITS - 1);
        const float* ph = p.x + (long long)hs * 66;
        const float ms = ph[0], ls = ph[1];                      // first in the queue: the weights' shuffles start when these two land
        float as[EPT][LM1_SPLITS];
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = min(tid + i * (int)blockDim.x, p.K - 1);
            const float* pa = p.x + (long long)(e >> 6) * LM1_SPLITS * 66 + 2 + (e & 63);
#pragma unroll
            for (int s = 0; s < LM1_SPLITS; ++s) as[i][s] = pa[s * 66];
        }
        issue_weights();
        {
            float M = ms;
#pragma unroll
            for (int o = 1; o < LM1_SPLITS; o <<= 1) M = fmaxf(M, __shfl_xor(M, o));
            const float w = (ms == LM1_NEG_INF) ? 0.f : expf(ms - M);
            float L = ls * w;
#pragma unroll
            for (int o = 1; o < LM1_SPLITS; o <<= 1) L += __shfl_xor(L, o);
            if (tid < (p.K >> 6) * LM1_SPLITS) mw[tid] = w / L;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int e = tid + i * (int)blockDim.x;
            if (e < steps * 64) {
                float o = 0.f;
                if (e < p.K) {
#pragma unroll
                    for (int s = 0; s < LM1_SPLITS; ++s) o += as[i][s] * mw[(e >> 6) * LM1_SPLITS + s];
                }
                xs[e] = o;
            }
        }
        for (int e = tid + EPT * (int)blockDim.x; e < steps * 64; e += blockDim.x) {      // (beyond 4 elements per lane: not reached at the supported widths, d <= 1024)
            float o = 0.f;
            if (e < p.K) {
                const float* pa = p.x + (long long)(e >> 6) * LM1_SPLITS * 66 + 2 + (e & 63);
                float a2[LM1_SPLITS];
#pragma unroll
                for (int s = 0; s < LM1_SPLITS; ++s) a2[s] = pa[s * 66];
#pragma unroll
                for (int s = 0; s < LM1_SPLITS; ++s) o += a2[s] * mw[(e >> 6) * LM1_SPLITS + s];
            }
            xs[e] = o;
        }
    } else {
        // (requesting the vector BEFORE the weight rows - llm_kernels.h XFIRST - measured the same on this model: 327 vs 321 us per token, round 6; the weights go first)
        issue_weights();
        for (int e = tid * 4; e < steps * 64; e += 256 * NW) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < p.K) t = *reinterpret_cast<const float4*>(p.x + e);           // K % 4 == 0
            *reinterpret_cast<float4*>(&xs[e]) = t;
        }
    }
}

// ---- the decode GEMVs: y[N] = act(pro(x)[K] . W[N][K]^T + bias) (+ res), for the single sequence (NBT = 0) or for NBT = 1 / 2 / 4 / 8 slots of the lock-step batch -------
// Two kernels, each ONE body for both: a lane owns a (row, k-subset) and carries one accumulator per slot, so for every slot the products, their order, the 16-lane
// reduction and the combine of the waves' partial sums are those of the single sequence - a slot's output has the bits of cv_lm1_step on that sequence alone, whatever
// the slot count and whichever slot it sits in, and every weight row is read ONCE per step.  A lane's WHOLE share of its row is requested up front and kept in registers:
// the weights do not depend on the previous kernel's output, the input vector does, so the prologue's dependent loads (x, gamma, beta) wait under them - slot 0's
// prologue issues them right behind its own small operands; they are issued before everything when slot 0 is inactive.  The slots' input vectors go through LDS G at a
// time - all of them when the form's K <= 1024 (every LayerNorm / merge prologue), two per pass for the K <= 4096 forms (static LDS: 8 x 16.6 KB do not fit) - with a
// barrier between the passes, which does not touch any lane's order of accumulation.  A slot whose flag (Lm1Dyn::pad0) is clear is skipped: no pointer of it is read,
// nothing of it is written.  NBT = 0 reads no flag, takes p.dyn / p.st as the one sequence's and publishes the position as the first kernel of a step does.
typedef unsigned lm1_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned lm1_u32x4 __attribute__((ext_vector_type(4)));
constexpr int lm1_lds_slots(int KW, int SL) { return KW <= 1024 || SL < 2 ? SL : 2; }

// block 0 publishes the position(s) the rest of the step reads
static __device__ __forceinline__ void lm1_publish(const Lm1GemvArgs& p) {
    if (blockIdx.x != 0 || (int)threadIdx.x >= max(p.nb, 1)) return;
    if (p.set_pos == -2) p.dyn[threadIdx.x].pos = p.st[threadIdx.x].pos;
    else if (p.set_pos >= 0 && p.nb == 0) p.dyn->pos = p.set_pos;
}

// a + the lane's products of one step, added in k order.  W16 = false: the four words of w are fp32 values, against xa.  W16 = true (the model's fp16 mode, cv_lm1_use_bf16):
// a word is two bf16 (the lower k in the low half), widened here - the products and their order are those of the fp32 matrix rounded to bf16; two words go against
// xa, the other two of a 16-byte load against xb.
template <bool W16, typename V>
static __device__ __forceinline__ float lm1_fma_step(float a, const V& w, const float4& xa, const float4& xb) {
    if constexpr (W16) {
        a += __uint_as_float(w[0] << 16) * xa.x; a += __uint_as_float(w[0] & 0xffff0000u) * xa.y;
        a += __uint_as_float(w[1] << 16) * xa.z; a += __uint_as_float(w[1] & 0xffff0000u) * xa.w;
        if constexpr (sizeof(V) == 16) {
            a += __uint_as_float(w[2] << 16) * xb.x; a += __uint_as_float(w[2] & 0xffff0000u) * xb.y;
            a += __uint_as_float(w[3] << 16) * xb.z; a += __uint_as_float(w[3] & 0xffff0000u) * xb.w;
        }
    } else {
        a += __uint_as_float(w[0]) * xa.x; a += __uint_as_float(w[1]) * xa.y; a += __uint_as_float(w[2]) * xa.z; a += __uint_as_float(w[3]) * xa.w;
    }
    return a;
}

// The narrow form (gemm_conv.h's gemv_f32_kernel: same lane / wave / k order, same combine): 4 RPG output rows per workgroup, a 16-lane group per RPG rows, a lane four
// k-values of every 64-float step (fp32: 16 bytes; W16: the SAME four as 8 bytes of the bf16 [N][Kp] matrix), the NW waves split K.
// S: steps of a wave's share, all held in registers (4: K <= 1024; 8 with NW = 8: the K = 4096 product whose 1024 rows are only 256 workgroups; 16: K <= 4096 over 4 waves).
// RPG: output rows per 16-lane group.  A row's products and their order do not depend on it; what does is how much of the prologue (the input vector, its LayerNorm,
// the barrier) a workgroup pays per byte of weights and how many weight bytes a CU has in flight (options "gemv_rows" / "gemv_rows16": the single sequence only).
template <int S, int NW, bool W16, int NBT, int RPG = 1>
static __global__ __launch_bounds__(64 * NW) void lm1_gemv_kernel(Lm1GemvArgs p) {
    static_assert(RPG == 1 || NBT == 0, "rows per group are an option of the single sequence");
    constexpr int SL = NBT ? NBT : 1, KW = S * NW * 64, G = lm1_lds_slots(KW, SL), XS = KW + 64;       // KW: the longest input the registers cover
    __shared__ __attribute__((aligned(16))) float xs[G * XS];
    __shared__ float part[SL][NW][4 * RPG];
    __shared__ float mw[G][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, sub = lane & 15;
    const int steps = (p.Kp + 63) / 64;
    lm1_publish(p);
    bool on[SL];
#pragma unroll
    for (int s = 0; s < SL; ++s) on[s] = NBT == 0 || (s < p.nb && p.dyn[min(s, p.nb - 1)].pad0 != 0);
    const int row0 = ((int)blockIdx.x * 4 + grp) * RPG;           // this group's rows row0 .. row0 + RPG - 1 (clamped below: the reductions are wave collectives)
    const int s0 = wave * steps / NW, s1 = (wave + 1) * steps / NW;
    using raw_t = typename std::conditional<W16, lm1_u32x2, lm1_u32x4>::type;
    raw_t w[RPG][S];
    auto load_all = [&] {
#pragma unroll
        for (int i = 0; i < RPG; ++i) {
            const long long ro = (long long)min(row0 + i, p.N - 1) * p.ldw;
#pragma unroll
            for (int u = 0; u < S; ++u) {                       // unconditional loads (clamped step) keep the vmcnt bookkeeping exact
                const int k = min(min(s0 + u, max(s1 - 1, 0)) * 64 + sub * 4, p.Kp - 4);
                if constexpr (W16) w[i][u] = __builtin_nontemporal_load(reinterpret_cast<const lm1_u32x2*>(reinterpret_cast<const unsigned short*>(p.W) + ro + k));
                else w[i][u] = __builtin_nontemporal_load(reinterpret_cast<const lm1_u32x4*>(p.W + ro + k));
            }
        }
    };
    if (!on[0]) load_all();                                     // (slot 0's prologue requests them behind its own small operands)
    float acc[SL][RPG];
#pragma unroll
    for (int s = 0; s < SL; ++s)
#pragma unroll
        for (int i = 0; i < RPG; ++i) acc[s][i] = 0.f;
#pragma unroll
    for (int p0 = 0; p0 < SL; p0 += G) {
        if (p0 > 0) __syncthreads();                            // every lane is done with the previous pass's vectors
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int sl = p0 + g;
            if (on[sl]) {
                Lm1GemvArgs ps = p;
                ps.x = p.x + sl * p.sx;
                lm1_gemv_prologue<NW>(ps, xs + g * XS, mw[g], steps, [&] { if (sl == 0) load_all(); });
            }
        }
        __syncthreads();
        // ---- the rows' dot products (gemv_f32_kernel: same loads, same order)
#pragma unroll
        for (int u = 0; u < S; ++u) {
            if (s0 + u < s1) {
                const int k = (s0 + u) * 64 + sub * 4;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (on[p0 + g]) {
                        const float4 x = *reinterpret_cast<const float4*>(&xs[g * XS + k]);
#pragma unroll
                        for (int i = 0; i < RPG; ++i) acc[p0 + g][i] = lm1_fma_step<W16>(acc[p0 + g][i], w[i][u], x, x);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        if (on[s]) {
#pragma unroll
            for (int i = 0; i < RPG; ++i) {
                const float a = group16_sum(acc[s][i]);
                if (sub == 0) part[s][wave][grp * RPG + i] = a;
            }
        }
    }
    __syncthreads();
    static_assert(RPG * SL <= 16, "a lane of the group per (row, slot)");
    const int sl = sub / RPG, gi = grp * RPG + sub % RPG, n = row0 + sub % RPG;      // lane `sub` of wave 0's group finishes row `sub % RPG` of slot `sub / RPG`
    if (wave != 0 || sl >= (NBT ? min(p.nb, NBT) : 1) || n >= p.N) return;
    if (NBT != 0 && p.dyn[sl].pad0 == 0) return;
    float v = ((part[sl][0][gi] + part[sl][1][gi]) + part[sl][2][gi]) + part[sl][3][gi];
    if (NW == 8) v = (((v + part[sl][4 % NW][gi]) + part[sl][5 % NW][gi]) + part[sl][6 % NW][gi]) + part[sl][7 % NW][gi];
    if (p.bias) v += p.bias[n];
    v = apply_act(p.act, v, 0.f);
    if (p.res) v += p.res[sl * p.sres + n];
    float* y = p.layer >= 0 ? p.dyn[sl].rows[p.layer] + (long long)p.dyn[sl].pos * p.N : p.y + sl * p.sy;
    y[n] = v;
}

// The wide form, laid out over the lanes the way the CosyVoice2 decode GEMVs are (llm_kernels.h gemv_norm_kernel), round 6: a 16-lane group owns a whole row and a lane
// ONE 16-byte load per step - W16: 8 consecutive k-values of a 128-float step of the bf16 matrix (option "gemv16_wide", default 1); W16 = false: 4 of a 64-float step of
// the fp32 matrix (option "gemv_wide"; KSPLIT = false only: the split forms ARE lm1_gemv_kernel's).  STEPS: steps of a lane's share, all held in registers.
//   KSPLIT = false: a wave's four groups keep their rows to themselves over the whole K (K <= STEPS steps) - 4 NW rows per workgroup, e.g. 256 workgroups for the
//                   [4096][1024] products: the input row and its LayerNorm are made once per 16 rows instead of once per 4 (lm1_gemv_kernel: 1024 workgroups, each
//                   re-reading 16 KB of x / gamma / beta against 8 KB of weights);
//   KSPLIT = true:  the NW waves share 4 rows and split K (the [1024][4096] product and the products with few rows), partial sums combined in wave order.
// The k order of a row's sum differs from lm1_gemv_kernel's: results agree to fp32 rounding, the weights are the same values.
template <bool W16, int STEPS, int NW, bool KSPLIT, int NBT>
static __global__ __launch_bounds__(64 * NW) void lm1_gemv16_kernel(Lm1GemvArgs p) {
    constexpr int SK = W16 ? 128 : 64, LK = W16 ? 8 : 4;        // k-values per step / per lane and step
    // KW: the input LDS of a slot - the longest K the registers cover; the single sequence keeps the LM1_MAX_K it had before the kernel took slots (1024 measures the same:
    // profiles/lm1_gemv_fold_ab.txt)
    constexpr int SL = NBT ? NBT : 1, KW = NBT ? STEPS * SK * (KSPLIT ? NW : 1) : LM1_MAX_K, G = lm1_lds_slots(KW, SL), XS = KW + 64;
    __shared__ __attribute__((aligned(16))) float xs[G * XS];
    __shared__ float part[SL][NW][4];
    __shared__ float mw[G][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, sub = lane & 15;
    const int steps = p.Kp / SK;                                 // steps of a row (pick_form checks Kp % SK == 0)
    lm1_publish(p);
    bool on[SL];
#pragma unroll
    for (int s = 0; s < SL; ++s) on[s] = NBT == 0 || (s < p.nb && p.dyn[min(s, p.nb - 1)].pad0 != 0);
    const int row0 = KSPLIT ? (int)blockIdx.x * 4 + grp : ((int)blockIdx.x * NW + wave) * 4 + grp;
    const int s0 = KSPLIT ? wave * steps / NW : 0, s1 = KSPLIT ? (wave + 1) * steps / NW : steps;
    lm1_u32x4 w[STEPS];
    auto load_all = [&] {
        const long long ro = (long long)min(row0, p.N - 1) * p.ldw + sub * LK;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {                       // unconditional loads (clamped step): the vmcnt bookkeeping stays exact
            const long long k = ro + (long long)min(s0 + s, max(s1 - 1, 0)) * SK;
            if constexpr (W16) w[s] = __builtin_nontemporal_load(reinterpret_cast<const lm1_u32x4*>(reinterpret_cast<const unsigned short*>(p.W) + k));
            else w[s] = __builtin_nontemporal_load(reinterpret_cast<const lm1_u32x4*>(p.W + k));
            order_memory();                                     // requested in the order the steps are consumed: vmcnt retires in issue order, and left alone the scheduler
        }                                                       // issues step 0 seventh of eight - the first product then waits for seven loads (10 % of the whole-row forms' time)
    };
    if (!on[0]) load_all();
    float acc[SL];
#pragma unroll
    for (int s = 0; s < SL; ++s) acc[s] = 0.f;
#pragma unroll
    for (int p0 = 0; p0 < SL; p0 += G) {
        if (p0 > 0) __syncthreads();
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int sl = p0 + g;
            if (on[sl]) {
                Lm1GemvArgs ps = p;
                ps.x = p.x + sl * p.sx;
                lm1_gemv_prologue<NW>(ps, xs + g * XS, mw[g], steps * SK / 64, [&] { if (sl == 0) load_all(); });
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            if (s0 + s < s1) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (on[p0 + g]) {
                        const float* xg = &xs[g * XS + (s0 + s) * SK + sub * LK];
                        const float4 xa = *reinterpret_cast<const float4*>(xg);
                        float4 xb = xa;
                        if constexpr (W16) xb = *reinterpret_cast<const float4*>(xg + 4);
                        acc[p0 + g] = lm1_fma_step<W16>(acc[p0 + g], w[s], xa, xb);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SL; ++s) if (on[s]) acc[s] = group16_sum(acc[s]);
    if constexpr (KSPLIT) {
#pragma unroll
        for (int s = 0; s < SL; ++s) if (on[s] && sub == 0) part[s][wave][grp] = acc[s];
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int s = 0; s < SL; ++s) if (on[s]) { float t = 0.f; for (int ww = 0; ww < NW; ++ww) t += part[s][ww][grp]; acc[s] = t; }
    }
    if (sub != 0 || row0 >= p.N) return;
    const int n = row0;
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        if (on[s]) {
            float v = acc[s];
            if (p.bias) v += p.bias[n];
            v = apply_act(p.act, v, 0.f);
            if (p.res) v += p.res[s * p.sres + n];
            float* y = p.layer >= 0 ? p.dyn[s].rows[p.layer] + (long long)p.dyn[s].pos * p.N : p.y + s * p.sy;
            y[n] = v;
        }
    }
}

// LayerNorm -> activation -> * scale of one row (the input layer's norm; its output is the residual stream, so it is materialised)
// (batched decode: workgroup b is slot b - sx / sy floats between the slots' rows, `dyns` their flags; the single step launches one workgroup with dyns = null)
struct Lm1NormArgs { const float* x; float* y; const float* g; const float* b; float eps, scale; int C, act; long long sx = 0, sy = 0; const Lm1Dyn* dyns = nullptr; };
static __global__ __launch_bounds__(64) void lm1_norm_kernel(Lm1NormArgs p) {
    const int lane = threadIdx.x;
    if (p.dyns) { if (p.dyns[blockIdx.x].pad0 == 0) return; p.x += (long long)blockIdx.x * p.sx; p.y += (long long)blockIdx.x * p.sy; }
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane * 4 + k * 256;
        v[k] = c < p.C ? *reinterpret_cast<const float4*>(p.x + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (lane * 4 + k * 256 < p.C) s += v[k].x + v[k].y + v[k].z + v[k].w;
    s = wave_sum(s);
    const float mean = s / (float)p.C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (lane * 4 + k * 256 < p.C) { const float a = v[k].x - mean, b = v[k].y - mean, cc = v[k].z - mean, d = v[k].w - mean; q += a * a + b * b + cc * cc + d * d; }
    q = wave_sum(q);
    const float rstd = rsqrtf(q / (float)p.C + p.eps);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane * 4 + k * 256;
        if (c >= p.C) continue;
        float o[4] = {(v[k].x - mean) * rstd, (v[k].y - mean) * rstd, (v[k].z - mean) * rstd, (v[k].w - mean) * rstd};
        const float4 g = *reinterpret_cast<const float4*>(p.g + c); o[0] *= g.x; o[1] *= g.y; o[2] *= g.z; o[3] *= g.w;
        const float4 b = *reinterpret_cast<const float4*>(p.b + c); o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w;
        const float4 t = apply_act4(p.act, make_float4(o[0], o[1], o[2], o[3]), 0.f);
        *reinterpret_cast<float4*>(p.y + c) = make_float4(t.x * p.scale, t.y * p.scale, t.z * p.scale, t.w * p.scale);
    }
}

// One query (the row at `pos`), head h, key range s of LM1_SPLITS:  score_j = ((q + u) . k_j + (q + v) . p_(n - 1 - j)) * scale  (attention.py:300-326; for the last
// query rel_shift leaves column j = relative position n - 1 - j), partial softmax (m, l, acc[64]) over the range -> part[h][s][66].
// ONE pass: a 16-lane group owns a key (4 of the 64 dimensions per lane) and requests its k, p AND v rows together, LM1_AU keys per group in flight - up to
// 16 * LM1_AU * LM1_SPLITS = 512 keys the whole context is requested before the first score exists (the kernel is a chain of latencies, not of bytes); every
// group keeps a running (m, l, acc) over its keys, the 16 groups merge through LDS.
constexpr int LM1_AU = 4;
// (batched decode: blockIdx.z is the slot - its own Lm1Dyn and its own block of `part`, slot_part floats further; an inactive slot returns at once)
struct Lm1AttnArgs { const Lm1Dyn* dyn; int layer, d, heads; float scale; float* part; long long slot_part = 0; int batched = 0; };
static __global__ __launch_bounds__(256) void lm1_attn_kernel(Lm1AttnArgs p) {
    __shared__ float gm[16], gl[16];
    __shared__ float gacc[16][64];
    const int h = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, sub = tid & 15, kg = tid >> 4;
    if (p.batched) { p.dyn += blockIdx.z; p.part += (long long)blockIdx.z * p.slot_part; if (p.dyn->pad0 == 0) return; }
    const int pos = p.dyn->pos, n = pos + 1, d = p.d;
    const int per = (n + LM1_SPLITS - 1) / LM1_SPLITS, j0 = min(n, s * per), j1 = min(n, j0 + per), cnt = j1 - j0;
    const float* rows = p.dyn->rows[p.layer];
    const float* qrow = rows + (long long)pos * 4 * d + h * 64;
    const float* tab = p.dyn->tabs[p.layer] + (long long)(p.dyn->n_tab - n) * d + h * 64;
    float* out = p.part + ((long long)h * LM1_SPLITS + s) * 66;
    float4 kx[LM1_AU], px[LM1_AU], vx[LM1_AU];
    auto issue = [&](int i0) {
#pragma unroll
        for (int u = 0; u < LM1_AU; ++u) {                      // unconditional (clamped) loads: all 3 * LM1_AU in flight together
            const int j = min(j0 + min(i0 + u * 16 + kg, max(cnt - 1, 0)), pos);      // (an empty range still reads a valid row: no branch around the loads)
            const float* r = rows + (long long)j * 4 * d + h * 64 + sub * 4;
            kx[u] = *reinterpret_cast<const float4*>(r + 2 * d);
            vx[u] = *reinterpret_cast<const float4*>(r + 3 * d);
            px[u] = *reinterpret_cast<const float4*>(tab + (long long)j * d + sub * 4);
        }
    };
    float m_run = LM1_NEG_INF, l_run = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i0 = 0;; i0 += 16 * LM1_AU) {
        issue(i0);
        // the query is requested WITH the sweep's rows (an offset the compiler cannot see through keeps these two loads inside the loop: hoisted, they are waited
        // for before the rows are requested - two round trips instead of one)
        const int zero = cv_opaque_zero();
        const float4 qu = *reinterpret_cast<const float4*>(qrow + sub * 4 + zero), qv = *reinterpret_cast<const float4*>(qrow + d + sub * 4 + zero);
        float sc[LM1_AU];
        float mt = m_run;
#pragma unroll
        for (int u = 0; u < LM1_AU; ++u) {
            float a = qu.x * kx[u].x; a += qu.y * kx[u].y; a += qu.z * kx[u].z; a += qu.w * kx[u].w;
            float b = qv.x * px[u].x; b += qv.y * px[u].y; b += qv.z * px[u].z; b += qv.w * px[u].w;
            const float sj = (group16_sum(a) + group16_sum(b)) * p.scale;         // (collectives outside the select)
            sc[u] = (i0 + u * 16 + kg < cnt) ? sj : LM1_NEG_INF;
            mt = fmaxf(mt, sc[u]);
        }
        if (mt != LM1_NEG_INF) {                                // (a group with no key in this sweep and none before keeps its empty state)
            const float alpha = (m_run == LM1_NEG_INF) ? 0.f : expf(m_run - mt);
            l_run *= alpha; acc.x *= alpha; acc.y *= alpha; acc.z *= alpha; acc.w *= alpha;
#pragma unroll
            for (int u = 0; u < LM1_AU; ++u) {
                const float e = (sc[u] == LM1_NEG_INF) ? 0.f : expf(sc[u] - mt);
                l_run += e; acc.x += e * vx[u].x; acc.y += e * vx[u].y; acc.z += e * vx[u].z; acc.w += e * vx[u].w;
            }
            m_run = mt;
        }
        if (i0 + 16 * LM1_AU >= cnt) break;
    }
    if (sub == 0) { gm[kg] = m_run; gl[kg] = l_run; }
    *reinterpret_cast<float4*>(&gacc[kg][sub * 4]) = acc;
    __syncthreads();
    if (tid >= 64) return;
    float M = LM1_NEG_INF;
#pragma unroll
    for (int g = 0; g < 16; ++g) M = fmaxf(M, gm[g]);
    float L = 0.f, a = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {                              // fixed group order
        const float w = (gm[g] == LM1_NEG_INF) ? 0.f : expf(gm[g] - M);
        L += gl[g] * w; a += gacc[g][tid] * w;
    }
    out[2 + tid] = a;
    if (tid == 0) { out[0] = M; out[1] = L; }
}

static __global__ void lm1_bind_kernel(Lm1Dyn* dyn, Lm1Dyn v) { if (threadIdx.x == 0 && blockIdx.x == 0) *dyn = v; }
// a slot of the batched decode: rebinding (a grown cache) keeps the slot's flag and position; the flag is set when a request is parked and cleared when the slot is freed
static __global__ void lm1_bind_slot_kernel(Lm1Dyn* dyn, Lm1Dyn v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { v.pad0 = dyn->pad0; v.pos = dyn->pos; *dyn = v; }
}
static __global__ void lm1_slot_flag_kernel(Lm1Dyn* dyn, DecodeState* st, int on) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { dyn->pad0 = on; if (!on) st->done = 1; }
}
static __global__ void lm1_advance_slots_kernel(DecodeState* st, int nb) { if ((int)threadIdx.x < nb && !st[threadIdx.x].done) st[threadIdx.x].pos += 1; }

struct Lm1Layer {
    const float *ln1_g, *ln1_b, *w_qkv, *b_qkv, *w_out, *b_out, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
};

}  // namespace cv

using namespace cv;

struct cv_lm1 {
    int n_layers = 0, d = 0, heads = 0, ffn = 0, d_in = 0, n_out = 0, act = 0, cap = 0;
    float xscale = 1.f;
    std::vector<Lm1Layer> L;
    const float *embed_w = nullptr, *embed_b = nullptr, *embed_g = nullptr, *embed_beta = nullptr, *after_g = nullptr, *after_b = nullptr, *dec_w = nullptr, *dec_b = nullptr;
    // fp16 mode of this model (cv_lm1_use_bf16): the same matrices as bf16 [N][Kp]; null = fp32
    struct L16 { const void *w_qkv = nullptr, *w_out = nullptr, *w1 = nullptr, *w2 = nullptr; };
    std::vector<L16> L16s; const void* embed_w16 = nullptr; const void* dec_w16 = nullptr; bool w16 = false;
    int wide16 = 1;                    // bf16 matrices on lm1_gemv16_kernel (16-byte loads, whole rows per lane group; option "gemv16_wide", env CV_LM1_WIDE16); 0: lm1_gemv_kernel<.., true>
    int wide32 = 1;                    // the same for the fp32 matrices of the [N >= 2048][K <= 1024] products (option "gemv_wide", env CV_LM1_WIDE)
    int rows32 = 1, rows16 = 1;        // output rows per 16-lane group of the decode GEMVs over fp32 / bf16 matrices (option "gemv_rows" / "gemv_rows16": 1 | 2 | 4; the same bits)
    DevBuf dyn, x0, x1, h, ff, part;
    // the device-resident decode loop (cv_lm1_decode_begin / cv_lm1_decode): loop state, sampling parameters, emitted tokens, the next input row, logits, injected uniforms
    DevBuf dstate, dsp, dtokens, xin, dlogits, duniforms;
    int max_tokens = 0; const float* emb_table = nullptr; DecodeState host_state{}; std::vector<int> host_tokens; int loop_open = 0;
    hipGraphExec_t graph = nullptr; float* graph_logits = nullptr; hipStream_t graph_stream = nullptr;
    hipStream_t own_stream = nullptr;          // a NULL stream argument means this (blocking) stream: it orders itself against the legacy default stream, and it can be captured
    int use_graph = 0, bound = 0;              // measured on the MI355X (profiles/r4_cv1_fused_step_timing.txt): the replayed graph is 3 % SLOWER per token than the same 72 launches issued eagerly
    long long steps = 0, graph_replays = 0;
    // the lock-step batched decode (cv_lm1_batch_*): per-slot copies of everything above that belongs to ONE sequence
    struct Slot { int bound = 0, open = 0, cap = 0, returned = 0; DecodeState host{}; };
    struct Batch {
        int nb = 0, tok_cap = 0, uni_cap = 0;
        Slot slots[LM1_MAX_SLOTS];
        DevBuf dyns, sts, sps, tokens, uniforms, xin, logits, x0, x1, h, ff, part;
        const float* emb_table = nullptr;
        std::vector<DecodeState> host_states; std::vector<int> host_tokens;
        hipStream_t stream = nullptr;
    } batch;
    long long batch_steps = 0;
    ~cv_lm1() { if (graph) (void)hipGraphExecDestroy(graph); if (own_stream) (void)hipStreamDestroy(own_stream); }
};

namespace {

inline int kp_of(int K) { return (K + 31) / 32 * 32; }

hipStream_t resolve(cv_lm1* m, void* s) {
    if (s) return as_stream(s);
    if (!m->own_stream) CV_HIP(hipStreamCreate(&m->own_stream));
    return m->own_stream;
}

// ---- the kernel form of a decode GEMV ---------------------------------------------------------------------------------------------------------------------
// ONE table for the single-sequence step (NBT = 0) and the lock-step batch (NBT = 1 / 2 / 4 / 8 slots): a slot of the batch goes through another instantiation of the
// kernel the single step picks for the same (N, K, dtype, prologue), and that is what keeps a slot's bits those of the single step.
enum Lm1Form {      // kernel                                               longest K (the slots' vectors in LDS at a time; NBT = 0 of lm1_gemv16_kernel: LDS for 4096)
    LM1_F16_ROWS,   // lm1_gemv16_kernel<true, 8, 4, false, NBT>            1024 (all)   bf16, 16-byte loads, 16 whole rows per workgroup
    LM1_F16_SPLIT,  // lm1_gemv16_kernel<true, 2, 4, true, NBT>             1024 (all)   bf16, 4 waves split K
    LM1_F16_SPLIT8, // lm1_gemv16_kernel<true, 4, 8, true, NBT>             4096 (two)   bf16, 8 waves split K
    LM1_F32_ROWS,   // lm1_gemv16_kernel<false, 16, 4, false, NBT>          1024 (all)   fp32, 16 whole rows per workgroup
    LM1_U4,         // lm1_gemv_kernel<4, 4, W16, NBT, RPG>                 1024 (all)   a wave's share is at most 4 steps
    LM1_U8_NW8,     // lm1_gemv_kernel<8, 8, W16, NBT, RPG>                 4096 (two)   8 waves, 8 steps each
    LM1_U8          // lm1_gemv_kernel<16, 4, W16, NBT, RPG>                4096 (two)   4 waves, 16 steps each
};
struct Lm1Pick { Lm1Form form; int rows; bool rpg; };      // rows: output rows per workgroup; rpg: an lm1_gemv_kernel form (single sequence: rows times RPG, option "gemv_rows")

Lm1Pick pick_form(bool h16, int wide16, int wide32, int pro, int N, int K) {
    const int kp = kp_of(K), steps = (kp + 63) / 64;
    if (h16 && wide16 && kp % 128 == 0) {                      // 16-byte loads, whole rows per lane group (lm1_gemv16_kernel)
        const int st = kp / 128;
        if (st <= 8 && N >= 2048) return {LM1_F16_ROWS, 16, false};
        if (st <= 8) return {LM1_F16_SPLIT, 4, false};
        if (st <= 32 && pro == LM1_PRO_NONE) return {LM1_F16_SPLIT8, 4, false};
    }
    if (!h16 && wide32 && kp % 64 == 0 && kp <= 1024 && N >= 2048) return {LM1_F32_ROWS, 16, false};     // fp32 matrices, whole rows per lane group
    if (steps <= 16) return {LM1_U4, 4, true};
    if (pro == LM1_PRO_NONE && N <= 2048) return {LM1_U8_NW8, 4, true};
    return {LM1_U8, 4, true};
}

// What a step works on: one sequence, or the nb slots of the batch - a slot's row one row width after the previous slot's.
struct Lm1Seq {
    int nb;                                    // 0: the single sequence (cv_lm1_step / cv_lm1_decode); 1..8: the slots of cv_lm1_batch_*
    Lm1Dyn* dyn; DecodeState* st; float *x0, *x1, *h, *ff, *part;
};
// ... and what the device loop adds (decode_step): sampling parameters, emitted tokens, the next input row, logits, injected uniforms
struct Lm1Loop { SampleParams* sp; int* tokens; float *xin, *logits, *uniforms; const float* emb_table; int tok_cap, uni_cap; };
Lm1Seq seq_single(cv_lm1* m) { return {0, m->dyn.as<Lm1Dyn>(), m->dstate.as<DecodeState>(), m->x0.as<float>(), m->x1.as<float>(), m->h.as<float>(), m->ff.as<float>(), m->part.as<float>()}; }
Lm1Loop loop_single(cv_lm1* m) { return {m->dsp.as<SampleParams>(), m->dtokens.as<int>(), m->xin.as<float>(), m->dlogits.as<float>(), m->duniforms.as<float>(), m->emb_table, m->max_tokens, 0}; }
Lm1Seq seq_batch(cv_lm1* m) {
    cv_lm1::Batch& B = m->batch;
    return {B.nb, B.dyns.as<Lm1Dyn>(), B.sts.as<DecodeState>(), B.x0.as<float>(), B.x1.as<float>(), B.h.as<float>(), B.ff.as<float>(), B.part.as<float>()};
}
Lm1Loop loop_batch(cv_lm1* m) {
    cv_lm1::Batch& B = m->batch;
    return {B.sps.as<SampleParams>(), B.tokens.as<int>(), B.xin.as<float>(), B.logits.as<float>(), B.uniforms.as<float>(), B.emb_table, B.tok_cap, B.uni_cap};
}

// the launch of form f for NBT slots (0: the single sequence, the only one with rpg > 1 rows per lane group)
template <int NBT>
void launch_gemv(Lm1Pick f, bool h16, int rpg, const Lm1GemvArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.N + f.rows * rpg - 1) / (f.rows * rpg)));
#define LM1_GEMV16(W16_, STEPS_, NW_, KSPLIT_) hipLaunchKernelGGL((lm1_gemv16_kernel<W16_, STEPS_, NW_, KSPLIT_, NBT>), grid, dim3(64 * NW_), 0, s, a)
#define LM1_GEMV(S_, NW_, W16_, RPG_) hipLaunchKernelGGL((lm1_gemv_kernel<S_, NW_, W16_, NBT, RPG_>), grid, dim3(64 * NW_), 0, s, a)
#define LM1_GEMV_R(S_, NW_, W16_) do { if constexpr (NBT != 0) LM1_GEMV(S_, NW_, W16_, 1); else if (rpg == 4) LM1_GEMV(S_, NW_, W16_, 4); \
                                       else if (rpg == 2) LM1_GEMV(S_, NW_, W16_, 2); else LM1_GEMV(S_, NW_, W16_, 1); } while (0)
#define LM1_GEMV_H(S_, NW_) do { if (h16) LM1_GEMV_R(S_, NW_, true); else LM1_GEMV_R(S_, NW_, false); } while (0)
    switch (f.form) {
    case LM1_F16_ROWS:   LM1_GEMV16(true, 8, 4, false); break;
    case LM1_F16_SPLIT:  LM1_GEMV16(true, 2, 4, true); break;
    case LM1_F16_SPLIT8: LM1_GEMV16(true, 4, 8, true); break;
    case LM1_F32_ROWS:   LM1_GEMV16(false, 16, 4, false); break;
    case LM1_U4:         LM1_GEMV_H(4, 4); break;
    case LM1_U8_NW8:     LM1_GEMV_H(8, 8); break;
    case LM1_U8:         LM1_GEMV_H(16, 4); break;
    }
#undef LM1_GEMV_H
#undef LM1_GEMV_R
#undef LM1_GEMV
#undef LM1_GEMV16
}

// One decode GEMV on q's sequence or slots (sx / sres / sy: floats between two slots' x / res / y).  W16: the bf16 copy of W (cv_lm1_use_bf16) or null
void gemv(cv_lm1* m, const Lm1Seq& q, int pro, const float* x, long long sx, const float* g, const float* b, float eps, const float* W, const void* W16, const float* bias,
          const float* res, long long sres, float* y, long long sy, int layer, int set_pos, int N, int K, int act, hipStream_t s) {
    CV_CHECK(K % 4 == 0 && K <= LM1_MAX_K && (pro != LM1_PRO_LN || K <= 1024), "cv_lm1: a GEMV input of up to 4096 floats (1024 under the LayerNorm prologue), K % 4 == 0");
    const bool h16 = m->w16 && W16 != nullptr;
    const Lm1Pick f = pick_form(h16, m->wide16, m->wide32, pro, N, K);
    const Lm1GemvArgs a{x, g, b, eps, h16 ? reinterpret_cast<const float*>(W16) : W, (long long)kp_of(K), bias, res, y, q.dyn, layer, set_pos, q.st, N, K, kp_of(K), act, pro, sx, sres, sy, q.nb};
    if (q.nb == 0) launch_gemv<0>(f, h16, !f.rpg ? 1 : h16 ? m->rows16 : m->rows32, a, s);
    else if (q.nb == 1) launch_gemv<1>(f, h16, 1, a, s);
    else if (q.nb == 2) launch_gemv<2>(f, h16, 1, a, s);
    else if (q.nb <= 4) launch_gemv<4>(f, h16, 1, a, s);
    else launch_gemv<8>(f, h16, 1, a, s);
}

// The decode attention of one layer: nb == 0 is the single-sequence launch on dyn[0], nb >= 1 the batched one (blockIdx.z = slot, a slot's partials heads * LM1_SPLITS * 66
// floats after the previous slot's).  Shared by walk() and the kernel's test entry point (cv_lm1_attention).
void launch_attn(const Lm1Dyn* dyn, int layer, int d, int heads, float scale, float* part, int nb, hipStream_t s) {
    Lm1AttnArgs aa{dyn, layer, d, heads, scale, part};
    if (nb > 0) { aa.slot_part = (long long)heads * LM1_SPLITS * 66; aa.batched = 1; }
    hipLaunchKernelGGL(lm1_attn_kernel, dim3(heads, LM1_SPLITS, nb > 0 ? nb : 1), dim3(256), 0, s, aa);
}

// everything of a step after its first kernel (the input layer's Linear: q.h), for the single sequence and for the slots of the batch
void walk(cv_lm1* m, const Lm1Seq& q, float* logits, hipStream_t s) {
    const int d = m->d, ffn = m->ffn;
    const long long sp = (long long)m->heads * LM1_SPLITS * 66;
    Lm1NormArgs na{q.h, q.x0, m->embed_g, m->embed_beta, 1e-5f, m->xscale, d, m->act};
    if (q.nb) { na.sx = d; na.sy = d; na.dyns = q.dyn; }
    hipLaunchKernelGGL(lm1_norm_kernel, dim3(q.nb ? q.nb : 1), dim3(64), 0, s, na);
    for (int i = 0; i < m->n_layers; ++i) {
        const Lm1Layer& L = m->L[i];
        const cv_lm1::L16 H = m->w16 ? m->L16s[i] : cv_lm1::L16{};
        gemv(m, q, LM1_PRO_LN, q.x0, d, L.ln1_g, L.ln1_b, 1e-12f, L.w_qkv, H.w_qkv, L.b_qkv, nullptr, 0, nullptr, 0, i, -1, 4 * d, d, ACT_NONE, s);
        launch_attn(q.dyn, i, d, m->heads, 0.125f, q.part, q.nb, s);
        gemv(m, q, LM1_PRO_MERGE, q.part, sp, nullptr, nullptr, 0.f, L.w_out, H.w_out, L.b_out, q.x0, d, q.x1, d, -1, -1, d, d, ACT_NONE, s);
        gemv(m, q, LM1_PRO_LN, q.x1, d, L.ln2_g, L.ln2_b, 1e-12f, L.w1, H.w1, L.b1, nullptr, 0, q.ff, ffn, -1, -1, ffn, d, m->act, s);
        gemv(m, q, LM1_PRO_NONE, q.ff, ffn, nullptr, nullptr, 0.f, L.w2, H.w2, L.b2, q.x1, d, q.x0, d, -1, -1, d, ffn, ACT_NONE, s);
    }
    gemv(m, q, LM1_PRO_LN, q.x0, d, m->after_g, m->after_b, 1e-5f, m->dec_w, m->dec_w16, m->dec_b, nullptr, 0, logits, m->n_out, -1, -1, m->n_out, d, ACT_NONE, s);
}

// the first kernel of a step: the input layer's Linear on x (pos >= 0: the caller's row and position; -2: the parked rows and the positions of the device loop)
void embed(cv_lm1* m, const Lm1Seq& q, const float* x, int set_pos, hipStream_t s) {
    gemv(m, q, LM1_PRO_NONE, x, m->d_in, nullptr, nullptr, 0.f, m->embed_w, m->embed_w16, m->embed_b, nullptr, 0, q.h, m->d, -1, set_pos, m->d, m->d_in, ACT_NONE, s);
}

// one step of the device loop (cv_lm1_decode; cv_lm1_batch_decode: a lock-step step of every active slot): the step on the parked input, the sampler, the advance
void decode_step(cv_lm1* m, const Lm1Seq& q, const Lm1Loop& l, hipStream_t s) {
    embed(m, q, l.xin, -2, s);
    walk(m, q, l.logits, s);
    SampleArgs sa{};
    sa.logits = l.logits; sa.V = m->n_out; sa.sp = l.sp; sa.uniforms = l.uniforms;
    sa.st = q.st; sa.tokens = l.tokens; sa.max_tokens = l.tok_cap;
    sa.emb_table_f32 = l.emb_table; sa.emb_dim = m->d_in; sa.h_out = l.xin;
    if (q.nb) { sa.slot_logits = m->n_out; sa.slot_uniforms = l.uni_cap; sa.slot_tokens = l.tok_cap; sa.slot_h = m->d_in; }
    hipLaunchKernelGGL(sample_kernel, dim3(q.nb ? q.nb : 1), dim3(1024), 0, s, sa);
    if (q.nb) hipLaunchKernelGGL(lm1_advance_slots_kernel, dim3(1), dim3(64), 0, s, q.st, q.nb);
    else hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, s, q.st);
    ++(q.nb ? m->batch_steps : m->steps);
}

// a per-slot array grows (a request with a longer token budget than any before): the slots' contents move to the new pitch
void grow_slots(DevBuf& buf, size_t old_pitch, size_t new_pitch, int nb, hipStream_t s) {
    DevBuf fresh;
    fresh.ensure(new_pitch * nb);
    CV_HIP(hipMemsetAsync(fresh.p, 0, new_pitch * nb, s));
    for (int i = 0; i < nb && old_pitch; ++i)
        CV_HIP(hipMemcpyAsync(static_cast<char*>(fresh.p) + i * new_pitch, static_cast<char*>(buf.p) + i * old_pitch, old_pitch, hipMemcpyDeviceToDevice, s));
    CV_HIP(hipStreamSynchronize(s));
    std::swap(buf.p, fresh.p); std::swap(buf.bytes, fresh.bytes);
}

// the device block of a sequence over caller-made cache rows and tables (cv_lm1_bind / cv_lm1_batch_bind; `who`: the entry point's name)
// held_pos: the position of the request the slot holds, which the new cache must still cover (-1: none)
Lm1Dyn checked_dyn(const char* who, const cv_lm1* m, float* const* rows, const float* const* tabs, int n_tab, int cap, int held_pos = -1) {
    auto need = [&](bool ok, const char* what) { if (!ok) throw cv::Error(std::string(who) + ": " + what); };
    need(cap >= 1 && cap <= LM1_SPLITS * LM1_MAX_KEYS_PER_SPLIT, "a cache of up to 32768 positions");
    need(n_tab >= cap, "the relative-position tables must cover the cache (n_tab >= cap)");
    need(held_pos < cap, "the new cache ends before the slot's position");
    Lm1Dyn v{};
    v.n_tab = n_tab;
    for (int i = 0; i < m->n_layers; ++i) {
        need(rows[i] && tabs[i] && aligned16(rows[i]) && aligned16(tabs[i]), "cache / table buffers present and 16B aligned");
        v.rows[i] = rows[i]; v.tabs[i] = tabs[i];
    }
    return v;
}

// a request of the device loop (cv_lm1_decode_begin / cv_lm1_batch_open): its position and sampling parameters, checked (len_cap: the longest max_len the token
// array takes - a slot's holds max_tokens) ...
SampleParams checked_params(const char* who, const cv_lm1* m, int pos, int cap, const cv_sampling* sp, int max_tokens, int len_cap, const float* host_uniforms, int n_uniforms) {
    auto need = [&](bool ok, const char* what) { if (!ok) throw cv::Error(std::string(who) + ": " + what); };
    need(pos >= 0 && pos < cap && max_tokens >= 1, "position beyond the bound cache");
    need(m->n_out <= 8192, "the device sampler holds at most 8192 logits");                 // (a batch: cv_lm1_batch_begin has refused it already)
    need(sp->max_len > 0 && sp->max_len <= len_cap && sp->eos >= 0 && sp->eos + sp->n_stop <= m->n_out, "bad sampling parameters");
    need(sp->mode == 0 || (sp->top_k > 0 && sp->top_k <= 64 && sp->win_size >= 0), "bad RAS parameters");
    need(!sp->use_uniforms || (host_uniforms && n_uniforms >= 2), "use_uniforms needs the uniforms");
    return SampleParams{sp->mode, sp->eos, sp->n_stop, sp->min_len, sp->max_len, sp->top_p, sp->top_k, sp->win_size, sp->tau_r, sp->use_uniforms, (unsigned long long)sp->seed};
}
// ... and parked on the device: the loop state (returned), the parameters, the first input row and the injected uniforms, at the given addresses
DecodeState park_request(int pos, const SampleParams& hp, const float* x_row, int d_in, const float* host_uniforms, int n_uniforms, DecodeState* dst, SampleParams* dsp, float* dxin,
                         float* duniforms, hipStream_t s) {
    DecodeState st{}; st.pos = pos; st.stop_token = -1;
    CV_HIP(hipMemcpyAsync(dst, &st, sizeof(st), hipMemcpyHostToDevice, s));
    CV_HIP(hipMemcpyAsync(dsp, &hp, sizeof(hp), hipMemcpyHostToDevice, s));
    CV_HIP(hipMemcpyAsync(dxin, x_row, (size_t)d_in * 4, hipMemcpyDeviceToDevice, s));
    if (hp.use_uniforms) CV_HIP(hipMemcpyAsync(duniforms, host_uniforms, (size_t)std::min(n_uniforms, 2 * hp.max_len) * 4, hipMemcpyHostToDevice, s));
    return st;                                                  // (the copies read stack / caller memory: the caller synchronises before it returns)
}

}  // namespace

extern "C" {

cv_lm1* cv_lm1_create(const cv_lm1_config* c, const cv_lm1_layer_weights* layers) {
    cv_lm1* m = nullptr;
    int rc = guarded([&] {
        CV_CHECK(c && layers, "cv_lm1_create: null argument");
        CV_CHECK(c->n_layers >= 1 && c->n_layers <= LM1_MAX_LAYERS, "cv_lm1_create: 1..32 layers");
        CV_CHECK(c->d == c->heads * 64 && c->d <= 1024 && c->d % 4 == 0, "cv_lm1_create: 64-wide heads, model width up to 1024");
        CV_CHECK(c->ffn % 4 == 0 && c->ffn <= LM1_MAX_K && c->d_in % 4 == 0 && c->d_in <= LM1_MAX_K && c->n_out >= 1, "cv_lm1_create: widths");
        CV_CHECK(c->act == CV_ACT_RELU || c->act == CV_ACT_SILU || c->act == CV_ACT_NONE, "cv_lm1_create: activation");
        auto ok = [](const void* p) { return p && aligned16(p); };
        m = new cv_lm1();
        m->n_layers = c->n_layers; m->d = c->d; m->heads = c->heads; m->ffn = c->ffn; m->d_in = c->d_in; m->n_out = c->n_out; m->act = c->act; m->xscale = c->xscale;
        for (int i = 0; i < c->n_layers; ++i) {
            const cv_lm1_layer_weights& w = layers[i];
            CV_CHECK(ok(w.ln1_g) && ok(w.ln1_b) && ok(w.w_qkv) && ok(w.b_qkv) && ok(w.w_out) && ok(w.b_out) && ok(w.ln2_g) && ok(w.ln2_b) && ok(w.w1) && ok(w.b1) && ok(w.w2) && ok(w.b2),
                     "cv_lm1_create: every layer tensor present and 16B aligned");
            m->L.push_back(Lm1Layer{w.ln1_g, w.ln1_b, w.w_qkv, w.b_qkv, w.w_out, w.b_out, w.ln2_g, w.ln2_b, w.w1, w.b1, w.w2, w.b2});
        }
        CV_CHECK(ok(c->embed_w) && ok(c->embed_b) && ok(c->embed_g) && ok(c->embed_beta) && ok(c->after_g) && ok(c->after_b) && ok(c->dec_w) && ok(c->dec_b),
                 "cv_lm1_create: input layer / after_norm / decoder tensors present and 16B aligned");
        m->embed_w = c->embed_w; m->embed_b = c->embed_b; m->embed_g = c->embed_g; m->embed_beta = c->embed_beta;
        m->after_g = c->after_g; m->after_b = c->after_b; m->dec_w = c->dec_w; m->dec_b = c->dec_b;
        m->dyn.ensure(sizeof(Lm1Dyn)); m->x0.ensure((size_t)c->d * 4); m->x1.ensure((size_t)c->d * 4); m->h.ensure((size_t)c->d * 4);
        m->ff.ensure((size_t)c->ffn * 4); m->part.ensure((size_t)c->heads * LM1_SPLITS * 66 * 4);
        CV_HIP(hipMemset(m->dyn.p, 0, sizeof(Lm1Dyn)));
        if (const char* e = getenv("CV_LM1_GRAPH")) m->use_graph = atoi(e) != 0;
        if (const char* e = getenv("CV_LM1_WIDE16")) m->wide16 = atoi(e) != 0;
        if (const char* e = getenv("CV_LM1_WIDE")) m->wide32 = atoi(e) != 0;
        if (const char* e = getenv("CV_LM1_ROWS")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) m->rows32 = v; }         // A/B knobs (options "gemv_rows" / "gemv_rows16")
        if (const char* e = getenv("CV_LM1_ROWS16")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) m->rows16 = v; }
    });
    if (rc != 0) { delete m; return nullptr; }
    return m;
}

void cv_lm1_destroy(cv_lm1* m) { delete m; }

int cv_lm1_use_bf16(cv_lm1* m, const cv_lm1_layer_bf16* layers, const void* embed_w, const void* dec_w) {
    return guarded([&] {
        CV_CHECK(m, "cv_lm1_use_bf16: null handle");
        std::lock_guard<std::recursive_mutex> lk(runtime_lock());
        if (m->graph) { (void)hipGraphExecDestroy(m->graph); m->graph = nullptr; }       // a captured step holds the kernel choice and the matrix addresses
        if (!layers) { m->w16 = false; m->L16s.clear(); m->embed_w16 = m->dec_w16 = nullptr; return; }
        m->L16s.clear();
        for (int i = 0; i < m->n_layers; ++i) {
            const cv_lm1_layer_bf16& w = layers[i];
            CV_CHECK(w.w_qkv && w.w_out && w.w1 && w.w2 && aligned16(w.w_qkv) && aligned16(w.w_out) && aligned16(w.w1) && aligned16(w.w2), "cv_lm1_use_bf16: four 16B-aligned matrices per layer");
            cv_lm1::L16 h; h.w_qkv = w.w_qkv; h.w_out = w.w_out; h.w1 = w.w1; h.w2 = w.w2;
            m->L16s.push_back(h);
        }
        CV_CHECK((!embed_w || aligned16(embed_w)) && (!dec_w || aligned16(dec_w)), "cv_lm1_use_bf16: 16B-aligned matrices");
        m->embed_w16 = embed_w; m->dec_w16 = dec_w; m->w16 = true;
    });
}

int cv_lm1_bind(cv_lm1* m, float* const* rows, const float* const* tabs, int32_t n_tab, int32_t cap, void* stream) {
    return guarded([&] {
        CV_CHECK(m && rows && tabs, "cv_lm1_bind: null argument");
        const Lm1Dyn v = checked_dyn("cv_lm1_bind", m, rows, tabs, n_tab, cap);
        hipLaunchKernelGGL(lm1_bind_kernel, dim3(1), dim3(64), 0, resolve(m, stream), m->dyn.as<Lm1Dyn>(), v);
        m->cap = cap; m->bound = 1;
    });
}

int cv_lm1_step(cv_lm1* m, const float* x_row, int32_t pos, float* logits, void* stream) {
    return guarded([&] {
        CV_CHECK(m && x_row && logits && aligned16(x_row), "cv_lm1_step: null / unaligned argument");
        CV_CHECK(m->bound, "cv_lm1_step: cv_lm1_bind first");
        CV_CHECK(pos >= 0 && pos < m->cap, "cv_lm1_step: position beyond the bound cache");
        hipStream_t s = resolve(m, stream);
        const Lm1Seq q = seq_single(m);
        embed(m, q, x_row, pos, s);                             // the first kernel publishes the position the rest of the step reads
        ++m->steps;
        if (!m->use_graph) { walk(m, q, logits, s); return; }
        if (!m->graph || m->graph_logits != logits || m->graph_stream != s) {
            std::lock_guard<std::recursive_mutex> lk(runtime_lock());
            if (m->graph) { (void)hipGraphExecDestroy(m->graph); m->graph = nullptr; }
            hipGraph_t g = capture_graph(s, [&] { walk(m, q, logits, s); });
            hipError_t e = hipGraphInstantiate(&m->graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) { m->graph = nullptr; CV_HIP(e); }
            m->graph_logits = logits; m->graph_stream = s;
        }
        { std::lock_guard<std::recursive_mutex> lk(runtime_lock()); CV_HIP(hipGraphLaunch(m->graph, s)); }
        ++m->graph_replays;
    });
}

// ---- the decode loop on the device (round 5; reference: the python loop of TransformerLM.inference, llm/llm.py:196-223, one host round trip per token) ------------------
// cv_lm1_decode_begin parks the first input row, the position of the row it will write and the request's sampling parameters on the device; every step of
// cv_lm1_decode is then [input Linear on the parked row, publishing the position] [the 72 launches of cv_lm1_step] [sample_kernel: arg-max or repetition-aware
// sampling on the logits, eos masked below min_len, the sampled token's speech_embedding row parked as the next input] [advance]: no logits, no token and no embedding
// row cross the host boundary per step.  Tokens come back once per call (n_steps steps), like cv_llm_decode.
int cv_lm1_decode_begin(cv_lm1* m, const float* x_row, int32_t pos, const cv_sampling* sp, const float* emb_table, int32_t max_tokens, const float* host_uniforms, int32_t n_uniforms,
                        void* stream) {
    return guarded([&] {
        CV_CHECK(m && x_row && sp && emb_table && aligned16(x_row) && aligned16(emb_table), "cv_lm1_decode_begin: null / unaligned argument");
        CV_CHECK(m->bound, "cv_lm1_decode_begin: cv_lm1_bind first");
        const SampleParams hp = checked_params("cv_lm1_decode_begin", m, pos, m->cap, sp, max_tokens, INT_MAX, host_uniforms, n_uniforms);
        hipStream_t s = resolve(m, stream);
        m->dstate.ensure(sizeof(DecodeState)); m->dsp.ensure(sizeof(SampleParams)); m->dtokens.ensure((size_t)max_tokens * 4); m->xin.ensure((size_t)m->d_in * 4);
        m->dlogits.ensure((size_t)m->n_out * 4);
        m->max_tokens = max_tokens; m->emb_table = emb_table; m->host_tokens.assign(max_tokens, 0);
        if (sp->use_uniforms) m->duniforms.ensure((size_t)2 * sp->max_len * 4);
        m->host_state = park_request(pos, hp, x_row, m->d_in, host_uniforms, n_uniforms, m->dstate.as<DecodeState>(), m->dsp.as<SampleParams>(), m->xin.as<float>(),
                                     m->duniforms.as<float>(), s);
        CV_HIP(hipStreamSynchronize(s));
        m->loop_open = 1;
    });
}

int cv_lm1_decode(cv_lm1* m, int32_t n_steps, int32_t* out_tokens, int32_t* n_out, int32_t* finished, void* stream) {
    return guarded([&] {
        CV_CHECK(m && out_tokens && n_out && finished && n_steps > 0, "cv_lm1_decode: bad arguments");
        CV_CHECK(m->loop_open, "cv_lm1_decode: cv_lm1_decode_begin first");
        CV_CHECK(m->host_state.done || m->host_state.pos + n_steps <= m->cap, "cv_lm1_decode: the bound cache ends before these steps do");
        hipStream_t s = resolve(m, stream);
        const int before = m->host_state.n_tokens;
        const Lm1Seq q = seq_single(m);
        const Lm1Loop l = loop_single(m);
        for (int i = 0; i < n_steps; ++i) decode_step(m, q, l, s);
        CV_HIP(hipMemcpyAsync(&m->host_state, q.st, sizeof(DecodeState), hipMemcpyDeviceToHost, s));
        CV_HIP(hipMemcpyAsync(m->host_tokens.data(), m->dtokens.p, (size_t)m->max_tokens * 4, hipMemcpyDeviceToHost, s));
        CV_HIP(hipStreamSynchronize(s));
        CV_HIP(hipGetLastError());
        const int after = std::min(m->host_state.n_tokens, m->max_tokens);
        *n_out = std::max(0, after - before);
        for (int k = 0; k < *n_out; ++k) out_tokens[k] = m->host_tokens[before + k];
        *finished = m->host_state.done ? 1 : 0;
    });
}

// ---- lock-step batched decode (no counterpart in the reference: TransformerLM.inference, llm/llm.py:162-223, is batch-1; the Qwen2 path's cv_llm_batch_* is the model) ----
// Up to LM1_MAX_SLOTS requests advance one token per step and every matrix of the step is streamed once for all of them; a slot's tokens, logits and cache rows are
// those of cv_lm1_decode on that request alone.  Slots are bound (cache rows, tables), opened (first input row, position, sampling parameters) and released one by
// one, also between two cv_lm1_batch_decode calls - that is how a finished request's slot takes the next request.
int cv_lm1_batch_begin(cv_lm1* m, int32_t nb, void* stream) {
    return guarded([&] {
        CV_CHECK(m, "cv_lm1_batch_begin: null handle");
        CV_CHECK(nb >= 1 && nb <= LM1_MAX_SLOTS, "cv_lm1_batch_begin: 1..8 slots");
        CV_CHECK(m->n_out <= 8192, "cv_lm1_batch_begin: the device sampler holds at most 8192 logits");
        hipStream_t s = resolve(m, stream);
        cv_lm1::Batch& B = m->batch;
        CV_HIP(hipStreamSynchronize(s));
        const size_t n = (size_t)nb;
        B.dyns.ensure(n * sizeof(Lm1Dyn)); B.sts.ensure(n * sizeof(DecodeState)); B.sps.ensure(n * sizeof(SampleParams));
        B.xin.ensure(n * m->d_in * 4); B.logits.ensure(n * m->n_out * 4); B.x0.ensure(n * m->d * 4); B.x1.ensure(n * m->d * 4); B.h.ensure(n * m->d * 4);
        B.ff.ensure(n * m->ffn * 4); B.part.ensure(n * m->heads * LM1_SPLITS * 66 * 4);
        if (B.nb != nb) { B.tok_cap = 0; B.uni_cap = 0; }       // (the per-slot pitches belong to a slot count)
        B.nb = nb; B.emb_table = nullptr; B.stream = s;
        B.host_states.assign(n, DecodeState{});
        for (int i = 0; i < LM1_MAX_SLOTS; ++i) B.slots[i] = cv_lm1::Slot{};
        std::vector<DecodeState> st(n);
        for (auto& e : st) { e = DecodeState{}; e.done = 1; e.stop_token = -1; }
        CV_HIP(hipMemsetAsync(B.dyns.p, 0, n * sizeof(Lm1Dyn), s));
        CV_HIP(hipMemsetAsync(B.sps.p, 0, n * sizeof(SampleParams), s));
        CV_HIP(hipMemsetAsync(B.logits.p, 0, n * m->n_out * 4, s));
        CV_HIP(hipMemcpyAsync(B.sts.p, st.data(), n * sizeof(DecodeState), hipMemcpyHostToDevice, s));
        CV_HIP(hipStreamSynchronize(s));
    });
}

int cv_lm1_batch_bind(cv_lm1* m, int32_t slot, float* const* rows, const float* const* tabs, int32_t n_tab, int32_t cap, void* stream) {
    return guarded([&] {
        CV_CHECK(m && rows && tabs, "cv_lm1_batch_bind: null argument");
        CV_CHECK(m->batch.nb > 0, "cv_lm1_batch_bind: cv_lm1_batch_begin first");
        CV_CHECK(slot >= 0 && slot < m->batch.nb, "cv_lm1_batch_bind: slot out of range");
        cv_lm1::Slot& S = m->batch.slots[slot];
        const Lm1Dyn v = checked_dyn("cv_lm1_batch_bind", m, rows, tabs, n_tab, cap, S.open && !S.host.done ? S.host.pos : -1);
        hipStream_t s = resolve(m, stream);
        Lm1Dyn* dslot = m->batch.dyns.as<Lm1Dyn>() + slot;
        hipLaunchKernelGGL(lm1_bind_slot_kernel, dim3(1), dim3(64), 0, s, dslot, v);
        S.cap = cap; S.bound = 1; m->batch.stream = s;
    });
}

int cv_lm1_batch_open(cv_lm1* m, int32_t slot, const float* x_row, int32_t pos, const cv_sampling* sp, const float* emb_table, int32_t max_tokens, const float* host_uniforms,
                      int32_t n_uniforms, void* stream) {
    return guarded([&] {
        CV_CHECK(m && x_row && sp && emb_table && aligned16(x_row) && aligned16(emb_table), "cv_lm1_batch_open: null / unaligned argument");
        cv_lm1::Batch& B = m->batch;
        CV_CHECK(B.nb > 0, "cv_lm1_batch_open: cv_lm1_batch_begin first");
        CV_CHECK(slot >= 0 && slot < B.nb, "cv_lm1_batch_open: slot out of range");
        cv_lm1::Slot& S = B.slots[slot];
        CV_CHECK(S.bound, "cv_lm1_batch_open: cv_lm1_batch_bind first");
        CV_CHECK(!S.open, "cv_lm1_batch_open: the slot holds a request (cv_lm1_batch_release first)");
        const SampleParams hp = checked_params("cv_lm1_batch_open", m, pos, S.cap, sp, max_tokens, max_tokens, host_uniforms, n_uniforms);
        bool others = false;
        for (int i = 0; i < B.nb; ++i) others = others || B.slots[i].open;
        CV_CHECK(!others || B.emb_table == emb_table, "cv_lm1_batch_open: the slots of a batch share one embedding table");
        hipStream_t s = resolve(m, stream);
        if (max_tokens > B.tok_cap) { const int cap = std::max(max_tokens, 2 * B.tok_cap); grow_slots(B.tokens, (size_t)B.tok_cap * 4, (size_t)cap * 4, B.nb, s); B.tok_cap = cap; }
        if (sp->use_uniforms && 2 * sp->max_len > B.uni_cap) {
            const int cap = std::max(2 * sp->max_len, 2 * B.uni_cap); grow_slots(B.uniforms, (size_t)B.uni_cap * 4, (size_t)cap * 4, B.nb, s); B.uni_cap = cap;
        }
        B.host_tokens.resize((size_t)B.nb * B.tok_cap);
        Lm1Dyn* dslot = B.dyns.as<Lm1Dyn>() + slot; DecodeState* sslot = B.sts.as<DecodeState>() + slot;      // (plain values for the launch: a launch captures its arguments by value)
        const DecodeState st = park_request(pos, hp, x_row, m->d_in, host_uniforms, n_uniforms, sslot, B.sps.as<SampleParams>() + slot, B.xin.as<float>() + (size_t)slot * m->d_in,
                                            B.uniforms.as<float>() + (size_t)slot * B.uni_cap, s);
        hipLaunchKernelGGL(lm1_slot_flag_kernel, dim3(1), dim3(64), 0, s, dslot, sslot, 1);
        CV_HIP(hipStreamSynchronize(s));                        // the host copies above are stack / caller memory
        S.open = 1; S.returned = 0; S.host = st; B.host_states[slot] = st; B.emb_table = emb_table; B.stream = s;
    });
}

int cv_lm1_batch_decode(cv_lm1* m, int32_t n_steps, int32_t* out_tokens, int32_t* n_out, int32_t* finished, void* stream) {
    return guarded([&] {
        CV_CHECK(m && out_tokens && n_out && finished && n_steps > 0, "cv_lm1_batch_decode: bad arguments");
        cv_lm1::Batch& B = m->batch;
        CV_CHECK(B.nb > 0, "cv_lm1_batch_decode: cv_lm1_batch_begin first");
        bool any = false;
        for (int i = 0; i < B.nb; ++i) {
            const cv_lm1::Slot& S = B.slots[i];
            any = any || S.open;
            CV_CHECK(!S.open || S.host.done || S.host.pos + n_steps <= S.cap, "cv_lm1_batch_decode: a slot's bound cache ends before these steps do");
        }
        CV_CHECK(any, "cv_lm1_batch_decode: no open slot (cv_lm1_batch_open first)");
        hipStream_t s = resolve(m, stream);
        B.stream = s;
        const Lm1Seq q = seq_batch(m);
        const Lm1Loop l = loop_batch(m);
        for (int i = 0; i < n_steps; ++i) decode_step(m, q, l, s);
        CV_HIP(hipMemcpyAsync(B.host_states.data(), B.sts.p, (size_t)B.nb * sizeof(DecodeState), hipMemcpyDeviceToHost, s));
        CV_HIP(hipMemcpyAsync(B.host_tokens.data(), B.tokens.p, (size_t)B.nb * B.tok_cap * 4, hipMemcpyDeviceToHost, s));
        CV_HIP(hipStreamSynchronize(s));
        CV_HIP(hipGetLastError());
        for (int i = 0; i < B.nb; ++i) {
            cv_lm1::Slot& S = B.slots[i];
            if (!S.open) { n_out[i] = 0; finished[i] = 1; continue; }
            S.host = B.host_states[i];
            const int after = std::min(S.host.n_tokens, B.tok_cap);
            n_out[i] = std::max(0, std::min(after - S.returned, (int)n_steps));
            for (int k = 0; k < n_out[i]; ++k) out_tokens[(size_t)i * n_steps + k] = B.host_tokens[(size_t)i * B.tok_cap + S.returned + k];
            S.returned += n_out[i];
            finished[i] = S.host.done ? 1 : 0;
        }
    });
}

int cv_lm1_batch_release(cv_lm1* m, int32_t slot) {
    return guarded([&] {
        CV_CHECK(m, "cv_lm1_batch_release: null handle");
        cv_lm1::Batch& B = m->batch;
        CV_CHECK(B.nb > 0, "cv_lm1_batch_release: cv_lm1_batch_begin first");
        CV_CHECK(slot >= 0 && slot < B.nb, "cv_lm1_batch_release: slot out of range");
        hipStream_t s = B.stream ? B.stream : resolve(m, nullptr);
        Lm1Dyn* dslot = B.dyns.as<Lm1Dyn>() + slot; DecodeState* sslot = B.sts.as<DecodeState>() + slot;
        hipLaunchKernelGGL(lm1_slot_flag_kernel, dim3(1), dim3(64), 0, s, dslot, sslot, 0);
        CV_HIP(hipStreamSynchronize(s));                        // the caller may free the slot's cache rows when this returns
        B.slots[slot] = cv_lm1::Slot{};
    });
}

int cv_lm1_batch_logits(cv_lm1* m, int32_t slot, float* host_out, void* stream) {
    return guarded([&] {
        CV_CHECK(m && host_out, "cv_lm1_batch_logits: null argument");
        CV_CHECK(m->batch.nb > 0, "cv_lm1_batch_logits: cv_lm1_batch_begin first");
        CV_CHECK(slot >= 0 && slot < m->batch.nb, "cv_lm1_batch_logits: slot out of range");
        CV_CHECK(m->batch.slots[slot].open, "cv_lm1_batch_logits: the slot holds no request");
        hipStream_t s = resolve(m, stream);
        CV_HIP(hipMemcpyAsync(host_out, m->batch.logits.as<float>() + (size_t)slot * m->n_out, (size_t)m->n_out * 4, hipMemcpyDeviceToHost, s));
        CV_HIP(hipStreamSynchronize(s));
    });
}

// ---- test entry points of the decode kernels (tests/test_zzz_cosyvoice1_hip_kernels.py): the production launch helpers on caller-made operands -----------------------
int cv_lm1_attention(int32_t nb, const float* const* rows, const float* const* tabs, const int32_t* n_tab, const int32_t* pos, int32_t d, int32_t heads, float scale, float* part,
                     void* stream) {
    return guarded([&] {
        CV_CHECK(rows && tabs && n_tab && pos && part, "cv_lm1_attention: null argument");
        CV_CHECK(nb >= 0 && nb <= LM1_MAX_SLOTS, "cv_lm1_attention: nb is 0 (the single-sequence launch) or 1..8 slots");
        CV_CHECK(heads >= 1 && d == 64 * heads && d <= 1024, "cv_lm1_attention: 64-wide heads, model width up to 1024");
        CV_CHECK(std::isfinite(scale) && scale > 0.f, "cv_lm1_attention: bad scale (finite and positive)");
        CV_CHECK((reinterpret_cast<uintptr_t>(part) & 3) == 0, "cv_lm1_attention: unaligned part");
        const int n = nb > 0 ? nb : 1;
        std::vector<Lm1Dyn> h((size_t)n, Lm1Dyn{});
        for (int i = 0; i < n; ++i) {
            if (nb > 0 && pos[i] < 0) continue;                 // an inactive slot: flag clear, nothing of it is read
            CV_CHECK(pos[i] >= 0 && pos[i] < LM1_SPLITS * LM1_MAX_KEYS_PER_SPLIT, "cv_lm1_attention: a position of up to 32767");
            CV_CHECK(n_tab[i] >= pos[i] + 1, "cv_lm1_attention: the relative-position table must cover the keys (n_tab >= pos + 1)");
            CV_CHECK(rows[i] && tabs[i] && aligned16(rows[i]) && aligned16(tabs[i]), "cv_lm1_attention: cache / table buffers of an active slot present and 16B aligned");
            h[i].pos = pos[i]; h[i].n_tab = n_tab[i]; h[i].pad0 = 1;
            h[i].rows[0] = const_cast<float*>(rows[i]); h[i].tabs[0] = tabs[i];
        }
        hipStream_t s = as_stream(stream);
        DevBuf dyn;
        dyn.ensure(h.size() * sizeof(Lm1Dyn));
        CV_HIP(hipMemcpyAsync(dyn.p, h.data(), h.size() * sizeof(Lm1Dyn), hipMemcpyHostToDevice, s));
        launch_attn(dyn.as<Lm1Dyn>(), 0, d, heads, scale, part, nb, s);
        CV_HIP(hipStreamSynchronize(s));                        // the device block is this call's own
        CV_HIP(hipGetLastError());
    });
}

namespace {
// what both GEMV hooks refuse (gemv() itself checks K); `who` is the hook's name
void check_gemv_hook(const char* who, cv_lm1* m, int pro, const float* x, const float* g, const float* b, float eps, const float* W, const void* W16, const float* bias,
                     const float* res, const float* y, int N, int K, int act) {
    auto fail = [&](const char* what) { throw cv::Error(std::string(who) + ": " + what); };
    if (!m) fail("null handle");
    if (pro != LM1_PRO_NONE && pro != LM1_PRO_LN && pro != LM1_PRO_MERGE) fail("bad prologue (0 none, 1 LayerNorm, 2 merge)");
    if (!x || !y || !aligned16(x) || (reinterpret_cast<uintptr_t>(y) & 3) != 0) fail("null / unaligned x or y");
    if ((W == nullptr) == (W16 == nullptr)) fail("exactly one of W (fp32) and W16 (bf16)");
    if (!aligned16(W) || !aligned16(W16)) fail("unaligned matrix");
    if (W16 && !m->w16) fail("W16 needs a handle in bf16 mode (cv_lm1_use_bf16)");
    if (N < 1 || K < 4 || K % 4 != 0 || K > LM1_MAX_K) fail("bad shape (N >= 1, K % 4 == 0, 4 <= K <= 4096)");
    if (pro == LM1_PRO_LN && (K > 1024 || !g || !b || !aligned16(g) || !aligned16(b) || !(std::isfinite(eps) && eps >= 0.f)))
        fail("the LayerNorm prologue takes K <= 1024, 16B-aligned gamma / beta and a finite eps >= 0");
    if (pro == LM1_PRO_MERGE && (K % 64 != 0 || K > 1024)) fail("the merge prologue takes K = 64 heads <= 1024");
    if (act != ACT_NONE && act != ACT_RELU && act != ACT_SILU) fail("bad activation (none, relu, silu)");
    if ((reinterpret_cast<uintptr_t>(bias) & 3) != 0 || (reinterpret_cast<uintptr_t>(res) & 3) != 0) fail("unaligned bias / res");
}
}  // namespace

int cv_lm1_gemv(cv_lm1* m, int32_t pro, const float* x, const float* g, const float* b, float eps, const float* W, const void* W16, const float* bias, const float* res, float* y,
                int32_t N, int32_t K, int32_t act, void* stream) {
    return guarded([&] {
        check_gemv_hook("cv_lm1_gemv", m, pro, x, g, b, eps, W, W16, bias, res, y, N, K, act);
        gemv(m, seq_single(m), pro, x, 0, g, b, eps, W, W16, bias, res, 0, y, 0, -1, -1, N, K, act, resolve(m, stream));
    });
}

int cv_lm1_gemv_batch(cv_lm1* m, int32_t nb, uint32_t active_mask, int32_t pro, const float* x, int64_t sx, const float* g, const float* b, float eps, const float* W,
                      const void* W16, const float* bias, const float* res, int64_t sres, float* y, int64_t sy, int32_t N, int32_t K, int32_t act, void* stream) {
    return guarded([&] {
        check_gemv_hook("cv_lm1_gemv_batch", m, pro, x, g, b, eps, W, W16, bias, res, y, N, K, act);
        cv_lm1::Batch& B = m->batch;
        CV_CHECK(nb >= 1 && nb <= LM1_MAX_SLOTS && B.nb == nb, "cv_lm1_gemv_batch: cv_lm1_batch_begin with these nb slots (1..8) first");
        CV_CHECK((active_mask >> nb) == 0, "cv_lm1_gemv_batch: a mask bit beyond the slots");
        CV_CHECK(sx >= 0 && sx % 4 == 0 && sres >= 0 && sy >= 0, "cv_lm1_gemv_batch: bad slot strides (sx a multiple of 4 floats, none negative)");
        for (int i = 0; i < nb; ++i) CV_CHECK(!B.slots[i].open, "cv_lm1_gemv_batch: the handle has an open slot");
        hipStream_t s = resolve(m, stream);
        auto flags = [&](uint32_t mask) {
            for (int i = 0; i < nb; ++i) {
                Lm1Dyn* dslot = B.dyns.as<Lm1Dyn>() + i; DecodeState* sslot = B.sts.as<DecodeState>() + i;
                hipLaunchKernelGGL(lm1_slot_flag_kernel, dim3(1), dim3(64), 0, s, dslot, sslot, (int)((mask >> i) & 1u));
            }
        };
        flags(active_mask);
        try { gemv(m, seq_batch(m), pro, x, sx, g, b, eps, W, W16, bias, res, sres, y, sy, -1, -1, N, K, act, s); }
        catch (...) { flags(0); throw; }
        flags(0);
    });
}

int64_t cv_lm1_stat(const cv_lm1* m, const char* name) {
    if (!m || !name) return -1;
    const std::string n(name);
    if (n == "steps") return m->steps;
    if (n == "graph_replays") return m->graph_replays;
    if (n == "batch_steps") return m->batch_steps;
    if (n == "launches_per_step") return 3 + 5LL * m->n_layers;
    return -1;
}

int cv_lm1_set_option(cv_lm1* m, const char* name, int32_t value) {
    return guarded([&] {
        CV_CHECK(m && name, "cv_lm1_set_option: null argument");
        const std::string n(name);
        if (n == "graph") m->use_graph = value != 0;
        else if (n == "gemv16_wide" || n == "gemv_wide") {
            std::lock_guard<std::recursive_mutex> lk(runtime_lock());
            if (m->graph) { (void)hipGraphExecDestroy(m->graph); m->graph = nullptr; }
            (n == "gemv_wide" ? m->wide32 : m->wide16) = value != 0;
        }
        else if (n == "gemv_rows" || n == "gemv_rows16") {
            CV_CHECK(value == 1 || value == 2 || value == 4, "cv_lm1_set_option: gemv_rows must be 1, 2 or 4");
            std::lock_guard<std::recursive_mutex> lk(runtime_lock());
            if (m->graph) { (void)hipGraphExecDestroy(m->graph); m->graph = nullptr; }
            (n == "gemv_rows" ? m->rows32 : m->rows16) = value;
        }
        else CV_CHECK(false, "cv_lm1_set_option: unknown option");
    });
}

}  // extern "C"
