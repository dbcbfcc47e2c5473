// rr_ce_w.hip -- K5 at encoder shapes other than hidden 384 / 12 heads / FFN 1536 (BERT-base 768 / 12 / 3072, bge-large
// 1024 / 16 / 4096, TinyBERT 128 / 2 / 512, ...): the small kernels of the wide-range fp32 forward (rr_ce.hip, ce_forward_x3)
// at a RUNTIME width, and its split-operand attention at head dim 32 or 64.  The four GEMMs of a layer are ce_gemm_x3 itself
// (runtime M, N, K); ce_forward_w in rr_ce.hip composes the launches.  RR_CE_PRECISION_F32 only: every product carries its
// operands as three bf16 terms, six matrix-core products, fp32 accumulation -- any fp32 range, no flag.
//
//   ce_embed_ln_w<NV>      word + position + type embedding, LayerNorm; one wave per token, NV = hidden / 64 values per lane
//   ce_add_ln_w<NV>        residual + LayerNorm, the same shape; both in the reduction order of their 384-wide siblings
//                          (lane + 64 i, then ce_w_wave_sum): at hidden 384 they return ce_embed_ln's / ce_add_ln_f32's bits
//   ce_attention_x3w<HD>   softmax(Q K^T / sqrt(HD)) V of one (sequence, head); HD 32 is ce_attention_x3 operation for operation
//                          (its bits), HD 64 the same scheme with four k-steps per score tile and two 32-row blocks of O^T
//   ce_head_w              [CLS] gather; tanh(pooler) + classifier
#include <cmath>
#include <vector>

#include "rr_common.h"
#include "rr_ce_w.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x16r __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float ce_w_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ------------------------------------------------------------------ embeddings + LayerNorm, residual + LayerNorm
// Two-pass statistics, eps under the square root.  `inv_h` = 1.f / hidden from the host (the constant of the 384 kernels).
template <int NV>
__global__ __launch_bounds__(256) void ce_embed_ln_w(const int32_t* __restrict__ tok, const int32_t* __restrict__ typ,
                                                     const int32_t* __restrict__ pos, int T, int vocab, int n_pos, int n_typ,
                                                     const float* __restrict__ we, const float* __restrict__ pe,
                                                     const float* __restrict__ te, const float* __restrict__ g,
                                                     const float* __restrict__ b, float eps, float inv_h, float* __restrict__ h32) {
    constexpr int H = 64 * NV;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    int id = tok[t], ty = typ[t], po = pos[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);          // ids are validated on the host; stay in bounds anyway
    ty = ty < 0 ? 0 : (ty >= n_typ ? n_typ - 1 : ty);
    po = po < 0 ? 0 : (po >= n_pos ? n_pos - 1 : po);
    float x[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        x[i] = (we[(int64_t)id * H + c] + te[(int64_t)ty * H + c]) + pe[(int64_t)po * H + c];
        s += x[i];
    }
    const float mean = ce_w_wave_sum(s) * inv_h;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { const float d = x[i] - mean; v += d * d; }
    const float rstd = rsqrtf(ce_w_wave_sum(v) * inv_h + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        h32[(int64_t)t * H + c] = (x[i] - mean) * rstd * g[c] + b[c];
    }
}

// `parts` > 1: y is that many [T][H] partial products, `pstride` floats apart (FFN-2 summed over K in chunks, see
// ce_forward_w): x = ((y0 + y1) + ...) + h32.  One part: x = y + h32, ce_add_ln_f32's first operation.
template <int NV>
__global__ __launch_bounds__(256) void ce_add_ln_w(const float* __restrict__ y, int parts, int64_t pstride, float* __restrict__ h32, int T,
                                                   const float* __restrict__ g, const float* __restrict__ b, float eps, float inv_h) {
    constexpr int H = 64 * NV;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    float x[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        float yv = y[(int64_t)t * H + c];
        for (int p = 1; p < parts; ++p) yv += y[p * pstride + (int64_t)t * H + c];
        x[i] = yv + h32[(int64_t)t * H + c];
        s += x[i];
    }
    const float mean = ce_w_wave_sum(s) * inv_h;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { const float d = x[i] - mean; v += d * d; }
    const float rstd = 1.0f / sqrtf(ce_w_wave_sum(v) * inv_h + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        h32[(int64_t)t * H + c] = (x[i] - mean) * rstd * g[c] + b[c];
    }
}

// ------------------------------------------------------------------ split-operand attention at head dim 32 / 64
// The scheme of ce_attention_x3 (rr_ce.hip): K, V, Q and the probabilities P as three bf16 terms, six
// v_mfma_f32_32x32x16_bf16 per k-step with the smallest terms first, a base-2 online softmax in fp32 registers, V^T stored
// with bits 2 and 3 of the key swapped inside a 32-key tile so that the score accumulator IS the B operand of O^T += V^T P^T.
// Workgroup = one (sequence, head), 8 waves, wave w owns query tiles w and w + 8.  What the head dim changes:
//   * S^T = K Q^T takes HD / 16 k-steps; O^T has HD / 32 blocks of 32 dims per query tile;
//   * the key chunk: 256 keys at HD 32 (112 128 B of LDS, what ce_attention_x3 takes), 128 keys at HD 64
//     (3 * 128 * 72 * 2 + 3 * 64 * 136 * 2 = 107 520 B; 256 keys would need 211 968 B of a CU's 160 KiB).
// The row stride 3 * hidden and the head count (grid y) are runtime values; `scale` = 1 / sqrt(HD) from the host.
template <int HD> struct ce_w_att {
    static constexpr int KC = HD == 32 ? 256 : 128;           // keys per LDS chunk
    static constexpr int KLD = HD + 8;                        // bf16 per K row
    static constexpr int VLD = KC + 8;                        // bf16 per V^T row
    static constexpr int LDS = (3 * KC * KLD + 3 * HD * VLD) * 2;
};
struct ce_w_bf16x3 { __bf16 hi, mid, lo; };
__device__ __forceinline__ ce_w_bf16x3 ce_w_split3(float x) {
    ce_w_bf16x3 r;
    r.hi = (__bf16)x;
    const float r1 = x - (float)r.hi;
    r.mid = (__bf16)r1;
    r.lo = (__bf16)(r1 - (float)r.mid);
    return r;
}

template <int HD>
__global__ __launch_bounds__(512, 2) void ce_attention_x3w(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                           float* __restrict__ ctx, float scale, int hidden) {
    constexpr int KC = ce_w_att<HD>::KC, KLD = ce_w_att<HD>::KLD, VLD = ce_w_att<HD>::VLD;
    constexpr int KS = HD / 16, DB = HD / 32, C4 = HD / 4;    // k-steps of S^T, 32-dim blocks of O^T, 4-dim groups of a row
    extern __shared__ __attribute__((aligned(16))) unsigned short x3w_lds[];
    unsigned short* Kt = x3w_lds;                                          // [3][KC][KLD]
    unsigned short* Vt = x3w_lds + 3 * KC * KLD;                           // [3][HD][VLD]
    const int seq = blockIdx.x, head = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = cu[seq], S = cu[seq + 1] - t0;
    const int c = lane & 31, h = lane >> 5;
    const int64_t ld = 3 * (int64_t)hidden;
    const float scale2 = scale * 1.4426950408889634f;        // the softmax in base 2
    constexpr int NT = 2;                                     // query tiles per wave: w and w + 8
    f32x16r o[NT][DB];
    float mx[NT], l[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        mx[t] = -INFINITY;
        l[t] = 0.f;
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[t][d][e] = 0.f;
    }
    for (int k0 = 0; k0 < S; k0 += KC) {
        const int kn = S - k0 < KC ? S - k0 : KC;             // keys of this chunk
        const int knp = (kn + 31) & ~31;
        __syncthreads();                                      // the previous chunk has been read
        // ---- K: thread -> (key, 4 dims): three 8-byte stores
        for (int i = tid; i < knp * C4; i += 512) {
            const int j = i / C4, c4 = i % C4;
            f32x4 k4 = {0.f, 0.f, 0.f, 0.f};
            if (j < kn) k4 = *reinterpret_cast<const f32x4*>(qkv + (int64_t)(t0 + k0 + j) * ld + hidden + head * HD + 4 * c4);
            __bf16 t3[3][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const ce_w_bf16x3 x3 = ce_w_split3(k4[e]);
                t3[0][e] = x3.hi; t3[1][e] = x3.mid; t3[2][e] = x3.lo;
            }
#pragma unroll
            for (int t = 0; t < 3; ++t)
                *reinterpret_cast<bf16x4*>(Kt + (t * KC + j) * KLD + 4 * c4) = bf16x4{t3[t][0], t3[t][1], t3[t][2], t3[t][3]};
        }
        // ---- V^T: thread -> (key pair 2 m, 2 m + 1; 4 dims): per dim and term one 4-byte store at the pair's slot
        for (int i = tid; i < (knp >> 1) * C4; i += 512) {
            const int m = i / C4, c4 = i % C4;
            const int j = 2 * m;
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
            if (j < kn) va = *reinterpret_cast<const f32x4*>(qkv + (int64_t)(t0 + k0 + j) * ld + 2 * hidden + head * HD + 4 * c4);
            if (j + 1 < kn) vb = *reinterpret_cast<const f32x4*>(qkv + (int64_t)(t0 + k0 + j + 1) * ld + 2 * hidden + head * HD + 4 * c4);
            // slot of key j inside its 32-key tile: bits 2 and 3 swapped
            const int in = j & 31;
            const int slot = (j & ~31) + (in & 0x13) + ((in & 4) << 1) + ((in & 8) >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const ce_w_bf16x3 xa = ce_w_split3(va[e]), xb = ce_w_split3(vb[e]);
                const __bf16 a3[3] = {xa.hi, xa.mid, xa.lo}, b3[3] = {xb.hi, xb.mid, xb.lo};
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    *reinterpret_cast<bf16x2v*>(Vt + (t * HD + 4 * c4 + e) * VLD + slot) = bf16x2v{a3[t], b3[t]};
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int q0 = 32 * (wave + 8 * t);
            if (q0 >= S) continue;                            // (wave-uniform)
            int qrow = q0 + c;
            qrow = qrow < S ? qrow : S - 1;                   // (lanes past the sequence: a valid row, never stored)
            // ---- Q terms of this tile: lane (query c, h), k-step s: dims 16 s + 8 h .. + 7
            bf16x8 qb[3][KS];
            {
                const float* qp = qkv + (int64_t)(t0 + qrow) * ld + head * HD + 8 * h;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const f32x4 q0v = *reinterpret_cast<const f32x4*>(qp + 16 * ks), q1v = *reinterpret_cast<const f32x4*>(qp + 16 * ks + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const ce_w_bf16x3 x0 = ce_w_split3(q0v[e]), x1 = ce_w_split3(q1v[e]);
                        qb[0][ks][e] = x0.hi; qb[1][ks][e] = x0.mid; qb[2][ks][e] = x0.lo;
                        qb[0][ks][4 + e] = x1.hi; qb[1][ks][4 + e] = x1.mid; qb[2][ks][4 + e] = x1.lo;
                    }
                }
            }
            for (int j0 = 0; j0 < knp; j0 += 32) {
                // ---- S^T = K Q^T (smallest terms first)
                f32x16r sT;
#pragma unroll
                for (int e = 0; e < 16; ++e) sT[e] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    bf16x8 ka[3];
#pragma unroll
                    for (int tt = 0; tt < 3; ++tt)
                        ka[tt] = *reinterpret_cast<const bf16x8*>(Kt + (tt * KC + j0 + c) * KLD + 16 * ks + 8 * h);
                    sT = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[2], qb[0][ks], sT, 0, 0, 0);
                    sT = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[0], qb[2][ks], sT, 0, 0, 0);
                    sT = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[1], qb[1][ks], sT, 0, 0, 0);
                    sT = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[1], qb[0][ks], sT, 0, 0, 0);
                    sT = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[0], qb[1][ks], sT, 0, 0, 0);
                    sT = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[0], qb[0][ks], sT, 0, 0, 0);
                }
                float cm = -INFINITY;
                if (k0 + j0 + 32 > S) {                       // only the sequence's last tile holds padding keys
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int key = k0 + j0 + 8 * (e >> 2) + 4 * h + (e & 3);
                        sT[e] = key < S ? sT[e] * scale2 : -INFINITY;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) sT[e] *= scale2;
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) cm = fmaxf(cm, sT[e]);
                cm = fmaxf(cm, __shfl_xor(cm, 32, 64));       // the query's other 16 keys of this tile
                if (cm > mx[t]) {                             // (per lane: a query's two lanes decide alike)
                    const float r = __builtin_amdgcn_exp2f(mx[t] - cm);
                    l[t] *= r;
#pragma unroll
                    for (int d = 0; d < DB; ++d)
#pragma unroll
                        for (int e = 0; e < 16; ++e) o[t][d][e] *= r;
                    mx[t] = cm;
                }
                // ---- probabilities, split as they sit: registers 8 s .. 8 s + 7 = the B operand of k-step s
                bf16x8 pb[3][2];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(sT[e] - mx[t]);      // masked keys: exp2(-inf) = 0
                    l[t] += pe;
                    const ce_w_bf16x3 p3 = ce_w_split3(pe);
                    pb[0][e >> 3][e & 7] = p3.hi; pb[1][e >> 3][e & 7] = p3.mid; pb[2][e >> 3][e & 7] = p3.lo;
                }
                // ---- O^T += V^T P^T: A = V^T terms, lane (dim 32 d + c, h), k-step s: slots 16 s + 8 h .. + 7 of this tile
#pragma unroll
                for (int d = 0; d < DB; ++d)
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        bf16x8 va[3];
#pragma unroll
                        for (int tt = 0; tt < 3; ++tt)
                            va[tt] = *reinterpret_cast<const bf16x8*>(Vt + (tt * HD + 32 * d + c) * VLD + j0 + 16 * ks + 8 * h);
                        o[t][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[2], pb[0][ks], o[t][d], 0, 0, 0);
                        o[t][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[0], pb[2][ks], o[t][d], 0, 0, 0);
                        o[t][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[1], pb[1][ks], o[t][d], 0, 0, 0);
                        o[t][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[1], pb[0][ks], o[t][d], 0, 0, 0);
                        o[t][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[0], pb[1][ks], o[t][d], 0, 0, 0);
                        o[t][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[0], pb[0][ks], o[t][d], 0, 0, 0);
                    }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int q0 = 32 * (wave + 8 * t);
        const float lt = l[t] + __shfl_xor(l[t], 32, 64);
        if (q0 + c < S) {
            const float inv = 1.0f / lt;
            float* op = ctx + (int64_t)(t0 + q0 + c) * hidden + head * HD + 4 * h;
#pragma unroll
            for (int d = 0; d < DB; ++d)
#pragma unroll
                for (int g = 0; g < 4; ++g)                   // register 4 g + i = dim 32 d + 8 g + 4 h + i: 16 contiguous bytes per g
                    *reinterpret_cast<f32x4*>(op + 32 * d + 8 * g) =
                        f32x4{o[t][d][4 * g] * inv, o[t][d][4 * g + 1] * inv, o[t][d][4 * g + 2] * inv, o[t][d][4 * g + 3] * inv};
        }
    }
}

// ------------------------------------------------------------------ [CLS] gather, pooler + classifier (fp32)
__global__ __launch_bounds__(256) void ce_head_w(const float* __restrict__ h32, const int32_t* __restrict__ cu, int H,
                                                 const float* __restrict__ wp, const float* __restrict__ bp,
                                                 const float* __restrict__ wc, const float* __restrict__ bc, int n_labels,
                                                 int mode, float* __restrict__ out) {
    __shared__ float x[CE_W_MAX_H], pooled[CE_W_MAX_H];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, seq = blockIdx.x;
    const int nv = H >> 6;
    const float* src = h32 + (int64_t)cu[seq] * H;
    if (mode == 1) {                                       // RR_CE_OUT_CLS: last_hidden_state[:, 0]
        for (int c = tid; c < H; c += 256) out[(int64_t)seq * H + c] = src[c];
        return;
    }
    for (int c = tid; c < H; c += 256) x[c] = src[c];
    __syncthreads();
    // pooled[j] = tanh(Wp[j] . x + bp[j]); a wave takes rows j = wave, wave + 4, ..., eight rows' loads in flight at a time
    // (H % 128 == 0: a wave's H / 4 rows are whole groups of eight)
    for (int j0 = wave; j0 < H; j0 += 32) {
        float s8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + 4 * u;
            float s = 0.f;
            for (int i = 0; i < nv; ++i) s = __builtin_fmaf(wp[(int64_t)j * H + lane + 64 * i], x[lane + 64 * i], s);
            s8[u] = s;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float s = ce_w_wave_sum(s8[u]);
            if (lane == 0) pooled[j0 + 4 * u] = tanhf(s + bp[j0 + 4 * u]);
        }
    }
    __syncthreads();
    for (int l = wave; l < n_labels; l += 4) {
        float s = 0.f;
        for (int i = 0; i < nv; ++i) s = __builtin_fmaf(wc[(int64_t)l * H + lane + 64 * i], pooled[lane + 64 * i], s);
        s = ce_w_wave_sum(s);
        if (lane == 0) out[(int64_t)seq * n_labels + l] = s + bc[l];
    }
}

// ------------------------------------------------------------------ host side: the launches, one helper each
int ce_w_check_shape(const char* who, int hidden, int n_heads, int ffn, bool with_ffn) {
    RR_REQUIRE(hidden >= 128 && hidden <= CE_W_MAX_H && hidden % 128 == 0,
               "%s: hidden %d is not a multiple of 128 in [128, %d]", who, hidden, CE_W_MAX_H);
    RR_REQUIRE(n_heads >= 1 && hidden % n_heads == 0 && (hidden / n_heads == 32 || hidden / n_heads == 64),
               "%s: head dim %g (hidden %d / %d heads) is not 32 or 64", who, n_heads >= 1 ? (double)hidden / n_heads : 0.0, hidden, n_heads);
    RR_REQUIRE(!with_ffn || (ffn >= 128 && ffn <= CE_W_MAX_FFN && ffn % 128 == 0),
               "%s: ffn %d is not a multiple of 128 in [128, %d]", who, ffn, CE_W_MAX_FFN);
    return RR_OK;
}

int ce_w_set_attributes() {
    RR_HIP_TRY(hipFuncSetAttribute((const void*)ce_attention_x3w<32>, hipFuncAttributeMaxDynamicSharedMemorySize, ce_w_att<32>::LDS));
    RR_HIP_TRY(hipFuncSetAttribute((const void*)ce_attention_x3w<64>, hipFuncAttributeMaxDynamicSharedMemorySize, ce_w_att<64>::LDS));
    return RR_OK;
}

// NV = hidden / 64 is even (hidden % 128 == 0) and at most 16
#define CE_W_BY_WIDTH(hidden, LAUNCH)                                                             \
    switch ((hidden) / 128) {                                                                     \
        case 1: LAUNCH(2); break;  case 2: LAUNCH(4); break;  case 3: LAUNCH(6); break;  case 4: LAUNCH(8); break;   \
        case 5: LAUNCH(10); break; case 6: LAUNCH(12); break; case 7: LAUNCH(14); break; default: LAUNCH(16); break; \
    }

void ce_w_embed_ln(const int32_t* tok, const int32_t* typ, const int32_t* pos, int T, int hidden, int vocab, int n_pos, int n_typ,
                   const float* we, const float* pe, const float* te, const float* g, const float* b, float eps, float* h32,
                   hipStream_t st) {
    const float inv_h = 1.f / (float)hidden;
#define CE_W_LAUNCH(NV) \
    hipLaunchKernelGGL((ce_embed_ln_w<NV>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, tok, typ, pos, T, vocab, n_pos, n_typ, we, pe, te, g, b, eps, inv_h, h32)
    CE_W_BY_WIDTH(hidden, CE_W_LAUNCH)
#undef CE_W_LAUNCH
}

void ce_w_add_ln(const float* y, int parts, int64_t pstride, float* h32, int T, int hidden, const float* g, const float* b, float eps,
                 hipStream_t st) {
    const float inv_h = 1.f / (float)hidden;
#define CE_W_LAUNCH(NV) \
    hipLaunchKernelGGL((ce_add_ln_w<NV>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, y, parts, pstride, h32, T, g, b, eps, inv_h)
    CE_W_BY_WIDTH(hidden, CE_W_LAUNCH)
#undef CE_W_LAUNCH
}

void ce_w_attention(const float* qkv, const int32_t* cu, int n_seqs, int hidden, int n_heads, float* ctx, hipStream_t st) {
    const dim3 grid((unsigned)n_seqs, (unsigned)n_heads);
    if (hidden / n_heads == 32)
        hipLaunchKernelGGL((ce_attention_x3w<32>), grid, dim3(512), ce_w_att<32>::LDS, st, qkv, cu, ctx, 0.17677669529663687f /* 1 / sqrt(32) */, hidden);
    else
        hipLaunchKernelGGL((ce_attention_x3w<64>), grid, dim3(512), ce_w_att<64>::LDS, st, qkv, cu, ctx, 0.125f /* 1 / sqrt(64) */, hidden);
}

void ce_w_head(const float* h32, const int32_t* cu, int n_seqs, int hidden, const float* wp, const float* bp, const float* wc,
               const float* bc, int n_labels, int mode, float* out, hipStream_t st) {
    hipLaunchKernelGGL(ce_head_w, dim3((unsigned)n_seqs), dim3(256), 0, st, h32, cu, hidden, wp, bp, wc, bc, n_labels, mode, out);
}

#ifdef RR_DEBUG_HARNESS
// tests/test_gpu_k5_wide_kernels.py: the kernels above one launch at a time on caller data (device pointers, fp32 row-major),
// through the launchers ce_forward_w calls.  Every argument is checked before anything is launched; every entry waits.
// qkv [T][3 hidden] with Q UNSCALED, cu_seqlens [n_seqs + 1] on the device with cu[0] = 0, cu[n_seqs] = T and every length in
// [1, 512] (checked here on a host copy: the kernel trusts them) -> ctx [T][hidden]
extern "C" int rr_debug_ce_w_attention(const float* d_qkv, int32_t T, const int32_t* d_cu, int32_t n_seqs, int32_t hidden, int32_t n_heads,
                                       float* d_ctx) {
    RR_REQUIRE(T >= 1 && n_seqs >= 1 && n_seqs <= T && d_qkv && d_cu && d_ctx, "rr_debug_ce_w_attention: bad arguments");
    if (int rc = ce_w_check_shape("rr_debug_ce_w_attention", hidden, n_heads, 0, false)) return rc;
    if (int rc = ce_w_set_attributes()) return rc;
    std::vector<int32_t> cu((size_t)n_seqs + 1);
    RR_HIP_TRY(hipMemcpy(cu.data(), d_cu, sizeof(int32_t) * cu.size(), hipMemcpyDeviceToHost));
    RR_REQUIRE(cu[0] == 0 && cu[n_seqs] == T, "rr_debug_ce_w_attention: cu_seqlens run from %d to %d, not from 0 to %d", cu[0], cu[n_seqs], T);
    for (int i = 0; i < n_seqs; ++i)
        RR_REQUIRE(cu[i + 1] - cu[i] >= 1 && cu[i + 1] - cu[i] <= 512, "rr_debug_ce_w_attention: sequence %d has %d tokens, outside [1, 512]",
                   i, cu[i + 1] - cu[i]);
    ce_w_attention(d_qkv, d_cu, n_seqs, hidden, n_heads, d_ctx, nullptr);
    RR_HIP_TRY(hipGetLastError());
    RR_HIP_TRY(hipDeviceSynchronize());
    return RR_OK;
}

// h[t] = LayerNorm(y[t] + h[t]) * g + b for T rows of `hidden`, in place as in the forward pass
extern "C" int rr_debug_ce_w_add_ln(const float* d_y, float* d_h, int32_t T, int32_t hidden, const float* d_g, const float* d_b, float eps) {
    RR_REQUIRE(T >= 1 && d_y && d_h && d_g && d_b, "rr_debug_ce_w_add_ln: bad arguments");
    RR_REQUIRE(hidden >= 128 && hidden <= CE_W_MAX_H && hidden % 128 == 0, "rr_debug_ce_w_add_ln: hidden %d is not a multiple of 128 in [128, %d]",
               hidden, CE_W_MAX_H);
    ce_w_add_ln(d_y, 1, 0, d_h, T, hidden, d_g, d_b, eps, nullptr);
    RR_HIP_TRY(hipGetLastError());
    RR_HIP_TRY(hipDeviceSynchronize());
    return RR_OK;
}
#endif
