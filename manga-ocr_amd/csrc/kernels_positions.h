// Token positions: where in the crop each token was read.
//
// The cross-attention of the last decoder layer over the 14 x 14 patch grid, recomputed AFTER a batch has decoded from the
// rows its decode steps recorded (the LayerNorm-1 outputs the query projection read): per (row, position) the softmax of
// every head over the 197 encoder keys, the mean of the twelve probability maps, and of that map the centre, spread and
// mass over the 196 patches.  The decode steps' attention kernels are not involved.
//
// attn_positions_kernel: one block = one wave per (row, tile of 16 positions); it loops over the 12 heads.
//   * bf16: S^T = K_h Q_h^T on v_mfma_f32_16x16x32_bf16, 13 key tiles x 2 k-steps per head.  The KEY tile is the A
//     operand and the 16 queries the B operand, so lane (l15, g) ends up with the scores of ONE position (l15) for the
//     keys 16 kt + 4 g + r of every key tile: softmax and map are lane-local plus two exchanges across the four lane
//     groups.  Both operands are d-contiguous in memory (A[row key][k = 8 g + j], B[k = 8 g + j][col position]): every
//     fragment is one 16-byte global load, no LDS, no transposed copy.
//   * fp32: the same lane <-> (position, key) map, the scores as k-ordered fmaf chains (parity engines; not tuned).
//   * the 13th key tile holds keys 192 .. 207 of which 192 .. 196 exist: the loads of the others are clamped to key 196
//     (nothing behind a row's 197 keys is read) and their scores are -inf before the maximum.
//   * the head-mean map stays in registers (13 x 4 values per lane); the five sums are reduced across the four lane groups;
//     the spread is the second pass sum a (u - cx)^2 / mass - the definition's sum a u^2 / mass - cx^2 without its
//     cancellation.
//   * a tile behind the row's length exits at once; positions behind it inside a tile are computed on the last valid
//     query and not written.
//   * the gathered-query form (PosParams::trail set; beam search): row r of the launch is a finished
//     hypothesis, and the query of its position p lies in the row that RAN that step - row (r / K) K + trail[r][p + 1] of
//     the query block, position p.  Keys, lengths and outputs stay by row r.  One byte load per lane before the head loop:
//     it moves the lane's query base and nothing else, the key loop is the same instructions.
#pragma once
#include "common.h"
#include "kernels_latent.h"      // row16_sum

#define POS_KEYS 197
#define POS_KT 13                // key tiles of 16
#define POS_FIELDS 5

struct PosParams {
    const void* q;              // [rows][..][768] T: position t of row r at q + r * q_row_stride + t * 768
    const void* k;              // [rows][197][768] T: key j of row r at k + r * k_row_stride + j * 768
    long long q_row_stride, k_row_stride;      // elements
    const int* len;             // [rows]: positions 0 .. len[r] + len_bias - 1 of row r are computed (at most T)
    int len_bias;
    int T;
    float* out_pos;             // position t of row r at out_pos + r * pos_row_stride + t * 5 (cx, cy, sx, sy, mass)
    long long pos_row_stride;   // floats
    float* out_map;             // nullable: [rows][T][197] the head-mean map
    // the gathered-query form (null: every row reads its own queries)
    const uint8_t* trail;       // [rows][trail_ld]: [p + 1] = the row, 0 .. K - 1 of r's group of K, that holds the query of position p
    long long trail_ld;
    int K;                      // rows is a multiple of it
};

template <typename T>
__global__ __launch_bounds__(64) void attn_positions_kernel(PosParams p) {
    const int r = blockIdx.y, t0 = blockIdx.x * 16;
    const int n = min(p.len[r] + p.len_bias, p.T);
    if (t0 >= n) return;
    const int lane = threadIdx.x, l15 = lane & 15, g = lane >> 4;
    const int pos = min(t0 + l15, n - 1);
    int qr = r;
    if (p.trail) qr = r - r % p.K + min((int)p.trail[(size_t)r * p.trail_ld + pos + 1], p.K - 1);
    const T* const qrow = reinterpret_cast<const T*>(p.q) + (size_t)qr * p.q_row_stride + (size_t)pos * 768;
    const T* const kbase = reinterpret_cast<const T*>(p.k) + (size_t)r * p.k_row_stride;
    float amap[POS_KT][4];
#pragma unroll
    for (int kt = 0; kt < POS_KT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) amap[kt][i] = 0.f;

    for (int h = 0; h < 12; ++h) {
        float s[POS_KT][4];
        if constexpr (sizeof(T) == 2) {
            const bf16_t* const qh = reinterpret_cast<const bf16_t*>(qrow) + 64 * h + 8 * g;
            const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(qh), q1 = *reinterpret_cast<const bf16x8*>(qh + 32);
#pragma unroll
            for (int kt = 0; kt < POS_KT; ++kt) {
                const int key = min(16 * kt + l15, POS_KEYS - 1);
                const bf16_t* const kr = reinterpret_cast<const bf16_t*>(kbase) + (size_t)key * 768 + 64 * h + 8 * g;
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(kr), a1 = *reinterpret_cast<const bf16x8*>(kr + 32);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, q0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, q1, acc, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[kt][i] = acc[i];
            }
        } else {
            const float* const qh = reinterpret_cast<const float*>(qrow) + 64 * h;
            float4 qv[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) qv[d] = *reinterpret_cast<const float4*>(qh + 4 * d);
#pragma unroll
            for (int kt = 0; kt < POS_KT; ++kt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = min(16 * kt + 4 * g + i, POS_KEYS - 1);
                    const float* const kr = reinterpret_cast<const float*>(kbase) + (size_t)key * 768 + 64 * h;
                    float acc = 0.f;
#pragma unroll
                    for (int d = 0; d < 16; ++d) {
                        const float4 kv = *reinterpret_cast<const float4*>(kr + 4 * d);
                        acc = fmaf(qv[d].x, kv.x, acc); acc = fmaf(qv[d].y, kv.y, acc);
                        acc = fmaf(qv[d].z, kv.z, acc); acc = fmaf(qv[d].w, kv.w, acc);
                    }
                    s[kt][i] = acc;
                }
        }
        // softmax over the 197 keys of this lane's position (52 here, the rest in the lanes l15 + 16, + 32, + 48), in fp32
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < POS_KT; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = s[kt][i] * 0.125f;
                if (kt == POS_KT - 1 && 16 * kt + 4 * g + i >= POS_KEYS) v = -INFINITY;
                s[kt][i] = v;
                m = fmaxf(m, v);
            }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < POS_KT; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) { s[kt][i] = __expf(s[kt][i] - m); sum += s[kt][i]; }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int kt = 0; kt < POS_KT; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) amap[kt][i] = fmaf(s[kt][i], inv, amap[kt][i]);
    }

    // the mean of the twelve maps; centre, spread and mass over the patches (key 0 is CLS; key k >= 1 is patch row (k - 1) / 14,
    // column (k - 1) % 14, at u = (column + 0.5) / 14, v = (row + 0.5) / 14)
    const bool live = t0 + l15 < n;
    float mass = 0.f, su = 0.f, sv = 0.f;
    float* const mrow = p.out_map ? p.out_map + ((size_t)r * p.T + pos) * POS_KEYS : nullptr;
#pragma unroll
    for (int kt = 0; kt < POS_KT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = 16 * kt + 4 * g + i;
            const float a = amap[kt][i] * (1.0f / 12.0f);
            amap[kt][i] = a;
            if (key < POS_KEYS) {
                if (mrow && live) mrow[key] = a;
                if (key >= 1) {
                    const int pi = (key - 1) / 14, pj = (key - 1) - 14 * pi;
                    mass += a;
                    su = fmaf(a, ((float)pj + 0.5f) / 14.0f, su);
                    sv = fmaf(a, ((float)pi + 0.5f) / 14.0f, sv);
                }
            }
        }
    mass += __shfl_xor(mass, 16, 64); mass += __shfl_xor(mass, 32, 64);
    su += __shfl_xor(su, 16, 64); su += __shfl_xor(su, 32, 64);
    sv += __shfl_xor(sv, 16, 64); sv += __shfl_xor(sv, 32, 64);
    const bool some = mass >= 1e-20f;
    const float cx = some ? su / mass : 0.5f, cy = some ? sv / mass : 0.5f;
    float vu = 0.f, vv = 0.f;
#pragma unroll
    for (int kt = 0; kt < POS_KT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = 16 * kt + 4 * g + i;
            if (key >= 1 && key < POS_KEYS) {
                const int pi = (key - 1) / 14, pj = (key - 1) - 14 * pi;
                const float du = ((float)pj + 0.5f) / 14.0f - cx, dv = ((float)pi + 0.5f) / 14.0f - cy;
                vu = fmaf(amap[kt][i], du * du, vu);
                vv = fmaf(amap[kt][i], dv * dv, vv);
            }
        }
    vu += __shfl_xor(vu, 16, 64); vu += __shfl_xor(vu, 32, 64);
    vv += __shfl_xor(vv, 16, 64); vv += __shfl_xor(vv, 32, 64);
    if (g == 0 && live) {
        float* const o = p.out_pos + (size_t)r * p.pos_row_stride + (size_t)(t0 + l15) * POS_FIELDS;
        o[0] = cx; o[1] = cy;
        o[2] = some ? sqrtf(fmaxf(vu / mass, 0.f)) : 0.f;
        o[3] = some ? sqrtf(fmaxf(vv / mass, 0.f)) : 0.f;
        o[4] = mass;
    }
}

// Small-batch decode path (kernels_smallm.h): its LayerNorm 1 is the prologue of the cross-query projection and never
// reaches memory, so a batch that records positions writes T(LayerNorm(a_f32[slot])) - the prologue's expression and
// reduction order, a 16-lane group per row - to hist[rowmap[slot]][step[slot]].
template <typename T>
__global__ __launch_bounds__(256) void hist_ln_rows_kernel(const float* __restrict__ a_f32, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, T* __restrict__ hist,
                                                           long long hist_row_stride, const int* __restrict__ step,
                                                           const int* __restrict__ rowmap, int rows) {
    const int slot = blockIdx.x * 16 + (threadIdx.x >> 4), l15 = threadIdx.x & 15;
    if (slot >= rows) return;
    const float* const xr = a_f32 + (size_t)slot * 768 + 4 * l15;
    float4 v[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j] = *reinterpret_cast<const float4*>(xr + 64 * j);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    const float mean = row16_sum(s) * (1.0f / 768);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const float d0 = v[j].x - mean, d1 = v[j].y - mean, d2 = v[j].z - mean, d3 = v[j].w - mean;
        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    const float rstd = 1.0f / sqrtf(row16_sum(q) * (1.0f / 768) + eps);
    T* const dst = hist + (size_t)rowmap[slot] * hist_row_stride + (size_t)step[slot] * 768 + 4 * l15;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const float4 gm = *reinterpret_cast<const float4*>(gamma + 4 * l15 + 64 * j);
        const float4 bt = *reinterpret_cast<const float4*>(beta + 4 * l15 + 64 * j);
        const float o[4] = {(v[j].x - mean) * rstd * gm.x + bt.x, (v[j].y - mean) * rstd * gm.y + bt.y,
                            (v[j].z - mean) * rstd * gm.z + bt.z, (v[j].w - mean) * rstd * gm.w + bt.w};
        elem<T>::st4(dst + 64 * j, o);
    }
}
