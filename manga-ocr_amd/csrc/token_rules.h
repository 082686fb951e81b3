// The rules that end a decode step, each written once: the building blocks shared by the LM-head epilogue (kernels_gemm.h),
// dec_token_kernel and the init kernels (kernels_decode.h) and beam_select_kernel (kernels_beam.h).  Every block is
// __forceinline__ and takes what it reads as arguments, so a kernel form pays for the rules it names and nothing else.
#pragma once
#include "common.h"

// The first edge of a state's range [lo, hi) whose token is >= c (hi: none).  A state's edge tokens ascend strictly, so the
// edge on token c, if the state has one, is the one returned.
__device__ __forceinline__ int edge_lower_bound(const int* edge_token, int lo, int hi, int c) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edge_token[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The weights of the edges of a state (its range [e0, e1)) that fall into columns c .. c + 3, added to the four logits of v:
// one binary search, then at most four edges.  Constant indices only: no register is indexed.  A weight of exactly 0 - every
// edge of a hard automaton - is "no weight" and is skipped, so a logit of -0.0f keeps its sign.  The token kernel's slab path.
// The LM head's group is wider (16 or 64 columns of the tile in LDS) and the beam selection adds its weights behind
// (v - gmax) - log S, not into v: both walk from edge_lower_bound with a loop of their own and restate the skip.
__device__ __forceinline__ void add_edge_weights4(float4& v, const int* edge_token, const float* edge_weight, int e0, int e1, int c) {
    for (int lo = edge_lower_bound(edge_token, e0, e1, c); lo < e1; ++lo) {
        const int d = edge_token[lo] - c;
        if (d >= 4) break;
        const float wgt = edge_weight[lo];
        if (wgt != 0.f) {
            if (d == 0) v.x += wgt; else if (d == 1) v.y += wgt; else if (d == 2) v.z += wgt; else v.w += wgt;
        }
    }
}

// A(state) into the `words` mask words in LDS, by the whole block: an OPEN state (a soft automaton's state with a default
// edge) allows every token and EOS iff it accepts; any other state allows its edges' tokens, and EOS iff it accepts; a state
// < 0 (DEAD) allows nothing.  Two barriers: behind the fill and behind the bits.  The AND with the row's base or set word is
// the caller's.  `open` is a compile-time false where the form has no default edges.
__device__ __forceinline__ void state_mask_to_lds(unsigned* s_mask, int state, bool open, const int* edge_begin, const int* edge_token,
                                                  const uint8_t* accepting, int eos_id, int V, int words, int tid, int nthreads) {
    if (tid < words) s_mask[tid] = open ? ~0u : 0u;
    __syncthreads();
    if (open) {
        if (tid == 0 && !accepting[state] && (unsigned)eos_id < (unsigned)V) s_mask[eos_id >> 5] &= ~(1u << (eos_id & 31));
    } else if (state >= 0) {
        const int e1 = edge_begin[state + 1];
        for (int i = edge_begin[state] + tid; i < e1; i += nthreads) {
            const int a = edge_token[i];
            if ((unsigned)a < (unsigned)V) atomicOr(&s_mask[a >> 5], 1u << (a & 31));
        }
        if (tid == 0 && accepting[state] && (unsigned)eos_id < (unsigned)V) atomicOr(&s_mask[eos_id >> 5], 1u << (eos_id & 31));
    }
    __syncthreads();
}

// The n-gram bans of a row that holds L tokens rid[0 .. L - 1], on its mask in LDS: the 256 threads split the windows
// i = 0 .. L - n, a window whose n - 1 key tokens equal the row's last n - 1 clears the bit of its follower.  n = 1 has an
// empty key: every token of the row is banned.  L < n has no window.  For blocks of 256 threads (the stride of the split).
__device__ __forceinline__ void ngram_ban_windows(unsigned* s_mask, const int* rid, int L, int n, int V, int tid) {
    const int* key = rid + (L - n + 1);         // the row's last n - 1 tokens
    for (int i = tid; i <= L - n; i += 256) {
        bool same = true;
        for (int k = 0; k < n - 1 && same; ++k) same = rid[i + k] == key[k];
        const int ban = rid[i + n - 1];
        if (same && (unsigned)ban < (unsigned)V) atomicAnd(&s_mask[ban >> 5], ~(1u << (ban & 31)));
    }
}

// Word w of the first mask of a row: its base set's word, minus the start token when n = 1 (ban_start) - the one token the row
// holds when its first token is chosen.
__device__ __forceinline__ unsigned base_row_word(const unsigned* base_mask, int set, int words, int w, bool ban_start, int start_id) {
    unsigned m = base_mask[(size_t)set * words + w];
    if (ban_start && w == (start_id >> 5)) m &= ~(1u << (start_id & 31));
    return m;
}

// The slab path's logits of slot b, the 24 a thread holds (columns tid * 4 + j * 1024 + 0 .. 3): bias + slab_0 + slab_1 + ...
// in fp32, in this order.  (The beam winners' per-column re-sum in beam_select_kernel spells the same order out for one column.)
// For blocks of 256 threads and V = 6 * 1024 columns, like the a[6] its callers hold.
__device__ __forceinline__ void sum_slab_row(float4 (&a)[6], const float* vbias, const float* slabs, int nslab, long long slab_stride, int b,
                                             int V, int tid) {
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = *reinterpret_cast<const float4*>(vbias + tid * 4 + j * 1024);
    for (int s = 0; s < nslab; ++s) {
        const float* sp = slabs + (size_t)s * slab_stride + (size_t)b * V + tid * 4;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float4 x = *reinterpret_cast<const float4*>(sp + j * 1024);
            a[j].x += x.x; a[j].y += x.y; a[j].z += x.z; a[j].w += x.w;
        }
    }
}

// The next input of slot b (row `row` of the batch): LN(word[tok] + type[0] + pos[ps]) (modeling_bert.py:98-106), block-wide
// over D = 768 (3 per thread, 256 threads), stored to x_f32 and x_t by slot and, by row at position ps, to the layer-0
// key/value source `cache` and its e4m3 twin `cache8` where they are given.  Three barriers; s_red (4 floats) is read last
// before the stores, so a caller that comes back (the beam loop) puts one more barrier behind the call.  For blocks of 256 threads.
template <typename T, int D>
__device__ __forceinline__ void embed_ln_store(int tok, int ps, int b, int row, const float* word, const float* type0, const float* pos,
                                               const float* gamma, const float* beta, float* x_f32, T* x_t, float eps, T* cache,
                                               long long cache_batch_stride, uint8_t* cache8, float inv_sx8, float* s_red, int tid) {
    constexpr int PER = D / 256;
    const int lane = tid & 63, wave = tid >> 6;
    float v[PER];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int d = tid + i * 256;
        float e = word[(size_t)tok * D + d] + type0[d];
        e = e + pos[(size_t)ps * D + d];
        v[i] = e; s += e;
    }
    s = wave_sum(s);
    if (lane == 0) s_red[wave] = s;
    __syncthreads();
    const float mean = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) * (1.0f / D);
    __syncthreads();
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { const float d = v[i] - mean; q += d * d; }
    q = wave_sum(q);
    if (lane == 0) s_red[wave] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf((s_red[0] + s_red[1] + s_red[2] + s_red[3]) * (1.0f / D) + eps);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int d = tid + i * 256;
        const float o = (v[i] - mean) * rstd * gamma[d] + beta[d];
        x_f32[(size_t)b * D + d] = o;
        elem<T>::st(x_t + (size_t)b * D + d, o);
        if (cache) elem<T>::st(cache + (size_t)row * cache_batch_stride + (size_t)ps * D + d, o);
        if (cache8) cache8[(size_t)row * cache_batch_stride + (size_t)ps * D + d] = (uint8_t)(pack4_fp8(o * inv_sx8, 0.f, 0.f, 0.f) & 0xff);
    }
}
