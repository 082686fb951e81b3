// MFMA GEMM for the recogniser's dense layers:  C[M,N] = A[M,K] . W[N,K]^T  (+ epilogue)
//
// Both operands are K-contiguous (activations row-major, weights in torch.nn.Linear's
// [out,in] layout), so A and W tiles are staged the same way.  One kernel template serves
//   T = bf16_t : v_mfma_f32_32x32x16_bf16, fp32 accumulate             (throughput mode)
//   T = float  : v_mfma_f32_32x32x2_f32, an exact k-ordered fmaf chain  (parity mode)
// because a K-tile is defined in BYTES: 128 B per row (64 bf16 / 32 f32).
//
// Structure (cdna_hip_programming.md §5, "2-buffer glds" form):
//   * 256 threads = 4 waves as 2x2; each wave owns a (BM/2)x(BN/2) sub-tile = TMxTN MFMA tiles.
//   * global -> LDS by global_load_lds_dwordx4 (no VGPR round trip).  One wave-instruction
//     writes 1 KiB = 8 rows x 128 B, lane-linear; the bank-conflict swizzle is therefore
//     applied on the SOURCE address and on the fragment read (rule 21):
//         16-byte chunk c of row r lives at chunk  c ^ ((r >> 1) & 7).
//     With 128-B rows two rows share one 256-B bank row; (r>>1)&7 makes every ds_read_b128
//     16-lane group hit 16 distinct 16-B slots (conflict-free).
//   * double-buffered: tile t+1 is in flight while tile t is multiplied; one barrier per K-tile.
//   * epilogue through LDS (fp32 tile) so that global stores / residual loads are full
//     16-byte, row-contiguous accesses; bias / GELU / residual / position-embedding are fused.
//   * blockIdx -> tile map is XCD-aware (bijective remap, §5 T1): the 8 XCDs each get a
//     contiguous run of tiles, so tiles sharing an A row-panel share an L2.
#pragma once
#include "common.h"
#include "token_rules.h"
#include <type_traits>

#ifndef MOCR_GEMM_MFMA16
#define MOCR_GEMM_MFMA16 1      // 1: v_mfma_f32_16x16x32_bf16 in gemm_kernel's bf16 path (+2..6 % at M = 806,912, r01); 0: 32x32x16
#endif

enum GemmEpilogue {
    EPI_SLAB = 0,        // fp32 partial sums of K-slice blockIdx.z -> out[z][m][n]   (split-K, no bias)
    EPI_BIAS = 1,        // out T   = acc + bias
    EPI_BIAS_GELU = 2,   // out T   = gelu(acc + bias)
    EPI_BIAS_RESID = 3,  // out f32 = (acc + bias) + resid        (out may alias resid)
    EPI_PATCH = 4,       // patch-embed: out f32[b*197+1+p] = (acc + bias) + pos[1+p]
    EPI_BIAS_F32 = 5,    // out f32 = acc + bias
    EPI_ARGMAX = 6,      // LM head: per (row, N-tile) the fp32 max of acc + bias and its column (lowest column wins ties):
                         //   out f32 [M][ntn] values, cand_idx int [M][ntn] columns - the logits never go to memory
    EPI_ARGMAX_LSE = 7,  // token scores: EPI_ARGMAX + cand_sum f32 [M][ntn] = the tile's sum of exp(acc + bias - the tile's max),
                         //   from which the token kernel gets the chosen token's log-probability; the logits still stay in LDS
    EPI_TOPK = 8,        // token alternatives: EPI_ARGMAX_LSE + top_val f32 / top_idx int [M][ntn][4] = the tile's four largest
                         //   acc + bias and their columns (value descending, lower column first on a tie); entry 0 = the arg-max
    EPI_ARGMAX_M = 9,    // token constraints: the three LM-head epilogues above with the row's allowed-token set applied - a column
    EPI_ARGMAX_LSE_M = 10, //   outside the set counts as -inf in the max, the exp sum and the four best (GemmParams::tok_mask /
    EPI_TOPK_M = 11      //   set_of_row / rowmap); a tile without an allowed column leaves (-inf, 0x7fffffff), sum 0
};

struct GemmParams {
    const void* A;
    const void* W;
    const float* bias;
    void* out;
    const float* resid;
    const float* pos;      // EPI_PATCH: [tokens][N] position embeddings
    int* cand_idx;         // EPI_ARGMAX: [M][ntn] winning columns
    int M, N;              // logical output size (rows >= M are computed but not stored)
    int lda, ldw, ldo;     // leading dimensions in elements
    int k_per_split;       // elements of K handled by one blockIdx.z
    long long slab_stride; // EPI_SLAB: elements between slabs
    int ntn;               // tiles along N
    int patches;           // EPI_PATCH: patches per image (196)
    long long a_yoff, w_yoff, o_yoff, b_yoff;  // element offsets per blockIdx.y (per-head batched GEMMs; EPI_BIAS only)
    int ablate;            // diagnostics only (MOCR_GEMM_ABLATE): 1 no MFMA, 2 no DMA after tile 0, 4 no epilogue
    int group_n;           // tile order: N-tiles per column group (0 = all: plain row-major tile order)
    int ntm;               // tiles along M
    int stagger;           // wide2: the first-round blocks start up to this many x 1024 cycles late (0 = together)
    int first_round;       // blocks that start at launch (one per CU)
    // LayerNorm folded into the encoder's persistent GEMMs (gemm_pers_kernel LNF, kernels_gemm_pers.h):
    float* ln_part;        // [M][4][2] per-row partial (sum, sum of squares) over each 256-column slice of the fp32 rows:
                           // written by the fp32-residual GEMM (slice = its N-tile), read by the GEMM that multiplies the rows
    const float* csum;     // [N] column sums of the folded weight W o gamma (as rounded to bf16)
    void* xb;              // fp32-residual GEMM: bf16 copy of the output rows, [M][ldo]
    float ln_eps;
    float* cand_sum;       // EPI_ARGMAX_LSE: [M][ntn] sum of exp(logit - tile max) over the tile's columns
    float* top_val;        // EPI_TOPK: [M][ntn][4] the tile's four largest logits, descending ...
    int* top_idx;          // ... and their columns
    // EPI_*_M (token constraints): GEMM row m is decode slot m, which decodes batch row rowmap[m] under set set_of_row[row]
    const unsigned* tok_mask;   // [sets][N / 32] bit n of a set's row = column n is allowed; set 0 is all ones
    const int* set_of_row;      // [rows of the batch] set of every row, indexed by ROW like ids
    const int* rowmap;          // [M] slot -> row (null: identity)
    // Forced prefixes (EPI_ARGMAX_LSE_M / EPI_TOPK_M; tgt_val null = none: the launcher picks gemm_kernel's TGT by it).  Slot m decodes row
    // rowmap[m] at step step[m]; a step below the row's prefix_len has the target column prefix[row * prefix_ld + step]
    const int* prefix;          // [rows of the batch][prefix_ld] the caller-given tokens (without the start token), by ROW
    const int* prefix_len;      // [rows of the batch] by ROW
    int prefix_ld;
    const int* step;            // [M] by slot
    float* tgt_val;             // [M] by slot: acc + bias of the target column, -inf when the row's set leaves it out
};

// Soft token automata (EPI_*_M with gemm_kernel's SOFT): GemmParams plus the rows' states and the arena's tables, the argument of
// the SOFT instantiations alone - every other form takes GemmParams as it was, so its argument block does not change.
struct GemmParamsSoft : GemmParams {
    const int* aut_state;       // [rows of the batch] by ROW: the global state the row is in (< 0: no automaton / dead)
    const int* edge_begin;      // [states + 1]
    const int* edge_token;      // [edges] a state's tokens strictly ascending
    const float* edge_weight;   // [edges] what the edge adds to its token's logit
};

// Repetition penalty (EPI_*_M with gemm_kernel's PEN, which is SOFT too): GemmParamsSoft plus the rows' seen tokens and their
// penalties, the argument of the PEN instantiations alone.  aut_state may be null here: a penalty without any automaton.
struct GemmParamsPen : GemmParamsSoft {
    const unsigned* seen_mask;      // [rows of the batch][N / 32] by ROW: bit n = token n is in the row (start, forced, chosen)
    const float* penalty_of_row;    // [rows of the batch] by ROW: finite, > 0; 1 = off
};

// Linear tile id -> (tm, tn).  Tiles are ordered column-group by column-group: inside a group of
// `group_n` N-tiles the order is M-major / N-minor, so the blocks resident on one XCD at a time cover
// a few M-tiles x group_n N-tiles and the group's weight slice (group_n*BN rows of W) stays in that
// XCD's 4 MiB L2 while the A row-panels stream through it once per group.
__device__ __forceinline__ void gemm_tile_of(const GemmParams& p, int bid, int& tm, int& tn) {
    const int gn = p.group_n > 0 && p.group_n < p.ntn ? p.group_n : p.ntn;
    const int per_group = p.ntm * gn;
    int g = bid / per_group;
    const int ngroups = (p.ntn + gn - 1) / gn;
    if (g >= ngroups) g = ngroups - 1;
    const int r = bid - g * per_group;
    const int gw = min(gn, p.ntn - g * gn);
    tm = r / gw;
    tn = g * gn + r - tm * gw;
}

// Read the fp32 tile back from LDS row by row and apply the fused epilogue; every global access is
// a 16-byte, row-contiguous access.  NT = threads in the block.
// SWZ: the tile was written with its 16-column groups XOR-swizzled by (row>>2)&3 (the 16x16 MFMA's four
// lane groups sit 4 rows apart = the same bank; the swizzle spreads them over the banks).
template <typename T, int BM, int BN, int EPI, int NT, bool SWZ = false>
__device__ __forceinline__ void gemm_epilogue(const float* sC, const GemmParams& p, int m0, int n0, int tid, int z) {
    constexpr int TPR = BN / 4;      // threads per output row (4 columns each)
    constexpr int RPI = NT / TPR;    // rows per pass
    const int col = (tid % TPR) * 4;
    const int n = n0 + col;
    float bias4[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EPI != EPI_SLAB) {
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + n);
        bias4[0] = bv.x; bias4[1] = bv.y; bias4[2] = bv.z; bias4[3] = bv.w;
    }
#pragma unroll 4
    for (int it = 0; it < BM / RPI; ++it) {
        const int row = it * RPI + tid / TPR;
        const int m = m0 + row;
        if (m >= p.M) continue;
        const float4 cv = *reinterpret_cast<const float4*>(&sC[row * BN + (SWZ ? (col ^ (((row >> 2) & 3) << 4)) : col)]);
        float v[4] = {cv.x + bias4[0], cv.y + bias4[1], cv.z + bias4[2], cv.w + bias4[3]};
        if constexpr (EPI == EPI_SLAB) {
            float* o = reinterpret_cast<float*>(p.out) + (size_t)z * p.slab_stride + (size_t)m * p.ldo + n;
            *reinterpret_cast<float4*>(o) = cv;
        } else if constexpr (EPI == EPI_BIAS) {
            if constexpr (sizeof(T) == 2) {
                if (p.ablate & 8) {     // experiment: streaming (non-temporal) output stores
                    unsigned long long u = (unsigned long long)f2bf(v[0]) | ((unsigned long long)f2bf(v[1]) << 16) |
                                           ((unsigned long long)f2bf(v[2]) << 32) | ((unsigned long long)f2bf(v[3]) << 48);
                    __builtin_nontemporal_store(u, reinterpret_cast<unsigned long long*>(reinterpret_cast<T*>(p.out) + (size_t)m * p.ldo + n));
                    continue;
                }
            }
            elem<T>::st4(reinterpret_cast<T*>(p.out) + (size_t)m * p.ldo + n, v);
        } else if constexpr (EPI == EPI_BIAS_GELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_for<T>(v[e]);
            elem<T>::st4(reinterpret_cast<T*>(p.out) + (size_t)m * p.ldo + n, v);
        } else if constexpr (EPI == EPI_BIAS_RESID) {
            const float4 rv = *reinterpret_cast<const float4*>(p.resid + (size_t)m * p.ldo + n);
            float* o = reinterpret_cast<float*>(p.out) + (size_t)m * p.ldo + n;
            *reinterpret_cast<float4*>(o) = make_float4(v[0] + rv.x, v[1] + rv.y, v[2] + rv.z, v[3] + rv.w);
        } else if constexpr (EPI == EPI_PATCH) {
            const int b = m / p.patches, pi = m - b * p.patches;
            const float4 pv = *reinterpret_cast<const float4*>(p.pos + (size_t)(1 + pi) * p.N + n);
            float* o = reinterpret_cast<float*>(p.out) + ((size_t)b * (p.patches + 1) + 1 + pi) * p.ldo + n;
            *reinterpret_cast<float4*>(o) = make_float4(v[0] + pv.x, v[1] + pv.y, v[2] + pv.z, v[3] + pv.w);
        } else {  // EPI_BIAS_F32
            float* o = reinterpret_cast<float*>(p.out) + (size_t)m * p.ldo + n;
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// EPI_ARGMAX: every output row of the tile is reduced to (max of acc + bias, its column; the lowest column wins ties).
// NT / BM threads share a row (adjacent lanes); a thread scans its BN / (NT/BM) physical columns of the LDS tile 4 at a
// time, starting at a row-dependent rotation so that the 16 lanes of a ds_read_b128 group hit 16 different 16-byte
// slots.  SWZ: the tile's 16-column groups are XORed with (row>>2)&3 (see gemm_epilogue): physical -> logical column.
// LSE (EPI_ARGMAX_LSE): once the row's threads agree on the tile's max, each walks its columns a second time - same
// rotation, same swizzle, so as conflict-free as the first walk - and sums exp(v - max) in fp32; cand_sum[m][tile] gets the
// row's sum (>= 1: the max itself contributes exp(0)).  v = acc + bias is recomputed with the same fp32 add as in the first
// walk, so v - max is exactly 0 at the winning column and <= 0 everywhere else.
// TOPK (EPI_TOPK, implies LSE): the first walk keeps the thread's four best instead of its best (Top4: the same order, so
// entry 0 is the arg-max the other variants find), the row's threads merge their lists by shuffles, and part 0 also writes
// the row's list, top_val / top_idx [m][tile][0..3], as two 16-byte stores.
// MASK (EPI_*_M, token constraints): the row's set decides which columns exist.  A thread's CPP physical columns are one
// CPP-aligned group of logical columns (the swizzle XORs multiples of 16 below CPP, or moves a 16-column group whole), so
// its mask bits are 16 bits of one word or two whole words of the set's row, loaded once; a float4 starts at a multiple of 4,
// so its four bits are one nibble.  A column outside the set takes (-inf, index sentinel) in the first walk - it wins no
// comparison, not even the tie of two -inf against the initial entry - and contributes 0, by select, to the exp sum: a tile
// with no allowed column stores best = -inf, the sentinel and cand_sum = 0 (never exp(-inf - -inf)), which the token
// kernel's merge cand_sum * exp(cand_val - gmax) turns into 0 * 0.  Rows m >= M read set 0.
// Forced prefixes (MASK with LSE and TGT - a template parameter, so that batches without a prefix run the code they always
// ran, see profiles/prefix_cost.jsonl; GemmParams::tgt_val is set): a row whose step is below its prefix length has a target
// column.  The one thread of the one tile whose column group holds it stores tgt_val[m] = allowed ? sC + bias : -inf - the
// same fp32 add as in the first walk, so the value equals the tile's `best` bit for bit when the target wins.  One writer
// per row, a plain vector store; rows without a target leave tgt_val[m] alone.
// SOFT (implies MASK; p is a GemmParamsSoft): soft token automata.  Before the first walk the thread that owns the column group
// [g0, g0 + CPP) of row m reads the row's state - written by the previous step's token kernel, an earlier launch -, binary-
// searches g0 in the state's ascending edge tokens and adds the weight of every edge inside its group to the tile value in
// LDS, at the swizzled column.  A thread reads and writes its own group only, so there is no barrier; the max walk, the exp-sum
// walk, the four best and the target column then see logit + weight with no further change.  Rows without an automaton, dead
// rows and rows >= M add nothing.
// PEN (implies SOFT; p is a GemmParamsPen): repetition penalty.  The thread loads the `seen` bits of its column group exactly
// as it loads mbits - half a word or two words of seen_mask[row], by ROW - and the row's p.  Wherever a walk forms
// v = (tile value + edge weight) + bias of a seen column it takes pen_logit(v, p) instead, before the mask's select: in the
// first walk (plain and TOPK), in the exp-sum walk - the same expression, so v' - best is exactly 0 at the winner - and at the
// target column.  Rows m >= M read nothing (no bit, p = 1).  The edge weights are skipped where aut_state is null.
// What an LM-head epilogue does is a function of EPI alone; TGT, SOFT and PEN come with gemm_kernel's own flags and P, the
// parameter struct they need, is deduced.
constexpr bool epi_is_lm_head(int epi) {
    return epi == EPI_ARGMAX || epi == EPI_ARGMAX_LSE || epi == EPI_TOPK || epi == EPI_ARGMAX_M || epi == EPI_ARGMAX_LSE_M || epi == EPI_TOPK_M;
}
constexpr bool epi_mask(int epi) { return epi == EPI_ARGMAX_M || epi == EPI_ARGMAX_LSE_M || epi == EPI_TOPK_M; }
constexpr bool epi_topk(int epi) { return epi == EPI_TOPK || epi == EPI_TOPK_M; }
constexpr bool epi_lse(int epi) { return epi_topk(epi) || epi == EPI_ARGMAX_LSE || epi == EPI_ARGMAX_LSE_M; }

// A thread's group of a row of a bit table (a set's mask, a row's seen words): bit (c - g0) = column c of [g0, g0 + CPP) -
// half a word (CPP = 16, g0 a multiple of 16) or two whole words (CPP = 64, g0 a multiple of 64), loaded once.
template <int CPP>
__device__ __forceinline__ unsigned long long group_bits(const unsigned* wrow, int g0) {
    static_assert(CPP == 16 || CPP == 64, "the group is half a mask word or two words");
    if constexpr (CPP == 64) {
        const uint2 w2 = *reinterpret_cast<const uint2*>(wrow + (g0 >> 5));
        return ((unsigned long long)w2.y << 32) | w2.x;
    } else {
        return wrow[g0 >> 5] >> (g0 & 31);
    }
}

// The effective logit of a column that exists: v = (tile value + edge weight) + bias, penalised where the row has seen the
// column's token.  Every walk forms it with this one expression, so v - best is exactly 0 at the winner.  A column outside
// the row's set does not exist; what that means is the walk's own: (-inf, index sentinel) in the four-best walk, no
// comparison in the max walk, a term of 0 in the exp sum, -inf at the target column.
template <bool PEN>
__device__ __forceinline__ float lm_logit(float acc, float bias, bool seen, float pp) {
    const float v = acc + bias;
    if constexpr (PEN) return seen ? pen_logit(v, pp) : v;
    return v;
}

template <int BM, int BN, int NT, bool SWZ, int EPI, bool TGT, bool SOFT, bool PEN, typename P>
__device__ __forceinline__ void gemm_epilogue_argmax(const float* sC, const P& p, int m0, int n0, int tid) {
    constexpr bool LSE = epi_lse(EPI), TOPK = epi_topk(EPI), MASK = epi_mask(EPI);
    static_assert(!SOFT || MASK, "the weighted LM head is a masked one");
    static_assert(!PEN || SOFT, "the penalised LM head is the weighted one too");
    constexpr int TPRW = NT / BM, CPP = BN / TPRW;
    static_assert(TPRW == 2 || TPRW == 4, "two or four threads per row");
    const int row = tid / TPRW, part = tid % TPRW;
    const int m = m0 + row;
    const int sw = SWZ ? (((row >> 2) & 3) << 4) : 0;
    const int rot = 4 * (row % (CPP / 4));
    float best = -INFINITY;
    int bi = 0x7fffffff;
    // MASK: bit (c - g0) of mbits = logical column c of the thread's group [g0, g0 + CPP) is allowed
    unsigned long long mbits = ~0ull;
    const int g0 = n0 + (CPP < 64 ? ((part * CPP) ^ sw) : part * CPP);
    if constexpr (MASK) {
        int set = 0;
        if (m < p.M) set = p.set_of_row[p.rowmap ? p.rowmap[m] : m];
        mbits = group_bits<CPP>(p.tok_mask + (size_t)set * (p.N >> 5), g0);
    }
    // PEN: bit (c - g0) of sbits = logical column c of the thread's group is in the row; pp = the row's penalty
    unsigned long long sbits = 0ull;
    float pp = 1.f;
    if constexpr (PEN) {
        if (m < p.M) {
            const int brow = p.rowmap ? p.rowmap[m] : m;
            sbits = group_bits<CPP>(p.seen_mask + (size_t)brow * (p.N >> 5), g0);
            pp = p.penalty_of_row[brow];
        }
    }
    if constexpr (SOFT) {
        bool weigh = m < p.M;
        if constexpr (PEN) weigh = weigh && p.aut_state != nullptr;
        if (weigh) {
            const int s = p.aut_state[p.rowmap ? p.rowmap[m] : m];
            if (s >= 0) {
                float* const srow = const_cast<float*>(sC) + row * BN;
                const int e1 = p.edge_begin[s + 1];
                for (int lo = edge_lower_bound(p.edge_token, p.edge_begin[s], e1, g0); lo < e1; ++lo) {
                    const int tok = p.edge_token[lo];
                    if (tok >= g0 + CPP) break;
                    const float wgt = p.edge_weight[lo];
                    if (wgt != 0.f) srow[(tok - n0) ^ sw] += wgt;      // (as the target column: logical tok - n0 sits at physical (tok - n0) ^ sw)
                }
            }
        }
    }
    // the four bits of a float4 that starts at logical column n: one nibble of the group's bits (constants where the form has none)
    auto allowed4 = [&](int n) { return MASK ? (unsigned)(mbits >> (n - g0)) & 15u : 15u; };
    auto seen4 = [&](int n) { return PEN ? (unsigned)(sbits >> (n - g0)) & 15u : 0u; };
    Top4 top;
    if constexpr (TOPK) {
        topn_clear(top);
#pragma unroll 2        // (a short body keeps the registers of the 128 x 128 variants below EPI_ARGMAX_LSE's: DESIGN.md 4.5)
        for (int q = 0; q < CPP / 4; ++q) {
            const int pc = part * CPP + ((rot + 4 * q) % CPP);
            const float4 cv = *reinterpret_cast<const float4*>(&sC[row * BN + pc]);
            const int n = n0 + (pc ^ sw);
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + n);
            const unsigned nib = allowed4(n), snib = seen4(n);
            topn_insert(top, (nib & 1) ? lm_logit<PEN>(cv.x, bv.x, snib & 1, pp) : -INFINITY, (nib & 1) ? n : 0x7fffffff);
            topn_insert(top, (nib & 2) ? lm_logit<PEN>(cv.y, bv.y, snib & 2, pp) : -INFINITY, (nib & 2) ? n + 1 : 0x7fffffff);
            topn_insert(top, (nib & 4) ? lm_logit<PEN>(cv.z, bv.z, snib & 4, pp) : -INFINITY, (nib & 4) ? n + 2 : 0x7fffffff);
            topn_insert(top, (nib & 8) ? lm_logit<PEN>(cv.w, bv.w, snib & 8, pp) : -INFINITY, (nib & 8) ? n + 3 : 0x7fffffff);
        }
#pragma unroll
        for (int o = TPRW / 2; o > 0; o >>= 1) top4_merge_xor(top, o);
        best = top.v[0]; bi = top.i[0];
    } else {
#pragma unroll
        for (int q = 0; q < CPP / 4; ++q) {
            const int pc = part * CPP + ((rot + 4 * q) % CPP);          // physical column of this float4
            const float4 cv = *reinterpret_cast<const float4*>(&sC[row * BN + pc]);
            const int n = n0 + (pc ^ sw);                                // logical (global) column of cv.x
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + n);
            const unsigned nib = allowed4(n), snib = seen4(n);
            const float v[4] = {lm_logit<PEN>(cv.x, bv.x, snib & 1, pp), lm_logit<PEN>(cv.y, bv.y, snib & 2, pp),
                                lm_logit<PEN>(cv.z, bv.z, snib & 4, pp), lm_logit<PEN>(cv.w, bv.w, snib & 8, pp)};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (((nib >> e) & 1) && (v[e] > best || (v[e] == best && n + e < bi))) { best = v[e]; bi = n + e; }
        }
#pragma unroll
        for (int o = TPRW / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
    }
    float esum = 0.f;
    if constexpr (LSE) {
#pragma unroll
        for (int q = 0; q < CPP / 4; ++q) {
            const int pc = part * CPP + ((rot + 4 * q) % CPP);
            const float4 cv = *reinterpret_cast<const float4*>(&sC[row * BN + pc]);
            const int n = n0 + (pc ^ sw);
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + n);
            const unsigned nib = allowed4(n), snib = seen4(n);
            esum += (((nib & 1) ? __expf(lm_logit<PEN>(cv.x, bv.x, snib & 1, pp) - best) : 0.f) +
                     ((nib & 2) ? __expf(lm_logit<PEN>(cv.y, bv.y, snib & 2, pp) - best) : 0.f)) +
                    (((nib & 4) ? __expf(lm_logit<PEN>(cv.z, bv.z, snib & 4, pp) - best) : 0.f) +
                     ((nib & 8) ? __expf(lm_logit<PEN>(cv.w, bv.w, snib & 8, pp) - best) : 0.f));
        }
#pragma unroll
        for (int o = TPRW / 2; o > 0; o >>= 1) esum += __shfl_xor(esum, o, 64);
    }
    if constexpr (MASK && LSE && TGT) {
        if (m < p.M) {
            const int brow = p.rowmap ? p.rowmap[m] : m;
            const int t = p.step[m];
            if ((unsigned)t < (unsigned)p.prefix_len[brow]) {
                const int tgt = p.prefix[(size_t)brow * p.prefix_ld + t];
                if (tgt >= g0 && tgt < g0 + CPP) {          // (logical column tgt - n0 sits at physical column (tgt - n0) ^ sw)
                    const float v = lm_logit<PEN>(sC[row * BN + ((tgt - n0) ^ sw)], p.bias[tgt], (sbits >> (tgt - g0)) & 1ull, pp);
                    p.tgt_val[m] = ((mbits >> (tgt - g0)) & 1ull) ? v : -INFINITY;
                }
            }
        }
    }
    if (part == 0 && m < p.M) {
        const size_t c = (size_t)m * p.ntn + n0 / BN;
        reinterpret_cast<float*>(p.out)[c] = best;
        p.cand_idx[c] = bi;
        if constexpr (LSE) p.cand_sum[c] = esum;
        if constexpr (TOPK) {
            *reinterpret_cast<float4*>(p.top_val + 4 * c) = make_float4(top.v[0], top.v[1], top.v[2], top.v[3]);
            *reinterpret_cast<int4*>(p.top_idx + 4 * c) = make_int4(top.i[0], top.i[1], top.i[2], top.i[3]);
        }
    }
}

__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)p;
}

// s_waitcnt vmcnt(N) needs an immediate: N = DMA instructions that may stay in flight
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N == 0 || N == 4 || N == 6 || N == 8 || N == 12 || N == 16 || N == 20 || N == 22 || N == 24 || N == 63, "add the count");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if constexpr (N == 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else if constexpr (N == 22) asm volatile("s_waitcnt vmcnt(22)" ::: "memory");
    else if constexpr (N == 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
}

// NST = depth of the LDS ring: K-tile t+NST-1 is issued while K-tile t is multiplied.  NST = 2 is
// the plain double buffer; the latency-bound skinny GEMMs of the decode step use NST = 4 (64x64
// tile: 4 x 16 KiB) so a DMA has three K-tiles of time to land.
// TGT (EPI_ARGMAX_LSE_M / EPI_TOPK_M only): the epilogue also stores the forced prefixes' target column (GemmParams::tgt_val).
// SOFT (the three EPI_*_M forms only): the epilogue first adds the rows' automaton edge weights; the argument is a GemmParamsSoft.
// PEN (with SOFT): ... and applies the rows' repetition penalties to their seen columns; the argument is a GemmParamsPen.
template <typename T, int BM, int BN, int EPI, int NST = 2, bool TGT = false, bool SOFT = false, bool PEN = false>
__global__ __launch_bounds__(256) void gemm_kernel(std::conditional_t<PEN, GemmParamsPen, std::conditional_t<SOFT, GemmParamsSoft, GemmParams>> p) {
    static_assert(!SOFT || EPI == EPI_ARGMAX_M || EPI == EPI_ARGMAX_LSE_M || EPI == EPI_TOPK_M, "edge weights go into the masked LM head");
    static_assert(!PEN || SOFT, "the penalised LM head is the weighted one too");
    constexpr int TM = BM / 64, TN = BN / 64;          // 32x32 MFMA tiles per wave
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
    constexpr int LPT = (BM / 8 + BN / 8) / 4;         // DMA instructions per wave per K-tile
    static_assert(BM * BN * 4 <= NST * STAGE, "fp32 epilogue tile must fit the staging buffers");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r32 = lane & 31, hh = lane >> 5;

    // XCD-aware bijective remap of the linear block id (8 XCDs, round-robin dispatch)
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    int tn, tm;
    gemm_tile_of(p, bid, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = blockIdx.z * p.k_per_split;
    const int nt = p.k_per_split / (128 / (int)sizeof(T));

    const char* Ab = (const char*)p.A + ((size_t)m0 * p.lda + kbeg + (size_t)blockIdx.y * p.a_yoff) * sizeof(T);
    const char* Wb = (const char*)p.W + ((size_t)n0 * p.ldw + kbeg + (size_t)blockIdx.y * p.w_yoff) * sizeof(T);
    const size_t a_row = (size_t)p.lda * sizeof(T), w_row = (size_t)p.ldw * sizeof(T);

    // per-lane part of the staging addresses: lane -> (row within 8-row piece, physical chunk)
    const int prow = lane >> 3, pchunk = lane & 7;

    auto stage = [&](int t, int buf) {
        char* sa = smem + buf * STAGE;
        char* sb = sa + A_BYTES;
#pragma unroll
        for (int pc = wave; pc < BM / 8; pc += 4) {
            const int row = pc * 8 + prow;
            const int c = pchunk ^ ((row >> 1) & 7);
            glds16(Ab + (size_t)row * a_row + (size_t)t * 128 + c * 16, sa + pc * 1024);
        }
#pragma unroll
        for (int pc = wave; pc < BN / 8; pc += 4) {
            const int row = pc * 8 + prow;
            const int c = pchunk ^ ((row >> 1) & 7);
            glds16(Wb + (size_t)row * w_row + (size_t)t * 128 + c * 16, sb + pc * 1024);
        }
    };

    f32x16 acc[TM][TN];
    f32x4 acc16[2 * TM][2 * TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
        for (int j = 0; j < 2 * TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc16[i][j][r] = 0.f;

    int rowA[TM], rowB[TN], swA[TM], swB[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) { rowA[i] = wm * (BM / 2) + i * 32 + r32; swA[i] = (rowA[i] >> 1) & 7; }
#pragma unroll
    for (int j = 0; j < TN; ++j) { rowB[j] = wn * (BN / 2) + j * 32 + r32; swB[j] = (rowB[j] >> 1) & 7; }

#pragma unroll
    for (int i = 0; i < NST - 1; ++i)
        if (i < nt) stage(i, i);
    for (int t = 0; t < nt; ++t) {
        // tile t has landed: each wave waits for its own DMA, allowing the min(NST-2, nt-1-t) newer
        // tiles to stay in flight; the raw barrier (no vmcnt drain) covers the other waves' pieces
        // and tells that everyone has finished reading the slot tile t+NST-1 is about to overwrite
        const int newer = nt - 1 - t;
        if constexpr (NST == 2) {
            wait_vmcnt<0>();
        } else if constexpr (NST == 3) {
            if (newer >= 1) wait_vmcnt<LPT>(); else wait_vmcnt<0>();
        } else {
            static_assert(NST == 4, "ring depth");
            if (newer >= 2) wait_vmcnt<2 * LPT>(); else if (newer == 1) wait_vmcnt<LPT>(); else wait_vmcnt<0>();
        }
        // Also every LDS read this wave has issued must be BACK before the barrier: hipcc sinks the last MFMAs of the
        // previous K-tile (and the lgkmcnt wait for their fragments) below it, and behind the barrier the slot those
        // reads come from is handed to the DMA.  Under LDS contention (several blocks per CU) such a read has been seen
        // to lose that race (kernels_qqt.h, r01).
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + NST - 1 < nt) stage(t + NST - 1, (t + NST - 1) % NST);
        const char* sa = smem + (t % NST) * STAGE;
        const char* sb = sa + A_BYTES;
        if constexpr (sizeof(T) == 2 && MOCR_GEMM_MFMA16) {
            // 16x16x32 shape: the same LDS bytes per FLOP as 32x32x16, but the chip holds a higher clock
            // on it (MI355X_MICROARCH.md, DVFS give-back item 7)
            const int l15 = lane & 15, g4 = lane >> 4;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int c = 4 * s + g4;
                bf16x8 a[2 * TM], b[2 * TN];
#pragma unroll
                for (int i = 0; i < 2 * TM; ++i) {
                    const int row = wm * (BM / 2) + i * 16 + l15;
                    a[i] = *(const bf16x8*)(sa + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
                }
#pragma unroll
                for (int j = 0; j < 2 * TN; ++j) {
                    const int row = wn * (BN / 2) + j * 16 + l15;
                    b[j] = *(const bf16x8*)(sb + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
                    for (int j = 0; j < 2 * TN; ++j)
                        acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc16[i][j], 0, 0, 0);
            }
        } else if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int c = 2 * s + hh;
                bf16x8 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *(const bf16x8*)(sa + rowA[i] * 128 + ((c ^ swA[i]) << 4));
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *(const bf16x8*)(sb + rowB[j] * 128 + ((c ^ swB[j]) << 4));
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int k = 2 * s + hh;            // A[i=lane&31][k=lane>>5] of a 32x32x2 step
                const int c = k >> 2, o = (k & 3) * 4;
                float a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *(const float*)(sa + rowA[i] * 128 + ((c ^ swA[i]) << 4) + o);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *(const float*)(sb + rowB[j] * 128 + ((c ^ swB[j]) << 4) + o);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: accumulators -> LDS (fp32 [BM][BN]) -> fused epilogue -> 16-byte global stores
    __syncthreads();
    float* sC = reinterpret_cast<float*>(smem);
    constexpr bool SWZ = sizeof(T) == 2 && MOCR_GEMM_MFMA16;
    if constexpr (SWZ) {
#pragma unroll
        for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
            for (int j = 0; j < 2 * TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // C/D map of the 16x16 MFMA: col = lane&15, row = 4*(lane>>4) + r
                    const int row = wm * (BM / 2) + i * 16 + 4 * (lane >> 4) + r;
                    const int col = wn * (BN / 2) + j * 16 + (lane & 15);
                    sC[row * BN + (col ^ (((row >> 2) & 3) << 4))] = acc16[i][j][r];
                }
    } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
                const int row = wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                const int col = wn * (BN / 2) + j * 32 + r32;
                sC[row * BN + col] = acc[i][j][r];
            }
    }
    __syncthreads();

    if constexpr (epi_is_lm_head(EPI)) {
        gemm_epilogue_argmax<BM, BN, 256, SWZ, EPI, TGT, SOFT, PEN>(sC, p, m0, n0, tid);
    } else if constexpr (EPI == EPI_BIAS) {
        GemmParams q = p;
        q.out = reinterpret_cast<T*>(p.out) + (size_t)blockIdx.y * p.o_yoff;
        q.bias = p.bias + (size_t)blockIdx.y * p.b_yoff;
        gemm_epilogue<T, BM, BN, EPI, 256, SWZ>(sC, q, m0, n0, tid, blockIdx.z);
    } else {
        gemm_epilogue<T, BM, BN, EPI, 256, SWZ>(sC, p, m0, n0, tid, blockIdx.z);
    }
}

// ------------------------------------------------------------------------------------------------
// Fragment registers and LDS reads of the 256 x 256 encoder tile (gemm_pers_kernel, kernels_gemm_pers.h; also the r02
// kernel it replaced, kernels_gemm_lab.h): 8 waves as 2(M) x 4(N), a wave owns 128 x 64 = 8 x 4 tiles of
// v_mfma_f32_16x16x32_bf16 with SWAPPED operands (W fragment as A), one 32-deep k-step per K-tile: 12 ds_read_b128 for
// 32 MFMAs.  LDS image of a K-tile: 64-B rows, 16-B chunk c of row r at chunk c ^ 2*((r>>3)&1) (conflict-free for the
// four 16-lane groups of a ds_read_b128); one DMA piece = 1 KiB = 16 rows x 64 B, swizzle applied on the source address.
// ------------------------------------------------------------------------------------------------
struct WideFrags { bf16x8 fb[4]; bf16x8 fa[8]; };

// first six fragment reads of a K-tile (the four W fragments, then A fragments 0 and 1)
#define MOCR_W2_READ_HEAD(F, aA, aB)                                                                                    \
    asm volatile("ds_read_b128 %0, %7\n\tds_read_b128 %1, %7 offset:1024\n\tds_read_b128 %2, %7 offset:2048\n\t"        \
                 "ds_read_b128 %3, %7 offset:3072\n\tds_read_b128 %4, %6\n\tds_read_b128 %5, %6 offset:1024"             \
                 : "=&v"(F.fb[0]), "=&v"(F.fb[1]), "=&v"(F.fb[2]), "=&v"(F.fb[3]), "=&v"(F.fa[0]), "=&v"(F.fa[1])       \
                 : "v"(aA), "v"(aB)                                                                                      \
                 : "memory")
// the other six A fragments
#define MOCR_W2_READ_TAIL(F, aA)                                                                                        \
    asm volatile("ds_read_b128 %0, %6 offset:2048\n\tds_read_b128 %1, %6 offset:3072\n\tds_read_b128 %2, %6 offset:4096\n\t" \
                 "ds_read_b128 %3, %6 offset:5120\n\tds_read_b128 %4, %6 offset:6144\n\tds_read_b128 %5, %6 offset:7168" \
                 : "=&v"(F.fa[2]), "=&v"(F.fa[3]), "=&v"(F.fa[4]), "=&v"(F.fa[5]), "=&v"(F.fa[6]), "=&v"(F.fa[7])       \
                 : "v"(aA)                                                                                               \
                 : "memory")
// the same reads from the 64-deep image of gemm_pers_kernel's K64 form: 128-byte rows, fragments 2 KiB apart
#define MOCR_W2K_READ_HEAD(F, aA, aB)                                                                                   \
    asm volatile("ds_read_b128 %0, %7\n\tds_read_b128 %1, %7 offset:2048\n\tds_read_b128 %2, %7 offset:4096\n\t"        \
                 "ds_read_b128 %3, %7 offset:6144\n\tds_read_b128 %4, %6\n\tds_read_b128 %5, %6 offset:2048"             \
                 : "=&v"(F.fb[0]), "=&v"(F.fb[1]), "=&v"(F.fb[2]), "=&v"(F.fb[3]), "=&v"(F.fa[0]), "=&v"(F.fa[1])       \
                 : "v"(aA), "v"(aB)                                                                                      \
                 : "memory")
#define MOCR_W2K_READ_TAIL(F, aA)                                                                                       \
    asm volatile("ds_read_b128 %0, %6 offset:4096\n\tds_read_b128 %1, %6 offset:6144\n\tds_read_b128 %2, %6 offset:8192\n\t" \
                 "ds_read_b128 %3, %6 offset:10240\n\tds_read_b128 %4, %6 offset:12288\n\tds_read_b128 %5, %6 offset:14336" \
                 : "=&v"(F.fa[2]), "=&v"(F.fa[3]), "=&v"(F.fa[4]), "=&v"(F.fa[5]), "=&v"(F.fa[6]), "=&v"(F.fa[7])       \
                 : "v"(aA)                                                                                               \
                 : "memory")
// a half tile's wave (64 x 64, gemm_pers_kernel STRIP): A fragments 2 and 3 only
#define MOCR_W2_READ_TAIL2(F, aA)                                                                                       \
    asm volatile("ds_read_b128 %0, %2 offset:2048\n\tds_read_b128 %1, %2 offset:3072"                                   \
                 : "=&v"(F.fa[2]), "=&v"(F.fa[3])                                                                        \
                 : "v"(aA)                                                                                               \
                 : "memory")
#define MOCR_W2_GROUP(F, g)                                                                                             \
    _Pragma("unroll") for (int ii = 0; ii < 2; ++ii) _Pragma("unroll") for (int j = 0; j < 4; ++j)                        \
        acc[j][2 * (g) + ii] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F.fb[j], F.fa[2 * (g) + ii], acc[j][2 * (g) + ii], 0, 0, 0); \
    __builtin_amdgcn_sched_barrier(0)

