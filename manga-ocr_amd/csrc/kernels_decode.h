// Row-wise kernels of the greedy decode step (BERT decoder with post-LN residual blocks,
// TF/models/bert/modeling_bert.py:282-293, 340-351, 466-496; greedy loop TF/generation/utils.py:
// 2783-2973).  The skinny projections (M = batch) run as split-K GEMMs that leave fp32 partial
// slabs; every consumer below sums the slabs in a fixed order (deterministic, unlike float
// atomics), adds the bias and fuses the element-wise work that follows.
#pragma once
#include "common.h"
#include "token_rules.h"
#include <type_traits>

// out = LayerNorm( [gelu]( sum_s slab_s + bias ) [+ resid] ) ; writes fp32 (next residual) and T
// (next GEMM operand).  One block of D/4 threads per row, one float4 per thread; the slab loads
// are issued four at a time (independent accumulators) so the row costs ~nslab/4 memory round
// trips instead of nslab.
template <typename T, int D, bool GELU>
__global__ __launch_bounds__(D / 4) void dec_add_ln_kernel(const float* __restrict__ slabs, int nslab, long long slab_stride,
                                                           const float* __restrict__ bias, const float* __restrict__ resid,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ out_f32, T* __restrict__ out_t, int rows, float eps,
                                                           T* __restrict__ cache = nullptr, long long cache_batch_stride = 0,
                                                           const int* __restrict__ step = nullptr, uint8_t* __restrict__ cache8 = nullptr,
                                                           float inv_sx8 = 0.f, const int* __restrict__ rowmap = nullptr) {
    constexpr int NW = D / 256;                      // waves per block
    __shared__ float s_red[2][NW];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = tid * 4;
    const float* sp = slabs + (size_t)row * D + c;
    const float4 bv = *reinterpret_cast<const float4*>(bias + c);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (resid) r = *reinterpret_cast<const float4*>(resid + (size_t)row * D + c);
    // eight slab loads in flight at a time; indices past nslab are clamped (a valid, cached
    // address) and weighted 0 - a per-load branch would serialise the loads
    float v[4] = {bv.x, bv.y, bv.z, bv.w};
    for (int s0 = 0; s0 < nslab; s0 += 8) {
        float4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const float4*>(sp + (size_t)min(s0 + u, nslab - 1) * slab_stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float w = (s0 + u < nslab) ? 1.f : 0.f;
            v[0] += w * x[u].x; v[1] += w * x[u].y; v[2] += w * x[u].z; v[3] += w * x[u].w;
        }
    }
    if (GELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_for<T>(v[e]);
    }
    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
    float sm = wave_sum((v[0] + v[1]) + (v[2] + v[3]));
    if (lane == 0) s_red[0][wave] = sm;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += s_red[0][w];
    const float mean = tot * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float d = v[e] - mean; q += d * d; }
    q = wave_sum(q);
    if (lane == 0) s_red[1][wave] = q;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += s_red[1][w];
    const float rstd = 1.0f / sqrtf(tot * (1.0f / D) + eps);
    const float4 g = *reinterpret_cast<const float4*>(gamma + c);
    const float4 b = *reinterpret_cast<const float4*>(beta + c);
    float o[4] = {(v[0] - mean) * rstd * g.x + b.x, (v[1] - mean) * rstd * g.y + b.y, (v[2] - mean) * rstd * g.z + b.z,
                  (v[3] - mean) * rstd * g.w + b.w};
    if (out_f32) *reinterpret_cast<float4*>(out_f32 + (size_t)row * D + c) = make_float4(o[0], o[1], o[2], o[3]);
    elem<T>::st4(out_t + (size_t)row * D + c, o);
    // latent attention: this row is also the key/value source of position step[row] for the next layer
    const int crow = rowmap ? rowmap[row] : row;     // the per-row caches stay where the row started (compacted batches)
    if (cache) elem<T>::st4(cache + (size_t)crow * cache_batch_stride + (size_t)step[row] * D + c, o);
    // fp8 attention mode: the same row as e4m3 bytes with the cache's static scale (kernels_latent8.h)
    if (cache8)
        *reinterpret_cast<unsigned*>(cache8 + (size_t)crow * cache_batch_stride + (size_t)step[row] * D + c) =
            pack4_fp8(o[0] * inv_sx8, o[1] * inv_sx8, o[2] * inv_sx8, o[3] * inv_sx8);
}

// out T = gelu( sum_s slab_s + bias )   (the decoder FFN's intermediate activation)
template <typename T>
__global__ void dec_bias_gelu_kernel(const float* __restrict__ slabs, int nslab, long long slab_stride,
                                     const float* __restrict__ bias, T* __restrict__ out, int rows, int N) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= (long long)rows * N) return;
    const int c = (int)(i % N);
    float4 a0 = *reinterpret_cast<const float4*>(bias + c);
    float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = 0;
    for (; s + 2 <= nslab; s += 2) {
        const float4 x0 = *reinterpret_cast<const float4*>(slabs + (size_t)s * slab_stride + i);
        const float4 x1 = *reinterpret_cast<const float4*>(slabs + (size_t)(s + 1) * slab_stride + i);
        a0.x += x0.x; a0.y += x0.y; a0.z += x0.z; a0.w += x0.w;
        a1.x += x1.x; a1.y += x1.y; a1.z += x1.z; a1.w += x1.w;
    }
    if (s < nslab) {
        const float4 x0 = *reinterpret_cast<const float4*>(slabs + (size_t)s * slab_stride + i);
        a0.x += x0.x; a0.y += x0.y; a0.z += x0.z; a0.w += x0.w;
    }
    float o[4] = {gelu_for<T>(a0.x + a1.x), gelu_for<T>(a0.y + a1.y), gelu_for<T>(a0.z + a1.z), gelu_for<T>(a0.w + a1.w)};
    elem<T>::st4(out + i, o);
}

// Per-sequence decode state, all device resident so a decode step is a fixed launch sequence
// (replayable as a HIP graph): no host value changes from step to step.
struct DecState {
    int* ids;          // [B][max_len] int32 output rows (ids[b][0] = start_id)
    int* step;         // [B] position of the token being consumed
    int* finished;     // [B]
    int* len;          // [B] tokens in the row incl. start and EOS
    int* n_unfinished; // [1]
    const int* forced; // [B][forced_T] teacher-forced inputs (test hook) or null
    int forced_T;
    float* logits_out; // [B][forced_T][V] (test hook) or null
    int ids_ld;        // row stride of ids
    int max_len;       // generate(max_length): a row is finished when it holds max_len tokens
    int start_id, eos_id, pad_id;
    int n_real;        // rows >= n_real are padding (the batch is rounded up to a graph-friendly row count): born finished
    // Decode SLOT -> ROW of the batch (r04).  ids / finished / len and the per-row key/value caches are indexed by row and
    // never move; the activations of a step (x, slabs, ...) and `step` are indexed by slot.  Identity from the start token
    // on; compact_rows (engine.hip) rewrites it so that the unfinished rows occupy the first slots and the decode steps
    // can run on fewer of them - a finished row stops costing, as in the reference, where every crop is its own
    // generate() call (TF/generation/utils.py:2929-2937, src/core/workers.py:213-225).
    int* rowmap;
    // Token scores (nullable): [B][ids_ld] float32, by row like ids.  scores[row][t + 1] = log-probability of ids[row][t + 1]
    // (fp32 log-softmax of the step's LM-head logits at the chosen token), 0 for a finished row's pad ids.
    float* scores;
    // Token alternatives (nullable, both or neither; need scores): [B][ids_ld][4] int32 / float32, by row like ids.
    // alt_ids[row][t + 1][k] = the token with the k-th largest logit of the step that chose ids[row][t + 1] (equal logits: the
    // lower id first - the greedy pick's order, so entry 0 is that id), alt_logp its fp32 log-softmax; -1 / 0 for a finished row.
    int* alt_ids;
    float* alt_logp;
    // Token constraints (nullable, both or neither): tok_mask [sets][V / 32], bit v of a set's row = token v may be emitted
    // (set 0: every token; EOS is in every set), and set_of_row [B], the set of every row - by ROW like ids, so a compaction
    // moves nothing.  A token outside its row's set counts as a logit of -inf in the argmax, the softmax and the alternatives.
    const unsigned* tok_mask;
    const int* set_of_row;
    // No-repeat n-grams (nullable, all four or none): row_mask [B][V / 32], the EFFECTIVE set of every row's next step = its
    // base set base_mask[base_set_of_row[row]] minus the tokens that would complete an n-gram the row already holds
    // (n = ngram_of_row[row], 0: off).  All by ROW like ids.  Such a state has tok_mask = row_mask and set_of_row = the
    // identity, so the LM head and the MASK code of the token kernel read a row's own mask; ngram_init_kernel fills it at the
    // start of a batch and the NGRAM token kernel rebuilds it after every token.
    unsigned* row_mask;
    const unsigned* base_mask;
    const int* base_set_of_row;
    const int* ngram_of_row;
    // Forced prefixes (nullable, all or none; honoured by the SCORES && MASK kernels - the engine runs such a batch in that
    // mode): prefix [B][prefix_ld] / prefix_len [B] by ROW like ids, the caller-given tokens behind the start token.  The
    // step that fills ids[row][t + 1] with t < prefix_len[row] stores prefix[row][t] instead of its arg-max.  tgt_val [B] by
    // SLOT: the LM head's value of that column (candidate path; GemmParams::tgt_val).
    const int* prefix;
    const int* prefix_len;
    int prefix_ld;
    const float* tgt_val;
};

// Token automata: the last argument of dec_token_kernel, read by its AUTOMATON form only (all six pointers set, and the
// state has the four n-gram pointers) - a trailing argument, so that every other form keeps the argument block it had.  The
// engine's tables in CSR form over GLOBAL state numbers - edge_begin [states + 1], edge_token / edge_next [edges] (a state's
// tokens strictly ascending, never EOS), accepting [states] - and by ROW like ids base_of_row [B], the global number of the
// row's start state (-1: the row brings no automaton), and state [B], the state the row is in (global; AUT_STATE_DEAD once
// a stored token had no edge).  automaton_init_kernel sets a row's state and first mask, the AUTOMATON token kernel walks the
// state and rebuilds the mask after every token.
struct DecAutomata {
    const int* edge_begin;
    const int* edge_token;
    const int* edge_next;
    const uint8_t* accepting;
    const int* base_of_row;
    int* state;
};

constexpr int AUT_STATE_NONE = -1, AUT_STATE_DEAD = -2;     // = MOCR_STATE_NONE / MOCR_STATE_DEAD (mocr.h)
constexpr int AUT_DEFAULT_FALLBACK = 1 << 30;               // = MOCR_DEFAULT_FALLBACK: a bit of a default_next value
constexpr int AUT_DEFAULT_STATE = AUT_DEFAULT_FALLBACK - 1; // ... and the bits of its state

// Soft token automata (mocr.h, "soft token automata"): the argument of dec_token_kernel's SOFT form in the place of DecAutomata -
// the same six pointers plus the two arena arrays a soft batch reads: edge_weight [edges], the fp32 bias an edge adds to its
// token's logit (0 for every automaton created without weights), and default_next [states], where an OPEN state sends a
// token without an edge (global; -1: the state is closed).  Only the SOFT instantiations take this type, so every other form
// keeps the argument block it had.
struct DecSoftAutomata : DecAutomata {
    const float* edge_weight;
    const int* default_next;
};

// Repetition penalty (mocr.h, "repetition penalty"): what dec_token_kernel's PEN form takes behind the automaton tables - by ROW
// like ids, so a compaction moves nothing: seen_mask [B][V / 32], bit v = token v is in the row (the start token, forced prefix
// tokens, chosen tokens; penalty_init_kernel sets the start bit, the PEN token kernel every stored token's), and
// penalty_of_row [B], finite and > 0, 1 = off.
struct DecPenalty {
    unsigned* seen_mask;
    const float* penalty_of_row;
};

// ... and the argument of the PEN form in the place of DecSoftAutomata: its eight pointers, which may all be null here (a
// penalty without any automaton), with the DecPenalty trailing.  Only the PEN instantiations take this type.
struct DecPenAutomata : DecSoftAutomata {
    DecPenalty pen;
};

// End of a decode step, one block per sequence:
//   logits = sum_s slab_s + bias  -> fp32 argmax (lowest index wins ties, like torch.argmax)
//   finished rows emit pad_id (utils.py:2929); EOS or reaching max_len finishes a row (:2936)
//   then the NEXT step's input embedding: LN(word[tok] + type[0] + pos[t+1])  (modeling_bert.py:98-106)
// FIRST = true: no logits yet; emits the start token's embedding at position 0.
// SCORES = true (st.scores set): also the log-probability of the arg-max token, logit_max - logsumexp(logits) = -log S with
//   S = sum_j exp(logit_j - max) >= 1, in fp32.  Candidate path: the LM head left cand_sum[c] = sum over tile c of
//   exp(logit - cand_val[c]) (EPI_ARGMAX_LSE), so S = sum_c cand_sum[c] * exp(cand_val[c] - max).  Slab path: the summed
//   logits are in this block's registers.  Either way a second short pass once the block knows the max.
// TOPK = true (st.alt_ids / st.alt_logp set; implies SCORES): also the row's four best logits.  Candidate path: the LM head
//   left every tile's four best (EPI_TOPK: top_val / top_idx [n][ncand][4]) and the top four of a row are the top four of
//   the union of its tiles' top fours; slab path: from the 24 logits a thread holds.  A thread-local sorted list (Top4,
//   kernels_gemm.h), merged across the wave by shuffles and across the four waves through LDS.  Entry k scores
//   (val_k - max) - log S; entry 0 is written as the score itself, -log S (0 - log S would lose the sign of a -0 score).
// MASK = true (st.tok_mask / st.set_of_row set): the row's allowed-token set applies.  Candidate path: the LM head (EPI_*_M)
//   already left out the other columns; a tile with none comes as (-inf, index sentinel, sum 0), wins no comparison, adds
//   0 * exp(-inf - max) = 0 to S and its unfilled list entries (-inf, sentinel) never enter a list.  Slab path: the thread's 24
//   summed logits take -inf where the set's bit is clear (one nibble of one word per float4), before the argmax; in the
//   alternatives they carry the index sentinel too.  EOS is in every set, so the row's max is finite; a set of fewer than
//   four tokens leaves (-inf, sentinel) entries, written as id -1 / log-probability -inf.
// NGRAM = true (st.row_mask / base_mask / base_set_of_row / ngram_of_row set; implies MASK): no_repeat_ngram_size of
//   transformers' NoRepeatNGramLogitsProcessor under greedy search.  The step's own masking is the MASK code above, on
//   st.tok_mask = st.row_mask through the identity st.set_of_row.  Once thread 0 has stored the token, the row holds
//   L = t + 2 tokens and the block rebuilds row_mask[row] for the step that will choose ids[L]: the 192 words of the base set
//   go to LDS, the threads split the windows i = 0 .. L - n, a window whose n - 1 key tokens equal the row's last n - 1
//   clears the bit of its follower ids[i + n - 1] (LDS atomic AND), and the words go back with plain vector stores.  n = 1
//   has an empty key: every token of the row is banned.  L + 1 < n (and L + 1 = n) has no window: the base set is written.
//   A finished row and a row with n = 0 (its mask is its base set since ngram_init_kernel) skip all of it.  An unfinished
//   row's history never holds EOS, so EOS is never banned and the row's max stays finite.
//   Slab path: every read of the row's mask for THIS step (the nibbles above) precedes the argmax reduction's
//   __syncthreads, and the rewrite follows the barrier behind thread 0's token, so no thread reads a word already rewritten.
// Forced prefixes (SCORES && MASK, st.prefix set): a step t < prefix_len[row] runs like any other - the same max, S and
//   alternatives - but thread 0 stores, finishes on and feeds back prefix[row][t].  Its score is (v - gmax) + (-log S), v the
//   forced column's masked logit: tgt_val[slot] on the candidate path, published through LDS by the thread that holds the
//   column on the slab path (before the argmax reduction's barrier).  A token outside the effective set has v = -inf and
//   scores -inf; a forced token that IS the arg-max takes the free step's expression (a -0 score keeps its sign).
// AUTOMATON = true (the six pointers of `aut` set; implies NGRAM): rows decode under token automata (mocr.h, "token
//   automata").  The step's own masking is again the MASK code on st.row_mask.  Behind the barrier that follows thread 0's
//   token, a row that brings an automaton and was unfinished before the step
//   1. walks: unless the token is EOS, the threads stride over the old state's edges and the one that holds the token (a
//      state's tokens are distinct: at most one thread) publishes its target through LDS; no match, or a dead state: DEAD;
//   2. if the row is still unfinished, rebuilds row_mask[row]: zero the LDS words, OR in the bits of the new state's edge
//      tokens (LDS atomics) and EOS if it accepts, AND the base set's words, apply the n-gram windows as above, and if a
//      block-wide OR finds no bit left, the dead-end rule: the mask becomes {EOS}.  The words go back with vector stores;
//   3. thread 0 stores the new state.  Every thread read the old state before the barrier of step 1 or 2 that precedes it.
//   A row without an automaton takes the NGRAM path; a row that was finished before the step touches neither mask nor state.
// SOFT = true (the eight pointers of `aut`, a DecSoftAutomata; implies AUTOMATON): soft token automata.  Three things differ.
//   Slab path: before the masking, a thread adds the weights of the row's state's edges that fall into its 24 columns - per
//   float4 one binary search in the state's ascending tokens - so the argmax, the exp sum, the alternatives and the forced
//   column's value see logit + weight; the read of the row's state precedes the argmax reduction's barrier like the mask
//   reads.  (Candidate path: the LM head's SOFT form has already added them.)  Walk: a token without an edge moves the row to
//   default_next[state], DEAD only where that is -1; where the value carries AUT_DEFAULT_FALLBACK, the token is walked from
//   the default state - to the target of that state's edge on it, if it has one (one more scan and barrier).  Mask rebuild: an open state starts from all ones, EOS by `accepting`,
//   instead of zero plus the OR of the edge bits.  Rows under a hard automaton read weight 0 / default -1 and do what the
//   AUTOMATON form does.
// PEN = true (`aut` is a DecPenAutomata; implies SOFT): transformers' repetition_penalty under greedy search, per row.  Slab
//   path: after the SOFT addition and before the MASK select a thread takes pen_logit(v, p) (common.h) of each of its 24
//   logits whose bit is set in seen_mask[row] - one nibble of one word per float4 - so the argmax, the exp sum, the
//   alternatives and the forced column's value see the penalised logits; logits_out has been stored before and stays raw.
//   (Candidate path: the LM head's PEN form has already applied it.)  Both paths: once thread 0 has stored the token of a row
//   that was unfinished before the step, chosen or forced, it sets the token's bit - a plain load, OR and vector store by the
//   row's one writer; the next reader is the next step's LM head or token kernel, a later launch.  Every read of the row's
//   seen words for THIS step precedes the argmax reduction's barrier, the write follows it: the n-gram mask's argument.  A row
//   finished before the step writes nothing.  The automaton pointers may be null: then no row has a state or a start state.
template <typename T, int D, bool FIRST, bool SCORES = false, bool TOPK = false, bool MASK = false, bool NGRAM = false,
          bool AUTOMATON = false, bool SOFT = false, bool PEN = false>
__global__ __launch_bounds__(256) void dec_token_kernel(const float* __restrict__ slabs, int nslab, long long slab_stride,
                                                        const float* __restrict__ vbias, int V,
                                                        DecState st,
                                                        const float* __restrict__ word, const float* __restrict__ type0,
                                                        const float* __restrict__ pos, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ x_f32,
                                                        T* __restrict__ x_t, float eps, T* __restrict__ cache = nullptr,
                                                        long long cache_batch_stride = 0,
                                                        const float* __restrict__ cand_val = nullptr,
                                                        const int* __restrict__ cand_idx = nullptr, int ncand = 0,
                                                        uint8_t* __restrict__ cache8 = nullptr, float inv_sx8 = 0.f,
                                                        const float* __restrict__ cand_sum = nullptr,
                                                        const float* __restrict__ top_val = nullptr,
                                                        const int* __restrict__ top_idx = nullptr,
                                                        std::conditional_t<PEN, DecPenAutomata, std::conditional_t<SOFT, DecSoftAutomata, DecAutomata>> aut = {}) {
    static_assert(!TOPK || (SCORES && !FIRST), "alternatives come with scores, from the second token on");
    static_assert(!MASK || !FIRST, "the start token is not constrained");
    static_assert(!NGRAM || MASK, "the n-gram bans are applied through the row's mask");
    static_assert(!AUTOMATON || NGRAM, "an automaton's sets are applied through the row's mask");
    static_assert(!SOFT || AUTOMATON, "weights and default edges belong to an automaton");
    static_assert(!PEN || SOFT, "the penalty form is the soft one too");
    constexpr int MW = 192;                             // mask words of a row (vocab 6144)
    __shared__ __attribute__((aligned(16))) unsigned s_mask[NGRAM ? MW : 4];
    __shared__ int s_ng, s_L;                           // NGRAM: the row's n (0: leave the mask alone) and its token count
    __shared__ int s_abase, s_awalk, s_alive, s_anext;  // AUTOMATON: the row's start state (-1: none or finished before), whether the
                                                        // stored token moves the state, whether the mask is rebuilt, the edge's target
    __shared__ int s_afall;                             // SOFT: the target of the default state's edge (MOCR_DEFAULT_FALLBACK)
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    __shared__ float s_red[4];
    __shared__ int s_tok, s_pos;
    __shared__ float s_fv;                              // forced prefixes, slab path: the forced column's masked logit
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = FIRST ? b : st.rowmap[b];       // slot b decodes row `row` of the batch
    if (FIRST) {
        if (tid == 0) {
            st.rowmap[b] = b;
            st.ids[(size_t)b * st.ids_ld] = st.start_id;
            st.step[b] = 0; st.finished[b] = b >= st.n_real ? 1 : 0; st.len[b] = st.max_len;
            s_tok = st.start_id; s_pos = 0;
            if (b == 0) *st.n_unfinished = st.n_real;
        }
    } else {
        const int t = st.step[b];
        int ftok = -1;                                   // the step's forced token (block-uniform), -1: a free step
        if constexpr (SCORES && MASK) {
            if (st.prefix && (unsigned)t < (unsigned)st.prefix_len[row]) ftok = st.prefix[(size_t)row * st.prefix_ld + t];
        }
        float best = -INFINITY;
        int bi = 0x7fffffff;
        constexpr int NC = 6;                            // vocab = NC * 1024 columns (6144)
        float4 a[NC];
        unsigned abits = 0xffffffu;                      // MASK, slab path: bit 4 j + e = the thread's logit a[j].e is allowed
        if (cand_val) {
            // the LM-head GEMM already reduced every 64/128-column tile (EPI_ARGMAX): ncand candidates per row
            for (int c = tid; c < ncand; c += 256) {
                const float cv = cand_val[(size_t)b * ncand + c];
                const int ci = cand_idx[(size_t)b * ncand + c];
                if (cv > best || (cv == best && ci < bi)) { best = cv; bi = ci; }
            }
        } else {
        int se0 = 0, se1 = 0;                            // SOFT: the edge range of the row's state (empty: NONE or DEAD)
        if constexpr (SOFT) {
            bool has = true;                             // PEN: the automaton pointers may be null
            if constexpr (PEN) has = aut.state != nullptr;
            if (has) {
                const int sst = aut.state[row];
                if (sst >= 0) { se0 = aut.edge_begin[sst]; se1 = aut.edge_begin[sst + 1]; }
            }
        }
        sum_slab_row(a, vbias, slabs, nslab, slab_stride, b, V, tid);
        float pp = 1.f;                                  // PEN: the row's penalty and its seen words
        const unsigned* seen = nullptr;
        if constexpr (PEN) { pp = aut.pen.penalty_of_row[row]; seen = aut.pen.seen_mask + (size_t)row * (V >> 5); }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = tid * 4 + j * 1024;
            if (st.logits_out)
                *reinterpret_cast<float4*>(st.logits_out + ((size_t)b * st.forced_T + t) * V + c) = a[j];
            if constexpr (SOFT) {
                add_edge_weights4(a[j], aut.edge_token, aut.edge_weight, se0, se1, c);
            }
            if constexpr (PEN) {
                const unsigned snib = (seen[c >> 5] >> (c & 31)) & 15u;
                if (snib & 1) a[j].x = pen_logit(a[j].x, pp);
                if (snib & 2) a[j].y = pen_logit(a[j].y, pp);
                if (snib & 4) a[j].z = pen_logit(a[j].z, pp);
                if (snib & 8) a[j].w = pen_logit(a[j].w, pp);
            }
            if constexpr (MASK) {
                const unsigned nib = (st.tok_mask[(size_t)st.set_of_row[row] * (V >> 5) + (c >> 5)] >> (c & 31)) & 15u;
                if (j == 0) abits = 0;
                abits |= nib << (4 * j);
                a[j].x = (nib & 1) ? a[j].x : -INFINITY; a[j].y = (nib & 2) ? a[j].y : -INFINITY;
                a[j].z = (nib & 4) ? a[j].z : -INFINITY; a[j].w = (nib & 8) ? a[j].w : -INFINITY;
                if constexpr (SCORES) {
                    if ((ftok & ~3) == c) s_fv = (ftok & 2) ? ((ftok & 1) ? a[j].w : a[j].z) : ((ftok & 1) ? a[j].y : a[j].x);
                }
            }
            if (a[j].x > best) { best = a[j].x; bi = c; }
            if (a[j].y > best) { best = a[j].y; bi = c + 1; }
            if (a[j].z > best) { best = a[j].z; bi = c + 2; }
            if (a[j].w > best) { best = a[j].w; bi = c + 3; }
        }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; }
        __syncthreads();
        if constexpr (SCORES) {
            const float gmax = fmaxf(fmaxf(s_val[0], s_val[1]), fmaxf(s_val[2], s_val[3]));     // = the winner's logit
            float es = 0.f;
            if (cand_val) {
                for (int c = tid; c < ncand; c += 256)
                    es += cand_sum[(size_t)b * ncand + c] * __expf(cand_val[(size_t)b * ncand + c] - gmax);
            } else {
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    es += (__expf(a[j].x - gmax) + __expf(a[j].y - gmax)) + (__expf(a[j].z - gmax) + __expf(a[j].w - gmax));
            }
            es = wave_sum(es);
            if (lane == 0) s_red[wave] = es;             // (s_red is free until the embedding's LayerNorm below)
            __syncthreads();
        }
        Top4 top;
        if constexpr (TOPK) {
            __shared__ float s_tv[4][4];
            __shared__ int s_ti[4][4];
            topn_clear(top);
            if (cand_val) {
                for (int c = tid; c < ncand; c += 256) {
                    const float4 tv = *reinterpret_cast<const float4*>(top_val + ((size_t)b * ncand + c) * 4);
                    const int4 ti = *reinterpret_cast<const int4*>(top_idx + ((size_t)b * ncand + c) * 4);
                    topn_insert(top, tv.x, ti.x); topn_insert(top, tv.y, ti.y);
                    topn_insert(top, tv.z, ti.z); topn_insert(top, tv.w, ti.w);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    const int c = tid * 4 + j * 1024;
                    if constexpr (MASK) {
                        const unsigned nib = abits >> (4 * j);
                        topn_insert(top, a[j].x, (nib & 1) ? c : 0x7fffffff); topn_insert(top, a[j].y, (nib & 2) ? c + 1 : 0x7fffffff);
                        topn_insert(top, a[j].z, (nib & 4) ? c + 2 : 0x7fffffff); topn_insert(top, a[j].w, (nib & 8) ? c + 3 : 0x7fffffff);
                    } else {
                    topn_insert(top, a[j].x, c); topn_insert(top, a[j].y, c + 1);
                    topn_insert(top, a[j].z, c + 2); topn_insert(top, a[j].w, c + 3);
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) top4_merge_xor(top, o);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { s_tv[wave][k] = top.v[k]; s_ti[wave][k] = top.i[k]; }
            }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < 4; ++w)
#pragma unroll
                    for (int k = 0; k < 4; ++k) topn_insert(top, s_tv[w][k], s_ti[w][k]);
            }
        }
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (s_val[w] > best || (s_val[w] == best && s_idx[w] < bi)) { best = s_val[w]; bi = s_idx[w]; }
            if ((unsigned)bi >= (unsigned)V) bi = 0;      // all-NaN logits win no comparison: stay inside the embedding table
            int fin = st.finished[row];
            int tok = fin ? st.pad_id : bi;
            if (st.forced) tok = (t + 1 < st.forced_T) ? st.forced[(size_t)b * st.forced_T + t + 1] : st.pad_id;
            const bool force = ftok >= 0 && !fin;
            if (force) tok = ftok;
            if (t + 1 < st.ids_ld) st.ids[(size_t)row * st.ids_ld + t + 1] = tok;
            if constexpr (PEN) {                         // the stored token is in the row from the next step on
                if (!fin && t + 1 < st.ids_ld && (unsigned)tok < (unsigned)V) {
                    unsigned* const sw = aut.pen.seen_mask + (size_t)row * (V >> 5) + (tok >> 5);
                    *sw = *sw | (1u << (tok & 31));
                }
            }
            if constexpr (SCORES) {
                const float S = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
                const float score = -logf(S);
                float tscore = score;                    // the stored token's: a forced one that is not the step's pick scores its own logit
                if constexpr (MASK) {
                    if (force && ftok != bi) tscore = ((cand_val ? st.tgt_val[b] : s_fv) - best) + score;
                }
                if (t + 1 < st.ids_ld) st.scores[(size_t)row * st.ids_ld + t + 1] = fin ? 0.f : tscore;
                if constexpr (TOPK) {
                    if (t + 1 < st.ids_ld) {
                        const size_t o = ((size_t)row * st.ids_ld + t + 1) * 4;
                        int4 ai = make_int4(-1, -1, -1, -1);
                        float4 al = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (!fin) {
                            const float gmax = top.v[0];
                            ai = make_int4((unsigned)top.i[0] < (unsigned)V ? top.i[0] : -1, (unsigned)top.i[1] < (unsigned)V ? top.i[1] : -1,
                                           (unsigned)top.i[2] < (unsigned)V ? top.i[2] : -1, (unsigned)top.i[3] < (unsigned)V ? top.i[3] : -1);
                            al = make_float4(score, (top.v[1] - gmax) + score, (top.v[2] - gmax) + score, (top.v[3] - gmax) + score);
                        }
                        *reinterpret_cast<int4*>(st.alt_ids + o) = ai;
                        *reinterpret_cast<float4*>(st.alt_logp + o) = al;
                    }
                }
            }
            if (!fin && !st.forced && (tok == st.eos_id || t + 2 >= st.max_len)) {
                st.finished[row] = 1;
                st.len[row] = t + 2;
                atomicSub(st.n_unfinished, 1);
            }
            st.step[b] = t + 1;
            s_tok = tok; s_pos = t + 1;
            if constexpr (NGRAM) {
                // (a row that is or has just become finished keeps its mask: nothing reads it again; V != 32 MW or a token
                // the row's stride did not take: no rebuild either)
                const bool live = !fin && !st.finished[row] && t + 2 <= st.ids_ld && V == 32 * MW;
                s_ng = live ? st.ngram_of_row[row] : 0;
                s_L = t + 2;
                if constexpr (AUTOMATON) {
                    bool none = fin != 0;                // PEN: the automaton pointers may be null
                    if constexpr (PEN) none = none || aut.base_of_row == nullptr;
                    s_abase = none ? -1 : aut.base_of_row[row];
                    s_awalk = tok != st.eos_id;
                    s_alive = live;
                    s_anext = AUT_STATE_DEAD;
                    if constexpr (SOFT) s_afall = AUT_STATE_DEAD;
                }
            }
        }
    }
    __syncthreads();
    bool plain = true;                                  // the row rebuilds its mask the NGRAM way (or not at all)
    if constexpr (AUTOMATON) {
        const int abase = s_abase;                      // block-uniform, like everything read from LDS here
        if (abase >= 0) {
            plain = false;
            const int n = s_ng, L = s_L, tok = s_tok;
            const bool walk = s_awalk != 0, live = s_alive != 0;
            int state = aut.state[row];              // (thread 0 stores the new one behind at least one more barrier)
            if (walk) {
                if (state >= 0) {
                    const int e1 = aut.edge_begin[state + 1];
                    for (int i = aut.edge_begin[state] + tid; i < e1; i += 256)
                        if (aut.edge_token[i] == tok) s_anext = aut.edge_next[i];
                }
                __syncthreads();
                const int old = state;
                state = s_anext;
                if constexpr (SOFT) {                   // (an edge's target is >= 0: DEAD here means no edge)
                    const int dn = state == AUT_STATE_DEAD && old >= 0 ? aut.default_next[old] : -1;    // block-uniform
                    if (dn >= 0) {
                        state = dn & AUT_DEFAULT_STATE;
                        if (dn & AUT_DEFAULT_FALLBACK) {    // the token is walked from the default state: its edge, if it has one
                            // (a word of its own: a thread may still be reading s_anext above)
                            const int f1 = aut.edge_begin[state + 1];
                            for (int i = aut.edge_begin[state] + tid; i < f1; i += 256)
                                if (aut.edge_token[i] == tok) s_afall = aut.edge_next[i];
                            __syncthreads();
                            if (s_afall >= 0) state = s_afall;
                        }
                    }
                }
            }
            if (live) {
                bool open = false;                      // SOFT: the new state allows every token, EOS iff it accepts
                if constexpr (SOFT) open = state >= 0 && aut.default_next[state] >= 0;
                state_mask_to_lds(s_mask, state, open, aut.edge_begin, aut.edge_token, aut.accepting, st.eos_id, V, MW, tid, 256);
                if (tid < MW) s_mask[tid] &= st.base_mask[(size_t)st.base_set_of_row[row] * MW + tid];
                __syncthreads();
                if (n > 0) ngram_ban_windows(s_mask, st.ids + (size_t)row * st.ids_ld, L, n, V, tid);
                __syncthreads();
                // the dead-end rule
                const int any = __syncthreads_or(tid < MW && s_mask[tid] != 0u);
                if (!any && tid == 0 && (unsigned)st.eos_id < (unsigned)V) s_mask[st.eos_id >> 5] = 1u << (st.eos_id & 31);
                __syncthreads();
                if (tid < MW / 4)
                    reinterpret_cast<uint4*>(st.row_mask + (size_t)row * MW)[tid] = reinterpret_cast<const uint4*>(s_mask)[tid];
            }
            if (tid == 0 && walk) aut.state[row] = state;
        }
    }
    if constexpr (NGRAM) {
        const int n = s_ng, L = s_L;                    // block-uniform
        if (plain && n > 0) {
            const int* rid = st.ids + (size_t)row * st.ids_ld;      // ids[row][0 .. L - 1], the last one stored before the barrier
            if (tid < MW) s_mask[tid] = st.base_mask[(size_t)st.base_set_of_row[row] * MW + tid];
            __syncthreads();
            ngram_ban_windows(s_mask, rid, L, n, V, tid);
            __syncthreads();
            if (tid < MW / 4)
                reinterpret_cast<uint4*>(st.row_mask + (size_t)row * MW)[tid] = reinterpret_cast<const uint4*>(s_mask)[tid];
        }
    }
    const int tok = s_tok, ps = s_pos;
    // the next input: embedding + LayerNorm, to x and the layer-0 key/value source
    embed_ln_store<T, D>(tok, ps, b, row, word, type0, pos, gamma, beta, x_f32, x_t, eps, cache, cache_batch_stride, cache8, inv_sx8, s_red, tid);
}

// Start of a batch with no-repeat n-grams, one block of 192 threads per row: row_mask[row] = the row's base set.  The first
// generated token is chosen with L = 1 token in the row (the start token): n = 1 bans it already, n >= 2 bans nothing yet.
__global__ __launch_bounds__(192) void ngram_init_kernel(unsigned* __restrict__ row_mask, const unsigned* __restrict__ base_mask,
                                                         const int* __restrict__ base_set_of_row, const int* __restrict__ ngram_of_row,
                                                         int rows, int words, int start_id) {
    const int row = blockIdx.x;
    if (row >= rows) return;
    const bool ban_start = ngram_of_row[row] == 1 && (unsigned)start_id < (unsigned)(words * 32);
    for (int w = threadIdx.x; w < words; w += blockDim.x)
        row_mask[(size_t)row * words + w] = base_row_word(base_mask, base_set_of_row[row], words, w, ban_start, start_id);
}

// Start of a batch with a repetition penalty, one block of 192 threads per row: the sibling of ngram_init_kernel.  The row's
// seen words are zeroed and the start token's bit is set - every word has one writer.
__global__ __launch_bounds__(192) void penalty_init_kernel(unsigned* __restrict__ seen_mask, int rows, int words, int start_id) {
    const int row = blockIdx.x;
    if (row >= rows) return;
    for (int w = threadIdx.x; w < words; w += blockDim.x)
        seen_mask[(size_t)row * words + w] = ((unsigned)start_id < (unsigned)(words * 32) && w == (start_id >> 5)) ? 1u << (start_id & 31) : 0u;
}

// Start of a batch with token automata, one block of 192 threads per row (words <= 192): the sibling of ngram_init_kernel.
// A row that brings an automaton (aut_base_of_row[row] >= 0) starts in its start state with the mask A(start) AND its base
// set, minus the start token when n = 1, and {EOS} if nothing is left (the dead-end rule); a row without one gets what
// ngram_init_kernel gives it and the state AUT_STATE_NONE.  SOFT (soft token automata; default_next is read by this form
// alone): the start state may be OPEN (default_next[base] >= 0) - then A(start) is every token, EOS iff the state accepts.
template <bool SOFT>
__global__ __launch_bounds__(192) void automaton_init_kernel(unsigned* __restrict__ row_mask, const unsigned* __restrict__ base_mask,
                                                             const int* __restrict__ base_set_of_row, const int* __restrict__ ngram_of_row,
                                                             int rows, int words, int start_id, int eos_id,
                                                             const int* __restrict__ edge_begin, const int* __restrict__ edge_token,
                                                             const uint8_t* __restrict__ accepting,
                                                             const int* __restrict__ aut_base_of_row, int* __restrict__ aut_state,
                                                             const int* __restrict__ default_next) {
    __shared__ unsigned s_mask[192];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= rows) return;
    const int V = words * 32;
    const int base = aut_base_of_row[row];              // block-uniform
    const bool ban_start = ngram_of_row[row] == 1 && (unsigned)start_id < (unsigned)V;
    if (tid == 0) aut_state[row] = base >= 0 ? base : AUT_STATE_NONE;
    if (base < 0) {
        for (int w = tid; w < words; w += blockDim.x)
            row_mask[(size_t)row * words + w] = base_row_word(base_mask, base_set_of_row[row], words, w, ban_start, start_id);
        return;
    }
    bool open = false;                                  // block-uniform
    if constexpr (SOFT) open = default_next[base] >= 0;
    state_mask_to_lds(s_mask, base, open, edge_begin, edge_token, accepting, eos_id, V, words, tid, blockDim.x);
    unsigned m = 0u;
    if (tid < words) m = s_mask[tid] & base_row_word(base_mask, base_set_of_row[row], words, tid, ban_start, start_id);
    const int any = __syncthreads_or(m != 0u);
    if (!any && (unsigned)eos_id < (unsigned)V && tid == (eos_id >> 5)) m = 1u << (eos_id & 31);
    if (tid < words) row_mask[(size_t)row * words + tid] = m;
}

// End of a batch with token automata: the rows' states in their automata's own numbering (a state of automaton h is
// global state aut_first[h] + s), AUT_STATE_DEAD as it is, AUT_STATE_NONE for a row without an automaton.
__global__ __launch_bounds__(256) void automaton_state_out_kernel(const int* __restrict__ aut_state, const int* __restrict__ aut_base_of_row,
                                                                  int* __restrict__ out, int rows) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int base = aut_base_of_row[row], s = aut_state[row];
    out[row] = base < 0 ? AUT_STATE_NONE : s >= 0 ? s - base : s;
}

// ------------------------------------------------------------------------------------------------
// Row compaction (r04): finished rows stop costing.
// In the reference every crop is its own generate() call and stops at its own EOS (TF/generation/utils.py:2929-2937,
// called per crop at src/ui/main_window.py:9801).  A merged batch decodes in lockstep; between two chunks of steps the
// scheduler (engine.hip: compact_rows) moves the unfinished rows to the first slots and lets the next chunk run on fewer
// slots.  Only the step's input rows (x_f32 / x_t) move: ids, finished, len and every key/value cache are indexed by ROW
// through DecState::rowmap and stay where they are.
//
// compact_plan_kernel, ONE block: stable partition of the np slots by "row unfinished" -> new_map[s'] = row of new slot
// s', src_slot[s'] = the slot it comes from.  The finished rows fill the slots behind the live ones (any slot the next
// chunks still run - the row count is rounded up to a graph-friendly grid - then holds a finished row: it emits pad_id
// into that row's tail, which is what an uncompacted batch does to it).
__global__ __launch_bounds__(1024) void compact_plan_kernel(const int* __restrict__ rowmap, const int* __restrict__ finished, int np,
                                                            int* __restrict__ new_map, int* __restrict__ src_slot) {
    __shared__ int s_cnt[1024];
    const int tid = threadIdx.x;
    const int per = (np + 1023) / 1024, s0 = tid * per, s1 = min(np, s0 + per);
    int live = 0;
    for (int s = s0; s < s1; ++s) live += finished[rowmap[s]] ? 0 : 1;
    s_cnt[tid] = live;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {          // inclusive scan
        const int v = tid >= off ? s_cnt[tid - off] : 0;
        __syncthreads();
        s_cnt[tid] += v;
        __syncthreads();
    }
    const int n_live = s_cnt[1023];
    int pl = s_cnt[tid] - live;                          // live slots in front of s0
    for (int s = s0; s < s1; ++s) {
        const int row = rowmap[s];
        const bool lv = !finished[row];
        const int dst = lv ? pl : n_live + (s - pl);
        new_map[dst] = row; src_slot[dst] = s;
        pl += lv ? 1 : 0;
    }
}

// phase 0: tmp[s'] = x[src_slot[s']] for the np_new slots that stay; phase 1: x[s'] = tmp[s'], rowmap = new_map (np_old entries).
// One block of D/4 threads per slot.
template <typename T, int D>
__global__ __launch_bounds__(D / 4) void compact_move_kernel(int phase, const int* __restrict__ new_map, const int* __restrict__ src_slot,
                                                              float* __restrict__ x_f32, T* __restrict__ x_t, float* __restrict__ tmp_f32,
                                                              T* __restrict__ tmp_t, int* __restrict__ rowmap, int np_new, int np_old) {
    const int s = blockIdx.x, c = threadIdx.x * 4;
    if (phase == 0) {
        const int src = src_slot[s];
        *reinterpret_cast<float4*>(tmp_f32 + (size_t)s * D + c) = *reinterpret_cast<const float4*>(x_f32 + (size_t)src * D + c);
        float v[4];
        elem<T>::ld4(x_t + (size_t)src * D + c, v);
        elem<T>::st4(tmp_t + (size_t)s * D + c, v);
    } else {
        *reinterpret_cast<float4*>(x_f32 + (size_t)s * D + c) = *reinterpret_cast<const float4*>(tmp_f32 + (size_t)s * D + c);
        float v[4];
        elem<T>::ld4(tmp_t + (size_t)s * D + c, v);
        elem<T>::st4(x_t + (size_t)s * D + c, v);
        for (int i = s * (D / 4) + threadIdx.x; i < np_old; i += gridDim.x * (D / 4)) rowmap[i] = new_map[i];
    }
}
