// Beam search on the device (GenerationMixin._beam_search of transformers 5.x, do_sample = False, one EOS id, a prompt of
// one token): the selection that ends a decode step in place of the greedy token kernel, and the reorder of the
// self-attention caches that follows it.  Beam k of crop c is row c K + k of the batch; the K rows of a crop sit in K
// neighbouring decode slots (a crop's rows finish together and the compaction is a stable partition, so a group of slots
// g K .. g K + K - 1 always holds one crop's rows in beam order).
#pragma once
#include "common.h"
#include "kernels_decode.h"

constexpr int BEAM_MAX = 4;             // = MOCR_MAX_BEAMS
constexpr int BEAM_HIST = 320;          // tokens of a history the selection keeps in LDS: ids_ld <= this (the attention kernels' limit)
#define BEAM_NEG 1.0e9f                 // transformers' "minus infinity" of beam scores

// Per-lane beam state, by ROW like ids (a compaction moves nothing).
struct BeamState {
    float* beam_score;      // [rows] accumulated log-probability of the running beam
    int* parent;            // [rows] the beam (0 .. K - 1, of the same crop) whose history and caches the row continues
    int* hyp_ids;           // [rows][ids_ld] the crop's K finished hypotheses, best first, pad_id behind their length
    int* hyp_len;           // [rows] 0: the slot never received a finished sequence
    float* hyp_score;       // [rows] -1e9 then
    int* heuristic_open;    // [crops] is_early_stop_heuristic_unsatisfied
    float length_penalty;
    int early_stopping;     // 0 false, 1 true, 2 "never"
    int ngram;              // no_repeat_ngram_size, 0: off
    // the token form of the selection (all nullable; the plain form reads none of them)
    float* beam_logp;       // [rows][ids_ld] the running beam's token log-probabilities, by row like ids: [0] = 0 (the start token)
    float* hyp_logp;        // [rows][ids_ld] those of the finished hypotheses, 0 behind their length: moves as hyp_ids does
    const unsigned* tok_mask;   // [sets][V / 32] the engine's token-set bit table ...
    const int* set_of_row;      // [rows] ... and the set of every row (the K rows of a crop name the same one)
    // the trail form (both or neither; every other form reads neither): transformers' beam_indices, relative to the crop's group
    uint8_t* beam_trail;    // [rows][ids_ld] [t], t >= 1: the beam 0 .. K - 1 whose row ran the step that appended token t; by row like ids
    uint8_t* hyp_trail;     // [rows][ids_ld] those of the finished hypotheses, 0 behind their length: moves as hyp_ids does
};

// Token automata under beam search (mocr.h, "beam search under a token automaton"): the LAST argument of beam_select_kernel,
// read by its AUT form only - a trailing argument, so that BeamState and every other argument stay where they were.  The
// engine's tables in CSR form over GLOBAL state numbers (DecAutomata's), and by ROW like ids: base_of_row, the global number of
// the crop's start state (-1: the crop brings no automaton; its K rows name the same one), state, the state every running
// beam is in (AUT_STATE_DEAD once a chosen token had no edge), and hyp_state, the state of every finished hypothesis behind
// its last token other than EOS - it moves as hyp_ids does.
struct BeamAutomata {
    const int* edge_begin;
    const int* edge_token;
    const int* edge_next;
    const uint8_t* accepting;
    const int* base_of_row;
    int* state;
    int* hyp_state;
};

// Soft token automata under beam search (mocr.h, "beam search under soft token automata"): the trailing argument of the SOFT
// form in the place of BeamAutomata - the same seven pointers plus the arena's two soft arrays (DecSoftAutomata's): edge_weight
// [edges], the fp32 bias an edge adds to its token's log-probability, and default_next [states], where an OPEN state sends a
// token without an edge (global, AUT_DEFAULT_FALLBACK as in the greedy form; -1: the state is closed).  Only the SOFT
// instantiations take this type, so every other form keeps the argument block it had.
struct BeamSoftAutomata : BeamAutomata {
    const float* edge_weight;
    const int* default_next;
};

// Start of a beam batch under token automata, beside beam_init_kernel (as automaton_init_kernel is to ngram_init_kernel):
// every running beam in its crop's start state, every finished slot without one.
__global__ __launch_bounds__(256) void beam_automaton_init_kernel(const int* __restrict__ base_of_row, int* __restrict__ state,
                                                                  int* __restrict__ hyp_state, int rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int base = base_of_row[r];
    state[r] = base >= 0 ? base : AUT_STATE_NONE;
    hyp_state[r] = AUT_STATE_NONE;
}

// Start of a beam batch, one block of 64 threads per row: running scores [0, -1e9, ...], an empty finished set.
__global__ __launch_bounds__(64) void beam_init_kernel(BeamState bs, int K, int rows, int ids_ld, int pad_id) {
    const int r = blockIdx.x;
    if (r >= rows) return;
    for (int i = threadIdx.x; i < ids_ld; i += 64) bs.hyp_ids[(size_t)r * ids_ld + i] = pad_id;
    if (bs.beam_logp)
        for (int i = threadIdx.x; i < ids_ld; i += 64) bs.beam_logp[(size_t)r * ids_ld + i] = 0.f;
    if (bs.hyp_logp)
        for (int i = threadIdx.x; i < ids_ld; i += 64) bs.hyp_logp[(size_t)r * ids_ld + i] = 0.f;
    if (bs.beam_trail)
        for (int i = threadIdx.x; i < ids_ld; i += 64) bs.beam_trail[(size_t)r * ids_ld + i] = 0;
    if (bs.hyp_trail)
        for (int i = threadIdx.x; i < ids_ld; i += 64) bs.hyp_trail[(size_t)r * ids_ld + i] = 0;
    if (threadIdx.x == 0) {
        bs.beam_score[r] = (r % K == 0) ? 0.f : -BEAM_NEG;
        bs.parent[r] = r % K;
        bs.hyp_len[r] = 0;
        bs.hyp_score[r] = -BEAM_NEG;
        if (r % K == 0) bs.heuristic_open[r / K] = 1;
    }
}

// End of a beam step, one block of 256 threads per crop (slots g K .. g K + K - 1):
//   per beam: logits = sum_s slab_s + bias (the slab path of dec_token_kernel, the same fp32 sums), the row's max and log S,
//     the beam's n-gram bans from ITS history (the window scan of the NGRAM token kernel, from scratch, in LDS), and
//     score = ((logit - max) - log S) + beam_score - log_softmax over the full row first, bans as -inf without renormalising;
//   the 2 K best of the K V scores (TopN: equal scores go to the lower flat index beam V + token);
//   thread 0: the stopping rule (EOS, or the token completes max_len), the K running beams of the next step (the best
//     candidates that did not stop), the finished set (its K entries merged with the stopped candidates among the first K,
//     score / (tokens generated) ^ length_penalty), the early-stop heuristic and the end of the crop;
//   the block: ids[row_k] = the parent's history plus the token (the K old histories are in LDS before anything is
//     written), new hypotheses into hyp_ids, and every new beam's next input LN(word[tok] + type0 + pos[t + 1]) into x_f32 /
//     x_t of its slot and into the layer-0 cache row of position t + 1.
// The two -1e9 guards of _update_finished_beams ("beams full and early_stopping", "heuristic satisfied") hold exactly when
// the crop's own end condition holds, and a crop that ended is frozen: its block only advances `step`, like the block of
// a trailing partial group of padding slots.  (The guards are applied all the same, for states given through the hook.)
//
// TOK, the token form (token sets and token scores; the plain form is the code above and compiles to what it was):
//   s_mask starts from the crop's row of the token-set table instead of all-ones and then takes the bans; it is applied at
//     every step.  A token outside the set is -inf exactly like a banned one - log_softmax over the full row first, no
//     renormalising (transformers' PrefixConstrainedLogitsProcessor), NOT the greedy sets' renormalised softmax;
//   max and log S of every beam stay in LDS, and behind thread 0's section 2 K lanes recompute lp = (v - max) - log S of the
//     2 K winners from (parent, token), one winner each: v = bias + slab 0 + ... + slab nslab - 1 in the order of the row pass,
//     so it is the very fp32 value the selection ranked, and running' = lp + running holds exactly (score - running would
//     round differently);
//   beam_logp travels with ids (through s_lhist), hyp_logp with hyp_ids (through s_lhyp);
//   with fewer than 2 K finite scores a winner can be dead (-inf): it never enters the finished set (-inf < -1e9), and the
//     next running beams are the best K of (score, -1e9 on the stopped ones) by value, the earlier candidate first among
//     equals - the plain form's "those that did not stop, then the stopped ones" whenever no candidate is dead.
//
// TRAIL, the trail form (token positions of the hypotheses; orthogonal to TOK, and without it the code is what it was):
//   beam_trail[row][t] is the beam, 0 .. K - 1 of the crop's group, whose row ran the step that appended token t - the row
//     that step's recordings (the engine's pos_hist) lie in, since those are written by row and never reordered.  It travels
//     with ids (through s_thist), and the entry of the token this step appends is the candidate's parent; hyp_trail travels
//     with hyp_ids (through s_thyp), the shift under an inserted hypothesis included.  One byte per entry: K <= 4.
// AUT, the automaton form (implies TOK; a crop whose base_of_row is -1 takes the token form's path, bit for bit):
//   every beam walks the crop's automaton with a state of its own.  Beam k's mask is built in LDS from the edge range of its
//     state - zero, barrier, the 256 threads stride over the edges (the universal state: 6,143 of them, 24 a thread) with LDS
//     atomicOr plus the EOS bit iff the state accepts, barrier, AND the crop's set word - and then takes the n-gram bans as in
//     the token form.  A DEAD beam, or a set that meets no edge, leaves an empty mask: a dead beam, the token form's DEAD
//     CANDIDATES rule.  There is no dead-end rule.  Every branch is block-uniform (the base and the states come from LDS);
//   behind thread 0's section, beside the lanes that recompute lp, one lane per winner finds next(state of the parent, token)
//     by binary search over the parent's edges (a state's tokens are strictly ascending): AUT_STATE_DEAD when absent.  Thread
//     0's decisions need no state;
//   a new running beam takes its candidate's state; a hypothesis that enters the finished set keeps the parent's state if it
//     stopped on EOS (EOS moves nothing) and the candidate's if it stopped by length (the last token walks, as in greedy).
//     The K old beam states and the K old hypothesis states are in LDS before any state is written - the argument of s_hist.
// SOFT, the soft form (implies AUT; `aut` is a BeamSoftAutomata; every other form compiles to what it was).  transformers'
//   generate(num_beams = K, sequence_bias = ...): the bias is a logits processor BEHIND the log_softmax, so it enters the
//   ranked score, the running score and the token score, and nothing renormalises - not the greedy soft rule, which adds the
//   weight before its softmax.  Three places differ from the AUT form.
//   The mask of beam k: an OPEN state (default_next >= 0) starts from all ones with the EOS bit cleared unless it accepts,
//     instead of zero plus the OR of the edge bits; the set AND and the bans follow as before.  Openness comes from the state
//     in LDS: the branch is block-uniform.
//   The row pass: gmax and log S are those of the raw row.  Per float4 a thread binary-searches the state's ascending edge
//     tokens for its first column (dec_token_kernel's SOFT slab path) and keeps the weights of the edges inside it; the
//     score is (((v - gmax) - log S) + w) + running, w skipped where it is 0, so a hard row keeps every bit.  The mask comes
//     after: a weight never revives a masked token.
//   The winners: the lane's binary search gives the edge, hence its target AND its weight - the token score is re-formed as
//     ((v - gmax) - log S) + w, the very value ranked, so running' = s + running holds exactly.  A miss in an open state
//     follows default_next; under AUT_DEFAULT_FALLBACK the token is looked up once more in the default state's edges.  A
//     candidate that stopped on EOS and is carried on at score - 1e9 is no special case: EOS is never an edge, so an open
//     state sends it along its default edge and a closed one to DEAD, as before.
// LDS, static, at K = 4: ids and hypotheses 2 x 5 KiB, their log-probabilities 2 x 5 KiB (token form only), their trails
// 2 x 1.25 KiB (trail form only), the mask 768 B, under 1 KiB of lists - 24 KiB of the 64 KiB a block may declare (the
// automaton form's K + K + 2 K states and the base: 68 B more).
template <typename T, int K, bool TOK = false, bool TRAIL = false, bool AUT = false, bool SOFT = false>
__global__ __launch_bounds__(256) void beam_select_kernel(const float* __restrict__ slabs, int nslab, long long slab_stride,
                                                          const float* __restrict__ vbias, int V, DecState st, BeamState bs, int np,
                                                          const float* __restrict__ word, const float* __restrict__ type0,
                                                          const float* __restrict__ pos, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ x_f32,
                                                          T* __restrict__ x_t, float eps, T* __restrict__ cache,
                                                          long long cache_batch_stride, uint8_t* __restrict__ cache8, float inv_sx8,
                                                          std::conditional_t<SOFT, BeamSoftAutomata, BeamAutomata> aut = {}) {
    static_assert(K >= 2 && K <= BEAM_MAX, "2 .. 4 beams");
    static_assert(!AUT || TOK, "the automaton form is a token form: its masks and the dead-candidate rule");
    static_assert(!SOFT || AUT, "weights and default edges belong to an automaton");
    constexpr int D = 768, MW = 192, NC = 6, C2 = 2 * K;
    __shared__ int s_hist[K][BEAM_HIST];
    __shared__ int s_hyp[K][BEAM_HIST];
    __shared__ unsigned s_mask[MW];
    __shared__ float s_red[4];
    __shared__ float s_cv[4][C2];
    __shared__ int s_ci[4][C2];
    __shared__ int s_row[K], s_ntok[K], s_npar[K];
    __shared__ int s_hsrc[K], s_hlen[K];              // finished slot j <- (>= 0: old slot, < 0: candidate -1 - i), its length
    __shared__ int s_ctok[C2], s_cpar[C2];
    __shared__ int s_new, s_done;
    constexpr int KT = TOK ? K : 1, HT = TOK ? BEAM_HIST : 1;
    __shared__ float s_lhist[KT][HT];
    __shared__ float s_lhyp[KT][HT];
    constexpr int KR = TRAIL ? K : 1, HR = TRAIL ? BEAM_HIST : 4;
    __shared__ uint8_t s_thist[KR][HR];
    __shared__ uint8_t s_thyp[KR][HR];
    __shared__ float s_gmax[K], s_logS[K], s_clp[C2];
    __shared__ int s_clive[C2], s_nsrc[K];            // the candidate is not dead; the candidate new beam k was made from
    constexpr int KA = AUT ? K : 1;
    __shared__ int s_ast[KA], s_hst[KA], s_cst[2 * KA];   // the K beams' states, the K hypotheses' states, the 2 K candidates' next states
    __shared__ int s_abase;                               // the crop's start state (-1: it brings no automaton)
    static_assert(sizeof(s_hist) + sizeof(s_hyp) + sizeof(s_lhist) + sizeof(s_lhyp) + sizeof(s_thist) + sizeof(s_thyp) + sizeof(s_mask) +
                          sizeof(s_ast) + sizeof(s_hst) + sizeof(s_cst) + sizeof(s_abase) + 1024 <= 65536,
                  "static LDS of the selection: the histories, the mask, the states and under 1 KiB of lists");
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot0 = g * K;
    if (slot0 + K > np) {                             // a trailing partial group: padding slots, born finished
        if (slot0 + tid < np) st.step[slot0 + tid] += 1;
        return;
    }
    const int t = st.step[slot0];
    const int row0 = st.rowmap[slot0];
    // the crop has ended (or is padding); a live crop's step is below max_len - 1 <= ids_ld - 1 (it would have ended on length)
    if (st.finished[row0] || (unsigned)t >= (unsigned)(st.max_len - 1)) {
        if (tid < K) st.step[slot0 + tid] = t + 1;
        return;
    }
    const int L = t + 1;                              // tokens every running beam holds
    const int crop = row0 / K;
    if (tid < K) s_row[tid] = st.rowmap[slot0 + tid];
    if constexpr (AUT) {                              // the K old states of both kinds, before any is written
        if (tid < K) { s_ast[tid] = aut.state[st.rowmap[slot0 + tid]]; s_hst[tid] = aut.hyp_state[crop * K + tid]; }
        if (tid == 0) s_abase = aut.base_of_row[row0];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int i = tid; i < L; i += 256) s_hist[k][i] = st.ids[(size_t)s_row[k] * st.ids_ld + i];
    if constexpr (TOK) {
        if (bs.beam_logp) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                for (int i = tid; i < L; i += 256) s_lhist[k][i] = bs.beam_logp[(size_t)s_row[k] * st.ids_ld + i];
        }
    }
    if constexpr (TRAIL) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            for (int i = tid; i < L; i += 256) s_thist[k][i] = bs.beam_trail[(size_t)s_row[k] * st.ids_ld + i];
    }
    __syncthreads();

    unsigned setw = 0xffffffffu;                      // this thread's word of the crop's set (its K rows name one set): read once
    if constexpr (TOK) {
        if (bs.tok_mask && tid < MW) setw = bs.tok_mask[(size_t)bs.set_of_row[row0] * MW + tid];
    }
    TopN<C2> top;
    topn_clear(top);
    const int n = bs.ngram;
    for (int k = 0; k < K; ++k) {
        const int b = slot0 + k;
        float4 a[NC];
        sum_slab_row(a, vbias, slabs, nslab, slab_stride, b, V, tid);
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < NC; ++j) mx = fmaxf(fmaxf(mx, fmaxf(a[j].x, a[j].y)), fmaxf(a[j].z, a[j].w));
        mx = wave_max(mx);
        if (lane == 0) s_red[wave] = mx;
        int se0 = 0, se1 = 0;                         // SOFT: the edge range of beam k's state (empty: no automaton, or DEAD)
        if constexpr (AUT) {
            if (s_abase >= 0) {                       // block-uniform: A(state of beam k), then the crop's set
                const int sk = s_ast[k];
                bool open = false;
                if constexpr (SOFT) {
                    open = sk >= 0 && aut.default_next[sk] >= 0;
                    if (sk >= 0) { se0 = aut.edge_begin[sk]; se1 = aut.edge_begin[sk + 1]; }
                }
                state_mask_to_lds(s_mask, sk, open, aut.edge_begin, aut.edge_token, aut.accepting, st.eos_id, V, MW, tid, 256);
                if (tid < MW) s_mask[tid] &= setw;
            } else {
                if (tid < MW) s_mask[tid] = setw;
            }
        } else if constexpr (TOK) {
            if (tid < MW) s_mask[tid] = setw;
        } else {
            if (n > 0 && tid < MW) s_mask[tid] = 0xffffffffu;
        }
        __syncthreads();
        const float gmax = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
        __syncthreads();
        float es = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j)
            es += (__expf(a[j].x - gmax) + __expf(a[j].y - gmax)) + (__expf(a[j].z - gmax) + __expf(a[j].w - gmax));
        es = wave_sum(es);
        if (lane == 0) s_red[wave] = es;
        if (n > 0) ngram_ban_windows(s_mask, s_hist[k], L, n, V, tid);     // the bans of this beam's own history
        __syncthreads();
        const float logS = logf((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
        const float bsc = bs.beam_score[s_row[k]];
        if constexpr (TOK) {
            if (tid == 0) { s_gmax[k] = gmax; s_logS[k] = logS; }
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = tid * 4 + j * 1024;
            const unsigned nib = (TOK || n > 0) ? (s_mask[c >> 5] >> (c & 31)) & 15u : 15u;
            const float v[4] = {a[j].x, a[j].y, a[j].z, a[j].w};
            if constexpr (SOFT) {
                // the weights of the state's edges inside this float4 (constant indices only: no register is indexed)
                float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
                for (int lo = edge_lower_bound(aut.edge_token, se0, se1, c); lo < se1; ++lo) {
                    const int d = aut.edge_token[lo] - c;
                    if (d >= 4) break;
                    const float wgt = aut.edge_weight[lo];
                    if (d == 0) w0 = wgt; else if (d == 1) w1 = wgt; else if (d == 2) w2 = wgt; else w3 = wgt;
                }
                const float w[4] = {w0, w1, w2, w3};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float lp = (v[q] - gmax) - logS;
                    const float s = w[q] != 0.f ? lp + w[q] : lp;
                    const float sc = ((nib >> q) & 1) ? s + bsc : -INFINITY;
                    topn_insert(top, sc, k * V + c + q);
                }
                continue;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float sc = ((nib >> q) & 1) ? ((v[q] - gmax) - logS) + bsc : -INFINITY;
                topn_insert(top, sc, k * V + c + q);
            }
        }
        __syncthreads();                              // s_red / s_mask are the next beam's
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) topn_merge_xor(top, o);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < C2; ++i) { s_cv[wave][i] = top.v[i]; s_ci[wave][i] = top.i[i]; }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
#pragma unroll
            for (int i = 0; i < C2; ++i) topn_insert(top, s_cv[w][i], s_ci[w][i]);
        float cv[C2];
        int ctok[C2], cpar[C2];
        bool stop[C2];
        const bool stop_len = t + 2 >= st.max_len;
        bool all_stop = true;
#pragma unroll
        for (int i = 0; i < C2; ++i) {
            const bool ok = (unsigned)top.i[i] < (unsigned)(K * V);      // (all-NaN logits win no comparison: stay inside the tables)
            cv[i] = top.v[i];
            cpar[i] = ok ? top.i[i] / V : 0;
            ctok[i] = ok ? top.i[i] - cpar[i] * V : 0;
            stop[i] = ctok[i] == st.eos_id || stop_len;
            all_stop = all_stop && stop[i];
            s_ctok[i] = ctok[i]; s_cpar[i] = cpar[i];
            if constexpr (TOK) s_clive[i] = ok && cv[i] > -INFINITY;      // (a dead candidate: masked, or the child of a dead beam)
        }
        // the running beams of the next step: the best K candidates after -1e9 on those that stopped = the ones that did
        // not stop, in order, then (only when fewer than K are left: the crop ends) the stopped ones
        float rsc[K];
        if constexpr (TOK) {
            // (by value: a dead candidate that did not stop ranks behind a stopped one's score - 1e9)
            float adj[C2];
            bool used[C2];
#pragma unroll
            for (int i = 0; i < C2; ++i) { adj[i] = stop[i] ? cv[i] - BEAM_NEG : cv[i]; used[i] = false; }
#pragma unroll
            for (int k = 0; k < K; ++k) {             // (constant indices only: the lists stay in registers)
                int b = -1, bt = 0, bp = 0;
                float bv = 0.f;
#pragma unroll
                for (int i = 0; i < C2; ++i) {
                    const bool take = !used[i] && (b < 0 || adj[i] > bv);
                    b = take ? i : b; bv = take ? adj[i] : bv; bt = take ? ctok[i] : bt; bp = take ? cpar[i] : bp;
                }
#pragma unroll
                for (int i = 0; i < C2; ++i) used[i] = used[i] || i == b;
                rsc[k] = bv;
                s_ntok[k] = bt; s_npar[k] = bp; s_nsrc[k] = b;
            }
        } else {
            int nr = 0;
#pragma unroll
            for (int pass = 0; pass < 2; ++pass)
#pragma unroll
                for (int i = 0; i < C2; ++i)
                    if (nr < K && stop[i] == (pass == 1)) {
                        rsc[nr] = pass ? cv[i] - BEAM_NEG : cv[i];
                        s_ntok[nr] = ctok[i]; s_npar[nr] = cpar[i];
                        ++nr;
                    }
        }
        // the finished set: its K entries (sorted) merged with the stopped candidates among the first K
        const float div = powf((float)L, bs.length_penalty);            // (cur_len + 1 - prompt) ^ length_penalty, L tokens generated
        float hs[K], ns[K];
        int hl[K], src[K], nl[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { hs[j] = bs.hyp_score[crop * K + j]; hl[j] = min(max(bs.hyp_len[crop * K + j], 0), st.ids_ld); }
        // (the reference's two guards: a full set under early_stopping = true, or a satisfied heuristic, takes nothing more -
        // states the engine never steps, since such a crop has ended; the operator hook can present them)
        bool guard = bs.early_stopping == 1 || !bs.heuristic_open[crop];
        if (bs.heuristic_open[crop])
            for (int j = 0; j < K; ++j) guard = guard && hl[j] > 0;
        int io = 0, ic = 0, any_new = 0;                                // the next old entry (io <= j < K), the next candidate
        for (int j = 0; j < K; ++j) {
            while (ic < K && !stop[ic]) ++ic;
            const float cs = ic < K ? (guard ? cv[ic] / div - BEAM_NEG : cv[ic] / div) : -INFINITY;
            if (ic < K && cs > hs[io]) { ns[j] = cs; nl[j] = t + 2; src[j] = -1 - ic; ++ic; any_new = 1; }      // (equal: the old entry first)
            else { ns[j] = hs[io]; nl[j] = hl[io]; src[j] = io; ++io; }
        }
        bool all_fin = true;
        for (int j = 0; j < K; ++j) {
            bs.hyp_score[crop * K + j] = ns[j]; bs.hyp_len[crop * K + j] = nl[j];
            s_hsrc[j] = src[j]; s_hlen[j] = src[j] >= 0 ? nl[j] : 0;
            all_fin = all_fin && nl[j] > 0;
        }
        // the heuristic of the next iteration (cur_len = t + 2) and the three-way end condition
        const float hyp_len_best = (bs.early_stopping == 2 && bs.length_penalty > 0.f) ? (float)(st.max_len - 1) : (float)(t + 1);
        const float best_possible = rsc[0] / powf(hyp_len_best, bs.length_penalty);
        const int open = bs.heuristic_open[crop] && best_possible > ns[K - 1];
        bs.heuristic_open[crop] = open;
        const bool done = !open || (all_fin && bs.early_stopping == 1) || all_stop;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int r = s_row[k];
            bs.beam_score[r] = rsc[k];
            bs.parent[r] = done ? k : s_npar[k];
            st.step[slot0 + k] = t + 1;
            if (done) { st.finished[r] = 1; st.len[r] = t + 2; }
        }
        if (done) atomicSub(st.n_unfinished, K);
        s_new = any_new; s_done = done ? 1 : 0;
    }
    __syncthreads();
    if constexpr (TOK) {
        // the winners' log-probabilities, one lane each (no decision above needed them): the row pass's own sums, in its order
        if (tid < C2) {
            float lp = -INFINITY;
            if (s_clive[tid]) {
                const int p = s_cpar[tid], c = s_ctok[tid];
                float v = vbias[c];
                for (int s = 0; s < nslab; ++s) v += slabs[(size_t)s * slab_stride + (size_t)(slot0 + p) * V + c];
                lp = (v - s_gmax[p]) - s_logS[p];
            }
            s_clp[tid] = lp;
            if constexpr (AUT) {
                // ... and their states: next(state of the parent, token), a binary search over the parent's ascending tokens
                int ns = AUT_STATE_NONE;
                if (s_abase >= 0) {
                    ns = AUT_STATE_DEAD;
                    const int sp = s_ast[s_cpar[tid]], c = s_ctok[tid];
                    if (sp >= 0) {
                        const int lo = edge_lower_bound(aut.edge_token, aut.edge_begin[sp], aut.edge_begin[sp + 1], c);
                        if (lo < aut.edge_begin[sp + 1] && aut.edge_token[lo] == c) {
                            ns = aut.edge_next[lo];
                            if constexpr (SOFT) {       // the edge's weight: the token score is the value the row pass ranked
                                const float wgt = aut.edge_weight[lo];
                                if (s_clive[tid] && wgt != 0.f) s_clp[tid] = lp + wgt;
                            }
                        } else if constexpr (SOFT) {    // a miss: along the default edge of an open state, DEAD in a closed one
                            const int dn = aut.default_next[sp];
                            if (dn >= 0) {
                                ns = dn & AUT_DEFAULT_STATE;
                                if (dn & AUT_DEFAULT_FALLBACK) {    // the token is walked from the default state: its edge, if it has one
                                    const int f1 = aut.edge_begin[ns + 1];
                                    const int flo = edge_lower_bound(aut.edge_token, aut.edge_begin[ns], f1, c);
                                    if (flo < f1 && aut.edge_token[flo] == c) ns = aut.edge_next[flo];
                                }
                            }
                        }
                    }
                }
                s_cst[tid] = ns;
            }
        }
        __syncthreads();
    }
    if (s_new) {                                      // block-uniform: the old hypotheses to LDS, then every slot from its source
#pragma unroll
        for (int j = 0; j < K; ++j)
            for (int i = tid; i < s_hlen[j]; i += 256) s_hyp[s_hsrc[j] >= 0 ? s_hsrc[j] : 0][i] = bs.hyp_ids[(size_t)(crop * K + s_hsrc[j]) * st.ids_ld + i];
        if constexpr (TOK) {
            if (bs.hyp_logp) {
#pragma unroll
                for (int j = 0; j < K; ++j)
                    for (int i = tid; i < s_hlen[j]; i += 256)
                        s_lhyp[s_hsrc[j] >= 0 ? s_hsrc[j] : 0][i] = bs.hyp_logp[(size_t)(crop * K + s_hsrc[j]) * st.ids_ld + i];
            }
        }
        if constexpr (TRAIL) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                for (int i = tid; i < s_hlen[j]; i += 256)
                    s_thyp[s_hsrc[j] >= 0 ? s_hsrc[j] : 0][i] = bs.hyp_trail[(size_t)(crop * K + s_hsrc[j]) * st.ids_ld + i];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < K; ++j) {
            int* dst = bs.hyp_ids + (size_t)(crop * K + j) * st.ids_ld;
            const int src = s_hsrc[j];
            if (src == j) continue;
            if (src >= 0) {
                for (int i = tid; i < st.ids_ld; i += 256) dst[i] = i < s_hlen[j] ? s_hyp[src][i] : st.pad_id;
            } else {
                const int ci = -1 - src;
                for (int i = tid; i < st.ids_ld; i += 256) dst[i] = i < L ? s_hist[s_cpar[ci]][i] : i == L ? s_ctok[ci] : st.pad_id;
            }
        }
        if constexpr (TOK) {
            if (bs.hyp_logp) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    float* dst = bs.hyp_logp + (size_t)(crop * K + j) * st.ids_ld;
                    const int src = s_hsrc[j];
                    if (src == j) continue;
                    if (src >= 0) {
                        for (int i = tid; i < st.ids_ld; i += 256) dst[i] = i < s_hlen[j] ? s_lhyp[src][i] : 0.f;
                    } else {
                        const int ci = -1 - src;
                        for (int i = tid; i < st.ids_ld; i += 256) dst[i] = i < L ? s_lhist[s_cpar[ci]][i] : i == L ? s_clp[ci] : 0.f;
                    }
                }
            }
        }
        if constexpr (AUT) {
            // the hypotheses' states move with them: an old slot's from LDS, a new one's from its candidate - the parent's
            // state behind EOS, the candidate's own behind a token that completed max_len
            if (tid < K) {
                const int src = s_hsrc[tid];
                if (src != tid) {
                    int v;
                    if (src >= 0) v = s_hst[src];
                    else {
                        const int ci = -1 - src;
                        v = s_abase < 0 ? AUT_STATE_NONE : s_ctok[ci] == st.eos_id ? s_ast[s_cpar[ci]] : s_cst[ci];
                    }
                    aut.hyp_state[crop * K + tid] = v;
                }
            }
        }
        if constexpr (TRAIL) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                uint8_t* dst = bs.hyp_trail + (size_t)(crop * K + j) * st.ids_ld;
                const int src = s_hsrc[j];
                if (src == j) continue;
                if (src >= 0) {
                    for (int i = tid; i < st.ids_ld; i += 256) dst[i] = i < s_hlen[j] ? s_thyp[src][i] : (uint8_t)0;
                } else {
                    const int ci = -1 - src;
                    for (int i = tid; i < st.ids_ld; i += 256)
                        dst[i] = i < L ? s_thist[s_cpar[ci]][i] : i == L ? (uint8_t)s_cpar[ci] : (uint8_t)0;
                }
            }
        }
    }
    if (s_done) return;                               // block-uniform
    // the new beams' rows: the parent's history plus the token
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int* dst = st.ids + (size_t)s_row[k] * st.ids_ld;
        const int p = s_npar[k];
        if (p != k)
            for (int i = tid; i < L; i += 256) dst[i] = s_hist[p][i];
        if (tid == 0 && L < st.ids_ld) dst[L] = s_ntok[k];
    }
    if constexpr (TOK) {
        if (bs.beam_logp) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float* dst = bs.beam_logp + (size_t)s_row[k] * st.ids_ld;
                const int p = s_npar[k];
                if (p != k)
                    for (int i = tid; i < L; i += 256) dst[i] = s_lhist[p][i];
                if (tid == 0 && L < st.ids_ld) dst[L] = s_clp[s_nsrc[k]];
            }
        }
    }
    if constexpr (AUT) {
        if (tid < K) aut.state[s_row[tid]] = s_cst[s_nsrc[tid]];
    }
    if constexpr (TRAIL) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint8_t* dst = bs.beam_trail + (size_t)s_row[k] * st.ids_ld;
            const int p = s_npar[k];
            if (p != k)
                for (int i = tid; i < L; i += 256) dst[i] = s_thist[p][i];
            if (tid == 0 && L < st.ids_ld) dst[L] = (uint8_t)p;
        }
    }
    // every new beam's next input (the tail of dec_token_kernel); s_red is the next beam's behind one more barrier
    for (int k = 0; k < K; ++k) {
        embed_ln_store<T, D>(s_ntok[k], t + 1, slot0 + k, s_row[k], word, type0, pos, gamma, beta, x_f32, x_t, eps, cache, cache_batch_stride,
                             cache8, inv_sx8, s_red, tid);
        __syncthreads();
    }
}

// In-place reorder of a self-attention cache behind the selection: dst beam k <- src beam parent[k], positions 0 .. t of
// every (layer, segment); position t + 1 was written by the selection for the NEW order and is not touched.  One generic
// kernel over a strided view in bytes: [layers][rows][segments][positions][pos_bytes] - the latent xcache / x8cache have one
// segment per (layer, row), the classic kcache / vcache one per head.  A thread owns one 16-byte piece offset within a crop's
// group of K rows: it loads the K beams' pieces into registers and stores them permuted, so no two threads share a byte and
// the permutation needs no barrier, no scratch and no second cache - cycles and "all from beam 0" alike.
struct BeamPermuteView {
    char* base;
    long long layer_stride, row_stride, seg_stride;     // bytes
    int segs, pos_bytes;                                 // pos_bytes: a multiple of 16
};

template <int K>
__global__ __launch_bounds__(256) void beam_permute_kernel(BeamPermuteView v, const int* __restrict__ parent, const int* __restrict__ rowmap,
                                                           const int* __restrict__ finished, const int* __restrict__ step, int np, int max_pos) {
    const int slot0 = blockIdx.x * K;
    if (slot0 + K > np) return;
    int row[K], par[K];
    bool ident = true;
#pragma unroll
    for (int k = 0; k < K; ++k) row[k] = rowmap[slot0 + k];
    if (finished[row[0]]) return;                      // a crop that has ended keeps its caches (nothing reads them again)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        par[k] = min(max(parent[row[k]], 0), K - 1);
        ident = ident && par[k] == k;
    }
    if (ident) return;
    // the selection has advanced step to t + 1: positions 0 .. t (max_pos, which sized the grid, bounds it)
    const long long nbytes = (long long)min(max(step[slot0], 0), max_pos) * v.pos_bytes;
    const long long off = ((long long)blockIdx.z * 256 + threadIdx.x) * 16;
    if (off >= nbytes) return;
    const int layer = blockIdx.y / v.segs, seg = blockIdx.y - layer * v.segs;
    char* const p0 = v.base + (long long)layer * v.layer_stride + (long long)seg * v.seg_stride + off;
    uint4 r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = *reinterpret_cast<const uint4*>(p0 + (long long)row[k] * v.row_stride);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (par[k] == k) continue;
        uint4 x = r[0];
#pragma unroll
        for (int j = 1; j < K; ++j) x = par[k] == j ? r[j] : x;
        *reinterpret_cast<uint4*>(p0 + (long long)row[k] * v.row_stride) = x;
    }
}
